"""libsslam_window.so, libsslam_place.so, libsslam_conf.so, libsslam_weight.so and libsslam_track.so run at the size limits their
headers state, at the smallest sizes that reach the paths the older cases never take, and with operands past 2^31 bytes
(tests/online_limit_cases.py builds the cases, tests/test_online_limit_cases_cpu.py holds them to their names), bit for bit and for
every output against the restatements (tests/window_ref.py, place_ref.py, confidence_ref.py, weighted_refine_ref.py,
sslam_amd/track_numpy.py): tolerance none.

An operand past 2^31 bytes is built on the device from its at most 11 distinct items (tests/periodic.py) and compared there, as
integer bits, over the whole output.  After the passing comparison every case changes one input element at the far end and compares
with the restatement's new result: the output changes there and, where the items are independent, nowhere else.  A call one past a
limit is refused by the entry itself, with its stated code, nothing launched and poisoned outputs untouched.

Every test frees what it allocated, prints its peak of device memory and asserts it below 24 GiB.  One test at a time.
profiles/online_limits.txt holds the audit of the index expressions, the measured durations and the peaks."""
import ctypes as C

import numpy as np
import pytest

import conf_table as ct
import online_limit_cases as oc
import periodic as pd
import place_table as pt
import track_table as tt
import weight_table as wt
import window_table as wnt
from test_gpu_graph_limits import _far_end, _poison, _ptr, _raw, _same, _untouched
from test_gpu_size_limits import _dev, _memory

pytestmark = pytest.mark.gpu
FILL = -77                                # what a state no step may touch is filled with


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def lib():
    from sslam_amd import lib
    return lib


def _same_dict(T, got, want, keys, what):
    for key in keys:
        w = np.asarray(want[key])
        _same(T, got[key], w.astype(w.dtype if w.dtype.kind == "f" else np.int32).reshape(tuple(got[key].shape)), f"{what}, {key}")


def _refused(T, count, call, code, outs, what):
    """`call()` is one entry with an argument one past a limit on real operands: `code`, nothing launched, the poisoned outs untouched."""
    _poison(T, outs)
    n0 = count()
    rc = call()
    T.cuda.synchronize()
    assert rc == code, (what, rc)
    assert count() == n0, f"{what}: a refused call launches nothing"
    _untouched(T, outs, what)


def _differs(T, a, b):
    return not T.equal(_raw(T, a), _raw(T, b))


# =============================================================================================================== libsslam_track.so
def track_ids_by_frames(T, prev, prev_frame, resume=None):
    """sslt_track_ids restated frame by frame in torch, where prev (n_bank, K) lives: a root takes the next number in (frame, slot)
    order, any other node its predecessor's root and that node's age + 1.  -> (TRACK_ID_KEYS' tensors as a dict, (root, age)).
    resume: (root, age, f0) of an earlier call whose frames before f0 still stand."""
    n_bank, k = prev.shape
    n = n_bank * k
    dev = prev.device
    pf = prev_frame.tolist()
    own = T.arange(n, dtype=T.int32, device=dev).view(n_bank, k)
    has = (prev >= 0) & (prev < k)
    idx = prev.clamp(0, k - 1).long()
    if resume is None:
        root, age, f0 = own.clone(), T.zeros((n_bank, k), dtype=T.int32, device=dev), 0
    else:
        root, age, f0 = resume[0].clone(), resume[1].clone(), resume[2]
    for f in range(f0, n_bank):
        p = pf[f]
        if not 0 <= p < f:
            root[f], age[f] = own[f], 0
            continue
        root[f] = T.where(has[f], root[p].gather(0, idx[f]), own[f])
        age[f] = T.where(has[f], age[p].gather(0, idx[f]) + 1, 0)
    del has, idx
    flat = root.view(-1)
    is_root = flat == own.view(-1)
    number = T.cumsum(is_root, 0, dtype=T.int32) - is_root.int()          # the exclusive scan of the root flags
    track_id = number[flat.long()].view(n_bank, k)
    roots = T.nonzero(is_root).flatten()
    nt = int(roots.numel())
    del is_root, number
    root_frame, root_slot = T.full((n,), -1, dtype=T.int32, device=dev), T.full((n,), -1, dtype=T.int32, device=dev)
    root_frame[:nt], root_slot[:nt] = (roots // k).int(), (roots % k).int()
    del roots
    length = T.zeros(n, dtype=T.int32, device=dev)
    length[:nt] = T.bincount(track_id.view(-1), minlength=nt)[:nt].int()
    out = dict(track_id=track_id, age=age.clone(), n_tracks=T.tensor([nt], dtype=T.int32, device=dev), root_frame=root_frame, root_slot=root_slot,
               length=length)
    return out, (root, age)


def _equal_tensors(T, got, want, keys, what):
    """Device tensors against device tensors of the restatement, on integer bits."""
    for key in keys:
        g, w = _raw(T, got[key]).reshape(-1), _raw(T, want[key]).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        bad = int((g != w).sum())
        assert bad == 0, f"{what}, {key}: differs from the restatement in {bad} elements of {g.numel()}, the first at flat index {int(T.nonzero(g != w)[0])}"
        print(f"{what}, {key}: 0 mismatching elements of {g.numel()}")


def _link_ops(T, c, matches=None):
    return dict(first=_dev(T, c["first"]), second=_dev(T, c["second"]), matches=_dev(T, c["matches"] if matches is None else matches),
                count=_dev(T, c["count"]), mask=_dev(T, c["mask"]))


@pytest.mark.parametrize("name", list(oc.IDS_BANKS))
def test_ids_tiles(T, lib, name):
    """262 144, 262 272 and 525 312 nodes: 256, 257 and 513 tiles of the numbering scan - one, two and three chunks of
    ids_scan_tiles_kernel, whose carry decides every id, root_frame and root_slot past node 262 144, and n_tracks."""
    c = oc.ids_tiles(name)
    n_bank, k = c["n_bank"], c["K"]
    assert -(-n_bank * k // tt.SCAN_TILE) == int(name.rsplit("_", 1)[1])
    with _memory(T, name):
        o = _link_ops(T, c)
        links = lib.link_pairs(o["first"], o["second"], o["matches"], o["count"], n_bank, k, mask=o["mask"])
        _same_dict(T, links, c["links"], lib.LINK_KEYS, name)
        n0 = lib.track_launch_count()
        got = lib.track_ids(links["prev"], links["prev_frame"])
        assert lib.track_launch_count() - n0 == tt.launches("sslt_track_ids", n_bank)
        _same_dict(T, got, c["want"], lib.TRACK_ID_KEYS, name)
        got = lib.track_ids(_dev(T, c["prev_far"]), links["prev_frame"])
        _same_dict(T, got, c["want_far"], lib.TRACK_ID_KEYS, name + ", the last node's predecessor removed")
        del o, links, got


def _link_outs(T, lib, n_bank, k):
    return [T.empty(shape, dtype=dt, device="cuda") for shape, dt in lib.link_shapes(n_bank, k).values()]


def test_links_k_4096(T, lib):
    """K = n1 = 4096 on three frames: lo1[], lo2[] of link_slots_kernel to their ends.  K = 4097 and n_bank * K = 2^31 are refused."""
    c = oc.links_k_4096()
    name, n_bank, k = c["name"], c["n_bank"], c["K"]
    assert k == tt.LIMITS["sslt_link_pairs"]["largest"]["K"] == c["n1"]
    with _memory(T, name):
        o = _link_ops(T, c)
        outs = _link_outs(T, lib, n_bank, k)
        entry = lambda nb, kk: lib.track().sslt_link_pairs(_ptr(o["first"]), _ptr(o["second"]), 2, _ptr(o["matches"]), _ptr(o["count"]), _ptr(o["mask"]),      # noqa: E731
                                                           k, nb, kk, *[_ptr(t) for t in outs], None)
        _refused(T, lib.track_launch_count, lambda: entry(n_bank, k + 1), tt.E_UNSUPPORTED, outs, "K 4097")
        _refused(T, lib.track_launch_count, lambda: entry((1 << 31) // k, k), tt.E_UNSUPPORTED, outs, "n_bank * K 2^31")
        for nb, kk in ((n_bank, k + 1), ((1 << 31) // k, k)):
            with pytest.raises(lib.SslamHipError, match="unsupported"):
                lib.link_pairs(o["first"], o["second"], o["matches"], o["count"], nb, kk, mask=o["mask"])
        n0 = lib.track_launch_count()
        links = lib.link_pairs(o["first"], o["second"], o["matches"], o["count"], n_bank, k, mask=o["mask"])
        assert lib.track_launch_count() - n0 == tt.launches("sslt_link_pairs")
        _same_dict(T, links, c["links"], lib.LINK_KEYS, name)
        got = lib.track_ids(links["prev"], links["prev_frame"])
        _same_dict(T, got, c["want"], lib.TRACK_ID_KEYS, name)
        ids, ws = [got[key] for key in lib.TRACK_ID_KEYS], T.empty(64, dtype=T.uint8, device="cuda")
        _refused(T, lib.track_launch_count, lambda: lib.track().sslt_track_ids(_ptr(links["prev"]), _ptr(links["prev_frame"]), (1 << 31) // k, k, _ptr(ws),
                                                                               *[_ptr(t) for t in ids], None), tt.E_UNSUPPORTED, ids, "sslt_track_ids, n_bank * K 2^31")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.check_track_sizes("track_ids", (1 << 31) // k, k)
        links = lib.link_pairs(o["first"], o["second"], _dev(T, c["matches_far"]), o["count"], n_bank, k, mask=o["mask"])
        _same_dict(T, links, c["links_far"], lib.LINK_KEYS, name + ", the last slot's idx2 changed")
        _same_dict(T, lib.track_ids(links["prev"], links["prev_frame"]), c["want_far"], lib.TRACK_ID_KEYS, name + ", the last slot's idx2 changed")
        del o, outs, links, got, ids, ws


def _bank_steps(T, lib, c, matches, what):
    """The three online steps of links_k_4096's rows on a fresh device bank: every step's outputs against `outs`; -> the state."""
    state, out = lib.alloc_track_state(c["n_bank"], c["K"]), lib.alloc_track_out(c["K"])
    o = _link_ops(T, c, matches)
    rows = [(0, -1, T.zeros(1, dtype=T.int32, device="cuda"), None)] + [(r, int(c["first"][r]), o["count"][r:r + 1], o["mask"][r]) for r in range(2)]
    for i, (r, first, count, mask) in enumerate(rows):
        n0 = lib.track_launch_count()
        got = lib.track_step(state, o["matches"][r], count, T.tensor([first], dtype=T.int32, device="cuda"), mask=mask, out=out)
        assert lib.track_launch_count() - n0 == 1
        _same_dict(T, got, what[0][i], lib.TRACK_OUT_KEYS, f"{c['name']}, step {i}")
    _same_dict(T, state, what[1], lib.TRACK_STATE_KEYS, f"{c['name']}, the state")
    return state


def test_step_k_4096(T, lib):
    """Three online steps at K = n1 = 4096: lo1[], lo2[], pv[] of track_step_kernel to their ends, the id scan over 16 chunks.  The
    state equals the batch entries' outputs bit for bit.  K = 4097 is refused."""
    c = oc.step_k_4096()
    name, k = c["name"], c["K"]
    assert k == tt.LIMITS["sslt_track_step"]["largest"]["K"]
    with _memory(T, name):
        state = _bank_steps(T, lib, c, None, (c["outs"], c["state"]))
        o = _link_ops(T, c)
        batch = lib.link_pairs(o["first"], o["second"], o["matches"], o["count"], c["n_bank"], k, mask=o["mask"])
        batch.update(lib.track_ids(batch["prev"], batch["prev_frame"]))
        _equal_tensors(T, state, batch, lib.LINK_KEYS + ("track_id", "age"), name + ", the state against the batch entries")
        assert int(state["next_id"][0]) == int(batch["n_tracks"][0])
        far = _bank_steps(T, lib, c, c["matches_far"], (c["outs_far"], c["state_far"]))
        assert _differs(T, far["prev"], state["prev"]) and _differs(T, far["track_id"], state["track_id"])
        st = [state[key] for key in lib.TRACK_STATE_KEYS]
        out = lib.alloc_track_out(k)
        outs = [out[key] for key in lib.TRACK_OUT_KEYS]
        before = {key: v.clone() for key, v in state.items()}
        one = T.zeros(1, dtype=T.int32, device="cuda")
        _refused(T, lib.track_launch_count, lambda: lib.track().sslt_track_step(*[_ptr(t) for t in st], _ptr(o["matches"]), _ptr(one), None, _ptr(one), k, k + 1,
                                                                                3, *[_ptr(t) for t in outs], None), tt.E_UNSUPPORTED, outs, "K 4097")
        _equal_tensors(T, state, before, lib.TRACK_STATE_KEYS, name + ", the state after the refused call")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.alloc_track_state(3, k + 1)
        del state, far, o, batch, st, out, outs, before


def _blocks(T, c, key, rows=None, last=None, dtype=None):
    """The operand `key` of the big bank: (n_bank, ...) with frame 4 j + i the frame i of block j's distinct block, and the lone last
    frame `last`.  rows: the distinct blocks (d, 4, ...) where they are not c[key]."""
    nb, marked = c["n_blocks"], c["marked"]
    d = pd.n_distinct(marked)
    distinct = _dev(T, (c[key] if rows is None else rows)[:d])
    out = T.empty((c["n_bank"],) + tuple(distinct.shape[2:]), dtype=distinct.dtype, device="cuda")
    pd.build(distinct, nb, marked, out=out[:nb * oc.BLOCK].view((nb, oc.BLOCK) + tuple(distinct.shape[2:])))
    out[c["n_bank"] - 1] = last
    return out


def _rows_of_pairs(T, c, key):
    """The per-row operand `key` (matches, count, mask) of the big bank's 32 776 rows."""
    nb, marked = c["n_blocks"], c["marked"]
    t = pd.build(_dev(T, c[key][:pd.n_distinct(marked)]), nb, marked)
    return t.view((nb * oc.BLOCK,) + tuple(t.shape[2:]))


def test_link_pairs_past_2_31(T, lib):
    """32 776 rows (i, i + 1) at K = n1 = 4096: matches is 2.148 GB, 134 M nodes.  prev and next of every block against its distinct
    block's; then the last link of the last block moved."""
    c = oc.link_pairs_past_2_31()
    name, nb, marked, k, n_bank, n_pairs = c["name"], c["n_blocks"], c["marked"], c["K"], c["n_bank"], c["n_pairs"]
    d = pd.n_distinct(marked)
    assert n_pairs * k * 16 > 1 << 31 and n_bank * k <= tt.LIMITS["sslt_link_pairs"]["largest"]["nodes"]
    with _memory(T, name):
        matches, count, mask = (_rows_of_pairs(T, c, key) for key in ("matches", "count", "mask"))
        assert matches.numel() * 8 > 1 << 31
        first = T.arange(n_pairs, dtype=T.int32, device="cuda")
        second = first + 1
        links = lib.link_pairs(first, second, matches, count, n_bank, k, mask=mask)
        expected = {key: _dev(T, c[key][:d]) for key in ("prev", "next")}
        view = lambda t: t[:n_bank - 1].view(nb, oc.BLOCK, k)      # noqa: E731
        for key in ("prev", "next"):
            pd.report(view(links[key]), expected[key], marked, f"{name}, {key}")
            assert bool((links[key][n_bank - 1] == -1).all())
        frames = T.arange(n_bank, dtype=T.int32, device="cuda")
        assert T.equal(links["prev_frame"], frames - 1)
        frames[n_bank - 1] = -2
        assert T.equal(links["next_frame"], frames + 1)
        matches.view(nb, oc.BLOCK, k, 2)[nb - 1] = _dev(T, c["matches"][d])
        links = lib.link_pairs(first, second, matches, count, n_bank, k, mask=mask)
        _far_end(T, name, nb, marked, expected, {key: c[key][d] for key in expected}, {key: view(links[key]) for key in expected}, ("prev", "next"))
        del matches, count, mask, first, second, links, expected, frames


def _big_links(T, c, far=False):
    """prev, next, prev_frame, next_frame of a bank of blocks on the device, from the distinct blocks' links (c["prev"], c["next"])."""
    lk = c
    d = pd.n_distinct(c["marked"])
    n_bank = c["n_bank"]
    out = {key: _blocks(T, c, key, lk[key], -1) for key in ("prev", "next")}
    if far:
        for key in out:
            out[key][n_bank - 1 - oc.BLOCK:n_bank - 1] = _dev(T, lk[key][d])
    frames = T.arange(n_bank, dtype=T.int32, device="cuda")
    out["prev_frame"] = frames - 1
    out["next_frame"] = frames + 1
    out["next_frame"][n_bank - 1] = -1
    return out


def test_track_ids_past_2_31(T, lib):
    """The 134 M-node bank of the link case: a 2.7 GB workspace, 131 k scan tiles in 513 chunks.  The expectation is the frame-by-frame
    restatement in torch on the device (tests/test_online_limit_cases_cpu.py holds it to track_ref on small banks)."""
    c = oc.link_pairs_past_2_31()
    name, n_bank, k = "track_ids_past_2_31", c["n_bank"], c["K"]
    assert tt.workspace_bytes(n_bank, k) > 1 << 31 and -(-n_bank * k // tt.SCAN_TILE) > 131000
    with _memory(T, name):
        links = _big_links(T, c)
        want, state = track_ids_by_frames(T, links["prev"], links["prev_frame"])
        assert int(want["n_tracks"][0]) == c["n_blocks"] * c["tracks_per_block"] + k
        n0 = lib.track_launch_count()
        got = lib.track_ids(links["prev"], links["prev_frame"])
        assert lib.track_launch_count() - n0 == tt.launches("sslt_track_ids", n_bank)
        _equal_tensors(T, got, want, lib.TRACK_ID_KEYS, name)
        far = _big_links(T, c, far=True)
        assert _differs(T, far["prev"], links["prev"])
        del links
        want2, _ = track_ids_by_frames(T, far["prev"], far["prev_frame"], resume=state + (n_bank - 1 - oc.BLOCK,))
        assert _differs(T, want2["root_slot"], want["root_slot"]) and T.equal(want2["n_tracks"], want["n_tracks"])
        del want, state
        got = lib.track_ids(far["prev"], far["prev_frame"], out=got)
        _equal_tensors(T, got, want2, lib.TRACK_ID_KEYS, name + ", the last link moved")
        del got, want2, far


PER_TRACK = ("xyz", "n_obs", "n_kept", "status", "weight_sum", "rms")


@pytest.mark.parametrize("which", ["landmarks_past_2_31", "landmarks_poses_past_2_31"])
def test_landmarks_past_2_31(T, lib, which):
    """landmarks_past_2_31: the 134 M-node bank through sslt_landmarks, xyz is 3.2 GB.  landmarks_poses_past_2_31: 22 369 641 frames of
    4 keypoints, the poses are 2.1475 GB.  Every block's tracks and four frames of residual and kept against its distinct block's,
    the last frame's K tracks of one member, the rows past n_tracks; then the last block's last link moved, or the last element of
    its last pose: the last block's rows change, no other."""
    c = getattr(oc, which)()
    name, nb, marked, k, n_bank, nt = c["name"], c["n_blocks"], c["marked"], c["K"], c["n_bank"], c["tracks_per_block"]
    d = pd.n_distinct(marked)
    assert (n_bank * k * 24 if which == "landmarks_past_2_31" else n_bank * 96) > 1 << 31
    with _memory(T, name):
        ops = {key: _blocks(T, c, key, None, _dev(T, c[key][d + 1][0])) for key in ("kp", "depth", "C", "weight")}
        expected = {key: _dev(T, np.ascontiguousarray(c["want"][key][:d])) for key in lib.LANDMARK_KEYS}
        lone = {key: _dev(T, c["lone"][key]) for key in lib.LANDMARK_KEYS}

        def run(far):
            links = _big_links(T, c, far)
            if far:
                for key, t in ops.items():
                    t[n_bank - 1 - oc.BLOCK:n_bank - 1] = _dev(T, c[key][d])
            ids = lib.track_ids(links["prev"], links["prev_frame"])
            assert int(ids["n_tracks"][0]) == nb * nt + k
            n0 = lib.track_launch_count()
            got = lib.landmarks(ops["kp"], ops["depth"], ops["C"], oc.tc.CAMERA, links["next"], links["next_frame"], ids["root_frame"], ids["root_slot"],
                                ids["n_tracks"], weight=ops["weight"])
            assert lib.track_launch_count() - n0 == tt.launches("sslt_landmarks")
            return got

        def views(got):
            v = {key: got[key][:nb * nt].view((nb, nt) + tuple(got[key].shape[1:])) for key in PER_TRACK}
            v.update({key: got[key][:n_bank - 1].view(nb, oc.BLOCK, k) for key in ("residual", "kept")})
            return v

        got = run(False)
        for key, v in views(got).items():
            pd.report(v, expected[key], marked, f"{name}, {key}")
        for key in PER_TRACK:
            _same(T, got[key][nb * nt:nb * nt + k], c["lone"][key], f"{name}, the last frame's tracks, {key}")
            rest = _raw(T, got[key][nb * nt + k:])
            assert bool((rest == (-1 if key == "status" else 0)).all()), f"{name}, {key}: the rows past n_tracks"
        for key in ("residual", "kept"):
            _same(T, got[key][n_bank - 1], c["lone"][key][0], f"{name}, the last frame, {key}")
        del got
        got = run(True)
        _far_end(T, name, nb, marked, expected, {key: c["want"][key][d] for key in expected}, views(got),
                 ("xyz", "n_kept", "residual", "kept") if which == "landmarks_past_2_31" else ("xyz", "residual"))
        for key in PER_TRACK:
            _same(T, got[key][nb * nt:nb * nt + k], c["lone"][key], f"{name}, last link moved, the last frame's tracks, {key}")
        del got, ops, expected, lone


# sslt_landmarks with kp_bank itself past 2^31 bytes takes 65 537 frames of 4096 keypoints: the operands and outputs of that one call are 88
# bytes a node, 22.0 GiB, before any expectation - past the 22 GiB that case was given.  It is not run (profiles/online_limits.txt, finding 3;
# tests/test_online_limit_cases_cpu.py holds the arithmetic).


def test_track_step_past_2_31(T, lib):
    """capacity * K = 600 M nodes, 2.4 GB a state array.  Steps at t = 131 072 (byte 2^31 of prev) with a link row, at t + 1 without,
    at capacity - 1 with the row (t + 1, capacity - 1), and on the full bank.  Only the rows of those frames change."""
    c = oc.track_step_past_2_31()
    name, k, cap, t, rows = c["name"], c["K"], c["capacity"], c["t"], c["rows"]
    assert cap * k * 4 > 1 << 31 and t * k * 4 == 1 << 31
    with _memory(T, name):
        shapes = lib.track_state_shapes(cap, k)
        state = {key: T.full(shape, FILL, dtype=dt, device="cuda") for key, (shape, dt) in shapes.items()}
        state["track_id"][t - 1], state["age"][t - 1] = _dev(T, c["filled"]["track_id"]), _dev(T, c["filled"]["age"])
        state["next"][t - 1], state["next_frame"][t - 1] = -1, -1
        state["t"][0], state["next_id"][0] = t, 5000
        out = lib.alloc_track_out(k)
        o = _link_ops(T, rows)
        far_matches = _dev(T, rows["matches_far"][1])
        first = T.zeros(1, dtype=T.int32, device="cuda")

        def step(i, r, matches=None, what=c["outs"]):
            first[0] = c["first"][i]
            got = lib.track_step(state, o["matches"][r] if matches is None else matches, o["count"][r:r + 1], first, mask=o["mask"][r], out=out)
            _same_dict(T, got, what[i], lib.TRACK_OUT_KEYS, f"{name}, step {i}")

        def check(want, what):
            frames = c["frames"]
            for key in ("prev", "next", "track_id", "age"):
                for i, f in enumerate(frames):
                    if i or key == "next":
                        _same(T, state[key][f], want[key][i], f"{what}, {key} of frame {f}")
                touched = T.nonzero((state[key] != FILL).any(dim=1)).flatten().tolist()
                assert touched == (frames if key in ("next", "track_id", "age") else frames[1:]), f"{what}, {key}: rows {touched[:8]} were written"
            for key in ("prev_frame", "next_frame"):
                got = state[key][frames].tolist()
                assert got[1:] == want[key][1:].tolist() and (key == "prev_frame" or got[0] == want[key][0]), (what, key, got)
                touched = T.nonzero(state[key] != FILL).flatten().tolist()
                assert touched == (frames if key == "next_frame" else frames[1:]), f"{what}, {key}: frames {touched[:8]} were written"
            assert int(state["t"][0]) == cap and int(state["next_id"][0]) == want["next_id"]

        step(0, 0)
        step(1, 1)
        assert int(state["t"][0]) == t + 2
        id_before = int(state["next_id"][0])
        state["t"][0] = cap - 1
        step(2, 1)
        step(3, 1)                                                       # the bank is full: status 4, nothing written
        check(c["state"], name)
        state["t"][0], state["next_id"][0] = cap - 1, id_before
        state["next_frame"][t + 1], state["next"][t + 1] = -1, -1
        step(2, 1, far_matches, c["outs_far"])
        check(c["state_far"], name + ", the last link's idx2 changed")
        assert _differs(T, _dev(T, c["state_far"]["prev"][3]), _dev(T, c["state"]["prev"][3]))
        outs = [out[key] for key in lib.TRACK_OUT_KEYS]
        st = [state[key] for key in lib.TRACK_STATE_KEYS]
        one_past = (1 << 31) // k
        _refused(T, lib.track_launch_count, lambda: lib.track().sslt_track_step(*[_ptr(x) for x in st], _ptr(o["matches"]), _ptr(o["count"]), None, _ptr(first), k,
                                                                                k, one_past, *[_ptr(x) for x in outs], None), tt.E_UNSUPPORTED, outs,
                 "capacity * K 2^31")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.check_track_sizes("track_step", one_past, k, limit_k=True)
        del state, out, o, far_matches, first, outs, st


# =============================================================================================================== libsslam_place.so
def _place_state(T, st):
    return dict(t=_dev(T, np.asarray(st["t"], np.int32).reshape(1)), raw=_dev(T, st["raw"]), sum=_dev(T, st["sum"]))


def _place_run(T, lib, c, which, far, what):
    outs, final = oc.place_expected(which, far)
    state = _place_state(T, c["far_state"] if far else c["state"])
    out = lib.alloc_place_out(c["per_frame"], c["d"])
    desc, scores = _dev(T, c["desc"]), _dev(T, c["scores"])
    for i, want in enumerate(outs):
        s = int(c["slot"][min(c["t0"] + i, c["capacity"] - 1)])
        n0 = lib.place_launch_count()
        got = lib.place_step(state, desc[s], scores[s], c["min_gap"], c["min_sim"], c["per_frame"], oc.SUPPRESS[which], out=out)
        assert lib.place_launch_count() - n0 == 3
        _same_dict(T, got, want, lib.PLACE_OUT_KEYS, f"{what}, t = {c['t0'] + i}")
    _same_dict(T, state, dict(final, t=np.asarray(final["t"]).reshape(1)), lib.PLACE_STATE_KEYS, f"{what}, the state")
    return outs, state, out


def test_bank_at_the_capacity_limit(T, lib):
    """capacity 4096, d 256, per_frame 8: the steps at t = 4094 and 4095 on the restatement's uploaded state, then one on the full
    bank.  S[4096] of pick_kernel to its end, all 128 similarity groups, picks under three values of suppress.  capacity 4097 and
    per_frame 9 are refused."""
    c = oc.bank_at_the_capacity_limit()
    name = c["name"]
    L = pt.LIMITS["sslp_place_step"]["largest"]
    assert (c["capacity"], c["d"], c["per_frame"]) == (L["capacity"], L["d"], L["per_frame"])
    with _memory(T, name):
        for which in oc.SUPPRESS:
            outs, state, out = _place_run(T, lib, c, which, False, f"{name}, {which}")
            print(f"{name}, {which}: counts {[int(o['count'][0]) for o in outs]}")
        base = oc.place_expected("exactly_8")[0][0]
        outs, state, out = _place_run(T, lib, c, "exactly_8", True, f"{name}, raw[4064, 255] changed")
        at = base["first"].tolist().index(4064)
        assert outs[0]["sim"][at] != base["sim"][at] and np.array_equal(np.delete(outs[0]["sim"], at), np.delete(base["sim"], at))
        st, o = [state[key] for key in lib.PLACE_STATE_KEYS], [out[key] for key in lib.PLACE_OUT_KEYS]
        desc, scores = _dev(T, c["desc"][0]), _dev(T, c["scores"][0])
        ws = T.empty(4 * c["capacity"], dtype=T.uint8, device="cuda")
        entry = lambda cap, per: lib.place().sslp_place_step(*[_ptr(x) for x in st], _ptr(desc), _ptr(scores), cap, c["k"], c["d"], 30, C.c_float(0.3), per,      # noqa: E731
                                                             5, _ptr(ws), *[_ptr(x) for x in o], None)
        before = {key: v.clone() for key, v in state.items()}
        _refused(T, lib.place_launch_count, lambda: entry(c["capacity"] + 1, 8), pt.E_UNSUPPORTED, o, "capacity 4097")
        _refused(T, lib.place_launch_count, lambda: entry(c["capacity"], 9), pt.E_UNSUPPORTED, o, "per_frame 9")
        _equal_tensors(T, state, before, lib.PLACE_STATE_KEYS, name + ", the state after the refused calls")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.place_step(dict(state, raw=T.zeros((c["capacity"] + 1, c["d"]), device="cuda")), desc, scores)
        del state, out, st, o, desc, scores, ws, before


def test_bank_at_the_keypoint_limit(T, lib):
    """k 4096, d 256: raw_kernel's 4096-step chains.  Four steps of a bank of five; then the last descriptor element changed.
    k = 4097 is refused."""
    c = oc.bank_at_the_keypoint_limit()
    name, k, d = c["name"], c["k"], c["d"]
    assert k == pt.LIMITS["sslp_place_step"]["largest"]["k"]
    with _memory(T, name):
        for desc_np, outs, final, what in ((c["desc"], c["outs"], c["state"], name), (c["desc_far"], c["outs_far"], c["state_far"], name + ", last element changed")):
            state, out = lib.alloc_place_state(c["capacity"], d), lib.alloc_place_out(c["per_frame"], d)
            desc, scores = _dev(T, desc_np), _dev(T, c["scores"])
            for i, want in enumerate(outs):
                got = lib.place_step(state, desc[i], scores[i], c["min_gap"], c["min_sim"], c["per_frame"], c["suppress"], out=out)
                _same_dict(T, got, want, lib.PLACE_OUT_KEYS, f"{what}, t = {i}")
            _same_dict(T, state, dict(final, t=np.asarray(final["t"]).reshape(1)), lib.PLACE_STATE_KEYS, f"{what}, the state")
        assert c["outs_far"][-1]["sig"].tobytes() != c["outs"][-1]["sig"].tobytes()
        st, o = [state[key] for key in lib.PLACE_STATE_KEYS], [out[key] for key in lib.PLACE_OUT_KEYS]
        ws = T.empty(4 * c["capacity"], dtype=T.uint8, device="cuda")
        _refused(T, lib.place_launch_count, lambda: lib.place().sslp_place_step(*[_ptr(x) for x in st], _ptr(desc), _ptr(scores), c["capacity"], k + 1, d, 1,
                                                                                C.c_float(-2.0), 2, 0, _ptr(ws), *[_ptr(x) for x in o], None),
                 pt.E_UNSUPPORTED, o, "k 4097")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.place_step(state, T.zeros((k + 1, d), device="cuda"), T.zeros(k + 1, device="cuda"))
        del state, out, desc, scores, st, o, ws


LOG_FILL = dict(log_first=77, log_second=78, log_T=5.0, log_info=6.0)


def test_edge_log_past_2_31(T, lib):
    """n_slots 16, capacity 800 000: log_info is 2.15 GB.  One step at the frame whose rows hold its byte 2^31, one at capacity - 1,
    one on the full log: only those two frames' rows change in the four logs.  n_slots 17 is refused."""
    c = oc.edge_log_past_2_31()
    name, E, cap = c["name"], c["n_slots"], c["capacity"]
    assert cap * E * 168 > 1 << 31 and E == pt.LIMITS["sslp_edge_log_step"]["largest"]["n_slots"]
    with _memory(T, name):
        shapes = lib.edge_log_shapes(cap, E)
        state = {key: T.empty(shape, dtype=dt, device="cuda") for key, (shape, dt) in shapes.items()}
        for key, v in LOG_FILL.items():
            state[key].fill_(v)
        assert state["log_info"].numel() * 8 > 1 << 31
        out = {key: T.zeros(shape, dtype=dt, device="cuda") for key, (shape, dt) in lib.edge_log_out_shapes(E).items()}

        def step(s, what):
            state["t"][0] = s["t"]
            ins = [_dev(T, s["ins"][key]) for key in ("slot_first", "new_T", "new_info", "new_status", "new_inliers")]
            n0 = lib.place_launch_count()
            got = lib.edge_log_step(state, *ins, c["n_odometry"], c["min_inliers"], c["loop_min_inliers"], out=out)
            assert lib.place_launch_count() - n0 == 1
            _same_dict(T, got, s["out"], lib.EDGE_LOG_OUT_KEYS, what)
            assert int(state["t"][0]) == s["t_after"]
            return ins

        def check(steps, what):
            frames = [s["t"] for s in steps]
            for key, fill in LOG_FILL.items():
                for s in steps:
                    _same(T, state[key][s["t"] * E:(s["t"] + 1) * E], s["rows"][key], f"{what}, {key} of frame {s['t']}")
                log = state[key].view(cap, -1)
                touched = T.nonzero((log != fill).any(dim=1)).flatten().tolist()
                assert touched == frames, f"{what}, {key}: the frames {touched[:8]} were written"
                print(f"{what}, {key}: 0 mismatching rows outside the frames {frames}")

        for i, s in enumerate(c["steps"]):
            ins = step(s, f"{name}, step {i} at t = {s['t']}")
        assert c["steps"][2]["out"]["status"][0] == 4 and c["steps"][0]["t"] == c["t_far"]
        check(c["steps"][:2], name)
        step(c["far"], f"{name}, the last element of new_info changed")
        check([c["steps"][0], c["far"]], name + ", the last element of new_info changed")
        assert c["far"]["rows"]["log_info"].tobytes() != c["steps"][1]["rows"]["log_info"].tobytes()
        st, o = [state[key] for key in lib.EDGE_LOG_STATE_KEYS], [out[key] for key in lib.EDGE_LOG_OUT_KEYS]
        state["t"][0] = 5
        _refused(T, lib.place_launch_count, lambda: lib.place().sslp_edge_log_step(*[_ptr(x) for x in st], *[_ptr(x) for x in ins], E + 1, 8, 12, 20, cap,
                                                                                   *[_ptr(x) for x in o], None), pt.E_UNSUPPORTED, o, "n_slots 17")
        assert int(state["t"][0]) == 5
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.check_edge_log_sizes(cap, E + 1)
        del state, out, ins, st, o


# ============================================================================================================== libsslam_window.so
def test_windows_at_the_count_limit(T, lib):
    """65 535 windows of 2 frames, capacity 400: the trajectory is 2.5 GB, the workspace 12.1 GB.  Six steps, every output of every
    step and the whole state; then the last step again with one element of the last window's new_T changed.  65 536 windows are
    refused."""
    c = oc.windows_at_the_count_limit()
    name, n, marked, cap, steps = c["name"], c["n"], c["marked"], c["capacity"], c["steps"]
    d = pd.n_distinct(marked)
    assert n == wnt.LIMITS["sslw_window_step"]["largest"]["n_windows"] and n * cap * 96 > 1 << 31
    with _memory(T, name):
        state = lib.alloc_window_state(2, 1, cap, n)
        state["trajectory"].fill_(7.25)
        assert state["trajectory"].numel() * 8 > 1 << 31
        out = lib.alloc_window_out(2, 1, n)
        ws = T.empty(lib.window_workspace_bytes(n, 2, 1), dtype=T.uint8, device="cuda")
        assert ws.numel() == c["workspace_bytes"] > 12 * 10 ** 9
        sp = _dev(T, c["spacings"])
        keys = ("T", "info", "status", "inliers")
        args = (None, c["min_inliers"], c["chi"], c["damping"], c["n_iter"])

        def inputs(i):
            return [pd.build(_dev(T, np.ascontiguousarray(c["ins"][key][i])), n, marked) for key in keys]

        st, o = [state[key] for key in lib.WINDOW_STATE_KEYS], [out[key] for key in lib.WINDOW_OUT_KEYS]
        ins = inputs(0)
        _refused(T, lib.window_launch_count, lambda: lib.window().sslw_window_step(*[_ptr(x) for x in st], _ptr(sp), *[_ptr(x) for x in ins], None, n + 1, 2, 1,
                                                                                   c["min_inliers"], C.c_double(c["chi"]), C.c_double(c["damping"]), c["n_iter"], cap,
                                                                                   _ptr(ws), *[_ptr(x) for x in o], None), wnt.E_UNSUPPORTED, o, "65 536 windows")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.check_window_sizes(2, 1, cap, n + 1)
        for key in lib.WINDOW_OUT_KEYS:
            out[key].zero_()
        for i in range(steps):
            if i == steps - 1:
                small = {key: state[key].clone() for key in lib.WINDOW_STATE_KEYS if key != "trajectory"}
                rows = state["trajectory"][:, steps - 2:steps].clone()
            ins = inputs(i)
            n0 = lib.window_launch_count()
            got = lib.window_step(state, sp, *ins, *args, out=out, workspace=ws)
            assert lib.window_launch_count() - n0 == 1
            for key in lib.WINDOW_OUT_KEYS:
                pd.report(got[key].view(n, -1), _dev(T, c["want"][i][key]).view(d, -1), marked, f"{name}, step {i}, {key}")
        expected = {key: _dev(T, c["state"][key]).view(d, -1) for key in lib.WINDOW_STATE_KEYS}
        for key in lib.WINDOW_STATE_KEYS:
            pd.report(state[key].view(n, -1), expected[key], marked, f"{name}, the state, {key}")
        for key, v in small.items():
            state[key].copy_(v)
        state["trajectory"][:, steps - 2:steps] = rows
        ins[0][n - 1] = _dev(T, c["T_far"])
        got = lib.window_step(state, sp, *ins, *args, out=out, workspace=ws)
        exp_out = {key: _dev(T, c["want"][steps - 1][key]).view(d, -1) for key in lib.WINDOW_OUT_KEYS}
        _far_end(T, name, n, marked, exp_out, {key: np.asarray(c["out_far"][key]).reshape(-1) for key in exp_out}, {key: got[key].view(n, -1) for key in exp_out},
                 ("C_window",))
        _far_end(T, name + ", the state", n, marked, expected, {key: np.asarray(c["state_far"][key]).reshape(-1) for key in expected},
                 {key: state[key].view(n, -1) for key in expected}, ("ring_T", "trajectory"))
        del state, out, ws, sp, st, o, ins, small, rows, expected, exp_out, got


def test_window_at_a_far_frame(T, lib):
    """One window whose trajectory holds 22 369 700 frames, 2.1475 GB: steps at the frame whose row holds byte 2^31, at the next, at
    capacity - 1 and at capacity.  Five rows of the trajectory are written, no other."""
    c = oc.window_at_a_far_frame()
    name, cap = c["name"], c["capacity"]
    assert cap * 96 > 1 << 31
    with _memory(T, name):
        state = lib.alloc_window_state(2, 1, cap)
        state["trajectory"].fill_(7.25)

        def load(small, t):
            for key, v in small.items():
                state[key].copy_(_dev(T, np.asarray(v)).view(state[key].shape))
            state["t"][0] = t

        def step(i, T_new=None):
            ins = [_dev(T, np.ascontiguousarray(c["ins"][key][i])) for key in ("T", "info", "status", "inliers")]
            if T_new is not None:
                ins[0] = _dev(T, T_new)
            return lib.window_step(state, sp, *ins, None, c["min_inliers"], c["chi"], c["damping"], c["n_iter"], out=out)

        def check(rows, what):
            for f, want in rows.items():
                _same(T, state["trajectory"][0, f], want, f"{what}, the trajectory's row {f}")
            touched = T.nonzero((state["trajectory"][0] != 7.25).any(dim=1)).flatten().tolist()
            assert touched == sorted(rows), f"{what}: the rows {touched[:8]} of the trajectory were written"
            print(f"{what}: 0 mismatching rows outside the frames {sorted(rows)}")

        out, sp = lib.alloc_window_out(2, 1), _dev(T, c["spacings"])
        load(c["start"], c["t0"])
        for i, t in enumerate(c["frames"]):
            state["t"][0] = t
            _same_dict(T, step(i), c["outs"][i], lib.WINDOW_OUT_KEYS, f"{name}, t = {t}")
        check(c["rows"], name)
        _same_dict(T, {key: state[key] for key in c["final"]}, c["final"], list(c["final"]), name + ", the state")
        load(c["before_third"], cap - 1)
        _same_dict(T, step(2, c["T_far"]), c["out_far"], lib.WINDOW_OUT_KEYS, f"{name}, new_T changed, t = {cap - 1}")
        assert c["rows_far"][cap - 1].tobytes() != c["rows"][cap - 1].tobytes()
        check({**c["rows"], **c["rows_far"]}, name + ", new_T changed")
        del state, out, sp


# ================================================================================================================ libsslam_conf.so
def _packed(T, lib):
    return _dev(T, lib.confidence_pack(oc.conf_weights()))


@pytest.mark.parametrize("which", list(oc.CONF_ROWS))
def test_confidence_rows_past_2_31(T, lib, which):
    """1 450 003 rows at D = 256: x is 2.23 GB; 2 100 003 rows: desc passes 2^31 bytes too.  The last tile is ragged and the XCD split
    has a remainder."""
    c = oc.confidence_rows(which)
    name, n, marked = c["name"], c["n"], c["marked"]
    d = pd.n_distinct(marked)
    with _memory(T, name):
        packed = _packed(T, lib)
        x, desc = pd.build(_dev(T, c["x"]), n, marked), pd.build(_dev(T, c["desc"]), n, marked)
        assert x.numel() * 4 > 1 << 31 and n <= ct.LIMITS["sslc_confidence_rows"]["largest"]["rows"]
        assert (desc.numel() * 4 > 1 << 31) == (which == "confidence_rows_desc_past_2_31")
        expected = _dev(T, c["want"]).view(d, 1)
        n0 = lib.conf_launch_count()
        out = lib.confidence_rows(x, desc, packed)
        assert lib.conf_launch_count() - n0 == 1 and out.shape == (n,)
        pd.report(out.view(n, 1), expected, marked, name)
        x[n - 1] = _dev(T, c["x_far"])
        out = lib.confidence_rows(x, desc, packed, out=out)
        _far_end(T, name, n, marked, dict(conf=expected), dict(conf=np.asarray(c["want_far"]).reshape(1)), dict(conf=out.view(n, 1)), ("conf",))
        _refused(T, lib.conf_launch_count, lambda: lib.conf().sslc_confidence_rows(_ptr(x), _ptr(desc), 1 << 31, c["D"], _ptr(packed), _ptr(out), None),
                 ct.E_UNSUPPORTED, [out], "2^31 rows")
        del packed, x, desc, expected, out


def test_gather_confidence_past_2_31(T, lib):
    """G = 40, 3500 frames, K = 5: feat is 2.15e9 floats, 8.6 GB - its float index, not only its byte offset, passes 2^31."""
    c = oc.gather_confidence_past_2_31()
    name, n, marked, k = c["name"], c["n"], c["marked"], c["K"]
    d = pd.n_distinct(marked)
    with _memory(T, name):
        packed = _packed(T, lib)
        feat = pd.build(_dev(T, c["feat"]), n, marked)
        kp, desc = pd.build(_dev(T, c["kp"]), n, marked), pd.build(_dev(T, c["desc"]), n, marked)
        assert feat.numel() > 1 << 31
        expected = _dev(T, c["want"])
        n0 = lib.conf_launch_count()
        out = lib.gather_confidence(feat, kp, desc, packed)
        assert lib.conf_launch_count() - n0 == 1 and out.shape == (n, k)
        pd.report(out, expected, marked, name)
        feat[n - 1] = _dev(T, c["feat_far"])
        out = lib.gather_confidence(feat, kp, desc, packed, out=out)
        _far_end(T, name, n, marked, dict(conf=expected), dict(conf=c["want_far"]), dict(conf=out), ("conf",))
        _refused(T, lib.conf_launch_count, lambda: lib.conf().sslc_gather_confidence(_ptr(feat), 1 << 29, c["G"], _ptr(kp), 4, _ptr(desc), c["D"], _ptr(packed),
                                                                                     _ptr(out), None), ct.E_UNSUPPORTED, [out], "n_frames * K 2^31")
        del packed, feat, kp, desc, expected, out


def test_confidence_filter_past_2_31(T, lib):
    """K = 4096, 131 080 frames: conf, slot and conf_out are 2.15 GB each.  K = 4097 is refused."""
    c = oc.confidence_filter_past_2_31()
    name, n, marked, k = c["name"], c["n"], c["marked"], c["K"]
    d = pd.n_distinct(marked)
    with _memory(T, name):
        conf = pd.build(_dev(T, c["conf"]), n, marked)
        assert conf.numel() * 4 > 1 << 31
        expected = {key: _dev(T, v).view(d, -1) for key, v in c["want"].items()}
        outs = [T.empty(shape, dtype=dt, device="cuda") for shape, dt in lib.confidence_filter_shapes(n, k).values()]
        _refused(T, lib.conf_launch_count, lambda: lib.conf().sslc_confidence_filter(_ptr(conf), n // 2, k + 1, C.c_float(0.5), *[_ptr(t) for t in outs], None),
                 ct.E_UNSUPPORTED, outs, "K 4097")
        with pytest.raises(lib.SslamHipError, match="unsupported"):
            lib.confidence_filter(conf.view(-1)[:2 * (k + 1)].view(2, k + 1))
        n0 = lib.conf_launch_count()
        got = dict(zip(lib.CONF_FILTER_KEYS, lib.confidence_filter(conf, c["threshold"], out=tuple(outs))))
        assert lib.conf_launch_count() - n0 == 1
        for key in lib.CONF_FILTER_KEYS:
            pd.report(got[key].view(n, -1), expected[key], marked, f"{name}, {key}")
        conf[n - 1] = _dev(T, c["conf_far"])
        got = dict(zip(lib.CONF_FILTER_KEYS, lib.confidence_filter(conf, c["threshold"], out=tuple(outs))))
        _far_end(T, name, n, marked, expected, {key: np.asarray(v).reshape(-1) for key, v in c["want_far"].items()},
                 {key: got[key].view(n, -1) for key in expected}, lib.CONF_FILTER_KEYS)
        del conf, expected, outs, got


@pytest.mark.parametrize("name", list(oc.TAKE_SHAPES))
def test_take_rows(T, lib, name):
    """width 256.  K = 16, 131 080 frames: src and dst are 2.15 GB each.  K = 47, 178 481 frames: 2 147 483 392 words, 8.6 GB each, the
    most the entry takes at this width.  One frame more than that, and 2^31 words, are refused."""
    c = oc.take_rows(name)
    name, n, marked, k, w = c["name"], c["n"], c["marked"], c["K"], c["width"]
    with _memory(T, name):
        src, slot = pd.build(_dev(T, c["src"]), n, marked), pd.build(_dev(T, c["slot"]), n, marked)
        assert src.numel() * 4 > 1 << 31
        expected = _dev(T, c["want"])
        dst = T.empty_like(src)
        _refused(T, lib.conf_launch_count, lambda: lib.conf().sslc_take_rows(_ptr(src), _ptr(slot), 1 << 23, 1, w, _ptr(dst), None), ct.E_UNSUPPORTED, [dst],
                 "2^31 words")
        _refused(T, lib.conf_launch_count, lambda: lib.conf().sslc_take_rows(_ptr(src), _ptr(slot), oc.TAKE_SHAPES["take_rows_at_the_word_limit"][0] + 1, 47, w,
                                                                             _ptr(dst), None), ct.E_UNSUPPORTED, [dst], "one frame past the word limit")
        n0 = lib.conf_launch_count()
        assert lib.take_rows(src, slot, out=dst) is dst and lib.conf_launch_count() - n0 == 1
        pd.report(dst, expected, marked, name)
        slot[n - 1] = _dev(T, c["slot_far"])
        lib.take_rows(src, slot, out=dst)
        _far_end(T, name, n, marked, dict(dst=expected), dict(dst=c["want_far"]), dict(dst=dst), ("dst",))
        del src, slot, expected, dst


# ============================================================================================================== libsslam_weight.so
def _pair_lists(T, c):
    a, b = oc.pair_frames(c["n"], c["marked"], c["periods"])
    return _dev(T, a.astype(np.int32)), _dev(T, b.astype(np.int32))


@pytest.mark.parametrize("mode", [wt.WEIGHT_PRODUCT, wt.WEIGHT_EXPECTED_ERROR])
def test_match_weights_past_2_31(T, lib, mode):
    """n1 = 4096, 32 776 pairs: matches is 2.148 GB, conf_bank 2.1476 GB, read all over.  n_pairs * n1 = 2^31 is refused."""
    c = oc.match_weights_past_2_31()
    name, n, marked, k = f"{c['name']}, mode {mode}", c["n"], c["marked"], c["K"]
    d = pd.n_distinct(marked)
    with _memory(T, name):
        bank = _dev(T, c["conf"]).repeat(c["periods"], 1)
        matches, count = pd.build(_dev(T, c["matches"]), n, marked), pd.build(_dev(T, c["count"]), n, marked)
        assert matches.numel() * 8 > 1 << 31 and bank.numel() * 4 > 1 << 31 and bank.shape == (c["n_bank"], k)
        first, second = _pair_lists(T, c)
        first[pd.slots(n, marked, "cuda") == c["absent"]] = c["n_bank"]        # past the bank: absent pairs
        expected = _dev(T, c["want"][mode])
        out = T.empty((n, k), dtype=T.float32, device="cuda")
        _refused(T, lib.weight_launch_count, lambda: lib.weight().sslu_match_weights(_ptr(bank), c["n_bank"], k, _ptr(first), _ptr(second), 1 << 19, _ptr(matches),
                                                                                     _ptr(count), k, mode, C.c_double(0.5), _ptr(out), None),
                 wt.E_UNSUPPORTED, [out], "n_pairs * n1 2^31")
        n0 = lib.weight_launch_count()
        assert lib.match_weights(bank, first, second, matches, count, mode, c["sigma0"], out=out) is out and lib.weight_launch_count() - n0 == 1
        pd.report(out, expected, marked, name)
        matches[n - 1] = _dev(T, c["matches_far"])
        lib.match_weights(bank, first, second, matches, count, mode, c["sigma0"], out=out)
        _far_end(T, name, n, marked, dict(weight=expected), dict(weight=c["want_far"][mode]), dict(weight=out), ("weight",))
        del bank, matches, count, first, second, expected, out


def test_weighted_refine_past_2_31(T, lib):
    """sslu_pose_refine_weighted_pairs on 32 776 pairs at K = n1 = 4096, one iteration: matches is 2.148 GB, kp_bank 2.1476 GB.
    K = 4097 is refused."""
    c = oc.weighted_refine_past_2_31()
    name, n, marked, k = c["name"], c["n"], c["marked"], c["K"]
    d = pd.n_distinct(marked)
    keys = lib.POSE_REFINE_WEIGHTED_KEYS
    with _memory(T, name):
        bank, depth = _dev(T, c["bank"]).repeat(c["periods"], 1, 1), _dev(T, c["depth_bank"]).repeat(c["periods"], 1)
        matches, count = pd.build(_dev(T, c["matches"]), n, marked), pd.build(_dev(T, c["count"]), n, marked)
        weight, T_in = pd.build(_dev(T, c["weight"]), n, marked), pd.build(_dev(T, c["T_in"]), n, marked)
        assert matches.numel() * 8 > 1 << 31 and bank.numel() * 4 > 1 << 31
        first, second = _pair_lists(T, c)
        expected = {key: _dev(T, np.ascontiguousarray(c["want"][key])).view(d, -1) for key in keys}
        shapes = lib.pose_refine_weighted_shapes(n, k)
        outs = [T.empty(shapes[key][0], dtype=shapes[key][1], device="cuda") for key in keys]
        cam = c["cam"]
        doubles = [C.c_double(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.depth_scale, c["scale_x"], c["scale_y"], cam.width, cam.height, c["threshold"])]
        _refused(T, lib.weight_launch_count, lambda: lib.weight().sslu_pose_refine_weighted_pairs(
            _ptr(bank), _ptr(depth), c["n_bank"] // 2, k + 1, _ptr(first), _ptr(second), n, _ptr(matches), _ptr(count), k, *doubles, _ptr(T_in),
            C.c_double(c["huber"]), c["n_iter"], _ptr(weight), *[_ptr(t) for t in outs], None), wt.E_UNSUPPORTED, outs, "K 4097")

        def run():
            n0 = lib.weight_launch_count()
            got = lib.pose_refine_weighted(bank, depth, first, second, matches, count, cam, T_in, weight, c["scale_x"], c["scale_y"], c["threshold"],
                                           c["huber"], c["n_iter"], out=tuple(outs))
            assert lib.weight_launch_count() - n0 == 1
            return {key: t.view(n, -1) for key, t in zip(keys, got)}

        got = run()
        for key in keys:
            pd.report(got[key], expected[key], marked, f"{name}, {key}")
        matches[n - 1] = _dev(T, c["matches_far"])
        _far_end(T, name, n, marked, expected, {key: np.asarray(v).reshape(-1) for key, v in c["want_far"].items()}, run(), ("cost_in", "info"))
        del bank, depth, matches, count, weight, T_in, first, second, expected, outs, got
