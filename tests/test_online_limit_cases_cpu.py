"""The cases of tests/online_limit_cases.py held to what their names say, by the restatements alone and without a device: each
sits at the size its name gives - read from tests/window_table.py, place_table.py, conf_table.py, weight_table.py, track_table.py -,
the named operand passes 2^31 bytes, the marked positions are what tests/periodic.py marks, the restatement takes the paths the device
test relies on, and the far-end change shows in the restatement's output.  One past each limit of the five tables is refused by the
entry - called with pointers it never follows - and by the sslam_amd.lib wrapper with the same verdict.  The frame-by-frame torch
restatement of sslt_track_ids that tests/test_gpu_online_limits.py takes its largest expectation from is held to tests/track_ref.py's
union-find here.  The cases are built once per process (the builders cache)."""
import ctypes as C

import numpy as np
import pytest

import conf_table as ct
import online_limit_cases as oc
import place_table as pt
import track_cases as tc
import track_ref as tr
import track_table as tt
import weight_table as wt
import window_table as wnt
from sslam_amd import track_numpy as tn

FAR = 1 << 31
E_INVALID, E_UNSUPPORTED = -1, -2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.array_equal(_bits(a), _bits(b))


def _periodic(c, n, frame_bytes, extra=()):
    """The marks are periodic.py's for the case's item: 0, the holder of byte 2^31, n - 1 (and `extra`); at most 11 distinct items."""
    import periodic as pd
    marked = c["marked"]
    assert n * frame_bytes > FAR, "the named operand passes 2^31 bytes"
    assert marked == sorted(set(pd.marks(n, frame_bytes)) | set(extra)) and len(set(marked)) == 3 + len(extra)
    assert marked[0] == 0 and marked[1] == FAR // frame_bytes and marked[-1] == n - 1
    assert oc.marks(n, frame_bytes) == pd.marks(n, frame_bytes)
    assert np.array_equal(oc.slots(n, marked), pd.slots(n, marked).numpy())
    assert pd.n_distinct(marked) == oc.P + len(marked) <= 11
    return oc.P + len(marked)


# =============================================================================================================== libsslam_track.so
def _link_set(c):
    """The links of a case's prev as ((frame, slot), (frame, slot)) pairs."""
    prev, pf = c["links"]["prev"], c["links"]["prev_frame"]
    f, s = np.nonzero(prev >= 0)
    return set(zip(zip(pf[f].tolist(), prev[f, s].tolist()), zip(f.tolist(), s.tolist())))


@pytest.mark.parametrize("name", list(oc.IDS_BANKS))
def test_ids_tiles(name):
    c = oc.ids_tiles(name)
    n_bank, k, w = c["n_bank"], c["K"], c["want"]
    n = n_bank * k
    tiles = -(-n // tt.SCAN_TILE)
    assert (n, tiles) == {"ids_tiles_256": (262144, 256), "ids_tiles_257": (262272, 257), "ids_tiles_513": (525312, 513)}[name]
    chunks = -(-tiles // oc.CHUNK_TILES)
    assert chunks == {"ids_tiles_256": 1, "ids_tiles_257": 2, "ids_tiles_513": 3}[name]
    is_root = w["age"].reshape(-1) == 0
    per_tile = np.add.reduceat(is_root.astype(np.int64), np.arange(0, n, tt.SCAN_TILE))
    assert len(per_tile) == tiles and (per_tile > 0).all(), "roots in every tile, so in every chunk of the tile scan"
    assert int(w["n_tracks"][0]) == is_root.sum() > n // 2
    for b in range(1, chunks):                                   # the chains cross every chunk boundary, and ids past it need the carry
        f = b * oc.CHUNK_TILES * tt.SCAN_TILE // k
        assert (w["age"][f, :oc.IDS_LONG] > 0).all() and (c["links"]["prev_frame"][f] == f - 1), f"chains enter frame {f}"
        first_id = int(w["track_id"][f][w["age"][f] == 0].min())
        assert first_id == is_root[:f * k].sum() > 0, "the first root of the chunk takes the carry"
    assert w["age"].max() >= 90 and w["length"].max() >= 90
    assert (c["links"]["prev_frame"][c["gaps"]] == -1).all() and c["links"]["prev_frame"][1002] == 1000 and c["links"]["prev_frame"][1001] == -1
    assert (c["links"]["prev_frame"][[8, 9]] == [7, 8]).all(), "the rows named again are no link rows"
    # the far end: the last node becomes a root - one track more, the last id
    wf = c["want_far"]
    assert c["prev_far"][n_bank - 1, k - 1] == -1 != c["links"]["prev"][n_bank - 1, k - 1]
    assert wf["n_tracks"][0] == w["n_tracks"][0] + 1 == wf["track_id"][n_bank - 1, k - 1] + 1 and wf["root_slot"][w["n_tracks"][0]] == k - 1
    assert (wf["track_id"].reshape(-1)[:-1] == w["track_id"].reshape(-1)[:-1]).all()
    # the method of the header, in numpy: pointer jumping and the tiled scan
    m = tr.track_ids(c["links"]["prev"], c["links"]["prev_frame"])
    for key in tn.TRACK_KEYS:
        assert np.array_equal(m[key], w[key]), key


def test_ids_tiles_257_against_the_union_find():
    """track_numpy's expectation of the 257-tile case against track_ref.brute_force: the definition, no method."""
    c = oc.ids_tiles("ids_tiles_257")
    links, track_id, age, lengths = tr.brute_force(c["first"], c["second"], c["matches"], c["count"], c["mask"], c["n_bank"], c["K"])
    assert links == _link_set(c)
    assert np.array_equal(track_id, c["want"]["track_id"]) and np.array_equal(age, c["want"]["age"])
    assert np.array_equal(lengths, c["want"]["length"][:len(lengths)]) and len(lengths) == c["want"]["n_tracks"][0]


def test_links_and_steps_at_k_4096():
    c = oc.step_k_4096()
    k = c["K"]
    assert k == c["n1"] == tt.LIMITS["sslt_link_pairs"]["largest"]["K"] == tt.LIMITS["sslt_track_step"]["largest"]["K"] == tt.MAX_K and c["n_bank"] == 3
    m, mask = c["matches"], c["mask"]
    for p in range(2):
        for col in (0, 1):
            v = m[p, :, col]
            ok = v[(v >= 0) & (v < k)]
            assert len(np.unique(ok)) < len(ok), "an index named twice"
            assert (v == -1).any() and (v == k).any() and (v == 2 ** 40).any()
        assert (mask[p] == 0).any() and (mask[p] == -1).any()
    by_method = tr.link_pairs(c["first"], c["second"], m, c["count"], mask, 3, k)
    for key in tn.LINK_KEYS:
        assert np.array_equal(by_method[key], c["links"][key]), key
    i1, i2 = c["far_link"]
    assert c["links"]["prev"][2, i2] == i1 and c["links"]["next"][1, i1] == i2 and i2 == k - 1, "the last slot of the last row is a link, to the last node"
    assert c["links_far"]["prev"][2, i2] == -1 and c["links_far"]["next"][1, i1] == -1
    assert (c["links_far"]["prev"] != c["links"]["prev"]).sum() == 1 and c["want_far"]["n_tracks"][0] == c["want"]["n_tracks"][0] + 1
    linked = (c["links"]["prev"][1:] >= 0).sum(axis=1)
    assert (linked > 3500).all() and (linked < k).all()
    assert c["links"]["prev"][1:, -256:].max() >= 0 and (c["links"]["prev"][1:, -256:] == -1).any(), "links and roots in the 16th chunk of the step's scan"
    # the online bank equals the batch restatement
    outs, state = c["outs"], c["state"]
    for key in tn.LINK_KEYS:
        assert np.array_equal(state[key], c["links"][key]), key
    assert np.array_equal(state["track_id"], c["want"]["track_id"]) and np.array_equal(state["age"], c["want"]["age"])
    assert state["next_id"][0] == c["want"]["n_tracks"][0] and [int(o["n_new"][0]) for o in outs] == [k, k - linked[0], k - linked[1]]
    assert _differ(c["state_far"]["prev"], state["prev"]) and c["state_far"]["next_id"][0] == state["next_id"][0] + 1


def test_the_big_bank():
    c = oc.link_pairs_past_2_31()
    k, nb = c["K"], c["n_blocks"]
    d = _periodic(c, nb, oc.BLOCK * k * 16)                              # matches, by blocks of four rows
    assert c["n_pairs"] == 32776 == nb * oc.BLOCK and c["n_bank"] == 32777 and c["n_pairs"] * k * 16 == 2148007936
    assert c["n_bank"] * k <= tt.LIMITS["sslt_link_pairs"]["largest"]["nodes"] and c["n_bank"] * k > 134e6
    assert tt.workspace_bytes(c["n_bank"], k) > 2.68e9 and c["n_bank"] * k * 24 > 3.2e9
    assert c["matches"].shape == (d + 2, oc.BLOCK, k, 2) and c["prev"].shape == (d + 1, oc.BLOCK, k)
    assert c["tracks_per_block"] == 7384
    for g in range(d + 1):
        links, tracks = oc.block_tracks(c, g)
        assert tracks["n_tracks"][0] == c["tracks_per_block"] and sorted(set(tracks["length"][:7384].tolist())) == [1, 2, 3, 4]
        by_method = tr.link_pairs(np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32), c["matches"][g], c["count"][g], c["mask"][g], 5, k)
        assert np.array_equal(by_method["prev"][:4], c["prev"][g]) and np.array_equal(by_method["next"][:4], c["next"][g])
    assert len({c["prev"][g].tobytes() for g in range(d)}) == d, "every distinct block has links of its own"
    changed = np.argwhere(c["matches"][d] != c["matches"][d - 1])
    assert changed.tolist() == [[2, oc.BIG_LINKS - 1, 1]], "the far end: the idx2 of the last link of the last block"
    assert (c["prev"][d] != c["prev"][d - 1]).sum() == 2 and (c["next"][d] != c["next"][d - 1]).sum() == 1
    # the landmarks
    lm = oc.landmarks_past_2_31()
    w = lm["want"]
    assert w["xyz"].shape == (d + 1, 7384, 3) and w["residual"].shape == (d + 1, oc.BLOCK, k)
    status = w["status"][:d]
    assert all((status == s).any(axis=1).all() for s in (0, 1, 2)), "every block has refitted tracks, first means and tracks of no observation"
    assert w["n_obs"][:d].max(axis=1).tolist() == [4, 4, 4, 3] + [4] * (d - 4) and ((w["n_kept"] < w["n_obs"]) & (w["n_kept"] > 0)).any(), "an observation that is not kept"
    assert w["n_obs"][3].sum() < 0.8 * w["n_obs"][2].sum(), "block 3 has a frame whose C row is not finite: a quarter of its observations are none"
    assert len({w["xyz"][g].tobytes() for g in range(d)}) == d
    for key in ("xyz", "n_kept", "residual", "kept"):
        assert _differ(w[key][d], w[key][d - 1]), key
    assert (lm["lone"]["n_obs"] <= 1).all() and lm["lone"]["xyz"].shape == (k, 3) and (lm["lone"]["status"] >= 1).all()
    # the poses past 2^31 bytes
    p = oc.landmarks_poses_past_2_31()
    assert p["n_bank"] == 22369641 == oc.BLOCK * p["n_blocks"] + 1 and p["n_bank"] * 96 == 2147485536 > FAR and p["K"] == 4 and p["tracks_per_block"] == 10
    dp = _periodic(p, p["n_blocks"], oc.BLOCK * 96)
    assert p["marked"][1] == (FAR // 96) // oc.BLOCK and p["n_bank"] * p["K"] * 88 + p["n_bank"] * 96 < 12 << 30
    assert np.argwhere(p["C"][dp] != p["C"][dp - 1]).tolist() == [[oc.BLOCK - 1, 11]] and all(np.array_equal(p[key][dp], p[key][dp - 1]) for key in ("matches", "kp", "prev"))
    assert _differ(p["want"]["xyz"][dp], p["want"]["xyz"][dp - 1]) and _differ(p["want"]["residual"][dp], p["want"]["residual"][dp - 1])
    assert np.array_equal(p["want"]["n_obs"][dp], p["want"]["n_obs"][dp - 1]) and (p["want"]["status"][:dp] == 0).any(axis=1).all()
    assert len({p["want"]["xyz"][g].tobytes() for g in range(dp)}) == dp
    # kp_bank itself past 2^31 bytes: out of reach under the cap
    kb = oc.KP_BANK_PAST_2_31
    assert kb["n_bank"] * kb["K"] * 8 > FAR >= (kb["n_bank"] - 1) * kb["K"] * 8 and kb["n_bank"] * kb["K"] * kb["bytes_per_node"] > 22 << 30


def test_track_step_past_2_31():
    c = oc.track_step_past_2_31()
    k, cap, t = c["K"], c["capacity"], c["t"]
    assert cap * k == 600002560 <= tt.LIMITS["sslt_track_step"]["largest"]["nodes"] and t == 131072 and t * k * 4 == FAR
    assert c["frames"] == [t - 1, t, t + 1, cap - 1] and c["first"] == [t - 1, -1, t + 1, t + 1]
    outs, st = c["outs"], c["state"]
    assert [int(o["status"][0]) for o in outs] == [0, 0, 0, 4] and (outs[3]["track_id"] == -1).all() and outs[3]["n_new"][0] == 0
    assert st["prev_frame"].tolist()[1:] == [t - 1, -1, t + 1] and st["next_frame"].tolist() == [t, -1, cap - 1, -1]
    inherited = st["prev"][1] >= 0
    assert inherited.sum() > 3500 and np.array_equal(st["track_id"][1][inherited], c["filled"]["track_id"][st["prev"][1][inherited]])
    assert np.array_equal(st["age"][1][inherited], c["filled"]["age"][st["prev"][1][inherited]] + 1)
    assert (st["prev"][2] == -1).all() and (st["age"][2] == 0).all() and outs[1]["n_new"][0] == k
    assert st["next_id"] == 5000 + sum(int(o["n_new"][0]) for o in outs)
    assert _differ(c["state_far"]["prev"][3], st["prev"][3]) and _differ(c["state_far"]["next"][2], st["next"][2])
    assert c["state_far"]["next_id"] == st["next_id"] + 1 and np.array_equal(c["state_far"]["prev"][:3], st["prev"][:3])


def test_the_torch_restatement_of_track_ids_against_the_union_find():
    """track_ids_by_frames of tests/test_gpu_online_limits.py on small banks on the CPU: against track_ref.brute_force, and resumed
    after a change of the last frames."""
    import torch
    from test_gpu_online_limits import track_ids_by_frames
    for name in ("n9_k257", "n33_k70", "scan_past_1025", "bridged_gap", "row_rules", tc.ONE_TRACK):
        c = tc.links(name)
        links = tn.link_pairs(c["first"], c["second"], c["matches"], c["count"], c["mask"], c["n_bank"], c["K"])
        _, track_id, age, lengths = tr.brute_force(c["first"], c["second"], c["matches"], c["count"], c["mask"], c["n_bank"], c["K"])
        prev, pf = torch.from_numpy(links["prev"].copy()), torch.from_numpy(links["prev_frame"].copy())
        got, state = track_ids_by_frames(torch, prev, pf)
        want = tn.track_ids(links["prev"], links["prev_frame"])
        assert np.array_equal(got["track_id"].numpy(), track_id) and np.array_equal(got["age"].numpy(), age), name
        assert np.array_equal(got["length"].numpy()[:len(lengths)], lengths) and int(got["n_tracks"][0]) == len(lengths)
        for key in tn.TRACK_KEYS:
            assert got[key].dtype == torch.int32 and np.array_equal(got[key].numpy(), want[key]), (name, key)
        if c["n_bank"] > 2:
            prev2 = links["prev"].copy()
            prev2[-1] = -1
            got2, _ = track_ids_by_frames(torch, torch.from_numpy(prev2), pf, resume=state + (c["n_bank"] - 2,))
            want2 = tn.track_ids(prev2, links["prev_frame"])
            for key in tn.TRACK_KEYS:
                assert np.array_equal(got2[key].numpy(), want2[key]), (name, key, "resumed")


# =============================================================================================================== libsslam_place.so
def test_bank_at_the_capacity_limit():
    c = oc.bank_at_the_capacity_limit()
    L = pt.LIMITS["sslp_place_step"]["largest"]
    assert (c["capacity"], c["d"], c["per_frame"]) == (L["capacity"], L["d"], L["per_frame"]) == (4096, 256, 8) and c["t0"] == 4094
    own = list(oc.OWN_FRAMES) + [4094]
    assert all((c["slot"] == c["slot"][f]).sum() == 1 for f in own), "descriptors of their own"
    assert len(set(c["slot"][list(oc.PLANTED_FRAMES)].tolist())) == 1 and len(c["desc"]) == 14
    assert 256 % 256 == 512 % 256 and {256, 512} <= set(oc.PLANTED_FRAMES), "two of the equal values fall to one thread of the pick's stride loop"
    st = c["state"]
    assert int(st["t"]) == 4094 and np.array_equal(st["raw"][4000], oc.raw_of(c["desc"][c["slot"][4000]], c["scores"][c["slot"][4000]]))
    total = np.zeros(256, np.float32)
    for i in range(4094):
        total = total + st["raw"][i]
    assert np.array_equal(total, st["sum"]), "the running sum, in its order"
    candidates = sorted(set(oc.OWN_FRAMES[:4]) | set(oc.PLANTED_FRAMES))
    everything, _ = oc.place_steps(c, 0, per_frame=16, n=2)             # the restatement has no per_frame limit: all candidates, by similarity
    for o in everything:
        assert o["count"][0] == 11 and sorted(o["first"][:11].tolist()) == candidates
        ties = o["sim"][np.isin(o["first"], oc.PLANTED_FRAMES)]
        assert len(set(ties.tolist())) == 1 and o["first"][np.isin(o["first"], oc.PLANTED_FRAMES)].tolist() == list(oc.PLANTED_FRAMES), "equal values, lowest frame first"
    assert 4064 == 4094 - c["min_gap"], "the last frame old enough at t = 4094 is a candidate: S[4064], the 128th group's one frame"
    nine, _ = oc.place_steps(c, oc.SUPPRESS["exactly_8"], per_frame=9, n=2)
    for which, counts in (("many_left", [8, 8, 0]), ("exactly_8", [8, 8, 0]), ("fewer_than_8", [4, 4, 0])):
        outs, final = oc.place_expected(which)
        assert [int(o["count"][0]) for o in outs] == counts and [int(o["status"][0]) for o in outs] == [0, 0, 4]
        assert int(final["t"]) == 4096 and not (final["raw"][4094:] == np.float32(-7.5)).any()
        assert (outs[0]["first"][counts[0]:] == -1).all() and (outs[2]["first"] == -1).all()
    assert [int(o["count"][0]) for o in nine] == [8, 8], "suppress 1 leaves exactly eight picks: a ninth finds nothing"
    base, far = oc.place_expected("exactly_8")[0][0], oc.place_expected("exactly_8", True)[0][0]
    at = base["first"].tolist().index(4064)
    assert np.array_equal(base["first"], far["first"]) and base["sim"][at] != far["sim"][at] and np.array_equal(np.delete(base["sim"], at), np.delete(far["sim"], at))


def test_bank_at_the_keypoint_limit():
    c = oc.bank_at_the_keypoint_limit()
    assert c["k"] == pt.LIMITS["sslp_place_step"]["largest"]["k"] == 4096 and c["d"] == 256 and c["desc"].shape == (4, 4096, 256)
    assert (c["k"] - 1) * c["d"] + c["d"] - 1 == 1048575
    assert [int(o["count"][0]) for o in c["outs"]] == [0, 1, 2, 2] and all(o["status"][0] == 0 for o in c["outs"])
    assert _differ(c["state_far"]["raw"][3], c["state"]["raw"][3]) and np.array_equal(c["state_far"]["raw"][:3], c["state"]["raw"][:3])
    assert _differ(c["outs_far"][3]["sig"], c["outs"][3]["sig"]) and _differ(c["outs_far"][3]["sim"], c["outs"][3]["sim"])


def test_edge_log_past_2_31():
    c = oc.edge_log_past_2_31()
    E, cap = c["n_slots"], c["capacity"]
    assert E == pt.LIMITS["sslp_edge_log_step"]["largest"]["n_slots"] == 16 and cap == 800000 and cap * E * 168 == 2150400000 > FAR
    assert cap * E * 96 < FAR, "log_T stays below"
    t = c["t_far"]
    assert t * E * 168 <= FAR < (t + 1) * E * 168 and [s["t"] for s in c["steps"]] == [t, cap - 1, cap]
    for s in c["steps"][:2]:
        logged = s["out"]["logged"]
        assert logged.tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 1] and s["t_after"] == s["t"] + 1
        rows = s["rows"]
        assert (rows["log_second"] == s["t"]).all() and np.array_equal(rows["log_first"] >= 0, logged == 1)
        assert np.array_equal(_bits(rows["log_info"][logged == 1]), _bits(s["ins"]["new_info"][logged == 1])) and not rows["log_info"][logged == 0].any()
    full = c["steps"][2]
    assert full["out"]["status"][0] == 4 and not full["out"]["logged"].any() and full["rows"] is None and full["t_after"] == cap
    far = c["far"]
    diff = np.argwhere(far["rows"]["log_info"] != c["steps"][1]["rows"]["log_info"])
    assert diff.tolist() == [[E - 1, 20]] and np.array_equal(far["rows"]["log_T"], c["steps"][1]["rows"]["log_T"])


# ============================================================================================================== libsslam_window.so
def test_windows_at_the_count_limit():
    c = oc.windows_at_the_count_limit()
    n, cap, steps = c["n"], c["capacity"], c["steps"]
    assert n == wnt.LIMITS["sslw_window_step"]["largest"]["n_windows"] == wnt.MAX_WINDOWS == 65535 and (c["window"], cap, steps) == (2, 400, 6)
    d = _periodic(c, n, cap * 96)                                        # the trajectory
    assert n * cap * 96 == 2516544000 and c["marked"][1] == 55924 and c["workspace_bytes"] == 8 * n * (48 + 23040 + 2) > 12e9
    assert c["workspace_bytes"] + n * cap * 96 < 16 << 30
    assert c["ins"]["T"].shape == (steps, d, 1, 12) and c["state"]["trajectory"].shape == (d, cap, 12)
    traj = c["state"]["trajectory"]
    assert (traj[:, steps:] == 7.25).all() and not (traj[:, :steps] == 7.25).any(), "six rows of every trajectory are written, no other"
    assert len({traj[g, :steps].tobytes() for g in range(d)}) == d
    lost = np.stack([w["lost"] for w in c["want"]])
    assert lost.sum() == 3 and lost[3, 2] == lost[2, 4] == lost[4, 5] == 1, "three frames are lost: status 3, too few inliers, a NaN"
    status = np.stack([w["status"] for w in c["want"]])
    assert (status[0] == 3).all() and (status[1:] == 0).sum() == 5 * d - 4 and sorted(status[1:][status[1:] != 0].tolist()) == [1, 3, 3, 3]
    assert (c["state"]["t"] == steps).all()
    last = c["want"][steps - 1]
    assert _differ(c["out_far"]["C_window"], last["C_window"][d - 1]) and _differ(c["state_far"]["trajectory"], traj[d - 1])
    assert np.array_equal(c["state_far"]["trajectory"][:steps - 1], traj[d - 1][:steps - 1]), "the last frame's pose alone moves"
    assert np.argwhere(c["T_far"] != c["ins"]["T"][steps - 1, d - 1]).tolist() == [[0, 11]]


def test_window_at_a_far_frame():
    c = oc.window_at_a_far_frame()
    cap, t0 = c["capacity"], c["t0"]
    assert cap * 96 == 2147491200 > FAR and t0 == 22369621 and t0 * 96 <= FAR < (t0 + 1) * 96 and c["frames"] == [t0, t0 + 1, cap - 1, cap]
    assert cap <= wnt.LIMITS["sslw_window_step"]["largest"]["capacity"] and cap < wnt.MAX_FRAME
    assert c["start"]["ring_second"].tolist() == [t0 - 1, t0 - 2] and c["start"]["ring_first"].tolist() == [t0 - 2, t0 - 3]
    assert [int(o["base"]) for o in c["outs"]] == [t0 - 1, t0, cap - 2, cap - 1] and [int(o["status"]) for o in c["outs"]] == [0, 0, 0, 0]
    assert [int(o["used_edges"]) for o in c["outs"]] == [1, 1, 1, 1] and all(o["admitted"][0] == 1 for o in c["outs"])
    assert sorted(c["rows"]) == [t0 - 1, t0, t0 + 1, cap - 2, cap - 1] and len({r.tobytes() for r in c["rows"].values()}) == 4 and \
        np.array_equal(c["rows"][cap - 2], c["rows"][t0 + 1]), "the window's fixed first node after the jump is the pose the ring held"
    assert int(c["final"]["t"]) == cap + 1 and c["final"]["ring_second"].tolist() == [cap, cap - 1]
    assert _differ(c["rows_far"][cap - 1], c["rows"][cap - 1]) and np.array_equal(c["rows_far"][cap - 2], c["rows"][cap - 2])
    assert _differ(c["out_far"]["C_window"], c["outs"][2]["C_window"])


# ================================================================================================================ libsslam_conf.so
@pytest.mark.parametrize("name", list(oc.CONF_ROWS))
def test_confidence_rows_past_2_31(name):
    c = oc.confidence_rows(name)
    n = c["n"]
    tiles = -(-n // ct.TILE_ROWS)
    assert c["D"] == ct.LIMITS["sslc_confidence_rows"]["largest"]["D"] == 256
    if name == "confidence_rows_past_2_31":
        d = _periodic(c, n, 384 * 4)
        assert n * 384 * 4 == 2227204608 and n * 256 * 4 < FAR
        assert (n % ct.TILE_ROWS, tiles, tiles % 8) == (19, 45313, 1), "a ragged last tile, a remainder of the XCD split"
    else:
        d = _periodic(c, n, 384 * 4, extra=(FAR // 1024,))
        assert n * 256 * 4 == 2150403072 > FAR and c["marked"] == [0, 1398101, 2097152, n - 1]
        assert (n % ct.TILE_ROWS, tiles, tiles % 8) == (3, 65626, 2)
    assert c["want"].shape == (d,) and c["want"].dtype == np.float32 and len(set(c["want"].tolist())) == d and (c["want"] > 0).all() and (c["want"] < 1).all()
    assert c["want_far"] != c["want"][-1] and np.argwhere(c["x_far"] != c["x"][-1]).tolist() == [[383]]


def test_gather_confidence_past_2_31():
    c = oc.gather_confidence_past_2_31()
    n, g, k = c["n"], c["G"], c["K"]
    fb = g * g * 384 * 4
    d = _periodic(c, n, fb, extra=(4 * FAR // fb,))
    assert (g, n, k) == (40, 3500, 5) and n * g * g * 384 == 2150400000 > FAR, "the float index, not only the byte offset, passes 2^31"
    assert c["marked"] == [0, 873, 3495, 3499] and d == 11
    assert n * k <= ct.LIMITS["sslc_gather_confidence"]["largest"]["rows"] and -(-n * k // ct.TILE_ROWS) % 8
    assert c["want"].shape == (d, k) and len(set(c["want"].reshape(-1).tolist())) == d * k
    assert (c["kp"][:, k - 1] == g - 1).all() and np.argwhere(c["feat_far"] != c["feat"][-1]).tolist() == [[g - 1, g - 1, 383]]
    assert c["want_far"][k - 1] != c["want"][-1, k - 1] and np.array_equal(c["want_far"][:k - 1], c["want"][-1, :k - 1])


def test_confidence_filter_past_2_31():
    c = oc.confidence_filter_past_2_31()
    n, k = c["n"], c["K"]
    _periodic(c, n, k * 4)
    assert k == ct.LIMITS["sslc_confidence_filter"]["largest"]["K"] == 4096 and n * k * 4 == 2147614720 and c["marked"][1] == 131072
    w = c["want"]
    assert w["count"][1] == 1 and w["slot"][1, 0] == 77 and (w["slot"][1] == 77).all() and w["confidence"][1, 0] == np.float32(0.4925) and not w["confidence"][1, 1:].any()
    assert w["count"][2] == k and w["count"][5] == 1 and w["slot"][5, 0] == 0 and 0 < w["count"][3] < k
    assert (w["confidence"][4, :w["count"][4]] == np.float32(0.5)).sum() >= k // 3, "values equal to the threshold pass"
    assert c["want_far"]["count"] == w["count"][-1] + 1 and c["want_far"]["slot"][c["want_far"]["count"] - 1] == k - 1
    assert _differ(c["want_far"]["slot"], w["slot"][-1]) and _differ(c["want_far"]["confidence"], w["confidence"][-1])


@pytest.mark.parametrize("name", list(oc.TAKE_SHAPES))
def test_take_rows(name):
    c = oc.take_rows(name)
    n, k, w = c["n"], c["K"], c["width"]
    d = _periodic(c, n, k * w * 4)
    words = ct.LIMITS["sslc_take_rows"]["largest"]["words"]
    if name == "take_rows_past_2_31":
        assert (k, w) == (16, 256) and n * k * w * 4 == 2147614720
    else:
        assert n * k == words // w and n * k * w == 2147483392 <= words < (n + 1) * k * w and 2 * n * k * w * 4 + n * k * 4 < 17 << 30
    assert {-1, k, 2 ** 31 - 1, -2 ** 31} <= set(c["slot"][:, 3].tolist()) and (c["slot"][:, 5] == c["slot"][:, 6]).all()
    bad = (c["slot"] < 0) | (c["slot"] >= k)
    assert bad.sum() >= 6 and not c["want"][bad].any() and c["want"][~bad].any(axis=-1).all()
    assert np.array_equal(c["want"][:, 5], c["want"][:, 6]) and c["want"].shape == (d, k, w) and c["want"].dtype == np.int32
    assert _differ(c["want_far"][k - 1], c["want"][-1, k - 1]) and np.array_equal(c["want_far"][:k - 1], c["want"][-1, :k - 1])


# ============================================================================================================== libsslam_weight.so
def test_match_weights_past_2_31():
    c = oc.match_weights_past_2_31()
    n, k = c["n"], c["K"]
    d = _periodic(c, n, k * 16)
    assert (n, k, c["n1"]) == (32776, 4096, 4096) and n * k * 16 == 2148007936 and c["marked"][1] == 32768
    assert n * k <= wt.LIMITS["sslu_match_weights"]["largest"]["slots"] < 16 * n * k
    assert c["n_bank"] == c["periods"] * oc.BANK_PERIOD == 131080 and c["n_bank"] * k * 4 > FAR and c["conf"].shape == (oc.BANK_PERIOD, k)
    a, b = oc.pair_frames(n, c["marked"], c["periods"])
    s = oc.slots(n, c["marked"])
    assert (a % oc.BANK_PERIOD == 2 * s).all() and (b == a + 1).all() and a.max() == c["n_bank"] - 2 * d + 2 * s[a.argmax()] and b.max() < c["n_bank"]
    assert (b[c["marked"][1]:] * k * 4 > FAR).any() and (a // oc.BANK_PERIOD == c["periods"] - 1).any(), "pairs read past byte 2^31 of the bank, and its last period"
    for mode in (wt.WEIGHT_PRODUCT, wt.WEIGHT_EXPECTED_ERROR):
        w = c["want"][mode]
        assert w.shape == (d, k) and w.dtype == np.float32 and not w[c["absent"]].any() and not w[2].any() and not w[3, 1000:].any() and w[3, :1000].any()
        assert len({w[g].tobytes() for g in range(d)}) == d - 2 and np.isfinite(w).all() and (w >= 0).all()
        assert c["want_far"][mode][k - 1] != w[-1, k - 1] and np.array_equal(c["want_far"][mode][:k - 1], w[-1, :k - 1])
    assert _differ(c["want"][0], c["want"][1])


def test_weighted_refine_past_2_31():
    c = oc.weighted_refine_past_2_31()
    n, k = c["n"], c["K"]
    d = _periodic(c, n, k * 16)
    L = wt.LIMITS["sslu_pose_refine_weighted_pairs"]["largest"]
    assert (k, c["n1"]) == (L["K"], L["n1"]) == (4096, 4096) and c["n_iter"] == 1
    assert c["n_bank"] == 65540 and c["n_bank"] * k * 8 > FAR and c["bank"].shape == (oc.BANK_PERIOD, k, 2)
    w = c["want"]
    assert set(w) == set(("T", "status", "iterations", "selected_count", "usable_count", "inlier_count_in", "inlier_count", "inlier_of_slot", "cost_in",
                          "cost", "rms", "info", "weight_sum"))
    assert (w["iterations"] == 1).all() and (w["status"] == 0).any() and (w["selected_count"] > 2500).all() and (w["selected_count"] < w["usable_count"]).all()
    assert (w["usable_count"] > wt.CHUNK).all(), "rows past the LDS chunk: weights read from global memory"
    assert len({w["info"][g].tobytes() for g in range(d)}) == d and w["status"][-1] == 0 and (w["cost"][w["status"] == 0] < w["cost_in"][w["status"] == 0]).all()
    for key in ("cost_in", "cost", "info", "T"):
        assert _differ(c["want_far"][key], w[key][-1]), key
    assert np.argwhere(c["matches_far"] != c["matches"][-1]).tolist() == [[int(c["count"][-1]) - 1, 1]]


# ==================================================================================================== one past every limit
PTRS = [0x10000 * (i + 1) for i in range(32)]      # aligned to 64 KB and never followed: every call below is refused before the launch
# entry -> (library, its arguments in order: "p" a pointer, or (name, default, ctype))
_I, _D, _F, _LL = C.c_int, C.c_double, C.c_float, C.c_longlong
SIGNATURES = {
    "sslw_window_step": ("window", ["p"] * 13 + [("n_windows", 1, _I), ("window", 4, _I), ("n_spacings", 3, _I), ("min_inliers", 12, _I), ("chi", 4.0, _D),
                                                 ("damping", 0.0, _D), ("n_iter", 2, _I), ("capacity", 100, _LL)] + ["p"] * 15),
    "sslp_place_step": ("place", ["p"] * 5 + [("capacity", 100, _I), ("k", 5, _I), ("d", 128, _I), ("min_gap", 30, _I), ("min_sim", 0.3, _F),
                                              ("per_frame", 2, _I), ("suppress", 5, _I)] + ["p"] * 7),
    "sslp_edge_log_step": ("place", ["p"] * 10 + [("n_slots", 4, _I), ("n_odometry", 2, _I), ("min_inliers", 12, _I), ("loop_min_inliers", 12, _I),
                                                  ("capacity", 100, _LL)] + ["p"] * 2),
    "sslc_confidence_rows": ("conf", ["p", "p", ("rows", 64, _LL), ("D", 128, _I), "p", "p"]),
    "sslc_gather_confidence": ("conf", ["p", ("n_frames", 2, _I), ("G", 4, _I), "p", ("K", 8, _I), "p", ("D", 128, _I), "p", "p"]),
    "sslc_confidence_filter": ("conf", ["p", ("n_frames", 2, _I), ("K", 8, _I), ("threshold", 0.5, _F), "p", "p", "p"]),
    "sslc_take_rows": ("conf", ["p", "p", ("n_frames", 2, _I), ("K", 8, _I), ("width", 4, _I), "p"]),
    "sslu_match_weights": ("weight", ["p", ("n_bank", 3, _I), ("K", 8, _I), "p", "p", ("n_pairs", 2, _I), "p", "p", ("n1", 8, _I), ("mode", 0, _I),
                                      ("sigma0", 1.0, _D), "p"]),
    "sslu_pose_refine_weighted_pairs": ("weight", ["p", "p", ("n_bank", 3, _I), ("K", 8, _I), "p", "p", ("n_pairs", 2, _I), "p", "p", ("n1", 8, _I)] +
                                        [(v, x, _D) for v, x in (("fx", 525.0), ("fy", 525.0), ("cx", 319.5), ("cy", 239.5), ("depth_scale", 5000.0),
                                                                 ("scale_x", 1.0), ("scale_y", 1.0), ("view_w", 640.0), ("view_h", 480.0), ("threshold", 3.0))] +
                                        ["p", ("huber", 1.0, _D), ("n_iter", 5, _I), "p"] + ["p"] * 13),
    "sslt_link_pairs": ("track", ["p", "p", ("n_pairs", 3, _I), "p", "p", "p", ("n1", 8, _I), ("n_bank", 5, _I), ("K", 8, _I), "p", "p", "p", "p"]),
    "sslt_track_ids": ("track", ["p", "p", ("n_bank", 5, _I), ("K", 8, _I)] + ["p"] * 7),
    "sslt_landmarks": ("track", ["p", "p", "p", ("n_bank", 5, _I), ("K", 8, _I)] +
                       [(v, x, _D) for v, x in (("fx", 525.0), ("fy", 525.0), ("cx", 319.5), ("cy", 239.5), ("depth_scale", 5000.0), ("scale_x", 1.0),
                                                ("scale_y", 1.0), ("view_w", 640.0), ("view_h", 480.0), ("threshold", 3.0))] +
                       ["p"] * 6 + [("min_obs", 2, _I)] + ["p"] * 8),
    "sslt_track_step": ("track", ["p"] * 12 + [("n1", 8, _I), ("K", 8, _I), ("capacity", 5, _I)] + ["p"] * 4),
}


def _entry(entry, **over):
    """One C entry with never-followed pointers and valid scalars, `over` replacing sizes by name -> its return code; nothing launched.
    Only for calls that the entry refuses: an accepted one would launch on these pointers."""
    from sslam_amd import lib
    which, spec = SIGNATURES[entry]
    L, count = getattr(lib, which)(), getattr(lib, f"{which}_launch_count")
    ptr = iter(PTRS)
    over_given = bool(over)
    args = [C.c_void_p(next(ptr)) if a == "p" else a[2](over.pop(a[0], a[1])) for a in spec]
    assert not over, over
    before = count()
    assert over_given, "a call with every size valid is not made here"
    rc = getattr(L, entry)(*args, None)
    assert count() == before, f"{entry}: a refusal launched something"
    return rc


def _wrapper_refuses(call, kind="unsupported"):
    from sslam_amd import lib
    if kind == "invalid":
        with pytest.raises(ValueError):
            call()
    else:
        with pytest.raises(lib.SslamHipError):
            call()


def test_every_signature_is_accepted_as_it_stands():
    """The argument lists of SIGNATURES are the entries': as long as the prototypes, and with a NULL for every pointer each entry
    answers SSLAM_E_INVALID - it judges its pointers first - where the same sizes one past a limit answer SSLAM_E_UNSUPPORTED below."""
    from sslam_amd import lib
    for entry, (which, spec) in SIGNATURES.items():
        L = getattr(lib, which)()
        assert len(getattr(L, entry).argtypes) == len(spec) + 1, entry
        args = [C.c_void_p(0) if a == "p" else a[2](a[1]) for a in spec]
        assert getattr(L, entry)(*args, None) == E_INVALID, entry


def test_one_past_each_limit_is_refused_by_the_entry_and_by_the_wrapper():
    import torch
    from sslam_amd import lib
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)      # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)      # noqa: E731
    # ---- window
    L = wnt.LIMITS["sslw_window_step"]["largest"]
    for over, sizes in ((dict(window=33), (33, 1, 100, 1)), (dict(n_spacings=9), (4, 9, 100, 1)), (dict(n_windows=65536), (4, 3, 100, 65536)),
                        (dict(capacity=L["capacity"] + 1), (4, 3, L["capacity"] + 1, 1)), (dict(capacity=L["capacity"] // 65535 + 1, n_windows=65535),
                                                                                          (4, 3, L["capacity"] // 65535 + 1, 65535))):
        assert _entry("sslw_window_step", **over) == E_UNSUPPORTED, over
        _wrapper_refuses(lambda: lib.check_window_sizes(*sizes))
    assert lib.check_window_sizes(32, 8, L["capacity"], 1) == (32, 8, L["capacity"], 1) and lib.check_window_sizes(2, 1, 400, 65535)[3] == 65535
    # ---- place
    L = pt.LIMITS["sslp_place_step"]["largest"]
    for over, call in ((dict(capacity=L["capacity"] + 1), lambda: lib.check_place_sizes(L["capacity"] + 1, 5, 128)),
                       (dict(k=L["k"] + 1), lambda: lib.check_place_sizes(100, L["k"] + 1, 128)),
                       (dict(per_frame=L["per_frame"] + 1), lambda: lib.alloc_place_out(L["per_frame"] + 1, 128, device="cpu"))):
        assert _entry("sslp_place_step", **over) == E_UNSUPPORTED, over
        _wrapper_refuses(call, "invalid" if "per_frame" in over else "unsupported")
    assert _entry("sslp_place_step", d=192) == E_UNSUPPORTED
    _wrapper_refuses(lambda: lib.check_place_sizes(100, 5, 192), "invalid")
    assert lib.check_place_sizes(L["capacity"], L["k"], L["d"]) == (4096, 4096, 256)
    L = pt.LIMITS["sslp_edge_log_step"]["largest"]
    for over, sizes in ((dict(n_slots=17, n_odometry=2), (100, 17)), (dict(capacity=L["capacity"] + 1, n_slots=1, n_odometry=1), (L["capacity"] + 1, 1)),
                        (dict(capacity=L["capacity"] // 16 + 1, n_slots=16), (L["capacity"] // 16 + 1, 16))):
        assert _entry("sslp_edge_log_step", **over) == E_UNSUPPORTED, over
        _wrapper_refuses(lambda: lib.check_edge_log_sizes(*sizes))
    assert lib.check_edge_log_sizes(L["capacity"], 1) == (L["capacity"], 1) and lib.check_edge_log_sizes(oc.LOG_CAPACITY, 16) == (800000, 16)
    # ---- conf: confidence_rows, gather_confidence and take_rows hand their sizes to the entry as they are: its verdict is the wrapper's
    assert _entry("sslc_confidence_rows", rows=1 << 31) == E_UNSUPPORTED and _entry("sslc_confidence_rows", D=192) == E_UNSUPPORTED
    assert _entry("sslc_gather_confidence", n_frames=1 << 28, K=8) == E_UNSUPPORTED and _entry("sslc_gather_confidence", D=64) == E_UNSUPPORTED
    assert _entry("sslc_take_rows", n_frames=1 << 19, K=16, width=256) == E_UNSUPPORTED and _entry("sslc_take_rows", n_frames=1 << 30, K=1 << 30) == E_UNSUPPORTED
    assert _entry("sslc_confidence_filter", K=ct.FILTER_MAX_K + 1) == E_UNSUPPORTED
    _wrapper_refuses(lambda: lib.confidence_filter(f32(2, ct.FILTER_MAX_K + 1)))
    with pytest.raises(ValueError, match="CUDA"):                    # accepted as far as a host without a device can tell
        lib.confidence_filter(f32(2, ct.FILTER_MAX_K))
    # ---- weight
    assert _entry("sslu_match_weights", n_pairs=1 << 19, n1=4096) == E_UNSUPPORTED and _entry("sslu_match_weights", n_pairs=1 << 30, n1=2) == E_UNSUPPORTED
    assert _entry("sslu_pose_refine_weighted_pairs", K=wt.MAX_K + 1) == E_UNSUPPORTED
    assert _entry("sslu_pose_refine_weighted_pairs", K=8, n1=9) == E_INVALID
    kp = torch.zeros((2, wt.MAX_K + 1, 2))
    m, cnt, T_in = torch.zeros((1, 8, 2), dtype=torch.int64), i32(1), torch.zeros((1, 12), dtype=torch.float64)
    _wrapper_refuses(lambda: lib.pose_refine_weighted(kp, i32(2, wt.MAX_K + 1), i32(1), i32(1), m, cnt, tc.CAMERA, T_in, f32(1, 8)))
    _wrapper_refuses(lambda: lib.pose_refine_weighted(torch.zeros((2, 8, 2)), i32(2, 8), i32(1), i32(1), torch.zeros((1, 9, 2), dtype=torch.int64), cnt,
                                                      tc.CAMERA, T_in, f32(1, 9)), "invalid")
    # ---- track
    for entry, bank in (("sslt_link_pairs", "n_bank"), ("sslt_track_ids", "n_bank"), ("sslt_landmarks", "n_bank"), ("sslt_track_step", "capacity")):
        assert _entry(entry, **{bank: 1 << 19, "K": 4096}) == E_UNSUPPORTED, entry
        limit_k = entry in ("sslt_link_pairs", "sslt_track_step")
        _wrapper_refuses(lambda: lib.check_track_sizes(entry, 1 << 19, 4096, limit_k=limit_k))
        assert lib.check_track_sizes(entry, (1 << 19) - 1, 4096, limit_k=limit_k) == ((1 << 19) - 1, 4096)
        if limit_k:
            assert _entry(entry, K=tt.MAX_K + 1) == E_UNSUPPORTED, entry
            _wrapper_refuses(lambda: lib.check_track_sizes(entry, 3, tt.MAX_K + 1, limit_k=True))
    assert lib.check_track_sizes("track_ids", 3, tt.MAX_K + 1) == (3, tt.MAX_K + 1), "sslt_track_ids and sslt_landmarks keep no row in LDS"
