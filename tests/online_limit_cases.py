"""The cases of tests/test_gpu_online_limits.py: libsslam_window.so, libsslam_place.so, libsslam_conf.so, libsslam_weight.so and
libsslam_track.so at the limits their headers state (tests/window_table.py, place_table.py, conf_table.py, weight_table.py,
track_table.py: every size below is read from the tables' `largest`), at the smallest sizes that reach a path the older cases
never take, and with operands past 2^31 bytes.  Each case carries the expectation of the existing restatements (window_ref,
place_ref, confidence_ref, weighted_refine_ref, track_ref / sslam_amd.track_numpy) and, for the far end, one changed input element
with the restatement's new result.  tests/test_online_limit_cases_cpu.py holds every case to what its name says.

An operand past 2^31 bytes is periodic as in tests/periodic.py - 7 repeating items and items of their own at 0, at the holder of
byte 2^31 and at the end: only the P + len(marked) distinct items exist here, the device test expands them.  marks() and slots()
restate periodic.marks and periodic.slots without torch (the CPU test holds them equal).

Builders are cached per process.  Case generation uses random numbers freely: nothing here is what the device computes.
No torch, no GPU: importable anywhere."""
from __future__ import annotations

import functools

import numpy as np

import conf_table as ct
import confidence_cases as cc
import confidence_ref as cr
import place_ref as pr
import place_table as pt
import pose_ransac_cases as rc
import pose_refine_cases as pc
import track_cases as tc
import track_table as tt
import weight_table as wt
import weighted_refine_ref as wr
import window_cases as wc
import window_ref as wf
import window_table as wnt
from sslam_amd import track_numpy as tn

P = 7
FAR = 1 << 31


def marks(n, frame_bytes, far_byte=FAR):
    m = {0, n - 1}
    if far_byte < n * frame_bytes:
        m.add(far_byte // frame_bytes)
    return sorted(m)


def slots(n, marked):
    s = np.arange(n, dtype=np.int64) % P
    s[np.asarray(marked, np.int64)] = P + np.arange(len(marked))
    return s


# =============================================================================================================== libsslam_track.so
MAX_K = tt.LIMITS["sslt_link_pairs"]["largest"]["K"]
IDS_K, IDS_N1, IDS_LONG = 128, 40, 4
IDS_BANKS = {"ids_tiles_256": 2048, "ids_tiles_257": 2049, "ids_tiles_513": 4104}
CHUNK_TILES = 256                         # the tiles ids_scan_tiles_kernel scans at a time: one per thread


def _dirty(rng, m, mask, p, k, lo=0, kind=None):
    """track_cases.links' dirt on row p, in slots lo ..: an idx1 named twice, an idx2 named twice, an index -1, K or 2^40, a mask 0 or -1."""
    kind = p if kind is None else kind
    j = lo + rng.permutation(m.shape[1] - lo)
    m[p, j[0], 0] = m[p, j[1], 0]
    m[p, j[2], 1] = m[p, j[3], 1]
    m[p, j[4], rng.integers(0, 2)] = (-1, k, 2 ** 40)[kind % 3]
    mask[p, j[5]] = (0, -1)[kind % 2]


@functools.lru_cache(maxsize=None)
def ids_tiles(name: str) -> dict:
    """A bank of n_bank frames of 128 slots whose numbering scan has 256, 257 or 513 tiles: 1, 2 or 3 chunks of
    ids_scan_tiles_kernel.  Rows (i, i + 1) of 40 slots, so every frame - every tile of 8 frames - holds at least 88 roots; slots
    0 .. 3 of every frame are one chain each (rotating), broken where a frame has no row (every 300th, and not at a chunk's first
    frame): chains cross every chunk boundary.  One bridged row (i - 1, i + 1), rows with counts -2 and n1 + 7, the dirt of
    track_cases.links.  far: prev with its last element - the last node's predecessor - changed."""
    n_bank, k, n1 = IDS_BANKS[name], IDS_K, IDS_N1
    rng = np.random.default_rng(300 + n_bank)
    gaps = set(range(150, n_bank, 300)) - {2048, 4096}
    bridge = 1001
    rows = [(i - 1, i) for i in range(1, n_bank) if i not in gaps and i not in (bridge, bridge + 1)] + [(bridge - 1, bridge + 1)]
    rows += [(5, 9), (7, 8)]                                   # named again, later: not the lowest rows of their frames, no link rows
    n_rows = len(rows)
    m = np.zeros((n_rows, n1, 2), np.int64)
    for p in range(n_rows):
        m[p, :IDS_LONG, 0], m[p, :IDS_LONG, 1] = np.arange(IDS_LONG), (np.arange(IDS_LONG) + 1) % IDS_LONG
        m[p, IDS_LONG:, 0] = IDS_LONG + rng.permutation(k - IDS_LONG)[:n1 - IDS_LONG]
        m[p, IDS_LONG:, 1] = IDS_LONG + rng.permutation(k - IDS_LONG)[:n1 - IDS_LONG]
    count = np.full(n_rows, n1, np.int32)
    mask = np.ones((n_rows, n1), np.int32)
    for p in range(n_rows):
        _dirty(rng, m, mask, p, k, IDS_LONG)
    count[40::97], count[77::97] = n1 + 7, -2
    first, second = np.array([a for a, _ in rows], np.int32), np.array([b for _, b in rows], np.int32)
    last = int(np.flatnonzero(second == n_bank - 1)[0])
    m[last, n1 - 1], mask[last, n1 - 1], count[last] = (k - 2, k - 1), 1, n1     # the last node has a predecessor, by the last slot
    m[last, :n1 - 1][m[last, :n1 - 1] >= k - 2] = k - 3
    links = tn.link_pairs(first, second, m, count, mask, n_bank, k)
    assert links["prev"][n_bank - 1, k - 1] == k - 2
    prev_far = links["prev"].copy()
    prev_far[n_bank - 1, k - 1] = -1                           # the last node becomes a root: the last id, one track more
    return dict(name=name, n_bank=n_bank, K=k, n1=n1, first=first, second=second, matches=m, count=count, mask=mask, gaps=sorted(gaps),
                links=links, want=tn.track_ids(links["prev"], links["prev_frame"]), prev_far=prev_far, want_far=tn.track_ids(prev_far, links["prev_frame"]))


@functools.lru_cache(maxsize=None)
def links_k_4096() -> dict:
    """K = n1 = 4096, three frames, rows (0, 1) and (1, 2): lo1, lo2 of link_slots_kernel filled to their ends, 16 strides of 256
    slots; the dirt of track_cases.links, a mask.  The last slot of the last row is a link; far: its idx2 is -1."""
    k, n_bank = MAX_K, 3
    rng = np.random.default_rng(311)
    m = np.stack([np.stack([rng.permutation(k), rng.permutation(k)], axis=1) for _ in range(2)]).astype(np.int64)
    mask = np.ones((2, k), np.int32)
    for p in range(2):
        for kind in range(40):
            _dirty(rng, m, mask, p, k, kind=kind)
    mask[:, 1000:1100:3] = 0
    count = np.array([k - 3, k], np.int32)
    i1, i2 = 17, 4095                                          # the last slot of all: a link of its own
    for col, v in ((0, i1), (1, i2)):
        m[1, :k - 1, col][m[1, :k - 1, col] == v] = -1
    m[1, k - 1], mask[1, k - 1] = (i1, i2), 1
    first, second = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    far = m.copy()
    far[1, k - 1, 1] = -1
    links = tn.link_pairs(first, second, m, count, mask, n_bank, k)
    links_far = tn.link_pairs(first, second, far, count, mask, n_bank, k)
    return dict(name="links_k_4096", n_bank=n_bank, K=k, n1=k, first=first, second=second, matches=m, count=count, mask=mask,
                far_link=(i1, i2), links=links, want=tn.track_ids(links["prev"], links["prev_frame"]), matches_far=far,
                links_far=links_far, want_far=tn.track_ids(links_far["prev"], links_far["prev_frame"]))


def bank_steps(c, matches=None):
    """The three online steps of links_k_4096's rows through track_numpy.TrackBank: (the steps' outputs, the final state)."""
    matches = c["matches"] if matches is None else matches
    bank = tn.TrackBank(c["n_bank"], c["K"])
    outs = [bank.step(matches[0], 0, None, -1)]
    outs += [bank.step(matches[r], c["count"][r], c["mask"][r], int(c["first"][r])) for r in range(2)]
    return outs, bank.state


@functools.lru_cache(maxsize=None)
def step_k_4096() -> dict:
    """links_k_4096's rows stepped online at K = n1 = 4096 on a bank of capacity 3: lo1, lo2, pv of track_step_kernel filled to
    their ends, the id scan carrying across 16 chunks.  The state equals the batch entries' outputs."""
    c = links_k_4096()
    outs, state = bank_steps(c)
    outs_far, state_far = bank_steps(c, c["matches_far"])
    return dict(c, name="step_k_4096", outs=outs, state=state, outs_far=outs_far, state_far=state_far)


# ---- the bank of 134 M nodes: sslt_link_pairs, sslt_track_ids, sslt_landmarks past 2^31 bytes
BLOCK = 4                                 # frames of a block: the links stay inside it
BIG_PAIRS = 32776                         # rows (i, i + 1): matches is 32776 * 4096 * 16 bytes = 2.148 GB
BIG_LINKS = 3000                          # links of every row that has any: every block holds 4 K - 3 * 3000 tracks
BIG_DEPTHS = 300                          # keypoints of a frame with a depth: the observations the host restates


@functools.lru_cache(maxsize=None)
def big_bank() -> dict:
    """The distinct blocks of the 134 M-node bank: 32 776 rows (i, i + 1) at K = n1 = 4096 over 32 777 frames.  A block is four frames
    and the four rows that start in it: three rows of 3000 links each between its frames - true correspondences of a planted scene of
    4096 points, row r linking the points 300 r .. 300 r + 2999 - and a fourth row, into the next block, of no link (its count is
    0 or its slots are all dirt).  Every block so holds 4 * 4096 - 9000 = 7384 tracks of lengths 1 .. 4, and is independent of its
    neighbours.  8194 blocks, periodic with blocks of their own at 0, 8192 (the holder of byte 2^31 of `matches`) and 8193; the last
    frame, 32 776, stands alone.  300 keypoints of a frame have a depth; one weight in 50 is 0, NaN, inf, negative or subnormal.
    Row d of every operand is the last block with the idx2 of its last link - row 2's slot 2999, of a point with a depth - changed to
    a slot no link names, of another point with a depth: one node of the block's last frame loses its predecessor, another gains it,
    the number of tracks stays, and a track observes a point that is not its own."""
    k, n1 = MAX_K, MAX_K
    n_blocks = BIG_PAIRS // BLOCK
    assert n_blocks * BLOCK == BIG_PAIRS
    item_bytes = BLOCK * n1 * 16
    marked = marks(n_blocks, item_bytes)
    d = P + len(marked)
    cam = tc.CAMERA
    ops = {key: [] for key in ("matches", "count", "mask", "kp", "depth", "C", "weight")}
    for g in range(d + 2):                                     # d: the changed last block; d + 1: the lone last frame (one frame used)
        gg = min(g, d - 1)                                     # block d is block d - 1 again, but for its one changed element
        rng = np.random.default_rng(400 + gg if g != d + 1 else 499)
        Pw = np.stack([rng.uniform(-1.0, 1.0, k), rng.uniform(-0.7, 0.7, k), rng.uniform(1.5, 4.0, k)], axis=1)
        C = tc.poses(400 + gg, BLOCK)
        perm = np.stack([rng.permutation(k) for _ in range(BLOCK)])
        kp, depth = np.zeros((BLOCK, k, 2), np.float32), np.zeros((BLOCK, k), np.int32)
        seen = np.zeros(k, bool)
        seen[rng.permutation(600)[:BIG_DEPTHS // 2]] = True    # among the points of the shorter tracks ..
        seen[600 + rng.permutation(2400)[:BIG_DEPTHS // 2]] = True           # .. and of the tracks through all four frames
        for f in range(BLOCK):
            px, z = tc.project(C[f], Pw, cam)
            kp[f, perm[f]] = (px + rng.normal(size=px.shape) * 0.3).astype(np.float32)
            depth[f, perm[f]] = np.where(seen, np.rint(z * cam.depth_scale), 0).astype(np.int32)
        kp[2, perm[2, 600 + int(np.flatnonzero(seen[600:3000])[0])]] += np.float32(15.0)      # one observation of a whole track far off: not kept
        m = np.zeros((BLOCK, n1, 2), np.int64)
        mask = np.ones((BLOCK, n1), np.int32)
        count = np.zeros(BLOCK, np.int32)
        for r in range(BLOCK - 1):
            pts = 300 * r + rng.permutation(BIG_LINKS)
            j = int(np.flatnonzero(seen[pts])[-1])             # the last link of the row is one of a point with a depth
            pts[[j, BIG_LINKS - 1]] = pts[[BIG_LINKS - 1, j]]
            m[r, :BIG_LINKS, 0], m[r, :BIG_LINKS, 1] = perm[r, pts], perm[r + 1, pts]
            free = np.setdiff1d(np.arange(k), pts)
            free2 = perm[r + 1, free]
            if r == BLOCK - 2:
                far2 = perm[r + 1, free[seen[free]][0]]        # a slot of the next frame no link names, of a point with a depth
            m[r, BIG_LINKS:, 0] = m[r, rng.integers(0, BIG_LINKS, n1 - BIG_LINKS), 0]      # an idx1 named again, lower slots win
            m[r, BIG_LINKS:, 1] = free2[rng.integers(0, len(free2), n1 - BIG_LINKS)]
            m[r, BIG_LINKS + 5::7, rng.integers(0, 2)] = (-1, k, 2 ** 40)[r]
            mask[r, BIG_LINKS + 3::11] = (0, -1)[r % 2]
            count[r] = (n1, n1 + 9, BIG_LINKS + 500)[(gg + r) % 3]
        m[BLOCK - 1] = rng.integers(0, k, (n1, 2))             # the row into the next block: real indices, none a link
        if gg % 2:
            count[BLOCK - 1] = -3
        else:
            count[BLOCK - 1], mask[BLOCK - 1] = n1, 0
        weight = rng.uniform(2.0 ** -6, 1.0, (BLOCK, k)).astype(np.float32)
        bad = rng.permutation(BLOCK * k)[:BLOCK * k // 50]
        weight.reshape(-1)[bad] = np.array([0.0, np.nan, np.inf, -1.0, 1e-41], np.float32)[np.arange(len(bad)) % 5]
        if gg == 3:
            C[1, 7] = np.inf                                   # a frame whose C row is not finite: none of its members observes
        if g == d:
            m[2, BIG_LINKS - 1, 1] = far2
        for key, v in zip(ops, (m, count, mask, kp, depth, C, weight)):
            ops[key].append(v)
    ops = {key: np.stack(v) for key, v in ops.items()}
    return dict(ops, name="big_bank", K=k, n1=n1, n_blocks=n_blocks, n_pairs=BIG_PAIRS, n_bank=BIG_PAIRS + 1, item_bytes=item_bytes,
                marked=marked, tracks_per_block=BLOCK * k - (BLOCK - 1) * BIG_LINKS)


def block_links(c, g) -> dict:
    """link_pairs of distinct block g alone, as a bank of five frames: its four and the next block's first (which takes no link)."""
    first, second = np.arange(BLOCK, dtype=np.int32), np.arange(1, BLOCK + 1, dtype=np.int32)
    return tn.link_pairs(first, second, c["matches"][g], c["count"][g], c["mask"][g], BLOCK + 1, c["K"])


def _with_links(c, name, links_per_row):
    """The bank with prev and next of every distinct block's four frames (d + 1, 4, K)."""
    d = P + len(c["marked"])
    got = [block_links(c, g) for g in range(d + 1)]
    for x in got:
        assert (x["prev"][BLOCK] == -1).all() and (x["prev"][0] == -1).all() and (x["next"][BLOCK - 1] == -1).all(), "no link leaves a block"
        assert ((x["prev"][:BLOCK] >= 0).sum(), (x["next"][:BLOCK] >= 0).sum()) == ((BLOCK - 1) * links_per_row,) * 2
    return dict(c, name=name, prev=np.stack([x["prev"][:BLOCK] for x in got]), next=np.stack([x["next"][:BLOCK] for x in got]))


@functools.lru_cache(maxsize=None)
def link_pairs_past_2_31() -> dict:
    """sslt_link_pairs on the big bank: per distinct block prev and next of its four frames (4, K), prev_frame and next_frame being
    f - 1 and f + 1 throughout."""
    return _with_links(big_bank(), "link_pairs_past_2_31", BIG_LINKS)


def block_tracks(c, g, lone=False) -> tuple:
    """(links, tracks) of distinct block g alone (lone: of the bank's last frame alone, which block d + 1's first frame is)."""
    if lone:
        links = dict(prev=np.full((1, c["K"]), -1, np.int32), next=np.full((1, c["K"]), -1, np.int32), prev_frame=np.full(1, -1, np.int32),
                     next_frame=np.full(1, -1, np.int32))
    else:
        links = {key: v[:BLOCK].copy() for key, v in block_links(c, g).items()}
        links["next_frame"][BLOCK - 1] = -1                    # inside the bank it names the next block's first frame: no slot follows it
    return links, tn.track_ids(links["prev"], links["prev_frame"])


def _landmark_case(c, name):
    """Per distinct block the rows of its tracks (xyz, n_obs, n_kept, status, weight_sum, rms) and its four frames of residual and
    kept, from track_numpy.landmarks on the block alone; `lone`: the same for the bank's last frame, whose K tracks of one member
    follow the blocks'."""
    d = P + len(c["marked"])
    nt = c["tracks_per_block"]
    out = {key: [] for key in tn.LANDMARK_KEYS}
    for g in range(d + 2):
        lone = g == d + 1
        links, tr = block_tracks(c, g, lone)
        f = 1 if lone else BLOCK
        assert int(tr["n_tracks"][0]) == (c["K"] if lone else nt)
        r = tn.landmarks(c["kp"][g][:f], c["depth"][g][:f], c["C"][g][:f], tc.CAMERA, links["next"], links["next_frame"], tr["root_frame"],
                         tr["root_slot"], tr["n_tracks"], c["weight"][g][:f])
        for key in tn.LANDMARK_KEYS:
            out[key].append(r[key][:int(tr["n_tracks"][0])] if key not in ("residual", "kept") else r[key])
    lone = {key: out[key].pop() for key in tn.LANDMARK_KEYS}
    return dict(c, name=name, want={key: np.stack(v) for key, v in out.items()}, lone=lone)


@functools.lru_cache(maxsize=None)
def landmarks_past_2_31() -> dict:
    """sslt_landmarks on the big bank: 7384 tracks a block, xyz is 134 M * 24 bytes = 3.2 GB.  far: the last link of the last block."""
    return _landmark_case(link_pairs_past_2_31(), "landmarks_past_2_31")


FRAMES_K, FRAMES_BLOCKS, FRAMES_LINKS = 4, 5592410, 2      # 22 369 641 frames of 4 slots: C is 2 147 485 536 bytes


@functools.lru_cache(maxsize=None)
def landmarks_poses_past_2_31() -> dict:
    """sslt_landmarks on a bank of 22 369 641 frames of 4 keypoints, 89 M nodes: the poses C are 2.1475 GB, frame 22 369 621 - in block
    5 592 405 - holds their byte 2^31.  Blocks of four frames as in the big bank: three rows of 2 links and 2 slots that are none, a
    fourth row of no link; 16 - 6 = 10 tracks a block.  Every keypoint but one a block has a depth.  far: the last element of the
    last block's last C row."""
    k, n1, nb = FRAMES_K, FRAMES_K, FRAMES_BLOCKS
    marked = marks(nb, BLOCK * 96)
    d = P + len(marked)
    cam = tc.CAMERA
    ops = {key: [] for key in ("matches", "count", "mask", "kp", "depth", "C", "weight")}
    for g in range(d + 2):
        gg = min(g, d - 1)
        rng = np.random.default_rng(450 + gg if g != d + 1 else 498)
        Pw = np.stack([rng.uniform(-1.0, 1.0, k), rng.uniform(-0.7, 0.7, k), rng.uniform(1.5, 4.0, k)], axis=1)
        C = tc.poses(450 + gg, BLOCK)
        perm = np.stack([rng.permutation(k) for _ in range(BLOCK)])
        kp, depth = np.zeros((BLOCK, k, 2), np.float32), np.zeros((BLOCK, k), np.int32)
        for f in range(BLOCK):
            px, z = tc.project(C[f], Pw, cam)
            kp[f, perm[f]] = (px + rng.normal(size=px.shape) * 0.3).astype(np.float32)
            depth[f, perm[f]] = np.rint(z * cam.depth_scale).astype(np.int32)
        depth[rng.integers(0, BLOCK), rng.integers(0, k)] = 0
        if gg % 3 == 1:
            kp[2, perm[2, 0]] += np.float32(15.0)
        m, mask, count = np.zeros((BLOCK, n1, 2), np.int64), np.ones((BLOCK, n1), np.int32), np.zeros(BLOCK, np.int32)
        for r in range(BLOCK - 1):
            pts = rng.permutation(k)
            m[r, :2, 0], m[r, :2, 1] = perm[r, pts[:2]], perm[r + 1, pts[:2]]
            m[r, 2] = (m[r, 0, 0], perm[r + 1, pts[2]])        # an idx1 named again
            m[r, 3] = ((-1, k, 2 ** 40)[r], perm[r + 1, pts[3]])
            count[r] = (n1, n1 + 9, 3)[(gg + r) % 3]
        m[BLOCK - 1], count[BLOCK - 1] = rng.integers(0, k, (n1, 2)), (-3 if gg % 2 else 0)
        weight = rng.uniform(2.0 ** -6, 1.0, (BLOCK, k)).astype(np.float32)
        if gg % 4 == 2:
            weight[rng.integers(0, BLOCK), rng.integers(0, k)] = (0.0, np.nan, np.inf)[gg % 3]
        if gg == 3:
            C[1, 7] = np.inf
        if g == d:
            C[BLOCK - 1, 11] += 0.05
        for key, v in zip(ops, (m, count, mask, kp, depth, C, weight)):
            ops[key].append(v)
    c = dict({key: np.stack(v) for key, v in ops.items()}, K=k, n1=n1, n_blocks=nb, n_pairs=nb * BLOCK, n_bank=nb * BLOCK + 1, item_bytes=BLOCK * 96,
             marked=marked, tracks_per_block=BLOCK * k - (BLOCK - 1) * FRAMES_LINKS)
    return _landmark_case(_with_links(c, "", FRAMES_LINKS), "landmarks_poses_past_2_31")


KP_BANK_PAST_2_31 = dict(n_bank=65537, K=MAX_K, bytes_per_node=88)      # 8 + 4 + 4 + 4 + 4 in, 24 + 4 + 4 + 4 + 8 + 8 + 8 + 4 out


# ---- sslt_track_step on a bank of 600 M nodes
STEP_CAPACITY = 146485                    # * 4096 = 600 002 560 nodes: prev, next, track_id and age are 2.4 GB each


@functools.lru_cache(maxsize=None)
def track_step_past_2_31() -> dict:
    """The online bank at capacity * K = 600 M nodes.  The counter is set to t = 131 072, the frame holding byte 2^31 of `prev`, frame
    t - 1 having been filled by the test (ids from 1000 on in a scrambled order, ages, next_frame -1).  Steps: (1) at t with the link
    row (t - 1, t); (2) at t + 1 with no row; (3) the counter set to capacity - 1, the row (t + 1, capacity - 1); (4) the bank is
    full: status 4.  The restatement runs on a bank of four frames, `frames` naming what they stand for; far: step 3 again with the
    idx2 of the row's last link changed."""
    k, cap = MAX_K, STEP_CAPACITY
    t = FAR // (4 * k)
    assert cap * k <= tt.LIMITS["sslt_track_step"]["largest"]["nodes"] and t * k * 4 <= FAR < (t + 1) * k * 4 and t + 1 < cap - 1
    c = links_k_4096()
    rng = np.random.default_rng(331)
    filled = dict(track_id=(1000 + rng.permutation(k)).astype(np.int32), age=rng.integers(0, 50, k).astype(np.int32))
    frames = [t - 1, t, t + 1, cap - 1]

    def run(matches3):
        bank = tn.TrackBank(4, k)
        st = bank.state
        st["t"][0], st["next_id"][0] = 1, 5000
        st["track_id"][0], st["age"][0], st["next_frame"][0], st["prev_frame"][0], st["next"][0], st["prev"][0] = \
            filled["track_id"], filled["age"], -1, -1, -1, -1
        outs = [bank.step(c["matches"][0], c["count"][0], c["mask"][0], 0), bank.step(c["matches"][1], c["count"][1], c["mask"][1], -1),
                bank.step(matches3, c["count"][1], c["mask"][1], 2)]
        outs.append(bank.step(matches3, c["count"][1], c["mask"][1], 2))
        rows = {key: st[key].copy() for key in ("prev", "next", "track_id", "age")}
        real = lambda v: np.array([frames[x] if x >= 0 else -1 for x in v], np.int32)      # noqa: E731
        return outs, dict(rows, prev_frame=real(st["prev_frame"]), next_frame=real(st["next_frame"]), next_id=int(st["next_id"][0]))

    outs, state = run(c["matches"][1])
    outs_far, state_far = run(c["matches_far"][1])
    return dict(name="track_step_past_2_31", K=k, capacity=cap, t=t, frames=frames, filled=filled, rows=c, first=[t - 1, -1, t + 1, t + 1],
                outs=outs, state=state, outs_far=outs_far, state_far=state_far)


# =============================================================================================================== libsslam_place.so
PLACE = pt.LIMITS["sslp_place_step"]["largest"]
OWN_FRAMES = (0, 31, 32, 4064, 4095)      # descriptors of their own: the first frame, both sides of the first group's end, the last
PLANTED_FRAMES = (255, 256, 512, 1000, 1001, 2000, 4000)       # one descriptor, bit for bit: equal similarities in different waves, 256 and 512 in one thread
SUPPRESS = dict(many_left=0, exactly_8=1, fewer_than_8=600)


def _unit_rows(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def raw_of(desc, scores):
    """place_ref.step's raw sum of one frame: the fmaf chain over the keypoints."""
    acc = np.zeros(desc.shape[1], np.float32)
    for kk in range(len(scores)):
        acc = pr.fmaf32(scores[kk], desc[kk], acc)
    return acc


@functools.lru_cache(maxsize=None)
def bank_at_the_capacity_limit() -> dict:
    """capacity 4096, d 256, k 3, per_frame 8, min_gap 30, min_sim 0.3.  Frame i shows place i % 7 of seven unrelated places, except:
    the frames of OWN_FRAMES and the frames 4094 (the first frame stepped) hold descriptors of their own near one query place Q, and
    the frames of PLANTED_FRAMES all hold one more descriptor near Q, bit for bit.  At t = 4094 and t = 4095 the candidates are so
    the eleven frames 0, 31, 32, 255, 256, 512, 1000, 1001, 2000, 4000, 4064 and no other: suppress 0 leaves candidates after the
    eighth pick, suppress 1 leaves exactly eight picks (31 | 32, 255 | 256 and 1000 | 1001 fall to one each), suppress 600 fewer.
    `state`: the restatement's state after the frames 0 .. 4093 - raw by the fmaf chain, sum by the running float32 additions -
    never stepped: the device test uploads it.  far: raw[4064, 255] of that state changed, the last word similarity_kernel reads at
    t = 4094."""
    cap, d, k, per = PLACE["capacity"], PLACE["d"], 3, PLACE["per_frame"]
    rng = np.random.default_rng(501)
    places = _unit_rows(rng.standard_normal((P + 1, d)))
    q = places[P]
    family = _unit_rows(q + 0.5 * _unit_rows(rng.standard_normal((len(OWN_FRAMES) + 2, d))))      # own frames, 4094, the planted one
    slot = np.arange(cap) % P
    slot[list(OWN_FRAMES)] = P + np.arange(len(OWN_FRAMES))
    slot[cap - 2] = P + len(OWN_FRAMES)
    slot[list(PLANTED_FRAMES)] = P + len(OWN_FRAMES) + 1
    centre = np.concatenate([places[:P], family])
    desc = _unit_rows(centre[:, None, :] + 0.1 * _unit_rows(rng.standard_normal((len(centre), k, d))))
    scores = rng.uniform(0.1, 1.0, (len(centre), k)).astype(np.float32)
    raw_d = np.stack([raw_of(desc[i], scores[i]) for i in range(len(centre))])
    t0 = cap - 2
    state = pr.fresh_state(cap, d)
    state["raw"][:t0] = raw_d[slot[:t0]]
    total = np.zeros(d, np.float32)
    for i in range(t0):
        total = total + state["raw"][i]
    state["sum"][...], state["t"][...] = total, t0
    state["raw"][t0:] = np.float32(-7.5)                       # the two rows the steps write
    far_state = {key: v.copy() for key, v in state.items()}
    far_state["raw"][4064, d - 1] += np.float32(0.25)
    return dict(name="bank_at_the_capacity_limit", capacity=cap, d=d, k=k, per_frame=per, min_gap=30, min_sim=0.3, slot=slot, desc=desc, scores=scores,
                state=state, far_state=far_state, t0=t0)


def place_steps(c, suppress, state=None, per_frame=None, n=3):
    """The steps t0, t0 + 1 and one on the full bank through place_ref.step on a copy of the case's state: (outputs, final state)."""
    st = {key: v.copy() for key, v in (c["state"] if state is None else state).items()}
    outs = []
    for i in range(n):
        s = c["slot"][min(c["t0"] + i, c["capacity"] - 1)]
        outs.append(pr.step(st, c["desc"][s], c["scores"][s], c["min_gap"], c["min_sim"], c["per_frame"] if per_frame is None else per_frame, suppress))
    return outs, st


@functools.lru_cache(maxsize=None)
def place_expected(which: str, far: bool = False):
    c = bank_at_the_capacity_limit()
    return place_steps(c, SUPPRESS[which], c["far_state"] if far else None)


@functools.lru_cache(maxsize=None)
def bank_at_the_keypoint_limit() -> dict:
    """k 4096, d 256, capacity 5, min_gap 1: raw_kernel's chain of 4096 fmaf per column, dp[kk * d] to word 1 048 575.  Four frames
    near one place are stepped; far: the last descriptor element of the last frame."""
    k, d, cap, n = PLACE["k"], PLACE["d"], 5, 4
    rng = np.random.default_rng(502)
    q = _unit_rows(rng.standard_normal(d))
    desc = _unit_rows(q + 0.8 * _unit_rows(rng.standard_normal((n, k, d))) + 0.3 * _unit_rows(rng.standard_normal((n, 1, d))))
    scores = rng.uniform(0.1, 1.0, (n, k)).astype(np.float32)
    far = desc.copy()
    far[n - 1, k - 1, d - 1] += np.float32(0.5)
    c = dict(name="bank_at_the_keypoint_limit", capacity=cap, d=d, k=k, per_frame=2, min_gap=1, min_sim=-2.0, suppress=0, desc=desc, scores=scores,
             desc_far=far)
    c["outs"], c["state"] = pr.run(desc, scores, cap, 1, -2.0, 2, 0)
    c["outs_far"], c["state_far"] = pr.run(far, scores, cap, 1, -2.0, 2, 0)
    return c


LOG_SLOTS, LOG_CAPACITY = pt.LIMITS["sslp_edge_log_step"]["largest"]["n_slots"], 800000


@functools.lru_cache(maxsize=None)
def edge_log_past_2_31() -> dict:
    """n_slots 16, capacity 800 000: log_info is 12.8 M rows of 168 bytes, 2.15 GB.  One step at the frame whose rows hold byte 2^31
    of log_info, one at capacity - 1, one on the full log.  Sixteen slots of every kind: logged odometry and loop slots, too few
    inliers of either kind, status 3, a first of -1, of t and past t, NaN in T and inf in info.  `rows`: per step the sixteen rows
    the restatement writes; far: the last element of new_info, of a logged slot, changed in the step at capacity - 1."""
    E, cap = LOG_SLOTS, LOG_CAPACITY
    t_far = FAR // 168 // E
    assert t_far * E * 168 <= FAR < (t_far + 1) * E * 168 and t_far < cap - 1
    rng = np.random.default_rng(503)

    def inputs(t, seed):
        r = np.random.default_rng(seed)
        T, info = r.standard_normal((E, 12)), r.standard_normal((E, 21))
        first = r.integers(0, t, E).astype(np.int32)
        status, inliers = r.integers(0, 3, E).astype(np.int32), r.integers(30, 200, E).astype(np.int32)
        first[1], first[2], first[3] = -1, t, t + 5
        status[4] = 3
        inliers[5], inliers[9] = 11, 19                        # below min_inliers 12 (odometry); below loop_min_inliers 20 (loop)
        inliers[6], inliers[10] = 12, 20                       # exactly at either
        T[7, 3], info[11, 20] = np.nan, np.inf
        first[E - 1], status[E - 1], inliers[E - 1] = t - 1, 0, 100      # the last slot is logged
        return dict(slot_first=first, new_T=T, new_info=info, new_status=status, new_inliers=inliers)

    def run(t, ins):
        st = pr.fresh_log(cap, E)                              # zero pages of the host: only the step's rows are ever touched
        st["t"][...] = t
        out = pr.log_step(st, ins["slot_first"], ins["new_T"], ins["new_info"], ins["new_status"], ins["new_inliers"], 8, 12, 20)
        lo, hi = t * E, (t + 1) * E
        rows = None if t >= cap else {key: st[key][lo:hi].copy() for key in pr.LOG_STATE_KEYS[1:]}
        return dict(out=out, rows=rows, t_after=int(st["t"]))

    steps = [dict(t=t, ins=inputs(t, 510 + i)) for i, t in enumerate((t_far, cap - 1, cap))]
    for s in steps:
        s.update(run(s["t"], s["ins"]))
    far_ins = {key: v.copy() for key, v in steps[1]["ins"].items()}
    far_ins["new_info"][E - 1, 20] += 1.0
    del rng
    return dict(name="edge_log_past_2_31", n_slots=E, capacity=cap, n_odometry=8, min_inliers=12, loop_min_inliers=20, t_far=t_far, steps=steps,
                far=dict(t=cap - 1, ins=far_ins, **run(cap - 1, far_ins)))


# ============================================================================================================== libsslam_window.so
WINDOWS = wnt.LIMITS["sslw_window_step"]["largest"]["n_windows"]
WINDOW_CAPACITY, WINDOW_STEPS = 400, 6


@functools.lru_cache(maxsize=None)
def windows_at_the_count_limit() -> dict:
    """65 535 windows of 2 frames, one spacing, capacity 400: the trajectory is 65 535 * 400 * 96 bytes = 2.5 GB, window 55 924 holds
    its byte 2^31, the workspace is 12.1 GB.  Six steps of distinct planted windows (tests/window_cases.py), periodic with windows
    of their own at 0, 55 924 and 65 534; the trajectories start filled with 7.25 so that a stray write shows.  far: the last step
    again, with one element of window 65 534's new_T changed."""
    n, cap, steps = WINDOWS, WINDOW_CAPACITY, WINDOW_STEPS
    frame_bytes = cap * 96
    marked = marks(n, frame_bytes)
    d = P + len(marked)
    cases = [wc.window_case(f"window_{g}", 2, (1,), steps, 600 + g, capacity=cap) for g in range(d)]
    cases[2]["status"][3, 0] = 3                               # a refused pair: the frame is lost, the pose carried over
    cases[4]["inliers"][2, 0] = 5
    cases[5]["T"][4, 0, 6] = np.nan
    ins = wc.stacked(cases)                                    # (steps, d, S, ...)
    outs, states, before_last = [], [], []
    for c in cases:
        st = wf.fresh_state(2, 1, cap)
        st["trajectory"][...] = 7.25
        o = []
        for i in range(steps):
            if i == steps - 1:
                before_last.append({key: v.copy() for key, v in st.items()})
            o.append(wf.step(st, c["spacings"], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], None, c["min_inliers"], c["chi"],
                             c["damping"], c["n_iter"]))
        outs.append(o)
        states.append(st)
    want = [{key: np.stack([outs[g][i][key] for g in range(d)]) for key in wf.OUT_KEYS} for i in range(steps)]
    state = {key: np.stack([states[g][key] for g in range(d)]) for key in wf.STATE_KEYS}
    c = cases[d - 1]
    T_far = c["T"][steps - 1].copy()
    T_far[0, 11] += 0.125
    st = before_last[d - 1]
    out_far = wf.step(st, c["spacings"], T_far, c["info"][steps - 1], c["status"][steps - 1], c["inliers"][steps - 1], None, c["min_inliers"], c["chi"],
                      c["damping"], c["n_iter"])
    return dict(name="windows_at_the_count_limit", n=n, window=2, spacings=np.array([1], np.int32), capacity=cap, steps=steps, frame_bytes=frame_bytes,
                marked=marked, ins=ins, want=want, state=state, T_far=T_far, out_far=out_far, state_far=st, min_inliers=c["min_inliers"], chi=c["chi"],
                damping=c["damping"], n_iter=c["n_iter"], workspace_bytes=wnt.workspace_bytes(n, 2, 1))


FAR_WINDOW_CAPACITY = 22369700            # frames of one window's trajectory: 2 147 491 200 bytes


@functools.lru_cache(maxsize=None)
def window_at_a_far_frame() -> dict:
    """One window of 2 frames whose trajectory holds 22 369 700 frames, 2.1475 GB: `frame * 12` past 2^31 bytes.  The restatement steps
    a planted window three times from 0, its frame numbers are then moved up by an even 22 369 618 - the ring's rows are t % 2 - and it
    steps at t = 22 369 621 (whose trajectory row holds byte 2^31) and t + 1, then - the counter set - at capacity - 1 and at capacity,
    which writes the row capacity - 1 alone.  `rows`: frame -> the trajectory row the restatement leaves; far: the step at
    capacity - 1 with one element of new_T changed."""
    cap, W = FAR_WINDOW_CAPACITY, 2
    t0 = FAR // 96
    assert t0 * 96 <= FAR < (t0 + 1) * 96 and t0 % 2 == 1 and t0 + 1 < cap - 1 and cap * 96 > FAR
    c = wc.window_case("window_at_a_far_frame", W, (1,), 8, 640, capacity=cap)
    args = (None, c["min_inliers"], c["chi"], c["damping"], c["n_iter"])
    st = wf.fresh_state(W, 1, 8)
    for i in range(3):
        wf.step(st, c["spacings"], c["T"][i], c["info"][i], c["status"][i], c["inliers"][i], *args)
    shift = t0 - 3
    st["trajectory"] = np.zeros((cap, 12))                     # zero pages of the host: only the steps' rows are ever touched
    st["t"][...] = t0
    st["ring_first"][st["ring_first"] >= 0] += shift
    st["ring_second"] += shift
    start = {key: st[key].copy() for key in wf.STATE_KEYS if key != "trajectory"}
    frames = [t0, t0 + 1, cap - 1, cap]
    outs, before_third = [], None
    for i, t in enumerate(frames):
        st["t"][...] = t
        if i == 2:
            before_third = {key: st[key].copy() for key in wf.STATE_KEYS if key != "trajectory"}
        outs.append(wf.step(st, c["spacings"], c["T"][3 + i], c["info"][3 + i], c["status"][3 + i], c["inliers"][3 + i], *args))
    written = [t0 - 1, t0, t0 + 1, cap - 2, cap - 1]
    rows = {f: st["trajectory"][f].copy() for f in written}
    final = {key: st[key].copy() for key in wf.STATE_KEYS if key != "trajectory"}
    T_far = c["T"][5].copy()
    T_far[0, 11] += 0.125
    far = dict(before_third, trajectory=st["trajectory"])
    far["t"] = np.array(cap - 1, np.int32)
    out_far = wf.step(far, c["spacings"], T_far, c["info"][5], c["status"][5], c["inliers"][5], *args)
    rows_far = {f: far["trajectory"][f].copy() for f in (cap - 2, cap - 1)}
    return dict(name="window_at_a_far_frame", capacity=cap, window=W, spacings=c["spacings"], t0=t0, frames=frames, ins={key: c[key][3:7] for key in
                ("T", "info", "status", "inliers")}, start=start, outs=outs, rows=rows, final=final, before_third=before_third, T_far=T_far,
                out_far=out_far, rows_far=rows_far, min_inliers=c["min_inliers"], chi=c["chi"], damping=c["damping"], n_iter=c["n_iter"])


# ================================================================================================================ libsslam_conf.so
CONF_D = ct.LIMITS["sslc_confidence_rows"]["largest"]["D"]
CONF_HEAD = "wide"                        # tests/confidence_cases.py's head of descriptor width 256


def conf_weights():
    return cr.weight_list(cc.head_state(CONF_HEAD))


CONF_ROWS = {"confidence_rows_past_2_31": 1450003, "confidence_rows_desc_past_2_31": 2100003}


@functools.lru_cache(maxsize=None)
def confidence_rows(name: str) -> dict:
    """confidence_rows_past_2_31: 1 450 003 rows at D = 256 - x is 2.23 GB, row 1 398 101 holds its byte 2^31.  45 313 tiles of 32 rows:
    the last tile holds 19 rows, and 45 313 = 8 * 5664 + 1, so one XCD takes a tile more than the others.
    confidence_rows_desc_past_2_31: 2 100 003 rows - desc passes 2^31 bytes as well (row 2 097 152), x is 3.2 GB; 65 626 tiles, a
    remainder of 2.  The marks are x's and desc's.  far: x[rows - 1, 383]."""
    n, d = CONF_ROWS[name], CONF_D
    assert n % ct.TILE_ROWS and -(-n // ct.TILE_ROWS) % 8
    marked = sorted(set(marks(n, ct.DINO_DIM * 4)) | set(marks(n, d * 4)))
    nd = P + len(marked)
    rng = np.random.default_rng(701)
    x, desc = (1.5 * rng.standard_normal((nd, ct.DINO_DIM))).astype(np.float32), _unit_rows(rng.standard_normal((nd, d)))
    x_far = x[-1].copy()
    x_far[-1] += np.float32(6.0)
    w = conf_weights()
    return dict(name=name, n=n, D=d, frame_bytes=ct.DINO_DIM * 4, marked=marked, x=x, desc=desc, want=cr.confidence_rows(x, desc, w),
                x_far=x_far, want_far=cr.confidence_rows(x_far[None], desc[-1:], w)[0])


GATHER_G, GATHER_FRAMES, GATHER_K = 40, 3500, 5


@functools.lru_cache(maxsize=None)
def gather_confidence_past_2_31() -> dict:
    """G = 40, 3500 frames, K = 5: feat is 3500 * 1600 * 384 = 2.15e9 floats, 8.6 GB - frame 873 holds its byte 2^31, frame 3495 its
    float 2^31 (byte 2^33): the marks are both, 0 and the end.  17 500 rows, 547 tiles.  The last keypoint of every frame sits on the
    last cell; far: the last float of the last frame's map."""
    n, g, k, d = GATHER_FRAMES, GATHER_G, GATHER_K, CONF_D
    fb = g * g * ct.DINO_DIM * 4
    marked = sorted(set(marks(n, fb)) | set(marks(n, fb, 4 * FAR)))
    assert len(marked) == 4 and n * g * g * ct.DINO_DIM > FAR
    nd = P + len(marked)
    rng = np.random.default_rng(702)
    feat = (1.5 * rng.standard_normal((nd, g, g, ct.DINO_DIM))).astype(np.float32)
    kp = rng.uniform(0, g - 1, (nd, k, 2)).astype(np.float32)
    kp[:, 0] = (0.0, 0.0)
    kp[:, k - 1] = (g - 1, g - 1)
    desc = _unit_rows(rng.standard_normal((nd, k, d)))
    feat_far = feat[-1].copy()
    feat_far[g - 1, g - 1, -1] += np.float32(6.0)
    w = conf_weights()
    return dict(name="gather_confidence_past_2_31", n=n, G=g, K=k, D=d, frame_bytes=fb, marked=marked, feat=feat, kp=kp, desc=desc,
                want=cr.gather_confidence(feat, kp, desc, w), feat_far=feat_far, want_far=cr.gather_confidence(feat_far[None], kp[-1:], desc[-1:], w)[0])


FILTER_K, BIG_FRAMES = ct.LIMITS["sslc_confidence_filter"]["largest"]["K"], 131080      # * 4096 * 4 bytes = 2.1476 GB


@functools.lru_cache(maxsize=None)
def confidence_filter_past_2_31() -> dict:
    """K = 4096, 131 080 frames: conf, slot and conf_out are 2.15 GB each, frame 131 072 holds byte 2^31.  Threshold 0.5.  Among the
    distinct frames: none passes (the largest alone is kept, twice the largest), all pass, NaNs, values equal to the threshold.
    far: the last confidence of the last frame, from below the threshold to above it."""
    n, k = BIG_FRAMES, FILTER_K
    marked = marks(n, k * 4)
    nd = P + len(marked)
    rng = np.random.default_rng(703)
    conf = rng.uniform(0.0, 1.0, (nd, k)).astype(np.float32)
    conf[1] = rng.uniform(0.0, 0.49, k)
    conf[1, [77, 3000]] = np.float32(0.4925)                   # none passes: the first of the two largest
    conf[2] = rng.uniform(0.5, 1.0, k)
    conf[3, ::5], conf[3, 4095] = np.nan, np.nan
    conf[4, ::3] = np.float32(0.5)
    conf[5] = np.nan
    conf[-1, k - 1] = np.float32(0.25)
    far = conf[-1].copy()
    far[k - 1] = np.float32(0.75)
    return dict(name="confidence_filter_past_2_31", n=n, K=k, threshold=0.5, frame_bytes=k * 4, marked=marked, conf=conf,
                want=dict(zip(("slot", "count", "confidence"), cr.confidence_filter(conf, 0.5))), conf_far=far,
                want_far={key: v[0] for key, v in zip(("slot", "count", "confidence"), cr.confidence_filter(far[None], 0.5))})


TAKE_WIDTH = 256
TAKE_SHAPES = {"take_rows_past_2_31": (BIG_FRAMES, 16), "take_rows_at_the_word_limit": (178481, 47)}


@functools.lru_cache(maxsize=None)
def take_rows(name: str) -> dict:
    """width 256.  take_rows_past_2_31: K = 16, 131 080 frames - src and dst are 2 097 280 rows of 1 KB, 2.1476 GB each.
    take_rows_at_the_word_limit: K = 47, 178 481 frames - 8 388 607 rows, 2 147 483 392 words, the most rows of this width below the
    limit of 2^31 - 1 words; 8.6 GB each; one frame more is refused.  The slots include -1, K, 2^31 - 1, the most negative int and
    repeats.  far: the last slot of the last frame."""
    (n, k), w = TAKE_SHAPES[name], TAKE_WIDTH
    assert n * k * w <= ct.LIMITS["sslc_take_rows"]["largest"]["words"]
    marked = marks(n, k * w * 4)
    nd = P + len(marked)
    rng = np.random.default_rng(704)
    src = rng.integers(-2 ** 31, 2 ** 31, (nd, k, w), dtype=np.int64).astype(np.int32)
    slot = rng.integers(0, k, (nd, k)).astype(np.int32)
    slot[:, 3] = np.array([-1, k, 2 ** 31 - 1, -2 ** 31, k + 1, -2, 0, k - 1, -1, k])[:nd]
    slot[:, 5] = slot[:, 6]
    slot[-1, k - 1] = 2
    far = slot[-1].copy()
    far[k - 1] = k - 1
    return dict(name=name, n=n, K=k, width=w, frame_bytes=k * w * 4, marked=marked, src=src, slot=slot, want=cr.take_rows(src, slot),
                slot_far=far, want_far=cr.take_rows(src[-1:], far[None])[0])


# ============================================================================================================== libsslam_weight.so
PAIR_BYTES = MAX_K * 16                   # one pair's matches at n1 = 4096
BANK_PERIOD = 20                          # frames of the distinct bank: pair slot s reads frames 2 s and 2 s + 1 of some period


def pair_frames(n_pairs, marked, periods):
    """first, second (n_pairs,) int64: pair p reads the frames 2 s, 2 s + 1 (s its slot of the distinct set) of period (p + 1) %
    periods of a bank that repeats its BANK_PERIOD distinct frames - so the pairs read all over the bank, and pair 32 768, which holds
    byte 2^31 of `matches`, reads the bank's last period, past ITS byte 2^31, with both period counts used here."""
    s = slots(n_pairs, marked)
    base = BANK_PERIOD * ((np.arange(n_pairs, dtype=np.int64) + 1) % periods)
    return base + 2 * s, base + 2 * s + 1


@functools.lru_cache(maxsize=None)
def match_weights_past_2_31() -> dict:
    """n1 = K = 4096, 32 776 pairs: matches is 2.148 GB, pair 32 768 holds its byte 2^31; conf_bank is 131 080 frames of 4096
    floats, 2.1476 GB, 6554 periods of twenty distinct frames, read by the pairs all over (pair_frames).  Both modes.  The pairs of
    slot 5 name a first frame past the bank: absent, weight 0.  Counts of 0, below n1 and above it; indices -1, K and 2^40;
    confidences 0, 1, the least normal float and 1e-30.  far: the idx2 of the last slot of the last pair."""
    n, k, n1 = BIG_PAIRS, MAX_K, MAX_K
    n_bank = BIG_FRAMES
    periods = n_bank // BANK_PERIOD
    assert periods * BANK_PERIOD == n_bank and n * n1 <= wt.LIMITS["sslu_match_weights"]["largest"]["slots"]
    marked = marks(n, PAIR_BYTES)
    nd = P + len(marked)
    assert 2 * nd == BANK_PERIOD
    rng = np.random.default_rng(801)
    conf = rng.uniform(0.05, 1.0, (BANK_PERIOD, k)).astype(np.float32)
    conf.reshape(-1)[rng.permutation(conf.size)[:400]] = np.array([0.0, 1.0, 1.17549435e-38, 1e-30], np.float32)[np.arange(400) % 4]
    m = rng.integers(0, k, (nd, n1, 2)).astype(np.int64)
    for g in range(nd):
        j = rng.permutation(n1)[:60]
        m[g, j[:20], 0], m[g, j[20:40], 1], m[g, j[40:], 0] = -1, k, 2 ** 40
    count = np.array([n1, n1 + 5, 0, 1000, -4, n1, 257, n1, n1, n1], np.int32)[:nd]
    first_d, second_d = 2 * np.arange(nd, dtype=np.int32), 2 * np.arange(nd, dtype=np.int32) + 1
    absent = 5
    first_d[absent] = -1                                       # stands for "past the bank": the device test names n_bank there
    m[-1, n1 - 1] = (9, 11)
    far = m[-1].copy()
    far[n1 - 1, 1] = 12
    conf[2 * (nd - 1) + 1, 11], conf[2 * (nd - 1) + 1, 12] = 0.5, 0.25
    want = {mode: wr.match_weights(conf, first_d, second_d, m, count, mode, 0.5) for mode in (wt.WEIGHT_PRODUCT, wt.WEIGHT_EXPECTED_ERROR)}
    want_far = {mode: wr.match_weights(conf, first_d[-1:], second_d[-1:], far[None], count[-1:], mode, 0.5)[0] for mode in want}
    return dict(name="match_weights_past_2_31", n=n, K=k, n1=n1, n_bank=n_bank, periods=periods, frame_bytes=PAIR_BYTES, marked=marked, conf=conf,
                matches=m, count=count, absent=absent, sigma0=0.5, want=want, matches_far=far, want_far=want_far)


REFINE_PERIODS = 3277                     # * 20 frames of 4096 keypoints: kp_bank is 65 540 * 32 KB = 2.1476 GB


@functools.lru_cache(maxsize=None)
def weighted_refine_past_2_31() -> dict:
    """sslu_pose_refine_weighted_pairs at K = n1 = 4096 on 32 776 pairs, n_iter 1: matches is 2.148 GB, weights and inlier_of_slot
    537 MB, kp_bank 65 540 frames, 2.1476 GB, read all over by the pairs (pair_frames).  Ten distinct pairs of
    tests/pose_ransac_cases.py's planted two-view scenes, 5 % outliers, from a prior 2 degrees and 5 cm off; weights in 2^-10 .. 1 with
    zeros, NaNs, infinities, negative and subnormal ones.  far: the idx2 of the last listed slot of the last pair."""
    n, k = BIG_PAIRS, MAX_K
    marked = marks(n, PAIR_BYTES)
    nd = P + len(marked)
    specs = [dict(outliers=0.05)] * nd
    specs[1], specs[4] = dict(outliers=0.3, holes=True, bad_idx=True), dict(outliers=0.05, count=3000)
    c = rc._case("weighted_refine_past_2_31", k, k, specs, 1, rc.SCALE_448, 811)
    assert c["first"].tolist() == list(range(0, 2 * nd, 2)) and len(c["bank"]) == BANK_PERIOD
    T_in = pc._initial("prior", c, None)
    rng = np.random.default_rng(812)
    weight = rng.uniform(2.0 ** -10, 1.0, (nd, k)).astype(np.float32)
    bad = rng.permutation(weight.size)[:500]
    weight.reshape(-1)[bad] = np.array([0.0, np.nan, np.inf, -1.0, 1e-41], np.float32)[np.arange(500) % 5]
    threshold, huber, n_iter = 60.0, 20.0, 1
    run = lambda first, second, m, cnt, w, T: wr.stacked(wr.refine_pairs(c["bank"], c["depth_bank"], first, second, m, cnt, w, c["cam"],      # noqa: E731
                                                                         threshold, huber, n_iter, T, c["scale_x"], c["scale_y"]))
    want = run(c["first"], c["second"], c["matches"], c["count"], weight, T_in)
    far = c["matches"][-1].copy()
    j = int(c["count"][-1]) - 1
    far[j, 1] = far[j - 1, 1]
    weight[-1, j] = np.float32(1.0)
    want = run(c["first"], c["second"], c["matches"], c["count"], weight, T_in)
    want_far = run(c["first"][-1:], c["second"][-1:], far[None], c["count"][-1:], weight[-1:], T_in[-1:])
    return dict(name="weighted_refine_past_2_31", n=n, K=k, n1=k, n_bank=REFINE_PERIODS * BANK_PERIOD, periods=REFINE_PERIODS, frame_bytes=PAIR_BYTES,
                marked=marked, bank=c["bank"], depth_bank=c["depth_bank"], matches=c["matches"], count=c["count"], weight=weight, T_in=T_in,
                cam=c["cam"], scale_x=c["scale_x"], scale_y=c["scale_y"], threshold=threshold, huber=huber, n_iter=n_iter, want=want,
                matches_far=far, want_far={key: v[0] for key, v in want_far.items()})
