"""include/sslam_track.h in numpy: the four entries of libsslam_track.so as the header states them - match lists to links
(link_pairs), links to tracks (track_ids), tracks to map points (landmarks, float64 scalars in the header's order, nothing through
np.dot, @, np.sum or np.linalg) and the online bank (TrackBank).  It needs no GPU and gives the bits the device entries give:
evaluation.build_tracks, evaluation.track_landmarks and evaluation.TrackBank run it, as evaluation.PoseWindow runs window_numpy.  A
caller on the device uses SequencePipeline.link_matches / track_ids / landmarks / track_step."""
from __future__ import annotations

import numpy as np

MAX_K = 4096
SCAN_TILE = 1024
LINK_KEYS = ("prev", "next", "prev_frame", "next_frame")
TRACK_KEYS = ("track_id", "age", "n_tracks", "root_frame", "root_slot", "length")
LANDMARK_KEYS = ("xyz", "n_obs", "n_kept", "status", "weight_sum", "rms", "residual", "kept")
BANK_STATE_KEYS = ("t", "next_id", "prev", "next", "prev_frame", "next_frame", "track_id", "age")
BANK_OUT_KEYS = ("track_id", "age", "n_new", "status")
COUNTER_OUT_OF_RANGE = 4
_QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def workspace_bytes(n_bank: int, k: int) -> int:
    """sslt_track_workspace_bytes, restated."""
    n = n_bank * k
    return 20 * n + 4 * (-(-n // SCAN_TILE))


def link_slots(matches, count, mask, k: int):
    """The LINK SLOT rule on one row: matches (n1, 2) int64, count, mask (n1,) int32 or None -> the links (idx1, idx2) as two int
    arrays, in slot order."""
    m = np.asarray(matches, np.int64)
    n1 = len(m)
    cnt = min(max(int(count), 0), n1)
    i1, i2 = m[:cnt, 0], m[:cnt, 1]
    valid = (i1 >= 0) & (i1 < k) & (i2 >= 0) & (i2 < k)
    if mask is not None:
        valid &= np.asarray(mask)[:cnt] == 1
    j = np.flatnonzero(valid)
    lo1, lo2 = np.full(k, n1, np.int64), np.full(k, n1, np.int64)
    np.minimum.at(lo1, i1[j], j)
    np.minimum.at(lo2, i2[j], j)
    link = j[(lo1[i1[j]] == j) & (lo2[i2[j]] == j)]
    return i1[link].astype(np.int32), i2[link].astype(np.int32)


def link_pairs(first, second, matches, count, mask, n_bank: int, k: int) -> dict:
    """sslt_link_pairs: first, second (P,) int32; matches (P, n1, 2) int64; count (P,) int32; mask (P, n1) int32 or None ->
    LINK_KEYS' arrays: prev, next (n_bank, k) and prev_frame, next_frame (n_bank,) int32, -1 meaning none."""
    first, second = np.asarray(first, np.int64), np.asarray(second, np.int64)
    prev, nxt = np.full((n_bank, k), -1, np.int32), np.full((n_bank, k), -1, np.int32)
    prev_frame, next_frame = np.full(n_bank, -1, np.int32), np.full(n_bank, -1, np.int32)
    valid = (first >= 0) & (first < second) & (second < n_bank)
    seen_first, seen_second = set(), set()
    for p in np.flatnonzero(valid):
        a, b = int(first[p]), int(second[p])
        lowest = a not in seen_first and b not in seen_second
        seen_first.add(a), seen_second.add(b)
        if not lowest:
            continue
        i1, i2 = link_slots(matches[p], count[p], None if mask is None else mask[p], k)
        nxt[a, i1], prev[b, i2] = i2, i1
        next_frame[a], prev_frame[b] = b, a
    return dict(prev=prev, next=nxt, prev_frame=prev_frame, next_frame=next_frame)


def track_ids(prev, prev_frame) -> dict:
    """sslt_track_ids: prev (n_bank, k), prev_frame (n_bank,) int32 -> TRACK_KEYS' arrays.  Frames ascend along a chain, so one pass
    over the frames in order sees every predecessor before its successor."""
    prev, prev_frame = np.asarray(prev, np.int32), np.asarray(prev_frame, np.int32)
    n_bank, k = prev.shape
    n = n_bank * k
    root = np.arange(n, dtype=np.int64).reshape(n_bank, k)
    age = np.zeros((n_bank, k), np.int32)
    for f in range(n_bank):
        pf = int(prev_frame[f])
        if not 0 <= pf < f:
            continue
        has = (prev[f] >= 0) & (prev[f] < k)
        root[f, has], age[f, has] = root[pf, prev[f, has]], age[pf, prev[f, has]] + 1
    flat = root.reshape(-1)
    is_root = flat == np.arange(n)
    number = np.cumsum(is_root) - is_root                  # the exclusive scan of the root flags
    track_id = number[flat].astype(np.int32).reshape(n_bank, k)
    n_tracks = int(is_root.sum())
    roots = np.flatnonzero(is_root)
    root_frame, root_slot, length = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    root_frame[:n_tracks], root_slot[:n_tracks] = roots // k, roots % k
    length[:n_tracks] = np.bincount(track_id.reshape(-1), minlength=n_tracks)
    return dict(track_id=track_id, age=age, n_tracks=np.array([n_tracks], np.int32), root_frame=root_frame, root_slot=root_slot, length=length)


def members(i: int, nxt, next_frame, root_frame, root_slot) -> list:
    """The members (frame, slot) of track i, by the header's walk."""
    n_bank, k = nxt.shape
    f, s = int(root_frame[i]), int(root_slot[i])
    out = []
    if not (0 <= f < n_bank and 0 <= s < k):
        return out
    while True:
        out.append((f, s))
        nf, ns = int(next_frame[f]), int(nxt[f, s])
        if not (f < nf < n_bank and 0 <= ns < k):
            return out
        f, s = nf, ns


def _camera(camera, scale_x, scale_y):
    return tuple(np.float64(v) for v in (camera.fx, camera.fy, camera.cx, camera.cy, camera.depth_scale, scale_x, scale_y))


def world_point(x, y, d, c, cam):
    """Xw = R^T (Xc - t) of keypoint (x, y) (float64) with raw depth d under the C row c (12,), the header's operations."""
    fx, fy, cx, cy, ds, sx, sy = cam
    u, v, z = x * sx, y * sy, np.float64(d) / ds
    X, Y = ((u - cx) * z) / fx, ((v - cy) * z) / fy
    ex, ey, ez = X - c[3], Y - c[7], z - c[11]
    return [(c[j] * ex + c[4 + j] * ey) + c[8 + j] * ez for j in range(3)]


def score(c, cam, L, x, y):
    """s of the point L in the frame with C row c against keypoint (x, y): dx*dx + dy*dy, +inf unless Z' > 0."""
    fx, fy, cx, cy, _, sx, sy = cam
    Xp = ((c[0] * L[0] + c[1] * L[1]) + c[2] * L[2]) + c[3]
    Yp = ((c[4] * L[0] + c[5] * L[1]) + c[6] * L[2]) + c[7]
    Zp = ((c[8] * L[0] + c[9] * L[1]) + c[10] * L[2]) + c[11]
    up, vp = (fx * Xp) / Zp + cx, (fy * Yp) / Zp + cy
    dx, dy = up / sx - x, vp / sy - y
    return dx * dx + dy * dy if Zp > 0.0 else np.float64(np.inf)


def landmarks(kp_bank, kp_depth_bank, C, camera, nxt, next_frame, root_frame, root_slot, n_tracks, weight=None, threshold=3.0,
              min_obs: int = 2, scale_x=1.0, scale_y=1.0) -> dict:
    """sslt_landmarks: kp_bank (n_bank, k, 2) fp32, kp_depth_bank (n_bank, k) int32, C (n_bank, 12) float64, camera an object with
    fx, fy, cx, cy, depth_scale; the links and roots of link_pairs and track_ids; weight (n_bank, k) fp32 or None ->
    LANDMARK_KEYS' arrays, per track (n_bank * k rows) and per keypoint."""
    kp = np.asarray(kp_bank, np.float32).astype(np.float64)
    depth, C = np.asarray(kp_depth_bank, np.int32), np.asarray(C, np.float64).reshape(len(kp), 12)
    n_bank, k = depth.shape
    n = n_bank * k
    cam, thr = _camera(camera, scale_x, scale_y), np.float64(threshold)
    g_bank = None if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    nt = min(max(int(np.asarray(n_tracks).reshape(-1)[0]), 0), n)
    xyz, rms, weight_sum = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    n_obs, n_kept, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    residual, kept = np.full((n_bank, k), -1.0), np.zeros((n_bank, k), np.int32)
    row_ok = np.isfinite(C).all(axis=1)
    zero = np.float64(0.0)
    with np.errstate(**_QUIET):
        for i in range(nt):
            obs = []
            for f, s in members(i, nxt, next_frame, root_frame, root_slot):
                g = np.float64(1.0) if g_bank is None else g_bank[f, s]
                if depth[f, s] > 0 and row_ok[f] and g > 0 and g - g == 0:
                    x, y = kp[f, s]
                    obs.append((f, s, g, x, y, world_point(x, y, depth[f, s], C[f], cam)))
            n_obs[i], status[i] = len(obs), 2
            if not obs:
                continue
            W0, S = zero, [zero, zero, zero]
            for _, _, g, _, _, Xw in obs:
                W0, S = W0 + g, [S[j] + g * Xw[j] for j in range(3)]
            L0 = [S[j] / W0 for j in range(3)]
            W, S, keep = zero, [zero, zero, zero], []
            for f, s, g, x, y, Xw in obs:
                if np.sqrt(score(C[f], cam, L0, x, y)) < thr:
                    W, S = W + g, [S[j] + g * Xw[j] for j in range(3)]
                    keep.append((f, s))
                    kept[f, s] = 1
            status[i] = 0 if len(keep) >= min_obs else 1
            L = [S[j] / W for j in range(3)] if status[i] == 0 else L0
            ss = zero
            for f, s, g, x, y, Xw in obs:
                sc = score(C[f], cam, L, x, y)
                residual[f, s] = np.sqrt(sc)
                if kept[f, s] == 1:
                    ss = ss + sc
            xyz[i], n_kept[i], weight_sum[i] = L, len(keep), W
            rms[i] = np.sqrt(ss / np.float64(len(keep))) if keep else zero
    return dict(xyz=xyz, n_obs=n_obs, n_kept=n_kept, status=status, weight_sum=weight_sum, rms=rms, residual=residual, kept=kept)


class TrackBank:
    """sslt_track_step's state and step in numpy: a bank of `capacity` frames of k slots.  step() takes one link row - the match list
    of (frame `first`, this frame) - and returns this frame's track_id, age (k,), n_new and status; after n steps the rows 0 .. n - 1
    of the state equal link_pairs + track_ids over the rows stepped so far."""

    def __init__(self, capacity: int, k: int):
        if capacity < 1 or not 1 <= k <= MAX_K or capacity * k > 0x7fffffff:
            raise ValueError(f"capacity >= 1, 1 <= k <= {MAX_K} and capacity * k <= 2^31 - 1 expected, got {capacity}, {k}")
        self.capacity, self.k = int(capacity), int(k)
        self.reset()

    def reset(self) -> None:
        c, k = self.capacity, self.k
        self.state = dict(t=np.zeros(1, np.int32), next_id=np.zeros(1, np.int32), prev=np.zeros((c, k), np.int32),
                          next=np.zeros((c, k), np.int32), prev_frame=np.zeros(c, np.int32), next_frame=np.zeros(c, np.int32),
                          track_id=np.zeros((c, k), np.int32), age=np.zeros((c, k), np.int32))

    def step(self, matches, count, mask=None, first: int = -1) -> dict:
        st, k = self.state, self.k
        t, id0 = int(st["t"][0]), int(st["next_id"][0])
        if not 0 <= t < self.capacity:
            return dict(track_id=np.full(k, -1, np.int32), age=np.full(k, -1, np.int32), n_new=np.zeros(1, np.int32),
                        status=np.array([COUNTER_OUT_OF_RANGE], np.int32))
        a = int(first)
        link_row = 0 <= a < t and st["next_frame"][a] == -1
        pv = np.full(k, -1, np.int32)
        if link_row:
            i1, i2 = link_slots(matches, count, mask, k)
            pv[i2] = i1
            st["next"][a, i1] = i2
            st["next_frame"][a] = t
        fresh = pv < 0
        ids, ages = np.zeros(k, np.int32), np.zeros(k, np.int32)
        ids[fresh] = id0 + np.cumsum(fresh)[fresh] - 1
        if link_row:
            ids[~fresh], ages[~fresh] = st["track_id"][a, pv[~fresh]], st["age"][a, pv[~fresh]] + 1
        n_new = int(fresh.sum())
        st["prev"][t], st["next"][t], st["track_id"][t], st["age"][t] = pv, -1, ids, ages
        st["prev_frame"][t], st["next_frame"][t] = (a if link_row else -1), -1
        st["t"][0], st["next_id"][0] = t + 1, id0 + n_new
        return dict(track_id=ids.copy(), age=ages.copy(), n_new=np.array([n_new], np.int32), status=np.zeros(1, np.int32))

    def tracks(self) -> dict:
        """The rows stepped so far as link_pairs' and track_ids' arrays (copies)."""
        n = int(self.state["t"][0])
        return {key: self.state[key][:n].copy() for key in LINK_KEYS + ("track_id", "age")}


def build_tracks(first, second, matches, count=None, mask=None, n_frames: int | None = None, k: int | None = None) -> dict:
    """Match lists to tracks in one call: link_pairs, then track_ids -> both dicts merged.  matches (P, n1, 2); count None: every
    slot of every row is listed; n_frames None: the largest `second` + 1; k None: the largest index + 1."""
    matches = np.asarray(matches, np.int64)
    first, second = np.asarray(first, np.int32).reshape(-1), np.asarray(second, np.int32).reshape(-1)
    if matches.ndim != 3 or matches.shape[2] != 2 or len(matches) != len(first) or len(first) != len(second) or not len(first):
        raise ValueError("first, second (P,) and matches (P, n1, 2) with P >= 1 expected")
    count = np.full(len(first), matches.shape[1], np.int32) if count is None else np.asarray(count, np.int32).reshape(-1)
    n_bank = int(second.max()) + 1 if n_frames is None else int(n_frames)
    k = max(int(matches.max()) + 1, 1) if k is None else int(k)
    if n_bank < 1 or not 1 <= k <= MAX_K or n_bank * k > 0x7fffffff or len(count) != len(first):
        raise ValueError(f"n_frames >= 1, 1 <= k <= {MAX_K}, n_frames * k <= 2^31 - 1 and count (P,) expected")
    links = link_pairs(first, second, matches, count, None if mask is None else np.asarray(mask, np.int32), n_bank, k)
    return {**links, **track_ids(links["prev"], links["prev_frame"])}


def track_landmarks(keypoints, kp_depth, C, tracks: dict, camera, threshold: float = 3.0, min_obs: int = 2, weights=None,
                    scale_x: float = 1.0, scale_y: float = 1.0) -> dict:
    """The map points of build_tracks' tracks under the world -> camera poses C (n, 12) or (n, 3, 4): landmarks() with its refusals."""
    if min_obs < 2 or not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("min_obs >= 2 and a finite threshold >= 0 expected")
    return landmarks(keypoints, kp_depth, C, camera, tracks["next"], tracks["next_frame"], tracks["root_frame"], tracks["root_slot"],
                     tracks["n_tracks"], weights, threshold, min_obs, scale_x, scale_y)


def length_statistics(length, n_tracks) -> dict:
    """Track length as a figure of merit: mean, median, max, the share of tracks with length >= 2, and a histogram (entry l the
    number of tracks of length l)."""
    n = int(np.asarray(n_tracks).reshape(-1)[0])
    ln = np.asarray(length)[:n].astype(np.int64)
    if n == 0:
        return dict(n_tracks=0, mean=0.0, median=0.0, max=0, share_ge_2=0.0, histogram=np.zeros(1, np.int64))
    return dict(n_tracks=n, mean=float(ln.mean()), median=float(np.median(ln)), max=int(ln.max()), share_ge_2=float((ln >= 2).mean()),
                histogram=np.bincount(ln))
