"""The restatement libsslam_track.so is held to bit for bit (tests/test_gpu_tracks.py), written from the contract in
include/sslam_track.h.  link_pairs and track_ids are written here a second time, by the header's METHOD - per-frame lowest rows,
per-index lowest slots, pointer jumping in ceil(log2 n_bank) rounds over (root, distance) pairs, the tiled exclusive scan - beside
the vectorised forms of sslam_amd/track_numpy.py; tests/test_tracks_cpu.py holds the two to each other and both to brute_force():
union-find over the link set with ids assigned by sorting the roots.  landmarks and the online bank are track_numpy's, whose float64
arithmetic is scalar and in the header's order already; plain_landmarks() is an INDEPENDENT evaluation (matrix products, np.sum) for
a tolerance check.

Tolerance against the device: NONE - integers, and float64 + - * / sqrt rounded once in one order on both sides.
"""
from __future__ import annotations

import numpy as np

from sslam_amd import track_numpy as tn
from sslam_amd.track_numpy import (BANK_OUT_KEYS, BANK_STATE_KEYS, LANDMARK_KEYS, LINK_KEYS, TRACK_KEYS, TrackBank, landmarks,  # noqa: F401
                                   members)

NONE = 0x7fffffff
SCAN_TILE = 1024


def link_pairs(first, second, matches, count, mask, n_bank, k):
    """sslt_link_pairs by its five launches."""
    P, n1 = len(first), matches.shape[1]
    prev, nxt = np.full((n_bank, k), -1, np.int32), np.full((n_bank, k), -1, np.int32)
    prev_frame, next_frame = np.full(n_bank, NONE, np.int64), np.full(n_bank, NONE, np.int64)
    valid = lambda p: 0 <= first[p] < second[p] < n_bank
    for p in range(P):                                               # (b)
        if valid(p):
            prev_frame[second[p]] = min(prev_frame[second[p]], p)
            next_frame[first[p]] = min(next_frame[first[p]], p)
    for p in range(P):                                               # (c)
        if not valid(p) or prev_frame[second[p]] != p or next_frame[first[p]] != p:
            continue
        a, b = int(first[p]), int(second[p])
        cnt = min(max(int(count[p]), 0), n1)
        ok = lambda j: 0 <= matches[p, j, 0] < k and 0 <= matches[p, j, 1] < k and (mask is None or mask[p, j] == 1)
        lo1, lo2 = {}, {}
        for j in range(cnt):
            if ok(j):
                lo1.setdefault(int(matches[p, j, 0]), j), lo2.setdefault(int(matches[p, j, 1]), j)
        for j in range(cnt):
            if ok(j) and lo1[int(matches[p, j, 0])] == j and lo2[int(matches[p, j, 1])] == j:
                nxt[a, matches[p, j, 0]], prev[b, matches[p, j, 1]] = matches[p, j, 1], matches[p, j, 0]
    pf = np.full(n_bank, -1, np.int32)                               # (d)
    for f in range(n_bank):
        r = prev_frame[f]
        if r != NONE and next_frame[first[r]] == r:
            pf[f] = first[r]
    nf = np.full(n_bank, -1, np.int32)                               # (e)
    for f in range(n_bank):
        r = next_frame[f]
        if r != NONE and pf[second[r]] == f:
            nf[f] = second[r]
    return dict(prev=prev, next=nxt, prev_frame=pf, next_frame=nf)


def track_ids(prev, prev_frame):
    """sslt_track_ids by its method: pointer jumping, then the tiled scan."""
    n_bank, k = prev.shape
    n = n_bank * k
    root, dist = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
    for f in range(n_bank):
        pf = int(prev_frame[f])
        if 0 <= pf < f:
            has = (prev[f] >= 0) & (prev[f] < k)
            root[f * k:(f + 1) * k][has], dist[f * k:(f + 1) * k][has] = pf * k + prev[f][has], 1
    reach = 1
    while reach < n_bank:                                            # ceil(log2 n_bank) rounds, double buffered
        root, dist = root[root], dist + dist[root]
        reach *= 2
    flag = root == np.arange(n)
    tiles = [int(flag[i:i + SCAN_TILE].sum()) for i in range(0, n, SCAN_TILE)]
    offset = np.concatenate([[0], np.cumsum(tiles)]).astype(np.int64)
    id_of = np.full(n, -1, np.int64)
    for ti, i in enumerate(range(0, n, SCAN_TILE)):
        local = flag[i:i + SCAN_TILE]
        id_of[i:i + SCAN_TILE][local] = offset[ti] + np.cumsum(local)[local] - 1
    n_tracks = int(offset[-1])
    root_frame, root_slot, length = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    roots = np.flatnonzero(flag)
    root_frame[id_of[roots]], root_slot[id_of[roots]] = roots // k, roots % k
    track_id = id_of[root].astype(np.int32)
    np.add.at(length, track_id, 1)
    return dict(track_id=track_id.reshape(n_bank, k), age=dist.astype(np.int32).reshape(n_bank, k), n_tracks=np.array([n_tracks], np.int32),
                root_frame=root_frame, root_slot=root_slot, length=length)


def brute_force(first, second, matches, count, mask, n_bank, k):
    """The DEFINITION, no method: the link set by exhaustive comparison of rows and of slots, union-find over it, ids by sorting the
    roots' (frame, slot).  -> (links as a set of ((a, i1), (b, i2)), track_id (n_bank, k), age, lengths per id)."""
    P, n1 = len(first), matches.shape[1]
    valid_row = [bool(0 <= first[p] < second[p] < n_bank) for p in range(P)]
    links = set()
    for p in range(P):
        if not valid_row[p] or any(valid_row[q] and (second[q] == second[p] or first[q] == first[p]) for q in range(p)):
            continue
        cnt = min(max(int(count[p]), 0), n1)
        ok = [bool(0 <= matches[p, j, 0] < k and 0 <= matches[p, j, 1] < k and (mask is None or mask[p, j] == 1)) for j in range(cnt)]
        for j in range(cnt):
            if ok[j] and not any(ok[q] and (matches[p, q, 0] == matches[p, j, 0] or matches[p, q, 1] == matches[p, j, 1]) for q in range(j)):
                links.add(((int(first[p]), int(matches[p, j, 0])), (int(second[p]), int(matches[p, j, 1]))))
    parent = {(f, s): (f, s) for f in range(n_bank) for s in range(k)}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for u, v in links:
        ru, rv = find(u), find(v)
        parent[max(ru, rv)] = min(ru, rv)                            # the earliest (frame, slot) stays the representative
    reps = sorted({find(x) for x in parent})
    number = {r: i for i, r in enumerate(reps)}
    track_id = np.array([[number[find((f, s))] for s in range(k)] for f in range(n_bank)], np.int32)
    pred = {v: u for u, v in links}
    age = np.zeros((n_bank, k), np.int32)
    for f in range(n_bank):
        for s in range(k):
            x, a = (f, s), 0
            while x in pred:
                x, a = pred[x], a + 1
            age[f, s] = a
    return links, track_id, age, np.bincount(track_id.reshape(-1), minlength=len(reps)).astype(np.int32)


def link_set(links: dict) -> set:
    """link_pairs' arrays as brute_force's set, checking that prev and next say the same."""
    nxt, prev, nf, pf = links["next"], links["prev"], links["next_frame"], links["prev_frame"]
    fwd = {((a, i1), (int(nf[a]), int(nxt[a, i1]))) for a in range(len(nf)) for i1 in range(nxt.shape[1]) if nxt[a, i1] >= 0}
    back = {((int(pf[b]), int(prev[b, i2])), (b, i2)) for b in range(len(pf)) for i2 in range(prev.shape[1]) if prev[b, i2] >= 0}
    assert fwd == back, "prev and next disagree"
    return fwd


def plain_landmarks(kp_bank, kp_depth_bank, C, camera, tracks, weight=None, threshold=3.0, min_obs=2):
    """An independent evaluation of xyz, n_kept and status per track: matrix products and np.sum, scale 1."""
    n_bank, k = kp_depth_bank.shape
    C = np.asarray(C, np.float64).reshape(n_bank, 3, 4)
    Kinv = lambda x, y, z: np.array([(x - camera.cx) * z / camera.fx, (y - camera.cy) * z / camera.fy, z])
    nt = int(tracks["n_tracks"][0])
    xyz, n_kept, status = np.zeros((nt, 3)), np.zeros(nt, np.int32), np.zeros(nt, np.int32)
    for i in range(nt):
        pts, ws, px = [], [], []
        for f, s in members(i, tracks["next"], tracks["next_frame"], tracks["root_frame"], tracks["root_slot"]):
            g = 1.0 if weight is None else float(weight[f, s])
            if kp_depth_bank[f, s] > 0 and np.isfinite(C[f]).all() and np.isfinite(g) and g > 0:
                Xc = Kinv(float(kp_bank[f, s, 0]), float(kp_bank[f, s, 1]), kp_depth_bank[f, s] / camera.depth_scale)
                pts.append(C[f, :, :3].T @ (Xc - C[f, :, 3])), ws.append(g), px.append((f, kp_bank[f, s].astype(np.float64)))
        if not pts:
            status[i] = 2
            continue
        pts, ws = np.array(pts), np.array(ws)
        L0 = (ws[:, None] * pts).sum(0) / ws.sum()
        keep = []
        for (f, xy) in px:
            q = C[f, :, :3] @ L0 + C[f, :, 3]
            uv = np.array([camera.fx * q[0] / q[2] + camera.cx, camera.fy * q[1] / q[2] + camera.cy])
            keep.append(bool(q[2] > 0 and np.linalg.norm(uv - xy) < threshold))
        keep = np.array(keep)
        n_kept[i] = keep.sum()
        status[i] = 0 if n_kept[i] >= min_obs else 1
        xyz[i] = (ws[keep, None] * pts[keep]).sum(0) / ws[keep].sum() if status[i] == 0 else L0
    return xyz, n_kept, status
