"""The two CPU studies of sub-cell localisation that tests/test_subcell_cpu.py asserts on and DESIGN.md §4j records: planted Gaussian
bumps located by the restatement (tests/subcell_ref.py), and relative poses estimated from cell-centre and from refined keypoints
by the restatements of the pose stages (tests/pose_ransac_ref.py, tests/pose_refine_ref.py).  numpy and the CPU oracle only.
"""
import numpy as np

import pose_ransac_ref as rr
import pose_refine_ref as fr
import subcell_ref as ref
from pose_depth_ref import Cam

F = np.float32


def bump_errors(sigma=1.0, draws=2000, g=15, seed=0, noise=0.0):
    """Planted bumps base + amp exp(-r^2 / 2 sigma^2) on a g x g grid, the peak uniform within the centre cell: the error in
    cells of the grid (the cell itself) and of the restatement -> dict(grid_rms, rms, max) over `draws` seeded draws."""
    rng = np.random.default_rng(seed)
    c = g // 2
    err, grid = np.empty(draws), np.empty(draws)
    for i in range(draws):
        px, py = c + rng.uniform(-0.5, 0.5), c + rng.uniform(-0.5, 0.5)
        field = ref.bump_field(g, px, py, sigma)
        if noise:
            field = (field + rng.normal(0.0, noise, field.shape)).astype(F)
        cell = int(np.argmax(field))
        xy, _, _ = ref.subcell_keypoints(field[None], np.array([[cell]], np.int32))
        err[i] = np.hypot(float(xy[0, 0, 0]) - px, float(xy[0, 0, 1]) - py)
        grid[i] = np.hypot(cell % g - px, cell // g - py)
    return dict(grid_rms=float(np.sqrt(np.mean(grid ** 2))), rms=float(np.sqrt(np.mean(err ** 2))), max=float(err.max()))


G, SIZE, LATTICE = 28, 448, 6            # the shipped grid; a 6 x 6 lattice of planted points, 4 cells apart


def _frame(points_px):
    """Saliency (G, G) fp32 of sigma = 1 cell bumps at the pixel positions (n, 2), pixel = 16 * cell + 8."""
    yy, xx = np.mgrid[0:G, 0:G].astype(np.float64)
    f = np.full((G, G), 0.1)
    for u, v in (points_px - 8.0) / 16.0:
        f += 0.8 * np.exp(-((xx - u) ** 2 + (yy - v) ** 2) / 2.0)
    return f.astype(F)


def _identity(kp_cells, points_px):
    """For each selected cell (K, 2) the planted point whose bump it is the peak of (within 0.75 cells), else -1."""
    pos = (points_px - 8.0) / 16.0
    d = np.linalg.norm(kp_cells[:, None, :].astype(np.float64) - pos[None], axis=2)
    j = d.argmin(axis=1)
    return np.where(d[np.arange(len(j)), j] <= 0.75, j, -1)


def pose_pair(seed, threshold=8.0, n_hyp=128, n_iter=5):
    """One planted pair: LATTICE^2 3-D points seen by two cameras a small rigid motion apart, each frame's saliency rendered as
    bumps at the points' projections, keypoints selected by the oracle, matches by planted identity, depths the planted ones;
    RANSAC + refinement once on the cell centres and once on the refined keypoints.
    -> dict(cell=(rot deg, trans m), sub=(rot deg, trans m), matches=int)."""
    from oracle import ora
    from pose_depth_ref import rigid, rotation
    rng = np.random.default_rng(1000 + seed)
    cam, sx, sy = Cam(), 640.0 / SIZE, 480.0 / SIZE
    n = LATTICE * LATTICE
    lat = 4.0 * np.arange(LATTICE) + 4.0
    cells = np.stack(np.meshgrid(lat, lat), axis=-1).reshape(n, 2) + rng.uniform(-0.5, 0.5, (n, 2))
    pa = 16.0 * cells + 8.0                                          # frame a, keypoint units (pixels of the 448 input)
    z = rng.uniform(1.5, 4.0, n)
    da = np.round(z * cam.depth_scale).astype(np.int32)
    Xa = rr.back_project(pa.astype(F), da, cam, sx, sy)
    axis = rng.normal(size=3)
    T = rigid(rotation(axis / np.linalg.norm(axis), np.radians(rng.uniform(0.5, 2.0))), rng.uniform(-0.05, 0.05, 3))
    T = np.asarray(T, np.float64).reshape(-1)[:12]
    Xb = Xa @ T.reshape(3, 4)[:, :3].T + T.reshape(3, 4)[:, 3]
    pb = np.stack([(cam.fx * Xb[:, 0] / Xb[:, 2] + cam.cx) / sx, (cam.fy * Xb[:, 1] / Xb[:, 2] + cam.cy) / sy], axis=1)
    db = np.round(Xb[:, 2] * cam.depth_scale).astype(np.int32)
    sal = np.stack([_frame(pa), _frame(pb)])
    kp, _, idx, _ = ora.select_keypoints(sal, n, 2, 0.5)
    ids = [_identity(kp[f], p) for f, p in ((0, pa), (1, pb))]
    where_b = {int(j): r for r, j in enumerate(ids[1]) if j >= 0}
    rows = [(r, where_b[int(j)]) for r, j in enumerate(ids[0]) if j >= 0 and int(j) in where_b]
    matches = np.zeros((n, 2), np.int64)
    matches[:len(rows)] = rows
    depth = [np.where(ids[0] >= 0, da[np.maximum(ids[0], 0)], 0).astype(np.int32),
             np.where(ids[1] >= 0, db[np.maximum(ids[1], 0)], 0).astype(np.int32)]
    out = dict(matches=len(rows))
    for name, bank in (("cell", ora.patch_to_pixel(kp)), ("sub", ref.subcell_keypoints(sal, idx)[1])):
        est = rr.ransac(bank[0], bank[1], depth[0], depth[1], matches, len(rows), cam, threshold, n_hyp, seed, sx, sy)
        fin = fr.refine(bank[0], bank[1], depth[0], depth[1], matches, len(rows), cam, threshold, threshold / 3.0, n_iter, est["T"], sx, sy)
        out[name] = rr.pose_error(fin["T"], T)
    return out


def pose_study(pairs=40):
    """-> dict(cell_median, sub_median: translation error in metres; cell_rot_median, sub_rot_median: degrees; share: the share of
    pairs whose refined-keypoint translation error is the smaller; ratio_median: the median of sub / cell translation error)."""
    runs = [pose_pair(s) for s in range(pairs)]
    ct, st = np.array([r["cell"][1] for r in runs]), np.array([r["sub"][1] for r in runs])
    cr, sr = np.array([r["cell"][0] for r in runs]), np.array([r["sub"][0] for r in runs])
    return dict(cell_median=float(np.median(ct)), sub_median=float(np.median(st)), cell_rot_median=float(np.median(cr)),
                sub_rot_median=float(np.median(sr)), share=float(np.mean(st < ct)), ratio_median=float(np.median(st / ct)),
                matches_min=int(min(r["matches"] for r in runs)))
