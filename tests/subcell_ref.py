"""sslx_subcell_keypoints (include/sslam_ext.h) restated in numpy float32, operation by operation in the header's order: the CPU
tests hold it to the float64 parabola, the GPU tests hold the kernel to it bit for bit.  No torch, no GPU: importable anywhere.
"""
import numpy as np

FLAG_X, FLAG_Y, FLAG_RANGE = 1, 2, 4
F = np.float32


def axis_offset(c, m, p, border):
    """One axis, arrays of fp32 (c the cell, m the lower, p the upper neighbour; border: bool array) -> (off fp32, refined bool).
    Every operation on float32 arrays, so each is rounded to fp32 once, as the kernel's."""
    c, m, p = (np.asarray(v, F) for v in (c, m, p))
    with np.errstate(all="ignore"):
        a = c - m
        b = c - p
        is_max = (a >= F(0)) & (b >= F(0))                 # a NaN fails
        den = a + b
        positive = den > F(0)                              # a NaN fails
        off = (a - b) / (den + den)
        inside = (off >= F(-0.5)) & (off <= F(0.5))        # catches the NaN of infinite inputs
    refined = ~np.asarray(border, bool) & is_max & positive & inside
    return np.where(refined, off, F(0.0)).astype(F), refined


def subcell_keypoints(sal, idx):
    """sal (n, G, G) fp32, idx (n, K) int32 -> (kp_xy_sub (n, K, 2) fp32, kp_pixel_sub (n, K, 2) fp32, flags (n, K) int32)."""
    sal = np.ascontiguousarray(sal, F)
    idx = np.ascontiguousarray(idx, np.int32)
    n, g = sal.shape[0], sal.shape[1]
    assert sal.shape == (n, g, g) and idx.shape[0] == n
    cells = g * g
    in_range = (idx >= 0) & (idx < cells)
    cell = np.where(in_range, idx, 0).astype(np.int64)
    y, x = cell // g, cell % g
    bx, by = (x == 0) | (x == g - 1), (y == 0) | (y == g - 1)
    flat = sal.reshape(n, cells)
    take = lambda c: np.take_along_axis(flat, c, axis=1)
    c = take(cell)
    # a border axis has no neighbour on one side: its offset is +0.0 whatever is passed, the cell itself here
    ox, rx = axis_offset(c, take(np.where(bx, cell, cell - 1)), take(np.where(bx, cell, cell + 1)), bx)
    oy, ry = axis_offset(c, take(np.where(by, cell, cell - g)), take(np.where(by, cell, cell + g)), by)
    xy = np.stack([x.astype(F) + ox, y.astype(F) + oy], axis=-1).astype(F)
    xy[~in_range] = F(0.0)
    px = (xy * F(16.0)).astype(F) + F(8.0)
    flags = np.where(in_range, rx * FLAG_X + ry * FLAG_Y, FLAG_RANGE).astype(np.int32)
    return xy, px.astype(F), flags


def parabola_vertex64(c, m, p):
    """The vertex of the float64 parabola through (-1, m), (0, c), (1, p): (p - m) / (2 (2c - m - p))."""
    c, m, p = (np.asarray(v, np.float64) for v in (c, m, p))
    return (p - m) / (2.0 * (2.0 * c - m - p))


def bump_field(g, cx, cy, sigma, base=0.1, amp=0.8):
    """The planted field of the CPU study: base + amp * exp(-r^2 / (2 sigma^2)) around (cx, cy), in cells, float64 -> fp32 (g, g)."""
    yy, xx = np.mgrid[0:g, 0:g].astype(np.float64)
    return (base + amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma ** 2))).astype(F)
