"""A0 (both output forms) and A9 in their reworked kernels (batched row loads and non-temporal stores in A0, the tiled kernel's
idiom in A9), bit for bit against the CPU oracle's A0 and A9 (`ora.resize_rgb`, `ora.intensity`: what
`oracle_check.oracle_block(with_a0=True)` calls).

A0: 48 x 64 -> 32 (one tile, partial in x), 100 x 150 -> 80 (a full and a partial tile in x), 480 x 640 -> 448 with 2 frames (the
bench's class), a vertical upscale and a size with seven vertical taps; 1, 8 and 9 frames (the grid deals frames to XCDs in
eights); an output base that is 4- but not 16-byte aligned inside a poisoned buffer, next to the 16-byte aligned one; a `size`
that is no multiple of 4 - `sslam_preprocess_u8` accepts any positive size, so that case runs (the patch entry needs
size % 16 == 0 and has no such case); an identity resize whose pixels take every byte value in every channel (the whole
normalisation table).  A9: the image corners, half-integer coordinates (rint is half-to-even), coordinates outside the image on
both sides, K = 1 and K = 65 over 3 frames."""
import numpy as np
import pytest

from oracle import ora

pytestmark = pytest.mark.gpu

# h, w, size, frames; bilinear, five taps both ways unless noted.  64 -> 80 rows is a vertical upscale (3 taps), 200 -> 64 rows
# uses 7 of 9 vertical taps (and 16-row tiles)
SHAPES = [(48, 64, 32, 1), (100, 150, 80, 1), (480, 640, 448, 2), (64, 150, 80, 1), (200, 150, 64, 1)]
_cases = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def hip():
    from sslam_amd import lib
    return lib


def _images(h, w, n):
    return np.random.default_rng(h * 7919 + w * 13 + n).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _case(h, w, size, n, imgs=None):
    """Images and the oracle's planar fp32 result, computed once per shape; no test writes to them."""
    key = (h, w, size, n, imgs is None)
    if key not in _cases:
        im = _images(h, w, n) if imgs is None else imgs
        chw = np.stack([ora.resize_rgb(im[i], size)[1] for i in range(n)])
        _cases[key] = (im, chw)
    return _cases[key]


def _tables(T, hip, h, w, size, bicubic=False):
    tabs = []
    for n_in in (w, h):
        b, c, k = hip.resample_table(n_in, size, bicubic)
        tabs.append((T.from_numpy(b).cuda(), T.from_numpy(c).cuda(), k))
    return tabs


def _patch_rows(T, chw, size):
    n, g = chw.shape[0], size // 16
    rows = chw.reshape(n, 3, g, 16, g, 16).transpose(0, 2, 4, 1, 3, 5).reshape(n, g * g, 768)
    return T.from_numpy(np.ascontiguousarray(rows)).to(T.bfloat16).view(T.int16)          # one rounding to nearest even


def _bits(T, got, want):
    assert T.equal(got.cpu().contiguous().view(T.int32), T.from_numpy(np.ascontiguousarray(want)).view(T.int32))


@pytest.mark.parametrize("h,w,size,n", SHAPES)
def test_a0_fp32_image_sizes(T, hip, h, w, size, n):
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    _bits(T, hip.preprocess_u8(T.from_numpy(imgs).cuda(), size, th, tv), chw)


@pytest.mark.parametrize("h,w,size,n", SHAPES)
def test_a0_patch_image_sizes(T, hip, h, w, size, n):
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    got = hip.preprocess_u8_patches(T.from_numpy(imgs).cuda(), size, th, tv)
    assert got is not None
    assert T.equal(got.cpu().view(T.int16), _patch_rows(T, chw, size))


@pytest.mark.parametrize("n", [1, 8, 9])
def test_a0_frame_counts(T, hip, n):
    h, w, size = 48, 64, 32
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    x = T.from_numpy(imgs).cuda()
    _bits(T, hip.preprocess_u8(x, size, th, tv), chw)
    assert T.equal(hip.preprocess_u8_patches(x, size, th, tv).cpu().view(T.int16), _patch_rows(T, chw, size))


@pytest.mark.parametrize("h,w,size,n", SHAPES[:2])
@pytest.mark.parametrize("lead", [1, 2, 3, 4])
def test_a0_fp32_output_placement(T, hip, h, w, size, n, lead):
    """The output starts `lead` floats into a 256-byte aligned buffer: 4-byte aligned always, 16-byte aligned only at lead 4.
    The floats before and after the region keep their poison."""
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    count, poison = n * 3 * size * size, -(2.0 ** 100)
    buf = T.full((lead + count + 4,), poison, dtype=T.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    out = buf[lead:lead + count].view(n, 3, size, size)
    assert out.data_ptr() % 4 == 0 and (out.data_ptr() % 16 == 0) == (lead == 4)
    hip.preprocess_u8(T.from_numpy(imgs).cuda(), size, th, tv, out=out)
    _bits(T, out, chw)
    assert bool((buf[:lead] == poison).all()) and bool((buf[lead + count:] == poison).all())


@pytest.mark.parametrize("lead", [1, 2, 4])
def test_a0_patch_output_placement(T, hip, lead):
    """bf16 patch rows `lead` halves into an aligned buffer: 2-, 4- and 8-byte aligned bases (8-byte stores only at the last)."""
    h, w, size, n = SHAPES[0]
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    count = n * 3 * size * size
    buf = T.full((lead + count + 8,), -(2.0 ** 100), dtype=T.bfloat16, device="cuda")
    poison = buf[:1].clone().view(T.int16)
    out = buf[lead:lead + count].view(n, (size // 16) ** 2, 768)
    assert (out.data_ptr() % 8 == 0) == (lead == 4)
    assert hip.preprocess_u8_patches(T.from_numpy(imgs).cuda(), size, th, tv, out=out) is not None
    assert T.equal(out.cpu().view(T.int16), _patch_rows(T, chw, size))
    assert bool((buf[:lead].view(T.int16) == poison).all()) and bool((buf[lead + count:].view(T.int16) == poison).all())


@pytest.mark.parametrize("h,size", [(48, 30), (100, 50), (100, 66)])
def test_a0_general_entry_size_not_a_multiple_of_four(T, hip, h, size):
    """sslam_preprocess_u8 takes any positive size: rows of `size` floats are then only 4-byte aligned (30: 11 horizontal taps, the
    general kernel; 50 and 66: the tiled kernel, 66 with a second, partial tile)."""
    w, n = 150, 2
    imgs, chw = _case(h, w, size, n)
    th, tv = _tables(T, hip, h, w, size)
    count, poison = n * 3 * size * size, -(2.0 ** 100)
    buf = T.full((count + 4,), poison, dtype=T.float32, device="cuda")
    out = buf[:count].view(n, 3, size, size)
    hip.preprocess_u8(T.from_numpy(imgs).cuda(), size, th, tv, out=out)
    _bits(T, out, chw)
    assert bool((buf[count:] == poison).all())


def test_a0_every_byte_value_in_every_channel(T, hip):
    """An identity resize (32 x 32 -> 32: the centre tap is 1) of pixels that take every byte value in every channel: every entry
    of the normalisation table, as the fp32 image and as bf16 patch rows."""
    size = 32
    v = np.arange(size * size, dtype=np.int64)
    img = np.stack([v % 256, (v * 7 + 3) % 256, 255 - v % 256], -1).astype(np.uint8).reshape(1, size, size, 3)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    imgs, chw = _case(size, size, size, 1, imgs=img)
    mean, sd = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    want = ((imgs[0].astype(np.float32) / np.float32(255.0) - mean) / sd).transpose(2, 0, 1)
    assert np.array_equal(want.view(np.uint32), chw[0].view(np.uint32))                    # the oracle resized nothing
    th, tv = _tables(T, hip, size, size, size)
    x = T.from_numpy(imgs).cuda()
    _bits(T, hip.preprocess_u8(x, size, th, tv), chw)
    assert T.equal(hip.preprocess_u8_patches(x, size, th, tv).cpu().view(T.int16), _patch_rows(T, chw, size))


def _keypoints(size, n, K):
    """Corners, half-integers (to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2), outside on both sides; random ones fill the rest."""
    s = float(size)
    special = np.float32([[0, 0], [s - 1, s - 1], [0.5, 1.5], [2.5, 3.5], [s - 1.5, s - 0.5], [-3.25, -0.5], [s + 4.75, s - 0.5],
                          [-1e6, 5], [7, 1e6], [s - 1, 0], [0, s - 1]])
    rng = np.random.default_rng(size * 31 + K)
    kp = (rng.random((n, K, 2)) * (size + 8) - 4).astype(np.float32)
    for f in range(n):
        for j in range(min(K, len(special))):
            kp[f, j] = special[(j + f * 3) % len(special)]                                # K = 1: a different special point per frame
    return kp


# A9 resamples with Pillow's default filter, bicubic (as the pipeline's tables for it are): the issue's three image sizes - 9 / 9 / 7
# horizontal taps, so the first two run the general kernel and the third the tiled one at 7 x 7 taps - and two sizes in its other
# tap classes (an upscale both ways: 5 x 5; an upscale of the rows only: 7 x 5)
A9_SHAPES = [s[:3] for s in SHAPES[:3]] + [(64, 64, 80), (60, 100, 80)]


@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("h,w,size", A9_SHAPES)
def test_a9_coordinates(T, hip, h, w, size, K):
    n = 3
    imgs = _images(h, w, n)
    kp = _keypoints(size, n, K)
    want = np.stack([ora.intensity(imgs[i], size, kp[i]) for i in range(n)])
    th, tv = _tables(T, hip, h, w, size, bicubic=True)
    buf = T.full((n * K + 2,), -(2.0 ** 100), dtype=T.float32, device="cuda")
    out = buf[1:1 + n * K].view(n, K)
    hip.keypoint_intensity(T.from_numpy(imgs).cuda(), size, th, tv, T.from_numpy(kp).cuda(), out=out)
    _bits(T, out, want)
    assert float(buf[0]) == -(2.0 ** 100) and float(buf[-1]) == -(2.0 ** 100)
