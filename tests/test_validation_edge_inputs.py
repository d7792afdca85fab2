"""CPU tests of tests/val_edge_cases.py: the inputs of tests/test_gpu_validation_edges.py have the properties those tests rely on.
Numpy and the CPU oracle only."""
import numpy as np
import pytest

import val_edge_cases as vec
import val_ref
from oracle import ora


def test_sizes_cover_the_segment_shapes():
    assert vec.seams(512) == [] and vec.seams(544) == [512] and vec.seams(1024) == [512] and vec.seams(1040) == [512, 1024]
    widths = {s: [min(vec.SEG, s - c0) for c0 in range(0, s, vec.SEG)] for s in vec.SIZES}
    assert widths == {512: [512], 544: [512, 32], 1024: [512, 512], 1040: [512, 512, 16]}
    assert {s for s, n in vec.SIZES_FRAMES if n == 2} == {544, 1040} and {s for s, _ in vec.SIZES_FRAMES} == set(vec.SIZES)


@pytest.mark.parametrize("size", vec.SIZES)
def test_seam_images_are_zero_away_from_the_seams(size):
    img = vec.image("seams", size, 0)
    keep = np.zeros(size, bool)
    for c0 in vec.seams(size):
        keep[c0 - 2:c0 + 2] = True
        cols = img[:, 2:-2, c0 - 2:c0 + 2]
        assert (cols != 0).all() and not np.array_equal(cols[..., 1], cols[..., 2]), "both sides of the seam hold their own values"
        # a halo read as zero moves EVERY cell along the seam by several tolerances, and most by hundreds of them
        zeroed = img.copy()
        zeroed[:, :, c0 - 1] = 0.0
        gray = 8.0 * np.abs(0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2]).max()
        d = np.abs(val_ref.sobel_pool(img)[0] - val_ref.sobel_pool(zeroed)[0])[:, c0 // 16]
        tol = val_ref.tolerance(0.0, scale=gray)
        assert (d > 4 * tol).all() and np.median(d) > 100 * tol, (size, c0, float(d.min()), float(np.median(d)))
    assert not img[:, 2:-2, ~keep].any()
    assert (img[:, :2] != 0).all() and (img[:, -2:] != 0).all()
    assert not np.array_equal(vec.image("seams", size, 0), vec.image("seams", size, 1))


@pytest.mark.parametrize("size", vec.SIZES)
def test_peak_sits_in_the_right_segment_of_the_right_frame(size):
    last = (size - 1) // vec.SEG
    for frame in (0, 1):
        mag = val_ref.sobel_magnitude(vec.image("peak_last", size, frame))
        y, x = np.unravel_index(mag.argmax(), mag.shape)
        py, px = vec.peak_position(size, frame)
        assert abs(int(y) - py) <= 1 and abs(int(x) - px) <= 1
        assert x // vec.SEG == (last if frame == 0 else 0)
        # every other segment's own maximum is far below: a maximum taken from another segment or frame cannot pass
        for seg in range(last + 1):
            if seg != x // vec.SEG:
                assert mag[:, seg * vec.SEG:(seg + 1) * vec.SEG].max() < 0.25 * mag.max()
    # a frame of its own seed is the same array in a batch of one and of two
    assert np.array_equal(vec.images("peak_last", size, 2)[0], vec.images("peak_last", size, 1)[0])


@pytest.mark.parametrize("size", vec.SIZES)
def test_position_check_reaches_both_sides_of_every_seam(size):
    """Index arithmetic alone: the compared neighbourhoods hold the same real pixels, and for every seam a compared cell lies
    directly left of it and one directly right."""
    a, b, c = vec.shifted_images(size)
    for_b, for_c = vec.shift_cells(size)
    g = size // 16
    assert for_b == list(range(1, g - 2)) and for_c == list(range(2, g - 1))
    for gx in (for_b[0], for_b[-1]):
        assert np.array_equal(a[:, :, 16 * gx - 1:16 * gx + 17], b[:, :, 16 * gx + 15:16 * gx + 33])
    for gx in (for_c[0], for_c[-1]):
        assert np.array_equal(a[:, :, 16 * gx - 1:16 * gx + 17], c[:, :, 16 * gx - 17:16 * gx + 1])
    assert not np.array_equal(a[:, :, :16], b[:, :, :16]) and not np.array_equal(a[:, :, -16:], c[:, :, -16:])
    cells = vec.compared_cells(size)
    for c0 in vec.seams(size):
        left, right = c0 // 16 - 1, c0 // 16
        assert any(left in cells[k] for k in "ABC"), (size, c0, "left")
        assert any(right in cells[k] for k in "ABC"), (size, c0, "right")
    # the cell right of the seam at 1024 of size 1040 is the image's last: zero padding on its right, which no moved image
    # has anywhere else - it is reached through the crop
    cc = vec.crop_cells(size)
    if size == 1040:
        assert not any(64 in cells[k] for k in "BC") and cc == (64, 33, 33)
        crop = a[:, :vec.CROP, -vec.CROP:]
        assert np.array_equal(crop[:, :, -17:], a[:, :vec.CROP, -17:]) and crop.shape == (3, 544, 544)
    if size == 1024:
        assert cc == (63, 33, 33)      # an interior cell of the crop's second segment against the last cell of a full one


def _f32_sims(d1, d2):
    return ora.sim_matrix(d1, d2)


def test_cluster_similarities():
    a, b, c = vec.cluster(129, +1, 1), vec.cluster(65, +1, 2), vec.cluster(65, -1, 3)
    assert np.allclose(np.linalg.norm(a.astype(np.float64), axis=1), 1.0, atol=1e-6)
    same, opposite = val_ref.sims(a, b), val_ref.sims(a, c)
    print(f"same-sign similarities in [{same.min():.3f}, {same.max():.3f}], opposite-sign in [{opposite.min():.3f}, {opposite.max():.3f}]")
    assert same.min() > 0.8 and opposite.max() < -0.8


@pytest.mark.parametrize("name", vec.CLAMPED)
def test_fully_clamped_cases(name):
    """Every |s| >= 0.6 in float64 and in the fp32 similarity matrix: at T = 0.01 every logit is exactly +-50 with a margin no
    rounding crosses, and the float64 reference is the closed form."""
    first, second, n_high = vec.clamped_case(name)
    assert first.shape == (vec.CLAMP_N1, 128) and second.shape == (vec.CLAMP_N2, 128)
    s64, s32 = val_ref.sims(first, second), _f32_sims(first, second)
    assert (np.abs(s64) >= 0.6).all() and (np.abs(s32) >= 0.6).all()
    assert np.array_equal(np.sign(s64), np.sign(s32)) and ((s64 > 0).sum(axis=1) == n_high).all()
    x = val_ref.logits(first, second, vec.CLAMP_T)
    assert set(np.unique(x)) <= {-50.0, 50.0}
    x32 = np.clip(s32 / np.float32(vec.CLAMP_T), np.float32(-50), np.float32(50))
    assert np.array_equal(x32.astype(np.float64), x)
    ref = val_ref.row_lse(first, second, vec.CLAMP_T)
    assert (ref == vec.clamped_lse(n_high)).all(), (name, ref[0], vec.clamped_lse(n_high))
    want = {"all_high": 50 + np.log(65.0), "all_low": -50 + np.log(65.0), "mixed": 50 + np.log(30 + 35 * np.exp(-100.0)),
            "one_high": 50 + np.log(1 + 64 * np.exp(-100.0))}[name]
    assert vec.clamped_lse(n_high) == want
    if name == "all_low":
        assert (x.max(axis=1) == -50.0).all(), "the row maximum is itself clamped"
    if n_high not in (0, vec.CLAMP_N2):      # the interleaving: both kinds on both sides of the 64-candidate tile edge's lanes
        pos = np.nonzero(s64[0] > 0)[0]
        assert len(pos) == n_high and (n_high == 1 or (np.diff(pos) > 1).any())
    # exact ties: duplicated rows of the second side
    assert len(np.unique(second, axis=0)) < vec.CLAMP_N2


def test_partly_clamped_bank():
    import test_gpu_validation as tgv
    assert np.array_equal(vec.related_bank(vec.PARTLY_K), tgv._bank(vec.PARTLY_K, True))
    assert np.array_equal(vec.unrelated_bank(65), tgv._bank(65, False))
    bank = vec.partly_clamped()
    for a, b in ((0, 1), (1, 0)):
        for raw in (val_ref.sims(bank[a], bank[b]) / vec.CLAMP_T, _f32_sims(bank[a], bank[b]).astype(np.float64) / vec.CLAMP_T):
            assert (raw < -50).sum() >= 16 and (raw > 50).any() and (np.abs(raw) < 40).sum() > raw.size // 2


def test_temperature_cases():
    bank = vec.unrelated_bank(65)
    s = val_ref.sims(bank[0], bank[1])
    assert np.abs(s / 1e3).max() < 1e-3 and np.abs(val_ref.row_lse(bank[0], bank[1], 1e3) - np.log(65.0)).max() < 1e-3
    assert np.abs(s / 1.0).max() <= 1.0 + 1e-6


@pytest.mark.parametrize("n1,n2", vec.SHAPES)
def test_rect_pairs(n1, n2):
    d1, d2 = vec.rect_pair(n1, n2)
    assert d1.shape == (2, n1, 128) and d2.shape == (2, n2, 128) and d1.dtype == d2.dtype == np.float32
    assert not np.array_equal(d1[0], d1[1])
    for p in range(2):
        nn12, nn21, mask = val_ref.mutual(d1[p], d2[p])
        assert mask.any() and nn12.shape == (n1,) and nn21.shape == (n2,)
        assert np.array_equal(mask, val_ref.mutual_rows(nn12, nn21))


def test_pair_rounds_bank_and_lists():
    bank = vec.rounds_bank()
    assert bank.shape == (vec.ROUNDS_FRAMES, vec.ROUNDS_K, 128) and len({b.tobytes() for b in bank}) == vec.ROUNDS_FRAMES
    first, second = vec.ROUNDS_LISTED
    assert len(first) == len(second) == 17
    absent = [p for p, (a, b) in enumerate(zip(first, second)) if not (0 <= a < 18 and 0 <= b < 18)]
    assert len(absent) == 2 and any(first[p] == -1 for p in absent)
    assert sum(a == b for a, b in zip(first, second)) >= 1
    pairs = [(a, b) for p, (a, b) in enumerate(zip(first, second)) if p not in absent]
    assert len(set(pairs)) < len(pairs), "a repeated pair"
    # 129 rows: two query blocks of 128, the second with one query; 9 and 17 pairs: a second and a third round of 8 with 7
    # surplus slots each
    assert -(-vec.ROUNDS_K // 128) == 2 and 9 % 8 and 17 % 8


def test_threshold_map():
    sal = vec.threshold_map()
    assert (sal == vec.HIGH).sum() == 4 and sal.dtype == np.float32
    above, below = np.nextafter(vec.HIGH, np.float32(1)), np.nextafter(vec.HIGH, np.float32(0))
    assert (sal == above).sum() == 1 and (sal == below).sum() == 1 and below < vec.HIGH < above
    assert (sal >= vec.HIGH).sum() == (sal > vec.HIGH).sum() + 4


@pytest.mark.parametrize("n1,n2", vec.PAIR_SHAPES)
@pytest.mark.parametrize("pattern", vec.PATTERNS)
def test_hand_made_index_arrays(pattern, n1, n2):
    if pattern == "identity" and n1 > n2:
        with pytest.raises(AssertionError):
            vec.index_arrays(pattern, n1, n2, 0)
        return
    z = vec.pair_arrays(pattern, n1, n2)
    assert z["nn12"].shape == (2, n1) and z["nn21"].shape == (2, n2) and z["nn12"].dtype == z["nn21"].dtype == np.int32
    for p in range(2):
        nn12, nn21 = z["nn12"][p].astype(np.int64), z["nn21"][p].astype(np.int64)
        mask = val_ref.mutual_rows(nn12, nn21)
        if pattern == "identity":
            assert mask.all()
        elif pattern == "none":
            assert ((nn12 >= 0) & (nn12 < n2)).all() and not mask.any()
            assert (nn21[nn12] != np.arange(n1)).all()
        else:
            out = (nn12 < 0) | (nn12 >= n2)
            assert out.sum() == max(1, n1 // 4) and not mask[out].any()
            assert (nn12 == -1).any() and (n1 < 8 or ((nn12 == n2).any() and (nn12 == vec.INT_MAX).any()))
            assert n1 == 1 or mask.any()
            clamped = nn21[np.clip(nn12, 0, n2 - 1)] == np.arange(n1)      # what a clamp in place of the guard would count
            assert clamped.sum() > mask.sum()
        s = val_ref.pair_sums(z["ce"][p], nn12, nn21, z["s12"][p, 0], z["s00"][p], 0.1)
        assert s["n_matches"] == mask.sum() and np.array_equal(s["mask"], mask)
        assert s["ce_sum"] == (0.0 if not mask.any() else float(z["ce"][p].astype(np.float64)[mask].sum()))
    # the 256-thread stride of the kernel: n1 on either side of it
    assert {n for n, _ in vec.PAIR_SHAPES} >= {1, 255, 256, 257, 1000}
