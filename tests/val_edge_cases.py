"""Numpy-only input builders for the validation kernels' edge tests: tests/test_validation_edge_inputs.py proves on the CPU that
they have the properties tests/test_gpu_validation_edges.py relies on.  Everything is seeded; a frame's image or a case's
descriptors are the same arrays wherever they are asked for."""
import numpy as np

import synth

SEG = 512                                   # pixel columns per workgroup of edge_pool_kernel
SIZES = (512, 544, 1024, 1040)              # one full segment; 512 + 32; two full; 512 + 512 + 16
SIZES_FRAMES = ((512, 1), (544, 1), (544, 2), (1024, 1), (1040, 1), (1040, 2))
KINDS = ("random", "seams", "peak_last")
PEAK = 40.0


def seams(size):
    """The first pixel column of every column segment but the first."""
    return list(range(SEG, size, SEG))


# ------------------------------------------------------------------------------------------------------------------ images
def _random(size, seed):
    rng = np.random.default_rng(1000 * size + seed)      # as _images("random") of test_gpu_validation.py, a frame at a time
    coarse = rng.normal(0, 1, (3, size // 8, size // 8))
    return (np.kron(coarse, np.ones((8, 8))) + rng.normal(0, 0.3, (3, size, size))).astype(np.float32)


def peak_position(size, frame):
    """(row, column) of the isolated pixel of `peak_last`: the last segment in frame 0, segment 0 in every other frame."""
    return size // 2 + 3, (size - 5 if frame == 0 else 5)


def image(kind, size, frame):
    """One fp32 frame (3, size, size)."""
    if kind == "random":
        return _random(size, frame)
    if kind == "seams":      # zero but for the four columns around every segment start and the two outermost rows at each end
        rng = np.random.default_rng(7000 * size + frame)
        img = np.zeros((3, size, size), np.float32)
        img[:, :2, :] = rng.normal(0, 1, (3, 2, size))
        img[:, -2:, :] = rng.normal(0, 1, (3, 2, size))
        for c0 in seams(size):
            img[:, :, c0 - 2:c0 + 2] = rng.normal(0, 1, (3, size, 4))      # every column its own values: both sides differ
        return img
    if kind == "peak_last":
        img = _random(size, 50 + frame) * np.float32(0.1)
        y, x = peak_position(size, frame)
        img[:, y, x] = np.float32(PEAK)
        return img
    raise ValueError(kind)


def images(kind, size, n):
    return np.stack([image(kind, size, f) for f in range(n)])


def saliency(size, n):
    g = size // 16
    return np.random.default_rng(31 * size + 5).uniform(0.02, 0.98, (2, g, g)).astype(np.float32)[:n]


def shifted_images(size):
    """(A, B, C): B is A moved right by 16 columns, C is A moved left by 16; the vacated columns hold other random values."""
    a = _random(size, 300)
    fill = _random(size, 301)
    b, c = fill.copy(), fill.copy()
    b[:, :, 16:] = a[:, :, :-16]
    c[:, :, :-16] = a[:, :, 16:]
    return a, b, c


def shift_cells(size):
    """Cell columns gx of A whose 18-column neighbourhood - pixel columns 16 gx - 1 .. 16 gx + 16 - holds the same real pixels
    in A and in the moved image (no zero padding in either, no vacated column): -> (for B: compare B[gx + 1], for C: C[gx - 1])."""
    g = size // 16
    for_b = [gx for gx in range(g) if 16 * gx - 1 >= 0 and 16 * gx + 16 <= size - 1 and 16 * (gx + 1) + 16 <= size - 1]
    for_c = [gx for gx in range(g) if 16 * gx + 16 <= size - 1 and 16 * (gx - 1) - 1 >= 0]
    return for_b, for_c


CROP = 544


def crop_cells(size):
    """The last cell column of an image has zero padding on its right, so no moved image can hold the same neighbourhood
    elsewhere.  The last CROP columns (and first CROP rows) of A as an image of their own do: cell (gy, CROP/16 - 1) of the crop
    has the neighbourhood of cell (gy, G - 1) of A for every cell row but the crop's last (zero padding below it there).
    -> (cell column of A, cell column of the crop, number of cell rows compared); None where size <= CROP."""
    if size <= CROP:
        return None
    return size // 16 - 1, CROP // 16 - 1, CROP // 16 - 1


def compared_cells(size):
    """{image name: set of its cell columns that the position check compares with a cell at another place}."""
    for_b, for_c = shift_cells(size)
    out = dict(A=set(for_b) | set(for_c), B={gx + 1 for gx in for_b}, C={gx - 1 for gx in for_c}, crop=set())
    cc = crop_cells(size)
    if cc:
        out["A"].add(cc[0])
        out["crop"].add(cc[1])
    return out


# ------------------------------------------------------------------------------------------------------------- descriptors
D = 128


def _unit(x):
    return (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def cluster(n, sign, seed):
    """n unit rows sign * v + 0.3 noise / sqrt(128), normalised, around one fixed unit vector v."""
    v = _unit(np.random.default_rng(4242).standard_normal((1, D)))
    noise = np.random.default_rng(9000 + seed).standard_normal((n, D))
    return _unit(float(sign) * v.astype(np.float64) + 0.3 * noise / np.sqrt(D))


CLAMP_T = 0.01
CLAMP_N1, CLAMP_N2 = 129, 65
CLAMPED = ("all_high", "all_low", "mixed", "one_high")


def clamped_case(name):
    """(first side (129, 128), second side (65, 128), number of same-sign rows of the second side): every similarity is
    beyond +-0.6, so that every logit at T = 0.01 is exactly +-50.  The last two rows of a group of four or more repeat its
    first two bit for bit (exact ties of the arg-max), and 65 is one row past the 64-candidate tile."""
    first = cluster(CLAMP_N1, +1, 1)
    n_high = dict(all_high=65, all_low=0, mixed=30, one_high=1)[name]
    high, low = cluster(n_high, +1, 2), cluster(CLAMP_N2 - n_high, -1, 3)
    for grp in (high, low):
        if len(grp) >= 4:
            grp[-2:] = grp[:2]
    second = np.concatenate([high, low])
    if name in ("mixed", "one_high"):      # a seeded interleaving / position
        second = second[np.random.default_rng(77 + n_high).permutation(CLAMP_N2)]
    return first, second, n_high


def clamped_lse(n_high):
    """The closed form of a fully clamped row: log(h e^50 + (65 - h) e^-50)."""
    if n_high == 0:
        return -50.0 + np.log(float(CLAMP_N2))
    return 50.0 + np.log(n_high + (CLAMP_N2 - n_high) * np.exp(-100.0))


def related_bank(k):
    """The "related" bank of test_gpu_validation.py (_bank(k, True)): 3 frames, 1 and 2 noisy copies of frame 0."""
    dup = min(k // 4, 8)
    d0, d1 = synth.descriptor_pair(11 + k, k, k, dup, noise=0.25)[:2]
    d2 = synth.descriptor_pair(11 + k, k, k, dup, noise=0.4)[1]
    return np.stack([d0, d1, d2])


def unrelated_bank(k):
    """_bank(k, False) of test_gpu_validation.py."""
    dup = min(k // 4, 8)
    return np.stack([synth.unit_descriptors(100 * k + f, k, 128, dup) for f in range(3)])


PARTLY_K = 129


def partly_clamped():
    """Frames 0 and 1 of the related bank at K = 129 with 16 rows of frame 1 replaced by NEGATED rows of frame 0: at T = 0.01
    raw logits near -100 (those rows against their originals), above 50 (the noisy copies) and unclamped ones (the rest)."""
    bank = related_bank(PARTLY_K)[:2].copy()
    rng = np.random.default_rng(1601)
    rows = rng.choice(PARTLY_K, 16, replace=False)
    bank[1, rows] = -bank[0, rng.choice(PARTLY_K, 16, replace=False)]
    return bank


SHAPES = ((1, 300), (129, 37), (37, 129), (200, 64), (64, 65))


def rect_pair(n1, n2, n_pairs=2):
    """(d1 (n_pairs, n1, 128), d2 (n_pairs, n2, 128)): the second side holds noisy copies of rows of the first (mutual matches
    exist) and both hold duplicated rows."""
    dup = min(min(n1, n2) // 4, 8)
    pairs = [synth.descriptor_pair(1000 * n1 + n2 + p, n1, n2, dup, noise=0.3)[:2] for p in range(n_pairs)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


ROUNDS_K, ROUNDS_FRAMES = 129, 18
ROUNDS_LISTED = ([0, 3, -1, 5, 5, 17, 2, 9, 16, 1, 18, 7, 0, 12, 4, 11, 8],       # pair 2 and pair 10 absent (-1; 18 = n_bank),
                 [1, 0, 4, 5, 6, 16, 13, 9, 3, 2, 1, 14, 1, 10, 15, 6, 17])      # 3 and 7 self pairs, 12 repeats pair 0


def rounds_bank():
    """18 frames of 129 descriptors: frame 0 and noisy, permuted copies of it."""
    d0 = synth.descriptor_pair(500, ROUNDS_K, ROUNDS_K, 8)[0]
    return np.stack([d0] + [synth.descriptor_pair(500, ROUNDS_K, ROUNDS_K, 8, noise=0.2 + 0.02 * f)[1] for f in range(1, ROUNDS_FRAMES)])


# ------------------------------------------------------------------------------------------------------- frame statistics
HIGH = np.float32(0.6)


def threshold_map():
    """A 5 x 5 saliency map with 0.6f in four cells and its two neighbouring floats in two more."""
    sal = np.random.default_rng(55).uniform(0.02, 0.98, (5, 5)).astype(np.float32)
    sal[0, 0] = sal[1, 3] = sal[4, 4] = sal[2, 2] = HIGH
    sal[3, 1] = np.nextafter(HIGH, np.float32(1.0))
    sal[0, 4] = np.nextafter(HIGH, np.float32(0.0))
    return sal


# --------------------------------------------------------------------------------------- hand-made arg-max arrays (section 4)
PAIR_SHAPES = ((1, 1), (255, 300), (256, 256), (257, 64), (1000, 37))
PATTERNS = ("identity", "none", "out_of_range")
INT_MAX = 2 ** 31 - 1


def index_arrays(pattern, n1, n2, seed):
    """(nn12 (n1,), nn21 (n2,)) int32 for one pair."""
    rng = np.random.default_rng(100_000 * seed + 300 * n1 + n2)
    if pattern == "identity":      # every row mutual
        assert n1 <= n2
        nn12 = np.arange(n1)
        nn21 = np.concatenate([np.arange(n1), rng.integers(0, n1, n2 - n1)])
    elif pattern == "none":        # nn21[nn12[i]] != i for every i; n1 (no row's index) where every row points at j
        nn12 = rng.integers(0, n2, n1)
        nn21 = np.empty(n2, np.int64)
        for j in range(n2):
            free = np.nonzero(nn12 != j)[0]
            nn21[j] = rng.choice(free) if len(free) else n1
    elif pattern == "out_of_range":
        nn12, nn21 = rng.integers(0, n2, n1), rng.integers(0, n1, n2)
        m = min(n1, n2) // 2      # make about half of the shorter side mutual
        js, rows = rng.choice(n2, m, replace=False), rng.choice(n1, m, replace=False)
        nn12[rows], nn21[js] = js, rows
        bad = rng.choice(n1, max(1, n1 // 4), replace=False)
        nn12[bad] = rng.choice([-1, n2, INT_MAX], len(bad))
        # rows that an index CLAMPED into the range would count: -1 -> 0 and n2 -> n2 - 1 point back at them
        nn12[bad[0]], nn21[0] = -1, bad[0]
        if len(bad) > 1:
            nn12[bad[1]], nn21[n2 - 1] = n2, bad[1]
    else:
        raise ValueError(pattern)
    return nn12.astype(np.int32), nn21.astype(np.int32)


def pair_arrays(pattern, n1, n2, n_pairs=2):
    """Everything val_pair_stats reads for n_pairs pairs: nn12, nn21, s12, ce, s00, sal1, sal2 (G = 3)."""
    rng = np.random.default_rng(17 * n1 + n2 + len(pattern))
    idx = [index_arrays(pattern, n1, n2, p) for p in range(n_pairs)]
    f = np.float32
    return dict(nn12=np.stack([i[0] for i in idx]), nn21=np.stack([i[1] for i in idx]),
                s12=rng.uniform(-1, 1, (n_pairs, n1)).astype(f), ce=rng.uniform(0, 6, (n_pairs, n1)).astype(f),
                s00=rng.uniform(-1, 1, n_pairs).astype(f), sal1=rng.uniform(0, 1, (n_pairs, 3, 3)).astype(f),
                sal2=rng.uniform(0, 1, (n_pairs, 3, 3)).astype(f))
