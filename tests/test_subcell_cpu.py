"""Sub-cell keypoint localisation without a GPU: the restatement (tests/subcell_ref.py) against the float64 parabola, its bounds,
the planted-bump and pose studies DESIGN.md §4j records, and the interface of libsslam_ext.so - include/sslam_ext.h,
sslam_amd.lib.EXT_EXPORTS and tests/ext_table.py hold the same entries; the built library's symbols are tests/test_libraries_cpu.py - with every host-side
check raising before the library is loaded."""
import os
import re

import numpy as np
import pytest

import ext_table as et
import subcell_cases as sc
import subcell_ref as ref
import subcell_study as study

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sslam_ext.h")


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_the_float64_parabola_vertex():
    """Over maxima of random fp32 triples with well-separated values: within 1e-6 cells of (p - m) / (2 (2c - m - p)) in float64."""
    rng = np.random.default_rng(1)
    c = rng.uniform(0.5, 1.0, 200000).astype(F)
    m = (c - rng.uniform(0.01, 0.4, c.size).astype(F)).astype(F)
    p = (c - rng.uniform(0.01, 0.4, c.size).astype(F)).astype(F)
    off, refined = ref.axis_offset(c, m, p, np.zeros(c.size, bool))
    assert refined.all()
    assert np.abs(off.astype(np.float64) - ref.parabola_vertex64(c, m, p)).max() <= 1e-6


def _adversarial_triples():
    rng = np.random.default_rng(2)
    n = 1_000_000
    bits = rng.integers(0, 2 ** 32, (3, n), dtype=np.uint64).astype(np.uint32).view(F)        # any fp32, NaN and inf among them
    bits = np.where(np.isfinite(bits), bits, F(0.5))
    c = bits[0]
    kind = rng.integers(0, 8, n)
    m, p = bits[1].copy(), bits[2].copy()
    tiny = (rng.integers(0, 64, n).astype(F) * sc.DMIN).astype(F)
    near = rng.uniform(0, 1, n).astype(F)
    with np.errstate(all="ignore"):
        m = np.where(kind == 1, c, m)                                        # one neighbour equal to the centre: exactly +-0.5
        p = np.where(kind == 2, c, p)
        m, p = np.where(kind == 3, c, m), np.where(kind == 3, c, p)          # all equal
        c3 = np.where(kind == 4, tiny + F(3) * sc.DMIN, c)                   # denormal values and differences
        m, p = np.where(kind == 4, tiny, m), np.where(kind == 4, (tiny * F(0.5)).astype(F), p)
        c = c3
        m = np.where(kind == 5, np.nextafter(c, F(-np.inf)), m)              # one ulp below
        p = np.where(kind == 6, F(-0.0), p)                                  # signed zeros
        c = np.where(kind == 6, F(0.0), c)
        m = np.where(kind == 7, (near * c).astype(F), m)                     # moderate: around the centre's own size
        p = np.where(kind == 7, ((F(1) - near) * c).astype(F), p)
    return c.astype(F), m.astype(F), p.astype(F)


def test_the_offset_never_leaves_half_a_cell():
    c, m, p = _adversarial_triples()
    off, refined = ref.axis_offset(c, m, p, np.zeros(c.size, bool))
    assert np.isfinite(off).all() and (np.abs(off) <= F(0.5)).all()
    assert refined.sum() > 100000                       # the sweep does refine
    assert (off[~refined].view(np.uint32) == 0).all()   # an axis that is not refined: +0.0, bit for bit
    # exactly half a cell where one neighbour equals the centre and the other lies below it
    with np.errstate(all="ignore"):
        twice_b, twice_a = (c - p) + (c - p), (c - m) + (c - m)          # den + den must not overflow: then off is 0, not a half
    one = (m == c) & (p < c) & np.isfinite(twice_b)
    assert one.sum() > 1000 and (off[one] == F(-0.5)).all() and refined[one].all()
    other = (p == c) & (m < c) & np.isfinite(twice_a)
    assert other.sum() > 1000 and (off[other] == F(0.5)).all() and refined[other].all()
    flat = (m == c) & (p == c)
    assert flat.sum() > 1000 and not refined[flat].any()
    # the rule |a - b| <= a + b in fp32, on every maximum with finite differences: the range test alone never rejects
    with np.errstate(all="ignore"):
        a, b = c - m, c - p
        den = a + b
        q = (a - b) / (den + den)
    maxima = (a >= 0) & (b >= 0) & (den > 0) & np.isfinite(a) & np.isfinite(b)
    assert (np.abs(q[maxima]) <= F(0.5)).all() and refined[maxima].all()


def test_planted_cases_decide_away_from_the_thresholds():
    names = set()
    for case in sc.cases():
        sc.check_decisions(case)
        names.add(case["name"])
    assert {"edges_and_corners", "plateau", "one_sided_ties", "pad_repeats", "nan_and_inf", "idx_out_of_range", "denormal_differences"} <= names


def test_planted_cases_give_what_they_were_planted_for():
    by = {c["name"]: c for c in sc.cases()}
    xy, px, fl = ref.subcell_keypoints(by["plateau"]["sal"], by["plateau"]["idx"])
    assert (fl == 0).all() and (xy.view(np.uint32) == np.stack([np.arange(16) % 4, np.arange(16) // 4], -1).astype(F).view(np.uint32)).all()
    xy, px, fl = ref.subcell_keypoints(by["one_sided_ties"]["sal"], by["one_sided_ties"]["idx"])
    cell = lambda x, y: y * 6 + x
    assert tuple(xy[0, cell(2, 2)]) == (2.5, 2.5) and tuple(xy[0, cell(3, 3)]) == (2.5, 2.5) and fl[0, cell(2, 2)] == 3
    assert tuple(xy[0, cell(1, 2)]) == (1.0, 2.5) and fl[0, cell(1, 2)] == ref.FLAG_Y          # x: a plateau along the ridge
    assert (px == xy * F(16) + F(8)).all()
    xy, px, fl = ref.subcell_keypoints(by["idx_out_of_range"]["sal"], by["idx_out_of_range"]["idx"])
    out = (by["idx_out_of_range"]["idx"] < 0) | (by["idx_out_of_range"]["idx"] >= 16)
    assert out.sum() == 8 and (fl[out] == ref.FLAG_RANGE).all() and (xy[out].view(np.uint32) == 0).all() and (px[out] == 8).all()
    assert (fl[~out] & ref.FLAG_RANGE == 0).all()
    xy, px, fl = ref.subcell_keypoints(by["nan_and_inf"]["sal"], by["nan_and_inf"]["idx"])
    assert np.isfinite(xy).all() and (fl[:3, 0] == 0).all()          # a NaN or infinite centre is never refined
    assert fl[3, 0] & ref.FLAG_X == 0                                # nor an axis between two infinite neighbours
    assert (fl[4] == 0).all()                                        # nor anything in a field of infinities
    xy, px, fl = ref.subcell_keypoints(by["denormal_differences"]["sal"], by["denormal_differences"]["idx"])
    assert (fl == 3).all() and xy[0, 0, 0] == F(1.0) + F(1.0) / F(6.0) and xy[0, 0, 1] == 1.0
    xy, px, fl = ref.subcell_keypoints(by["edges_and_corners"]["sal"], by["edges_and_corners"]["idx"])
    x, y = np.arange(25) % 5, np.arange(25) // 5
    assert (fl[:, (x == 0) | (x == 4)] & ref.FLAG_X == 0).all() and (fl[:, (y == 0) | (y == 4)] & ref.FLAG_Y == 0).all()


def test_shifting_the_field_by_whole_cells_shifts_the_result_exactly():
    rng = np.random.default_rng(3)
    small = np.stack([ref.bump_field(9, 4.3, 3.8, 1.0), rng.random((9, 9), dtype=F)])
    idx = np.tile(np.arange(81, dtype=np.int32), (2, 1))
    xy0, _, fl0 = ref.subcell_keypoints(small, idx)
    x0, y0 = idx % 9, idx // 9
    inner = (x0 > 0) & (x0 < 8) & (y0 > 0) & (y0 < 8)                      # the cells whose neighbours move with them
    f = np.arange(2)[:, None]
    offx = ref.axis_offset(small[f, y0, x0], small[f, y0, np.maximum(x0 - 1, 0)], small[f, y0, np.minimum(x0 + 1, 8)], ~inner)[0]
    offy = ref.axis_offset(small[f, y0, x0], small[f, np.maximum(y0 - 1, 0), x0], small[f, np.minimum(y0 + 1, 8), x0], ~inner)[0]
    assert (xy0[inner] == np.stack([x0.astype(F) + offx, y0.astype(F) + offy], -1)[inner]).all() and (fl0[inner] != 0).any()
    for dx, dy in ((0, 0), (3, 0), (0, 5), (7, 2)):
        big = np.zeros((2, 20, 20), F)
        big[:, dy:dy + 9, dx:dx + 9] = small
        moved = ((y0 + dy) * 20 + (x0 + dx)).astype(np.int32)
        xy, _, fl = ref.subcell_keypoints(big, moved)
        assert (fl[inner] == fl0[inner]).all() and inner.sum() == 2 * 49
        # the offset is the same bits; the cell moved by exactly (dx, dy)
        want = np.stack([(x0 + dx).astype(F) + offx, (y0 + dy).astype(F) + offy], -1)
        assert (xy[inner].view(np.uint32) == want[inner].view(np.uint32)).all()
        assert (np.floor(xy + F(0.5))[inner] - np.floor(xy0 + F(0.5))[inner] == np.array([dx, dy], F)).all()


# ------------------------------------------------------------------------------------------------------------------ the studies
def test_planted_bumps_at_sigma_one():
    """base 0.1, amplitude 0.8, sigma 1 cell, 15 x 15 grid, the peak uniform within its cell, 2000 seeded draws.  Measured with
    this restatement: grid rms 0.4076 cells; parabola rms 0.0483, max 0.0674 cells - the analytic bias of a parabola on a
    Gaussian.  The bounds are the issue's: max <= 0.08, rms <= 0.06, rms at most a quarter of the grid's."""
    r = study.bump_errors(sigma=1.0, draws=2000)
    print(f"planted bumps sigma 1: grid rms {r['grid_rms']:.4f}, parabola rms {r['rms']:.4f}, max {r['max']:.4f} cells")
    assert r["max"] <= 0.08 and r["rms"] <= 0.06
    assert r["rms"] <= r["grid_rms"] / 4


def test_planted_bumps_under_noise_are_recorded():
    """The issue's noise rows, re-measured with the restatement (2000 seeded draws each, Gaussian noise on every cell; the issue
    sets no bound for them, DESIGN.md §4j records them): sigma 1, noise 0.005: rms 0.0500, max 0.0950; sigma 1, noise 0.02: rms
    0.0701, max 0.1909; sigma 2, noise 0.02: rms 0.1544, max 0.5003 - a flat bump under that noise is located no better than
    a third of the grid's own error.  This test runs the noisy path (500 draws each) and prints its figures; it asserts only
    that they are finite."""
    for sigma, noise in ((1.0, 0.005), (1.0, 0.02), (2.0, 0.02)):
        r = study.bump_errors(sigma=sigma, draws=500, noise=noise)
        print(f"planted bumps sigma {sigma}, noise {noise} (500 draws): rms {r['rms']:.4f}, max {r['max']:.4f} cells")
        assert np.isfinite([r["rms"], r["max"], r["grid_rms"]]).all()


def test_pose_study_refined_keypoints_give_the_better_translation():
    """40 seeded pairs, 36 planted points on a jittered lattice of the 28 x 28 grid rendered as sigma = 1 bumps, depths 1.5 - 4 m,
    0.5 - 2 degrees and up to 5 cm per axis between the cameras; oracle selection, matches by planted identity, RANSAC
    (128 hypotheses, threshold 8 keypoint units) and 5 refinement steps.  Measured with these restatements: median translation
    error 50.7 mm from the cell centres, 4.84 mm from the refined keypoints (rotation 1.63 and 0.110 degrees); refined smaller in
    40 of 40 pairs; median ratio 0.102.  Bounds: those figures with a margin of 1.5 (the run is seeded and deterministic; the
    margin covers libm differences): share >= 1 / 1.5, median ratio <= 0.154."""
    r = study.pose_study(40)
    print("pose study: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()))
    assert r["matches_min"] >= 30
    assert r["share"] >= 1.0 / 1.5
    assert r["ratio_median"] <= 0.102 * 1.5


# ---------------------------------------------------------------------------------------------------------------- the interface
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_symbols_exports_and_table_agree():
    """The table against the export list; that list against the header and the built library is tests/test_libraries_cpu.py."""
    from sslam_amd import lib
    declared = lib.EXT_EXPORTS
    assert set(et.ALIGN) | set(et.HOST_ONLY) == set(declared) and not set(et.ALIGN) & set(et.HOST_ONLY)


def test_a_row_names_the_device_pointers_of_its_prototype_and_the_header_states_it():
    elem = {"int32_t": 4, "float": 4}
    text = _header()
    for entry, row in et.ALIGN.items():
        m = re.search(r"\bint\s+" + entry + r"\s*\(([^;{]*?)\)\s*;", text)
        assert m, entry
        args = [re.match(r"(.*?)(\w+)$", " ".join(a.split())).groups() for a in m.group(1).split(",")]
        pointers = [(t.strip(), n) for t, n in args if "*" in t and n != "stream"]
        assert [n for _, n in pointers] == list(row), entry
        for t, n in pointers:
            assert row[n] in (4, 8, 16) and row[n] >= elem[t.replace("const", "").replace("*", "").strip()], (entry, n)
    raw = open(HEADER).read()
    start = raw.index("ALIGNMENT, every entry")
    stated = re.sub(r"\n \*\s+", " ", raw[start:raw.index("*/", start)]).strip()          # the block's lines joined, the margin dropped
    for line in et.header_lines():
        assert line + " " in stated + " ", f"include/sslam_ext.h does not state: {line}"
    assert len(re.findall(r"\bsslx_\w+: ", stated)) == len(et.ALIGN)
    for text_ in ("off = (a - b) / (den + den)", "a >= 0 && b >= 0", "den > 0", "off >= -0.5f && off <= 0.5f", "kp_xy_sub * 16.0f + 8.0f"):
        assert text_ in raw, text_


def test_every_check_comes_before_the_library_is_loaded(monkeypatch):
    import torch
    from sslam_amd import lib

    def boom():
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(lib, "ext", boom)
    sal, idx = torch.zeros((2, 4, 4)), torch.zeros((2, 5), dtype=torch.int32)
    bad = [(sal.double(), idx), (sal[0], idx), (torch.zeros((2, 4, 5)), idx), (sal, idx.long()), (sal, idx[:1]), (sal, idx[0]),
           (sal, torch.zeros((2, 0), dtype=torch.int32)), (sal.numpy(), idx), (sal, idx.numpy()), (sal.transpose(1, 2), idx),
           (torch.zeros((0, 4, 4)), torch.zeros((0, 5), dtype=torch.int32))]
    for s, i in bad:
        with pytest.raises(ValueError):
            lib.subcell_keypoints(s, i)
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.subcell_keypoints(torch.zeros((1, 65, 65)), torch.zeros((1, 5), dtype=torch.int32))
    with pytest.raises(lib.SslamHipError, match="unsupported"):
        lib.subcell_keypoints(torch.zeros((1, 4, 4)), torch.zeros((1, 4097), dtype=torch.int32))
    for out in ((torch.zeros((2, 5, 2)), torch.zeros((2, 5, 2))), (torch.zeros((2, 5, 2)), torch.zeros((2, 5, 2)), torch.zeros((2, 5))),
                (torch.zeros((2, 5, 2)), torch.zeros((2, 5)), torch.zeros((2, 5), dtype=torch.int32)),
                (torch.zeros((2, 5, 2)), None, torch.zeros((2, 5), dtype=torch.int32))):
        with pytest.raises(ValueError):
            lib.subcell_keypoints(sal, idx, out=out)
    with pytest.raises(ValueError, match="CUDA"):                    # well-formed host tensors: refused, still nothing loaded
        lib.subcell_keypoints(sal, idx)


def test_the_config_fields_are_opt_in_and_checked():
    from sslam_amd.pipeline import ExtractorConfig
    cfg = ExtractorConfig()
    assert cfg.subcell is False and cfg.subcell_descriptors is False
    assert list(ExtractorConfig.__dataclass_fields__)[-2:] == ["subcell", "subcell_descriptors"]
    assert ExtractorConfig(subcell=True, subcell_descriptors=True).subcell_descriptors
    with pytest.raises(ValueError, match="subcell"):
        ExtractorConfig(subcell_descriptors=True)


def test_the_numpy_drop_in_checks_its_arguments_first():
    import evaluation as dropin
    with pytest.raises(ValueError):
        dropin.refine_keypoints_subcell(np.zeros((4, 5), F), np.zeros((3, 2), F))
    with pytest.raises(ValueError):
        dropin.refine_keypoints_subcell(np.zeros((4, 4), F), np.zeros((3, 3), F))
    with pytest.raises(ValueError, match="whole cells"):
        dropin.refine_keypoints_subcell(np.zeros((4, 4), F), np.array([[1.5, 2.0]], F))


def test_the_selector_refines_on_the_cpu_as_the_restatement_does():
    """KeypointSelector.refine_keypoints on CPU tensors: the same formula in eager torch, bit for bit."""
    import torch
    from models.keypoint_selector import KeypointSelector
    sel = KeypointSelector()
    for case in sc.cases():
        if int(case["idx"].min()) < 0 or int(case["idx"].max()) >= case["sal"].shape[1] ** 2:
            continue
        g = case["sal"].shape[1]
        kp = np.stack([case["idx"] % g, case["idx"] // g], -1).astype(F)
        got = sel.refine_keypoints(torch.from_numpy(case["sal"])[..., None], torch.from_numpy(kp)).numpy()
        want = ref.subcell_keypoints(case["sal"], case["idx"])[0]
        assert got.dtype == F and (got.view(np.uint32) == want.view(np.uint32)).all(), case["name"]
    with pytest.raises(ValueError):
        sel.refine_keypoints(torch.zeros((1, 4, 4, 1)), torch.tensor([[[4.0, 0.0]]]))
