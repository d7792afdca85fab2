"""tests/guarded.py on CPU tensors: its two assertions fail when they should and pass when they should, for every dtype the
GPU tests guard (tests/test_gpu_guarded_outputs.py)."""
import numpy as np
import pytest
import torch as T

import guarded as gd

DTYPES = [T.float32, T.int32, T.int64, T.bfloat16, T.uint8]
SHAPES = [(3, 7), (1,), (5, 3, 2)]


def _fill(middle):
    """What a correct entry leaves: every payload element written with something that is not the sentinel."""
    if middle.dtype.is_floating_point:
        middle.copy_(T.arange(middle.numel(), dtype=T.float32).reshape(middle.shape))
    else:
        middle.copy_((T.arange(middle.numel()) % 100).reshape(middle.shape))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_alignment_and_sentinel(dtype, shape):
    whole, middle = gd.guarded(T, shape, dtype, device="cpu")
    assert middle.data_ptr() % 16 == 0 and middle.is_contiguous() and tuple(middle.shape) == shape and middle.dtype == dtype
    size = whole.element_size()
    assert middle.data_ptr() - whole.data_ptr() == gd.GUARD
    assert whole.numel() * size == 2 * gd.GUARD + middle.numel() * size
    idt, sentinel = gd._int_view(T, dtype)
    assert bool((whole.view(idt) == sentinel).all()), "every element starts as the sentinel"
    if dtype.is_floating_point:
        assert bool(T.isnan(whole.float()).all()), "the float sentinels are NaNs"


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clean_run_passes(dtype):
    whole, middle = gd.guarded(T, (4, 9), dtype, guard_bytes=gd.GUARD_WIDE, device="cpu")
    assert middle.data_ptr() - whole.data_ptr() == gd.GUARD_WIDE and middle.data_ptr() % 16 == 0
    _fill(middle)
    gd.assert_guards(whole, middle, "clean")
    gd.assert_written(middle, "clean")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["directly before", "directly after", "first of all", "last of all"])
def test_one_changed_guard_word_is_reported(dtype, where):
    whole, middle = gd.guarded(T, (4, 9), dtype, device="cpu")
    _fill(middle)
    g = gd.GUARD // whole.element_size()
    at = {"directly before": g - 1, "directly after": g + middle.numel(), "first of all": 0, "last of all": whole.numel() - 1}[where]
    idt, _ = gd._int_view(T, dtype)
    whole.view(idt)[at] ^= 1                                   # one bit of one guard element
    with pytest.raises(AssertionError, match="guard elements"):
        gd.assert_guards(whole, middle, where)
    gd.assert_written(middle, where)                           # the payload itself is complete


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("at", [0, 17, 35])
def test_one_unwritten_payload_element_is_reported(dtype, at):
    whole, middle = gd.guarded(T, (4, 9), dtype, device="cpu")
    _fill(middle)
    idt, sentinel = gd._int_view(T, dtype)
    middle.view(-1).view(idt)[at] = sentinel
    with pytest.raises(AssertionError, match=f"first at flat index {at}"):
        gd.assert_written(middle, "one element left")
    gd.assert_guards(whole, middle, "one element left")


def test_guarded_input_keeps_the_payload_and_fills_the_bands():
    x = np.random.default_rng(0).standard_normal((5, 11)).astype(np.float32)
    whole, middle = gd.guarded_input(T, x, device="cpu")
    assert middle.data_ptr() % 16 == 0 and np.array_equal(middle.numpy().view(np.uint32), x.view(np.uint32))
    g = gd.GUARD // 4
    assert bool(T.isnan(whole[:g]).all()) and bool(T.isnan(whole[g + x.size:]).all()), "NaN bands round a float input"
    gd.assert_guards(whole, middle, "input")
    img = np.random.default_rng(1).integers(0, 256, size=(2, 7, 9, 3), dtype=np.uint8)        # odd byte count
    for fill in (0x00, 0xFF):
        whole, middle = gd.guarded_input(T, img, fill=fill, device="cpu")
        assert np.array_equal(middle.numpy(), img) and middle.data_ptr() % 16 == 0
        assert bool((whole[:gd.GUARD] == fill).all()) and bool((whole[gd.GUARD + img.size:] == fill).all())
        gd.assert_guards(whole, middle, "image", fill=fill)
        whole[gd.GUARD + img.size] ^= 0x10
        with pytest.raises(AssertionError, match="behind"):
            gd.assert_guards(whole, middle, "image", fill=fill)
    idx = np.array([0, 3, -1], np.int32)
    whole, middle = gd.guarded_input(T, idx, device="cpu")
    assert np.array_equal(middle.numpy(), idx)


def test_dirty_workspace_and_refused_guard_sizes():
    for byte in (0x00, 0xFF):
        ws = gd.dirty(T, 1000, byte, device="cpu")
        assert ws.dtype == T.uint8 and ws.numel() == 1000 and bool((ws == byte).all())
    for bad in (0, 4096, gd.GUARD + 16):
        with pytest.raises(ValueError):
            gd.guarded(T, (3,), T.float32, guard_bytes=bad, device="cpu")
    with pytest.raises(ValueError):
        gd.guarded(T, (3,), T.float64, device="cpu")


# ---- placement: a payload `skew` bytes past a 256-byte boundary, strided operands, the Placement the loose-operand sweep uses
SKEWS = [0, 16, 240, 8, 248, 4, 252, 2, 254, 1, 3]


def _size(dtype):
    return T.empty((), dtype=dtype).element_size()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("skew", SKEWS)
def test_skewed_layout_lies_where_asked_and_keeps_both_bands(dtype, skew):
    if skew % _size(dtype):
        with pytest.raises(ValueError):
            gd.guarded(T, (4, 9), dtype, device="cpu", skew=skew)
        return
    x = (np.arange(36) % 100).reshape(4, 9)
    src = T.from_numpy(x).to(dtype)
    for whole, middle in (gd.guarded(T, (4, 9), dtype, device="cpu", skew=skew), gd.guarded_input(T, src, device="cpu", skew=skew)):
        # skew 0 is today's layout, on the allocation's own boundary (256 bytes on the device, 64 for a CPU tensor)
        assert middle.data_ptr() % (256 if skew else 16) == skew and middle.is_contiguous() and tuple(middle.shape) == (4, 9) and middle.dtype == dtype
        front = middle.data_ptr() - whole.data_ptr()
        back = whole.numel() * _size(dtype) - front - 36 * _size(dtype)
        assert front >= gd.GUARD and back >= gd.GUARD, "both bands keep guard_bytes at least"
        assert (front, back) == (gd.GUARD, gd.GUARD) if skew == 0 else front < gd.GUARD + 256 + skew
    whole, middle = gd.guarded_input(T, src, device="cpu", skew=skew)
    assert T.equal(middle, src)
    whole, middle = gd.guarded(T, (4, 9), dtype, device="cpu", skew=skew)
    idt, sentinel = gd._int_view(T, dtype)
    assert bool((whole.view(idt) == sentinel).all())
    _fill(middle)
    gd.assert_guards(whole, middle, "clean")
    gd.assert_written(middle, "clean")
    g = (middle.data_ptr() - whole.data_ptr()) // _size(dtype)
    for where, at in (("in front of", g - 1), ("behind", g + 36)):          # the band element adjacent to either end of the payload
        whole.view(idt)[at] ^= 1
        with pytest.raises(AssertionError, match=where):
            gd.assert_guards(whole, middle, where)
        whole.view(idt)[at] ^= 1
    gd.assert_guards(whole, middle, "restored")


@pytest.mark.parametrize("skew", [0, 1, 3, 16, 240])
def test_dirty_workspace_skewed(skew):
    ws = gd.dirty(T, 1000, 0xFF, device="cpu", skew=skew)
    assert ws.numel() == 1000 and bool((ws == 0xFF).all()) and (skew == 0 or ws.data_ptr() % 256 == skew)


def test_spread_lays_frames_a_stride_apart_with_sentinel_gaps():
    x = np.random.default_rng(2).standard_normal((3, 5, 4)).astype(np.float32)
    flat = gd.spread(x, 28)
    assert flat.shape == (2 * 28 + 20,) and flat.dtype == np.float32
    for f in range(3):
        assert np.array_equal(flat[f * 28:f * 28 + 20].view(np.uint32), x[f].reshape(-1).view(np.uint32))
        if f < 2:
            assert bool((flat[f * 28 + 20:(f + 1) * 28].view(np.uint32) == gd.SENTINEL).all()) and np.isnan(flat[f * 28 + 20:(f + 1) * 28]).all()
    assert np.array_equal(gd.spread(x, 20), x.reshape(-1)), "a dense stride is the array itself"
    img = np.random.default_rng(3).integers(0, 256, size=(2, 3, 5, 3), dtype=np.uint8)
    flat = gd.spread(img, 50, fill=0xFF)
    assert np.array_equal(flat[:45], img[0].reshape(-1)) and bool((flat[45:50] == 0xFF).all()) and np.array_equal(flat[50:], img[1].reshape(-1))
    idx = np.arange(6, dtype=np.int64).reshape(2, 3)
    assert gd.spread(idx, 4).view(np.uint64)[3] == gd.SENTINEL64
    with pytest.raises(ValueError):
        gd.spread(x, 19)
    whole, middle = gd.guarded_input(T, gd.spread(x, 28), device="cpu", skew=16)
    assert middle.data_ptr() % 256 == 16 and (middle.data_ptr() + 28 * 4) % 16 == 0
    gd.assert_guards(whole, middle, "strided input")


def test_placement_gives_every_operand_its_least_alignment():
    aligns = {"feat": 16, "kp_xy": 4, "images": 1, "workspace": 8, T.int64: 8}
    for mode, want in (("aligned", None), ("lo", {"feat": 16, "kp_xy": 4, "images": 1, "workspace": 8, "m": 8}),
                       ("hi", {"feat": 240, "kp_xy": 252, "images": 3, "workspace": 248, "m": 248})):
        with gd.placed(gd.Placement(aligns, mode)) as p:
            made = {"feat": gd.guarded_input(T, np.zeros((3, 4), np.float32), device="cpu", name="feat")[1],
                    "kp_xy": gd.guarded(T, (5, 2), T.float32, device="cpu", name="kp_xy")[1],
                    "images": gd.guarded_input(T, np.zeros(7, np.uint8), fill=0, device="cpu", name="images")[1],
                    "m": gd.guarded(T, (5, 2), T.int64, device="cpu", name="m")[1],          # by dtype
                    "workspace": gd.dirty(T, 100, 0, device="cpu")}
            own = gd.guarded(T, (3,), T.float32, device="cpu", skew=0)[1]                    # a skew of the caller's own is kept
            with pytest.raises(KeyError):
                gd.guarded(T, (3,), T.float32, device="cpu", name="unknown")
        assert gd.placement is None and own.data_ptr() % 16 == 0
        assert [r["name"] for r in p.made] == ["feat", "kp_xy", "images", "m", "workspace"]
        assert [r["kind"] for r in p.made] == ["in", "out", "in", "out", "ws"] and [r["align"] for r in p.made] == [16, 4, 1, 8, 8]
        for r in p.made:
            assert r["middle"] is made[r["name"]]
        if want:
            for k, t in made.items():
                assert t.data_ptr() % 256 == want[k], (mode, k)
                a = aligns.get(k, 8)
                assert a == 1 or (t.data_ptr() % a == 0 and t.data_ptr() % (2 * a) != 0), "at its alignment and no better"
    whole, middle = gd.guarded(T, (3,), T.float32, device="cpu")
    assert middle.data_ptr() - whole.data_ptr() == gd.GUARD, "without a placement: today's layout"
