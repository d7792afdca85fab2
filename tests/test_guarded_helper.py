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
