"""Poisoned, guarded buffers for the tests of where an entry of libsslam_hip.so writes (tests/test_gpu_guarded_outputs.py).

An output handed to an entry lies between two guard bands in ONE allocation, every element - bands and payload - a sentinel no
kernel result has: after the call the bands must still hold it (the entry wrote only inside its output) and no payload element
may (it wrote every element).  An input lies between bands of NaN bits (floats) or of a given byte (uint8 images), so that what a
kernel reads beyond it cannot be multiplied away unseen.  A workspace is filled with a byte of the caller's choice: an entry that
reads scratch before writing it gives other results under another fill.

Works on CPU tensors as on device tensors (tests/test_guarded_helper.py needs no GPU).  `T` is the torch module throughout, as in
the GPU tests' fixtures.
"""
import numpy as np

SENTINEL = 0x7FC0DEAD              # 4-byte elements: a NaN's bits (tests/test_gpu_validation_edges.py uses the same word)
SENTINEL64 = 0x7FC0DEAD7FC0DEAD    # int64: the same word twice
SENTINEL_BF16 = 0x7FDE             # bf16: a NaN's bits, the upper half of no rounded fp32 result
SENTINEL_U8 = 0xA5                 # uint8: a byte pattern

GUARD = 64 * 1024                  # the least guard band: one 128 x 128 fp32 tile
GUARD_WIDE = 256 * 1024            # descriptor width 256 and the ViT's 128 x 384 token tiles


def _int_view(T, dtype):
    """(integer dtype of the same width to compare and fill bits in, sentinel) of a payload dtype."""
    table = {T.float32: (T.int32, SENTINEL), T.int32: (T.int32, SENTINEL), T.int64: (T.int64, SENTINEL64),
             T.bfloat16: (T.int16, SENTINEL_BF16), T.uint8: (T.uint8, SENTINEL_U8)}
    if dtype not in table:
        raise ValueError(f"no sentinel for {dtype}")
    return table[dtype]


def _layout(T, n, dtype, guard_bytes, device, fill):
    """A flat tensor of dtype: guard_bytes of `fill`, n elements, guard_bytes of `fill`; the payload holds `fill` too."""
    if guard_bytes < GUARD or guard_bytes % 256:
        raise ValueError(f"guard_bytes must be a multiple of 256 and at least {GUARD}, got {guard_bytes}")
    idt, _ = _int_view(T, dtype)
    g = guard_bytes // T.empty((), dtype=dtype).element_size()
    whole = T.full((2 * g + n,), fill, dtype=idt, device=device).view(dtype)
    assert whole.data_ptr() % 16 == 0, "the allocator hands out 16-byte aligned blocks"
    return whole, g


def guarded(T, shape, dtype, guard_bytes=GUARD, device="cuda"):
    """-> (whole, middle): one flat allocation, every element the sentinel of `dtype`; `middle` is the contiguous view of `shape`
    between two bands of guard_bytes (a multiple of 256: middle keeps the 16-byte alignment the entries demand)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64))
    whole, g = _layout(T, n, dtype, guard_bytes, device, _int_view(T, dtype)[1])
    return whole, whole[g:g + n].view(shape)


def guarded_input(T, array, fill=None, guard_bytes=GUARD, device="cuda"):
    """The same layout for an input: `array` (numpy, or a tensor on any device: bf16 has no numpy type) copied between two bands
    of `fill` - the dtype's sentinel (NaN bits for floats) unless given; for a uint8 image a byte.  -> (whole, middle)."""
    src = array.contiguous() if isinstance(array, T.Tensor) else T.from_numpy(np.ascontiguousarray(array))
    if fill is None:
        fill = _int_view(T, src.dtype)[1]
    whole, g = _layout(T, src.numel(), src.dtype, guard_bytes, device, fill)
    middle = whole[g:g + src.numel()].view(src.shape)
    middle.copy_(src)
    return whole, middle


def _bands(T, whole, middle):
    idt, _ = _int_view(T, whole.dtype)
    size = whole.element_size()
    off = middle.data_ptr() - whole.data_ptr()
    assert off > 0 and off % size == 0 and middle.is_contiguous() and middle.dtype == whole.dtype, "middle is not a view of whole"
    g, n = off // size, middle.numel()
    assert g + n < whole.numel()
    w = whole.view(idt)
    return w[:g], w[g:g + n], w[g + n:]


def assert_guards(whole, middle, what, fill=None):
    """Both bands of `whole` around `middle` still hold the sentinel (or `fill`, for a guarded_input made with one), bit for bit."""
    import torch as T
    want = _int_view(T, whole.dtype)[1] if fill is None else fill
    front, _, back = _bands(T, whole, middle)
    for name, band in (("in front of", front), ("behind", back)):
        bad = (band != want).nonzero()
        if bad.numel():
            first, last = int(bad[0]), int(bad[-1])
            at = first - band.numel() if name == "in front of" else first
            raise AssertionError(f"{what}: {bad.shape[0]} guard elements {name} the payload were written; the first at element {at} "
                                 f"relative to the payload's {'start' if name == 'in front of' else 'end'} (the last {last - first} further), "
                                 f"now {int(band[first]) & (2 ** (8 * band.element_size()) - 1):#x}")


def assert_written(middle, what):
    """No element of the payload still holds the sentinel."""
    import torch as T
    idt, sentinel = _int_view(T, middle.dtype)
    left = (middle.reshape(-1).view(idt) == sentinel).nonzero()
    if left.numel():
        raise AssertionError(f"{what}: {left.shape[0]} of {middle.numel()} payload elements were never written; the first at flat "
                             f"index {int(left[0])}, the last at {int(left[-1])} (shape {tuple(middle.shape)})")


def dirty(T, nbytes, byte, device="cuda"):
    """A workspace of exactly nbytes filled with `byte`."""
    return T.full((int(nbytes),), int(byte), dtype=T.uint8, device=device)
