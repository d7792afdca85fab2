"""Poisoned, guarded buffers for the tests of where an entry of libsslam_hip.so writes (tests/test_gpu_guarded_outputs.py).

An output handed to an entry lies between two guard bands in ONE allocation, every element - bands and payload - a sentinel no
kernel result has: after the call the bands must still hold it (the entry wrote only inside its output) and no payload element
may (it wrote every element).  An input lies between bands of NaN bits (floats) or of a given byte (uint8 images), so that what a
kernel reads beyond it cannot be multiplied away unseen.  A workspace is filled with a byte of the caller's choice: an entry that
reads scratch before writing it gives other results under another fill.

Placement: `skew=` bytes puts a payload that far past a 256-byte boundary (both bands keep their size at least), spread() lays
frames a stride apart with sentinel gaps, and a Placement in force (`with placed(...)`) gives every operand made inside it the
least alignment its entry accepts - tests/test_gpu_loose_operands.py runs the guarded cases of the other files that way.

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
             T.bfloat16: (T.int16, SENTINEL_BF16), T.int16: (T.int16, SENTINEL_BF16), T.uint8: (T.uint8, SENTINEL_U8)}
    if dtype not in table:
        raise ValueError(f"no sentinel for {dtype}")
    return table[dtype]


class Placement:
    """Where the operands of the calls made inside `with placed(...)` lie (tests/test_gpu_loose_operands.py).  `aligns` maps an
    operand's name - the name tests/test_gpu_guarded_outputs.py::Bufs gives it, "workspace" for dirty() - or, failing that, its
    torch dtype to the alignment a in bytes that include/sslam_hip.h states for it; `mode` turns a into the skew:
      "aligned"  0: today's layout (the placement only records what was made);
      "lo"       a, just past a 256-byte boundary;      "hi"  256 - a, just before one;      for a = 1: 1 and 3.
    The address is then a multiple of a and of nothing larger.  An operand named by neither key is an error: every pointer of
    the call is placed.  Everything made is recorded in `made`: dicts of name, kind ("in" / "out" / "ws"), align, whole, middle."""

    def __init__(self, aligns, mode):
        assert mode in ("aligned", "lo", "hi"), mode
        self.aligns, self.mode, self.made = dict(aligns), mode, []

    def align(self, name, dtype):
        for key in (name, dtype):
            if key in self.aligns:
                return int(self.aligns[key])
        raise KeyError(f"no alignment stated for operand {name!r} ({dtype})")

    def skew(self, name, dtype):
        a = self.align(name, dtype)
        assert a in (1, 2, 4, 8, 16), (name, a)
        if self.mode == "aligned":
            return 0
        if a == 1:
            return 1 if self.mode == "lo" else 3
        return a if self.mode == "lo" else 256 - a


placement = None          # the Placement in force, or None: every layout as it always was


class placed:
    """with placed(Placement(...)) as p: ... - guarded(), guarded_input() and dirty() calls inside that pass no skew of their own
    take p's."""

    def __init__(self, p):
        self.p = p

    def __enter__(self):
        global placement
        assert placement is None, "placements do not nest"
        placement = self.p
        return self.p

    def __exit__(self, *exc):
        global placement
        placement = None


def _skew_of(skew, name, dtype, kind):
    """The skew of one layout: the caller's own, else the placement's, else 0 -> (skew, the record to complete or None)."""
    if skew is not None or placement is None:
        return int(skew or 0), None
    rec = dict(name=name, kind=kind, align=placement.align(name, dtype))
    placement.made.append(rec)
    return placement.skew(name, dtype), rec


def _layout(T, n, dtype, guard_bytes, device, fill, skew=0):
    """A flat tensor of dtype: a band of `fill`, n elements, a band of `fill`; the payload holds `fill` too.  -> (whole, g): the
    payload is whole[g:g + n].  With skew 0 both bands are guard_bytes and the payload lies on the allocation's own boundary;
    with a skew (a multiple of the element size below 256) the allocation's start is found modulo 256 and the front band is
    stretched by less than 256 bytes + skew so that the payload starts `skew` bytes past a 256-byte boundary - the back band is
    still guard_bytes, neither is shorter."""
    if guard_bytes < GUARD or guard_bytes % 256:
        raise ValueError(f"guard_bytes must be a multiple of 256 and at least {GUARD}, got {guard_bytes}")
    idt, _ = _int_view(T, dtype)
    size = T.empty((), dtype=dtype).element_size()
    if not 0 <= skew < 256 or skew % size:
        raise ValueError(f"skew must be a multiple of the element size {size} in [0, 256), got {skew}")
    g = guard_bytes // size
    if skew == 0:
        whole = T.full((2 * g + n,), fill, dtype=idt, device=device).view(dtype)
        assert whole.data_ptr() % 16 == 0, "the allocator hands out 16-byte aligned blocks"
        return whole, g
    whole = T.full((2 * g + n + 512 // size,), fill, dtype=idt, device=device).view(dtype)
    assert whole.data_ptr() % size == 0
    front = guard_bytes + (skew - whole.data_ptr() - guard_bytes) % 256
    g = front // size
    whole = whole[:g + n + guard_bytes // size]
    assert (whole.data_ptr() + front) % 256 == skew and front >= guard_bytes
    return whole, g


def guarded(T, shape, dtype, guard_bytes=GUARD, device="cuda", skew=None, name=None):
    """-> (whole, middle): one flat allocation, every element the sentinel of `dtype`; `middle` is the contiguous view of `shape`
    between two bands of guard_bytes at least (a multiple of 256: with skew 0 middle keeps the 16-byte alignment the entries
    demand; with `skew` bytes it starts that far past a 256-byte boundary).  skew None: 0, or what the Placement in force gives
    the operand `name`."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64))
    skew, rec = _skew_of(skew, name, dtype, "out")
    whole, g = _layout(T, n, dtype, guard_bytes, device, _int_view(T, dtype)[1], skew)
    middle = whole[g:g + n].view(shape)
    if rec is not None:
        rec.update(whole=whole, middle=middle)
    return whole, middle


def guarded_input(T, array, fill=None, guard_bytes=GUARD, device="cuda", skew=None, name=None):
    """The same layout for an input: `array` (numpy, or a tensor on any device: bf16 has no numpy type) copied between two bands
    of `fill` - the dtype's sentinel (NaN bits for floats) unless given; for a uint8 image a byte.  -> (whole, middle)."""
    src = array.contiguous() if isinstance(array, T.Tensor) else T.from_numpy(np.ascontiguousarray(array))
    if fill is None:
        fill = _int_view(T, src.dtype)[1]
    skew, rec = _skew_of(skew, name, src.dtype, "in")
    whole, g = _layout(T, src.numel(), src.dtype, guard_bytes, device, fill, skew)
    middle = whole[g:g + src.numel()].view(src.shape)
    middle.copy_(src)
    if rec is not None:
        rec.update(whole=whole, middle=middle)
    return whole, middle


def device_input(T, array, name=None):
    """An input of a test that does not guard its inputs: the plain device copy of `array`, as such a test always made it - but
    under a Placement the guarded, placed input named `name` (float64 and uint16, which have no sentinel of their own, travel as
    int64 / int16 bits).  A copy without a name is no operand of an entry - such tests compare with it - and stays plain."""
    if array is None:
        return None
    a = np.ascontiguousarray(array)
    if placement is None or name is None:
        return T.from_numpy(a).cuda()
    bits = {"f8": np.int64, "u2": np.int16}.get(a.dtype.str[1:])
    middle = guarded_input(T, a.view(bits) if bits else a, name=name)[1]
    return middle.view(T.from_numpy(a.reshape(-1)[:0]).dtype) if bits else middle


def spread(array, stride, fill=None):
    """A strided operand as ONE dense numpy array to hand to guarded_input(): the leading axis of `array` (frames, or rows)
    `stride` elements apart instead of dense - stride at least the elements of one frame - with the gaps, and nothing after the
    last frame, holding `fill`: the dtype's sentinel (NaN bits for floats) unless given, for a uint8 image a byte.
    -> the flat array of (frames - 1) * stride + frame elements; frame f starts at element f * stride."""
    a = np.ascontiguousarray(array)
    per = int(np.prod(a.shape[1:], dtype=np.int64))
    if stride < per:
        raise ValueError(f"a stride of {stride} elements does not hold a frame of {per}")
    bits = {4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.itemsize]
    if fill is None:
        fill = {4: SENTINEL, 8: SENTINEL64, 2: SENTINEL_BF16, 1: SENTINEL_U8}[a.itemsize]
    flat = np.full((a.shape[0] - 1) * stride + per, fill, bits)
    for f in range(a.shape[0]):
        flat[f * stride:f * stride + per] = a[f].reshape(-1).view(bits)
    return flat.view(a.dtype)


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


def dirty(T, nbytes, byte, device="cuda", skew=None):
    """A workspace of exactly nbytes filled with `byte`; under a Placement (or with a skew of its own) it starts that many bytes
    past a 256-byte boundary, and is still exactly nbytes long."""
    skew, rec = _skew_of(skew, "workspace", T.uint8, "ws")
    if skew == 0 or int(nbytes) == 0:
        ws = T.full((int(nbytes),), int(byte), dtype=T.uint8, device=device)
    else:
        whole = T.full((int(nbytes) + 512,), int(byte), dtype=T.uint8, device=device)
        off = (skew - whole.data_ptr()) % 256
        ws = whole[off:off + int(nbytes)]
        assert ws.data_ptr() % 256 == skew
    if rec is not None:
        rec.update(whole=ws, middle=ws)
    return ws
