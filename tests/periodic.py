"""Operands no host can hold: a bank of n frames built ON THE DEVICE from a few distinct frames, and the comparison of an output
of n frames with the few expectations that go with them.  Nothing of the operand's size crosses the bus or exists in host memory.

P = 7 base frames repeat: frame i is base frame i % 7.  7 is coprime to the eight XCDs and to every power of two, so an address
that wraps by 2^31 or 2^32 bytes lands on another phase of the period.  The frames at MARKED positions are frames of their own
(slots P, P + 1, ... of the distinct set), with their own expectation: frame 0, the frame holding byte 2^31 of the operand, the
last frame of a launch group and the first of the next, the last frame of all - without them a kernel that skipped or repeated
the far end could pass by periodicity alone.  Expectations come from the CPU oracle on the P + len(marks) distinct frames.

The comparison runs where the output lives, over the whole output, on integer bits; a failure names the first wrong frame and
the offset in bytes of its first wrong byte.  Works on CPU tensors as well (tests/test_size_limits_cpu.py).
"""
import torch

P = 7
FAR = 1 << 31
CHUNK_BYTES = 256 << 20          # the comparison's and the builder's working set


def marks(n, frame_bytes, group=None, far_byte=FAR):
    """The marked positions of an n-frame operand of frame_bytes per frame, ascending and distinct: 0, the frame holding byte
    `far_byte` (if the operand reaches it), the last frame of every launch group of `group` frames that has a successor and that
    successor (at most the first two cuts), and n - 1."""
    m = {0, n - 1}
    if far_byte is not None and far_byte < n * frame_bytes:
        m.add(far_byte // frame_bytes)
    if group is not None:
        for cut in (group, 2 * group):
            if 0 < cut < n:
                m.update((cut - 1, cut))
    return sorted(m)


def slots(n, marked, device="cpu"):
    """int64 tensor (n,): the slot of the distinct set that frame i holds - i % P, or P + j for the j-th marked position."""
    s = torch.arange(n, dtype=torch.int64, device=device) % P
    if len(marked):
        s[torch.as_tensor(list(marked), dtype=torch.int64, device=device)] = P + torch.arange(len(marked), dtype=torch.int64, device=device)
    return s


def n_distinct(marked):
    return P + len(marked)


def build(distinct, n, marked, out=None):
    """The operand: (n, *frame) of distinct's dtype on distinct's device, frame i = distinct[slot(i)].  `out`: a tensor of that
    shape to fill instead (a view at an odd base, for instance).  Filled in chunks: no index tensor of the operand's size."""
    assert distinct.shape[0] == n_distinct(marked), (distinct.shape, len(marked))
    if out is None:
        out = torch.empty((n,) + tuple(distinct.shape[1:]), dtype=distinct.dtype, device=distinct.device)
    assert out.shape[0] == n and out.shape[1:] == distinct.shape[1:] and out.dtype == distinct.dtype
    s = slots(n, marked, distinct.device)
    fb = max(1, distinct[0].numel() * distinct.element_size())
    step = max(1, CHUNK_BYTES // fb)
    for a in range(0, n, step):
        out[a:a + step] = distinct[s[a:a + step]]
    return out


def _bits(t):
    """The tensor's elements as integers of the same size (a NaN equals itself, -0.0 differs from 0.0)."""
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t if t.dtype == idt else t.view(idt)


def mismatches(out, expected, marked):
    """(frames, first): the ascending list of the frames of `out` (n, *frame) that differ from expected[slot(frame)] in any bit, and
    for the first of them (frame, byte offset of the first wrong byte within the whole output) - None if there is none."""
    n = out.shape[0]
    assert expected.shape[0] == n_distinct(marked) and expected.shape[1:] == out.shape[1:] and expected.dtype == out.dtype, \
        (out.shape, out.dtype, expected.shape, expected.dtype)
    assert out.is_contiguous()
    exp = _bits(expected.to(out.device).contiguous()).reshape(expected.shape[0], -1)
    got = _bits(out).reshape(n, -1)
    s = slots(n, marked, out.device)
    fb = max(1, got.shape[1] * got.element_size())
    step = max(1, CHUNK_BYTES // fb)
    bad = []
    for a in range(0, n, step):
        wrong = (got[a:a + step] != exp[s[a:a + step]]).any(dim=1)
        if bool(wrong.any()):
            bad += (torch.nonzero(wrong).flatten() + a).tolist()
    if not bad:
        return [], None
    f = bad[0]
    raw_g, raw_e = got[f].contiguous().view(torch.uint8), exp[int(s[f])].contiguous().view(torch.uint8)
    within = int(torch.nonzero(raw_g != raw_e).flatten()[0])
    return bad, (f, f * fb + within)


def report(out, expected, marked, what=""):
    """'0 mismatching frames of N' - or the assertion that names the first wrong frame and its offset in bytes."""
    bad, first = mismatches(out, expected, marked)
    n = out.shape[0]
    if bad:
        f, off = first
        raise AssertionError(f"{what}: {len(bad)} mismatching frames of {n}; the first is frame {f} (slot {int(slots(n, marked)[f])}"
                             f"{', marked' if f in set(marked) else ''}), first wrong byte at offset {off} of the output; "
                             f"frames {bad[:8]}{'...' if len(bad) > 8 else ''}")
    line = f"{what}: 0 mismatching frames of {n}"
    print(line)
    return line
