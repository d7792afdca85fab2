"""sslam_amd.readback.Readback: what goes in comes back bit for bit, under its name, in its shape and the dtype asked for, through ONE
device-to-host transfer - for every dtype it takes, at the values where a float64 carrier could be thought to lose something."""
import numpy as np
import pytest
import torch

from sslam_amd.readback import Readback

I32, F32 = np.iinfo(np.int32), np.finfo(np.float32)
CASES = {
    "int32": (np.array([I32.min, -1, 0, 1, I32.max], dtype=np.int32), np.int32),
    "int64": (np.array([-(2 ** 53 - 1), -2 ** 31 - 1, 0, 2 ** 31, 2 ** 53 - 1], dtype=np.int64), np.int64),
    "float32": (np.array([F32.smallest_subnormal, -F32.smallest_subnormal, F32.tiny, F32.max, -F32.max, np.inf, -np.inf, np.nan, -0.0, 0.1],
                         dtype=np.float32), np.float32),
    "float64": (np.array([np.finfo(np.float64).smallest_subnormal, np.finfo(np.float64).max, -np.inf, np.nan, -0.0, 1.0 / 3.0]), np.float64),
    "bool": (np.array([True, False, False, True]), np.bool_),
    "empty": (np.zeros((0,), dtype=np.float64), np.float64),
    "empty_rows": (np.zeros((0, 21), dtype=np.int32), np.int32),
    "three_d": (np.arange(2 * 3 * 4, dtype=np.int32).reshape(2, 3, 4) - 7, np.int32),
    "scalar": (np.array(-5, dtype=np.int32), np.int32),
    "widened": (np.array([3, -4], dtype=np.int32), np.int64),           # counts come back as int64 where the caller asks for it
}


def round_trip(device):
    reads, real = [], torch.Tensor.cpu
    rb = Readback()
    for name, (a, dtype) in CASES.items():
        rb.add(name, torch.from_numpy(a).to(device), dtype)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch.Tensor, "cpu", lambda t, *args, **kw: (reads.append(t.numel()), real(t, *args, **kw))[1])
        got = rb.fetch()
    assert len(reads) == 1 and reads[0] == sum(a.size for a, _ in CASES.values()), reads
    assert list(got) == list(CASES)
    for name, (a, dtype) in CASES.items():
        g = got[name]
        assert isinstance(g, np.ndarray) and g.dtype == np.dtype(dtype) and g.shape == a.shape, (name, g.dtype, g.shape)
        assert g.tobytes() == a.astype(dtype).tobytes(), (name, g, a)
        assert g.flags.owndata, name
    return got


def test_round_trips_are_bit_exact_and_read_once():
    got = round_trip("cpu")
    # every array owns its memory: none is a view of the carrier or of another piece
    for a in got.values():
        for b in got.values():
            assert a is b or a.size == 0 or not np.shares_memory(a, b)
    got["int32"][:] = 0
    assert got["widened"].tolist() == [3, -4]


def test_rows_are_cut_to_a_count_the_device_holds():
    rb, xyz = Readback(), torch.arange(15, dtype=torch.float64).reshape(5, 3)
    rb.add("n", torch.tensor([2], dtype=torch.int32), np.int64)
    rb.add("xyz", xyz, np.float64, rows="n")
    rb.add("id", torch.arange(5, dtype=torch.int32), np.int32, rows="n")
    rb.add("after", torch.tensor([7.5]), np.float64)
    got = rb.fetch()
    assert got["xyz"].tobytes() == xyz[:2].numpy().tobytes() and got["xyz"].shape == (2, 3) and got["xyz"].flags.owndata
    assert got["id"].tolist() == [0, 1] and got["after"].tolist() == [7.5] and list(got) == ["n", "xyz", "id", "after"]
    with pytest.raises(ValueError, match="no piece"):
        rb.add("late", xyz, np.float64, rows="missing")


def test_refusals():
    rb = Readback()
    rb.add("a", torch.zeros(3), np.float64)
    with pytest.raises(ValueError, match="taken"):
        rb.add("a", torch.zeros(2), np.float64)
    for bad in (torch.zeros(2, dtype=torch.float16), torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.int16), np.zeros(2), None):
        with pytest.raises(ValueError, match="tensor expected"):
            rb.add("b", bad, np.float64)
    assert list(rb.fetch()) == ["a"]


@pytest.mark.gpu
def test_round_trips_from_the_device():
    round_trip("cuda:0")
