"""The pair-list matcher (sslam_sim_argmax_pairs / sslam_match_finalize_pairs) and the multi-spacing FrameStepper, as far as a
machine without a GPU can see them: the two entries against the header, the built library and sslam_amd.lib; the host-side
argument checks of the C entries, which return before anything is launched; and the ValueErrors of lib.sim_argmax_pairs,
SequencePipeline.match_pairs and FrameStepper(spacings=...), which must come before any device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sslam_sim_argmax_pairs", "sslam_match_finalize_pairs")
E_INVALID = -1
# never dereferenced: every call below is refused by the entry's own checks, which come before the launch
GOOD, GOOD2, ODD = 0x10000, 0x20000, 0x10004


def _header():
    return open(os.path.join(ROOT, "include", "sslam_hip.h")).read()


def test_pair_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = _header()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/sslam_hip.h"
        assert name in lib.EXPORTS
        assert hasattr(so, name), f"{name} is not exported by the library"
    L = lib.lib()
    # the pair-list entries take the bank once, the two lists and the bank's frame count: their argument counts follow
    assert len(L.sslam_sim_argmax_pairs.argtypes) == 15
    assert len(L.sslam_match_finalize_pairs.argtypes) == 20
    assert L.sslam_version() > 300, "a new entry raises the version"


def _sim(L, bank=GOOD, stride=512, n_bank=4, K=4, first=GOOD2, second=GOOD2, n_pairs=2, nn12=GOOD, nn21=GOOD, ws=None):
    return L.sslam_sim_argmax_pairs(bank, stride, n_bank, K, first, second, n_pairs, nn12, None, nn21, None, None, ws, 0, None)


def _fin(L, nn12=GOOD, s12=GOOD, nn21=GOOD, K=4, n_bank=4, first=GOOD2, second=GOOD2, n_pairs=2, scores=GOOD, matches=GOOD,
         quality=GOOD, count=GOOD):
    f = ctypes.c_float
    return L.sslam_match_finalize_pairs(nn12, s12, nn21, K, n_bank, first, second, n_pairs, scores, K, None, f(0.7), f(0.3), f(0.5),
                                        f(0.7), f(0.15), matches, quality, count, None)


def test_c_entries_refuse_bad_arguments_without_a_device():
    from sslam_amd import lib
    L = lib.lib()
    before = lib.launch_count()
    for kw in (dict(bank=None), dict(first=None), dict(second=None), dict(nn12=None), dict(nn21=None),
               dict(n_pairs=0), dict(n_pairs=-3), dict(K=0), dict(n_bank=0),
               dict(bank=ODD), dict(stride=510), dict(first=GOOD2 + 2), dict(second=GOOD2 + 1), dict(ws=GOOD + 4)):
        assert _sim(L, **kw) == E_INVALID, kw
    for kw in (dict(nn12=None), dict(s12=None), dict(nn21=None), dict(first=None), dict(second=None), dict(scores=None),
               dict(matches=None), dict(quality=None), dict(count=None),
               dict(n_pairs=0), dict(K=0), dict(n_bank=0), dict(first=GOOD2 + 2), dict(second=GOOD2 + 1)):
        assert _fin(L, **kw) == E_INVALID, kw
    assert lib.launch_count() == before, "a refused call launches nothing"
    # the workspace rule is the strided entry's: nothing below 16 pairs, one 64-bit key per (pair, candidate) from there
    assert L.sslam_sim_argmax_workspace_bytes(500, 5) == 0
    assert L.sslam_sim_argmax_workspace_bytes(500, 84) == 84 * 500 * 8


def _lists(*rows, dtype=torch.int32):
    return [torch.tensor(r, dtype=dtype) for r in rows]


def test_binding_checks_the_pair_lists_before_any_device_work():
    from sslam_amd import lib
    bank = torch.zeros((3, 4, lib.D_OUT))                      # host tensors: a check that let them through would fail on the device
    before = lib.launch_count()
    with pytest.raises(ValueError, match="int32"):
        lib.sim_argmax_pairs(bank, *_lists([0, 1], [1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="int32"):
        lib.sim_argmax_pairs(bank, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int64))
    with pytest.raises(ValueError, match="unequal"):
        lib.sim_argmax_pairs(bank, *_lists([0, 1], [1, 2, 0]))
    with pytest.raises(ValueError, match="1-D"):
        lib.sim_argmax_pairs(bank, *_lists([[0, 1]], [[1, 2]]))
    with pytest.raises(ValueError, match="empty"):
        lib.sim_argmax_pairs(bank, *_lists([], []))
    with pytest.raises(ValueError, match="bank"):
        lib.sim_argmax_pairs(torch.zeros((3, 4, 64)), *_lists([0], [1]))
    with pytest.raises(ValueError, match="bank"):
        lib.sim_argmax_pairs(bank.double(), *_lists([0], [1]))
    with pytest.raises(ValueError):                             # well-formed host tensors: refused for where they live
        lib.sim_argmax_pairs(bank, *_lists([0], [1]))
    nn = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        lib.match_finalize_pairs(nn, nn.float(), nn, *_lists([0, 1], [1, 2], dtype=torch.int64), torch.zeros((3, 4)), None,
                                 0.7, 0.3, 0.5, 0.7, 0.15)
    with pytest.raises(ValueError, match="unequal"):
        lib.match_finalize_pairs(nn, nn.float(), nn, *_lists([0, 1], [1]), torch.zeros((3, 4)), None, 0.7, 0.3, 0.5, 0.7, 0.15)
    with pytest.raises(ValueError, match="intensity"):
        lib.match_finalize_pairs(nn, nn.float(), nn, *_lists([0, 1], [1, 2]), torch.zeros((3, 4)), torch.zeros((2, 4)),
                                 0.7, 0.3, 0.5, 0.7, 0.15)
    assert lib.launch_count() == before


def test_match_pairs_checks_its_lists_before_any_device_work():
    from sslam_amd import lib
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    pipe = SequencePipeline.__new__(SequencePipeline)          # no packing, no device: the checks come first
    pipe.cfg = ExtractorConfig()
    desc, scores = torch.zeros((3, 4, lib.D_OUT)), torch.zeros((3, 4))
    before = lib.launch_count()
    first64, second64 = _lists([0, 1], [1, 2], dtype=torch.int64)
    with pytest.raises(ValueError, match="int32"):
        pipe.match_pairs(desc, scores, first=first64, second=second64)
    with pytest.raises(ValueError, match="unequal"):
        pipe.match_pairs(desc, scores, first=[0, 1], second=[1, 2, 0])
    with pytest.raises(ValueError, match="1-D"):
        pipe.match_pairs(desc, scores, first=[[0, 1]], second=[[1, 2]])
    with pytest.raises(ValueError, match="32-bit integers"):
        pipe.match_pairs(desc, scores, first=[0.5, 1.0], second=[1, 2])
    with pytest.raises(ValueError, match="32-bit integers"):
        pipe.match_pairs(desc, scores, first=[0, 2 ** 40], second=[1, 2])
    with pytest.raises(ValueError, match="both pair lists"):
        pipe.match_pairs(desc, scores, first=[0, 1])
    with pytest.raises(ValueError, match="scores"):
        pipe.match_pairs(desc, torch.zeros((2, 4)), first=[0], second=[1])
    assert lib.launch_count() == before


@pytest.mark.parametrize("bad", [(0,), (1, 0, 5), (-1, 2), (1, -5), (1, 1), (5, 1, 5), (), (1.5,), (True,), "15", 5, [1, "2"]])
def test_frame_stepper_refuses_bad_spacings_before_any_allocation(bad):
    from sslam_amd.online import FrameStepper
    with pytest.raises(ValueError, match="spacings"):
        FrameStepper(None, 480, 640, use_graph=False, tokens_in=True, spacings=bad)     # no pipeline is ever looked at


def test_frame_stepper_keeps_its_signature():
    from sslam_amd.online import FrameStepper
    params = list(inspect.signature(FrameStepper.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "pipe", "height", "width", "use_graph", "tokens_in", "spacings"]
    assert [p.default for p in params[4:]] == [True, False, None]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)
    assert list(inspect.signature(FrameStepper.step).parameters) == ["self", "image_u8", "tokens"]
