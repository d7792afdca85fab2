"""The named launch forms of the bf16 ViT, as far as a machine without a GPU can see them: the header's constants and entries
against sslam_amd.lib and the built library, the host-side workspace rule of sslam_vit_workspace_bytes_form, and the argument
checks of SequencePipeline(vit_form=) and DinoBackbone(vit_form=), which must raise before anything touches a device."""
import ctypes
import os
import re

import pytest
import torch

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sslam_vit_workspace_bytes_form", "sslam_vit_forward_form", "sslam_vit_forward_patches_form")
SIZES = (16, 48, 64, 208, 224, 448, 640, 960)


def _header():
    return open(os.path.join(ROOT, "include", "sslam_hip.h")).read()


def test_form_constants_equal_the_header():
    from sslam_amd import lib
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(SSLAM_VIT_\w+)\s+(\d+)\s*$", _header(), flags=re.M)}
    assert defs == {"SSLAM_VIT_FORM_THROUGHPUT": lib.VIT_FORM_THROUGHPUT, "SSLAM_VIT_FORM_SMALL": lib.VIT_FORM_SMALL,
                    "SSLAM_VIT_FORM_FEW_FRAME": lib.VIT_FORM_FEW_FRAME, "SSLAM_VIT_FEW_FRAME_MAX_FRAMES": lib.VIT_FEW_FRAME_MAX_FRAMES}
    assert lib.VIT_FEW_FRAME_MAX_FRAMES == 8
    assert len({lib.VIT_FORM_THROUGHPUT, lib.VIT_FORM_SMALL, lib.VIT_FORM_FEW_FRAME}) == 3


def test_named_form_entries_are_declared_exported_and_listed():
    from sslam_amd import lib
    hdr = _header()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/sslam_hip.h"
        assert name in lib.EXPORTS
        assert hasattr(so, name), f"{name} is not exported by the library"
    L = lib.lib()
    assert L.sslam_vit_workspace_bytes_form.restype is ctypes.c_longlong
    assert len(L.sslam_vit_forward_form.argtypes) == len(L.sslam_vit_forward.argtypes) + 1
    assert len(L.sslam_vit_forward_patches_form.argtypes) == len(L.sslam_vit_forward_patches.argtypes) + 1


@pytest.mark.parametrize("size", SIZES)
def test_workspace_bytes_by_form(size):
    from sslam_amd import lib
    few = [lib.vit_workspace_bytes(n, size, lib.VIT_FORM_FEW_FRAME) for n in range(1, 9)]
    assert all(b >= a for a, b in zip(few, few[1:])), few              # a buffer for a batch serves every shorter launch
    for n in range(1, 9):
        base = lib.vit_workspace_bytes(n, size)
        assert lib.vit_workspace_bytes(n, size, None) == base
        assert lib.vit_workspace_bytes(n, size, lib.VIT_FORM_SMALL) == base
        assert lib.vit_workspace_bytes(n, size, lib.VIT_FORM_THROUGHPUT) == base
        assert few[n - 1] >= base
        assert few[n - 1] > base, "the few-frame form keeps attention partials"
    for n in (9, 40):                                                   # the named old forms are legal at any frame count
        assert lib.vit_workspace_bytes(n, size, lib.VIT_FORM_SMALL) == lib.vit_workspace_bytes(n, size)
        assert lib.vit_workspace_bytes(n, size, lib.VIT_FORM_THROUGHPUT) == lib.vit_workspace_bytes(n, size)
    with pytest.raises(ValueError):
        lib.vit_workspace_bytes(9, size, lib.VIT_FORM_FEW_FRAME)
    for bogus in (3, -1, 99):
        with pytest.raises(ValueError):
            lib.vit_workspace_bytes(1, size, bogus)


class _Stub(torch.nn.Module):
    """Any module with embed_dim = 384: nothing is built, converted or fetched by the constructors under test."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.embed_dim = 384


@pytest.mark.parametrize("with_vit", [False, True])
def test_pipeline_checks_vit_form_before_any_device_work(with_vit):
    from sslam_amd.pipeline import ExtractorConfig, SequencePipeline
    kw = dict(vit=_Stub()) if with_vit else {}
    args = (ExtractorConfig(), synth.selector_state(0), synth.refiner_state(0))
    with pytest.raises(ValueError, match="vit_form"):
        SequencePipeline(*args, device="cuda", vit_form="bogus", **kw)
    with pytest.raises(ValueError, match="vit_form"):
        SequencePipeline(*args, device="cuda", vit_form="few_frame", vit_precision="fp32", **kw)
    with pytest.raises(ValueError, match="vit_form"):
        SequencePipeline(*args, device="cuda", vit_form="bogus", vit_precision="fp32", **kw)


def test_dino_backbone_vit_form_argument():
    from models.dino_backbone import DinoBackbone
    with pytest.raises(ValueError, match="vit_form"):
        DinoBackbone(dino=_Stub(), vit_form="few_frame")                          # default precision: fp32
    with pytest.raises(ValueError, match="vit_form"):
        DinoBackbone(dino=_Stub(), vit_precision="eager", vit_form="few_frame")
    for prec in ("bf16", "fp32", "eager"):
        with pytest.raises(ValueError, match="vit_form"):
            DinoBackbone(dino=_Stub(), vit_precision=prec, vit_form="bogus")
    bb = DinoBackbone(dino=_Stub(), vit_precision="bf16", vit_form="few_frame")
    assert bb.vit_form == "few_frame" and bb.vit_precision == "bf16"
    plain = DinoBackbone(dino=_Stub())
    assert plain.vit_form is None and DinoBackbone(dino=_Stub(), vit_precision="bf16").vit_form is None
    assert list(bb.state_dict().keys()) == list(plain.state_dict().keys())
    # the reference's positional arguments are where they were
    pos = DinoBackbone("vit_small_patch16_dinov3.lvd1689m", 224, True, _Stub(), "bf16", "few_frame")
    assert (pos.input_size, pos.vit_precision, pos.vit_form) == (224, "bf16", "few_frame")


def test_forward_features_refuses_an_unknown_form_before_the_device():
    from sslam_amd.vit_hip import HipViT
    hv = HipViT.__new__(HipViT)                      # no packing, no device: the check comes first
    with pytest.raises(ValueError, match="form"):
        hv.forward_features(torch.zeros(1, 3, 16, 16), form="bogus")
