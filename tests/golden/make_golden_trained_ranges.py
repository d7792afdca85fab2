#!/usr/bin/env python3
"""Generate tests/golden/trained_ranges.npz by RUNNING the reference's own modules (pattern of make_golden.py; runs only where
the reference is present).  Outputs only: every input is regenerated from the seeds of tests/synth.py and tests/stress_cases.py.

  * models.descriptor_refiner.DescriptorRefiner at num_layers 2, 3, 5, 10 (0, 1, 3, 8 residual blocks) with
    synth.refiner_state(3, n_blocks=depth), on the first 40 rows of stress_cases.refiner_rows: fp32, and as .double()
  * models.keypoint_selector.KeypointSelector with stress_cases.steep_selector(0, 256, 60 | 200) on the oracle's batch-normed
    synth.tokens(48, 28, 2): the saliency map in fp32 and in float64

The reference's select_keypoints is deliberately NOT recorded on these maps: torch.topk among hundreds of cells at exactly
1.0f is implementation-defined, so even the keypoint set is no property of the reference there.

Usage:  python tests/golden/make_golden_trained_ranges.py        (writes next to this file)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import torch  # noqa: E402

import stress_cases  # noqa: E402
import synth  # noqa: E402
from make_golden import _import_reference, save, t  # noqa: E402
from oracle import ora  # noqa: E402

torch.set_num_threads(4)

DEPTHS = (0, 1, 3, 8)
SCALES = (60, 200)
ROWS = 40


def main():
    M = _import_reference()
    out = {}
    x = stress_cases.refiner_rows(ROWS)
    for depth in DEPTHS:
        ref = M["ref"].DescriptorRefiner(synth.C_FEAT, 384, 128, depth + 2).eval()
        ref.load_state_dict({k: t(v) for k, v in synth.refiner_state(3, n_blocks=depth).items()})
        with torch.no_grad():
            out[f"refine_d{depth}_f32"] = ref(t(x)[None])[0].numpy()
            out[f"refine_d{depth}_f64"] = ref.double()(t(x).double()[None])[0].numpy()
    feat = ora.bn_tokens(synth.tokens(48, 28, 2))[0].reshape(2, 28, 28, 384)
    for scale in SCALES:
        sel = M["sel"].KeypointSelector(synth.C_FEAT, 256).eval()
        sel.load_state_dict({k: t(v) for k, v in stress_cases.steep_selector(0, 256, scale).items()})
        with torch.no_grad():
            out[f"steep{scale}_f32"] = sel(t(feat))[..., 0].numpy()
            out[f"steep{scale}_f64"] = sel.double()(t(feat).double())[..., 0].numpy()
    save("trained_ranges", depths=np.array(DEPTHS), scales=np.array(SCALES), rows=ROWS, **out)


if __name__ == "__main__":
    main()
