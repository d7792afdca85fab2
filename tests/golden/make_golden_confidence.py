#!/usr/bin/env python3
"""Golden vectors of the keypoint confidence head, produced like make_golden.py by RUNNING the reference's own code in the
authoring container: models/uncertainty_estimator.py, UncertaintyEstimator - forward in float32 and in float64, the three outputs
of filter_keypoints_by_confidence at four thresholds, and the two calibration losses.  Heads and inputs are regenerated from seeds
by the tests (tests/confidence_cases.py); confidence.npz stores the reference's outputs only.

Usage:  python tests/golden/make_golden_confidence.py
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import make_golden as mg
from make_golden import t
import confidence_cases as cases  # (path set up by make_golden)


def main():
    sys.path.insert(0, mg.REF)
    import models.uncertainty_estimator as m_unc
    out = {}
    err = cases.error_array()
    for name, (d, _, _) in cases.HEADS.items():
        head = m_unc.UncertaintyEstimator(cases.DINO_DIM, d, cases.HIDDEN_DIM).eval()
        head.load_state_dict({k: t(v) for k, v in cases.head_state(name).items()})
        x, desc, kp = cases.head_inputs(name)
        with torch.no_grad():
            conf = head(t(x), t(desc))
            out[f"{name}_conf"] = conf.numpy()
            out[f"{name}_conf_f64"] = head.double()(t(x).double(), t(desc).double()).numpy()
            head.float()
            out[f"{name}_calibration_loss"] = head.compute_calibration_loss(conf, t(err)).numpy()
            out[f"{name}_expected_error_loss"] = head.compute_expected_error_loss(conf, t(err)).numpy()
            assert conf.shape == (cases.B, cases.N, 1) and conf.dtype == torch.float32
            c = conf[..., 0].numpy()
            print(f"{name}: confidence {c.min():.7g} .. {c.max():.7g}, max |f32 - f64| {np.abs(c - out[f'{name}_conf_f64'][..., 0]).max():.3g}")
            if name != cases.FILTER_HEAD:
                continue
            srt = np.sort(c, axis=1)
            assert (srt[:, -1] > srt[:, -2]).all(), "every frame's maximum must be unique: the reference's arg-max picks any of equal ones"
            for tag, thr in cases.thresholds(c).items():
                fk, fd, fc = head.filter_keypoints_by_confidence(t(kp), t(desc), conf.clone(), threshold=float(thr))
                out[f"filter_{tag}_threshold"] = np.float32(thr)
                out[f"filter_{tag}_keypoints"], out[f"filter_{tag}_descriptors"], out[f"filter_{tag}_confidence"] = fk.numpy(), fd.numpy(), fc.numpy()
                print(f"  filter {tag}: threshold {float(thr):.7g}, kept {[int((c[b] >= thr).sum()) for b in range(cases.B)]}, padded to {fk.shape[1]}")
            assert out["filter_none_keypoints"].shape[1] == 1
    mg.save("confidence", **out)


if __name__ == "__main__":
    main()
