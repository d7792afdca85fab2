#!/usr/bin/env python3
"""Golden vectors at descriptor width 256, produced like make_golden.py by RUNNING the reference's own code in the authoring
container: DescriptorRefiner(384, 384, 256, 4) and the five matchers on 256-wide descriptors.  Inputs and weights are
regenerated from seeds by the tests (tests/d256_cases.py, tests/synth.py); d256.npz stores the reference's outputs only.

Usage:  python tests/golden/make_golden_d256.py
"""
from __future__ import annotations

import numpy as np
import torch

import make_golden as mg
from make_golden import t
import d256_cases as cases  # (path set up by make_golden)

TIE_MARGIN = 4e-6       # below this a top-1 / top-2 gap may re-associate under another summation order


def main():
    M = mg._import_reference()
    out = {}
    # ---- refiner: the reference's module at output_dim 256, on free rows and on one gathered frame
    ref = M["ref"].DescriptorRefiner(384, 384, cases.D, 4).eval()
    ref.load_state_dict({k: t(v) for k, v in cases.refiner_state().items()})
    g = cases.GATHER_GRID
    bb = mg.make_backbone(M["bb"], g)
    feat = mg.bn_features(M["bb"], cases.gather_tokens(), g)
    with torch.no_grad():
        out["mlp_out"] = ref(t(cases.mlp_rows())[None])[0].numpy()
        out["gather_desc"] = ref(bb.extract_at_keypoints(feat, t(cases.gather_keypoints())))[0].numpy()
    assert out["mlp_out"].shape == (70, cases.D) and out["gather_desc"].shape == (cases.GATHER_K, cases.D)
    # ---- matchers
    mq = M["vms"].SequenceMatcher.match_with_quality
    for tag, (seed, n, m, dup) in cases.PAIRS.items():
        d1, d2, s1, s2, i1, i2 = cases.pair(seed, n, m, dup)
        assert d1.shape == (n, cases.D) and d2.shape == (m, cases.D) and dup > 0
        out[f"{tag}_rowgap"], out[f"{tag}_colgap"] = mg.gaps(d1, d2)
        assert out[f"{tag}_rowgap"] > TIE_MARGIN and out[f"{tag}_colgap"] > TIE_MARGIN, tag
        for rtag, kw in cases.RUNS.items():
            mt, q = mq(d1, d2, s1, s2, **kw(i1, i2))
            assert mt.dtype == np.int64 and q.dtype == np.float32
            out[f"{tag}_{rtag}_matches"], out[f"{tag}_{rtag}_quality"] = mt.astype(np.int16), q
        m2 = M["vm"].MatchVisualizer.find_matches(None, d1, d2, ratio_thresh=cases.M2_RATIO)
        out[f"{tag}_m2_ij"] = np.array([(a, b) for a, b, _ in m2], np.int16).reshape(-1, 2)
        out[f"{tag}_m2_sim"] = np.array([c for _, _, c in m2], np.float32)
        m4, dist = M["tdq"].DescriptorQualityTester.find_mutual_nearest_neighbors(None, d1, d2, cases.M4_RATIO)
        out[f"{tag}_m4_matches"], out[f"{tag}_m4_dist"] = m4.astype(np.int16), dist.astype(np.float32)
        # M5 (test_tracking.py:159-161), restated as make_golden.py does: three numpy calls inside a longer method
        sim = d1 @ d2.T
        out[f"{tag}_m5_count"] = int((sim.max(axis=1) > cases.M5_THRESHOLD).sum())
    fm = M["train"].SemanticSLAMTrainer._find_matches
    b1, b2 = zip(*[cases.pair(seed, 200, 200, 10, noise)[:2] for seed, noise in cases.M3_CASES])
    for a, b in zip(b1, b2):
        assert min(mg.gaps(a, b)) > TIE_MARGIN
    with torch.no_grad():
        out["m3_matches"] = fm(None, t(np.stack(b1)), t(np.stack(b2))).numpy().astype(np.int16)
    mg.save("d256", **out)


if __name__ == "__main__":
    main()
