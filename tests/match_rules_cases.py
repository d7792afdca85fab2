"""What tests/test_match_rules_api.py (CPU) and tests/test_gpu_match_rules.py share: the three rules with their threshold sets,
the oracle's answer for one pair under one rule, and the oracle-extracted frames the input condition is checked on.

The thresholds are chosen for the synthetic sequence (synth.token_sequence, K = 500), on which each rule's middle threshold keeps
some rows and rejects others - the committed goldens do not discriminate (M2 at 0.8 keeps every mutual pair of them).  The input
condition is asserted on the ORACLE alone (test_match_rules_api.py), so the GPU tests cannot pass on rules that select nothing."""
import numpy as np

import synth
from oracle import ora

RATIO, MNN_RATIO, TRACKED = "ratio", "mnn_ratio", "tracked"                   # MatchRule's constructors
THRESHOLDS = {MNN_RATIO: (0.6, 0.7, 0.9), RATIO: (0.8, 1.0, 1.6), TRACKED: (0.8, 0.98, 0.99)}
LOOSEST = {MNN_RATIO: 0.9, RATIO: 0.8, TRACKED: 0.8}                          # the threshold of each set that keeps most
MIDDLE = {name: t[1] for name, t in THRESHOLDS.items()}
CONDITION_PAIRS = ((0, 1), (0, 2), (0, 5))
N_COND, K = 6, 500


def oracle_rule(name: str, d1: np.ndarray, d2: np.ndarray, param: float):
    """(matches (c, 2) int64 ascending in idx1, value (c,) fp32) of one pair under one rule, by oracle/ora.py."""
    if name == RATIO:
        m2 = ora.find_matches_m2(d1, d2, param)
        return (np.array([(a, b) for a, b, _ in m2], np.int64).reshape(-1, 2), np.array([c for *_, c in m2], np.float32))
    if name == MNN_RATIO:
        m4, dist = ora.find_mnn_m4(d1, d2, param)
        return m4, np.ascontiguousarray(dist, np.float32)
    assert name == TRACKED
    nn12, s12, _, _ = ora.sim_argmax(d1, d2)
    idx = np.flatnonzero(s12 > np.float32(param))                             # test/test_tracking.py:160-161
    return np.stack([idx, nn12[idx]], axis=1).astype(np.int64), s12[idx]


def oracle_descriptors(n_frames: int = N_COND) -> np.ndarray:
    """(n_frames, K, 128): the synthetic sequence extracted by the oracle alone (what smoke() compares the HIP path with)."""
    toks = synth.token_sequence(n_frames, 28)
    feat = ora.bn_tokens(toks)[0].reshape(n_frames, 28, 28, 384)
    kp, _, _, st = ora.select_keypoints(ora.selector_saliency(feat, synth.selector_state(0)), K)
    assert not st.any()
    return ora.refine(ora.gather(feat, kp), synth.refiner_state(0))
