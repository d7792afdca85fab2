"""Batched extraction + matching pipeline on one MI355X: the streaming counterpart of the reference's per-pair
harness (SequenceMatcher.extract + process_spacing, semantic-slam/visualize_matches_sequence.py:69-104, 272-357).

Differences from the reference harness, by design: every frame is extracted ONCE and its
descriptors reused for all pairs (as test/test_tracking.py:176-177 does); a whole chunk of frames goes through each
fused HIP stage in one launch; BatchNorm statistics stay per frame so results equal the reference's
B = 1 calls; nothing synchronises with the host until the caller reads the outputs.

PyTorch is plumbing only (device buffers, streams); all arithmetic runs in libsslam_hip.so via sslam_amd.lib.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass

import numpy as np
import torch

from . import lib

PATCH = 16
N_PREFIX = 5   # CLS + 4 register tokens, dino_backbone.py:51,91
MAX_PAIRS_PER_LAUNCH = 65535


@dataclass
class ExtractorConfig:
    """Shapes and thresholds; defaults = semantic-slam/configs/train_config.yaml:5-17 and the CLI defaults of
    visualize_matches_sequence.py:381-388."""
    input_size: int = 448
    num_keypoints: int = 500
    nms_radius: int = 2
    min_score_percentile: float = 0.50
    bn_train_mode: bool = True          # visualize_* scripts never call backbone.eval()
    bn_eps: float = 1e-5
    saliency_weight: float = 0.3
    min_saliency: float = 0.5
    min_descriptor_sim: float = 0.7
    min_intensity: float = 0.15
    use_intensity: bool = True
    spacing: int = 1
    chunk_frames: int = 1024            # frames per launch group; 1024 x 28^2 x 384 fp32 = 1.2 GB of features
    precision: str = "fp32"             # "fp32": bit-exact vs the CPU reference (the product default and the parity claim);
                                        # "bf16": BASELINE configs[1] throughput mode - saliency CNN + descriptor MLP on bf16
                                        # MFMA (fp32 accumulate), everything else unchanged; NOT index-exact
    confidence: bool = False            # behind A7, the keypoint confidence head (include/sslam_conf.h) at the keypoints the
                                        # descriptors were gathered at: extract() gains `confidence` (n, K); every other output
                                        # keeps its bytes.  Needs SequencePipeline(confidence_state=...) and precision="fp32".
                                        # (It stands in front of the two subcell fields, which tests/test_subcell_cpu.py holds last.)
    subcell: bool = False               # after A5, move each keypoint to the vertex of the per-axis parabola through its cell's
                                        # saliency and its neighbours' (include/sslam_ext.h): extract() gains keypoints_subpatch,
                                        # keypoints_subpixel and subcell_flags; every other output keeps its bits
    subcell_descriptors: bool = False   # with subcell: A6 + A7 gather the descriptors at keypoints_subpatch, not at the cell

    def __post_init__(self):
        if self.subcell_descriptors and not self.subcell:
            raise ValueError("subcell_descriptors=True gathers at the refined keypoints: it needs subcell=True")

    @property
    def grid(self) -> int:
        return self.input_size // PATCH

    def launch_group(self) -> int:
        """Frames per launch group: chunk_frames, but never more than one 32-bit buffer descriptor can span (the saliency CNN
        addresses the fp32 feature map through a single descriptor: < 4 GiB per launch; 2 965 frames at G = 40 are 7.3 GB)."""
        return max(1, min(self.chunk_frames, (2 ** 32 - 1) // (self.grid ** 2 * 384 * 4)))


@dataclass(frozen=True)
class MatchRule:
    """One of the reference's sibling matchers as the rule of the matcher stage (`rule=` of SequencePipeline.match / match_pairs,
    harness.StreamingSequence, online.RuleFrameStepper; include/sslam_hip.h states each rule).  `param` is the threshold rounded
    to fp32 once, as a Python float: the reference compares fp32 arrays with a Python scalar, which numpy rounds to fp32 first.
    Built by the three constructors, whose names and defaults are the reference's arguments."""
    kind: int
    param: float

    @staticmethod
    def _fp32(name: str, v) -> float:
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        with np.errstate(over="ignore"):
            r = float(np.float32(v))
        if not math.isfinite(r):
            raise ValueError(f"{name} = {v!r} is not finite in fp32")
        return r

    @classmethod
    def ratio(cls, ratio_thresh: float = 0.8) -> "MatchRule":
        """M2, MatchVisualizer.find_matches (visualize_matches.py:102-124): mutual nearest neighbours whose similarity exceeds
        ratio_thresh times the row's runner-up; `value` is the similarity."""
        return cls(lib.RULE_RATIO_BEST, cls._fp32("ratio_thresh", ratio_thresh))

    @classmethod
    def mnn_ratio(cls, ratio_threshold: float = 0.9) -> "MatchRule":
        """M4, find_mutual_nearest_neighbors (test/test_descriptor_quality.py:97-142): mutual nearest neighbours with
        runner-up / (best + 1e-8) below ratio_threshold; `value` is the cosine DISTANCE 1 - similarity."""
        return cls(lib.RULE_RATIO_SECOND, cls._fp32("ratio_threshold", ratio_threshold))

    @classmethod
    def tracked(cls, match_threshold: float = 0.8) -> "MatchRule":
        """M5, the tracking count (test/test_tracking.py:158-161): rows whose best similarity exceeds match_threshold, no mutual
        check - `match_count` is the reference's count, `matches` row (i, nn12[i]), `value` the similarity.  Reads the row
        direction only: the matcher takes the rows-only similarity launch."""
        return cls(lib.RULE_TRACKED, cls._fp32("match_threshold", match_threshold))

    def __post_init__(self):
        if self.kind not in (lib.RULE_RATIO_BEST, lib.RULE_RATIO_SECOND, lib.RULE_TRACKED):
            raise ValueError(f"unknown rule kind {self.kind!r}")
        if self._fp32("param", self.param) != self.param:
            raise ValueError(f"param {self.param!r} is not an fp32 value: use the constructors")


def _checked_rule(rule, k: int):
    """rule=: None or a MatchRule; M4 on fewer than two candidates raises what the reference's np.sort(...)[:, 1] raises."""
    if rule is not None and not isinstance(rule, MatchRule):
        raise ValueError(f"rule must be None or a MatchRule, got {type(rule).__name__}")
    if rule is not None and rule.kind == lib.RULE_RATIO_SECOND and k < 2:
        raise IndexError(f"index 1 is out of bounds for axis 1 with size {k}")
    return rule


@dataclass(frozen=True)
class PoseWeights:
    """How a match's weight in the pose refinement is made of its two keypoints' confidences (`weights=` of
    SequencePipeline.match_weights, odometry.odometry / odometry_graph, online.PoseFrameStepper; include/sslam_weight.h states
    both forms).  Built by the two constructors."""
    mode: int
    sigma0: float = 1.0

    @classmethod
    def product(cls) -> "PoseWeights":
        """w = c1 * c2: a match is trusted as far as both of its keypoints are."""
        return cls(lib.WEIGHT_PRODUCT, 1.0)

    @classmethod
    def expected_error(cls, sigma0: float = 1.0) -> "PoseWeights":
        """w = sigma0^2 / (sigma0^2 + e1^2 + e2^2), e = 1 / (c + 1e-6) - 1: the confidence read as the reference's
        compute_expected_error_loss trains it, 1 / (1 + expected error), and the match weighted by its inverse variance against a
        floor of sigma0 (in the error's units)."""
        return cls(lib.WEIGHT_EXPECTED_ERROR, sigma0)

    def __post_init__(self):
        if self.mode not in (lib.WEIGHT_PRODUCT, lib.WEIGHT_EXPECTED_ERROR) or isinstance(self.mode, bool):
            raise ValueError(f"unknown weight mode {self.mode!r}")
        if isinstance(self.sigma0, bool) or not isinstance(self.sigma0, numbers.Real) or not math.isfinite(self.sigma0) or not self.sigma0 > 0:
            raise ValueError(f"sigma0 must be a finite number > 0, got {self.sigma0!r}")
        if self.mode == lib.WEIGHT_PRODUCT and self.sigma0 != 1.0:
            raise ValueError("the product form takes no sigma0: use the constructors")


def _checked_weights(weights):
    """weights=: None or a PoseWeights."""
    if weights is not None and not isinstance(weights, PoseWeights):
        raise ValueError(f"weights must be None or a PoseWeights, got {type(weights).__name__}")
    return weights


@dataclass(frozen=True)
class PoseSettings:
    """How the pose of a pair is estimated, judged ONCE where a public call of odometry or a stepper of online takes the values and
    handed on whole: RANSAC's threshold (keypoint units), hypotheses and seed; refine, and with it the refinement's huber (None:
    threshold / 3) and iterations; weights, None or the PoseWeights of the weighted refinement.  The fields hold the checked values;
    without refine, huber and iterations are kept as given and read by nobody."""
    threshold: float = 3.0
    hypotheses: int = 256
    seed: int = 0
    refine: bool = False
    huber: float | None = None
    iterations: int = 5
    weights: PoseWeights | None = None

    def __post_init__(self):
        checked = dict(threshold=lib.check_threshold(self.threshold), hypotheses=lib.check_hypotheses(self.hypotheses), seed=lib.check_seed(self.seed))
        if not isinstance(self.refine, bool):
            raise ValueError(f"refine must be a bool, got {self.refine!r}")
        if self.refine:
            checked.update(huber=lib.check_huber(checked["threshold"] / 3.0 if self.huber is None else self.huber),
                           iterations=lib.check_iterations(self.iterations))
        if _checked_weights(self.weights) is not None and not self.refine:
            raise ValueError("weights= weights the refinement: it needs refine=True")
        for key, v in checked.items():
            object.__setattr__(self, key, v)

    def check_pipeline(self, pipe) -> None:
        """The one check that needs the pipeline: weights are made of the confidence it must extract.  Without weights `pipe` is not
        touched (it may be None)."""
        if self.weights is not None and not getattr(pipe.cfg, "confidence", False):
            raise ValueError("weights= is made of the keypoint confidence: the pipeline needs ExtractorConfig(confidence=True)")


@dataclass(frozen=True)
class GraphSettings:
    """The solver settings of a pose graph - optimize_pose_graph, optimize_pose_graph_sparse, pose_window_step: huber_chi, damping and
    the most Gauss-Newton iterations (include/sslam_graph.h), judged once like PoseSettings.  The band is no setting: it follows from
    the pair lists (odometry._check_graph)."""
    huber_chi: float = 4.0
    damping: float = 0.0
    iterations: int = 8

    def __post_init__(self):
        for key, v in dict(huber_chi=lib.check_positive("huber_chi", self.huber_chi), damping=lib.check_damping(self.damping),
                           iterations=lib.check_graph_iterations(self.iterations)).items():
            object.__setattr__(self, key, v)


def _np(v):
    """A tensor, wherever it lives, or anything array-like as a numpy array."""
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _host_pair_list(name: str, t):
    """A host sequence of frame indices as an int32 tensor (tensors pass through: lib.check_pair_lists judges them)."""
    if isinstance(t, torch.Tensor):
        return t
    a = np.asarray(t)
    if a.dtype.kind not in "iu" or (a.size and (int(a.min()) < -2 ** 31 or int(a.max()) > 2 ** 31 - 1)):
        raise ValueError(f"pair list `{name}` must hold 32-bit integers, got {a.dtype}")
    return torch.from_numpy(a.astype(np.int32))


def _checked_match_lists(matches, n_pairs: int, k: int | None = None):
    """The `matches` dictionary of a pose method, judged against its pair lists; returns its (P, n1, 2) tensor.  k: the scoring
    methods' lists - k slots and a `value`; None: any list of a matcher or of rank_matches()."""
    keys = ("matches", "match_count") if k is None else ("matches", "value", "match_count")
    source = "match() / match_pairs() / rank_matches()" if k is None else "match_pairs(rule=...)"
    if not isinstance(matches, dict) or any(key not in matches for key in keys):
        raise ValueError(f"matches must be the dictionary {source} returned: {', '.join(keys)}")
    mt = matches["matches"]
    if not isinstance(mt, torch.Tensor) or mt.dim() != 3 or int(mt.shape[0]) != n_pairs or mt.shape[2] != 2 or \
            (k is not None and int(mt.shape[1]) != k):
        raise ValueError(f"matches holds {tuple(getattr(mt, 'shape', ()))}, the pair lists ask for ({n_pairs}, {'n1' if k is None else k}, 2)")
    return mt


REFINER_ORDER_HEAD = ["input_proj.weight", "input_proj.bias"]
REFINER_ORDER_BLOCK = ["norm1.weight", "norm1.bias", "fc1.weight", "fc1.bias", "norm2.weight", "norm2.bias",
                       "fc2.weight", "fc2.bias"]
REFINER_ORDER_TAIL = ["output_proj.weight", "output_proj.bias"]


def _graph_edge_rows(first, second, T, info, n_nodes, judge):
    """What optimize_pose_graph and optimize_pose_graph_sparse judge alike, on the host alone: n_nodes, the edge lists (host
    sequences become lists of int; device tensors give fa = fb = None), T and info as rows or as the dictionaries that hold them.
    judge(fa, fb): the caller's own arguments, judged between the lists and the rows.
    -> n_nodes, fa, fb, the T rows, the info rows, the refinement status or None, the number of edge slots."""
    if isinstance(n_nodes, bool) or not isinstance(n_nodes, (int, np.integer)) or n_nodes < 1:
        raise ValueError(f"n_nodes must be an integer >= 1, got {n_nodes!r}")
    status = info.get("status") if isinstance(info, dict) else None
    t_rows = T["T"] if isinstance(T, dict) and "T" in T else T
    info_rows = info["info"] if isinstance(info, dict) and "info" in info else info
    if isinstance(first, torch.Tensor) != isinstance(second, torch.Tensor):
        raise ValueError("first and second must both be device tensors or both host sequences")
    fa = fb = None
    if not isinstance(first, torch.Tensor):
        fa, fb = [int(v) for v in first], [int(v) for v in second]
        if len(fa) != len(fb) or not fa:
            raise ValueError("first and second must name the same number of edges, at least one")
    judge(fa, fb)
    for name, t, cols in (("T", t_rows, 12), ("info", info_rows, 21)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 2 or int(t.shape[1]) != cols or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 device tensor of shape (E, {cols}) or a dictionary holding one")
    n_edges = int(t_rows.shape[0])
    if int(info_rows.shape[0]) != n_edges or (fa is not None and len(fa) != n_edges):
        raise ValueError(f"{n_edges} transforms for {int(info_rows.shape[0])} information matrices and {len(fa) if fa is not None else '?'} edges")
    return int(n_nodes), fa, fb, t_rows, info_rows, status, n_edges


def _graph_edge_lists(fa, fb, first, second, status, dev):
    """The edge lists on the device (host lists go there now); a refinement status of 3 makes the slot absent, without a read-back."""
    if fa is not None:
        first = torch.tensor(fa, dtype=torch.int32, device=dev)
        second = torch.tensor(fb, dtype=torch.int32, device=dev)
    if status is not None:
        first = torch.where(status == lib.REFINE_NOT_ATTEMPTED, torch.full_like(first, -1), first)
    return first, second


def refiner_weight_list(sd: dict):
    n_blocks = len({k.split(".")[1] for k in sd if k.startswith("residual_blocks.")})
    keys = list(REFINER_ORDER_HEAD)
    for i in range(n_blocks):
        keys += [f"residual_blocks.{i}.{k}" for k in REFINER_ORDER_BLOCK]
    keys += REFINER_ORDER_TAIL
    return [np.ascontiguousarray(_np(sd[k]), np.float32) for k in keys], n_blocks


class PackedSelector:
    """Device-resident, kernel-order copy of a KeypointSelector state_dict."""

    @staticmethod
    def supported(conv0_weight_shape) -> bool:
        """Shapes the saliency-CNN kernels are built for: Conv2d(384 -> 128 | 256, 3x3)."""
        sh = tuple(conv0_weight_shape)
        return len(sh) == 4 and sh[0] in (128, 256) and sh[1:] == (lib.C_FEAT, 3, 3)

    def __init__(self, sd: dict, device, bf16: bool = False):
        w1 = np.ascontiguousarray(_np(sd["conv.0.weight"]), np.float32)
        self.hidden = int(w1.shape[0])
        if not self.supported(w1.shape):
            raise lib.SslamHipError(f"selector shape {w1.shape} unsupported by the HIP kernels (hidden 128/256, C 384)")
        self.w1p = torch.from_numpy(lib.pack_conv3x3(w1)).to(device)
        self.b1 = torch.from_numpy(np.ascontiguousarray(_np(sd["conv.0.bias"]), np.float32)).to(device)
        self.w2 = torch.from_numpy(np.ascontiguousarray(_np(sd["conv.2.weight"]), np.float32).reshape(-1)).to(device)
        self.b2 = torch.from_numpy(np.ascontiguousarray(_np(sd["conv.2.bias"]), np.float32).reshape(-1)).to(device)
        self.w1p_bf16 = None
        if bf16:
            self.w1p_bf16 = torch.from_numpy(lib.pack_conv3x3_bf16(w1)).to(device).view(torch.bfloat16)

    @classmethod
    def empty(cls, hidden: int, device, bf16: bool = False) -> "PackedSelector":
        """Uninitialised device buffers of the packed shapes: the receiving side of the rank-0 weight broadcast (shard.py)."""
        self = cls.__new__(cls)
        self.hidden = int(hidden)
        if not cls.supported((hidden, lib.C_FEAT, 3, 3)):
            raise lib.SslamHipError(f"selector hidden {hidden} unsupported by the HIP kernels (128/256)")
        f32 = dict(dtype=torch.float32, device=device)
        self.w1p = torch.empty(9 * lib.C_FEAT * hidden, **f32)
        self.b1, self.w2, self.b2 = torch.empty(hidden, **f32), torch.empty(hidden, **f32), torch.empty(1, **f32)
        self.w1p_bf16 = torch.empty(9 * lib.C_FEAT * hidden, dtype=torch.bfloat16, device=device) if bf16 else None
        return self

    def tensors(self) -> list:
        """Every device buffer the kernels read, in a fixed order (what broadcast_weights sends)."""
        return [t for t in (self.w1p, self.b1, self.w2, self.b2, self.w1p_bf16) if t is not None]


class PackedRefiner:
    """Device-resident packed DescriptorRefiner weights (one buffer, sslam_refiner_layout order)."""

    @staticmethod
    def supported(input_dim: int, hidden_dim: int, output_dim: int, n_blocks: int) -> bool:
        """Shapes the fused descriptor-MLP kernel is built for: 384 -> 384 -> 128 | 256 with up to 8 residual blocks."""
        return (input_dim, hidden_dim) == (lib.C_FEAT, lib.HID) and output_dim in lib.WIDTHS and 0 <= n_blocks <= 8

    def __init__(self, sd: dict, device, bf16: bool = False):
        ws, self.n_blocks = refiner_weight_list(sd)
        self.output_dim = int(ws[-2].shape[0]) if ws[-2].ndim == 2 else -1
        if ws[0].shape != (lib.HID, lib.C_FEAT) or self.output_dim not in lib.WIDTHS or ws[-2].shape != (self.output_dim, lib.HID):
            raise lib.SslamHipError("refiner shape unsupported by the HIP kernels (384 -> 384 -> 128 | 256)")
        if bf16 and self.output_dim != lib.D_OUT:
            raise lib.SslamHipError(f"precision='bf16' has no {self.output_dim}-wide refiner: the bf16 descriptor MLP is built for "
                                    f"output width {lib.D_OUT} only (use precision='fp32')")
        self.packed = torch.from_numpy(lib.pack_refiner(ws, self.n_blocks)).to(device)
        self.packed_bf16 = torch.from_numpy(lib.pack_refiner_bf16(ws, self.n_blocks)).to(device) if bf16 else None

    @classmethod
    def empty(cls, n_blocks: int, device, bf16: bool = False, output_dim: int = lib.D_OUT) -> "PackedRefiner":
        """Uninitialised packed buffers for `n_blocks` residual blocks and descriptors of width `output_dim` (receiving side of
        the weight broadcast)."""
        self = cls.__new__(cls)
        self.n_blocks = int(n_blocks)
        self.output_dim = lib.check_width(output_dim, "refiner output width")
        if bf16 and self.output_dim != lib.D_OUT:
            raise lib.SslamHipError(f"precision='bf16' has no {self.output_dim}-wide refiner: the bf16 descriptor MLP is built for "
                                    f"output width {lib.D_OUT} only (use precision='fp32')")
        self.packed = torch.empty(int(lib.refiner_layout(n_blocks, self.output_dim).total), dtype=torch.float32, device=device)
        self.packed_bf16 = (torch.empty(int(lib.lib().sslam_refiner_bf16_bytes(n_blocks)), dtype=torch.uint8, device=device)
                            if bf16 else None)
        return self

    def tensors(self) -> list:
        return [t for t in (self.packed, self.packed_bf16) if t is not None]


class PackedConfidence:
    """Device-resident packed UncertaintyEstimator weights (one buffer, sslc_confidence_layout order)."""

    @staticmethod
    def supported(dino_dim: int, descriptor_dim: int, hidden_dim: int) -> bool:
        """Shapes the confidence kernel is built for: 384 + (128 | 256) -> 128 -> 64 -> 1."""
        return lib.confidence_supported(dino_dim, descriptor_dim, hidden_dim)

    def __init__(self, sd: dict, device):
        ws = [np.ascontiguousarray(_np(sd[k]), np.float32) for k in lib.CONF_STATE_KEYS]
        hidden = int(ws[0].shape[0]) if ws[0].ndim == 2 else -1
        self.descriptor_dim = int(ws[0].shape[1]) - lib.C_FEAT if ws[0].ndim == 2 else -1
        if not self.supported(lib.C_FEAT, self.descriptor_dim, hidden):
            raise lib.SslamHipError("confidence head shape unsupported by the HIP kernels (384 + 128 | 256 -> 128 -> 64 -> 1)")
        self.packed = torch.from_numpy(lib.confidence_pack(ws)).to(device)

    def tensors(self) -> list:
        return [self.packed]


class ResampleTables:
    """Pillow coefficient tables on the device, cached per (height, width, size, filter)."""

    def __init__(self, device):
        self.device = device
        self._cache = {}

    def get(self, h: int, w: int, size: int, bicubic: bool):
        key = (h, w, size, bicubic)
        if key not in self._cache:
            tabs = []
            for n_in in (w, h):
                b, c, k = lib.resample_table(n_in, size, bicubic)
                tabs.append((torch.from_numpy(b).to(self.device), torch.from_numpy(c).to(self.device), k))
            self._cache[key] = tuple(tabs)
        return self._cache[key]


class SequencePipeline:
    def __init__(self, cfg: ExtractorConfig, selector_state: dict | None, refiner_state: dict | None, bn_state: dict | None = None,
                 device="cuda", vit=None, empty_shapes: tuple | None = None, vit_precision: str = "bf16",
                 vit_form: str | None = None, confidence_state: dict | None = None):
        """vit: optional sslam_amd.vit.DinoV3ViT, or any module whose weights convert to it (vit.KEY_MAPS) - enables
        run(images, tokens=None): images -> A0 -> HIP ViT (A1) -> ...; vit_precision "bf16" (throughput form, bf16 MFMA
        operands) or "fp32" (the reference's numerics for A1: fp32 operands on the fp32 matrix pipe, csrc/vit_f32.hip)
        vit_form: None, or "few_frame" (bf16 ViT only): batches of up to 8 frames - run() on a short sequence, every step of an
        online.FrameStepper - take the bf16 ViT's few-frame launch form (HipViT.forward_features); larger batches are untouched.
        selector_state / refiner_state None + empty_shapes=(selector hidden, refiner blocks[, descriptor width = 128]):
        uninitialised packed buffers, to be filled by the rank-0 weight broadcast (shard.pipeline_from_rank0).
        descriptor_dim: the refiner's output width (128 or 256), from its state or from empty_shapes; every descriptor buffer,
        bank and matcher launch of this pipeline follows it.  precision="bf16" with a 256-wide refiner raises SslamHipError.
        confidence_state: the state_dict of an UncertaintyEstimator (mlp.0, mlp.2, mlp.4) whose descriptor_dim is this pipeline's:
        packed for the confidence kernel; cfg.confidence=True launches it in every extraction, filter_by_confidence uses its
        output.  cfg.confidence=True without it, or with precision="bf16" (the head has no bf16 form), raises ValueError."""
        self.cfg = cfg
        self.device = torch.device(device)
        lib.lib()   # fail loudly if the HIP library is not built
        if cfg.subcell:
            lib.ext()   # nor the second one, where this pipeline launches from it
        if cfg.precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {cfg.precision!r}")
        if vit_precision not in ("bf16", "fp32"):          # checked whether or not a ViT is given: a typo must not pass silently
            raise ValueError(f"vit_precision must be 'bf16' or 'fp32', got {vit_precision!r}")
        if vit_form not in (None, "few_frame"):
            raise ValueError(f"vit_form must be None or 'few_frame', got {vit_form!r}")
        if vit_form == "few_frame" and vit_precision != "bf16":
            raise ValueError("vit_form='few_frame' names a launch form of the bf16 ViT; the fp32 ViT already follows the batch")
        if cfg.confidence and confidence_state is None:
            raise ValueError("confidence=True needs confidence_state, the state_dict of the confidence head")
        if cfg.confidence and cfg.precision == "bf16":
            raise ValueError("confidence=True needs precision='fp32': the confidence head has no bf16 form")
        self.bf16 = cfg.precision == "bf16"
        if selector_state is None or refiner_state is None:
            if empty_shapes is None:
                raise ValueError("state dicts or empty_shapes=(hidden, n_blocks[, descriptor width]) required")
            self.selector = PackedSelector.empty(empty_shapes[0], self.device, self.bf16)
            self.refiner = PackedRefiner.empty(empty_shapes[1], self.device, self.bf16,
                                               output_dim=empty_shapes[2] if len(empty_shapes) > 2 else lib.D_OUT)
        else:
            self.selector = PackedSelector(selector_state, self.device, self.bf16)
            self.refiner = PackedRefiner(refiner_state, self.device, self.bf16)
        self.confidence = None
        if confidence_state is not None:
            lib.conf()   # the seventh library, where this pipeline launches from it
            self.confidence = PackedConfidence(confidence_state, self.device)
            if self.confidence.descriptor_dim != self.descriptor_dim:
                raise ValueError(f"the confidence head takes descriptors of width {self.confidence.descriptor_dim}, the refiner writes "
                                 f"{self.descriptor_dim}")
        self._ws = None             # caller-owned scratch handed to the *_ws entries (the library never allocates)
        self._stage = {}            # pipeline-owned stage temporaries (features, their bf16 copy, the A0 image): see _stage_buffer
        c = lib.C_FEAT
        bn = bn_state or {}
        f32 = dict(dtype=torch.float32, device=self.device)
        self.bn_gamma = torch.as_tensor(_np(bn.get("weight", np.ones(c))), **f32).contiguous()
        self.bn_beta = torch.as_tensor(_np(bn.get("bias", np.zeros(c))), **f32).contiguous()
        self.bn_mean = torch.as_tensor(_np(bn.get("running_mean", np.zeros(c))), **f32).contiguous()
        self.bn_var = torch.as_tensor(_np(bn.get("running_var", np.ones(c))), **f32).contiguous()
        self.tables = ResampleTables(self.device)
        self.vit_hip = None
        if vit is not None:
            from .vit import DinoV3ViT, convert_module
            from .vit_hip import HipViT
            if not isinstance(vit, DinoV3ViT):
                # a third-party module (timm's, transformers-keyed, ...): its weights, converted and verified (vit.convert_module);
                # this pipeline has no eager path, so a module that does not convert is an error here
                conv, why = convert_module(vit)
                if conv is None:
                    raise lib.SslamHipError(f"{type(vit).__name__} cannot run on the HIP ViT: {why}")
                vit = conv
            # the packers copy every tensor to the device themselves: the caller's module is NOT moved (nn.Module.to works in place)
            if vit_precision == "fp32":
                from .vit_hip import HipViTF32
                self.vit_hip = HipViTF32(vit, self.device)
            else:
                self.vit_hip = HipViT(vit, self.device)
        self.vit_precision, self.vit_form = vit_precision, vit_form

    @property
    def descriptor_dim(self) -> int:
        """The refiner's output width (128 or 256): the width of every descriptor buffer, bank and matcher launch here."""
        return int(getattr(getattr(self, "refiner", None), "output_dim", lib.D_OUT))

    def weight_tensors(self) -> list:
        """Every device buffer of packed weights / BatchNorm state, in a fixed order (6.7 MB fp32 at the shipped shapes)."""
        return self.selector.tensors() + self.refiner.tensors() + [self.bn_gamma, self.bn_beta, self.bn_mean, self.bn_var]

    def workspace(self, n_frames: int, n_pairs: int) -> torch.Tensor | None:
        """The pipeline's scratch tensor, grown to sslam_workspace_bytes(n_frames, G, K, n_pairs): one buffer for all
        stages of a step (they run in stream order on the caller's stream)."""
        need = lib.workspace_bytes(max(1, n_frames), self.cfg.grid, self.cfg.num_keypoints, max(0, n_pairs))
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stage_buffer(self, name: str, shape: tuple, dtype) -> torch.Tensor:
        """A pipeline-owned temporary of a stage, allocated once and reused by every launch group of every pass (grown by
        replacement, never shrunk): the multi-GB intermediates - a launch group's fp32 features are 2.5 GB at G = 40 - do not
        go back to the caching allocator between groups, whose state otherwise decided whether a pass ran at 52 k or 96 k
        frames/s (bf16 mode, 2 965 frames).  Stages run in stream order on the caller's stream, so a buffer is free again by the
        time the next group's producer writes it; results a CALLER keeps are never placed here (reuse=False paths allocate)."""
        need = 1
        for d in shape:
            need *= int(d)
        t = self._stage.get(name)
        if t is None or t.numel() < need or t.dtype != dtype:
            t = torch.empty(need, dtype=dtype, device=self.device)
            self._stage[name] = t
        return t[:need].view(shape)

    # ---------------------------------------------------------------------------------------------- stages
    def preprocess(self, images_u8: torch.Tensor, reuse: bool = False) -> torch.Tensor:
        """A0: (N, H, W, 3) uint8 -> (N, 3, S, S) fp32, Pillow-exact (the ViT input).
        reuse: write into the pipeline's own A0 buffer (valid until the next reuse=True call) instead of a fresh tensor."""
        n, h, w, _ = images_u8.shape
        size = self.cfg.input_size
        th, tv = self.tables.get(h, w, size, False)
        out = self._stage_buffer("a0_image", (n, 3, size, size), torch.float32) if reuse else None
        return lib.preprocess_u8(images_u8, size, th, tv, out=out)

    def tokens_from_images(self, images_u8: torch.Tensor, vit_chunk: int | None = None, out: torch.Tensor | None = None,
                           batch_frames: int | None = None) -> torch.Tensor:
        """A0 + A1: (N, H, W, 3) uint8 -> (N, 5 + G*G, 384) fp32 tokens via the HIP ViT, `vit_chunk` frames at a time.
        Default chunk: HipViT.chunk_frames - whole rounds of the ViT's row-tile workgroups (82 frames at 448 x 448), alternating between two streams.
        batch_frames: the length of the sequence these frames are a piece of, when the caller feeds it in pieces (the streaming
        harness): the fp32 ViT picks its attention form by the batch, so that a frame's tokens do not depend on the cuts.
        Routes: the bf16 ViT takes A0 as bf16 patch rows where the tiled resampler covers the frames (<= 7 horizontal taps, a
        dword-aligned batch base), else the fp32 image, as the fp32 ViT always does - the same tokens either way.
        Cuts: fp32 - vit_chunk and the pieces change no bit (few-frame form up to 8 frames of the BATCH, one-pass above);
        bf16 - the form follows each LAUNCH GROUP (HipViT.forward_features), so the frames of a short last group may differ
        from the same frames in a full group, within the bf16 bars against float64; with vit_form="few_frame" a batch of up to 8
        frames runs the few-frame form in every group, and then neither vit_chunk nor the pieces change a bit."""
        if self.vit_hip is None:
            raise lib.SslamHipError("this pipeline was built without a ViT: pass tokens, or construct it with vit=")
        if vit_chunk is None:
            vit_chunk = self.vit_hip.chunk_frames(self.cfg.input_size)
        shape = (images_u8.shape[0], N_PREFIX + self.cfg.grid ** 2, lib.C_FEAT)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous fp32 tensor of shape {shape}")
        # A0 runs over 16 launch groups at a time (bounds the ViT input: 1.6 GB of bf16 patch rows at 448 x 448); the ViT then
        # alternates those groups between its two streams.  A0 writes the patch-embedding operand directly (bf16 rows of 768 per
        # patch): no fp32 image, no im2patch pass; resampling ratios its tiled kernel does not cover take the fp32 image.
        span = 16 * vit_chunk
        size = self.cfg.input_size
        n, h, w, _ = images_u8.shape
        th, tv = self.tables.get(h, w, size, False)
        for a in range(0, n, span):
            b = min(a + span, n)
            # the fp32 ViT consumes the fp32 image (its patch embedding is an fp32 contraction too); bf16: the patch rows
            patches = lib.preprocess_u8_patches(images_u8[a:b], size, th, tv) if self.vit_precision == "bf16" else None
            whole = max(n, batch_frames or 0)
            if patches is not None:
                self.vit_hip.forward_features(None, out=out[a:b], chunk=vit_chunk, patches=patches, size=size, form=self.vit_form,
                                              batch_frames=whole)
            else:
                # the fp32 ViT picks its form by the batch; the bf16 one per launch group unless vit_form names one (HipViT.forward_features)
                kw = dict(batch_frames=whole) if self.vit_precision == "fp32" else dict(form=self.vit_form, batch_frames=whole)
                self.vit_hip.forward_features(self.preprocess(images_u8[a:b], reuse=self.vit_hip.n_streams < 2), out=out[a:b], chunk=vit_chunk,
                                              **kw)
        return out

    def preprocess_patches(self, images_u8: torch.Tensor):
        """A0 as the ViT consumes it: (N, H, W, 3) uint8 -> (N, G*G, 768) bf16 patch rows (None: ratio not covered, see lib)."""
        n, h, w, _ = images_u8.shape
        th, tv = self.tables.get(h, w, self.cfg.input_size, False)
        return lib.preprocess_u8_patches(images_u8, self.cfg.input_size, th, tv)

    def features(self, tokens: torch.Tensor, bf16_copy: bool = False, reuse: bool = False):
        """A2: (N, 5 + G*G, 384) ViT tokens -> (N, G, G, 384) per-frame-normalised patch features
        (bf16_copy: also their bf16 copy, written in the same pass, for the bf16-mode saliency CNN).
        reuse: write into the pipeline's own feature buffers (valid until the next reuse=True call) - what extract() does."""
        g = self.cfg.grid
        if tokens.shape[1] != N_PREFIX + g * g:
            raise AssertionError(f"Expected {g * g} patches, got {tokens.shape[1] - N_PREFIX}")   # dino_backbone.py:94
        flat = (tokens.shape[0], g * g, lib.C_FEAT)
        o32 = self._stage_buffer("features", flat, torch.float32) if reuse else None
        o16 = self._stage_buffer("features_bf16", flat, torch.bfloat16) if (reuse and bf16_copy) else None
        r = lib.bn_tokens(tokens, N_PREFIX, 1, self.bn_gamma, self.bn_beta, self.bn_mean, self.bn_var,
                          self.cfg.bn_train_mode, self.cfg.bn_eps, out=o32, want_stats=False, bf16_copy=bf16_copy, out_bf16=o16)
        shape = (tokens.shape[0], g, g, lib.C_FEAT)
        return (r[0].view(shape), r[3].view(shape)) if bf16_copy else r[0].view(shape)

    def launch_group(self) -> int:
        """Frames per launch group (ExtractorConfig.launch_group: chunk_frames, capped by the 4 GiB a buffer descriptor spans)."""
        return self.cfg.launch_group()

    def alloc_extract(self, n: int, with_intensity: bool) -> dict:
        """Output buffers of extract() for n frames (every launch group writes its slice: nothing is concatenated)."""
        cfg, dev = self.cfg, self.device
        g, K = cfg.grid, cfg.num_keypoints
        f32 = dict(dtype=torch.float32, device=dev)
        out = dict(saliency=torch.empty((n, g, g), **f32), keypoints_patch=torch.empty((n, K, 2), **f32),
                   keypoints_pixel=torch.empty((n, K, 2), **f32), scores=torch.empty((n, K), **f32),
                   idx=torch.empty((n, K), dtype=torch.int32, device=dev), descriptors=torch.empty((n, K, self.descriptor_dim), **f32),
                   status=torch.empty((n,), dtype=torch.int32, device=dev))
        if with_intensity:
            out["intensity"] = torch.empty((n, K), **f32)
        if cfg.subcell:
            for key, (shape, dtype) in lib.subcell_shapes(n, K).items():
                out[key] = torch.empty(shape, dtype=dtype, device=dev)
        if cfg.confidence:
            out["confidence"] = torch.empty((n, K), **f32)
        return out

    @staticmethod
    def geometry_keypoints(out: dict) -> torch.Tensor:
        """The keypoint bank (N, K, 2), in pixels of the input, that geometry should read from what extract() - or a stepper, or
        result["frames"] of the harness - returned: the refined keypoints_subpixel where the pipeline ran with subcell=True, else
        the cell centres keypoints_pixel."""
        return out["keypoints_subpixel"] if "keypoints_subpixel" in out else out["keypoints_pixel"]

    def extract(self, tokens: torch.Tensor, images_u8: torch.Tensor | None = None, out: dict | None = None,
                images_ready: "torch.cuda.Event | None" = None) -> dict:
        """A2..A9 for any number of frames (launch groups of `launch_group()` frames).  Returns device tensors; no host
        synchronisation unless num_keypoints exceeds the number of grid cells (the only case `status` can be set).
        out: buffers from alloc_extract (or row slices of them) to write into - the sharded runner and the streaming
        scheduler pass slices of sequence-sized buffers, so nothing is copied afterwards.
        images_ready: event after which images_u8 holds the frames (an upload in flight on another stream): the current
        stream waits for it in front of the FIRST kernel that reads pixels - A9, the last stage - so A2..A7, which read
        only the tokens, run while the upload is still in flight."""
        n, step = tokens.shape[0], self.launch_group()
        if out is None:
            out = self.alloc_extract(n, images_u8 is not None)
        elif self.cfg.subcell and any(key not in out for key in lib.SUBCELL_KEYS):      # judged before anything is launched
            raise ValueError(f"out must hold {', '.join(lib.SUBCELL_KEYS)} under subcell=True (alloc_extract)")
        elif self.cfg.confidence and "confidence" not in out:
            raise ValueError("out must hold confidence under confidence=True (alloc_extract)")
        for a in range(0, n, step):
            b = min(a + step, n)
            self._extract_group(tokens[a:b], None if images_u8 is None else images_u8[a:b], {k: v[a:b] for k, v in out.items()},
                                images_ready if a == 0 else None)
        if self.cfg.num_keypoints > self.cfg.grid ** 2 and bool(out["status"].any()):
            # torch.topk raises there in the reference (keypoint_selector.py:160 / :176)
            raise RuntimeError("selected index k out of range")
        return out

    def _extract_group(self, tokens: torch.Tensor, images_u8: torch.Tensor | None, out: dict, images_ready=None) -> None:
        cfg, s = self.cfg, self.selector
        ws = self.workspace(tokens.shape[0], 0)
        if self.bf16:
            feat, feat_bf = self.features(tokens, bf16_copy=True, reuse=True)
            lib.selector_saliency_bf16(feat_bf, s.w1p_bf16, s.b1, s.w2, s.b2, s.hidden, out=out["saliency"])
            del feat_bf
        else:
            feat = self.features(tokens, reuse=True)
            lib.selector_saliency(feat, s.w1p, s.b1, s.w2, s.b2, s.hidden, out=out["saliency"], workspace=ws)
        lib.select_keypoints(out["saliency"], cfg.num_keypoints, cfg.nms_radius, cfg.min_score_percentile,
                             out=(out["keypoints_patch"], out["scores"], out["idx"], out["keypoints_pixel"], out["status"]))
        if cfg.subcell:
            lib.subcell_keypoints(out["saliency"], out["idx"], out=tuple(out[key] for key in lib.SUBCELL_KEYS))
        # A6's bilinear gather takes fractional coordinates as it takes whole ones; A9 and the matcher keep the cell centres
        kp = out["keypoints_subpatch"] if cfg.subcell_descriptors else out["keypoints_patch"]
        if self.bf16:
            lib.gather_refine_bf16(feat, kp, self.refiner.packed_bf16, self.refiner.n_blocks, out=out["descriptors"])
        else:
            lib.gather_refine(feat, kp, self.refiner.packed, self.refiner.n_blocks, out=out["descriptors"], workspace=ws)
        if cfg.confidence:
            # the head reads the features where the descriptors read them: one more gather inside its kernel, nothing 384 wide stored
            lib.gather_confidence(feat, kp, out["descriptors"], self.confidence.packed, out=out["confidence"])
        if images_ready is not None:
            torch.cuda.current_stream(self.device).wait_event(images_ready)
        if images_u8 is not None and "intensity" in out:
            n, h, w, _ = images_u8.shape
            th, tv = self.tables.get(h, w, cfg.input_size, True)
            lib.keypoint_intensity(images_u8, cfg.input_size, th, tv, out["keypoints_pixel"], out=out["intensity"])

    def filter_by_confidence(self, out: dict, threshold: float = 0.5) -> dict:
        """The frames of extract() (confidence=True) with their low-confidence keypoints dropped, in extract()'s form and shapes:
        per frame the keypoints with confidence >= threshold come first, in their order, and the rest of the K slots repeats the
        last kept one (UncertaintyEstimator.filter_keypoints_by_confidence's pad, and what the selector's own pad does: a
        repeated keypoint); a frame in which none passes keeps its most confident keypoint.  Every per-keypoint array of `out`
        (keypoints, scores, idx, descriptors, intensity, the subcell ones) is taken through `slot`; `confidence` is the kept
        confidences followed by zeros; `count` (n,) and `slot` (n, K) int32 are added; saliency and status pass through.
        The result goes into match / match_pairs unchanged.  One filter launch and one take per array; no host read."""
        if "confidence" not in out:
            raise ValueError("out holds no confidence: extract() under ExtractorConfig(confidence=True) writes it")
        slot, count, conf = lib.confidence_filter(out["confidence"], threshold)
        n, k = slot.shape
        res = {}
        for key, v in out.items():
            if key == "confidence":
                res[key] = conf
            elif key in ("saliency", "status") or v.dim() < 2 or tuple(v.shape[:2]) != (n, k):
                res[key] = v
            else:
                res[key] = lib.take_rows(v, slot)
        res["count"], res["slot"] = count, slot
        return res

    def alloc_match(self, n_pairs: int, k: int | None = None, rule: MatchRule | None = None) -> dict:
        """Output buffers of match() for n_pairs pairs (fixed capacity K per pair + device-side count).
        rule: the buffers of match(rule=...): `value` in place of `quality` (a distance must not pass for a quality)."""
        k = self.cfg.num_keypoints if k is None else k
        dev = self.device
        return {"matches": torch.empty((n_pairs, k, 2), dtype=torch.int64, device=dev),
                ("quality" if rule is None else "value"): torch.empty((n_pairs, k), dtype=torch.float32, device=dev),
                "match_count": torch.empty((n_pairs,), dtype=torch.int32, device=dev)}

    def _desc_width(self, desc) -> int:
        """The width of a (N, K, width) descriptor tensor handed to the matcher: this pipeline's descriptor_dim."""
        if desc.dim() != 3 or int(desc.shape[2]) != self.descriptor_dim:
            raise ValueError(f"desc (N, K, {self.descriptor_dim}) expected, got {tuple(desc.shape)}")
        return self.descriptor_dim

    @staticmethod
    def _rule_result(res: dict, aux: list) -> dict:
        """The arg-max arrays a rule's launches produced (nn12, sim; second and nn21 where the rule reads them), beside its outputs."""
        for key in aux[0]:
            res[key] = aux[0][key] if len(aux) == 1 else torch.cat([x[key] for x in aux])
        return res

    def _match_rule(self, rule: MatchRule, desc, sp: int, res: dict) -> dict:
        """match() under a rule: the same cuts, the rule's finalize entry; RULE_TRACKED takes the rows-only similarity launch."""
        n, k, dw = desc.shape[0], desc.shape[1], self._desc_width(desc)
        n_pairs, aux = n - sp, []
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):
            m = min(MAX_PAIRS_PER_LAUNCH, n_pairs - a)
            d1, d2 = desc[a:a + m], desc[a + sp:a + sp + m]
            if rule.kind == lib.RULE_TRACKED:
                nn12, s12, sec = lib.sim_argmax_rows(d1, k * dw, k, d2, k * dw, k, m)
                nn21 = None
            else:
                nn12, s12, nn21, _, sec = lib.sim_argmax(d1, k * dw, k, d2, k * dw, k, m, want_second=True,
                                                         workspace=self.workspace(0, m))
            lib.match_finalize_rule(nn12, s12, sec, nn21, k, k, m, rule.kind, rule.param,
                                    out=(res["matches"][a:a + m], res["value"][a:a + m], res["match_count"][a:a + m]))
            aux.append({key: t for key, t in (("nn12", nn12), ("sim", s12), ("second", sec), ("nn21", nn21)) if t is not None})
        return self._rule_result(res, aux)

    def _match_pairs_rule(self, rule: MatchRule, desc, first, second, n_pairs: int, res: dict) -> dict:
        aux = []
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):
            m = min(MAX_PAIRS_PER_LAUNCH, n_pairs - a)
            f, s = first[a:a + m], second[a:a + m]
            if rule.kind == lib.RULE_TRACKED:
                nn12, s12, sec = lib.sim_argmax_rows_pairs(desc, f, s)
                nn21 = None
            else:
                nn12, s12, nn21, _, sec = lib.sim_argmax_pairs(desc, f, s, want_second=True, workspace=self.workspace(0, m))
            lib.match_finalize_rule_pairs(nn12, s12, sec, nn21, f, s, desc.shape[0], rule.kind, rule.param,
                                          out=(res["matches"][a:a + m], res["value"][a:a + m], res["match_count"][a:a + m]))
            aux.append({key: t for key, t in (("nn12", nn12), ("sim", s12), ("second", sec), ("nn21", nn21)) if t is not None})
        return self._rule_result(res, aux)

    def match(self, desc, scores, intensity=None, spacing: int | None = None, out: dict | None = None,
              rule: MatchRule | None = None) -> dict:
        """M1 for all pairs (i, i + spacing) inside the batch.  desc (N, K, descriptor_dim), scores (N, K), intensity (N, K).
        out: row slices of alloc_match buffers to write into (the streaming scheduler passes slices of sequence-sized ones).
        rule: a MatchRule - the same pairs under M2 / M4 / M5 instead (scores, intensity and the M1 thresholds are not read).
        Returns matches, match_count and `value` (similarity; distance 1 - similarity under mnn_ratio) - no `quality` key - with
        nn12 and sim, and second and nn21 under the two ratio rules (tracked computes neither); out: alloc_match(rule=) buffers."""
        cfg = self.cfg
        sp = cfg.spacing if spacing is None else spacing
        n, k, dw = desc.shape[0], desc.shape[1], self._desc_width(desc)
        rule = _checked_rule(rule, k)
        n_pairs = n - sp
        if n_pairs <= 0:
            z = torch.zeros
            return {"matches": z((0, k, 2), dtype=torch.int64, device=desc.device),
                    ("quality" if rule is None else "value"): z((0, k), dtype=torch.float32, device=desc.device),
                    "match_count": z((0,), dtype=torch.int32, device=desc.device)}
        if rule is not None:
            return self._match_rule(rule, desc, sp, dict(out) if out is not None else self.alloc_match(n_pairs, k, rule))
        use_int = cfg.use_intensity and intensity is not None
        res = dict(out) if out is not None else self.alloc_match(n_pairs, k)
        aux = []
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # the pair index is a 16-bit grid dimension
            m = min(MAX_PAIRS_PER_LAUNCH, n_pairs - a)
            d1, d2 = desc[a:a + m], desc[a + sp:a + sp + m]
            nn12, s12, nn21, _, _ = lib.sim_argmax(d1, k * dw, k, d2, k * dw, k, m, workspace=self.workspace(0, m))
            lib.match_finalize(nn12, s12, nn21, k, k, m, scores[a:], k, scores[a + sp:], k,
                               intensity[a:] if use_int else None, intensity[a + sp:] if use_int else None,
                               1.0 - cfg.saliency_weight, cfg.saliency_weight, cfg.min_saliency,
                               cfg.min_descriptor_sim, cfg.min_intensity,
                               out=(res["matches"][a:a + m], res["quality"][a:a + m], res["match_count"][a:a + m]))
            aux.append((nn12, nn21, s12))
        for i, key in enumerate(("nn12", "nn21", "sim")):       # the arg-max arrays (diagnostics): one launch in practice
            res[key] = aux[0][i] if len(aux) == 1 else torch.cat([x[i] for x in aux])
        return res

    def match_pairs(self, desc, scores, intensity=None, first=None, second=None, out: dict | None = None,
                    rule: MatchRule | None = None) -> dict:
        """M1 for a LIST of pairs of the bank desc (N, K, descriptor_dim) / scores (N, K) / intensity (N, K): row p matches frame first[p]
        against frame second[p] - any two frames, in any order, as often as listed; an index outside [0, N) (-1 by convention)
        makes the pair absent: count 0, zero rows.  first / second: 1-D int32 device tensors (they may be written by earlier work
        of the stream: nothing here reads them on the host), or host sequences of ints, uploaded once.
        Returns match()'s dictionary with one row per listed pair, in list order; per pair the same bits as match() on the same
        two frames.  out: alloc_match buffers (or row slices of them) to write into.
        rule: a MatchRule - the listed pairs under M2 / M4 / M5, returning what match(rule=) returns."""
        cfg = self.cfg
        if first is None or second is None:
            raise ValueError("match_pairs needs both pair lists, first= and second=")
        if desc.dim() != 3 or scores.dim() != 2 or tuple(scores.shape) != tuple(desc.shape[:2]) or desc.shape[2] != self.descriptor_dim:
            raise ValueError(f"desc (N, K, {self.descriptor_dim}) and scores (N, K) expected, got {tuple(desc.shape)} and "
                             f"{tuple(scores.shape)}")
        rule = _checked_rule(rule, desc.shape[1])
        first, second = _host_pair_list("first", first), _host_pair_list("second", second)
        n_pairs = lib.check_pair_lists(first, second)             # a malformed list is refused before anything is uploaded
        first, second = (t if t.is_cuda else t.to(desc.device) for t in (first, second))
        lib.check_pair_lists(first, second, desc.device)
        k = desc.shape[1]
        if rule is not None:
            return self._match_pairs_rule(rule, desc, first, second, n_pairs,
                                          dict(out) if out is not None else self.alloc_match(n_pairs, k, rule))
        use_int = cfg.use_intensity and intensity is not None
        res = dict(out) if out is not None else self.alloc_match(n_pairs, k)
        aux = []
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match() cuts
            m = min(MAX_PAIRS_PER_LAUNCH, n_pairs - a)
            f, s = first[a:a + m], second[a:a + m]
            nn12, s12, nn21, _, _ = lib.sim_argmax_pairs(desc, f, s, workspace=self.workspace(0, m))
            lib.match_finalize_pairs(nn12, s12, nn21, f, s, scores, intensity if use_int else None,
                                     1.0 - cfg.saliency_weight, cfg.saliency_weight, cfg.min_saliency,
                                     cfg.min_descriptor_sim, cfg.min_intensity,
                                     out=(res["matches"][a:a + m], res["quality"][a:a + m], res["match_count"][a:a + m]))
            aux.append((nn12, nn21, s12))
        for i, key in enumerate(("nn12", "nn21", "sim")):
            res[key] = aux[0][i] if len(aux) == 1 else torch.cat([x[i] for x in aux])
        return res

    def alloc_ranked(self, n_pairs: int, best: int, k: int | None = None, rule: MatchRule | None = None) -> dict:
        """Output buffers of rank_matches() for n_pairs pairs: the `best` best rows of lists of capacity k (num_keypoints by
        default).  rule: as in alloc_match - `value` in place of `quality`."""
        k = self.cfg.num_keypoints if k is None else k
        best = lib.check_best(best, k)
        _checked_rule(rule, k)
        dev = self.device
        return {"matches": torch.empty((n_pairs, best, 2), dtype=torch.int64, device=dev),
                ("quality" if rule is None else "value"): torch.empty((n_pairs, best), dtype=torch.float32, device=dev),
                "match_count": torch.empty((n_pairs,), dtype=torch.int32, device=dev),
                "slot": torch.empty((n_pairs, best), dtype=torch.int32, device=dev)}

    def rank_matches(self, m: dict, best: int | None = None, rule: MatchRule | None = None, out: dict | None = None) -> dict:
        """The stage after the matcher, as the reference's callers have it (visualize_matches_sequence.py:224-225,
        visualize_matches.py:150-151): every pair's `best` best matches, better first, equal values in the list's own order
        (ascending idx1) - one launch, nothing read on the host.  m: what match() / match_pairs() returned (or alloc_match buffers
        they wrote): matches, match_count and `quality` (M1) or `value` (a rule).  rule: the rule m was matched under - better is
        SMALLER exactly under MatchRule.mnn_ratio, whose value is a distance; None for M1.  best=None ranks whole lists.
        Returns matches (P, best, 2), quality | value (P, best), match_count (P,) = min(count, best) and slot (P, best) int32, the
        row of m each kept row came from; rows past the count are zero.  out: alloc_ranked buffers (or row slices of them).
        m itself is left as it is."""
        val = "quality" if rule is None else "value"
        if not isinstance(m, dict) or any(key not in m for key in ("matches", "match_count")):
            raise ValueError("rank_matches takes the dictionary match() / match_pairs() returned")
        matches = m["matches"]
        if not isinstance(matches, torch.Tensor) or matches.dim() != 3:
            raise ValueError("matches (P, K, 2) expected")
        k = int(matches.shape[1])
        best = lib.check_best(best, k)                              # a bad best, a bad rule: before any device work
        rule = _checked_rule(rule, k)
        if val not in m:
            raise ValueError(f"this match dictionary holds no `{val}`: " +
                             ("pass the rule it was matched under" if rule is None else "it was not matched under a rule"))
        n_pairs = int(matches.shape[0])
        res = dict(out) if out is not None else self.alloc_ranked(n_pairs, best, k, rule)
        if val not in res or any(key not in res for key in ("matches", "match_count")):
            raise ValueError(f"out must hold matches, {val} and match_count (alloc_ranked with the same rule)")
        if n_pairs == 0:
            return res
        lib.match_rank(matches, m[val], m["match_count"], best, ascending=rule is not None and rule.kind == lib.RULE_RATIO_SECOND,
                       out=(res["matches"], res[val], res["match_count"], res.get("slot")))
        return res

    def _pose_buffers(self, shapes_of, keys, n_pairs: int, k: int | None, out: dict | None = None, alloc: str = "") -> dict:
        """The buffers of a pose method: fresh ones for n_pairs pairs of k rows (num_keypoints by default) from a lib.*_shapes
        function, or the caller's `out`, which must hold every key (`alloc` names the method that makes them)."""
        if out is not None:
            if any(key not in out for key in keys):
                raise ValueError(f"out must hold {', '.join(keys)} ({alloc})")
            return dict(out)
        shapes = shapes_of(n_pairs, self.cfg.num_keypoints if k is None else k)
        return {key: torch.empty(shapes[key][0], dtype=shapes[key][1], device=self.device) for key in keys}

    def _pose_operands(self, what: str, keypoints_pixel, first, second, *kp_depth):
        """What the pose methods check alike, before any device work: the bank keypoints_pixel (N, K, 2), the kp_depth (N, K) of a
        method that takes one, and the two pair lists (as match_pairs takes them; host sequences are uploaded once).
        Returns (first, second - on the bank's device -, n_pairs, K, that device)."""
        if not isinstance(keypoints_pixel, torch.Tensor) or keypoints_pixel.dim() != 3 or keypoints_pixel.shape[2] != 2:
            raise ValueError("keypoints_pixel (N, K, 2) expected")
        for d in kp_depth:
            if not isinstance(d, torch.Tensor) or tuple(d.shape) != tuple(keypoints_pixel.shape[:2]):
                raise ValueError(f"kp_depth {tuple(keypoints_pixel.shape[:2])} int32 expected: keypoint_depth() of the same bank")
        if first is None or second is None:
            raise ValueError(f"{what} needs both pair lists, first= and second=")
        first, second = _host_pair_list("first", first), _host_pair_list("second", second)
        n_pairs = lib.check_pair_lists(first, second)             # a malformed list is refused before anything is uploaded
        dev = keypoints_pixel.device
        first, second = (x if x.is_cuda else x.to(dev) for x in (first, second))
        lib.check_pair_lists(first, second, dev)
        return first, second, n_pairs, int(keypoints_pixel.shape[1]), dev

    def alloc_pose_scores(self, n_pairs: int, k: int | None = None, with_matches: bool = True) -> dict:
        """Output buffers of pose_scores() for n_pairs pairs of k keypoints (num_keypoints by default); with_matches: also the
        tp / fp / fn / value_sum a match list is scored into."""
        return self._pose_buffers(lib.pose_score_shapes, lib.POSE_SCORE_KEYS + (lib.MATCH_SCORE_KEYS if with_matches else ()), n_pairs, k)

    def pose_scores(self, keypoints_pixel, first, second, H, threshold: float = 3.0, matches: dict | None = None,
                    out: dict | None = None) -> dict:
        """The scoring stage (csrc/evaluate.hip): for every listed pair of the bank keypoints_pixel (N, K, 2) - what extract()
        returns under that name - warp frame first[p]'s keypoints by H[p], find the nearest keypoint of frame second[p] and keep the
        rows nearer than `threshold` pixels: the reference's repeatability count and its ground-truth matches
        (test/test_repeatability.py:79-128, test/test_descriptor_quality.py:144-185).
        first / second: as match_pairs takes them (1-D int32 device tensors or host sequences; -1 = absent pair).  H: (P, 3, 3) or
        (P, 9) float64, a device tensor or a host array (uploaded once), or None for the raw coordinates.
        matches: what match_pairs(rule=MatchRule.mnn_ratio()) returned for the same lists (matches, value, match_count) - then the
        list of every pair is scored against the ground truth as evaluate_matches does (:187-231).
        Returns device tensors, one row per listed pair: gt_matches (P, K, 2) int64, gt_count (P,) int32 (= the repeatable count),
        gt_of_row (P, K) int32, dist_sum, dist_median (P,) float64, and with matches tp, fp, fn (P,) int32, value_sum (P,) float64.
        out: alloc_pose_scores buffers (or row slices of them).  Two launches per 65 535 pairs, nothing read on the host."""
        first, second, n_pairs, k, dev = self._pose_operands("pose_scores", keypoints_pixel, first, second)
        t = lib.check_threshold(threshold)
        if H is not None:
            if not isinstance(H, torch.Tensor):
                H = torch.from_numpy(np.ascontiguousarray(np.asarray(H, dtype=np.float64)))
            if H.dtype != torch.float64 or tuple(H.shape) not in ((n_pairs, 9), (n_pairs, 3, 3)):
                raise ValueError(f"H must be float64 of shape ({n_pairs}, 3, 3) or ({n_pairs}, 9), got {H.dtype} {tuple(H.shape)}")
            H = H.to(dev).contiguous()
        if matches is not None:
            _checked_match_lists(matches, n_pairs, k)
        res = self._pose_buffers(lib.pose_score_shapes, lib.POSE_SCORE_KEYS + (lib.MATCH_SCORE_KEYS if matches is not None else ()),
                                 n_pairs, k, out, "alloc_pose_scores")
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match_pairs cuts
            b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
            lib.pose_nn_pairs(keypoints_pixel, first[a:b], second[a:b], None if H is None else H[a:b], t,
                              out=tuple(res[key][a:b] for key in lib.POSE_SCORE_KEYS))
            if matches is not None:
                lib.match_score_pairs(matches["matches"][a:b], matches["value"][a:b], matches["match_count"][a:b],
                                      res["gt_of_row"][a:b], res["gt_count"][a:b], out=tuple(res[key][a:b] for key in lib.MATCH_SCORE_KEYS))
        return res

    def depth_scales(self, camera) -> tuple:
        """(scale_x, scale_y): from this pipeline's keypoint units (input_size wide and high) to the depth pixels of `camera`."""
        _, _, _, _, _, w, h = lib.check_camera(camera)
        return w / self.cfg.input_size, h / self.cfg.input_size

    def keypoint_depth(self, depth_u16, keypoints_pixel, out=None):
        """The raw depth under every keypoint (csrc/evaluate.hip): depth_u16 (n, h, w) uint16 device tensor - TUM's raw
        values, metres times 5000 - for the n frames whose keypoints_pixel (n, K, 2) extract() returned; the keypoint is taken to
        the depth image by w / input_size and h / input_size and rounded to the nearest pixel.  Returns (n, K) int32: the raw
        value, 0 where the sensor measured nothing, -1 outside the image.  out: an (n, K) int32 tensor (a slice of a sequence-sized
        bank: depth images need not stay on the device).  One launch, nothing read on the host."""
        if not isinstance(depth_u16, torch.Tensor) or depth_u16.dim() != 3:
            raise ValueError("depth_u16 (n, h, w) uint16 expected")
        return lib.keypoint_depth(depth_u16, keypoints_pixel, int(depth_u16.shape[2]) / self.cfg.input_size,
                                  int(depth_u16.shape[1]) / self.cfg.input_size, out=out)

    def alloc_pose_depth_scores(self, n_pairs: int, k: int | None = None, with_matches: bool = True) -> dict:
        """Output buffers of pose_depth_scores() for n_pairs pairs of k keypoints (num_keypoints by default)."""
        return self._pose_buffers(lib.pose_depth_score_shapes,
                                  lib.POSE_DEPTH_SCORE_KEYS + (lib.MATCH_KNOWN_SCORE_KEYS if with_matches else ()), n_pairs, k)

    def pose_depth_scores(self, keypoints_pixel, kp_depth, first, second, T, camera, threshold: float = 3.0,
                          matches: dict | None = None, out: dict | None = None) -> dict:
        """pose_scores() against the translation-aware ground truth (csrc/evaluate.hip): every keypoint of frame first[p] is
        back-projected with its depth kp_depth (N, K) int32 - keypoint_depth()'s output for the same bank - moved by T[p] and
        projected into frame second[p]; from there the nearest-keypoint search and the list scoring of pose_scores().
        T: (P, 3, 4), (P, 12) or (P, 4, 4) float64 (device tensor or host array; of a 4 x 4 the top three rows count), camera a
        coordinates -> camera b coordinates in metres: evaluation.pair_transforms.  camera: an evaluation.Camera; its width x height
        is the depth image, which the keypoints are scaled to by width / input_size and height / input_size.
        Returns device tensors per listed pair: gt_matches, gt_count, gt_of_row (-2: the row has no ground truth), valid_count,
        dist_sum, dist_median, and with matches tp, fp, fn, unknown, value_sum (include/sslam_hip.h).  out:
        alloc_pose_depth_scores buffers.  Two launches per 65 535 pairs, nothing read on the host."""
        first, second, n_pairs, k, dev = self._pose_operands("pose_depth_scores", keypoints_pixel, first, second, kp_depth)
        t = lib.check_threshold(threshold)
        sx, sy = self.depth_scales(camera)
        if T is None:
            raise ValueError("T (P, 3, 4) float64 is required: evaluation.pair_transforms(poses, pairs)")
        if not isinstance(T, torch.Tensor):
            T = torch.from_numpy(np.ascontiguousarray(np.asarray(T, dtype=np.float64)))
        if T.dtype != torch.float64 or tuple(T.shape) not in ((n_pairs, 12), (n_pairs, 3, 4), (n_pairs, 4, 4)):
            raise ValueError(f"T must be float64 of shape ({n_pairs}, 3, 4), ({n_pairs}, 12) or ({n_pairs}, 4, 4), got {T.dtype} {tuple(T.shape)}")
        if T.dim() == 3 and T.shape[1] == 4:
            T = T[:, :3]
        T = T.to(dev).contiguous().reshape(n_pairs, 12)
        if matches is not None:
            _checked_match_lists(matches, n_pairs, k)
        res = self._pose_buffers(lib.pose_depth_score_shapes,
                                 lib.POSE_DEPTH_SCORE_KEYS + (lib.MATCH_KNOWN_SCORE_KEYS if matches is not None else ()), n_pairs, k,
                                 out, "alloc_pose_depth_scores")
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match_pairs cuts
            b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
            lib.pose_depth_nn_pairs(keypoints_pixel, kp_depth, first[a:b], second[a:b], T[a:b], camera, sx, sy, t,
                                    out=tuple(res[key][a:b] for key in lib.POSE_DEPTH_SCORE_KEYS))
            if matches is not None:
                lib.match_score_known_pairs(matches["matches"][a:b], matches["value"][a:b], matches["match_count"][a:b],
                                            res["gt_of_row"][a:b], res["gt_count"][a:b],
                                            out=tuple(res[key][a:b] for key in lib.MATCH_KNOWN_SCORE_KEYS))
        return res

    def alloc_pose(self, n_pairs: int, k: int | None = None) -> dict:
        """Output buffers of estimate_poses() for n_pairs pairs whose match lists hold k slots (num_keypoints by default)."""
        return self._pose_buffers(lib.pose_ransac_shapes, lib.POSE_RANSAC_KEYS, n_pairs, k)

    def estimate_poses(self, keypoints_pixel, kp_depth, first, second, matches: dict, camera, threshold: float = 3.0,
                       hypotheses: int = 256, seed: int = 0, out: dict | None = None) -> dict:
        """Geometric verification (csrc/pose_estimate.hip): for every listed pair of the bank keypoints_pixel (N, K, 2), the rigid
        motion its match list agrees on.  The matches whose two keypoints both have a depth measurement - kp_depth (N, K) int32,
        keypoint_depth()'s output for the same bank - are back-projected; `hypotheses` 3-point samples are solved in closed form
        (Horn), scored by reprojection into the second frame against `threshold` (in this pipeline's keypoint units), and the best
        is refitted over its inliers.
        first / second: as match_pairs takes them.  matches: the dictionary match() / match_pairs() returned for the same pairs
        under any rule, or rank_matches()' output (matches (P, n1, 2), match_count (P,)).  camera: an evaluation.Camera.  seed:
        the sampler's 64-bit seed; a pair's result depends on its own rows and the seed alone, not on its place in the list.
        Returns device tensors per listed pair: T (P, 12) float64 [R | t] camera first -> camera second in metres,
        inlier_count, usable_count, best_hypothesis, refit_kept (P,) int32, inlier_of_slot (P, n1) int32 (1 inlier, 0 not, -1 no
        depth; 0 past the count), rms (P,) float64 (include/sslam_hip.h).  A pair with fewer than 3 usable matches gets the
        identity and best_hypothesis -1.  out: alloc_pose buffers (or row slices).  One launch per 65 535 pairs, no host read."""
        first, second, n_pairs, _, _ = self._pose_operands("estimate_poses", keypoints_pixel, first, second, kp_depth)
        t = lib.check_threshold(threshold)
        n_hyp, seed = lib.check_hypotheses(hypotheses), lib.check_seed(seed)
        sx, sy = self.depth_scales(camera)
        mt = _checked_match_lists(matches, n_pairs)
        res = self._pose_buffers(lib.pose_ransac_shapes, lib.POSE_RANSAC_KEYS, n_pairs, int(mt.shape[1]), out, "alloc_pose")
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match_pairs cuts
            b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
            lib.pose_ransac_pairs(keypoints_pixel, kp_depth, first[a:b], second[a:b], mt[a:b], matches["match_count"][a:b], camera, sx, sy,
                                  t, n_hyp, seed, out=tuple(res[key][a:b] for key in lib.POSE_RANSAC_KEYS))
        return res

    def alloc_pose_refine(self, n_pairs: int, k: int | None = None, weighted: bool = False) -> dict:
        """Output buffers of refine_poses() for n_pairs pairs whose match lists hold k slots (num_keypoints by default); weighted:
        with `weight_sum`, for a call that passes weights."""
        if weighted:
            return self._pose_buffers(lib.pose_refine_weighted_shapes, lib.POSE_REFINE_WEIGHTED_KEYS, n_pairs, k)
        return self._pose_buffers(lib.pose_refine_shapes, lib.POSE_REFINE_KEYS, n_pairs, k)

    def match_weights(self, confidence, first, second, matches: dict, weights: PoseWeights, out=None):
        """Per-match weights for refine_poses(weights=) (csrc_weight/weighted_refine.hip): confidence (N, K) fp32, extract()'s
        `confidence` for the bank the pairs index (ExtractorConfig(confidence=True)); first / second and matches as estimate_poses
        takes them; weights: a PoseWeights.  Returns a (P, n1) float32 device tensor aligned with the match slots, +0.0 where a
        slot holds no match.  out: such a tensor (or a row slice).  One launch per 65 535 pairs, no host read."""
        if not isinstance(weights, PoseWeights):
            raise ValueError(f"weights must be a PoseWeights, got {type(weights).__name__}")
        if not isinstance(confidence, torch.Tensor) or confidence.dim() != 2:
            raise ValueError("confidence (N, K) float32 expected: extract()'s `confidence`")
        first, second = (_host_pair_list(name, t) for name, t in (("first", first), ("second", second)))
        n_pairs = lib.check_pair_lists(first, second)             # a malformed list is refused before anything is uploaded
        first, second = (t if t.device == confidence.device else t.to(confidence.device) for t in (first, second))
        mt = _checked_match_lists(matches, n_pairs)
        n1 = int(mt.shape[1])
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n_pairs, n1) or
                                not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape ({n_pairs}, {n1})")
        res = torch.empty((n_pairs, n1), dtype=torch.float32, device=confidence.device) if out is None else out
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match_pairs cuts
            b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
            lib.match_weights(confidence, first[a:b], second[a:b], mt[a:b], matches["match_count"][a:b], weights.mode, weights.sigma0,
                              out=res[a:b])
        return res

    def refine_poses(self, keypoints_pixel, kp_depth, first, second, matches: dict, camera, pose, threshold: float = 3.0,
                     huber: float | None = None, iterations: int = 5, out: dict | None = None, weights=None) -> dict:
        """Pose refinement (csrc/pose_refine.hip): for every listed pair, up to `iterations` Gauss-Newton steps on the Huber cost of
        the reprojection error into the second frame, from the initial pose `pose` - the dictionary estimate_poses() returned for
        the same pairs, or any (P, 12) float64 device tensor of [R | t] rows (a motion model's prediction, the previous step's
        output).  The rows refined over are the usable matches that are inliers of `pose` at `threshold` (keypoint units), fixed
        for the call; huber: the Huber delta in keypoint units, threshold / 3 if None.  keypoints_pixel, kp_depth, first, second,
        matches, camera: as estimate_poses takes them.
        Returns device tensors per listed pair: T (P, 12) float64, status (0 refined, 1 no step accepted, 2 refined but fewer
        inliers: not kept, 3 not attempted), iterations, selected_count, usable_count, inlier_count_in, inlier_count (P,) int32,
        inlier_of_slot (P, n1) int32, cost_in, cost, rms (P,) float64 and info (P, 21) float64, the upper triangle of the 6 x 6
        information matrix in the parameters (vx, vy, vz, wx, wy, wz) of a left perturbation in the second camera
        (include/sslam_hip.h).  Under status 1, 2 and 3 T is `pose` bit for bit.  out: alloc_pose_refine buffers (or row slices).
        One launch per 65 535 pairs, no host read.
        weights: None, or a (P, n1) float32 device tensor aligned with the match slots - match_weights()' output, or any other:
        the weighted entry runs instead (include/sslam_weight.h: a row whose weight is not finite and > 0 is not selected, a
        selected row's weight multiplies its terms, info is the weighted information matrix), the dictionary also holds
        `weight_sum` (P,) float64, and out is alloc_pose_refine(weighted=True)'s."""
        first, second, n_pairs, _, _ = self._pose_operands("refine_poses", keypoints_pixel, first, second, kp_depth)
        t = lib.check_threshold(threshold)
        n_iter = lib.check_iterations(iterations)
        hub = lib.check_huber(t / 3.0 if huber is None else huber)
        sx, sy = self.depth_scales(camera)
        mt = _checked_match_lists(matches, n_pairs)
        t_in = pose["T"] if isinstance(pose, dict) and "T" in pose else pose
        if not isinstance(t_in, torch.Tensor) or t_in.dtype != torch.float64 or tuple(t_in.shape) != (n_pairs, 12) or not t_in.is_contiguous():
            raise ValueError(f"pose must be estimate_poses()' dictionary or a contiguous float64 tensor of shape ({n_pairs}, 12)")
        if weights is not None:
            if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(mt.shape[:2]) or \
                    not weights.is_contiguous():
                raise ValueError(f"weights must be None or a contiguous float32 tensor of shape {tuple(mt.shape[:2])}: match_weights()' output")
            res = self._pose_buffers(lib.pose_refine_weighted_shapes, lib.POSE_REFINE_WEIGHTED_KEYS, n_pairs, int(mt.shape[1]), out,
                                     "alloc_pose_refine(weighted=True)")
            for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):
                b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
                lib.pose_refine_weighted(keypoints_pixel, kp_depth, first[a:b], second[a:b], mt[a:b], matches["match_count"][a:b], camera,
                                         t_in[a:b], weights[a:b], sx, sy, t, hub, n_iter,
                                         out=tuple(res[key][a:b] for key in lib.POSE_REFINE_WEIGHTED_KEYS))
            return res
        res = self._pose_buffers(lib.pose_refine_shapes, lib.POSE_REFINE_KEYS, n_pairs, int(mt.shape[1]), out, "alloc_pose_refine")
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match_pairs cuts
            b = min(a + MAX_PAIRS_PER_LAUNCH, n_pairs)
            lib.pose_refine_pairs(keypoints_pixel, kp_depth, first[a:b], second[a:b], mt[a:b], matches["match_count"][a:b], camera, t_in[a:b],
                                  sx, sy, t, hub, n_iter, out=tuple(res[key][a:b] for key in lib.POSE_REFINE_KEYS))
        return res

    @staticmethod
    def optimize_pose_graph(first, second, T, info, n_nodes: int, C_init=None, band: int | None = None, huber_chi: float = 4.0,
                            damping: float = 0.0, iterations: int = 8) -> dict:
        """The pose graph over the relative poses of one sequence (csrc_graph/pose_graph.hip): world -> camera poses of n_nodes
        frames, frame 0 the anchor, minimising the Huber cost of the edges' residuals under their information matrices.
        first / second: the frames a < b of every edge, 1-D int32 device tensors or host sequences (-1 in first: an absent slot).
        T: (E, 12) float64 device tensor, camera a -> camera b, or the dictionary estimate_poses() / refine_poses() returned for
        these pairs; info: (E, 21) float64 device tensor, or refine_poses()' dictionary - the edges whose refinement status is 3
        (not attempted: their info is zero) then become absent, on the device, without a read-back.
        C_init: (n_nodes, 12) float64 world -> camera, or None: the chain of the edges (i, i + 1) (sslg_chain_poses) - with host
        lists they are looked up (each must be listed), with device lists they must be the first n_nodes - 1 slots, in order.
        band: the most b - a of a used edge; None: the largest b - a of the host lists (device lists need it given).
        huber_chi, damping, iterations: include/sslam_graph.h.  Returns device tensors: C (n_nodes, 12) float64, status,
        iterations, used_edges, skipped_edges, failed_row () int32, cost_in, cost () float64, edge_chi2 (E,) float64.  Two
        launches at most, no host read.  It reads nothing of the pipeline (a static method: the drop-in calls it without one)."""
        def judge(fa, fb):
            nonlocal band
            if band is None and fa is None:
                raise ValueError("band= is required with device edge lists: the largest b - a is not read back")
            if band is None:
                band = max([b - a for a, b in zip(fa, fb) if 0 <= a < b] or [1])
            band = lib.check_band(band)
            lib.check_positive("huber_chi", huber_chi), lib.check_damping(damping), lib.check_graph_iterations(iterations)
        n_nodes, fa, fb, t_rows, info_rows, status, n_edges = _graph_edge_rows(first, second, T, info, n_nodes, judge)
        host = fa is not None
        chain_rows = None
        if C_init is None and n_nodes > 1:
            if host:
                where = {(a, b): e for e, (a, b) in reversed(list(enumerate(zip(fa, fb))))}
                missing = [i for i in range(n_nodes - 1) if (i, i + 1) not in where]
                if missing:
                    raise ValueError(f"C_init=None chains the edges (i, i + 1): ({missing[0]}, {missing[0] + 1}) is not listed")
                chain_rows = [where[(i, i + 1)] for i in range(n_nodes - 1)]
            elif n_edges < n_nodes - 1:
                raise ValueError(f"C_init=None chains the first {n_nodes - 1} slots: only {n_edges} are listed")
        dev = t_rows.device
        first, second = _graph_edge_lists(fa, fb, first, second, status, dev)
        if C_init is None:
            if n_nodes == 1:
                rows = t_rows[:0]
            elif chain_rows is None or chain_rows == list(range(n_nodes - 1)):
                rows = t_rows[:n_nodes - 1]
            else:
                rows = t_rows.index_select(0, torch.tensor(chain_rows, dtype=torch.int64, device=dev))
            C_init = lib.chain_poses(rows.contiguous(), n_nodes)[0]
        res = lib.pose_graph(first.contiguous(), second, t_rows, info_rows, C_init, band, huber_chi, damping, iterations)
        return {key: t[0] for key, t in zip(lib.POSE_GRAPH_KEYS, res)}

    def find_loop_candidates(self, descriptors, scores, min_gap: int = 30, min_sim: float = 0.3, per_frame: int = 2,
                             suppress: int = 5) -> dict:
        """Loop-closure candidates (csrc_loop/loop.hip): every frame's place signature - the score-weighted sum of its descriptors,
        centred on the sequence's mean and normalised - and, for every frame i, up to per_frame older frames j <= i - min_gap
        whose signature's similarity to i's is at least min_sim, best first, none within `suppress` frames of a better one.
        descriptors (N, K, descriptor_dim), scores (N, K): what extract() returned.  Returns device tensors in match_pairs'
        pair-list form: first, second (N * per_frame,) int32 - the older frame and i, both -1 in an empty slot: an absent pair -
        sim (N * per_frame,) float32, count (N,) int32, and signatures (N, descriptor_dim).  Three launches, no host read."""
        lib.check_loop_arguments(min_gap, min_sim, per_frame, suppress)
        sig = lib.frame_signatures(descriptors, scores)
        res = dict(zip(lib.LOOP_CANDIDATE_KEYS, lib.loop_candidates(sig, min_gap, min_sim, per_frame, suppress)))
        res["signatures"] = sig
        return res

    @staticmethod
    def optimize_pose_graph_sparse(first, second, T, info, n_nodes: int, C_init, huber_chi: float = 4.0, damping: float = 0.0,
                                   iterations: int = 8, cg_iterations: int = 512, cg_tol: float = 1e-3) -> dict:
        """The pose graph with edges anywhere (csrc_loop/loop.hip): optimize_pose_graph without a band - loop-closure edges are
        used like any other - the step solved by block-Jacobi preconditioned conjugate gradients, at most cg_iterations per step,
        stopped at the relative tolerance cg_tol.  first, second, T, info: as optimize_pose_graph takes them (a refinement status
        of 3 makes the slot absent, on the device).  C_init (n_nodes, 12) float64 world -> camera is required: the banded graph's
        C, or the chain.  Returns optimize_pose_graph's device tensors and cg_steps (16,) int32, the CG iterations of every step
        (include/sslam_loop.h).  One launch, no host read."""
        def judge(fa, fb):
            lib.check_positive("huber_chi", huber_chi), lib.check_damping(damping), lib.check_graph_iterations(iterations)
            lib.check_cg_iterations(cg_iterations), lib.check_cg_tol(cg_tol)
        n_nodes, fa, fb, t_rows, info_rows, status, _ = _graph_edge_rows(first, second, T, info, n_nodes, judge)
        if not isinstance(C_init, torch.Tensor) or tuple(C_init.shape) != (n_nodes, 12):
            raise ValueError(f"C_init must be a float64 device tensor of shape ({n_nodes}, 12)")
        first, second = _graph_edge_lists(fa, fb, first, second, status, t_rows.device)
        res = lib.pose_graph_sparse(first.contiguous(), second, t_rows, info_rows, C_init, huber_chi, damping, iterations, cg_iterations, cg_tol)
        return {key: t[0] for key, t in zip(lib.POSE_GRAPH_SPARSE_KEYS, res)}

    def alloc_pose_window(self, window: int, spacings, capacity: int = 4096, n_windows: int = 1) -> dict:
        """The buffers of pose_window_step() (csrc_window/window.hip) for n_windows sliding windows of `window` frames over the
        pairs (t - s, t) of `spacings` (distinct positive ints): "state" - lib.alloc_window_state's fresh state, with the trajectory of
        the first `capacity` frames -, "out" - lib.alloc_window_out's outputs -, "spacings" (S,) int32 and "workspace", all on this
        pipeline's device.  A spacing of `window` or more is allowed and never admitted."""
        from .online import _checked_spacings             # online imports this module
        sp = _checked_spacings(spacings, below=2 ** 31)
        w, s, cap, nw = lib.check_window_sizes(window, len(sp), capacity, n_windows)
        dev = self.device
        return dict(state=lib.alloc_window_state(w, s, cap, nw, dev), out=lib.alloc_window_out(w, s, nw, dev),
                    spacings=torch.tensor(sp, dtype=torch.int32, device=dev),
                    workspace=torch.empty(lib.window_workspace_bytes(nw, w, s), dtype=torch.uint8, device=dev))

    @staticmethod
    def pose_window_step(state: dict, refined: dict, out: dict | None = None, min_inliers: int = 12, huber_chi: float = 4.0,
                         damping: float = 0.0, iterations: int = 2) -> dict:
        """One frame of the online estimator (sslw_window_step, include/sslam_window.h): the S refined pairs of this frame - `refined`,
        the dictionary refine_poses() returned for the pairs (t - spacings[k], t) in the order of the spacings; its T, info, status
        and inlier_count are read, (S, ...) rows for one window or (n_windows * S, ...) - enter the ring of `state`
        (alloc_pose_window's dictionary), the frame's pose is predicted from the nearest admitted pair, and the window's poses are
        optimised with its oldest frame held.  A pair is admitted when its frame is in the window, its status is not 3, it has at
        least min_inliers inliers and its numbers are finite.  huber_chi, damping, iterations: as optimize_pose_graph takes them;
        frame 0 stands at [I | 0] (lib.window_step takes a start pose).  Returns lib.WINDOW_OUT_KEYS' device tensors - `out`, or the
        state's own "out" buffers.  One launch, no host read: the frame counter is device memory, so the call can be captured."""
        if not isinstance(state, dict) or any(k not in state for k in ("state", "out", "spacings", "workspace")):
            raise ValueError("state must be alloc_pose_window()'s dictionary")
        if not isinstance(refined, dict) or any(k not in refined for k in ("T", "info", "status", "inlier_count")):
            raise ValueError("refined must be refine_poses()' dictionary: T, info, status and inlier_count are read")
        s = int(state["spacings"].shape[0])
        nw = int(state["state"]["t"].shape[0])
        rows = {}
        for key, tail in (("T", (12,)), ("info", (21,)), ("status", ()), ("inlier_count", ())):
            t = refined[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (nw * s,) + tail or not t.is_contiguous():
                raise ValueError(f"refined `{key}` must be a contiguous tensor of shape {(nw * s,) + tail}")
            rows[key] = t.view((nw, s) + tail)
        return lib.window_step(state["state"], state["spacings"], rows["T"], rows["info"], rows["status"], rows["inlier_count"], None,
                               min_inliers, huber_chi, damping, iterations, out=state["out"] if out is None else out,
                               workspace=state["workspace"])

    def alloc_place_bank(self, capacity: int, min_gap: int = 30, min_sim: float = 0.3, per_frame: int = 2, suppress: int = 5) -> dict:
        """The buffers of place_step() (csrc_place/place.hip) for a place bank of up to `capacity` frames (1 .. 4096) at this
        pipeline's descriptor width: "state" - lib.alloc_place_state's fresh state -, "out" - lib.alloc_place_out's outputs -,
        "workspace", and the retrieval's arguments min_gap, min_sim, per_frame, suppress as find_loop_candidates takes them."""
        gap, sim, per, sup = lib.check_loop_arguments(min_gap, min_sim, per_frame, suppress)
        cap, _, d = lib.check_place_sizes(capacity, 1, self.descriptor_dim)
        dev = self.device
        return dict(state=lib.alloc_place_state(cap, d, dev), out=lib.alloc_place_out(per, d, dev), min_gap=gap, min_sim=sim, per_frame=per,
                    suppress=sup, workspace=torch.empty(lib.place_workspace_bytes(cap), dtype=torch.uint8, device=dev))

    @staticmethod
    def place_step(state: dict, descriptors, scores, out: dict | None = None) -> dict:
        """One frame of the online loop retrieval (sslp_place_step, include/sslam_place.h): the frame's descriptors (K, D) or
        (1, K, D) and scores, as extract() returned them, enter the bank of `state` (alloc_place_bank's dictionary), and the frame's
        most similar older frames come back in match_pairs' pair-list form: first, second (per_frame,) int32 global frame indices
        (-1, -1 an empty slot), sim, count, status (1,) and sig (D,) - row t of find_loop_candidates over the frames so far, bit for
        bit; status 4 and an absent row once the bank is full.  Returns `out`, or the state's own "out" buffers.  Three launches, no
        host read: the frame counter is device memory, so the call can be captured."""
        if not isinstance(state, dict) or any(k not in state for k in ("state", "out", "workspace", "min_gap", "min_sim", "per_frame", "suppress")):
            raise ValueError("state must be alloc_place_bank()'s dictionary")
        return lib.place_step(state["state"], descriptors, scores, state["min_gap"], state["min_sim"], state["per_frame"], state["suppress"],
                              out=state["out"] if out is None else out, workspace=state["workspace"])

    def alloc_edge_log(self, capacity: int, n_slots: int) -> dict:
        """The buffers of edge_log_step() for `capacity` frames of n_slots (1 .. 16) pairs each: "state" - lib.alloc_edge_log's fresh
        log - and "out" - logged (n_slots,), status (1,)."""
        cap, e = lib.check_edge_log_sizes(capacity, n_slots)
        dev = self.device
        return dict(state=lib.alloc_edge_log(cap, e, dev),
                    out={k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in lib.edge_log_out_shapes(e).items()})

    @staticmethod
    def edge_log_step(log: dict, slot_first, refined: dict, n_odometry: int, min_inliers: int = 12, loop_min_inliers: int = 12,
                      out: dict | None = None) -> dict:
        """One frame of the edge log (sslp_edge_log_step): the frame's E refined pairs - `refined`, refine_poses()' dictionary, whose T,
        info, status and inlier_count are read; slot_first (E,) int32, the GLOBAL index of each pair's older frame, -1 for none - are
        appended to `log` (alloc_edge_log's dictionary) as row t * E + e.  The first n_odometry slots are logged with at least
        min_inliers inliers, the others with loop_min_inliers; a slot that fails a test is logged absent.  The log's first n * E rows
        are optimize_pose_graph_sparse's operands over the n frames logged.  Returns logged (E,), status (1,) - `out`, or the log's
        own.  One launch, no host read."""
        if not isinstance(log, dict) or any(k not in log for k in ("state", "out")):
            raise ValueError("log must be alloc_edge_log()'s dictionary")
        if not isinstance(refined, dict) or any(k not in refined for k in ("T", "info", "status", "inlier_count")):
            raise ValueError("refined must be refine_poses()' dictionary: T, info, status and inlier_count are read")
        return lib.edge_log_step(log["state"], slot_first, refined["T"], refined["info"], refined["status"], refined["inlier_count"], n_odometry,
                                 min_inliers, loop_min_inliers, out=log["out"] if out is None else out)

    @staticmethod
    def _link_mask(mask):
        """mask of link_matches() / track_step(): None, an int32 tensor, or the dictionary of estimate_poses() / refine_poses(),
        whose inlier_of_slot is read."""
        return mask["inlier_of_slot"] if isinstance(mask, dict) and "inlier_of_slot" in mask else mask

    def link_matches(self, first, second, matches: dict, mask=None, n_frames: int | None = None, k: int | None = None,
                     out: dict | None = None) -> dict:
        """Match lists to links (sslt_link_pairs, include/sslam_track.h): first / second as match_pairs takes them, matches the
        dictionary a matcher or rank_matches() returned for them, mask None or the inlier_of_slot (P, n1) int32 of estimate_poses()
        or refine_poses() (or that dictionary): only slots with mask == 1 count.  n_frames: the frames of the bank, required; k: its
        slots per frame, num_keypoints by default.  A row links iff first < second and it is the lowest row with that second and
        with that first; a slot links iff it is the lowest valid slot naming its idx1 and its idx2.  Returns prev, next (n_frames, k),
        prev_frame, next_frame (n_frames,) int32 device tensors, -1 meaning none.  Five launches, no host read."""
        if n_frames is None:
            raise ValueError("link_matches needs n_frames=, the number of frames of the bank")
        first, second = _host_pair_list("first", first), _host_pair_list("second", second)
        n_pairs = lib.check_pair_lists(first, second)
        mt = _checked_match_lists(matches, n_pairs)
        first, second = (x if x.is_cuda else x.to(mt.device) for x in (first, second))
        return lib.link_pairs(first, second, mt, matches["match_count"], n_frames, self.cfg.num_keypoints if k is None else k,
                              mask=self._link_mask(mask), out=out)

    @staticmethod
    def track_ids(links: dict, out: dict | None = None, workspace=None) -> dict:
        """Links to tracks (sslt_track_ids): links is link_matches()' dictionary (prev and prev_frame are read) or a track bank's
        state.  Returns the links and track_id, age (n_frames, k), n_tracks (1,), root_frame, root_slot, length (n_frames * k,) int32
        in ONE dictionary - landmarks()' `tracks`: roots numbered in ascending (frame, slot) order, a keypoint without a link a
        track of length 1.  5 + ceil(log2 n_frames) launches, no host read."""
        if not isinstance(links, dict) or any(key not in links for key in lib.LINK_KEYS):
            raise ValueError(f"links must be link_matches()' dictionary: {', '.join(lib.LINK_KEYS)}")
        return {**{key: links[key] for key in lib.LINK_KEYS}, **lib.track_ids(links["prev"], links["prev_frame"], out=out, workspace=workspace)}

    def landmarks(self, keypoints_pixel, kp_depth, C, tracks: dict, camera, threshold: float = 3.0, min_obs: int = 2, weights=None,
                  out: dict | None = None) -> dict:
        """Tracks to map points (sslt_landmarks): keypoints_pixel (N, K, 2), kp_depth (N, K) as the pose methods take them, C (N, 12)
        float64 world -> camera poses - a graph's C -, tracks: track_ids()' dictionary, camera as estimate_poses takes it.  weights:
        None (1 for every keypoint) or extract()'s `confidence` (N, K) float32 as it is.  Per track: the weighted mean of the
        observations' world points, the observations within `threshold` (keypoint units) of its reprojection are kept, and with
        min_obs of them the mean is taken again over those.  Returns lib.LANDMARK_KEYS' device tensors.  Two launches, no host read."""
        if not isinstance(tracks, dict) or any(key not in tracks for key in ("next", "next_frame", "root_frame", "root_slot", "n_tracks")):
            raise ValueError("tracks must be track_ids()' dictionary: next, next_frame, root_frame, root_slot and n_tracks are read")
        sx, sy = self.depth_scales(camera)
        return lib.landmarks(keypoints_pixel, kp_depth, C, camera, tracks["next"], tracks["next_frame"], tracks["root_frame"],
                             tracks["root_slot"], tracks["n_tracks"], weights, sx, sy, threshold, min_obs, out=out)

    def alloc_track_bank(self, capacity: int, k: int | None = None) -> dict:
        """The buffers of track_step() for a track bank of up to `capacity` frames of k slots (num_keypoints by default): "state" -
        lib.alloc_track_state's fresh state - and "out" - lib.alloc_track_out's outputs."""
        kk = self.cfg.num_keypoints if k is None else k
        return dict(state=lib.alloc_track_state(capacity, kk, self.device), out=lib.alloc_track_out(kk, self.device))

    @staticmethod
    def track_step(state: dict, matches_row: dict, first, mask=None, row: int = 0, out: dict | None = None) -> dict:
        """One frame of the online tracks (sslt_track_step): row `row` of matches_row - a matcher's dictionary for this step's pairs -
        is the link row (first, this frame); first: a (1,) int32 DEVICE tensor, the bank frame of the row's first member, -1 for
        none (the first frame); mask as link_matches takes it.  Returns this frame's track_id, age (k,), n_new, status (1,) - `out`,
        or the bank's own.  After n steps the bank's rows equal link_matches() + track_ids() over the rows stepped so far, bit for
        bit.  One launch, no host value, no host read: the call can be captured."""
        if not isinstance(state, dict) or any(key not in state for key in ("state", "out")):
            raise ValueError("state must be alloc_track_bank()'s dictionary")
        if not isinstance(matches_row, dict) or any(key not in matches_row for key in ("matches", "match_count")):
            raise ValueError("matches_row must be a matcher's dictionary: matches and match_count are read")
        mk = SequencePipeline._link_mask(mask)
        return lib.track_step(state["state"], matches_row["matches"][row:row + 1], matches_row["match_count"][row:row + 1], first,
                              mask=None if mk is None else mk[row:row + 1], out=state["out"] if out is None else out)

    def validation_stats(self, out: dict, images: torch.Tensor, spacing: int | None = None, first=None, second=None,
                         temperature: float = 0.1) -> dict:
        """The validation stage (csrc/validate.hip): the per-frame and per-pair statistics from which validation.compose puts
        together the trainer's seven loss terms and five metrics (train.py:292-408 under no_grad), for the N frames `out` holds
        (what extract() / run() returned: saliency (N, G, G), descriptors (N, K, descriptor_dim)) and the pairs (i, i + spacing) - or the
        listed pairs first / second, as match_pairs takes them (1-D int32 device tensors or host sequences; -1 = absent pair:
        zero rows, which compose refuses).
        images: (N, H, W, 3) uint8 - resampled here by A0 into the fp32 ViT input, a launch group at a time - or that fp32
        image itself, (N, 3, S, S) with S = input_size.
        Only launches on the current stream (a fixed number for given shapes), no host read-back: capturable.
        Returns device tensors: per frame sal_mean, sal_var, sal_max, sal_dx, sal_dy, sal_high, sal_ss, edge_a, edge_e,
        edge_mean, edge_max (N,), desc_mean, desc_m2 (N, descriptor_dim), pooled (N, G, G); per pair first, second (int32), repeat,
        ce_sum, pad_ce (P,), n_matches (P,) int32, lse, ce, sim (P, K), nn12, nn21 (P, K) int32; and the numbers grid,
        num_keypoints, temperature."""
        cfg = self.cfg
        t = lib.check_temperature(temperature)
        sal, desc = out["saliency"], out["descriptors"]
        n, k, g, dw = int(desc.shape[0]), int(desc.shape[1]), cfg.grid, self._desc_width(desc)
        if tuple(sal.shape) != (n, g, g):
            raise ValueError(f"saliency {tuple(sal.shape)} does not go with {n} frames of a {g} x {g} grid")
        listed = first is not None or second is not None
        if listed:
            if first is None or second is None:
                raise ValueError("validation_stats needs both pair lists, first= and second=")
            if spacing is not None:
                raise ValueError("give spacing= or the two pair lists, not both")
            first, second = _host_pair_list("first", first), _host_pair_list("second", second)
            n_pairs = lib.check_pair_lists(first, second)
        else:
            sp = cfg.spacing if spacing is None else spacing
            if isinstance(sp, bool) or not isinstance(sp, numbers.Integral) or sp < 1:
                raise ValueError(f"spacing must be an integer >= 1, got {sp!r}")
            n_pairs = n - int(sp)
            if n_pairs <= 0:
                raise ValueError(f"{n} frames hold no pair at spacing {sp}")
        if not isinstance(images, torch.Tensor) or images.shape[0] != n:
            raise ValueError(f"images must be a tensor of the same {n} frames")
        if images.dtype == torch.uint8:
            if images.dim() != 4 or images.shape[3] != 3:
                raise ValueError("uint8 images must have shape (N, H, W, 3)")
        elif images.dtype != torch.float32 or tuple(images.shape[1:]) != (3, cfg.input_size, cfg.input_size):
            raise ValueError(f"images must be uint8 (N, H, W, 3) or fp32 (N, 3, {cfg.input_size}, {cfg.input_size})")
        dev = desc.device
        # ---- per frame: Sobel / pool over the fp32 image, then one workgroup per frame
        pooled = torch.empty((n, g, g), dtype=torch.float32, device=dev)
        emax = torch.empty((n,), dtype=torch.float32, device=dev)
        step = self.launch_group()
        for a in range(0, n, step):
            b = min(a + step, n)
            img = self.preprocess(images[a:b], reuse=True) if images.dtype == torch.uint8 else images[a:b]
            lib.edge_pool(img, out=(pooled[a:b], emax[a:b]))
        fstats, dmean, dm2 = lib.val_frame_stats(sal, pooled, emax, desc)
        res = {key: fstats[:, slot] for key, slot in lib.VAL_FRAME_SLOTS.items()}
        res.update(desc_mean=dmean, desc_m2=dm2, pooled=pooled)
        # ---- per pair: the arg-max launch gives the row maxima the log-sum-exp launch starts from
        if listed:
            first, second = (x if x.is_cuda else x.to(dev) for x in (first, second))
            lib.check_pair_lists(first, second, dev)
        else:
            first = torch.arange(n_pairs, dtype=torch.int32, device=dev)
            second = first + int(sp)
        parts = []
        for a in range(0, n_pairs, MAX_PAIRS_PER_LAUNCH):       # cut as match() cuts
            m = min(MAX_PAIRS_PER_LAUNCH, n_pairs - a)
            if listed:
                f, s = first[a:a + m], second[a:a + m]
                nn12, s12, nn21, _, _ = lib.sim_argmax_pairs(desc, f, s, workspace=self.workspace(0, m))
                lse, ce, s00 = lib.row_lse_pairs(desc, f, s, s12, t)
                pstats, cnt = lib.val_pair_stats_pairs(sal, f, s, nn12, nn21, s12, ce, s00, t)
            else:
                d1, d2 = desc[a:a + m], desc[a + sp:a + sp + m]
                nn12, s12, nn21, _, _ = lib.sim_argmax(d1, k * dw, k, d2, k * dw, k, m, workspace=self.workspace(0, m))
                lse, ce, s00 = lib.row_lse(d1, k * dw, k, d2, k * dw, k, m, s12, t)
                pstats, cnt = lib.val_pair_stats(sal[a:a + m], sal[a + sp:a + sp + m], nn12, nn21, s12, ce, s00, t)
            parts.append(dict(pstats=pstats, n_matches=cnt, lse=lse, ce=ce, sim=s12, nn12=nn12, nn21=nn21))
        cat = {key: parts[0][key] if len(parts) == 1 else torch.cat([x[key] for x in parts]) for key in parts[0]}
        pstats = cat.pop("pstats")
        res.update(cat)
        res.update({key: pstats[:, slot] for key, slot in lib.VAL_PAIR_SLOTS.items() if key != "matches"})
        res.update(first=first, second=second, grid=g, num_keypoints=k, temperature=t)
        return res

    def run(self, images_u8: torch.Tensor | None, tokens: torch.Tensor | None = None, with_preprocess: bool = False) -> dict:
        """One pass of the hot path over a frame sequence: extract every frame once, match (i, i+spacing).
        tokens=None: compute them from the images with the HIP ViT (A0 + A1)."""
        cfg = self.cfg
        if tokens is None:
            tokens = self.tokens_from_images(images_u8)
            with_preprocess = False
        vit_in = None
        if with_preprocess and images_u8 is not None:
            step = self.launch_group()
            for a in range(0, images_u8.shape[0], step):
                vit_in = self.preprocess(images_u8[a:a + step], reuse=True)      # A0: would feed the ViT (A1)
        out = dict(self.extract(tokens, images_u8))
        out.update(self.match(out["descriptors"], out["scores"], out.get("intensity")))
        if vit_in is not None:
            out["vit_input_last_chunk"] = vit_in
        return out
