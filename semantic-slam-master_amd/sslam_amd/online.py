"""The ONLINE caller's step - one frame in, its features and the matches against the previous frame out - on static buffers,
optionally replayed from a HIP graph.

Every caller the reference has works frame by frame (B = 1): `visualize_matches_sequence.py:306-357` extracts and matches pair
by pair, `test/test_tracking.py:146-178` keeps the previous frame's descriptors and matches each new frame against them,
`test/test_performance.py:89-131` times one image at a time (the "143 FPS" of its notes is that protocol).  `FrameStepper` is
that loop on the HIP path: the frame is copied into a static buffer, A0 -> A1 -> A2 .. A9 run on it, M1 matches it against the
previous frame's descriptors (kept on the device), and the frame's descriptors become the previous ones - no concatenation, no
allocation per frame, no host synchronisation (the caller reads what it wants from the returned views).

`use_graph=True` captures that step ONCE with `torch.cuda.graph` (hipGraph underneath) and replays it: one graph launch instead
of 8 (tokens in) / 72 (bf16 ViT inside) / 96 (fp32 ViT inside) library calls.  The C ABI was shaped for this (no allocation, no
synchronisation, no host read-back inside the library; caller-owned workspace), and the replay is bit-identical - but MEASURED it
buys nothing on this chip: 0.297 against 0.289 ms per frame with tokens in, 1.215 against 1.209 ms with the bf16 ViT inside,
2.12 against 2.11 ms with the fp32 ViT (tools/online_probe.py).  At B = 1 the step is bound by the DURATION of its ~70 dependent
kernels (a frame is 7 row tiles: most launches occupy a few dozen of the 256 CUs for 5-20 us each), not by the host's launch rate -
the host is already ahead of the device.  It is kept as an option because it takes the host out of the loop (0 library calls per
frame), which matters to a caller that has other work for its CPU thread.

Results are the kernels' results: bit-identical to the same frames going through `SequencePipeline.run` as one batch of up to 8
frames (tests/test_gpu_harness.py::test_online_stepper_*).  A step is a batch of ONE frame, so the ViT inside runs its few-frame
form (fp32: key-split attention; bf16: the small form) whatever sequence it steps through; a longer batch's tokens (fp32 one-pass,
bf16 fused MLP) agree with a step's within the float64 bars, not bit for bit (test_frame_stepper_runs_the_few_frame_form).
A pipeline built with vit_form="few_frame" steps in the bf16 ViT's FEW-FRAME form instead (key-split attention, K-split down
projection: include/sslam_hip.h) - the stepper itself takes no argument for it, a step being a batch of one - as ordinary launches
and from the captured graph alike (one stream, no parallel branches; the larger workspace is among the buffers the stepper holds);
its steps equal that pipeline's run() over up to 8 frames bit for bit (tests/test_gpu_vit_few_frame.py).

`spacings=(1, 5, 10, 15, 20)` (any distinct positive ints) makes a step match the frame against SEVERAL earlier frames - the
reference's own five spacings (visualize_matches_sequence.py:369), or a front end's "this frame against my last few" - still on
static buffers and from one captured graph.  The frames live in a bank of max(spacings) + 1 slots: slot max(spacings) is the
static slot the extraction writes, the others are a ring, frame j in slot j mod max(spacings).  The step counter t is DEVICE
memory, and the body derives from it, with a handful of torch ops on the stream, the matcher's pair list (first[s] = the slot of
frame t - s, or -1 while t < s: an absent pair; second = the static slot), runs ONE sslam_sim_argmax_pairs +
sslam_match_finalize_pairs over all spacings (include/sslam_hip.h: the pair list is read by the kernels), copies the frame into
ring slot t mod max(spacings) with a device-indexed copy and increments t.  No host value that changes between steps enters the
body, so the replayed graph is the same step for every frame.  `spacings=None` is the one-spacing stepper above, untouched.

`WindowPoseFrameStepper` puts the pose stage and the sliding-window estimator (include/sslam_window.h) behind that multi-spacing
matcher, still in the one captured step: the frame's trajectory while the sequence runs, not after it has ended.
`LoopWindowPoseFrameStepper` adds loop closures to it (include/sslam_place.h): a place bank that grows by one frame per step proposes
older frames, they are verified with the step's other pairs, and every verified pair goes to an edge log the sparse pose graph reads
on demand (close_loops()).
"""
from __future__ import annotations

import torch

from . import lib
from .pipeline import N_PREFIX, GraphSettings, PoseSettings, SequencePipeline, _checked_rule
from .readback import Readback


BANK_KEYS = ("descriptors", "scores", "intensity", "keypoints_pixel")      # what an earlier frame is kept for


def bank_keys(pipe) -> tuple:
    """BANK_KEYS, extended by the refined keypoints and their flags when the pipeline localises them (ExtractorConfig.subcell)."""
    return BANK_KEYS + (lib.SUBCELL_KEYS if pipe.cfg.subcell else ())


def _checked_spacings(spacings, below=None) -> tuple:
    """below: the spacings must also be smaller than it (the pose window keeps them as int32 on the device)."""
    if isinstance(spacings, (str, bytes)) or not hasattr(spacings, "__iter__"):
        raise ValueError(f"spacings must be a sequence of distinct positive ints, got {spacings!r}")
    sp = tuple(spacings)
    if not sp or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 or (below is not None and s >= below) for s in sp) or \
            len(set(sp)) != len(sp):
        raise ValueError(f"spacings must be a non-empty sequence of distinct positive ints, got {spacings!r}")
    return sp


class FrameStepper:
    rule = None         # M1.  Only RuleFrameStepper (below) sets a pipeline.MatchRule, in its constructor; with None every call
                        # this class makes into the pipeline is the call it made before rules existed (_rule_kw)

    def __init__(self, pipe: SequencePipeline, height: int, width: int, use_graph: bool = True, tokens_in: bool = False,
                 spacings=None):
        """pipe: a SequencePipeline (with vit= unless tokens_in).  height / width: the frames' size (uint8 RGB).
        tokens_in: the caller brings the ViT's tokens with every frame (the third-party ViT stays outside).
        use_graph=False: the same step as ordinary launches (the A/B for the graph, and the fallback while debugging).
        With the ViT inside, every step runs its few-frame form (a batch of one): the tokens of SequencePipeline.run over up to
        8 frames bit for bit, those of a longer batch within the float64 bars (module docstring).  Which few-frame form the bf16
        ViT runs is the pipeline's choice (SequencePipeline(vit_form=...)): the small form by default, "few_frame" by name.
        spacings: None - match against the previous frame (above); a sequence of distinct positive ints - match every frame
        against the frames that many steps back, all in one launch pair (module docstring; step() says what comes back).
        The matcher is M1; the class attribute `rule` is set only by the subclass RuleFrameStepper."""
        if spacings is not None:
            spacings = _checked_spacings(spacings)       # before anything is allocated
        cfg = pipe.cfg
        if cfg.num_keypoints > cfg.grid ** 2:
            raise ValueError("num_keypoints > grid cells: that case reads a status word back on the host (SURVEY H6) and cannot be captured")
        if not tokens_in and pipe.vit_hip is None:
            raise lib.SslamHipError("this pipeline was built without a ViT: pass tokens_in=True, or construct it with vit=")
        self.pipe, self.cfg, self.device = pipe, cfg, pipe.device
        self.tokens_in, self.use_graph = tokens_in, use_graph
        self.bank_keys = bank_keys(pipe)
        dev, K = self.device, cfg.num_keypoints
        self.image = torch.zeros((1, height, width, 3), dtype=torch.uint8, device=dev)
        self.tokens = torch.zeros((1, N_PREFIX + cfg.grid ** 2, lib.C_FEAT), dtype=torch.float32, device=dev)
        self.spacings = spacings
        self.n_frames = 0
        self._graph = None
        self._aux = None
        self._held = None
        if spacings is not None:
            self._init_bank(spacings)
            return
        # slot 0: the previous frame, slot 1: this frame - the matcher's pair (0, 1) without any concatenation
        self.pair = pipe.alloc_extract(2, True)
        for v in self.pair.values():
            v.zero_()
        self.cur = {k: v[1:2] for k, v in self.pair.items()}
        self.m = pipe.alloc_match(1, K, **self._rule_kw())

    def _rule_kw(self) -> dict:
        """rule None adds no argument to a pipeline call (harness.StreamingSequence's convention: a pipeline that knows no `rule`
        still serves the stepper without one)."""
        return {} if self.rule is None else {"rule": self.rule}

    def _after_match(self) -> None:
        """What a subclass enqueues behind the matcher's finalize launch, on the same stream (RankedFrameStepper: the rank launch)."""

    def _ring_size(self, spacings: tuple) -> int:
        """The slots of the feature ring: the furthest a spacing reaches back.  LoopWindowPoseFrameStepper keeps more."""
        return max(spacings)

    def _extra_pairs(self) -> int:
        """Rows the step's ONE pair list holds behind the spacings' (LoopWindowPoseFrameStepper: its loop candidates)."""
        return 0

    def _before_match(self) -> None:
        """What a subclass enqueues between the extraction and the matcher, on the same stream; it may fill the extra pairs."""

    def _init_bank(self, spacings: tuple) -> None:
        pipe, dev = self.pipe, self.device
        ring = self.ring = self._ring_size(spacings)
        one = pipe.alloc_extract(1, True)
        for v in one.values():
            v.zero_()
        # slots 0 .. ring - 1: frame j in slot j mod ring; slot `ring`: the static slot of the frame being extracted
        self.bank = {k: torch.zeros((ring + 1,) + tuple(one[k].shape[1:]), dtype=one[k].dtype, device=dev) for k in self.bank_keys}
        self._ring = {k: v[:ring] for k, v in self.bank.items()}
        self.cur = {k: (self.bank[k][ring:ring + 1] if k in self.bank_keys else v) for k, v in one.items()}
        pairs = len(spacings) + self._extra_pairs()
        self.m = pipe.alloc_match(pairs, self.cfg.num_keypoints, **self._rule_kw())
        i64 = dict(dtype=torch.int64, device=dev)
        self._t = torch.zeros((1,), **i64)                                   # the step counter: frames since reset()
        self._sp = torch.tensor(spacings, **i64)
        self._back, self._back_slot, self._first64 = (torch.zeros((len(spacings),), **i64) for _ in range(3))
        self._seen = torch.zeros((len(spacings),), dtype=torch.bool, device=dev)
        self._absent = torch.full((len(spacings),), -1, **i64)
        self._slot = torch.zeros((1,), **i64)
        self.pair_first = torch.full((pairs,), -1, dtype=torch.int32, device=dev)               # the matcher's pair lists
        self.pair_second = torch.full((pairs,), ring, dtype=torch.int32, device=dev)
        # the spacings' rows: the whole lists, unless a subclass asked for extra pairs behind them
        self.first_slot, self.second_slot = self.pair_first[:len(spacings)], self.pair_second[:len(spacings)]

    # the captured region: only launches on the current stream, static buffers on both sides
    def _body(self) -> None:
        p = self.pipe
        if self.spacings is not None:
            return self._body_spacings()
        if not self.tokens_in:
            p.tokens_from_images(self.image, out=self.tokens)
        p.extract(self.tokens, self.image, out=self.cur)
        self._aux = p.match(self.pair["descriptors"], self.pair["scores"], self.pair["intensity"], spacing=1, out=self.m,
                            **self._rule_kw())
        self._after_match()
        for k in self.bank_keys:      # this frame becomes the previous one
            self.pair[k][0].copy_(self.pair[k][1])

    def _body_spacings(self) -> None:
        p, ring = self.pipe, self.ring
        if not self.tokens_in:
            p.tokens_from_images(self.image, out=self.tokens)
        p.extract(self.tokens, self.image, out=self.cur)
        # the pair list from the device's own counter t: frame t - s sits in ring slot (t - s) mod ring once t >= s, else -1
        torch.sub(self._t, self._sp, out=self._back)
        torch.ge(self._back, 0, out=self._seen)
        torch.remainder(self._back, ring, out=self._back_slot)
        torch.where(self._seen, self._back_slot, self._absent, out=self._first64)
        self.first_slot.copy_(self._first64)
        self._before_match()
        self._aux = p.match_pairs(self.bank["descriptors"], self.bank["scores"], self.bank["intensity"], first=self.pair_first,
                                  second=self.pair_second, out=self.m, **self._rule_kw())
        self._after_match()
        # this frame takes the ring slot of frame t - ring, which no spacing reaches any more
        torch.remainder(self._t, ring, out=self._slot)
        for k in self.bank_keys:
            self._ring[k].index_copy_(0, self._slot, self.cur[k])
        self._t.add_(1)

    def _capture(self) -> None:
        # warm-up outside the capture: resampling tables, RoPE tables, workspaces and the ViT's buffers are created on first use
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._body()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        if self.spacings is not None:
            self._t.zero_()                      # the warm-up passes counted as frames: the first real frame is frame 0
        # The graph bakes in the ADDRESSES of buffers the stepper does not own: the pipeline's scratch, the ViT's workspaces, the
        # resampling and RoPE tables.  Their owners grow them by replacement (a later, larger pipe.run / tokens_from_images drops
        # the old tensor), which would leave the graph reading and writing freed memory.  The stepper therefore keeps its own
        # reference to every one of them from the warm-up on: a replaced buffer stays alive - and exclusively the graph's - for
        # as long as the graph does.  (The bank, the counter and the pair lists of the multi-spacing step are the stepper's own.)
        self._held = self._external_buffers()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._body()
        self._graph = g

    def _external_buffers(self) -> list:
        p, held = self.pipe, []
        held.append(p._ws)
        held.extend(p._stage.values())
        held.extend(p.tables._cache.values())
        vh = p.vit_hip
        if vh is not None:
            held.extend(getattr(vh, "_side_ws", []) or [])
            held.extend(getattr(vh, "_ws", []) or [])
            held.extend(vh._rope.values())
            held.append(vh._keep)
        return held

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        """image_u8: (H, W, 3) or (1, H, W, 3) uint8, on the device or in host memory (pinned: the copy is asynchronous).
        tokens: (T, 384) / (1, T, 384) fp32 when the stepper was built with tokens_in.  Returns this frame's saliency /
        keypoints_pixel / scores / idx / descriptors / intensity - and, on a pipeline with subcell=True, keypoints_subpatch /
        keypoints_subpixel / subcell_flags, whose launch is part of the captured graph, and on one with confidence=True the
        frame's `confidence` (K,), its launch captured likewise (the stepper allocates through alloc_extract; the confidence
        is returned per frame and not kept in the bank) - (views of static buffers, (K, ...) without
        the batch axis) and,
        from the second frame on, matches (K, 2) int64 / quality (K,) / match_count against the previous frame (None before).
        With spacings: matches (S, K, 2) / quality (S, K) / match_count (S,), one row per spacing in the order given (views of
        static buffers; a spacing that reaches back before the first frame has count 0 and zero rows), and pair_first: a host
        list of the global index of each row's first frame, -1 where there is none yet.  The second frame is this one.
        Under a rule (RuleFrameStepper) `value` takes the place of `quality` everywhere above."""
        if self.use_graph and self._graph is None:
            self._capture()                      # runs the body on whatever the buffers hold; the first real frame has no previous one
        self.image.copy_(image_u8.reshape(self.image.shape), non_blocking=True)
        if self.tokens_in:
            if tokens is None:
                raise ValueError("this stepper takes the frame's tokens (tokens_in=True)")
            self.tokens.copy_(tokens.reshape(self.tokens.shape), non_blocking=True)
        if self.use_graph:
            self._graph.replay()
        else:
            self._body()
        first = self.n_frames == 0
        self.n_frames += 1
        out = {k: v[0] for k, v in self.cur.items()}
        val = "quality" if self.rule is None else "value"
        if self.spacings is not None:
            t = self.n_frames - 1
            out.update(matches=self.m["matches"], match_count=self.m["match_count"],
                       pair_first=[t - s if t >= s else -1 for s in self.spacings])
            out[val] = self.m[val]
            return out
        out["matches"] = None if first else self.m["matches"][0]
        out[val] = None if first else self.m[val][0]
        out["match_count"] = None if first else self.m["match_count"][0]
        return out

    def reset(self) -> None:
        """Forget the previous frame (the next step returns no matches); with spacings: every earlier frame - the device's
        counter is zeroed here, outside the graph."""
        self.n_frames = 0
        if self.spacings is not None:
            self._t.zero_()

    def frame(self, index: int) -> dict:
        """With spacings: the bank rows (descriptors, scores, intensity, keypoints_pixel; with subcell=True the refined keypoints
        and their flags too) of the frame with global index `index`,
        one of the last max(spacings) stepped - what a pair_first entry names."""
        if self.spacings is None or not max(0, self.n_frames - self.ring) <= index < self.n_frames:
            raise ValueError(f"frame {index} is not in the bank")
        return {k: v[index % self.ring] for k, v in self.bank.items()}


class RuleFrameStepper(FrameStepper):
    """FrameStepper whose matcher stage applies a pipeline.MatchRule - the ratio tests M2 / M4, or M5's tracking count, which is
    the loop of test/test_tracking.py:146-178 as it stands: keep the previous descriptors, count the rows whose best similarity
    exceeds 0.8.  Same step, same buffers, one-spacing body and spacings= body, ordinary launches and the captured graph: the
    rule's finalize kernel stands where M1's stood (and, for tracked, the rows-only similarity launch where the two-direction one
    stood) on the same one stream - no parallel branches, no host value entering the body; rule and threshold are baked in like
    the M1 thresholds are.  step() returns `value` in place of `quality`.
    A class of its own, since FrameStepper's constructor signature is pinned by its tests; rule=None is FrameStepper."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, use_graph: bool = True, tokens_in: bool = False,
                 spacings=None, rule=None):
        self.rule = _checked_rule(rule, pipe.cfg.num_keypoints)      # before anything is allocated
        super().__init__(pipe, height, width, use_graph=use_graph, tokens_in=tokens_in, spacings=spacings)

    def _take_depth(self, depth_u16) -> None:
        """The depth input of the steppers that take one (they own self.depth, the static buffer): the frame's raw depth image is
        judged, the step captured first if it has not been - before the frame's depth goes into its static buffer, as the image
        does in FrameStepper.step - and the image copied."""
        if not isinstance(depth_u16, torch.Tensor) or depth_u16.dtype != torch.uint16 or depth_u16.numel() != self.depth.numel():
            raise ValueError(f"depth_u16 must be a uint16 tensor of shape {tuple(self.depth.shape[1:])}")
        if self.use_graph and self._graph is None:
            self._capture()
        self.depth.copy_(depth_u16.reshape(self.depth.shape), non_blocking=True)


class RankedFrameStepper(RuleFrameStepper):
    """RuleFrameStepper whose step also ranks: behind the finalize launch, on the same one stream, sslam_match_rank keeps the
    `best` best matches of every pair of the step (visualize_matches_sequence.py:224-225; best=50 is that script's --max_matches
    default) - in the one-spacing body and the spacings= body, as ordinary launches and inside the captured graph, where the
    count stays a device value that nothing reads on the host.  step() returns what the parent returns, untouched, plus "best":
    matches (best, 2) / quality | value (best,) / match_count / slot (best,) - with spacings (S, best, 2) / (S, best) / (S,) /
    (S, best) - as views of static buffers (None before the second frame of the one-spacing stepper); rows past the count are
    zero, slot is the row of the step's own match arrays each kept row came from.  rule=None ranks M1's quality; under
    MatchRule.mnn_ratio the smaller distance is the better one (SequencePipeline.rank_matches)."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, use_graph: bool = True, tokens_in: bool = False,
                 spacings=None, rule=None, best: int = 50):
        self.best = lib.check_best(best, pipe.cfg.num_keypoints)      # before anything is allocated
        super().__init__(pipe, height, width, use_graph=use_graph, tokens_in=tokens_in, spacings=spacings, rule=rule)
        self.ranked = pipe.alloc_ranked(1 if self.spacings is None else len(self.spacings), self.best, self.cfg.num_keypoints,
                                        rule=self.rule)

    def _after_match(self) -> None:
        self.pipe.rank_matches(self.m, self.best, rule=self.rule, out=self.ranked)

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        first = self.n_frames == 0
        out = super().step(image_u8, tokens)
        if self.spacings is not None:
            out["best"] = dict(self.ranked)
        else:
            out["best"] = None if first else {k: v[0] for k, v in self.ranked.items()}
        return out


class PoseFrameStepper(RuleFrameStepper):
    """RuleFrameStepper whose step also estimates the camera's motion since the previous frame: the online form of
    sslam_amd.odometry, previous-frame form only (no spacings=).  step() takes the frame's raw depth image beside it; behind the
    finalize launch, on the same one stream - as ordinary launches or inside the captured graph - the depth under this frame's
    keypoints is gathered (sslam_keypoint_depth) into slot 1 of a two-slot bank, sslam_pose_ransac_pairs runs on pair (0, 1) with
    the step's own match list, and slot 1 is handed over to slot 0 as the frame's features are.  The sampler depends on the
    seed alone, not on the pair's place, so a step's pose is bit for bit the row the batched odometry() gives for the same two
    frames.  step() returns what the parent returns plus "pose": T (12,) float64 [R | t] previous camera -> this camera,
    inlier_count, usable_count, best_hypothesis, refit_kept, inlier_of_slot (K,), rms - views of static buffers, None before the
    second frame.  rule: MatchRule.mnn_ratio(0.9) if None, as odometry() has it.
    refine=True puts sslam_pose_refine_pairs behind the RANSAC launch, on the same stream and inside the same graph
    (SequencePipeline.refine_poses from RANSAC's pose: huber, threshold / 3 if None, and iterations as odometry() takes them):
    "pose" keeps RANSAC's keys untouched and gains "refined", the refinement's outputs (T, status, iterations, ..., info (21,)) as
    views of static buffers.  With refine=False no further buffer is allocated and no further launch is made.
    weights: with refine=True on a pipeline with ExtractorConfig(confidence=True), a pipeline.PoseWeights: sslu_match_weights
    makes the step's match weights of the two frames' confidences (self.pair["confidence"], whose slot 1 is handed over to slot 0
    as the depth is) and sslu_pose_refine_weighted_pairs runs in sslam_pose_refine_pairs' place (include/sslam_weight.h), both
    inside the captured step: one launch more per step, "refined" gains weight_sum, and its info is the weighted information
    matrix.  With weights=None there is no new buffer and no new launch."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, depth_height: int, depth_width: int, camera=None,
                 use_graph: bool = True, tokens_in: bool = False, rule=None, threshold: float = 3.0, hypotheses: int = 256,
                 seed: int = 0, refine: bool = False, huber=None, iterations: int = 5, weights=None):
        from .evaluation import Camera, check_depth_size
        from .pipeline import MatchRule
        st = self.settings = PoseSettings(threshold, hypotheses, seed, refine, huber, iterations, weights)      # before anything is allocated
        st.check_pipeline(pipe)
        self.threshold, self.huber, self.refine, self.weights = st.threshold, st.huber, st.refine, st.weights
        self.camera = Camera() if camera is None else camera
        check_depth_size(depth_width, depth_height, self.camera)      # before anything is allocated
        super().__init__(pipe, height, width, use_graph=use_graph, tokens_in=tokens_in, spacings=None,
                         rule=MatchRule.mnn_ratio(0.9) if rule is None else rule)
        dev, K = self.device, self.cfg.num_keypoints
        self.depth = torch.zeros((1, depth_height, depth_width), dtype=torch.uint16, device=dev)
        self.kp_depth = torch.full((2, K), -1, dtype=torch.int32, device=dev)       # slot 0: the previous frame's, slot 1: this frame's
        self._first = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._second = torch.ones((1,), dtype=torch.int32, device=dev)
        self.pose = pipe.alloc_pose(1, K)
        self.refined = pipe.alloc_pose_refine(1, K, weighted=weights is not None) if refine else None
        self.weight = torch.zeros((1, K), dtype=torch.float32, device=dev) if weights is not None else None

    def _after_match(self) -> None:
        p, st = self.pipe, self.settings
        kp = p.geometry_keypoints(self.pair)          # the refined bank on a pipeline with subcell=True, else the cell centres
        p.keypoint_depth(self.depth, kp[1:2], out=self.kp_depth[1:2])
        p.estimate_poses(kp, self.kp_depth, self._first, self._second, self.m, self.camera, st.threshold, st.hypotheses, st.seed, out=self.pose)
        if st.refine:
            if st.weights is not None:
                p.match_weights(self.pair["confidence"], self._first, self._second, self.m, st.weights, out=self.weight)
            p.refine_poses(kp, self.kp_depth, self._first, self._second, self.m, self.camera, self.pose, st.threshold, st.huber, st.iterations,
                           out=self.refined, weights=self.weight)
            if st.weights is not None:
                self.pair["confidence"][0].copy_(self.pair["confidence"][1])
        self.kp_depth[0].copy_(self.kp_depth[1])

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, depth_u16: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        """image_u8, tokens: as FrameStepper.step takes them; depth_u16: (h, w) or (1, h, w) uint16, the frame's raw depth image."""
        self._take_depth(depth_u16)
        first = self.n_frames == 0
        out = super().step(image_u8, tokens)
        out["pose"] = None if first else {k: v[0] for k, v in self.pose.items()}
        if self.refine and not first:
            out["pose"]["refined"] = {k: v[0] for k, v in self.refined.items()}
        return out

    def reset(self) -> None:
        super().reset()
        self.kp_depth.fill_(-1)


class WindowPoseFrameStepper(RuleFrameStepper):
    """RuleFrameStepper over several spacings whose step also estimates the camera's trajectory: the online form of
    odometry_graph.  step() takes the frame's raw depth image beside it; behind the matcher's finalize launch, on the same one
    stream - as ordinary launches or inside the captured graph - the depth under this frame's keypoints is gathered
    (sslam_keypoint_depth) into the static slot of a depth ring that lies beside the feature ring, ONE sslam_pose_ransac_pairs and
    ONE sslam_pose_refine_pairs launch run over the step's pairs with the matcher's own pair_first / pair_second lists (an absent
    pair comes out with refinement status 3; a subclass may have asked for extra pairs behind the S spacing rows), and
    sslw_window_step (include/sslam_window.h), on the S spacing rows, admits the refined pairs into a ring of
    the last `window` frames' edges, predicts the frame's pose from the nearest admitted pair and optimises the window's poses with
    its oldest frame held.  The window's frame counter is device memory like the stepper's own, so no host value enters the
    body.  The static slot is then handed over to the ring with the frame's features.
    The geometry bank follows pipe.geometry_keypoints (the refined keypoints on a pipeline with subcell=True), as in
    PoseFrameStepper, whose signature and behaviour this class leaves alone.
    step() returns what RuleFrameStepper returns with spacings, plus "pose": RANSAC's keys with a leading S axis (T (S, 12), ...)
    and "refined", the refinement's outputs (T, status, ..., info (S, 21)); and "window": lib.WINDOW_OUT_KEYS' tensors without the
    window axis (C_window (window, 12), base, n_nodes, admitted (S,), predicted_from, lost, status, ...) - all views of static
    buffers.  window: max(spacings) + 1 if None; a spacing of `window` or more is matched and refined but never admitted.
    rule: MatchRule.mnn_ratio(0.9) if None, as odometry() has it; huber: threshold / 3 if None; iterations: the refinement's;
    min_inliers, huber_chi, damping, graph_iterations: SequencePipeline.pose_window_step's; capacity: the frames trajectory()
    keeps."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, depth_height: int, depth_width: int, camera=None,
                 use_graph: bool = True, tokens_in: bool = False, rule=None, spacings=(1, 5, 10, 15, 20), window=None,
                 threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, huber=None, iterations: int = 5, min_inliers: int = 12,
                 huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 2, capacity: int = 4096):
        from .evaluation import Camera, check_depth_size
        from .pipeline import MatchRule
        sp = _checked_spacings(spacings, below=2 ** 31)                  # everything is judged before anything is allocated
        st = self.settings = PoseSettings(threshold, hypotheses, seed, True, huber, iterations)
        self.threshold, self.huber = st.threshold, st.huber
        self.window, _, self.capacity, _ = lib.check_window_sizes(max(sp) + 1 if window is None else window, len(sp), capacity)
        self.min_inliers = lib.check_int("min_inliers", min_inliers, 0, 2 ** 31 - 1)
        self.graph_settings = GraphSettings(huber_chi, damping, graph_iterations)
        self.camera = Camera() if camera is None else camera
        check_depth_size(depth_width, depth_height, self.camera)
        super().__init__(pipe, height, width, use_graph=use_graph, tokens_in=tokens_in, spacings=sp,
                         rule=MatchRule.mnn_ratio(0.9) if rule is None else rule)
        dev, K, P = self.device, self.cfg.num_keypoints, len(sp) + self._extra_pairs()
        self.depth = torch.zeros((1, depth_height, depth_width), dtype=torch.uint16, device=dev)
        self.kp_depth = torch.full((self.ring + 1, K), -1, dtype=torch.int32, device=dev)      # the depth ring, slot for slot beside the bank
        self.pose = pipe.alloc_pose(P, K)
        self.refined = pipe.alloc_pose_refine(P, K)
        # the spacings' rows, which the window reads: all of the rows, unless a subclass asked for extra pairs behind them
        self._window_rows = {k: self.refined[k][:len(sp)] for k in ("T", "info", "status", "inlier_count")}
        self.win = pipe.alloc_pose_window(self.window, sp, self.capacity)

    def _after_match(self) -> None:
        p, ring, st, g = self.pipe, self.ring, self.settings, self.graph_settings
        kp = p.geometry_keypoints(self.bank)
        p.keypoint_depth(self.depth, kp[ring:ring + 1], out=self.kp_depth[ring:ring + 1])
        p.estimate_poses(kp, self.kp_depth, self.pair_first, self.pair_second, self.m, self.camera, st.threshold, st.hypotheses, st.seed,
                         out=self.pose)
        p.refine_poses(kp, self.kp_depth, self.pair_first, self.pair_second, self.m, self.camera, self.pose, st.threshold, st.huber,
                       st.iterations, out=self.refined)
        p.pose_window_step(self.win, self._window_rows, None, self.min_inliers, g.huber_chi, g.damping, g.iterations)
        self._after_window()
        torch.remainder(self._t, ring, out=self._slot)                   # the ring slot the frame's features take, right after this
        self.kp_depth[:ring].index_copy_(0, self._slot, self.kp_depth[ring:ring + 1])

    def _after_window(self) -> None:
        """What a subclass enqueues behind the window step, before the static depth slot is handed over to the ring
        (LoopWindowPoseFrameStepper: its edge log)."""

    def _reset_window(self) -> None:
        st = self.win["state"]
        st["t"].zero_()
        st["ring_first"].fill_(-1)
        self.kp_depth.fill_(-1)

    def _capture(self) -> None:
        super()._capture()
        self._reset_window()                     # the warm-up passes stepped the window too: the first real frame is frame 0

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, depth_u16: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        """image_u8, tokens: as FrameStepper.step takes them; depth_u16: (h, w) or (1, h, w) uint16, the frame's raw depth image."""
        self._take_depth(depth_u16)
        out = super().step(image_u8, tokens)
        out["pose"] = dict(self.pose, refined=dict(self.refined))
        out["window"] = {k: v[0] for k, v in self.win["out"].items()}
        return out

    def trajectory(self):
        """Camera -> world poses (n, 4, 4) float64 of the frames 0 .. min(n_frames, capacity) - 1, each as it stood when it left the
        window (or stands now): odometry_graph's convention.  One read-back."""
        from .odometry import camera_to_world
        return camera_to_world(self.win["state"]["trajectory"][0, :min(self.n_frames, self.capacity)])

    def reset(self) -> None:
        """Forget every earlier frame: the device's counters are zeroed and the ring's slots made absent here, outside the graph."""
        super().reset()
        self._reset_window()


class LoopWindowPoseFrameStepper(WindowPoseFrameStepper):
    """WindowPoseFrameStepper that also notices when the camera is back where it was: loop closures while the sequence runs
    (include/sslam_place.h).  Opt-in: the parent, its signature and its bytes are left alone.
    The feature, depth and keypoint banks are a ring of `capacity` slots, not of max(spacings): while t < capacity frame j sits in
    slot j, so every frame the place bank can name is still there to be matched.  The bank's bytes: (capacity + 1) * K * D * 4 for
    the descriptors - 262 MB at capacity 1024, K = 500, D = 128 - beside (capacity + 1) * K * 24 for scores, intensity, keypoints and
    depth.  capacity (max(spacings) .. 4096) is also the frames the place bank, the edge log and trajectory() keep.
    One step, on one stream, as ordinary launches or from the one captured graph: extract; sslp_place_step on the static slot's
    descriptors and scores; the pair lists become the S spacing rows followed by the L = per_frame candidate rows (a candidate's
    older frame is its bank slot, its second the static slot, -1 -1 an empty slot); ONE match_pairs; ONE RANSAC and ONE refinement
    launch over the S + L rows; sslw_window_step on views of the first S rows - the window's outputs are the bytes
    WindowPoseFrameStepper gives for the same frames -; sslp_edge_log_step over all S + L rows, the spacing rows held to
    min_inliers, the candidate rows to loops["min_inliers"]; the static slot is handed over to the ring.  Both new counters are
    device memory: no host value enters the body.
    loops: None (odometry.LOOP_DEFAULTS) or a dictionary of some of min_gap, min_sim, per_frame, suppress, min_inliers.
    step() returns the parent's dictionary with S + L rows in matches / match_count / value and "pose" (pair_first keeps naming the S
    spacing rows: the candidates' frames are device values), "window" as the parent returns it, and "loops": the place step's
    first, second, sim (L,), count, status (1,), sig (D,), the log's logged (S + L,) and log_status (1,), and "refined": the
    refinement's outputs of the L candidate rows - all views of static buffers.
    Past `capacity` frames the spacings, the window and the trajectory carry on (the ring wraps); the place and log entries answer
    status 4 and the candidate rows read absent.  Nobody has measured this on real RGB-D data."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, depth_height: int, depth_width: int, camera=None,
                 use_graph: bool = True, tokens_in: bool = False, rule=None, spacings=(1, 5, 10, 15, 20), window=None,
                 threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, huber=None, iterations: int = 5, min_inliers: int = 12,
                 huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 2, loops=None, capacity: int = 1024):
        from .odometry import check_loops
        sp = _checked_spacings(spacings, below=2 ** 31)                  # everything is judged before anything is allocated
        self.loops = check_loops(loops)
        lib.check_int("min_inliers", self.loops["min_inliers"], 0, 2 ** 31 - 1)
        cap = lib.check_place_sizes(lib.check_int("capacity", capacity, 1), 1, pipe.descriptor_dim if pipe is not None else lib.D_OUT)[0]
        if len(sp) <= lib.WINDOW_MAX_SPACINGS:                           # more spacings than that: the parent refuses them by name
            lib.check_edge_log_sizes(cap, len(sp) + self.loops["per_frame"])
            if cap < max(sp):
                raise ValueError(f"capacity must be at least max(spacings) = {max(sp)}: the ring holds every frame a spacing reaches, got {cap}")
        self._ring_slots = cap
        super().__init__(pipe, height, width, depth_height, depth_width, camera=camera, use_graph=use_graph, tokens_in=tokens_in, rule=rule,
                         spacings=sp, window=window, threshold=threshold, hypotheses=hypotheses, seed=seed, huber=huber, iterations=iterations,
                         min_inliers=min_inliers, huber_chi=huber_chi, damping=damping, graph_iterations=graph_iterations, capacity=cap)
        o, S, L, dev = self.loops, len(sp), self.loops["per_frame"], self.device
        self.place = pipe.alloc_place_bank(cap, o["min_gap"], o["min_sim"], L, o["suppress"])
        self.log = pipe.alloc_edge_log(cap, S + L)
        self._slot_first = torch.full((S + L,), -1, dtype=torch.int32, device=dev)      # the GLOBAL older frame of every row, for the log
        self._global64 = torch.zeros((S,), dtype=torch.int64, device=dev)
        self._filled = torch.zeros((L,), dtype=torch.bool, device=dev)
        self._static32 = torch.full((L,), self.ring, dtype=torch.int32, device=dev)
        self._absent32 = torch.full((L,), -1, dtype=torch.int32, device=dev)
        self._tail = {k: v[S:] for k, v in self.refined.items()}

    def _ring_size(self, spacings: tuple) -> int:
        return self._ring_slots

    def _extra_pairs(self) -> int:
        return self.loops["per_frame"]

    def _before_match(self) -> None:
        S, po = len(self.spacings), self.place["out"]
        self.pipe.place_step(self.place, self.cur["descriptors"], self.cur["scores"])
        # while the place step answers, its counter is below capacity and frame j sits in ring slot j: the candidate IS its slot
        self.pair_first[S:].copy_(po["first"])
        torch.ge(po["first"], 0, out=self._filled)
        torch.where(self._filled, self._static32, self._absent32, out=self.pair_second[S:])

    def _after_window(self) -> None:
        S = len(self.spacings)
        torch.where(self._seen, self._back, self._absent, out=self._global64)      # frame t - s, or -1 before it exists
        self._slot_first[:S].copy_(self._global64)
        self._slot_first[S:].copy_(self.place["out"]["first"])
        self.pipe.edge_log_step(self.log, self._slot_first, self.refined, S, self.min_inliers, self.loops["min_inliers"])

    def _reset_window(self) -> None:
        super()._reset_window()
        self.place["state"]["t"].zero_()                                 # both new counters; nothing else of either state is read before it is written
        self.log["state"]["t"].zero_()

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, depth_u16: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        out = super().step(image_u8, depth_u16, tokens)
        out["loops"] = dict(self.place["out"], logged=self.log["out"]["logged"], log_status=self.log["out"]["status"], refined=dict(self._tail))
        return out

    def close_loops(self, huber_chi: float = 4.0, damping: float = 0.0, iterations: int = 8, cg_iterations: int = 512, cg_tol: float = 1e-3) -> dict:
        """The corrected trajectory, any time between steps: optimize_pose_graph_sparse over the edge log's first n * (S + L) slots
        and n nodes, n = min(frames stepped, capacity), from the window's committed trajectory.  Runs outside the captured step,
        makes ONE read-back and changes no state: stepping on gives the bytes it would have given without the call.
        Returns trajectory (n, 4, 4) camera -> world (odometry_graph's convention), C (n, 12) world -> camera as the solver wrote
        it, status, iterations, used_edges, skipped_edges, failed_row, cost_in, cost, cg_steps (16,), edge_chi2 (n * (S + L),) in
        log order, and loop_edges (P, 2): the logged loop slots [older frame, frame].  A frame with no logged edge - every pair of
        it refused - leaves its block zero: status 2 at damping 0 and the window's trajectory back, as the batch graph answers."""
        import numpy as np
        from .odometry import _GRAPH_INT, camera_to_world
        g = GraphSettings(huber_chi, damping, iterations)
        lib.check_cg_iterations(cg_iterations), lib.check_cg_tol(cg_tol)
        n = min(self.n_frames, self.capacity)
        if n < 1:
            raise ValueError("close_loops needs at least one stepped frame")
        S, E = len(self.spacings), len(self.spacings) + self.loops["per_frame"]
        st, rows = self.log["state"], n * E
        r = self.pipe.optimize_pose_graph_sparse(st["log_first"][:rows], st["log_second"][:rows], st["log_T"][:rows], st["log_info"][:rows], n,
                                                 self.win["state"]["trajectory"][0, :n], g.huber_chi, g.damping, g.iterations, cg_iterations, cg_tol)
        rb = Readback()
        for key in _GRAPH_INT + ("cg_steps",):
            rb.add(key, r[key], np.int64)
        for key in ("cost_in", "cost", "C", "edge_chi2"):
            rb.add(key, r[key], np.float64)
        rb.add("log_first", st["log_first"][:rows].reshape(n, E), np.int64)
        host = rb.fetch()                                                # the ONE read-back
        out = {key: host[key].item() for key in _GRAPH_INT + ("cost_in", "cost")}
        first = host["log_first"]
        frame, slot = np.nonzero(first[:, S:] >= 0)
        out.update(C=host["C"], trajectory=camera_to_world(host["C"]), cg_steps=host["cg_steps"], edge_chi2=host["edge_chi2"],
                   loop_edges=np.stack([first[frame, S + slot], frame], axis=1).astype(np.int64))
        return out


class TrackWindowPoseFrameStepper(WindowPoseFrameStepper):
    """WindowPoseFrameStepper that also follows every keypoint through the sequence: feature tracks while the sequence runs, and a
    landmark map on demand (include/sslam_track.h).  Opt-in: the parent, its signature and its bytes are left
    alone.  Behind the parent's launches, on the same stream - as ordinary launches or inside the one captured graph -
    sslt_track_step runs on the step's spacing-1 row: its match list, masked by that row's refined inlier_of_slot, links this frame's
    keypoints to the previous frame's; a linked keypoint inherits its track id and its age plus one, the others open new tracks.  The
    row's first frame is a device value made of the stepper's own counter, so no host value enters the body.  The frame's geometry
    keypoints and depths are kept in a bank of `capacity` frames beside the track bank's state (a row more takes the frames past it).
    spacings must hold 1.  step() returns the parent's dictionary plus track_id, track_age (K,), n_new and track_status (1,) - 4
    once `capacity` frames are in the bank - as views of static buffers.  landmarks() runs outside the captured step."""

    def __init__(self, pipe: SequencePipeline, height: int, width: int, depth_height: int, depth_width: int, camera=None,
                 use_graph: bool = True, tokens_in: bool = False, rule=None, spacings=(1, 5, 10, 15, 20), window=None,
                 threshold: float = 3.0, hypotheses: int = 256, seed: int = 0, huber=None, iterations: int = 5, min_inliers: int = 12,
                 huber_chi: float = 4.0, damping: float = 0.0, graph_iterations: int = 2, capacity: int = 4096):
        sp = _checked_spacings(spacings, below=2 ** 31)                  # everything is judged before anything is allocated
        if 1 not in sp:
            raise ValueError(f"spacings must hold 1: the tracks follow the previous frame's matches, got {spacings!r}")
        lib.check_track_sizes("track_step", lib.check_int("capacity", capacity, 1), pipe.cfg.num_keypoints, limit_k=True)
        self._row1 = sp.index(1)
        super().__init__(pipe, height, width, depth_height, depth_width, camera=camera, use_graph=use_graph, tokens_in=tokens_in, rule=rule,
                         spacings=sp, window=window, threshold=threshold, hypotheses=hypotheses, seed=seed, huber=huber, iterations=iterations,
                         min_inliers=min_inliers, huber_chi=huber_chi, damping=damping, graph_iterations=graph_iterations, capacity=capacity)
        dev, K, cap = self.device, self.cfg.num_keypoints, self.capacity
        self.tracks = pipe.alloc_track_bank(cap, K)
        self.track_kp = torch.zeros((cap + 1, K, 2), dtype=torch.float32, device=dev)          # row `cap`: the frames past the bank
        self.track_depth = torch.full((cap + 1, K), -1, dtype=torch.int32, device=dev)
        self._track_first64 = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._track_first = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self._track_row = torch.zeros((1,), dtype=torch.int64, device=dev)

    def _after_match(self) -> None:
        super()._after_match()
        p, ring, r = self.pipe, self.ring, self._row1
        torch.where(self._seen[r:r + 1], self._back[r:r + 1], self._absent[r:r + 1], out=self._track_first64)      # frame t - 1, or -1
        self._track_first.copy_(self._track_first64)
        p.track_step(self.tracks, self.m, self._track_first, mask=self.refined["inlier_of_slot"], row=r)
        torch.clamp(self._t, max=self.capacity, out=self._track_row)
        self.track_kp.index_copy_(0, self._track_row, p.geometry_keypoints(self.bank)[ring:ring + 1])
        self.track_depth.index_copy_(0, self._track_row, self.kp_depth[ring:ring + 1])

    def _reset_window(self) -> None:
        super()._reset_window()
        self.tracks["state"]["t"].zero_()                                # both counters; nothing else of the state is read before it is written
        self.tracks["state"]["next_id"].zero_()

    @torch.no_grad()
    def step(self, image_u8: torch.Tensor, depth_u16: torch.Tensor, tokens: torch.Tensor | None = None) -> dict:
        out = super().step(image_u8, depth_u16, tokens)
        o = self.tracks["out"]
        out.update(track_id=o["track_id"], track_age=o["age"], n_new=o["n_new"], track_status=o["status"])
        return out

    def landmarks(self, threshold: float = 3.0, min_obs: int = 2) -> dict:
        """The tracks and the landmark map so far, any time between steps: sslt_track_ids over the stored links and sslt_landmarks
        under trajectory()'s poses, n = min(frames stepped, capacity) frames.  Runs outside the captured step, makes ONE read-back and
        changes no state.  Returns n_tracks, track_id, age (n, K), length, status, n_kept (n_tracks,), rms and landmarks (n_tracks, 3)
        world points."""
        import numpy as np
        thr, mo = lib.check_threshold(threshold), lib.check_min_obs(min_obs)
        n = min(self.n_frames, self.capacity)
        if n < 1:
            raise ValueError("landmarks needs at least one stepped frame")
        st, K = self.tracks["state"], self.cfg.num_keypoints
        tr = self.pipe.track_ids({key: st[key][:n] for key in lib.LINK_KEYS})
        lm = self.pipe.landmarks(self.track_kp[:n], self.track_depth[:n], self.win["state"]["trajectory"][0, :n], tr, self.camera, thr, mo)
        rb = Readback()
        for key in ("n_tracks", "track_id", "age"):
            rb.add(key, tr[key], np.int32)
        for key, t, dtype in (("length", tr["length"], np.int32), ("status", lm["status"], np.int32), ("n_kept", lm["n_kept"], np.int32),
                              ("rms", lm["rms"], np.float64), ("landmarks", lm["xyz"], np.float64)):
            rb.add(key, t, dtype, rows="n_tracks")                       # a row per keypoint on the device, n_tracks of them filled
        host = rb.fetch()                                                # the ONE read-back
        return dict(host, n_tracks=int(host["n_tracks"][0]))
