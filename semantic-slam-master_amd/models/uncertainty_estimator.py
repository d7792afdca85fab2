"""Drop-in for the reference's `models.uncertainty_estimator` (semantic-slam/models/uncertainty_estimator.py).

Same class (`UncertaintyEstimator`), constructor, attributes and state_dict keys (`mlp.0`, `mlp.2`, `mlp.4`), the same five methods
with the same signatures and return shapes.  Under `torch.no_grad()` on CUDA tensors `forward` runs the whole head as ONE fused HIP
kernel (sslc_confidence_rows, include/sslam_conf.h) and `filter_keypoints_by_confidence` runs the filter and the takes on the
device, reading one number back (the padded length); with autograd enabled, on CPU tensors, or at widths the kernel is not built
for, both run as ordinary torch ops on the same Parameters.  The two losses are plain torch, forward and backward: they are
reductions of B * N numbers and a trainer needs autograd through them.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from sslam_amd import lib
from sslam_amd.pipeline import PackedConfidence


class UncertaintyEstimator(nn.Module):
    """Per-keypoint confidence in [0, 1] from [feature at the keypoint | refined descriptor]."""

    def __init__(self, dino_dim: int = 384, descriptor_dim: int = 128, hidden_dim: int = 128):
        super().__init__()
        self.dino_dim = dino_dim
        self.descriptor_dim = descriptor_dim
        self.mlp = nn.Sequential(nn.Linear(dino_dim + descriptor_dim, hidden_dim), nn.ReLU(inplace=True),
                                 nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(inplace=True),
                                 nn.Linear(hidden_dim // 2, 1), nn.Sigmoid())
        self._packed = None
        self._packed_key = None
        self._warned = False

    def _packed_weights(self) -> PackedConfidence:
        ps = list(self.parameters())
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in ps)
        if self._packed is None or key != self._packed_key:
            self._packed = PackedConfidence(self.state_dict(), ps[0].device)
            self._packed_key = key
        return self._packed

    def _hip_ok(self, x: torch.Tensor) -> bool:
        """HIP path only for 384 + 128 | 256 -> 128 -> 64 -> 1 (any other widths the reference accepts run as eager torch ops) and
        when weights and input share a GPU."""
        w1 = self.mlp[0].weight
        if not PackedConfidence.supported(self.dino_dim, w1.shape[1] - self.dino_dim, w1.shape[0]):
            if not self._warned:
                warnings.warn(f"UncertaintyEstimator: {self.dino_dim} + {w1.shape[1] - self.dino_dim} -> {w1.shape[0]} is outside the "
                              f"HIP kernel's shapes (384 + 128 | 256 -> 128); using the eager torch path")
                self._warned = True
            return False
        return w1.device == x.device

    def forward(self, dino_features: torch.Tensor, descriptors: torch.Tensor) -> torch.Tensor:
        """(B, N, dino_dim) features at the keypoints, (B, N, descriptor_dim) descriptors -> (B, N, 1) confidence."""
        needs_graph = torch.is_grad_enabled() and (dino_features.requires_grad or descriptors.requires_grad or
                                                   any(p.requires_grad for p in self.parameters()))
        if dino_features.is_cuda and descriptors.is_cuda and not needs_graph and dino_features.dim() == 3 and \
                dino_features.numel() > 0 and self._hip_ok(dino_features) and descriptors.device == dino_features.device:
            pk = self._packed_weights()
            x = dino_features.detach().contiguous().float()
            d = descriptors.detach().contiguous().float()
            return lib.confidence_rows(x, d, pk.packed).unsqueeze(-1)
        return self.mlp(torch.cat([dino_features, descriptors], dim=-1))

    def compute_calibration_loss(self, predicted_confidence: torch.Tensor, actual_error: torch.Tensor,
                                 epsilon: float = 1e-6) -> torch.Tensor:
        """MSE between the confidence (B, N, 1) and 1 - error / (largest error + epsilon), error (B, N)."""
        target = 1 - (actual_error / (actual_error.max() + epsilon)).unsqueeze(-1)
        return F.mse_loss(predicted_confidence, target)

    def compute_expected_error_loss(self, predicted_confidence: torch.Tensor, actual_error: torch.Tensor) -> torch.Tensor:
        """L1 between the error a confidence stands for, 1 / (confidence + 1e-6) - 1, and the error (B, N)."""
        return F.l1_loss(1 / (predicted_confidence.squeeze(-1) + 1e-6) - 1, actual_error)

    def filter_keypoints_by_confidence(self, keypoints: torch.Tensor, descriptors: torch.Tensor, confidence: torch.Tensor,
                                       threshold: float = 0.5) -> tuple:
        """keypoints (B, N, 2), descriptors (B, N, D), confidence (B, N, 1) -> the same three with, per frame, only the keypoints
        of confidence >= threshold (the most confident one where none passes), padded to the longest frame's length M by
        repeating the frame's last kept keypoint and descriptor, the confidence by zeros: (B, M, 2), (B, M, D), (B, M, 1)."""
        f32 = all(t.dtype == torch.float32 for t in (keypoints, descriptors, confidence))
        needs_graph = torch.is_grad_enabled() and any(t.requires_grad for t in (keypoints, descriptors, confidence))
        if f32 and not needs_graph and confidence.is_cuda and keypoints.device == descriptors.device == confidence.device and \
                confidence.shape[1] <= lib.CONF_FILTER_MAX_K and confidence.numel() > 0:
            slot, count, conf = lib.confidence_filter(confidence.detach()[..., 0].contiguous(), threshold)
            kp = lib.take_rows(keypoints.detach().contiguous(), slot)
            desc = lib.take_rows(descriptors.detach().contiguous(), slot)
            m = int(count.max())      # the one host read: the padded length
            return kp[:, :m], desc[:, :m], conf[:, :m].unsqueeze(-1)
        c = confidence[..., 0]
        n = c.shape[1]
        keep = c >= threshold
        none = ~keep.any(dim=1)
        keep[none, c.argmax(dim=1)[none]] = True
        count = keep.sum(dim=1, keepdim=True)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)      # the kept slots first, each group ascending
        j = torch.arange(n, device=c.device)[None, :]
        slot = torch.where(j < count, order, order.gather(1, count - 1))[:, :int(count.max())]
        live = j[:, :slot.shape[1]] < count
        take = lambda t: t.gather(1, slot[..., None].expand(-1, -1, t.shape[-1]))       # noqa: E731
        return take(keypoints), take(descriptors), torch.where(live, c.gather(1, slot), torch.zeros((), dtype=c.dtype, device=c.device))[..., None]
