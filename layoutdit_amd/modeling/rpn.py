"""The detector's region proposal network in eval mode - what torchvision's ``FasterRCNN`` runs on ``DiTWithFPN``'s maps
(ref ``src/layoutdit/modeling/model.py:40-55``: ``rpn_anchor_generator=AnchorGenerator(...)``, everything else default) -
re-designed for the MI355X instead of translated:

* :class:`AnchorGenerator` builds the anchors on the host once per geometry (they depend on nothing else) and caches them;
* :class:`RPNHead` runs on the FPN's NHWC maps with existing kernels: the 3x3 convolution is the implicit-im2col fp32 MFMA GEMM
  of the FPN, the two 1x1 convolutions are ONE ``ldit_linear_f32`` on the pixel rows, whose (h, w, a) row order already is
  torchvision's flattening order;
* ``filter_proposals`` - per-level top-k, decode, clip, small-box / score filter, NMS per level, top-N per image - is three
  launches (``csrc/proposals.hip``) with fixed-size padded results: no device-to-host synchronisation per level and batch as with
  torchvision's ``nms``, no data-dependent shape, capturable in a graph.  ``forward(..., padded=True)`` returns those padded
  tensors; the list form of torchvision slices them by the count (one synchronisation).

Inference only: anchor matching, sampling and the RPN losses are not implemented, ``train()`` mode is refused.  torchvision is
not installed offline: the semantics are restated from its documented behaviour (``tests/rpn_oracle.py``) - parity unpinned with
respect to torchvision itself, as for the FPN.  Parameter names follow torchvision, so detector checkpoints load
(``rpn.head.conv.0.0.weight`` ...).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import ops


class AnchorGenerator(nn.Module):
    """torchvision's ``AnchorGenerator(sizes, aspect_ratios)``: one tuple of sizes and of aspect ratios per feature level."""

    def __init__(self, sizes=((128, 256, 512),), aspect_ratios=((0.5, 1.0, 2.0),)):
        super().__init__()
        if not isinstance(sizes[0], (list, tuple)):
            sizes = tuple((s,) for s in sizes)
        if not isinstance(aspect_ratios[0], (list, tuple)):
            aspect_ratios = (aspect_ratios,) * len(sizes)
        if len(sizes) != len(aspect_ratios):
            raise ValueError("AnchorGenerator: sizes and aspect_ratios must name the same number of levels")
        self.sizes = tuple(tuple(s) for s in sizes)
        self.aspect_ratios = tuple(tuple(r) for r in aspect_ratios)
        self._cache: Dict[tuple, Tuple[torch.Tensor, Tuple[int, ...]]] = {}

    def num_anchors_per_location(self) -> List[int]:
        return [len(s) * len(r) for s, r in zip(self.sizes, self.aspect_ratios)]

    def base_anchors(self) -> List[np.ndarray]:
        """Per level, float32 [A, 4]: round([-ws, -hs, ws, hs] / 2), hs = sqrt(r) s, ws = s / sqrt(r); ratio-major, size-minor."""
        out = []
        for sizes, ratios in zip(self.sizes, self.aspect_ratios):
            s = np.asarray(sizes, dtype=np.float32)
            h_r = np.sqrt(np.asarray(ratios, dtype=np.float32))
            w_r = (np.float32(1.0) / h_r).astype(np.float32)
            ws = (w_r[:, None] * s[None, :]).reshape(-1)
            hs = (h_r[:, None] * s[None, :]).reshape(-1)
            out.append(np.round(np.stack([-ws, -hs, ws, hs], axis=1) / np.float32(2.0)).astype(np.float32))
        return out

    def host_anchors(self, grid_sizes: Sequence[Tuple[int, int]], image_size: Tuple[int, int]) -> Tuple[np.ndarray, Tuple[int, ...]]:
        """float32 [Ntot, 4] anchors in (level, y, x, anchor) order and the anchors per level."""
        if len(grid_sizes) != len(self.sizes):
            raise ValueError(f"AnchorGenerator: {len(grid_sizes)} feature levels, built for {len(self.sizes)}")
        levels = []
        for (gh, gw), base in zip(grid_sizes, self.base_anchors()):
            sh, sw = image_size[0] // gh, image_size[1] // gw
            sy, sx = np.meshgrid(np.arange(gh, dtype=np.float32) * sh, np.arange(gw, dtype=np.float32) * sw, indexing="ij")
            shifts = np.stack([sx.reshape(-1), sy.reshape(-1), sx.reshape(-1), sy.reshape(-1)], axis=1)
            levels.append((shifts[:, None, :] + base[None, :, :]).reshape(-1, 4))
        return np.concatenate(levels, axis=0).astype(np.float32), tuple(int(a.shape[0]) for a in levels)

    def forward(self, grid_sizes: Sequence[Tuple[int, int]], image_size: Tuple[int, int], device) -> Tuple[torch.Tensor, Tuple[int, ...]]:
        key = (tuple(map(tuple, grid_sizes)), tuple(image_size), str(device))
        hit = self._cache.get(key)
        if hit is None:
            a, level_sizes = self.host_anchors(grid_sizes, image_size)
            hit = (torch.from_numpy(a).to(device), level_sizes)
            self._cache[key] = hit
        return hit


class _ConvRelu(nn.Sequential):
    """torchvision's ``Conv2dNormActivation(c, c, 3, norm_layer=None)``: convolution at index 0, ReLU at index 1."""

    def __init__(self, c: int):
        super().__init__(nn.Conv2d(c, c, kernel_size=3, padding=1), nn.ReLU(inplace=True))


class RPNHead(nn.Module):
    """torchvision's ``RPNHead(in_channels, num_anchors)``: ``conv.0.0`` (3x3 + ReLU), ``cls_logits`` and ``bbox_pred`` (1x1)."""

    def __init__(self, in_channels: int = 256, num_anchors: int = 3):
        super().__init__()
        self.conv = nn.Sequential(_ConvRelu(in_channels))
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1)
        self.in_channels, self.num_anchors = in_channels, num_anchors
        for m in self.modules():                          # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)
        self._packed = None

    def _operands(self):
        """The 3x3 weight as [Cout, 3, 3, Cin] and both 1x1 convolutions as one [5 A (padded to a multiple of 4), C] matrix,
        re-laid when a parameter changes."""
        ps = (self.conv[0][0].weight, self.conv[0][0].bias, self.cls_logits.weight, self.cls_logits.bias, self.bbox_pred.weight,
              self.bbox_pred.bias)
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in ps)
        if self._packed is None or self._packed[0] != key:
            A, Cc = self.num_anchors, self.in_channels
            rows = (5 * A + 3) // 4 * 4
            w = torch.zeros((rows, Cc), device=ps[0].device, dtype=torch.float32)
            b = torch.zeros((rows,), device=ps[0].device, dtype=torch.float32)
            w[:A] = ps[2].detach().reshape(A, Cc)
            w[A:5 * A] = ps[4].detach().reshape(4 * A, Cc)
            b[:A] = ps[3].detach()
            b[A:5 * A] = ps[5].detach()
            self._packed = (key, ps[0].detach().permute(0, 2, 3, 1).contiguous(), ps[1].detach(), w, b)
        return self._packed[1:]

    def forward_level(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """One map ``[B, C, h, w]`` (any memory layout; channels-last costs no copy) -> objectness logits ``[B, h w A]`` and box
        deltas ``[B, h w A, 4]`` in (y, x, anchor) order."""
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"RPNHead: expected [B, {self.in_channels}, h, w], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"RPNHead: expected float32 features, got {x.dtype}")
        w3, b3, w1, b1 = self._operands()
        B, Cc, h, w = x.shape
        A = self.num_anchors
        t = ops.conv3x3_nhwc(x.detach().permute(0, 2, 3, 1).contiguous(), w3, b3)
        torch.relu_(t)
        y = ops.linear(t.view(B * h * w, Cc), w1, b1)                  # [B h w, 5 A (+ pad)]: logits | deltas per pixel row
        return y[:, :A].reshape(B, h * w * A), y[:, A:5 * A].reshape(B, h * w * A, 4)

    def forward(self, features: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """All levels: logits ``[B, Ntot]`` and deltas ``[B, Ntot, 4]``, levels concatenated in the order given."""
        per_level = [self.forward_level(f) for f in features]
        return (torch.cat([p[0] for p in per_level], dim=1).contiguous(), torch.cat([p[1] for p in per_level], dim=1).contiguous())


class RegionProposalNetwork(nn.Module):
    """torchvision's ``RegionProposalNetwork`` in eval mode.  ``forward(features, image_size)`` returns the list of proposal
    boxes per image; with ``padded=True`` the fixed-size form ``(boxes [B, post, 4], scores [B, post], count [B])``."""

    def __init__(self, anchor_generator: AnchorGenerator, head: RPNHead, pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000,
                 nms_thresh: float = 0.7, score_thresh: float = 0.0, min_size: float = 1e-3):
        super().__init__()
        self.anchor_generator, self.head = anchor_generator, head
        self.pre_nms_top_n, self.post_nms_top_n = int(pre_nms_top_n), int(post_nms_top_n)
        self.nms_thresh, self.score_thresh, self.min_size = float(nms_thresh), float(score_thresh), float(min_size)
        self._groups: Dict[tuple, torch.Tensor] = {}

    def _level_ids(self, level_sizes: Sequence[int], batch: int, device) -> torch.Tensor:
        """int32 [B, Ksum]: the level of every top-k column - the NMS groups.  Constant per geometry, cached."""
        key = (tuple(level_sizes), batch, self.pre_nms_top_n, str(device))
        g = self._groups.get(key)
        if g is None:
            ids = np.concatenate([np.full(min(self.pre_nms_top_n, n), l, dtype=np.int32) for l, n in enumerate(level_sizes)])
            g = torch.from_numpy(np.tile(ids, (batch, 1))).to(device)
            self._groups[key] = g
        return g

    def filter_proposals_padded(self, logits: torch.Tensor, deltas: torch.Tensor, anchors: torch.Tensor, level_sizes: Sequence[int],
                                image_size: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The three launches: top-k per level, decode, batched NMS with the level as group.  No synchronisation."""
        idx = ops.rpn_topk(logits, level_sizes, self.pre_nms_top_n)
        boxes, scores = ops.rpn_decode(logits, deltas, anchors, idx, image_size, self.min_size, self.score_thresh)
        groups = self._level_ids(level_sizes, logits.shape[0], logits.device)
        _, count, out_boxes, out_scores = ops.batched_nms_padded(boxes, scores, groups, self.nms_thresh, self.post_nms_top_n)
        return out_boxes, out_scores, count

    def forward(self, features: Union[Dict[str, torch.Tensor], Sequence[torch.Tensor]], image_size: Tuple[int, int], padded: bool = False):
        if self.training:
            raise RuntimeError("RegionProposalNetwork: inference only (anchor matching, sampling and the RPN losses are not "
                               "implemented) - call .eval() first")
        feats = list(features.values()) if isinstance(features, dict) else list(features)
        with torch.no_grad():
            logits, deltas = self.head(feats)
            anchors, level_sizes = self.anchor_generator([tuple(f.shape[-2:]) for f in feats], tuple(image_size), logits.device)
            A = self.head.num_anchors
            if any(n != f.shape[-2] * f.shape[-1] * A for n, f in zip(level_sizes, feats)):
                raise ValueError("RegionProposalNetwork: the anchor generator and the head disagree on anchors per location")
            boxes, scores, count = self.filter_proposals_padded(logits, deltas, anchors, level_sizes, image_size)
        if padded:
            return boxes, scores, count
        return [boxes[i, :n] for i, n in enumerate(count.tolist())]
