"""The detector's box head in eval mode - what torchvision's ``FasterRCNN`` runs on the proposals (ref
``src/layoutdit/modeling/model.py:34-55``: ``box_roi_pool=MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)``, everything
else default: ``TwoMLPHead(256 * 7 * 7, 1024)``, ``FastRCNNPredictor(1024, num_classes)``, ``box_score_thresh=0.05``,
``box_nms_thresh=0.5``, ``box_detections_per_img=100``, ``BoxCoder`` weights (10, 10, 5, 5)) - re-designed for the MI355X instead of
translated:

* :class:`MultiScaleRoIAlign` is ONE launch on the FPN's channels-last maps and the padded proposals of the RPN
  (``csrc/roi_heads.hip``): the level of a box is decided inside the kernel (torchvision: one ``nonzero`` per level, a host
  synchronisation each), the ``pool`` level is read through its strided view, and the pooled row comes out in (ph, pw, c) order;
* :class:`TwoMLPHead` runs ``fc6`` on those rows with its weight columns re-ordered once from torchvision's (c, ph, pw) flattening,
  ``relu_`` in place, ``fc7`` alike; :class:`FastRCNNPredictor` is ONE ``ldit_linear_f32`` with ``cls_score`` and ``bbox_pred``
  stacked;
* ``postprocess_detections`` is one launch (softmax, decode, clip, filters) and the batched NMS of the RPN stage keyed by label,
  with fixed-size padded results: ``forward(..., padded=True)`` never synchronises; the list form slices by the count (one
  synchronisation).

Inference only: proposal sampling, matching and the losses are not implemented, ``train()`` mode is refused.  torchvision is not
installed offline: the semantics are restated from its documented behaviour (``tests/roi_oracle.py``) - parity unpinned with
respect to torchvision itself, as for the FPN and the RPN.  Parameter names follow torchvision, so detector checkpoints load
(``roi_heads.box_head.fc6.weight`` ...).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from .. import ops


def _param_key(*ps) -> tuple:
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in ps)


def _nhwc_f32(f: torch.Tensor) -> torch.Tensor:
    """The map as the kernel reads it: float32 with channel stride 1 (no copy for the FPN's own outputs and their strided views)."""
    if f.dtype != torch.float32:
        f = f.float()
    if f.stride(1) != 1:
        f = f.contiguous(memory_format=torch.channels_last)
    return f


class MultiScaleRoIAlign(nn.Module):
    """torchvision's ``MultiScaleRoIAlign(featmap_names, output_size, sampling_ratio)`` on padded proposals."""

    def __init__(self, featmap_names: Sequence[str], output_size: int = 7, sampling_ratio: int = 2, canonical_scale: int = 224,
                 canonical_level: int = 4):
        super().__init__()
        if isinstance(output_size, (tuple, list)):
            if len(output_size) != 2 or output_size[0] != output_size[1]:
                raise NotImplementedError("MultiScaleRoIAlign: a square output size is built")
            output_size = output_size[0]
        self.featmap_names = list(featmap_names)
        self.output_size, self.sampling_ratio = int(output_size), int(sampling_ratio)
        self.canonical_scale, self.canonical_level = float(canonical_scale), float(canonical_level)

    def forward(self, features: Union[Dict[str, torch.Tensor], Sequence[torch.Tensor]], boxes: torch.Tensor, count: Optional[torch.Tensor],
                image_size: Tuple[int, int]) -> torch.Tensor:
        """``features``: the named maps (or the maps themselves, finest first), ``boxes`` [B, R, 4], ``count`` int32 [B] or None.
        Returns ``[B * R, P, P, C]``; rows past the count are zero."""
        feats = [features[n] for n in self.featmap_names] if isinstance(features, dict) else list(features)
        return ops.roi_align_levels([_nhwc_f32(f.detach()) for f in feats], boxes, count, image_size, self.output_size,
                                    self.sampling_ratio, self.canonical_scale, self.canonical_level)


class TwoMLPHead(nn.Module):
    """torchvision's ``TwoMLPHead(in_channels, representation_size)``: ``fc6``, ``fc7``, a ReLU after each."""

    def __init__(self, in_channels: int = 256 * 7 * 7, representation_size: int = 1024):
        super().__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        self._packed = None

    def fc6_weight_hwc(self, channels: int, ph: int, pw: int) -> torch.Tensor:
        """``fc6.weight`` with its columns re-ordered from torchvision's ``flatten(start_dim=1)`` of (c, ph, pw) to (ph, pw, c) - the
        order of a pooled row; re-laid when the parameter changes."""
        w = self.fc6.weight
        if channels * ph * pw != w.shape[1]:
            raise ValueError(f"TwoMLPHead: pooled rows of {ph} x {pw} x {channels} do not match fc6's {w.shape[1]} inputs")
        key = (_param_key(w), channels, ph, pw)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, w.detach().view(w.shape[0], channels, ph, pw).permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous())
        return self._packed[1]

    def forward(self, pooled: torch.Tensor) -> torch.Tensor:
        """``pooled`` [M, P, P, C] (channels innermost) -> [M, representation_size]."""
        if pooled.dim() != 4:
            raise ValueError(f"TwoMLPHead: expected pooled rows [M, P, P, C], got {tuple(pooled.shape)}")
        M, ph, pw, Cc = pooled.shape
        x = ops.linear(pooled.reshape(M, ph * pw * Cc), self.fc6_weight_hwc(Cc, ph, pw), self.fc6.bias.detach())
        torch.relu_(x)
        x = ops.linear(x, self.fc7.weight.detach(), self.fc7.bias.detach())
        torch.relu_(x)
        return x


class FastRCNNPredictor(nn.Module):
    """torchvision's ``FastRCNNPredictor(in_channels, num_classes)``: ``cls_score`` and ``bbox_pred``, run as one GEMM."""

    def __init__(self, in_channels: int = 1024, num_classes: int = 6):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)
        self.num_classes = int(num_classes)
        self._packed = None

    def _operands(self):
        """Both layers as one [5 NC (padded to a multiple of 4), in_channels] matrix, re-laid when a parameter changes."""
        ps = (self.cls_score.weight, self.cls_score.bias, self.bbox_pred.weight, self.bbox_pred.bias)
        key = _param_key(*ps)
        if self._packed is None or self._packed[0] != key:
            NC = self.num_classes
            rows = (5 * NC + 3) // 4 * 4
            w = torch.zeros((rows, ps[0].shape[1]), device=ps[0].device, dtype=torch.float32)
            b = torch.zeros((rows,), device=ps[0].device, dtype=torch.float32)
            w[:NC], w[NC:5 * NC] = ps[0].detach(), ps[2].detach()
            b[:NC], b[NC:5 * NC] = ps[1].detach(), ps[3].detach()
            self._packed = (key, w, b)
        return self._packed[1:]

    def forward_stacked(self, x: torch.Tensor) -> torch.Tensor:
        """[M, in_channels] -> [M, 5 NC (+ pad)]: the class logits in columns [0, NC), the deltas in [NC, 5 NC)."""
        w, b = self._operands()
        return ops.linear(x, w, b)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        y, NC = self.forward_stacked(x), self.num_classes
        return y[:, :NC], y[:, NC:5 * NC]


class RoIHeads(nn.Module):
    """torchvision's ``RoIHeads`` in eval mode (box branch).  ``forward(features, proposals, count, image_size)`` returns the list of
    ``{boxes, labels, scores}`` per image; with ``padded=True`` the fixed-size form ``(boxes [B, D, 4], scores [B, D], labels [B, D],
    count [B])``, ``D = detections_per_img``."""

    def __init__(self, box_roi_pool: MultiScaleRoIAlign, box_head: TwoMLPHead, box_predictor: FastRCNNPredictor,
                 bbox_reg_weights: Optional[Sequence[float]] = None, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                 detections_per_img: int = 100, min_size: float = 1e-2):
        super().__init__()
        self.box_roi_pool, self.box_head, self.box_predictor = box_roi_pool, box_head, box_predictor
        self.bbox_reg_weights = tuple(float(w) for w in (bbox_reg_weights or (10.0, 10.0, 5.0, 5.0)))
        self.score_thresh, self.nms_thresh, self.min_size = float(score_thresh), float(nms_thresh), float(min_size)
        self.detections_per_img = int(detections_per_img)

    def head_padded(self, features, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size: Tuple[int, int]) -> torch.Tensor:
        """RoIAlign and the three GEMMs: ``[B * R, 5 NC (+ pad)]`` logits | deltas per proposal row."""
        pooled = self.box_roi_pool(features, proposals, count, image_size)
        return self.box_predictor.forward_stacked(self.box_head(pooled))

    def forward(self, features, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size: Tuple[int, int], padded: bool = False):
        if self.training:
            raise RuntimeError("RoIHeads: inference only (proposal sampling, matching and the box losses are not implemented) - "
                               "call .eval() first")
        if proposals.dim() != 3 or proposals.shape[-1] != 4:
            raise ValueError(f"RoIHeads: expected padded proposals [B, R, 4], got {tuple(proposals.shape)}")
        ops._check_candidates(proposals.shape[1], self.box_predictor.num_classes)
        with torch.no_grad():
            y = self.head_padded(features, proposals, count, image_size)
            boxes, scores, labels, kept = ops.box_detections_padded(y, proposals, count, image_size, self.box_predictor.num_classes,
                                                                    self.score_thresh, self.nms_thresh, self.detections_per_img,
                                                                    self.min_size, self.bbox_reg_weights)
        if padded:
            return boxes, scores, labels, kept
        return [{"boxes": boxes[i, :n], "labels": labels[i, :n].to(torch.int64), "scores": scores[i, :n]} for i, n in enumerate(kept.tolist())]
