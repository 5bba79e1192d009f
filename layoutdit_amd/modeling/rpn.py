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

Training (``train()`` mode with targets): ``assign_targets_to_anchors`` - ``Matcher(0.7, 0.3, allow_low_quality_matches=True)``,
``BalancedPositiveNegativeSampler(256, 0.5)``, ``BoxCoder(1, 1, 1, 1).encode`` - is ONE launch and ``compute_loss`` with both
gradients two more (``csrc/rpn_train.hip``): fixed-size results instead of torchvision's ``nonzero`` / ``randperm``, the sampler
driven by random keys drawn on the device, so still no synchronisation.  :class:`RPNHead` is differentiated by one
``torch.autograd.Function`` per level, which reads the head's cached operands and whose backward is the FPN's and the box head's
(``grad_ops.py``): ``linear_bwd`` for the 1x1 pair (``ldit_linear_f32`` on the transposed weight, its 15 columns padded to the
GEMM's 32), ``conv3x3_bwd`` for the 3x3 (the same implicit-im2col GEMM on the flipped weight), all three weight gradients bf16
MFMA GEMMs on reduction-major operands with fp32 accumulation (they carry bf16 operand rounding, like the encoder's), the biases
``ldit_colsum_f32``.  ``train()`` mode WITHOUT targets stays refused.

torchvision is not installed offline: the semantics are restated from its documented behaviour (``tests/rpn_oracle.py``,
``tests/rpn_train_oracle.py``) - parity unpinned with respect to torchvision itself, as for the FPN.  Parameter names follow
torchvision, so detector checkpoints load (``rpn.head.conv.0.0.weight`` ...).

The dtype options are ``grad_ops.py``'s.  What is particular to this head: under ``neck_dtype`` / ``train_dtype="bf16"`` the 3x3 has
bias and ReLU in the GEMM's epilogue (bf16 activation rows; no ``relu_`` launch, no fp32 activation) and the 1x1 pair is one bf16
GEMM whose fp32 value is stored unrounded; what :class:`_RPNHeadLevelFn` then saves are the map's slack-padded bf16 copy and the bf16
activation - the 3x3's wgrad operand, the ReLU mask and the 1x1 pair's wgrad operand as they stand.  ``grad_dtype`` concerns the 3x3's
dgrad; the 1x1 pair's own (32 padded columns) stays on the fp32 GEMM.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from .grad_ops import (BF16_K, OperandCache, check_dtype, conv3x3_bwd, conv3x3_dgrad_bf16, conv3x3_fwd_bf16, dtype_setter, linear_bwd,
                       pad_grad_row, stack_rows)


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


def _level_forward(x, operands, A: int, slack: bool = False):
    """One level on :meth:`RPNHead._operands` or, on the bf16 matrix pipe, :meth:`RPNHead._operands_bf16` (the 3x3 with bias and ReLU in
    the GEMM's epilogue, the 1x1 pair as one bf16 GEMM with its fp32 value stored unrounded).  Returns ``(logits [B, h w A], deltas
    [B, h w A, 4])`` and what a backward reads: the NHWC map - under bf16 its zero-padded bf16 copy, with the wgrad's ``slack`` rows
    where asked - and the 3x3's activation rows."""
    w3, b3, w1, b1 = operands
    B, Cc, h, w = x.shape
    xn = x.detach().permute(0, 2, 3, 1).contiguous()                                      # NHWC; free for channels-last maps
    if w3.dtype == torch.bfloat16:
        t, xn = conv3x3_fwd_bf16(xn, w3, b3, _lib.EPI_BIAS_RELU, slack=slack)             # bf16 [B h w, C]
        y = ops.linear_bf16(t, w1, b1, _lib.EPI_F32)                                      # fp32 [B h w, 5 A (+ pad)]
    else:
        t = ops.conv3x3_nhwc(xn, w3, b3).view(B * h * w, Cc)
        torch.relu_(t)
        y = ops.linear(t, w1, b1)                                      # [B h w, 5 A (+ pad)]: logits | deltas per pixel row
    return (y[:, :A].reshape(B, h * w * A), y[:, A:5 * A].reshape(B, h * w * A, 4)), xn, t


class _RPNHeadLevelFn(torch.autograd.Function):
    """One level of :class:`RPNHead` with gradients for the map and all six parameters.
    apply(x [B, C, h, w], w3, b3, w_cls, b_cls, w_box, b_box, head) -> (logits [B, h w A], deltas [B, h w A, 4]).
    ``head``: the :class:`RPNHead` whose parameters these are.  The forward is :func:`_level_forward` on its cached operands - the bf16
    ones under ``train_dtype="bf16"`` with a channel count the bf16 GEMM takes - and reads both options there, keeping ``grad_dtype`` on
    ``ctx``: a setter called between forward and backward does not change that backward.  The backward takes the 3x3's dgrad operand
    from the head's cache."""

    @staticmethod
    def forward(ctx, x, w3, b3, wc, bc, wb, bb, head):
        B, Cc, h, w = x.shape
        bf16 = check_dtype("train_dtype", head.train_dtype) == "bf16" and Cc % BF16_K == 0
        out, xn, t = _level_forward(x, head._operands_bf16() if bf16 else head._operands(), head.num_anchors, slack=True)
        ctx.saved = (xn, t, w3.detach(), head._operands()[2])
        ctx.shape = (B, h, w, Cc)
        ctx.head, ctx.grad_dtype = head, check_dtype("grad_dtype", head.grad_dtype)
        return out

    @staticmethod
    def backward(ctx, d_logits, d_deltas):
        if ctx.saved is None:
            raise RuntimeError("RPNHead: backward through a level a second time (its saved maps are freed after the first)")
        xn, t, w3, w1 = ctx.saved
        ctx.saved = None
        A, grad_dtype = ctx.head.num_anchors, ctx.grad_dtype
        B, h, w, Cc = ctx.shape
        M = B * h * w
        need = ctx.needs_input_grad
        dy = pad_grad_row(((A, d_logits), (4 * A, d_deltas)), M, xn.device)   # the gradient of the pixel rows [M, logits | deltas | 0]
        # (K = 32 is below the bf16 GEMM's k-tile: this dgrad is the fp32 GEMM under either setting)
        dt, g1, gb = linear_bwd(dy, t, w1, True, need[3] or need[5], need[4] or need[6], grad_dtype)                # [M, C], [K, C], [K]
        g_x, g_w3, g_b3 = conv3x3_bwd(dt.view(B, h, w, Cc), xn, w3, need[0], need[1], need[2], grad_dtype, act=t,
                                      dgrad_w=ctx.head._dgrad_operand_bf16)
        return (g_x.permute(0, 3, 1, 2) if need[0] else None, g_w3, g_b3,
                g1[:A].reshape(A, Cc, 1, 1) if need[3] else None, gb[:A] if need[4] else None,
                g1[A:5 * A].reshape(4 * A, Cc, 1, 1) if need[5] else None, gb[A:5 * A] if need[6] else None, None)


class _RPNLossFn(torch.autograd.Function):
    """``ldit_rpn_loss_f32`` as a differentiable node: the kernel has already written both gradients for unit upstream, the
    backward scales them by the two upstream scalars."""

    @staticmethod
    def forward(ctx, logits, deltas, labels, reg_targets, sampled, beta):
        loss, d_logits, d_deltas = ops.rpn_loss(logits.detach(), deltas.detach(), labels, reg_targets, sampled, beta)
        ctx.save_for_backward(d_logits, d_deltas)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_obj, g_box):
        d_logits, d_deltas = ctx.saved_tensors
        return d_logits * g_obj, d_deltas * g_box, None, None, None, None


class RPNHead(nn.Module):
    """torchvision's ``RPNHead(in_channels, num_anchors)``: ``conv.0.0`` (3x3 + ReLU), ``cls_logits`` and ``bbox_pred`` (1x1)."""

    def __init__(self, in_channels: int = 256, num_anchors: int = 3, neck_dtype: str = "f32", grad_dtype: str = "f32", train_dtype: str = "f32"):
        super().__init__()
        self.neck_dtype = check_dtype("neck_dtype", neck_dtype)
        self.grad_dtype = check_dtype("grad_dtype", grad_dtype)
        self.train_dtype = check_dtype("train_dtype", train_dtype)
        self.conv = nn.Sequential(_ConvRelu(in_channels))
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1)
        self.in_channels, self.num_anchors = in_channels, num_anchors
        for m in self.modules():                          # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)
        self._operand_cache = OperandCache()

    set_neck_dtype = dtype_setter("neck_dtype", """``"f32"`` or ``"bf16"``: how the head runs from now on where no gradient is wanted, on
        the same weights.""")
    set_grad_dtype = dtype_setter("grad_dtype", """``"f32"`` or ``"bf16"``: the matrix pipe of the 3x3 convolution's input-gradient GEMM
        in the backward from now on (the 1x1 pair's 32 padded columns keep theirs on the fp32 GEMM).""")
    set_train_dtype = dtype_setter("train_dtype", """``"f32"`` or ``"bf16"``: how the head's forward runs from now on where a gradient IS
        wanted (:class:`_RPNHeadLevelFn`) - ``"bf16"``: the launches of ``neck_dtype="bf16"``.""")

    def _params(self):
        return (self.conv[0][0].weight, self.conv[0][0].bias, self.cls_logits.weight, self.cls_logits.bias, self.bbox_pred.weight,
                self.bbox_pred.bias)

    def _operands(self):
        """``(w3, b3, w1, b1)``: the 3x3 weight as [Cout, 3, 3, Cin] with its bias, and both 1x1 convolutions as one [5 A (padded
        to a multiple of 4), C] matrix with theirs, re-laid when a parameter changes."""
        w3, b3, wc, bc, wb, bb = ps = self._params()
        return self._operand_cache.get("f32", ps, lambda: (w3.detach().permute(0, 2, 3, 1).contiguous(), b3.detach(),
                                                           *stack_rows((wc.flatten(1), wb.flatten(1)), (bc, bb), 4)))

    def _operands_bf16(self):
        """:meth:`_operands` with both matrices as bf16 copies (``neck_dtype`` / ``train_dtype="bf16"``; the biases stay fp32, the
        stacked matrix's zero padding rows stay zero), cached beside them under the same key."""
        def build():
            w3, b3, w1, b1 = self._operands()
            return ops.cast_bf16(w3), b3, ops.cast_bf16(w1), b1
        return self._operand_cache.get("bf16", self._params(), build)

    def _dgrad_operand_bf16(self) -> torch.Tensor:
        """The weight operand of the 3x3 convolution's dgrad under ``grad_dtype="bf16"`` (flipped, in/out-swapped, bf16), re-made
        when the parameter changes."""
        w3 = self.conv[0][0].weight
        return self._operand_cache.get("dgrad", (w3,), lambda: conv3x3_dgrad_bf16(w3))

    def forward_level(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """One map ``[B, C, h, w]`` (any memory layout; channels-last costs no copy) -> objectness logits ``[B, h w A]`` and box
        deltas ``[B, h w A, 4]`` in (y, x, anchor) order."""
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"RPNHead: expected [B, {self.in_channels}, h, w], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"RPNHead: expected float32 features, got {x.dtype}")
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            # gradients are wanted: one differentiable node per level, on the operands of the eval path below
            return _RPNHeadLevelFn.apply(x, *self._params(), self)
        return _level_forward(x, self._operands_bf16() if self.neck_dtype == "bf16" else self._operands(), self.num_anchors)[0]

    def forward(self, features: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """All levels: logits ``[B, Ntot]`` and deltas ``[B, Ntot, 4]``, levels concatenated in the order given."""
        per_level = [self.forward_level(f) for f in features]
        return (torch.cat([p[0] for p in per_level], dim=1).contiguous(), torch.cat([p[1] for p in per_level], dim=1).contiguous())


class RegionProposalNetwork(nn.Module):
    """torchvision's ``RegionProposalNetwork``.  Eval mode: ``forward(features, image_size)`` returns the list of proposal boxes
    per image; with ``padded=True`` the fixed-size form ``(boxes [B, post, 4], scores [B, post], count [B])``.  Train mode with
    ``targets``: ``(proposals, {"loss_objectness", "loss_rpn_box_reg"})`` - the proposals detached and from the train top-n."""

    def __init__(self, anchor_generator: AnchorGenerator, head: RPNHead, pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000,
                 nms_thresh: float = 0.7, score_thresh: float = 0.0, min_size: float = 1e-3, pre_nms_top_n_train: int = 2000,
                 post_nms_top_n_train: int = 2000, fg_iou_thresh: float = 0.7, bg_iou_thresh: float = 0.3,
                 batch_size_per_image: int = 256, positive_fraction: float = 0.5):
        super().__init__()
        self.anchor_generator, self.head = anchor_generator, head
        self.pre_nms_top_n, self.post_nms_top_n = int(pre_nms_top_n), int(post_nms_top_n)
        self.pre_nms_top_n_train, self.post_nms_top_n_train = int(pre_nms_top_n_train), int(post_nms_top_n_train)
        self.nms_thresh, self.score_thresh, self.min_size = float(nms_thresh), float(score_thresh), float(min_size)
        self.fg_iou_thresh, self.bg_iou_thresh = float(fg_iou_thresh), float(bg_iou_thresh)
        self.batch_size_per_image, self.positive_fraction = int(batch_size_per_image), float(positive_fraction)
        self.smooth_l1_beta = 1.0 / 9.0                               # torchvision's compute_loss
        self._groups: Dict[tuple, torch.Tensor] = {}

    def _top_n(self) -> Tuple[int, int]:
        return (self.pre_nms_top_n_train, self.post_nms_top_n_train) if self.training else (self.pre_nms_top_n, self.post_nms_top_n)

    def _level_ids(self, level_sizes: Sequence[int], batch: int, device, pre_nms_top_n: Optional[int] = None) -> torch.Tensor:
        """int32 [B, Ksum]: the level of every top-k column - the NMS groups.  Constant per geometry, cached."""
        k = self.pre_nms_top_n if pre_nms_top_n is None else pre_nms_top_n
        key = (tuple(level_sizes), batch, k, str(device))
        g = self._groups.get(key)
        if g is None:
            ids = np.concatenate([np.full(min(k, n), l, dtype=np.int32) for l, n in enumerate(level_sizes)])
            g = torch.from_numpy(np.tile(ids, (batch, 1))).to(device)
            self._groups[key] = g
        return g

    def filter_proposals_padded(self, logits: torch.Tensor, deltas: torch.Tensor, anchors: torch.Tensor, level_sizes: Sequence[int],
                                image_size: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The three launches: top-k per level, decode, batched NMS with the level as group.  No synchronisation."""
        pre, post = self._top_n()
        idx = ops.rpn_topk(logits, level_sizes, pre)
        boxes, scores = ops.rpn_decode(logits, deltas, anchors, idx, image_size, self.min_size, self.score_thresh)
        groups = self._level_ids(level_sizes, logits.shape[0], logits.device, pre)
        _, count, out_boxes, out_scores = ops.batched_nms_padded(boxes, scores, groups, self.nms_thresh, post)
        return out_boxes, out_scores, count

    @staticmethod
    def pad_targets(targets, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's list of ``{"boxes": [G_i, 4], ...}`` -> ``(gt_boxes fp32 [B, Gmax, 4], gt_count int32 [B])``.  The shapes
        are known on the host: copies, no synchronisation.  A padded pair passes through."""
        if isinstance(targets, (tuple, list)) and len(targets) == 2 and isinstance(targets[0], torch.Tensor):
            gt_boxes, gt_count = targets
            if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or tuple(gt_count.shape) != (gt_boxes.shape[0],):
                raise ValueError(f"RegionProposalNetwork: padded targets {tuple(gt_boxes.shape)} / {tuple(gt_count.shape)} are not "
                                 "[B, Gmax, 4] / [B]")
            return gt_boxes.to(device=device, dtype=torch.float32).contiguous(), gt_count.to(device=device, dtype=torch.int32).contiguous()
        boxes = [t["boxes"] for t in targets]
        for bx in boxes:
            if bx.dim() != 2 or bx.shape[1] != 4:
                raise ValueError(f"RegionProposalNetwork: target boxes {tuple(bx.shape)} are not [G, 4]")
        gmax = max(max(int(bx.shape[0]) for bx in boxes), 1)
        gt_boxes = torch.zeros((len(boxes), gmax, 4), device=device, dtype=torch.float32)
        for i, bx in enumerate(boxes):
            if bx.shape[0]:
                gt_boxes[i, :bx.shape[0]] = bx.detach().to(device=device, dtype=torch.float32)
        gt_count = torch.tensor([int(bx.shape[0]) for bx in boxes], dtype=torch.int32).to(device)
        return gt_boxes, gt_count

    def compute_loss_padded(self, logits: torch.Tensor, deltas: torch.Tensor, anchors: torch.Tensor, gt_boxes: torch.Tensor,
                            gt_count: torch.Tensor, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Keys, target assignment and the two losses: three launches of this library behind one ``randint``.  No synchronisation."""
        B, N = logits.shape
        if gt_boxes.shape[0] != B:
            raise ValueError(f"RegionProposalNetwork: {gt_boxes.shape[0]} targets for {B} images")
        keys = torch.randint(0, 2 ** 31 - 1, (B, N), device=logits.device, dtype=torch.int32, generator=generator)
        labels, _, reg_targets, sampled = ops.rpn_targets(anchors, gt_boxes, gt_count, keys, self.fg_iou_thresh, self.bg_iou_thresh,
                                                          self.batch_size_per_image, self.positive_fraction)
        return _RPNLossFn.apply(logits, deltas, labels, reg_targets, sampled, self.smooth_l1_beta)

    def forward(self, features: Union[Dict[str, torch.Tensor], Sequence[torch.Tensor]], image_size: Tuple[int, int], targets=None,
                padded: bool = False, generator: Optional[torch.Generator] = None):
        if self.training and targets is None:
            raise RuntimeError("RegionProposalNetwork: inference only without targets (in train mode the RPN losses need them) - "
                               "pass targets or call .eval() first")
        feats = list(features.values()) if isinstance(features, dict) else list(features)
        losses = None
        if self.training:
            logits, deltas = self.head(feats)                         # differentiable when gradients are wanted
        else:
            with torch.no_grad():
                logits, deltas = self.head(feats)
        with torch.no_grad():
            anchors, level_sizes = self.anchor_generator([tuple(f.shape[-2:]) for f in feats], tuple(image_size), logits.device)
            A = self.head.num_anchors
            if any(n != f.shape[-2] * f.shape[-1] * A for n, f in zip(level_sizes, feats)):
                raise ValueError("RegionProposalNetwork: the anchor generator and the head disagree on anchors per location")
            boxes, scores, count = self.filter_proposals_padded(logits.detach(), deltas.detach(), anchors, level_sizes, image_size)
        if self.training:
            gt_boxes, gt_count = self.pad_targets(targets, logits.device)
            obj, box = self.compute_loss_padded(logits, deltas, anchors, gt_boxes, gt_count, generator)
            losses = {"loss_objectness": obj, "loss_rpn_box_reg": box}
        out = (boxes, scores, count) if padded else [boxes[i, :n] for i, n in enumerate(count.tolist())]
        return (out, losses) if self.training else out
