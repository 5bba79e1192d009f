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

Training (``train()`` mode with targets): ``select_training_samples`` - the GT boxes join the proposals, ``Matcher(0.5, 0.5)``,
``BalancedPositiveNegativeSampler(512, 0.25)``, ``BoxCoder(10, 10, 5, 5).encode`` - is ONE launch with fixed-size results and
``fastrcnn_loss`` with its gradient two more (``csrc/roi_train.hip``); the sampler is driven by random keys drawn on the device, so
nothing synchronises.  :class:`MultiScaleRoIAlign` is differentiated by one ``torch.autograd.Function`` over the five maps whose
backward is ONE gather launch without atomics; :class:`TwoMLPHead` and :class:`FastRCNNPredictor` by one function each whose
backward is ``grad_ops.linear_bwd`` per layer, which the RPN head and the FPN laterals share (``ldit_linear_f32`` on the transposed
weights, bf16 MFMA weight gradients with fp32 accumulation, ``ldit_colsum_f32`` for the biases; ``fc6``'s gradient is permuted back
to torchvision's columns).
The sampled rows come out positives first, not in torchvision's candidate order - the losses are sums.  ``train()`` mode WITHOUT
targets stays refused.  torchvision is not
installed offline: the semantics are restated from its documented behaviour (``tests/roi_oracle.py``) - parity unpinned with
respect to torchvision itself, as for the FPN and the RPN.  Parameter names follow torchvision, so detector checkpoints load
(``roi_heads.box_head.fc6.weight`` ...).

The dtype options are ``grad_ops.py``'s.  What is particular to this stage: under ``head_dtype="bf16"`` RoIAlign rounds its fp32 rows
to bf16 at the store (``ldit_roi_align_levels_bf16`` - half the bytes written and read back), ``fc6`` and ``fc7`` have the ReLU in the
GEMM's epilogue (no ``relu_`` launch) and the predictor stores its fp32 value unrounded.  ``train_dtype="bf16"`` runs those launches
where :meth:`RoIHeads.head_padded` wants a gradient as ONE node, :class:`_BoxHeadBF16Fn`, from the fp32 maps to the fp32 result - one
node, because autograd converts a gradient to the dtype of the forward output it belongs to: bf16 rows handed from a RoIAlign node to
a head node would have fc6's fp32 input gradient rounded to bf16 on the way back.  A head with a reduction length that is no multiple
of 64 keeps the three nodes and every launch of ``"f32"``; so does a :class:`TwoMLPHead` called on its own (fp32 rows in, fp32 out).
``grad_dtype`` concerns fc6's and fc7's dgrad; the predictor's (32 padded columns), RoIAlign's backward and the losses stay fp32.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from .. import _lib, ops
from .grad_ops import BF16_K, OperandCache, check_dtype, dtype_setter, linear_bwd, linear_dgrad_bf16, pad_grad_row, stack_rows


def _nhwc_f32(f: torch.Tensor) -> torch.Tensor:
    """The map as the kernel reads it: float32 with channel stride 1 (no copy for the FPN's own outputs and their strided views)."""
    if f.dtype != torch.float32:
        f = f.float()
    if f.stride(1) != 1:
        f = f.contiguous(memory_format=torch.channels_last)
    return f


class _RoIAlignLevelsFn(torch.autograd.Function):
    """``ldit_roi_align_levels_f32`` with a gradient for every map: the forward keeps the level of each row, the backward is ONE launch
    of the gather kernel (``csrc/roi_train.hip``) and hands autograd NCHW views of the NHWC gradients it wrote - a strided view such
    as ``pool`` gets a gradient of its own shape, autograd adds it into the viewed map.
    apply(boxes, count, image_size, output_size, sampling_ratio, canonical_scale, canonical_level, *maps) -> [B R, P, P, C]."""

    @staticmethod
    def forward(ctx, boxes, count, image_size, output_size, sampling_ratio, canonical_scale, canonical_level, *maps):
        out, levels = ops.roi_align_levels([_nhwc_f32(f.detach()) for f in maps], boxes, count, image_size, output_size, sampling_ratio,
                                           canonical_scale, canonical_level, return_levels=True)
        ctx.save_for_backward(boxes, levels) if count is None else ctx.save_for_backward(boxes, levels, count)
        ctx.geometry = ([tuple(f.shape[-2:]) for f in maps], tuple(image_size), output_size, sampling_ratio)
        return out

    @staticmethod
    def backward(ctx, d_out):
        boxes, levels = ctx.saved_tensors[:2]
        count = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        shapes, image_size, output_size, sampling_ratio = ctx.geometry
        grads = ops.roi_align_levels_bwd(d_out.contiguous(), boxes, count, levels, shapes, image_size, output_size, sampling_ratio)
        return (None,) * 7 + tuple(grads)


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
                image_size: Tuple[int, int], out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """``features``: the named maps (or the maps themselves, finest first), ``boxes`` [B, R, 4], ``count`` int32 [B] or None.
        Returns ``[B * R, P, P, C]``; rows past the count are zero.  ``out_dtype=torch.bfloat16`` (no gradient): the rows rounded
        to bf16 at the kernel's store."""
        feats = [features[n] for n in self.featmap_names] if isinstance(features, dict) else list(features)
        if out_dtype != torch.float32:
            return ops.roi_align_levels([_nhwc_f32(f.detach()) for f in feats], boxes, count, image_size, self.output_size,
                                        self.sampling_ratio, self.canonical_scale, self.canonical_level, out_dtype=out_dtype)
        if torch.is_grad_enabled() and any(f.requires_grad for f in feats):
            # gradients are wanted for the maps: the differentiable node (the path below is untouched)
            return _RoIAlignLevelsFn.apply(boxes.detach(), count, tuple(image_size), self.output_size, self.sampling_ratio,
                                           self.canonical_scale, self.canonical_level, *feats)
        return ops.roi_align_levels([_nhwc_f32(f.detach()) for f in feats], boxes, count, image_size, self.output_size,
                                    self.sampling_ratio, self.canonical_scale, self.canonical_level)


def _mlp_bwd(d7, x0, h6, h7, w6p, w7, pooled_shape, need, grad_dtype: str, head: "TwoMLPHead"):
    """fc7 then fc6 of a :class:`TwoMLPHead` backwards: ``d7`` the gradient of the head's output before its ReLU mask, ``x0`` [M, K] the
    pooled rows, ``h6`` / ``h7`` the two activations (the masks), ``w6p`` fc6's weight in the rows' (ph, pw, c) column order; ``need``:
    (pooled rows, fc6.weight, fc6.bias, fc7.weight, fc7.bias).  Returns those five gradients, fc6's weight gradient permuted back to
    torchvision's (c, ph, pw) columns and the rows' in ``pooled_shape``."""
    M, ph, pw, Cc = pooled_shape
    operands = lambda i: (lambda: head.dgrad_operands_bf16(Cc, ph, pw)[i])                # noqa: E731
    d6, g_w7, g_b7 = linear_bwd(d7, h6, w7.contiguous(), True, need[3], need[4], grad_dtype, act=h7, dgrad_w=operands(1))
    g_x, g_w6p, g_b6 = linear_bwd(d6, x0, w6p, need[0], need[1], need[2], grad_dtype, act=h6, dgrad_w=operands(0))
    if g_w6p is not None:
        g_w6p = g_w6p.view(-1, ph, pw, Cc).permute(0, 3, 1, 2).reshape(g_w6p.shape[0], -1)
    return (g_x.view(M, ph, pw, Cc) if g_x is not None else None), g_w6p, g_b6, g_w7, g_b7


def _predictor_bwd(dy, x, w, NC: int, need, grad_dtype: str = "f32"):
    """The stacked predictor GEMM backwards: ``dy`` [M, a multiple of 32 columns], ``w`` the stacked weight; ``need``: (input,
    cls_score.weight, .bias, bbox_pred.weight, .bias).  Returns those five gradients, the stacked ones split back into the layers'."""
    g_x, g_w, g_b = linear_bwd(dy, x, w, need[0], need[1] or need[3], need[2] or need[4], grad_dtype)
    return (g_x, g_w[:NC] if need[1] else None, g_b[:NC] if need[2] else None, g_w[NC:5 * NC] if need[3] else None,
            g_b[NC:5 * NC] if need[4] else None)


class _TwoMLPHeadFn(torch.autograd.Function):
    """:class:`TwoMLPHead` with gradients for the pooled rows and the four parameters.
    apply(pooled [M, P, P, C], fc6.weight, fc6.bias, fc7.weight, fc7.bias, head) -> [M, representation_size].  ``head``: the
    :class:`TwoMLPHead` whose parameters these are; the forward reads its ``grad_dtype`` and keeps it on ``ctx`` - a setter called
    between forward and backward does not change that backward - and the backward takes the dgrad operands from its cache."""

    @staticmethod
    def forward(ctx, pooled, w6, b6, w7, b7, head):
        M, ph, pw, Cc = pooled.shape
        x0 = pooled.detach().reshape(M, ph * pw * Cc)
        w6p = w6.detach().view(w6.shape[0], Cc, ph, pw).permute(0, 2, 3, 1).reshape(w6.shape[0], -1).contiguous()      # (ph, pw, c) columns
        h6 = ops.linear(x0, w6p, b6.detach())
        torch.relu_(h6)
        h7 = ops.linear(h6, w7.detach().contiguous(), b7.detach())
        torch.relu_(h7)
        ctx.saved = (x0, h6, h7, w6p, w7.detach())
        ctx.pooled_shape = (M, ph, pw, Cc)
        ctx.head, ctx.grad_dtype = head, check_dtype("grad_dtype", head.grad_dtype)
        return h7.clone()                                             # the saved activation is the ReLU mask: keep it private

    @staticmethod
    def backward(ctx, d7):
        if ctx.saved is None:
            raise RuntimeError("TwoMLPHead: backward a second time (its saved activations are freed after the first)")
        saved, ctx.saved = ctx.saved, None
        return _mlp_bwd(d7.contiguous(), *saved, ctx.pooled_shape, ctx.needs_input_grad, ctx.grad_dtype, ctx.head) + (None,)


class _PredictorFn(torch.autograd.Function):
    """:class:`FastRCNNPredictor`'s stacked GEMM with gradients for its input and the four parameters; the stacked weight gradient
    is split back into ``cls_score`` and ``bbox_pred``.  apply(x [M, K], cls_score.weight, .bias, bbox_pred.weight, .bias) ->
    [M, 5 NC (padded to a multiple of 32)]: the padding columns are zero."""

    @staticmethod
    def forward(ctx, x, wc, bc, wb, bb):
        NC = wc.shape[0]
        w, b = stack_rows((wc, wb), (bc, bb), 32)                     # 32: the K of the dgrad GEMM, a multiple of 8 for the wgrad
        x = x.detach().contiguous()
        ctx.saved = (x, w)
        ctx.NC = NC
        return ops.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("FastRCNNPredictor: backward a second time (its saved input is freed after the first)")
        (x, w), ctx.saved = ctx.saved, None
        return _predictor_bwd(dy.contiguous(), x, w, ctx.NC, ctx.needs_input_grad)


class _BoxHeadBF16Fn(torch.autograd.Function):
    """The box head under ``train_dtype="bf16"``, RoIAlign -> fc6 -> fc7 -> predictor as one node: fp32 maps and the eight parameters in,
    fp32 ``[M, 5 NC (+ pad)]`` out, every bf16 tensor inside.  The forward is ``head_dtype="bf16"``'s - ``ldit_roi_align_levels_bf16``,
    :meth:`TwoMLPHead.layers_bf16`, :meth:`FastRCNNPredictor.forward_stacked_bf16` on the modules' cached operands.  The backward is
    the fp32 head's, :func:`_predictor_bwd` and :func:`_mlp_bwd`, on the saved bf16 rows and activations (wgrad operands and ReLU masks
    as they stand), then :class:`_RoIAlignLevelsFn`'s one gather launch on the fp32 ``g_x`` of fc6's dgrad.  The box head's
    ``grad_dtype`` is read in the forward and kept on ``ctx``: a setter called between forward and backward does not change that
    backward.
    apply(roi_heads, boxes, count, image_size, *maps (5), fc6.weight, fc6.bias, fc7.weight, fc7.bias, cls_score.weight, .bias,
    bbox_pred.weight, .bias) -> [B R, 5 NC (+ pad)]."""

    @staticmethod
    def forward(ctx, heads, boxes, count, image_size, *args):
        maps, pool, head, pred = args[:-8], heads.box_roi_pool, heads.box_head, heads.box_predictor
        x0, levels = ops.roi_align_levels([_nhwc_f32(f.detach()) for f in maps], boxes, count, image_size, pool.output_size,
                                          pool.sampling_ratio, pool.canonical_scale, pool.canonical_level, return_levels=True,
                                          out_dtype=torch.bfloat16)
        M, ph, pw, Cc = x0.shape
        h6, h7 = head.layers_bf16(x0)
        y = pred.forward_stacked_bf16(h7)
        ctx.saved = (boxes, count, levels, x0, h6, h7, head.fc6_weight_hwc(Cc, ph, pw), args[-6].detach(), pred._operands()[0])
        ctx.geometry = ([tuple(f.shape[-2:]) for f in maps], tuple(image_size), pool.output_size, pool.sampling_ratio)
        ctx.head, ctx.grad_dtype = head, check_dtype("grad_dtype", head.grad_dtype)
        ctx.NC = pred.num_classes
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.saved is None:
            raise RuntimeError("RoIHeads: backward through the box head a second time (its saved activations are freed after the first)")
        boxes, count, levels, x0, h6, h7, w6p, w7, wp = ctx.saved
        ctx.saved = None
        shapes, image_size, output_size, sampling_ratio = ctx.geometry
        M, ph, pw, Cc = x0.shape
        nmaps = len(shapes)
        need = ctx.needs_input_grad[4:]                               # maps, then (w6, b6, w7, b7, wc, bc, wb, bb)
        need_maps, np_ = any(need[:nmaps]), need[nmaps:]
        # (the predictor's 32 columns are below the bf16 GEMM's k-tile: its dgrad is the fp32 GEMM under either grad_dtype)
        d7, *g_pred = _predictor_bwd(pad_grad_row(((dy.shape[1], dy),), M, dy.device), h7, wp, ctx.NC, (True,) + np_[4:], ctx.grad_dtype)
        g_x, *g_mlp = _mlp_bwd(d7, x0.view(M, ph * pw * Cc), h6, h7, w6p, w7, (M, ph, pw, Cc), (need_maps,) + np_[:4], ctx.grad_dtype, ctx.head)
        g_maps = (None,) * nmaps
        if need_maps:
            g_maps = tuple(ops.roi_align_levels_bwd(g_x, boxes, count, levels, shapes, image_size, output_size, sampling_ratio))
        return (None,) * 4 + g_maps + tuple(g_mlp) + tuple(g_pred)


class _BoxLossFn(torch.autograd.Function):
    """``ldit_box_loss_f32`` as a differentiable node: the kernel has already written both gradients for unit upstream into their
    column ranges of one buffer, the backward scales each range by its upstream scalar."""

    @staticmethod
    def forward(ctx, head_out, labels, reg_targets, sampled, num_classes, beta):
        loss, d_head = ops.box_loss(head_out.detach().contiguous(), labels, reg_targets, sampled, num_classes, beta)
        ctx.save_for_backward(d_head)
        ctx.NC = int(num_classes)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        (d_head,) = ctx.saved_tensors
        NC, ld = ctx.NC, d_head.shape[1]
        scale = torch.cat([g_cls.reshape(1).expand(NC), g_box.reshape(1).expand(4 * NC), d_head.new_zeros(ld - 5 * NC)])
        return d_head * scale, None, None, None, None, None


def _wants_grad(module: nn.Module, x: torch.Tensor) -> bool:
    return module.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


class TwoMLPHead(nn.Module):
    """torchvision's ``TwoMLPHead(in_channels, representation_size)``: ``fc6``, ``fc7``, a ReLU after each."""

    def __init__(self, in_channels: int = 256 * 7 * 7, representation_size: int = 1024, grad_dtype: str = "f32", train_dtype: str = "f32"):
        super().__init__()
        self.grad_dtype = check_dtype("grad_dtype", grad_dtype)
        self.train_dtype = check_dtype("train_dtype", train_dtype)
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        self._operand_cache = OperandCache()

    set_grad_dtype = dtype_setter("grad_dtype", """``"f32"`` or ``"bf16"``: the matrix pipe of the two input-gradient GEMMs of the backward
        from now on (``grad_ops.linear_bwd``).""")
    set_train_dtype = dtype_setter("train_dtype", """``"f32"`` or ``"bf16"``: how :meth:`RoIHeads.head_padded` runs this head from now on
        where a gradient IS wanted - ``"bf16"``: the launches of ``head_dtype="bf16"`` inside :class:`_BoxHeadBF16Fn`.  :meth:`forward`
        on its own (fp32 rows in, fp32 out) does not depend on it.""")

    def fc6_weight_hwc(self, channels: int, ph: int, pw: int) -> torch.Tensor:
        """``fc6.weight`` with its columns re-ordered from torchvision's ``flatten(start_dim=1)`` of (c, ph, pw) to (ph, pw, c) - the
        order of a pooled row; re-laid when the parameter changes."""
        w = self.fc6.weight
        if channels * ph * pw != w.shape[1]:
            raise ValueError(f"TwoMLPHead: pooled rows of {ph} x {pw} x {channels} do not match fc6's {w.shape[1]} inputs")
        return self._operand_cache.get("fc6_hwc", (w,), lambda: w.detach().view(w.shape[0], channels, ph, pw).permute(0, 2, 3, 1)
                                       .reshape(w.shape[0], -1).contiguous(), channels, ph, pw)

    def operands_bf16(self, channels: int, ph: int, pw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The bf16 GEMM's weight operands: :meth:`fc6_weight_hwc` and ``fc7.weight`` rounded to bf16, re-made when a parameter
        changes."""
        return self._operand_cache.get("bf16", (self.fc6.weight, self.fc7.weight),
                                       lambda: (ops.cast_bf16(self.fc6_weight_hwc(channels, ph, pw)),
                                                ops.cast_bf16(self.fc7.weight.detach().contiguous())), channels, ph, pw)

    def dgrad_operands_bf16(self, channels: int, ph: int, pw: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The weight operands of the two dgrad GEMMs under ``grad_dtype="bf16"``: :meth:`fc6_weight_hwc` and ``fc7.weight``, each
        transposed and rounded to bf16, re-made when a parameter changes."""
        return self._operand_cache.get("dgrad", (self.fc6.weight, self.fc7.weight),
                                       lambda: (linear_dgrad_bf16(self.fc6_weight_hwc(channels, ph, pw)), linear_dgrad_bf16(self.fc7.weight)),
                                       channels, ph, pw)

    def layers_bf16(self, pooled: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``pooled`` bf16 [M, P, P, C] -> both activations, bf16 [M, representation_size] each: fc6 and fc7 on the bf16 GEMM, the ReLU
        in its epilogue.  No gradient."""
        if pooled.dim() != 4 or pooled.dtype != torch.bfloat16:
            raise ValueError(f"TwoMLPHead: expected bfloat16 pooled rows [M, P, P, C], got {pooled.dtype} {tuple(pooled.shape)}")
        M, ph, pw, Cc = pooled.shape
        w6, w7 = self.operands_bf16(Cc, ph, pw)
        h6 = ops.linear_bf16(pooled.reshape(M, ph * pw * Cc), w6, self.fc6.bias.detach(), _lib.EPI_BIAS_RELU)
        return h6, ops.linear_bf16(h6, w7, self.fc7.bias.detach(), _lib.EPI_BIAS_RELU)

    def forward_bf16(self, pooled: torch.Tensor) -> torch.Tensor:
        """:meth:`layers_bf16`'s second activation: the head's bf16 output."""
        return self.layers_bf16(pooled)[1]

    def forward(self, pooled: torch.Tensor) -> torch.Tensor:
        """``pooled`` [M, P, P, C] (channels innermost) -> [M, representation_size]."""
        if pooled.dim() != 4:
            raise ValueError(f"TwoMLPHead: expected pooled rows [M, P, P, C], got {tuple(pooled.shape)}")
        M, ph, pw, Cc = pooled.shape
        if Cc * ph * pw != self.fc6.weight.shape[1]:
            raise ValueError(f"TwoMLPHead: pooled rows of {ph} x {pw} x {Cc} do not match fc6's {self.fc6.weight.shape[1]} inputs")
        if _wants_grad(self, pooled):
            # gradients are wanted: the differentiable node (the eval path below and its cache are untouched)
            return _TwoMLPHeadFn.apply(pooled, self.fc6.weight, self.fc6.bias, self.fc7.weight, self.fc7.bias, self)
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
        self._operand_cache = OperandCache()

    def _operands(self):
        """Both layers as one [5 NC (padded to a multiple of 4), in_channels] matrix, re-laid when a parameter changes."""
        wc, bc, wb, bb = self.cls_score.weight, self.cls_score.bias, self.bbox_pred.weight, self.bbox_pred.bias
        return self._operand_cache.get("f32", (wc, bc, wb, bb), lambda: stack_rows((wc, wb), (bc, bb), 4))

    def forward_stacked_bf16(self, x: torch.Tensor) -> torch.Tensor:
        """bf16 [M, in_channels] -> fp32 [M, 5 NC (+ pad)] on the bf16 GEMM: the stacked weight rounded to bf16 (re-made when a
        parameter changes), fp32 bias, the accumulator stored unrounded; the padding columns are zero.  No gradient."""
        w, b = self._operands()
        w16 = self._operand_cache.get("bf16", (self.cls_score.weight, self.bbox_pred.weight), lambda: ops.cast_bf16(w))
        return ops.linear_bf16(x, w16, b, _lib.EPI_F32)

    def forward_stacked(self, x: torch.Tensor) -> torch.Tensor:
        """[M, in_channels] -> [M, 5 NC (+ pad)]: the class logits in columns [0, NC), the deltas in [NC, 5 NC)."""
        if _wants_grad(self, x):
            # gradients are wanted: the differentiable node, its row padded to a multiple of 32 columns (the eval path is untouched)
            return _PredictorFn.apply(x, self.cls_score.weight, self.cls_score.bias, self.bbox_pred.weight, self.bbox_pred.bias)
        w, b = self._operands()
        return ops.linear(x, w, b)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        y, NC = self.forward_stacked(x), self.num_classes
        return y[:, :NC], y[:, NC:5 * NC]


class RoIHeads(nn.Module):
    """torchvision's ``RoIHeads`` (box branch).  Eval mode: ``forward(features, proposals, count, image_size)`` returns the list of
    ``{boxes, labels, scores}`` per image; with ``padded=True`` the fixed-size form ``(boxes [B, D, 4], scores [B, D], labels [B, D],
    count [B])``, ``D = detections_per_img``.  Train mode with ``targets`` (the reference's list of ``{"boxes", "labels"}`` or the
    padded triple of :meth:`pad_targets`): ``{"loss_classifier", "loss_box_reg"}``; ``generator`` seeds the sampler's keys."""

    def __init__(self, box_roi_pool: MultiScaleRoIAlign, box_head: TwoMLPHead, box_predictor: FastRCNNPredictor,
                 bbox_reg_weights: Optional[Sequence[float]] = None, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                 detections_per_img: int = 100, min_size: float = 1e-2, fg_iou_thresh: float = 0.5, bg_iou_thresh: float = 0.5,
                 batch_size_per_image: int = 512, positive_fraction: float = 0.25, head_dtype: str = "f32",
                 grad_dtype: Optional[str] = None, train_dtype: Optional[str] = None):
        super().__init__()
        self.head_dtype = check_dtype("head_dtype", head_dtype)
        self.box_roi_pool, self.box_head, self.box_predictor = box_roi_pool, box_head, box_predictor
        if grad_dtype is not None:                                    # None: the box head keeps the setting it was built with
            self.set_grad_dtype(grad_dtype)
        if train_dtype is not None:                                   # (alike)
            self.set_train_dtype(train_dtype)
        self.bbox_reg_weights = tuple(float(w) for w in (bbox_reg_weights or (10.0, 10.0, 5.0, 5.0)))
        self.score_thresh, self.nms_thresh, self.min_size = float(score_thresh), float(nms_thresh), float(min_size)
        self.detections_per_img = int(detections_per_img)
        self.fg_iou_thresh, self.bg_iou_thresh = float(fg_iou_thresh), float(bg_iou_thresh)
        self.batch_size_per_image, self.positive_fraction = int(batch_size_per_image), float(positive_fraction)
        self.smooth_l1_beta = 1.0 / 9.0                               # torchvision's fastrcnn_loss

    def head_padded(self, features, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size: Tuple[int, int]) -> torch.Tensor:
        """RoIAlign and the three GEMMs: ``[B * R, 5 NC (+ pad)]`` fp32 logits | deltas per proposal row.  ``head_dtype="bf16"``
        in eval mode, where no gradient is wanted: bf16 pooled rows, ``fc6`` / ``fc7`` on the bf16 GEMM with the ReLU epilogue, the
        predictor on it with an fp32 result - no fp32 pooled tensor, no ``relu_`` launch."""
        if self.head_dtype == "bf16" and not self.training and not self._wants_grad(features):
            pooled = self.box_roi_pool(features, proposals, count, image_size, out_dtype=torch.bfloat16)
            return self.box_predictor.forward_stacked_bf16(self.box_head.forward_bf16(pooled))
        if self.train_dtype == "bf16" and self._trains_bf16(features):
            feats = [features[n] for n in self.box_roi_pool.featmap_names] if isinstance(features, dict) else list(features)
            head, pred = self.box_head, self.box_predictor
            return _BoxHeadBF16Fn.apply(self, proposals.detach(), count, tuple(image_size), *feats, head.fc6.weight, head.fc6.bias,
                                        head.fc7.weight, head.fc7.bias, pred.cls_score.weight, pred.cls_score.bias, pred.bbox_pred.weight,
                                        pred.bbox_pred.bias)
        pooled = self.box_roi_pool(features, proposals, count, image_size)
        return self.box_predictor.forward_stacked(self.box_head(pooled))

    def _trains_bf16(self, features) -> bool:
        """Whether this call is the one ``train_dtype="bf16"`` concerns: train mode, a gradient wanted by a map or a parameter, and
        three reduction lengths the bf16 GEMM takes (else: every launch of ``"f32"``)."""
        head, pred = self.box_head, self.box_predictor
        if not (self.training and head.training and pred.training and torch.is_grad_enabled()):
            return False
        if not (self._wants_grad(features) or any(p.requires_grad for m in (head, pred) for p in m.parameters())):
            return False
        return head.fc6.in_features % BF16_K == 0 and head.fc6.out_features % BF16_K == 0 and head.fc7.out_features % BF16_K == 0

    set_head_dtype = dtype_setter("head_dtype", """``"f32"`` or ``"bf16"``: how the eval-mode head runs from now on.""")

    @property
    def grad_dtype(self) -> str:
        """The box head's setting (:meth:`TwoMLPHead.set_grad_dtype`): fc6's and fc7's dgrad GEMMs.  RoIAlign's backward, the
        predictor (32 padded columns: below the bf16 GEMM's k-tile) and the losses are fp32 under either."""
        return self.box_head.grad_dtype

    def set_grad_dtype(self, grad_dtype: str) -> "RoIHeads":
        self.box_head.set_grad_dtype(grad_dtype)
        return self

    @property
    def train_dtype(self) -> str:
        """The box head's setting (:meth:`TwoMLPHead.set_train_dtype`): under ``"bf16"`` :meth:`head_padded` runs RoIAlign, fc6, fc7 and
        the predictor as one bf16 node where a gradient is wanted."""
        return self.box_head.train_dtype

    def set_train_dtype(self, train_dtype: str) -> "RoIHeads":
        self.box_head.set_train_dtype(train_dtype)
        return self

    def _wants_grad(self, features) -> bool:
        feats = features.values() if isinstance(features, dict) else features
        return torch.is_grad_enabled() and any(f.requires_grad for f in feats)

    @staticmethod
    def pad_targets(targets, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The reference's list of ``{"boxes": [G_i, 4], "labels": [G_i]}`` -> ``(gt_boxes fp32 [B, Gmax, 4], gt_labels int32
        [B, Gmax], gt_count int32 [B])``.  The shapes are known on the host: copies, no synchronisation.  A padded triple passes
        through."""
        if isinstance(targets, (tuple, list)) and len(targets) == 3 and isinstance(targets[0], torch.Tensor):
            gt_boxes, gt_labels, gt_count = targets
            if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]) or \
                    tuple(gt_count.shape) != (gt_boxes.shape[0],):
                raise ValueError(f"RoIHeads: padded targets {tuple(gt_boxes.shape)} / {tuple(gt_labels.shape)} / {tuple(gt_count.shape)} are "
                                 "not [B, Gmax, 4] / [B, Gmax] / [B]")
            return (gt_boxes.to(device=device, dtype=torch.float32).contiguous(), gt_labels.to(device=device, dtype=torch.int32).contiguous(),
                    gt_count.to(device=device, dtype=torch.int32).contiguous())
        for t in targets:
            bx, lb = t["boxes"], t["labels"]
            if bx.dim() != 2 or bx.shape[1] != 4 or tuple(lb.shape) != (bx.shape[0],):
                raise ValueError(f"RoIHeads: target boxes {tuple(bx.shape)} / labels {tuple(lb.shape)} are not [G, 4] / [G]")
        gmax = max(max(int(t["boxes"].shape[0]) for t in targets), 1)
        gt_boxes = torch.zeros((len(targets), gmax, 4), device=device, dtype=torch.float32)
        gt_labels = torch.zeros((len(targets), gmax), device=device, dtype=torch.int32)
        for i, t in enumerate(targets):
            g = int(t["boxes"].shape[0])
            if g:
                gt_boxes[i, :g] = t["boxes"].detach().to(device=device, dtype=torch.float32)
                gt_labels[i, :g] = t["labels"].detach().to(device=device, dtype=torch.int32)
        gt_count = torch.tensor([int(t["boxes"].shape[0]) for t in targets], dtype=torch.int32).to(device)
        return gt_boxes, gt_labels, gt_count

    def select_training_samples_padded(self, proposals: torch.Tensor, count: Optional[torch.Tensor], gt_boxes: torch.Tensor,
                                       gt_labels: torch.Tensor, gt_count: torch.Tensor, generator: Optional[torch.Generator] = None):
        """Keys and ``ldit_roi_targets_f32``: ``(rois [B, S, 4], labels, reg_targets, matched, sampled)``.  No synchronisation."""
        B, R = proposals.shape[:2]
        if gt_boxes.shape[0] != B:
            raise ValueError(f"RoIHeads: {gt_boxes.shape[0]} targets for {B} images")
        if count is None:
            count = torch.full((B,), R, device=proposals.device, dtype=torch.int32)
        keys = torch.randint(0, 2 ** 31 - 1, (B, R + gt_boxes.shape[1]), device=proposals.device, dtype=torch.int32, generator=generator)
        return ops.roi_targets(proposals.detach().contiguous(), count, gt_boxes, gt_labels, gt_count, keys, self.fg_iou_thresh,
                               self.bg_iou_thresh, self.batch_size_per_image, self.positive_fraction, self.bbox_reg_weights)

    def losses_padded(self, features, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size: Tuple[int, int], gt_boxes: torch.Tensor,
                      gt_labels: torch.Tensor, gt_count: torch.Tensor, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """Sampling, RoIAlign on the sampled rows, the head and ``fastrcnn_loss``: differentiable down to the maps, no
        synchronisation."""
        rois, labels, reg_targets, _, sampled = self.select_training_samples_padded(proposals, count, gt_boxes, gt_labels, gt_count, generator)
        rows = sampled.sum(dim=1, dtype=torch.int32)                  # the sampled rows sit in front of the padding
        y = self.head_padded(features, rois, rows, image_size)
        cls, box = _BoxLossFn.apply(y, labels, reg_targets, sampled, self.box_predictor.num_classes, self.smooth_l1_beta)
        return {"loss_classifier": cls, "loss_box_reg": box}

    def forward(self, features, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size: Tuple[int, int], targets=None,
                padded: bool = False, generator: Optional[torch.Generator] = None):
        if self.training:
            if targets is None:
                raise RuntimeError("RoIHeads: inference only without targets (in train mode the box losses need them) - pass targets or "
                                   "call .eval() first")
            if proposals.dim() != 3 or proposals.shape[-1] != 4:
                raise ValueError(f"RoIHeads: expected padded proposals [B, R, 4], got {tuple(proposals.shape)}")
            gt_boxes, gt_labels, gt_count = self.pad_targets(targets, proposals.device)
            return self.losses_padded(features, proposals, count, image_size, gt_boxes, gt_labels, gt_count, generator)
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
