"""``DiTWithFPN`` with the reference's surface (ref ``src/layoutdit/modeling/dit_backbone.py:65-90``): ``DiTBackbone`` +
torchvision's ``FeaturePyramidNetwork([C] * 4, 256, extra_blocks=LastLevelMaxPool())``, ``out_channels = 256``,
``forward(x) -> OrderedDict{p2, p3, p4, p5, pool}`` - re-designed for the MI355X instead of translated:

* the four 1x1 lateral convolutions run on the TOKENS of the taps (``ldit_linear_f32`` on ``[B * 197, C]``), not on the
  rescaled maps: a 1x1 convolution commutes with the bilinear rescale of ``DiTBackbone.forward`` (both are linear and the
  rescale's weights sum to one), so the 768-channel ``p2`` map (616 MB at bs=64) is never materialised and the p2 lateral
  costs 16x fewer FLOPs;
* rescale + top-down nearest add is one NHWC kernel per level (``ldit_fpn_merge_f32``);
* the 3x3 output convolutions are implicit-im2col fp32 MFMA GEMMs on the NHWC maps (``ldit_conv3x3_nhwc_f32``); their
  results are returned as ``[B, 256, H, W]`` tensors in channels-last memory (exactly the kind of strided NCHW view the
  reference's own ``p4`` is, ref dit_backbone.py:52-54);
* ``LastLevelMaxPool`` (``max_pool2d(kernel 1, stride 2)``) is a strided view.

torchvision is not installed offline and its source is not part of the reference: the FPN arithmetic is
restated from its documented forward (``oracle/fpn_oracle_torch.py``) - **parity unpinned** with respect to torchvision itself.
Parameter names follow torchvision (``fpn.inner_blocks.{i}.0.weight`` ...), so detector checkpoints load.

Training (round 3): ``self.fpn(feats)`` is differentiated as the reference's loop does it (ref dit_backbone.py:87-90 under
ref trainer.py:169-178) - :class:`_FPNFn` is one ``torch.autograd.Function`` over the whole stage whose backward runs on the
library's kernels: the 3x3 convolutions through ``grad_ops.conv3x3_bwd`` and the laterals through ``grad_ops.linear_bwd``, which
the RPN head and the box head share (dgrad = the forward's fp32 GEMM on the flipped / transposed weight, wgrad = bf16 MFMA
GEMMs on reduction-major operands with fp32 accumulation, so gradients of the FPN weights carry bf16 operand rounding, like the
encoder's), the merge adjoint and the bias column sums in ``csrc/fpn_bwd.hip``.  Gradients reach the four taps, hence the
encoder (``layoutdit_amd.training``).  Oracle: autograd of ``oracle/fpn_oracle_torch.py`` (parity unpinned, as above).

The dtype options are ``grad_ops.py``'s.  What is particular to this stage: ``neck_dtype`` and ``train_dtype`` concern the four 3x3
output convolutions - per level the merged fp32 map is copied once into a zero-padded bf16 map and ``ldit_conv3x3_nhwc_bf16``
writes the fp32 NHWC result, so every consumer sees the tensors it sees today; under ``train_dtype`` that copy carries the slack
rows of the wgrad taps and is what :class:`_FPNFn` saves in the merged map's place.  ``grad_dtype`` concerns the eight dgrad GEMMs of
:class:`_FPNFn`'s backward, 3x3s and laterals.  Laterals and merges stay fp32 in every forward.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib, ops
from ..config import DiTConfig
from .dit_backbone import DiTBackbone
from .grad_ops import (BF16_K, OperandCache, check_dtype, conv3x3_bwd, conv3x3_dgrad_bf16, conv3x3_fwd_bf16, dtype_setter, linear_bwd,
                       linear_dgrad_bf16)


class _Conv(nn.Sequential):
    """``Conv2dNormActivation(in, out, k, padding, norm_layer=None, activation_layer=None)``: a Sequential holding the
    convolution at index 0 - gives the parameters torchvision's key names (``...{i}.0.weight``)."""

    def __init__(self, cin: int, cout: int, k: int):
        super().__init__(nn.Conv2d(cin, cout, kernel_size=k, padding=k // 2))


class _FPNParams(nn.Module):
    def __init__(self, in_channels_list, out_channels: int):
        super().__init__()
        self.inner_blocks = nn.ModuleList([_Conv(c, out_channels, 1) for c in in_channels_list])
        self.layer_blocks = nn.ModuleList([_Conv(out_channels, out_channels, 3) for _ in in_channels_list])
        for m in self.modules():                     # torchvision's init: kaiming_uniform_(a=1), zero bias
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)


def _fpn_forward(bb_scales, gh: int, gw: int, toks, lat_w, lat_b, conv_w_ohwi, conv_b, keep_inner: bool):
    """The stage on fp32 contiguous token tensors [B, 1+P, C]; returns NHWC outputs (coarsest last) and, with ``keep_inner``, what the
    backward reads of the four merged maps.  A level whose ``conv_w_ohwi`` is a bf16 copy runs its 3x3 on the bf16 MFMA GEMM
    (``grad_ops.conv3x3_fwd_bf16``) and keeps the slack-padded bf16 copy of its map in the map's place; laterals, merges and the fp32
    NHWC results are what they are without it."""
    B, T, Cc = toks[0].shape
    lats = [ops.linear(toks[i].reshape(B * T, Cc), lat_w[i], lat_b[i]).view(B, T, -1) for i in range(4)]
    inner, outs, inners = None, [None] * 4, [None] * 4
    for i in (3, 2, 1, 0):                                            # coarsest first (top-down)
        inner = kept = ops.fpn_merge(lats[i], gh, gw, bb_scales[i], top=inner)
        if conv_w_ohwi[i].dtype == torch.bfloat16:
            rows, kept = conv3x3_fwd_bf16(inner, conv_w_ohwi[i], conv_b[i], _lib.EPI_F32, slack=keep_inner)
            outs[i] = rows.view(*inner.shape[:3], -1)
        else:
            outs[i] = ops.conv3x3_nhwc(inner, conv_w_ohwi[i], conv_b[i])
        if keep_inner:
            inners[i] = kept
    return outs, inners


class _FPNFn(torch.autograd.Function):
    """p2..p5 = FPN(taps) with gradients for the taps and for every FPN parameter.
    apply(stage, gh, gw, t0..t3, lw0, lb0, .. lw3, lb3, cw0, cb0, .. cw3, cb3) -> (p2, p3, p4, p5) as [B, 256, h, w] channels-last views.
    ``stage``: the :class:`DiTWithFPN` whose parameters these are.  The forward reads its ``train_dtype`` (``"bf16"``: a level the bf16
    GEMM takes runs on the cached :meth:`DiTWithFPN._ohwi_bf16`) and its ``grad_dtype``, which it keeps on ``ctx``: a setter called
    between forward and backward does not change that backward.  The backward takes its dgrad operands from the stage's cache."""

    @staticmethod
    def forward(ctx, stage, gh, gw, *args):
        toks = [_f32c(t.detach()) for t in args[0:4]]
        lw = [args[4 + 2 * i].detach() for i in range(4)]
        lb = [args[5 + 2 * i].detach() for i in range(4)]
        cw = [args[12 + 2 * i].detach() for i in range(4)]
        cb = [args[13 + 2 * i].detach() for i in range(4)]
        Ch, Cc = lw[0].shape[0], toks[0].shape[2]
        bf16 = check_dtype("train_dtype", stage.train_dtype) == "bf16"
        conv_w = [stage._ohwi_bf16(i) if bf16 and w.shape[1] % BF16_K == 0 else w.permute(0, 2, 3, 1).contiguous() for i, w in enumerate(cw)]
        outs, inners = _fpn_forward(stage.backbone.scales, gh, gw, toks, [w.reshape(Ch, Cc) for w in lw], lb, conv_w, cb, keep_inner=True)
        ctx.stage, ctx.grid, ctx.grad_dtype = stage, (gh, gw), check_dtype("grad_dtype", stage.grad_dtype)
        ctx.shapes = [tuple(o.shape) for o in outs]                   # of the merged maps too: the 3x3 keeps the channel count
        ctx.toks, ctx.inners, ctx.lw, ctx.cw = toks, inners, lw, cw
        return tuple(o.permute(0, 3, 1, 2) for o in outs)

    @staticmethod
    def backward(ctx, *dps):
        (gh, gw), scales, grad_dtype = ctx.grid, ctx.stage.backbone.scales, ctx.grad_dtype
        operand = lambda kind, i: partial(ctx.stage._dgrad_operands_bf16, kind, i)          # noqa: E731
        if ctx.inners is None:
            raise RuntimeError("DiTWithFPN: backward through the FPN a second time (its saved maps are freed after the first)")
        toks, inners, lw, cw = ctx.toks, ctx.inners, ctx.lw, ctx.cw
        ctx.inners = None
        B, T, Cc = toks[0].shape
        Ch = lw[0].shape[0]
        need = ctx.needs_input_grad[3:]                              # lines up with ``args``: t0..t3, (lw, lb) x 4, (cw, cb) x 4
        d_inner = [None] * 4
        g_cw, g_cb = [None] * 4, [None] * 4
        for i in range(4):                                            # finest first: the top-down adjoint flows fine -> coarse
            dp = dps[i]
            if dp is not None:
                dy = dp.permute(0, 2, 3, 1)
                dy = dy.float() if dy.dtype != torch.float32 else dy
                dy = dy.contiguous()                                  # NHWC [B, h, w, Ch]; a no-op for channels-last gradients
                d_inner[i], g_cw[i], g_cb[i] = conv3x3_bwd(dy, inners[i], cw[i], True, need[12 + 2 * i], need[13 + 2 * i], grad_dtype,
                                                           dgrad_w=operand("conv", i))
            else:
                d_inner[i] = torch.zeros(ctx.shapes[i], device=toks[0].device, dtype=torch.float32)
            if i > 0:
                ops.fpn_merge_bwd(d_inner[i - 1], gh, gw, scales[i - 1], d_top=d_inner[i], want_lat=False)
            inners[i] = None
        g_tok, g_lw, g_lb = [None] * 4, [None] * 4, [None] * 4
        for i in range(4):
            d_lat = ops.fpn_merge_bwd(d_inner[i], gh, gw, scales[i])                     # [B, T, Ch], CLS row zero
            d_inner[i] = None
            g_x, g_w, g_lb[i] = linear_bwd(d_lat.view(B * T, Ch), toks[i].view(B * T, Cc), lw[i].reshape(Ch, Cc), need[i],
                                           need[4 + 2 * i], need[5 + 2 * i], grad_dtype, dgrad_w=operand("lat", i))
            g_tok[i] = g_x.view(B, T, Cc) if need[i] else None
            g_lw[i] = g_w.view(Ch, Cc, 1, 1) if need[4 + 2 * i] else None
        grads = [None] * 3 + g_tok
        for i in range(4):
            grads += [g_lw[i], g_lb[i]]
        for i in range(4):
            grads += [g_cw[i], g_cb[i]]
        return tuple(grads)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = ops.widen_f16(t.contiguous()) if t.dtype == torch.float16 else t.float()
    return t.contiguous()


class DiTWithFPN(nn.Module):
    def __init__(self, pretrained: bool = False, config: Optional[DiTConfig] = None, checkpoint: Optional[str] = None,
                 compute_dtype: str = "f32", qat: bool = False, neck_dtype: str = "f32", grad_dtype: str = "f32", train_dtype: str = "f32"):
        super().__init__()
        self.neck_dtype = check_dtype("neck_dtype", neck_dtype)
        self.grad_dtype = check_dtype("grad_dtype", grad_dtype)
        self.train_dtype = check_dtype("train_dtype", train_dtype)
        self.backbone = DiTBackbone(pretrained=pretrained, config=config, checkpoint=checkpoint, compute_dtype=compute_dtype, qat=qat)
        self.fpn = _FPNParams([self.backbone.hidden_size] * 4, 256)
        self.out_channels = 256
        self._operand_cache = OperandCache()

    set_neck_dtype = dtype_setter("neck_dtype", """``"f32"`` or ``"bf16"``: how the four 3x3 output convolutions run from now on where no
        gradient is wanted, on the same weights.""")
    set_grad_dtype = dtype_setter("grad_dtype", """``"f32"`` or ``"bf16"``: the matrix pipe of the FPN's eight input-gradient GEMMs in the
        backward from now on (four 3x3 output convolutions, four laterals).  The encoder below has its own ``compute_dtype``.""")
    set_train_dtype = dtype_setter("train_dtype", """``"f32"`` or ``"bf16"``: how the four 3x3 output convolutions run from now on where a
        gradient IS wanted (:class:`_FPNFn`'s forward) - ``"bf16"``: as ``neck_dtype="bf16"`` runs them where none is.""")

    def _ohwi(self, i: int) -> torch.Tensor:
        """3x3 weight of level i as [Cout, 3, 3, Cin] (GEMM operand layout), re-laid when the parameter changes."""
        w = self.fpn.layer_blocks[i][0].weight
        return self._operand_cache.get(("ohwi", i), (w,), lambda: w.detach().permute(0, 2, 3, 1).contiguous())

    def _ohwi_bf16(self, i: int) -> torch.Tensor:
        """The bf16 copy of :meth:`_ohwi` (``neck_dtype`` / ``train_dtype="bf16"``), cached beside it under the same key."""
        return self._operand_cache.get(("ohwi_bf16", i), (self.fpn.layer_blocks[i][0].weight,), lambda: ops.cast_bf16(self._ohwi(i)))

    def _dgrad_operands_bf16(self, kind: str, i: int) -> torch.Tensor:
        """The weight operand of a dgrad GEMM under ``grad_dtype="bf16"``, re-made when the parameter changes: ``"conv"`` - level i's
        3x3 weight flipped, in/out-swapped, bf16; ``"lat"`` - its lateral weight transposed [C, 256], bf16."""
        w = (self.fpn.layer_blocks if kind == "conv" else self.fpn.inner_blocks)[i][0].weight
        return self._operand_cache.get(("dgrad", kind, i), (w,), lambda: conv3x3_dgrad_bf16(w) if kind == "conv"
                                       else linear_dgrad_bf16(w.reshape(w.shape[0], w.shape[1])))

    def forward(self, x: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        bb = self.backbone
        B, _, H, W = x.shape
        p = bb.dit.config.patch_size
        gh, gw = H // p, W // p
        hs = bb.dit(x, taps=bb.layer_idxs).hidden_states
        toks = [hs[idx] for idx in bb.layer_idxs]
        lat = [self.fpn.inner_blocks[i][0] for i in range(4)]
        conv = [self.fpn.layer_blocks[i][0] for i in range(4)]
        wants_grad = torch.is_grad_enabled() and (any(t.requires_grad for t in toks)
                                                  or any(q.requires_grad for q in self.fpn.parameters()))
        if wants_grad:
            # one differentiable stage: gradients for the taps (hence the encoder) and for every FPN parameter
            args = list(toks)
            for m in lat:
                args += [m.weight, m.bias]
            for m in conv:
                args += [m.weight, m.bias]
            results = list(_FPNFn.apply(self, gh, gw, *args))
        else:
            Cc = bb.hidden_size
            bf16_conv = self.neck_dtype == "bf16"
            outs, _ = _fpn_forward(bb.scales, gh, gw, [_f32c(t.detach()) for t in toks],
                                   [m.weight.detach().reshape(256, Cc) for m in lat], [m.bias.detach() for m in lat],
                                   [self._ohwi_bf16(i) if bf16_conv else self._ohwi(i) for i in range(4)],
                                   [m.bias.detach() for m in conv], keep_inner=False)
            results = [o.permute(0, 3, 1, 2) for o in outs]          # [B, 256, h, w], channels-last memory
        feats = OrderedDict((f"p{i + 2}", r) for i, r in enumerate(results))
        feats["pool"] = results[3][:, :, ::2, ::2]                    # LastLevelMaxPool: max_pool2d(kernel 1, stride 2)
        if x.dtype == torch.float16 and not wants_grad:
            feats = OrderedDict((k, ops.narrow_f16(v.contiguous())) for k, v in feats.items())
        return feats
