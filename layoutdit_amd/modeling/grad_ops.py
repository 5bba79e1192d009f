"""What the detector's differentiable stages (``dit_fpn.py``, ``rpn.py``, ``roi_heads.py``) share: the backward of a 3x3 convolution
and of a linear layer on the library's kernels, two layers stacked into one GEMM operand, and the cache of a re-laid operand.  Each
stage keeps ONE ``autograd.Function`` (the order in which autograd sums a shared parameter's gradients is part of the bits)."""
from __future__ import annotations

import torch

from .. import ops


def flip_ihwo(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 weight -> the operand of its dgrad convolution: [Cin, 3, 3, Cout] with the taps flipped."""
    return w.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous()


def conv3x3_bwd(dy_nhwc: torch.Tensor, x_nhwc: torch.Tensor, weight_oihw: torch.Tensor, need_x: bool, need_w: bool, need_b: bool):
    """Gradients of ``y = conv3x3(x, weight, padding=1) + bias`` on NHWC fp32 maps: ``(g_x NHWC, g_w OIHW, g_b)``, ``None`` and no
    launch for one that is not needed.  ``g_x``: the forward's implicit-im2col fp32 GEMM on the flipped weight.  ``g_w``: one bf16
    MFMA GEMM per tap (fp32 accumulation, bf16 operand rounding) on the zero-padded maps as reduction-major operands
    [B (h+2)(w+2), C] - a tap is a constant row offset into the padded input, kept inside the buffer by ``slack`` zero rows."""
    B, h, w, Cout = dy_nhwc.shape
    g_x = ops.conv3x3_nhwc(dy_nhwc, flip_ihwo(weight_oihw)) if need_x else None
    g_b = ops.colsum(dy_nhwc.view(B * h * w, Cout)) if need_b else None
    g_w = None
    if need_w:
        slack = w + 3
        dy_p = ops.pad_nhwc_bf16(dy_nhwc)
        x_p = ops.pad_nhwc_bf16(x_nhwc, slack_rows=slack)
        K = dy_p.shape[0]
        taps = []
        for ky in range(3):
            for kx in range(3):
                shift = (ky - 1) * (w + 2) + (kx - 1)
                taps.append(ops.wgrad_bf16(dy_p, x_p, K, w_row_offset=slack + shift))      # [co, ci]
        g_w = torch.stack(taps, dim=2).view(Cout, x_nhwc.shape[3], 3, 3)                    # [co, ci, ky, kx] (layout plumbing)
    return g_x, g_w, g_b


def linear_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, need_x: bool, need_w: bool, need_b: bool):
    """Gradients of ``y = x @ weight.T + bias``: ``(g_x, g_w, g_b)``, ``None`` and no launch for one that is not needed.  ``g_x``:
    ``ldit_linear_f32`` on the transposed weight; ``g_w``: a bf16 MFMA GEMM on reduction-major operands (fp32 accumulation, bf16
    operand rounding); ``g_b``: ``ldit_colsum_f32``.  ``dy`` [M, N], N % 32 == 0 (the K of the fp32 GEMM), ``x`` [M, K], ``weight``
    [<= N, K]: where ``dy`` ends in zero padding columns that the weight has no rows for, the transposed weight is zero-extended
    to N columns, and ``g_w`` and ``g_b`` have N rows."""
    g_x = None
    if need_x:
        if weight.shape[0] == dy.shape[1]:
            wt = weight.t().contiguous()
        else:
            wt = torch.zeros((weight.shape[1], dy.shape[1]), device=dy.device, dtype=torch.float32)
            wt[:, :weight.shape[0]] = weight.t()
        g_x = ops.linear(dy, wt)
    g_w = ops.wgrad_bf16(ops.cast_bf16(dy), ops.cast_bf16(x), dy.shape[0]) if need_w else None
    g_b = ops.colsum(dy) if need_b else None
    return g_x, g_w, g_b


def stack_rows(weights, biases, multiple: int):
    """Layers that read the same input as ONE GEMM operand ``(w, b)``: their [n_i, K] weights one below the other in a contiguous
    fp32 matrix whose row count is rounded up to ``multiple``, the biases alike; the padding is zero."""
    rows = (sum(w.shape[0] for w in weights) + multiple - 1) // multiple * multiple
    w = torch.zeros((rows, weights[0].shape[1]), device=weights[0].device, dtype=torch.float32)
    b = torch.zeros((rows,), device=weights[0].device, dtype=torch.float32)
    r = 0
    for wi, bi in zip(weights, biases):
        w[r:r + wi.shape[0]], b[r:r + wi.shape[0]] = wi.detach(), bi.detach()
        r += wi.shape[0]
    return w, b


NECK_DTYPES = ("f32", "bf16")


def check_neck_dtype(neck_dtype: str) -> str:
    """The option of the FPN, the RPN head and the detector that holds them: how their 3x3 convolutions run where no gradient is
    wanted."""
    if neck_dtype not in NECK_DTYPES:
        raise ValueError(f"neck_dtype {neck_dtype!r}: the FPN and the RPN head are built for {' and '.join(repr(d) for d in NECK_DTYPES)}")
    return neck_dtype


def conv3x3_bf16(x_nhwc: torch.Tensor, weight_ohwi_bf16: torch.Tensor, bias, epilogue: int) -> torch.Tensor:
    """The eval-mode bf16 3x3 convolution of an fp32 NHWC map: one launch for its zero-padded bf16 copy, one for the implicit-im2col
    bf16 MFMA GEMM on it.  Returns the pixel rows ``[B h w, Cout]`` (fp32 for ``EPI_F32``, else bf16)."""
    B, h, w, _ = x_nhwc.shape
    return ops.conv3x3_nhwc_bf16(ops.pad_nhwc_bf16(x_nhwc), B, h, w, weight_ohwi_bf16, bias, epilogue)


def param_key(*params: torch.Tensor) -> tuple:
    """Changes when one of the parameters is replaced, moved or written in place (autograd's version counter)."""
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in params)


class ParamCache:
    """One value derived from parameters under one key (:func:`param_key` of them and whatever else it depends on), rebuilt when
    the key changes.  ``clear()`` after an update that moves no version counter."""

    def __init__(self):
        self.key = self.value = None

    def get(self, key, build):
        if self.value is None or self.key != key:
            self.key, self.value = key, build()
        return self.value

    def clear(self) -> None:
        self.key = self.value = None
