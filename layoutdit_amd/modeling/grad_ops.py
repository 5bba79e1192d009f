"""What the detector's differentiable stages (``dit_fpn.py``, ``rpn.py``, ``roi_heads.py``) share: the backward of a 3x3 convolution
and of a linear layer on the library's kernels, the bf16 3x3 forward, two layers stacked into one GEMM operand, and the cache of
re-laid operands.  Each stage keeps ONE ``autograd.Function`` (the order in which autograd sums a shared parameter's gradients is
part of the bits).

The four dtype options of the stages and of the detector that holds them, each ``"f32"`` (the default) or ``"bf16"``
(:func:`check_dtype`), each a constructor argument, a property and a ``set_*`` method returning ``self``.  None touches a parameter
or the ``state_dict``; a bf16 copy of a weight lives in the module's :class:`OperandCache` beside its fp32 re-layout.

* ``neck_dtype`` (FPN, RPN head) and ``head_dtype`` (box head) - the path that wants NO gradient: the 3x3 convolutions
  (:func:`conv3x3_fwd_bf16`) and the linear layers on the bf16 MFMA GEMM, fp32 accumulation, bf16 operand rounding, fp32 results.
* ``train_dtype`` - the forward that WANTS a gradient: the launches of ``neck_dtype`` / ``head_dtype="bf16"`` on the same cached
  operands (bit-equal results), saving the bf16 tensors the backward reads again as they stand.  Eval mode and
  ``no_grad`` never read it.
* ``grad_dtype`` - the backward alone: the input-gradient (dgrad) GEMMs of :func:`conv3x3_bwd` / :func:`linear_bwd` on the bf16
  copy of the incoming gradient that the wgrad reads.  No forward reads it.

A stage's autograd node takes the stage module itself, reads ``train_dtype`` and ``grad_dtype`` in its forward and keeps them on
``ctx`` - a setter called between forward and backward does not change that backward - and takes the dgrad operands from the
module's cache.  A reduction length that is no multiple of :data:`BF16_K` keeps every fp32 launch under any option."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib, ops


def flip_ihwo(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 weight -> the operand of its dgrad convolution: [Cin, 3, 3, Cout] with the taps flipped."""
    return w.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous()


DTYPES = ("f32", "bf16")
BF16_K = 64                    # the k-tile of the bf16 GEMM: a reduction length it takes is a multiple of it


def check_dtype(option: str, value: str) -> str:
    """``value`` if it is one ``option`` (``neck_dtype``, ``head_dtype``, ``grad_dtype``, ``train_dtype``) can take."""
    if value not in DTYPES:
        raise ValueError(f"{option} {value!r}: the detector's stages are built for {' and '.join(repr(d) for d in DTYPES)}")
    return value


def dtype_setter(option: str, doc: str):
    """The ``set_<option>`` method of a stage that keeps ``option`` as a plain attribute: validates, assigns, returns ``self``."""
    def setter(self, value: str):
        setattr(self, option, check_dtype(option, value))
        return self
    setter.__name__, setter.__doc__ = f"set_{option}", doc
    return setter


def padded_middle(x_p: torch.Tensor, B: int, h: int, w: int) -> torch.Tensor:
    """The padded map ``[B (h+2) (w+2), C]`` inside ``ops.pad_nhwc_bf16(x, slack_rows=w + 3)`` - what ``ops.conv3x3_nhwc_bf16`` reads;
    the whole buffer is what the nine wgrad taps of :func:`conv3x3_bwd` read."""
    return x_p[w + 3:w + 3 + B * (h + 2) * (w + 2)]


def conv3x3_dgrad_bf16(weight_oihw: torch.Tensor) -> torch.Tensor:
    """The bf16 operand of a 3x3 convolution's dgrad under ``grad_dtype="bf16"``: :func:`flip_ihwo` rounded to bf16."""
    return ops.cast_bf16(flip_ihwo(weight_oihw))


def linear_dgrad_bf16(weight: torch.Tensor) -> torch.Tensor:
    """The bf16 operand of a linear layer's dgrad under ``grad_dtype="bf16"``: the transposed weight [K, N] rounded to bf16."""
    return ops.cast_bf16(weight.detach().t().contiguous())


def conv3x3_bwd(dy_nhwc: torch.Tensor, x_nhwc: torch.Tensor, weight_oihw: torch.Tensor, need_x: bool, need_w: bool, need_b: bool,
                grad_dtype: str = "f32", act: Optional[torch.Tensor] = None, dgrad_w=None):
    """Gradients of ``y = conv3x3(x, weight, padding=1) + bias`` on NHWC fp32 maps: ``(g_x NHWC, g_w OIHW, g_b)``, ``None`` and no
    launch for one that is not needed.  ``g_x``: the forward's implicit-im2col fp32 GEMM on the flipped weight.  ``g_w``: one bf16
    MFMA GEMM per tap (fp32 accumulation, bf16 operand rounding) on the zero-padded maps as reduction-major operands
    [B (h+2)(w+2), C] - a tap is a constant row offset into the padded input, kept inside the buffer by ``slack`` zero rows.

    ``act`` (same shape as ``dy``): ``dy`` is first masked by the ReLU whose output ``act`` is.  The fused launch of ``"bf16"``
    selects, ``where(act > 0, dy, 0)``; the fp32 GEMM's arm multiplies, ``dy * (act > 0)`` - what the default configuration has
    always done: equal for a finite ``dy`` but for the sign of a zero, and a non-finite ``dy`` at a masked position gives NaN there.

    ``grad_dtype="bf16"`` with ``Cout % 64 == 0``: ONE launch (``ldit_relu_bwd_pad_nhwc_bf16``) masks ``dy``, writes its zero-padded
    bf16 copy and sums ``g_b``; that copy is the operand of the wgrad taps - ``g_w`` and ``g_b`` have the bits of the ``"f32"``
    setting - and of ``g_x = ldit_conv3x3_nhwc_bf16(copy, dgrad_w)``: bf16 operand rounding, fp32 accumulation, fp32 result.
    ``dgrad_w``: a callable returning the cached :func:`conv3x3_dgrad_bf16` of the weight (made here without one).  A ``Cout`` that
    is no multiple of 64 - the bf16 GEMM's k-tile - stays on the fp32 GEMM: every launch of the ``"f32"`` setting.

    What a forward under ``train_dtype="bf16"`` saved is read as it stands: a bf16 ``x_nhwc`` is the slack-padded copy
    ``ops.pad_nhwc_bf16(x, slack_rows=w + 3)`` the forward convolved (no pad launch here), a bf16 ``act`` is the mask without an fp32
    copy of it.  Every gradient has the bits of the call on their fp32 widenings."""
    B, h, w, Cout = dy_nhwc.shape
    if act is not None:
        act = act.view(dy_nhwc.shape)
    bf16 = check_dtype("grad_dtype", grad_dtype) == "bf16" and Cout % BF16_K == 0
    if bf16:
        dy_p, g_b = ops.relu_bwd_pad_nhwc_bf16(dy_nhwc, act, want_colsum=need_b)
        g_x = None
        if need_x:
            w16 = dgrad_w() if dgrad_w is not None else conv3x3_dgrad_bf16(weight_oihw)
            g_x = ops.conv3x3_nhwc_bf16(dy_p, B, h, w, w16, None, _lib.EPI_F32).view(B, h, w, -1)
    else:
        if act is not None:
            dy_nhwc = dy_nhwc * (act > 0)
        g_x = ops.conv3x3_nhwc(dy_nhwc, flip_ihwo(weight_oihw)) if need_x else None
        g_b = ops.colsum(dy_nhwc.view(B * h * w, Cout)) if need_b else None
    g_w = None
    if need_w:
        slack = w + 3
        if not bf16:
            dy_p = ops.pad_nhwc_bf16(dy_nhwc)
        x_p = x_nhwc if x_nhwc.dtype == torch.bfloat16 else ops.pad_nhwc_bf16(x_nhwc, slack_rows=slack)
        K = dy_p.shape[0]
        if x_p.dim() != 2 or x_p.shape[0] != K + 2 * slack:
            raise ValueError(f"conv3x3_bwd: a bf16 x {tuple(x_p.shape)} is not the padded copy [{K} + 2 * {slack}, Cin] of the convolution's input")
        taps = []
        for ky in range(3):
            for kx in range(3):
                shift = (ky - 1) * (w + 2) + (kx - 1)
                taps.append(ops.wgrad_bf16(dy_p, x_p, K, w_row_offset=slack + shift))      # [co, ci]
        g_w = torch.stack(taps, dim=2).view(Cout, x_p.shape[1], 3, 3)                        # [co, ci, ky, kx] (layout plumbing)
    return g_x, g_w, g_b


def linear_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, need_x: bool, need_w: bool, need_b: bool,
               grad_dtype: str = "f32", act: Optional[torch.Tensor] = None, dgrad_w=None):
    """Gradients of ``y = x @ weight.T + bias``: ``(g_x, g_w, g_b)``, ``None`` and no launch for one that is not needed.  ``g_x``:
    ``ldit_linear_f32`` on the transposed weight; ``g_w``: a bf16 MFMA GEMM on reduction-major operands (fp32 accumulation, bf16
    operand rounding); ``g_b``: ``ldit_colsum_f32``.  ``dy`` [M, N], N % 32 == 0 (the K of the fp32 GEMM), ``x`` [M, K], ``weight``
    [<= N, K]: where ``dy`` ends in zero padding columns that the weight has no rows for, the transposed weight is zero-extended
    to N columns, and ``g_w`` and ``g_b`` have N rows.

    ``act`` (same shape as ``dy``): ``dy`` is first masked by the ReLU whose output ``act`` is.  The fused launch of ``"bf16"``
    selects, ``where(act > 0, dy, 0)``; the fp32 GEMM's arm multiplies, ``dy * (act > 0)`` - what the default configuration has
    always done: equal for a finite ``dy`` but for the sign of a zero, and a non-finite ``dy`` at a masked position gives NaN there.

    ``grad_dtype="bf16"`` with ``N % 64 == 0`` and a weight of N rows: ONE launch (``ldit_relu_bwd_bf16``) masks ``dy``, writes its
    bf16 copy and sums ``g_b``; that copy is the operand of the wgrad - ``g_w`` and ``g_b`` have the bits of the ``"f32"`` setting -
    and of ``g_x = ldit_linear_bf16_ex(copy, dgrad_w)`` with ``LDIT_EPI_F32``, any M: bf16 operand rounding, fp32 accumulation, fp32
    result.  ``dgrad_w``: a callable returning the cached :func:`linear_dgrad_bf16` of the weight (made here without one).  A
    reduction length N that is no multiple of 64 - the bf16 GEMM's k-tile; the 32 padded columns of the box predictor and of the
    RPN head's 1x1 pair, a few GFLOP - stays on the fp32 GEMM: every launch of the ``"f32"`` setting.

    A bf16 ``x`` (the layer's input as a forward under ``train_dtype="bf16"`` saved it) is the wgrad's operand as it stands - no cast
    launch - and a bf16 ``act`` the mask without an fp32 copy of it: every gradient has the bits of the call on their fp32 widenings."""
    x16 = (lambda: x) if x.dtype == torch.bfloat16 else (lambda: ops.cast_bf16(x))
    if check_dtype("grad_dtype", grad_dtype) == "bf16" and dy.shape[1] % BF16_K == 0 and weight.shape[0] == dy.shape[1]:
        dy16, g_b = ops.relu_bwd_bf16(dy, act, want_colsum=need_b)
        g_x = None
        if need_x:
            g_x = ops.linear_bf16(dy16, dgrad_w() if dgrad_w is not None else linear_dgrad_bf16(weight), None, _lib.EPI_F32)
        g_w = ops.wgrad_bf16(dy16, x16(), dy.shape[0]) if need_w else None
        return g_x, g_w, g_b
    if act is not None:
        dy = dy * (act > 0)
    g_x = None
    if need_x:
        if weight.shape[0] == dy.shape[1]:
            wt = weight.t().contiguous()
        else:
            wt = torch.zeros((weight.shape[1], dy.shape[1]), device=dy.device, dtype=torch.float32)
            wt[:, :weight.shape[0]] = weight.t()
        g_x = ops.linear(dy, wt)
    g_w = ops.wgrad_bf16(ops.cast_bf16(dy), x16(), dy.shape[0]) if need_w else None
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


def conv3x3_fwd_bf16(x_nhwc: torch.Tensor, weight_ohwi_bf16: torch.Tensor, bias, epilogue: int, slack: bool = False):
    """The bf16 3x3 convolution of an fp32 NHWC map: one launch for its zero-padded bf16 copy, one for the implicit-im2col bf16 MFMA
    GEMM on it.  Returns the pixel rows ``[B h w, Cout]`` (fp32 for ``EPI_F32``, else bf16) and the copy; with ``slack`` the copy
    carries the ``w + 3`` zero rows at either end that the wgrad taps of :func:`conv3x3_bwd` want - what a training forward saves."""
    B, h, w, _ = x_nhwc.shape
    x_p = ops.pad_nhwc_bf16(x_nhwc, slack_rows=w + 3 if slack else 0)
    rows = ops.conv3x3_nhwc_bf16(padded_middle(x_p, B, h, w) if slack else x_p, B, h, w, weight_ohwi_bf16, bias, epilogue)
    return rows, x_p


def pad_grad_row(blocks, M: int, device) -> torch.Tensor:
    """Column blocks ``(width, gradient or None)`` side by side as fp32 ``[M, K]``, K their width rounded up to 32 - the K the fp32
    dgrad GEMM wants, a multiple of 8 for the bf16 wgrad; a missing block and the padding are zero."""
    K = (sum(n for n, _ in blocks) + 31) // 32 * 32
    dy = torch.zeros((M, K), device=device, dtype=torch.float32)
    col = 0
    for n, d in blocks:
        if d is not None:
            dy[:, col:col + n] = d.reshape(M, n)
        col += n
    return dy


def param_key(*params: torch.Tensor) -> tuple:
    """Changes when one of the parameters is replaced, moved or written in place (autograd's version counter)."""
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in params)


class ParamCache:
    """One value derived from parameters under one key (:func:`param_key` of them and whatever else it depends on), rebuilt when
    the key changes: one entry of an :class:`OperandCache`."""

    def __init__(self):
        self.key = self.value = None

    def get(self, key, build):
        if self.value is None or self.key != key:
            self.key, self.value = key, build()
        return self.value

    def clear(self) -> None:
        self.key = self.value = None


class OperandCache:
    """A module's values derived from its parameters, by name: each entry is a :class:`ParamCache` keyed on :func:`param_key` of its
    parameters and whatever else it depends on, and is rebuilt alone when that key changes.  ``clear()`` after an update that moves
    no version counter."""

    def __init__(self):
        self._entries = {}

    def get(self, name, params, build, *extra):
        return self._entries.setdefault(name, ParamCache()).get((param_key(*params), *extra), build)

    def filled(self, name=None) -> bool:
        """Whether the entry ``name`` - without one: any entry - holds a value."""
        return any(e.value is not None for n, e in self._entries.items() if name is None or n == name)

    def clear(self) -> None:
        self._entries.clear()
