"""The contract of ``grad_dtype="bf16"`` restated in float64 on the CPU: the input gradient of a linear layer and
of a 3x3 / padding 1 convolution is the exact product of ``dy`` and the weight AFTER both were rounded to bf16 (torch's CPU cast: to
nearest even), and a ReLU between two layers is a selection (``torch.where``), never a multiplication.  The library differs from
this only by its fp32 accumulation.  ``*_exact``: the same gradients without the rounding - plain float64 autograd."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F


def bf16(t: torch.Tensor) -> torch.Tensor:
    """The float64 value of every element after rounding to bf16 (through fp32, as the operands reach the kernels)."""
    return t.detach().float().to(torch.bfloat16).double()


def relu_select(dy: torch.Tensor, act: Optional[torch.Tensor]) -> torch.Tensor:
    """``dy`` where the activation is positive, else 0: a non-finite ``dy`` under a masked position gives 0; +-0 and NaN mask."""
    return dy if act is None else torch.where(act > 0, dy, torch.zeros_like(dy))


def linear_gx(dy: torch.Tensor, weight: torch.Tensor, act: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g_x [M, K] of ``y = x @ weight.T``: ``bf16(dy) @ bf16(weight)``, the products and sums in float64."""
    return bf16(relu_select(dy, act)) @ bf16(weight)


def linear_gx_exact(dy: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    x = torch.zeros(dy.shape[0], weight.shape[1], dtype=torch.float64, requires_grad=True)
    (F.linear(x, weight.double()) * dy.double()).sum().backward()
    return x.grad


def _conv_gx(dy_nhwc: torch.Tensor, weight_oihw: torch.Tensor) -> torch.Tensor:
    x = torch.zeros(dy_nhwc.shape[0], weight_oihw.shape[1], dy_nhwc.shape[1], dy_nhwc.shape[2], dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, weight_oihw, padding=1) * dy_nhwc.permute(0, 3, 1, 2)).sum().backward()
    return x.grad.permute(0, 2, 3, 1).contiguous()


def conv3x3_gx(dy_nhwc: torch.Tensor, weight_oihw: torch.Tensor, act: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g_x NHWC [B, h, w, Cin] of ``y = conv3x3(x, weight, padding=1)`` for ``dy`` NHWC [B, h, w, Cout]: float64 autograd on the
    bf16-rounded ``dy`` and weight (the convolution is linear in each, so this IS the product of the rounded operands)."""
    return _conv_gx(bf16(relu_select(dy_nhwc, act)), bf16(weight_oihw))


def conv3x3_gx_exact(dy_nhwc: torch.Tensor, weight_oihw: torch.Tensor) -> torch.Tensor:
    return _conv_gx(dy_nhwc.double(), weight_oihw.double())
