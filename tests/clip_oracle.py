"""Float64 restatement of global-norm clipping and the grouped AdamW of csrc/optim_multi.hip (``ldit_grads_check_norm_multi_f32``,
``ldit_clip_finish``, ``ldit_adamw_groups_multi_f32``) on top of tests/optim_oracle.py: ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.AdamW`` with parameter groups.  Plain Python / numpy, no torch."""
import math

import numpy as np

from tests import optim_oracle as oo

FIELDS = ("max_norm", "total_norm", "clip_coef", "clipped_steps")


def new_clip(max_norm=float("inf")):
    return {"max_norm": float(max_norm), "total_norm": 0.0, "clip_coef": 0.0, "clipped_steps": 0}


def sum_of_squares(grads):
    """Over every element of every gradient, in float64 (math.fsum over the per-tensor sums: no order to speak of)."""
    return math.fsum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads)


def clip_coef(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1)"""
    return min(1.0, max_norm / (total_norm + 1e-6))


def finish(state, clip, grads):
    """After ``optim_oracle.advance``: the norm of the UNSCALED gradients and, unless the step is skipped, the coefficient and the
    count.  ``grads`` are the loss-scaled gradients the check saw."""
    c = dict(clip)
    with np.errstate(all="ignore"):
        c["total_norm"] = math.sqrt(sum_of_squares(grads)) * state["inv_scale_used"] if all(np.isfinite(g).all() for g in grads) else float("nan")
    if not state["skip"]:
        c["clip_coef"] = clip_coef(c["total_norm"], c["max_norm"])
        c["clipped_steps"] += int(c["clip_coef"] < 1.0)
    return c


def adamw_groups(p, g, m, v, state, lr_scale=1.0, weight_decay=0.0, coef=1.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """One update of one tensor with its group's learning-rate scale and decay on the gradient ``g * coef * inv_scale_used``."""
    s = dict(state)
    s["lr"] = state["lr"] * lr_scale
    return oo.adamw(p, g, m, v, s, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_mul=coef)
