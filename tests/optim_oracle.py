"""Float64 restatement of the detector's optimizer step (csrc/optim_multi.hip): the loss-scale / step-count state machine of
``ldit_opt_advance`` (``torch.amp.GradScaler.step`` + ``.update`` and the optimizer's step count) and the AdamW update of
``ldit_adamw_multi_f32`` (``torch.optim.AdamW``: decoupled weight decay, bias corrections).  Plain Python / numpy, no torch: the tests
compare it with ``torch.amp.GradScaler`` / ``torch.optim.AdamW`` on one side and with the kernels on the other."""
import math

import numpy as np

FIELDS = ("found_inf", "skip", "step", "growth_tracker", "skipped_steps", "scale", "inv_scale_used", "lr", "bc1", "bc2_sqrt")


def new_state(scale=65536.0, lr=1e-4):
    return {"found_inf": 0, "skip": 0, "step": 0, "growth_tracker": 0, "skipped_steps": 0, "scale": float(scale),
            "inv_scale_used": 1.0 / float(scale), "lr": float(lr), "bc1": 1.0, "bc2_sqrt": 1.0}


def check(state, grads):
    """found_inf |= some element of some gradient is NaN or infinite"""
    if any(g.size and not np.isfinite(g).all() for g in grads):
        state["found_inf"] = 1
    return state


def advance(state, beta1=0.9, beta2=0.999, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    s = dict(state)
    s["skip"] = int(s["found_inf"] != 0)
    s["inv_scale_used"] = 1.0 / s["scale"]
    s["found_inf"] = 0
    if not s["skip"]:
        s["step"] += 1
        s["bc1"] = 1.0 - beta1 ** s["step"]
        s["bc2_sqrt"] = math.sqrt(1.0 - beta2 ** s["step"])
        s["growth_tracker"] += 1
        if s["growth_tracker"] == growth_interval:
            s["scale"] *= growth_factor
            s["growth_tracker"] = 0
    else:
        s["scale"] *= backoff_factor
        s["growth_tracker"] = 0
        s["skipped_steps"] += 1
    return s


def adamw(p, g, m, v, state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_mul=1.0):
    """One update of (p, m, v) in float64 for the gradient ``g * grad_mul * inv_scale_used``; unchanged copies when ``skip`` is set."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if state["skip"]:
        return p.copy(), m.copy(), v.copy()
    gr = g * (grad_mul * state["inv_scale_used"])
    lr = state["lr"]
    m = beta1 * m + (1.0 - beta1) * gr
    v = beta2 * v + (1.0 - beta2) * gr * gr
    p = p * (1.0 - lr * weight_decay) - (lr / state["bc1"]) * (m / (np.sqrt(v) / state["bc2_sqrt"] + eps))
    return p, m, v
