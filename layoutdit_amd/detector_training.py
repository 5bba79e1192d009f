"""The detector's train step: the other half of the reference's iteration (ref ``src/layoutdit/training/trainer.py:164-183``) -

    scaler.scale(sum(loss_dict.values())).backward(); scaler.step(optimizer); scaler.update()        # AdamW(model.parameters())
    scheduler.step()                                                                                 # StepLR, once per epoch

- on ``LayoutDetectionModel.losses`` and the multi-tensor optimizer kernels of ``csrc/optim_multi.hip``.  Every parameter of the
detector that received a gradient - the box head, the RPN head, the FPN and the encoder - is updated by three kernels per 64 tensors
(non-finite check, state machine, AdamW), and the skip decision, the step count, the bias corrections, the loss scale and the learning
rate live in one 40-byte device block (``ldit_opt_state``): between ``backward()`` and the updated weights nothing is read on the host.
``torch.optim.AdamW`` + ``torch.amp.GradScaler`` on the same model launch a group of kernels per parameter tensor and read
``found_inf`` back once per iteration.

One parameter group, no gradient clipping, no data parallelism.  PyTorch is plumbing: it owns the memory, the
stream and autograd's graph; the arithmetic of the update is the library's.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, ops

_FIELD = {n: i for i, n in enumerate(_lib.OPT_STATE_FIELDS)}
_INT_FIELDS = ("found_inf", "skip", "step", "growth_tracker", "skipped_steps")
_FLOAT_FIELDS = ("scale", "inv_scale_used", "lr", "bc1", "bc2_sqrt")


class DetectorTrainStep:
    """``step(images, targets)`` = the reference's iteration on a :class:`LayoutDetectionModel` in train mode; ``apply()`` = its
    optimizer half alone, on the gradients the parameters currently hold.

    ``loss_scaling=False`` keeps the scale at 1 (the loss is not multiplied); a step whose gradients hold a NaN or an infinity is
    still skipped and counted.  ``step_size=None`` keeps the learning rate constant; otherwise :meth:`epoch_end` is ``StepLR``."""

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 0.0, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 step_size: Optional[int] = None, gamma: float = 0.1, init_scale: float = 65536.0, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000, loss_scaling: bool = True):
        from .modeling.detector import LayoutDetectionModel
        if not isinstance(model, LayoutDetectionModel):
            raise TypeError("DetectorTrainStep: expected a LayoutDetectionModel (the encoder alone trains with TrainStep)")
        self.model = model
        self.encoder = model.model.backbone.backbone.dit
        if self.encoder.compute_dtype in ("fp8", "mxfp8"):
            raise NotImplementedError(f"DetectorTrainStep: the {self.encoder.compute_dtype} encoder is not covered - 'fp8' and 'mxfp8' are inference "
                                      "builds, and the quantisation-aware 'mxfp8' build (qat=True) needs the update that re-quantises its MX "
                                      "operands, which is TrainStep's (ldit_adamw_step_mxfp8); build the detector with compute_dtype 'f32' or 'bf16'")
        self._require_train_mode()
        params = list(model.named_parameters())
        if not params:
            raise ValueError("DetectorTrainStep: the model has no parameters")
        self.device = params[0][1].device
        if self.device.type != "cuda" or any(p.device != self.device for _, p in params):
            raise ValueError("DetectorTrainStep: every parameter must live on one GPU (libldit_hip has no CPU path) - call .to(device) first")
        if step_size is not None and int(step_size) < 1:
            raise ValueError("DetectorTrainStep: step_size must be a positive number of epochs")
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.step_size, self.gamma = None if step_size is None else int(step_size), float(gamma)
        self.loss_scaling = bool(loss_scaling)
        self.growth_factor, self.backoff_factor = (float(growth_factor), float(backoff_factor)) if self.loss_scaling else (1.0, 1.0)
        self.growth_interval = int(growth_interval)
        self.epochs = 0
        self._names = {id(p): n for n, p in params}
        self._state = ops.new_opt_state(self.device, float(init_scale) if self.loss_scaling else 1.0, self.lr)
        self._state_f = self._state.view(torch.float32)
        self._mom: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}        # parameter name -> (exp_avg, exp_avg_sq)
        self._pending: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}    # loaded moments of parameters not seen yet
        self._enc = None                                                     # (FlatState, flat exp_avg, flat exp_avg_sq)

    # ---- the iteration ----------------------------------------------------------------------------------------------------------------
    def step(self, images: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]],
             generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """One iteration: gradients cleared, ``model.losses``, backward on the scaled sum, check / advance / update.  Returns the four
        unscaled, detached losses.  From the backward on there is no host synchronisation; the loss scale enters the graph as a device
        tensor.  (The input transform's host bookkeeping is ``model.losses``'s own.)"""
        self._require_train_mode()
        for p in self.model.parameters():
            p.grad = None
        losses = self.model.losses(images, targets, generator=generator)
        total = sum(losses.values())
        if self.loss_scaling:
            total = total * self._state_f[_FIELD["scale"]]
        total.backward()
        self.apply()
        return {k: v.detach() for k, v in losses.items()}

    @torch.no_grad()
    def apply(self) -> None:
        """The optimizer half alone, on the gradients the parameters hold now (made with the current loss scale): non-finite check,
        state machine, AdamW - or nothing, if the check fired.  No synchronisation; capturable once every moment exists (after one
        eager call).  A replayed graph moves the weights behind this object's back: call :meth:`invalidate_caches` after replays."""
        self._require_train_mode()
        params, grads, exp_avgs, exp_avg_sqs, mirrors, st, current = self._segments()
        if params:
            ops.grads_check_multi(grads, self._state)
        ops.opt_advance(self._state, self.betas, self.growth_factor, self.backoff_factor, self.growth_interval)
        if params:
            ops.adamw_multi(params, grads, exp_avgs, exp_avg_sqs, self._state, self.betas, self.eps, self.weight_decay, 1.0, mirrors)
        self.invalidate_caches(_mirror_current=current)

    def invalidate_caches(self, _mirror_current: bool = False) -> None:
        """The update goes through raw pointers, so no tensor version moves and every copy of the weights keyed on versions is stale:
        the encoder's packed inference block and resampled position tables, the FPN's re-laid 3x3 weights, the RPN head's and the box
        head's stacked / re-ordered matrices and their bf16 copies.  The training mirror of the encoder was refreshed by the update itself where it was
        current before (``_mirror_current``); otherwise the next forward rebuilds it."""
        from .modeling.dit_fpn import DiTWithFPN
        from .modeling.roi_heads import FastRCNNPredictor, TwoMLPHead
        from .modeling.rpn import RPNHead
        st = getattr(self.encoder, "_flat_state", None)
        if st is not None:
            if _mirror_current and st.native:
                st._packed_version = st.version()         # the update wrote bf16(p) beside every p it changed
                st._dirty = False
            else:
                st.mark_dirty()                           # another grid: the position slot is re-derived from its parameter
        self.encoder._packed_key = None
        self.encoder._pos_cache.clear()
        for mod in self.model.modules():
            if isinstance(mod, DiTWithFPN):
                for c in mod._cache + mod._cache_bf16:
                    c.clear()
            elif isinstance(mod, RPNHead):
                mod._packed.clear()
                mod._packed_bf16.clear()                  # the bf16 neck's operands likewise
            elif isinstance(mod, (TwoMLPHead, FastRCNNPredictor)):
                mod._packed.clear()
                mod._packed_bf16.clear()                  # the bf16 head's operands are keyed on versions like the fp32 re-layouts

    def epoch_end(self) -> None:
        """``StepLR(step_size, gamma).step()``: after every ``step_size`` calls the learning rate is multiplied by ``gamma``; the new
        value reaches the device block through a fill (no synchronisation)."""
        self.epochs += 1
        if self.step_size is not None and self.epochs % self.step_size == 0:
            self.lr *= self.gamma
            self._state_f[_FIELD["lr"]].fill_(self.lr)

    # ---- segments -----------------------------------------------------------------------------------------------------------------------
    def _require_train_mode(self) -> None:
        if not self.model.training:
            raise RuntimeError("DetectorTrainStep: the model is in eval mode - call .train() first")

    def _restore(self, name: str, views: Tuple[torch.Tensor, torch.Tensor]) -> None:
        loaded = self._pending.pop(name, None)
        if loaded is not None:
            for dst, src in zip(views, loaded):
                if tuple(dst.shape) != tuple(src.shape):
                    raise ValueError(f"DetectorTrainStep: loaded moment of {name} has shape {tuple(src.shape)}, the parameter {tuple(dst.shape)}")
                dst.copy_(src)

    def _moments(self, name: str, p: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        mv = self._mom.get(name)
        if mv is None:
            mv = (torch.zeros(p.shape, dtype=torch.float32, device=p.device), torch.zeros(p.shape, dtype=torch.float32, device=p.device))
            self._restore(name, mv)
            self._mom[name] = mv
        return mv

    def _bind_encoder(self, st) -> None:
        """The encoder's moments as two flat blocks in the layout of its parameter block, so that block can be ONE segment; the
        per-parameter moments are views of them.  Re-made (values carried over) when the encoder re-homed its parameters."""
        if self._enc is not None and self._enc[0] is st:
            return
        m, v = torch.zeros_like(st.params), torch.zeros_like(st.params)
        for _, p, off, shape in st.named:
            name = self._names[id(p)]
            views = (m[off: off + p.numel()].view(shape), v[off: off + p.numel()].view(shape))
            old = self._mom.get(name)
            if old is not None:
                views[0].copy_(old[0])
                views[1].copy_(old[1])
            else:
                self._restore(name, views)
            self._mom[name] = views
        self._enc = (st, m, v)

    def _segments(self):
        """Lists of (param, grad, exp_avg, exp_avg_sq, mirror) over every parameter that holds a gradient, the encoder's flat state
        (or None) and whether its training mirror is current.  At the position table's own grid, with the gradients autograd's views
        of one flat block, the whole encoder is a single segment with its bf16 mirror attached."""
        params, grads, exp_avgs, exp_avg_sqs, mirrors = [], [], [], [], []
        st = getattr(self.encoder, "_flat_state", None)
        if st is not None and not st.intact():
            st = None                                     # re-homed since (.to() / assign): plain parameters until the next forward
        in_flat, current = {}, False
        if st is not None:
            self._bind_encoder(st)
            in_flat = {id(p): (off, p) for _, p, off, _ in st.named}
            current = not st._dirty and st._packed_version == st.version()
            mirror = st.packed[: 2 * st.numel].view(torch.bfloat16)
            g = st.grads
            whole = st.native and g.dtype == torch.float32 and g.is_contiguous() and all(
                p.grad is not None and p.grad.dtype == torch.float32 and p.grad.data_ptr() == g.data_ptr() + 4 * off for off, p in in_flat.values())
            if whole:
                params.append(st.params), grads.append(g), exp_avgs.append(self._enc[1]), exp_avg_sqs.append(self._enc[2]), mirrors.append(mirror)
        else:
            whole = False
        for name, p in self.model.named_parameters():
            if p.grad is None or (whole and id(p) in in_flat):
                continue
            g = p.grad
            if g.dtype != torch.float32 or g.device != p.device:
                raise ValueError(f"DetectorTrainStep: the gradient of {name} is {g.dtype} on {g.device}; expected float32 beside its parameter")
            m, v = self._moments(name, p)
            params.append(p.detach()), grads.append(g.contiguous()), exp_avgs.append(m), exp_avg_sqs.append(v)
            if id(p) in in_flat:
                off = in_flat[id(p)][0]
                mirrors.append(mirror[off: off + p.numel()])
            else:
                mirrors.append(None)
        return params, grads, exp_avgs, exp_avg_sqs, mirrors, st, current

    # ---- state ------------------------------------------------------------------------------------------------------------------------------
    def _read_state(self) -> Dict[str, float]:
        host = self._state.cpu()
        hf = host.view(torch.float32)
        out = {n: int(host[_FIELD[n]]) for n in _INT_FIELDS}
        out.update({n: float(hf[_FIELD[n]]) for n in _FLOAT_FIELDS})
        return out

    @property
    def scale(self) -> float:
        """The loss scale the next backward will use.  Synchronises (reads the device block)."""
        return self._read_state()["scale"]

    @property
    def steps(self) -> int:
        """Optimizer steps taken, skipped ones not counted.  Synchronises."""
        return self._read_state()["step"]

    @property
    def skipped_steps(self) -> int:
        """Steps skipped because a gradient was not finite.  Synchronises."""
        return self._read_state()["skipped_steps"]

    def state_dict(self) -> dict:
        """Everything a resumed run needs: the device block's fields, both moments keyed by the model's parameter names, the host-side
        schedule.  Synchronises."""
        moments = {n: (m.detach().clone(), v.detach().clone()) for n, (m, v) in self._mom.items()}
        moments.update({n: (m.clone(), v.clone()) for n, (m, v) in self._pending.items() if n not in moments})
        return {"state": self._read_state(), "exp_avg": {n: mv[0] for n, mv in moments.items()},
                "exp_avg_sq": {n: mv[1] for n, mv in moments.items()}, "lr": self.lr, "epochs": self.epochs}

    def load_state_dict(self, sd: dict) -> None:
        names = set(self._names.values())
        unknown = [n for n in sd["exp_avg"] if n not in names]
        if unknown or set(sd["exp_avg"]) != set(sd["exp_avg_sq"]):
            raise KeyError(f"DetectorTrainStep.load_state_dict: moments do not match the model's parameter names (e.g. {unknown[:3]})")
        host = torch.zeros(len(_FIELD), dtype=torch.int32)
        hf = host.view(torch.float32)
        for n in _INT_FIELDS:
            host[_FIELD[n]] = int(sd["state"][n])
        for n in _FLOAT_FIELDS:
            hf[_FIELD[n]] = float(sd["state"][n])
        self._state.copy_(host)
        self.lr, self.epochs = float(sd["lr"]), int(sd["epochs"])
        self._pending = {n: (sd["exp_avg"][n].detach().to(self.device, torch.float32), sd["exp_avg_sq"][n].detach().to(self.device, torch.float32))
                         for n in sd["exp_avg"]}
        with torch.no_grad():
            for n, views in self._mom.items():            # moments that exist already take their values now, the others when first needed
                if n in self._pending:
                    self._restore(n, views)
                else:
                    views[0].zero_()
                    views[1].zero_()
