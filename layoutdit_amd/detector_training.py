"""The detector's train step: the other half of the reference's iteration (ref ``src/layoutdit/training/trainer.py:164-183``) -

    scaler.scale(sum(loss_dict.values())).backward(); scaler.step(optimizer); scaler.update()        # AdamW(model.parameters())
    scheduler.step()                                                                                 # StepLR, once per epoch

- on ``LayoutDetectionModel.losses`` and the multi-tensor optimizer kernels of ``csrc/optim_multi.hip``.  Every parameter of the
detector that received a gradient - the box head, the RPN head, the FPN and the encoder - is updated by three kernels per 64 tensors
(non-finite check, state machine, AdamW), and the skip decision, the step count, the bias corrections, the loss scale and the learning
rate live in one 40-byte device block (``ldit_opt_state``): between ``backward()`` and the updated weights nothing is read on the host.
``torch.optim.AdamW`` + ``torch.amp.GradScaler`` on the same model launch a group of kernels per parameter tensor and read
``found_inf`` back once per iteration.

Optional, and with the same property: ``max_grad_norm`` clips the global gradient norm
(``torch.nn.utils.clip_grad_norm_``), ``param_groups`` give tensors their own learning-rate scale and weight decay
(:func:`detector_param_groups`: no decay on biases, norms, LayerScale and the tokens; a layer-wise decayed rate across the encoder),
``warmup_iters`` ramps the rate up linearly.  The norm, the clip coefficient and the count of clipped steps live in a second,
16-byte device block (``ldit_clip_state``); one more small launch, one pass over the gradients as before.

The encoder may be the quantisation-aware mxfp8 build (``LayoutDetectionModel(compute_dtype="mxfp8", qat=True)``):
the same launches, then ONE that re-quantises every layer's MX operands from the updated masters (``ldit_requant_train_mirror``),
reading the same device block - a skipped step stores nothing there either.

Gradient accumulation and data-parallel ranks: ``accumulate=A`` makes every ``A``-th ``step()`` the update, on the
mean gradient of the ``A`` micro-batches; ``rank=`` (a ``dp.Rank`` of an initialised process group) sums over the ranks before the
update.  Both go through one flat fp32 bucket that one multi-tensor launch folds the gradients into (``ldit_grads_accumulate_multi_f32``)
and that the launches above read instead of ``p.grad``; the mean's ``1 / (A * world)`` rides in the loss multiplier, so no kernel of the
update changes.  Every rank decides from the same reduced bits, hence alike, without exchanging a flag.

An exponential moving average of the weights: with ``ema_decay`` the update's launch also moves an fp32 shadow of
every parameter it touches towards the new value (``ldit_adamw_ema_groups_multi_f32``: one more read and write per element, the same
skip decision, no further launch), and ``with step.ema_weights():`` exchanges weights and shadows in one launch to evaluate on the average.

PyTorch is plumbing: it owns the memory, the stream and autograd's graph; the arithmetic of
the update is the library's.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist

from . import _lib, ops
from .augment import DetectorAugment
from .dp import Rank, all_reduce_sum, broadcast_from_main

_FIELD = {n: i for i, n in enumerate(_lib.OPT_STATE_FIELDS)}
_INT_FIELDS = ("found_inf", "skip", "step", "growth_tracker", "skipped_steps")
_FLOAT_FIELDS = ("scale", "inv_scale_used", "lr", "bc1", "bc2_sqrt")
_CLIP = {n: i for i, n in enumerate(_lib.CLIP_STATE_FIELDS)}
_ENCODER = "model.backbone.backbone.dit."
BUCKET_ALIGN = 64                                                    # fp32 elements: every slice of the bucket starts on 256 bytes


def bucket_layout(lengths: Sequence[int]) -> Tuple[Tuple[int, ...], int]:
    """Where the slices of the gradient bucket lie: ``(offsets, total)`` in fp32 elements for segments of these lengths, in their
    order - every offset a multiple of ``BUCKET_ALIGN`` (256 bytes), slices disjoint, ``total`` covering the last one.  A segment of
    length 0 takes no room.  A pure function of the tuple of lengths."""
    offsets, at = [], 0
    for n in lengths:
        n = int(n)
        if n < 0:
            raise ValueError(f"bucket_layout: negative segment length {n}")
        offsets.append(at)
        at += -(-n // BUCKET_ALIGN) * BUCKET_ALIGN
    return tuple(offsets), at


def _numel(shape) -> int:
    n = 1
    for v in shape:
        n *= int(v)
    return n


def warmup_lr(lr: float, it: int, warmup_iters: int, warmup_factor: float) -> float:
    """The learning rate of iteration ``it`` (0-based): a line from ``lr * warmup_factor`` at 0 to ``lr`` at ``warmup_iters``."""
    if it >= warmup_iters:
        return lr
    return lr * (warmup_factor + (1.0 - warmup_factor) * it / warmup_iters)


def resolve_param_groups(model, param_groups: Sequence[dict], weight_decay: float = 0.0) -> Dict[str, Tuple[float, float]]:
    """``param_groups`` (a list of ``{"params": names or parameters, "lr_scale": float, "weight_decay": float}``) as parameter name ->
    ``(lr_scale, weight_decay)``; ``weight_decay`` is what a group without one takes.  Refused with a ``ValueError``: a name or a
    tensor that is no parameter of ``model``, a parameter named twice, a negative value."""
    by_id = {id(p): n for n, p in model.named_parameters()}
    names = set(by_id.values())
    hyper: Dict[str, Tuple[float, float]] = {}
    for gi, group in enumerate(param_groups):
        if not isinstance(group, dict) or "params" not in group:
            raise ValueError(f"param_groups[{gi}] is not a dict with a 'params' entry")
        scale, wd = float(group.get("lr_scale", 1.0)), float(group.get("weight_decay", weight_decay))
        if not scale >= 0.0 or not wd >= 0.0:
            raise ValueError(f"param_groups[{gi}]: negative lr_scale or weight_decay ({scale}, {wd})")
        members: Iterable[Union[str, torch.Tensor]] = group["params"]
        if isinstance(members, (str, torch.Tensor)):
            members = [members]
        for q in members:
            name = q if isinstance(q, str) else by_id.get(id(q))
            if name is None or name not in names:
                raise ValueError(f"param_groups[{gi}] names an unknown parameter ({q if isinstance(q, str) else 'a tensor'})")
            if name in hyper:
                raise ValueError(f"parameter {name} is named in two groups")
            hyper[name] = (scale, wd)
    return hyper


def detector_param_groups(model, layer_decay: Optional[float] = None, no_decay: bool = True, weight_decay: float = 0.05) -> List[dict]:
    """The usual groups for fine-tuning a DiT / BEiT backbone under a detector, as ``param_groups`` for :class:`DetectorTrainStep`:
    lists of parameter NAMES, every parameter of ``model.named_parameters()`` in exactly one.

    ``no_decay``: weight decay 0 for every 1-d parameter (biases, LayerNorm, LayerScale) and for ``cls_token`` and
    ``position_embeddings``.  ``layer_decay``: inside the encoder ``lr_scale = layer_decay ** (L + 1 - k)`` for layer ``k = 1 .. L``
    (``encoder.layer.{k - 1}``) and ``k = 0`` for the embeddings; everything else - the rest of the encoder, FPN, RPN, box head - 1."""
    if layer_decay is not None and not 0.0 < float(layer_decay) <= 1.0:
        raise ValueError("detector_param_groups: layer_decay must lie in (0, 1]")
    if not float(weight_decay) >= 0.0:
        raise ValueError("detector_param_groups: weight_decay must be >= 0")
    L = model.model.backbone.backbone.dit.config.num_hidden_layers
    groups: Dict[Tuple[float, float], List[str]] = {}
    for name, p in model.named_parameters():
        scale = 1.0
        if layer_decay is not None and name.startswith(_ENCODER):
            rest = name[len(_ENCODER):]
            if rest.startswith("embeddings."):
                scale = float(layer_decay) ** (L + 1)
            elif rest.startswith("encoder.layer."):
                scale = float(layer_decay) ** (L - int(rest.split(".")[2]))
        plain = no_decay and (p.dim() <= 1 or name.endswith(("cls_token", "position_embeddings")))
        groups.setdefault((scale, 0.0 if plain else float(weight_decay)), []).append(name)
    return [{"params": names, "lr_scale": s, "weight_decay": w} for (s, w), names in groups.items()]


class DetectorTrainStep:
    """``step(images, targets)`` = the reference's iteration on a :class:`LayoutDetectionModel` in train mode; ``apply()`` = its
    optimizer half alone, on the gradients the parameters currently hold.

    ``loss_scaling=False`` keeps the scale at 1 (the loss is not multiplied); a step whose gradients hold a NaN or an infinity is
    still skipped and counted.  ``step_size=None`` keeps the learning rate constant; otherwise :meth:`epoch_end` is ``StepLR``.

    ``max_grad_norm``: the gradients are multiplied by ``min(1, max_grad_norm / (norm + 1e-6))``, ``norm`` the L2 norm of all unscaled
    gradients (of the parameters' own elements; nothing else of the encoder's flat block enters).  ``param_groups``: a list of
    ``{"params": names or parameters, "lr_scale": float, "weight_decay": float}``; a parameter no group names has ``lr_scale`` 1 and
    the constructor's ``weight_decay``.  ``warmup_iters``: for that many first calls of :meth:`step` the learning rate is
    :func:`warmup_lr`.  With all four left alone the step is the three launches it always was.

    ``accumulate``: micro-batches per update.  Every :meth:`step` is one micro-batch; its gradients are folded into one flat fp32
    bucket (:meth:`accumulate_grads`) and the ``accumulate``-th call updates from the bucket: the mean gradient, since the loss was
    multiplied by ``scale / (accumulate * world)``.  ``rank``: this process's :class:`~layoutdit_amd.dp.Rank`; with ``world > 1`` the
    bucket is summed over the ranks (one collective) before the update, and ``broadcast_parameters`` makes rank 0's weights everybody's
    at construction.  ``iters``, the warmup and :attr:`steps` count updates, not micro-batches.  With ``accumulate == 1`` and one rank
    there is no bucket and nothing changes.

    ``augment``: a :class:`~layoutdit_amd.augment.DetectorAugment`; every :meth:`step` then trains on windows of its pages - random
    crop, scale jitter and flip - drawn on the host from the augment's own generator: the windowed input transform
    and one launch for the targets, no copy of a page and no synchronisation.  Without it the step launches what it always did.

    ``ema_decay``: keep an exponential moving average of every updated parameter, ``e += (1 - d) * (p - e)`` inside the update's own
    launch, with ``d = min(ema_decay, (1 + n) / (10 + n))`` after ``n`` taken steps (``ema_warmup=False``: ``d = ema_decay``);
    :meth:`ema_state_dict` returns it, ``with step.ema_weights():`` evaluates on it.  With ``None`` no launch and no bit changes."""

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 0.0, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 step_size: Optional[int] = None, gamma: float = 0.1, init_scale: float = 65536.0, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000, loss_scaling: bool = True, max_grad_norm: Optional[float] = None,
                 param_groups: Optional[Sequence[dict]] = None, warmup_iters: int = 0, warmup_factor: float = 1e-3, accumulate: int = 1,
                 rank: Optional[Rank] = None, broadcast_parameters: bool = True, augment: Optional[DetectorAugment] = None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True):
        from .modeling.detector import LayoutDetectionModel
        if not isinstance(model, LayoutDetectionModel):
            raise TypeError("DetectorTrainStep: expected a LayoutDetectionModel (the encoder alone trains with TrainStep)")
        if int(accumulate) < 1:
            raise ValueError("DetectorTrainStep: accumulate must be at least 1 (micro-batches per update)")
        if rank is not None and not isinstance(rank, Rank):
            raise TypeError("DetectorTrainStep: rank must be a layoutdit_amd.dp.Rank (dp.init() returns one)")
        if rank is not None and rank.world > 1:
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError(f"DetectorTrainStep: rank {rank.rank} of {rank.world} without an initialised process group - call dp.init() first")
            if dist.get_world_size() != rank.world:
                raise RuntimeError(f"DetectorTrainStep: rank.world = {rank.world}, the process group has {dist.get_world_size()} ranks")
        if augment is not None and not isinstance(augment, DetectorAugment):
            raise TypeError("DetectorTrainStep: augment must be a layoutdit_amd.augment.DetectorAugment")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"DetectorTrainStep: ema_decay must lie in [0, 1) (None: no moving average), got {ema_decay}")
        self.model = model
        self.augment = augment
        if augment is not None:                                              # what keeps a box under a window is the augment's to say
            model.model.transform.min_visibility, model.model.transform.min_size = augment.min_visibility, augment.min_size
        self.encoder = model.model.backbone.backbone.dit
        if self.encoder.compute_dtype == "fp8" or (self.encoder.compute_dtype == "mxfp8" and not getattr(self.encoder, "qat", False)):
            raise NotImplementedError(f"DetectorTrainStep: the {self.encoder.compute_dtype} encoder is not covered - 'fp8' and 'mxfp8' are inference "
                                      "builds with no training forward (TrainStep refuses them too); build the detector with compute_dtype "
                                      "'f32' or 'bf16', or with compute_dtype 'mxfp8' and qat=True (quantisation-aware training)")
        self._require_train_mode()
        params = list(model.named_parameters())
        if not params:
            raise ValueError("DetectorTrainStep: the model has no parameters")
        self.device = params[0][1].device
        if self.device.type != "cuda" or any(p.device != self.device for _, p in params):
            raise ValueError("DetectorTrainStep: every parameter must live on one GPU (libldit_hip has no CPU path) - call .to(device) first")
        if step_size is not None and int(step_size) < 1:
            raise ValueError("DetectorTrainStep: step_size must be a positive number of epochs")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("DetectorTrainStep: max_grad_norm must be positive (None: no clipping)")
        if int(warmup_iters) < 0 or not 0.0 <= float(warmup_factor) <= 1.0:
            raise ValueError("DetectorTrainStep: warmup_iters must be >= 0 and warmup_factor lie in [0, 1]")
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.warmup_iters, self.warmup_factor, self.iters = int(warmup_iters), float(warmup_factor), 0
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
        self.ema_decay, self.ema_warmup = None if ema_decay is None else float(ema_decay), bool(ema_warmup)
        self._ema: Dict[str, torch.Tensor] = {}                              # parameter name -> its fp32 shadow (the moving average)
        self._ema_pending: Dict[str, torch.Tensor] = {}                      # loaded shadows of parameters not seen yet
        self._enc_ema = None                                                 # (FlatState, the encoder's shadows as one flat block)
        self._shadows: List[Optional[torch.Tensor]] = []                     # per segment of the last _segments() call
        self._averaged = None                                                # inside ema_weights(): what its exit swaps back
        # parameter name -> (lr_scale, weight_decay), or None: one group, the three launches of section 21
        self._hyper = None if param_groups is None else resolve_param_groups(model, param_groups, self.weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip = None if max_grad_norm is None else ops.new_clip_state(self.device, self.max_grad_norm)
        self._partials: Optional[torch.Tensor] = None                        # one float64 per 1 024 gradient elements, made with the moments
        self._partials_key = None
        self._grouped = self._hyper is not None or self._clip is not None
        self.accumulate, self.rank, self.world = int(accumulate), rank, 1 if rank is None else int(rank.world)
        self._use_bucket = self.accumulate > 1 or self.world > 1
        self._loss_mul = 1.0 / (self.accumulate * self.world)
        self.pending_micro_batches = 0                                       # folds since the last apply()
        self._bucket: Optional[torch.Tensor] = None                          # made at the first fold, never re-made
        self._bucket_key: Optional[tuple] = None                             # ((first parameter of the segment, its length), ...)
        self._bucket_slices: List[torch.Tensor] = []
        self._bucket_members: List[list] = []                                # per slice: (parameter name, offset in the slice, shape)
        self._members: List[list] = []                                       # the same, of the last _segments() call
        self._layout_agreed = False
        if self.world > 1 and broadcast_parameters:
            broadcast_from_main(rank, list(model.parameters()) + list(model.buffers()))
            self.invalidate_caches()

    def _hyper_of(self, name: str) -> Tuple[float, float]:
        return (1.0, self.weight_decay) if self._hyper is None else self._hyper.get(name, (1.0, self.weight_decay))

    # ---- the iteration ----------------------------------------------------------------------------------------------------------------
    def step(self, images: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]],
             generator: Optional[torch.Generator] = None, windows=None) -> Dict[str, torch.Tensor]:
        """One iteration: gradients cleared, ``model.losses``, backward on the scaled sum, check / advance / update.  Returns the four
        unscaled, detached losses.  From the backward on there is no host synchronisation; the loss scale enters the graph as a device
        tensor.  (The input transform's host bookkeeping is ``model.losses``'s own.)

        With ``accumulate`` or ranks every call is one micro-batch: the loss is multiplied by ``scale * (1 / (accumulate * world))`` -
        one fp32 product of the block's scale and a constant, on the device -, the gradients are folded into the bucket, and only the
        ``accumulate``-th call goes on to :meth:`apply`.  The losses returned are this call's, of this rank.

        ``windows``: this call's windows (``LayoutDetectionModel.losses``); left out, an ``augment`` draws them - one draw per call."""
        self._require_own_weights("step")
        self._require_train_mode()
        if windows is None and self.augment is not None:
            windows = self.augment.sample([img.shape[-2:] for img in images])
        if self.pending_micro_batches == 0 and self.warmup_iters and self.iters <= self.warmup_iters:   # the last of these fills writes the full rate
            self._write_lr()
        for p in self.model.parameters():
            p.grad = None
        if windows is None:
            losses = self.model.losses(images, targets, generator=generator)
        else:
            losses = self.model.losses(images, targets, generator=generator, windows=windows)
        total = sum(losses.values())
        if self._use_bucket:
            total = total * (self._state_f[_FIELD["scale"]] * self._loss_mul if self.loss_scaling else self._loss_mul)
        elif self.loss_scaling:
            total = total * self._state_f[_FIELD["scale"]]
        total.backward()
        if self._use_bucket:
            self.accumulate_grads()
        if self.pending_micro_batches >= self.accumulate or not self._use_bucket:
            self.iters += 1
            self.apply()
        return {k: v.detach() for k, v in losses.items()}

    # ---- the gradient bucket ------------------------------------------------------------------------------------------------------------
    @property
    def bucket(self) -> Optional[torch.Tensor]:
        """The flat fp32 gradient bucket, or None: before the first fold, and always with ``accumulate == 1`` on one rank."""
        return self._bucket

    def accumulated_grads(self) -> Dict[str, torch.Tensor]:
        """Parameter name -> its gradient in the bucket (a view): ``scale / (accumulate * world)`` times the sum over the micro-batches
        folded since the last update, and over the ranks once :meth:`apply` reduced it."""
        return {name: self._bucket_slices[i][off: off + _numel(shape)].view(shape)
                for i, members in enumerate(self._bucket_members) for name, off, shape in members}

    def _bind_bucket(self, grads: List[torch.Tensor]) -> List[torch.Tensor]:
        """The bucket's slices for the segments ``_segments()`` just returned.  The layout is fixed by the first fold; segments that do
        not repeat it (a parameter that got no gradient this time, another input grid) are refused."""
        key = tuple((members[0][0], g.numel()) for members, g in zip(self._members, grads))
        if self._bucket is None:
            offsets, total = bucket_layout([n for _, n in key])
            flat = torch.zeros(total + BUCKET_ALIGN, dtype=torch.float32, device=self.device)
            first = (-flat.data_ptr() % (4 * BUCKET_ALIGN)) // 4              # the allocator's blocks are aligned already: 0
            self._bucket = flat[first: first + total]
            self._bucket_key, self._bucket_members = key, [list(m) for m in self._members]
            self._bucket_slices = [self._bucket[o: o + n] for o, (_, n) in zip(offsets, key)]
        elif key != self._bucket_key:
            i = next((i for i, (a, b) in enumerate(zip(key, self._bucket_key)) if a != b), min(len(key), len(self._bucket_key)))
            now = "no segment" if i >= len(key) else f"{key[i][0]} ({key[i][1]} elements)"
            was = "no segment" if i >= len(self._bucket_key) else f"{self._bucket_key[i][0]} ({self._bucket_key[i][1]} elements)"
            raise RuntimeError(f"DetectorTrainStep: the gradients do not repeat the bucket's layout, fixed at the first fold: segment {i} is "
                               f"{now}, the bucket has {was} there (a parameter without a gradient in this micro-batch, or another input grid)")
        return self._bucket_slices

    @torch.no_grad()
    def accumulate_grads(self) -> None:
        """Fold the gradients the parameters hold now into the bucket: the first fold since the last :meth:`apply` overwrites it (bit
        for bit), later ones add (one fp32 addition per element).  ``ceil(S / ops.ACC_MAX_SEGMENTS)`` launches, no synchronisation."""
        if not self._use_bucket:
            raise RuntimeError("DetectorTrainStep.accumulate_grads: built with accumulate=1 on one rank, there is no bucket - apply() reads p.grad")
        self._require_own_weights("accumulate_grads")
        self._require_train_mode()
        grads = self._segments()[1]
        ops.grads_accumulate_multi(self._bind_bucket(grads), grads, overwrite=self.pending_micro_batches == 0)
        self.pending_micro_batches += 1

    def _reduce_bucket(self) -> None:
        """The bucket summed over the ranks: one collective.  Every rank receives the same bits."""
        if not self._layout_agreed:                                           # once, host side: better than a mis-sized collective
            keys = [None] * self.world
            dist.all_gather_object(keys, self._bucket_key)
            if any(k != keys[0] for k in keys):
                bad = next(r for r, k in enumerate(keys) if k != keys[0])
                raise RuntimeError(f"DetectorTrainStep: the ranks' gradient buckets differ in layout (rank {bad} against rank 0): "
                                   "every rank must give the same parameters a gradient")
            self._layout_agreed = True
        if self._bucket.numel():
            all_reduce_sum(self.rank, self._bucket)

    @torch.no_grad()
    def apply(self) -> None:
        """The optimizer half alone, on the gradients the parameters hold now (made with the current loss scale): non-finite check,
        state machine, AdamW - or nothing, if the check fired.  No synchronisation; capturable once every moment exists (after one
        eager call).  A replayed graph moves the weights behind this object's back: call :meth:`invalidate_caches` after replays.

        Under the quantisation-aware mxfp8 encoder (``qat=True``) one launch follows, with the same state block: the MX operands of
        the encoder's training mirror re-made from the updated masters (``ops.requant_train_mirror``), so that the mirror is a fresh
        ``ldit_pack_train`` of them - where the mirror was current before the update; otherwise the next forward packs, as ever.

        With a bucket in use (``accumulate > 1`` or ranks) the gradients are the bucket's slices, as :meth:`accumulate_grads` left
        them, after their sum over the ranks - ordered on the current stream under RCCL, no host wait; the launches are the same.

        With ``ema_decay`` the update is ``ops.adamw_ema_groups_multi`` in place of ``adamw_multi`` / ``adamw_groups_multi``: the same
        bits in the parameters, the moments and the mirror, and every segment's shadow moved in the same launch."""
        self._require_own_weights("apply")
        self._require_train_mode()
        params, grads, exp_avgs, exp_avg_sqs, mirrors, st, current, hyper = self._segments()
        shadows = self._shadows
        if self._use_bucket:
            if self.pending_micro_batches == 0:
                raise RuntimeError("DetectorTrainStep.apply: nothing was folded into the bucket since the last update - call "
                                   "accumulate_grads() after each backward (step() does)")
            grads = self._bind_bucket(grads)
            if self.world > 1:
                self._reduce_bucket()
            self.pending_micro_batches = 0
        if not self._grouped:
            if params:
                ops.grads_check_multi(grads, self._state)
            ops.opt_advance(self._state, self.betas, self.growth_factor, self.backoff_factor, self.growth_interval)
            if params and self.ema_decay is not None:
                # lr_scale 1, one weight decay and no clip block: adamw_multi's bits (csrc/optim_multi.hip), and the shadows beside them
                ops.adamw_ema_groups_multi(params, grads, exp_avgs, exp_avg_sqs, self._state, [1.0] * len(params), [self.weight_decay] * len(params),
                                           shadows, self.ema_decay, self.ema_warmup, None, self.betas, self.eps, mirrors)
            elif params:
                ops.adamw_multi(params, grads, exp_avgs, exp_avg_sqs, self._state, self.betas, self.eps, self.weight_decay, 1.0, mirrors)
        else:
            # check (+ sum of squares) -> state machine -> (norm, clip coefficient) -> update: each needs its predecessor complete
            # over the WHOLE parameter set, like the three launches above
            n = 0
            if self._clip is not None:
                key = tuple(g.numel() for g in grads)
                if self._partials is None or key != self._partials_key:
                    need = max(ops.grad_norm_partials(grads), 1)
                    if self._partials is None or self._partials.numel() < need:
                        self._partials = torch.empty(need, dtype=torch.float64, device=self.device)
                    self._partials_key = key
                if params:
                    n = ops.grads_check_norm_multi(grads, self._state, self._partials)
            elif params:
                ops.grads_check_multi(grads, self._state)
            ops.opt_advance(self._state, self.betas, self.growth_factor, self.backoff_factor, self.growth_interval)
            if self._clip is not None:
                ops.clip_finish(self._state, self._clip, self._partials, n)
            if params and self.ema_decay is not None:
                ops.adamw_ema_groups_multi(params, grads, exp_avgs, exp_avg_sqs, self._state, [h[0] for h in hyper], [h[1] for h in hyper],
                                           shadows, self.ema_decay, self.ema_warmup, self._clip, self.betas, self.eps, mirrors)
            elif params:
                ops.adamw_groups_multi(params, grads, exp_avgs, exp_avg_sqs, self._state, [h[0] for h in hyper], [h[1] for h in hyper],
                                       self._clip, self.betas, self.eps, mirrors)
        if st is not None and st.mx and current and st.native:
            # quantisation-aware mxfp8 encoder: the AdamW launches wrote bf16(p) over the whole mirror; one more launch re-makes every
            # layer's MX operands (codes, scales, dequantised copies, folded bias) from the updated masters - or nothing, on a skipped step
            ops.requant_train_mirror(st, self._state)
        self.invalidate_caches(_mirror_current=current)

    def invalidate_caches(self, _mirror_current: bool = False) -> None:
        """The update goes through raw pointers, so no tensor version moves and every copy of the weights keyed on versions is stale:
        the encoder's packed inference block and resampled position tables, every stage's ``OperandCache`` (re-laid, stacked and
        re-ordered matrices, their bf16 copies, the dgrad operands).  The training mirror of the encoder was refreshed by the update itself where it was
        current before (``_mirror_current``); otherwise the next forward rebuilds it."""
        from .modeling.grad_ops import OperandCache
        st = getattr(self.encoder, "_flat_state", None)
        if st is not None:
            if _mirror_current and st.native:
                st._packed_version = st.version()         # the update wrote bf16(p) beside every p it changed
                st._dirty = False
            else:
                st.mark_dirty()                           # another grid: the position slot is re-derived from its parameter
        self.encoder._packed_key = None
        self.encoder._pos_cache.clear()
        for mod in self.model.modules():                  # every stage keeps its derived weights in one cache, under one name
            cache = getattr(mod, "_operand_cache", None)
            if isinstance(cache, OperandCache):
                cache.clear()

    def epoch_end(self) -> None:
        """``StepLR(step_size, gamma).step()``: after every ``step_size`` calls the learning rate is multiplied by ``gamma``; the new
        value reaches the device block through a fill (no synchronisation)."""
        self.epochs += 1
        if self.step_size is not None and self.epochs % self.step_size == 0:
            self.lr *= self.gamma
            self._write_lr()

    def _write_lr(self) -> None:
        """The learning rate of the next iteration into the device block (a fill: no synchronisation)."""
        self._state_f[_FIELD["lr"]].fill_(warmup_lr(self.lr, self.iters, self.warmup_iters, self.warmup_factor))

    # ---- segments -----------------------------------------------------------------------------------------------------------------------
    def _require_train_mode(self) -> None:
        if not self.model.training:
            raise RuntimeError("DetectorTrainStep: the model is in eval mode - call .train() first")

    def _require_own_weights(self, what: str) -> None:
        if self._averaged is not None:
            raise RuntimeError(f"DetectorTrainStep.{what}: inside ema_weights() the parameters hold the moving average and the shadows "
                               "hold the trained weights - leave the block first")

    def _restore_shadow(self, name: str, view: torch.Tensor) -> None:
        loaded = self._ema_pending.pop(name, None)
        if loaded is not None:
            if tuple(view.shape) != tuple(loaded.shape):
                raise ValueError(f"DetectorTrainStep: loaded moving average of {name} has shape {tuple(loaded.shape)}, the parameter {tuple(view.shape)}")
            view.copy_(loaded)

    def _shadow(self, name: str, p: torch.Tensor) -> Optional[torch.Tensor]:
        """The parameter's moving average: an fp32 clone of it at first sight - before its first update - or what was loaded."""
        if self.ema_decay is None:
            return None
        e = self._ema.get(name)
        if e is None:
            e = p.detach().clone(memory_format=torch.contiguous_format)
            self._restore_shadow(name, e)
            self._ema[name] = e
        return e

    def _bind_encoder_ema(self, st) -> None:
        """The encoder's shadows as one flat block in the layout of its parameter block, like its moments: a clone of that block at
        first sight; re-made, the averages carried over, when the encoder re-homed its parameters."""
        if self.ema_decay is None or (self._enc_ema is not None and self._enc_ema[0] is st):
            return
        flat = st.params.detach().clone()
        for _, p, off, shape in st.named:
            name = self._names[id(p)]
            view = flat[off: off + p.numel()].view(shape)
            old = self._ema.get(name)
            if old is not None:
                view.copy_(old)
            else:
                self._restore_shadow(name, view)
            self._ema[name] = view
        self._enc_ema = (st, flat)

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
        of one flat block, the whole encoder is a single segment with its bf16 mirror attached.

        With clipping or groups (``hyper``: one ``(lr_scale, weight_decay)`` per segment, else None) the block never enters whole: the
        gradient block is ``torch.empty_like`` and the backward promises the named slots only, so the key-bias third of every layer
        (no parameter: BEiT's key has no bias) may hold whatever the allocator left, which a norm must not see.  The encoder then
        enters as runs of neighbouring named slots with equal hyper-parameters, mirror slices at the matching offsets: the norm
        covers the parameters' own elements and nothing else."""
        params, grads, exp_avgs, exp_avg_sqs, mirrors = [], [], [], [], []
        hyper = [] if self._grouped else None
        members = self._members = []                      # per segment: (parameter name, offset in the segment, shape); for the bucket only
        shadows = self._shadows = []                      # per segment: its moving average (ema_decay), else None
        track = self._use_bucket
        st = getattr(self.encoder, "_flat_state", None)
        if st is not None and not st.intact():
            st = None                                     # re-homed since (.to() / assign): plain parameters until the next forward
        in_flat, current, taken = {}, False, set()
        if st is not None:
            self._bind_encoder(st)
            self._bind_encoder_ema(st)
            flat_ema = None if self._enc_ema is None else self._enc_ema[1]
            in_flat = {id(p): (off, p) for _, p, off, _ in st.named}
            current = not st._dirty and st._packed_version == st.version()
            mirror = st.packed[: 2 * st.numel].view(torch.bfloat16)
            g = st.grads
            whole = not self._grouped and st.native and g.dtype == torch.float32 and g.is_contiguous() and all(
                p.grad is not None and p.grad.dtype == torch.float32 and p.grad.data_ptr() == g.data_ptr() + 4 * off for off, p in in_flat.values())
            if whole:
                params.append(st.params), grads.append(g), exp_avgs.append(self._enc[1]), exp_avg_sqs.append(self._enc[2]), mirrors.append(mirror)
                shadows.append(flat_ema)
                if track:
                    members.append([(self._names[id(p)], off, shape) for _, p, off, shape in st.named])
            elif self._grouped and g.dtype == torch.float32 and g.is_contiguous():
                runs = []                                 # [first offset, end offset, (lr_scale, weight_decay)] over slots whose gradient is autograd's view
                for off, p in sorted(in_flat.values(), key=lambda e: e[0]):
                    if p.grad is None or p.grad.dtype != torch.float32 or p.grad.data_ptr() != g.data_ptr() + 4 * off:
                        continue
                    h = self._hyper_of(self._names[id(p)])
                    if runs and runs[-1][1] == off and runs[-1][2] == h:
                        runs[-1][1] = off + p.numel()
                    else:
                        runs.append([off, off + p.numel(), h, []])
                    runs[-1][3].append((self._names[id(p)], off - runs[-1][0], tuple(p.shape)))
                    taken.add(id(p))
                for a, b, h, inside in runs:
                    if track:
                        members.append(inside)
                    params.append(st.params[a:b]), grads.append(g[a:b]), exp_avgs.append(self._enc[1][a:b]), exp_avg_sqs.append(self._enc[2][a:b])
                    mirrors.append(mirror[a:b]), hyper.append(h)
                    shadows.append(None if flat_ema is None else flat_ema[a:b])
        else:
            whole = False
        for name, p in self.model.named_parameters():
            if p.grad is None or (whole and id(p) in in_flat) or id(p) in taken:
                continue
            g = p.grad
            if g.dtype != torch.float32 or g.device != p.device:
                raise ValueError(f"DetectorTrainStep: the gradient of {name} is {g.dtype} on {g.device}; expected float32 beside its parameter")
            m, v = self._moments(name, p)
            params.append(p.detach()), grads.append(g.contiguous()), exp_avgs.append(m), exp_avg_sqs.append(v)
            shadows.append(self._shadow(name, p))
            if track:
                members.append([(name, 0, tuple(p.shape))])
            if id(p) in in_flat:
                off = in_flat[id(p)][0]
                mirrors.append(mirror[off: off + p.numel()])
            else:
                mirrors.append(None)
            if hyper is not None:
                hyper.append(self._hyper_of(name))
        return params, grads, exp_avgs, exp_avg_sqs, mirrors, st, current, hyper

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

    @property
    def grad_norm(self) -> torch.Tensor:
        """The global L2 norm of the last step's unscaled gradients, before clipping: a 0-dim view of the device block (no
        synchronisation; non-finite after a skipped step).  Needs ``max_grad_norm``."""
        if self._clip is None:
            raise RuntimeError("DetectorTrainStep.grad_norm: built without max_grad_norm, no norm is formed")
        return self._clip[_CLIP["total_norm"]]

    @property
    def clipped_steps(self) -> int:
        """Steps taken whose clip coefficient was below 1.  Synchronises."""
        if self._clip is None:
            raise RuntimeError("DetectorTrainStep.clipped_steps: built without max_grad_norm")
        return int(self._clip.cpu().view(torch.int32)[_CLIP["clipped_steps"]])

    # ---- the moving average ----------------------------------------------------------------------------------------------------------------
    def _require_ema(self, what: str) -> None:
        if self.ema_decay is None:
            raise RuntimeError(f"DetectorTrainStep.{what}: built without ema_decay, no moving average is kept")

    @torch.no_grad()
    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's ``state_dict()`` with every parameter that has a shadow replaced by a clone of it: what a fresh
        ``LayoutDetectionModel`` of the same construction loads to evaluate on the average.  Parameters that never had a gradient, and
        buffers, are the model's own entries."""
        self._require_ema("ema_state_dict")
        out = dict(self.model.state_dict())
        if self._averaged is not None:                    # inside ema_weights() the model holds the average already
            return {k: (v.detach().clone() if k in self._ema else v) for k, v in out.items()}
        for name in self._names.values():
            e = self._ema.get(name, self._ema_pending.get(name))
            if e is not None and name in out:
                out[name] = e.detach().clone().view(out[name].shape)
        return out

    def _swap_lists(self):
        """(parameters, shadows, mirrors) of one ``ops.swap_multi``: at the encoder's own grid its flat block against its flat shadow,
        the bf16 mirror attached; every other parameter that has a shadow on its own."""
        a, b, mirrors, in_flat = [], [], [], set()
        st = getattr(self.encoder, "_flat_state", None)
        if st is not None and not st.intact():
            st = None
        if st is not None and st.native and self._enc_ema is not None and self._enc_ema[0] is st:
            a.append(st.params), b.append(self._enc_ema[1]), mirrors.append(st.packed[: 2 * st.numel].view(torch.bfloat16))
            in_flat = {id(p) for _, p, _, _ in st.named}
        for name, p in self.model.named_parameters():
            e = self._ema.get(name)
            if e is None or id(p) in in_flat:
                continue
            if not p.is_contiguous():
                raise ValueError(f"DetectorTrainStep.ema_weights: parameter {name} is not contiguous")
            a.append(p.detach()), b.append(e), mirrors.append(None)
        return a, b, mirrors, st

    @contextmanager
    def ema_weights(self):
        """``with step.ema_weights():`` - the model holds the moving average and is in eval mode: ONE ``ops.swap_multi`` exchanges
        every parameter with its shadow (the elements move as integers; parameters without a shadow stay), every derived copy of the
        weights is dropped (:meth:`invalidate_caches`), and ``evaluate(model, batches)`` / ``forward_padded`` see the average with no
        further change - under the quantisation-aware mxfp8 encoder, the mxfp8 inference build of the averaged masters.  On exit the
        same launch swaps back bit for bit, the caches are dropped again, the encoder's training mirror is re-packed from the restored
        masters where it was current before, and the mode the model was in returns.  Inside, :meth:`step`, :meth:`apply`,
        :meth:`accumulate_grads` and :meth:`state_dict` are refused: weights and shadows have changed places."""
        self._require_ema("ema_weights")
        self._require_own_weights("ema_weights")
        if self.pending_micro_batches:
            raise RuntimeError(f"DetectorTrainStep.ema_weights: {self.pending_micro_batches} of {self.accumulate} micro-batches are folded into "
                               "the gradient bucket - evaluate after the update")
        with torch.no_grad():
            for name, p in self.model.named_parameters():     # loaded averages of parameters no update has bound yet
                if name in self._ema_pending and name not in self._ema:
                    self._shadow(name, p)
        a, b, mirrors, st = self._swap_lists()
        current = st is not None and not st._dirty and st._packed_version == st.version()
        was_training = self.model.training
        ops.swap_multi(a, b, mirrors)
        self._averaged = (a, b, mirrors)
        self.invalidate_caches()
        self.model.eval()
        try:
            yield self.model
        finally:
            ops.swap_multi(a, b, mirrors)
            self._averaged = None
            self.invalidate_caches()
            if current and st.intact():
                st.repack(force=True)                     # the swaps wrote bf16 of whole blocks: the training mirror is a fresh pack again
            self.model.train(was_training)

    def state_dict(self) -> dict:
        """Everything a resumed run needs: the device block's fields, both moments keyed by the model's parameter names, the host-side
        schedule - and, with ``ema_decay``, the shadows under ``"ema"``.  Synchronises.  Refused in the middle of an accumulation: the
        bucket is not part of it."""
        self._require_own_weights("state_dict")
        if self.pending_micro_batches:
            raise RuntimeError(f"DetectorTrainStep.state_dict: {self.pending_micro_batches} of {self.accumulate} micro-batches are folded into the "
                               "gradient bucket, which no state dictionary holds - save after the update")
        moments = {n: (m.detach().clone(), v.detach().clone()) for n, (m, v) in self._mom.items()}
        moments.update({n: (m.clone(), v.clone()) for n, (m, v) in self._pending.items() if n not in moments})
        out = {"state": self._read_state(), "exp_avg": {n: mv[0] for n, mv in moments.items()},
               "exp_avg_sq": {n: mv[1] for n, mv in moments.items()}, "lr": self.lr, "epochs": self.epochs, "iters": self.iters}
        if self._clip is not None:
            host = self._clip.cpu()
            out["clip"] = {n: (int(host.view(torch.int32)[i]) if n == "clipped_steps" else float(host[i])) for n, i in _CLIP.items()}
        if self.augment is not None:
            out["augment"] = self.augment.state_dict()
        if self.ema_decay is not None:
            shadow = {n: e.detach().clone() for n, e in self._ema.items()}
            shadow.update({n: e.clone() for n, e in self._ema_pending.items() if n not in shadow})
            out["ema"] = {"shadow": shadow, "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup}
        return out

    def load_state_dict(self, sd: dict) -> None:
        self._require_own_weights("load_state_dict")
        names = set(self._names.values())
        unknown = [n for n in sd["exp_avg"] if n not in names]
        if unknown or set(sd["exp_avg"]) != set(sd["exp_avg_sq"]):
            raise KeyError(f"DetectorTrainStep.load_state_dict: moments do not match the model's parameter names (e.g. {unknown[:3]})")
        ema = sd.get("ema") if self.ema_decay is not None else None      # a step built without ema_decay keeps none
        if ema:
            unknown = [n for n in ema["shadow"] if n not in names]
            if unknown:
                raise KeyError(f"DetectorTrainStep.load_state_dict: moving averages do not match the model's parameter names (e.g. {unknown[:3]})")
        host = torch.zeros(len(_FIELD), dtype=torch.int32)
        hf = host.view(torch.float32)
        for n in _INT_FIELDS:
            host[_FIELD[n]] = int(sd["state"][n])
        for n in _FLOAT_FIELDS:
            hf[_FIELD[n]] = float(sd["state"][n])
        self._state.copy_(host)
        self.lr, self.epochs = float(sd["lr"]), int(sd["epochs"])
        # a dictionary written before warmup existed has no count: every apply() was one iteration, taken or skipped
        self.iters = int(sd["iters"]) if "iters" in sd else int(sd["state"]["step"]) + int(sd["state"]["skipped_steps"])
        if self._clip is not None and "clip" in sd:
            host = torch.zeros(len(_CLIP), dtype=torch.float32)
            for n, i in _CLIP.items():
                if n == "clipped_steps":
                    host.view(torch.int32)[i] = int(sd["clip"][n])
                else:
                    host[i] = float(sd["clip"][n])
            self._clip.copy_(host)
        if self.augment is not None and "augment" in sd:
            self.augment.load_state_dict(sd["augment"])
        self._pending = {n: (sd["exp_avg"][n].detach().to(self.device, torch.float32), sd["exp_avg_sq"][n].detach().to(self.device, torch.float32))
                         for n in sd["exp_avg"]}
        with torch.no_grad():
            for n, views in self._mom.items():            # moments that exist already take their values now, the others when first needed
                if n in self._pending:
                    self._restore(n, views)
                else:
                    views[0].zero_()
                    views[1].zero_()
        if self.ema_decay is not None:
            # every shadow is dropped and re-made when first needed: a clone of the parameter as it is then, overwritten by the loaded
            # average where the dictionary holds one (one written without ema_decay holds none: the average restarts at the weights)
            self._ema, self._enc_ema = {}, None
            self._ema_pending = {n: t.detach().to(self.device, torch.float32).clone() for n, t in ema["shadow"].items()} if ema else {}
            if ema:
                self.ema_decay, self.ema_warmup = float(ema["ema_decay"]), bool(ema["ema_warmup"])
