"""The moving average of the weights inside the detector's update and the evaluation on it on the GPU:
ldit_adamw_ema_groups_multi_f32 and ldit_swap_multi_f32 through layoutdit_amd.ops and DetectorTrainStep(ema_decay=...), against the
float64 restatement tests/ema_oracle.py.

Gates: after five steps the shadows err against float64 at most TWICE as much as torch.Tensor.lerp_ in fp32 on the CPU does on the same
per-step p and w (the rule of tests/test_gpu_detector_step.py), while p, m, v and the mirrors are the bits of ops.adamw_multi without
an average; a skipped step changes no bit of a shadow and does not age the warmup; the swap moves bits (-0.0, infinities, NaN payloads),
writes bf16(new a) and undoes itself; ema_state_dict() is the recurrence over the model's own weights; inside ema_weights() the model
computes what a fresh detector loaded from ema_state_dict() computes, and leaving it restores every bit and the next step; the shadows
stand still through a folding call, replay from a graph, resume from a state dictionary and agree across two ranks, bit for bit."""
import copy
import hashlib
import os
import socket
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp                      # noqa: E402

from layoutdit_amd import dp, ops, synth                # noqa: E402
from layoutdit_amd.config import DiTConfig              # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel   # noqa: E402
from layoutdit_amd.training import DetectorTrainStep    # noqa: E402
from tests import ema_oracle as eo                      # noqa: E402
from tests import optim_oracle as oo                    # noqa: E402
from tests import rpn_train_oracle as to                # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
PAD, SENTINEL = 8, 12345.0
LR, WD, SCALE = 1e-2, 0.01, 1024.0
F = {n: i for i, n in enumerate(oo.FIELDS)}


class Padded:
    """Views that sit PAD sentinels inside parents of their own; ``off`` may put one a single element off the 16-byte grid."""

    def __init__(self):
        self.parents = []

    def view(self, n, dtype=torch.float32, off=PAD):
        parent = torch.full((n + 2 * PAD + 1,), SENTINEL, dtype=dtype, device=DEV)
        self.parents.append((parent, off, n))
        return parent[off: off + n]

    def snapshot(self):
        """Every parent as its bits (a NaN must compare equal to itself)."""
        return [t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int16) for t, _, _ in self.parents]

    def sentinels_intact(self):
        for parent, off, n in self.parents:
            edge = torch.cat([parent[:off], parent[off + n:]])
            if not bool((edge == torch.full((), SENTINEL, dtype=parent.dtype, device=DEV)).all()):
                return False
        return True


# ---- the update against the oracle --------------------------------------------------------------------------------------------------
ALL_OFF, SHADOW_OFF, NO_SHADOW = 1, 2, 3


class Problem(Padded):
    """Segments in the style of tests/test_gpu_detector_step.py::Problem, each with an fp32 shadow: lengths 0, 1, 3, 4, 5, 1023, 1024,
    1025, one of 2049 with a bf16 mirror, one of 1030 that lies one element off the 16-byte grid entirely (shadow included), one of
    1030 whose shadow ALONE does, one of 1027 without a shadow, tiny ones up to ops.EMA_MAX_SEGMENTS + 1 non-empty segments (a second
    launch) and 4099 last.  ``ema=False``: the same tensors without shadows, for the twin that runs ops.adamw_multi."""

    def __init__(self, seed=0, ema=True):
        super().__init__()
        rng = np.random.RandomState(seed)
        spec = [(0, 0, False), (1, 0, False), (3, 0, False), (4, 0, False), (5, 0, False), (1023, 0, False), (1024, 0, False), (1025, 0, False),
                (2049, 0, True), (1030, ALL_OFF, False), (1030, SHADOW_OFF, False), (1027, NO_SHADOW, False), (7, ALL_OFF, True)]
        tiny = [1, 2, 3, 5, 7]
        while sum(1 for n, _, _ in spec if n) < ops.EMA_MAX_SEGMENTS:
            spec.append((tiny[len(spec) % 5], 0, False))
        spec.append((4099, 0, False))
        assert sum(1 for n, _, _ in spec if n) == ops.EMA_MAX_SEGMENTS + 1
        self.spec = spec
        self.p, self.g, self.m, self.v, self.mirror, self.e, self.p0 = [], [], [], [], [], [], []
        for n, kind, mirrored in spec:
            off = PAD + (1 if kind == ALL_OFF else 0)
            p0 = rng.normal(0, 1, size=n).astype(np.float32)
            self.p0.append(p0)
            p, g, m, v = (self.view(n, off=off) for _ in range(4))
            p.copy_(torch.from_numpy(p0))
            for t in (g, m, v):
                t.zero_()
            self.p.append(p), self.g.append(g), self.m.append(m), self.v.append(v)
            self.mirror.append(self.view(n, BF, off=off) if mirrored else None)
            e = None
            if ema and kind != NO_SHADOW:
                e = self.view(n, off=PAD + 1 if kind in (ALL_OFF, SHADOW_OFF) else PAD)
                e.copy_(p)                                                                # a clone of the parameter before its first update
            self.e.append(e)
        assert self.p[9].data_ptr() % 16 == 4 and self.p[10].data_ptr() % 16 == 0 and self.p[0].data_ptr() % 16 == 0
        if ema:
            assert self.e[9].data_ptr() % 16 == 4 and self.e[10].data_ptr() % 16 == 4 and self.e[8].data_ptr() % 16 == 0 and self.e[11] is None
        self.state = ops.new_opt_state(DEV, scale=SCALE, lr=LR)

    def set_grads(self, grads, scale):
        for g, h in zip(self.g, grads):
            g.copy_(torch.from_numpy(h) * scale)

    def _front(self, growth_interval):
        ops.grads_check_multi(self.g, self.state)
        ops.opt_advance(self.state, (0.9, 0.999), 2.0, 0.5, growth_interval)

    def apply(self, growth_interval=2000):
        self._front(growth_interval)
        ops.adamw_multi(self.p, self.g, self.m, self.v, self.state, (0.9, 0.999), 1e-8, WD, 1.0, self.mirror)

    def apply_ema(self, decay, warmup=True, growth_interval=2000):
        """The plain step's call: (1, weight_decay) per segment and no clip block."""
        self._front(growth_interval)
        ops.adamw_ema_groups_multi(self.p, self.g, self.m, self.v, self.state, [1.0] * len(self.p), [WD] * len(self.p), self.e, decay, warmup,
                                   None, (0.9, 0.999), 1e-8, self.mirror)

    def read_state(self):
        host = self.state.cpu()
        hf = host.view(torch.float32)
        return {n: (int(host[i]) if i < 5 else float(hf[i])) for n, i in F.items()}


def _grads(seed, prob):
    rng = np.random.RandomState(seed)
    return [rng.normal(0, 0.1, size=n).astype(np.float32) for n, _, _ in prob.spec]


def _errors(pairs):
    """(max |got - want|, max |cpu - want|) over (got, cpu fp32, float64 want) triples."""
    a = max(float(np.abs(got.astype(np.float64) - want).max()) for got, _, want in pairs)
    b = max(float(np.abs(cpu.astype(np.float64) - want).max()) for _, cpu, want in pairs)
    return a, b


def test_update_matches_the_float64_oracle_within_twice_torch_lerp_and_is_adamw_multi_beside_it():
    prob, twin = Problem(ema=True), Problem(ema=False)
    live = [i for i, (n, kind, _) in enumerate(prob.spec) if n and kind != NO_SHADOW]
    e64 = {i: prob.p0[i].astype(np.float64) for i in live}
    e32 = {i: torch.from_numpy(prob.p0[i].copy()) for i in live}
    for step in range(5):
        grads = _grads(100 + step, prob)                                              # fresh inputs every step, nothing fed back
        prob.set_grads(grads, SCALE)
        twin.set_grads(grads, SCALE)
        prob.apply_ema(0.9)
        twin.apply()
        w = eo.ema_weight(step + 1, 0.9)                                              # all five under the warmup: 1 - (2 + step) / (11 + step)
        assert w == float(np.float32(1.0 - (2.0 + step) / (11.0 + step)))
        for i in live:
            p = prob.p[i].cpu()                                                        # the same per-step p and w for all three
            e64[i] = eo.ema(e64[i], p.numpy(), 1.0 - w)
            e32[i].lerp_(p, w)
    torch.cuda.synchronize()
    assert prob.read_state() == twin.read_state() and prob.read_state()["step"] == 5
    a, b = _errors([(prob.e[i].cpu().numpy(), e32[i].numpy(), e64[i]) for i in live])
    print(f"shadow: kernel max error vs float64 {a:.4e}, torch.Tensor.lerp_ (fp32, CPU) {b:.4e}, ratio {a / b:.3f}")
    assert a <= 2.0 * b
    for i, (n, kind, _) in enumerate(prob.spec):
        what = f"segment {i} (n = {n}, kind {kind})"
        assert torch.equal(prob.p[i], twin.p[i]) and torch.equal(prob.m[i], twin.m[i]) and torch.equal(prob.v[i], twin.v[i]), what
        if prob.mirror[i] is not None:
            assert torch.equal(prob.mirror[i], twin.mirror[i]) and torch.equal(prob.mirror[i], prob.p[i].to(BF)), what
        if n:
            assert not torch.equal(prob.p[i].cpu(), torch.from_numpy(prob.p0[i])), what                  # the null-shadow segment moved too
    assert prob.sentinels_intact() and twin.sentinels_intact()


def test_skipped_step_moves_no_shadow_and_does_not_age_the_warmup():
    DECAY = 0.9999                                                                        # far above the warmup's value: the warmup decides
    prob = Problem(seed=1)
    for step in range(2):
        prob.set_grads(_grads(7 + step, prob), SCALE)
        prob.apply_ema(DECAY)
    grads = _grads(20, prob)
    assert prob.spec[-1][0] == 4099
    grads[-1][-1] = np.nan
    prob.set_grads(grads, SCALE)
    before = prob.snapshot()
    prob.apply_ema(DECAY)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, prob.snapshot()))              # p, m, v, mirrors, shadows (and g): not a bit
    got = prob.read_state()
    assert (got["step"], got["skipped_steps"], got["skip"], got["scale"]) == (2, 1, 1, SCALE / 2)
    # the next taken step is the THIRD taken one: d = 4 / 13, not the 5 / 14 of a host that counted calls
    prob.set_grads(_grads(21, prob), SCALE / 2)
    e_before = [None if e is None else e.cpu().numpy().astype(np.float64) for e in prob.e]
    prob.apply_ema(DECAY)
    torch.cuda.synchronize()
    got = prob.read_state()
    assert (got["step"], got["skipped_steps"], got["skip"]) == (3, 1, 0)
    d3, d4 = eo.ema_decay_at(3, DECAY), eo.ema_decay_at(4, DECAY)
    assert (d3, d4) == (4 / 13, 5 / 14)
    told_apart = 0.0
    for i, (n, kind, _) in enumerate(prob.spec):
        if not n or prob.e[i] is None:
            continue
        p = prob.p[i].cpu().numpy().astype(np.float64)
        want = eo.ema(e_before[i], p, 1.0 - eo.ema_weight(3, DECAY))
        # one subtraction, one multiplication and one addition in fp32 on |values| < 8: within 1.5 ulp of 8, 4 allowed
        np.testing.assert_allclose(prob.e[i].cpu().numpy().astype(np.float64), want, rtol=0, atol=4 * float(np.spacing(np.float32(4.0))))
        told_apart = max(told_apart, float(np.abs(eo.ema(e_before[i], p, d4) - want).max()))
    assert told_apart > 20 * 4 * float(np.spacing(np.float32(4.0)))                      # the other count would have been seen
    assert prob.sentinels_intact()


def test_no_warmup_uses_the_decay_itself():
    prob = Problem(seed=2)
    prob.set_grads(_grads(5, prob), SCALE)
    prob.apply_ema(0.75, warmup=False)
    torch.cuda.synchronize()
    for i, (n, kind, _) in enumerate(prob.spec):
        if n and prob.e[i] is not None:
            want = eo.ema(prob.p0[i], prob.p[i].cpu().numpy(), 0.75)
            np.testing.assert_allclose(prob.e[i].cpu().numpy().astype(np.float64), want, rtol=0, atol=4 * float(np.spacing(np.float32(4.0))))


# ---- the exchange ---------------------------------------------------------------------------------------------------------------------
SPECIALS = (0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x00000001)       # -0.0, +-inf, two NaNs with payloads, a denormal


def _as_i32(x):
    return x - (1 << 32) if x >= (1 << 31) else x


class SwapProblem(Padded):
    """Pairs of lengths 0, 1, 3, 4, 5, 1023, 1024, 1025, 2049 with a mirror, 1030 one element off the grid on every side (mirror
    included), 1030 with b ALONE off the grid, tiny ones up to ops.SWAP_MAX_SEGMENTS + 1 non-empty pairs and 4099 with a mirror last;
    the special bit patterns planted at the head, in the quads' body and in the last elements of both sides."""

    def __init__(self, seed=3):
        super().__init__()
        rng = np.random.RandomState(seed)
        spec = [(0, 0, False), (1, 0, False), (3, 0, False), (4, 0, False), (5, 0, True), (1023, 0, False), (1024, 0, False), (1025, 0, True),
                (2049, 0, True), (1030, ALL_OFF, True), (1030, SHADOW_OFF, False)]
        tiny = [1, 2, 3, 5, 7]
        while sum(1 for n, _, _ in spec if n) < ops.SWAP_MAX_SEGMENTS:
            spec.append((tiny[len(spec) % 5], 0, False))
        spec.append((4099, 0, True))
        assert sum(1 for n, _, _ in spec if n) == ops.SWAP_MAX_SEGMENTS + 1
        self.spec, self.a, self.b, self.mirror = spec, [], [], []
        for n, kind, mirrored in spec:
            a = self.view(n, off=PAD + (1 if kind == ALL_OFF else 0))
            b = self.view(n, off=PAD + (1 if kind in (ALL_OFF, SHADOW_OFF) else 0))
            for t, shift in ((a, 0), (b, 3)):
                t.copy_(torch.from_numpy(rng.normal(0, 1, size=n).astype(np.float32)))
                bits = t.view(torch.int32)
                for k, s in enumerate(SPECIALS):
                    for at in (k + shift, n // 2 + k + shift, n - 1 - k - shift):
                        if 0 <= at < n:
                            bits[at] = _as_i32(s)
            self.a.append(a), self.b.append(b)
            self.mirror.append(self.view(n, BF, off=PAD + (1 if kind == ALL_OFF else 0)) if mirrored else None)
        assert self.a[9].data_ptr() % 16 == 4 and self.mirror[9].data_ptr() % 8 == 2 and self.a[10].data_ptr() % 16 == 0 and self.b[10].data_ptr() % 16 == 4


def _bits(t):
    return t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _is_bf16_of(mirror, a):
    """mirror == bf16(a): bit for bit where a is a number, a NaN where a is one (which NaN the conversion makes is not pinned)."""
    want = a.to(BF)
    nan = torch.isnan(a)
    return bool((torch.isnan(mirror) == nan).all()) and torch.equal(_bits(mirror)[~nan], _bits(want)[~nan])


def test_swap_moves_bits_writes_the_mirror_and_undoes_itself():
    prob = SwapProblem()
    a0, b0 = [_bits(t) for t in prob.a], [_bits(t) for t in prob.b]
    planted = sum(int((_bits(t) == _as_i32(SPECIALS[3])).sum()) for t in prob.a + prob.b)
    assert planted > 20 and bool(torch.isnan(prob.a[-1]).any()) and bool(torch.isinf(prob.b[-1]).any())
    start = prob.snapshot()
    ops.swap_multi(prob.a, prob.b, prob.mirror)                                       # capacity + 1 pairs: the last one rides in a second launch
    torch.cuda.synchronize()
    for i, (n, kind, _) in enumerate(prob.spec):
        what = f"pair {i} (n = {n}, kind {kind})"
        assert torch.equal(_bits(prob.a[i]), b0[i]) and torch.equal(_bits(prob.b[i]), a0[i]), what
        if prob.mirror[i] is not None:
            assert _is_bf16_of(prob.mirror[i], prob.a[i]), what                          # bits: -0.0 keeps its sign
    assert prob.sentinels_intact()
    ops.swap_multi(prob.a, prob.b, prob.mirror)
    torch.cuda.synchronize()
    for (parent, _, _), was, now in zip(prob.parents, start, prob.snapshot()):
        if parent.dtype == torch.float32:
            assert torch.equal(was, now)                                                # every fp32 parent bit for bit, sentinels included
    for i, mi in enumerate(prob.mirror):
        if mi is not None:
            assert torch.equal(_bits(prob.a[i]), a0[i]) and _is_bf16_of(mi, prob.a[i])
    assert prob.sentinels_intact()
    ops.swap_multi(prob.a, prob.b)                                                    # without mirrors: they keep what they held
    held = [None if mi is None else _bits(mi) for mi in prob.mirror]
    ops.swap_multi(prob.a, prob.b)
    torch.cuda.synchronize()
    assert all(mi is None or torch.equal(_bits(mi), h) for mi, h in zip(prob.mirror, held))
    assert all(torch.equal(_bits(t), x) for t, x in zip(prob.a, a0)) and prob.sentinels_intact()
    ops.swap_multi([], [])
    empty = torch.zeros(0, device=DEV)
    ops.swap_multi([empty], [empty])


# ---- the detector --------------------------------------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _cfg():
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    return cfg


def _model(compute_dtype="bf16", qat=False, train=True):
    """The smallest detector of tests/test_gpu_detector_step.py, identically initialised every time."""
    cfg = _cfg()
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, compute_dtype=compute_dtype, qat=qat)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    return model.to(DEV).train() if train else model.to(DEV).eval()


def _encoder(model):
    return model.model.backbone.backbone.dit


@pytest.fixture(scope="module")
def batch():
    images = [torch.from_numpy(synth.synth_images(1, 120, 200, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 224, 224, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV),
                "labels": torch.tensor([1, 3], device=DEV)},
               {"boxes": torch.from_numpy(np.ascontiguousarray(to.scene(7, 7))).to(DEV),
                "labels": torch.from_numpy(np.arange(7, dtype=np.int64) % 5 + 1).to(DEV)}]
    return images, targets


@pytest.fixture(scope="module")
def pages():
    return torch.from_numpy(synth.synth_images(2, 224, 224, seed=31, kind="uniform")).to(DEV)


def _backward(model, batch, scale):
    for p in model.parameters():
        p.grad = None
    losses = model.losses(*batch, generator=_seeded(2))
    (sum(losses.values()) * scale).backward()
    return losses


def _copy_state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_ema_state_dict_is_the_recurrence_over_the_models_weights(batch):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE, ema_decay=0.5)
    initial = _copy_state(model)
    e64 = {k: v.double().cpu().numpy() for k, v in initial.items()}
    e32 = {k: v.cpu().clone() for k, v in initial.items()}
    had_grad = None
    for k in range(1, 5):
        step.step(*batch, generator=_seeded(1 + k))
        with_grad = {n for n, p in model.named_parameters() if p.grad is not None}
        had_grad = with_grad if had_grad is None else had_grad
        assert with_grad == had_grad
        w = eo.ema_weight(k, 0.5)                                                      # 2/11, 3/12, 4/13, 5/14: the warmup, below 0.5
        assert w == float(np.float32(1.0 - (1.0 + k) / (10.0 + k)))
        now = model.state_dict()
        for n in had_grad:
            p = now[n].detach().cpu()
            e64[n] = eo.ema(e64[n], p.numpy(), 1.0 - w)
            e32[n].lerp_(p, w)
    torch.cuda.synchronize()
    assert (step.steps, step.skipped_steps) == (4, 0) and len(had_grad) > 60 and any("dit" in n for n in had_grad)
    got = step.ema_state_dict()
    now = model.state_dict()
    assert set(got) == set(now)
    a, b = _errors([(got[n].cpu().numpy(), e32[n].numpy(), e64[n]) for n in had_grad])
    print(f"ema_state_dict over {len(had_grad)} tensors: max error vs float64 {a:.4e}, torch.Tensor.lerp_ (fp32, CPU) {b:.4e}, ratio {a / b:.3f}")
    assert a <= 2.0 * b
    params = {n for n, _ in model.named_parameters()}
    untouched = [k for k in now if k not in had_grad]
    assert any(k in params for k in untouched)                                           # the encoder's inert mask token, for one
    for k in untouched:                                                                  # no gradient ever, and buffers: the model's own
        assert torch.equal(got[k], now[k]) and torch.equal(got[k], initial[k]), k
    for n in had_grad:
        assert not torch.equal(got[n], now[n]) and not torch.equal(got[n], initial[n]), n
        assert got[n].data_ptr() != now[n].data_ptr()
    fresh = _model()
    fresh.load_state_dict(got)
    assert _same(_copy_state(fresh), got)


@pytest.mark.parametrize("compute_dtype,qat", [("bf16", False), ("mxfp8", True)])
def test_ema_weights_evaluates_on_the_average_and_restores_every_bit(batch, pages, compute_dtype, qat):
    model, never = _model(compute_dtype, qat), _model(compute_dtype, qat)
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE, ema_decay=0.5)
    twin = DetectorTrainStep(never, lr=1e-3, init_scale=SCALE, ema_decay=0.5)
    for k in (2, 3):
        step.step(*batch, generator=_seeded(k))
        twin.step(*batch, generator=_seeded(k))
    assert step.steps == 2
    average = step.ema_state_dict()
    fresh = _model(compute_dtype, qat=False, train=False)                                # mxfp8: the inference build
    fresh.load_state_dict(average)
    want = [t.clone() for t in fresh.forward_padded(pages)]
    st = _encoder(model)._flat_state
    assert not st._dirty and st._packed_version == st.version()
    weights, mirror = _copy_state(model), st.packed.clone()
    with step.ema_weights() as inside:
        assert inside is model and not model.training
        got = [t.clone() for t in model.forward_padded(pages)]
        assert _same(_copy_state(model), average)
        assert _same(step.ema_state_dict(), average)
        for call in (lambda: step.step(*batch), step.apply, step.state_dict, lambda: step.load_state_dict({})):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with step.ema_weights():
                pass
    torch.cuda.synchronize()
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    own = [t.clone() for t in model.eval().forward_padded(pages)]
    assert not all(torch.equal(g, o) for g, o in zip(got, own))                          # the average is not the weights
    model.train()
    assert model.training and _same(_copy_state(model), weights)
    assert torch.equal(st.packed, mirror) and st is _encoder(model)._flat_state
    assert _same(step.ema_state_dict(), average)
    la, lb = step.step(*batch, generator=_seeded(9)), twin.step(*batch, generator=_seeded(9))
    torch.cuda.synchronize()
    assert all(torch.equal(la[k], lb[k]) for k in la)
    assert _same(_copy_state(model), _copy_state(never)) and _same(step.ema_state_dict(), twin.ema_state_dict())
    assert torch.equal(step._state, twin._state)


def test_a_folding_call_leaves_the_shadows_alone(batch):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE, accumulate=2, ema_decay=0.5)
    initial = _copy_state(model)
    step.step(*batch, generator=_seeded(2))
    torch.cuda.synchronize()
    assert step.pending_micro_batches == 1 and len(step._ema) > 60                       # made where the moments are made: at first sight
    assert all(torch.equal(e, initial[n]) for n, e in step._ema.items())
    assert _same(step.ema_state_dict(), initial)
    with pytest.raises(RuntimeError, match="micro-batches"):
        with step.ema_weights():
            pass
    step.step(*batch, generator=_seeded(3))
    torch.cuda.synchronize()
    assert (step.pending_micro_batches, step.steps) == (0, 1)
    now, got = model.state_dict(), step.ema_state_dict()
    w = eo.ema_weight(1, 0.5)
    for n in step._ema:
        assert not torch.equal(got[n], initial[n]), n
        want = eo.ema(initial[n].cpu().numpy(), now[n].cpu().numpy(), 1.0 - w)
        peak = float(np.abs(want).max())
        np.testing.assert_allclose(got[n].cpu().numpy().astype(np.float64), want, rtol=0, atol=2 * float(np.spacing(np.float32(peak))), err_msg=n)


def test_apply_with_ema_is_graph_capturable(batch):
    eager_model, graph_model = _model(), _model()
    _backward(eager_model, batch, SCALE)
    _backward(graph_model, batch, SCALE)
    eager = DetectorTrainStep(eager_model, lr=1e-3, weight_decay=0.01, init_scale=SCALE, ema_decay=0.9)
    for _ in range(3):
        eager.apply()
    captured = DetectorTrainStep(graph_model, lr=1e-3, weight_decay=0.01, init_scale=SCALE, ema_decay=0.9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.apply()                                                                # the first of the three: eager, makes moments and shadows
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.apply()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    captured.invalidate_caches()
    assert (eager.steps, captured.steps) == (3, 3)
    assert _same(_copy_state(eager_model), _copy_state(graph_model))
    ma, mb = eager.state_dict(), captured.state_dict()
    assert _same(ma["exp_avg"], mb["exp_avg"]) and _same(ma["exp_avg_sq"], mb["exp_avg_sq"])
    assert len(ma["ema"]["shadow"]) > 60 and _same(ma["ema"]["shadow"], mb["ema"]["shadow"])
    assert torch.equal(eager._state, captured._state)
    assert not _same(ma["ema"]["shadow"], {n: eager_model.state_dict()[n] for n in ma["ema"]["shadow"]})


def test_state_round_trip_carries_the_shadows(batch):
    first, second, third = _model(), _model(), _model()
    a = DetectorTrainStep(first, lr=1e-3, weight_decay=0.01, init_scale=SCALE, ema_decay=0.5)
    a.step(*batch, generator=_seeded(2))
    a.step(*batch, generator=_seeded(3))
    sd = copy.deepcopy(a.state_dict())
    assert sd["state"]["step"] == 2 and sd["ema"]["ema_decay"] == 0.5 and sd["ema"]["ema_warmup"] is True
    assert set(sd["ema"]["shadow"]) == set(sd["exp_avg"]) and any("dit" in k for k in sd["ema"]["shadow"])
    second.load_state_dict(first.state_dict())
    third.load_state_dict(first.state_dict())
    b = DetectorTrainStep(second, lr=5.0, weight_decay=0.01, ema_decay=0.25, ema_warmup=False)
    b.load_state_dict(sd)
    assert (b.ema_decay, b.ema_warmup) == (0.5, True)
    assert _same(b.ema_state_dict(), a.ema_state_dict())                               # loaded values count before any update bound them
    # without the entry: it loads, and the shadows are the parameters as they are when first needed
    c = DetectorTrainStep(third, lr=1e-3, weight_decay=0.01, ema_decay=0.5)
    c.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
    assert _same(c.ema_state_dict(), _copy_state(third))
    with pytest.raises(KeyError, match="moving averages"):
        bad = dict(sd, ema=dict(sd["ema"], shadow=dict(sd["ema"]["shadow"], no_such_parameter=torch.zeros(1))))
        DetectorTrainStep(_model(), ema_decay=0.5).load_state_dict(bad)
    resumed = _copy_state(third)
    la, lb, lc = (s.step(*batch, generator=_seeded(4)) for s in (a, b, c))
    torch.cuda.synchronize()
    assert all(torch.equal(la[k], lb[k]) and torch.equal(la[k], lc[k]) for k in la)
    assert _same(_copy_state(first), _copy_state(second)) and _same(_copy_state(first), _copy_state(third))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["state"] == sb["state"] and sa["state"]["step"] == 3
    assert _same(sa["ema"]["shadow"], sb["ema"]["shadow"]) and _same(a.ema_state_dict(), b.ema_state_dict())
    # c's average restarted at the resumed weights and took the third taken step's weight
    now, got = third.state_dict(), c.ema_state_dict()
    w = eo.ema_weight(3, 0.5)
    for n in sa["ema"]["shadow"]:
        want = eo.ema(resumed[n].cpu().numpy(), now[n].cpu().numpy(), 1.0 - w)
        peak = float(np.abs(want).max())
        np.testing.assert_allclose(got[n].cpu().numpy().astype(np.float64), want, rtol=0, atol=2 * float(np.spacing(np.float32(peak))), err_msg=n)
    # a step built without ema_decay ignores the entry and writes none
    plain = DetectorTrainStep(_model(), lr=1e-3)
    plain.load_state_dict(sd)
    assert "ema" not in plain.state_dict()
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.ema_state_dict()


# ---- two ranks -------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _digests(sd):
    return {k: hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in sd.items()}


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from tests import detector_accum_cases as cases
    r = dp.init(backend="gloo")
    try:
        m = cases.model()
        if rank == 1:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01)
        step = DetectorTrainStep(m, lr=1e-3, init_scale=cases.SCALE, rank=r, ema_decay=0.5)
        out = {"broadcast": _digests(m.state_dict()), "ema": [], "params": []}
        mine = cases.micro_batches()[rank]
        for _ in range(2):
            step.step(*mine, generator=cases.seeded(cases.GEN_SEEDS[rank]))
            torch.cuda.synchronize()
            out["ema"].append(_digests(step.ema_state_dict()))
            out["params"].append(_digests(m.state_dict()))
        out["steps"] = step.steps
        q.put((rank, out, None))
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise
    finally:
        dp.finalize(r)


def test_two_ranks_hold_the_same_average():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(world):
            rank, out, err = q.get(timeout=300)
            assert err is None, f"rank {rank} failed:\n{err}"
            got[rank] = out
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    a, b = got[0], got[1]
    assert a["steps"] == b["steps"] == 2 and a["broadcast"] == b["broadcast"]
    for it in range(2):
        assert a["ema"][it] == b["ema"][it] and a["params"][it] == b["params"][it], it       # nothing exchanged: the same reduced bits
        assert a["ema"][it] != a["params"][it] and a["ema"][it] != a["broadcast"]
    assert a["ema"][0] != a["ema"][1]
