"""The detector's optimizer step on the GPU (csrc/optim_multi.hip through layoutdit_amd.ops and DetectorTrainStep) against the float64
restatement tests/optim_oracle.py and against the reference-style loop (torch.optim.AdamW on unscaled gradients).

Gates: the kernels' p, m, v after five steps err against float64 at most TWICE as much as torch.optim.AdamW in fp32
on the CPU does on the same inputs (the two differ in where lr / (1 - beta1^t) is rounded, tests/test_gpu_train.py); the bf16 mirror is
bf16(p) bit for bit; nothing next to a segment is written; a step with a NaN / infinity changes no bit and only backs the scale off;
one whole detector step agrees with the reference-style loop to 2 ulp of each tensor's largest parameter (the fused-vs-torch first-step
bound); eval after a step sees the new weights; apply() replays from a graph bit for bit; the state resumes bit for bit."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import ops, synth                  # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel    # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402
from tests import optim_oracle as oo                  # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
PAD, SENTINEL = 8, 12345.0
LR, WD, SCALE = 1e-2, 0.01, 1024.0
F = {n: i for i, n in enumerate(oo.FIELDS)}


# ---- the kernels against the oracle ------------------------------------------------------------------------------------------------
class Problem:
    """Segments of lengths 5, 0, 1, 3, 4, 1023, 1024, 1025, one of 1030 that starts one element into its parent (4-byte aligned
    pointers), one of 2049 with a bf16 mirror, tiny ones (one misaligned WITH a mirror, one whose exp_avg alone is misaligned) up to
    ops.OPT_MAX_SEGMENTS + 1 non-empty segments, and 4099 last.  Every tensor sits PAD sentinels inside its own parent."""

    def __init__(self, seed=0):
        rng = np.random.RandomState(seed)
        spec = [(5, 0, False), (0, 0, False), (1, 0, False), (3, 0, False), (4, 0, False), (1023, 0, False), (1024, 0, False), (1025, 0, False),
                (1030, 1, False), (2049, 0, True), (7, 1, True), (6, 2, False)]
        tiny = [1, 2, 3, 5, 7]
        while sum(1 for n, _, _ in spec if n) < ops.OPT_MAX_SEGMENTS:
            spec.append((tiny[len(spec) % 5], 0, False))
        spec.append((4099, 0, False))
        assert sum(1 for n, _, _ in spec if n) == ops.OPT_MAX_SEGMENTS + 1
        self.spec, self.parents = spec, []
        self.p, self.g, self.m, self.v, self.mirror, self.p0 = [], [], [], [], [], []
        for n, shift, mirrored in spec:
            def view(dtype=torch.float32, off=PAD + (shift if shift == 1 else 0)):
                parent = torch.full((n + 2 * PAD + 1,), SENTINEL, dtype=dtype, device=DEV)
                self.parents.append((parent, off, n))
                return parent[off: off + n]
            p0 = rng.normal(0, 1, size=n).astype(np.float32)
            self.p0.append(p0)
            p, g, v = view(), view(), view()
            m = view(off=PAD + 1) if shift else view()                                   # shift 2: exp_avg alone off the 16-byte grid
            p.copy_(torch.from_numpy(p0))
            m.zero_()
            v.zero_()
            g.zero_()
            self.p.append(p), self.g.append(g), self.m.append(m), self.v.append(v)
            self.mirror.append(view(BF) if mirrored else None)
        assert self.p[8].data_ptr() % 16 == 4 and self.p[0].data_ptr() % 16 == 0 and self.m[11].data_ptr() % 16 == 4 and self.p[11].data_ptr() % 16 == 0
        self.state = ops.new_opt_state(DEV, scale=SCALE, lr=LR)

    def set_grads(self, grads, scale):
        for g, h in zip(self.g, grads):
            g.copy_(torch.from_numpy(h) * scale)

    def apply(self, growth_interval=2000):
        ops.grads_check_multi(self.g, self.state)
        ops.opt_advance(self.state, (0.9, 0.999), 2.0, 0.5, growth_interval)
        ops.adamw_multi(self.p, self.g, self.m, self.v, self.state, (0.9, 0.999), 1e-8, WD, 1.0, self.mirror)

    def read_state(self):
        host = self.state.cpu()
        hf = host.view(torch.float32)
        return {n: (int(host[i]) if i < 5 else float(hf[i])) for n, i in F.items()}

    def snapshot(self):
        """Every parent as its bits (a NaN gradient must compare equal to itself)."""
        return [t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int16) for t, _, _ in self.parents]

    def sentinels_intact(self):
        for parent, off, n in self.parents:
            edge = torch.cat([parent[:off], parent[off + n:]])
            if not bool((edge == torch.full((), SENTINEL, dtype=parent.dtype, device=DEV)).all()):
                return False
        return True


def _grads(seed, prob):
    rng = np.random.RandomState(seed)
    return [rng.normal(0, 0.1, size=n).astype(np.float32) for n, _, _ in prob.spec]


def test_kernels_match_the_float64_oracle_within_twice_torch_adamw():
    prob = Problem()
    st = oo.new_state(scale=SCALE, lr=LR)
    ref = [(p0.astype(np.float64), np.zeros(len(p0)), np.zeros(len(p0))) for p0 in prob.p0]
    cpu = [torch.nn.Parameter(torch.from_numpy(p0.copy())) for p0 in prob.p0]
    opt = torch.optim.AdamW(cpu, lr=LR, weight_decay=WD, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for step in range(5):
        grads = _grads(100 + step, prob)                                              # fresh inputs every step, nothing fed back
        prob.set_grads(grads, SCALE)
        prob.apply()
        st = oo.advance(oo.check(st, grads))
        ref = [oo.adamw(p, g.astype(np.float64) * SCALE, m, v, st, weight_decay=WD) for (p, m, v), g in zip(ref, grads)]
        for q, g in zip(cpu, grads):
            q.grad = torch.from_numpy(g.copy())                                       # pre-unscaled
        opt.step()
    torch.cuda.synchronize()
    got = prob.read_state()
    assert (got["step"], got["skipped_steps"], got["growth_tracker"], got["scale"], got["found_inf"], got["skip"]) == (5, 0, 5, SCALE, 0, 0)
    assert got["bc1"] == float(np.float32(st["bc1"])) and got["bc2_sqrt"] == float(np.float32(st["bc2_sqrt"]))
    err = {"p": [0.0, 0.0], "m": [0.0, 0.0], "v": [0.0, 0.0]}
    for i, (n, _, _) in enumerate(prob.spec):
        if n == 0:
            continue
        mine = {"p": prob.p[i], "m": prob.m[i], "v": prob.v[i]}
        theirs = {"p": cpu[i].detach(), "m": opt.state[cpu[i]]["exp_avg"], "v": opt.state[cpu[i]]["exp_avg_sq"]}
        for k, want in zip("pmv", ref[i]):
            err[k][0] = max(err[k][0], float(np.abs(mine[k].cpu().numpy().astype(np.float64) - want).max()))
            err[k][1] = max(err[k][1], float(np.abs(theirs[k].numpy().astype(np.float64) - want).max()))
    for k, (a, b) in err.items():
        print(f"{k}: kernel max error vs float64 {a:.4e}, torch.optim.AdamW (fp32, CPU) {b:.4e}, ratio {a / b:.3f}")
    for k, (a, b) in err.items():
        assert a <= 2.0 * b, k
    for i, mi in enumerate(prob.mirror):
        if mi is not None:
            assert torch.equal(mi, prob.p[i].to(BF)), f"mirror of segment {i}"
    assert prob.sentinels_intact()


@pytest.mark.parametrize("where", ["nan_last_element_of_last_segment", "inf_in_scalar_tail_of_first_segment"])
def test_non_finite_gradient_skips_the_step_and_backs_the_scale_off(where):
    prob = Problem(seed=1)
    grads = _grads(7, prob)
    if where.startswith("nan"):
        assert prob.spec[-1][0] == 4099
        grads[-1][-1] = np.nan
    else:
        assert prob.spec[0][0] == 5
        grads[0][4] = np.inf                                                          # element 4 of 5: behind the one full quad
    prob.set_grads(grads, SCALE)
    before = prob.snapshot()
    prob.apply()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, prob.snapshot()))            # p, m, v, mirrors (and g): not a bit
    got = prob.read_state()
    assert (got["step"], got["scale"], got["growth_tracker"], got["skipped_steps"], got["skip"], got["found_inf"]) == (0, SCALE / 2, 0, 1, 1, 0)
    # the next clean step is step 1 (its bias corrections), made with the halved scale
    grads = _grads(8, prob)
    prob.set_grads(grads, SCALE / 2)
    prob.apply(growth_interval=2)
    st = oo.new_state(scale=SCALE / 2, lr=LR)
    st = oo.advance(st, growth_interval=2)
    got = prob.read_state()
    assert (got["step"], got["skip"], got["growth_tracker"], got["scale"]) == (1, 0, 1, SCALE / 2)
    assert got["bc1"] == float(np.float32(1.0 - 0.9)) and got["bc2_sqrt"] == float(np.float32(np.sqrt(1.0 - 0.999)))
    for i, (n, _, _) in enumerate(prob.spec):
        want, _, _ = oo.adamw(prob.p0[i].astype(np.float64), grads[i].astype(np.float64) * (SCALE / 2), np.zeros(n), np.zeros(n), st, weight_decay=WD)
        # fp32 evaluation of a handful of operations on |p| < 8: a few ulp of 8; the step-2 corrections would be off by ~LR / 2
        np.testing.assert_allclose(prob.p[i].cpu().numpy(), want, rtol=0, atol=4e-6)
    # growth_interval = 2: the second clean step in a row doubles the scale
    prob.set_grads(_grads(9, prob), SCALE / 2)
    prob.apply(growth_interval=2)
    got = prob.read_state()
    assert (got["step"], got["scale"], got["growth_tracker"], got["skipped_steps"]) == (2, SCALE, 0, 1)
    assert prob.sentinels_intact()


# ---- the detector --------------------------------------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _cfg():
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    return cfg


def _model(compute_dtype="f32"):
    """The smallest detector of tests/test_gpu_roi_train.py, identically initialised every time."""
    cfg = _cfg()
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, compute_dtype=compute_dtype)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    return model.to(DEV).train()


@pytest.fixture(scope="module")
def batch():
    images = [torch.from_numpy(synth.synth_images(1, 120, 200, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 224, 224, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV),
                "labels": torch.tensor([1, 3], device=DEV)},
               {"boxes": torch.from_numpy(np.ascontiguousarray(to.scene(7, 7))).to(DEV),
                "labels": torch.from_numpy(np.arange(7, dtype=np.int64) % 5 + 1).to(DEV)}]
    return images, targets


def _backward(model, batch, scale):
    """Gradients of scale * sum(losses) on every parameter, the way DetectorTrainStep.step makes them."""
    for p in model.parameters():
        p.grad = None
    losses = model.losses(*batch, generator=_seeded(2))
    (sum(losses.values()) * scale).backward()
    return losses


def _copy_state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_one_detector_step_equals_the_reference_style_loop(batch):
    """One step of DetectorTrainStep against losses -> sum * scale -> backward -> unscale -> torch.optim.AdamW(model.parameters()):
    every state_dict entry within 2 ulp of that tensor's max |p|, every parameter with a gradient moved, the others untouched.

    Measured on an MI355X: worst difference 1.000 ulp, no tensor over the bound.  The tensors that decide it are the ZERO-INITIALISED
    bias vectors: after one step such a tensor IS its update, lr * m / (sqrt(v) / sqrt(bc2) + eps) ~ lr, so the bound is two ulp of
    the update itself.  Meeting it needs the kernel to round where torch does: lr / bc1 formed in double and rounded once (a float
    division of the block's two floats lands one ulp off torch's step size half the time) and (1 - beta2) * (g * g) with the square
    first as addcmul_ forms it; with a float division and ((1 - beta2) g) g four bias vectors were at 3.00 ulp."""
    a, b = _model(), _model()
    initial = _copy_state(a)
    _backward(a, batch, SCALE)
    with torch.no_grad():
        for p in a.parameters():
            if p.grad is not None:
                p.grad.mul_(1.0 / SCALE)                                                # GradScaler.unscale_
    torch.optim.AdamW(a.parameters(), lr=1e-3, weight_decay=0.0).step()
    step = DetectorTrainStep(b, lr=1e-3, weight_decay=0.0, init_scale=SCALE)
    losses = step.step(*batch, generator=_seeded(2))
    torch.cuda.synchronize()
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    assert all(not v.requires_grad and np.isfinite(v.item()) for v in losses.values())
    assert (step.steps, step.skipped_steps, step.scale) == (1, 0, SCALE)
    sa, sb = a.state_dict(), b.state_dict()
    had_grad = {n for n, p in b.named_parameters() if p.grad is not None}
    assert len(had_grad) > 60
    worst, over = 0.0, []
    for k in sa:
        x, y = sa[k].double(), sb[k].double()
        peak = float(x.abs().max())
        ulp = float(np.spacing(np.float32(peak)))
        diff = float((x - y).abs().max())
        worst = max(worst, diff / ulp if ulp else 0.0)
        if diff > 2.0 * ulp:
            over.append(f"{k}: {diff:.3e} = {diff / ulp:.2f} ulp of max |p| = {peak:.3e}")
        if k in had_grad:
            assert not torch.equal(sb[k], initial[k]), f"{k} had a gradient and did not move"
        else:
            assert torch.equal(sb[k], initial[k]), k
    print(f"fused step vs losses -> backward -> unscale -> torch.optim.AdamW: worst difference {worst:.3f} ulp of a tensor's max |p|; "
          f"{len(over)} of {len(sa)} tensors over 2 ulp:", *over, sep="\n  ")
    assert not over, over


def test_twenty_steps_lower_the_loss(batch):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3)
    history = [step.step(*batch, generator=_seeded(2)) for _ in range(20)]
    totals = [float(sum(v.item() for v in h.values())) for h in history]
    print("summed loss over 20 steps:", [round(v, 4) for v in totals], "steps", step.steps, "skipped", step.skipped_steps, "scale", step.scale)
    assert all(np.isfinite(v.item()) for h in history for v in h.values())
    assert totals[-1] < totals[0]
    assert step.steps + step.skipped_steps == 20 and step.steps > 0


def test_eval_after_a_step_sees_the_new_weights(batch):
    model = _model()
    x = torch.from_numpy(synth.synth_images(2, 224, 224, seed=31, kind="uniform")).to(DEV)
    before = [t.clone() for t in model.eval().forward_padded(x)]                       # fills every cache with the old weights
    model.train()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE)
    step.step(*batch, generator=_seeded(2))
    assert step.steps == 1
    fresh = _model()
    fresh.load_state_dict(model.state_dict())
    after, want = model.eval().forward_padded(x), fresh.eval().forward_padded(x)
    torch.cuda.synchronize()
    for got, ref in zip(after, want):
        assert torch.equal(got, ref)
    assert not all(torch.equal(got, old) for got, old in zip(after, before))
    # the training forward too: the bf16 mirror the update wrote equals a fresh pack of the updated parameters
    model.train(), fresh.train()
    la, lb = model.losses(*batch, generator=_seeded(2)), fresh.losses(*batch, generator=_seeded(2))
    assert all(torch.equal(la[k], lb[k]) for k in la)


def test_apply_is_graph_capturable(batch):
    eager_model, graph_model = _model(), _model()
    _backward(eager_model, batch, SCALE)
    _backward(graph_model, batch, SCALE)
    eager = DetectorTrainStep(eager_model, lr=1e-3, weight_decay=0.01, init_scale=SCALE)
    for _ in range(3):
        eager.apply()
    captured = DetectorTrainStep(graph_model, lr=1e-3, weight_decay=0.01, init_scale=SCALE)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.apply()                                                                # the first of the three: eager, makes the moments
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.apply()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    captured.invalidate_caches()
    assert (eager.steps, captured.steps) == (3, 3)
    sa, sb = eager_model.state_dict(), graph_model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    ma, mb = eager.state_dict(), captured.state_dict()
    assert all(torch.equal(ma["exp_avg_sq"][k], mb["exp_avg_sq"][k]) and torch.equal(ma["exp_avg"][k], mb["exp_avg"][k]) for k in ma["exp_avg"])


def test_state_round_trip_and_step_lr(batch):
    first, second = _model(), _model()
    a = DetectorTrainStep(first, lr=1e-3, weight_decay=0.01, init_scale=SCALE, growth_interval=2, step_size=2, gamma=0.5)
    _backward(first, batch, SCALE)
    a.apply()
    a.apply()                                                                           # two clean steps at interval 2: the scale doubled
    sd = copy.deepcopy(a.state_dict())
    assert sd["state"]["scale"] == 2 * SCALE and sd["state"]["step"] == 2 and set(sd["exp_avg"]) <= set(dict(first.named_parameters()))
    assert "model.roi_heads.box_head.fc6.weight" in sd["exp_avg"] and any("dit" in k for k in sd["exp_avg"])
    second.load_state_dict(first.state_dict())
    b = DetectorTrainStep(second, lr=5.0, step_size=2, gamma=0.5, weight_decay=0.01, growth_interval=2)
    b.load_state_dict(sd)
    _backward(first, batch, 2 * SCALE)
    _backward(second, batch, 2 * SCALE)
    a.apply()
    b.apply()
    torch.cuda.synchronize()
    sa, sb = first.state_dict(), second.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a.state_dict()["state"] == b.state_dict()["state"] and b.lr == 1e-3 and b.steps == 3
    # StepLR(2, 0.5) through a one-element segment with a constant gradient: Adam moves it by the learning rate every step
    p, g = torch.ones(1, device=DEV), torch.full((1,), 3.0 * SCALE, device=DEV)
    m, v = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    c = DetectorTrainStep(_model(), lr=1e-3, step_size=2, gamma=0.5, init_scale=SCALE)
    moved = []
    for _ in range(3):
        c.epoch_end()
        was = p.item()
        ops.opt_advance(c._state)
        ops.adamw_multi([p], [g], [m], [v], c._state)
        moved.append(was - p.item())
    print("one-element segment moved by", moved, "learning rate", c.lr)
    assert moved[0] == pytest.approx(1e-3, rel=1e-3) and moved[1] == pytest.approx(5e-4, rel=1e-3) and moved[2] == pytest.approx(5e-4, rel=1e-3)
    assert c.lr == 5e-4 and c.state_dict()["state"]["lr"] == float(np.float32(5e-4))


def test_refusals():
    with pytest.raises(NotImplementedError, match="TrainStep"):
        DetectorTrainStep(_model("mxfp8"))
    model = _model().eval()
    with pytest.raises(RuntimeError, match="train"):
        DetectorTrainStep(model)
    step = DetectorTrainStep(model.train())
    model.eval()
    with pytest.raises(RuntimeError, match="train"):
        step.apply()
    with pytest.raises(RuntimeError, match="train"):
        step.step([], [])
