"""The detector trained on the quantisation-aware mxfp8 encoder (LayoutDetectionModel(compute_dtype="mxfp8", qat=True) under
DetectorTrainStep) and the one kernel that keeps the step's contract, ldit_requant_train_mirror.

Gates: the kernel's mirror is ldit_pack_train's byte for byte, guard bands intact, a skipped step stores nothing; after apply() the
encoder's training mirror is a fresh pack of the updated masters (default path and clipped + grouped path); one step agrees with the
reference-style loop to 2 ulp of each tensor's largest parameter (section 21's bound); eval after training is the mxfp8 inference
build; the encoder's gradients are those of the pinned straight-through backward; twenty steps lower the loss; apply() replays from a
graph and the state resumes, bit for bit."""
import copy
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, ops, synth                                  # noqa: E402
from layoutdit_amd.config import DiTConfig                                  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel                     # noqa: E402
from layoutdit_amd.training import DetectorTrainStep, detector_param_groups  # noqa: E402
from tests import guarded                                                   # noqa: E402
from tests import rpn_train_oracle as to                                    # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
SCALE = 1024.0
SKIP = _lib.OPT_STATE_FIELDS.index("skip")


# ---- the kernel against the existing pack ------------------------------------------------------------------------------------------
def _lcfg(hidden, mlp, layers):
    return _lib.LditCfg(hidden=hidden, layers=layers, heads=hidden // 64, mlp=mlp, patch=16, in_ch=3, img_h=32, img_w=32, ln_eps=1e-12,
                        n_taps=0, dtype=_lib.DTYPE_MXFP8, flags=0)


def _layout(cfg):
    n_off = 4 + 14 * cfg.layers + 1
    offs = (C.c_int64 * n_off)()
    _lib.check(_lib.load().ldit_flat_param_layout(C.byref(cfg), offs, n_off))
    return list(offs)


def _masters(cfg):
    """master1: plain values.  master2: plain vectors; every matrix made of 32-blocks whose largest element is 1.5 * 2^(e + 8) - block
    scale exponent e before the q fold - with e walking the documented range -124 .. 119, the other elements that times U(-1, 1); then,
    at the head of the first layer's wqkv (rows the q fold covers) and of the LAST layer's w2 (the end of the block): an all-zero
    block, a block of negative zeros, a block whose amax is its single non-zero element, a block mixing both zeros with values."""
    offs = _layout(cfg)
    n = offs[-1]
    rng = np.random.RandomState(cfg.hidden + cfg.mlp + cfg.layers)
    m1 = rng.normal(0, 0.05, size=n).astype(np.float32)
    m2 = rng.normal(0, 0.05, size=n).astype(np.float32)
    Cc, F = cfg.hidden, cfg.mlp
    e_next = 0
    for l in range(cfg.layers):
        o = offs[4 + 14 * l: 4 + 14 * (l + 1)]
        m1[o[3] + Cc: o[3] + 2 * Cc] = 0.0                                           # the key third of the fused bias: no parameter
        m2[o[3] + Cc: o[3] + 2 * Cc] = 0.0
        for start, size in ((o[2], 3 * Cc * Cc), (o[4], Cc * Cc), (o[9], F * Cc), (o[11], Cc * F)):
            nb = size // 32
            e = (np.arange(nb) + e_next) % 244 - 124
            e_next += nb
            blocks = rng.uniform(-1.0, 1.0, size=(nb, 32))
            blocks[np.arange(nb), rng.randint(0, 32, size=nb)] = rng.choice([-1.0, 1.0], size=nb)
            m2[start: start + size] = (blocks * np.ldexp(1.5, e + 8)[:, None]).astype(np.float32).reshape(-1)
    assert np.isfinite(m2).all()
    first, last = offs[4 + 2], offs[4 + 14 * (cfg.layers - 1) + 11]
    for at in (first, last):
        m2[at: at + 32] = 0.0
        m2[at + 32: at + 64] = -0.0
        m2[at + 64: at + 96] = 0.0
        m2[at + 64 + 17] = -3.0e-3
        m2[at + 96: at + 128] = np.tile(np.array([0.0, -0.0, 0.25, -0.5], dtype=np.float32), 8)
    assert np.signbit(m2[first + 32]) and m2[first + 32] == 0.0
    return offs, m1, m2


def _pack(cfg, master, mirror):
    _lib.check(_lib.load().ldit_pack_train(C.byref(cfg), master.data_ptr(), mirror.data_ptr(), mirror.numel(),
                                           torch.cuda.current_stream().cuda_stream))


def _state_block(skip):
    st = ops.new_opt_state(DEV, scale=SCALE, lr=1e-3)
    st[SKIP] = skip
    return st


@pytest.mark.parametrize("hidden,mlp,layers", [(128, 128, 1), (128, 512, 3), (256, 384, 2)])
def test_kernel_remakes_the_mx_operands_of_a_fresh_pack_byte_for_byte(hidden, mlp, layers):
    cfg = _lcfg(hidden, mlp, layers)
    lib = _lib.load()
    offs, m1, m2 = _masters(cfg)
    n = offs[-1]
    nbytes = lib.ldit_train_mirror_bytes(C.byref(cfg))
    assert nbytes > 2 * n
    made = guarded.build({"master1": guarded.In(m1), "master2": guarded.In(m2), "A": guarded.Out((nbytes,), torch.uint8),
                          "B": guarded.Out((nbytes,), torch.uint8), "S": guarded.Out((nbytes,), torch.uint8)}, guarded.POISON, DEV)
    master1, master2, A, B, S = (made[k].view for k in ("master1", "master2", "A", "B", "S"))
    _pack(cfg, master2, A)
    cast = master2.to(BF)                                                            # what the AdamW kernels' mirror write leaves
    for mirror in (B, S):
        _pack(cfg, master1, mirror)
        mirror[: 2 * n].view(BF).copy_(cast)
    torch.cuda.synchronize()
    assert not torch.equal(made["A"].parent, made["B"].parent)
    before = made["S"].parent.clone()
    st = types.SimpleNamespace(mx=True, params=master2, packed=B, lcfg=cfg)
    ops.requant_train_mirror(st)                                                     # state = NULL: it runs
    ops.requant_train_mirror(types.SimpleNamespace(mx=True, params=master2, packed=S, lcfg=cfg), _state_block(1))
    torch.cuda.synchronize()
    assert torch.equal(made["A"].parent, made["B"].parent)                           # the whole byte range, padding included
    assert torch.equal(made["S"].parent, before)                                     # skip = 1: not a bit
    ops.requant_train_mirror(types.SimpleNamespace(mx=True, params=master2, packed=S, lcfg=cfg), _state_block(0))
    torch.cuda.synchronize()
    assert torch.equal(made["S"].parent, made["A"].parent)                           # skip = 0: as with no state block
    for k in ("A", "B", "S"):
        made[k].check_surroundings()
    made["master1"].check_unchanged()
    made["master2"].check_unchanged()
    # the special blocks did what the format says: scale byte 0 and zero codes for the zero blocks, signs kept
    mx0 = (2 * n + 255) // 256 * 256
    assert int(B[mx0:].max()) > 0 and bool((B[2 * offs[4 + 2]: 2 * offs[4 + 2] + 64].view(BF) == 0).all())
    assert bool(torch.signbit(B[: 2 * n].view(BF)[offs[4 + 2] + 32: offs[4 + 2] + 64].float()).all())


# ---- the detector --------------------------------------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _cfg():
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    return cfg


def _model(qat=True):
    """The smallest detector of tests/test_gpu_detector_step.py on the mxfp8 encoder, identically initialised every time."""
    cfg = _cfg()
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, compute_dtype="mxfp8", qat=qat)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    return model.to(DEV).train() if qat else model.to(DEV).eval()


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


def _backward(model, batch, scale):
    for p in model.parameters():
        p.grad = None
    losses = model.losses(*batch, generator=_seeded(2))
    (sum(losses.values()) * scale).backward()
    return losses


def _fresh_pack(st):
    fresh = st.packed.clone()          # (bytes no pack writes keep their values: only what a pack makes is compared)
    _pack(st.lcfg, st.params, fresh)
    return fresh


def _same_mirror(sa, sb):
    """Two models' mirrors agree on every byte a pack writes.  The padding between the mirror's sections is written by nothing and
    holds what its torch.empty found, so the two are not compared raw: b's bytes are laid over a copy of a's padding."""
    over = sa.packed.clone()
    _pack(sa.lcfg, sb.params, over)                      # what a pack writes for b's master, over a's padding
    return torch.equal(sb.packed, _fresh_pack(sb)) and torch.equal(sa.params, sb.params) and torch.equal(over, sa.packed)


def _step_kwargs(model, path):
    if path == "default":
        return {}
    return {"max_grad_norm": 1.0, "param_groups": detector_param_groups(model, layer_decay=0.75)}


@pytest.mark.parametrize("path", ["default", "clipped_grouped"])
def test_apply_keeps_the_training_mirror_a_fresh_pack(batch, path):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE, **_step_kwargs(model, path))
    assert model.qat and _encoder(model).qat
    wq = _encoder(model).encoder.layer[0].attention.attention.query.weight
    initial = wq.detach().clone()
    step.step(*batch, generator=_seeded(2))
    st = _encoder(model)._flat_state
    assert st.mx and st.native and not st._dirty and st._packed_version == st.version()       # the next forward does not repack
    torch.cuda.synchronize()
    assert not torch.equal(wq.detach(), initial)
    assert step.steps == 1 and step.skipped_steps == 0
    assert torch.equal(st.packed, _fresh_pack(st))
    # a step made to skip: masters, moments and mirror keep every bit
    _backward(model, batch, step.scale)
    victim = _encoder(model).encoder.layer[1].intermediate.dense.weight
    victim.grad.view(-1)[5] = float("nan")
    params, mirror = st.params.clone(), st.packed.clone()
    moments = {k: (m.clone(), v.clone()) for k, (m, v) in step._mom.items()}
    others = {k: v.detach().clone() for k, v in model.state_dict().items()}
    step.apply()
    torch.cuda.synchronize()
    assert step.skipped_steps == 1 and step.steps == 1
    assert torch.equal(st.params, params) and torch.equal(st.packed, mirror)
    assert all(torch.equal(step._mom[k][0], m) and torch.equal(step._mom[k][1], v) for k, (m, v) in moments.items())
    assert all(torch.equal(v, others[k]) for k, v in model.state_dict().items())
    assert not st._dirty and torch.equal(st.packed, _fresh_pack(st))


def test_one_step_equals_the_reference_style_loop(batch):
    """losses -> sum * scale -> backward -> unscale -> torch.optim.AdamW -> mark_parameters_changed() against DetectorTrainStep.step on
    the same initial weights and generator seed: every state_dict entry within 2 ulp of that tensor's max |p|."""
    a, b = _model(), _model()
    _backward(a, batch, SCALE)
    with torch.no_grad():
        for p in a.parameters():
            if p.grad is not None:
                p.grad.mul_(1.0 / SCALE)
    torch.optim.AdamW(a.parameters(), lr=1e-3, weight_decay=0.0).step()
    _encoder(a).mark_parameters_changed()
    step = DetectorTrainStep(b, lr=1e-3, weight_decay=0.0, init_scale=SCALE)
    initial = {k: v.detach().clone() for k, v in b.state_dict().items()}
    step.step(*batch, generator=_seeded(2))
    torch.cuda.synchronize()
    assert (step.steps, step.skipped_steps, step.scale) == (1, 0, SCALE)
    sa, sb = a.state_dict(), b.state_dict()
    had_grad = {n for n, p in b.named_parameters() if p.grad is not None}
    assert len(had_grad) > 60 and any("dit" in n for n in had_grad)
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
    print(f"qat detector step vs the reference-style loop: worst difference {worst:.3f} ulp of a tensor's max |p|; "
          f"{len(over)} of {len(sa)} tensors over 2 ulp:", *over, sep="\n  ")
    assert not over, over


def test_eval_after_training_is_the_inference_build(batch):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=SCALE)
    for _ in range(3):
        step.step(*batch, generator=_seeded(2))
    assert step.steps + step.skipped_steps == 3 and step.steps > 0
    x = torch.from_numpy(synth.synth_images(2, 224, 224, seed=31, kind="uniform")).to(DEV)
    inference = _model(qat=False)
    inference.load_state_dict(model.state_dict())
    got, want = model.eval().forward_padded(x), inference.forward_padded(x)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    untrained = _model(qat=False).forward_padded(x)
    assert not all(torch.equal(g, u) for g, u in zip(got, untrained))
    # the training forward reads the mirror the step kept: it equals a fresh qat detector's on the same weights
    fresh = _model()
    fresh.load_state_dict(model.state_dict())
    model.train()
    la, lb = model.losses(*batch, generator=_seeded(2)), fresh.losses(*batch, generator=_seeded(2))
    assert sorted(la) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    assert all(torch.equal(la[k], lb[k]) for k in la)


def test_detector_hands_the_encoder_the_pinned_backward(batch):
    """The gradients arriving at the encoder's taps, recorded by tensor hooks, put through FlatState.forward / backward into a separate
    block give the encoder parameters' .grad bit for bit: between the detector's loss and the encoder there is nothing but the
    straight-through backward tests/test_gpu_mxfp8_qat.py pins to its oracle."""
    model = _model()
    enc = _encoder(model)
    seen = {}

    def record(module, args, kwargs, out):
        seen["x"] = args[0].detach().clone()
        seen["taps"] = list(kwargs["taps"])
        seen["grads"] = {}
        for idx, h in enumerate(out.hidden_states):
            if h is not None:
                h.register_hook(lambda g, idx=idx: seen["grads"].__setitem__(idx, g.detach().to(torch.float32).contiguous().clone()))

    handle = enc.register_forward_hook(record, with_kwargs=True)
    _backward(model, batch, SCALE)
    handle.remove()
    taps, x = seen["taps"], seen["x"]
    assert sorted(seen["grads"]) == sorted(set(taps)) and x.dtype == torch.float32
    st = enc._flat_state
    # a tap asked for twice: the later output is the one the detector reads, the earlier one receives a zero gradient
    dtaps = [seen["grads"][t] if t not in taps[i + 1:] else torch.zeros_like(seen["grads"][t]) for i, t in enumerate(taps)]
    saved = st.new_saved(x.shape[0])
    flat = torch.full_like(st.grads, float("nan"))
    st.forward(x, taps, None, saved)
    st.backward(x, taps, dtaps, None, saved, st.lcfg.layers, 0, grads=flat)
    torch.cuda.synchronize()
    assert len(st.named) > 40
    for name, p, off, shape in st.named:
        assert p.grad is not None, name
        assert torch.equal(p.grad, flat[off: off + p.numel()].view(shape)), name


def test_twenty_steps_lower_the_loss(batch):
    model = _model()
    step = DetectorTrainStep(model, lr=1e-3)
    history = [step.step(*batch, generator=_seeded(2)) for _ in range(20)]
    totals = [float(sum(v.item() for v in h.values())) for h in history]
    print("qat detector, summed loss over 20 steps:", [round(v, 4) for v in totals], "steps", step.steps, "skipped", step.skipped_steps,
          "scale", step.scale)
    assert all(np.isfinite(v.item()) for h in history for v in h.values())
    assert totals[-1] < totals[0]
    assert step.steps + step.skipped_steps == 20 and step.steps > 0


def test_apply_is_graph_capturable_mirror_included(batch):
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
    ea, eb = _encoder(eager_model)._flat_state, _encoder(graph_model)._flat_state
    assert torch.equal(ea.packed, _fresh_pack(ea)), "eager: the mirror is not a fresh pack"
    assert torch.equal(eb.packed, _fresh_pack(eb)), "replayed: the mirror is not a fresh pack"
    assert _same_mirror(ea, eb)


def test_state_round_trip_gives_a_bit_identical_next_step(batch):
    first, second = _model(), _model()
    a = DetectorTrainStep(first, lr=1e-3, weight_decay=0.01, init_scale=SCALE, growth_interval=2)
    a.step(*batch, generator=_seeded(2))
    a.step(*batch, generator=_seeded(3))
    sd = copy.deepcopy(a.state_dict())
    assert sd["state"]["step"] + sd["state"]["skipped_steps"] == 2 and any("dit" in k for k in sd["exp_avg"])
    second.load_state_dict(first.state_dict())
    b = DetectorTrainStep(second, lr=5.0, weight_decay=0.01, growth_interval=2)
    b.load_state_dict(sd)
    la, lb = a.step(*batch, generator=_seeded(4)), b.step(*batch, generator=_seeded(4))
    torch.cuda.synchronize()
    assert all(torch.equal(la[k], lb[k]) for k in la)
    sa, sb = first.state_dict(), second.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a.state_dict()["state"] == b.state_dict()["state"]
    assert _same_mirror(_encoder(first)._flat_state, _encoder(second)._flat_state)
