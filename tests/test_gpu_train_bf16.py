"""``train_dtype="bf16"`` on the GPU: the two ReLU-backward entry points with a bf16 ``act`` against the existing
ones on the widened ``act`` (bit for bit), ``grad_ops.linear_bwd`` / ``conv3x3_bwd`` on the bf16 tensors a bf16 forward saves against
the same calls on their fp32 widenings (bit for bit), each stage's training forward against its eval forward under ``neck_dtype`` /
``head_dtype="bf16"`` (bit for bit), each stage's gradients against float64 autograd of the plain model, and the detector with
``DetectorTrainStep``.

Gates: 2e-5 relative L2 where only fp32 accumulation differs from the reference (the project's fp32 gate: a bias gradient that is a
column sum of the incoming gradient), 3e-2 for a gradient with bf16 operand rounding upstream (the project's gradient gate), 2e-2 for
a loss of the bf16 forward against the fp32 forward (the project's bf16 forward gate).  Measured values: section 32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                     # noqa: E402

from layoutdit_amd import _lib, config as cfgs, ops, synth                     # noqa: E402
from layoutdit_amd.config import DiTConfig                                     # noqa: E402
from layoutdit_amd.detector_training import DetectorTrainStep                  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel                        # noqa: E402
from layoutdit_amd.modeling.dit_fpn import DiTWithFPN                          # noqa: E402
from layoutdit_amd.modeling.grad_ops import conv3x3_bwd, linear_bwd            # noqa: E402
from layoutdit_amd.modeling.roi_heads import FastRCNNPredictor, MultiScaleRoIAlign, RoIHeads, TwoMLPHead, _BoxHeadBF16Fn    # noqa: E402
from layoutdit_amd.modeling.rpn import RPNHead                                 # noqa: E402
from oracle import oracle                                                      # noqa: E402
from oracle.fpn_oracle_torch import backbone_maps_t, fpn_forward_t             # noqa: E402
from tests import guarded                                                      # noqa: E402
from tests import roi_oracle as ro                                             # noqa: E402
from tests import roi_train_oracle as bo                                       # noqa: E402
from tests import rpn_train_oracle as to                                       # noqa: E402
from tests.guarded import In, Out, Scratch                                     # noqa: E402
from tests.util import rel_l2                                                  # noqa: E402

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
NC = 6
F32_GATE, BF16_GATE, FWD_GATE = 2e-5, 3e-2, 2e-2
MAPS = [(1, 1, 1, 64), (2, 5, 7, 64), (2, 14, 14, 256)]
NAMES = ["p2", "p3", "p4", "p5", "pool"]


def _normal(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).normal(0, scale, size=shape).astype(np.float32))


def _rel(got, ref):
    return rel_l2(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy())


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


SUBNORMAL = 2.0 ** -130                              # a bf16 subnormal (the smallest normal is 2^-126): positive, so it does not mask


def _problem(seed, *shape):
    """``(dy fp32, act bf16)``: ``act`` normal (about half of it negative) with +0, -0, NaN, a negative value and a bf16 subnormal planted;
    ``dy`` normal, non-finite under the four that mask and 2.5 under the subnormal - as many of the five as the tensor has elements."""
    dy, act = _normal(seed, *shape), _normal(seed + 1, *shape).to(BF)
    where = np.random.RandomState(seed + 2).permutation(dy.numel())[:5]
    plant = [(0.0, float("inf")), (-0.0, float("nan")), (float("nan"), float("-inf")), (-1.0, float("nan")), (SUBNORMAL, 2.5)]
    for idx, (a, d) in zip(where, plant):
        act.view(-1)[idx], dy.view(-1)[idx] = a, d
    if dy.numel() >= 5:
        sub = act.view(-1)[where[4]]
        assert float(sub) == SUBNORMAL and 0 < float(sub) < 2.0 ** -126
    return dy, act


def _same_column_sums(got, want):
    """Finite columns bit-equal; a column that holds an unmasked inf or NaN is non-finite in both."""
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin)
    assert torch.equal(_bits(got[fin]), _bits(want[fin]))


def _twin(specs, call):
    return guarded.twin_run(specs, call, device=DEV, sync=torch.cuda.synchronize)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the entry points with a bf16 act against the existing ones on act.float() ---------------------------------------------------------
@pytest.mark.parametrize("pad_ld", [0, 3])
@pytest.mark.parametrize("N", [1, 4, 64, 68])
@pytest.mark.parametrize("M", [1, 5, 513, 1030])                                              # 513 crosses the 512-row block
def test_relu_bwd_bf16_act16_equals_the_fp32_act_entry(M, N, pad_ld):
    lib = _lib.load()
    dy, act = _problem(300 + M + N, M, N)
    ld = N + pad_ld
    need = int(lib.ldit_colsum_scratch_bytes(M, N))
    for with_act in (True, False):
        want_out, want_cs = ops.relu_bwd_bf16(dy.to(DEV), act.float().to(DEV) if with_act else None)      # the existing entry point
        want_out, want_cs = want_out.cpu(), want_cs.cpu()
        assert bool(torch.isfinite(want_cs).all()) or not with_act
        for with_cs in (True, False):
            s = {"dy": In(dy, ld=ld), "out": Out((M, N), BF, ld=ld)}
            if with_act:
                s["act"] = In(act, ld=ld)
            if with_cs:
                s["cs"], s["scratch"] = Out((N,), F32), Scratch(max(need, 16))
            res = _twin(s, lambda t: _lib.check(lib.ldit_relu_bwd_bf16_act16(
                _p(t["dy"]), ld, _p(t.get("act")), ld, _p(t["out"]), ld, M, N, _p(t.get("cs")), _p(t.get("scratch")), need if with_cs else 0,
                _s())))
            for run in (res.clean, res.poisoned):
                assert torch.equal(_bits(run["out"]), _bits(want_out)), (with_act, with_cs)
                if with_cs:
                    _same_column_sums(run["cs"], want_cs)
    # the wrapper dispatches on act's dtype
    out, cs = ops.relu_bwd_bf16(dy.to(DEV), act.to(DEV))
    want_out, want_cs = ops.relu_bwd_bf16(dy.to(DEV), act.float().to(DEV))
    assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(_bits(cs), _bits(want_cs))
    assert bool(torch.isfinite(cs).all()) and bool(torch.isfinite(out.float()).all())           # every non-finite dy sat under a mask
    assert ops.relu_bwd_bf16(dy.to(DEV), act.to(DEV), want_colsum=False)[1] is None


@pytest.mark.parametrize("B,H,W,Cc", MAPS)                                                    # the last crosses a 512-row block
def test_relu_bwd_pad_nhwc_bf16_act16_equals_the_fp32_act_entry(B, H, W, Cc):
    lib = _lib.load()
    dy, act = _problem(400 + H, B, H, W, Cc)
    M = B * H * W
    need = int(lib.ldit_colsum_scratch_bytes(M, Cc))
    border = torch.ones(B, H + 2, W + 2, dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    for with_act in (True, False):
        want_out, want_cs = ops.relu_bwd_pad_nhwc_bf16(dy.to(DEV), act.float().to(DEV) if with_act else None)
        want_out, want_cs = want_out.view(B, H + 2, W + 2, Cc).cpu(), want_cs.cpu()
        for with_cs in (True, False):
            s = {"dy": In(dy), "out": Out((B, H + 2, W + 2, Cc), BF)}
            if with_act:
                s["act"] = In(act)
            if with_cs:
                s["cs"], s["scratch"] = Out((Cc,), F32), Scratch(max(need, 16))
            res = _twin(s, lambda t: _lib.check(lib.ldit_relu_bwd_pad_nhwc_bf16_act16(
                _p(t["dy"]), _p(t.get("act")), _p(t["out"]), B, H, W, Cc, _p(t.get("cs")), _p(t.get("scratch")), need if with_cs else 0, _s())))
            for run in (res.clean, res.poisoned):
                assert torch.equal(_bits(run["out"]), _bits(want_out)), (with_act, with_cs)
                assert not _bits(run["out"])[border].any()                                 # every border element is (+)zero
                if with_cs:
                    _same_column_sums(run["cs"], want_cs)
    out, cs = ops.relu_bwd_pad_nhwc_bf16(dy.to(DEV), act.to(DEV))
    want_out, want_cs = ops.relu_bwd_pad_nhwc_bf16(dy.to(DEV), act.float().to(DEV))
    assert tuple(out.shape) == (B * (H + 2) * (W + 2), Cc) and torch.equal(_bits(out), _bits(want_out)) and torch.equal(_bits(cs), _bits(want_cs))
    assert bool(torch.isfinite(cs).all())


def test_relu_bwd_act16_refusals_on_device_buffers():
    lib = _lib.load()
    dy, act, out = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV, dtype=BF), torch.full((6 * 4 * 8,), 7.0, device=DEV, dtype=BF)
    cs, scratch = torch.zeros(8, device=DEV), torch.zeros(64, device=DEV)
    plain, padded = lib.ldit_relu_bwd_bf16_act16, lib.ldit_relu_bwd_pad_nhwc_bf16_act16
    assert plain(_p(dy), 8, _p(act) + 1, 8, _p(out), 8, 4, 8, _p(cs), _p(scratch), 32, _s()) == _lib.LDIT_EINVAL
    assert plain(_p(dy), 8, _p(act), 7, _p(out), 8, 4, 8, _p(cs), _p(scratch), 32, _s()) == _lib.LDIT_EINVAL
    assert plain(_p(dy), 8, _p(act), 8, _p(out), 8, 4, 8, _p(cs), _p(scratch), 31, _s()) == _lib.LDIT_EWORKSPACE
    assert plain(_p(dy), 8, _p(act), 8, _p(out), 8, 1 << 31, 8, None, None, 0, _s()) == _lib.LDIT_EUNSUPPORTED
    assert padded(_p(dy), _p(act) + 2, _p(out), 1, 2, 2, 8, _p(cs), _p(scratch), 32, _s()) == _lib.LDIT_EINVAL
    assert padded(_p(dy), _p(act), _p(out), 1, 2, 2, 6, _p(cs), _p(scratch), 32, _s()) == _lib.LDIT_EINVAL
    assert padded(_p(dy), _p(act), _p(out), 1, 2, 2, 8, _p(cs), _p(scratch), 31, _s()) == _lib.LDIT_EWORKSPACE
    assert padded(_p(dy), _p(act), _p(out), 1 << 16, 1 << 8, 1 << 7, 8, None, None, 0, _s()) == _lib.LDIT_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(cs.any())                                 # a refusal launches nothing
    # a plain-form act that is only 2-byte aligned is taken (one column per thread)
    act_odd = torch.zeros(4 * 8 + 1, device=DEV, dtype=BF)[1:].view(4, 8)
    assert plain(_p(dy), 8, _p(act_odd), 8, _p(out), 8, 4, 8, None, None, 0, _s()) == _lib.LDIT_OK
    torch.cuda.synchronize()


def _widenings_agree(got, want, dy, act16, selects: bool):
    """``got`` (bf16 ``x`` / ``act``) has the bits of ``want`` (their fp32 widenings).  The fused launch of the bf16 arm SELECTS: every
    non-finite ``dy`` of :func:`_problem` sits under a mask, so all is finite.  The fp32 arm MULTIPLIES, ``dy * (act > 0)``: those
    positions are NaN, in both calls alike, and ``g_b`` is non-finite in exactly the columns that hold one."""
    for g, r, name in zip(got, want, ("g_x", "g_w", "g_b")):
        assert g.dtype == F32, name
        if selects:
            assert bool(torch.isfinite(g).all()) and torch.equal(g, r), name
        else:
            fin = torch.isfinite(r)
            assert torch.equal(torch.isfinite(g), fin) and torch.equal(g[fin], r[fin]), name
    if not selects:
        masked = dy * (act16.float() > 0)
        assert torch.equal(torch.isfinite(got[2]), torch.isfinite(masked).all(dim=0)) and not bool(torch.isfinite(got[2]).all())


# ---- 2. the backward helpers on what a bf16 forward saves ---------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("K", [64, 3136])
@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("M", [1, 32, 74])
def test_linear_bwd_reads_bf16_x_and_act_as_their_widenings(M, N, K, grad_dtype):
    dy, act16 = _problem(M + N + K, M, N)
    x16, w = _normal(M + K, M, K).to(BF).to(DEV), _normal(N + K, N, K, scale=0.1).to(DEV)
    dy, act16 = dy.to(DEV), act16.to(DEV)
    got = linear_bwd(dy, x16, w, True, True, True, grad_dtype=grad_dtype, act=act16)
    want = linear_bwd(dy, x16.float(), w, True, True, True, grad_dtype=grad_dtype, act=act16.float())
    _widenings_agree(got, want, dy.view(M, N), act16.view(M, N), selects=grad_dtype == "bf16")
    assert tuple(got[0].shape) == (M, K) and tuple(got[1].shape) == (N, K) and tuple(got[2].shape) == (N,)


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,h,w,Cc", MAPS)
def test_conv3x3_bwd_reads_the_saved_padded_copy_and_bf16_act(B, h, w, Cc, grad_dtype):
    dy, act16 = _problem(h + Cc, B, h, w, Cc)
    x32 = _normal(h + Cc + 1, B, h, w, Cc).to(BF).float().to(DEV)                              # the widening of the saved map
    wt = _normal(2 * Cc, Cc, Cc, 3, 3, scale=0.05).to(DEV)
    dy, act16 = dy.to(DEV), act16.to(DEV)
    x16p = ops.pad_nhwc_bf16(x32, slack_rows=w + 3)                                           # what the forward saves
    assert tuple(x16p.shape) == (B * (h + 2) * (w + 2) + 2 * (w + 3), Cc)
    got = conv3x3_bwd(dy, x16p, wt, True, True, True, grad_dtype=grad_dtype, act=act16)
    want = conv3x3_bwd(dy, x32, wt, True, True, True, grad_dtype=grad_dtype, act=act16.float())
    _widenings_agree(got, want, dy.view(-1, Cc), act16.view(-1, Cc), selects=grad_dtype == "bf16")
    assert tuple(got[0].shape) == (B, h, w, Cc) and tuple(got[1].shape) == (Cc, Cc, 3, 3)
    with pytest.raises(ValueError, match="padded copy"):
        conv3x3_bwd(dy, ops.pad_nhwc_bf16(x32), wt, False, True, False, grad_dtype=grad_dtype)  # a copy without the slack rows


# ---- the RPN head -------------------------------------------------------------------------------------------------------------------------
def _rpn_head(Cc, **kw):
    torch.manual_seed(5)
    head = RPNHead(Cc, 3, **kw)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
    return head.to(DEV)


@pytest.mark.parametrize("B,h,w,Cc", MAPS)
def test_rpn_head_training_forward_equals_the_bf16_eval_forward(B, h, w, Cc):
    head = _rpn_head(Cc, train_dtype="bf16").train()
    x = _normal(h + Cc, B, h, w, Cc).to(DEV).permute(0, 3, 1, 2)
    lg, dl = head.forward_level(x.clone().requires_grad_(True))
    assert lg.requires_grad and dl.requires_grad and lg.dtype == F32 and dl.dtype == F32
    with torch.no_grad():                                                                     # train mode without a gradient: the eval branch
        f32_train = head.forward_level(x)
    head.eval().set_neck_dtype("bf16")
    with torch.no_grad():
        lg_e, dl_e = head.forward_level(x)
    assert torch.equal(lg.detach(), lg_e) and torch.equal(dl.detach(), dl_e)
    assert not torch.equal(f32_train[0], lg_e)                                                # no_grad never read the option
    head.set_neck_dtype("f32")
    with torch.no_grad():
        assert torch.equal(f32_train[0], head.forward_level(x)[0])


def test_rpn_head_below_the_k_tile_keeps_the_f32_launches():
    x = _normal(3, 2, 5, 7, 96).to(DEV).permute(0, 3, 1, 2)                                   # 96 channels: no multiple of 64
    outs = []
    for d in ("f32", "bf16"):
        head = _rpn_head(96, train_dtype=d).train()
        xg = x.clone().requires_grad_(True)
        lg, dl = head.forward_level(xg)
        (lg.sum() + dl.sum()).backward()
        outs.append((lg.detach(), dl.detach(), xg.grad, head.conv[0][0].weight.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def _rpn_run(train_dtype, grad_dtype, xs, gl, gd):
    head = _rpn_head(64, train_dtype=train_dtype, grad_dtype=grad_dtype).train()
    feats = [torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    total = 0
    for f, a, b in zip(feats, gl, gd):
        lg, dl = head.forward_level(f)
        total = total + (lg * torch.from_numpy(a).to(DEV)).sum() + (dl * torch.from_numpy(b).to(DEV)).sum()
    total.backward()
    grads = {k: p.grad for k, p in head.named_parameters()}
    grads.update({f"input{i}": f.grad for i, f in enumerate(feats)})
    assert all(g.dtype == F32 for g in grads.values())
    return grads, {k: v.detach().cpu().double() for k, v in head.named_parameters()}


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_rpn_head_gradients_against_float64_autograd(grad_dtype):
    rng = np.random.RandomState(2)
    shapes, B = [(5, 7), (1, 1)], 2
    xs = [rng.normal(0, 1, size=(B, h, w, 64)).astype(np.float32) for h, w in shapes]
    gl = [rng.normal(0, 1, size=(B, h * w * 3)).astype(np.float32) for h, w in shapes]
    gd = [rng.normal(0, 1, size=(B, h * w * 3, 4)).astype(np.float32) for h, w in shapes]
    g32, params = _rpn_run("f32", grad_dtype, xs, gl, gd)
    g16, _ = _rpn_run("bf16", grad_dtype, xs, gl, gd)
    ref = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref_x = [torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    rt = 0
    for x, a, b in zip(ref_x, gl, gd):
        t = F.relu(F.conv2d(x, ref["conv.0.0.weight"], ref["conv.0.0.bias"], padding=1))
        lg = F.conv2d(t, ref["cls_logits.weight"], ref["cls_logits.bias"]).permute(0, 2, 3, 1).reshape(B, -1)
        dl = F.conv2d(t, ref["bbox_pred.weight"], ref["bbox_pred.bias"])
        _, _, h, w = dl.shape
        dl = dl.view(B, 3, 4, h, w).permute(0, 3, 4, 1, 2).reshape(B, -1, 4)
        rt = rt + (lg * torch.from_numpy(a).double()).sum() + (dl * torch.from_numpy(b).double()).sum()
    rt.backward()
    want = {k: v.grad for k, v in ref.items()}
    want.update({f"input{i}": x.grad for i, x in enumerate(ref_x)})
    # the 1x1 pair's biases are column sums of the incoming gradient: no bf16 operand upstream
    exact = ("cls_logits.bias", "bbox_pred.bias")
    for k in want:
        e, e32 = _rel(g16[k], want[k]), _rel(g32[k], want[k])
        print(f"rpn head grad_dtype={grad_dtype} {k}: train_dtype bf16 {e:.3e}, f32 {e32:.3e}")
        assert e < (F32_GATE if k in exact else BF16_GATE), k
        assert e32 < (F32_GATE if k in exact else BF16_GATE), k
    for k in exact:
        assert torch.equal(g16[k], g32[k]), k
    assert not torch.equal(g16["input0"], g32["input0"])                                     # the forward really changed
    again, _ = _rpn_run("bf16", grad_dtype, xs, gl, gd)
    assert all(torch.equal(again[k], g16[k]) for k in g16)                                   # two backward passes: the same bits


# ---- the FPN -------------------------------------------------------------------------------------------------------------------------------
def test_fpn_training_forward_equals_the_bf16_eval_forward():
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(0)
    m = DiTWithFPN(config=cfg, train_dtype="bf16")
    m.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    with torch.no_grad():
        for p in m.fpn.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.05)
    m = m.to(DEV).train()
    x = torch.from_numpy(synth.synth_images(2, 64, 64, seed=5, kind="uniform")).to(DEV)
    seen = {}
    hook = m.backbone.dit.register_forward_hook(lambda mod, args, out: seen.setdefault("out", out))
    train = m(x)
    hook.remove()
    assert all(f.requires_grad and f.dtype == F32 for f in train.values())
    # the stage's inputs are the encoder's taps: the eval run below is handed the very tensors the training run saw
    hook = m.backbone.dit.register_forward_hook(lambda mod, args, out: seen["out"])
    m.eval().set_neck_dtype("bf16")
    with torch.no_grad():
        ev16 = m(x)
        ev32 = m.set_neck_dtype("f32")(x)
    hook.remove()
    for k in train:
        assert torch.equal(train[k].detach(), ev16[k]), k
    assert not torch.equal(ev32["p2"], ev16["p2"])


def _fpn_run(train_dtype, grad_dtype, cfg, w, x, ws):
    torch.manual_seed(0)
    m = DiTWithFPN(config=cfg, compute_dtype="f32", grad_dtype=grad_dtype, train_dtype=train_dtype)
    m.backbone.dit.load_numpy(w)
    with torch.no_grad():
        for p in m.fpn.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.05)
    m = m.to(DEV).train()
    feats = m(torch.from_numpy(x).to(DEV))
    if ws is None:
        ws = {k: _normal(60 + i, *f.shape, scale=1.0 / np.sqrt(f.numel())) for i, (k, f) in enumerate(feats.items())}
    sum((f * ws[k].to(DEV)).sum() for k, f in feats.items()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.fpn.named_parameters()}
    enc = {name: p.grad.detach().clone() for name, p, _, _ in m.backbone.dit._flat_state.named}
    return m, grads, enc, ws


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_fpn_gradients_against_float64_autograd(grad_dtype):
    """DiTWithFPN at the micro geometry of tests/test_gpu_grad_bf16.py::test_fpn_stage."""
    from oracle.vit_oracle_torch import train_reference
    cfg = cfgs.vit_micro()
    cfg.drop_path_rate = 0.0
    cfg.taps = [1, 1, 2, 3]
    w = synth.synth_weights(cfg, 3)
    B, size, g = 2, 64, 4
    x = synth.synth_images(B, size, size, seed=5, kind="uniform")
    m, g32, e32, ws = _fpn_run("f32", grad_dtype, cfg, w, x, None)
    _, g16, e16, _ = _fpn_run("bf16", grad_dtype, cfg, w, x, ws)
    taps_np, _ = oracle.vit_forward(cfg, w, x)
    taps_t = [torch.from_numpy(t).double().requires_grad_(True) for t in taps_np]
    wt = {k: p.detach().cpu().double().requires_grad_(True) for k, p in m.fpn.named_parameters()}
    ref = fpn_forward_t(backbone_maps_t(taps_t, g, g), wt)
    sum((ref[k] * ws[k].double()).sum() for k in ref).backward()
    for k, r in wt.items():
        e, e_f32 = _rel(g16[k], r.grad), _rel(g32[k], r.grad)
        print(f"fpn grad_dtype={grad_dtype} {k}: train_dtype bf16 {e:.3e}, f32 {e_f32:.3e}")
        # a 3x3 output convolution's bias gradient is a column sum of the gradient the stage is handed
        exact = k.startswith("layer_blocks") and k.endswith("bias")
        assert e < (F32_GATE if exact else BF16_GATE) and e_f32 < (F32_GATE if exact else BF16_GATE), k
        # the stage is linear and this loss is linear in its outputs, so no gradient depends on the forward's values: the wgrad taps
        # read the padded bf16 copy the forward saved where the "f32" setting pads the saved map again - the same bits
        assert torch.equal(g16[k], g32[k]), k
    assert all(torch.equal(e16[k], e32[k]) for k in e16)
    _, enc_ref = train_reference(cfg, w, x, [t.grad.float().numpy() for t in taps_t], taps=m.backbone.layer_idxs)
    for short, hf in (("0.w1", "encoder.layer.0.intermediate.dense.weight"), ("patch_w", "embeddings.patch_embeddings.projection.weight")):
        e = rel_l2(e16[short].cpu().numpy(), enc_ref[hf])
        print(f"fpn -> encoder grad_dtype={grad_dtype} {short}: train_dtype bf16 {e:.3e}, f32 {rel_l2(e32[short].cpu().numpy(), enc_ref[hf]):.3e}")
        assert e < BF16_GATE, short
    _, again, enc_again, _ = _fpn_run("bf16", grad_dtype, cfg, w, x, ws)
    assert all(torch.equal(again[k], g16[k]) for k in g16) and all(torch.equal(enc_again[k], e16[k]) for k in e16)


# ---- the box head ----------------------------------------------------------------------------------------------------------------------------
SIZE, CH, REP, S_ROWS = (96, 160), 64, 64, 20


def _map_sizes(size):
    h, w = size
    return [(h // 4, w // 4), (h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32), ((h // 32 + 1) // 2, (w // 32 + 1) // 2)]


def _box_heads(**kw):
    torch.manual_seed(9)
    head, pred = TwoMLPHead(CH * 49, REP), FastRCNNPredictor(REP, NC)
    with torch.no_grad():
        for p in list(head.parameters()) + list(pred.parameters()):
            p.copy_(torch.randn_like(p) * (0.05 if p.dim() == 2 else 0.3))
    return RoIHeads(MultiScaleRoIAlign(NAMES, 7, 2), head, pred, **kw).to(DEV)


@pytest.fixture(scope="module")
def box_problem():
    sizes = _map_sizes(SIZE)
    rng = np.random.RandomState(17)
    maps = [rng.normal(0, 1, size=(2, h, w, CH)).astype(np.float32) for h, w in sizes]
    boxes = np.stack([ro.make_boxes(11 + b, S_ROWS, SIZE, sizes)[0] for b in range(2)])
    count = np.asarray([S_ROWS, S_ROWS // 2], dtype=np.int32)
    boxes[1, S_ROWS // 2:] = 0.0
    gy = rng.normal(0, 1, size=(2 * S_ROWS, 5 * NC)).astype(np.float32)
    gy[S_ROWS + S_ROWS // 2:] = 0.0                                                           # padding rows carry no gradient
    return maps, boxes, count, gy


def _leaves(maps):
    return [_dev(m).permute(0, 3, 1, 2).requires_grad_(True) for m in maps]


def _box_run(heads, problem, leaves=None, feats=None):
    maps, boxes, count, gy = problem
    leaves = _leaves(maps) if leaves is None else leaves
    feats = dict(zip(NAMES, leaves)) if feats is None else feats
    for p in heads.parameters():
        p.grad = None
    y = heads.head_padded(feats, _dev(boxes), _dev(count), SIZE)
    (y[:, :5 * NC] * _dev(gy)).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in heads.named_parameters()}
    grads.update({f"map{i}": f.grad for i, f in enumerate(leaves)})
    return y, grads


def test_box_head_training_forward_equals_the_bf16_eval_forward(box_problem):
    maps, boxes, count, _ = box_problem
    heads = _box_heads(train_dtype="bf16").train()
    y = heads.head_padded(dict(zip(NAMES, _leaves(maps))), _dev(boxes), _dev(count), SIZE)
    assert y.requires_grad and y.dtype == F32 and isinstance(y.grad_fn, _BoxHeadBF16Fn._backward_cls)
    plain = [_dev(m).permute(0, 3, 1, 2) for m in maps]
    with torch.no_grad():                                                                     # train mode without a gradient: fp32, as today
        y_ng = heads.head_padded(dict(zip(NAMES, plain)), _dev(boxes), _dev(count), SIZE)
    heads.eval().set_head_dtype("bf16")
    with torch.no_grad():
        y_e = heads.head_padded(dict(zip(NAMES, plain)), _dev(boxes), _dev(count), SIZE)
    assert torch.equal(y.detach(), y_e)
    assert not torch.equal(y_ng, y_e) and _rel(y_ng[:, :5 * NC], y_e[:, :5 * NC]) < FWD_GATE
    # a frozen head on maps that want a gradient is the same node; with nothing that wants one it is not entered
    heads.train().requires_grad_(False)
    y_f = heads.head_padded(dict(zip(NAMES, _leaves(maps))), _dev(boxes), _dev(count), SIZE)
    assert torch.equal(y_f.detach(), y_e) and isinstance(y_f.grad_fn, _BoxHeadBF16Fn._backward_cls)
    assert not heads.head_padded(dict(zip(NAMES, plain)), _dev(boxes), _dev(count), SIZE).requires_grad


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_box_head_gradients_against_float64_autograd(box_problem, grad_dtype):
    maps, boxes, count, gy = box_problem
    h32, h16 = _box_heads(grad_dtype=grad_dtype).train(), _box_heads(grad_dtype=grad_dtype, train_dtype="bf16").train()
    (y32, g32), (y16, g16) = _box_run(h32, box_problem), _box_run(h16, box_problem)
    assert isinstance(y16.grad_fn, _BoxHeadBF16Fn._backward_cls) and not isinstance(y32.grad_fn, _BoxHeadBF16Fn._backward_cls)
    _, levels = ops.roi_align_levels([_dev(m).permute(0, 3, 1, 2) for m in maps], _dev(boxes), _dev(count), SIZE, return_levels=True)
    lv = levels.cpu().numpy()
    pooled, _ = ro.roi_align_levels(maps, boxes, count, SIZE, levels=lv)
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in h32.named_parameters()}
    xr = torch.from_numpy(pooled).requires_grad_(True)
    t = F.relu(F.linear(xr.permute(0, 3, 1, 2).flatten(1), ref["box_head.fc6.weight"], ref["box_head.fc6.bias"]))
    t = F.relu(F.linear(t, ref["box_head.fc7.weight"], ref["box_head.fc7.bias"]))
    yr = torch.cat([F.linear(t, ref["box_predictor.cls_score.weight"], ref["box_predictor.cls_score.bias"]),
                    F.linear(t, ref["box_predictor.bbox_pred.weight"], ref["box_predictor.bbox_pred.bias"])], dim=1)
    (yr * torch.from_numpy(gy).double()).sum().backward()
    e_fwd = _rel(y16[:, :5 * NC], yr)
    print(f"box head forward against float64: train_dtype bf16 {e_fwd:.3e}, f32 {_rel(y32[:, :5 * NC], yr):.3e}")
    assert e_fwd < FWD_GATE
    want = {k: v.grad for k, v in ref.items()}
    map_ref, _ = bo.roi_align_levels_bwd(xr.grad.numpy(), boxes, count, lv, _map_sizes(SIZE), SIZE)
    want.update({f"map{i}": torch.from_numpy(r).permute(0, 3, 1, 2) for i, r in enumerate(map_ref)})
    exact = ("box_predictor.cls_score.bias", "box_predictor.bbox_pred.bias")                 # column sums of the incoming gradient
    for k in want:
        if not bool(want[k].any()):
            assert not bool(g16[k].any()), k                                                 # a level no box fell on
            continue
        e, e32 = _rel(g16[k], want[k]), _rel(g32[k], want[k])
        print(f"box head grad_dtype={grad_dtype} {k}: train_dtype bf16 {e:.3e}, f32 {e32:.3e}")
        assert g16[k].dtype == F32
        assert e < (F32_GATE if k in exact else BF16_GATE) and e32 < (F32_GATE if k in exact else BF16_GATE), k
    for k in exact:
        assert torch.equal(g16[k], g32[k]), k
    again = _box_run(h16, box_problem)[1]
    assert all(torch.equal(again[k], g16[k]) for k in g16)                                   # two backward passes: the same bits


def test_box_head_is_one_node_with_fp32_map_gradients(box_problem):
    maps, boxes, count, gy = box_problem
    heads = _box_heads(train_dtype="bf16", grad_dtype="bf16").train()
    _, free = _box_run(heads, box_problem)                                                   # five independent maps
    assert all(free[f"map{i}"].dtype == F32 and free[f"map{i}"].shape == (2, CH) + tuple(s) for i, s in enumerate(_map_sizes(SIZE)))
    # `pool` as the strided view of p5 that DiTWithFPN returns: its gradient arrives in p5
    p5 = _dev(np.zeros((2, 3, 5, CH), dtype=np.float32)).permute(0, 3, 1, 2)
    p5[:, :, ::2, ::2] = _dev(maps[4]).permute(0, 3, 1, 2)
    p5[:, :, 1::2, :], p5[:, :, :, 1::2] = _dev(maps[3]).permute(0, 3, 1, 2)[:, :, 1::2, :], _dev(maps[3]).permute(0, 3, 1, 2)[:, :, :, 1::2]
    leaves = _leaves(maps[:3]) + [p5.clone().requires_grad_(True)]
    feats = dict(zip(NAMES[:4], leaves))
    feats["pool"] = leaves[3][:, :, ::2, ::2]
    only_p5 = [m.copy() for m in maps]
    only_p5[3] = leaves[3].detach().permute(0, 2, 3, 1).cpu().numpy()
    _, ref = _box_run(heads, (only_p5, boxes, count, gy))
    y, got = _box_run(heads, (maps, boxes, count, gy), leaves=leaves, feats=feats)
    want = ref["map3"].clone()
    want[:, :, ::2, ::2] += ref["map4"]
    assert torch.equal(got["map3"], want) and bool(ref["map4"].any()) and got["map3"].dtype == F32
    # a second backward raises, as the three fp32 nodes do
    y = heads.head_padded(dict(zip(NAMES, _leaves(maps))), _dev(boxes), _dev(count), SIZE)
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        y.sum().backward()


def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def test_box_head_stage_peak_memory_is_lower():
    """``losses_padded`` + ``backward`` of the stage at 2 x 512 sampled rows of 64 x 7 x 7: the saved rows and activations are bf16."""
    sizes = _map_sizes((224, 224))
    rng = np.random.RandomState(4)
    maps = [rng.normal(0, 1, size=(2, h, w, CH)).astype(np.float32) for h, w in sizes]
    proposals = _dev(np.stack([ro.make_boxes(31 + b, 600, (224, 224), sizes)[0] for b in range(2)]))
    count = _dev(np.asarray([600, 600], dtype=np.int32))
    gt_boxes = _dev(np.stack([to.scene(7, 7), to.scene(8, 7)]).astype(np.float32))
    gt_labels = _dev((np.arange(14, dtype=np.int32) % 5 + 1).reshape(2, 7))
    gt_count = _dev(np.asarray([7, 7], dtype=np.int32))
    peak = {}
    for d in ("f32", "bf16"):
        heads = _box_heads(train_dtype=d, grad_dtype="bf16").train()
        feats = dict(zip(NAMES, _leaves(maps)))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        losses = heads.losses_padded(feats, proposals, count, (224, 224), gt_boxes, gt_labels, gt_count, generator=_seeded(3))
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        peak[d] = torch.cuda.max_memory_allocated() - base
        assert all(np.isfinite(float(v)) for v in losses.values())
        del heads, feats, losses
    print(f"box head stage, peak allocated above the inputs: f32 {peak['f32'] / 2 ** 20:.1f} MiB, bf16 {peak['bf16'] / 2 ** 20:.1f} MiB")
    assert peak["bf16"] < peak["f32"]


# ---- 5. the detector -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    """The smallest detector of tests/test_gpu_detector_step.py, identically initialised every time."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, **kw)
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


def _losses_and_grads(model, batch):
    for p in model.parameters():
        p.grad = None
    losses = model.losses(*batch, generator=_seeded(2))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in losses.items()}, {n: (None if p.grad is None else p.grad.detach().clone())
                                                                for n, p in model.named_parameters()}


def test_detector_rpn_losses_follow_the_f32_setting(batch):
    model = _model()
    l32 = {k: float(v) for k, v in model.rpn_losses(*batch, generator=_seeded(2)).items()}
    assert model.set_train_dtype("bf16").train_dtype == "bf16"
    got = model.rpn_losses(*batch, generator=_seeded(2))
    sum(got.values()).backward()                                                              # ... and they are differentiable
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.model.rpn.head.parameters())
    for k, v in got.items():
        e = abs(float(v) - l32[k]) / abs(l32[k])
        print(f"detector {k}: train_dtype bf16 {float(v):.6f}, f32 {l32[k]:.6f}, relative difference {e:.3e}")
        assert e < FWD_GATE and float(v) != l32[k], k


def test_detector_f32_setting_and_eval_mode_are_the_model_without_the_argument(batch):
    plain, model = _model(), _model(train_dtype="bf16")
    pages = torch.from_numpy(synth.synth_images(2, 224, 224, seed=3, kind="uniform")).to(DEV)
    plain.eval(), model.eval()
    with torch.no_grad():
        a, b = plain.forward_padded(pages), model.forward_padded(pages)                       # eval mode never reads the option
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    plain.train(), model.train().set_train_dtype("f32")
    for grad_dtype in ("f32", "bf16"):
        (la, ga), (lb, gb) = _losses_and_grads(plain.set_grad_dtype(grad_dtype), batch), _losses_and_grads(model.set_grad_dtype(grad_dtype), batch)
        assert sorted(la) == sorted(lb) and all(torch.equal(la[k], lb[k]) for k in la)
        assert all((ga[n] is None and gb[n] is None) or torch.equal(ga[n], gb[n]) for n in ga), grad_dtype
    # all four combinations of the two training options run and give finite losses and gradients
    for train_dtype in ("f32", "bf16"):
        for grad_dtype in ("f32", "bf16"):
            l, g = _losses_and_grads(model.set_train_dtype(train_dtype).set_grad_dtype(grad_dtype), batch)
            assert all(np.isfinite(float(v)) for v in l.values()), (train_dtype, grad_dtype)
            assert all(x is None or bool(torch.isfinite(x).all()) for x in g.values()), (train_dtype, grad_dtype)


def test_twenty_steps_in_bf16_lower_the_loss_and_caches_follow_the_weights(batch):
    model = _model(train_dtype="bf16", grad_dtype="bf16")
    step = DetectorTrainStep(model, lr=1e-3)
    m = model.model
    history = []
    for i in range(20):
        history.append(step.step(*batch, generator=_seeded(2)))
        if i < 2:
            # after apply() every bf16 operand the training forward reads is gone; the next forward re-makes it from the new weights
            assert not any(s._operand_cache.filled() for s in (m.rpn.head, m.roi_heads.box_head, m.roi_heads.box_predictor, m.backbone))
    totals = [float(sum(v.item() for v in h.values())) for h in history]
    print("summed loss over 20 steps, train_dtype bf16, grad_dtype bf16:", [round(v, 4) for v in totals], "steps", step.steps, "skipped",
          step.skipped_steps)
    assert all(np.isfinite(v.item()) for h in history for v in h.values())
    assert step.steps == 20 and step.skipped_steps == 0
    assert totals[-1] <= 0.5 * totals[0]
    # the next training forward is that of a fresh model loaded from the updated state_dict
    nxt = {k: v.detach().clone() for k, v in model.losses(*batch, generator=_seeded(5)).items()}
    fresh = _model(train_dtype="bf16", grad_dtype="bf16")
    fresh.load_state_dict(model.state_dict())
    ref = fresh.losses(*batch, generator=_seeded(5))
    assert all(torch.equal(nxt[k], ref[k].detach()) for k in nxt)
