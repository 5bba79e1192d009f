"""``grad_dtype="bf16"`` on the GPU: the fused ReLU-backward / bf16 copy / bias-gradient launch against the three
kernels it replaces (bit for bit), ``grad_ops.linear_bwd`` / ``conv3x3_bwd`` in both settings on the same inputs (weight and bias
gradients bit-equal, the input gradient against the float64 contract oracle ``tests/grad_bf16_oracle.py`` and against plain
float64), the three differentiable stages against float64 autograd, and the detector with ``DetectorTrainStep``.

Gates: 2e-5 relative L2 where only the fp32 accumulation differs from the reference (the project's fp32 gate), 3e-2 for a gradient
with bf16 operand rounding upstream (the project's gate for its bf16-operand weight gradients).  Measured values: section 30."""
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
from layoutdit_amd.modeling.roi_heads import FastRCNNPredictor, TwoMLPHead     # noqa: E402
from layoutdit_amd.modeling.rpn import RPNHead                                 # noqa: E402
from oracle import oracle                                                      # noqa: E402
from oracle.fpn_oracle_torch import backbone_maps_t, fpn_forward_t             # noqa: E402
from tests import grad_bf16_oracle as go                                       # noqa: E402
from tests import guarded                                                      # noqa: E402
from tests import rpn_train_oracle as to                                       # noqa: E402
from tests.guarded import In, Out, Scratch                                     # noqa: E402
from tests.util import rel_l2                                                  # noqa: E402

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
NC = 6
F32_GATE, BF16_GATE = 2e-5, 3e-2


def _normal(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).normal(0, scale, size=shape).astype(np.float32))


def _rel(got, ref):
    return rel_l2(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy())


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _problem(seed, *shape):
    """``(dy, act)``: ``act`` normal (about half of it masks) with an exact +0, a -0 and a NaN planted; ``dy`` normal with an inf and
    a NaN under masked positions and one inf under an unmasked one - as many of the four as the tensor has elements."""
    dy, act = _normal(seed, *shape), _normal(seed + 1, *shape)
    n = dy.numel()
    where = np.random.RandomState(seed + 2).permutation(n)[:4]
    plant = [(0.0, float("inf")), (-0.0, float("nan")), (float("nan"), 1.5), (1.0, float("inf"))]
    for idx, (a, d) in zip(where, plant):
        act.view(-1)[idx], dy.view(-1)[idx] = a, d
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


# ---- 1. the fused kernel, plain form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_ld", [0, 3])
@pytest.mark.parametrize("M,N", [(1, 1), (3, 5), (511, 8), (512, 64), (513, 257), (1025, 32)])
def test_relu_bwd_bf16_equals_the_kernels_it_replaces(M, N, pad_ld):
    lib = _lib.load()
    dy, act = _problem(100 + M, M, N)
    ld = N + pad_ld
    need = int(lib.ldit_colsum_scratch_bytes(M, N))
    assert need == ((M + 511) // 512) * N * 4
    for with_act in (True, False):
        w = (torch.where(act > 0, dy, torch.zeros_like(dy)) if with_act else dy).to(DEV)
        want_out, want_cs = ops.cast_bf16(w).cpu(), ops.colsum(w).cpu()                    # the existing kernels
        for with_cs in (True, False):
            s = {"dy": In(dy, ld=ld), "out": Out((M, N), BF, ld=ld)}
            if with_act:
                s["act"] = In(act, ld=ld)
            if with_cs:
                s["cs"], s["scratch"] = Out((N,), F32), Scratch(max(need, 16))
            res = _twin(s, lambda t: _lib.check(lib.ldit_relu_bwd_bf16(
                _p(t["dy"]), ld, _p(t.get("act")), ld, _p(t["out"]), ld, M, N, _p(t.get("cs")), _p(t.get("scratch")), need if with_cs else 0,
                _s())))
            for run in (res.clean, res.poisoned):
                assert torch.equal(_bits(run["out"]), _bits(want_out)), (with_act, with_cs)
                if with_cs:
                    _same_column_sums(run["cs"], want_cs)
    # the wrapper: the same two results from contiguous tensors
    out, cs = ops.relu_bwd_bf16(dy.to(DEV), act.to(DEV))
    w = torch.where(act > 0, dy, torch.zeros_like(dy)).to(DEV)
    assert torch.equal(_bits(out), _bits(ops.cast_bf16(w)))
    _same_column_sums(cs, ops.colsum(w))
    assert ops.relu_bwd_bf16(dy.to(DEV), None, want_colsum=False)[1] is None


# ---- 2. the fused kernel, padded form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", [(1, 1, 1, 4), (1, 7, 4, 12), (2, 3, 5, 64), (3, 14, 14, 256)])     # the last crosses a 512-row block
def test_relu_bwd_pad_nhwc_bf16_equals_the_kernels_it_replaces(B, H, W, Cc):
    lib = _lib.load()
    dy, act = _problem(200 + H, B, H, W, Cc)
    M = B * H * W
    need = int(lib.ldit_colsum_scratch_bytes(M, Cc))
    border = torch.ones(B, H + 2, W + 2, dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    for with_act in (True, False):
        w = (torch.where(act > 0, dy, torch.zeros_like(dy)) if with_act else dy).to(DEV)
        want_out = ops.pad_nhwc_bf16(w).view(B, H + 2, W + 2, Cc).cpu()
        want_cs = ops.colsum(w.view(M, Cc)).cpu()
        for with_cs in (True, False):
            s = {"dy": In(dy), "out": Out((B, H + 2, W + 2, Cc), BF)}
            if with_act:
                s["act"] = In(act)
            if with_cs:
                s["cs"], s["scratch"] = Out((Cc,), F32), Scratch(max(need, 16))
            res = _twin(s, lambda t: _lib.check(lib.ldit_relu_bwd_pad_nhwc_bf16(
                _p(t["dy"]), _p(t.get("act")), _p(t["out"]), B, H, W, Cc, _p(t.get("cs")), _p(t.get("scratch")), need if with_cs else 0, _s())))
            for run in (res.clean, res.poisoned):
                assert torch.equal(_bits(run["out"]), _bits(want_out)), (with_act, with_cs)
                assert not _bits(run["out"])[border].any()                                 # every border element is (+)zero
                if with_cs:
                    _same_column_sums(run["cs"], want_cs)
    out, cs = ops.relu_bwd_pad_nhwc_bf16(dy.to(DEV), act.to(DEV))
    w = torch.where(act > 0, dy, torch.zeros_like(dy)).to(DEV)
    assert tuple(out.shape) == (B * (H + 2) * (W + 2), Cc) and torch.equal(_bits(out), _bits(ops.pad_nhwc_bf16(w)))
    _same_column_sums(cs, ops.colsum(w.view(M, Cc)))


# ---- 3. / 4. one layer's backward in both settings -----------------------------------------------------------------------------------------
def _both(fn):
    a, b = fn("f32"), fn("bf16")
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("K", [64, 1568])
@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("M", [1, 32, 74])
def test_linear_bwd_in_both_settings(M, N, K):
    dy, x, w = _normal(M + N, M, N), _normal(M + K, M, K), _normal(N + K, N, K, scale=0.1)
    dyd, xd, wd = dy.to(DEV), x.to(DEV), w.to(DEV)
    (gx32, gw32, gb32), (gx16, gw16, gb16) = _both(lambda d: linear_bwd(dyd, xd, wd, True, True, True, grad_dtype=d))
    assert torch.equal(gw32, gw16) and torch.equal(gb32, gb16)                             # one bf16 copy of dy serves dgrad and wgrad
    assert tuple(gx16.shape) == (M, K) and gx16.dtype == F32
    e_contract, e_exact = _rel(gx16, go.linear_gx(dy, w)), _rel(gx16, go.linear_gx_exact(dy, w))
    print(f"linear_bwd M={M} N={N} K={K}: g_x against the contract oracle {e_contract:.3e}, against float64 {e_exact:.3e}; "
          f"f32 setting against float64 {_rel(gx32, go.linear_gx_exact(dy, w)):.3e}")
    assert e_contract < F32_GATE and e_exact < BF16_GATE
    assert not torch.equal(gx32, gx16)
    assert torch.equal(gx16, linear_bwd(dyd, xd, wd, True, False, False, grad_dtype="bf16")[0])       # bit-reproducible
    # the mask the launch applies is a selection
    act = _normal(M + 7, M, N)
    dyn = dy.clone()
    masked = (act <= 0).nonzero()
    if len(masked):
        dyn[tuple(masked[0])] = float("nan")
    gxm, _, gbm = linear_bwd(dyn.to(DEV), xd, wd, True, False, True, grad_dtype="bf16", act=act.to(DEV))
    assert _rel(gxm, go.linear_gx(dyn, w, act)) < F32_GATE and bool(torch.isfinite(gbm).all())


@pytest.mark.parametrize("M", [1, 74])
def test_linear_bwd_below_the_k_tile_stays_fp32(M):
    dy, x, w = _normal(M, M, 32), _normal(M + 1, M, 64), _normal(M + 2, 32, 64, scale=0.1)
    (a, b) = _both(lambda d: linear_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), True, True, True, grad_dtype=d))
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # ... and so does a weight that lacks rows for dy's zero padding columns (the box predictor's stacked matrix)
    dy64, w40 = _normal(M + 3, M, 64), _normal(M + 4, 40, 64, scale=0.1)
    dy64[:, 40:] = 0
    (a, b) = _both(lambda d: linear_bwd(dy64.to(DEV), x.to(DEV), w40.to(DEV), True, False, True, grad_dtype=d))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("B,h,w,Cin,Cout", [(1, 1, 1, 64, 128), (2, 5, 7, 64, 64), (2, 14, 14, 256, 256)])
def test_conv3x3_bwd_in_both_settings(B, h, w, Cin, Cout):
    dy, x, wt = _normal(h + Cout, B, h, w, Cout), _normal(h + Cin, B, h, w, Cin), _normal(Cin + Cout, Cout, Cin, 3, 3, scale=0.05)
    dyd, xd, wd = dy.to(DEV), x.to(DEV), wt.to(DEV)
    (gx32, gw32, gb32), (gx16, gw16, gb16) = _both(lambda d: conv3x3_bwd(dyd, xd, wd, True, True, True, grad_dtype=d))
    assert torch.equal(gw32, gw16) and torch.equal(gb32, gb16)
    assert tuple(gx16.shape) == (B, h, w, Cin) and gx16.dtype == F32
    e_contract, e_exact = _rel(gx16, go.conv3x3_gx(dy, wt)), _rel(gx16, go.conv3x3_gx_exact(dy, wt))
    print(f"conv3x3_bwd {B}x{h}x{w} {Cin}->{Cout}: g_x against the contract oracle {e_contract:.3e}, against float64 {e_exact:.3e}; "
          f"f32 setting against float64 {_rel(gx32, go.conv3x3_gx_exact(dy, wt)):.3e}")
    assert e_contract < F32_GATE and e_exact < BF16_GATE
    assert not torch.equal(gx32, gx16)
    assert torch.equal(gx16, conv3x3_bwd(dyd, xd, wd, True, False, False, grad_dtype="bf16")[0])
    act = _normal(h + 9, B, h, w, Cout)
    gxm, gwm, gbm = conv3x3_bwd(dyd, xd, wd, True, True, True, grad_dtype="bf16", act=act.to(DEV))
    keep = torch.where(act > 0, dy, torch.zeros_like(dy)).to(DEV)
    ref = conv3x3_bwd(keep, xd, wd, True, True, True, grad_dtype="bf16")
    assert all(torch.equal(p, q) for p, q in zip((gxm, gwm, gbm), ref))
    assert _rel(gxm, go.conv3x3_gx(dy, wt, act)) < F32_GATE


def test_conv3x3_bwd_below_the_k_tile_stays_fp32():
    dy, x, wt = _normal(1, 2, 5, 7, 32), _normal(2, 2, 5, 7, 64), _normal(3, 32, 64, 3, 3, scale=0.05)
    (a, b) = _both(lambda d: conv3x3_bwd(dy.to(DEV), x.to(DEV), wt.to(DEV), True, True, True, grad_dtype=d))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 5. the stages -----------------------------------------------------------------------------------------------------------------------
def _heads_run(M, grad_dtype):
    """The inputs of tests/test_gpu_roi_train.py::test_heads_backward_matches_float64_autograd."""
    torch.manual_seed(M)
    Cc, rep = 32, 64
    head, pred = TwoMLPHead(Cc * 49, rep, grad_dtype=grad_dtype).to(DEV).train(), FastRCNNPredictor(rep, NC).to(DEV).train()
    with torch.no_grad():
        for p in list(head.parameters()) + list(pred.parameters()):
            p.copy_(torch.randn_like(p) * (0.1 if p.dim() == 2 else 0.3))
    rng = np.random.RandomState(M)
    x = rng.normal(0, 1, size=(M, 7, 7, Cc)).astype(np.float32)
    gy = rng.normal(0, 1, size=(M, 5 * NC)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = pred.forward_stacked(head(xd))
    (y[:, :5 * NC] * torch.from_numpy(gy).to(DEV)).sum().backward()
    grads = {k: p.grad for k, p in list(head.named_parameters()) + list(pred.named_parameters())}
    grads["input"] = xd.grad
    params = {k: v.detach().cpu().double() for k, v in list(head.named_parameters()) + list(pred.named_parameters())}
    return y.detach(), grads, params, x, gy


@pytest.mark.parametrize("M", [74, 32])
def test_box_head_stage(M):
    y32, g32, params, x, gy = _heads_run(M, "f32")
    y16, g16, _, _, _ = _heads_run(M, "bf16")
    assert torch.equal(y32, y16)                                                           # no forward bit changes
    ref = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    xr = torch.from_numpy(x).double().requires_grad_(True)
    t = F.relu(F.linear(xr.permute(0, 3, 1, 2).flatten(1), ref["fc6.weight"], ref["fc6.bias"]))
    t = F.relu(F.linear(t, ref["fc7.weight"], ref["fc7.bias"]))
    yr = torch.cat([F.linear(t, ref["cls_score.weight"], ref["cls_score.bias"]), F.linear(t, ref["bbox_pred.weight"], ref["bbox_pred.bias"])], dim=1)
    (yr * torch.from_numpy(gy).double()).sum().backward()
    want = {k: v.grad for k, v in ref.items()}
    want["input"] = xr.grad
    no_bf16_upstream = ("cls_score.bias", "bbox_pred.bias", "fc7.bias")
    for k in want:
        e = _rel(g16[k], want[k])
        print(f"box head M={M} {k}: bf16 setting {e:.3e}, f32 setting {_rel(g32[k], want[k]):.3e}")
        assert e < (F32_GATE if k in no_bf16_upstream else BF16_GATE), k
    assert not torch.equal(g16["input"], g32["input"]) and not torch.equal(g16["fc6.bias"], g32["fc6.bias"])
    for k in ("cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias", "fc7.weight", "fc7.bias"):
        assert torch.equal(g16[k], g32[k]), k                                              # nothing upstream of them changed
    again = _heads_run(M, "bf16")[1]
    assert all(torch.equal(again[k], g16[k]) for k in g16)                                 # bit-reproducible


def _rpn_run(grad_dtype, xs, gl, gd):
    torch.manual_seed(5)
    head = RPNHead(64, 3, grad_dtype=grad_dtype)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
    head = head.to(DEV).train()
    feats = [torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    total, outs = 0, []
    for f, a, b in zip(feats, gl, gd):
        lg, dl = head.forward_level(f)
        outs += [lg.detach(), dl.detach()]
        total = total + (lg * torch.from_numpy(a).to(DEV)).sum() + (dl * torch.from_numpy(b).to(DEV)).sum()
    total.backward()
    grads = {k: p.grad for k, p in head.named_parameters()}
    grads.update({f"input{i}": f.grad for i, f in enumerate(feats)})
    return outs, grads, {k: v.detach().cpu().double() for k, v in head.named_parameters()}


def test_rpn_head_stage():
    rng = np.random.RandomState(2)
    shapes, B = [(5, 7), (1, 1)], 2
    xs = [rng.normal(0, 1, size=(B, h, w, 64)).astype(np.float32) for h, w in shapes]
    gl = [rng.normal(0, 1, size=(B, h * w * 3)).astype(np.float32) for h, w in shapes]
    gd = [rng.normal(0, 1, size=(B, h * w * 3, 4)).astype(np.float32) for h, w in shapes]
    o32, g32, params = _rpn_run("f32", xs, gl, gd)
    o16, g16, _ = _rpn_run("bf16", xs, gl, gd)
    assert all(torch.equal(p, q) for p, q in zip(o32, o16))
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
    for k in want:
        e = _rel(g16[k], want[k])
        print(f"rpn head {k}: bf16 setting {e:.3e}, f32 setting {_rel(g32[k], want[k]):.3e}")
        # the only bf16 dgrad of the stage is the 3x3's, the last GEMM of its backward: no bias gradient has one upstream
        assert e < (F32_GATE if k.endswith("bias") else BF16_GATE), k
    for k in params:
        assert torch.equal(g16[k], g32[k]), k                                              # weight and bias gradients: the same bits
    assert not torch.equal(g16["input0"], g32["input0"]) and not torch.equal(g16["input1"], g32["input1"])
    again = _rpn_run("bf16", xs, gl, gd)[1]
    assert all(torch.equal(again[k], g16[k]) for k in g16)


def _fpn_run(grad_dtype, cfg, w, x, ws):
    torch.manual_seed(0)
    m = DiTWithFPN(config=cfg, compute_dtype="f32", grad_dtype=grad_dtype)
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
    return m, {k: f.detach() for k, f in feats.items()}, grads, enc, ws


def test_fpn_stage():
    """DiTWithFPN at the micro geometry of tests/test_gpu_fpn.py::test_dit_with_fpn_trains_like_the_reference."""
    from oracle.vit_oracle_torch import train_reference
    cfg = cfgs.vit_micro()
    cfg.drop_path_rate = 0.0
    cfg.taps = [1, 1, 2, 3]
    w = synth.synth_weights(cfg, 3)
    B, size, g = 2, 64, 4
    x = synth.synth_images(B, size, size, seed=5, kind="uniform")
    m, f32_, g32, e32, ws = _fpn_run("f32", cfg, w, x, None)
    _, f16_, g16, e16, _ = _fpn_run("bf16", cfg, w, x, ws)
    assert all(torch.equal(f32_[k], f16_[k]) for k in f32_)
    taps_np, _ = oracle.vit_forward(cfg, w, x)
    taps_t = [torch.from_numpy(t).double().requires_grad_(True) for t in taps_np]
    wt = {k: p.detach().cpu().double().requires_grad_(True) for k, p in m.fpn.named_parameters()}
    ref = fpn_forward_t(backbone_maps_t(taps_t, g, g), wt)
    sum((ref[k] * ws[k].double()).sum() for k in ref).backward()
    for k, r in wt.items():
        e = _rel(g16[k], r.grad)
        print(f"fpn {k}: bf16 setting {e:.3e}, f32 setting {_rel(g32[k], r.grad):.3e}")
        assert e < BF16_GATE, k
    _, enc_ref = train_reference(cfg, w, x, [t.grad.float().numpy() for t in taps_t], taps=m.backbone.layer_idxs)
    for short, hf in (("0.w1", "encoder.layer.0.intermediate.dense.weight"), ("2.wq", "encoder.layer.2.attention.attention.query.weight"),
                      ("patch_w", "embeddings.patch_embeddings.projection.weight"), ("1.lam2", "encoder.layer.1.lambda_2"),
                      ("pos", "embeddings.position_embeddings")):
        e = rel_l2(e16[short].cpu().numpy(), enc_ref[hf])
        print(f"fpn -> encoder {short}: bf16 setting {e:.3e}, f32 setting {rel_l2(e32[short].cpu().numpy(), enc_ref[hf]):.3e}")
        assert e < BF16_GATE, short
    # the four 3x3 convolutions are the stage's outputs: their weight and bias gradients see no dgrad at all
    for i in range(4):
        for leaf in ("weight", "bias"):
            assert torch.equal(g16[f"layer_blocks.{i}.0.{leaf}"], g32[f"layer_blocks.{i}.0.{leaf}"])
    assert not torch.equal(g16["inner_blocks.0.0.weight"], g32["inner_blocks.0.0.weight"])
    assert not torch.equal(e16["patch_w"], e32["patch_w"])
    _, _, again, enc_again, _ = _fpn_run("bf16", cfg, w, x, ws)
    assert all(torch.equal(again[k], g16[k]) for k in g16) and all(torch.equal(enc_again[k], e16[k]) for k in e16)


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _model(grad_dtype="f32"):
    """The smallest detector of tests/test_gpu_detector_step.py, identically initialised every time."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, grad_dtype=grad_dtype)
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


def test_model_gradients_follow_the_f32_setting(batch):
    model = _model()
    l32, g32 = _losses_and_grads(model, batch)
    assert model.set_grad_dtype("bf16").grad_dtype == "bf16"
    l16, g16 = _losses_and_grads(model, batch)
    assert sorted(l32) == sorted(l16) and all(torch.equal(l32[k], l16[k]) for k in l32)    # losses, samples, proposals: the same bits
    assert [n for n in g32 if g32[n] is not None] == [n for n in g16 if g16[n] is not None]
    worst, changed = ("", 0.0), 0
    for n, a in g32.items():
        if a is None or not bool(a.any()):
            continue
        e = _rel(g16[n], a)
        changed += int(not torch.equal(g16[n], a))
        if e > worst[1]:
            worst = (n, e)
        assert e < BF16_GATE, (n, e)
    print(f"detector: worst parameter gradient, bf16 against f32 setting: {worst[0]} {worst[1]:.3e}; {changed} tensors changed")
    assert changed > 40                                                                    # the encoder, the laterals, fc6: every stage below a dgrad
    # eval mode and no_grad never read the option
    model.eval()
    with torch.no_grad():
        a = model.forward_padded(torch.from_numpy(synth.synth_images(2, 224, 224, seed=3, kind="uniform")).to(DEV))
        model.set_grad_dtype("f32")
        b = model.forward_padded(torch.from_numpy(synth.synth_images(2, 224, 224, seed=3, kind="uniform")).to(DEV))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_twenty_steps_in_bf16_setting_lower_the_loss(batch):
    model = _model("bf16")
    step = DetectorTrainStep(model, lr=1e-3)
    head = model.model.roi_heads.box_head
    history, fc6_grads, stale = [], [], 0
    for i in range(20):
        history.append(step.step(*batch, generator=_seeded(2)))
        if i < 2:
            fc6_grads.append(head.fc6.bias.grad.detach().clone())
            # after apply() the cached dgrad operand is gone; the next backward re-makes it from the weights as they are now
            m = model.model
            assert not any(s._operand_cache.filled() for s in (head, m.roi_heads.box_predictor, m.rpn.head, m.backbone))
            fresh = head.dgrad_operands_bf16(256, 7, 7)[1]
            stale += int(not torch.equal(fresh, ops.cast_bf16(head.fc7.weight.detach().t().contiguous())))
            head._operand_cache.clear()
    totals = [float(sum(v.item() for v in h.values())) for h in history]
    print("summed loss over 20 steps, bf16 setting:", [round(v, 4) for v in totals], "steps", step.steps, "skipped", step.skipped_steps)
    assert all(np.isfinite(v.item()) for h in history for v in h.values())
    assert step.steps + step.skipped_steps == 20 and step.steps > 0
    assert totals[-1] < totals[0]
    assert stale == 0 and not torch.equal(fc6_grads[0], fc6_grads[1])                      # the second step's gradients are its own
