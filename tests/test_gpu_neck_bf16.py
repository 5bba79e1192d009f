"""The bf16 eval-mode neck on the GPU: ldit_conv3x3_nhwc_bf16 - the implicit-im2col mode of the bf16 MFMA GEMM on
the zero-padded bf16 map of ldit_pad_nhwc_f32_bf16 - and neck_dtype="bf16" of DiTWithFPN / RPNHead / LayoutDetectionModel.

Footprint coverage (the line tests/test_gpu_footprint.py's table would carry):
  ldit_conv3x3_nhwc_bf16         here    1x1 / 5x9 / 7x7 maps, EPI_F32 (ldy > Cout) / EPI_BIAS / EPI_BIAS_RELU, ragged N, tile auto and 3

The main gate is a bit-equality with code the suite already pins: the kernel walks k = (tap, channel) in 64-deep tiles through the
row-major kernel's own pipeline, so its result IS ops.linear_bf16 with the same epilogue on the im2col matrix built (with torch
indexing) from the same padded bf16 map.  The numeric gates are derived, not observed: against float64 on the bf16-rounded operands
the worst-case fp32 accumulation error over K = 9 Cin terms, K 2^-24 S with S = conv(|x|, |w|) + |b|, plus 2^-8 |ref| (half a bf16
ulp, doubled) where the result is stored as bf16; against the fp32 path on the unrounded operands the project's bf16 gate, rel-L2
2e-2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import _lib, ops, synth           # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel    # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402
from tests import guarded                             # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402
from tests.guarded import In, Out                     # noqa: E402
from tests.util import rel_l2                         # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
EF32, BIAS, RELU = _lib.EPI_F32, _lib.EPI_BIAS, _lib.EPI_BIAS_RELU
EPILOGUES = {"f32": EF32, "bias": BIAS, "relu": RELU}
SWITCHES = ("LDIT_GEMM_BF16_TILE",)
# (B, H, W, Cin, Cout): eight taps all padding and M <= 64 | W no multiple of the 8-row DMA piece (pieces straddle image rows and
# the image boundary), ragged N | two k-tiles per tap | 392 rows: a full 256-row tile plus a ragged one, a tile that straddles two
# images, four k-tiles per tap | the RPN head's stacked-width N
SHAPES = [(1, 1, 1, 64, 64), (2, 5, 9, 64, 50), (2, 7, 7, 128, 256), (2, 14, 14, 256, 256), (3, 4, 4, 256, 16)]


@pytest.fixture(autouse=True)
def _cleanup():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()
    yield
    for s in SWITCHES:
        _lib.set_switch(s, None)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rand(seed, *shape, scale=1.0):
    """Zero-mean normal values (synth's counter-based generator: the same on every box)."""
    return (scale * synth.normal(seed, 9, int(np.prod(shape)))).astype(np.float32).reshape(shape)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(shape):
    """fp32 x [B, H, W, Cin], w [Cout, 3, 3, Cin] and bias, zero-mean so that about half of the outputs are negative; their bf16 forms
    (the padded map as the library writes it, the weight as the library casts it) and the im2col matrix of the padded map.  Made
    once per shape and left unchanged."""
    if shape not in _CASES:
        B, H, W, Cin, Cout = shape
        x = _dev(_rand(1 + H * W, B, H, W, Cin))
        w = _dev(_rand(2 + Cout, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5))
        b = _dev(_rand(3 + Cin, Cout, scale=0.1))
        xp = ops.pad_nhwc_bf16(x)
        w16 = ops.cast_bf16(w)
        img = xp.view(B, H + 2, W + 2, Cin)
        cols = torch.cat([img[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)], dim=3).reshape(B * H * W, 9 * Cin).contiguous()
        _CASES[shape] = dict(x=x, w=w, b=b, xp=xp, w16=w16, cols=cols)
    return _CASES[shape]


def test_padded_map_is_the_rounded_map_in_a_zero_frame():
    """What the gates below build on: the padded map holds bf16(x) inside and bf16 +0 on the frame, in every bit."""
    B, H, W, Cin, _ = shape = SHAPES[1]
    c = _case(shape)
    img = c["xp"].view(B, H + 2, W + 2, Cin)
    assert torch.equal(img[:, 1:-1, 1:-1], c["x"].to(BF))
    frame = img.clone()
    frame[:, 1:-1, 1:-1] = 0
    assert not frame.view(torch.int16).any()


@pytest.mark.parametrize("tile", ["auto", "2", "3", "4", "5"])
@pytest.mark.parametrize("epi", sorted(EPILOGUES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_is_the_row_major_gemm_on_the_im2col_matrix(shape, epi, tile):
    B, H, W, Cin, Cout = shape
    c = _case(shape)
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_BF16_TILE", tile)
    got = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], EPILOGUES[epi])
    again = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], EPILOGUES[epi])
    want = ops.linear_bf16(c["cols"], c["w16"].view(Cout, 9 * Cin), c["b"], EPILOGUES[epi])
    assert got.dtype == (torch.float32 if epi == "f32" else BF) and tuple(got.shape) == (B * H * W, Cout) and got.is_contiguous()
    assert torch.equal(got, want)                                                                   # the main gate
    assert torch.equal(got, again)                                                                  # two runs bit-identical
    if epi == "relu":
        plain = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], BIAS)
        clamped, positive = int((plain.float() < 0).sum()), int((plain.float() > 0).sum())
        assert clamped > 0 and positive > 0, (clamped, positive)                                    # the case exercises both branches
        assert torch.equal(got, torch.relu(plain)) and not (got.view(torch.int16) < 0).any()        # relu of EPI_BIAS, bit for bit
    else:
        assert int((got.float() < 0).sum()) > 0 and int((got.float() > 0).sum()) > 0


def test_conv_without_a_bias():
    B, H, W, Cin, Cout = shape = SHAPES[1]
    c = _case(shape)
    got = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], None, EF32)
    assert torch.equal(got, ops.linear_bf16(c["cols"], c["w16"].view(Cout, 9 * Cin), None, EF32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_matches_float64_and_the_fp32_path(shape):
    B, H, W, Cin, Cout = shape
    c = _case(shape)
    K = 9 * Cin
    x64 = c["xp"].view(B, H + 2, W + 2, Cin)[:, 1:-1, 1:-1].double().cpu().permute(0, 3, 1, 2)      # the bf16-rounded operands
    w64, b64 = c["w16"].double().cpu().permute(0, 3, 1, 2), c["b"].double().cpu()
    ref = F.conv2d(x64, w64, b64, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    S = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1).permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    for name, e in sorted(EPILOGUES.items()):
        got = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], e).double().cpu()
        want = torch.relu(ref) if e == RELU else ref
        gate = K * 2.0 ** -24 * S + (0.0 if e == EF32 else 2.0 ** -8) * ref.abs()
        err = (got - want).abs()
        print(f"conv {shape} {name} vs float64 on the bf16 operands: largest |err| / gate {float((err / gate).max()):.3f}")
        assert (err <= gate).all(), name
    got = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], EF32)
    f32 = ops.conv3x3_nhwc(c["x"], c["w"], c["b"]).view(B * H * W, Cout)
    err = rel_l2(got.cpu().numpy(), f32.cpu().numpy())
    print(f"conv {shape} bf16 vs the fp32 kernel on the unrounded operands: rel-L2 {err:.3e}")
    assert err <= 2e-2


# ---- 2. footprint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["auto", "3"])
@pytest.mark.parametrize("epi", sorted(EPILOGUES))
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_conv_footprint(shape, epi, tile):
    """Surroundings 0x00 then 0xFF: outputs bit-equal, the 0xA5 bands around the output (its gap columns included) and every input
    parent untouched, every output element written and finite - and the strided output holds the dense call's bits."""
    B, H, W, Cin, Cout = shape
    c = _case(shape)
    lib = _lib.load()
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_BF16_TILE", tile)
    e = EPILOGUES[epi]
    ldy = Cout + 8 if e == EF32 else (Cout + 7) // 8 * 8 + 16
    specs = dict(xp=In(c["xp"].cpu()), w=In(c["w16"].cpu().view(Cout, 9 * Cin)), b=In(c["b"].cpu()),
                 y=Out((B * H * W, Cout), torch.float32 if e == EF32 else BF, ld=ldy))

    def call(t):
        _lib.check(lib.ldit_conv3x3_nhwc_bf16(t["xp"].data_ptr(), t["w"].data_ptr(), t["b"].data_ptr(), t["y"].data_ptr(), ldy, B, H, W, Cin,
                                              Cout, e, torch.cuda.current_stream().cuda_stream))

    res = guarded.twin_run(specs, call, device=DEV, sync=torch.cuda.synchronize)
    guarded.assert_written(res.poisoned["y"], "y")
    guarded.assert_finite(res.poisoned["y"], "y")
    dense = ops.conv3x3_nhwc_bf16(c["xp"], B, H, W, c["w16"], c["b"], e)
    assert torch.equal(res.clean["y"], dense.cpu())


# ---- 3. large row indices --------------------------------------------------------------------------------------------------------------
def test_full_size_rows_of_the_last_image():
    """B = 64, 56 x 56, 256 -> 256 (the p2 level of the flagship batch): 200 704 rows, a padded map of 55 M elements.  The rows of the
    first and the last image equal that image convolved alone - a wrong row mapping or a wrapped offset cannot pass."""
    B, H, W, Cc = 64, 56, 56, 256
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    x = torch.randn(B, H, W, Cc, device=DEV, generator=g)
    w16 = (torch.randn(Cc, 3, 3, Cc, device=DEV, generator=g) * 0.02).to(BF)
    b = torch.randn(Cc, device=DEV, generator=g) * 0.1
    y = ops.conv3x3_nhwc_bf16(ops.pad_nhwc_bf16(x), B, H, W, w16, b, EF32)
    assert tuple(y.shape) == (B * H * W, Cc) and bool(torch.isfinite(y).all())
    for i in (0, B - 1):
        alone = ops.conv3x3_nhwc_bf16(ops.pad_nhwc_bf16(x[i:i + 1].contiguous()), 1, H, W, w16, b, EF32)
        assert torch.equal(y[i * H * W:(i + 1) * H * W], alone) and alone.abs().max() > 0, i


# ---- 4. the modules --------------------------------------------------------------------------------------------------------------------
def _randomise_neck(model, gen_seed=13):
    """Non-trivial neck weights: the FPN's zero biases and the RPN head's 0.01-std weights made random values of ordinary size."""
    g = torch.Generator()
    g.manual_seed(gen_seed)
    m = model.model
    with torch.no_grad():
        for blk in list(m.backbone.fpn.inner_blocks) + list(m.backbone.fpn.layer_blocks):
            blk[0].bias.copy_(torch.randn(blk[0].bias.shape, generator=g) * 0.1)
        for p in m.rpn.head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))


@pytest.fixture(scope="module")
def detector():
    """Hidden 128, 3 layers, B = 2, 224 x 224, random neck weights - plus the fp32 neck's results, computed once and left unchanged."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    _randomise_neck(model)
    with torch.no_grad():
        pred = model.model.roi_heads.box_predictor
        pred.cls_score.weight.copy_(torch.randn_like(pred.cls_score.weight) * 0.3)
        pred.bbox_pred.weight.copy_(torch.randn_like(pred.bbox_pred.weight) * 0.2)
    model = model.to(DEV).eval()
    batch = torch.from_numpy(synth.synth_images(2, 224, 224, seed=77)).to(DEV)
    m = model.model
    with torch.no_grad():
        assert model.neck_dtype == "f32"
        feats = {k: v.clone(memory_format=torch.preserve_format) for k, v in m.backbone(batch).items()}
        levels = [m.rpn.head.forward_level(f) for f in feats.values()]
        ref = {"feats": feats, "levels": [(a.clone(), b.clone()) for a, b in levels],
               "det32": tuple(t.clone() for t in model.forward_padded(batch))}
    return model, batch, ref


@pytest.fixture()
def bf16_detector(detector):
    model, batch, ref = detector
    model.set_neck_dtype("bf16")
    yield model, batch, ref
    model.set_neck_dtype("f32")


def test_bf16_fpn_maps(bf16_detector):
    model, batch, ref = bf16_detector
    with torch.no_grad():
        got = model.model.backbone(batch)
        again = model.model.backbone(batch)
    assert list(got) == list(ref["feats"]) == ["p2", "p3", "p4", "p5", "pool"]
    for k, want in ref["feats"].items():
        g = got[k]
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(want.shape) and torch.equal(g, again[k])
        if k != "pool":
            assert g.stride() == want.stride() and g.permute(0, 2, 3, 1).is_contiguous()            # channels-last, as the fp32 path's
            err = rel_l2(g.cpu().numpy(), want.cpu().numpy())
            print(f"FPN {k} bf16 vs fp32: rel-L2 {err:.3e}")
            assert err <= 2e-2 and not torch.equal(g, want)
    p5, pool = got["p5"], got["pool"]
    assert pool.data_ptr() == p5.data_ptr() and pool.stride() == p5[:, :, ::2, ::2].stride() and torch.equal(pool, p5[:, :, ::2, ::2])


def test_bf16_rpn_head(bf16_detector):
    model, batch, ref = bf16_detector
    head = model.model.rpn.head
    A = head.num_anchors
    with torch.no_grad():
        for (k, f), (l32, d32) in zip(ref["feats"].items(), ref["levels"]):                          # the fp32 maps in, either head
            l16, d16 = head.forward_level(f)
            l16b, d16b = head.forward_level(f)
            assert l16.dtype == d16.dtype == torch.float32
            assert tuple(l16.shape) == tuple(l32.shape) and tuple(d16.shape) == tuple(d32.shape)
            assert l16.stride() == l32.stride() and d16.stride() == d32.stride()
            assert torch.equal(l16, l16b) and torch.equal(d16, d16b)
            el, ed = rel_l2(l16.cpu().numpy(), l32.cpu().numpy()), rel_l2(d16.cpu().numpy(), d32.cpu().numpy())
            print(f"RPN head on {k} bf16 vs fp32: logits rel-L2 {el:.3e}, deltas rel-L2 {ed:.3e}")
            assert el <= 2e-2 and ed <= 2e-2 and not torch.equal(l16, l32)
        # the stacked 1x1 matrix: 5 A = 15 rows padded to 16; the padding row and its output column stay exactly zero
        w3, b3, w1, b1 = head._operands_bf16()
        assert w3.dtype == w1.dtype == BF and b3.dtype == b1.dtype == torch.float32 and tuple(w1.shape) == (16, 256)
        assert not w1[5 * A:].view(torch.int16).any() and not b1[5 * A:].any()
        f = ref["feats"]["p4"]
        B, Cc, h, w = f.shape
        xn = f.permute(0, 2, 3, 1).contiguous()
        t = ops.conv3x3_nhwc_bf16(ops.pad_nhwc_bf16(xn), B, h, w, w3, b3, RELU)
        y = ops.linear_bf16(t, w1, b1, EF32)
        assert t.dtype == BF and float(t.float().min()) == 0.0 and not y[:, 5 * A:].any()
        assert torch.equal(head.forward_level(f)[0], y[:, :A].reshape(B, h * w * A))


def _iou(a, b):
    lt, rb = torch.maximum(a[:, None, :2], b[None, :, :2]), torch.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(dim=2)
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])                                      # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def test_bf16_detector_runs_and_the_fp32_default_comes_back(detector):
    model, batch, ref = detector
    model.set_neck_dtype("bf16")
    try:
        with torch.no_grad():
            got = model.forward_padded(batch)
            again = model.forward_padded(batch)
            for g, a in zip(got, again):
                assert torch.equal(g, a)                                                            # two runs bit-identical
            # reported, not gated (top-k and NMS are discontinuous): detections with a same-label partner of IoU >= 0.9 under the
            # other setting
            d32, n = ref["det32"], got[3].tolist()
            for b in range(2):
                n16, n32 = n[b], int(d32[3][b])
                if n16 and n32:
                    hit = (_iou(got[0][b, :n16], d32[0][b, :n32]) >= 0.9) & (got[2][b, :n16, None] == d32[2][b, None, :n32])
                    print(f"image {b}: {int(hit.any(dim=1).sum())} of {n16} bf16-neck detections have an fp32 partner (same label, "
                          f"IoU >= 0.9); {int(hit.any(dim=0).sum())} of {n32} fp32 detections have a bf16-neck partner")
                else:
                    print(f"image {b}: {n16} bf16-neck detections, {n32} fp32 detections")
            # ragged images through forward: the padded form scaled back
            rng = np.random.RandomState(5)
            images = [_dev(rng.rand(3, 180, 300).astype(np.float32)), _dev(rng.rand(3, 333, 211).astype(np.float32))]
            out = model(images)
            pb, ps, pl, pc = model.forward_padded(model.model.transform(images)[0].tensors)
            assert len(out) == 2
            for i, d in enumerate(out):
                k = int(pc[i])
                assert set(d) == {"boxes", "labels", "scores"} and tuple(d["boxes"].shape) == (k, 4)
                assert torch.equal(d["scores"], ps[i, :k]) and torch.equal(d["labels"], pl[i, :k].long())
    finally:
        model.set_neck_dtype("f32")
    with torch.no_grad():
        det32 = model.forward_padded(batch)
        feats = model.model.backbone(batch)
    for g, w in zip(det32, ref["det32"]):
        assert torch.equal(g, w)                                                                    # the fp32 detections, bit for bit
    for k, w in ref["feats"].items():
        assert torch.equal(feats[k], w)


def test_bf16_padded_detector_is_graph_capturable(bf16_detector):
    model, batch, _ = bf16_detector
    other = torch.from_numpy(synth.synth_images(2, 224, 224, seed=78)).to(DEV)
    with torch.no_grad():
        eager = [tuple(t.clone() for t in model.forward_padded(x)) for x in (batch, other)]         # the eager call fills every cache
        static_x = batch.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.forward_padded(static_x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = model.forward_padded(static_x)
        for x, want in zip((other, batch), reversed(eager)):
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(static_out, want):
                assert torch.equal(a, b)


# ---- 5. training untouched, caches invalidated -----------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _train_model(neck_dtype="f32"):
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, neck_dtype=neck_dtype)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    _randomise_neck(model)
    return model.to(DEV).train()


@pytest.fixture(scope="module")
def train_batch():
    images = [torch.from_numpy(synth.synth_images(1, 120, 200, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 224, 224, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV),
                "labels": torch.tensor([1, 3], device=DEV)},
               {"boxes": torch.from_numpy(np.ascontiguousarray(to.scene(7, 7))).to(DEV),
                "labels": torch.from_numpy(np.arange(7, dtype=np.int64) % 5 + 1).to(DEV)}]
    return images, targets


def test_losses_and_gradients_do_not_depend_on_neck_dtype(train_batch):
    model = _train_model()

    def run():
        model.zero_grad(set_to_none=True)
        losses = model.losses(*train_batch, generator=_seeded(2))
        sum(losses.values()).backward()
        return {k: v.detach().clone() for k, v in losses.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    l32, g32 = run()
    model.set_neck_dtype("bf16")
    l16, g16 = run()
    assert sorted(l32) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    for k in l32:
        assert torch.equal(l32[k], l16[k]), k
    assert sorted(g32) == sorted(g16) and any("fpn.layer_blocks" in k for k in g32) and any("rpn.head.conv" in k for k in g32)
    for k in g32:
        assert torch.equal(g32[k], g16[k]), k


def test_train_step_invalidates_the_bf16_neck_operands(train_batch):
    model = _train_model("bf16")
    x = torch.from_numpy(synth.synth_images(2, 224, 224, seed=31, kind="uniform")).to(DEV)
    bb, head = model.model.backbone, model.model.rpn.head

    def neck_out(mod):
        with torch.no_grad():
            feats = mod.model.backbone(x)
            return feats["p2"].clone(), mod.model.rpn.head.forward_level(feats["p3"])[0].clone()

    model.eval().forward_padded(x)                                                                  # fills the bf16 caches with the old weights
    before = neck_out(model)
    assert all(bb._operand_cache.filled(("ohwi_bf16", i)) for i in range(4)) and head._operand_cache.filled("bf16")
    model.train()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=1024.0)
    step.step(*train_batch, generator=_seeded(2))
    assert step.steps == 1
    fresh = _train_model("bf16")
    fresh.load_state_dict(model.state_dict())
    after, want = model.eval().forward_padded(x), fresh.eval().forward_padded(x)
    for got, w in zip(after, want):
        assert torch.equal(got, w)
    got, want = neck_out(model), neck_out(fresh)
    for g, w, b in zip(got, want, before):
        assert torch.equal(g, w) and not torch.equal(g, b)                                          # a stale bf16 operand fails here
