"""The bf16 eval-mode box head on the GPU: ldit_roi_align_levels_bf16, LDIT_EPI_BIAS_RELU of the bf16 GEMM,
EPI_F32 through ops.linear_bf16, and head_dtype="bf16" of RoIHeads / LayoutDetectionModel.

Most gates are bit-equalities with code the suite already pins against an oracle: the bf16 pooled rows ARE the fp32 kernel's rows
rounded to nearest even; the ReLU epilogue IS relu of the EPI_BIAS output (the max sits on the fp32 value and rounding to bf16 is
monotone and keeps the sign).  The numeric gates are derived, not observed: a bf16 result carries half an ulp (2^-9 relative, doubled
for slack) on top of the worst-case fp32 accumulation error K 2^-24 sum |x| |w|; whole chains use the project's bf16 gate, rel-L2 2e-2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import _lib, ops, synth           # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import FastRCNNPredictor, LayoutDetectionModel, TwoMLPHead    # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402
from tests import roi_oracle as roi                   # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402
from tests.util import max_rel, rel_l2                # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
NC = 6
GEOMETRIES = {(224, 224): [(56, 56), (28, 28), (14, 14), (7, 7)], (96, 160): [(24, 40), (12, 20), (6, 10), (3, 5)]}
SWITCHES = ("LDIT_GEMM_BF16_TILE", "LDIT_GEMM_BF16_TAIL_LAUNCH", "LDIT_GEMM_DIRECT_EPILOGUE")


@pytest.fixture(autouse=True)
def _cleanup():
    _lib.load()
    yield
    for s in SWITCHES:
        _lib.set_switch(s, None)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rand(seed, *shape, scale=1.0):
    """Zero-mean normal values (synth's counter-based generator: the same on every box)."""
    return (scale * synth.normal(seed, 9, int(np.prod(shape)))).astype(np.float32).reshape(shape)


# ---- 1. RoIAlign -------------------------------------------------------------------------------------------------------------------
def _feature_maps(seed, image_size, B, Cc, batch_step=1):
    rng = np.random.RandomState(seed)
    feats = []
    for h, w in GEOMETRIES[image_size]:
        nhwc = _dev(rng.normal(0, 1.5, size=(B * batch_step, h, w, Cc)).astype(np.float32))
        feats.append(nhwc[::batch_step].permute(0, 3, 1, 2))
    feats.append(feats[3][:, :, ::2, ::2])
    return feats


def _roi_case(image_size, R, Cc, batch_step=1):
    B = 2
    feats = _feature_maps(7 * R + Cc, image_size, B, Cc, batch_step)
    sizes = [tuple(f.shape[-2:]) for f in feats]
    boxes = np.stack([roi.make_boxes(100 * R + b, R, image_size, sizes)[0] for b in range(B)])
    return feats, _dev(boxes), _dev(np.asarray([R, R // 2], dtype=np.int32))


def _check_bf16_rows(feats, boxes, count, image_size, R):
    for cnt in (count, None):
        want, want_lv = ops.roi_align_levels(feats, boxes, cnt, image_size, return_levels=True)
        got, got_lv = ops.roi_align_levels(feats, boxes, cnt, image_size, return_levels=True, out_dtype=BF)
        again = ops.roi_align_levels(feats, boxes, cnt, image_size, out_dtype=BF)
        assert got.dtype == BF and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
        assert torch.equal(got, want.to(BF))                                                        # the fp32 kernel's value, rounded once
        assert torch.equal(got_lv, want_lv) and torch.equal(got, again)                             # levels unchanged; bit-reproducible
        assert got.float().abs().max() > 0
    got = ops.roi_align_levels(feats, boxes, count, image_size, out_dtype=BF)
    half = R // 2
    assert not got[R + half:].view(torch.int16).any()                                               # padding rows: bf16 +0, every bit


@pytest.mark.parametrize("Cc", [12, 256, 264])            # 264: the smallest width that runs the second channel pass
@pytest.mark.parametrize("R", [1, 37, 130])
@pytest.mark.parametrize("image_size", [(224, 224), (96, 160)])
def test_bf16_roi_align_is_the_fp32_kernel_rounded_at_the_store(image_size, R, Cc):
    feats, boxes, count = _roi_case(image_size, R, Cc)
    _check_bf16_rows(feats, boxes, count, image_size, R)


def test_fp32_roi_align_second_channel_pass_matches_the_oracle():
    """C = 264 > 256: lanes 0 and 1 take a second pass over the channels - neither dtype was tested there.  The fp32 rows against the
    float64 oracle at the existing gate (2^-13 max |map|); the bf16 rows are pinned to the fp32 ones above."""
    feats, boxes, count = _roi_case((224, 224), 37, 264)
    out, levels = ops.roi_align_levels(feats, boxes, count, (224, 224), return_levels=True)
    maps = [f.permute(0, 2, 3, 1).cpu().numpy() for f in feats]
    ref, ref_levels = roi.roi_align_levels(maps, boxes.cpu().numpy(), count.cpu().numpy(), (224, 224))
    np.testing.assert_array_equal(levels.cpu().numpy(), ref_levels)
    peak = max(float(np.abs(m).max()) for m in maps)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"roi_align C=264: max abs err {err:.3e}, bound {2.0 ** -13 * peak:.3e}")
    assert err <= 2.0 ** -13 * peak


def test_bf16_roi_align_with_a_non_contiguous_batch_stride():
    feats, boxes, count = _roi_case((224, 224), 37, 256, batch_step=2)
    assert feats[0].stride(0) == 2 * 56 * 56 * 256
    _check_bf16_rows(feats, boxes, count, (224, 224), 37)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.roi_align_levels(feats, boxes, count, (224, 224), out_dtype=torch.float16)


# ---- 2. the ReLU epilogue ----------------------------------------------------------------------------------------------------------
_OPERANDS = {}


def _operands(M, N, K):
    """bf16 x, w and an fp32 bias, all zero-mean so that about half of the outputs are clamped; made once per shape."""
    if (M, N, K) not in _OPERANDS:
        x = _dev(_rand(1 + M, M, K)).to(BF)
        w = _dev(_rand(2 + N, N, K, scale=0.05)).to(BF)
        b = _dev(_rand(3 + K, N, scale=0.1))
        _OPERANDS[(M, N, K)] = (x, w, b)
    return _OPERANDS[(M, N, K)]


def _relu_equals_relu_of_bias(M, N, K):
    x, w, b = _operands(M, N, K)
    plain = ops.linear_bf16(x, w, b, _lib.EPI_BIAS)
    got = ops.linear_bf16(x, w, b, _lib.EPI_BIAS_RELU)
    assert got.dtype == BF and tuple(got.shape) == (M, N)
    clamped, positive = int((plain.float() < 0).sum()), int((plain.float() > 0).sum())
    assert clamped > 0 and positive > 0, (clamped, positive)                                        # the case exercises both branches
    assert torch.equal(got, torch.relu(plain))                                                      # relu of the EPI_BIAS output, bit for bit
    assert not (got.view(torch.int16) < 0).any()                                                    # no sign bit survives
    return got


@pytest.mark.parametrize("tile", ["auto", "1", "2", "3", "4", "5"])
@pytest.mark.parametrize("M,N,K", [(37, 50, 64), (394, 576, 192), (513, 3072, 768), (2000, 1024, 12544)])
def test_relu_epilogue_is_relu_of_the_bias_epilogue(M, N, K, tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_BF16_TILE", tile)
    _relu_equals_relu_of_bias(M, N, K)


@pytest.mark.parametrize("M,N,K", [(16, 1024, 1024), (37, 200, 256)])
def test_relu_epilogue_on_the_tail_kernel(M, N, K):
    _relu_equals_relu_of_bias(M, N, K)


@pytest.mark.parametrize("tail_launch", [None, "1"])
def test_relu_epilogue_on_the_peeled_tail(tail_launch):
    """M = 1040 = 4 x 256 + 16 at N = 1024: the 16 rows are peeled - riding in the main launch, or (switch) as a launch of their own."""
    _lib.set_switch("LDIT_GEMM_BF16_TAIL_LAUNCH", tail_launch)
    got = _relu_equals_relu_of_bias(1040, 1024, 1024)
    _lib.set_switch("LDIT_GEMM_BF16_TAIL_LAUNCH", None)
    x, w, b = _operands(1040, 1024, 1024)
    alone = ops.linear_bf16(x[-16:].contiguous(), w, b, _lib.EPI_BIAS_RELU)
    assert torch.equal(got[-16:], alone)                                                            # the tail / tile contract holds for it


@pytest.mark.parametrize("M,N,K", [(394, 576, 192), (513, 3072, 768), (1040, 1024, 1024)])
def test_relu_epilogue_direct_stores_equal_the_slab_path(M, N, K):
    slab = _relu_equals_relu_of_bias(M, N, K)
    _lib.set_switch("LDIT_GEMM_DIRECT_EPILOGUE", "1")
    direct = _relu_equals_relu_of_bias(M, N, K)
    assert torch.equal(slab, direct)


def test_relu_epilogue_matches_float64():
    """test_linear_bf16_bias's own gate (rel-L2 3e-3, element-wise 1.6e-2 of max(|ref|, 1)) against float64 on the bf16-rounded
    operands."""
    M, N, K = 394, 576, 192
    x, w, b = _operands(M, N, K)
    got = ops.linear_bf16(x, w, b, _lib.EPI_BIAS_RELU).float().cpu().numpy()
    ref = torch.relu(x.double().cpu() @ w.double().cpu().T + b.double().cpu()).numpy()
    print(f"relu epilogue vs float64: rel-L2 {rel_l2(got, ref):.3e}, max rel {max_rel(got, ref):.3e}")
    assert rel_l2(got, ref) < 3e-3 and max_rel(got, ref) < 1.6e-2


@pytest.mark.parametrize("N", [30, 32])
def test_f32_epilogue_through_linear_bf16(N):
    M, K = 74, 1024
    x, w, b = _operands(M, N, K)
    got = ops.linear_bf16(x, w, b, _lib.EPI_F32)
    assert got.dtype == torch.float32 and tuple(got.shape) == (M, N)
    ref = (x.double().cpu() @ w.double().cpu().T + b.double().cpu()).numpy()
    err = rel_l2(got.cpu().numpy(), ref)
    print(f"EPI_F32 through linear_bf16, N={N}: rel-L2 {err:.3e}")
    assert err < 2e-5


# ---- 3. the head at M = 74 -----------------------------------------------------------------------------------------------------------
def _stage_gate(name, got, x, w, b, K, relu):
    """|got - relu(ref)| <= 2^-8 |ref| + K 2^-24 S per element, ref = float64 on the device's own bf16 input and the bf16-rounded
    weight, S = |x| @ |w|^T: half a bf16 ulp (2^-9) doubled, plus the worst-case fp32 accumulation error over K terms."""
    x64, w64 = x.double().cpu(), w.double().cpu()
    ref = x64 @ w64.T + b.double().cpu()
    S = x64.abs() @ w64.abs().T
    want = torch.relu(ref) if relu else ref
    gate = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * S
    err = (got.double().cpu() - want).abs()
    live = gate > 0                                                                                 # (a padding column has ref = S = 0: exact)
    print(f"{name}: largest |err| / gate {float((err[live] / gate[live]).max()):.3f}")
    assert (err <= gate).all(), name


def test_bf16_head_gemms_match_float64_linears():
    torch.manual_seed(3)
    head, pred = TwoMLPHead(256 * 7 * 7, 1024).to(DEV).eval(), FastRCNNPredictor(1024, NC).to(DEV).eval()
    M = 74
    pooled = _dev(synth.normal(9, 1, M * 12544).astype(np.float32).reshape(M, 7, 7, 256))
    cpu = {k: v.detach().cpu().double() for k, v in list(head.state_dict().items()) + list(pred.state_dict().items())}
    with torch.no_grad():
        p16 = ops.cast_bf16(pooled)
        w6, w7 = head.operands_bf16(256, 7, 7)
        assert w6.dtype == BF and torch.equal(w6, head.fc6_weight_hwc(256, 7, 7).to(BF)) and torch.equal(w7, head.fc7.weight.detach().to(BF))
        x6 = ops.linear_bf16(p16.reshape(M, -1), w6, head.fc6.bias.detach(), _lib.EPI_BIAS_RELU)
        x7 = head.forward_bf16(p16)
        y = pred.forward_stacked_bf16(x7)
        assert pred._operand_cache.filled("bf16")
        wp = pred._operand_cache.get("bf16", (pred.cls_score.weight, pred.bbox_pred.weight), None)  # the entry itself: nothing to build
        assert torch.equal(x7, ops.linear_bf16(x6, w7, head.fc7.bias.detach(), _lib.EPI_BIAS_RELU))
    assert x7.dtype == BF and y.dtype == torch.float32 and tuple(y.shape) == (M, 32)
    _stage_gate("fc6", x6, p16.reshape(M, -1), w6, head.fc6.bias.detach(), 12544, True)
    _stage_gate("fc7", x7, x6, w7, head.fc7.bias.detach(), 1024, True)
    _stage_gate("predictor", y, x7, wp, pred._operands()[1], 1024, False)
    assert float(x7.float().min()) == 0.0 and not y[:, 30:].any()                                   # clamped values exist; padding columns zero
    # the whole head against float64 linears on the fp32 pooled rows and the fp32 weights: the project's bf16 gate
    chw = pooled.cpu().double().permute(0, 3, 1, 2).flatten(start_dim=1)
    r7 = F.relu(F.linear(F.relu(F.linear(chw, cpu["fc6.weight"], cpu["fc6.bias"])), cpu["fc7.weight"], cpu["fc7.bias"]))
    ref_l, ref_d = F.linear(r7, cpu["cls_score.weight"], cpu["cls_score.bias"]), F.linear(r7, cpu["bbox_pred.weight"], cpu["bbox_pred.bias"])
    el, ed = rel_l2(y[:, :NC].cpu().numpy(), ref_l.numpy()), rel_l2(y[:, NC:5 * NC].cpu().numpy(), ref_d.numpy())
    print(f"bf16 head vs float64 on fp32 operands: logits rel-L2 {el:.3e}, deltas rel-L2 {ed:.3e}")
    assert el <= 2e-2 and ed <= 2e-2


# ---- 4. the detector ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    """The fixture of tests/test_gpu_roi.py: hidden 128, 3 layers, B = 2, 224 x 224, the background bias raised until at most 60
    candidates per image clear the score threshold - plus the fp32 head's results, computed once and left unchanged."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    m = model.model
    with torch.no_grad():
        for p in m.rpn.head.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
        pred = m.roi_heads.box_predictor
        pred.cls_score.weight.copy_(torch.randn_like(pred.cls_score.weight) * 0.3)
        pred.bbox_pred.weight.copy_(torch.randn_like(pred.bbox_pred.weight) * 0.2)
        pred.cls_score.bias.zero_()
    model = model.to(DEV).eval()
    batch = torch.from_numpy(synth.synth_images(2, 224, 224, seed=77)).to(DEV)
    with torch.no_grad():
        feats = m.backbone(batch)
        proposals, _, count = m.rpn(feats, (224, 224), padded=True)
        y = m.roi_heads.head_padded(feats, proposals, count, (224, 224)).cpu().double().numpy()
        cnt = count.cpu().numpy()
        valid = [y[b * 1000:b * 1000 + cnt[b], :NC] for b in range(2)]
        bias = 0.0
        while max(int((roi.softmax64(v + np.eye(NC)[0] * bias)[:, 1:] > 0.05).sum()) for v in valid) > 60:
            bias += 0.25
        pred.cls_score.bias[0] = bias
        assert model.head_dtype == "f32"
        feats = {k: v.clone() for k, v in feats.items()}                                            # the test's own copy of the maps
        ref = {"feats": feats, "proposals": proposals.clone(), "count": count.clone(),
               "y32": m.roi_heads.head_padded(feats, proposals, count, (224, 224)).clone(),
               "det32": tuple(t.clone() for t in model.forward_padded(batch))}
    return model, batch, ref


@pytest.fixture()
def bf16_detector(detector):
    model, batch, ref = detector
    model.set_head_dtype("bf16")
    yield model, batch, ref
    model.set_head_dtype("f32")


def test_bf16_head_output_and_candidates(bf16_detector):
    model, batch, ref = bf16_detector
    rh, R = model.model.roi_heads, 1000
    feats, proposals, count = ref["feats"], ref["proposals"], ref["count"]
    with torch.no_grad():
        y16 = rh.head_padded(feats, proposals, count, (224, 224))
        again = rh.head_padded(feats, proposals, count, (224, 224))
    y32 = ref["y32"]
    assert y16.dtype == torch.float32 and tuple(y16.shape) == tuple(y32.shape) and torch.equal(y16, again) and not torch.equal(y16, y32)
    assert not y16[:, 5 * NC:].any()
    cnt = count.cpu().numpy()
    rows = torch.cat([torch.arange(b * R, b * R + int(cnt[b])) for b in range(2)]).to(DEV)
    # (a) the head output over the valid rows
    el = rel_l2(y16[rows, :NC].cpu().numpy(), y32[rows, :NC].cpu().numpy())
    ed = rel_l2(y16[rows, NC:5 * NC].cpu().numpy(), y32[rows, NC:5 * NC].cpu().numpy())
    print(f"detector head bf16 vs fp32 over {len(rows)} valid rows: logits rel-L2 {el:.3e}, deltas rel-L2 {ed:.3e}")
    assert el <= 2e-2 and ed <= 2e-2
    # (b) the candidates: no filter can flip at score_thresh = 0 and min_size = 0, only padding is -inf
    b16, s16, l16 = ops.box_postprocess(y16, proposals, count, (224, 224), NC, score_thresh=0.0, min_size=0.0)
    b32, s32, l32 = ops.box_postprocess(y32, proposals, count, (224, 224), NC, score_thresh=0.0, min_size=0.0)
    assert torch.equal(l16, l32) and torch.equal(torch.isneginf(s16), torch.isneginf(s32))
    d_logit = (y16[:, :NC] - y32[:, :NC]).abs().max(dim=1).values.view(2, R)                       # per proposal row
    worst = 0.0
    for b in range(2):
        n = int(cnt[b])
        ok = ~torch.isneginf(s32[b])
        assert int(ok.sum()) == n * (NC - 1) and not ok[n * (NC - 1):].any()
        d_score = (s16[b] - s32[b]).abs()[ok].view(n, NC - 1)
        bound = 0.5 * d_logit[b, :n, None] + 1e-6                                                   # softmax is 1/2-Lipschitz in the max norm
        worst = max(worst, float((d_score / bound).max()))
        assert (d_score <= bound).all()
    print(f"candidate scores: largest |d score| / (0.5 max |d logit| + 1e-6) = {worst:.3f}")


def _iou(a, b):
    lt, rb = torch.maximum(a[:, None, :2], b[None, :, :2]), torch.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(dim=2)
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])                                      # noqa: E731
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def test_bf16_detector_wiring(bf16_detector):
    model, batch, ref = bf16_detector
    rh = model.model.roi_heads
    feats, proposals, count = ref["feats"], ref["proposals"], ref["count"]
    with torch.no_grad():
        y16 = rh.head_padded(feats, proposals, count, (224, 224))
        want = ops.box_detections_padded(y16, proposals, count, (224, 224), NC, rh.score_thresh, rh.nms_thresh, rh.detections_per_img,
                                         rh.min_size, rh.bbox_reg_weights)
        got = model.forward_padded(batch)
        again = model.forward_padded(batch)
        as_list = rh(feats, proposals, count, (224, 224))
    for g, w, a in zip(got, want, again):
        assert torch.equal(g, w) and torch.equal(g, a)                                              # (c) the wiring; two runs bit-identical
    n = got[3].tolist()
    assert all(1 <= k < 100 for k in n)
    for b, d in enumerate(as_list):                                                                 # the list form is the padded form sliced
        assert torch.equal(d["boxes"], got[0][b, :n[b]]) and torch.equal(d["scores"], got[1][b, :n[b]])
        assert d["labels"].dtype == torch.int64 and torch.equal(d["labels"], got[2][b, :n[b]].long())
    # (f) reported, not gated (NMS is discontinuous): detections with a same-label partner of IoU >= 0.9 under the other dtype
    d32 = ref["det32"]
    for b in range(2):
        n16, n32 = n[b], int(d32[3][b])
        iou = _iou(got[0][b, :n16], d32[0][b, :n32])
        same = got[2][b, :n16, None] == d32[2][b, None, :n32]
        hit = (iou >= 0.9) & same
        print(f"image {b}: {int(hit.any(dim=1).sum())} of {n16} bf16 detections have an fp32 partner (same label, IoU >= 0.9); "
              f"{int(hit.any(dim=0).sum())} of {n32} fp32 detections have a bf16 partner")
    # forward on ragged images runs, and is the padded form scaled back
    rng = np.random.RandomState(5)
    images = [_dev(rng.rand(3, 180, 300).astype(np.float32)), _dev(rng.rand(3, 333, 211).astype(np.float32))]
    out = model(images)
    pb, ps, pl, pc = model.forward_padded(model.model.transform(images)[0].tensors)
    assert len(out) == 2
    for i, d in enumerate(out):
        k = int(pc[i])
        assert set(d) == {"boxes", "labels", "scores"} and tuple(d["boxes"].shape) == (k, 4)
        assert torch.equal(d["scores"], ps[i, :k]) and torch.equal(d["labels"], pl[i, :k].long())


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
    assert not torch.equal(eager[0][0], eager[1][0])


def test_fp32_default_is_unchanged_after_the_bf16_head_ran(detector):
    model, batch, ref = detector
    model.set_head_dtype("bf16")
    with torch.no_grad():
        det16 = model.forward_padded(batch)
    model.set_head_dtype("f32")
    with torch.no_grad():
        det32 = model.forward_padded(batch)
        y32 = model.model.roi_heads.head_padded(ref["feats"], ref["proposals"], ref["count"], (224, 224))
    assert torch.equal(y32, ref["y32"])
    for got, want in zip(det32, ref["det32"]):
        assert torch.equal(got, want)
    assert not all(torch.equal(a, b) for a, b in zip(det16, det32))


# ---- 5 / 6. training untouched, caches invalidated ---------------------------------------------------------------------------------------
def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _train_model(head_dtype="f32"):
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, head_dtype=head_dtype)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
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


def test_losses_do_not_depend_on_head_dtype(train_batch):
    model = _train_model()
    l32 = model.losses(*train_batch, generator=_seeded(2))
    with torch.no_grad():                                                                           # (the encoder's no-grad forward is another path)
        l32_nograd = model.losses(*train_batch, generator=_seeded(2))
    model.set_head_dtype("bf16")
    l16 = model.losses(*train_batch, generator=_seeded(2))
    with torch.no_grad():
        l16_nograd = model.losses(*train_batch, generator=_seeded(2))
    assert sorted(l32) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    for k in l32:
        assert torch.equal(l32[k], l16[k]) and torch.equal(l32_nograd[k], l16_nograd[k]), k
    assert l16["loss_classifier"].requires_grad                                                     # still the differentiable fp32 path


def test_train_step_invalidates_the_bf16_operands(train_batch):
    model = _train_model("bf16")
    x = torch.from_numpy(synth.synth_images(2, 224, 224, seed=31, kind="uniform")).to(DEV)
    rh = model.model.roi_heads

    def head_out(mod):
        m = mod.model
        with torch.no_grad():
            feats = m.backbone(x)
            proposals, _, count = m.rpn(feats, (224, 224), padded=True)
            return m.roi_heads.head_padded(feats, proposals, count, (224, 224))

    before = [t.clone() for t in model.eval().forward_padded(x)]                                    # fills the bf16 caches with the old weights
    y_before = head_out(model)
    assert rh.box_head._operand_cache.filled("bf16") and rh.box_predictor._operand_cache.filled("bf16")
    model.train()
    step = DetectorTrainStep(model, lr=1e-3, init_scale=1024.0)
    step.step(*train_batch, generator=_seeded(2))
    assert step.steps == 1
    fresh = _train_model("bf16")
    fresh.load_state_dict(model.state_dict())
    after, want = model.eval().forward_padded(x), fresh.eval().forward_padded(x)
    for got, w in zip(after, want):
        assert torch.equal(got, w)
    y_after, y_want = head_out(model), head_out(fresh)
    assert torch.equal(y_after, y_want) and not torch.equal(y_after, y_before)                      # a stale bf16 operand fails here
    assert len(before) == 4


# ---- 7. full size ------------------------------------------------------------------------------------------------------------------------
def test_full_size_rows_and_the_last_tile():
    """B = 64, R = 1000, C = 256: 64 000 rows of 12 544 bf16 = 1.6 GB, the only size where a 32-bit offset could wrap.  Rows 0, 31 999
    and 63 999 equal the same box pooled alone from its own image's maps; fc6 on the last 16 rows alone has the bits of those rows of
    the full GEMM."""
    B, R, Cc = 64, 1000, 256
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    feats = [torch.randn(B, s, s, Cc, device=DEV, generator=g).permute(0, 3, 1, 2) for s in (56, 28, 14, 7)]
    feats.append(feats[3][:, :, ::2, ::2])
    ctr = torch.rand(B, R, 2, device=DEV, generator=g) * 224
    size = torch.exp(torch.rand(B, R, 2, device=DEV, generator=g) * (np.log(224.0) - np.log(8.0)) + np.log(8.0))
    boxes = torch.cat([ctr - 0.5 * size, ctr + 0.5 * size], dim=-1).clamp(0, 224).contiguous()
    pooled = ops.roi_align_levels(feats, boxes, None, (224, 224), out_dtype=BF)
    assert tuple(pooled.shape) == (B * R, 7, 7, Cc) and pooled.numel() * 2 > 2 ** 30
    for row in (0, 31999, 63999):
        b, r = divmod(row, R)
        alone = ops.roi_align_levels([f[b:b + 1] for f in feats], boxes[b:b + 1, r:r + 1].contiguous(), None, (224, 224), out_dtype=BF)
        assert torch.equal(pooled[row], alone[0]) and pooled[row].float().abs().max() > 0, row
    w6 = (torch.randn(1024, 49 * Cc, device=DEV, generator=g) * 0.02).to(BF)
    b6 = torch.randn(1024, device=DEV, generator=g) * 0.1
    x = pooled.view(B * R, -1)
    full = ops.linear_bf16(x, w6, b6, _lib.EPI_BIAS_RELU)
    alone = ops.linear_bf16(x[-16:].contiguous(), w6, b6, _lib.EPI_BIAS_RELU)
    assert torch.equal(full[-16:], alone) and float(alone.float().max()) > 0 and float(alone.float().min()) == 0.0
