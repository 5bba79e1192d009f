"""The box head on the GPU (csrc/roi_heads.hip through the C ABI, modeling/roi_heads.py, modeling/detector.py) against the numpy
oracle tests/roi_oracle.py: RoIAlign levels EXACTLY and values within 2^-13 * max|map|; postprocess scores within 4 * 2^-23
relative, boxes within the RPN decode bound, labels and the -inf pattern exactly, the NMS behind it exactly; the head's GEMMs
within the fp32 gate; the whole detector stage by stage with each oracle fed the device's own output of the stage before."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import ops, synth                  # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import FastRCNNPredictor, LayoutDetectionModel, TwoMLPHead    # noqa: E402
from tests import roi_oracle as roi                   # noqa: E402
from tests import rpn_oracle as ro                    # noqa: E402
from tests.util import rel_l2                         # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
NC = 6
GEOMETRIES = {(224, 224): [(56, 56), (28, 28), (14, 14), (7, 7)], (96, 160): [(24, 40), (12, 20), (6, 10), (3, 5)]}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _feature_maps(seed, image_size, B, Cc, batch_step=1):
    """p2..p5 as [B, C, h, w] views of channels-last memory and `pool` = p5[:, :, ::2, ::2] (a strided view, never copied);
    batch_step = 2: every map is every other image of a batch twice as large (a non-contiguous batch stride)."""
    rng = np.random.RandomState(seed)
    feats = []
    for h, w in GEOMETRIES[image_size]:
        nhwc = _dev(rng.normal(0, 1.5, size=(B * batch_step, h, w, Cc)).astype(np.float32))
        feats.append(nhwc[::batch_step].permute(0, 3, 1, 2))
    feats.append(feats[3][:, :, ::2, ::2])
    return feats


def _host_maps(feats):
    return [f.permute(0, 2, 3, 1).cpu().numpy() for f in feats]


def _roi_case(image_size, R, Cc, batch_step=1):
    B = 2
    feats = _feature_maps(7 * R + Cc, image_size, B, Cc, batch_step)
    sizes = [tuple(f.shape[-2:]) for f in feats]
    boxes = np.stack([roi.make_boxes(100 * R + b, R, image_size, sizes)[0] for b in range(B)])
    count = np.asarray([R, R // 2], dtype=np.int32)
    return feats, boxes, count


@pytest.mark.parametrize("Cc", [12, 256])
@pytest.mark.parametrize("R", [1, 37, 130])
@pytest.mark.parametrize("image_size", [(224, 224), (96, 160)])
def test_roi_align_levels_matches_the_float64_oracle(image_size, R, Cc):
    feats, boxes, count = _roi_case(image_size, R, Cc)
    assert feats[4].data_ptr() == feats[3].data_ptr() and not feats[4].is_contiguous(memory_format=torch.channels_last)
    out, levels = ops.roi_align_levels(feats, _dev(boxes), _dev(count), image_size, return_levels=True)
    out2, levels2 = ops.roi_align_levels(feats, _dev(boxes), _dev(count), image_size, return_levels=True)
    assert tuple(out.shape) == (2 * R, 7, 7, Cc) and tuple(levels.shape) == (2, R) and levels.dtype == torch.int32
    assert torch.equal(out, out2) and torch.equal(levels, levels2)                                  # bit-reproducible
    maps = _host_maps(feats)
    ref, ref_levels = roi.roi_align_levels(maps, boxes, count, image_size)
    np.testing.assert_array_equal(levels.cpu().numpy(), ref_levels)                                # exact boundaries included
    got = out.cpu().numpy()
    peak = max(float(np.abs(m).max()) for m in maps)
    err = float(np.abs(got - ref).max())
    print(f"roi_align {image_size} R={R} C={Cc}: max abs err {err:.3e}, bound {2.0 ** -13 * peak:.3e}")
    assert err <= 2.0 ** -13 * peak
    for b in range(2):
        assert not got[b * R + count[b]:(b + 1) * R].any()                                         # padding rows exactly zero
        assert got[b * R:b * R + count[b]].any() or R == 1
    # count = None: every row valid
    full = ops.roi_align_levels(feats, _dev(boxes), None, image_size).cpu().numpy()
    ref_full, _ = roi.roi_align_levels(maps, boxes, None, image_size)
    assert np.abs(full - ref_full).max() <= 2.0 ** -13 * peak


def test_roi_align_levels_with_a_non_contiguous_batch_stride():
    feats, boxes, count = _roi_case((224, 224), 37, 256, batch_step=2)
    assert feats[0].stride(0) == 2 * 56 * 56 * 256
    out, levels = ops.roi_align_levels(feats, _dev(boxes), _dev(count), (224, 224), return_levels=True)
    maps = _host_maps(feats)
    ref, ref_levels = roi.roi_align_levels(maps, boxes, count, (224, 224))
    np.testing.assert_array_equal(levels.cpu().numpy(), ref_levels)
    peak = max(float(np.abs(m).max()) for m in maps)
    assert np.abs(out.cpu().numpy() - ref).max() <= 2.0 ** -13 * peak
    with pytest.raises(ValueError, match="channels-last"):
        ops.roi_align_levels([f.contiguous() for f in feats], _dev(boxes), _dev(count), (224, 224))


# ---- postprocess -----------------------------------------------------------------------------------------------------------------
def _post_inputs(seed, R, thr=0.05, min_size=1e-2):
    """Head output [2 R, 32] and proposals [2, R, 4]; the seed is stepped until no score lies within 1e-6 of the threshold and no
    clipped side within 1e-4 of min_size.  Hand-placed rows (when they fit): a proposal outside the image after decoding (zero
    width: dropped), deltas far above the clamp."""
    while True:
        rng = np.random.RandomState(seed)
        head = np.zeros((2 * R, 32), dtype=np.float32)
        head[:, :NC] = rng.normal(0, 2.0, size=(2 * R, NC))
        head[:, NC:5 * NC] = rng.normal(0, 2.0, size=(2 * R, 4 * NC))
        head[:, 30:] = rng.normal(0, 1, size=(2 * R, 2))                                            # pad columns: never read
        ctr = rng.uniform(10, 214, size=(2, R, 2))
        size = np.exp(rng.uniform(math.log(4.0), math.log(150.0), size=(2, R, 2)))
        props = np.clip(np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=-1), 0, 224).astype(np.float32)
        if R >= 8:
            head[2::7, NC + 2::4] += 30.0                                                           # dw / 5 above log(1000 / 16)
            # far off the right edge / the top (width / height 0).  Far enough that dx w dwarfs the proposal's centre: the bound
            # is relative to the DECODED centre, a shift that nearly cancels the centre loses the proposal's own ulps instead
            head[3::11, NC + 0::4] += 3000.0
            head[5::13, NC + 1::4] -= 3000.0
        count = np.asarray([R, R // 2], dtype=np.int32)
        ok = True
        for b in range(2):
            box, _, _, prob, _ = roi.postprocess(head[b * R:(b + 1) * R], props[b], count[b], 224, 224, NC, thr, min_size)
            wd, ht = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
            ok &= bool((np.abs(prob - float(np.float32(thr))) > 1e-6).all() and (np.abs(wd - min_size) > 1e-4).all()
                       and (np.abs(ht - min_size) > 1e-4).all())
        if ok:
            return head, props, count
        seed += 1


def _decode_bound(terms):
    pcx, pcy, pw, ph = terms
    bx = 8 * EPS * np.maximum(np.maximum(np.abs(pcx), pw), 1.0)
    by = 8 * EPS * np.maximum(np.maximum(np.abs(pcy), ph), 1.0)
    return np.stack([bx, by, bx, by], axis=1)


def _check_postprocess(head, props, count, boxes, scores, labels, R, thr=0.05, strict_pattern=True):
    """Device boxes / scores / labels [2, R (NC - 1)] against the float64 oracle; returns the number of valid candidates."""
    n_valid = 0
    for b in range(2):
        box, score, lab, prob, terms = roi.postprocess(head[b * R:(b + 1) * R], props[b], None if count is None else count[b], 224, 224,
                                                       NC, thr)
        assert (np.abs(boxes[b].astype(np.float64) - box) <= _decode_bound(terms)).all()
        np.testing.assert_array_equal(labels[b], lab)
        valid = np.isfinite(score)
        if strict_pattern:
            np.testing.assert_array_equal(np.isneginf(scores[b]), ~valid)
        else:                                                # real data: candidates on the edge of a filter may fall either way
            wd, ht = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
            clear = (np.abs(prob - float(np.float32(thr))) > 1e-6) & (np.abs(wd - 1e-2) > 1e-4) & (np.abs(ht - 1e-2) > 1e-4)
            np.testing.assert_array_equal(np.isneginf(scores[b])[clear], ~valid[clear])
            valid &= np.isfinite(scores[b])
        rel = np.abs(scores[b][valid].astype(np.float64) - prob[valid]) / prob[valid]
        assert rel.size == 0 or rel.max() <= 4 * EPS, rel.max()
        n_valid += int(valid.sum())
    return n_valid


def _check_nms(boxes, scores, labels, keep, kept, out_labels, max_out=100):
    for b in range(boxes.shape[0]):
        ref_keep, ref_count = ro.nms(boxes[b], scores[b], labels[b], 0.5, max_out)                  # fed the device's boxes and scores
        assert kept[b] == ref_count
        np.testing.assert_array_equal(keep[b], ref_keep)
        np.testing.assert_array_equal(out_labels[b, :ref_count], labels[b][ref_keep[:ref_count]])
        assert not out_labels[b, ref_count:].any()


@pytest.mark.parametrize("R", [1, 37, 300, 1000])
def test_postprocess_and_detections_match_the_oracle(R):
    head, props, count = _post_inputs(50 + R, R)
    d_head, d_props, d_count = _dev(head), _dev(props), _dev(count)
    boxes, scores, labels = (t.cpu().numpy() for t in ops.box_postprocess(d_head, d_props, d_count, (224, 224), NC))
    assert boxes.shape == (2, R * 5, 4) and scores.shape == (2, R * 5) and labels.dtype == np.int32
    n_valid = _check_postprocess(head, props, count, boxes, scores, labels, R)
    assert np.isneginf(scores[1, (R // 2) * 5:]).all() and (R < 37 or 0 < n_valid < 2 * R * 5)
    if R >= 37:
        zero_w = boxes[0][:, 2] == boxes[0][:, 0]
        assert zero_w.any() and np.isneginf(scores[0][zero_w]).all() and boxes.max() == 224.0 and boxes.min() == 0.0
    keep, kept, _, _ = ops.batched_nms_padded(_dev(boxes), _dev(scores), _dev(labels), 0.5, 100)
    ob, osc, ol, oc = ops.box_detections_padded(d_head, d_props, d_count, (224, 224), NC)
    assert tuple(ob.shape) == (2, 100, 4) and tuple(osc.shape) == (2, 100) and ol.dtype == torch.int32 and torch.equal(oc, kept)
    _check_nms(boxes, scores, labels, keep.cpu().numpy(), kept.cpu().numpy(), ol.cpu().numpy())
    for b in range(2):
        n = int(kept[b])
        assert torch.equal(ob[b, :n].cpu(), torch.from_numpy(boxes[b])[keep[b, :n].cpu().long()]) and not ob[b, n:].any() and not osc[b, n:].any()
    # count = None: the padding rows of image 1 take part
    _, scores_all, _ = ops.box_postprocess(d_head, d_props, None, (224, 224), NC)
    _check_postprocess(head, props, None, boxes, scores_all.cpu().numpy(), labels, R)


def test_postprocess_drops_a_score_exactly_at_the_threshold():
    """Two equal logits and the rest -inf: both scores are exactly 0.5.  At threshold 0.5 they are dropped (strict >, where the RPN
    stage keeps >=); just below it they are kept.  A proposal of zero width is dropped whatever its score."""
    head = np.zeros((2, 32), dtype=np.float32)
    head[:, :NC] = [-np.inf, 1.5, -np.inf, 1.5, -np.inf, -np.inf]
    props = np.asarray([[[10, 10, 50, 60]], [[30, 10, 30, 60]]], dtype=np.float32)
    for thr, keeps in ((0.5, False), (float(np.nextafter(np.float32(0.5), np.float32(0))), True)):
        boxes, scores, labels = (t.cpu().numpy() for t in ops.box_postprocess(_dev(head), _dev(props), None, (224, 224), NC, score_thresh=thr))
        assert list(labels[0]) == [1, 2, 3, 4, 5]
        np.testing.assert_array_equal(boxes[0], np.tile(props[0], (5, 1)))
        if keeps:
            assert scores[0, 0] == 0.5 and scores[0, 2] == 0.5
        assert np.isneginf(scores[0, [1, 3, 4]]).all() and (keeps or np.isneginf(scores[0]).all())
        assert np.isneginf(scores[1]).all()


# ---- the head's GEMMs ------------------------------------------------------------------------------------------------------------
def test_head_gemms_match_float64_linears():
    torch.manual_seed(3)
    head, pred = TwoMLPHead(256 * 7 * 7, 1024).to(DEV).eval(), FastRCNNPredictor(1024, NC).to(DEV).eval()
    M = 74
    pooled = torch.from_numpy(synth.normal(9, 1, M * 12544).astype(np.float32).reshape(M, 7, 7, 256)).to(DEV)
    cpu = {k: v.detach().cpu().double() for k, v in list(head.state_dict().items()) + list(pred.state_dict().items())}
    with torch.no_grad():
        w6 = head.fc6_weight_hwc(256, 7, 7)
        x6 = ops.linear(pooled.reshape(M, -1), w6, head.fc6.bias.detach())
        x7 = head(pooled)
        y = pred.forward_stacked(x7)
        logits, deltas = pred(x7)
    chw = pooled.cpu().double().permute(0, 3, 1, 2).flatten(start_dim=1)                            # torchvision's flattening
    ref6 = F.linear(chw, cpu["fc6.weight"], cpu["fc6.bias"])
    assert rel_l2(x6.cpu().numpy(), ref6.numpy()) < 2e-5
    ref7 = F.relu(F.linear(F.relu(x6.cpu().double()), cpu["fc7.weight"], cpu["fc7.bias"]))          # fed the device's fc6
    assert rel_l2(x7.cpu().numpy(), ref7.numpy()) < 2e-5 and float(x7.min()) == 0.0
    ref_l = F.linear(x7.cpu().double(), cpu["cls_score.weight"], cpu["cls_score.bias"])            # fed the device's fc7
    ref_d = F.linear(x7.cpu().double(), cpu["bbox_pred.weight"], cpu["bbox_pred.bias"])
    assert tuple(y.shape) == (M, 32) and tuple(logits.shape) == (M, NC) and tuple(deltas.shape) == (M, 4 * NC)
    assert rel_l2(logits.cpu().numpy(), ref_l.numpy()) < 2e-5 and rel_l2(deltas.cpu().numpy(), ref_d.numpy()) < 2e-5
    assert not y[:, 30:].any()


# ---- the whole detector ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    """The smallest encoder (3 layers, 128 wide) under the reference's FPN / RPN / box head at B = 2, 224 x 224.  Synthetic weights;
    the background bias of cls_score is set from the head's own logits so that a few dozen candidates per image pass the score
    threshold (the tests assert 1 <= detections < 100 per image)."""
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
        # raise the background bias in steps until at most 60 candidates of either image clear score 0.05 (float64 softmax on the
        # device's logits); the tests assert that at least one detection per image is left
        valid = [y[b * 1000:b * 1000 + cnt[b], :NC] for b in range(2)]
        bias = 0.0
        while max(int((roi.softmax64(v + np.eye(NC)[0] * bias)[:, 1:] > 0.05).sum()) for v in valid) > 60:
            bias += 0.25
        pred.cls_score.bias[0] = bias
    return model, batch


def test_detector_stage_by_stage(detector):
    model, batch = detector
    m = model.model
    R = 1000
    with torch.no_grad():
        feats = m.backbone(batch)
        proposals, _, count = m.rpn(feats, (224, 224), padded=True)
        names = list(feats)
        assert names == ["p2", "p3", "p4", "p5", "pool"] and tuple(proposals.shape) == (2, R, 4)
        pooled, levels = ops.roi_align_levels(list(feats.values()), proposals, count, (224, 224), return_levels=True)
        assert torch.equal(pooled, m.roi_heads.box_roi_pool(feats, proposals, count, (224, 224)))
        x7 = m.roi_heads.box_head(pooled)
        y = m.roi_heads.box_predictor.forward_stacked(x7)
        assert torch.equal(y, m.roi_heads.head_padded(feats, proposals, count, (224, 224)))
        boxes, scores, labels = ops.box_postprocess(y, proposals, count, (224, 224), NC)
        keep, kept, _, _ = ops.batched_nms_padded(boxes, scores, labels, 0.5, 100)
        pb, ps, pl, pc = m.roi_heads(feats, proposals, count, (224, 224), padded=True)
        as_list = m.roi_heads(feats, proposals, count, (224, 224))
    cnt, props = count.cpu().numpy(), proposals.cpu().numpy()
    assert (cnt > 50).all()
    # RoIAlign: fed the device's maps and proposals; the level of a box on a level boundary may fall either way, as may a sample
    # on the far edge of its map - those rows are compared at the device's level / left out
    maps = [f.permute(0, 2, 3, 1).cpu().numpy() for f in feats.values()]
    sizes = [mp.shape[1:3] for mp in maps]
    scales = roi.infer_scales(sizes, (224, 224))
    lv = levels.cpu().numpy()
    rows = []
    for b in range(2):
        sel = np.arange(0, cnt[b], 5)                                   # every fifth proposal
        ref_lv = roi.box_levels(props[b, sel], 2, 6)
        clear = roi.level_margin(props[b, sel]) > 1e-4
        np.testing.assert_array_equal(lv[b, sel][clear], ref_lv[clear])
        assert (lv[b, :cnt[b]] >= 0).all() and (lv[b, cnt[b]:] == -1).all()
        safe = roi.edge_margin(props[b, sel], lv[b, sel], sizes, scales) > 1e-3
        rows += [(b, r) for r in sel[safe]]
    got = pooled.cpu().numpy()
    peak = max(float(np.abs(mp).max()) for mp in maps)
    worst = 0.0
    for b, r in rows:
        ref = roi.roi_align_row(maps[lv[b, r]][b].astype(np.float64), props[b, r].astype(np.float64), scales[lv[b, r]])
        worst = max(worst, float(np.abs(got[b * R + r] - ref).max()))
    print(f"detector roi_align: {len(rows)} rows, max abs err {worst:.3e}, bound {2.0 ** -13 * peak:.3e}")
    assert len(rows) > 100 and worst <= 2.0 ** -13 * peak
    for b in range(2):
        assert not got[b * R + cnt[b]:(b + 1) * R].any()
    # the head: 64 rows against float64 linears fed the device's pooled rows
    sel = torch.arange(0, 2 * R, 2 * R // 64)[:64]
    sd = {k: v.detach().cpu().double() for k, v in m.roi_heads.state_dict().items()}
    chw = pooled[sel.to(DEV)].cpu().double().permute(0, 3, 1, 2).flatten(start_dim=1)
    r7 = F.relu(F.linear(F.relu(F.linear(chw, sd["box_head.fc6.weight"], sd["box_head.fc6.bias"])), sd["box_head.fc7.weight"], sd["box_head.fc7.bias"]))
    ref_y = torch.cat([F.linear(r7, sd["box_predictor.cls_score.weight"], sd["box_predictor.cls_score.bias"]),
                       F.linear(r7, sd["box_predictor.bbox_pred.weight"], sd["box_predictor.bbox_pred.bias"])], dim=1)
    assert rel_l2(y[sel.to(DEV), :5 * NC].cpu().numpy(), ref_y.numpy()) < 2e-5
    # postprocess fed the device's head output; NMS fed the device's candidates
    y_h, boxes_h, scores_h, labels_h = y.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
    _check_postprocess(y_h, props, cnt, boxes_h, scores_h, labels_h, R, strict_pattern=False)
    _check_nms(boxes_h, scores_h, labels_h, keep.cpu().numpy(), kept.cpu().numpy(), pl.cpu().numpy())
    n = kept.cpu().numpy()
    print("detections per image:", n.tolist())
    assert ((n >= 1) & (n < 100)).all()
    # the module: padded form = those launches, list form = padded sliced by the count
    assert torch.equal(pc, kept) and tuple(pb.shape) == (2, 100, 4) and tuple(ps.shape) == (2, 100) and tuple(pl.shape) == (2, 100)
    for b in range(2):
        assert torch.equal(pb[b, :n[b]], boxes[b][keep[b, :n[b]].long()]) and torch.equal(ps[b, :n[b]], scores[b][keep[b, :n[b]].long()])
        assert not pb[b, n[b]:].any() and not ps[b, n[b]:].any() and not pl[b, n[b]:].any()
        d = as_list[b]
        assert torch.equal(d["boxes"], pb[b, :n[b]]) and torch.equal(d["scores"], ps[b, :n[b]])
        assert d["labels"].dtype == torch.int64 and torch.equal(d["labels"], pl[b, :n[b]].long())
        assert (d["scores"][:-1] >= d["scores"][1:]).all() and d["scores"].min() > 0.05 and d["labels"].min() >= 1 and d["labels"].max() <= 5
    fb, fs, fl, fc = model.forward_padded(batch)
    assert torch.equal(fb, pb) and torch.equal(fs, ps) and torch.equal(fl, pl) and torch.equal(fc, pc)


def test_detector_forward_on_ragged_images(detector):
    model, _ = detector
    rng = np.random.RandomState(5)
    images = [torch.from_numpy(rng.rand(3, 180, 300).astype(np.float32)).to(DEV), torch.from_numpy(rng.rand(3, 333, 211).astype(np.float32)).to(DEV)]
    out = model(images)
    assert len(out) == 2
    batch = model.model.transform(images)[0].tensors
    pb, ps, pl, pc = model.forward_padded(batch)
    for i, (img, d) in enumerate(zip(images, out)):
        h, w = img.shape[-2:]
        n = int(pc[i])
        assert set(d) == {"boxes", "labels", "scores"} and tuple(d["boxes"].shape) == (n, 4) and tuple(d["labels"].shape) == (n,)
        assert torch.equal(d["scores"], ps[i, :n]) and torch.equal(d["labels"], pl[i, :n].long())
        if n:
            b = d["boxes"]
            slack = 1 + 2.0 ** -22                                      # the two fp32 roundings of the scale back (ratio, product)
            assert b[:, 0::2].min() >= 0 and b[:, 0::2].max() <= w * slack and b[:, 1::2].min() >= 0 and b[:, 1::2].max() <= h * slack
            scale = torch.tensor([w / 224, h / 224, w / 224, h / 224], device=DEV)
            assert torch.allclose(b, pb[i, :n] * scale, rtol=1e-6, atol=1e-4)


def test_padded_detector_is_graph_capturable(detector):
    """Pixels to padded detections allocate nothing in the library and never synchronise: captured once on a single stream,
    replayed on a new batch written into the captured input, equal to the eager result."""
    model, batch = detector
    other = torch.from_numpy(synth.synth_images(2, 224, 224, seed=78)).to(DEV)
    with torch.no_grad():
        eager = [tuple(t.clone() for t in model.forward_padded(x)) for x in (batch, other)]
        static_x = batch.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.forward_padded(static_x)                                                          # warm-up on a side stream
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = model.forward_padded(static_x)
        for x, ref in zip((other, batch), reversed(eager)):
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(static_out, ref):
                assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])
