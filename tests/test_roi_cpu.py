"""CPU-only checks of the box head: the C ABI declares, exports and validates the two entry points without a device; the modules
have torchvision's parameter names and the detector the reference's state_dict keys; the fc6 column re-ordering is torchvision's
flatten; the numpy oracle (tests/roi_oracle.py) passes hand-computed cases and agrees with an independent restatement through
F.grid_sample.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from layoutdit_amd import _lib, config as cfgs, ops
from layoutdit_amd.modeling import (DiTWithFPN, FastRCNNPredictor, LayoutDetectionModel, MultiScaleRoIAlign, RoIHeads, RPNHead,
                                    TwoMLPHead)
from tests import roi_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_roi_align_levels_f32", "ldit_box_postprocess_f32")
SIZES_224 = [(56, 56), (28, 28), (14, 14), (7, 7), (4, 4)]


def test_header_declares_and_library_exports_the_box_head_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6       # purely additive


def _roi_args(L=5, Cc=256, P=7, S=2, maps=None, boxes=16, out=16, k=(2, 6), stride_x=None):
    ptrs = (C.c_void_p * L)(*([16 * (i + 1) for i in range(L)] if maps is None else maps))
    hs = (C.c_int32 * L)(*([7] * L))
    scales = (C.c_float * L)(*([0.25] * L))
    sb = (C.c_int64 * L)(*([49 * Cc] * L))
    sy = (C.c_int64 * L)(*([7 * Cc] * L))
    sx = (C.c_int64 * L)(*([Cc if stride_x is None else stride_x] * L))
    return (ptrs, hs, hs, scales, sb, sy, sx, L, Cc, boxes, None, 2, 10, P, S, k[0], k[1], 224.0, 4.0, out, None, None)


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    roi = lib.ldit_roi_align_levels_f32
    assert roi(*_roi_args(boxes=None)) == _lib.LDIT_EINVAL and "null" in err()
    assert roi(*_roi_args(out=None)) == _lib.LDIT_EINVAL and "null" in err()
    assert roi(*_roi_args(maps=[16, 32, None, 64, 80])) == _lib.LDIT_EINVAL and "null" in err()
    assert roi(*_roi_args(maps=[16, 32, 40, 64, 80])) == _lib.LDIT_EINVAL and "aligned" in err()
    assert roi(*_roi_args(out=8)) == _lib.LDIT_EINVAL and "aligned" in err()
    assert roi(*_roi_args(Cc=254)) == _lib.LDIT_EUNSUPPORTED and "multiple of 4" in err()
    assert roi(*_roi_args(L=9, k=(2, 10))) == _lib.LDIT_EUNSUPPORTED and "levels" in err()
    assert roi(*_roi_args(P=5)) == _lib.LDIT_EUNSUPPORTED and "output size" in err()
    assert roi(*_roi_args(S=3)) == _lib.LDIT_EUNSUPPORTED
    assert roi(*_roi_args(k=(2, 7))) == _lib.LDIT_EINVAL                              # six levels asked of five maps
    assert roi(*_roi_args(stride_x=128)) == _lib.LDIT_EINVAL                          # pixels would overlap
    w = (C.c_float * 4)(10, 10, 5, 5)
    post = lib.ldit_box_postprocess_f32
    assert post(None, 32, 16, None, 2, 10, 6, 224.0, 224.0, w, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL and "null" in err()
    assert post(16, 32, 16, None, 2, 10, 6, 224.0, 224.0, None, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL
    assert post(16, 32, 16, None, 2, 10, 6, 224.0, 224.0, w, 0.05, 0.01, 16, 16, None, None) == _lib.LDIT_EINVAL
    assert post(16, 32, 16, None, 2, 10, 6, 224.0, 224.0, w, 0.05, 0.01, 16, 8, 16, None) == _lib.LDIT_EINVAL and "aligned" in err()
    assert post(16, 28, 16, None, 2, 10, 6, 224.0, 224.0, w, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL and "row stride" in err()
    assert post(16, 32, 16, None, 2, 10, 1, 224.0, 224.0, w, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL
    assert post(16, 32, 16, None, 2, 0, 6, 224.0, 224.0, w, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL
    bad = (C.c_float * 4)(10, 0, 5, 5)
    assert post(16, 32, 16, None, 2, 10, 6, 224.0, 224.0, bad, 0.05, 0.01, 16, 16, 16, None) == _lib.LDIT_EINVAL and "weights" in err()
    # the ops level: no CPU path, and more candidates than the batched NMS takes are refused with a clear error
    with pytest.raises(ValueError, match="8192"):
        ops._check_candidates(1639, 6)
    ops._check_candidates(1638, 6)
    with pytest.raises(ValueError, match="GPU"):
        ops.box_postprocess(torch.zeros(20, 32), torch.zeros(2, 10, 4), None, (224, 224), 6)
    with pytest.raises(ValueError, match="GPU"):
        ops.roi_align_levels([torch.zeros(2, 8, 4, 4)], torch.zeros(2, 10, 4), None, (16, 16))
    assert ops.infer_scales([torch.zeros(1, 4, h, w) for h, w in SIZES_224], (224, 224)) == [1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64]
    assert ops.infer_scales([torch.zeros(1, 4, 3, 5), torch.zeros(1, 4, 2, 3)], (96, 160)) == [1 / 32, 1 / 64]


def test_modules_have_torchvisions_surface():
    head, pred = TwoMLPHead(12544, 1024), FastRCNNPredictor(1024, 6)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {"fc6.weight": (1024, 12544), "fc6.bias": (1024,),
                                                                         "fc7.weight": (1024, 1024), "fc7.bias": (1024,)}
    assert {k: tuple(v.shape) for k, v in pred.state_dict().items()} == {"cls_score.weight": (6, 1024), "cls_score.bias": (6,),
                                                                         "bbox_pred.weight": (24, 1024), "bbox_pred.bias": (24,)}
    w, b = pred._operands()
    assert tuple(w.shape) == (32, 1024) and torch.equal(w[:6], pred.cls_score.weight) and torch.equal(w[6:30], pred.bbox_pred.weight)
    assert not w[30:].any() and torch.equal(b[6:30], pred.bbox_pred.bias)
    with torch.no_grad():
        pred.cls_score.bias.add_(1.0)
    assert torch.equal(pred._operands()[1][:6], pred.cls_score.bias)                  # re-laid when a parameter changes
    pool = MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)
    assert not list(pool.state_dict()) and (pool.output_size, pool.sampling_ratio) == (7, 2)
    rh = RoIHeads(pool, head, pred)
    assert (rh.score_thresh, rh.nms_thresh, rh.detections_per_img, rh.bbox_reg_weights) == (0.05, 0.5, 100, (10.0, 10.0, 5.0, 5.0))
    assert sorted(rh.state_dict()) == sorted(["box_head." + k for k in head.state_dict()] + ["box_predictor." + k for k in pred.state_dict()])
    with pytest.raises(RuntimeError, match="inference only"):
        rh.train()([torch.zeros(1, 256, 4, 4)], torch.zeros(1, 3, 4), None, (224, 224))
    with pytest.raises(ValueError, match="8192"):
        rh.eval()([torch.zeros(1, 256, 4, 4)], torch.zeros(1, 2000, 4), None, (224, 224))
    with pytest.raises(ValueError, match="GPU"):                                      # no CPU path
        rh.eval()([torch.zeros(1, 256, 4, 4).to(memory_format=torch.channels_last)], torch.zeros(1, 3, 4), None, (16, 16))


def test_detector_has_the_references_state_dict_keys():
    cfg = cfgs.vit_micro()
    m = LayoutDetectionModel(config=cfg)
    want = ["model.backbone." + k for k in DiTWithFPN(config=cfg).state_dict()]
    want += ["model.rpn.head." + k for k in RPNHead(256, 3).state_dict()]
    want += ["model.roi_heads.box_head." + k for k in ("fc6.weight", "fc6.bias", "fc7.weight", "fc7.bias")]
    want += ["model.roi_heads.box_predictor." + k for k in ("cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias")]
    sd = m.state_dict()
    assert sorted(sd) == sorted(want)
    assert any(k.startswith("model.backbone.backbone.dit.") for k in sd) and "model.backbone.fpn.inner_blocks.0.0.weight" in sd
    assert tuple(sd["model.roi_heads.box_predictor.cls_score.weight"].shape) == (6, 1024)       # 5 classes + background
    assert tuple(sd["model.roi_heads.box_head.fc6.weight"].shape) == (1024, 12544)
    assert tuple(sd["model.rpn.head.cls_logits.weight"].shape) == (3, 256, 1, 1)
    gen = m.model.rpn.anchor_generator
    assert gen.sizes == ((32,), (64,), (128,), (256,), (512,)) and gen.aspect_ratios == ((0.5, 1.0, 2.0),) * 5
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()([torch.zeros(3, 32, 32)])
    with pytest.raises(RuntimeError, match="inference only"):
        m.train().forward_padded(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError, match="GPU"):                                      # no CPU path
        m.eval()([torch.zeros(3, 32, 32)])


def test_fc6_columns_are_torchvisions_flatten_reordered():
    torch.manual_seed(0)
    head = TwoMLPHead(8 * 7 * 7, 16)
    chw = torch.randn(5, 8, 7, 7)                                                     # torchvision's pooled tensor [M, C, P, P]
    ref = F.linear(chw.flatten(start_dim=1), head.fc6.weight, head.fc6.bias)
    hwc = chw.permute(0, 2, 3, 1).contiguous()                                        # this library's pooled rows [M, P, P, C]
    w = head.fc6_weight_hwc(8, 7, 7)
    got = F.linear(hwc.reshape(5, -1), w, head.fc6.bias)
    assert torch.allclose(got, ref, rtol=0, atol=1e-5) and not torch.equal(w, head.fc6.weight)
    assert head.fc6_weight_hwc(8, 7, 7) is w                                          # cached ...
    with torch.no_grad():
        head.fc6.weight.mul_(2.0)
    assert torch.equal(head.fc6_weight_hwc(8, 7, 7), w * 2)                           # ... until the parameter changes
    with pytest.raises(ValueError, match="fc6"):
        head.fc6_weight_hwc(8, 7, 6)


def _maps(seed, sizes, B, Cc):
    rng = np.random.RandomState(seed)
    return [rng.normal(0, 1, size=(B, h, w, Cc)) for h, w in sizes]


def test_oracle_roi_align_hand_cases():
    # a constant map gives a constant output, whatever the box (inside the map)
    maps = [np.full((1, h, w, 4), 3.25) for h, w in SIZES_224]
    boxes = np.asarray([[[10.3, 20.9, 100.2, 77.7], [0, 0, 224, 224], [50.5, 60.5, 51, 61]]], dtype=np.float32)
    out, lv = ro.roi_align_levels(maps, boxes, None, (224, 224))
    assert out.shape == (3, 7, 7, 4) and list(lv[0]) == [0, 2, 0]
    np.testing.assert_allclose(out, 3.25, rtol=0, atol=1e-12)
    # a map linear in x and y gives the bin centres exactly (the 4 samples of a bin are symmetric about its centre)
    h = w = 56
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    lin = np.stack([xx, yy, 2 * xx - 3 * yy + 1, np.ones_like(xx)], axis=-1)[None]
    box = np.asarray([8.0, 12.0, 92.0, 68.0])                                          # 2 .. 23 x 3 .. 17 cells at scale 1 / 4
    got = ro.roi_align_row(lin[0], box, 0.25)
    cx = 2.0 + (np.arange(7) + 0.5) * (21.0 / 7)
    cy = 3.0 + (np.arange(7) + 0.5) * (14.0 / 7)
    np.testing.assert_allclose(got[:, :, 0], np.tile(cx, (7, 1)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, :, 1], np.tile(cy[:, None], (1, 7)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, :, 2], 2 * cx[None, :] - 3 * cy[:, None] + 1, rtol=0, atol=1e-11)
    # the degenerate box x1 = x2 = 224 on the right edge: roi_w = 1 and every sample lies beyond w = 56 - all zeros
    maps = _maps(1, SIZES_224, 1, 4)
    out, lv = ro.roi_align_levels(maps, np.asarray([[[224, 20, 224, 60]]], dtype=np.float32), None, (224, 224))
    assert lv[0, 0] == 0 and not out.any()
    assert (ro.sample_coords(224, 224, 0.25) > 56).all()
    # padding rows are zero and carry level -1
    out, lv = ro.roi_align_levels(maps, np.asarray([[[0, 0, 50, 50], [0, 0, 60, 60]]], dtype=np.float32), [1], (224, 224))
    assert out[0].any() and not out[1].any() and list(lv[0]) == [0, -1]
    # a sample in (-1, 0) is clamped to 0, one in (h - 1, h] carries its weight on the last row alone
    lo, hi, wlo, whi = ro.axis_terms(np.asarray([-0.5, -1.0, -1.01, 6.4, 7.0, 7.01, 2.25]), 7)
    assert list(lo) == [0, 0, 0, 6, 6, 6, 2] and list(hi) == [1, 1, 1, 6, 6, 6, 3]
    np.testing.assert_allclose(wlo, [1, 1, 0, 1, 1, 0, 0.75])
    np.testing.assert_allclose(whi, [0, 0, 0, 0, 0, 0, 0.25])


def test_oracle_levels_at_the_exact_boundaries():
    f = lambda s: [0, 0, s, s]                                                         # noqa: E731
    boxes = np.asarray([f(56), f(112), f(224), f(55.9), f(112.1), f(111.9), f(223.9), [8, 4, 72, 53], [16, 0, 144, 98], f(20),
                        [0, 0, 0, 0], f(448), f(447.9), f(896), f(5000)], dtype=np.float32)
    k = ro.box_levels(boxes, 2, 6) + 2
    # sqrt(area) exactly 56 / 112 / 224 belongs to the UPPER level (the 1e-6 term); 55.9 is clamped up to k_min
    assert list(k) == [2, 3, 4, 2, 3, 2, 3, 2, 3, 2, 2, 5, 4, 6, 6]
    # without the 1e-6 term float32 arithmetic could land just below: the float32 evaluation agrees on the exact boxes
    b32 = boxes[:3]
    s = np.sqrt((b32[:, 2] - b32[:, 0]) * (b32[:, 3] - b32[:, 1]))
    k32 = np.floor(np.float32(4) + np.log2(s / np.float32(224)) + np.float32(1e-6))
    assert list(k32) == [2, 3, 4]
    assert ro.level_margin(boxes[:3]).max() == 0 and ro.level_margin(boxes[3:5]).min() > 5e-4
    for img, sizes in (((224, 224), SIZES_224), ((96, 160), [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)])):
        assert ro.infer_scales(sizes, img) == [1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64]
        b, exact = ro.make_boxes(3, 130, img, sizes)
        assert b.shape == (130, 4) and exact.sum() >= 2
        lv = ro.box_levels(b, 2, 6)
        assert set(lv) >= {0, 1, 3, 4}                                                 # the strided `pool` level is reached


def _grid_sample_restatement(fmap, box, scale, P=7, S=2):
    """Independent restatement: F.grid_sample(align_corners=True) evaluates the bilinear surface at pixel coordinates, the bin is
    the mean of its S x S samples.  Valid where every sample lies in [0, h - 1] x [0, w - 1] (borders are handled differently)."""
    h, w, _ = fmap.shape
    ys, xs = ro.sample_coords(box[1], box[3], scale, P, S), ro.sample_coords(box[0], box[2], scale, P, S)
    gy, gx = np.meshgrid(2 * ys / (h - 1) - 1, 2 * xs / (w - 1) - 1, indexing="ij")
    grid = torch.from_numpy(np.stack([gx, gy], axis=-1))[None]
    src = torch.from_numpy(fmap).permute(2, 0, 1)[None]
    val = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]       # [C, P S, P S]
    return val.reshape(-1, P, S, P, S).mean(dim=(2, 4)).permute(1, 2, 0).numpy(), (ys.min() >= 0 and ys.max() <= h - 1
                                                                                    and xs.min() >= 0 and xs.max() <= w - 1)


def test_oracle_agrees_with_a_grid_sample_restatement():
    maps = _maps(2, SIZES_224, 1, 8)
    boxes, _ = ro.make_boxes(4, 130, (224, 224), SIZES_224)
    scales = ro.infer_scales(SIZES_224, (224, 224))
    lv = ro.box_levels(boxes, 2, 6)
    peak = max(np.abs(m).max() for m in maps)
    n_ok = 0
    for bx, l in zip(boxes.astype(np.float64), lv):
        ref, interior = _grid_sample_restatement(maps[l][0], bx, scales[l])
        if not interior:
            continue
        n_ok += 1
        assert np.abs(ro.roi_align_row(maps[l][0], bx, scales[l]) - ref).max() <= 1e-5 * peak
    assert n_ok >= 65                                                                 # at least half of the boxes qualify


def test_oracle_postprocess_hand_cases():
    NC = 4
    head = np.zeros((5, 5 * NC))
    props = np.asarray([[10, 20, 50, 40], [100, 100, 140, 120], [0, 0, 224, 224], [200, 200, 220, 220], [30, 30, 60, 60]], dtype=np.float32)
    # row 0: equal logits - every score is exactly 1 / 4; zero deltas - the proposal itself
    # row 1: class 2 dominant; deltas of class 2: centre + (0.5 w, -0.5 h) after / 10, w x 2 after / 5, dh clamped
    head[1, :NC] = [0.0, 1.0, 5.0, -2.0]
    head[1, NC + 8:NC + 12] = [5.0, -5.0, 5 * np.log(2.0), 50.0]
    # row 3: class 1 pushed off the right / bottom edge: clipped to a box of zero width
    head[3, :NC] = [0.0, 4.0, 0.0, 0.0]
    head[3, NC + 4:NC + 8] = [100.0, 100.0, 0.0, 0.0]
    box, score, labels, prob, _ = ro.postprocess(head, props, 4, 224, 224, NC, score_thresh=0.25)
    assert box.shape == (15, 4) and list(labels[:6]) == [1, 2, 3, 1, 2, 3]            # candidate r (NC - 1) + (c - 1)
    np.testing.assert_allclose(prob[:3], 0.25, rtol=0, atol=0)
    assert np.isneginf(score[:3]).all()                                               # exactly the threshold: dropped (strict >)
    np.testing.assert_allclose(box[0], props[0])
    _, score_low, _, _, _ = ro.postprocess(head, props, 4, 224, 224, NC, score_thresh=0.2)
    np.testing.assert_allclose(score_low[:3], 0.25)                                   # ... and kept just below it
    e = np.exp(np.asarray([0.0, 1.0, 5.0, -2.0]) - 5.0)
    np.testing.assert_allclose(prob[3:6], (e / e.sum())[1:], rtol=1e-15)
    assert np.isneginf(score[3]) and score[4] == prob[4] and np.isneginf(score[5])
    # anchor 1: w 40, h 20, centre (120, 110) -> centre (140, 100), w 80, h = 20 * 1000 / 16 = 1250 (clamped), clipped to the image
    np.testing.assert_allclose(box[4], [100, 0, 180, 224], atol=1e-9)
    np.testing.assert_allclose(box[3], props[1])                                      # class 1 of the same row: zero deltas
    assert prob[9] > 0.9 and np.isneginf(score[9]) and box[9, 0] == 224 and box[9, 2] == 224       # zero width: dropped, box written
    assert np.isneginf(score[12:]).all() and np.isfinite(prob[12:]).all()             # row 4 >= count: padding
    np.testing.assert_allclose(box[12], props[4])
    # min_size: a 0.009-wide box is dropped, a 0.011-wide one kept
    thin = np.asarray([[10, 10, 10.009, 30], [10, 10, 10.011, 30]], dtype=np.float64)
    _, s, _, _, _ = ro.postprocess(np.zeros((2, 10)), thin, None, 224, 224, 2, score_thresh=0.05)
    assert np.isneginf(s[0]) and s[1] == 0.5
