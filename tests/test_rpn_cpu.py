"""CPU-only checks of the region-proposal stage: the C ABI declares, exports and validates the four entry points without a
device; the anchor generator reproduces torchvision's documented construction; RPNHead has torchvision's parameter names; the
numpy oracle (tests/rpn_oracle.py) passes hand-computed cases.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib
from layoutdit_amd.modeling import AnchorGenerator, RegionProposalNetwork, RPNHead
from tests import rpn_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_rpn_topk_f32", "ldit_rpn_decode_f32", "ldit_nms_batched_f32", "ldit_nms_workspace_bytes")


def test_header_declares_and_library_exports_the_proposal_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6       # purely additive


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    sizes = (C.c_int64 * 5)(9408, 2352, 588, 147, 48)
    # top-k
    assert lib.ldit_rpn_topk_f32(None, sizes, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL and "null" in err()
    assert lib.ldit_rpn_topk_f32(16, None, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL
    assert lib.ldit_rpn_topk_f32(8, sizes, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL and "aligned" in err()
    assert lib.ldit_rpn_topk_f32(16, sizes, 5, 2, 0, 16, None) == _lib.LDIT_EINVAL
    big = (C.c_int64 * 2)(16385, 48)
    assert lib.ldit_rpn_topk_f32(16, big, 2, 2, 1000, 16, None) == _lib.LDIT_EUNSUPPORTED and "16384" in err()
    many = (C.c_int64 * 9)(*([8] * 9))
    assert lib.ldit_rpn_topk_f32(16, many, 9, 2, 4, 16, None) == _lib.LDIT_EUNSUPPORTED and "levels" in err()
    zero = (C.c_int64 * 2)(16, 0)
    assert lib.ldit_rpn_topk_f32(16, zero, 2, 2, 4, 16, None) == _lib.LDIT_EINVAL
    # decode
    assert lib.ldit_rpn_decode_f32(16, 16, 16, None, 2, 100, 10, 224.0, 224.0, 1e-3, 0.0, 16, 16, None) == _lib.LDIT_EINVAL and "null" in err()
    assert lib.ldit_rpn_decode_f32(16, 16, 16, 16, 2, 100, 10, 224.0, 224.0, 1e-3, 0.0, 16, 4, None) == _lib.LDIT_EINVAL and "aligned" in err()
    assert lib.ldit_rpn_decode_f32(16, 16, 16, 16, 2, 100, 0, 224.0, 224.0, 1e-3, 0.0, 16, 16, None) == _lib.LDIT_EINVAL
    assert lib.ldit_rpn_decode_f32(16, 16, 16, 16, 2, 100, 10, 0.0, 224.0, 1e-3, 0.0, 16, 16, None) == _lib.LDIT_EINVAL
    # NMS
    nms = lib.ldit_nms_batched_f32
    assert nms(None, 16, None, 3, 300, 0.7, 100, 16, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL and "null" in err()
    assert nms(16, 16, None, 3, 300, 0.7, 100, None, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, None, 3, 300, 0.7, 100, 16, None, None, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, 4, 3, 300, 0.7, 100, 16, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL and "aligned" in err()
    assert nms(16, 16, None, 3, 300, 0.7, 100, 16, 16, 24, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, None, 3, 300, 0.7, 0, 16, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, None, 0, 300, 0.7, 100, 16, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, None, 3, 300, float("nan"), 100, 16, 16, None, None, None, 0, None) == _lib.LDIT_EINVAL
    assert nms(16, 16, None, 3, 8193, 0.7, 100, 16, 16, None, None, None, 0, None) == _lib.LDIT_EUNSUPPORTED and "8192" in err()
    # workspace: whatever ldit_nms_workspace_bytes asks for must be there in full
    need = lib.ldit_nms_workspace_bytes(3, 4783)
    assert need == lib.ldit_nms_workspace_bytes(3, 4783) and need % 16 == 0
    if need:
        assert nms(16, 16, None, 3, 4783, 0.7, 100, 16, 16, None, None, 16, need - 1, None) == _lib.LDIT_EWORKSPACE
        assert nms(16, 16, None, 3, 4783, 0.7, 100, 16, 16, None, None, None, need, None) == _lib.LDIT_EWORKSPACE
    assert nms(16, 16, None, 3, 4783, 0.7, 100, 16, 16, None, None, 8, need, None) == _lib.LDIT_EINVAL      # misaligned workspace


EXPECTED_BASE = {
    32: [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]],
    64: [[-45, -23, 45, 23], [-32, -32, 32, 32], [-23, -45, 23, 45]],
    128: [[-91, -45, 91, 45], [-64, -64, 64, 64], [-45, -91, 45, 91]],
    256: [[-181, -91, 181, 91], [-128, -128, 128, 128], [-91, -181, 91, 181]],
    512: [[-362, -181, 362, 181], [-256, -256, 256, 256], [-181, -362, 181, 362]],
}


def _reference_generator():
    return AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)


def test_base_anchors_match_torchvisions_construction():
    base = _reference_generator().base_anchors()
    for got, size in zip(base, (32, 64, 128, 256, 512)):
        np.testing.assert_array_equal(got, np.asarray(EXPECTED_BASE[size], dtype=np.float32))
    # the un-nested spelling of torchvision's constructor
    g = AnchorGenerator(sizes=(32, 64), aspect_ratios=(0.5, 1.0, 2.0))
    assert g.sizes == ((32,), (64,)) and g.num_anchors_per_location() == [3, 3]
    # several sizes per level: ratio-major, size-minor
    g = AnchorGenerator(sizes=((32, 64),), aspect_ratios=((0.5, 1.0),))
    np.testing.assert_array_equal(g.base_anchors()[0], np.asarray([EXPECTED_BASE[32][0], EXPECTED_BASE[64][0], EXPECTED_BASE[32][1],
                                                                   EXPECTED_BASE[64][1]], dtype=np.float32))


def test_grid_anchors_at_224():
    g = _reference_generator()
    grids = [(56, 56), (28, 28), (14, 14), (7, 7), (4, 4)]
    a, level_sizes = g.host_anchors(grids, (224, 224))
    assert level_sizes == (9408, 2352, 588, 147, 48) and a.shape == (12543, 4) and a.dtype == np.float32
    off = 0
    for (gh, gw), stride, size in zip(grids, (4, 8, 16, 32, 56), (32, 64, 128, 256, 512)):
        lvl = a[off:off + gh * gw * 3].reshape(gh, gw, 3, 4)
        base = np.asarray(EXPECTED_BASE[size], dtype=np.float32)
        np.testing.assert_array_equal(lvl[0, 0], base)                                            # (y, x, anchor) order
        np.testing.assert_array_equal(lvl[0, 1], base + np.asarray([stride, 0, stride, 0], dtype=np.float32))
        np.testing.assert_array_equal(lvl[gh - 1, 2], base + np.asarray([2 * stride, (gh - 1) * stride] * 2, dtype=np.float32))
        off += gh * gw * 3
    t, ls = g(grids, (224, 224), "cpu")
    assert ls == level_sizes and torch.equal(t, torch.from_numpy(a))
    assert g(grids, (224, 224), "cpu")[0] is t                                                    # cached per geometry
    with pytest.raises(ValueError, match="levels"):
        g.host_anchors(grids[:3], (224, 224))


def test_rpn_modules_have_torchvisions_surface():
    head = RPNHead(256, 3)
    assert list(head.state_dict()) == ["conv.0.0.weight", "conv.0.0.bias", "cls_logits.weight", "cls_logits.bias", "bbox_pred.weight",
                                       "bbox_pred.bias"]
    sd = head.state_dict()
    assert tuple(sd["conv.0.0.weight"].shape) == (256, 256, 3, 3) and tuple(sd["cls_logits.weight"].shape) == (3, 256, 1, 1)
    assert tuple(sd["bbox_pred.weight"].shape) == (12, 256, 1, 1)
    rpn = RegionProposalNetwork(_reference_generator(), head)
    assert (rpn.pre_nms_top_n, rpn.post_nms_top_n, rpn.nms_thresh, rpn.score_thresh, rpn.min_size) == (1000, 1000, 0.7, 0.0, 1e-3)
    assert sorted(rpn.state_dict()) == sorted("head." + k for k in sd)
    with pytest.raises(RuntimeError, match="inference only"):
        rpn.train()([torch.zeros(1, 256, 4, 4)], (224, 224))
    with pytest.raises(ValueError, match="GPU"):                                                  # no CPU path
        rpn.eval()([torch.zeros(1, 256, 4, 4)], (224, 224))
    from layoutdit_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.nms(torch.zeros(3, 4), torch.zeros(3), 0.5)
    with pytest.raises(ValueError, match="GPU"):
        ops.rpn_topk(torch.zeros(2, 8), [8], 4)


def test_oracle_topk_hand_cases():
    v = np.asarray([1.0, np.nan, -np.inf, 3.0, 3.0, -0.0, 0.0, 2.0], dtype=np.float32)
    np.testing.assert_array_equal(ro.topk_indices(v, [8], 8), [3, 4, 7, 0, 5, 6, 2, 1])
    np.testing.assert_array_equal(ro.topk_indices(v, [8], 3), [3, 4, 7])
    np.testing.assert_array_equal(ro.topk_indices(v, [3, 5], 2), [0, 2, 3, 4])                     # per level, offsets added, k > n_l clipped below
    np.testing.assert_array_equal(ro.topk_indices(v, [2, 6], 4), [0, 1, 3, 4, 7, 5])


def test_oracle_decode_hand_cases():
    anchors = np.asarray([[0, 0, 10, 20], [100, 100, 140, 120], [200, 200, 220, 220], [-50, -50, -10, -10]], dtype=np.float32)
    deltas = np.asarray([[0, 0, 0, 0], [0.5, -0.5, np.log(2.0), 10.0], [1.0, 1.0, 0, 0], [0, 0, 0, 0]], dtype=np.float32)
    logits = np.asarray([0.0, 2.0, -2.0, 5.0], dtype=np.float32)
    box, score, _ = ro.decode(logits, deltas, anchors, np.arange(4), 224, 224, 1e-3, 0.0)
    np.testing.assert_allclose(box[0], [0, 0, 10, 20])                                            # identity
    # anchor 1: w 40 h 20, centre (120, 110) -> centre (140, 100), w 80, h = 20 * 1000/16 = 1250 (dh clamped), clipped to the image
    np.testing.assert_allclose(box[1], [100, 0, 180, 224], atol=1e-4)
    np.testing.assert_allclose(box[2], [220, 220, 224, 224])                                      # clipped right / bottom
    np.testing.assert_allclose(box[3], [0, 0, 0, 0])                                              # entirely outside: width exactly 0
    assert score[0] == 0.5 and abs(score[1] - 1 / (1 + np.exp(-2.0))) < 1e-12 and score[3] == -np.inf
    _, score, _ = ro.decode(logits, deltas, anchors, np.arange(4), 224, 224, 1e-3, 0.2)
    assert score[2] == -np.inf and score[0] == 0.5                                                # sigmoid(-2) = 0.119 < 0.2


def test_oracle_nms_hand_cases():
    f = np.float32
    # IoU exactly 0.5 at thr 0.5: kept (strict >)
    b = np.asarray([[0, 0, 10, 10], [0, 0, 10, 5]], dtype=f)
    assert ro.iou_f32(b[0], b[1:])[0] == f(0.5)
    keep, count = ro.nms(b, np.asarray([2, 1], dtype=f), None, 0.5, 4)
    assert count == 2 and list(keep) == [0, 1, -1, -1]
    keep, count = ro.nms(b, np.asarray([2, 1], dtype=f), None, 0.49, 4)
    assert count == 1 and list(keep) == [0, -1, -1, -1]
    # IoU exactly 7/10: 70 / 100 rounds to 0.7f, and 0.7f > 0.7f is false - a float64 comparison (0.7 > double(0.7f)) would suppress
    b = np.asarray([[0, 0, 10, 10], [0, 0, 10, 7]], dtype=f)
    assert ro.iou_f32(b[0], b[1:])[0] == f(0.7) and 0.7 > float(f(0.7))
    assert ro.nms(b, np.asarray([2, 1], dtype=f), None, 0.7, 2)[1] == 2
    # chain: A suppresses B, B would suppress C, C survives because B was never kept
    b = np.asarray([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]], dtype=f)
    assert ro.iou_f32(b[0], b[1:2])[0] > 0.5 and ro.iou_f32(b[1], b[2:])[0] > 0.5 and ro.iou_f32(b[0], b[2:])[0] < 0.5
    keep, count = ro.nms(b, np.asarray([3, 2, 1], dtype=f), None, 0.5, 3)
    assert count == 2 and list(keep) == [0, 2, -1]
    # groups separate, ties go to the lower index, -inf / NaN take no part, truncation
    same = np.asarray([[0, 0, 10, 10]] * 4, dtype=f)
    keep, count = ro.nms(same, np.asarray([1, 1, 1, 1], dtype=f), np.asarray([0, 1, 0, 1]), 0.5, 4)
    assert count == 2 and list(keep) == [0, 1, -1, -1]
    keep, count = ro.nms(same, np.asarray([-np.inf, np.nan, 1, 5], dtype=f), None, 0.5, 4)
    assert count == 1 and list(keep) == [3, -1, -1, -1]
    far = np.asarray([[0, 0, 1, 1], [5, 5, 6, 6], [9, 9, 10, 10]], dtype=f)
    keep, count = ro.nms(far, np.asarray([1, 3, 2], dtype=f), None, 0.5, 2)
    assert count == 2 and list(keep) == [1, 2]
    assert ro.nms(far, np.full(3, -np.inf, dtype=f), None, 0.5, 2)[1] == 0


def test_oracle_generators_are_exact_and_hit_the_threshold():
    b, s, g = ro.clustered_problem(7, 2783, n_groups=5)
    assert b.min() >= 0 and b.max() <= 224 and np.all(b * 4 == np.round(b * 4)) and np.all(b[:, 2:] > b[:, :2])
    assert len(np.unique(s)) == 2783 and g.min() == 0 and g.max() == 4
    _, count = ro.nms(b, s, None, 0.7, 2783)
    assert 60 <= 2783 - count <= 3800
    # the fp32 IoU of snapped boxes is the correctly rounded quotient of two exactly represented numbers
    d = b[:400].astype(np.float64)
    area = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
    iw = np.maximum(np.minimum(d[:, None, 2], d[None, :, 2]) - np.maximum(d[:, None, 0], d[None, :, 0]), 0)
    ih = np.maximum(np.minimum(d[:, None, 3], d[None, :, 3]) - np.maximum(d[:, None, 1], d[None, :, 1]), 0)
    exact = (iw * ih / (area[:, None] + area[None, :] - iw * ih)).astype(np.float32)
    got = np.stack([ro.iou_f32(b[i], b[:400]) for i in range(400)])
    np.testing.assert_array_equal(got, exact)
    b, s, g, seed = ro.random_problem_away_from_threshold(11, 512, 0.7, n_groups=3)
    assert b.shape == (512, 4) and seed >= 11 and 0 < ro.nms(b, s, g, 0.7, 512)[1] < 512
