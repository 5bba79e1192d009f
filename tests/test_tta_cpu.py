"""Test-time augmentation without a GPU: the numpy oracle against a brute-force float64 statement of the definition, the oracle's
identities, ``TestTimeAugment``'s checks and view order, the host checks of ``ops.tta_*`` and the C entries, and the ABI surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import layoutdit_amd
from layoutdit_amd import _lib, ops
from layoutdit_amd.tta import TestTimeAugment, TTAView

from . import tta_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_tta_pool_f32", "ldit_box_vote_f32")
F32 = np.float32


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("vote_thresh", [None, 0.6])
def test_oracle_agrees_with_the_brute_force_definition_where_the_margin_is_large(seed, vote_thresh):
    """The float32 oracle and the float64 loops take the same decisions when no IoU lies within 1e-4 of a threshold (float32 IoUs of
    boxes of this size are good to ~1e-6), and their boxes then differ by float32 rounding only."""
    views, specs, pages = to.random_views(seed, B=3, K=3, V=4, D=12)
    boxes, scores, labels, count, margin = to.merge(views, specs, pages, 0.5, 20, vote_thresh)
    assert margin >= 1e-4, margin                                # a condition on the inputs
    bb, bs, bl, bn = to.brute_force(views, specs, pages, 0.5, 20, vote_thresh)
    assert count.tolist() == bn.tolist() and int(count.min()) > 0
    assert np.array_equal(labels, bl) and np.array_equal(scores.astype(np.float64), bs)
    # coordinates up to 400, three float32 roundings (unmirror, ratio, product) of relative size 2^-24 each
    np.testing.assert_allclose(boxes.astype(np.float64), bb, rtol=0, atol=400 * 4 * 2.0 ** -24)


def test_one_plain_view_at_the_pages_size_without_vote_is_the_input_times_the_ratio():
    """Already class-wise suppressed detections (far apart), one plain view: the merge keeps every one, in score order, as ``box *
    (rw, rh, rw, rh)`` with the float32 ratios of ``resize_boxes``."""
    rng = np.random.RandomState(0)
    B, D, W, H = 2, 6, 96, 64
    pages = [(200, 300), (64, 96)]
    boxes = np.zeros((B, D, 4), F32)
    for d in range(D):
        boxes[:, d] = [16 * d + 0.5, 3.25, 16 * d + 9.75, 40.5]                       # disjoint columns
    scores = np.sort(rng.uniform(0.1, 1, (B, D)).astype(F32), axis=1)[:, ::-1].copy()
    labels = rng.randint(1, 4, (B, D)).astype(np.int32)
    count = np.array([D, 4], np.int32)
    ob, os_, ol, oc, _ = to.merge([(boxes, scores, labels, count)], [(W, H, 0)], pages, 0.5, D, None)
    assert oc.tolist() == [D, 4]
    for b, (oh, ow) in enumerate(pages):
        rw, rh = F32(float(ow) / float(W)), F32(float(oh) / float(H))
        n = count[b]
        assert np.array_equal(ob[b, :n], boxes[b, :n] * np.array([rw, rh, rw, rh], F32))
        assert np.array_equal(os_[b, :n], scores[b, :n]) and np.array_equal(ol[b, :n], labels[b, :n])
        assert not ob[b, n:].any() and not os_[b, n:].any() and not ol[b, n:].any()
    # the second page is the view's own size: ratio 1, the input's bits
    assert np.array_equal(ob[1, :4], boxes[1, :4])


def test_unmirroring_twice_is_the_identity_on_integer_boxes():
    rng = np.random.RandomState(4)
    x = np.sort(rng.randint(0, 225, size=(50, 2)), axis=1)
    y = np.sort(rng.randint(0, 225, size=(50, 2)), axis=1)
    b = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(F32)
    once = to.unmirror(b, 224)
    assert np.array_equal(to.unmirror(once, 224), b)
    assert np.array_equal(once[:, 0], 224 - b[:, 2]) and np.array_equal(once[:, [1, 3]], b[:, [1, 3]])
    touching = np.array([[0, 0, 224, 10]], F32)                                         # both borders: its own mirror image
    assert np.array_equal(to.unmirror(touching, 224), touching)


def test_oracle_edges_duplicates_labels_degenerate_and_empty():
    f = F32
    box = [10, 10, 50, 40]
    # exact duplicates across two views: the lower pool index survives, the vote returns the same box
    v = (np.array([[box]], f), np.array([[0.9]], f), np.array([[2]], np.int32), np.array([1], np.int32))
    ob, os_, ol, oc, _ = to.merge([v, v], [(64, 64, 0), (64, 64, 0)], [(64, 64)], 0.5, 4, 0.5)
    assert oc.tolist() == [1] and ol[0, 0] == 2 and np.array_equal(ob[0, 0], np.array(box, np.float64))
    pb, ps, pl = to.pool([v, v], [(64, 64, 0), (64, 64, 0)], [(64, 64)])
    keep, n = to.nms(pb[0], ps[0], pl[0], 0.5, 4)
    assert n == 1 and keep.tolist() == [0, -1, -1, -1]
    # two labels with identical boxes: both kept, neither votes for the other
    w = (np.array([[box, [12, 10, 50, 40]]], f), np.array([[0.9, 0.8]], f), np.array([[1, 2]], np.int32), np.array([2], np.int32))
    ob, _, ol, oc, _ = to.merge([w], [(64, 64, 0)], [(64, 64)], 0.5, 4, 0.0)
    assert oc.tolist() == [2] and ol[0, :2].tolist() == [1, 2]
    assert np.array_equal(ob[0, 0], np.array(box, np.float64)) and np.array_equal(ob[0, 1], np.array([12, 10, 50, 40], np.float64))
    # a zero-area box: kept (its IoU with anything is 0 or NaN) and votes only for itself
    z = (np.array([[[20, 20, 20, 20], box]], f), np.array([[0.9, 0.8]], f), np.array([[1, 1]], np.int32), np.array([2], np.int32))
    ob, _, _, oc, _ = to.merge([z], [(64, 64, 0)], [(64, 64)], 0.5, 4, 0.5)
    assert oc.tolist() == [2] and np.array_equal(ob[0, 0], np.array([20, 20, 20, 20], np.float64))
    # every view empty: count 0 and an all-zero result, whatever the padding rows hold
    e = (np.full((1, 3, 4), np.nan, f), np.full((1, 3), 3e38, f), np.full((1, 3), 7, np.int32), np.array([0], np.int32))
    ob, os_, ol, oc, margin = to.merge([e, e], [(64, 64, 0), (64, 64, 1)], [(64, 64)], 0.5, 4, 0.5)
    assert oc.tolist() == [0] and not ob.any() and not os_.any() and not ol.any() and margin == float("inf")


def test_view_order_is_plain_first_then_mirrored():
    t = TestTimeAugment(sizes=[(64, 64), (96, 64)], flip=True)
    assert t.views() == [TTAView(64, 64, 0), TTAView(96, 64, 0), TTAView(64, 64, 1), TTAView(96, 64, 1)]
    assert TestTimeAugment(sizes=[(96, 96)], flip=False).views() == [(96, 96, 0)]
    with pytest.raises(ValueError, match="pass the model"):
        TestTimeAugment().views()

    class _Stub:                                                  # what views() / merge_args() read of a LayoutDetectionModel
        class model:
            class transform:
                out_w, out_h = 96, 64

            class roi_heads:
                nms_thresh, detections_per_img = 0.4, 50

    assert TestTimeAugment().views(_Stub) == [(96, 64, 0), (96, 64, 1)]
    assert TestTimeAugment().merge_args(_Stub) == (0.4, 50, None)
    assert TestTimeAugment(nms_thresh=0.6, vote_thresh=0.7, detections_per_img=10).merge_args(_Stub) == (0.6, 10, 0.7)
    assert layoutdit_amd.TestTimeAugment is TestTimeAugment       # exported from the package


@pytest.mark.parametrize("kwargs,message", [
    (dict(sizes=[(64, 64)] * 9), "18 views"),
    (dict(sizes=[(64, 64)] * 17, flip=False), "17 views"),
    (dict(sizes=[(100, 64)]), "multiple of 32"),
    (dict(sizes=[(64, 0)]), "multiple of 32"),
    (dict(sizes=[(64,)]), "width, height"),
    (dict(sizes=[(64.0, 64)]), "width, height"),
    (dict(sizes=[]), "empty"),
    (dict(nms_thresh=1.5), "nms_thresh"),
    (dict(nms_thresh=float("nan")), "nms_thresh"),
    (dict(vote_thresh=-0.1), "vote_thresh"),
    (dict(detections_per_img=0), "detections_per_img"),
])
def test_test_time_augment_validates_at_construction(kwargs, message):
    with pytest.raises(ValueError, match=message):
        TestTimeAugment(**kwargs)


def _cpu_view(B, D):
    return (torch.zeros(B, D, 4), torch.zeros(B, D), torch.zeros(B, D, dtype=torch.int32), torch.zeros(B, dtype=torch.int32))


def test_ops_check_the_pool_limit_and_the_host_arguments_before_any_launch():
    """CPU tensors: every host check comes before the device is asked for."""
    assert ops.NMS_MAX_CANDIDATES == 8192
    with pytest.raises(ValueError, match=r"2 views x 4097 detections = 8194 pool entries per image, at most NMS_MAX_CANDIDATES = 8192"):
        ops.tta_merge([_cpu_view(1, 4097)] * 2, [(64, 64, 0), (64, 64, 1)], [(64, 64)])
    with pytest.raises(ValueError, match="NMS_MAX_CANDIDATES"):
        ops.tta_pool([_cpu_view(1, 600)] * 14, [(64, 64, 0)] * 14, [(64, 64)])
    with pytest.raises(ValueError, match="17 views"):
        ops.tta_pool([_cpu_view(1, 4)] * 17, [(64, 64, 0)] * 17, [(64, 64)])
    with pytest.raises(ValueError, match="1 view specs for 2 views"):
        ops.tta_pool([_cpu_view(1, 4)] * 2, [(64, 64, 0)], [(64, 64)])
    with pytest.raises(ValueError, match=r"view_specs\[1\]"):
        ops.tta_pool([_cpu_view(1, 4)] * 2, [(64, 64, 0), (64, 64, 2)], [(64, 64)])
    with pytest.raises(ValueError, match="2 original sizes for 1 images"):
        ops.tta_pool([_cpu_view(1, 4)], [(64, 64, 0)], [(64, 64), (64, 64)])
    with pytest.raises(ValueError, match=r"views\[1\]: labels"):
        ops.tta_pool([_cpu_view(1, 4), _cpu_view(1, 4)[:2] + (torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32))], [(64, 64, 0)] * 2, [(64, 64)])
    with pytest.raises(ValueError, match="vote_thresh"):
        ops.tta_merge([_cpu_view(1, 4)], [(64, 64, 0)], [(64, 64)], vote_thresh=1.01)
    with pytest.raises(ValueError, match="GPU"):                  # all host checks passed: only now the device matters
        ops.tta_merge([_cpu_view(1, 4)], [(64, 64, 0)], [(64, 64)])
    keep, kept = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="vote_thresh"):
        ops.box_vote(torch.zeros(1, 8, 4), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32), keep, kept, 2.0)
    with pytest.raises(ValueError, match="pool_labels"):
        ops.box_vote(torch.zeros(1, 8, 4), torch.zeros(1, 8), torch.zeros(1, 8), keep, kept, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        ops.box_vote(torch.zeros(1, 8, 4), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32), keep, kept, 0.5)


def test_c_entries_validate_their_arguments_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                        # noqa: E731
    EINVAL = _lib.LDIT_EINVAL

    def pool(V=2, B=1, D=4, specs=(64, 64, 0, 64, 64, 1), pages=(64, 64), ptr=4096, out=8192, null_view=False):
        p = (C.c_void_p * 16)(*([ptr] * 16))
        q = (C.c_void_p * 16)(*([None if null_view else ptr] * 16))
        return lib.ldit_tta_pool_f32(p, q, p, p, (C.c_int32 * len(specs))(*specs), (C.c_int32 * len(pages))(*pages), V, B, D, out, out, out, None)

    assert lib.ldit_tta_pool_f32(None, None, None, None, None, None, 1, 1, 1, None, None, None, None) == EINVAL
    assert err().startswith("tta_pool: null")
    assert pool(null_view=True) == EINVAL and "tta_pool: null" in err()
    for kw in (dict(V=0), dict(B=0), dict(D=0), dict(D=-3)):
        assert pool(**kw) == EINVAL and "tta_pool: bad geometry" in err()
    assert pool(V=17) == EINVAL and "tta_pool: 17 views" in err()
    assert pool(D=4097) == _lib.LDIT_EUNSUPPORTED and "8194 pool entries" in err()
    assert pool(ptr=4100) == EINVAL and "16-byte aligned" in err()
    assert pool(out=8200) == EINVAL and "16-byte aligned" in err()
    assert pool(specs=(64, 0, 0, 64, 64, 1)) == EINVAL and "tta_pool: view 0" in err()
    assert pool(specs=(64, 64, 0, 64, 64, 2)) == EINVAL and "tta_pool: view 1" in err()
    assert pool(pages=(64, -1)) == EINVAL and "tta_pool: image 0" in err()
    assert pool(out=4096) == EINVAL and "alias" in err()

    def vote(B=1, N=8, Dout=4, thr=0.5, pool_ptr=4096, out_boxes=8192, out_labels=12288, keep=16384):
        return lib.ldit_box_vote_f32(pool_ptr, 4096, 4096, keep, 4096, B, N, Dout, thr, out_boxes, out_labels, None)

    assert vote(out_labels=None) == EINVAL and err().startswith("box_vote: null")
    assert vote(keep=None) == EINVAL and err().startswith("box_vote: null")
    for kw in (dict(B=0), dict(N=0), dict(Dout=0)):
        assert vote(**kw) == EINVAL and "box_vote: bad geometry" in err()
    for thr in (-0.01, 1.01, float("nan")):
        assert vote(thr=thr) == EINVAL and "box_vote: vote_thresh" in err()
    assert vote(pool_ptr=4100) == EINVAL and "16-byte aligned" in err()
    assert vote(out_boxes=8200) == EINVAL and "16-byte aligned" in err()
    assert vote(N=8193) == _lib.LDIT_EUNSUPPORTED and "8193 pool entries" in err()
    assert vote(out_boxes=4096) == EINVAL and "alias" in err()


def test_header_declares_and_library_exports_both_entries_with_matching_arity():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    raw = open(os.path.join(ROOT, "include", "ldit.h")).read()
    assert "test-time augmentation" in raw
    lib = _lib.load()
    for n in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, text)
        assert m, f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), n
    assert lib.ldit_abi_version() == _lib.LDIT_ABI_VERSION                              # purely additive: the version stays


def test_python_surface_defaults_change_nothing():
    from layoutdit_amd.evaluation import evaluate
    from layoutdit_amd.modeling.detector import LayoutDetectionModel
    assert inspect.signature(LayoutDetectionModel.forward).parameters["tta"].default is None
    assert inspect.signature(evaluate).parameters["tta"].default is None
    assert list(inspect.signature(LayoutDetectionModel.forward).parameters)[:3] == ["self", "images", "targets"]
    sig = inspect.signature(ops.tta_merge).parameters
    assert (sig["nms_thresh"].default, sig["detections_per_img"].default, sig["vote_thresh"].default) == (0.5, 100, None)
    assert hasattr(LayoutDetectionModel, "forward_padded_tta")
