"""CPU-only checks of the RPN's training side: the C ABI declares, exports and validates the new entry points without a device;
the numpy oracle (tests/rpn_train_oracle.py) passes hand-computed cases of the matcher, the promotion quirk and the sampler; its
losses and gradients agree with float64 torch autograd; the test scenes make the fp32 IoU exact up to its one division; the
modules have the new constructor arguments and keep their refusals.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from layoutdit_amd import _lib, ops
from layoutdit_amd import config as cfgs
from layoutdit_amd.modeling import AnchorGenerator, LayoutDetectionModel, RegionProposalNetwork, RPNHead
from tests import rpn_train_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_rpn_targets_f32", "ldit_rpn_loss_f32", "ldit_rpn_loss_workspace_bytes")
f = np.float32


def _reference_anchors(size=(224, 224)):
    gen = AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)
    h, w = size
    grids = [(h // 4, w // 4), (h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32), ((h // 32 + 1) // 2, (w // 32 + 1) // 2)]
    return gen.host_anchors(grids, size)[0]


def test_header_declares_and_library_exports_the_training_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    tg = lib.ldit_rpn_targets_f32

    def targets(anchors=16, gt=16, cnt=16, keys=16, B=2, N=1000, G=8, fg=0.7, bg=0.3, bs=256, frac=0.5, lab=16, mat=16, reg=16, smp=16):
        return tg(anchors, gt, cnt, keys, B, N, G, fg, bg, bs, frac, lab, mat, reg, smp, None)

    for name in ("anchors", "gt", "cnt", "keys", "lab", "mat", "reg", "smp"):
        assert targets(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
        assert targets(**{name: 8}) == _lib.LDIT_EINVAL and "aligned" in err(), name
    assert targets(B=0) == _lib.LDIT_EINVAL and targets(N=0) == _lib.LDIT_EINVAL and targets(G=0) == _lib.LDIT_EINVAL
    assert targets(fg=0.3, bg=0.7) == _lib.LDIT_EINVAL and "bg" in err()              # bg_thr > fg_thr
    assert targets(fg=float("nan")) == _lib.LDIT_EINVAL
    assert targets(bs=0) == _lib.LDIT_EINVAL and targets(bs=-4) == _lib.LDIT_EINVAL and "batch_size" in err()
    for frac in (0.0, -0.5, 1.5, float("nan")):
        assert targets(frac=frac) == _lib.LDIT_EINVAL and "positive_fraction" in err(), frac
    assert targets(N=16385) == _lib.LDIT_EUNSUPPORTED and "16384" in err()
    assert targets(G=513) == _lib.LDIT_EUNSUPPORTED and "512" in err()                # Gmax: at least 256 must be handled

    ls = lib.ldit_rpn_loss_f32

    def loss(logits=16, deltas=16, labels=16, reg=16, smp=16, B=2, N=1000, beta=1 / 9, out=16, dl=16, dd=16, ws=16, nbytes=1 << 20):
        return ls(logits, deltas, labels, reg, smp, B, N, beta, out, dl, dd, ws, nbytes, None)

    for name in ("logits", "deltas", "labels", "reg", "smp", "out", "dl", "dd"):
        assert loss(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
        assert loss(**{name: 8}) == _lib.LDIT_EINVAL and "aligned" in err(), name
    assert loss(B=0) == _lib.LDIT_EINVAL and loss(N=0) == _lib.LDIT_EINVAL
    assert loss(beta=-1.0) == _lib.LDIT_EINVAL and loss(beta=float("nan")) == _lib.LDIT_EINVAL and "beta" in err()
    need = lib.ldit_rpn_loss_workspace_bytes(2, 12543)
    assert need > 0 and need % 16 == 0 and need == lib.ldit_rpn_loss_workspace_bytes(2, 12543)
    assert loss(N=12543, nbytes=need - 1) == _lib.LDIT_EWORKSPACE and loss(N=12543, ws=None, nbytes=need) == _lib.LDIT_EWORKSPACE
    assert loss(N=12543, ws=8, nbytes=need) == _lib.LDIT_EINVAL                       # misaligned workspace


def test_front_ends_refuse_cpu_tensors_and_bad_settings():
    a, gt = torch.zeros(8, 4), torch.zeros(1, 2, 4)
    cnt, keys = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.rpn_targets(a, gt, cnt, keys)
    with pytest.raises(ValueError, match="GPU"):
        ops.rpn_loss(torch.zeros(1, 8), torch.zeros(1, 8, 4), keys, torch.zeros(1, 8, 4), torch.zeros(1, 2, dtype=torch.int32))


def test_oracle_matcher_hand_cases():
    anchors = np.asarray([[0, 0, 10, 10], [0, 0, 10, 7], [0, 0, 10, 3], [50, 50, 60, 60], [100, 100, 110, 110]], dtype=f)
    # a GT equal to an anchor: positive with zero targets; IoU exactly 7/10 is positive; exactly 3/10 is ignored, not negative
    gt = np.asarray([[0, 0, 10, 10]], dtype=f)
    m, iou = to.match(anchors, gt)
    assert iou[0, 0] == f(1) and iou[0, 1] == f(0.7) and iou[0, 2] == f(0.3) and 0.7 > float(f(0.7)) and 0.3 < float(f(0.3))
    assert list(m) == [0, 0, -2, -1, -1]
    assert list(to.match(anchors, gt, bg_thr=float(np.nextafter(f(0.3), f(1))))[0]) == [0, 0, -1, -1, -1]
    t = to.encode(anchors, gt, m)
    assert not t[0].any() and not t[2:].any()
    np.testing.assert_allclose(t[1], [0, (5 - 3.5) / 7, 0, np.log(10 / 7)], rtol=1e-15)
    # duplicate GTs resolve to the lower index, also under promotion
    m, _ = to.match(anchors, np.asarray([[50, 50, 60, 60], [0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]], dtype=f))
    assert list(m) == [1, 1, -2, 0, -1]
    # the promotion quirk.  GT A's best anchor is anchor 0 (IoU 0.4, below both thresholds' positive side) - but anchor 0 overlaps
    # GT B more (0.5): it is promoted BY A and keeps its match to B.  B's own best is anchor 1 (IoU 1).
    anchors = np.asarray([[0, 0, 10, 10], [0, 0, 10, 5], [200, 200, 210, 210]], dtype=f)
    gt_a, gt_b = [0, 6, 10, 10], [0, 0, 10, 5]
    m, iou = to.match(anchors, np.asarray([gt_a, gt_b], dtype=f))
    assert iou[0, 0] == f(0.4) and iou[1, 0] == f(0.5) and iou[0].max() == f(0.4) and iou[1, 1] == f(1)
    assert list(m) == [1, 1, -1]
    assert list(to.match(anchors, np.asarray([gt_a], dtype=f))[0]) == [0, -1, -1]     # without B it is A's
    # an image without GT: everything negative, zero targets; GT rows past the count never matter
    m, _ = to.match(anchors, np.zeros((0, 4), dtype=f))
    assert list(m) == [-1, -1, -1] and not to.encode(anchors, np.zeros((0, 4)), m).any()
    gtb, cnt = to.pad_gt([np.asarray([gt_b], dtype=f), np.zeros((0, 4), dtype=f)], gmax=3)
    assert np.isnan(gtb[0, 1:]).all() and np.isnan(gtb[1]).all() and list(cnt) == [1, 0]
    lab, mat, reg, smp = to.targets(anchors, gtb, cnt, np.zeros((2, 3), dtype=np.int32))
    assert list(mat[0]) == [-2, 0, -1] and list(mat[1]) == [-1, -1, -1] and np.isfinite(reg).all()
    assert list(lab[0]) == [-1, 1, 0] and list(lab[1]) == [0, 0, 0] and list(smp[0]) == [1, 1] and list(smp[1]) == [0, 3]


def test_oracle_sampler_hand_cases():
    # more positives than the quota: the two smallest keys; negatives fill the rest; ignored anchors are never taken
    matched = np.asarray([0, 0, 0, 0, -1, -1, -1, -2, -2], dtype=np.int32)
    keys = np.asarray([5, 1, 9, 3, 7, 2, 8, 0, 0], dtype=np.int32)
    lab, taken = to.sample(matched, keys, batch_size=4, positive_fraction=0.5)
    assert taken == (2, 2) and list(lab) == [-1, 1, -1, 1, 0, 0, -1, -1, -1]
    # fewer negatives than needed: all of them, the batch stays short; fewer positives than the quota: negatives take the room
    lab, taken = to.sample(matched, keys, batch_size=16, positive_fraction=0.25)
    assert taken == (4, 3) and list(lab) == [1, 1, 1, 1, 0, 0, 0, -1, -1]
    lab, taken = to.sample(np.asarray([0, -1, -1, -1, -1], dtype=np.int32), np.asarray([4, 3, 2, 1, 0]), batch_size=4, positive_fraction=0.5)
    assert taken == (1, 3) and list(lab) == [1, -1, 0, 0, 0]
    # equal keys are broken by the anchor index; floor(bs * frac)
    lab, taken = to.sample(np.asarray([-1, 0, 0, 0, -1, -1], dtype=np.int32), np.zeros(6, dtype=np.int32), batch_size=3, positive_fraction=0.5)
    assert taken == (1, 2) and list(lab) == [0, 1, -1, -1, 0, -1]
    assert to.sample(np.zeros(300, dtype=np.int32), np.arange(300), 256, 0.5)[1] == (128, 0)


def test_oracle_losses_and_gradients_against_float64_autograd():
    rng = np.random.RandomState(0)
    B, N, beta = 2, 500, 1.0 / 9.0
    logits = rng.normal(0, 3, size=(B, N))
    logits[0, :4] = [80.0, -80.0, 0.0, -0.0]
    deltas, reg = rng.normal(0, 0.3, size=(B, N, 4)), rng.normal(0, 0.3, size=(B, N, 4))
    deltas[0, 0] = reg[0, 0] + [0.0, beta, -beta, 0.5 * beta]                          # the kink and the origin of smooth-L1
    labels = rng.choice([-1, 0, 1], size=(B, N), p=[0.5, 0.3, 0.2]).astype(np.int32)
    labels[0, :4] = [0, 1, 1, 0]
    got, dl, dd = to.loss(logits, deltas, labels, reg, beta)
    x = torch.from_numpy(logits).requires_grad_(True)
    d = torch.from_numpy(deltas).requires_grad_(True)
    lab = torch.from_numpy(labels)
    used, pos = lab >= 0, lab == 1
    obj = F.binary_cross_entropy_with_logits(x[used], pos[used].double())
    box = F.smooth_l1_loss(d[pos], torch.from_numpy(reg)[pos], beta=beta, reduction="sum") / used.sum()
    (obj + box).backward()
    np.testing.assert_allclose(got, [obj.item(), box.item()], rtol=1e-12)
    np.testing.assert_allclose(dl, x.grad.numpy(), rtol=1e-10, atol=1e-18)
    np.testing.assert_allclose(dd, d.grad.numpy(), rtol=1e-10, atol=1e-18)
    assert not dl[~used.numpy()].any() and not dd[~pos.numpy()].any() and np.isfinite(got).all()
    # no positive: the box loss is exactly zero; nothing sampled at all: zeros, not NaN
    got, _, dd = to.loss(logits, deltas, np.where(labels == 1, -1, labels), reg, beta)
    assert got[1] == 0.0 and not dd.any() and got[0] > 0
    got, dl, dd = to.loss(logits, deltas, np.full_like(labels, -1), reg, beta)
    assert not got.any() and not dl.any() and not dd.any()


def test_scenes_make_the_fp32_iou_exact_up_to_its_division():
    """The reference's anchors are integers in [-362, 530]; the scenes' GT boxes sit on the quarter-pixel grid inside the image.
    Then intersections and area sums are exact in fp32 and the fp32 quotient is the correctly rounded float64 one - which is what
    lets the GPU tests demand EQUAL labels.  Also pins what the 224 x 224 scenes exercise."""
    anchors = _reference_anchors()
    assert anchors.shape == (12543, 4) and anchors.min() == -362 and anchors.max() == 530 and np.all(anchors == np.round(anchors))
    counts = {}
    for g in (1, 7, 40):
        gt = to.scene(g, g)
        assert gt.shape == (g, 4) and np.all(gt * 4 == np.round(gt * 4)) and gt.min() >= 0 and gt.max() <= 224
        assert np.all(gt[:, 2:] - gt[:, :2] >= 4)
        a, q = anchors.astype(np.float64), gt.astype(np.float64)
        iw = np.maximum(np.minimum(a[None, :, 2], q[:, None, 2]) - np.maximum(a[None, :, 0], q[:, None, 0]), 0)
        ih = np.maximum(np.minimum(a[None, :, 3], q[:, None, 3]) - np.maximum(a[None, :, 1], q[:, None, 1]), 0)
        inter = iw * ih
        area_sum = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[None, :] + ((q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]))[:, None]
        assert np.all(inter == inter.astype(f)) and np.all(area_sum == area_sum.astype(f)) and np.all((area_sum - inter) == (area_sum - inter).astype(f))
        m, iou = to.match(anchors, gt)
        np.testing.assert_array_equal(iou, (inter / (area_sum - inter)).astype(f))
        best = iou.max(axis=0)
        by_thr = int((best >= f(0.7)).sum())
        counts[g] = (by_thr, int((m >= 0).sum()) - by_thr, int((m == -2).sum()), int((m == -1).sum()))
        assert sum(counts[g]) == 12543
    # G = 1 and G = 7: no anchor reaches 0.7, promotion is the only source of positives.  G = 40: every branch, and more positives
    # than the sampler's quota of 128
    assert counts[1][0] == 0 and counts[1][1] > 0 and counts[7][0] == 0 and counts[7][1] > 0
    assert counts[40] == (16, 591, 2212, 9724)


def test_modules_have_the_new_surface_and_keep_their_refusals():
    gen = AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)
    rpn = RegionProposalNetwork(gen, RPNHead(256, 3))
    assert (rpn.pre_nms_top_n, rpn.post_nms_top_n, rpn.nms_thresh, rpn.score_thresh, rpn.min_size) == (1000, 1000, 0.7, 0.0, 1e-3)
    assert (rpn.pre_nms_top_n_train, rpn.post_nms_top_n_train, rpn.fg_iou_thresh, rpn.bg_iou_thresh, rpn.batch_size_per_image,
            rpn.positive_fraction) == (2000, 2000, 0.7, 0.3, 256, 0.5)
    rpn = RegionProposalNetwork(gen, RPNHead(256, 3), 1000, 1000, 0.7, 0.0, 1e-3, 500, 300, 0.6, 0.2, 64, 0.25)   # after the existing ones
    assert (rpn.pre_nms_top_n_train, rpn.post_nms_top_n_train, rpn.fg_iou_thresh, rpn.bg_iou_thresh, rpn.batch_size_per_image,
            rpn.positive_fraction) == (500, 300, 0.6, 0.2, 64, 0.25)
    with pytest.raises(RuntimeError, match="inference only"):                                     # train mode without targets
        rpn.train()([torch.zeros(1, 256, 4, 4)], (224, 224))
    with pytest.raises(ValueError, match="GPU"):                                                  # with targets: no CPU path
        rpn.train()([torch.zeros(1, 256, 4, 4)], (224, 224), targets=[{"boxes": torch.zeros(0, 4)}])
    # the padded form of the reference's target list
    gt, cnt = RegionProposalNetwork.pad_targets([{"boxes": torch.tensor([[1.0, 2.0, 3.0, 4.0]])}, {"boxes": torch.zeros(0, 4)}], "cpu")
    assert tuple(gt.shape) == (2, 1, 4) and gt.dtype == torch.float32 and cnt.dtype == torch.int32 and cnt.tolist() == [1, 0]
    assert gt[0, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
    same = RegionProposalNetwork.pad_targets((gt, cnt), "cpu")
    assert torch.equal(same[0], gt) and torch.equal(same[1], cnt)
    model = LayoutDetectionModel(config=cfgs.vit_micro())
    with pytest.raises(RuntimeError, match="inference only"):                                     # the box head's losses do not exist
        model.train()([torch.zeros(3, 32, 32)], [{"boxes": torch.zeros(0, 4)}])
    with pytest.raises(RuntimeError, match="train"):
        model.eval().rpn_losses([torch.zeros(3, 32, 32)], [{"boxes": torch.zeros(0, 4)}])
