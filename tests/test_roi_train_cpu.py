"""CPU-only checks of the box head's training side: the C ABI declares, exports and validates the new entry points without a device;
the numpy oracle (tests/roi_train_oracle.py) passes hand-computed cases of the matcher and the sampler; its losses agree with float64
torch autograd of F.cross_entropy + F.smooth_l1_loss and its RoIAlign backward with autograd through the F.grid_sample restatement of
the forward; the fc6 gradient's column permutation is torchvision's flatten; the modules have the new constructor arguments and keep
their refusals.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from layoutdit_amd import _lib, ops
from layoutdit_amd import config as cfgs
from layoutdit_amd.modeling import FastRCNNPredictor, LayoutDetectionModel, MultiScaleRoIAlign, RoIHeads, TwoMLPHead
from tests import roi_oracle as ro
from tests import roi_train_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_roi_targets_f32", "ldit_roi_align_levels_bwd_f32", "ldit_box_loss_f32", "ldit_box_loss_workspace_bytes")
f = np.float32


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    w = (C.c_float * 4)(10, 10, 5, 5)

    def targets(props=16, cnt=16, gt=16, gtl=16, gtc=16, keys=16, B=2, R=1000, G=8, fg=0.5, bg=0.5, bs=512, frac=0.25, wts=w, rois=16, lab=16,
                reg=16, mat=16, smp=16):
        return lib.ldit_roi_targets_f32(props, cnt, gt, gtl, gtc, keys, B, R, G, fg, bg, bs, frac, wts, rois, lab, reg, mat, smp, None)

    for name in ("props", "cnt", "gt", "gtl", "gtc", "keys", "rois", "lab", "reg", "mat", "smp"):
        assert targets(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
        assert targets(**{name: 8}) == _lib.LDIT_EINVAL and "aligned" in err(), name
    assert targets(wts=None) == _lib.LDIT_EINVAL
    assert targets(B=0) == _lib.LDIT_EINVAL and targets(R=0) == _lib.LDIT_EINVAL and targets(G=0) == _lib.LDIT_EINVAL
    assert targets(fg=0.3, bg=0.7) == _lib.LDIT_EINVAL and "bg" in err()
    assert targets(fg=float("nan")) == _lib.LDIT_EINVAL
    assert targets(bs=0) == _lib.LDIT_EINVAL and "batch_size" in err()
    for frac in (0.0, -0.5, 1.5, float("nan")):
        assert targets(frac=frac) == _lib.LDIT_EINVAL and "positive_fraction" in err(), frac
    assert targets(wts=(C.c_float * 4)(10, 0, 5, 5)) == _lib.LDIT_EINVAL and "weights" in err()
    assert targets(R=4089, G=8) == _lib.LDIT_EUNSUPPORTED and "4096" in err()         # R + Gmax = 4097
    assert targets(R=2000, G=2097) == _lib.LDIT_EUNSUPPORTED

    L = 2
    maps, mh, mw = (C.c_void_p * L)(16, 32), (C.c_int32 * L)(8, 4), (C.c_int32 * L)(8, 4)
    sc = (C.c_float * L)(0.25, 0.125)
    sb, sy, sx = (C.c_int64 * L)(8 * 8 * 8, 4 * 4 * 8), (C.c_int64 * L)(64, 32), (C.c_int64 * L)(8, 8)

    def bwd(d_out=16, boxes=16, cnt=None, lv=16, B=2, S=5, maps=maps, mh=mh, sc=sc, sx=sx, L=L, Cc=8, P=7, sr=2):
        return lib.ldit_roi_align_levels_bwd_f32(d_out, boxes, cnt, lv, B, S, maps, mh, mw, sc, sb, sy, sx, L, Cc, P, sr, None)

    for name in ("d_out", "boxes", "lv", "maps"):
        assert bwd(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
    for name in ("d_out", "boxes", "lv", "cnt"):
        assert bwd(**{name: 8}) == _lib.LDIT_EINVAL and "aligned" in err(), name
    assert bwd(B=0) == _lib.LDIT_EINVAL and bwd(S=0) == _lib.LDIT_EINVAL and bwd(L=0) == _lib.LDIT_EINVAL
    assert bwd(L=9) == _lib.LDIT_EUNSUPPORTED and bwd(Cc=6) == _lib.LDIT_EUNSUPPORTED and "multiple of 4" in err()
    assert bwd(P=14) == _lib.LDIT_EUNSUPPORTED and bwd(sr=4) == _lib.LDIT_EUNSUPPORTED and "7 / 2" in err()
    assert bwd(maps=(C.c_void_p * L)(16, None)) == _lib.LDIT_EINVAL and "map 1" in err()
    assert bwd(maps=(C.c_void_p * L)(16, 8)) == _lib.LDIT_EINVAL
    assert bwd(mh=(C.c_int32 * L)(8, 0)) == _lib.LDIT_EINVAL and bwd(sc=(C.c_float * L)(0.25, 0.0)) == _lib.LDIT_EINVAL
    assert bwd(sx=(C.c_int64 * L)(8, 4)) == _lib.LDIT_EINVAL                            # pixel stride shorter than C

    def loss(head=16, ld=32, labels=16, reg=16, smp=16, B=2, M=1024, NC=6, beta=1 / 9, out=16, dh=16, ws=16, nbytes=1 << 20):
        return lib.ldit_box_loss_f32(head, ld, labels, reg, smp, B, M, NC, beta, out, dh, ws, nbytes, None)

    for name in ("head", "labels", "reg", "smp", "out", "dh"):
        assert loss(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
        assert loss(**{name: 8}) == _lib.LDIT_EINVAL and "aligned" in err(), name
    assert loss(B=0) == _lib.LDIT_EINVAL and loss(M=0) == _lib.LDIT_EINVAL and loss(NC=1) == _lib.LDIT_EINVAL
    assert loss(ld=29) == _lib.LDIT_EINVAL and "stride" in err()
    assert loss(beta=-1.0) == _lib.LDIT_EINVAL and loss(beta=float("nan")) == _lib.LDIT_EINVAL and "beta" in err()
    need = lib.ldit_box_loss_workspace_bytes(1024)
    assert need > 0 and need % 16 == 0 and lib.ldit_box_loss_workspace_bytes(0) == 0
    assert loss(nbytes=need - 1) == _lib.LDIT_EWORKSPACE and loss(ws=None, nbytes=need) == _lib.LDIT_EWORKSPACE
    assert loss(ws=8, nbytes=need) == _lib.LDIT_EINVAL


def test_front_ends_refuse_cpu_tensors_and_bad_settings():
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                               # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        ops.roi_targets(torch.zeros(1, 8, 4), i32(1), torch.zeros(1, 2, 4), i32(1, 2), i32(1), i32(1, 10))
    with pytest.raises(ValueError, match="GPU"):
        ops.box_loss(torch.zeros(8, 32), i32(1, 8), torch.zeros(1, 8, 4), i32(1, 2), 6)
    with pytest.raises(ValueError, match="GPU"):
        ops.roi_align_levels_bwd(torch.zeros(8, 7, 7, 4), torch.zeros(1, 8, 4), None, i32(1, 8), [(4, 4)], (16, 16))
    assert ops.ROI_TARGETS_MAX_CANDIDATES == 4096


def _one(props, gt, labels, keys, **kw):
    props = np.asarray(props, dtype=f).reshape(-1, 4)
    return bo.targets_image(props, len(props), np.asarray(gt, dtype=f).reshape(-1, 4), np.asarray(labels), np.asarray(keys), **kw)


def test_oracle_matcher_hand_cases():
    gt = [[0, 0, 10, 10], [50, 50, 60, 60]]
    # a proposal equal to a GT: positive, zero targets; IoU exactly 1 / 2 is positive at (0.5, 0.5); disjoint: background
    props = [[0, 0, 10, 10], [0, 0, 10, 5], [0, 0, 10, 4.75], [100, 100, 110, 110]]
    rois, lab, reg, mat, taken = _one(props, gt, [3, 4], np.arange(6), batch_size=8, positive_fraction=0.5)
    assert taken == (4, 2)                                                            # proposals 0, 1 and BOTH GT rows are positives
    assert list(lab) == [3, 3, 3, 4, 0, 0, -1, -1] and list(mat) == [0, 0, 0, 1, -1, -1, -1, -1]
    np.testing.assert_array_equal(rois[:6], np.asarray([props[0], props[1], gt[0], gt[1], props[2], props[3]], dtype=f))
    assert not reg[0].any() and not reg[2:].any() and not rois[6:].any()              # equal boxes, GT rows, negatives, padding
    np.testing.assert_allclose(reg[1], [0, 10 * (5 - 2.5) / 5, 0, 5 * np.log(2.0)], rtol=1e-15)
    # between the thresholds: ignored, never sampled
    _, lab, _, _, taken = _one(props, gt, [3, 4], np.arange(6), batch_size=8, positive_fraction=0.5, fg_thr=0.6, bg_thr=0.4)
    assert taken == (3, 1) and list(lab[:4]) == [3, 3, 4, 0]                          # 0.5 and 0.475 fall between
    # duplicate GTs go to the lowest index
    _, lab, _, mat, _ = _one([[0, 0, 10, 10]], [[50, 50, 60, 60], [0, 0, 10, 10], [0, 0, 10, 10]], [1, 2, 5], np.zeros(4), batch_size=4, positive_fraction=1.0)
    assert list(mat) == [1, 0, 1, 1] and list(lab) == [2, 1, 2, 2]                    # the third GT row matches the second
    # gt_count 0: every proposal background, and the padded batch form cuts rows past the counts off before looking at them
    rois, lab, reg, mat, taken = _one(props, np.zeros((0, 4)), [], np.arange(4)[::-1], batch_size=3)
    assert taken == (0, 3) and list(lab) == [0, 0, 0] and not reg.any()
    np.testing.assert_array_equal(rois, np.asarray(props, dtype=f)[[3, 2, 1]])        # (key, index) order
    pb = np.full((2, 4, 4), np.nan, dtype=f)
    pb[0, :2], pb[1, :1] = props[:2], props[3:]
    gb = np.full((2, 2, 4), np.nan, dtype=f)
    gb[0] = gt
    out = bo.targets(pb, [2, 1], gb, np.asarray([[3, 4], [-7, -7]]), [2, 0], np.zeros((2, 6), dtype=np.int32), batch_size=4)
    assert np.isfinite(out[0]).all() and np.isfinite(out[2]).all()
    assert out[4].tolist() == [[1, 0], [0, 1]] and out[1].tolist() == [[3, -1, -1, -1], [0, -1, -1, -1]]      # quota floor(4 * 0.25) = 1


def test_oracle_sampler_hand_cases():
    # 128 positives at (512, 0.25), GT rows always among the candidates, fewer negatives than the quota
    gt = [[0, 0, 100, 100]]
    props = [[0, 0, 100, 100 - 0.25 * i] for i in range(200)] + [[150, 150, 160, 160]] * 10
    keys = np.arange(211)[::-1].copy()
    rois, lab, _, _, taken = _one(props, gt, [2], keys)
    assert taken == (128, 10) and (lab[:128] == 2).all() and (lab[128:138] == 0).all() and (lab[138:] == -1).all()
    np.testing.assert_array_equal(rois[0], np.asarray(gt[0], dtype=f))                # the GT row has the smallest key here
    # equal keys: the candidate index breaks the tie; the GT row's index is R + g, after every proposal
    rois, lab, _, _, taken = _one(props, gt, [2], np.zeros(211), batch_size=8)
    assert taken == (2, 6)
    np.testing.assert_array_equal(rois[:2], np.asarray(props[:2], dtype=f))
    _, _, _, _, taken = _one(props[:3], gt, [2], np.zeros(4), batch_size=512)
    assert taken == (4, 0)                                                            # the GT row is always a positive


def test_oracle_losses_against_float64_autograd():
    rng = np.random.RandomState(0)
    M, NC, ld, beta = 300, 6, 32, 1.0 / 9.0
    head = rng.normal(0, 2, size=(M, ld))
    head[:4, :NC] = [[80, -80, 0, 0, 0, 0], [-80, 80, 80, 0, 0, 0], [0] * 6, [80] * 6]
    labels = rng.choice([-1, 0, 1, 2, 3, 4, 5], size=M, p=[0.3, 0.4, 0.06, 0.06, 0.06, 0.06, 0.06]).astype(np.int32)
    labels[:4] = [1, 0, 3, 5]
    reg = rng.normal(0, 0.3, size=(M, 4))
    head[0, NC + 4:NC + 8] = reg[0] + [0.0, beta, -beta, 0.5 * beta]                  # the kink and the origin of smooth-L1
    got, d = bo.loss(head, labels, reg, NC, beta)
    x = torch.from_numpy(head).requires_grad_(True)
    lab = torch.from_numpy(labels).long()
    used, pos = lab >= 0, lab >= 1
    cls = F.cross_entropy(x[used][:, :NC], lab[used])
    deltas = x[:, NC:5 * NC].reshape(M, NC, 4)
    box = F.smooth_l1_loss(deltas[pos, lab[pos]], torch.from_numpy(reg)[pos], beta=beta, reduction="sum") / used.sum()
    g_cls, = torch.autograd.grad(cls, x, retain_graph=True)
    g_box, = torch.autograd.grad(box, x)
    np.testing.assert_allclose(got, [cls.item(), box.item()], rtol=1e-12)
    np.testing.assert_allclose(d[:, :NC], g_cls.numpy()[:, :NC], rtol=1e-10, atol=1e-18)
    np.testing.assert_allclose(d[:, NC:], g_box.numpy()[:, NC:], rtol=1e-10, atol=1e-18)
    assert not g_cls.numpy()[:, NC:].any() and not g_box.numpy()[:, :NC].any() and not d[:, 5 * NC:].any() and not d[labels < 0].any()
    got, d = bo.loss(head, np.where(labels >= 1, 0, labels), reg, NC, beta)           # no positive: exactly zero
    assert got[1] == 0.0 and not d[:, NC:].any() and got[0] > 0
    got, d = bo.loss(head, np.full_like(labels, -1), reg, NC, beta)                   # nothing sampled: zeros, not NaN
    assert not got.any() and not d.any()


def _grid_sample_forward(fmap, box, scale, P=7, S=2):
    """tests/test_roi_cpu.py's independent restatement of the forward, differentiable: F.grid_sample(align_corners=True) evaluates the
    bilinear surface at pixel coordinates; valid where every sample lies in [0, h - 1] x [0, w - 1]."""
    h, w, _ = fmap.shape
    ys, xs = ro.sample_coords(box[1], box[3], scale, P, S), ro.sample_coords(box[0], box[2], scale, P, S)
    gy, gx = np.meshgrid(2 * ys / (h - 1) - 1, 2 * xs / (w - 1) - 1, indexing="ij")
    grid = torch.from_numpy(np.stack([gx, gy], axis=-1))[None]
    val = F.grid_sample(fmap.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
    return val.reshape(-1, P, S, P, S).mean(dim=(2, 4)).permute(1, 2, 0), (ys.min() >= 0 and ys.max() <= h - 1 and xs.min() >= 0
                                                                              and xs.max() <= w - 1)


def test_oracle_roi_align_backward_against_autograd_through_grid_sample():
    sizes, img, Cc = [(56, 56), (28, 28), (14, 14), (7, 7), (4, 4)], (224, 224), 3
    boxes, _ = ro.make_boxes(4, 60, img, sizes)
    scales = ro.infer_scales(sizes, img)
    lv = ro.box_levels(boxes, 2, 6)
    rng = np.random.RandomState(1)
    d_out = rng.normal(0, 1, size=(60, 7, 7, Cc))
    keep = []
    maps = [torch.zeros(h, w, Cc, dtype=torch.float64, requires_grad=True) for h, w in sizes]
    total = 0
    for r, (bx, l) in enumerate(zip(boxes.astype(np.float64), lv)):
        out, interior = _grid_sample_forward(maps[l], bx, scales[l])
        if interior:
            keep.append(r)
            total = total + (out * torch.from_numpy(d_out[r])).sum()
    assert len(keep) >= 30
    total.backward()
    sel = np.zeros(60, dtype=bool)
    sel[keep] = True
    levels = np.where(sel, lv, -1)[None]                                              # the other rows contribute nothing
    grads, touch = bo.roi_align_levels_bwd(d_out, boxes[None], None, levels, sizes, img)
    for g, s, m in zip(grads, touch, maps):
        np.testing.assert_allclose(g[0], np.zeros_like(g[0]) if m.grad is None else m.grad.numpy(), rtol=0, atol=1e-12)
        assert not g[0][s[0] == 0].any() and (s[0] >= 0).all()
    assert sum(int(s.sum()) for s in touch) > 0
    # hand case: one box clamped to a single cell of a 4 x 4 map puts all 49 bins' gradient on that cell, s = the 196 samples
    g, s = bo.roi_align_levels_bwd(np.ones((1, 7, 7, 1)), np.asarray([[[192.0, 192.0, 193.0, 193.0]]], dtype=f), None, [[0]], [(4, 4)], (256, 256))
    assert g[0][0, 3, 3, 0] == pytest.approx(49.0) and g[0].sum() == pytest.approx(49.0) and s[0][0, 3, 3] == 196 and s[0].sum() == 196
    # the float32 evaluation of the same definition stays inside the GPU tests' gate
    g32, _ = bo.roi_align_levels_bwd(d_out, boxes[None], None, levels, sizes, img, dtype=np.float32)
    for a, b, s in zip(g32, grads, touch):
        assert (np.abs(a.astype(np.float64) - b).max(axis=-1) <= 2.0 ** -15 * np.abs(d_out).max() * s).all()


def test_fc6_gradient_permutation_is_torchvisions_flatten():
    """The weight gradient computed on (ph, pw, c) rows and permuted back equals autograd of a CPU linear on torchvision's
    flatten(start_dim=1) of the (c, ph, pw) tensor."""
    torch.manual_seed(0)
    M, Cc, out = 5, 4, 6
    pooled = torch.randn(M, 7, 7, Cc, dtype=torch.float64)
    w = torch.randn(out, Cc * 49, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(M, out, dtype=torch.float64)
    (F.linear(pooled.permute(0, 3, 1, 2).flatten(1), w) * dy).sum().backward()
    g_hwc = dy.t() @ pooled.reshape(M, -1)                                            # what the wgrad GEMM returns
    back = g_hwc.view(out, 7, 7, Cc).permute(0, 3, 1, 2).reshape(out, -1)             # modeling/roi_heads.py's permutation
    torch.testing.assert_close(back, w.grad, rtol=1e-13, atol=1e-13)
    head = TwoMLPHead(Cc * 49, out)
    torch.testing.assert_close(F.linear(pooled.float().reshape(M, -1), head.fc6_weight_hwc(Cc, 7, 7)),
                               F.linear(pooled.float().permute(0, 3, 1, 2).flatten(1), head.fc6.weight), rtol=1e-5, atol=1e-5)


def test_modules_have_the_new_surface_and_keep_their_refusals():
    pool = MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)
    rh = RoIHeads(pool, TwoMLPHead(256 * 49, 1024), FastRCNNPredictor(1024, 6))
    assert (rh.fg_iou_thresh, rh.bg_iou_thresh, rh.batch_size_per_image, rh.positive_fraction, rh.smooth_l1_beta) == (0.5, 0.5, 512, 0.25, 1 / 9)
    rh2 = RoIHeads(pool, TwoMLPHead(256 * 49, 1024), FastRCNNPredictor(1024, 6), None, 0.05, 0.5, 100, 1e-2, 0.6, 0.4, 64, 0.5)   # after the existing ones
    assert (rh2.fg_iou_thresh, rh2.bg_iou_thresh, rh2.batch_size_per_image, rh2.positive_fraction) == (0.6, 0.4, 64, 0.5)
    with pytest.raises(RuntimeError, match="inference only"):                                     # train mode without targets
        rh.train()([torch.zeros(1, 256, 4, 4)], torch.zeros(1, 3, 4), None, (224, 224))
    with pytest.raises(ValueError, match="GPU"):                                                  # with targets: no CPU path
        rh.train()([torch.zeros(1, 256, 4, 4)], torch.zeros(1, 3, 4), None, (224, 224),
                   targets=[{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}])
    gt, lab, cnt = RoIHeads.pad_targets([{"boxes": torch.tensor([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 9.0, 9.0]]), "labels": torch.tensor([3, 1])},
                                         {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}], "cpu")
    assert tuple(gt.shape) == (2, 2, 4) and gt.dtype == torch.float32 and lab.dtype == torch.int32 and cnt.dtype == torch.int32
    assert cnt.tolist() == [2, 0] and lab.tolist() == [[3, 1], [0, 0]] and gt[0, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
    same = RoIHeads.pad_targets((gt, lab, cnt), "cpu")
    assert all(torch.equal(a, b) for a, b in zip(same, (gt, lab, cnt)))
    with pytest.raises(ValueError, match="labels"):
        RoIHeads.pad_targets([{"boxes": torch.zeros(2, 4), "labels": torch.zeros(3, dtype=torch.int64)}], "cpu")
    model = LayoutDetectionModel(config=cfgs.vit_micro())
    assert model.model.roi_heads.batch_size_per_image == 512
    tg = [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}]
    with pytest.raises(RuntimeError, match="inference only"):                                     # forward keeps torchvision's eval surface
        model.train()([torch.zeros(3, 32, 32)], tg)
    with pytest.raises(RuntimeError, match="inference only"):
        model.train().forward_padded(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match="train"):
        model.eval().losses([torch.zeros(3, 32, 32)], tg)
    with pytest.raises(ValueError, match="targets"):
        model.train().losses([torch.zeros(3, 32, 32)], None)
