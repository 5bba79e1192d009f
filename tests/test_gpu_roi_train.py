"""The box head's training side on the GPU (csrc/roi_train.hip through the C ABI, modeling/roi_heads.py, modeling/detector.py) against
the numpy oracle tests/roi_train_oracle.py.  Gates: labels, matches, sampler counts, row order and rois EXACTLY
(the oracle's IoU is float32 in the kernel's order of operations); regression targets within 8 * 2^-23 * max(|t|, w), w the
coordinate's coder weight (the RPN's gate scaled by the weight: a target is w times that encoding); losses and d_head within the
project's fp32 gate 2e-5 of float64; the RoIAlign backward element-wise within 2^-15 * max|d_out| * s(e) and exactly 0 where s(e) == 0
(s(e) = the (row, sample) pairs touching the element: a bilinear weight is off by at most ~2^-16, a sample carries two of them and
1 / 4; the factor leaves 4x for the summation), and adjoint to the device's own forward to 1e-5; the heads' backward against float64
autograd (inputs and biases 2e-5, weights 3e-2: bf16-operand GEMMs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import ops, synth                  # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import FastRCNNPredictor, LayoutDetectionModel, MultiScaleRoIAlign, RoIHeads, TwoMLPHead    # noqa: E402
from tests import roi_oracle as ro                    # noqa: E402
from tests import roi_train_oracle as bo              # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402
from tests.util import rel_l2                         # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
NC = 6
W = np.asarray(bo.WEIGHTS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _map_sizes(size):
    h, w = size
    return [(h // 4, w // 4), (h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32), ((h // 32 + 1) // 2, (w // 32 + 1) // 2)]


# ---- proposal targets ----------------------------------------------------------------------------------------------------------
def target_problem(R, gts, size=(224, 224)):
    """B = 2 images with gts = (G0, G1) GT boxes (rows past the count NaN, their labels garbage) and R proposals each: about half
    are jittered copies of GT boxes (positives, and more than the sampler's quota at R = 2000), the rest random; proposal 0 of image
    1 IS a GT box, proposal 1 overlaps it by exactly one half.  count = (R, R // 2), rows past it NaN.  Keys: full-range for image 0,
    three bits for image 1 (ties by index)."""
    rng = np.random.RandomState(1000 * R + 10 * gts[0] + gts[1])
    h, w = size
    gt_list = [to.scene(40 + g, g, size) for g in gts]
    gt_boxes, gt_count = to.pad_gt(gt_list)
    gmax = gt_boxes.shape[1]
    gt_labels = np.full((2, gmax), -12345, dtype=np.int32)
    for b, g in enumerate(gts):
        gt_labels[b, :g] = rng.randint(1, NC, size=g)
    props = np.empty((2, R, 4), dtype=np.float32)
    for b, gt in enumerate(gt_list):
        wh = np.exp(rng.uniform(np.log(6.0), np.log(0.7 * min(h, w)), size=(R, 2)))
        xy = rng.uniform(0, 1, size=(R, 2)) * (np.asarray([w, h]) - wh)
        bx = np.concatenate([xy, xy + wh], axis=1)
        if len(gt):
            pick = rng.rand(R) < 0.55
            src = gt[rng.randint(0, len(gt), size=R)].astype(np.float64)
            sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
            jit = src + rng.uniform(-0.22, 0.22, size=(R, 4)) * np.stack([sw, sh, sw, sh], axis=1)
            bx[pick] = jit[pick]
        props[b] = np.round(bx * 4.0) / 4.0
    if gts[1] and R >= 2:
        g = gt_list[1][0]
        props[1, 0] = g
        props[1, 1] = [g[0], g[1], g[0] + 0.5 * (g[2] - g[0]), g[3]]           # IoU exactly 1 / 2: positive at fg_thr = 0.5
    count = np.asarray([R, R // 2], dtype=np.int32)
    props[1, R // 2:] = np.nan
    keys = rng.randint(0, 2 ** 31 - 1, size=(2, R + gmax)).astype(np.int32)
    keys[1] = rng.randint(0, 8, size=R + gmax)
    return props, count, gt_boxes, gt_labels, gt_count, keys


@pytest.mark.parametrize("thresholds", [(0.5, 0.5), (0.6, 0.4)])
@pytest.mark.parametrize("sampler", [(512, 0.25), (16, 0.25)])
@pytest.mark.parametrize("gts", [(0, 7), (1, 40)])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 2000])
def test_targets_equal_the_oracle(R, gts, sampler, thresholds):
    props, count, gt_boxes, gt_labels, gt_count, keys = target_problem(R, gts)
    (S, frac), (fg, bg) = sampler, thresholds
    ref = bo.targets(props, count, gt_boxes, gt_labels, gt_count, keys, fg, bg, S, frac)
    args = (_dev(props), _dev(count), _dev(gt_boxes), _dev(gt_labels), _dev(gt_count), _dev(keys), fg, bg, S, frac)
    got = ops.roi_targets(*args)
    again = ops.roi_targets(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                      # bit-identical
    rois, lab, reg, mat, smp = (t.cpu().numpy() for t in got)
    ref_rois, ref_lab, ref_reg, ref_mat, ref_smp = ref
    np.testing.assert_array_equal(smp, ref_smp)
    np.testing.assert_array_equal(lab, ref_lab)
    np.testing.assert_array_equal(mat, ref_mat)
    assert rois.tobytes() == ref_rois.tobytes()                                    # the chosen candidates, bit for bit, in row order
    assert np.isfinite(reg).all() and np.isfinite(rois).all()
    bound = 8 * EPS * np.maximum(np.abs(ref_reg), W[None, None, :])
    err = np.abs(reg.astype(np.float64) - ref_reg)
    print(f"R={R} gts={gts}: sampled {smp.tolist()}, reg_targets max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert not reg[lab < 1].any() and (mat[lab < 1] == -1).all()                   # exactly zero where the row is no positive
    for b in range(2):
        p, q = smp[b]
        assert (lab[b, :p] >= 1).all() and (lab[b, p:p + q] == 0).all() and (lab[b, p + q:] == -1).all() and not rois[b, p + q:].any()
        if gts[b] == 0:
            assert p == 0 and q == min(S, int(count[b]))                           # the image without GT: all background
    if R == 2000 and gts == (1, 40):
        assert smp[1, 0] == int(S * frac) and smp[1].sum() <= S                    # the positive cap
        assert smp[1].sum() == S or (fg, bg) == (0.6, 0.4)                         # (with an ignored class the negatives can run short)
        assert smp[0, 0] > 0


# ---- losses --------------------------------------------------------------------------------------------------------------------
def _check_loss(head, lab, reg, smp):
    loss, dh = ops.box_loss(_dev(head), lab, reg, smp, NC)
    loss2, dh2 = ops.box_loss(_dev(head), lab, reg, smp, NC)
    assert torch.equal(loss, loss2) and torch.equal(dh, dh2)
    lab_h = lab.cpu().numpy().reshape(-1)
    ref, ref_d = bo.loss(head, lab_h, reg.cpu().numpy(), NC)
    loss, dh = loss.cpu().numpy().astype(np.float64), dh.cpu().numpy()
    assert int(smp.sum()) == int((lab_h >= 0).sum())                                # the normaliser the kernel reads
    for got, want in zip(loss, ref):
        print(f"loss {got:.9g} vs {want:.9g}")
        assert abs(got - want) <= 2e-5 * abs(want)
    assert rel_l2(dh[:, :NC], ref_d[:, :NC]) < 2e-5
    if (lab_h >= 1).any():
        assert rel_l2(dh[:, NC:], ref_d[:, NC:]) < 2e-5
    assert not dh[ref_d == 0].any()                                                 # padding rows / columns, other classes: exactly zero
    assert not dh[lab_h < 0].any() and not dh[:, 5 * NC:].any()
    return loss


@pytest.mark.parametrize("S", [16, 512])
def test_losses_and_gradients_match_the_float64_oracle(S):
    props, count, gt_boxes, gt_labels, gt_count, keys = target_problem(2000, (0, 40))
    _, lab, reg, _, smp = ops.roi_targets(_dev(props), _dev(count), _dev(gt_boxes), _dev(gt_labels), _dev(gt_count), _dev(keys), 0.5, 0.5, S, 0.25)
    M = 2 * S
    rng = np.random.RandomState(S)
    head = np.zeros((M, 32), dtype=np.float32)
    head[:, :NC] = rng.normal(0, 2.5, size=(M, NC))
    head[::7, 0], head[1::7, 3], head[2::7, :NC] = 80.0, -80.0, 80.0
    head[3::7, :NC] = [80, -80, 80, -80, 0, 0]
    head[:, NC:5 * NC] = rng.normal(0, 0.6, size=(M, 4 * NC))
    tgt, lab_h = reg.cpu().numpy().reshape(M, 4), lab.cpu().numpy().reshape(M)
    for r in np.flatnonzero(lab_h >= 1):                                           # both branches of smooth-L1 (beta 1/9) around the target
        head[r, NC + 4 * lab_h[r]:NC + 4 * lab_h[r] + 4] = tgt[r] + rng.normal(0, 0.12, size=4)
    head[:, 5 * NC:] = 7.0                                                          # padding columns are never read
    loss = _check_loss(head, lab, reg, smp)
    assert loss[0] > 0 and loss[1] > 0 and int(smp[1, 0]) == S // 4
    # a batch with no positive at all: the image without GT alone
    loss = _check_loss(head[:S], lab[:1].contiguous(), reg[:1].contiguous(), smp[:1].contiguous())
    assert loss[1] == 0.0 and loss[0] > 0


# ---- RoIAlign backward ---------------------------------------------------------------------------------------------------------
def _roi_boxes(S, size, flavour):
    sizes = _map_sizes(size)
    if flavour == "clustered":                                                     # many rows share the same few pixels
        rng = np.random.RandomState(S)
        c = np.asarray([0.4 * size[1], 0.5 * size[0]])
        wh = rng.uniform(6, 20, size=(2, S, 2))
        xy = c + rng.uniform(-3, 3, size=(2, S, 2))
        return np.concatenate([xy - wh / 2, xy + wh / 2], axis=2).astype(np.float32)
    return np.stack([ro.make_boxes(11 + b, S, size, sizes)[0] for b in range(2)])  # edges, one-cell boxes, boxes beyond the image


def _bwd_case(S, C, size, flavour="mixed", strided=False):
    sizes = _map_sizes(size)
    boxes = _roi_boxes(S, size, flavour)
    count = np.asarray([S, S // 2], dtype=np.int32)
    boxes[1, S // 2:] = np.nan
    rng = np.random.RandomState(S + C)
    d_out = rng.normal(0, 1, size=(2 * S, 7, 7, C)).astype(np.float32)
    maps = [rng.normal(0, 1, size=(2, h, w, C)).astype(np.float32) for h, w in sizes]
    feats = [_dev(m).permute(0, 3, 1, 2) for m in maps]
    out, levels = ops.roi_align_levels(feats, _dev(boxes), _dev(count), size, return_levels=True)
    bufs = None
    if strided:                                                                    # a batch stride that is not h w C, poisoned in between
        raw = [torch.full((2, h * w * C + 64), float("nan"), device=DEV) for h, w in sizes]
        bufs = [r[:, :h * w * C].view(2, h, w, C).permute(0, 3, 1, 2) for r, (h, w) in zip(raw, sizes)]
    args = (_dev(d_out), _dev(boxes), _dev(count), levels, sizes, size)
    grads = ops.roi_align_levels_bwd(*args, out=bufs)
    again = ops.roi_align_levels_bwd(*args)
    lv = levels.cpu().numpy()
    ref, touch = bo.roi_align_levels_bwd(d_out, boxes, count, lv, sizes, size)
    peak, worst = float(np.abs(d_out).max()), 0.0
    for l, (g, g2, r, s) in enumerate(zip(grads, again, ref, touch)):
        assert tuple(g.shape) == (2, C) + tuple(sizes[l]) and g.stride(1) == 1
        assert torch.equal(g, g2)                                                  # two runs (and two output layouts) bit-identical
        got = g.permute(0, 2, 3, 1).cpu().numpy()
        assert not got[s == 0].any(), f"level {l}: a gradient where no sample falls"
        err = np.abs(got.astype(np.float64) - r).max(axis=-1)
        bound = 2.0 ** -15 * peak * s
        worst = max(worst, float((err[s > 0] / bound[s > 0]).max()) if (s > 0).any() else 0.0)
        assert (err <= bound).all(), f"level {l}: {float((err / np.maximum(bound, 1e-300)).max()):.3f} x the gate"
    # the adjoint identity with the device's own forward, both sums in float64 on the host
    lhs = float((out.cpu().numpy().astype(np.float64) * d_out).sum())
    rhs = sum(float((m.astype(np.float64) * g.permute(0, 2, 3, 1).cpu().numpy()).sum()) for m, g in zip(maps, grads))
    print(f"S={S} C={C} {size} {flavour}: worst error / gate {worst:.4f}; <Ax, g> = {lhs:.9g}, <x, A'g> = {rhs:.9g}; levels used {sorted(set(lv[lv >= 0]))}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    if strided:
        assert all(torch.isnan(r[:, -64:]).all() for r in raw)                     # nothing written between the images
    return lv


@pytest.mark.parametrize("size", [(224, 224), (96, 160)])
@pytest.mark.parametrize("C", [12, 256])
@pytest.mark.parametrize("S", [1, 37, 130])
def test_roi_align_backward_matches_the_oracle_and_is_the_adjoint(S, C, size):
    lv = _bwd_case(S, C, size)
    if S == 130:
        assert 4 in lv and 0 in lv                                                 # the `pool` level has its own gradient


def test_roi_align_backward_clustered_boxes_and_strided_outputs():
    _bwd_case(130, 256, (224, 224), "clustered")
    _bwd_case(37, 12, (96, 160), "mixed", strided=True)


def test_roi_align_autograd_adds_the_pool_gradient_into_p5():
    """MultiScaleRoIAlign on maps that require gradients: `pool` is the view p5[:, :, ::2, ::2], its gradient arrives in p5."""
    size, S, C = (224, 224), 37, 12
    sizes = _map_sizes(size)
    rng = np.random.RandomState(3)
    leaves = [_dev(rng.normal(0, 1, size=(2, h, w, C)).astype(np.float32)).permute(0, 3, 1, 2).requires_grad_(True) for h, w in sizes[:4]]
    feats = dict(zip(["p2", "p3", "p4", "p5"], leaves))
    feats["pool"] = leaves[3][:, :, ::2, ::2]
    boxes, count = _dev(_roi_boxes(S, size, "mixed")), _dev(np.asarray([S, S], dtype=np.int32))
    pool = MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)
    out = pool(feats, boxes, count, size)
    g = _dev(rng.normal(0, 1, size=tuple(out.shape)).astype(np.float32))
    (out * g).sum().backward()
    _, levels = ops.roi_align_levels([f.detach() for f in feats.values()], boxes, count, size, return_levels=True)
    grads = ops.roi_align_levels_bwd(g, boxes, count, levels, sizes, size)
    for leaf, d in zip(leaves[:3], grads[:3]):
        assert torch.equal(leaf.grad, d)
    want = grads[3].clone()
    want[:, :, ::2, ::2] += grads[4]
    assert torch.equal(leaves[3].grad, want) and grads[4].abs().max() > 0


# ---- the heads' backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [74, 32])
def test_heads_backward_matches_float64_autograd(M):
    torch.manual_seed(M)
    Cc, rep = 32, 64                                                               # every GEMM depth a multiple of 32
    head, pred = TwoMLPHead(Cc * 49, rep).to(DEV).train(), FastRCNNPredictor(rep, NC).to(DEV).train()
    with torch.no_grad():
        for p in list(head.parameters()) + list(pred.parameters()):
            p.copy_(torch.randn_like(p) * (0.1 if p.dim() == 2 else 0.3))
    rng = np.random.RandomState(M)
    x = rng.normal(0, 1, size=(M, 7, 7, Cc)).astype(np.float32)
    gy = rng.normal(0, 1, size=(M, 5 * NC)).astype(np.float32)
    xd = _dev(x).requires_grad_(True)
    y = pred.forward_stacked(head(xd))
    assert y.requires_grad and y.shape[1] >= 5 * NC and not y[:, 5 * NC:].any()
    total = (y[:, :5 * NC] * _dev(gy)).sum()
    total.backward()
    # float64 CPU autograd of the F.linear restatement on torchvision's (c, ph, pw) flattening
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in list(head.named_parameters()) + list(pred.named_parameters())}
    xr = torch.from_numpy(x).double().requires_grad_(True)
    t = F.relu(F.linear(xr.permute(0, 3, 1, 2).flatten(1), ref["fc6.weight"], ref["fc6.bias"]))
    t = F.relu(F.linear(t, ref["fc7.weight"], ref["fc7.bias"]))
    yr = torch.cat([F.linear(t, ref["cls_score.weight"], ref["cls_score.bias"]), F.linear(t, ref["bbox_pred.weight"], ref["bbox_pred.bias"])], dim=1)
    rt = (yr * torch.from_numpy(gy).double()).sum()
    rt.backward()
    assert rel_l2(y[:, :5 * NC].detach().cpu().numpy(), yr.detach().numpy()) < 2e-5
    e = rel_l2(xd.grad.cpu().numpy(), xr.grad.numpy())
    print(f"M={M}: input gradient {e:.3e}")
    assert e < 2e-5
    for k, p in list(head.named_parameters()) + list(pred.named_parameters()):
        e = rel_l2(p.grad.cpu().numpy(), ref[k].grad.numpy())                      # fc6.weight in torchvision's column order
        print(f"{k}: {e:.3e}")
        assert e < (2e-5 if k.endswith("bias") else 3e-2), k


# ---- the stage and the model ---------------------------------------------------------------------------------------------------
SIZE = (96, 160)


def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _roi_heads(seed=5, spread=True):
    torch.manual_seed(seed)
    rh = RoIHeads(MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2), TwoMLPHead(256 * 49, 1024), FastRCNNPredictor(1024, NC))
    if spread:
        with torch.no_grad():
            for p in rh.box_predictor.parameters():
                p.mul_(4.0)
    return rh.to(DEV).train()


@pytest.fixture(scope="module")
def stage():
    """B = 2 at 96 x 160: synthetic channels-last maps of the five levels, 300 proposals per image (count 300 and 150), two images' GT
    in the reference's list form and as the padded triple."""
    feats = {}
    for i, ((h, w), name) in enumerate(zip(_map_sizes(SIZE), ["p2", "p3", "p4", "p5", "pool"])):
        nhwc = synth.normal(80 + i, 2, 2 * h * w * 256).astype(np.float32).reshape(2, h, w, 256)
        feats[name] = torch.from_numpy(nhwc).to(DEV).permute(0, 3, 1, 2)
    props, _, _, _, _, _ = target_problem(300, (7, 3), SIZE)
    gts = [to.scene(47, 7, SIZE), to.scene(43, 3, SIZE)]
    labels = [np.arange(7) % (NC - 1) + 1, np.asarray([2, 5, 1])]
    props[1, 150:] = 0.0
    targets = [{"boxes": _dev(g), "labels": _dev(l.astype(np.int64))} for g, l in zip(gts, labels)]
    gt_boxes, gt_count = to.pad_gt(gts, fill=0.0)
    gt_labels = np.zeros((2, 7), dtype=np.int32)
    gt_labels[0], gt_labels[1, :3] = labels[0], labels[1]
    return _roi_heads(), feats, _dev(props), _dev(np.asarray([300, 150], dtype=np.int32)), gts, gt_labels, targets, \
        (_dev(gt_boxes), _dev(gt_labels), _dev(gt_count))


def test_stage_losses_against_the_chained_oracles(stage):
    rh, feats, props, count, gts, gt_labels, targets, padded_targets = stage
    with torch.no_grad():
        losses = rh(feats, props, count, SIZE, targets=targets, generator=_seeded(3))
    assert sorted(losses) == ["loss_box_reg", "loss_classifier"]
    # stage by stage, every oracle fed the device's output of the stage before; the keys are the generator's first draw
    keys = torch.randint(0, 2 ** 31 - 1, (2, 307), device=DEV, dtype=torch.int32, generator=_seeded(3))
    gt_boxes, gt_count = to.pad_gt(gts)
    ref = bo.targets(props.cpu().numpy(), count.cpu().numpy(), gt_boxes, gt_labels, gt_count, keys.cpu().numpy())
    rois, lab, reg, mat, smp = rh.select_training_samples_padded(props, count, *padded_targets, generator=_seeded(3))
    np.testing.assert_array_equal(lab.cpu().numpy(), ref[1])
    np.testing.assert_array_equal(smp.cpu().numpy(), ref[4])
    assert rois.cpu().numpy().tobytes() == ref[0].tobytes() and int(smp[:, 0].min()) > 0
    with torch.no_grad():
        y = rh.head_padded(feats, rois, smp.sum(dim=1, dtype=torch.int32), SIZE)
    want, _ = bo.loss(y.cpu().numpy(), lab.cpu().numpy(), reg.cpu().numpy(), NC)
    got = [losses["loss_classifier"].item(), losses["loss_box_reg"].item()]
    print("stage losses", got, "oracle", list(want), "sampled", smp.tolist())
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-5 * abs(b)
    # padded targets and the same seed: identical; another seed: another sample; with gradients: the same numbers, differentiable
    with torch.no_grad():
        losses_p = rh(feats, props, count, SIZE, targets=padded_targets, padded=True, generator=_seeded(3))
        losses_o = rh(feats, props, count, SIZE, targets=padded_targets, padded=True, generator=_seeded(4))
    live = rh(feats, props, count, SIZE, targets=padded_targets, padded=True, generator=_seeded(3))
    for k in losses:
        assert torch.equal(losses[k], losses_p[k]) and torch.equal(losses[k], live[k].detach()) and live[k].requires_grad
    assert not torch.equal(losses["loss_classifier"], losses_o["loss_classifier"])


def test_padded_loss_forward_is_graph_capturable(stage):
    rh, feats, props, count, _, _, _, padded_targets = stage
    static = {k: f.clone(memory_format=torch.preserve_format) for k, f in feats.items()}
    inputs = [feats, {k: f.flip(0) * 0.5 for k, f in feats.items()}]

    def run():
        out = rh(static, props, count, SIZE, targets=padded_targets, padded=True)
        return out["loss_classifier"], out["loss_box_reg"]

    with torch.no_grad():
        eager = []
        for inp in inputs:
            for k in static:
                static[k].copy_(inp[k])
            torch.cuda.manual_seed(9)
            eager.append(tuple(t.clone() for t in run()))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                                                   # warm-up on a side stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        for inp, ref in zip(inputs, eager):
            for k in static:
                static[k].copy_(inp[k])
            torch.cuda.manual_seed(9)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, ref):
                assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_sgd_on_the_box_head_lowers_the_loss(stage):
    _, feats, props, count, _, _, _, padded_targets = stage
    rh = _roi_heads(seed=6, spread=False)
    history = []
    for _ in range(20):
        losses = rh(feats, props, count, SIZE, targets=padded_targets, padded=True, generator=_seeded(1))
        loss = losses["loss_classifier"] + losses["loss_box_reg"]
        rh.zero_grad()
        loss.backward()
        with torch.no_grad():
            for p in rh.parameters():
                p -= 0.01 * p.grad
        history.append(loss.item())
    print("summed loss over 20 SGD steps:", [round(v, 4) for v in history])
    assert all(np.isfinite(history)) and history[-1] < history[0]


def test_detector_losses_reach_every_stage():
    """LayoutDetectionModel.losses on the smallest encoder: the reference's four keys, and after backward() on their sum finite,
    non-zero gradients on the box head, the RPN head, the FPN and the encoder."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    model = model.to(DEV).train()
    images = [torch.from_numpy(synth.synth_images(1, 120, 200, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 224, 224, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV),
                "labels": torch.tensor([1, 3], device=DEV)},
               {"boxes": _dev(to.scene(7, 7)), "labels": _dev(np.arange(7, dtype=np.int64) % 5 + 1)}]
    losses = model.losses(images, targets, generator=_seeded(2))
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    total = sum(losses.values())
    assert all(np.isfinite(v.item()) for v in losses.values()) and losses["loss_classifier"].item() > 0
    total.backward()
    seen = {"roi_heads.box_head.fc6.weight": 0, "roi_heads.box_predictor.bbox_pred.weight": 0, "rpn.head.": 0, "backbone.fpn.": 0,
            "backbone.backbone.dit.": 0}
    for name, p in model.model.named_parameters():
        for prefix in seen:
            if name.startswith(prefix) and p.requires_grad and p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
                seen[prefix] += int(p.grad.abs().max().item() > 0)
    print("parameters with a non-zero gradient:", seen)
    assert seen["roi_heads.box_head.fc6.weight"] == 1 and seen["roi_heads.box_predictor.bbox_pred.weight"] == 1
    assert seen["rpn.head."] == 6 and seen["backbone.fpn."] == 16 and seen["backbone.backbone.dit."] > 10
    with pytest.raises(RuntimeError, match="inference only"):
        model(images, targets)
