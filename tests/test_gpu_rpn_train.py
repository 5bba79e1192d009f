"""The RPN's training side on the GPU (csrc/rpn_train.hip through the C ABI, modeling/rpn.py, modeling/detector.py) against the numpy
oracle tests/rpn_train_oracle.py: labels, matches and sampler counts EXACTLY (the oracle's IoU is float32 in the kernel's order of
operations and the scenes make it exact up to its one division, see tests/test_rpn_train_cpu.py), regression targets within
8 * 2^-23 * max(|t|, 1) of float64 (a few fp32 roundings plus logf, the decode bound's reasoning), losses and gradients within the
project's fp32 gate 2e-5, the head's backward against float64 autograd of the F.conv2d restatement (input gradient 2e-5; parameter
gradients 3e-2, the project's gradient gate: they are bf16-operand GEMMs), and the stage end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import ops, synth                  # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import AnchorGenerator, LayoutDetectionModel, RegionProposalNetwork, RPNHead    # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402
from tests.util import rel_l2                         # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
GT_COUNTS = (0, 1, 7, 40)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _generator():
    return AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)


def _grids(size):
    h, w = size
    return [(h // 4, w // 4), (h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32), ((h // 32 + 1) // 2, (w // 32 + 1) // 2)]


def _anchors(size):
    return _generator().host_anchors(_grids(size), size)[0]


def _problem(n):
    """B = 4 images with 0, 1, 7 and 40 GT boxes (rows past the count NaN); the anchors are the real set of a 96 x 160 or a
    224 x 224 image, or a random n of the latter's.  Keys: full-range for images 0 and 2, three bits for 1 and 3 (ties by index)."""
    size = (96, 160) if n == 3843 else (224, 224)
    anchors = _anchors(size)
    rng = np.random.RandomState(n)
    if n not in (3843, 12543):
        anchors = anchors[np.sort(rng.permutation(anchors.shape[0])[:n])]
    assert anchors.shape[0] == n
    gt_boxes, gt_count = to.pad_gt([to.scene(g, g, size) for g in GT_COUNTS])
    keys = rng.randint(0, 2 ** 31 - 1, size=(4, n)).astype(np.int32)
    keys[1::2] = rng.randint(0, 8, size=(2, n))
    return anchors, gt_boxes, gt_count, keys


@pytest.mark.parametrize("sampler", [(256, 0.5), (16, 0.5)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 3843, 12543])
def test_targets_equal_the_oracle(n, sampler):
    anchors, gt_boxes, gt_count, keys = _problem(n)
    bs, frac = sampler
    ref_lab, ref_mat, ref_reg, ref_smp = to.targets(anchors, gt_boxes, gt_count, keys, 0.7, 0.3, bs, frac)
    args = (_dev(anchors), _dev(gt_boxes), _dev(gt_count), _dev(keys), 0.7, 0.3, bs, frac)
    lab, mat, reg, smp = ops.rpn_targets(*args)
    lab2, mat2, reg2, smp2 = ops.rpn_targets(*args)
    assert torch.equal(lab, lab2) and torch.equal(mat, mat2) and torch.equal(reg, reg2) and torch.equal(smp, smp2)   # bit-identical
    lab, mat, reg, smp = lab.cpu().numpy(), mat.cpu().numpy(), reg.cpu().numpy(), smp.cpu().numpy()
    for b in range(4):
        np.testing.assert_array_equal(mat[b], ref_mat[b], err_msg=f"matched, image {b}")
        np.testing.assert_array_equal(smp[b], ref_smp[b], err_msg=f"sampled, image {b}")
        np.testing.assert_array_equal(lab[b], ref_lab[b], err_msg=f"labels, image {b}")
    assert np.isfinite(reg).all()
    err = np.abs(reg.astype(np.float64) - ref_reg)
    print(f"n={n}: reg_targets max err / bound = {(err / (8 * EPS * np.maximum(np.abs(ref_reg), 1.0))).max():.3f}")
    assert (err <= 8 * EPS * np.maximum(np.abs(ref_reg), 1.0)).all()
    assert not reg[mat < 0].any()                                                   # exactly zero where the anchor is no positive
    assert (mat[0] == -1).all() and smp[0, 0] == 0 and smp[0, 1] == min(bs, n)      # the image without GT
    if n == 12543:
        assert smp[3, 0] == bs // 2 and smp[3, 1] == bs - bs // 2                   # the positive cap
        assert (mat[3] >= 0).sum() > 128 and (mat[3] == -2).sum() > 0 and (mat[1] >= 0).sum() > 0


@pytest.fixture(scope="module")
def device_targets():
    """Labels, targets and counts of the 224 x 224 problem as the DEVICE computed them, for the loss tests."""
    anchors, gt_boxes, gt_count, keys = _problem(12543)
    return ops.rpn_targets(_dev(anchors), _dev(gt_boxes), _dev(gt_count), _dev(keys))


def _check_loss(logits, deltas, lab, reg, smp):
    loss, dl, dd = ops.rpn_loss(_dev(logits), _dev(deltas), lab, reg, smp)
    loss2, dl2, dd2 = ops.rpn_loss(_dev(logits), _dev(deltas), lab, reg, smp)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(dd, dd2)
    lab_h = lab.cpu().numpy()
    ref, ref_dl, ref_dd = to.loss(logits, deltas, lab_h, reg.cpu().numpy())
    loss, dl, dd = loss.cpu().numpy().astype(np.float64), dl.cpu().numpy(), dd.cpu().numpy()
    assert int(smp.sum()) == int((lab_h >= 0).sum())                                # the normaliser the kernel reads
    for got, want in zip(loss, ref):
        print(f"loss {got:.9g} vs {want:.9g}")
        assert abs(got - want) <= 2e-5 * abs(want)
    assert rel_l2(dl, ref_dl) < 2e-5
    assert not dl[lab_h < 0].any() and not dd[lab_h != 1].any()                     # exactly zero outside the loss
    if (lab_h == 1).any():
        assert rel_l2(dd, ref_dd) < 2e-5
    return loss


def test_losses_and_gradients_match_the_float64_oracle(device_targets):
    lab, _, reg, smp = device_targets
    B, N = lab.shape
    rng = np.random.RandomState(1)
    logits = rng.normal(0, 2.5, size=(B, N)).astype(np.float32)
    logits[:, ::97], logits[:, 1::97] = 80.0, -80.0
    deltas = (reg.cpu().numpy() + rng.normal(0, 0.12, size=(B, N, 4))).astype(np.float32)      # both branches of smooth-L1 (beta 1/9)
    loss = _check_loss(logits, deltas, lab, reg, smp)
    assert loss[0] > 0 and loss[1] > 0
    # a batch with no positive at all: the image without GT alone
    loss = _check_loss(logits[:1], deltas[:1], lab[:1].contiguous(), reg[:1].contiguous(), smp[:1].contiguous())
    assert loss[1] == 0.0 and loss[0] > 0
    # a size that is no multiple of anything, one image
    n = 1025
    loss = _check_loss(logits[3:, :n].copy(), deltas[3:, :n].copy(), lab[3:, :n].clone(), reg[3:, :n].clone(),
                       torch.tensor([[int((lab[3, :n] == 1).sum()), int((lab[3, :n] == 0).sum())]], dtype=torch.int32, device=DEV))
    assert loss[1] > 0


def _spread_head(seed=5):
    torch.manual_seed(seed)
    head = RPNHead(256, 3)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
    return head


def test_head_backward_matches_float64_autograd():
    head = _spread_head().to(DEV).train()
    rng = np.random.RandomState(2)
    shapes = [(8, 8), (3, 5)]
    xs = [rng.normal(0, 1, size=(2, h, w, 256)).astype(np.float32) for h, w in shapes]
    gl = [rng.normal(0, 1, size=(2, h * w * 3)).astype(np.float32) for h, w in shapes]
    gd = [rng.normal(0, 1, size=(2, h * w * 3, 4)).astype(np.float32) for h, w in shapes]
    feats = [_dev(x).permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    total = 0
    for f, a, b in zip(feats, gl, gd):
        lg, dl = head.forward_level(f)
        assert lg.requires_grad and dl.requires_grad
        total = total + (lg * _dev(a)).sum() + (dl * _dev(b)).sum()
    total.backward()
    # float64 CPU autograd of the F.conv2d restatement
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in head.named_parameters()}
    ref_x = [torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True) for x in xs]
    rt = 0
    for x, a, b in zip(ref_x, gl, gd):
        t = F.relu(F.conv2d(x, ref["conv.0.0.weight"], ref["conv.0.0.bias"], padding=1))
        lg = F.conv2d(t, ref["cls_logits.weight"], ref["cls_logits.bias"]).permute(0, 2, 3, 1).reshape(2, -1)
        dl = F.conv2d(t, ref["bbox_pred.weight"], ref["bbox_pred.bias"])
        B, _, h, w = dl.shape
        dl = dl.view(B, 3, 4, h, w).permute(0, 3, 4, 1, 2).reshape(B, -1, 4)
        rt = rt + (lg * torch.from_numpy(a).double()).sum() + (dl * torch.from_numpy(b).double()).sum()
    rt.backward()
    assert abs(total.item() - rt.item()) <= 2e-5 * abs(rt.item()) + 1e-3
    for f, x in zip(feats, ref_x):
        e = rel_l2(f.grad.cpu().numpy(), x.grad.numpy())
        print(f"input gradient {tuple(x.shape)}: {e:.3e}")
        assert e < 2e-5
    for k, p in head.named_parameters():
        e = rel_l2(p.grad.cpu().numpy(), ref[k].grad.numpy())
        print(f"{k}: {e:.3e}")
        assert e < (2e-5 if k.endswith("bias") else 3e-2), k        # biases are fp32 column sums, weights bf16-operand GEMMs


SIZE = (96, 160)


@pytest.fixture(scope="module")
def stage():
    """B = 2 at 96 x 160 (3 843 anchors): synthetic channels-last maps of the five levels, a head that spreads the logits, two
    images' GT in the reference's list form and in the padded form."""
    rpn = RegionProposalNetwork(_generator(), _spread_head()).to(DEV).train()
    feats = []
    for i, (h, w) in enumerate(_grids(SIZE)):
        nhwc = synth.normal(60 + i, 2, 2 * h * w * 256).astype(np.float32).reshape(2, h, w, 256)
        feats.append(torch.from_numpy(nhwc).to(DEV).permute(0, 3, 1, 2))
    gts = [to.scene(7, 7, SIZE), to.scene(3, 3, SIZE)]
    targets = [{"boxes": _dev(g), "labels": torch.ones(len(g), dtype=torch.int64, device=DEV)} for g in gts]
    gt_boxes, gt_count = to.pad_gt(gts, fill=0.0)
    return rpn, feats, gts, targets, (_dev(gt_boxes), _dev(gt_count))


def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def test_stage_losses_proposals_and_target_forms(stage):
    rpn, feats, gts, targets, padded_targets = stage
    with torch.no_grad():
        (boxes, scores, count), losses = rpn(feats, SIZE, targets=targets, padded=True, generator=_seeded(3))
        logits, deltas = rpn.head(feats)
    anchors, sizes = rpn.anchor_generator([tuple(f.shape[-2:]) for f in feats], SIZE, DEV)
    N = anchors.shape[0]
    assert N == 3843 and tuple(logits.shape) == (2, N)
    # the losses equal the oracle fed the device's logits and deltas (the keys are the generator's first draw)
    keys = torch.randint(0, 2 ** 31 - 1, (2, N), device=DEV, dtype=torch.int32, generator=_seeded(3)).cpu().numpy()
    gt_boxes, gt_count = to.pad_gt(gts)
    lab, _, reg, smp = to.targets(anchors.cpu().numpy(), gt_boxes, gt_count, keys)
    ref, _, _ = to.loss(logits.cpu().numpy(), deltas.cpu().numpy(), lab, reg)
    got = [losses["loss_objectness"].item(), losses["loss_rpn_box_reg"].item()]
    print("stage losses", got, "oracle", list(ref), "sampled", smp.tolist())
    assert smp[:, 0].min() > 0 and smp.sum() == 512
    for a, b in zip(got, ref):
        assert abs(a - b) <= 2e-5 * abs(b)
    # the proposals come from the train top-n: 2000 per level before and 2000 per image after the NMS
    assert tuple(boxes.shape) == (2, 2000, 4) and tuple(scores.shape) == (2, 2000) and count.dtype == torch.int32
    idx = ops.rpn_topk(logits, sizes, 2000)
    assert idx.shape[1] == sum(min(2000, n) for n in sizes) > sum(min(1000, n) for n in sizes)
    b2, s2 = ops.rpn_decode(logits, deltas, anchors, idx, SIZE, rpn.min_size, rpn.score_thresh)
    _, c3, b3, s3 = ops.batched_nms_padded(b2, s2, rpn._level_ids(sizes, 2, DEV, 2000), rpn.nms_thresh, 2000)
    assert torch.equal(boxes, b3) and torch.equal(scores, s3) and torch.equal(count, c3) and int(count.min()) > 0
    # list form, padded targets, the same seed: identical; another seed: another sample
    with torch.no_grad():
        props, losses_l = rpn(feats, SIZE, targets=targets, generator=_seeded(3))
        _, losses_p = rpn(feats, SIZE, targets=padded_targets, padded=True, generator=_seeded(3))
        _, losses_o = rpn(feats, SIZE, targets=padded_targets, padded=True, generator=_seeded(4))
    assert len(props) == 2 and all(torch.equal(props[i], boxes[i, :int(count[i])]) for i in range(2))
    for k in ("loss_objectness", "loss_rpn_box_reg"):
        assert torch.equal(losses[k], losses_l[k]) and torch.equal(losses[k], losses_p[k])
    assert not torch.equal(losses["loss_objectness"], losses_o["loss_objectness"])
    assert not props[0].requires_grad
    # with gradients the losses are the same numbers and differentiable
    _, live = rpn(feats, SIZE, targets=padded_targets, padded=True, generator=_seeded(3))
    assert live["loss_objectness"].requires_grad and live["loss_rpn_box_reg"].requires_grad
    assert torch.equal(live["loss_objectness"].detach(), losses["loss_objectness"])


def test_padded_train_forward_is_graph_capturable(stage):
    """Train mode, padded targets, no backward: head, proposals, keys, targets and losses captured once on a single stream, replayed
    on new features written into the captured inputs; the default generator is re-seeded before each eager run and each replay."""
    rpn, feats, _, _, padded_targets = stage
    inputs = [feats, [f.flip(0) * 0.5 for f in feats], [-f for f in feats]]
    static = [f.clone(memory_format=torch.preserve_format) for f in feats]

    def run():
        (b, s, c), losses = rpn(static, SIZE, targets=padded_targets, padded=True)
        return b, s, c, losses["loss_objectness"], losses["loss_rpn_box_reg"]

    with torch.no_grad():
        eager = []
        for inp in inputs:
            for st, f in zip(static, inp):
                st.copy_(f)
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
            for st, f in zip(static, inp):
                st.copy_(f)
            torch.cuda.manual_seed(9)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, ref):
                assert torch.equal(a, b)
    assert not torch.equal(eager[0][3], eager[2][3])


def test_sgd_on_the_head_lowers_the_loss(stage):
    _, feats, _, _, padded_targets = stage
    rpn = RegionProposalNetwork(_generator(), RPNHead(256, 3)).to(DEV).train()    # torchvision's init
    history = []
    for _ in range(20):
        _, losses = rpn(feats, SIZE, targets=padded_targets, padded=True, generator=_seeded(1))
        loss = losses["loss_objectness"] + losses["loss_rpn_box_reg"]
        rpn.zero_grad()
        loss.backward()
        with torch.no_grad():
            for p in rpn.parameters():
                p -= 0.01 * p.grad
        history.append(loss.item())
    print("summed loss over 20 SGD steps:", [round(v, 4) for v in history])
    assert all(np.isfinite(history)) and history[-1] < history[0]


def test_detector_rpn_losses_reach_every_stage():
    """LayoutDetectionModel.rpn_losses on the smallest encoder, then backward(): finite, non-zero gradients on the RPN head, the FPN
    and the encoder; the box head gets none."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    model = model.to(DEV).train()
    images = [torch.from_numpy(synth.synth_images(1, 120, 200, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 224, 224, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=DEV)},
               {"boxes": _dev(to.scene(7, 7))}]
    losses = model.rpn_losses(images, targets, generator=_seeded(2))
    assert sorted(losses) == ["loss_objectness", "loss_rpn_box_reg"]
    total = losses["loss_objectness"] + losses["loss_rpn_box_reg"]
    assert np.isfinite(total.item()) and losses["loss_objectness"].item() > 0 and losses["loss_rpn_box_reg"].item() > 0
    total.backward()
    seen = {"rpn.head.": 0, "backbone.fpn.": 0, "backbone.backbone.dit.": 0}
    for name, p in model.model.named_parameters():
        for prefix in seen:
            if name.startswith(prefix) and p.requires_grad and p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
                seen[prefix] += int(p.grad.abs().max().item() > 0)
        if name.startswith("roi_heads."):
            assert p.grad is None
    print("parameters with a non-zero gradient:", seen)
    assert seen["rpn.head."] == 6 and seen["backbone.fpn."] == 16 and seen["backbone.backbone.dit."] > 10
