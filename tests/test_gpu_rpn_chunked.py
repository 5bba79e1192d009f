"""The chunked RPN kernels on the GPU (ldit_rpn_topk_chunked_f32 in csrc/proposals.hip, ldit_rpn_targets_chunked_f32 in
csrc/rpn_train.hip): levels and images of more than S = ops.RPN_SORT_SLOTS = 16 384 anchors, which the sort buffer in LDS does not
hold at once.  Both are tournaments under a total order, so their results are DEFINED as what one sort of everything would give:
top-k indices, labels, matches and sampler counts are compared for EQUALITY with the numpy oracles (tests/rpn_oracle.py,
tests/rpn_train_oracle.py, both size-generic), regression targets within the existing gate 8 * 2^-23 * max(|t|, 1).  Where the old
entry points apply too (sizes <= S) the new ones must give their bits.  Then the dispatch in ``ops`` (the two tests that fail
without the feature) and the whole detector at 320 x 320: p2 has 80 * 80 * 3 = 19 200 anchors, an image 25 575."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, ops, synth            # noqa: E402
from layoutdit_amd.config import DiTConfig            # noqa: E402
from layoutdit_amd.modeling import AnchorGenerator, LayoutDetectionModel    # noqa: E402
from layoutdit_amd.modeling.roi_heads import _nhwc_f32                    # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402
from tests import rpn_oracle as ro                    # noqa: E402
from tests import rpn_train_oracle as to              # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -23
S = ops.RPN_SORT_SLOTS
K_SWEEP = (1, 40, 1000, 2000, 8192)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seeded(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------
def _topk_entry(name, logits, sizes, k):
    """One of the two C entry points, called directly (ops.rpn_topk chooses by size)."""
    B = logits.shape[0]
    idx = torch.full((B, sum(min(k, n) for n in sizes)), -7, device=DEV, dtype=torch.int32)
    ops._launch(logits.device, getattr(_lib.load(), name), logits.data_ptr(), (C.c_int64 * len(sizes))(*sizes), len(sizes), B, int(k),
                idx.data_ptr())
    return idx


def _check_topk(v, sizes, k):
    got = ops.rpn_topk(_dev(v), sizes, k).cpu().numpy()
    assert got.shape == (v.shape[0], sum(min(k, n) for n in sizes))
    for b in range(v.shape[0]):
        np.testing.assert_array_equal(got[b], ro.topk_indices(v[b], sizes, k), err_msg=f"image {b}")
    return got


def _sweep_sizes(k):
    """One more than the buffer; the anchors of exactly two chunks (the second takes S - k); one more than that; three and nearly
    five buffers."""
    return (S + 1, S + (S - k), S + (S - k) + 1, 49152, 76800)


@pytest.mark.parametrize("k", K_SWEEP)
@pytest.mark.parametrize("which", range(5))
def test_topk_single_level_equals_one_sort_of_the_whole_level(which, k):
    n = _sweep_sizes(k)[which]
    rng = np.random.RandomState(1000 * which + k)
    v = rng.normal(0, 2, size=(1, n)).astype(np.float32)
    _check_topk(v, (n,), k)


def test_topk_level_set_of_a_384_by_288_page():
    sizes = (96 * 72 * 3, 48 * 36 * 3, 24 * 18 * 3, 12 * 9 * 3, 6 * 5 * 3)       # p2 = 20 736 chunked, the others in one sort each
    assert sizes[0] == 20736 and max(sizes[1:]) < S
    rng = np.random.RandomState(3)
    v = rng.normal(0, 2, size=(2, sum(sizes))).astype(np.float32)
    for k in (1000, 2000):
        _check_topk(v, sizes, k)


@pytest.mark.parametrize("k", [40, 2000, 8192])
def test_topk_ties_straddle_every_chunk_boundary(k):
    rng = np.random.RandomState(k)
    n = 76800
    _check_topk(rng.randint(0, 8, size=(2, n)).astype(np.float32), (n,), k)      # 8 distinct values
    got = _check_topk(np.full((1, n), 0.25, dtype=np.float32), (n,), k)           # all equal: the first k indices
    np.testing.assert_array_equal(got[0], np.arange(k))


@pytest.mark.parametrize("k", [1000, 8192])
def test_topk_infinities_and_nans(k):
    rng = np.random.RandomState(k + 1)
    n = 49152
    v = rng.normal(0, 2, size=(2, n)).astype(np.float32)
    v[rng.rand(2, n) < 0.01] = -np.inf
    v[rng.rand(2, n) < 0.01] = np.nan
    _check_topk(v, (n,), k)
    # fewer than k finite entries: -inf behind them, NaN behind -inf, each by ascending index
    w = np.where(rng.rand(2, n) < 0.5, -np.inf, np.nan).astype(np.float32)
    finite = rng.permutation(n)[:k // 2]
    w[:, finite] = rng.normal(0, 2, size=(2, k // 2)).astype(np.float32)
    _check_topk(w, (n,), k)


@pytest.mark.parametrize("k", [1000, 8192])
def test_topk_winners_all_in_the_last_or_the_first_chunk(k):
    n = 76800
    ramp = np.arange(n, dtype=np.float32)[None]
    got = _check_topk(ramp, (n,), k)                                               # every chunk replaces the whole carry
    np.testing.assert_array_equal(got[0], np.arange(n - 1, n - 1 - k, -1))
    got = _check_topk(-ramp, (n,), k)                                              # the first sort's carry survives
    np.testing.assert_array_equal(got[0], np.arange(k))


def test_topk_chunked_entry_gives_the_old_entrys_bits_where_both_apply():
    rng = np.random.RandomState(9)
    for sizes in ((9408, 2352, 588, 147, 48), (S, 1), (S - 1, 7, 1000)):
        v = np.round(rng.normal(0, 2, size=(2, sum(sizes))) * 8).astype(np.float32) / 8
        v[rng.rand(*v.shape) < 0.01] = -np.inf
        v[rng.rand(*v.shape) < 0.002] = np.nan
        d = _dev(v)
        for k in (16, 1000, 8192):
            old, new = _topk_entry("ldit_rpn_topk_f32", d, sizes, k), _topk_entry("ldit_rpn_topk_chunked_f32", d, sizes, k)
            assert torch.equal(old, new), (sizes, k)
            assert torch.equal(new, _topk_entry("ldit_rpn_topk_chunked_f32", d, sizes, k))
    v = _dev(rng.randint(0, 8, size=(2, 76800)).astype(np.float32))               # two runs are bit-identical
    assert torch.equal(_topk_entry("ldit_rpn_topk_chunked_f32", v, (76800,), 2000), _topk_entry("ldit_rpn_topk_chunked_f32", v, (76800,), 2000))


# ---- targets -------------------------------------------------------------------------------------------------------------------------
def _generator():
    return AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)


def _grids(size):
    h, w = size
    return [(h // 4, w // 4), (h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32), ((h // 32 + 1) // 2, (w // 32 + 1) // 2)]


_ANCHORS = {}


def _anchors(side):
    if side not in _ANCHORS:
        _ANCHORS[side] = _generator().host_anchors(_grids((side, side)), (side, side))[0]
    return _ANCHORS[side]


def _synthetic_anchors(n):
    """n of the 640 x 640 set's anchors, in their order."""
    full = _anchors(640)
    return full[np.sort(np.random.RandomState(n).permutation(full.shape[0])[:n])]


def _targets_entry(name, anchors, gt_boxes, gt_count, keys, bs=256, frac=0.5):
    B, N = keys.shape
    lab = torch.full((B, N), -7, device=DEV, dtype=torch.int32)
    mat = torch.full((B, N), -7, device=DEV, dtype=torch.int32)
    reg = torch.full((B, N, 4), 7.0, device=DEV, dtype=torch.float32)
    smp = torch.full((B, 2), -7, device=DEV, dtype=torch.int32)
    ops._launch(anchors.device, getattr(_lib.load(), name), anchors.data_ptr(), gt_boxes.data_ptr(), gt_count.data_ptr(), keys.data_ptr(), B, N,
                gt_boxes.shape[1], 0.7, 0.3, int(bs), float(frac), lab.data_ptr(), mat.data_ptr(), reg.data_ptr(), smp.data_ptr())
    return lab, mat, reg, smp


def _check_targets(anchors, gts, keys, sampler=(256, 0.5), gmax=None):
    """ops.rpn_targets against the oracle: labels, matched, sampled EQUAL, reg_targets within the existing gate."""
    bs, frac = sampler
    gt_boxes, gt_count = to.pad_gt(gts, gmax=gmax)
    ref_lab, ref_mat, ref_reg, ref_smp = to.targets(anchors, gt_boxes, gt_count, keys, 0.7, 0.3, bs, frac)
    lab, mat, reg, smp = ops.rpn_targets(_dev(anchors), _dev(gt_boxes), _dev(gt_count), _dev(keys), 0.7, 0.3, bs, frac)
    lab, mat, reg, smp = lab.cpu().numpy(), mat.cpu().numpy(), reg.cpu().numpy(), smp.cpu().numpy()
    for b in range(len(gts)):
        np.testing.assert_array_equal(mat[b], ref_mat[b], err_msg=f"matched, image {b}")
        np.testing.assert_array_equal(smp[b], ref_smp[b], err_msg=f"sampled, image {b}")
        np.testing.assert_array_equal(lab[b], ref_lab[b], err_msg=f"labels, image {b}")
    assert np.isfinite(reg).all()
    err = np.abs(reg.astype(np.float64) - ref_reg)
    bound = 8 * EPS * np.maximum(np.abs(ref_reg), 1.0)
    print(f"N={anchors.shape[0]} sampler={sampler}: sampled {smp.tolist()}, positives {[int((m >= 0).sum()) for m in mat]}, "
          f"reg_targets max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert not reg[mat < 0].any()
    return lab, mat, smp


def _keys(seed, B, N):
    """Full-range keys for even images, three bits for odd ones (ties broken by the index, across chunks)."""
    rng = np.random.RandomState(seed)
    keys = rng.randint(0, 2 ** 31 - 1, size=(B, N)).astype(np.int32)
    keys[1::2] = rng.randint(0, 8, size=(keys[1::2].shape[0], N))
    return keys


@pytest.mark.parametrize("side", [288, 320, 512, 640])
def test_targets_on_real_anchor_sets(side):
    anchors = _anchors(side)
    assert anchors.shape[0] == {288: 20730, 320: 25575, 512: 65472, 640: 102300}[side]
    gts = [to.scene(side + g, g, (side, side)) for g in (37, 1)]                  # B = 2 with different counts
    _, mat, smp = _check_targets(anchors, gts, _keys(side, 2, anchors.shape[0]))
    assert (mat[0] >= 0).sum() > 0 and (mat[0] == -2).sum() > 0 and smp.sum() == 512


@pytest.mark.parametrize("g", [0, 1, 37])
@pytest.mark.parametrize("n", [S + 1, 65535, 65536, 65537])
def test_targets_around_the_old_keys_index_boundary(n, g):
    anchors = _synthetic_anchors(n)
    gts = [to.scene(n + g, g, (640, 640)), to.scene(n + g + 1, max(g // 2, 1), (640, 640))]
    _, mat, smp = _check_targets(anchors, gts, _keys(n + g, 2, n))
    if g == 0:
        assert (mat[0] == -1).all() and smp[0].tolist() == [0, 256]               # the image without GT


def test_targets_with_512_gt_boxes():
    n = S + 1
    _check_targets(_synthetic_anchors(n), [to.scene(5, 512, (640, 640))], _keys(5, 1, n), gmax=512)


@pytest.mark.parametrize("order", ["later_chunks_win", "first_chunk_wins"])
def test_targets_carry_replacement(order):
    """Keys that fall with the index: every chunk holds smaller keys than the carry, which is replaced whole each time.  Keys that
    rise with it: the first chunk's carry is never touched."""
    anchors = _anchors(512)
    n = anchors.shape[0]
    ramp = np.arange(n, dtype=np.int32)
    keys = np.stack([n - ramp if order == "later_chunks_win" else ramp] * 2)
    lab, mat, smp = _check_targets(anchors, [to.scene(1, 37, (512, 512)), to.scene(2, 0, (512, 512))], keys)
    neg = np.flatnonzero(mat[1] == -1)
    want = neg[-256:] if order == "later_chunks_win" else neg[:256]
    np.testing.assert_array_equal(np.flatnonzero(lab[1] == 0), want)


@pytest.mark.parametrize("sampler", [(256, 0.5), (512, 0.25), (4096, 0.5)])
def test_targets_samplers_and_both_sides_of_the_quota(sampler):
    bs, frac = sampler
    quota = int(bs * frac)
    anchors = _anchors(640)
    n = anchors.shape[0]
    few, many = to.scene(11, 2, (640, 640)), to.scene(12, 100, (640, 640))
    _, mat, smp = _check_targets(anchors, [few, many], _keys(bs, 2, n), sampler)
    pos = [int((m >= 0).sum()) for m in mat]
    assert pos[0] < 128 and smp[0].tolist() == [pos[0], bs - pos[0]]              # fewer positives than any quota: negatives fill
    assert pos[1] > 2048 and smp[1].tolist() == [quota, bs - quota]               # more than any quota: the positive cap


def test_targets_chunked_entry_gives_the_old_entrys_bits_where_both_apply():
    for n, bs in ((1, 256), (65, 16), (12543, 256), (S - 1, 512), (S, 256), (S, 4096)):
        anchors = _anchors(224) if n == 12543 else _synthetic_anchors(n)
        gt_boxes, gt_count = to.pad_gt([to.scene(n % 97, 40, (224, 224) if n == 12543 else (640, 640)), to.scene(3, 0)])
        args = (_dev(anchors), _dev(gt_boxes), _dev(gt_count), _dev(_keys(n, 2, n)), bs, 0.5)
        old, new = _targets_entry("ldit_rpn_targets_f32", *args), _targets_entry("ldit_rpn_targets_chunked_f32", *args)
        again = _targets_entry("ldit_rpn_targets_chunked_f32", *args)
        for a, b, c, what in zip(old, new, again, ("labels", "matched", "reg_targets", "sampled")):
            assert torch.equal(a, b), (n, bs, what)
            assert torch.equal(b, c), (n, bs, what)
    anchors = _anchors(640)                                                       # two runs above S are bit-identical
    gt_boxes, gt_count = to.pad_gt([to.scene(4, 37, (640, 640)), to.scene(5, 1, (640, 640))])
    args = (_dev(anchors), _dev(gt_boxes), _dev(gt_count), _dev(_keys(6, 2, anchors.shape[0])))
    for a, b in zip(_targets_entry("ldit_rpn_targets_chunked_f32", *args), _targets_entry("ldit_rpn_targets_chunked_f32", *args)):
        assert torch.equal(a, b)


# ---- the front end: these two raise LDIT_EUNSUPPORTED without the chunked kernels ------------------------------------------------------
def test_ops_rpn_topk_takes_a_level_of_16385_anchors():
    rng = np.random.RandomState(21)
    sizes = (S + 1, 48)
    v = np.round(rng.normal(0, 2, size=(2, sum(sizes))) * 8).astype(np.float32) / 8
    _check_topk(v, sizes, 1000)


def test_ops_rpn_targets_takes_16385_anchors():
    n = S + 1
    _check_targets(_synthetic_anchors(n), [to.scene(31, 7, (640, 640)), to.scene(32, 40, (640, 640))], _keys(33, 2, n))


# ---- the whole detector at 320 x 320 ----------------------------------------------------------------------------------------------------
SIDE = 320


def _detector(train):
    """The smallest encoder of the detector tests with a 20 x 20 position table, identically initialised every time."""
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512, image_size=SIDE)
    cfg.drop_path_rate = 0.0
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, fixed_size=(SIDE, SIDE))
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    with torch.no_grad():
        if not train:
            # eval: a head that spreads the logits.  The box deltas are kept small (sigma about 0.5): the decode gate
            # 8 * 2^-23 * max(|centre|, size, 1) presumes that the decoded centre does not cancel against the anchor's own - its error
            # is a rounding of dx * w, which |centre| bounds only then.  A float32 restatement of the kernel's arithmetic on the
            # 320 x 320 anchors stays inside the gate at normal deltas of sigma <= 1 (worst 0.73 of it in 127 875 rows) and exceeds it in 22
            # rows at sigma 1.5, with no fault of the kernel's (this head unscaled gives sigma about 1.9 on these features; scaled, 0.5).
            head = model.model.rpn.head
            for p in head.parameters():
                p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
            head.bbox_pred.weight.mul_(0.25)
    model = model.to(DEV)
    return model.train() if train else model.eval()


@pytest.fixture(scope="module")
def ragged_batch():
    images = [torch.from_numpy(synth.synth_images(1, 200, 310, seed=21, kind="uniform")[0]).to(DEV),
              torch.from_numpy(synth.synth_images(1, 333, 260, seed=22, kind="uniform")[0]).to(DEV)]
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 150.0, 90.0], [160.0, 40.0, 300.0, 180.0]], device=DEV),
                "labels": torch.tensor([1, 3], device=DEV)},
               {"boxes": _dev(to.scene(7, 7, (333, 260))), "labels": torch.from_numpy(np.arange(7, dtype=np.int64) % 5 + 1).to(DEV)}]
    return images, targets


def _check_decode(logits, deltas, anchors, idx, boxes, scores, side, min_size, thr):
    """tests/test_gpu_rpn.py's decode gates for an image of `side` x `side`."""
    ref_box, ref_score, (pcx, pcy, pw, ph) = ro.decode(logits, deltas, anchors, idx, side, side, min_size, thr)
    bx = 8 * EPS * np.maximum(np.maximum(np.abs(pcx), pw), 1.0)
    by = 8 * EPS * np.maximum(np.maximum(np.abs(pcy), ph), 1.0)
    assert (np.abs(boxes.astype(np.float64) - ref_box) <= np.stack([bx, by, bx, by], axis=1)).all()
    sig = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)[idx]))
    wd, ht = ref_box[:, 2] - ref_box[:, 0], ref_box[:, 3] - ref_box[:, 1]
    assert (np.abs(sig - thr) > 1e-5).all() and (np.abs(wd - min_size) > 1e-4).all() and (np.abs(ht - min_size) > 1e-4).all()
    valid = np.isfinite(ref_score)
    np.testing.assert_array_equal(np.isneginf(scores), ~valid)
    assert (np.abs(scores[valid] - ref_score[valid]) <= 8 * EPS * ref_score[valid] + 1e-38).all()


def test_detector_eval_proposals_equal_the_chained_oracle(ragged_batch):
    model = _detector(train=False)
    m = model.model
    images, _ = ragged_batch
    batch = m.transform(images)[0].tensors
    assert tuple(batch.shape) == (2, 3, SIDE, SIDE)
    with torch.no_grad():
        feats = list(m.backbone(batch).values())
        logits, deltas = m.rpn.head(feats)
        anchors, sizes = m.rpn.anchor_generator([tuple(f.shape[-2:]) for f in feats], (SIDE, SIDE), DEV)
        assert sizes == (19200, 4800, 1200, 300, 75) and tuple(logits.shape) == (2, 25575)
        idx = ops.rpn_topk(logits, sizes, 1000)
        boxes, scores = ops.rpn_decode(logits, deltas, anchors, idx, (SIDE, SIDE), 1e-3, 0.0)
        groups = m.rpn._level_ids(sizes, 2, DEV)
        keep, count, ob, osc = ops.batched_nms_padded(boxes, scores, groups, 0.7, 1000)
        pb, ps, pc = m.rpn(feats, (SIDE, SIDE), padded=True)
        det = model.forward_padded(batch)
    lg, dl, an = logits.cpu().numpy(), deltas.cpu().numpy(), anchors.cpu().numpy()
    print(f"320 x 320 detector: logits std {lg.std():.3f}, deltas std {dl.std():.3f} max |d| {np.abs(dl).max():.3f}")
    idx_h, boxes_h, scores_h, groups_h = idx.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), groups.cpu().numpy()
    assert idx_h.shape == (2, 3375)
    for b in range(2):
        np.testing.assert_array_equal(idx_h[b], ro.topk_indices(lg[b], sizes, 1000))            # fed the device's logits
        _check_decode(lg[b], dl[b], an, idx_h[b], boxes_h[b], scores_h[b], SIDE, 1e-3, 0.0)        # fed the device's indices
        ref_keep, ref_count = ro.nms(boxes_h[b], scores_h[b], groups_h[b], 0.7, 1000)              # fed the device's boxes and scores
        assert count[b].item() == ref_count and 0 < ref_count
        np.testing.assert_array_equal(keep[b].cpu().numpy(), ref_keep)
    assert torch.equal(pb, ob) and torch.equal(ps, osc) and torch.equal(pc, count)
    db, ds, dlab, dc = det
    assert tuple(db.shape[:1]) == (2,) and all(bool(torch.isfinite(t.float()).all()) for t in (db, ds))
    assert int(dc.min()) >= 0 and float(db.min()) >= 0.0 and float(db.max()) <= SIDE


def test_detector_losses_reach_every_stage(ragged_batch):
    model = _detector(train=True)
    losses = model.losses(*ragged_batch, generator=_seeded(2))
    assert sorted(losses) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"]
    assert all(np.isfinite(v.item()) for v in losses.values())
    sum(losses.values()).backward()
    seen = {"roi_heads.": 0, "rpn.head.": 0, "backbone.fpn.": 0, "backbone.backbone.dit.": 0}
    for name, p in model.model.named_parameters():
        for prefix in seen:
            if name.startswith(prefix) and p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
                seen[prefix] += int(p.grad.abs().max().item() > 0)
    print("parameters with a non-zero gradient:", seen)
    assert seen["roi_heads."] > 0 and seen["rpn.head."] == 6 and seen["backbone.fpn."] == 16 and seen["backbone.backbone.dit."] > 10


def test_detector_padded_train_forward_is_graph_capturable(ragged_batch):
    """Transformed pixels to the train proposals and the four losses, no backward: backbone, RPN and box head in train mode on padded
    targets, captured once on a single stream and replayed on other pixels written into the captured input; the default generator
    is re-seeded before each eager run and each replay."""
    model = _detector(train=True)
    m = model.model
    images, targets = ragged_batch
    image_list, scaled = m.transform(images, targets)
    gt_boxes, gt_count = m.rpn.pad_targets(scaled, DEV)
    gt_labels = torch.zeros(gt_boxes.shape[:2], dtype=torch.int32, device=DEV)
    for i, t in enumerate(scaled):
        gt_labels[i, :t["labels"].shape[0]] = t["labels"].to(torch.int32)
    inputs = [image_list.tensors, image_list.tensors.flip(0) * 0.5, -image_list.tensors]
    static = inputs[0].clone()

    def run():
        feats = {k: _nhwc_f32(v) for k, v in m.backbone(static).items()}
        (b, s, c), rl = m.rpn(feats, (SIDE, SIDE), targets=(gt_boxes, gt_count), padded=True)
        bl = m.roi_heads(feats, b, c, (SIDE, SIDE), targets=(gt_boxes, gt_labels, gt_count), padded=True)
        return b, s, c, rl["loss_objectness"], rl["loss_rpn_box_reg"], bl["loss_classifier"], bl["loss_box_reg"]

    with torch.no_grad():
        eager = []
        for inp in inputs:
            static.copy_(inp)
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
            static.copy_(inp)
            torch.cuda.manual_seed(9)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, ref):
                assert torch.equal(a, b)
    assert all(bool(torch.isfinite(t).all()) for t in eager[0][3:]) and not torch.equal(eager[0][3], eager[2][3])


def test_detector_twenty_steps_lower_the_loss(ragged_batch):
    model = _detector(train=True)
    step = DetectorTrainStep(model, lr=1e-3)
    history = [step.step(*ragged_batch, generator=_seeded(2)) for _ in range(20)]
    totals = [float(sum(v.item() for v in h.values())) for h in history]
    print("summed loss over 20 steps:", [round(v, 4) for v in totals], "steps", step.steps, "skipped", step.skipped_steps, "scale", step.scale)
    assert all(np.isfinite(v.item()) for h in history for v in h.values())
    assert totals[-1] < totals[0]
    assert step.steps == 20 and step.skipped_steps == 0
