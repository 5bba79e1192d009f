"""COCO box evaluation on the GPU (csrc/coco_eval.hip through ops.coco_match / ops.coco_accumulate and layoutdit_amd/evaluation.py)
against the float64 numpy oracle tests/coco_oracle.py.  Gates: codes, ranks and npig EXACTLY; precision and
recall within 1e-12 and the 12 numbers within 1e-9 (both sides do the same double operations on equal integer counts - only the
order of the final means differs, at most n 2^-53 for n <= 10 * 101 * K terms in [0, 1]); -1 cells exactly; streaming, repetition,
reset and graph replay bit for bit.  A scene is used only if the oracle finds every detection / GT IoU (plain and crowd form) at
least 1e-9 off every threshold: a seed that violates the margin fails its test."""
import numpy as np
import pytest
import torch

from layoutdit_amd import CocoBoxEvaluator, DiTConfig, evaluate, synth
from layoutdit_amd.modeling import LayoutDetectionModel
from tests import coco_oracle as co
from tests import roi_oracle as roi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-9
B, D, G, K = 3, 16, 8, 3


def _dev(batch):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in batch]


def _two_batches(seed):
    """Six images as two batches of B = 3: one image with detections and no GT, one with GT and no detections, one with neither, three
    with both; image 0's scores are quantised to eighths; rows past the counts are NaN with garbage labels; some labels are 0, K + 1."""
    first = co.scene(seed, [13, 16, 9], [6, 8, 0], D, G, K, tie_images=(0,))
    second = co.scene(1000 + seed, [0, 0, 11], [5, 0, 7], D, G, K, tie_images=())
    return first, second


def _cat(batches):
    return [np.concatenate([b[i] for b in batches]) for i in range(9)]


def _evaluator(batches, capacity=None, **kw):
    n = sum(len(b[3]) for b in batches)
    ev = CocoBoxEvaluator(kw.pop("num_classes", K), capacity or n, kw.pop("max_dets", D), kw.pop("max_gt", G), device=DEV)
    for b in batches:
        ev.update(*_dev(b))
    return ev


@pytest.fixture(scope="module")
def six_images():
    """Seed 0's six images, their oracle result (computed once, left unchanged) and the evaluator after two updates and compute()."""
    batches = _two_batches(0)
    ref = co.evaluate(*_cat(batches), num_classes=K, margin=MARGIN)
    ev = _evaluator(batches)
    stats = ev.compute()
    return batches, ref, ev, stats


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_match_equals_the_oracle_exactly(seed):
    batches = _two_batches(seed)
    assert np.isnan(batches[0][0][0, 13:]).all() and (batches[0][1][0, :13] * 8 % 1 == 0).all()
    labels = np.concatenate([b[2][i, :n] for b in batches for i, n in enumerate(b[3])])
    assert (labels == 0).any() and (labels == K + 1).any()
    ref = co.evaluate(*_cat(batches), num_classes=K, margin=MARGIN)
    ev = _evaluator(batches, capacity=8, max_dets=20)                     # rows wider than D and a store larger than the data
    code, rank, npig = ev.code.cpu().numpy(), ev.rank.cpu().numpy(), ev.npig.cpu().numpy()
    np.testing.assert_array_equal(code[:6, :D], ref["code"])
    np.testing.assert_array_equal(rank[:6, :D], ref["rank"])
    np.testing.assert_array_equal(npig[:6], ref["npig"])
    assert (code[:6, D:] == co.ABSENT).all() and (rank[:6, D:] == -1).all()                       # slots past D: absent
    assert (code[6:] == co.ABSENT).all() and (rank[6:] == -1).all() and not npig[6:].any()        # rows never written
    present = ref["rank"] >= 0
    assert {0, 1, 2, 3} <= set(np.unique(code[:6, :D]).tolist()) and present.sum() > 30
    scores, lab = ev.scores.cpu().numpy()[:6, :D], ev.labels.cpu().numpy()[:6, :D]
    full = _cat(batches)
    np.testing.assert_array_equal(scores[present], full[1][present])
    np.testing.assert_array_equal(lab[present], full[2][present])
    assert not scores[~present].any() and not lab[~present].any()         # nothing of a row past a count reaches the store
    assert ref["rank"][3].max() == -1 and ref["rank"][4].max() == -1 and ref["npig"][2].sum() == 0 and ref["npig"][4].sum() == 0


def test_at_the_caps():
    """D = G = 128, one category, 120 detections of it: the 20 of lowest score come out absent."""
    batch = co.scene(7, [120], [128], 128, 128, 1, tie_images=(), stray_labels=False)
    ref = co.evaluate(*batch, num_classes=1, margin=MARGIN)
    ev = _evaluator([batch], num_classes=1, max_dets=128, max_gt=128)
    stats = ev.compute().cpu().numpy()
    rank = ev.rank.cpu().numpy()
    np.testing.assert_array_equal(ev.code.cpu().numpy(), ref["code"])
    np.testing.assert_array_equal(rank, ref["rank"])
    np.testing.assert_array_equal(ev.npig.cpu().numpy(), ref["npig"])
    assert (rank[0, :120] >= 0).sum() == 100 and rank.max() == 99 and (rank[0, 120:] == -1).all()
    assert (ev.code.cpu().numpy()[0][rank[0] < 0] == co.ABSENT).all()
    assert np.abs(ev.precision.cpu().numpy() - ref["precision"]).max() <= 1e-12
    assert np.abs(stats - ref["stats"]).max() <= 1e-9


@pytest.mark.parametrize("name", sorted(co.anchor_cases()))
def test_hand_anchors_through_the_kernels(name):
    """The five hand-derived cases of tests/test_coco_eval_cpu.py, through update_lists and the kernels."""
    outputs, targets, classes = co.anchor_cases()[name]
    ref = co.evaluate(*co.pad_lists(outputs, targets), num_classes=classes, margin=1e-3, both_forms=False)
    ev = CocoBoxEvaluator(classes, 1, max_dets=4, max_gt=4, device=DEV)
    ev.update_lists([{k: torch.from_numpy(v).to(DEV) for k, v in o.items()} for o in outputs],
                    [{k: torch.from_numpy(v).to(DEV) for k, v in t.items()} for t in targets])
    stats = ev.compute().cpu().numpy()
    n = len(outputs[0]["scores"])
    np.testing.assert_array_equal(ev.code.cpu().numpy()[:, :n], ref["code"])
    np.testing.assert_array_equal(ev.npig.cpu().numpy(), ref["npig"])
    assert np.abs(stats - ref["stats"]).max() <= 1e-9 and ((stats == -1) == (ref["stats"] == -1)).all()
    expect = {"three_dets_two_gt": [(51 + 50 * 2 / 3) / 101] * 3 + [-1, -1, (51 + 50 * 2 / 3) / 101, .5, 1, 1, -1, -1, 1],
              "one_det_one_gt": [.4, 1, 0, -1, -1, .4, .4, .4, .4, -1, -1, .4],
              "empty_cells": [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1]}
    if name in expect:
        np.testing.assert_allclose(stats, expect[name], rtol=0, atol=1e-9)
    if name == "tie":
        assert (ev.code.cpu().numpy()[0, 1, 0] == 1).all()
    if name == "ignore_crowd_range":
        assert ev.npig.cpu().numpy()[0, 0].tolist() == [2, 0, 1, 1]
        assert ev.code.cpu().numpy()[0, :3, 0].tolist() == [[1] * 6 + [2] * 4, [2] * 10, [0] * 10]


def test_accumulation_matches_the_oracle(six_images):
    _, ref, ev, stats = six_images
    precision, recall, stats = ev.precision.cpu().numpy(), ev.recall.cpu().numpy(), stats.cpu().numpy()
    assert tuple(precision.shape) == (10, 101, K, 4, 3) and tuple(recall.shape) == (10, K, 4, 3) and stats.dtype == np.float64
    dp, dr, ds = np.abs(precision - ref["precision"]).max(), np.abs(recall - ref["recall"]).max(), np.abs(stats - ref["stats"]).max()
    print(f"coco accumulation: max |precision - oracle| = {dp:.3e}, recall {dr:.3e}, stats {ds:.3e}")
    assert dp <= 1e-12 and dr <= 1e-12 and ds <= 1e-9
    np.testing.assert_array_equal(precision == -1, ref["precision"] == -1)
    np.testing.assert_array_equal(recall == -1, ref["recall"] == -1)
    np.testing.assert_array_equal(stats == -1, ref["stats"] == -1)
    assert (ref["precision"] > 0).any() and ((ref["precision"] > 0) & (ref["precision"] < 0.99)).any()      # a non-trivial table
    assert len(np.unique(np.round(ref["stats"], 6))) >= 8
    assert ev.summary() == dict(zip(co.KEYS, stats.tolist()))


def _state(ev, stats):
    return [t.clone() for t in (ev.code, ev.rank, ev.npig, ev.scores, ev.labels, ev.precision, ev.recall, stats)]


def test_streaming_repetition_and_reset_are_bit_identical(six_images):
    batches, _, _, _ = six_images
    full = _cat(batches)
    parts = [[x[lo:hi] for x in full] for lo, hi in ((0, 1), (1, 4), (4, 6))]
    one = _evaluator([full])
    want = _state(one, one.compute())
    ev = _evaluator(parts)
    assert ev.num_images == 6
    got = _state(ev, ev.compute())
    again = _state(ev, ev.compute())                                      # computing twice changes nothing
    other = _evaluator(parts)
    twice = _state(other, other.compute())                                # a second evaluator on the same data
    ev.reset()
    assert ev.num_images == 0 and (ev.rank == -1).all() and (ev.code == co.ABSENT).all()
    for p in parts:
        ev.update(*_dev(p))
    after_reset = _state(ev, ev.compute())
    for name, state in (("streamed", got), ("again", again), ("twice", twice), ("reset", after_reset)):
        for a, b in zip(state, want):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name        # the bits, -1 and all
    empty = CocoBoxEvaluator(K, 2, D, G, device=DEV)
    assert (empty.compute() == -1).all() and (empty.precision == -1).all()             # nothing seen: every cell is -1


def test_update_lists_equals_update_on_the_padded_form(six_images):
    batches, _, _, _ = six_images
    batch = batches[0]
    boxes, scores, labels, count, gtb, gtl, gtc, crowd, area = batch
    outputs = [{"boxes": torch.from_numpy(boxes[i, :n]).to(DEV), "scores": torch.from_numpy(scores[i, :n]).to(DEV),
                "labels": torch.from_numpy(labels[i, :n].astype(np.int64)).to(DEV)} for i, n in enumerate(count)]
    targets = [{"boxes": torch.from_numpy(gtb[i, :g]).to(DEV), "labels": torch.from_numpy(gtl[i, :g].astype(np.int64)).to(DEV),
                "iscrowd": torch.from_numpy(crowd[i, :g].astype(np.int64)).to(DEV), "area": torch.from_numpy(area[i, :g]).to(DEV)}
               for i, g in enumerate(gtc)]
    a = CocoBoxEvaluator(K, 3, D, G, device=DEV)
    a.update_lists(outputs, targets)
    b = _evaluator([batch])
    for x, y in zip(_state(a, a.compute()), _state(b, b.compute())):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert a.num_images == 3


def test_compute_is_graph_capturable(six_images):
    """compute() allocates nothing in the library and never synchronises: captured once, replayed, equal to the eager bits."""
    batches, _, _, eager = six_images
    ev = _evaluator(batches)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.compute()                                                      # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    want_p = ev.precision.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = ev.compute()
    ev.precision.fill_(7.0)
    static.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.view(torch.uint8), eager.view(torch.uint8)) and torch.equal(ev.precision.view(torch.uint8), want_p.view(torch.uint8))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    """The smallest detector of the existing detector tests (hidden 128, 3 layers), eval mode, with tests/test_gpu_roi.py's recipe for
    weights that let a few dozen detections per image through, and four synthetic images of two different sizes."""
    NC = 6
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
    rng = np.random.RandomState(5)
    images = [torch.from_numpy(rng.rand(3, h, w).astype(np.float32)).to(DEV) for h, w in ((180, 300), (333, 211), (180, 300), (333, 211))]
    with torch.no_grad():
        batch = m.transform(images)[0].tensors
        feats = m.backbone(batch)
        proposals, _, count = m.rpn(feats, (224, 224), padded=True)
        y = m.roi_heads.head_padded(feats, proposals, count, (224, 224)).cpu().double().numpy()
        cnt = count.cpu().numpy()
        R = proposals.shape[1]
        valid = [y[b * R:b * R + cnt[b], :NC] for b in range(len(images))]
        bias = 0.0
        while max(int((roi.softmax64(v + np.eye(NC)[0] * bias)[:, 1:] > 0.05).sum()) for v in valid) > 60:
            bias += 0.25
        pred.cls_score.bias[0] = bias
    return model, images


def _forward(model, images):
    """model.forward in the batches evaluate() is given: two images at a time."""
    with torch.no_grad():
        return model(images[:2]) + model(images[2:])


def test_evaluate_end_to_end_matches_the_oracle_on_forwards_lists(detector):
    model, images = detector
    first = _forward(model, images)
    assert sum(len(o["scores"]) for o in first) >= 8
    # GT: every other detection of the first forward, shifted by 3 px, with its label
    targets = [{"boxes": o["boxes"][::2] + 3.0, "labels": o["labels"][::2]} for o in first]
    batches = [(images[:2], targets[:2]), (images[2:], targets[2:])]
    ev = CocoBoxEvaluator(5, 4, model.model.roi_heads.detections_per_img, 64, device=DEV)
    got = evaluate(model, batches, evaluator=ev)
    outs = _forward(model, images)
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}                        # noqa: E731
    padded = co.pad_lists([host(o) for o in outs], [host(t) for t in targets], D=100, G=64)
    ref = co.evaluate(*padded[:7], None, None, num_classes=5, margin=MARGIN)
    for i, o in enumerate(outs):
        n = len(o["scores"])
        assert (ev.rank[i, :n] >= 0).all() and (ev.rank[i, n:] == -1).all()
        assert torch.equal(ev.scores[i, :n], o["scores"]) and torch.equal(ev.labels[i, :n].long(), o["labels"])
    np.testing.assert_array_equal(ev.code.cpu().numpy(), ref["code"])
    np.testing.assert_array_equal(ev.npig.cpu().numpy(), ref["npig"])
    assert list(got) == list(co.KEYS)
    stats = np.asarray(list(got.values()))
    print("end to end:", {k: round(v, 4) for k, v in got.items()}, "max |stats - oracle| =", np.abs(stats - ref["stats"]).max())
    assert np.abs(stats - ref["stats"]).max() <= 1e-9
    assert got["AR100"] > 0 and got["mAP"] < 1                            # neither empty nor perfect
    assert evaluate(model, batches) == got                                # the default evaluator, capacity counted from the list


def test_evaluate_scores_the_boxes_of_forward(detector, monkeypatch):
    """The boxes handed to update() are torch.equal to model.forward's, image by image."""
    model, images = detector
    seen = []
    real = CocoBoxEvaluator.update

    def spy(self, boxes, scores, labels, count, *gt):
        seen.append((boxes.clone(), count.clone()))
        return real(self, boxes, scores, labels, count, *gt)

    monkeypatch.setattr(CocoBoxEvaluator, "update", spy)
    targets = [{"boxes": torch.tensor([[10.0, 10.0, 60.0, 80.0]], device=DEV), "labels": torch.tensor([1], device=DEV)} for _ in images]
    evaluate(model, [(images[:2], targets[:2]), (images[2:], targets[2:])])
    outs = _forward(model, images)
    boxes = torch.cat([b for b, _ in seen])
    counts = torch.cat([c for _, c in seen]).tolist()
    assert len(counts) == 4 and sum(counts) >= 8
    for i, (o, n) in enumerate(zip(outs, counts)):
        assert n == len(o["scores"]) and torch.equal(boxes[i, :n], o["boxes"])
