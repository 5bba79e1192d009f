"""Test-time augmentation on the GPU: ``ops.tta_pool`` / ``ops.box_vote`` / ``ops.tta_merge`` against the numpy oracle
(``tests/tta_oracle.py``), and the feature through ``LayoutDetectionModel`` and ``evaluate``.

Gates.  Keep decisions, order, labels, scores, counts and - without voting - all boxes are EXACTLY the oracle's.  Voted boxes are
within 1 fp32 ulp of the float64 oracle rounded to fp32, and bit-equal between two runs.  Exact comparison of decisions means
something only away from ties, so every input is checked on the CPU first: the oracle's smallest ``|IoU - thresh|`` over all pairs
it decided is at least ``MARGIN`` (float32 IoUs of boxes of these sizes carry errors around 1e-7).  That is a condition on the inputs
- the generator leaves a margin (``tta_oracle.relabel_near_ties``), the seeds are fixed - not a tolerance on the kernels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import CocoBoxEvaluator, DiTConfig, TestTimeAugment, _lib, evaluate, ops, synth   # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel                                                # noqa: E402
from tests import guarded                                                                              # noqa: E402
from tests import roi_oracle as roi                                                                    # noqa: E402
from tests import tta_oracle as to                                                                     # noqa: E402
from tests.guarded import In, Out                                                                      # noqa: E402

DEV = "cuda:0"
MARGIN = 1e-4
F32 = np.float32


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()


def _dev(views):
    return [tuple(torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in view) for view in views]


def _host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _within_one_ulp(got, ref64):
    ref = ref64.astype(F32)
    ok = (got == ref) | (got == np.nextafter(ref, F32(np.inf))) | (got == np.nextafter(ref, F32(-np.inf)))
    assert ok.all(), (got[~ok][:4], ref64[~ok][:4])


def _check_merge(views, specs, pages, nms_thresh, d_out, vote_thresh):
    """One merge against the oracle under the gates of this module; returns the GPU result on the host."""
    ref_b, ref_s, ref_l, ref_n, margin = to.merge(views, specs, pages, nms_thresh, d_out, vote_thresh)
    print(f"V={len(views)} D={views[0][1].shape[1]} vote={vote_thresh}: margin {margin:.3e}, kept {ref_n.tolist()}")
    assert margin >= MARGIN, f"the inputs decide a pair within {margin:.3e} of a threshold: pick another seed"
    dv = _dev(views)
    got = _host(ops.tta_merge(dv, specs, pages, nms_thresh, d_out, vote_thresh))
    again = _host(ops.tta_merge(dv, specs, pages, nms_thresh, d_out, vote_thresh))
    gb, gs, gl, gn = got
    assert gb.dtype == F32 and gs.dtype == F32 and gl.dtype == np.int32 and gn.dtype == np.int32
    assert gb.shape == ref_b.shape and gs.shape == ref_s.shape
    np.testing.assert_array_equal(gn, ref_n)
    np.testing.assert_array_equal(gl, ref_l)
    np.testing.assert_array_equal(gs.view(np.uint32), ref_s.view(np.uint32))
    if vote_thresh is None:
        np.testing.assert_array_equal(gb.view(np.uint32), ref_b.view(np.uint32))
    else:
        _within_one_ulp(gb, ref_b)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    return got


# ---- kernels: the grid -----------------------------------------------------------------------------------------------------------------
GRID = [(V, D) for V in (1, 2, 5) for D in (5, 64, 100)] + [(16, 128)]


def _grid_inputs(V, D):
    """Dense synthetic views (dozens of overlapping detections per object), then the generator's margin step: a detection that
    forms a same-class pair within 2 MARGIN of the NMS or the voting threshold gets a class of its own."""
    views, specs, pages = to.random_views(100 * V + D, B=3, K=3, V=V, D=D, n_objects=4 + D // 8, poison=True,
                                          sizes=((224, 224), (160, 192), (96, 64)))
    views, moved = to.relabel_near_ties(views, specs, pages, (0.5, 0.6), 2 * MARGIN)
    return views, specs, pages, moved


@pytest.mark.parametrize("V,D", GRID)
def test_merge_equals_the_oracle_on_the_grid(V, D, monkeypatch):
    """B = 3 ragged pages, K = 3 classes, pools that are no multiple of 64 and, at V = 16, D = 128, cross 1024 sorted positions.  The
    padding rows of every input hold NaN boxes, scores of 3e38 and labels of 2^31 - 1; every fresh output buffer holds 0xA5 bytes."""
    views, specs, pages, moved = _grid_inputs(V, D)
    total = sum(int(v[3].sum()) for v in views)
    print(f"V={V} D={D}: {total} detections, {moved} given a class of their own")
    assert any(f for _, _, f in specs) == (V > 1) and total > 0 and moved <= total // 10
    with guarded.fresh_memory(monkeypatch, guarded.CANARY):
        for vote_thresh in (None, 0.6):
            gb, gs, gl, gn = _check_merge(views, specs, pages, 0.5, min(100, V * D), vote_thresh)
            for b, n in enumerate(gn):                                             # (also implied by equality with the oracle)
                assert not gb[b, n:].any() and not gs[b, n:].any() and not gl[b, n:].any()
            assert np.isfinite(gb).all() and int(gn.max()) > 0


def test_pool_alone_equals_the_oracle_and_never_reads_padding(monkeypatch):
    views, specs, pages = to.random_views(3, B=3, K=3, V=5, D=7, poison=True, empty_views=(2,))
    with guarded.fresh_memory(monkeypatch, guarded.CANARY):
        pb, ps, pl = _host(ops.tta_pool(_dev(views), specs, pages))
    rb, rs, rl = to.pool(views, specs, pages)
    np.testing.assert_array_equal(pb.view(np.uint32), rb.view(np.uint32))
    np.testing.assert_array_equal(ps.view(np.uint32), rs.view(np.uint32))
    np.testing.assert_array_equal(pl, rl)
    assert (ps[:, 2 * 7:3 * 7] == -np.inf).all() and not pb[:, 2 * 7:3 * 7].any()      # the empty view


def test_empty_views(monkeypatch):
    views, specs, pages = to.random_views(2, B=3, K=3, V=3, D=9, poison=True, empty_views=(1,))
    assert not views[1][3].any()
    _check_merge(views, specs, pages, 0.5, 20, 0.6)
    views, specs, pages = to.random_views(2, B=3, K=3, V=3, D=9, poison=True, empty_views=(0, 1, 2))
    with guarded.fresh_memory(monkeypatch, guarded.CANARY):
        for vote_thresh in (None, 0.5):
            gb, gs, gl, gn = _host(ops.tta_merge(_dev(views), specs, pages, 0.5, 20, vote_thresh))
            assert gn.tolist() == [0, 0, 0] and not gb.any() and not gs.any() and not gl.any()


def _view(boxes, scores, labels, D=None):
    """One view of one image from lists, padded with poison to D rows."""
    n = len(scores)
    D = D or n
    b, s, l = np.full((1, D, 4), np.nan, F32), np.full((1, D), 3e38, F32), np.full((1, D), 0x7FFFFFFF, np.int32)
    b[0, :n], s[0, :n], l[0, :n] = np.asarray(boxes, F32).reshape(n, 4), scores, labels
    return b, s, l, np.array([n], np.int32)


def test_exact_duplicates_across_views_keep_the_lower_pool_index():
    box = [10.25, 12.5, 50.75, 40.0]
    v0, v1 = _view([box, [60, 10, 90, 40]], [0.9, 0.5], [2, 2], D=3), _view([box], [0.9], [2], D=3)
    specs, pages = [(96, 64, 0), (96, 64, 0)], [(64, 96)]
    dv = _dev([v0, v1])
    pool = ops.tta_pool(dv, specs, pages)
    keep, kept, _, _ = ops.batched_nms_padded(*pool, 0.5, 4)
    assert kept.tolist() == [2] and keep[0].tolist() == [0, 1, -1, -1]               # pool index 3 (the duplicate in view 1) is gone
    for vote_thresh in (None, 0.5):
        gb, gs, gl, gn = _check_merge([v0, v1], specs, pages, 0.5, 4, vote_thresh)
        assert gn.tolist() == [2] and gl[0].tolist() == [2, 2, 0, 0]
        np.testing.assert_array_equal(gb[0, 0], np.asarray(box, F32))               # the mean of two equal boxes is the box


def test_unmirroring_at_the_borders_and_on_integer_boxes():
    W, H = 96, 64
    rng = np.random.RandomState(6)
    x = np.sort(rng.choice(W, size=(20, 2)), axis=1)
    y = np.sort(rng.choice(H, size=(20, 2)), axis=1)
    x[:, 1] = np.maximum(x[:, 1], x[:, 0] + 1)
    y[:, 1] = np.maximum(y[:, 1], y[:, 0] + 1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(F32)
    boxes[0] = [0, 0, W, H]                                                           # touches both borders: its own mirror image
    boxes[1] = [0, 3, 7, 9]                                                           # left border -> right border
    scores = np.linspace(0.9, 0.1, 20).astype(F32)
    labels = (np.arange(20) % 3 + 1).astype(np.int32)
    view = _view(boxes, scores, labels, D=23)
    pb, ps, pl = _host(ops.tta_pool(_dev([view]), [(W, H, 1)], [(H, W)]))            # the page is the view: ratios 1
    want = np.stack([W - boxes[:, 2], boxes[:, 1], W - boxes[:, 0], boxes[:, 3]], axis=1)
    np.testing.assert_array_equal(pb[0, :20], want)                                    # exact on integers
    np.testing.assert_array_equal(pb[0, 0], boxes[0])
    np.testing.assert_array_equal(pb[0, 1], np.asarray([W - 7, 3, W, 9], F32))
    assert not pb[0, 20:].any() and (ps[0, 20:] == -np.inf).all() and not pl[0, 20:].any()
    back = (pb[:, :20].copy(), ps[:, :20].copy(), pl[:, :20].copy(), np.array([20], np.int32))
    pb2, _, _ = _host(ops.tta_pool(_dev([back]), [(W, H, 1)], [(H, W)]))
    np.testing.assert_array_equal(pb2[0], boxes)                                       # unmirroring twice: the identity
    pb3, _, _ = _host(ops.tta_pool(_dev([view]), [(W, H, 1)], [(200, 301)]))          # and scaled to a page, against the oracle
    np.testing.assert_array_equal(pb3.view(np.uint32), to.pool([view], [(W, H, 1)], [(200, 301)])[0].view(np.uint32))


def test_labels_never_vote_together_and_a_degenerate_box_votes_for_itself():
    box = [10, 10, 50, 40]
    v0 = _view([box, box, [20, 20, 20, 20], [12, 10, 50, 40]], [0.9, 0.8, 0.7, 0.6], [1, 2, 1, 1], D=5)
    specs, pages = [(64, 64, 0)], [(64, 64)]
    gb, gs, gl, gn = _check_merge([v0], specs, pages, 0.99, 5, 0.5)                   # IoU 0.95: nothing is suppressed
    assert gn.tolist() == [4] and gl[0].tolist() == [1, 2, 1, 1, 0]
    np.testing.assert_array_equal(gb[0, 1], np.asarray(box, F32))                     # label 2 stands alone: [12, 10, 50, 40] of label 1 did not vote
    np.testing.assert_array_equal(gb[0, 2], np.asarray([20, 20, 20, 20], F32))        # zero area: kept, IoU 0 with the others
    assert gb[0, 0, 0] > 10 and gb[0, 0, 0] < 12                                       # label 1: the two overlapping boxes averaged
    z = _view([[20, 20, 20, 20], [20, 20, 20, 20]], [0.9, 0.8], [1, 1])               # IoU 0 / 0 = NaN: never suppressed, never a voter
    gb, gs, gl, gn = _check_merge([z], specs, pages, 0.5, 4, 0.5)
    assert gn.tolist() == [2] and np.array_equal(gb[0, :2], np.full((2, 4), 20, F32))


def test_c_entries_under_guard_bands():
    """Both entries through the C ABI with every operand inside guard bands: the inputs' padding rows and surroundings 0x00 and then
    0xFF (NaN, -1), the outputs' footprint and surroundings 0xA5.  Nothing outside an output is written, no input changes, and the two
    runs agree bit for bit with each other and with the oracle."""
    lib = _lib.load()
    V, B, D, Dout = 3, 2, 11, 24
    views, specs, pages = to.random_views(5, B=B, K=2, V=V, D=D)
    pad = [np.arange(D)[None, :] >= v[3][:, None] for v in views]
    spec = {}
    for v, (bx, sc, lb, cn) in enumerate(views):
        spec[f"b{v}"], spec[f"s{v}"] = In(bx, pad=torch.from_numpy(pad[v])[:, :, None]), In(sc, pad=torch.from_numpy(pad[v]))
        spec[f"l{v}"], spec[f"c{v}"] = In(lb, pad=torch.from_numpy(pad[v])), In(cn)
    spec.update(pb=Out((B, V * D, 4)), ps=Out((B, V * D)), pl=Out((B, V * D), torch.int32))
    c_specs = (C.c_int32 * (3 * V))(*[x for s in specs for x in s])
    c_pages = (C.c_int32 * (2 * B))(*[x for h, w in pages for x in (w, h)])
    stream = torch.cuda.current_stream().cuda_stream

    def call_pool(t):
        ptrs = [(C.c_void_p * V)(*[t[f"{k}{v}"].data_ptr() for v in range(V)]) for k in "bslc"]
        _lib.check(lib.ldit_tta_pool_f32(*ptrs, c_specs, c_pages, V, B, D, t["pb"].data_ptr(), t["ps"].data_ptr(), t["pl"].data_ptr(), stream))

    res = guarded.twin_run(spec, call_pool, device=DEV, sync=torch.cuda.synchronize)
    rb, rs, rl = to.pool(views, specs, pages)
    for got in (res.clean, res.poisoned):
        assert got["pb"].numpy().tobytes() == rb.tobytes() and got["ps"].numpy().tobytes() == rs.tobytes()
        np.testing.assert_array_equal(got["pl"].numpy(), rl)

    keep = np.stack([to.nms(rb[b], rs[b], rl[b], 0.5, Dout)[0] for b in range(B)])
    kept = np.array([to.nms(rb[b], rs[b], rl[b], 0.5, Dout)[1] for b in range(B)], np.int32)
    assert 0 < kept.min() and kept.max() < Dout                                        # padding rows exist
    kpad = torch.from_numpy(np.arange(Dout)[None, :] >= kept[:, None])
    vspec = dict(pb=In(rb), ps=In(rs), pl=In(rl), keep=In(keep, pad=kpad), kept=In(kept), ob=Out((B, Dout, 4)), ol=Out((B, Dout), torch.int32))

    def call_vote(t):
        _lib.check(lib.ldit_box_vote_f32(t["pb"].data_ptr(), t["ps"].data_ptr(), t["pl"].data_ptr(), t["keep"].data_ptr(), t["kept"].data_ptr(),
                                         B, V * D, Dout, 0.6, t["ob"].data_ptr(), t["ol"].data_ptr(), stream))

    res = guarded.twin_run(vspec, call_vote, device=DEV, sync=torch.cuda.synchronize)
    want = np.zeros((B, Dout, 4))
    for b in range(B):
        for k in range(kept[b]):
            want[b, k] = to.vote(rb[b], rs[b], rl[b], int(keep[b, k]), 0.6)
    for got in (res.clean, res.poisoned):
        guarded.assert_written(got["ob"], "voted boxes"), guarded.assert_written(got["ol"], "labels")
        _within_one_ulp(got["ob"].numpy(), want)
        for b in range(B):
            assert got["ol"][b, :kept[b]].tolist() == rl[b][keep[b, :kept[b]]].tolist() and not got["ol"][b, kept[b]:].any()


def test_merge_alone_is_graph_capturable():
    """The three launches allocate nothing in the library and never synchronise: captured once on a single stream as the box-head
    tests capture their stage, replayed on other detections written into the captured inputs, bit-equal to the eager call."""
    specs, pages = None, None
    sets = []
    for seed in (11, 12):
        views, specs, pages = to.random_views(seed, B=3, K=3, V=4, D=30, pages=[(150, 200), (333, 211), (64, 96)])
        sets.append(_dev(views))
    eager = [tuple(t.clone() for t in ops.tta_merge(dv, specs, pages, 0.5, 40, 0.6)) for dv in sets]
    static = [tuple(t.clone() for t in view) for view in sets[0]]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.tta_merge(static, specs, pages, 0.5, 40, 0.6)                              # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.tta_merge(static, specs, pages, 0.5, 40, 0.6)
    for dv, ref in zip(reversed(sets), reversed(eager)):
        for dst, src in zip(static, dv):
            for a, b in zip(dst, src):
                a.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static_out, ref):
            assert torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


# ---- the model -----------------------------------------------------------------------------------------------------------------------
PAGE_SIZES = ((91, 149), (167, 105), (64, 96))               # (h, w): three ragged pages, the last one the model's own size
MODEL_SIZE = (96, 64)                                        # fixed_size = (width, height)
PAGE_SEED = 800                                              # every page then has detections in some view, margins >= 1e-3


def _codes(seed, h, w):
    """A page as a decoder leaves it: uint8 [h, w, 3] on the CPU."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _as_f32(hwc):
    return hwc.permute(2, 0, 1).contiguous().float().div(255).to(DEV)


def build_detector(page_seed=PAGE_SEED):
    """The smallest detector of the existing detector tests (hidden 128, 3 layers, 2 heads) at 96 x 64, eval mode, with
    tests/test_gpu_coco_eval.py's recipe for weights that let a few dozen detections per image through, and three uint8 pages."""
    NC = 6
    W, H = MODEL_SIZE
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg, fixed_size=MODEL_SIZE)
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
    pages = [_codes(page_seed + i, h, w) for i, (h, w) in enumerate(PAGE_SIZES)]
    with torch.no_grad():
        batch = m.transform([_as_f32(p) for p in pages])[0].tensors
        feats = m.backbone(batch)
        proposals, _, count = m.rpn(feats, (H, W), padded=True)
        y = m.roi_heads.head_padded(feats, proposals, count, (H, W)).cpu().double().numpy()
        cnt = count.cpu().numpy()
        R = proposals.shape[1]
        valid = [y[b * R:b * R + cnt[b], :NC] for b in range(len(pages))]
        bias = 0.0
        while max(int((roi.softmax64(v + np.eye(NC)[0] * bias)[:, 1:] > 0.05).sum()) for v in valid) > 40:
            bias += 0.25
        pred.cls_score.bias[0] = bias
    return model, pages


@pytest.fixture(scope="module")
def detector():
    model, pages = build_detector()
    return model, pages, [_as_f32(p) for p in pages]


def view_outputs(model, images, views):
    """The per-view ``forward_padded`` outputs through the public API, on the host."""
    t = model.model.transform
    mirror = [(0, 0, img.shape[-1], img.shape[-2], 1) for img in images]
    outs = []
    with torch.no_grad():
        for w, h, flip in views:
            batch = ops.preprocess(t._operands(images), size=(h, w), mean=t.mean, std=t.std, windows=mirror if flip else None)
            outs.append(_host(model.forward_padded(batch)))
    return outs


def test_one_plain_view_is_forward_padded_times_the_ratios(detector):
    model, _, images = detector
    tta = TestTimeAugment(flip=False)
    assert tta.views(model) == [(96, 64, 0)]
    with torch.no_grad():
        image_list, _ = model.model.transform(images)
        boxes, scores, labels, count = model.forward_padded(image_list.tensors)
        ratios = []
        for img, (nh, nw) in zip(images, image_list.image_sizes):                     # as evaluate forms them
            oh, ow = img.shape[-2:]
            rh, rw = float(oh) / float(nh), float(ow) / float(nw)
            ratios.append([rw, rh, rw, rh])
        want_boxes = boxes * torch.tensor(ratios, dtype=boxes.dtype).to(DEV)[:, None, :]
        got = model.forward_padded_tta(images, tta)
        assert int(count.sum()) >= 8 and got[0].shape == boxes.shape
        for g, w in zip(got, (want_boxes, scores, labels, count)):
            assert g.dtype == w.dtype and torch.equal(g, w)
        plain, with_tta = model(images), model(images, tta=tta)
    assert len(plain) == len(with_tta) == 3
    for x, y in zip(plain, with_tta):
        assert sorted(x) == sorted(y) == ["boxes", "labels", "scores"]
        for k in x:
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k


class _MirroredOnly(TestTimeAugment):
    def views(self, model=None):
        return [v for v in super().views(model) if v.flip]


def test_mirrored_view_equals_materialised_flipped_copies(detector):
    model, _, images = detector
    W, H = MODEL_SIZE
    with torch.no_grad():
        got = model.forward_padded_tta(images, _MirroredOnly())
        copies = [img.flip(-1).contiguous() for img in images]
        view = model.forward_padded(model.model.transform(copies)[0].tensors)
        want = ops.tta_merge([view], [(W, H, 1)], [tuple(i.shape[-2:]) for i in images], model.model.roi_heads.nms_thresh,
                             model.model.roi_heads.detections_per_img, None)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    rb, rs, rl, rn, margin = to.merge([_host(view)], [(W, H, 1)], PAGE_SIZES, 0.5, 100, None)    # mirrored back by the oracle's arithmetic
    print("mirrored view: margin", margin, "kept", rn.tolist())
    assert margin >= MARGIN and int(rn.sum()) >= 8
    gb, gs, gl, gn = _host(got)
    assert gb.tobytes() == rb.tobytes() and gs.tobytes() == rs.tobytes() and np.array_equal(gl, rl) and np.array_equal(gn, rn)


TWO_SIZES = [(96, 64), (64, 64)]


@pytest.mark.parametrize("vote_thresh", [None, 0.7])
def test_two_sizes_and_flip_equal_the_oracle_on_the_views(detector, vote_thresh):
    model, _, images = detector
    tta = TestTimeAugment(sizes=TWO_SIZES, flip=True, vote_thresh=vote_thresh)
    views = tta.views(model)
    assert views == [(96, 64, 0), (64, 64, 0), (96, 64, 1), (64, 64, 1)]
    outs = view_outputs(model, images, views)
    rb, rs, rl, rn, margin = to.merge(outs, views, PAGE_SIZES, 0.5, 100, vote_thresh)
    print(f"two sizes x flip, vote={vote_thresh}: margin {margin:.3e}, per-view counts {[o[3].tolist() for o in outs]}, kept {rn.tolist()}")
    assert margin >= MARGIN, "the pages decide a pair too close to a threshold: pick another PAGE_SEED"
    with torch.no_grad():
        gb, gs, gl, gn = _host(model.forward_padded_tta(images, tta))
    assert int(rn.sum()) >= 8
    np.testing.assert_array_equal(gn, rn)
    np.testing.assert_array_equal(gl, rl)
    assert gs.tobytes() == rs.tobytes()
    if vote_thresh is None:
        assert gb.tobytes() == rb.tobytes()
    else:
        _within_one_ulp(gb, rb)


def test_evaluate_with_one_plain_view_returns_the_same_numbers(detector):
    model, _, images = detector
    with torch.no_grad():
        first = model(images)
    assert sum(len(o["scores"]) for o in first) >= 8
    targets = [{"boxes": o["boxes"][::2] + 3.0, "labels": o["labels"][::2]} for o in first]
    batches = [(images[:2], targets[:2]), (images[2:], targets[2:])]
    plain = evaluate(model, batches)
    got = evaluate(model, batches, tta=TestTimeAugment(flip=False))
    assert len(got) == 12 and got == plain and got["AR100"] > 0
    small = CocoBoxEvaluator(5, 3, 50, 64, device=DEV)
    with pytest.raises(ValueError, match="max_dets"):
        evaluate(model, batches, evaluator=small, tta=TestTimeAugment(flip=False))
    assert evaluate(model, batches, evaluator=small, tta=TestTimeAugment(flip=False, detections_per_img=50))["AR100"] > 0


def test_uint8_interleaved_pages_give_the_bits_of_their_fp32_lists(detector):
    model, pages, images = detector
    tta = TestTimeAugment(sizes=TWO_SIZES, flip=True, vote_thresh=0.7)
    u8 = [p.to(DEV).permute(2, 0, 1) for p in pages]                                   # [h, w, 3] on the device, read in place
    assert [tuple(t.shape) for t in u8] == [(3, h, w) for h, w in PAGE_SIZES] and not u8[0].is_contiguous()
    with torch.no_grad():
        want, got = model.forward_padded_tta(images, tta), model.forward_padded_tta(u8, tta)
    assert int(want[3].sum()) >= 8
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_train_mode_is_refused(detector):
    model, _, images = detector
    model.train()
    try:
        with pytest.raises(RuntimeError, match="forward_padded_tta is inference only"):
            model.forward_padded_tta(images, TestTimeAugment())
        with pytest.raises(RuntimeError, match="inference only"):
            model(images, tta=TestTimeAugment())
    finally:
        model.eval()
