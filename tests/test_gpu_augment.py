"""Train-time augmentation on the GPU (csrc/misc.hip: preprocess_windows, csrc/augment.hip through the C ABI; ops, DetectorInputTransform,
LayoutDetectionModel.losses, DetectorTrainStep).  Every gate is an equality: the windowed input transform against
the existing entry on the materialised crop, the target kernel against the numpy oracle tests/augment_oracle.py, the detector's losses
and gradients under windows against the same model on the cropped pages, a train step with an augment against its own repetition."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import ops                                            # noqa: E402
from layoutdit_amd.augment import DetectorAugment, whole_page_windows   # noqa: E402
from layoutdit_amd.training import DetectorTrainStep                     # noqa: E402
from tests import augment_oracle as ao                                   # noqa: E402
from tests import detector_accum_cases as cases                          # noqa: E402
from tests import guarded                                                # noqa: E402

DEV = "cuda:0"
FORMATS = ("f32", "f16", "u8", "u8_hwc")
PAGES = ((37, 53), (64, 48), (5, 7), (1, 1))                              # h x w
SIZES = ((32, 32), (20, 30))                                              # out_h x out_w; 30: the out_w % 4 tail
SCALE = 1024.0


# ---- pixels --------------------------------------------------------------------------------------------------------------------------
def _codes(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, h, w), dtype=np.uint8)


def _page(codes, fmt):
    """The page of uint8 ``codes`` [3, h, w] on the device in one of the four formats; the interleaved one starts at byte 1 of its
    allocation (any alignment is accepted)."""
    t = torch.from_numpy(codes)
    if fmt == "u8":
        return t.to(DEV)
    if fmt == "u8_hwc":
        _, h, w = codes.shape
        store = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=DEV)
        store[1:].view(h, w, 3).copy_(t.permute(1, 2, 0))
        return store[1:].view(h, w, 3).permute(2, 0, 1)
    x = t.to(DEV).float() / 255.0
    return x.half() if fmt == "f16" else x


def _crop(page, window, fmt):
    """The materialised window: a fresh tensor in the page's own format and layout."""
    c = ao.crop_image(page, window)
    if fmt == "u8_hwc":
        return c.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    return c.contiguous()


def _windows_of(h, w):
    """The window cases of one page: whole (plain and mirrored), one column, one row, a window abutting each edge, odd and even widths
    under flip - those that fit the page."""
    cand = [(0, 0, w, h, 0), (0, 0, w, h, 1), (w // 2, 0, 1, h, 0), (w - 1, 0, 1, h, 1), (0, h // 2, w, 1, 0), (0, h - 1, w, 1, 1),
            (0, 1, w - 2, h - 2, 0), (2, 1, w - 2, h - 2, 0), (1, 0, w - 2, h - 2, 1), (1, 2, w - 2, h - 2, 0),
            (1, 1, 3, h - 2, 1), (1, 1, 4, h - 2, 1), (w - 5, h - 3, 5, 3, 1), (w - 6, 0, 6, 2, 1)]
    out = []
    for x0, y0, cw, ch, flip in cand:
        if cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0 and x0 + cw <= w and y0 + ch <= h and (x0, y0, cw, ch, flip) not in out:
            out.append((x0, y0, cw, ch, flip))
    return out


def _pixel_cases():
    pages, windows = [], []
    for k, (h, w) in enumerate(PAGES):
        for win in _windows_of(h, w):
            pages.append((h, w, 100 + k))
            windows.append(win)
    return pages, windows


def test_window_cases_cover_what_they_claim():
    wins = _windows_of(37, 53)
    assert len(wins) == 14 and len(_windows_of(1, 1)) == 2 and len(_windows_of(5, 7)) >= 12
    assert any(w[2] == 1 for w in wins) and any(w[3] == 1 for w in wins)
    assert {w[2] % 2 for w in wins if w[4]} == {0, 1}
    assert any(w[0] == 0 and w[2] < 53 for w in wins) and any(w[0] + w[2] == 53 and w[0] > 0 for w in wins)
    assert any(w[1] == 0 and w[3] < 37 for w in wins) and any(w[1] + w[3] == 37 and w[1] > 0 for w in wins)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_windowed_transform_equals_the_entry_on_the_materialised_crop(fmt, size):
    pages, windows = _pixel_cases()
    images = [_page(_codes(h, w, seed), fmt) for h, w, seed in pages]
    got = ops.preprocess(images, size=size, windows=windows)
    ref = ops.preprocess([_crop(img, win, fmt) for img, win in zip(images, windows)], size=size)
    assert got.shape == (len(images), 3) + size and torch.equal(got, ref)
    assert torch.equal(ops.preprocess(images, size=size, windows=torch.tensor(windows, dtype=torch.int32)), ref)


@pytest.mark.parametrize("fmt", FORMATS)
def test_second_launch_chunk_has_its_own_windows(fmt):
    """B = 50 > 48 images per launch: the images of the second launch (first = 48) read THEIR windows."""
    rng = np.random.default_rng(11)
    images = [_page(_codes(8, 8, 200 + i), fmt) for i in range(50)]
    windows = []
    for i in range(50):
        cw, ch = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        windows.append((int(rng.integers(0, 9 - cw)), int(rng.integers(0, 9 - ch)), cw, ch, int(rng.integers(0, 2))))
    windows[48], windows[49] = (1, 2, 5, 3, 1), (3, 0, 4, 8, 0)
    assert len(set(windows)) > 40
    got = ops.preprocess(images, size=(20, 30), windows=windows)
    ref = ops.preprocess([_crop(img, win, fmt) for img, win in zip(images, windows)], size=(20, 30))
    assert torch.equal(got, ref)


# ---- window isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_pixels_outside_the_window_do_not_reach_the_output(fmt):
    pages, windows = _pixel_cases()
    codes = [_codes(h, w, seed) for h, w, seed in pages]
    other = []
    for c, (x0, y0, cw, ch, _) in zip(codes, windows):
        o = (c.astype(np.int32) * 7 + 91).astype(np.uint8)                  # another value at every pixel (a bijection of the codes)
        assert (o != c).all()
        o[:, y0:y0 + ch, x0:x0 + cw] = c[:, y0:y0 + ch, x0:x0 + cw]
        other.append(o)
    a = ops.preprocess([_page(c, fmt) for c in codes], size=(20, 30), windows=windows)
    b = ops.preprocess([_page(o, fmt) for o in other], size=(20, 30), windows=windows)
    assert torch.equal(a, b)


@pytest.mark.parametrize("fmt", FORMATS)
def test_abutting_windows_read_nothing_outside_the_page(fmt):
    """tests/guarded.py: the page inside 0x00 and then 0xFF guard bands, identical geometry; windows that abut each edge of the page
    (and the whole page, which abuts all four) must give the same bits, and those of the materialised crop."""
    h, w = 9, 13
    codes = _codes(h, w, 300)
    data = {"f32": torch.from_numpy(codes).float() / 255.0, "f16": (torch.from_numpy(codes).float() / 255.0).half(),
            "u8": torch.from_numpy(codes), "u8_hwc": torch.from_numpy(codes)}[fmt]
    strides = (1, w * 3, 3) if fmt == "u8_hwc" else None
    for win in ((0, 0, w, h, 0), (0, 2, 5, 4, 1), (w - 6, 3, 6, 5, 0), (3, 0, 7, 2, 1), (2, h - 3, 8, 3, 0), (w - 1, h - 1, 1, 1, 0)):
        specs = {"page": guarded.In(data, strides=strides), "out": guarded.Out((1, 3, 20, 30))}
        res = guarded.twin_run(specs, lambda v: v["out"].copy_(ops.preprocess([v["page"]], size=(20, 30), windows=[win])), device=DEV,
                               sync=torch.cuda.synchronize)
        page = _page(codes, fmt) if fmt.startswith("u8") else data.to(DEV)        # the guarded page's own values (host-made quotients)
        ref = ops.preprocess([_crop(page, win, fmt)], size=(20, 30)).cpu()
        assert torch.equal(res.clean["out"], ref) and torch.equal(res.poisoned["out"], ref), win
        guarded.assert_finite(res.poisoned["out"])


# ---- windows=None ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_no_windows_is_the_old_entry(fmt):
    """``windows == NULL`` at the C ABI and ``windows=None`` in ops: whole pages, the sibling's bits; so are explicit whole-page windows."""
    import ctypes as C
    from layoutdit_amd import _lib
    lib = _lib.load()
    images = [_page(_codes(h, w, 400 + k), fmt) for k, (h, w) in enumerate(PAGES)]
    old = ops.preprocess(images, size=(20, 30))
    imgs, ptrs, hs, ws, code, ch = ops.image_list_args(images)
    out = torch.full((len(images), 3, 20, 30), float("nan"), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    none = C.POINTER(C.c_int32)()
    if fmt.startswith("u8"):
        rc = lib.ldit_preprocess_win_u8(ptrs, hs, ws, none, int(code == ops.IMG_U8_HWC), len(images), ch, 0.5, 0.5, 20, 30, out.data_ptr(), stream)
    else:
        entry = lib.ldit_preprocess_win_f16 if fmt == "f16" else lib.ldit_preprocess_win_f32
        rc = entry(ptrs, hs, ws, none, len(images), ch, 0.5, 0.5, 20, 30, out.data_ptr(), stream)
    _lib.check(rc)
    assert torch.equal(out, old)
    assert torch.equal(ops.preprocess(images, size=(20, 30), windows=None), old)
    assert torch.equal(ops.preprocess(images, size=(20, 30), windows=whole_page_windows(PAGES)), old)


# ---- targets ------------------------------------------------------------------------------------------------------------------------------------
def _target_problem(B, Gmax, seed):
    """Random fp32 boxes around 300 x 400 pages (outside, partly inside, inside their windows), some on the pixel grid, some with an edge
    exactly on a window's edge (degenerate after clipping); counts include 0 and Gmax; NaN boxes and label -1 behind the counts."""
    rng = np.random.default_rng(seed)
    h, w = 400, 300
    windows = []
    for i in range(B):
        cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        windows.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch, int(rng.integers(0, 2))))
    windows[0] = (0, 0, w, h, 0)
    windows[1] = (40, 60, 101, 150, 1)
    x = np.sort(rng.uniform(-40, w + 40, (B, Gmax, 2)), axis=2)
    y = np.sort(rng.uniform(-40, h + 40, (B, Gmax, 2)), axis=2)
    boxes = np.stack([x[..., 0], y[..., 0], x[..., 1], y[..., 1]], axis=-1).astype(np.float32)
    grid = rng.random((B, Gmax)) < 0.25
    boxes[grid] = np.round(boxes[grid])
    for i, (x0, y0, cw, ch, _) in enumerate(windows):                          # every 5th row touches its window along an edge
        for g in range(i % 5, Gmax, 5):
            side = (i + g) % 4
            if side == 0:
                boxes[i, g, 2] = x0                                               # right edge on the window's left edge: iw == 0
                boxes[i, g, 0] = x0 - 7.5
            elif side == 1:
                boxes[i, g, 0] = x0 + cw
                boxes[i, g, 2] = x0 + cw + 3.25
            elif side == 2:
                boxes[i, g, 3] = y0
                boxes[i, g, 1] = y0 - 2.0
            else:
                boxes[i, g, 1], boxes[i, g, 3] = y0 + ch, y0 + ch + 9.0
    count = rng.integers(0, Gmax + 1, B).astype(np.int32)
    count[0], count[1], count[2] = Gmax, 0, Gmax
    labels = rng.integers(1, 6, (B, Gmax)).astype(np.int32)
    for i in range(B):
        boxes[i, count[i]:] = np.nan
        labels[i, count[i]:] = -1
    return boxes, labels, count, windows


@pytest.mark.parametrize("B", [3, 50])
@pytest.mark.parametrize("Gmax", [1, 63, 64, 65, 130])
def test_targets_equal_the_oracle(Gmax, B, monkeypatch):
    boxes, labels, count, windows = _target_problem(B, Gmax, seed=1000 + 7 * Gmax + B)
    size = (224, 160)
    eb, el, ec = ao.augment_targets(boxes, labels, count, windows, size)
    args = (torch.from_numpy(boxes).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(count).to(DEV))
    with guarded.fresh_memory(monkeypatch, guarded.CANARY):                        # the outputs hold 0xA5 in every byte before the launch
        probe = torch.empty(4, dtype=torch.int32, device=DEV)
        gb, gl, gc = ops.augment_targets(*args, windows, size)
        nb, nl, nc = ops.augment_targets(args[0], None, args[2], windows, size)
    assert (probe.cpu().numpy().view(np.uint8) == guarded.CANARY).all()
    gb, gl, gc = gb.cpu().numpy(), gl.cpu().numpy(), gc.cpu().numpy()
    print(f"Gmax {Gmax} B {B}: kept {int(ec.sum())} of {int(count.sum())} boxes")
    assert np.array_equal(gc, ec) and np.array_equal(gl, el)
    assert np.array_equal(gb.view(np.uint32), eb.view(np.uint32))
    for i in range(B):                                                             # the padding is zero in every BYTE
        assert not gb[i, ec[i]:].view(np.uint32).any() and not gl[i, ec[i]:].any()
    assert nl is None and torch.equal(nb.cpu(), torch.from_numpy(eb)) and np.array_equal(nc.cpu().numpy(), ec)
    if Gmax >= 63:
        assert 0 < ec.sum() < count.sum() and ec[0] > 0                            # some dropped, some kept


def test_default_filters_and_the_two_thresholds_reach_the_kernel():
    boxes, labels, count, windows = _target_problem(3, 64, seed=5)
    args = (torch.from_numpy(boxes).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(count).to(DEV))
    for mv, ms in ((0.0, 0.0), (0.75, 0.0), (0.3, 6.5)):
        eb, el, ec = ao.augment_targets(boxes, labels, count, windows, (96, 160), mv, ms)
        gb, gl, gc = ops.augment_targets(*args, windows, (96, 160), min_visibility=mv, min_size=ms)
        assert np.array_equal(gc.cpu().numpy(), ec) and np.array_equal(gl.cpu().numpy(), el)
        assert np.array_equal(gb.cpu().numpy().view(np.uint32), eb.view(np.uint32))


# ---- capture ------------------------------------------------------------------------------------------------------------------------------------
def test_both_launches_are_graph_capturable():
    pages, windows = _pixel_cases()
    pages, windows = pages[:20], windows[:20]
    images = [_page(_codes(h, w, seed), "u8") for h, w, seed in pages]
    boxes, labels, count, twins = _target_problem(20, 65, seed=77)
    args = [torch.from_numpy(a).to(DEV) for a in (boxes, labels, count)]

    def run():
        return (ops.preprocess(images, size=(20, 30), windows=windows),) + ops.augment_targets(*args, twins, (20, 30))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    # other data behind the same pointers: the replay must read it
    for img, (h, w, seed) in zip(images, pages):
        img.copy_(torch.from_numpy(_codes(h, w, seed + 50)))
    boxes2, labels2, count2, _ = _target_problem(20, 65, seed=78)
    for dst, src in zip(args, (boxes2, labels2, count2)):
        dst.copy_(torch.from_numpy(src))
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    eb, el, ec = ao.augment_targets(boxes2, labels2, count2, twins, (20, 30))
    assert np.array_equal(captured[3].cpu().numpy(), ec) and np.array_equal(captured[1].cpu().numpy().view(np.uint32), eb.view(np.uint32))


# ---- the detector -------------------------------------------------------------------------------------------------------------------------------
LOSSES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")


@pytest.fixture(scope="module")
def model():
    return cases.model()


def test_whole_page_windows_leave_the_losses_alone(model):
    images, targets = cases.micro_batches()[0]
    windows = whole_page_windows([img.shape[-2:] for img in images])
    plain = model.losses(images, targets, generator=cases.seeded(3))
    windowed = model.losses(images, targets, generator=cases.seeded(3), windows=windows)
    assert sorted(plain) == sorted(LOSSES)
    for k in LOSSES:
        assert torch.equal(plain[k], windowed[k]), (k, plain[k].item(), windowed[k].item())
    rpn_plain = model.rpn_losses(images, targets, generator=cases.seeded(3))
    rpn_windowed = model.rpn_losses(images, [{"boxes": t["boxes"]} for t in targets], generator=cases.seeded(3), windows=windows)
    assert all(torch.equal(rpn_plain[k], rpn_windowed[k]) for k in rpn_plain)


def _crop_problem():
    """Three pages, their windows and boxes: the longest list (7 boxes, image 0, mirrored) keeps every box, so the padded width stays 7;
    image 1 loses its rows 1 (outside) and 3 (a sliver visible) from the middle, image 2 its first row."""
    from layoutdit_amd import synth
    rng = np.random.default_rng(21)
    images = [torch.from_numpy(synth.synth_images(1, h, w, seed=s, kind="uniform")[0]).to(DEV) for h, w, s in ((120, 200, 31), (224, 224, 32), (200, 160, 33))]
    windows = [(20, 10, 160, 100, 1), (30, 40, 150, 160, 0), (0, 50, 160, 150, 1)]
    x = np.sort(rng.uniform(22, 178, (7, 2)), axis=1)
    y = np.sort(rng.uniform(12, 108, (7, 2)), axis=1)
    a = np.stack([x[:, 0], y[:, 0], x[:, 0] + np.maximum(x[:, 1] - x[:, 0], 9.0), y[:, 0] + np.maximum(y[:, 1] - y[:, 0], 9.0)], axis=1)
    a[:, 2], a[:, 3] = np.minimum(a[:, 2], 179.5), np.minimum(a[:, 3], 109.5)
    b = np.array([[50.3, 60.1, 120.7, 130.9], [0.5, 1.5, 25.0, 30.0], [10.2, 100.4, 90.6, 150.8], [170.1, 50.2, 222.3, 120.4],
                  [100.9, 150.2, 170.3, 195.6]])
    c = np.array([[10.0, 5.0, 100.0, 45.0], [20.4, 70.3, 90.2, 160.1], [100.6, 30.7, 155.2, 120.9]])
    boxes = [a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)]
    labels = [np.arange(len(bx), dtype=np.int64) % 5 + 1 for bx in boxes]
    return images, windows, boxes, labels


def test_losses_under_windows_equal_the_losses_of_the_crops(model):
    images, windows, boxes, labels = _crop_problem()
    size = (224, 224)
    targets = [{"boxes": torch.from_numpy(bx).to(DEV), "labels": torch.from_numpy(lb).to(DEV)} for bx, lb in zip(boxes, labels)]
    crops, crop_targets, kept = [], [], []
    for img, win, bx, lb in zip(images, windows, boxes, labels):
        keep, cb = ao.crop_boxes(bx, win, size)
        kept.append(keep.tolist())
        crops.append(ao.crop_image(img, win).contiguous())
        crop_targets.append({"boxes": torch.from_numpy(cb[keep]).to(DEV), "labels": torch.from_numpy(lb[keep]).to(DEV)})
    assert kept == [[True] * 7, [True, False, True, False, True], [False, True, True]]
    assert max(len(bx) for bx in boxes) == max(int(t["boxes"].shape[0]) for t in crop_targets) == 7        # the padded width is the same

    def run(*args, **kw):
        for p in model.parameters():
            p.grad = None
        losses = model.losses(*args, generator=cases.seeded(4), **kw)
        sum(losses.values()).backward()
        return {k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    lw, gw = run(images, targets, windows=windows)
    lc, gc = run(crops, crop_targets)
    for k in LOSSES:
        assert torch.equal(lw[k], lc[k]), (k, lw[k].item(), lc[k].item())
    assert all(np.isfinite(v.item()) for v in lw.values()) and lw["loss_classifier"].item() > 0
    assert set(gw) == set(gc) and len(gw) > 30
    assert [n for n in gw if not torch.equal(gw[n], gc[n])] == []
    plain, _ = run(images, targets)
    assert any(not torch.equal(plain[k], lw[k]) for k in LOSSES)                    # the windows did change the problem


# ---- the train step -------------------------------------------------------------------------------------------------------------------------------
GEN_SEEDS = (2, 5, 8)


def _trained(steps, snapshot_after=None, **kw):
    m = cases.model()
    step = DetectorTrainStep(m, lr=1e-3, weight_decay=0.01, init_scale=SCALE, **kw)
    images, targets = cases.micro_batches()[0]
    snap = None
    for i in range(steps):
        step.step(images, targets, generator=cases.seeded(GEN_SEEDS[i]))
        if snapshot_after == i + 1:
            snap = (copy.deepcopy(m.state_dict()), copy.deepcopy(step.state_dict()))
    return m, step, snap


def _same_weights(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return [k for k in sa if not torch.equal(sa[k], sb[k])] == []


def test_train_step_with_an_augment_repeats_and_resumes():
    aug = lambda: DetectorAugment(seed=7, flip_prob=0.5)                              # noqa: E731
    first, step_a, _ = _trained(3, augment=aug())
    second, step_b, snap = _trained(3, snapshot_after=2, augment=aug())
    assert _same_weights(first, second)
    assert step_a.augment.sample([(10, 10)]) == step_b.augment.sample([(10, 10)])      # both generators stand where three draws left them
    assert "augment" in snap[1]
    # resumed after step 2: another process would build the model and the step anew, with whatever seed
    resumed = cases.model()
    resumed.load_state_dict(snap[0])
    step_c = DetectorTrainStep(resumed, lr=1e-3, weight_decay=0.01, init_scale=SCALE, augment=DetectorAugment(seed=1234, flip_prob=0.5))
    step_c.load_state_dict(snap[1])
    images, targets = cases.micro_batches()[0]
    step_c.step(images, targets, generator=cases.seeded(GEN_SEEDS[2]))
    torch.cuda.synchronize()
    assert _same_weights(first, resumed) and step_c.steps == step_a.steps
    # the windows did something: the un-augmented run ends elsewhere
    plain, _, _ = _trained(3)
    assert not _same_weights(first, plain)


def test_train_step_without_an_augment_is_the_old_step():
    with_arg, step_a, _ = _trained(2, augment=None)
    without, step_b, _ = _trained(2)
    assert _same_weights(with_arg, without)
    assert "augment" not in step_a.state_dict() and step_a.state_dict()["state"] == step_b.state_dict()["state"]
    # explicit windows without an augment: the whole pages are the old step too
    images, targets = cases.micro_batches()[0]
    explicit = cases.model()
    step_c = DetectorTrainStep(explicit, lr=1e-3, weight_decay=0.01, init_scale=SCALE)
    for i in range(2):
        step_c.step(images, targets, generator=cases.seeded(GEN_SEEDS[i]), windows=whole_page_windows([img.shape[-2:] for img in images]))
    assert _same_weights(explicit, without)
