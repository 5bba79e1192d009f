"""CPU-only checks of train-time augmentation: the numpy oracle of the target kernel (tests/augment_oracle.py)
against the code the project already trusts and at its edges; the window sampler; the host-side validation of windows in ``ops`` and in
the C ABI (both run before any launch); the new entry points declared and exported.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib, ops
from layoutdit_amd.augment import DetectorAugment, whole_page_windows
from layoutdit_amd.modeling.detector_input import resize_boxes
from tests import augment_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_preprocess_win_f32", "ldit_preprocess_win_f16", "ldit_preprocess_win_u8", "ldit_augment_targets_f32")
f = np.float32


def _boxes_in_page(rng, G, h, w, grid=None):
    """G random boxes inside an h x w page, at least 2 pixels a side; ``grid``: coordinates on multiples of it."""
    x = np.sort(rng.uniform(0, w, (G, 2)), axis=1)
    y = np.sort(rng.uniform(0, h, (G, 2)), axis=1)
    b = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)
    if grid:
        b = np.round(b / grid) * grid
    b[:, 2] = np.minimum(np.maximum(b[:, 2], b[:, 0] + 2), w)
    b[:, 0] = np.minimum(b[:, 0], b[:, 2] - 2)
    b[:, 3] = np.minimum(np.maximum(b[:, 3], b[:, 1] + 2), h)
    b[:, 1] = np.minimum(b[:, 1], b[:, 3] - 2)
    return b.astype(f)


# ---- oracle properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page,size", [((792, 612), (224, 224)), ((37, 53), (96, 160)), ((1000, 333), (224, 224))])
def test_whole_page_windows_reproduce_resize_boxes_bit_for_bit(page, size):
    h, w = page
    boxes = _boxes_in_page(np.random.default_rng(3), 40, h, w)
    keep, out = ao.kept_rows(boxes, (0, 0, w, h, 0), size, min_visibility=0.3, min_size=0.0)
    assert keep.all()
    ref = resize_boxes(torch.from_numpy(boxes), (h, w), size).numpy()
    assert ref.dtype == f and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    ob, ol, oc = ao.augment_targets(boxes[None], np.arange(1, 41, dtype=np.int32)[None], [40], [(0, 0, w, h, 0)], size, min_size=0.0)
    assert oc.tolist() == [40] and np.array_equal(ob[0], ref) and ol[0].tolist() == list(range(1, 41))


def test_flipping_twice_is_the_identity_on_quarter_pixel_coordinates():
    """Quarter-pixel coordinates below 2^12 and integer windows: every subtraction is exact, so mirroring in the window and mirroring
    the result again in the mirrored frame gives the boxes back.  The batch is the window (ratios 1), so nothing is scaled."""
    rng = np.random.default_rng(5)
    h, w = 600, 480
    win = (17, 40, 301, 222, 1)
    boxes = _boxes_in_page(rng, 64, h, w, grid=0.25)
    boxes[:, [0, 2]] = np.clip(boxes[:, [0, 2]], win[0], win[0] + win[2])            # inside the window: nothing is clipped
    boxes[:, [1, 3]] = np.clip(boxes[:, [1, 3]], win[1], win[1] + win[3])
    size = (win[3], win[2])
    _, once = ao.kept_rows(boxes, win, size, 0.0, 0.0)
    _, twice = ao.kept_rows(once, (0, 0, win[2], win[3], 1), size, 0.0, 0.0)
    _, plain = ao.kept_rows(boxes, win[:4] + (0,), size, 0.0, 0.0)
    assert np.array_equal(twice, plain)
    assert np.array_equal(once[:, 0], f(win[2]) - plain[:, 2]) and np.array_equal(once[:, 1], plain[:, 1])
    assert (once[:, 2] >= once[:, 0]).all()


def test_kept_rows_keep_their_order_and_padding_is_zero():
    rng = np.random.default_rng(7)
    B, Gmax, size = 3, 33, (224, 224)
    boxes = np.stack([_boxes_in_page(rng, Gmax, 400, 300) for _ in range(B)])
    labels = rng.integers(1, 6, (B, Gmax)).astype(np.int32)
    count = [33, 20, 0]
    boxes[1, 20:] = np.nan                                                            # behind the count: never read
    labels[1, 20:] = -1
    wins = [(50, 60, 200, 250, 0), (0, 0, 150, 400, 1), (10, 10, 20, 20, 0)]
    ob, ol, oc = ao.augment_targets(boxes, labels, count, wins, size)
    assert 0 < oc[0] < 33 and 0 < oc[1] < 20 and oc[2] == 0                           # something dropped, something kept
    for i in range(B):
        keep, out = ao.kept_rows(boxes[i, :count[i]], wins[i], size)
        idx = np.flatnonzero(keep)
        assert (np.diff(idx) > 0).all() and np.array_equal(ob[i, :oc[i]], out[idx]) and np.array_equal(ol[i, :oc[i]], labels[i, idx])
        assert not ob[i, oc[i]:].any() and not ol[i, oc[i]:].any()
    assert np.isfinite(ob).all() and (ol >= 0).all()


# ---- oracle edge cases -----------------------------------------------------------------------------------------------------------------
def test_oracle_edges_empty_outside_and_touching():
    size, win = (64, 64), (10, 20, 30, 40, 0)                                         # x [10, 40), y [20, 60)
    ob, ol, oc = ao.augment_targets(np.full((1, 4, 4), np.nan, f), np.full((1, 4), -1, np.int32), [0], [win], size)
    assert oc.tolist() == [0] and not ob.any() and not ol.any()                       # gt_count = 0: NaN rows never read
    outside = np.array([[0, 0, 9, 19], [41, 61, 50, 70], [0, 25, 5, 30], [12, 0, 20, 10]], f)
    touching = np.array([[0, 25, 10, 50],      # right edge on the window's left edge: iw == 0
                         [40, 25, 55, 50],     # left edge on the window's right edge
                         [15, 5, 30, 20],      # bottom edge on the window's top edge: ih == 0
                         [15, 60, 30, 70]], f)
    inside = np.array([[12, 22, 38, 58]], f)
    for group in (outside, touching):
        keep, _ = ao.kept_rows(group, win, size, min_visibility=0.0, min_size=0.0)
        assert not keep.any()
    keep, out = ao.kept_rows(np.concatenate([outside, inside, touching]), win, size, 0.0, 0.0)
    assert keep.tolist() == [False] * 4 + [True] + [False] * 4
    rw, rh = f(64.0 / 30.0), f(64.0 / 40.0)
    assert np.array_equal(out[4], np.array([f(2) * rw, f(2) * rh, f(28) * rw, f(38) * rh], f))
    # visibility: a box half inside is kept at 0.5 and dropped just above it; the size filter acts on the batch's pixels
    half = np.array([[0, 30, 20, 40]], f)                                             # 10 of its 20 columns visible
    assert ao.kept_rows(half, win, size, 0.5, 0.0)[0].tolist() == [True]
    assert ao.kept_rows(half, win, size, 0.51, 0.0)[0].tolist() == [False]
    small = np.array([[12, 22, 12.4, 30]], f)                                         # 0.4 px wide in the page, 0.853 in the batch
    assert ao.kept_rows(small, win, size, 0.0, 1.0)[0].tolist() == [False] and ao.kept_rows(small, win, size, 0.0, 0.85)[0].tolist() == [True]


# ---- DetectorAugment.sample --------------------------------------------------------------------------------------------------------------
def _valid(win, h, w):
    x0, y0, cw, ch, flip = win
    return all(isinstance(v, int) for v in win) and cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0 and x0 + cw <= w and y0 + ch <= h and flip in (0, 1)


def test_sampled_windows_are_valid_for_every_page_size():
    sizes = [(1, 1), (1, 7), (9, 1), (2, 2), (3, 5), (37, 53), (224, 224), (792, 612), (2000, 3000), (3000, 2000)]
    for aug in (DetectorAugment(seed=1, flip_prob=0.5), DetectorAugment(scale=(0.05, 1.0), ratio=(0.2, 5.0), seed=2, flip_prob=0.5),
                DetectorAugment(scale=(1.0, 1.0), ratio=(1.0, 1.0), seed=3)):
        seen_flip, seen_crop = set(), False
        for _ in range(40):
            wins = aug.sample(sizes)
            assert len(wins) == len(sizes)
            for (h, w), win in zip(sizes, wins):
                assert _valid(win, h, w), (win, h, w)
                seen_flip.add(win[4])
                seen_crop |= (win[2], win[3]) != (w, h)
        assert seen_flip == ({0, 1} if aug.flip_prob else {0})
        assert seen_crop == (aug.scale != (1.0, 1.0))
    # the area and the aspect are what the arguments say, up to the rounding to integers
    aug = DetectorAugment(scale=(0.25, 0.25), ratio=(1.0, 1.0), seed=4)
    assert all(w[2:4] == (1500, 1000) for w in aug.sample([(2000, 3000)] * 5))
    aug = DetectorAugment(scale=(0.5, 1.0), seed=5)
    shares = [w[2] * w[3] / (792 * 612) for w in aug.sample([(792, 612)] * 200)]
    assert 0.45 < min(shares) and max(shares) <= 1.0 and 0.65 < np.mean(shares) < 0.85
    with pytest.raises(ValueError, match="scale"):
        DetectorAugment(scale=(0.5, 1.5))
    with pytest.raises(ValueError, match="page 1"):
        aug.sample([(4, 4), (0, 3)])


def test_sampler_is_a_pure_function_of_seed_state_and_sizes():
    sizes = [(792, 612), (600, 800), (37, 53)]
    a, b = DetectorAugment(seed=7, flip_prob=0.5), DetectorAugment(seed=7, flip_prob=0.5)
    first = [a.sample(sizes) for _ in range(3)]
    assert first == [b.sample(sizes) for _ in range(3)]
    assert first[0] != first[1] and DetectorAugment(seed=8, flip_prob=0.5).sample(sizes) != first[0]
    whole = DetectorAugment(crop_prob=0.0, flip_prob=0.0, seed=7)
    assert whole.sample(sizes) == whole_page_windows(sizes) == [(0, 0, 612, 792, 0), (0, 0, 800, 600, 0), (0, 0, 53, 37, 0)]
    # a state_dict round trip continues the stream; the state is a copy, not a view of the live generator
    sd = a.state_dict()
    ahead = [a.sample(sizes) for _ in range(2)]
    c = DetectorAugment(seed=99, flip_prob=0.5)
    c.load_state_dict(sd)
    assert [c.sample(sizes) for _ in range(2)] == ahead
    c.load_state_dict(sd)
    assert c.sample(sizes) == ahead[0]


# ---- validation, before any launch ---------------------------------------------------------------------------------------------------
BAD_WINDOWS = [
    ([(0, 0, 8, 8, 0), (3, 0, 6, 8, 0)], r"windows\[1\].*leaves images\[1\]"),         # x0 + cw > w
    ([(0, 0, 8, 8, 0), (0, 5, 8, 4, 0)], r"windows\[1\].*leaves images\[1\]"),         # y0 + ch > h
    ([(0, 0, 8, 8, 0), (0, 0, 0, 8, 0)], r"windows\[1\].*images\[1\].*at least 1"),    # cw = 0
    ([(0, 0, 8, -2, 0), (0, 0, 8, 8, 0)], r"windows\[0\].*images\[0\].*at least 1"),   # ch < 0
    ([(0, 0, 8, 8, 0), (-1, 0, 4, 4, 0)], r"windows\[1\].*images\[1\].*negative"),
    ([(0, 0, 8, 8, 0), (0, 0, 8, 8, 2)], r"windows\[1\].*flip = 2.*images\[1\]"),
    ([(0, 0, 8, 8, 0), (0, 0, 8, 8, -1)], r"windows\[1\].*flip = -1"),
    ([(0, 0, 8, 8, 0), (0, 0, 8, 8)], r"windows\[1\].*images\[1\].*five integers"),    # wrong shape of a row
    ([(0, 0, 8, 8, 0), (0, 0, 7.5, 8, 0)], r"windows\[1\].*five integers"),            # no fractional windows
    ([(0, 0, 8, 8, 0)], r"1 windows for 2 images"),                                     # wrong number of rows
]


@pytest.mark.parametrize("windows,message", BAD_WINDOWS)
def test_ops_refuse_bad_windows_naming_the_image(windows, message):
    images = [torch.zeros(3, 8, 8), torch.zeros(3, 8, 8)]                              # CPU tensors: the windows are checked first
    with pytest.raises(ValueError, match=message):
        ops.preprocess(images, size=32, windows=windows)
    if "leaves" not in message:                                                         # the target side does not know the pages
        with pytest.raises(ValueError, match=message):
            ops.augment_targets(torch.zeros(2, 4, 4), None, torch.zeros(2, dtype=torch.int32), windows, 32)


def test_ops_window_forms_and_remaining_refusals():
    good = [(0, 0, 8, 8, 0), (1, 2, 3, 4, 1)]
    arr = ops.window_args(torch.tensor(good, dtype=torch.int32), 2, [(8, 8), (8, 8)])
    assert list(arr) == [0, 0, 8, 8, 0, 1, 2, 3, 4, 1] == list(ops.window_args(np.asarray(good), 2))
    with pytest.raises(ValueError, match="int32 on the CPU"):
        ops.window_args(torch.tensor(good, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match=r"\[2, 5\]"):
        ops.window_args(torch.zeros(10, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match=r"windows\[0\].*five integers"):
        ops.window_args(torch.zeros((2, 4), dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="GPU"):                                       # good windows: the next refusal is the CPU tensor
        ops.preprocess([torch.zeros(3, 8, 8)] * 2, size=32, windows=good)
    with pytest.raises(ValueError, match="GPU"):
        ops.augment_targets(torch.zeros(2, 4, 4), None, torch.zeros(2, dtype=torch.int32), good, 32)
    with pytest.raises(ValueError, match="Gmax, 4"):
        ops.augment_targets(torch.zeros(2, 4), None, torch.zeros(2, dtype=torch.int32), good, 32)


def test_c_entries_validate_windows_and_arguments_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                        # noqa: E731
    ptrs, hs, ws = (C.c_void_p * 2)(4096, 8192), (C.c_int32 * 2)(8, 8), (C.c_int32 * 2)(8, 8)

    def win(*rows):
        return (C.c_int32 * 10)(*[v for r in rows for v in r])

    ok = (0, 0, 8, 8, 0)
    for bad, word in (((3, 0, 6, 8, 0), "leaves"), ((0, 5, 8, 4, 0), "leaves"), ((0, 0, 0, 8, 0), "at least"), ((0, 0, 8, -1, 0), "at least"),
                      ((-1, 0, 4, 4, 0), "negative"), ((0, 0, 8, 8, 2), "flip")):
        for entry in (lib.ldit_preprocess_win_f32, lib.ldit_preprocess_win_f16):
            assert entry(ptrs, hs, ws, win(ok, bad), 2, 3, 0.5, 0.5, 32, 32, 4096, None) == _lib.LDIT_EINVAL
            assert "image 1" in err() and word in err(), (bad, err())
        for interleaved in (0, 1):
            assert lib.ldit_preprocess_win_u8(ptrs, hs, ws, win(bad, ok), interleaved, 2, 3, 0.5, 0.5, 32, 32, 4096, None) == _lib.LDIT_EINVAL
            assert "image 0" in err() and word in err()
        if word != "leaves":
            assert lib.ldit_augment_targets_f32(16, 16, 16, win(ok, bad), 2, 4, 32, 32, 0.3, 1.0, 32, 32, 32, None) == _lib.LDIT_EINVAL
            assert "image 1" in err() and word in err()
    assert lib.ldit_preprocess_win_u8(ptrs, hs, ws, win(ok, ok), 2, 2, 3, 0.5, 0.5, 32, 32, 4096, None) == _lib.LDIT_EINVAL and "interleaved" in err()
    assert lib.ldit_preprocess_win_f32(ptrs, hs, ws, win(ok, ok), 2, 3, 0.5, 0.5, 32, 32, None, None) == _lib.LDIT_EINVAL and "null" in err()
    assert lib.ldit_preprocess_win_f32(ptrs, hs, ws, None, 2, 3, 0.5, 0.5, 32, 32, None, None) == _lib.LDIT_EINVAL and "null" in err()
    aug = lib.ldit_augment_targets_f32

    def targets(gt=16, gtl=16, cnt=16, w=win(ok, ok), B=2, G=4, oh=32, ow=32, mv=0.3, ms=1.0, ob=32, ol=32, oc=48):
        return aug(gt, gtl, cnt, w, B, G, oh, ow, mv, ms, ob, ol, oc, None)

    for name in ("gt", "cnt", "w", "ob", "oc"):
        assert targets(**{name: None}) == _lib.LDIT_EINVAL and "null" in err(), name
    assert targets(gtl=16, ol=None) == _lib.LDIT_EINVAL and "out_labels" in err()
    assert targets(gt=8) == _lib.LDIT_EINVAL and "aligned" in err() and targets(ob=8) == _lib.LDIT_EINVAL
    assert targets(B=0) == _lib.LDIT_EINVAL and targets(G=0) == _lib.LDIT_EINVAL and targets(oh=0) == _lib.LDIT_EINVAL
    assert targets(G=513) == _lib.LDIT_EUNSUPPORTED and "512" in err() and ops.RPN_TARGETS_MAX_GT == 512
    assert targets(mv=-0.1) == _lib.LDIT_EINVAL and targets(ms=float("nan")) == _lib.LDIT_EINVAL and "min_size" in err()
    assert targets(ob=16) == _lib.LDIT_EINVAL and "alias" in err()


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_augmentation_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # siblings: the windowed entries take their sibling's arguments plus the windows, right behind the widths
    for kind in ("f32", "f16", "u8"):
        old, new = _lib.SIGNATURES["ldit_preprocess_" + kind], _lib.SIGNATURES["ldit_preprocess_win_" + kind]
        assert new[0] is old[0] and new[1][:3] == old[1][:3] and new[1][4:] == old[1][3:]
    assert lib.ldit_abi_version() == _lib.LDIT_ABI_VERSION                              # purely additive: the version stays


def test_python_surface_defaults_change_nothing():
    import inspect
    from layoutdit_amd.detector_training import DetectorTrainStep
    from layoutdit_amd.modeling import DetectorInputTransform, LayoutDetectionModel
    for fn, name in ((ops.preprocess, "windows"), (DetectorInputTransform.forward, "windows"), (LayoutDetectionModel.losses, "windows"),
                     (LayoutDetectionModel.rpn_losses, "windows"), (DetectorTrainStep.step, "windows"), (DetectorTrainStep.__init__, "augment")):
        assert inspect.signature(fn).parameters[name].default is None, fn
    sig = inspect.signature(DetectorAugment.__init__).parameters
    assert (sig["scale"].default, sig["crop_prob"].default, sig["flip_prob"].default, sig["min_visibility"].default, sig["min_size"].default,
            sig["seed"].default) == ((0.5, 1.0), 1.0, 0.0, 0.3, 1.0, 0)
    assert sig["ratio"].default == (3 / 4, 4 / 3)
    assert "windows" not in inspect.signature(LayoutDetectionModel.forward).parameters
    assert "windows" not in inspect.signature(LayoutDetectionModel.forward_padded).parameters
