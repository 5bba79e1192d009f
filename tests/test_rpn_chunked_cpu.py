"""CPU-only checks of the chunked RPN kernels' boundary (ldit_rpn_topk_chunked_f32, ldit_rpn_targets_chunked_f32): both are
declared, exported and validate their arguments without a device; their limits (2^20 anchors, k <= 8192, batch size <= 4096,
512 GT boxes) are refused with the number in the message while the old entry points keep refusing 16 385; the detector takes its
input size as an argument and is unchanged by default.  No kernel is launched here."""
import ctypes as C
import os
import re

from layoutdit_amd import _lib, ops
from layoutdit_amd import config as cfgs
from layoutdit_amd.modeling import LayoutDetectionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_rpn_topk_chunked_f32", "ldit_rpn_targets_chunked_f32")
MAX_N = 1 << 20


def _err():
    return _lib.load().ldit_last_error().decode()


def _targets(fn, anchors=16, gt=16, cnt=16, keys=16, B=2, N=100000, G=8, fg=0.7, bg=0.3, bs=256, frac=0.5, lab=16, mat=16, reg=16, smp=16):
    return fn(anchors, gt, cnt, keys, B, N, G, fg, bg, bs, frac, lab, mat, reg, smp, None)


def test_header_declares_and_library_exports_the_chunked_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert _lib.SIGNATURES["ldit_rpn_topk_chunked_f32"] == _lib.SIGNATURES["ldit_rpn_topk_f32"]          # same arguments
    assert _lib.SIGNATURES["ldit_rpn_targets_chunked_f32"] == _lib.SIGNATURES["ldit_rpn_targets_f32"]
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6   # purely additive
    assert ops.RPN_SORT_SLOTS == 16384


def test_null_and_misaligned_arguments_are_refused():
    lib = _lib.load()
    topk = lib.ldit_rpn_topk_chunked_f32
    sizes = (C.c_int64 * 5)(76800, 19200, 4800, 1200, 300)
    assert topk(None, sizes, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL and "null" in _err()
    assert topk(16, None, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL and "null" in _err()
    assert topk(16, sizes, 5, 2, 1000, None, None) == _lib.LDIT_EINVAL and "null" in _err()
    assert topk(8, sizes, 5, 2, 1000, 16, None) == _lib.LDIT_EINVAL and "aligned" in _err()
    assert topk(16, sizes, 5, 2, 1000, 8, None) == _lib.LDIT_EINVAL and "aligned" in _err()
    assert topk(16, sizes, 5, 2, 0, 16, None) == _lib.LDIT_EINVAL
    assert topk(16, (C.c_int64 * 2)(16, 0), 2, 2, 4, 16, None) == _lib.LDIT_EINVAL
    assert topk(16, (C.c_int64 * 9)(*([8] * 9)), 9, 2, 4, 16, None) == _lib.LDIT_EUNSUPPORTED and "levels" in _err()
    tg = lib.ldit_rpn_targets_chunked_f32
    for name in ("anchors", "gt", "cnt", "keys", "lab", "mat", "reg", "smp"):
        assert _targets(tg, **{name: None}) == _lib.LDIT_EINVAL and "null" in _err(), name
        assert _targets(tg, **{name: 8}) == _lib.LDIT_EINVAL and "aligned" in _err(), name
    assert _targets(tg, B=0) == _lib.LDIT_EINVAL and _targets(tg, N=0) == _lib.LDIT_EINVAL and _targets(tg, G=0) == _lib.LDIT_EINVAL
    assert _targets(tg, fg=0.3, bg=0.7) == _lib.LDIT_EINVAL and "bg" in _err()
    assert _targets(tg, bs=0) == _lib.LDIT_EINVAL and "batch_size" in _err()
    for frac in (0.0, 1.5, float("nan")):
        assert _targets(tg, frac=frac) == _lib.LDIT_EINVAL and "positive_fraction" in _err(), frac


def test_limits_are_refused_with_the_number_in_the_message():
    lib = _lib.load()
    topk = lib.ldit_rpn_topk_chunked_f32
    assert topk(16, (C.c_int64 * 2)(MAX_N + 1, 48), 2, 2, 1000, 16, None) == _lib.LDIT_EUNSUPPORTED and str(MAX_N) in _err()
    assert topk(16, (C.c_int64 * 2)(MAX_N, 48), 2, 2, 8193, 16, None) == _lib.LDIT_EUNSUPPORTED and "8192" in _err()
    tg = lib.ldit_rpn_targets_chunked_f32
    assert _targets(tg, N=MAX_N + 1) == _lib.LDIT_EUNSUPPORTED and str(MAX_N) in _err()
    assert _targets(tg, bs=4097) == _lib.LDIT_EUNSUPPORTED and "4096" in _err()
    assert _targets(tg, G=513) == _lib.LDIT_EUNSUPPORTED and "512" in _err()
    # the old entry points keep their limit
    assert lib.ldit_rpn_topk_f32(16, (C.c_int64 * 2)(16385, 48), 2, 2, 1000, 16, None) == _lib.LDIT_EUNSUPPORTED and "16384" in _err()
    assert _targets(lib.ldit_rpn_targets_f32, N=16385) == _lib.LDIT_EUNSUPPORTED and "16384" in _err()


def test_detector_takes_its_input_size_and_keeps_the_default():
    cfg = cfgs.vit_micro()
    default = LayoutDetectionModel(config=cfg)
    t = default.model.transform
    assert (t.out_h, t.out_w) == (224, 224)
    big = LayoutDetectionModel(config=cfg, fixed_size=(320, 320))
    t = big.model.transform
    assert (t.out_h, t.out_w) == (320, 320)
    wide = LayoutDetectionModel(config=cfg, fixed_size=(384, 288)).model.transform       # (width, height), as torchvision
    assert (wide.out_h, wide.out_w) == (288, 384)
    assert list(big.state_dict()) == list(default.state_dict())
    assert all(tuple(a.shape) == tuple(b.shape) for a, b in zip(big.state_dict().values(), default.state_dict().values()))
