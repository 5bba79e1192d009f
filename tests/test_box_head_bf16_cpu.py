"""Host-side checks of the bf16 eval-mode box head (no GPU, no launch): the new entry point and epilogue value exist, the bf16 RoIAlign
entry refuses what the fp32 one refuses, the linear entries without a ReLU epilogue refuse it, and ``head_dtype`` is an option of the
modules that leaves the checkpoint surface alone."""
import ctypes as C
import os
import re

import pytest
import torch

from layoutdit_amd import _lib
from layoutdit_amd.config import DiTConfig
from layoutdit_amd.modeling import FastRCNNPredictor, LayoutDetectionModel, MultiScaleRoIAlign, RoIHeads, TwoMLPHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_epilogue_value_exist():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bldit_roi_align_levels_bf16\s*\(", text)
    assert "ldit_roi_align_levels_bf16" in _lib.SIGNATURES and hasattr(lib, "ldit_roi_align_levels_bf16")
    assert _lib.SIGNATURES["ldit_roi_align_levels_bf16"] == _lib.SIGNATURES["ldit_roi_align_levels_f32"]     # the same arguments
    m = re.search(r"\bLDIT_EPI_BIAS_RELU\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.EPI_BIAS_RELU
    assert _lib.EPI_BIAS_RELU not in (_lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_SCALE_RESID, _lib.EPI_F32, _lib.EPI_GELU_BWD, 3)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6       # purely additive


def _roi_args(L=5, Cc=256, P=7, S=2, maps=None, boxes=16, out=16, k=(2, 6), stride_x=None):
    ptrs = (C.c_void_p * L)(*([16 * (i + 1) for i in range(L)] if maps is None else maps))
    hs = (C.c_int32 * L)(*([7] * L))
    scales = (C.c_float * L)(*([0.25] * L))
    sb = (C.c_int64 * L)(*([49 * Cc] * L))
    sy = (C.c_int64 * L)(*([7 * Cc] * L))
    sx = (C.c_int64 * L)(*([Cc if stride_x is None else stride_x] * L))
    return (ptrs, hs, hs, scales, sb, sy, sx, L, Cc, boxes, None, 2, 10, P, S, k[0], k[1], 224.0, 4.0, out, None, None)


REFUSALS = [
    (dict(boxes=None), "null"), (dict(out=None), "null"), (dict(maps=[16, 32, None, 64, 80]), "null"),
    (dict(maps=[16, 32, 40, 64, 80]), "aligned"), (dict(out=8), "aligned"), (dict(boxes=8), "aligned"),
    (dict(Cc=254), "multiple of 4"), (dict(L=9, k=(2, 10)), "levels"), (dict(P=5), "output size"), (dict(S=3), "sampling ratio"),
    (dict(k=(2, 7)), "do not fit"), (dict(stride_x=128), "stride"),
]


@pytest.mark.parametrize("kwargs,fragment", REFUSALS)
def test_bf16_roi_align_refuses_what_the_fp32_entry_refuses(kwargs, fragment):
    """Every pointer here is a small integer: a call that got past the host checks would fault, so a pass means 'refused before
    any launch'.  Both entries give the same code and the same message."""
    lib = _lib.load()
    rc32 = lib.ldit_roi_align_levels_f32(*_roi_args(**kwargs))
    msg32 = lib.ldit_last_error().decode()
    rc16 = lib.ldit_roi_align_levels_bf16(*_roi_args(**kwargs))
    msg16 = lib.ldit_last_error().decode()
    assert rc32 in (_lib.LDIT_EINVAL, _lib.LDIT_EUNSUPPORTED) and rc16 == rc32
    assert fragment in msg16 and msg16 == msg32


def test_linear_entries_without_a_relu_epilogue_refuse_it():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    relu = _lib.EPI_BIAS_RELU
    assert lib.ldit_linear_f32(16, 64, 16, None, 16, 64, 8, 64, 64, relu, None, None, None, None) == _lib.LDIT_EINVAL and "epilogue" in err()
    assert lib.ldit_linear_fp8(16, 128, 16, None, 16, 64, 8, 64, 128, relu, None, None, None, 1.0, 1.0, None, None) == _lib.LDIT_EINVAL
    assert "epilogue" in err()
    assert lib.ldit_linear_planes(16, 128, 16, None, 16, 64, 8, 64, 64, relu, None, None, None, 2, None) == _lib.LDIT_EINVAL and "epilogue" in err()
    assert lib.ldit_linear_mxfp8(16, 128, 16, 16, 16, None, 16, 64, None, 8, 64, 128, relu, None, None, None, None) == _lib.LDIT_EINVAL
    assert "epilogue" in err()
    assert lib.ldit_linear_bf16_tr(16, 64, 0, 16, 64, 16, 64, 8, 64, 64, relu, None, 1, 16, None) == _lib.LDIT_EINVAL and "epilogue" in err()
    # the two bf16 entries take it: what stops these calls is the NEXT host check (a null / misaligned operand), not the epilogue
    assert lib.ldit_linear_bf16(None, 64, 16, None, 16, 64, 8, 64, 64, relu, None, None, None, None) == _lib.LDIT_EINVAL and "epilogue" not in err()
    assert lib.ldit_linear_bf16_ex(None, 64, 16, None, 16, 64, 8, 64, 64, relu, None, None, None, None, None, None, 0, 1, None) == _lib.LDIT_EINVAL
    assert "epilogue" not in err()
    assert lib.ldit_linear_bf16(16, 64, 16, None, 16, 64, 8, 64, 64, 7, None, None, None, None) == _lib.LDIT_EINVAL and "epilogue" in err()


def _tiny_detector(**kw):
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    return LayoutDetectionModel(config=cfg, **kw)


def test_head_dtype_option():
    pool = MultiScaleRoIAlign(["p2", "p3", "p4", "p5", "pool"], 7, 2)
    rh = RoIHeads(pool, TwoMLPHead(64 * 49, 64), FastRCNNPredictor(64, 6))
    assert rh.head_dtype == "f32"                                                     # the default
    assert rh.set_head_dtype("bf16") is rh and rh.head_dtype == "bf16"
    assert RoIHeads(pool, TwoMLPHead(64 * 49, 64), FastRCNNPredictor(64, 6), head_dtype="bf16").head_dtype == "bf16"
    for bad in ("fp16", "BF16", None, torch.bfloat16):
        with pytest.raises(ValueError, match="head_dtype"):
            RoIHeads(pool, TwoMLPHead(64 * 49, 64), FastRCNNPredictor(64, 6), head_dtype=bad)
        with pytest.raises(ValueError, match="head_dtype"):
            rh.set_head_dtype(bad)
    assert rh.head_dtype == "bf16"                                                    # a refused value changes nothing
    with pytest.raises(ValueError, match="head_dtype"):
        _tiny_detector(head_dtype="fp16")
    model = _tiny_detector()
    assert model.head_dtype == "f32" and model.model.roi_heads.head_dtype == "f32"
    with pytest.raises(ValueError, match="head_dtype"):
        model.set_head_dtype("fp16")
    assert model.set_head_dtype("bf16") is model and model.head_dtype == "bf16" and model.model.roi_heads.head_dtype == "bf16"


def test_state_dict_does_not_depend_on_head_dtype():
    torch.manual_seed(0)
    a = _tiny_detector()
    b = _tiny_detector(head_dtype="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].dtype == sb[k].dtype and tuple(sa[k].shape) == tuple(sb[k].shape) for k in sa)
    assert all(p.dtype == torch.float32 for p in b.model.roi_heads.parameters())      # the parameters stay fp32
    before = {k: v.clone() for k, v in sa.items()}
    a.set_head_dtype("bf16")
    after = a.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not b.load_state_dict(sa, strict=True).missing_keys                        # one checkpoint, either setting


def test_bf16_head_has_no_cpu_path():
    pool = MultiScaleRoIAlign(["p2"], 7, 2)
    rh = RoIHeads(pool, TwoMLPHead(8 * 49, 64), FastRCNNPredictor(64, 6), head_dtype="bf16").eval()
    with pytest.raises(ValueError, match="GPU"):
        rh([torch.zeros(1, 8, 4, 4).to(memory_format=torch.channels_last)], torch.zeros(1, 3, 4), None, (16, 16))
