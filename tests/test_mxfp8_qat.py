"""Quantisation-aware training of the mxfp8 build (DiTEncoder(compute_dtype="mxfp8", qat=True)): what holds without a GPU -
the C ABI and its binding, the train-step buffer sizes of the LDIT_MXFP8 build, the refusal of every other dtype, and the
exactness rule the straight-through backward rests on (include/ldit.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from layoutdit_amd import _lib, config as cfgs
from tests.test_mxfp8_format import e4m3_values

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ldit_adamw_step_mxfp8", "ldit_layernorm_mxfp8_train", "ldit_attention_mxfp8_train", "ldit_linear_mxfp8_train")


def test_header_and_binding_declare_the_qat_entries_at_abi_6():
    hdr = open(os.path.join(ROOT, "include", "ldit.h")).read()
    assert re.search(r"#define\s+LDIT_ABI_VERSION\s+6\b", hdr)
    assert _lib.LDIT_ABI_VERSION == 6
    for fn in NEW:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", hdr), fn
        assert fn in _lib.SIGNATURES, fn
    assert "-124 <= e <= 119" in hdr                       # the exactness rule is stated where the ABI is


def _cfg(model, dtype, batch_img=224):
    c = _lib.LditCfg(hidden=model.hidden_size, layers=model.num_hidden_layers, heads=model.num_attention_heads,
                     mlp=model.intermediate_size, patch=model.patch_size, in_ch=3, img_h=batch_img, img_w=batch_img,
                     ln_eps=model.layer_norm_eps, n_taps=0, dtype=dtype, flags=0)
    return c


def _up(v, a=256):
    return (v + a - 1) // a * a


def test_vit_base_mxfp8_train_buffers_match_the_documented_layout():
    lib = _lib.load()
    m = cfgs.vit_base()
    mx, bf = _cfg(m, _lib.DTYPE_MXFP8), _cfg(m, _lib.DTYPE_BF16)
    B = 64
    M, Cc, F, L = B * m.tokens(224, 224), m.hidden_size, m.intermediate_size, m.num_hidden_layers
    flat = lib.ldit_flat_param_bytes(C.byref(mx))
    assert lib.ldit_train_mirror_bytes(C.byref(mx)) == _up(flat // 2) + lib.ldit_packed_bytes(C.byref(mx)) > 0
    assert lib.ldit_train_mirror_bytes(C.byref(bf)) == flat // 2
    saved = lib.ldit_train_saved_bytes(C.byref(mx), B)
    assert saved == (lib.ldit_train_saved_bytes(C.byref(bf), B) + L * _up(M * Cc * 2) + _up(M * Cc * 33 // 32)
                     + _up(M * F * 33 // 32)) > 0
    assert lib.ldit_train_workspace_bytes(C.byref(mx), B) == lib.ldit_train_workspace_bytes(C.byref(bf), B) > 0


def test_vit_tiny_has_no_mxfp8_train_step():
    lib = _lib.load()
    c = _cfg(cfgs.vit_tiny(), _lib.DTYPE_MXFP8)
    for size in (lib.ldit_train_mirror_bytes(C.byref(c)), lib.ldit_train_saved_bytes(C.byref(c), 2)):
        assert size == 0
        assert "multiples of 128" in lib.ldit_last_error().decode()


def test_fp8_train_step_still_refused_by_the_library():
    lib = _lib.load()
    c = _cfg(cfgs.vit_base(), _lib.DTYPE_FP8)
    assert lib.ldit_train_mirror_bytes(C.byref(c)) == 0
    assert lib.ldit_train_saved_bytes(C.byref(c), 2) == 0


@pytest.mark.parametrize("dtype", ["f32", "f32x3", "f32x6", "bf16", "fp8"])
def test_qat_is_refused_on_every_other_build(dtype):
    from layoutdit_amd.modeling import DiTBackbone, DiTEncoder, DiTWithFPN
    with pytest.raises(ValueError, match="qat=True"):
        DiTEncoder(cfgs.vit_micro(), compute_dtype=dtype, qat=True)
    with pytest.raises(ValueError, match="qat=True"):
        DiTBackbone(config=cfgs.vit_micro(), compute_dtype=dtype, qat=True)
    with pytest.raises(ValueError, match="qat=True"):
        DiTWithFPN(config=cfgs.vit_micro(), compute_dtype=dtype, qat=True)


def test_qat_keyword_reaches_the_encoder():
    from layoutdit_amd.modeling import DiTWithFPN, DiTEncoder
    assert DiTWithFPN(config=cfgs.vit_micro(), compute_dtype="mxfp8", qat=True).backbone.dit.qat
    assert not DiTEncoder(cfgs.vit_micro(), compute_dtype="mxfp8").qat


def _is_bf16(v: np.ndarray) -> np.ndarray:
    """True where the float64 value is exactly representable in bf16 (finite)"""
    t = torch.from_numpy(v)
    back = t.to(torch.bfloat16).to(torch.float64).numpy()
    return np.isfinite(back) & (back == v)


def test_exactness_rule_bf16_holds_every_dequantised_code_in_range():
    codes = e4m3_values()
    codes = codes[np.isfinite(codes)]
    assert codes.size == 254
    for e in range(-124, 120):
        v = codes * np.ldexp(1.0, e)
        assert _is_bf16(v).all(), e
    # just outside: the smallest subnormal code leaves bf16's range below, the largest code overflows above
    assert not _is_bf16(codes * np.ldexp(1.0, -125)).all()
    assert not _is_bf16(codes * np.ldexp(1.0, 120)).all()
