"""CPU-only checks of the detector on the quantisation-aware mxfp8 encoder: the constructor plumbing (qat reaches the encoder, the
state-dict keys do not change, every other dtype is the encoder's refusal), the C ABI of ldit_requant_train_mirror (declared, bound,
exported, its arguments validated before any launch) and what DetectorTrainStep / ops refuse without a device.  No kernel is
launched here."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from layoutdit_amd import _lib, ops, training
from layoutdit_amd import config as cfgs
from layoutdit_amd.detector_training import DetectorTrainStep
from layoutdit_amd.modeling import LayoutDetectionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ldit_requant_train_mirror"


def _small():
    return cfgs.DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)


def _cfg(hidden=128, layers=3, mlp=512, dtype=_lib.DTYPE_MXFP8, img=32):
    return _lib.LditCfg(hidden=hidden, layers=layers, heads=hidden // 64, mlp=mlp, patch=16, in_ch=3, img_h=img, img_w=img, ln_eps=1e-12,
                        n_taps=0, dtype=dtype, flags=0)


def test_qat_detector_constructs_with_the_plain_builds_keys():
    plain = LayoutDetectionModel(config=_small(), compute_dtype="mxfp8")
    qat = LayoutDetectionModel(config=_small(), compute_dtype="mxfp8", qat=True)
    assert qat.qat is True and plain.qat is False and LayoutDetectionModel(config=_small()).qat is False
    assert qat.model.backbone.backbone.dit.qat is True and qat.model.backbone.backbone.dit.compute_dtype == "mxfp8"
    assert list(qat.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in qat.named_parameters()] == [n for n, _ in plain.named_parameters()]
    with pytest.raises(AttributeError):
        qat.qat = False                                                                  # read-only: fixed at construction
    # the two builds load each other's checkpoints
    plain.load_state_dict(qat.state_dict())
    qat.load_state_dict(plain.state_dict())
    bf = LayoutDetectionModel(config=_small(), compute_dtype="bf16")
    bf.load_state_dict(qat.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(bf.state_dict().values(), qat.state_dict().values()))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_qat_on_another_dtype_is_the_encoders_refusal(dtype):
    with pytest.raises(ValueError, match="qat=True"):
        LayoutDetectionModel(config=_small(), compute_dtype=dtype, qat=True)


def test_header_declares_binding_describes_and_library_exports_the_entry():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text).group(1)
    got = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in args.split(",")]
    assert got == ["const ldit_cfg *", "const void *", "void *", "size_t", "const ldit_opt_state *", "ldit_stream"], got
    assert _lib.SIGNATURES[NAME] == (C.c_int, [C.POINTER(_lib.LditCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p])
    # declared behind the state block it reads
    assert text.index("} ldit_opt_state;") < text.index(NAME)


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    cfg = _cfg()
    need = lib.ldit_train_mirror_bytes(C.byref(cfg))
    flat = lib.ldit_flat_param_bytes(C.byref(cfg))
    assert need == (flat // 2 + 255) // 256 * 256 + lib.ldit_packed_bytes(C.byref(cfg)) > 0

    def call(cfg=cfg, params=1024, mirror=4096, nbytes=need, state=None):
        return lib.ldit_requant_train_mirror(None if cfg is None else C.byref(cfg), params, mirror, nbytes, state, None)

    assert call(cfg=None) == _lib.LDIT_EINVAL and "null" in err()
    assert call(params=None) == _lib.LDIT_EINVAL and "null" in err()
    assert call(mirror=None) == _lib.LDIT_EINVAL and "null" in err()
    assert call(params=1024 + 8) == _lib.LDIT_EINVAL and "16-byte" in err()
    assert call(mirror=4096 + 4) == _lib.LDIT_EINVAL and "16-byte" in err()
    assert call(state=258) == _lib.LDIT_EINVAL and "state" in err()
    assert call(nbytes=need - 1) == _lib.LDIT_EWORKSPACE and str(need) in err()
    assert call(nbytes=flat // 2) == _lib.LDIT_EWORKSPACE                               # the bf16 build's mirror: no MX section
    assert call(nbytes=0) == _lib.LDIT_EWORKSPACE
    # a dtype that is not LDIT_MXFP8: the train step's other build is refused here, every build without a train step by train_geometry
    assert call(cfg=_cfg(dtype=_lib.DTYPE_BF16)) == _lib.LDIT_EINVAL and "LDIT_MXFP8" in err()
    for dtype in (_lib.DTYPE_F32, _lib.DTYPE_FP8, _lib.DTYPE_F32X3):
        assert call(cfg=_cfg(dtype=dtype)) == _lib.LDIT_EUNSUPPORTED
    # a geometry the mxfp8 build lacks: hidden / mlp not multiples of 128, an image the patch does not divide
    assert call(cfg=_cfg(hidden=192)) == _lib.LDIT_EUNSUPPORTED and "128" in err()
    assert call(cfg=_cfg(mlp=448)) == _lib.LDIT_EUNSUPPORTED and "128" in err()
    assert call(cfg=_cfg(img=40)) == _lib.LDIT_EINVAL
    if not torch.cuda.is_available():
        # no device: the library's HIP error - there is nothing to fall back to.  (Where a device exists this well-formed call would
        # launch on made-up addresses; there only the refusals above are made.)
        assert call() == _lib.LDIT_EHIP and "hip" in err().lower()
    # no layer: nothing to re-quantise, nothing launched
    assert call(cfg=_cfg(layers=0), nbytes=lib.ldit_train_mirror_bytes(C.byref(_cfg(layers=0)))) == _lib.LDIT_OK


def test_front_end_refuses_what_it_cannot_run():
    cfg = _cfg()
    with pytest.raises(ValueError, match="mxfp8"):                                     # a bf16 flat state has no MX section
        ops.requant_train_mirror(types.SimpleNamespace(mx=False, params=torch.zeros(4), packed=torch.zeros(4, dtype=torch.uint8), lcfg=cfg))
    st = types.SimpleNamespace(mx=True, params=torch.zeros(4), packed=torch.zeros(4, dtype=torch.uint8), lcfg=cfg)
    with pytest.raises(ValueError, match="int32"):
        ops.requant_train_mirror(st, torch.zeros(10))
    with pytest.raises(ValueError, match="GPU"):
        ops.requant_train_mirror(st)


def test_detector_train_step_accepts_qat_and_keeps_refusing_the_inference_builds():
    for kw in ({"compute_dtype": "mxfp8"}, {"compute_dtype": "fp8"}):
        with pytest.raises(NotImplementedError, match="TrainStep"):
            DetectorTrainStep(LayoutDetectionModel(config=_small(), **kw).train())
    # the quantisation-aware build passes that gate: what stops it here is the missing device, like every other build
    with pytest.raises(ValueError, match="GPU"):
        DetectorTrainStep(LayoutDetectionModel(config=_small(), compute_dtype="mxfp8", qat=True).train())
    with pytest.raises(RuntimeError, match="train"):
        DetectorTrainStep(LayoutDetectionModel(config=_small(), compute_dtype="mxfp8", qat=True).eval())
    doc = training.TrainStep.__doc__
    assert "DetectorTrainStep" in doc and "only one that trains" not in doc
    assert "requant_train_mirror" in DetectorTrainStep.apply.__doc__
