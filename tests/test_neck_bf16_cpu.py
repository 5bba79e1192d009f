"""Host-side checks of the bf16 eval-mode neck (no GPU, no launch): ``ldit_conv3x3_nhwc_bf16`` is declared, bound and exported under
the unchanged ABI version, refuses on the host what its contract says it refuses, and ``neck_dtype`` is an option of the modules
that leaves the checkpoint surface alone."""
import os
import re

import pytest
import torch

from layoutdit_amd import _lib
from layoutdit_amd.config import DiTConfig
from layoutdit_amd.modeling import LayoutDetectionModel
from layoutdit_amd.modeling.dit_fpn import DiTWithFPN
from layoutdit_amd.modeling.rpn import RPNHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ldit_conv3x3_nhwc_bf16"


def test_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    # xpad, w, bias, y, ldy, B, H, W, Cin, Cout, epilogue, stream
    assert len(_lib.SIGNATURES[NAME][1]) == 12
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive


def _args(xpad=4096, w=8192, bias=None, y=16384, ldy=None, B=2, H=5, W=9, Cin=64, Cout=64, epilogue=_lib.EPI_F32):
    return (xpad, w, bias, y, Cout if ldy is None else ldy, B, H, W, Cin, Cout, epilogue, None)


EINVAL, EUNSUPPORTED = _lib.LDIT_EINVAL, _lib.LDIT_EUNSUPPORTED
REFUSALS = [
    (dict(xpad=None), EINVAL, "null"), (dict(w=None), EINVAL, "null"), (dict(y=None), EINVAL, "null"),
    (dict(xpad=4096 + 8), EINVAL, "aligned"), (dict(w=8192 + 2), EINVAL, "aligned"), (dict(y=16384 + 8), EINVAL, "aligned"),
    (dict(B=0), EINVAL, "empty"), (dict(H=0), EINVAL, "empty"), (dict(W=0), EINVAL, "empty"), (dict(Cin=0), EINVAL, "empty"),
    (dict(Cout=0, ldy=64), EINVAL, "empty"),
    (dict(epilogue=_lib.EPI_BIAS_GELU), EINVAL, "epilogue"), (dict(epilogue=_lib.EPI_SCALE_RESID), EINVAL, "epilogue"),
    (dict(epilogue=_lib.EPI_GELU_BWD), EINVAL, "epilogue"), (dict(epilogue=3), EINVAL, "epilogue"), (dict(epilogue=7), EINVAL, "epilogue"),
    (dict(ldy=63), EINVAL, "ldy"), (dict(Cout=50, ldy=48), EINVAL, "ldy"),
    (dict(Cin=32), EUNSUPPORTED, "multiple of 64"), (dict(Cin=96), EUNSUPPORTED, "multiple of 64"), (dict(Cin=200), EUNSUPPORTED, "multiple of 64"),
    (dict(B=64, H=510, W=510, Cin=128), EUNSUPPORTED, "2^31"),                      # padded map: 64 * 512 * 512 * 128 = 2^31
    (dict(B=64, H=512, W=512, Cin=64, Cout=128), EUNSUPPORTED, "2^31"),             # output: 2^24 rows * 128
    (dict(B=64, H=512, W=512, Cin=64, Cout=64, ldy=128), EUNSUPPORTED, "2^31"),     # ... counted with its row stride
    (dict(Cin=16384, Cout=16384), EUNSUPPORTED, "2^31"),                            # weight: 9 * 2^28
    (dict(B=1 << 40, H=1 << 40, W=1 << 40), EUNSUPPORTED, "2^31"),                  # (and no 64-bit wrap-around on the way)
]


@pytest.mark.parametrize("kwargs,code,fragment", REFUSALS)
def test_conv3x3_bf16_refuses_on_the_host(kwargs, code, fragment):
    """Every pointer here is a small integer: a call that got past the host checks would fault (or fail for want of a device), so
    a pass means 'refused before any launch', with the contract's code and a message that names the reason."""
    lib = _lib.load()
    rc = getattr(lib, NAME)(*_args(**kwargs))
    msg = lib.ldit_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith("conv3x3_bf16:") and fragment in msg, msg


def _tiny_detector(**kw):
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    return LayoutDetectionModel(config=cfg, **kw)


def test_neck_dtype_option():
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    for make in (lambda **kw: RPNHead(64, 3, **kw), lambda **kw: DiTWithFPN(config=cfg, **kw)):
        m = make()
        assert m.neck_dtype == "f32"                                                  # the default
        assert m.set_neck_dtype("bf16") is m and m.neck_dtype == "bf16"
        assert make(neck_dtype="bf16").neck_dtype == "bf16"
        for bad in ("fp16", "BF16", None, torch.bfloat16):
            with pytest.raises(ValueError, match="neck_dtype"):
                make(neck_dtype=bad)
            with pytest.raises(ValueError, match="neck_dtype"):
                m.set_neck_dtype(bad)
        assert m.neck_dtype == "bf16"                                                 # a refused value changes nothing
        assert m.set_neck_dtype("f32") is m and m.neck_dtype == "f32"
    with pytest.raises(ValueError, match="neck_dtype"):
        _tiny_detector(neck_dtype="fp16")
    model = _tiny_detector()
    stages = lambda: (model.neck_dtype, model.model.backbone.neck_dtype, model.model.rpn.head.neck_dtype)    # noqa: E731
    assert stages() == ("f32",) * 3 and model.head_dtype == "f32"
    with pytest.raises(ValueError, match="neck_dtype"):
        model.set_neck_dtype("fp16")
    assert stages() == ("f32",) * 3
    assert model.set_neck_dtype("bf16") is model and stages() == ("bf16",) * 3
    with pytest.raises(ValueError, match="neck_dtype"):
        model.set_neck_dtype(None)
    assert stages() == ("bf16",) * 3 and model.head_dtype == "f32"                    # ... and is its own option


def test_state_dict_does_not_depend_on_neck_dtype():
    torch.manual_seed(0)
    a = _tiny_detector()
    b = _tiny_detector(neck_dtype="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].dtype == sb[k].dtype and tuple(sa[k].shape) == tuple(sb[k].shape) for k in sa)
    assert all(p.dtype == torch.float32 for p in b.parameters())                      # the parameters stay fp32
    before = {k: v.clone() for k, v in sa.items()}
    a.set_neck_dtype("bf16")
    after = a.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not b.load_state_dict(sa, strict=True).missing_keys                        # one checkpoint, either setting
    sb = b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_bf16_neck_has_no_cpu_path():
    head = RPNHead(64, 3, neck_dtype="bf16").eval()
    with pytest.raises(ValueError, match="GPU"), torch.no_grad():
        head.forward_level(torch.zeros(1, 64, 4, 4).to(memory_format=torch.channels_last))
