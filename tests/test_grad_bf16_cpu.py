"""Host-side checks of ``grad_dtype`` (no GPU, no launch): the option of the detector and of its three differentiable stages, the
two new entry points as the header, the ctypes table and the library agree on them, and the float64 contract oracle the GPU tests
compare with."""
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib
from layoutdit_amd.config import DiTConfig
from layoutdit_amd.modeling import LayoutDetectionModel
from layoutdit_amd.modeling.dit_fpn import DiTWithFPN
from layoutdit_amd.modeling.roi_heads import FastRCNNPredictor, MultiScaleRoIAlign, RoIHeads, TwoMLPHead
from layoutdit_amd.modeling.rpn import RPNHead
from tests import grad_bf16_oracle as go
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)


def _detector(**kw):
    return LayoutDetectionModel(config=DiTConfig(**CFG), **kw)


def _stages(model):
    return model.model.backbone.grad_dtype, model.model.rpn.head.grad_dtype, model.model.roi_heads.grad_dtype


def test_grad_dtype_option_of_the_detector():
    model = _detector()
    assert model.grad_dtype == "f32" and _stages(model) == ("f32",) * 3                      # the default
    for bad in ("fp16", None, "BF16", torch.bfloat16):
        with pytest.raises(ValueError, match="grad_dtype"):
            model.set_grad_dtype(bad)
        assert _stages(model) == ("f32",) * 3                                                 # refused before any stage changes
        with pytest.raises(ValueError, match="grad_dtype"):
            _detector(grad_dtype=bad)
    assert model.set_grad_dtype("bf16") is model
    assert model.grad_dtype == "bf16" and _stages(model) == ("bf16",) * 3
    assert model.model.roi_heads.box_head.grad_dtype == "bf16"
    with pytest.raises(ValueError, match="grad_dtype"):
        model.set_grad_dtype("fp16")
    assert _stages(model) == ("bf16",) * 3
    assert (model.head_dtype, model.neck_dtype) == ("f32", "f32")                             # ... and is its own option
    assert _stages(_detector(grad_dtype="bf16")) == ("bf16",) * 3
    assert _stages(model.set_grad_dtype("f32")) == ("f32",) * 3


def test_grad_dtype_option_of_each_stage():
    pool = MultiScaleRoIAlign(["p2"], 7, 2)
    makers = (lambda **kw: RPNHead(64, 3, **kw), lambda **kw: DiTWithFPN(config=DiTConfig(**CFG), **kw),
              lambda **kw: TwoMLPHead(64 * 49, 64, **kw),
              lambda **kw: RoIHeads(pool, TwoMLPHead(64 * 49, 64), FastRCNNPredictor(64, 6), **kw))
    for make in makers:
        m = make()
        assert m.grad_dtype == "f32"
        assert m.set_grad_dtype("bf16") is m and m.grad_dtype == "bf16"
        assert make(grad_dtype="bf16").grad_dtype == "bf16"
        for bad in ("fp16", None):
            with pytest.raises(ValueError, match="grad_dtype"):
                m.set_grad_dtype(bad)
        assert m.grad_dtype == "bf16"
        with pytest.raises(ValueError, match="grad_dtype"):
            make(grad_dtype="fp16")
    # RoIHeads without the argument keeps what its box head was built with
    assert RoIHeads(pool, TwoMLPHead(64 * 49, 64, grad_dtype="bf16"), FastRCNNPredictor(64, 6)).grad_dtype == "bf16"


def test_state_dict_does_not_depend_on_grad_dtype():
    torch.manual_seed(0)
    a, b = _detector(), _detector(grad_dtype="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].dtype == sb[k].dtype and tuple(sa[k].shape) == tuple(sb[k].shape) for k in sa)
    before = {k: v.clone() for k, v in sa.items()}
    a.set_grad_dtype("bf16")
    after = a.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    assert not b.load_state_dict(sa, strict=True).missing_keys


NAMES = {  # name -> the header's arguments
    "ldit_relu_bwd_bf16": "dy lddy act ldact out ldout M N colsum scratch scratch_bytes stream".split(),
    "ldit_relu_bwd_pad_nhwc_bf16": "dy act out B H W C colsum scratch scratch_bytes stream".split(),
}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbols_are_declared_bound_and_exported(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert decl, f"{name} is not declared in include/ldit.h"
    args = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert args == NAMES[name]
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name][1]) == len(args)
    assert "#define LDIT_ABI_VERSION 6" in text and lib.ldit_abi_version() == 6                # purely additive


EINVAL, EUNSUPPORTED, EWORKSPACE = _lib.LDIT_EINVAL, _lib.LDIT_EUNSUPPORTED, _lib.LDIT_EWORKSPACE


def _plain(dy=4096, lddy=8, act=8192, ldact=8, out=16384, ldout=8, M=4, N=8, colsum=32768, scratch=65536, scratch_bytes=32):
    return (dy, lddy, act, ldact, out, ldout, M, N, colsum, scratch, scratch_bytes, None)


def _padded(dy=4096, act=8192, out=16384, B=1, H=2, W=2, C=8, colsum=32768, scratch=65536, scratch_bytes=32):
    return (dy, act, out, B, H, W, C, colsum, scratch, scratch_bytes, None)


REFUSALS = [
    ("ldit_relu_bwd_bf16", _plain(dy=None), EINVAL, "null"), ("ldit_relu_bwd_bf16", _plain(out=None), EINVAL, "null"),
    ("ldit_relu_bwd_bf16", _plain(scratch=None), EINVAL, "null"),
    ("ldit_relu_bwd_bf16", _plain(M=0), EINVAL, "geometry"), ("ldit_relu_bwd_bf16", _plain(N=0), EINVAL, "geometry"),
    ("ldit_relu_bwd_bf16", _plain(lddy=7), EINVAL, "geometry"), ("ldit_relu_bwd_bf16", _plain(ldact=7), EINVAL, "geometry"),
    ("ldit_relu_bwd_bf16", _plain(ldout=7), EINVAL, "geometry"),
    ("ldit_relu_bwd_bf16", _plain(dy=4098), EINVAL, "misaligned"), ("ldit_relu_bwd_bf16", _plain(act=8193), EINVAL, "misaligned"),
    ("ldit_relu_bwd_bf16", _plain(out=16385), EINVAL, "misaligned"),
    ("ldit_relu_bwd_bf16", _plain(scratch_bytes=31), EWORKSPACE, "scratch"),
    ("ldit_relu_bwd_bf16", _plain(M=1 << 31, scratch_bytes=1 << 40), EUNSUPPORTED, "2^31"),
    ("ldit_relu_bwd_bf16", _plain(N=1 << 31, lddy=1 << 31, ldact=1 << 31, ldout=1 << 31, scratch_bytes=1 << 40), EUNSUPPORTED, "2^31"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(dy=None), EINVAL, "null"), ("ldit_relu_bwd_pad_nhwc_bf16", _padded(out=None), EINVAL, "null"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(scratch=None), EINVAL, "null"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(B=0), EINVAL, "geometry"), ("ldit_relu_bwd_pad_nhwc_bf16", _padded(C=6), EINVAL, "geometry"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(dy=4104), EINVAL, "misaligned"), ("ldit_relu_bwd_pad_nhwc_bf16", _padded(act=8196), EINVAL, "misaligned"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(out=16388), EINVAL, "misaligned"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(scratch_bytes=31), EWORKSPACE, "scratch"),
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(B=1 << 16, H=1 << 8, W=1 << 7, colsum=None), EUNSUPPORTED, "2^31"),         # 2^31 pixel rows
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(B=64, H=1022, W=1022, C=128, colsum=None), EUNSUPPORTED, "2^33"),           # 2^33 padded elements
    ("ldit_relu_bwd_pad_nhwc_bf16", _padded(B=1 << 40, H=1 << 40, W=1 << 40, colsum=None), EUNSUPPORTED, "2^31"),       # no 64-bit wrap-around
]


@pytest.mark.parametrize("name,args,code,fragment", REFUSALS)
def test_relu_bwd_refuses_on_the_host(name, args, code, fragment):
    """Every pointer here is a small integer: a call that got past the host checks would fault (or fail for want of a device), so a
    pass means 'refused before any launch', with the contract's code and a message that names the entry and the reason."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.ldit_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith(name[len("ldit_"):] + ":") and fragment in msg, msg


def test_backward_helpers_refuse_a_bad_grad_dtype_before_any_launch():
    from layoutdit_amd.modeling import grad_ops
    t = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="grad_dtype"):
        grad_ops.linear_bwd(t, t, t[:, :64], True, True, True, grad_dtype="fp16")
    with pytest.raises(ValueError, match="grad_dtype"):
        grad_ops.conv3x3_bwd(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64), torch.zeros(64, 64, 3, 3), True, True, True, grad_dtype=None)
    with pytest.raises(ValueError, match="GPU"):                                              # no CPU path, no fall-back
        grad_ops.linear_bwd(t, t, torch.zeros(64, 64), True, True, True, grad_dtype="bf16")


# ---- the contract oracle ---------------------------------------------------------------------------------------------------------------
def _normal(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).normal(0, scale, size=shape).astype(np.float32))


def test_contract_oracle_linear():
    dy, w = _normal(1, 37, 128), _normal(2, 128, 200, scale=0.1)
    got, exact = go.linear_gx(dy, w), go.linear_gx_exact(dy, w)
    e = rel_l2(got.numpy(), exact.numpy())
    print(f"linear: bf16-operand g_x against float64 autograd {e:.3e}")
    assert e < 3e-2 and not torch.equal(got, exact)                                           # the rounding is really applied
    assert 1e-4 < e                                                                           # ... at bf16's size: two roundings of 2^-9
    # the mask is a selection: non-finite dy under a masked position (act = +0, -0, NaN, negative) is 0
    act = _normal(3, 37, 128)
    act[0, 0], act[0, 1], act[0, 2], act[0, 3] = 0.0, -0.0, float("nan"), -1.0
    bad = dy.clone()
    bad[0, 0], bad[0, 1], bad[0, 2], bad[0, 3] = float("inf"), float("nan"), float("-inf"), float("nan")
    masked = go.linear_gx(bad, w, act)
    assert bool(torch.isfinite(masked).all())
    keep = (act > 0).double()
    assert rel_l2(masked.numpy(), go.linear_gx(dy * keep.float(), w).numpy()) < 1e-12


def test_contract_oracle_conv3x3():
    dy, w = _normal(4, 2, 5, 7, 64), _normal(5, 64, 32, 3, 3, scale=0.05)
    got, exact = go.conv3x3_gx(dy, w), go.conv3x3_gx_exact(dy, w)
    assert tuple(got.shape) == (2, 5, 7, 32)
    e = rel_l2(got.numpy(), exact.numpy())
    print(f"conv3x3: bf16-operand g_x against float64 autograd {e:.3e}")
    assert 1e-4 < e < 3e-2 and not torch.equal(got, exact)
    # the restatement is the convolution's adjoint: <conv(x), dy> == <x, g_x>
    x = _normal(6, 2, 5, 7, 32).double()
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    assert abs(float((y * dy.double()).sum()) - float((x * exact).sum())) < 1e-9 * float(y.abs().sum())
