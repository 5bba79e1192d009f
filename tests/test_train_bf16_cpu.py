"""Host-side checks of ``train_dtype`` (no GPU, no launch): the option of the detector and of its stages - default, refusal before any
change, independence from ``head_dtype`` / ``neck_dtype`` / ``grad_dtype`` - the ``state_dict``, and the two entry points with a bf16
``act`` as the header, the ctypes table and the library agree on them."""
import os
import re

import pytest
import torch

from layoutdit_amd import _lib
from layoutdit_amd.config import DiTConfig
from layoutdit_amd.modeling import LayoutDetectionModel, grad_ops
from layoutdit_amd.modeling.dit_fpn import DiTWithFPN
from layoutdit_amd.modeling.roi_heads import FastRCNNPredictor, MultiScaleRoIAlign, RoIHeads, TwoMLPHead
from layoutdit_amd.modeling.rpn import RPNHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)


def _detector(**kw):
    return LayoutDetectionModel(config=DiTConfig(**CFG), **kw)


def _stages(model):
    m = model.model
    return m.backbone.train_dtype, m.rpn.head.train_dtype, m.roi_heads.train_dtype, m.roi_heads.box_head.train_dtype


def _others(model):
    return model.head_dtype, model.neck_dtype, model.grad_dtype


def test_train_dtype_option_of_the_detector():
    model = _detector()
    assert model.train_dtype == "f32" and _stages(model) == ("f32",) * 4                     # the default
    for bad in ("fp16", None, "BF16", torch.bfloat16):
        with pytest.raises(ValueError, match="train_dtype"):
            model.set_train_dtype(bad)
        assert _stages(model) == ("f32",) * 4                                                 # refused before any stage changes
        with pytest.raises(ValueError, match="train_dtype"):
            _detector(train_dtype=bad)
    assert model.set_train_dtype("bf16") is model
    assert model.train_dtype == "bf16" and _stages(model) == ("bf16",) * 4
    with pytest.raises(ValueError, match="train_dtype"):
        model.set_train_dtype("fp16")
    assert _stages(model) == ("bf16",) * 4
    assert _others(model) == ("f32",) * 3                                                     # ... and is its own option
    assert _stages(_detector(train_dtype="bf16")) == ("bf16",) * 4
    assert _stages(model.set_train_dtype("f32")) == ("f32",) * 4


@pytest.mark.parametrize("head_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("neck_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_train_dtype_is_independent_of_the_other_three(head_dtype, neck_dtype, grad_dtype):
    other = (head_dtype, neck_dtype, grad_dtype)
    for train_dtype in ("f32", "bf16"):
        model = _detector(head_dtype=head_dtype, neck_dtype=neck_dtype, grad_dtype=grad_dtype, train_dtype=train_dtype)
        assert _others(model) == other and _stages(model) == (train_dtype,) * 4
        flipped = "f32" if train_dtype == "bf16" else "bf16"
        model.set_train_dtype(flipped)
        assert _others(model) == other
        model.set_head_dtype("f32").set_neck_dtype("f32").set_grad_dtype("f32")
        assert _stages(model) == (flipped,) * 4


def test_train_dtype_option_of_each_stage():
    pool = MultiScaleRoIAlign(["p2"], 7, 2)
    makers = (lambda **kw: RPNHead(64, 3, **kw), lambda **kw: DiTWithFPN(config=DiTConfig(**CFG), **kw),
              lambda **kw: TwoMLPHead(64 * 49, 64, **kw),
              lambda **kw: RoIHeads(pool, TwoMLPHead(64 * 49, 64), FastRCNNPredictor(64, 6), **kw))
    for make in makers:
        m = make()
        assert m.train_dtype == "f32" and m.grad_dtype == "f32"
        assert m.set_train_dtype("bf16") is m and m.train_dtype == "bf16" and m.grad_dtype == "f32"
        assert make(train_dtype="bf16").train_dtype == "bf16"
        assert make(train_dtype="bf16", grad_dtype="bf16").grad_dtype == "bf16"
        for bad in ("fp16", None):
            with pytest.raises(ValueError, match="train_dtype"):
                m.set_train_dtype(bad)
        assert m.train_dtype == "bf16"
        with pytest.raises(ValueError, match="train_dtype"):
            make(train_dtype="fp16")
    # RoIHeads without the argument keeps what its box head was built with
    assert RoIHeads(pool, TwoMLPHead(64 * 49, 64, train_dtype="bf16"), FastRCNNPredictor(64, 6)).train_dtype == "bf16"
    assert grad_ops.check_dtype("train_dtype", "bf16") == "bf16" and grad_ops.DTYPES == ("f32", "bf16")


def test_state_dict_does_not_depend_on_train_dtype():
    torch.manual_seed(0)
    a, b = _detector(), _detector(train_dtype="bf16")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].dtype == sb[k].dtype and tuple(sa[k].shape) == tuple(sb[k].shape) for k in sa)
    before = {k: v.clone() for k, v in sa.items()}
    a.set_train_dtype("bf16")
    after = a.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    assert not b.load_state_dict(sa, strict=True).missing_keys
    assert b.train_dtype == "bf16"                                                            # loading does not touch it


NAMES = {  # name -> the header's arguments: those of the entry points with an fp32 act
    "ldit_relu_bwd_bf16_act16": "dy lddy act ldact out ldout M N colsum scratch scratch_bytes stream".split(),
    "ldit_relu_bwd_pad_nhwc_bf16_act16": "dy act out B H W C colsum scratch scratch_bytes stream".split(),
}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_symbols_are_declared_bound_and_exported(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert decl, f"{name} is not declared in include/ldit.h"
    args = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert args == NAMES[name]
    old = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name[:-len("_act16")], text)
    assert re.sub(r"\s+", " ", old.group(1)) == re.sub(r"\s+", " ", decl.group(1))            # the existing argument list
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-len("_act16")]]
    assert "#define LDIT_ABI_VERSION 6" in text and lib.ldit_abi_version() == 6                # purely additive


EINVAL, EUNSUPPORTED, EWORKSPACE = _lib.LDIT_EINVAL, _lib.LDIT_EUNSUPPORTED, _lib.LDIT_EWORKSPACE
PLAIN, PADDED = "ldit_relu_bwd_bf16_act16", "ldit_relu_bwd_pad_nhwc_bf16_act16"


def _plain(dy=4096, lddy=8, act=8192, ldact=8, out=16384, ldout=8, M=4, N=8, colsum=32768, scratch=65536, scratch_bytes=32):
    return (dy, lddy, act, ldact, out, ldout, M, N, colsum, scratch, scratch_bytes, None)


def _padded(dy=4096, act=8192, out=16384, B=1, H=2, W=2, C=8, colsum=32768, scratch=65536, scratch_bytes=32):
    return (dy, act, out, B, H, W, C, colsum, scratch, scratch_bytes, None)


REFUSALS = [
    (PLAIN, _plain(dy=None), EINVAL, "null"), (PLAIN, _plain(out=None), EINVAL, "null"), (PLAIN, _plain(scratch=None), EINVAL, "null"),
    (PLAIN, _plain(M=0), EINVAL, "geometry"), (PLAIN, _plain(N=0), EINVAL, "geometry"), (PLAIN, _plain(lddy=7), EINVAL, "geometry"),
    (PLAIN, _plain(ldact=7), EINVAL, "geometry"), (PLAIN, _plain(ldout=7), EINVAL, "geometry"),
    (PLAIN, _plain(dy=4098), EINVAL, "misaligned"), (PLAIN, _plain(act=8193), EINVAL, "misaligned"),      # act: its 2-byte element
    (PLAIN, _plain(out=16385), EINVAL, "misaligned"),
    (PLAIN, _plain(scratch_bytes=31), EWORKSPACE, "scratch"),
    (PLAIN, _plain(M=1 << 31, scratch_bytes=1 << 40), EUNSUPPORTED, "2^31"),
    (PLAIN, _plain(N=1 << 31, lddy=1 << 31, ldact=1 << 31, ldout=1 << 31, scratch_bytes=1 << 40), EUNSUPPORTED, "2^31"),
    (PADDED, _padded(dy=None), EINVAL, "null"), (PADDED, _padded(out=None), EINVAL, "null"), (PADDED, _padded(scratch=None), EINVAL, "null"),
    (PADDED, _padded(B=0), EINVAL, "geometry"), (PADDED, _padded(C=6), EINVAL, "geometry"),
    (PADDED, _padded(dy=4104), EINVAL, "misaligned"), (PADDED, _padded(act=8196), EINVAL, "misaligned"),  # act: 8 bytes, four elements
    (PADDED, _padded(act=8194), EINVAL, "misaligned"), (PADDED, _padded(out=16388), EINVAL, "misaligned"),
    (PADDED, _padded(scratch_bytes=31), EWORKSPACE, "scratch"),
    (PADDED, _padded(B=1 << 16, H=1 << 8, W=1 << 7, colsum=None), EUNSUPPORTED, "2^31"),
    (PADDED, _padded(B=64, H=1022, W=1022, C=128, colsum=None), EUNSUPPORTED, "2^33"),
    (PADDED, _padded(B=1 << 40, H=1 << 40, W=1 << 40, colsum=None), EUNSUPPORTED, "2^31"),
]


@pytest.mark.parametrize("name,args,code,fragment", REFUSALS)
def test_relu_bwd_act16_refuses_on_the_host(name, args, code, fragment):
    """Every pointer here is a small integer: a call that got past the host checks would fault (or fail for want of a device), so a
    pass means 'refused before any launch', with the contract's code and a message that names the entry and the reason."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.ldit_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith(name[len("ldit_"):] + ":") and fragment in msg, msg


def test_backward_helpers_take_no_cpu_tensors_whatever_their_dtype():
    t, t16 = torch.zeros(2, 64), torch.zeros(2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):                                              # no CPU path, no fall-back
        grad_ops.linear_bwd(t, t16, torch.zeros(64, 64), True, True, True, grad_dtype="bf16", act=t16)
    with pytest.raises(ValueError, match="grad_dtype"):
        grad_ops.linear_bwd(t, t16, torch.zeros(64, 64), True, True, True, grad_dtype="fp16", act=t16)
