"""CPU-only checks of the detector's optimizer step: the C ABI declares, exports and validates the three entry points of
csrc/optim_multi.hip without a device (and without one they fail with the library's HIP error, they do not fall back); the float64
restatement tests/optim_oracle.py follows torch.amp.GradScaler through skips, back-offs and growth and torch.optim.AdamW through five
steps; the ops wrappers and DetectorTrainStep refuse what they cannot run.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib, ops, training
from layoutdit_amd import config as cfgs
from layoutdit_amd.modeling import LayoutDetectionModel
from tests import optim_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_grads_check_multi_f32", "ldit_opt_advance", "ldit_adamw_multi_f32")
Seg = _lib.LditOptSegment


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_points():
    text = _header()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    # the declared parameter lists, type by type, against the ctypes table
    want = {"ldit_grads_check_multi_f32": ["const ldit_opt_segment *", "int32_t", "ldit_opt_state *", "ldit_stream"],
            "ldit_opt_advance": ["ldit_opt_state *", "double", "double", "float", "float", "int32_t", "ldit_stream"],
            "ldit_adamw_multi_f32": ["const ldit_opt_segment *", "int32_t", "const ldit_opt_state *", "double", "double", "float", "float", "float",
                                     "ldit_stream"]}
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double, "ldit_stream": C.c_void_p, "ldit_opt_state *": C.c_void_p, "const ldit_opt_state *": C.c_void_p,
             "const ldit_opt_segment *": C.POINTER(Seg)}
    for n, types in want.items():
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % n, text).group(1)
        got = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", " *").strip() for a in args.split(",")]
        assert got == types, (n, got)
        assert _lib.SIGNATURES[n] == (C.c_int, [ctype[t] for t in types])
    # the two structs: field order and size are part of the ABI
    body = re.search(r"typedef struct ldit_opt_state \{(.*?)\} ldit_opt_state;", text, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", body)
    assert tuple(f for _, f in fields) == _lib.OPT_STATE_FIELDS == oo.FIELDS
    assert [t for t, _ in fields] == ["int32_t"] * 5 + ["float"] * 5 and C.sizeof(_lib.LditOptState) == 40
    body = re.search(r"typedef struct ldit_opt_segment \{(.*?)\} ldit_opt_segment;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in Seg._fields_] == ["p", "g", "m", "v", "n", "bf16_mirror"] and C.sizeof(Seg) == 48


def _segs(*rows):
    arr = (Seg * max(len(rows), 1))()
    for s, (p, g, m, v, n, mirror) in zip(arr, rows):
        s.p, s.g, s.m, s.v, s.n, s.bf16_mirror = p, g, m, v, n, mirror
    return arr


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    good = (16, 32, 48, 64, 8, None)
    ST = 256

    def check(segs=_segs(good), S=1, state=ST):
        return lib.ldit_grads_check_multi_f32(segs, S, state, None)

    def update(segs=_segs(good), S=1, state=ST):
        return lib.ldit_adamw_multi_f32(segs, S, state, 0.9, 0.999, 1e-8, 0.0, 1.0, None)

    for fn in (check, update):
        assert fn(S=-1) == _lib.LDIT_EINVAL and "negative" in err()
        assert fn(segs=None) == _lib.LDIT_EINVAL and "null" in err()
        assert fn(state=None) == _lib.LDIT_EINVAL and "state" in err()
        assert fn(state=258) == _lib.LDIT_EINVAL and "aligned" in err()
        assert fn(segs=_segs((16, 32, 48, 64, -1, None))) == _lib.LDIT_EINVAL and "negative length" in err()
        assert fn(segs=_segs((16, None, 48, 64, 8, None))) == _lib.LDIT_EINVAL and "null" in err()
        assert fn(segs=_segs((16, 34, 48, 64, 8, None))) == _lib.LDIT_EINVAL and "4-byte" in err()
        assert fn(segs=_segs(good, (16, 32, 48, 64, -5, None)), S=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    for k in (0, 2, 3):                                                                # the update needs p, m and v as well
        row = list(good)
        row[k] = None
        assert update(segs=_segs(tuple(row))) == _lib.LDIT_EINVAL and "null" in err()
        row[k] = 18
        assert update(segs=_segs(tuple(row))) == _lib.LDIT_EINVAL and "4-byte" in err()
    assert update(segs=_segs((16, 32, 48, 64, 8, 65))) == _lib.LDIT_EINVAL and "mirror" in err()

    def advance(state=ST, b1=0.9, b2=0.999, growth=2.0, backoff=0.5, interval=2000):
        return lib.ldit_opt_advance(state, b1, b2, growth, backoff, interval, None)

    assert advance(state=None) == _lib.LDIT_EINVAL and "state" in err()
    assert advance(b1=1.0) == _lib.LDIT_EINVAL and advance(b2=-0.1) == _lib.LDIT_EINVAL and "betas" in err()
    assert advance(growth=0.5) == _lib.LDIT_EINVAL and advance(backoff=0.0) == _lib.LDIT_EINVAL and advance(backoff=2.0) == _lib.LDIT_EINVAL
    assert advance(b1=float("nan")) == _lib.LDIT_EINVAL and advance(growth=float("nan")) == _lib.LDIT_EINVAL
    assert advance(interval=0) == _lib.LDIT_EINVAL and "growth_interval" in err()

    if not torch.cuda.is_available():
        # no device: the library's HIP error, for empty work too - there is nothing to fall back to.  (Where a device exists these
        # well-formed calls would launch on made-up addresses; there only the launch-free ones are made.)
        assert check() == _lib.LDIT_EHIP and "hip" in err().lower()
        assert update() == _lib.LDIT_EHIP and advance() == _lib.LDIT_EHIP
        assert check(S=0) == _lib.LDIT_EHIP and update(segs=_segs((None, None, None, None, 0, None))) == _lib.LDIT_EHIP
    else:
        assert check(S=0) == _lib.LDIT_OK and update(segs=_segs((None, None, None, None, 0, None))) == _lib.LDIT_OK     # nothing to launch


def test_state_machine_follows_torch_grad_scaler():
    """The oracle's advance() against a real torch.amp.GradScaler + optimizer on the CPU through growth (interval 2), single and
    repeated back-offs and a skip right before a growth."""
    scaler = torch.amp.GradScaler("cpu", init_scale=8.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    p = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.AdamW([p], lr=0.1)
    st = oo.new_state(scale=8.0, lr=0.1)
    taken = 0
    for bad in [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0]:
        opt.zero_grad()
        before = p.detach().clone()
        scaler.scale((p * (float("inf") if bad else 1.0)).sum()).backward()
        used = scaler.get_scale()
        scaler.step(opt)
        scaler.update()
        st = oo.advance(oo.check(st, [p.grad.numpy()]), growth_interval=2)
        taken += 1 - bad
        assert st["skip"] == bad and torch.equal(before, p.detach()) == bool(bad)
        assert st["inv_scale_used"] == 1.0 / used and st["found_inf"] == 0
        assert st["scale"] == scaler.get_scale() and st["growth_tracker"] == int(scaler._growth_tracker.item())
        assert st["step"] == taken == int(opt.state[p]["step"])
    assert st["skipped_steps"] == 4 and st["step"] == 8 and st["scale"] == 4.0
    assert st["bc1"] == 1.0 - 0.9 ** 8 and st["bc2_sqrt"] == (1.0 - 0.999 ** 8) ** 0.5
    # a constant scale: growth and back-off 1 (loss_scaling=False) still skip and count
    st = oo.new_state(scale=1.0)
    st["found_inf"] = 1
    st = oo.advance(st, growth_factor=1.0, backoff_factor=1.0, growth_interval=1)
    assert (st["scale"], st["skip"], st["skipped_steps"], st["step"]) == (1.0, 1, 1, 0)
    st = oo.advance(st, growth_factor=1.0, backoff_factor=1.0, growth_interval=1)
    assert (st["scale"], st["skip"], st["step"], st["growth_tracker"]) == (1.0, 0, 1, 0)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_restatement_follows_torch_adamw_in_float64(wd):
    rng = np.random.RandomState(3)
    p0 = rng.normal(0, 1, size=257)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([ref], lr=1e-2, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    st = oo.new_state(scale=1024.0, lr=1e-2)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for i in range(5):
        g = rng.normal(0, 0.1, size=257)
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        st = oo.advance(st)
        p, m, v = oo.adamw(p, g * 1024.0, m, v, st, weight_decay=wd)                   # scaled gradients in, unscaled by the state
    np.testing.assert_allclose(p, ref.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(m, opt.state[ref]["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(v, opt.state[ref]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-20)
    st["found_inf"] = 1
    st = oo.advance(st)
    q, _, _ = oo.adamw(p, np.full(257, np.nan), m, v, st)
    np.testing.assert_array_equal(q, p)                                                # a skipped step changes nothing


def test_front_ends_refuse_wrong_dtypes_and_devices():
    f = lambda n=4: torch.zeros(n)                                                     # noqa: E731
    state = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(ValueError, match="float32"):
        ops.grads_check_multi([f().double()], state)
    with pytest.raises(ValueError, match="float32"):
        ops.adamw_multi([f()], [f().half()], [f()], [f()], state)
    with pytest.raises(ValueError, match="contiguous"):
        ops.adamw_multi([torch.zeros(4, 2)[:, 0]], [f()], [f()], [f()], state)
    with pytest.raises(ValueError, match="GPU"):
        ops.grads_check_multi([f()], state)
    with pytest.raises(ValueError, match="GPU"):
        ops.adamw_multi([f()], [f()], [f()], [f()], state)
    with pytest.raises(ValueError, match="GPU"):
        ops.opt_advance(state)
    with pytest.raises(ValueError, match="int32"):
        ops.opt_advance(torch.zeros(10))
    with pytest.raises(ValueError, match="int32"):
        ops.grads_check_multi([f()], torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError, match="segments"):
        ops.adamw_multi([f(), f()], [f()], [f()], [f()], state)
    assert ops.OPT_MAX_SEGMENTS == 64
    host = ops.new_opt_state("cpu", scale=1024.0, lr=3e-4)
    assert host.dtype == torch.int32 and host[:5].tolist() == [0] * 5
    assert host.view(torch.float32)[5:].tolist() == [1024.0, 1.0 / 1024.0, float(np.float32(3e-4)), 1.0, 1.0]


def test_detector_train_step_surface_and_refusals():
    assert training.DetectorTrainStep is not None and training.TrainStep is not None  # exported side by side
    from layoutdit_amd.detector_training import DetectorTrainStep
    assert training.DetectorTrainStep is DetectorTrainStep
    with pytest.raises(RuntimeError, match="train"):
        DetectorTrainStep(LayoutDetectionModel(config=cfgs.vit_micro()).eval())
    with pytest.raises(ValueError, match="GPU"):                                       # train mode, but no CPU path
        DetectorTrainStep(LayoutDetectionModel(config=cfgs.vit_micro()).train())
    small = cfgs.DiTConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512)
    for kw in ({"compute_dtype": "mxfp8"}, {"compute_dtype": "fp8"}):
        with pytest.raises(NotImplementedError, match="TrainStep"):
            DetectorTrainStep(LayoutDetectionModel(config=small, **kw).train())
    with pytest.raises(TypeError, match="LayoutDetectionModel"):
        DetectorTrainStep(torch.nn.Linear(2, 2))
    assert "DetectorTrainStep" in training.TrainStep.__doc__ and "outside this repository" not in training.TrainStep.__doc__
