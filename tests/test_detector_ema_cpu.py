"""CPU-only checks of the moving average of the weights under DetectorTrainStep: the C ABI declares, exports and
validates ldit_adamw_ema_groups_multi_f32 and ldit_swap_multi_f32 without a device; the two segment tables' capacities are what the
kernel-argument bound allows; the float64 restatement tests/ema_oracle.py is torch.lerp's arithmetic with the documented decay; the
front ends and the constructor refuse what they cannot run.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib, ops
from layoutdit_amd import config as cfgs
from layoutdit_amd.detector_training import DetectorTrainStep
from layoutdit_amd.modeling import LayoutDetectionModel
from tests import ema_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA, SWAP = "ldit_adamw_ema_groups_multi_f32", "ldit_swap_multi_f32"
Seg, Hyper, Swap = _lib.LditOptSegment, _lib.LditOptHyper, _lib.LditSwapSegment


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)


def _args(text, name):
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text).group(1)
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in args.split(",")]


def test_header_declares_and_library_exports_the_entry_points():
    text = _header()
    lib = _lib.load()
    for name in (EMA, SWAP):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared in include/ldit.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    assert _args(text, EMA) == ["const ldit_opt_segment *", "const ldit_opt_hyper *", "void *const *", "int32_t", "const ldit_opt_state *",
                                "const ldit_clip_state *", "double", "double", "float", "double", "int32_t", "ldit_stream"]
    assert _lib.SIGNATURES[EMA] == (C.c_int, [C.POINTER(Seg), C.POINTER(Hyper), C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_double, C.c_double, C.c_float, C.c_double, C.c_int32, C.c_void_p])
    assert _args(text, SWAP) == ["const ldit_swap_segment *", "int32_t", "ldit_stream"]
    assert _lib.SIGNATURES[SWAP] == (C.c_int, [C.POINTER(Swap), C.c_int32, C.c_void_p])
    body = re.search(r"typedef struct ldit_swap_segment \{(.*?)\} ldit_swap_segment;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in Swap._fields_] == ["a", "b", "n", "bf16_mirror"]
    assert C.sizeof(Swap) == 32 and C.sizeof(Seg) == 48                            # the public update segment did not grow


def test_segments_per_launch_are_what_the_kernel_argument_bound_allows():
    """An argument block is {segments, what rides beside each, prefix table of one more int than segments, count}, 8-byte aligned,
    under the file's 3 584 bytes: each exported count is the largest that fits, and the source's constants and static_asserts agree."""
    def block_bytes(per_segment, n):
        return -(-(per_segment * n + 4 * (n + 1) + 4) // 8) * 8

    src = open(os.path.join(ROOT, "layoutdit_amd", "csrc", "optim_multi.hip")).read()
    assert int(re.search(r"constexpr int EMA_SEGS = (\d+);", src).group(1)) == ops.EMA_MAX_SEGMENTS == _lib.EMA_MAX_SEGMENTS == 52
    assert int(re.search(r"constexpr int SWAP_SEGS = (\d+);", src).group(1)) == ops.SWAP_MAX_SEGMENTS == _lib.SWAP_MAX_SEGMENTS == 99
    assert re.search(r"static_assert\(sizeof\(EmaLaunch\) <= 3584", src) and re.search(r"static_assert\(sizeof\(SwapLaunch\) <= 3584", src)
    ema_segment = C.sizeof(Seg) + C.sizeof(Hyper) + C.sizeof(C.c_void_p)             # the segment, its hyper-parameters, its shadow
    assert block_bytes(ema_segment, ops.EMA_MAX_SEGMENTS) <= 3584 < block_bytes(ema_segment, ops.EMA_MAX_SEGMENTS + 1)
    assert block_bytes(C.sizeof(Swap), ops.SWAP_MAX_SEGMENTS) <= 3584 < block_bytes(C.sizeof(Swap), ops.SWAP_MAX_SEGMENTS + 1)
    # the capacities of the launches that exist already are what they were
    assert (ops.OPT_MAX_SEGMENTS, ops.OPT_GROUP_SEGMENTS, ops.ACC_MAX_SEGMENTS) == (64, 48, 127)


def _segs(*rows):
    arr = (Seg * max(len(rows), 1))()
    for s, (p, g, m, v, n, mirror) in zip(arr, rows):
        s.p, s.g, s.m, s.v, s.n, s.bf16_mirror = p, g, m, v, n, mirror
    return arr


def _hyper(n=1):
    arr = (Hyper * n)()
    for h in arr:
        h.lr_scale, h.weight_decay = 1.0, 0.0
    return arr


def _ptrs(*values):
    return (C.c_void_p * len(values))(*values)


def _swaps(*rows):
    arr = (Swap * max(len(rows), 1))()
    for s, (a, b, n, mirror) in zip(arr, rows):
        s.a, s.b, s.n, s.bf16_mirror = a, b, n, mirror
    return arr


def test_update_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    good = (256, 512, 768, 1024, 8, None)
    state = 4096

    def update(segs=_segs(good), hyper=_hyper(), ema=_ptrs(2048), S=1, decay=0.9, warmup=1, clip=None, b1=0.9):
        return lib.ldit_adamw_ema_groups_multi_f32(segs, hyper, ema, S, state, clip, b1, 0.999, 1e-8, decay, warmup, None)

    for decay in (1.0, -0.1, 1.5, float("nan")):
        assert update(decay=decay) == _lib.LDIT_EINVAL and "ema_decay must lie in [0, 1)" in err()
    assert update(segs=None) == _lib.LDIT_EINVAL and "null segment array" in err()
    assert update(S=-1) == _lib.LDIT_EINVAL and "negative segment count" in err()
    assert update(ema=_ptrs(2050)) == _lib.LDIT_EINVAL and "shadow" in err() and "4-byte" in err()
    assert update(segs=_segs(good, good), hyper=_hyper(2), ema=_ptrs(2048, 2049), S=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    assert update(segs=_segs((256, 512, 768, 1024, 8, 2049))) == _lib.LDIT_EINVAL and "mirror" in err()
    assert update(segs=_segs((256, 512, 768, 1024, -1, None))) == _lib.LDIT_EINVAL and "negative length" in err()
    assert update(segs=_segs((None, 512, 768, 1024, 8, None))) == _lib.LDIT_EINVAL and "null pointer" in err()
    assert update(segs=_segs((258, 512, 768, 1024, 8, None))) == _lib.LDIT_EINVAL and "4-byte" in err()
    assert update(hyper=None) == _lib.LDIT_EINVAL and "hyper" in err()
    assert update(clip=2) == _lib.LDIT_EINVAL and "clip" in err()
    assert update(b1=1.0) == _lib.LDIT_EINVAL and "betas" in err()
    too_long = (2 ** 31 - 1) * 1024 + 1
    assert update(segs=_segs((256, 512, 768, 1024, too_long, None))) == _lib.LDIT_EUNSUPPORTED and "2^41" in err()
    if not torch.cuda.is_available():
        # no device: the library's HIP error, after every argument passed - a null shadow and a null shadow array are both legal
        assert update() == _lib.LDIT_EHIP and "hip" in err().lower()
        assert update(ema=_ptrs(None)) == _lib.LDIT_EHIP and update(ema=None) == _lib.LDIT_EHIP and update(decay=0.0, warmup=0) == _lib.LDIT_EHIP
    else:
        assert update(S=0) == _lib.LDIT_OK


def test_swap_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    good = (256, 512, 8, None)

    def swap(segs=_swaps(good), S=1):
        return lib.ldit_swap_multi_f32(segs, S, None)

    assert swap(segs=None) == _lib.LDIT_EINVAL and "null segment array" in err()
    assert swap(S=-1) == _lib.LDIT_EINVAL and "negative segment count" in err()
    assert swap(segs=_swaps((256, 512, -1, None))) == _lib.LDIT_EINVAL and "negative length" in err()
    assert swap(segs=_swaps((None, 512, 8, None))) == _lib.LDIT_EINVAL and "null pointer" in err()
    assert swap(segs=_swaps((256, None, 8, None))) == _lib.LDIT_EINVAL and "null pointer" in err()
    assert swap(segs=_swaps((258, 512, 8, None))) == _lib.LDIT_EINVAL and "4-byte" in err()
    assert swap(segs=_swaps((256, 514, 8, None))) == _lib.LDIT_EINVAL and "4-byte" in err()
    assert swap(segs=_swaps((256, 512, 8, 1025))) == _lib.LDIT_EINVAL and "mirror" in err()
    assert swap(segs=_swaps(good, (256, 512, 8, 1025)), S=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    too_long = (2 ** 31 - 1) * 1024 + 1
    assert swap(segs=_swaps((256, 512, too_long, None))) == _lib.LDIT_EUNSUPPORTED and "2^41" in err()
    if not torch.cuda.is_available():
        assert swap() == _lib.LDIT_EHIP and "hip" in err().lower()
        assert swap(S=0) == _lib.LDIT_EHIP and swap(segs=_swaps((None, None, 0, None))) == _lib.LDIT_EHIP
    else:
        assert swap(S=0) == _lib.LDIT_OK and swap(segs=_swaps((None, None, 0, None))) == _lib.LDIT_OK   # empty segments: pointers not looked at


def test_decay_follows_the_warmup_formula():
    for decay in (0.0, 0.5, 0.9, 0.9999):
        for n in (1, 2, 3, 10, 100, 10 ** 6):
            assert eo.ema_decay_at(n, decay) == min(decay, (1 + n) / (10 + n))
            assert eo.ema_decay_at(n, decay, warmup=False) == decay
    assert eo.ema_decay_at(1, 0.9999) == 2 / 11 and eo.ema_decay_at(3, 0.9999) == 4 / 13
    assert eo.ema_decay_at(89990, 0.9999) == 0.9999 and eo.ema_decay_at(89989, 0.9999) < 0.9999        # where the warmup hands over
    steps = [eo.ema_decay_at(n, 0.9999) for n in range(1, 2000)]
    assert all(a < b for a, b in zip(steps, steps[1:]))                                                 # it only ever rises
    assert eo.ema_weight(3, 0.9999) == float(np.float32(1.0 - 4 / 13)) and eo.ema_weight(3, 0.25, warmup=False) == 0.75


def test_oracle_is_lerp_in_float64():
    rng = np.random.RandomState(0)
    e, p = rng.normal(size=257), rng.normal(size=257)
    for d in (0.0, 2 / 11, 0.5, 0.9, 0.9999):
        got = eo.ema(e, p, d)
        want = torch.lerp(torch.from_numpy(e), torch.from_numpy(p), 1.0 - d).numpy()
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(np.float64).eps * 8)
    assert np.array_equal(eo.ema(e, p, 0.0), e + (p - e)) and np.array_equal(eo.ema(e.astype(np.float32), p, 0.5), eo.ema(e.astype(np.float32).astype(np.float64), p, 0.5))


def test_front_ends_refuse_wrong_dtypes_devices_and_lengths():
    f = lambda n=4: torch.zeros(n)                                                     # noqa: E731
    state = torch.zeros(len(_lib.OPT_STATE_FIELDS), dtype=torch.int32)

    def update(shadows, decay=0.9, p=None, scales=(1.0,)):
        ops.adamw_ema_groups_multi([f() if p is None else p], [f()], [f()], [f()], state, list(scales), [0.0], shadows, decay)

    with pytest.raises(ValueError, match="float32"):
        update([f().double()])
    with pytest.raises(ValueError, match="float32"):
        update([f()], p=f().half())
    with pytest.raises(ValueError, match="contiguous"):
        update([torch.zeros(4, 2)[:, 0]])
    with pytest.raises(ValueError, match="shadows"):
        update([f(), f()])
    with pytest.raises(ValueError, match="elements"):
        update([f(5)])
    with pytest.raises(ValueError, match="ema_decay"):
        update([f()], decay=1.0)
    with pytest.raises(ValueError, match="ema_decay"):
        update([f()], decay=-0.1)
    with pytest.raises(ValueError, match="lr_scale"):
        update([f()], scales=(-1.0,))
    with pytest.raises(ValueError, match="GPU"):
        update([f()])
    with pytest.raises(ValueError, match="GPU"):
        update([None])
    with pytest.raises(ValueError, match="float32"):
        ops.swap_multi([f()], [f().double()])
    with pytest.raises(ValueError, match="float32"):
        ops.swap_multi([f().half()], [f()])
    with pytest.raises(ValueError, match="contiguous"):
        ops.swap_multi([torch.zeros(4, 2)[:, 0]], [f()])
    with pytest.raises(ValueError, match="segments"):
        ops.swap_multi([f(), f()], [f()])
    with pytest.raises(ValueError, match="length"):
        ops.swap_multi([f(5)], [f(4)])
    with pytest.raises(ValueError, match="mirrors"):
        ops.swap_multi([f()], [f()], [torch.zeros(4, dtype=torch.bfloat16)])          # a mirror lives on the GPU
    with pytest.raises(ValueError, match="GPU"):
        ops.swap_multi([f()], [f()])
    ops.swap_multi([], [])                                                            # nothing to exchange: no launch, no device needed


def test_constructor_refusals():
    model = LayoutDetectionModel(config=cfgs.vit_micro()).train()
    for bad in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            DetectorTrainStep(model, ema_decay=bad)
    # a legal decay and the default are refused for what a CPU model always was refused for
    with pytest.raises(ValueError, match="GPU"):
        DetectorTrainStep(model, ema_decay=0.9999, ema_warmup=False)
    with pytest.raises(ValueError, match="GPU"):
        DetectorTrainStep(model)
