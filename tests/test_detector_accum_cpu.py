"""CPU-only checks of gradient accumulation and data-parallel ranks under DetectorTrainStep: the C ABI declares,
exports and validates ldit_grads_accumulate_multi_f32 without a device; the segment table's capacity is what the kernel-argument
bound allows; the bucket's layout is a pure host function with 256-byte aligned slices; the constructor refuses what it cannot run.
No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

from layoutdit_amd import _lib, dp, ops
from layoutdit_amd import config as cfgs
from layoutdit_amd.detector_training import BUCKET_ALIGN, DetectorTrainStep, bucket_layout
from layoutdit_amd.modeling import LayoutDetectionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ldit_grads_accumulate_multi_f32"
Seg = _lib.LditAccSegment


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_point():
    text = _header()
    lib = _lib.load()
    assert re.search(r"\b%s\s*\(" % NAME, text), f"{NAME} not declared in include/ldit.h"
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text).group(1)
    got = [re.sub(r"\s*\w+$", "", a.strip()) for a in args.split(",")]
    assert got == ["const ldit_acc_segment *", "int32_t", "int32_t", "ldit_stream"]
    assert _lib.SIGNATURES[NAME] == (C.c_int, [C.POINTER(Seg), C.c_int32, C.c_int32, C.c_void_p])
    body = re.search(r"typedef struct ldit_acc_segment \{(.*?)\} ldit_acc_segment;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in Seg._fields_] == ["acc", "g", "n"]
    assert C.sizeof(Seg) == 24


def test_segments_per_launch_are_what_the_kernel_argument_bound_allows():
    """The launch's argument block is {segments, prefix table of one more int than segments, count}, 8-byte aligned, under the file's
    3 584 bytes: the exported count is the largest that fits, and the source's own constant and static_assert say the same."""
    def block_bytes(n):
        return -(-(C.sizeof(Seg) * n + 4 * (n + 1) + 4) // 8) * 8

    src = open(os.path.join(ROOT, "layoutdit_amd", "csrc", "optim_multi.hip")).read()
    assert int(re.search(r"constexpr int ACC_SEGS = (\d+);", src).group(1)) == ops.ACC_MAX_SEGMENTS == _lib.ACC_MAX_SEGMENTS
    assert re.search(r"static_assert\(sizeof\(AccLaunch\) <= 3584", src)
    assert block_bytes(ops.ACC_MAX_SEGMENTS) <= 3584 < block_bytes(ops.ACC_MAX_SEGMENTS + 1)
    assert ops.ACC_MAX_SEGMENTS == 127


def _segs(*rows):
    arr = (Seg * max(len(rows), 1))()
    for s, (acc, g, n) in zip(arr, rows):
        s.acc, s.g, s.n = acc, g, n
    return arr


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    good = (256, 512, 8)

    def fold(segs=_segs(good), S=1, overwrite=1):
        return lib.ldit_grads_accumulate_multi_f32(segs, S, overwrite, None)

    for ow in (0, 1):
        assert fold(segs=None, overwrite=ow) == _lib.LDIT_EINVAL and "null segment array" in err()
        assert fold(S=-1, overwrite=ow) == _lib.LDIT_EINVAL and "negative segment count" in err()
        assert fold(segs=_segs((256, 512, -1)), overwrite=ow) == _lib.LDIT_EINVAL and "negative length" in err()
        assert fold(segs=_segs((None, 512, 8)), overwrite=ow) == _lib.LDIT_EINVAL and "null pointer" in err()
        assert fold(segs=_segs((256, None, 8)), overwrite=ow) == _lib.LDIT_EINVAL and "null pointer" in err()
        assert fold(segs=_segs(good, (256, None, 1)), S=2, overwrite=ow) == _lib.LDIT_EINVAL and "segment 1" in err()
        assert fold(segs=_segs((258, 512, 8)), overwrite=ow) == _lib.LDIT_EINVAL and "4-byte" in err()
        # one segment whose grid alone passes the block bound of the file (2^31 - 1 workgroups of 1 024 elements)
        too_long = (2 ** 31 - 1) * 1024 + 1
        assert fold(segs=_segs((256, 512, too_long)), overwrite=ow) == _lib.LDIT_EUNSUPPORTED and "blocks" in err()
        assert fold(segs=_segs(good, (256, 512, too_long)), S=2, overwrite=ow) != _lib.LDIT_OK and "segment 1" in err()
    if not torch.cuda.is_available():
        # no device: the library's HIP error, for empty work too - there is nothing to fall back to.  (Where a device exists a
        # well-formed call would launch on made-up addresses; there only the launch-free ones are made.)
        assert fold() == _lib.LDIT_EHIP and "hip" in err().lower()
        assert fold(S=0) == _lib.LDIT_EHIP and fold(segs=_segs((None, None, 0))) == _lib.LDIT_EHIP
    else:
        assert fold(S=0) == _lib.LDIT_OK and fold(segs=_segs((None, None, 0))) == _lib.LDIT_OK      # empty segments: pointers not looked at


def test_front_end_refuses_wrong_dtypes_devices_and_lengths():
    f = lambda n=4: torch.zeros(n)                                                     # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        ops.grads_accumulate_multi([f()], [f().double()], True)
    with pytest.raises(ValueError, match="float32"):
        ops.grads_accumulate_multi([f().half()], [f()], False)
    with pytest.raises(ValueError, match="contiguous"):
        ops.grads_accumulate_multi([torch.zeros(4, 2)[:, 0]], [f()], True)
    with pytest.raises(ValueError, match="segments"):
        ops.grads_accumulate_multi([f(), f()], [f()], True)
    with pytest.raises(ValueError, match="length"):
        ops.grads_accumulate_multi([f(5)], [f(4)], True)
    with pytest.raises(ValueError, match="GPU"):
        ops.grads_accumulate_multi([f()], [f()], True)


def test_bucket_layout_is_a_pure_host_function_with_256_byte_slices():
    assert BUCKET_ALIGN * 4 == 256
    lengths = (5, 0, 1, 64, 65, 0, 1023, 1024, 1025, 7)
    offsets, total = bucket_layout(lengths)
    assert bucket_layout(list(lengths)) == (offsets, total) == bucket_layout(lengths)          # of the tuple of lengths, nothing else
    assert len(offsets) == len(lengths) and offsets[0] == 0
    assert all((4 * o) % 256 == 0 for o in offsets)
    for i in range(len(lengths) - 1):                                                        # disjoint, in order
        assert offsets[i] + lengths[i] <= offsets[i + 1]
    assert offsets[1] == offsets[2] == 64                                                     # a zero-length segment takes no room
    assert offsets[5] == offsets[6]
    assert total >= offsets[-1] + lengths[-1]                                                 # the total covers the last slice
    assert total - (offsets[-1] + lengths[-1]) < BUCKET_ALIGN                                 # ... and no more than its padding
    assert offsets == (0, 64, 64, 128, 192, 320, 320, 1344, 2368, 3456) and total == 3520
    assert bucket_layout(()) == ((), 0) and bucket_layout((0, 0)) == ((0, 0), 0)
    assert bucket_layout((64,)) == ((0,), 64) and bucket_layout((1 << 33,))[1] == 1 << 33
    with pytest.raises(ValueError, match="negative"):
        bucket_layout((4, -1))


def test_constructor_refusals():
    model = LayoutDetectionModel(config=cfgs.vit_micro()).train()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="accumulate"):
            DetectorTrainStep(model, accumulate=bad)
    assert not torch.distributed.is_initialized()
    with pytest.raises(RuntimeError, match="process group"):
        DetectorTrainStep(model, rank=dp.Rank(rank=1, world=2, local_rank=0, backend="gloo"))
    with pytest.raises(RuntimeError, match="process group"):
        DetectorTrainStep(model, accumulate=2, rank=dp.Rank(rank=0, world=4, local_rank=0, backend="nccl"), broadcast_parameters=False)
    with pytest.raises(TypeError, match="Rank"):
        DetectorTrainStep(model, rank=0)
    # a one-rank Rank needs no group, and the defaults are what they were: refused for what they always were refused for
    with pytest.raises(ValueError, match="GPU"):
        DetectorTrainStep(model, accumulate=2, rank=dp.Rank(rank=0, world=1, local_rank=0, backend="gloo"))
    with pytest.raises(ValueError, match="GPU"):
        DetectorTrainStep(model)
