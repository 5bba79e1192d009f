"""Host-side checks of the uint8 image path (no GPU, no launch): the three ``*_u8`` entries are declared, bound and exported under the
unchanged ABI version and refuse on the host what their siblings refuse plus a bad ``interleaved``; ``ops.image_list_args`` tells the
two memory layouts apart and refuses a mixed list; ``stage_images`` packs a ragged batch into one buffer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import layoutdit_amd
from layoutdit_amd import _lib, data, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldit_preprocess_u8", "ldit_embed_bf16_images_u8", "ldit_vit_forward_images_u8")
EINVAL, EUNSUPPORTED = _lib.LDIT_EINVAL, _lib.LDIT_EUNSUPPORTED


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), f"{n} not declared in include/ldit.h"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    # `interleaved` stands where half_in stands, or is added behind the three arrays
    sig = _lib.SIGNATURES
    assert sig["ldit_embed_bf16_images_u8"] == sig["ldit_embed_bf16_images"]
    assert sig["ldit_vit_forward_images_u8"] == sig["ldit_vit_forward_images"]
    f32 = sig["ldit_preprocess_f32"][1]
    assert sig["ldit_preprocess_u8"] == (C.c_int, f32[:3] + [C.c_int32] + f32[3:])
    for n in NAMES:
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % n, text).group(1)
        assert "int32_t interleaved" in args and len(args.split(",")) == len(sig[n][1])


def _lists(B=2):
    return (C.c_void_p * B)(*[4096 * (i + 1) + 1 for i in range(B)]), (C.c_int32 * B)(*[7] * B), (C.c_int32 * B)(*[5] * B)


def _pre(images="ok", heights="ok", widths="ok", interleaved=0, B=2, in_ch=3, mean=0.5, std=0.5, out_h=8, out_w=8, out=1 << 20):
    p, h, w = _lists(max(B, 1) if B < 100 else 2)
    return (p if images == "ok" else images, h if heights == "ok" else heights, w if widths == "ok" else widths, interleaved, B, in_ch,
            mean, std, out_h, out_w, out, None)


PRE_REFUSALS = [
    (dict(images=None), EINVAL, "null"), (dict(heights=None), EINVAL, "null"), (dict(widths=None), EINVAL, "null"),
    (dict(out=None), EINVAL, "null"),
    (dict(B=0), EINVAL, "geometry"), (dict(B=65536), EINVAL, "geometry"), (dict(in_ch=0), EINVAL, "geometry"),
    (dict(out_h=0), EINVAL, "geometry"), (dict(out_w=-1), EINVAL, "geometry"),
    (dict(std=0.0), EINVAL, "std"), (dict(std=-1.0), EINVAL, "std"), (dict(std=float("nan")), EINVAL, "std"),
    (dict(B=2, out_h=1 << 15, out_w=1 << 15), EUNSUPPORTED, "2^31"),
    (dict(interleaved=2), EINVAL, "interleaved"), (dict(interleaved=-1), EINVAL, "interleaved"),
    (dict(interleaved=2, images=None), EINVAL, ""),
]


@pytest.mark.parametrize("kwargs,code,fragment", PRE_REFUSALS)
def test_preprocess_u8_refuses_on_the_host(kwargs, code, fragment):
    """The image pointers are small odd integers: a call that got past the host checks would need a device, so a pass means
    'refused before any launch'.  The same cases, with the same codes, as ldit_preprocess_f32."""
    lib = _lib.load()
    rc = lib.ldit_preprocess_u8(*_pre(**kwargs))
    msg = lib.ldit_last_error().decode()
    assert rc == code and fragment in msg, (rc, msg)
    if "interleaved" not in kwargs:                                # the sibling refuses the same call the same way
        a = _pre(**kwargs)
        assert lib.ldit_preprocess_f32(*(a[:3] + a[4:])) == code


def _embed(images="ok", interleaved=0, std=0.5, pw=4096, pb=8192, cls=12288, pos=16384, out=20480, scratch=24576, B=2, in_ch=3, img_h=32,
           img_w=32, p=16, Cc=32):
    ptrs, h, w = _lists(2)
    return (ptrs if images == "ok" else images, h, w, interleaved, 0.5, std, pw, pb, cls, pos, out, scratch, B, in_ch, img_h, img_w, p, Cc, None)


EMBED_REFUSALS = [
    (dict(images=None), EINVAL, "null"), (dict(pw=None), EINVAL, "null"), (dict(scratch=None), EINVAL, "null"),
    (dict(B=0), EINVAL, "empty"), (dict(B=65536), EINVAL, "empty"), (dict(in_ch=0), EINVAL, "empty"),
    (dict(img_h=40), EINVAL, "multiple of patch"), (dict(std=0.0), EINVAL, "std"),
    (dict(out=20480 + 4), EINVAL, "aligned"), (dict(Cc=30), EINVAL, "aligned"),
    (dict(in_ch=1, p=4), EUNSUPPORTED, "multiple of 64"),
    (dict(B=65535, img_h=2048, img_w=2048), EUNSUPPORTED, "2^31"),
    (dict(interleaved=2), EINVAL, "interleaved"), (dict(interleaved=-1), EINVAL, "interleaved"),
]


@pytest.mark.parametrize("kwargs,code,fragment", EMBED_REFUSALS)
def test_embed_bf16_images_u8_refuses_on_the_host(kwargs, code, fragment):
    lib = _lib.load()
    rc = lib.ldit_embed_bf16_images_u8(*_embed(**kwargs))
    msg = lib.ldit_last_error().decode()
    assert rc == code and fragment in msg, (rc, msg)
    assert msg.startswith("embed_bf16_images_u8:")
    if "interleaved" not in kwargs:
        assert lib.ldit_embed_bf16_images(*_embed(**kwargs)) == code


def _cfg(dtype=_lib.DTYPE_BF16, img=32):
    c = layoutdit_amd.vit_micro()
    lc = _lib.LditCfg(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads, mlp=c.intermediate_size,
                      patch=c.patch_size, in_ch=3, img_h=img, img_w=img, n_taps=1, ln_eps=c.layer_norm_eps, dtype=dtype, flags=0)
    lc.taps[0] = c.num_hidden_layers
    return lc


def _fwd(lc, images="ok", interleaved=0, std=0.5, batch=2, packed=4096, taps="ok", ws=1 << 20, ws_bytes=None):
    ptrs, h, w = _lists(2)
    tap = (C.c_void_p * 1)(1 << 24)
    need = _lib.load().ldit_workspace_bytes(C.byref(lc), max(batch, 1))
    return (C.byref(lc), packed, ptrs if images == "ok" else images, h, w, interleaved, 0.5, std, batch, tap if taps == "ok" else taps, ws,
            need if ws_bytes is None else ws_bytes, None)


FWD_REFUSALS = [
    (dict(images=None), EINVAL, "image list"), (dict(std=0.0), EINVAL, "image list"), (dict(batch=65536), EINVAL, "image list"),
    (dict(batch=0), EINVAL, "batch"), (dict(packed=None), EINVAL, "null"), (dict(ws=None), EINVAL, "null"),
    (dict(packed=4096 + 4), EINVAL, "aligned"), (dict(taps=None), EINVAL, "tap_out"),
    (dict(ws_bytes=16), _lib.LDIT_EWORKSPACE, "workspace"),
    (dict(interleaved=2), EINVAL, "interleaved"), (dict(interleaved=-1), EINVAL, "interleaved"),
]


@pytest.mark.parametrize("dtype", [_lib.DTYPE_F32, _lib.DTYPE_BF16])
@pytest.mark.parametrize("kwargs,code,fragment", FWD_REFUSALS)
def test_vit_forward_images_u8_refuses_on_the_host(kwargs, code, fragment, dtype):
    lib = _lib.load()
    lc = _cfg(dtype)
    rc = lib.ldit_vit_forward_images_u8(*_fwd(lc, **kwargs))
    msg = lib.ldit_last_error().decode()
    assert rc == code and fragment in msg, (rc, msg)
    if "interleaved" not in kwargs:
        assert lib.ldit_vit_forward_images(*_fwd(lc, **kwargs)) == code


# ---- ops.image_list_args: dtype and layout of a list (the device is looked at last, so the rules can be read without one) -----------
def _hwc(h, w, c=3, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8))


def test_layouts_are_told_apart_by_strides():
    inter = _hwc(5, 7).permute(2, 0, 1)
    planar = inter.contiguous()
    assert inter.stride() == (1, 21, 3) and planar.stride() == (35, 7, 1)
    assert ops._u8_layouts(planar, "x") == (True, False) and ops._u8_layouts(inter, "x") == (False, True)
    # an axis of length 1 has no stride to speak of: such an image fits the list it is in
    assert ops._u8_layouts(_hwc(1, 1).permute(2, 0, 1), "x") == (True, True)
    assert ops._u8_layouts(_hwc(1, 1).permute(2, 0, 1).contiguous(), "x") == (True, True)
    assert ops._u8_layouts(_hwc(1, 7).permute(2, 0, 1), "x") == (False, True)
    assert ops._u8_layouts(_hwc(7, 1).permute(2, 0, 1), "x") == (False, True)
    assert ops._u8_layouts(_hwc(4, 6, c=1).permute(2, 0, 1), "x") == (True, True)
    for bad in (planar[:, :, ::2], planar[:, ::2], planar.flip(0)[:, :, :], inter[:, :, 1:], _hwc(5, 7).permute(2, 1, 0),
                torch.zeros(3, 5, 8, dtype=torch.uint8)[:, :, :7]):
        if bad.is_contiguous():
            continue
        with pytest.raises(ValueError, match="strides"):
            ops._u8_layouts(bad, "x")
    with pytest.raises(ValueError, match=r"\[C, h, w\]"):
        ops._u8_layouts(torch.zeros(5, 7, dtype=torch.uint8), "x")


def test_one_list_has_one_dtype_and_one_layout():
    inter, planar = _hwc(5, 7).permute(2, 0, 1), _hwc(6, 4).permute(2, 0, 1).contiguous()
    one = _hwc(1, 1).permute(2, 0, 1)
    with pytest.raises(ValueError, match=r"images\[1\].*one memory layout"):
        ops.image_list_args([inter, planar])
    with pytest.raises(ValueError, match=r"images\[2\].*one memory layout"):
        ops.image_list_args([one, planar, inter])
    with pytest.raises(ValueError, match=r"images\[1\].*uint8"):
        ops.image_list_args([planar, planar.float() / 255])
    with pytest.raises(ValueError):                  # (an fp32 list is checked as before, device first: the GPU tests name images[1])
        ops.image_list_args([planar.float() / 255, planar])
    with pytest.raises(ValueError, match=r"images\[1\].*strides"):
        ops.image_list_args([planar, planar[:, :, ::2]])
    with pytest.raises(ValueError, match="same C"):
        ops.image_list_args([inter, _hwc(5, 7, c=4).permute(2, 0, 1)])
    # well-formed lists get as far as the device check (there is no CPU path), in either layout and with a 1 x 1 image among them
    for good in ([planar, planar], [inter, inter], [one, inter], [one, planar], [one]):
        with pytest.raises(ValueError, match="on the GPU"):
            ops.image_list_args(good)
    with pytest.raises(ValueError, match="empty"):
        ops.image_list_args([])


@pytest.mark.parametrize("dtype", [torch.int8, torch.bfloat16, torch.int32, torch.float64])
def test_other_dtypes_are_still_refused(dtype):
    img = torch.zeros(3, 4, 4, dtype=dtype)
    for fn in (ops.image_list_args, ops.preprocess, layoutdit_amd.DetectorInputTransform()):
        with pytest.raises(ValueError):
            fn([img])
    with pytest.raises(ValueError):
        ops.image_list_args([torch.zeros(3, 4, 4, dtype=torch.uint8), img])


def test_input_transform_leaves_an_interleaved_page_where_it_is():
    tr = layoutdit_amd.DetectorInputTransform()
    inter = _hwc(5, 7).permute(2, 0, 1)
    got = tr._operands([inter, inter.contiguous()])
    assert got[0] is inter and got[0].stride() == (1, 21, 3)
    f = torch.rand(5, 7, 3).permute(2, 0, 1)
    assert tr._operands([f])[0].is_contiguous()                     # fp32 / fp16 as before


# ---- stage_images ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (7, 1), (31, 17), (12, 20)]


def test_stage_images_hwc_views_contents_and_one_buffer():
    pages = [_hwc(h, w, seed=i).numpy() for i, (h, w) in enumerate(SIZES)]
    pages[2] = torch.from_numpy(pages[2])                          # arrays and tensors, mixed
    pages[3] = np.ascontiguousarray(pages[3][:, ::-1])[:, ::-1]    # a non-contiguous input is packed densely
    out = data.stage_images(pages, "cpu", layout="hwc")
    assert len(out) == len(SIZES)
    base, off = out[0].untyped_storage().data_ptr(), 0
    for v, p, (h, w) in zip(out, pages, SIZES):
        assert v.dtype == torch.uint8 and tuple(v.shape) == (3, h, w) and v.device.type == "cpu"
        assert ops._u8_layouts(v, "v")[1]                          # interleaved: what the *_u8 entries take with interleaved = 1
        assert all(n == 1 or s == q for n, s, q in zip(v.shape, v.stride(), (1, 3 * w, 3)))
        assert v.untyped_storage().data_ptr() == base and v.storage_offset() == off         # one buffer, packed back to back
        assert torch.equal(v, torch.as_tensor(np.ascontiguousarray(p)).permute(2, 0, 1))
        off += 3 * h * w
    assert out[0].untyped_storage().nbytes() == off
    assert [o.data_ptr() % 4 for o in out] != [0] * len(out) or off % 4 == 0               # views start anywhere


def test_stage_images_chw_and_refusals():
    pages = [_hwc(h, w, seed=10 + i).permute(2, 0, 1).contiguous() for i, (h, w) in enumerate(SIZES)]
    out = data.stage_images(pages, torch.device("cpu"), layout="chw")
    off = 0
    for v, p in zip(out, pages):
        assert v.is_contiguous() and tuple(v.shape) == tuple(p.shape) and v.storage_offset() == off and torch.equal(v, p)
        off += p.numel()
    with pytest.raises(TypeError):
        data.stage_images(pages, "cpu")                            # the layout is stated, never guessed
    with pytest.raises(ValueError, match="layout"):
        data.stage_images(pages, "cpu", layout="nhwc")
    with pytest.raises(ValueError, match="empty"):
        data.stage_images([], "cpu", layout="chw")
    with pytest.raises(ValueError, match=r"images\[1\].*uint8"):
        data.stage_images([pages[0], pages[1].float()], "cpu", layout="chw")
    with pytest.raises(ValueError, match=r"images\[0\].*3-d"):
        data.stage_images([pages[0][0]], "cpu", layout="chw")
    with pytest.raises(ValueError, match=r"images\[1\].*channels"):
        data.stage_images([pages[3], pages[3].permute(1, 2, 0)], "cpu", layout="chw")
    assert layoutdit_amd.stage_images is data.stage_images and layoutdit_amd.StagingBuffer is data.StagingBuffer


def test_stage_images_reuses_the_buffer_passed_back_in():
    buf = data.StagingBuffer()
    big = [_hwc(31, 17, seed=1).numpy(), _hwc(12, 20, seed=2).numpy()]
    first = data.stage_images(big, "cpu", buf, layout="hwc")
    host = buf.host
    assert host is not None and host.numel() >= 3 * (31 * 17 + 12 * 20)
    kept = [v.clone() for v in first]
    small = [_hwc(7, 1, seed=3).numpy()]
    second = data.stage_images(small, "cpu", pinned=buf, layout="hwc")
    assert buf.host is host and buf.host.data_ptr() == host.data_ptr()                      # reused, not reallocated
    assert torch.equal(second[0], torch.from_numpy(small[0]).permute(2, 0, 1))
    assert all(torch.equal(a, b) for a, b in zip(first, kept))                              # the earlier batch is a copy of its own
    bigger = [_hwc(40, 40, seed=4).numpy()]
    third = data.stage_images(bigger, "cpu", buf, layout="hwc")
    assert buf.host.numel() >= 4800 and torch.equal(third[0], torch.from_numpy(bigger[0]).permute(2, 0, 1))      # ... and grows
