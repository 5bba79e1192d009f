"""Torch-tensor front ends of the single-kernel C entry points (``include/ldit.h``).

PyTorch is plumbing here: it owns device memory and the current HIP stream; all arithmetic is in ``libldit_hip.so``.
Every function requires CUDA(=HIP) fp32 contiguous tensors and raises otherwise - nothing silently runs in eager.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional, Sequence

import torch

from . import _lib


def _device(*tensors) -> torch.device:
    """The one device every tensor argument lives on (None entries skipped); mixed devices are an error."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"tensor arguments live on different devices ({dev} and {t.device})")
    if dev is None or dev.type != "cuda":
        raise ValueError("expected tensors on the GPU (libldit_hip has no CPU path)")
    return dev


def _launch(dev: torch.device, fn, *args) -> None:
    """Call one C entry point with the stream of the TENSORS' device (not of whatever device is current), with that
    device made current for the launch: the library enqueues on the stream it is handed and HIP launches on the
    current device, so both must be the operands' own."""
    with torch.cuda.device(dev):
        _lib.check(fn(*args, torch.cuda.current_stream(dev).cuda_stream))


def _req(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a tensor on the GPU (libldit_hip has no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS,
           lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``epilogue(x @ weight.T + bias)`` on the fp32 MFMA GEMM.  ``x``: [M, K], ``weight``: [N, K]."""
    lib = _lib.load()
    x, weight = _req(x, "x"), _req(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"weight {tuple(weight.shape)} does not match x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (out, "out"), (out2, "out2")):
        if t is not None:
            _req(t, n)
    _launch(_device(x, weight, bias, lam, residual, out, out2), lib.ldit_linear_f32, _ptr(x), K, _ptr(weight), _ptr(bias), _ptr(out), N, M, N, K, epilogue, _ptr(lam),
                                   _ptr(residual), _ptr(out2))
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    lib = _lib.load()
    x, gamma, beta = _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    _launch(_device(x, gamma, beta), lib.ldit_layernorm_f32, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), rows, C, eps)
    return y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None) -> torch.Tensor:
    """``q, k, v``: [B, N, H*D] token-major (may be column slices of one fused tensor: last-dim stride 1)."""
    lib = _lib.load()
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.float32 or t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise ValueError(f"{n}: expected GPU float32 [B,N,H*D] with unit last stride and dense batch stride")
    B, N, HD = q.shape
    D = HD // heads
    o = torch.empty((B, N, HD), device=q.device, dtype=torch.float32)
    _launch(_device(q, k, v), lib.ldit_attention_f32, _ptr(q), _ptr(k), _ptr(v), _ptr(o), B, N, heads, D, q.stride(1), k.stride(1),
                                      v.stride(1), HD, float(D ** -0.5 if scale is None else scale))
    return o


def embed(x: torch.Tensor, patch_w: torch.Tensor, patch_b: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor,
          patch: int) -> torch.Tensor:
    lib = _lib.load()
    x, patch_w, patch_b = _req(x, "x"), _req(patch_w, "patch_w"), _req(patch_b, "patch_b")
    cls, pos = _req(cls, "cls"), _req(pos, "pos")
    B, in_ch, H, W = x.shape
    Cc = patch_w.shape[0]
    T = (H // patch) * (W // patch) + 1
    out = torch.empty((B, T, Cc), device=x.device, dtype=torch.float32)
    _launch(_device(x, patch_w, patch_b, cls, pos), lib.ldit_embed_f32, _ptr(x), _ptr(patch_w), _ptr(patch_b), _ptr(cls), _ptr(pos), _ptr(out), B, in_ch, H, W,
                                  patch, Cc)
    return out


def embed_bf16(x: torch.Tensor, patch_w_bf16: torch.Tensor, patch_b: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor,
               patch: int) -> torch.Tensor:
    """The patch embedding of the bf16 / fp8 builds and of the train step: bf16 im2col of the batch + bf16 MFMA GEMM, fp32 out."""
    lib = _lib.load()
    x, patch_b, cls, pos = _req(x, "x"), _req(patch_b, "patch_b"), _req(cls, "cls"), _req(pos, "pos")
    if patch_w_bf16.dtype != torch.bfloat16 or not patch_w_bf16.is_contiguous():
        raise ValueError("patch_w_bf16 must be a contiguous bfloat16 tensor")
    B, in_ch, H, W = x.shape
    Cc = patch_w_bf16.shape[0]
    P = (H // patch) * (W // patch)
    out = torch.empty((B, P + 1, Cc), device=x.device, dtype=torch.float32)
    scratch = torch.empty((B * P, in_ch * patch * patch), device=x.device, dtype=torch.bfloat16)
    _launch(_device(x, patch_w_bf16, patch_b, cls, pos), lib.ldit_embed_bf16, _ptr(x), _ptr(patch_w_bf16), _ptr(patch_b), _ptr(cls),
            _ptr(pos), _ptr(out), _ptr(scratch), B, in_ch, H, W, patch, Cc)
    return out


def tap_to_map(tap: torch.Tensor, gh: int, gw: int, scale: float) -> torch.Tensor:
    lib = _lib.load()
    tap = _req(tap, "tap")
    B, T, Cc = tap.shape
    if T != gh * gw + 1:
        raise ValueError(f"tap has {T} tokens, grid {gh}x{gw} needs {gh * gw + 1}")
    out = torch.empty((B, Cc, int(gh * scale), int(gw * scale)), device=tap.device, dtype=torch.float32)
    _launch(_device(tap), lib.ldit_tap_to_map_f32, _ptr(tap), _ptr(out), B, gh, gw, Cc, float(scale))
    return out


def _req16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous float16 tensor on the GPU")
    return t


def widen_f16(x: torch.Tensor) -> torch.Tensor:
    """fp16 -> fp32 on the library's conversion kernel (fp16 pixel batches, ref trainer.py:153-155)."""
    lib = _lib.load()
    x = _req16(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _launch(_device(x), lib.ldit_cast_f16_f32, _ptr(x), _ptr(out), x.numel())
    return out


def narrow_f16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp16 (round to nearest even) on the library's conversion kernel."""
    lib = _lib.load()
    x = _req(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float16)
    _launch(_device(x), lib.ldit_cast_f32_f16, _ptr(x), _ptr(out), x.numel())
    return out


class _TapToMapFn(torch.autograd.Function):
    """tap_to_map with its adjoint (ldit_tap_to_map_bwd_f32), so DiTBackbone.forward stays differentiable in train mode."""

    @staticmethod
    def forward(ctx, tap, gh, gw, scale):
        ctx.geom = (gh, gw, float(scale))
        return tap_to_map(tap.detach(), gh, gw, scale)

    @staticmethod
    def backward(ctx, dmap):
        gh, gw, scale = ctx.geom
        lib = _lib.load()
        dmap = _req(dmap.contiguous(), "dmap")
        B, Cc = dmap.shape[0], dmap.shape[1]
        dtap = torch.empty((B, gh * gw + 1, Cc), device=dmap.device, dtype=torch.float32)
        _launch(_device(dmap), lib.ldit_tap_to_map_bwd_f32, _ptr(dmap), _ptr(dtap), B, gh, gw, Cc, scale)
        return dtap, None, None, None


def tap_to_map_autograd(tap: torch.Tensor, gh: int, gw: int, scale: float) -> torch.Tensor:
    return _TapToMapFn.apply(tap, gh, gw, scale)


def window_args(windows, count: int, sizes: Optional[Sequence[Sequence[int]]] = None):
    """Train-time windows as the C ABI takes them: the HOST int32 array ``[count][5]`` of ``(x0, y0, cw, ch, flip)`` per image, from
    a sequence of five-integer rows or a CPU int32 tensor ``[count, 5]``, checked on the host before anything is launched: ``cw, ch >=
    1``, ``x0, y0 >= 0``, ``flip`` 0 or 1 and, where ``sizes`` gives the pages' ``(h, w)``, ``x0 + cw <= w`` and ``y0 + ch <= h``.
    A ``ValueError`` names the image."""
    if isinstance(windows, torch.Tensor):
        if windows.is_cuda or windows.dtype != torch.int32:
            raise ValueError(f"windows: a tensor of windows must be int32 on the CPU (host descriptors), got {windows.dtype} on {windows.device}")
        if windows.dim() != 2:
            raise ValueError(f"windows: expected shape [{count}, 5], got {tuple(windows.shape)}")
        rows = windows.tolist()
    else:
        rows = list(windows)
    if len(rows) != count:
        raise ValueError(f"windows: {len(rows)} windows for {count} images (expected shape [{count}, 5])")
    flat = []
    for i, r in enumerate(rows):
        try:
            r = [operator.index(v) for v in r]           # integers only: a fractional window is not silently truncated
        except TypeError:
            r = None
        if r is None or len(r) != 5:
            raise ValueError(f"windows[{i}]: the window of images[{i}] must be five integers (x0, y0, cw, ch, flip), got {rows[i]!r}")
        x0, y0, cw, ch, flip = r
        if cw < 1 or ch < 1:
            raise ValueError(f"windows[{i}]: the window of images[{i}] has extent {cw} x {ch} (width x height); both must be at least 1")
        if x0 < 0 or y0 < 0:
            raise ValueError(f"windows[{i}]: the window of images[{i}] starts at ({x0}, {y0}); the origin must not be negative")
        if max(x0 + cw, y0 + ch) >= 2 ** 31:
            raise ValueError(f"windows[{i}]: the window of images[{i}] does not fit 32-bit pixel coordinates")
        if sizes is not None:
            h, w = int(sizes[i][0]), int(sizes[i][1])
            if x0 + cw > w or y0 + ch > h:
                raise ValueError(f"windows[{i}]: x [{x0}, {x0 + cw}) y [{y0}, {y0 + ch}) leaves images[{i}], a {w} x {h} page (width x height)")
        if flip not in (0, 1):
            raise ValueError(f"windows[{i}]: flip = {flip} for images[{i}]; it must be 0 or 1")
        flat.extend(r)
    return (C.c_int32 * (5 * count))(*flat)


def preprocess(images: Sequence[torch.Tensor], size=224, mean: float = 0.5, std: float = 0.5, windows=None) -> torch.Tensor:
    """The detector's input transform in one kernel (ref src/layoutdit/modeling/model.py:50-54: fixed_size 224,
    mean = std = 0.5): list of ``[3, h, w]`` images in [0, 1] (all fp32 or all fp16) -> normalised, bilinearly resized
    fp32 ``[B, 3, size, size]``.  A uint8 list (codes ``c`` standing for ``c / 255``, planar or interleaved: ``image_list_args``)
    gives, bit for bit, what the fp32 list ``img.float().div(255)`` gives (``ldit_preprocess_u8``).

    ``windows`` (train-time crop and flip; :func:`window_args`): per image ``(x0, y0, cw, ch, flip)``.  Row ``i`` is then, bit for bit,
    what this function gives for a contiguous copy of ``images[i][:, y0:y0 + ch, x0:x0 + cw]`` (``.flip(-1)`` where ``flip`` is 1) -
    without the copy, and without reading the page outside the window (``ldit_preprocess_win_*``)."""
    lib = _lib.load()
    wins = None
    if windows is not None:                              # host checks first: they need no GPU
        if any(not isinstance(t, torch.Tensor) or t.dim() != 3 for t in images):
            raise ValueError("every image must be [C, h, w] with the same C")
        wins = window_args(windows, len(images), [t.shape[-2:] for t in images])
    imgs, ptrs, hs, ws, fmt, ch = image_list_args(images)
    B = len(imgs)
    out_h, out_w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    out = torch.empty((B, ch, out_h, out_w), device=imgs[0].device, dtype=torch.float32)
    if wins is not None:
        if fmt in (IMG_U8, IMG_U8_HWC):
            _launch(_device(*imgs), lib.ldit_preprocess_win_u8, ptrs, hs, ws, wins, int(fmt == IMG_U8_HWC), B, ch, mean, std, out_h, out_w, _ptr(out))
        elif fmt == IMG_F16:
            _launch(_device(*imgs), lib.ldit_preprocess_win_f16, ptrs, hs, ws, wins, B, ch, mean, std, out_h, out_w, _ptr(out))
        else:
            _launch(_device(*imgs), lib.ldit_preprocess_win_f32, ptrs, hs, ws, wins, B, ch, mean, std, out_h, out_w, _ptr(out))
    elif fmt in (IMG_U8, IMG_U8_HWC):
        _launch(_device(*imgs), lib.ldit_preprocess_u8, ptrs, hs, ws, int(fmt == IMG_U8_HWC), B, ch, mean, std, out_h, out_w, _ptr(out))
    elif fmt == IMG_F16:
        _launch(_device(*imgs), lib.ldit_preprocess_f16, ptrs, hs, ws, B, ch, mean, std, out_h, out_w, _ptr(out))
    else:
        _launch(_device(*imgs), lib.ldit_preprocess_f32, ptrs, hs, ws, B, ch, mean, std, out_h, out_w, _ptr(out))
    return out


# how the images of one list are stored: planar fp32 / fp16 / uint8, or interleaved uint8
IMG_F32, IMG_F16, IMG_U8, IMG_U8_HWC = 0, 1, 2, 3


def _u8_layouts(t: torch.Tensor, name: str):
    """``(planar, interleaved)``: which of the two accepted memory layouts the uint8 ``[C, h, w]`` image has.  The stride of an axis
    of length 1 says nothing, so a 1 x 1 image (or a one-channel one) has both."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{name}: one list has one dtype: expected uint8 like images[0], got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 3:
        raise ValueError("every image must be [C, h, w] with the same C")
    ch, h, w = t.shape

    def has(strides):
        return all(n == 1 or s == q for n, s, q in zip(t.shape, t.stride(), strides))

    planar, interleaved = has((h * w, w, 1)), has((1, w * ch, ch))
    if not (planar or interleaved):
        raise ValueError(f"{name}: a uint8 [C, h, w] image must be contiguous (planar) or have the strides (1, w*C, C) of an "
                         f"interleaved [h, w, C] array permuted (2, 0, 1); got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return planar, interleaved


def image_list_args(images: Sequence[torch.Tensor]):
    """``(checked tensors, device pointers, heights, widths, format, channels)`` of a ragged list of ``[C, h, w]`` images (same C, one
    GPU) - the HOST arrays the image-list entries of the C ABI take.  One list has one dtype and one memory layout; ``format`` is
    ``IMG_F32`` / ``IMG_F16`` (contiguous, values in [0, 1]) or, for uint8 codes, ``IMG_U8`` (contiguous ``[C, h, w]``) /
    ``IMG_U8_HWC`` (strides ``(1, w*C, C)``: a decoder's ``[h, w, C]`` array under ``permute(2, 0, 1)``, never copied)."""
    if len(images) == 0:
        raise ValueError("empty image list")
    if isinstance(images[0], torch.Tensor) and images[0].dtype == torch.uint8:
        imgs = list(images)
        layouts = [_u8_layouts(t, f"images[{i}]") for i, t in enumerate(imgs)]
        if all(p for p, _ in layouts):
            fmt = IMG_U8
        elif all(q for _, q in layouts):
            fmt = IMG_U8_HWC
        else:
            first = next(i for i, l in enumerate(layouts) if l != (True, True))      # the image that sets the list's layout
            bad = next(i for i, l in enumerate(layouts) if not l[0 if layouts[first][0] else 1])
            kinds = ("planar", "interleaved") if layouts[first][0] else ("interleaved", "planar")
            raise ValueError(f"images[{bad}]: one list has one memory layout, but images[{first}] is {kinds[0]} and this uint8 image is {kinds[1]}")
    else:
        fmt = IMG_F16 if images[0].dtype == torch.float16 else IMG_F32
        imgs = [(_req16 if fmt == IMG_F16 else _req)(t, f"images[{i}]") for i, t in enumerate(images)]
    ch = imgs[0].shape[0]
    if any(t.dim() != 3 or t.shape[0] != ch for t in imgs):
        raise ValueError("every image must be [C, h, w] with the same C")
    for i, t in enumerate(imgs):         # (fp32 / fp16 images were checked above; a uint8 list's dtype and layout rules come first)
        if not t.is_cuda:
            raise ValueError(f"images[{i}]: expected a tensor on the GPU (libldit_hip has no CPU path)")
    B = len(imgs)
    ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in imgs])
    hs = (C.c_int32 * B)(*[t.shape[1] for t in imgs])
    ws = (C.c_int32 * B)(*[t.shape[2] for t in imgs])
    return imgs, ptrs, hs, ws, fmt, ch


def embed_bf16_images(images: Sequence[torch.Tensor], patch_w_bf16: torch.Tensor, patch_b: torch.Tensor, cls: torch.Tensor,
                      pos: torch.Tensor, patch: int, size=224, mean: float = 0.5, std: float = 0.5) -> torch.Tensor:
    """``embed_bf16(preprocess(images, size, mean, std), ...)`` with the input transform evaluated inside the im2col pass (SURVEY.md
    8(f)-2; ref model.py:50-54): same bits, no fp32 batch in between.  uint8 lists as for ``preprocess``."""
    lib = _lib.load()
    imgs, ptrs, hs, ws, fmt, ch = image_list_args(images)
    patch_b, cls, pos = _req(patch_b, "patch_b"), _req(cls, "cls"), _req(pos, "pos")
    if patch_w_bf16.dtype != torch.bfloat16 or not patch_w_bf16.is_contiguous():
        raise ValueError("patch_w_bf16 must be a contiguous bfloat16 tensor")
    out_h, out_w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    B, Cc = len(imgs), patch_w_bf16.shape[0]
    P = (out_h // patch) * (out_w // patch)
    dev = imgs[0].device
    out = torch.empty((B, P + 1, Cc), device=dev, dtype=torch.float32)
    scratch = torch.empty((B * P, ch * patch * patch), device=dev, dtype=torch.bfloat16)
    rest = (mean, std, _ptr(patch_w_bf16), _ptr(patch_b), _ptr(cls), _ptr(pos), _ptr(out), _ptr(scratch), B, ch, out_h, out_w, patch, Cc)
    if fmt in (IMG_U8, IMG_U8_HWC):
        _launch(_device(*imgs, patch_w_bf16, patch_b, cls, pos), lib.ldit_embed_bf16_images_u8, ptrs, hs, ws, int(fmt == IMG_U8_HWC), *rest)
    else:
        _launch(_device(*imgs, patch_w_bf16, patch_b, cls, pos), lib.ldit_embed_bf16_images, ptrs, hs, ws, int(fmt == IMG_F16), *rest)
    return out


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) on the library's conversion kernel."""
    lib = _lib.load()
    x = _req(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _launch(_device(x), lib.ldit_cast_f32_bf16, _ptr(x), _ptr(out), x.numel())
    return out


def linear_bf16(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS,
                lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 MFMA GEMM: ``x`` [M, K] bf16, ``weight`` [N, K] bf16, fp32 accumulation; bf16 result for the bias / GELU / ReLU
    epilogues (``EPI_BIAS_RELU``: ``relu`` of the ``EPI_BIAS`` result bit for bit), fp32 (in place on ``residual`` if ``out is
    residual``) for the scale+residual epilogue and for ``EPI_F32`` (``x @ weight.T + bias`` without the rounding of the result)."""
    lib = _lib.load()
    for t, n in ((x, "x"), (weight, "weight")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous bfloat16 GPU tensor")
    M, K = x.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device,
                          dtype=torch.float32 if epilogue in (_lib.EPI_SCALE_RESID, _lib.EPI_F32) else torch.bfloat16)
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (out2, "out2")):
        if t is not None:
            _req(t, n)
    if epilogue == _lib.EPI_F32:
        # the train step's entry has this epilogue (one K range, no side stores): the same GEMM, its fp32 value stored unrounded
        _launch(_device(x, weight, bias, out), lib.ldit_linear_bf16_ex, _ptr(x), K, _ptr(weight), _ptr(bias), _ptr(out), N, M, N, K, epilogue, None, None, None, None,
                None, None, 0, 1)
        return out
    _launch(_device(x, weight, bias, lam, residual, out, out2), lib.ldit_linear_bf16, _ptr(x), K, _ptr(weight), _ptr(bias), _ptr(out), N, M, N, K, epilogue, _ptr(lam),
                                    _ptr(residual), _ptr(out2))
    return out


def split_planes(x: torch.Tensor, planes: int) -> torch.Tensor:
    """fp32 [rows, cols] -> bf16 [rows, planes * cols]: p0 = bf16(x), p1 = bf16(x - p0), (p2 = bf16(x - p0 - p1)) side by side."""
    lib = _lib.load()
    x = _req(x, "x")
    rows, cols = x.shape
    out = torch.empty((rows, planes * cols), device=x.device, dtype=torch.bfloat16)
    _launch(_device(x), lib.ldit_split_f32_planes, _ptr(x), cols, _ptr(out), rows, cols, planes)
    return out


def attention_planes(qkv_planes: torch.Tensor, heads: int, planes: int) -> torch.Tensor:
    """The attention of the split-fp32 builds: ``qkv_planes`` bf16 [B, N, planes * 3C] = the planes of the fused q|k|v rows (q
    pre-multiplied by scale * log2 e); returns the planes of the fp32 result, bf16 [B, N, planes * C]."""
    lib = _lib.load()
    if not qkv_planes.is_cuda or qkv_planes.dtype != torch.bfloat16 or not qkv_planes.is_contiguous():
        raise ValueError("qkv_planes: expected a contiguous bfloat16 GPU tensor")
    B, N, W6 = qkv_planes.shape
    Cc = W6 // (3 * planes)
    out = torch.empty((B, N, planes * Cc), device=qkv_planes.device, dtype=torch.bfloat16)
    base = qkv_planes.data_ptr()
    _launch(_device(qkv_planes), lib.ldit_attention_planes, base, base + 2 * Cc, base + 4 * Cc, _ptr(out), B, N, heads, Cc // heads,
            W6, 3 * Cc, planes * Cc, planes)
    return out


def layernorm_planes(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, planes: int) -> torch.Tensor:
    lib = _lib.load()
    x, gamma, beta = _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    rows, Cc = x.shape
    out = torch.empty((rows, planes * Cc), device=x.device, dtype=torch.bfloat16)
    _launch(_device(x, gamma, beta), lib.ldit_layernorm_f32_planes, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), rows, Cc, float(eps), planes)
    return out


def linear_planes(xp: torch.Tensor, wp: torch.Tensor, planes: int, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS,
                  lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The GEMM of the split-fp32 builds: ``xp`` [M, planes*K], ``wp`` [N, planes*K] bf16 planes of fp32 operands (``split_planes``);
    3 (planes = 2) or 6 (planes = 3) plane products on the bf16 MFMA, fp32 accumulation.  fp32 result (bias / scale+residual),
    or the planes of erf-GELU(.) as bf16 [M, planes*N] (bias+GELU)."""
    lib = _lib.load()
    for t, n in ((xp, "xp"), (wp, "wp")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous bfloat16 GPU tensor")
    M, K = xp.shape[0], xp.shape[1] // planes
    N = wp.shape[0]
    if out is None:
        out = (torch.empty((M, planes * N), device=xp.device, dtype=torch.bfloat16) if epilogue == _lib.EPI_BIAS_GELU
               else torch.empty((M, N), device=xp.device, dtype=torch.float32))
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (out2, "out2")):
        if t is not None:
            _req(t, n)
    _launch(_device(xp, wp, bias, lam, residual, out, out2), lib.ldit_linear_planes, _ptr(xp), planes * K, _ptr(wp), _ptr(bias), _ptr(out),
            out.shape[1], M, N, K, epilogue, _ptr(lam), _ptr(residual), _ptr(out2), planes)
    return out


FP8_MAX = 448.0          # largest finite e4m3 magnitude


def amax(x: torch.Tensor) -> torch.Tensor:
    """max |x| as a one-element fp32 GPU tensor (no host sync)."""
    lib = _lib.load()
    x = _req(x, "x")
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    _launch(_device(x), lib.ldit_amax_f32, _ptr(x), x.numel(), _ptr(out))
    return out


def quant_fp8(x: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 -> fp8 e4m3 codes of ``x / scale`` (round to nearest even, saturating at +-448)."""
    lib = _lib.load()
    x = _req(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float8_e4m3fn)
    _launch(_device(x), lib.ldit_quant_f32_fp8, _ptr(x), _ptr(out), x.numel(), 1.0 / float(scale))
    return out


def quant_rows_fp8(w: torch.Tensor):
    """Per-output-channel weight quantisation: ``(codes [N, K] fp8 e4m3, scales [N] fp32)`` with
    ``w[n, :] ~= scales[n] * codes[n, :]``."""
    lib = _lib.load()
    w = _req(w, "w")
    N, K = w.shape
    codes = torch.empty((N, K), device=w.device, dtype=torch.float8_e4m3fn)
    scales = torch.empty(N, device=w.device, dtype=torch.float32)
    _launch(_device(w), lib.ldit_quant_rows_f32_fp8, _ptr(w), _ptr(codes), _ptr(scales), N, K)
    return codes, scales


def linear_fp8(x: torch.Tensor, weight: torch.Tensor, ab_scale: float, bias: Optional[torch.Tensor] = None,
               epilogue: int = _lib.EPI_BIAS, lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None, out_scale: float = 1.0,
               w_scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp8 MFMA GEMM: ``x`` [M, K], ``weight`` [N, K] fp8 e4m3 codes; the accumulator is multiplied by ``ab_scale`` (=
    scale_x * scale_w per tensor) or by ``ab_scale * w_scales[n]`` (``ab_scale`` = scale_x, ``w_scales`` per output
    channel); bf16 result for the bias epilogue, fp8 codes of ``gelu(.) / out_scale`` for the GELU epilogue, fp32 for the
    scale+residual epilogue."""
    lib = _lib.load()
    for t, n in ((x, "x"), (weight, "weight")):
        if not t.is_cuda or t.dtype != torch.float8_e4m3fn or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous float8_e4m3fn GPU tensor")
    M, K = x.shape
    N = weight.shape[0]
    if out is None:
        dt = {_lib.EPI_BIAS: torch.bfloat16, _lib.EPI_BIAS_GELU: torch.float8_e4m3fn, _lib.EPI_SCALE_RESID: torch.float32}[epilogue]
        out = torch.empty((M, N), device=x.device, dtype=dt)
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (out2, "out2"), (w_scales, "w_scales")):
        if t is not None:
            _req(t, n)
    _launch(_device(x, weight, bias, lam, residual, out, out2, w_scales), lib.ldit_linear_fp8, _ptr(x), K, _ptr(weight), _ptr(bias), _ptr(out), N, M, N, K, epilogue, _ptr(lam),
                                   _ptr(residual), _ptr(out2), float(ab_scale), 1.0 / float(out_scale), _ptr(w_scales))
    return out


def quant_mxfp8(x: torch.Tensor):
    """fp32 [rows, K] -> MX operand ``(codes [rows, K] float8_e4m3fn, scales [rows, K / 32] uint8)``: one E8M0 scale per 32
    consecutive elements of a row, ``x ~= codes * 2^(scales - 127)`` (the format: ``include/ldit.h``, ``LDIT_MXFP8``).
    ``x`` may be a row slice with unit column stride (its row stride a multiple of 4)."""
    lib = _lib.load()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x: expected a 2-d float32 GPU tensor with unit column stride")
    rows, K = x.shape
    codes = torch.empty((rows, K), device=x.device, dtype=torch.float8_e4m3fn)
    scales = torch.empty((rows, K // 32), device=x.device, dtype=torch.uint8)
    _launch(_device(x), lib.ldit_quant_mx_f32_fp8, _ptr(x), x.stride(0), _ptr(codes), _ptr(scales), rows, K)
    return codes, scales


def layernorm_mxfp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12):
    """LayerNorm over the last axis written as an MX operand ``(codes float8_e4m3fn, scales uint8 [rows, C / 32])``."""
    lib = _lib.load()
    x, gamma, beta = _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    codes = torch.empty((rows, C), device=x.device, dtype=torch.float8_e4m3fn)
    scales = torch.empty((rows, C // 32), device=x.device, dtype=torch.uint8)
    _launch(_device(x, gamma, beta), lib.ldit_layernorm_mxfp8, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(codes), _ptr(scales), rows, C,
            float(eps))
    return codes, scales


def linear_mxfp8(x, weight, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS,
                 lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None):
    """Block-scaled MX GEMM (``v_mfma_scale_f32_32x32x64_f8f6f4``): ``x`` = (codes [M, K], scales [M, K / 32]) and ``weight`` =
    (codes [N, K], scales [N, K / 32]) as :func:`quant_mxfp8` returns them; ``epilogue(x . weight^T + bias)`` with fp32
    accumulation.  bf16 result for the bias epilogue, an MX pair ``(codes [M, N], scales [M, N / 32])`` of ``gelu(.)`` for the
    GELU epilogue, fp32 for the scale+residual epilogue (``out`` may be ``residual``)."""
    lib = _lib.load()
    (xc, xs), (wc, ws) = x, weight
    for t, n in ((xc, "x codes"), (wc, "weight codes")):
        if not t.is_cuda or t.dtype != torch.float8_e4m3fn or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous float8_e4m3fn GPU tensor")
    M, K = xc.shape
    N = wc.shape[0]
    for t, n, shape in ((xs, "x scales", (M, K // 32)), (ws, "weight scales", (N, K // 32))):
        if not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{n}: expected a contiguous uint8 GPU tensor of shape {shape}")
    ys = None
    if epilogue == _lib.EPI_BIAS_GELU:
        if out is None:
            out = (torch.empty((M, N), device=xc.device, dtype=torch.float8_e4m3fn),
                   torch.empty((M, N // 32), device=xc.device, dtype=torch.uint8))
        out, ys = out
    elif out is None:
        out = torch.empty((M, N), device=xc.device, dtype=torch.bfloat16 if epilogue == _lib.EPI_BIAS else torch.float32)
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (out2, "out2")):
        if t is not None:
            _req(t, n)
    _launch(_device(xc, xs, wc, ws, bias, lam, residual, out, ys, out2), lib.ldit_linear_mxfp8, _ptr(xc), K, _ptr(xs), _ptr(wc),
            _ptr(ws), _ptr(bias), _ptr(out), N, _ptr(ys), M, N, K, epilogue, _ptr(lam), _ptr(residual), _ptr(out2))
    return (out, ys) if ys is not None else out


# ---- train variants of the mxfp8 forward's kernels (quantisation-aware training, DiTEncoder(qat=True)) ----------------------
def layernorm_mxfp8_train(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12):
    """:func:`layernorm_mxfp8` plus the bf16 row of the dequantised codes: ``(codes, scales, dequantised bf16 [rows, C])``."""
    lib = _lib.load()
    x, gamma, beta = _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    codes = torch.empty((rows, C), device=x.device, dtype=torch.float8_e4m3fn)
    scales = torch.empty((rows, C // 32), device=x.device, dtype=torch.uint8)
    deq = torch.empty((rows, C), device=x.device, dtype=torch.bfloat16)
    _launch(_device(x, gamma, beta), lib.ldit_layernorm_mxfp8_train, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(codes), _ptr(scales),
            _ptr(deq), rows, C, float(eps))
    return codes, scales, deq


def linear_mxfp8_train(x, weight, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_SCALE_RESID,
                       lam: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                       rowscale: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None):
    """:func:`linear_mxfp8` with the train step's side outputs.  Scale+residual: ``(Y fp32, Ypre bf16)`` - the branch output
    before LayerScale; ``rowscale`` (fp32 [M]) multiplies ``lam`` per row.  GELU: ``((codes, scales), gelu' bf16, dequantised
    output bf16)``."""
    lib = _lib.load()
    (xc, xs), (wc, ws) = x, weight
    M, K = xc.shape
    N = wc.shape[0]
    for t, n in ((bias, "bias"), (lam, "lam"), (residual, "residual"), (rowscale, "rowscale"), (out2, "out2")):
        if t is not None:
            _req(t, n)
    ypre = torch.empty((M, N), device=xc.device, dtype=torch.bfloat16)
    ys = yd = None
    if epilogue == _lib.EPI_BIAS_GELU:
        out = torch.empty((M, N), device=xc.device, dtype=torch.float8_e4m3fn)
        ys = torch.empty((M, N // 32), device=xc.device, dtype=torch.uint8)
        yd = torch.empty((M, N), device=xc.device, dtype=torch.bfloat16)
    else:
        out = torch.empty((M, N), device=xc.device, dtype=torch.float32)
    _launch(_device(xc, xs, wc, ws, bias, lam, residual, out2), lib.ldit_linear_mxfp8_train, _ptr(xc), K, _ptr(xs), _ptr(wc), _ptr(ws),
            _ptr(bias), _ptr(out), N, _ptr(ys), M, N, K, epilogue, _ptr(lam), _ptr(residual), _ptr(out2), _ptr(ypre), _ptr(rowscale),
            _ptr(yd))
    return ((out, ys), ypre, yd) if ys is not None else (out, ypre)


def attention_mxfp8_train(qkv: torch.Tensor, heads: int, scale: float = 0.0):
    """Attention over a fused bf16 ``q|k|v`` [B, N, 3C] with the MX output of the mxfp8 build plus the train step's side outputs:
    ``((codes, scales), lse fp32 [B, H, N], O bf16 before quantisation, dequantised O bf16)``.  ``scale == 0``: q arrives
    pre-multiplied by ``D^-1/2 log2 e`` (the packed builds' fold)."""
    lib = _lib.load()
    if not isinstance(qkv, torch.Tensor) or not qkv.is_cuda or qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or qkv.dim() != 3:
        raise ValueError("qkv: expected a contiguous bf16 [B, N, 3C] GPU tensor")
    B, N, C3 = qkv.shape
    C = C3 // 3
    codes = torch.empty((B * N, C), device=qkv.device, dtype=torch.float8_e4m3fn)
    scales = torch.empty((B * N, C // 32), device=qkv.device, dtype=torch.uint8)
    lse = torch.empty((B, heads, N), device=qkv.device, dtype=torch.float32)
    ob = torch.empty((B * N, C), device=qkv.device, dtype=torch.bfloat16)
    od = torch.empty((B * N, C), device=qkv.device, dtype=torch.bfloat16)
    base = _ptr(qkv)
    _launch(_device(qkv), lib.ldit_attention_mxfp8_train, base, base + 2 * C, base + 4 * C, _ptr(codes), _ptr(scales), _ptr(lse),
            _ptr(ob), _ptr(od), B, N, heads, C // heads, 3 * C, 3 * C, 3 * C, C, float(scale))
    return (codes, scales), lse, ob, od


def attention_bf16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
                   prescaled: bool = False) -> torch.Tensor:
    """bf16 fused attention; ``q, k, v``: bf16 [B, N, H*D] token-major (column slices of a fused tensor are fine)."""
    lib = _lib.load()
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise ValueError(f"{n}: expected GPU bfloat16 [B,N,H*D] with unit last stride and dense batch stride")
    B, N, HD = q.shape
    D = HD // heads
    o = torch.empty((B, N, HD), device=q.device, dtype=torch.bfloat16)
    # prescaled: q already carries scale * log2(e) (the packed inference path); the library is told so with scale = 0
    _launch(_device(q, k, v), lib.ldit_attention_bf16, _ptr(q), _ptr(k), _ptr(v), _ptr(o), B, N, heads, D, q.stride(1), k.stride(1),
                                       v.stride(1), HD, 0.0 if prescaled else float(D ** -0.5 if scale is None else scale))
    return o


def fpn_merge(lat: torch.Tensor, gh: int, gw: int, scale: float, top: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One level of the FPN top-down pathway, NHWC: ``bilinear_scale(lat tokens) + nearest(top)``.
    ``lat``: [B, 1 + gh*gw, Ch] (lateral 1x1 convolution of a tap's tokens); ``top``: [B, th, tw, Ch] NHWC or None."""
    lib = _lib.load()
    lat = _req(lat, "lat")
    B, T, Ch = lat.shape
    if T != gh * gw + 1:
        raise ValueError(f"lat has {T} tokens, grid {gh}x{gw} needs {gh * gw + 1}")
    if top is not None:
        top = _req(top, "top")
    out = torch.empty((B, int(gh * scale), int(gw * scale), Ch), device=lat.device, dtype=torch.float32)
    th, tw = (0, 0) if top is None else (top.shape[1], top.shape[2])
    _launch(_device(lat, top), lib.ldit_fpn_merge_f32, _ptr(lat), _ptr(top), _ptr(out), B, gh, gw, Ch, float(scale), th, tw)
    return out


_ZEROS = {}


def _zero_page(device: torch.device) -> torch.Tensor:
    z = _ZEROS.get(device)
    if z is None:
        z = torch.zeros(64, dtype=torch.float32, device=device)
        _ZEROS[device] = z
    return z


def conv3x3_nhwc(x: torch.Tensor, weight_ohwi: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / padding 1 convolution of an NHWC map as an implicit-im2col fp32 MFMA GEMM.  ``x``: [B, H, W, Cin];
    ``weight_ohwi``: [Cout, 3, 3, Cin] (= ``conv.weight.permute(0, 2, 3, 1)``); returns NHWC [B, H, W, Cout]."""
    lib = _lib.load()
    x, weight_ohwi = _req(x, "x"), _req(weight_ohwi, "weight_ohwi")
    B, H, W, Cin = x.shape
    Cout = weight_ohwi.shape[0]
    if tuple(weight_ohwi.shape) != (Cout, 3, 3, Cin):
        raise ValueError(f"weight {tuple(weight_ohwi.shape)} is not [Cout, 3, 3, {Cin}]")
    if bias is not None:
        _req(bias, "bias")
    y = torch.empty((B, H, W, Cout), device=x.device, dtype=torch.float32)
    _launch(_device(x, weight_ohwi, bias), lib.ldit_conv3x3_nhwc_f32, _ptr(x), _ptr(weight_ohwi), _ptr(bias), _ptr(y), B, H, W, Cin,
            Cout, _ptr(_zero_page(x.device)))
    return y


# ---- FPN backward building blocks (include/ldit.h "FPN backward") ------------------------------------------------------------
def fpn_merge_bwd(d_inner: torch.Tensor, gh: int, gw: int, scale: float, d_top: Optional[torch.Tensor] = None,
                  want_lat: bool = True) -> Optional[torch.Tensor]:
    """Adjoint of :func:`fpn_merge`.  ``d_inner``: [B, gh*s, gw*s, Ch] NHWC.  Returns ``d_lat`` [B, 1+gh*gw, Ch] (CLS row 0)
    and ACCUMULATES the nearest-upsample adjoint into ``d_top`` [B, th, tw, Ch] (in place) when given."""
    lib = _lib.load()
    d_inner = _req(d_inner, "d_inner")
    B, _, _, Ch = d_inner.shape
    if d_top is not None:
        _req(d_top, "d_top")
    d_lat = torch.empty((B, gh * gw + 1, Ch), device=d_inner.device, dtype=torch.float32) if want_lat else None
    th, tw = (0, 0) if d_top is None else (d_top.shape[1], d_top.shape[2])
    _launch(_device(d_inner, d_top), lib.ldit_fpn_merge_bwd_f32, _ptr(d_inner), _ptr(d_lat), _ptr(d_top), B, gh, gw, Ch, float(scale),
            th, tw)
    return d_lat


def pad_nhwc_bf16(x: torch.Tensor, slack_rows: int = 0) -> torch.Tensor:
    """bf16 zero-padded copy of an fp32 NHWC map as a 2-D operand: returns ``[slack + B*(H+2)*(W+2) + slack, C]`` bf16 whose
    middle rows are the padded pixels in (b, y, x) order and whose ``slack_rows`` leading / trailing rows are zero (room for
    the constant row offsets of the 3x3 taps, see ``layoutdit_amd/csrc/fpn_bwd.hip``)."""
    lib = _lib.load()
    x = _req(x, "x")
    B, H, W, Cc = x.shape
    rows = B * (H + 2) * (W + 2)
    # (the kernel writes every element of the padded map, borders included: only slack rows need the fill)
    alloc = torch.zeros if slack_rows else torch.empty
    buf = alloc((rows + 2 * slack_rows, Cc), device=x.device, dtype=torch.bfloat16)
    _launch(_device(x), lib.ldit_pad_nhwc_f32_bf16, _ptr(x), buf[slack_rows:].data_ptr(), B, H, W, Cc)
    return buf


def conv3x3_nhwc_bf16(xpad_rows: torch.Tensor, B: int, H: int, W: int, weight_ohwi_bf16: torch.Tensor,
                      bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_F32) -> torch.Tensor:
    """3x3 / padding 1 convolution on the bf16 MFMA GEMM's implicit-im2col mode.  ``xpad_rows``: what ``pad_nhwc_bf16(x)`` returns
    for an NHWC map ``x`` [B, H, W, Cin] (no slack rows): bf16 ``[B (H+2) (W+2), Cin]``; ``weight_ohwi_bf16``: bf16 [Cout, 3, 3, Cin].
    Returns the pixel rows ``[B H W, Cout]``: fp32 ``acc + bias`` for ``EPI_F32``, bf16 for ``EPI_BIAS`` / ``EPI_BIAS_RELU`` - bit for
    bit :func:`linear_bf16` with the same epilogue on the im2col matrix of the padded map."""
    lib = _lib.load()
    for t, n in ((xpad_rows, "xpad_rows"), (weight_ohwi_bf16, "weight_ohwi_bf16")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous bfloat16 GPU tensor")
    Cout, Cin = weight_ohwi_bf16.shape[0], weight_ohwi_bf16.shape[-1]
    if tuple(weight_ohwi_bf16.shape) != (Cout, 3, 3, Cin):
        raise ValueError(f"weight {tuple(weight_ohwi_bf16.shape)} is not [Cout, 3, 3, Cin]")
    if tuple(xpad_rows.shape) != (B * (H + 2) * (W + 2), Cin):
        raise ValueError(f"xpad_rows {tuple(xpad_rows.shape)} is not the padded map [{B} * {H + 2} * {W + 2}, {Cin}]")
    if bias is not None:
        _req(bias, "bias")
    y = torch.empty((B * H * W, Cout), device=xpad_rows.device, dtype=torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16)
    _launch(_device(xpad_rows, weight_ohwi_bf16, bias), lib.ldit_conv3x3_nhwc_bf16, _ptr(xpad_rows), _ptr(weight_ohwi_bf16), _ptr(bias),
            _ptr(y), Cout, B, H, W, Cin, Cout, epilogue)
    return y


def colsum(x: torch.Tensor) -> torch.Tensor:
    """``x.sum(0)`` of a contiguous fp32 [M, N] matrix (two stages, fixed order)."""
    lib = _lib.load()
    x = _req(x, "x")
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    need = ((M + 511) // 512) * N * 4                  # = ldit_colsum_scratch_bytes(M, N): one partial row per 512 rows
    scratch = torch.empty(max(need, 16), device=x.device, dtype=torch.uint8)
    _launch(_device(x), lib.ldit_colsum_f32, _ptr(x), M, N, N, _ptr(out), _ptr(scratch), need)
    return out


def colamax(x: torch.Tensor) -> torch.Tensor:
    """``x.abs().amax(0)`` of a contiguous fp32 [M, N] matrix (per-channel activation ranges, fp8 calibration)."""
    lib = _lib.load()
    x = _req(x, "x")
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    need = ((M + 511) // 512) * N * 4
    scratch = torch.empty(max(need, 16), device=x.device, dtype=torch.uint8)
    _launch(_device(x), lib.ldit_colamax_f32, _ptr(x), M, N, N, _ptr(out), _ptr(scratch), need)
    return out


def _colsum_buffers(M: int, N: int, device, want: bool):
    """``(colsum, scratch, scratch_bytes)`` of a fused column sum over an [M, N] matrix; all ``None`` / 0 when it is not wanted."""
    if not want:
        return None, None, 0
    need = ((M + 511) // 512) * N * 4                  # = ldit_colsum_scratch_bytes(M, N): one partial row per 512 rows
    return (torch.empty(N, device=device, dtype=torch.float32), torch.empty(max(need, 16), device=device, dtype=torch.uint8), need)


def _req_act(act: Optional[torch.Tensor], dy: torch.Tensor) -> Optional[torch.Tensor]:
    """``act`` of a ReLU backward: a contiguous GPU tensor of ``dy``'s shape, fp32 or - as a bf16 forward saved it - bf16."""
    if act is None:
        return None
    if isinstance(act, torch.Tensor) and act.dtype == torch.bfloat16:
        if not act.is_cuda or not act.is_contiguous():
            raise ValueError("act: expected a contiguous GPU tensor")
    else:
        _req(act, "act")
    if tuple(act.shape) != tuple(dy.shape):
        raise ValueError(f"act {tuple(act.shape)} does not match dy {tuple(dy.shape)}")
    return act


def _act16(act: Optional[torch.Tensor]) -> bool:
    return act is not None and act.dtype == torch.bfloat16


def relu_bwd_bf16(dy: torch.Tensor, act: Optional[torch.Tensor] = None, want_colsum: bool = True):
    """One pass between two layers of a backward: with ``w = torch.where(act > 0, dy, 0)`` (``w = dy`` without ``act``) returns
    ``(cast_bf16(w), colsum(w))`` bit for bit, the sum ``None`` where it is not wanted.  ``dy``: contiguous fp32 [M, N]; ``act``:
    the same, or bf16 (``ldit_relu_bwd_bf16_act16``: no fp32 copy of it is made, the results are those on ``act.float()``)."""
    lib = _lib.load()
    dy = _req(dy, "dy")
    act = _req_act(act, dy)
    M, N = dy.shape
    out = torch.empty((M, N), device=dy.device, dtype=torch.bfloat16)
    cs, scratch, need = _colsum_buffers(M, N, dy.device, want_colsum)
    entry = getattr(lib, "ldit_relu_bwd_bf16_act16" if _act16(act) else "ldit_relu_bwd_bf16")                  # one signature
    _launch(_device(dy, act), entry, _ptr(dy), N, _ptr(act), N, _ptr(out), N, M, N, _ptr(cs), _ptr(scratch), need)
    return out, cs


def relu_bwd_pad_nhwc_bf16(dy: torch.Tensor, act: Optional[torch.Tensor] = None, want_colsum: bool = True):
    """:func:`relu_bwd_bf16` on an NHWC map ``dy`` [B, H, W, C] with the copy in the zero-padded layout: returns
    ``(pad_nhwc_bf16(w), colsum(w.view(-1, C)))`` bit for bit - bf16 ``[B (H+2) (W+2), C]`` (no slack rows) and fp32 [C] or ``None``.
    A bf16 ``act`` goes to ``ldit_relu_bwd_pad_nhwc_bf16_act16``."""
    lib = _lib.load()
    dy = _req(dy, "dy")
    act = _req_act(act, dy)
    B, H, W, Cc = dy.shape
    out = torch.empty((B * (H + 2) * (W + 2), Cc), device=dy.device, dtype=torch.bfloat16)
    cs, scratch, need = _colsum_buffers(B * H * W, Cc, dy.device, want_colsum)
    entry = getattr(lib, "ldit_relu_bwd_pad_nhwc_bf16_act16" if _act16(act) else "ldit_relu_bwd_pad_nhwc_bf16")
    _launch(_device(dy, act), entry, _ptr(dy), _ptr(act), _ptr(out), B, H, W, Cc, _ptr(cs), _ptr(scratch), need)
    return out, cs


def _splits_for(K: int, M: int, N: int) -> int:
    """K-splits of a wgrad GEMM with an [M, N] output - the rule of csrc/api_train.hip pick_splits: enough 128 x 128 tiles for the
    machine (~512 / output tiles, at most 8), every split non-empty."""
    nk = (K + 63) // 64
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    s = max(1, min(nk, 8, 512 // max(t128, 1)))
    while s > 1 and ((nk + s - 1) // s) * (s - 1) >= nk:
        s -= 1
    return s


def wgrad_bf16(a: torch.Tensor, w: torch.Tensor, K: int, w_row_offset: int = 0) -> torch.Tensor:
    """``a[:K].T @ w[w_row_offset : w_row_offset + K]`` with both operands reduction-major bf16 (gemm_bf16_tr.hip, wgrad form):
    ``a`` [>= K, M], ``w`` [>= w_row_offset + K, N] contiguous.  fp32 [M, N]; K is split over workgroups into slabs that are
    summed in a fixed order."""
    lib = _lib.load()
    for t, n in ((a, "a"), (w, "w")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError(f"{n}: expected a contiguous 2-D bfloat16 GPU tensor")
    if a.shape[0] < K or w_row_offset < 0 or w.shape[0] < w_row_offset + K:
        raise ValueError("wgrad_bf16: K rows are not available in both operands")
    M, N = a.shape[1], w.shape[1]
    dev = _device(a, w)
    splits = _splits_for(K, M, N)
    slabs = torch.empty((splits, M, N), device=dev, dtype=torch.float32)
    _launch(_device(a, w), lib.ldit_linear_bf16_tr, a.data_ptr(), M, 1, w[w_row_offset:].data_ptr(), N, slabs.data_ptr(), N, M, N, K,
            _lib.EPI_F32, None, splits, _zero_page(dev).data_ptr())
    if splits == 1:
        return slabs[0]
    out = torch.empty((M, N), device=dev, dtype=torch.float32)
    _launch(_device(slabs), lib.ldit_reduce_slabs_f32, slabs.data_ptr(), out.data_ptr(), M * N, splits)
    return out


# ---- region proposals (include/ldit.h "region proposals"; csrc/proposals.hip) ------------------------------------------------
def _req_i32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 tensor on the GPU")
    return t


RPN_SORT_SLOTS = 16384                   # keys of the LDS sort buffer (SORT_MAX_N, csrc/sort_lds.h): above it the chunked kernels run


def rpn_topk(logits: torch.Tensor, level_sizes: Sequence[int], k: int) -> torch.Tensor:
    """Per-level top-k of the objectness logits.  ``logits``: [B, Ntot] with the levels concatenated (``sum(level_sizes) ==
    Ntot``).  Returns int32 [B, sum(min(k, n_l))]: for each level the positions on the concatenated axis of its largest logits,
    descending, ties by ascending index.  A level above ``RPN_SORT_SLOTS`` anchors (up to 2^20, ``k`` <= 8192) sends the call to
    the chunked kernel, which defines the same result.  No synchronisation."""
    lib = _lib.load()
    logits = _req(logits, "logits")
    sizes = [int(n) for n in level_sizes]
    if logits.dim() != 2 or sum(sizes) != logits.shape[1] or not sizes:
        raise ValueError(f"logits {tuple(logits.shape)} is not [B, sum(level_sizes) = {sum(sizes)}]")
    if k <= 0:
        raise ValueError("k must be positive")
    B = logits.shape[0]
    idx = torch.empty((B, sum(min(k, n) for n in sizes)), device=logits.device, dtype=torch.int32)
    args = (_ptr(logits), (C.c_int64 * len(sizes))(*sizes), len(sizes), B, int(k), _ptr(idx))
    if max(sizes) > RPN_SORT_SLOTS:
        _launch(_device(logits), lib.ldit_rpn_topk_chunked_f32, *args)
    else:
        _launch(_device(logits), lib.ldit_rpn_topk_f32, *args)
    return idx


def rpn_decode(logits: torch.Tensor, deltas: torch.Tensor, anchors: torch.Tensor, idx: torch.Tensor, image_size,
               min_size: float = 1e-3, score_thresh: float = 0.0):
    """Gather + ``BoxCoder(1, 1, 1, 1).decode`` + clip to ``image_size = (h, w)`` + sigmoid for the candidates ``idx`` [B, K] of
    :func:`rpn_topk`.  ``logits`` [B, Ntot], ``deltas`` [B, Ntot, 4], ``anchors`` [Ntot, 4].  Returns ``boxes`` [B, K, 4] and
    ``scores`` [B, K]; a candidate that is too small or scores below the threshold has score ``-inf``.  No synchronisation."""
    lib = _lib.load()
    logits, deltas, anchors, idx = _req(logits, "logits"), _req(deltas, "deltas"), _req(anchors, "anchors"), _req_i32(idx, "idx")
    B, Ntot = logits.shape
    if tuple(deltas.shape) != (B, Ntot, 4) or tuple(anchors.shape) != (Ntot, 4) or idx.dim() != 2 or idx.shape[0] != B:
        raise ValueError(f"rpn_decode: logits {tuple(logits.shape)}, deltas {tuple(deltas.shape)}, anchors {tuple(anchors.shape)}, "
                         f"idx {tuple(idx.shape)} do not fit together")
    K = idx.shape[1]
    boxes = torch.empty((B, K, 4), device=logits.device, dtype=torch.float32)
    scores = torch.empty((B, K), device=logits.device, dtype=torch.float32)
    _launch(_device(logits, deltas, anchors, idx), lib.ldit_rpn_decode_f32, _ptr(logits), _ptr(deltas), _ptr(anchors), _ptr(idx), B, Ntot, K,
            float(image_size[0]), float(image_size[1]), float(min_size), float(score_thresh), _ptr(boxes), _ptr(scores))
    return boxes, scores


def batched_nms_padded(boxes: torch.Tensor, scores: torch.Tensor, groups: Optional[torch.Tensor], iou_threshold: float, max_out: int,
                       gather: bool = True):
    """``P`` independent NMS problems with fixed-size results.  ``boxes`` [P, N, 4], ``scores`` [P, N], ``groups`` int32 [P, N] or
    None.  Returns ``(keep, count, out_boxes, out_scores)``: ``keep`` int32 [P, max_out] = the kept input indices in descending
    score order padded with -1, ``count`` int32 [P], and (``gather``) the kept rows [P, max_out, 4] / [P, max_out] with zero
    padding (else None).  Candidates with score ``-inf`` / NaN take no part.  No synchronisation."""
    lib = _lib.load()
    boxes, scores = _req(boxes, "boxes"), _req(scores, "scores")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]):
        raise ValueError(f"batched_nms_padded: boxes {tuple(boxes.shape)} / scores {tuple(scores.shape)} are not [P, N, 4] / [P, N]")
    if groups is not None and tuple(_req_i32(groups, "groups").shape) != tuple(scores.shape):
        raise ValueError(f"groups {tuple(groups.shape)} does not match scores {tuple(scores.shape)}")
    P, N = scores.shape
    if P == 0 or N == 0 or max_out <= 0:
        raise ValueError("batched_nms_padded: empty problem")
    dev = boxes.device
    keep = torch.empty((P, max_out), device=dev, dtype=torch.int32)
    count = torch.empty((P,), device=dev, dtype=torch.int32)
    out_boxes = torch.empty((P, max_out, 4), device=dev, dtype=torch.float32) if gather else None
    out_scores = torch.empty((P, max_out), device=dev, dtype=torch.float32) if gather else None
    need = _lib.nms_workspace_bytes(P, N)
    ws = torch.empty(need, device=dev, dtype=torch.uint8) if need else None
    _launch(_device(boxes, scores, groups), lib.ldit_nms_batched_f32, _ptr(boxes), _ptr(scores), _ptr(groups), P, N, float(iou_threshold),
            int(max_out), _ptr(keep), _ptr(count), _ptr(out_boxes), _ptr(out_scores), _ptr(ws), need)
    return keep, count, out_boxes, out_scores


def batched_nms(boxes: torch.Tensor, scores: torch.Tensor, idxs: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision ``batched_nms``: ``boxes`` [N, 4], ``scores`` [N], ``idxs`` [N] (any integer type).  int64 indices of the kept
    boxes, descending score.  Slices by the kept count, so it synchronises."""
    if boxes.dim() != 2 or boxes.shape[0] == 0:
        if boxes.dim() == 2:
            return torch.empty((0,), dtype=torch.int64, device=boxes.device)
        raise ValueError(f"boxes {tuple(boxes.shape)} is not [N, 4]")
    N = boxes.shape[0]
    groups = None if idxs is None else idxs.to(torch.int32).contiguous()[None]
    keep, count, _, _ = batched_nms_padded(boxes[None], scores[None], groups, iou_threshold, N, gather=False)
    return keep[0, :int(count[0])].to(torch.int64)


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision ``nms``.  Synchronises (see :func:`batched_nms`)."""
    return batched_nms(boxes, scores, None, iou_threshold)


# ---- RPN training (include/ldit.h "RPN training"; csrc/rpn_train.hip) ----------------------------------------------------------
RPN_TARGETS_MAX_ANCHORS = 16384          # per image (ldit_rpn_targets_f32; above it ldit_rpn_targets_chunked_f32, up to 2^20)
RPN_TARGETS_MAX_GT = 512


def rpn_targets(anchors: torch.Tensor, gt_boxes: torch.Tensor, gt_count: torch.Tensor, keys: torch.Tensor, fg_iou_thresh: float = 0.7,
                bg_iou_thresh: float = 0.3, batch_size_per_image: int = 256, positive_fraction: float = 0.5):
    """Anchor matching (``Matcher(fg, bg, allow_low_quality_matches=True)``), the balanced sampler on the caller's ``keys`` and
    ``BoxCoder(1, 1, 1, 1).encode`` in one launch.  ``anchors`` [N, 4], ``gt_boxes`` [B, Gmax, 4], ``gt_count`` int32 [B], ``keys``
    int32 [B, N] (non-negative random priorities).  Returns ``labels`` int32 [B, N] (1 / 0 / -1 = sampled positive / sampled
    negative / not in the loss), ``matched`` int32 [B, N] (GT index, -1 below the background threshold, -2 between the thresholds),
    ``reg_targets`` [B, N, 4] (zero where the anchor is no positive) and ``sampled`` int32 [B, 2].  More than ``RPN_SORT_SLOTS``
    anchors (up to 2^20, ``batch_size_per_image`` <= 4096) send the call to the chunked kernel, which defines the same result.  No
    synchronisation."""
    lib = _lib.load()
    anchors, gt_boxes = _req(anchors, "anchors"), _req(gt_boxes, "gt_boxes")
    gt_count, keys = _req_i32(gt_count, "gt_count"), _req_i32(keys, "keys")
    if anchors.dim() != 2 or anchors.shape[1] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise ValueError(f"rpn_targets: anchors {tuple(anchors.shape)} / gt_boxes {tuple(gt_boxes.shape)} are not [N, 4] / [B, Gmax, 4]")
    N, (B, Gmax) = anchors.shape[0], gt_boxes.shape[:2]
    if tuple(gt_count.shape) != (B,) or tuple(keys.shape) != (B, N):
        raise ValueError(f"rpn_targets: gt_count {tuple(gt_count.shape)} / keys {tuple(keys.shape)} are not [{B}] / [{B}, {N}]")
    if B == 0 or N == 0 or Gmax == 0:
        raise ValueError("rpn_targets: empty problem (pad gt_boxes to at least one row)")
    if batch_size_per_image <= 0 or not 0.0 < positive_fraction <= 1.0 or bg_iou_thresh > fg_iou_thresh:
        raise ValueError("rpn_targets: need batch_size_per_image > 0, 0 < positive_fraction <= 1 and bg_iou_thresh <= fg_iou_thresh")
    dev = anchors.device
    labels = torch.empty((B, N), device=dev, dtype=torch.int32)
    matched = torch.empty((B, N), device=dev, dtype=torch.int32)
    reg_targets = torch.empty((B, N, 4), device=dev, dtype=torch.float32)
    sampled = torch.empty((B, 2), device=dev, dtype=torch.int32)
    args = (_ptr(anchors), _ptr(gt_boxes), _ptr(gt_count), _ptr(keys), B, N, Gmax, float(fg_iou_thresh), float(bg_iou_thresh),
            int(batch_size_per_image), float(positive_fraction), _ptr(labels), _ptr(matched), _ptr(reg_targets), _ptr(sampled))
    if N > RPN_SORT_SLOTS:
        _launch(_device(anchors, gt_boxes, gt_count, keys), lib.ldit_rpn_targets_chunked_f32, *args)
    else:
        _launch(_device(anchors, gt_boxes, gt_count, keys), lib.ldit_rpn_targets_f32, *args)
    return labels, matched, reg_targets, sampled


def rpn_loss(logits: torch.Tensor, deltas: torch.Tensor, labels: torch.Tensor, reg_targets: torch.Tensor, sampled: torch.Tensor,
             beta: float = 1.0 / 9.0):
    """The RPN's two losses and their gradients for unit upstream.  ``logits`` [B, N], ``deltas`` [B, N, 4] and the results of
    :func:`rpn_targets`.  Returns ``loss`` [2] (objectness: mean BCE-with-logits over the sampled anchors of the batch; box:
    smooth-L1(``beta``) summed over the sampled positives and divided by the same count), ``d_logits`` [B, N] and ``d_deltas``
    [B, N, 4], exactly zero where an anchor is not in the loss.  No synchronisation."""
    lib = _lib.load()
    logits, deltas, reg_targets = _req(logits, "logits"), _req(deltas, "deltas"), _req(reg_targets, "reg_targets")
    labels, sampled = _req_i32(labels, "labels"), _req_i32(sampled, "sampled")
    if logits.dim() != 2 or 0 in logits.shape:
        raise ValueError(f"rpn_loss: logits {tuple(logits.shape)} is not a non-empty [B, N]")
    B, N = logits.shape
    if tuple(deltas.shape) != (B, N, 4) or tuple(reg_targets.shape) != (B, N, 4) or tuple(labels.shape) != (B, N) or tuple(sampled.shape) != (B, 2):
        raise ValueError(f"rpn_loss: logits {tuple(logits.shape)}, deltas {tuple(deltas.shape)}, labels {tuple(labels.shape)}, reg_targets "
                         f"{tuple(reg_targets.shape)}, sampled {tuple(sampled.shape)} do not fit together")
    if not beta >= 0.0:
        raise ValueError("rpn_loss: beta must be >= 0")
    dev = logits.device
    loss = torch.empty((4,), device=dev, dtype=torch.float32)[:2]               # 16 bytes: the library wants aligned operands
    d_logits = torch.empty((B, N), device=dev, dtype=torch.float32)
    d_deltas = torch.empty((B, N, 4), device=dev, dtype=torch.float32)
    need = _lib.rpn_loss_workspace_bytes(B, N)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    _launch(_device(logits, deltas, labels, reg_targets, sampled), lib.ldit_rpn_loss_f32, _ptr(logits), _ptr(deltas), _ptr(labels),
            _ptr(reg_targets), _ptr(sampled), B, N, float(beta), _ptr(loss), _ptr(d_logits), _ptr(d_deltas), _ptr(ws), need)
    return loss, d_logits, d_deltas


# ---- box head (include/ldit.h "box head"; csrc/roi_heads.hip) ------------------------------------------------------------------
NMS_MAX_CANDIDATES = 8192                # per problem (ldit_nms_batched_f32)


def infer_scales(features: Sequence[torch.Tensor], image_size) -> list:
    """torchvision's ``MultiScaleRoIAlign`` scale inference: per map ``2 ** round(log2(map / image))``, the same for both axes."""
    import math
    scales = []
    for f in features:
        per_axis = [2.0 ** float(round(math.log2(float(s) / float(o)))) for s, o in zip(f.shape[-2:], image_size)]
        if per_axis[0] != per_axis[1]:
            raise ValueError(f"map {tuple(f.shape[-2:])} of image {tuple(image_size)}: the two axes infer different scales {per_axis}")
        scales.append(per_axis[0])
    return scales


def roi_align_levels(features: Sequence[torch.Tensor], boxes: torch.Tensor, count: Optional[torch.Tensor], image_size,
                     output_size: int = 7, sampling_ratio: int = 2, canonical_scale: float = 224.0, canonical_level: float = 4.0,
                     return_levels: bool = False, out_dtype: torch.dtype = torch.float32):
    """``MultiScaleRoIAlign`` forward in one launch.  ``features``: the maps ``[B, C, h, w]`` finest first, float32 in channels-last
    memory (channel stride 1; any batch / row / pixel stride - ``p5[:, :, ::2, ::2]`` is consumed without a copy).  ``boxes`` [B, R, 4]
    and ``count`` int32 [B] (or None: every row valid) are what ``RegionProposalNetwork.forward(..., padded=True)`` returns.
    Returns ``[B * R, P, P, C]`` (the fc6 GEMM's A operand; rows ``r >= count[b]`` are zero) and, with ``return_levels``, the
    int32 ``[B, R]`` level of each row (-1 for padding rows).  ``out_dtype=torch.bfloat16``: the same rows rounded to bf16 (to
    nearest even) at the kernel's store - the A operand of the bf16 fc6 GEMM at half the bytes; the maps stay float32.  No
    synchronisation."""
    import math
    lib = _lib.load()
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"roi_align_levels: out_dtype {out_dtype} (torch.float32 or torch.bfloat16 is built)")
    feats = list(features)
    boxes = _req(boxes, "boxes")
    if not feats or boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError(f"roi_align_levels: boxes {tuple(boxes.shape)} is not [B, R, 4] or there is no feature map")
    B, R = boxes.shape[:2]
    if B == 0 or R == 0:
        raise ValueError("roi_align_levels: empty problem")
    Cc = feats[0].shape[1]
    for i, f in enumerate(feats):
        if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype != torch.float32:
            raise ValueError(f"features[{i}]: expected a float32 tensor on the GPU (libldit_hip has no CPU path)")
        if f.dim() != 4 or f.shape[0] != B or f.shape[1] != Cc:
            raise ValueError(f"features[{i}] {tuple(f.shape)} is not [{B}, {Cc}, h, w]")
        if f.stride(1) != 1:
            raise ValueError(f"features[{i}]: expected channels-last memory (channel stride 1), got strides {f.stride()}")
    if count is not None and tuple(_req_i32(count, "count").shape) != (B,):
        raise ValueError(f"count {tuple(count.shape)} is not [{B}]")
    scales = infer_scales(feats, image_size)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    L, P = len(feats), int(output_size)
    out = torch.empty((B * R, P, P, Cc), device=boxes.device, dtype=out_dtype)
    levels = torch.empty((B, R), device=boxes.device, dtype=torch.int32) if return_levels else None
    entry = getattr(lib, "ldit_roi_align_levels_bf16" if out_dtype == torch.bfloat16 else "ldit_roi_align_levels_f32")     # one signature
    _launch(_device(boxes, count, *feats), entry, (C.c_void_p * L)(*[f.data_ptr() for f in feats]),
            (C.c_int32 * L)(*[f.shape[2] for f in feats]), (C.c_int32 * L)(*[f.shape[3] for f in feats]), (C.c_float * L)(*scales),
            (C.c_int64 * L)(*[f.stride(0) for f in feats]), (C.c_int64 * L)(*[f.stride(2) for f in feats]),
            (C.c_int64 * L)(*[f.stride(3) for f in feats]), L, Cc, _ptr(boxes), _ptr(count), B, R, P, int(sampling_ratio), k_min, k_max,
            float(canonical_scale), float(canonical_level), _ptr(out), _ptr(levels))
    return (out, levels) if return_levels else out


def _check_candidates(R: int, num_classes: int) -> None:
    if R * (num_classes - 1) > NMS_MAX_CANDIDATES:
        raise ValueError(f"box head: {R} proposals x {num_classes - 1} foreground classes = {R * (num_classes - 1)} candidates per image, "
                         f"the batched NMS handles at most {NMS_MAX_CANDIDATES}")


def box_postprocess(head_out: torch.Tensor, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size, num_classes: int,
                    score_thresh: float = 0.05, min_size: float = 1e-2, weights=(10.0, 10.0, 5.0, 5.0)):
    """``postprocess_detections`` up to the NMS.  ``head_out`` [B * R, ld]: class logits in columns ``[0, NC)``, deltas in
    ``[NC, 5 NC)``; ``proposals`` [B, R, 4], ``count`` int32 [B] or None.  Returns ``boxes`` [B, R (NC - 1), 4], ``scores``
    [B, R (NC - 1)] (``-inf`` for a candidate that is filtered or belongs to a padding row) and ``labels`` int32, candidate
    ``r (NC - 1) + (c - 1)`` = (proposal r, class c).  No synchronisation."""
    lib = _lib.load()
    head_out, proposals = _req(head_out, "head_out"), _req(proposals, "proposals")
    NC = int(num_classes)
    if proposals.dim() != 3 or proposals.shape[2] != 4 or proposals.shape[0] == 0 or proposals.shape[1] == 0:
        raise ValueError(f"box_postprocess: proposals {tuple(proposals.shape)} is not a non-empty [B, R, 4]")
    B, R = proposals.shape[:2]
    if NC < 2 or head_out.dim() != 2 or head_out.shape[0] != B * R or head_out.shape[1] < 5 * NC:
        raise ValueError(f"box_postprocess: head_out {tuple(head_out.shape)} is not [{B * R}, >= {5 * NC}]")
    _check_candidates(R, NC)
    if count is not None and tuple(_req_i32(count, "count").shape) != (B,):
        raise ValueError(f"count {tuple(count.shape)} is not [{B}]")
    N = R * (NC - 1)
    boxes = torch.empty((B, N, 4), device=head_out.device, dtype=torch.float32)
    scores = torch.empty((B, N), device=head_out.device, dtype=torch.float32)
    labels = torch.empty((B, N), device=head_out.device, dtype=torch.int32)
    _launch(_device(head_out, proposals, count), lib.ldit_box_postprocess_f32, _ptr(head_out), head_out.shape[1], _ptr(proposals), _ptr(count),
            B, R, NC, float(image_size[0]), float(image_size[1]), (C.c_float * 4)(*[float(w) for w in weights]), float(score_thresh),
            float(min_size), _ptr(boxes), _ptr(scores), _ptr(labels))
    return boxes, scores, labels


def box_detections_padded(head_out: torch.Tensor, proposals: torch.Tensor, count: Optional[torch.Tensor], image_size, num_classes: int,
                          score_thresh: float = 0.05, nms_thresh: float = 0.5, detections_per_img: int = 100, min_size: float = 1e-2,
                          weights=(10.0, 10.0, 5.0, 5.0)):
    """:func:`box_postprocess`, the batched NMS keyed by label and the gather of the kept labels: ``(boxes [B, D, 4], scores [B, D],
    labels int32 [B, D], count int32 [B])`` with ``D = detections_per_img``, descending score, zero padding.  No synchronisation."""
    boxes, scores, labels = box_postprocess(head_out, proposals, count, image_size, num_classes, score_thresh, min_size, weights)
    keep, kept, out_boxes, out_scores = batched_nms_padded(boxes, scores, labels, nms_thresh, detections_per_img)
    picked = labels.gather(1, keep.clamp(min=0).to(torch.int64))
    return out_boxes, out_scores, torch.where(keep >= 0, picked, torch.zeros_like(picked)), kept


# ---- box head training (include/ldit.h "box head training"; csrc/roi_train.hip) ------------------------------------------------
ROI_TARGETS_MAX_CANDIDATES = 4096        # proposals + GT boxes per image (ldit_roi_targets_f32)


def roi_targets(proposals: torch.Tensor, count: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_count: torch.Tensor,
                keys: torch.Tensor, fg_iou_thresh: float = 0.5, bg_iou_thresh: float = 0.5, batch_size_per_image: int = 512,
                positive_fraction: float = 0.25, weights=(10.0, 10.0, 5.0, 5.0)):
    """``RoIHeads.select_training_samples`` in one launch: the GT boxes join the proposals, ``Matcher(fg, bg)``, the balanced sampler
    on the caller's ``keys`` and ``BoxCoder(weights).encode``.  ``proposals`` [B, R, 4] with ``count`` int32 [B], ``gt_boxes``
    [B, Gmax, 4], ``gt_labels`` int32 [B, Gmax], ``gt_count`` int32 [B], ``keys`` int32 [B, R + Gmax] (non-negative random
    priorities).  Returns, with ``S = batch_size_per_image``, ``rois`` [B, S, 4], ``labels`` int32 [B, S] (class / 0 = background /
    -1 = padding), ``reg_targets`` [B, S, 4], ``matched`` int32 [B, S] (GT index or -1) and ``sampled`` int32 [B, 2]; the sampled
    positives come first, then the background rows, each in (key, index) order, then zero padding.  No synchronisation."""
    lib = _lib.load()
    proposals, gt_boxes = _req(proposals, "proposals"), _req(gt_boxes, "gt_boxes")
    count, gt_labels = _req_i32(count, "count"), _req_i32(gt_labels, "gt_labels")
    gt_count, keys = _req_i32(gt_count, "gt_count"), _req_i32(keys, "keys")
    if proposals.dim() != 3 or proposals.shape[2] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise ValueError(f"roi_targets: proposals {tuple(proposals.shape)} / gt_boxes {tuple(gt_boxes.shape)} are not [B, R, 4] / [B, Gmax, 4]")
    (B, R), Gmax = proposals.shape[:2], gt_boxes.shape[1]
    if gt_boxes.shape[0] != B or tuple(gt_labels.shape) != (B, Gmax) or tuple(count.shape) != (B,) or tuple(gt_count.shape) != (B,) or \
            tuple(keys.shape) != (B, R + Gmax):
        raise ValueError(f"roi_targets: gt_boxes {tuple(gt_boxes.shape)}, gt_labels {tuple(gt_labels.shape)}, count {tuple(count.shape)}, gt_count "
                         f"{tuple(gt_count.shape)}, keys {tuple(keys.shape)} do not fit [{B}, {R}, 4] proposals")
    if B == 0 or R == 0 or Gmax == 0:
        raise ValueError("roi_targets: empty problem (pad gt_boxes to at least one row)")
    if batch_size_per_image <= 0 or not 0.0 < positive_fraction <= 1.0 or bg_iou_thresh > fg_iou_thresh:
        raise ValueError("roi_targets: need batch_size_per_image > 0, 0 < positive_fraction <= 1 and bg_iou_thresh <= fg_iou_thresh")
    if R + Gmax > ROI_TARGETS_MAX_CANDIDATES:
        raise ValueError(f"roi_targets: {R} proposals + {Gmax} GT boxes per image, at most {ROI_TARGETS_MAX_CANDIDATES} candidates are handled")
    dev, S = proposals.device, int(batch_size_per_image)
    rois = torch.empty((B, S, 4), device=dev, dtype=torch.float32)
    labels = torch.empty((B, S), device=dev, dtype=torch.int32)
    reg_targets = torch.empty((B, S, 4), device=dev, dtype=torch.float32)
    matched = torch.empty((B, S), device=dev, dtype=torch.int32)
    sampled = torch.empty((B, 2), device=dev, dtype=torch.int32)
    _launch(_device(proposals, count, gt_boxes, gt_labels, gt_count, keys), lib.ldit_roi_targets_f32, _ptr(proposals), _ptr(count), _ptr(gt_boxes),
            _ptr(gt_labels), _ptr(gt_count), _ptr(keys), B, R, Gmax, float(fg_iou_thresh), float(bg_iou_thresh), S, float(positive_fraction),
            (C.c_float * 4)(*[float(w) for w in weights]), _ptr(rois), _ptr(labels), _ptr(reg_targets), _ptr(matched), _ptr(sampled))
    return rois, labels, reg_targets, matched, sampled


def roi_align_levels_bwd(d_out: torch.Tensor, boxes: torch.Tensor, count: Optional[torch.Tensor], levels: torch.Tensor,
                         map_shapes: Sequence, image_size, output_size: int = 7, sampling_ratio: int = 2, out: Optional[Sequence[torch.Tensor]] = None):
    """The gradient of :func:`roi_align_levels` with respect to its maps, in one launch without atomics.  ``d_out`` [B * S, P, P, C],
    ``boxes`` [B, S, 4], ``count`` int32 [B] or None and ``levels`` int32 [B, S] as the forward returned them; ``map_shapes``: the
    ``(h, w)`` of every map, finest first.  Returns one gradient per map as a ``[B, C, h, w]`` tensor in channels-last memory (an
    NCHW view of the NHWC buffer the kernel writes), every element written exactly once; ``out`` supplies such tensors (channel
    stride 1, any batch / row / pixel stride) instead of fresh ones.  No synchronisation."""
    lib = _lib.load()
    d_out, boxes, levels = _req(d_out, "d_out"), _req(boxes, "boxes"), _req_i32(levels, "levels")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or 0 in boxes.shape:
        raise ValueError(f"roi_align_levels_bwd: boxes {tuple(boxes.shape)} is not a non-empty [B, S, 4]")
    B, S = boxes.shape[:2]
    P = int(output_size)
    if d_out.dim() != 4 or tuple(d_out.shape[:3]) != (B * S, P, P) or tuple(levels.shape) != (B, S):
        raise ValueError(f"roi_align_levels_bwd: d_out {tuple(d_out.shape)} / levels {tuple(levels.shape)} are not [{B * S}, {P}, {P}, C] / [{B}, {S}]")
    if count is not None and tuple(_req_i32(count, "count").shape) != (B,):
        raise ValueError(f"count {tuple(count.shape)} is not [{B}]")
    Cc = d_out.shape[3]
    shapes = [(int(h), int(w)) for h, w in map_shapes]
    if not shapes:
        raise ValueError("roi_align_levels_bwd: there is no feature map")
    if out is None:
        grads = [torch.empty((B, h, w, Cc), device=d_out.device, dtype=torch.float32).permute(0, 3, 1, 2) for h, w in shapes]
    else:
        grads = list(out)
        for i, (g, (h, w)) in enumerate(zip(grads, shapes)):
            if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.float32 or tuple(g.shape) != (B, Cc, h, w) or g.stride(1) != 1:
                raise ValueError(f"out[{i}]: expected a float32 [{B}, {Cc}, {h}, {w}] GPU tensor in channels-last memory")
        if len(grads) != len(shapes):
            raise ValueError("roi_align_levels_bwd: one output per map")
    scales = infer_scales(grads, image_size)
    L = len(grads)
    _launch(_device(d_out, boxes, count, levels, *grads), lib.ldit_roi_align_levels_bwd_f32, _ptr(d_out), _ptr(boxes), _ptr(count), _ptr(levels),
            B, S, (C.c_void_p * L)(*[g.data_ptr() for g in grads]), (C.c_int32 * L)(*[h for h, _ in shapes]), (C.c_int32 * L)(*[w for _, w in shapes]),
            (C.c_float * L)(*scales), (C.c_int64 * L)(*[g.stride(0) for g in grads]), (C.c_int64 * L)(*[g.stride(2) for g in grads]),
            (C.c_int64 * L)(*[g.stride(3) for g in grads]), L, Cc, P, int(sampling_ratio))
    return grads


def box_loss(head_out: torch.Tensor, labels: torch.Tensor, reg_targets: torch.Tensor, sampled: torch.Tensor, num_classes: int,
             beta: float = 1.0 / 9.0):
    """torchvision ``fastrcnn_loss`` and its gradient for unit upstream.  ``head_out`` [M, ld] (class logits in columns ``[0, NC)``,
    deltas in ``[NC, 5 NC)``) and ``labels`` [B, S] / ``reg_targets`` [B, S, 4] / ``sampled`` [B, 2] of :func:`roi_targets`, ``M = B S``.
    Returns ``loss`` [2] (classifier: cross-entropy summed over the sampled rows of the batch and divided by their number; box:
    smooth-L1(``beta``) over the sampled positives' own class, divided by the same number) and ``d_head`` [M, ld]: ONE buffer,
    columns ``[0, NC)`` the gradient of ``loss[0]``, columns ``[NC, 5 NC)`` that of ``loss[1]``, exactly zero everywhere else.
    No synchronisation."""
    lib = _lib.load()
    head_out, reg_targets = _req(head_out, "head_out"), _req(reg_targets, "reg_targets")
    labels, sampled = _req_i32(labels, "labels"), _req_i32(sampled, "sampled")
    NC = int(num_classes)
    if head_out.dim() != 2 or 0 in head_out.shape or NC < 2 or head_out.shape[1] < 5 * NC:
        raise ValueError(f"box_loss: head_out {tuple(head_out.shape)} is not a non-empty [M, >= {5 * NC}]")
    M, ld = head_out.shape
    if labels.numel() != M or reg_targets.numel() != 4 * M or reg_targets.shape[-1] != 4 or sampled.dim() != 2 or sampled.shape[1] != 2 or \
            sampled.shape[0] == 0:
        raise ValueError(f"box_loss: head_out {tuple(head_out.shape)}, labels {tuple(labels.shape)}, reg_targets {tuple(reg_targets.shape)}, "
                         f"sampled {tuple(sampled.shape)} do not fit together")
    if not beta >= 0.0:
        raise ValueError("box_loss: beta must be >= 0")
    dev = head_out.device
    loss = torch.empty((4,), device=dev, dtype=torch.float32)[:2]               # 16 bytes: the library wants aligned operands
    d_head = torch.empty((M, ld), device=dev, dtype=torch.float32)
    need = _lib.box_loss_workspace_bytes(M)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    _launch(_device(head_out, labels, reg_targets, sampled), lib.ldit_box_loss_f32, _ptr(head_out), ld, _ptr(labels), _ptr(reg_targets),
            _ptr(sampled), sampled.shape[0], M, NC, float(beta), _ptr(loss), _ptr(d_head), _ptr(ws), need)
    return loss, d_head


# ---- the detector's optimizer step (csrc/optim_multi.hip) -------------------------------------------------------------------------
OPT_MAX_SEGMENTS = _lib.OPT_MAX_SEGMENTS


def new_opt_state(device, scale: float = 1.0, lr: float = 1e-4) -> torch.Tensor:
    """A fresh ``ldit_opt_state`` block on ``device`` as an int32 tensor of ten 4-byte slots in ``_lib.OPT_STATE_FIELDS`` order
    (the five floats are read through ``.view(torch.float32)``): counters zero, ``scale`` and ``lr`` as given."""
    host = torch.zeros(len(_lib.OPT_STATE_FIELDS), dtype=torch.int32)
    f = host.view(torch.float32)
    f[_lib.OPT_STATE_FIELDS.index("scale")] = float(scale)
    f[_lib.OPT_STATE_FIELDS.index("inv_scale_used")] = 1.0 / float(scale)
    f[_lib.OPT_STATE_FIELDS.index("lr")] = float(lr)
    f[_lib.OPT_STATE_FIELDS.index("bc1")] = 1.0
    f[_lib.OPT_STATE_FIELDS.index("bc2_sqrt")] = 1.0
    return host.to(device)


def _req_opt_state(state: torch.Tensor) -> torch.Tensor:
    """The block's form; that it lives on the GPU beside the segments is _device's check."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.numel() != len(_lib.OPT_STATE_FIELDS) or not state.is_contiguous():
        raise ValueError(f"state: expected the contiguous int32 block of {len(_lib.OPT_STATE_FIELDS)} slots that new_opt_state makes")
    return state


def _req_list(ts, name: str, n: int):
    ts = list(ts)
    if len(ts) != n:
        raise ValueError(f"{name}: {len(ts)} tensors for {n} segments")
    for i, t in enumerate(ts):                   # the tensors' form only: where they live is _device's check, after every form check
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}[{i}]: expected a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}[{i}]: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}[{i}]: expected a contiguous tensor")
    return ts


def _opt_segments(params, grads, exp_avgs, exp_avg_sqs, mirrors):
    """The host array of ``ldit_opt_segment`` for lists of tensors (``params`` None: the check's view, gradients alone)."""
    grads = list(grads)
    grads = _req_list(grads, "grads", len(grads))
    S = len(grads)
    segs = (_lib.LditOptSegment * max(S, 1))()
    if params is None:
        for s, g in zip(segs, grads):
            s.g, s.n = g.data_ptr(), g.numel()
        return segs, S, grads
    params, exp_avgs, exp_avg_sqs = _req_list(params, "params", S), _req_list(exp_avgs, "exp_avgs", S), _req_list(exp_avg_sqs, "exp_avg_sqs", S)
    mirrors = [None] * S if mirrors is None else list(mirrors)
    if len(mirrors) != S:
        raise ValueError(f"mirrors: {len(mirrors)} entries for {S} segments")
    for i, (s, p, g, m, v, mi) in enumerate(zip(segs, params, grads, exp_avgs, exp_avg_sqs, mirrors)):
        if not (p.numel() == g.numel() == m.numel() == v.numel()):
            raise ValueError(f"segment {i}: params, grads and moments differ in length")
        if mi is not None:
            if not isinstance(mi, torch.Tensor) or not mi.is_cuda or mi.dtype != torch.bfloat16 or not mi.is_contiguous() or mi.numel() != p.numel():
                raise ValueError(f"mirrors[{i}]: expected a contiguous bfloat16 GPU tensor of the parameter's length")
            s.bf16_mirror = mi.data_ptr()
        s.p, s.g, s.m, s.v, s.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    return segs, S, params + grads + exp_avgs + exp_avg_sqs + [mi for mi in mirrors if mi is not None]


def grads_check_multi(grads: Sequence[torch.Tensor], state: torch.Tensor) -> None:
    """``state.found_inf |= 1`` if any element of any tensor of ``grads`` is NaN or infinite.  No synchronisation."""
    lib = _lib.load()
    state = _req_opt_state(state)
    segs, S, used = _opt_segments(None, grads, None, None, None)
    _launch(_device(state, *used), lib.ldit_grads_check_multi_f32, segs, S, _ptr(state))


def opt_advance(state: torch.Tensor, betas=(0.9, 0.999), growth_factor: float = 2.0, backoff_factor: float = 0.5,
                growth_interval: int = 2000) -> None:
    """``torch.amp.GradScaler``'s step / update decision and the optimizer's step count on the device state block (one thread):
    consumes ``found_inf``, sets ``skip`` and ``inv_scale_used``, advances ``step`` and the bias corrections or backs the scale off."""
    lib = _lib.load()
    state = _req_opt_state(state)
    _launch(_device(state), lib.ldit_opt_advance, _ptr(state), float(betas[0]), float(betas[1]), float(growth_factor), float(backoff_factor),
            int(growth_interval))


def adamw_multi(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
                exp_avg_sqs: Sequence[torch.Tensor], state: torch.Tensor, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                grad_mul: float = 1.0, mirrors: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """AdamW on every ``(param, grad, exp_avg, exp_avg_sq)`` of the lists in ``ceil(S / OPT_MAX_SEGMENTS)`` launches, or nothing at all
    when ``state.skip`` is set.  The learning rate, the bias corrections and the inverse loss scale are read from ``state`` on the
    device; ``mirrors[i]`` (bfloat16, optional) receives the rounded updated parameter.  Tensors may be views at any element offset."""
    lib = _lib.load()
    state = _req_opt_state(state)
    segs, S, used = _opt_segments(params, grads, exp_avgs, exp_avg_sqs, mirrors)
    _launch(_device(state, *used), lib.ldit_adamw_multi_f32, segs, S, _ptr(state), float(betas[0]), float(betas[1]), float(eps),
            float(weight_decay), float(grad_mul))


# -- global-norm clipping and per-segment hyper-parameters: check + norm -> opt_advance -> clip_finish -> adamw_groups_multi --
OPT_GROUP_SEGMENTS = _lib.OPT_GROUP_SEGMENTS


def new_clip_state(device, max_norm: float = float("inf")) -> torch.Tensor:
    """A fresh ``ldit_clip_state`` block on ``device`` as a float32 tensor of four 4-byte slots in ``_lib.CLIP_STATE_FIELDS`` order
    (``clipped_steps`` is read through ``.view(torch.int32)``): ``max_norm`` as given, everything else zero."""
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("max_norm must be positive")
    host = torch.zeros(len(_lib.CLIP_STATE_FIELDS), dtype=torch.float32)
    host[_lib.CLIP_STATE_FIELDS.index("max_norm")] = max_norm
    return host.to(device)


def _req_clip_state(clip: torch.Tensor) -> torch.Tensor:
    if not isinstance(clip, torch.Tensor) or clip.dtype != torch.float32 or clip.numel() != len(_lib.CLIP_STATE_FIELDS) or not clip.is_contiguous():
        raise ValueError(f"clip: expected the contiguous float32 block of {len(_lib.CLIP_STATE_FIELDS)} slots that new_clip_state makes")
    return clip


def _req_partials(partials: torch.Tensor) -> torch.Tensor:
    if not isinstance(partials, torch.Tensor) or partials.dtype != torch.float64 or partials.dim() != 1 or not partials.is_contiguous():
        raise ValueError("partials: expected a contiguous 1-d float64 tensor")
    return partials


def grad_norm_partials(grads: Sequence[torch.Tensor]) -> int:
    """The number of float64 partial sums ``grads_check_norm_multi`` writes for these tensors (host arithmetic, no launch)."""
    segs, S, _ = _opt_segments(None, grads, None, None, None)
    return _lib.grad_norm_partials(segs, S)


def grads_check_norm_multi(grads: Sequence[torch.Tensor], state: torch.Tensor, partials: torch.Tensor) -> int:
    """``grads_check_multi`` and, in the same pass, one float64 sum of squares per 1 024 elements of every tensor into the front of
    ``partials``.  Returns how many were written (what ``clip_finish`` is to be given).  No synchronisation."""
    lib = _lib.load()
    state, partials = _req_opt_state(state), _req_partials(partials)
    segs, S, used = _opt_segments(None, grads, None, None, None)
    need = _lib.grad_norm_partials(segs, S)
    if partials.numel() < need:
        raise ValueError(f"partials: {partials.numel()} elements, these gradients need {need}")
    _launch(_device(state, partials, *used), lib.ldit_grads_check_norm_multi_f32, segs, S, _ptr(state), _ptr(partials), partials.numel())
    return need


def clip_finish(state: torch.Tensor, clip: torch.Tensor, partials: torch.Tensor, n: int) -> None:
    """After ``opt_advance``: ``clip.total_norm`` = the global L2 norm of the unscaled gradients from the first ``n`` partials and,
    unless the step is skipped, ``clip.clip_coef = min(1, max_norm / (total_norm + 1e-6))``.  One workgroup, no synchronisation."""
    lib = _lib.load()
    state, clip, partials = _req_opt_state(state), _req_clip_state(clip), _req_partials(partials)
    n = int(n)
    if n < 0 or n > partials.numel():
        raise ValueError(f"n = {n} partials of a buffer of {partials.numel()}")
    _launch(_device(state, clip, partials), lib.ldit_clip_finish, _ptr(state), _ptr(clip), _ptr(partials), n)


def adamw_groups_multi(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
                       exp_avg_sqs: Sequence[torch.Tensor], state: torch.Tensor, lr_scales: Sequence[float], weight_decays: Sequence[float],
                       clip: Optional[torch.Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                       mirrors: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """``adamw_multi`` with the learning rate ``state.lr * lr_scales[i]`` and the weight decay ``weight_decays[i]`` for tensor ``i``, on
    gradients multiplied by ``clip.clip_coef`` as well (``clip`` None: by the inverse loss scale alone), in
    ``ceil(S / OPT_GROUP_SEGMENTS)`` launches.  No synchronisation."""
    lib = _lib.load()
    state = _req_opt_state(state)
    if clip is not None:
        clip = _req_clip_state(clip)
    segs, S, used = _opt_segments(params, grads, exp_avgs, exp_avg_sqs, mirrors)
    lr_scales, weight_decays = [float(x) for x in lr_scales], [float(x) for x in weight_decays]
    if len(lr_scales) != S or len(weight_decays) != S:
        raise ValueError(f"lr_scales / weight_decays: {len(lr_scales)} / {len(weight_decays)} entries for {S} segments")
    hyper = (_lib.LditOptHyper * max(S, 1))()
    for i, (h, s, w) in enumerate(zip(hyper, lr_scales, weight_decays)):
        if not s >= 0.0 or not w >= 0.0:
            raise ValueError(f"segment {i}: lr_scale and weight_decay must be >= 0")
        h.lr_scale, h.weight_decay = s, w
    _launch(_device(state, clip, *used), lib.ldit_adamw_groups_multi_f32, segs, hyper, S, _ptr(state), _ptr(clip), float(betas[0]),
            float(betas[1]), float(eps))


# -- gradient accumulation and data-parallel ranks: the fold into one flat gradient bucket, in front of the launches above --
ACC_MAX_SEGMENTS = _lib.ACC_MAX_SEGMENTS


def grads_accumulate_multi(accs: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], overwrite: bool) -> None:
    """``accs[i] = grads[i]`` bit for bit (``overwrite``: ``accs`` is never read) or ``accs[i] += grads[i]``, one fp32 addition per
    element, over the lists in ``ceil(S / ACC_MAX_SEGMENTS)`` launches.  Tensors may be views at any element offset; a pair must not
    overlap.  No synchronisation, nothing allocated."""
    lib = _lib.load()
    grads = list(grads)
    grads = _req_list(grads, "grads", len(grads))
    S = len(grads)
    accs = _req_list(accs, "accs", S)
    segs = (_lib.LditAccSegment * max(S, 1))()
    for i, (s, a, g) in enumerate(zip(segs, accs, grads)):
        if a.numel() != g.numel():
            raise ValueError(f"segment {i}: accs and grads differ in length ({a.numel()} and {g.numel()})")
        s.acc, s.g, s.n = a.data_ptr(), g.data_ptr(), g.numel()
    if S == 0:
        return
    _launch(_device(*accs, *grads), lib.ldit_grads_accumulate_multi_f32, segs, S, 1 if overwrite else 0)


# -- an exponential moving average of the weights inside the update's launch, and the exchange that evaluates on it --
EMA_MAX_SEGMENTS = _lib.EMA_MAX_SEGMENTS
SWAP_MAX_SEGMENTS = _lib.SWAP_MAX_SEGMENTS


def adamw_ema_groups_multi(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
                           exp_avg_sqs: Sequence[torch.Tensor], state: torch.Tensor, lr_scales: Sequence[float], weight_decays: Sequence[float],
                           shadows: Sequence[Optional[torch.Tensor]], ema_decay: float, ema_warmup: bool = True,
                           clip: Optional[torch.Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                           mirrors: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """``adamw_groups_multi`` and, in the same launches, ``shadows[i] += w * (params[i] - shadows[i])`` on the updated parameter for
    every ``i`` whose shadow is not None (float32, the parameter's length, overlapping nothing).  ``w = 1 - d`` with ``d = ema_decay``,
    or ``min(ema_decay, (1 + step) / (10 + step))`` under ``ema_warmup``, ``step`` the count of steps taken in ``state`` - formed on the
    device; a skipped step moves no shadow.  ``ceil(S / EMA_MAX_SEGMENTS)`` launches.  No synchronisation."""
    lib = _lib.load()
    state = _req_opt_state(state)
    if clip is not None:
        clip = _req_clip_state(clip)
    segs, S, used = _opt_segments(params, grads, exp_avgs, exp_avg_sqs, mirrors)
    lr_scales, weight_decays = [float(x) for x in lr_scales], [float(x) for x in weight_decays]
    if len(lr_scales) != S or len(weight_decays) != S:
        raise ValueError(f"lr_scales / weight_decays: {len(lr_scales)} / {len(weight_decays)} entries for {S} segments")
    hyper = (_lib.LditOptHyper * max(S, 1))()
    for i, (h, s, w) in enumerate(zip(hyper, lr_scales, weight_decays)):
        if not s >= 0.0 or not w >= 0.0:
            raise ValueError(f"segment {i}: lr_scale and weight_decay must be >= 0")
        h.lr_scale, h.weight_decay = s, w
    ema_decay = float(ema_decay)
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    shadows = list(shadows)
    if len(shadows) != S:
        raise ValueError(f"shadows: {len(shadows)} entries for {S} segments")
    ema = (C.c_void_p * max(S, 1))()
    given = _req_list([e for e in shadows if e is not None], "shadows", sum(e is not None for e in shadows))
    for i, e in enumerate(shadows):
        if e is not None:
            if e.numel() != segs[i].n:
                raise ValueError(f"shadows[{i}]: {e.numel()} elements beside a parameter of {segs[i].n}")
            ema[i] = e.data_ptr()
    _launch(_device(state, clip, *used, *given), lib.ldit_adamw_ema_groups_multi_f32, segs, hyper, ema, S, _ptr(state), _ptr(clip),
            float(betas[0]), float(betas[1]), float(eps), ema_decay, 1 if ema_warmup else 0)


def swap_multi(a: Sequence[torch.Tensor], b: Sequence[torch.Tensor], mirrors: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """``a[i] <-> b[i]`` bit for bit (the elements move as integers) over the lists in ``ceil(S / SWAP_MAX_SEGMENTS)`` launches;
    ``mirrors[i]`` (bfloat16, optional) receives the rounded new ``a[i]``.  Calling it twice restores every bit.  Tensors may be views
    at any element offset; a pair must not overlap.  No synchronisation, nothing allocated."""
    lib = _lib.load()
    a = list(a)
    S = len(a)
    a, b = _req_list(a, "a", S), _req_list(b, "b", S)
    mirrors = [None] * S if mirrors is None else list(mirrors)
    if len(mirrors) != S:
        raise ValueError(f"mirrors: {len(mirrors)} entries for {S} segments")
    segs = (_lib.LditSwapSegment * max(S, 1))()
    for i, (s, x, y, mi) in enumerate(zip(segs, a, b, mirrors)):
        if x.numel() != y.numel():
            raise ValueError(f"segment {i}: a and b differ in length ({x.numel()} and {y.numel()})")
        if mi is not None:
            if not isinstance(mi, torch.Tensor) or not mi.is_cuda or mi.dtype != torch.bfloat16 or not mi.is_contiguous() or mi.numel() != x.numel():
                raise ValueError(f"mirrors[{i}]: expected a contiguous bfloat16 GPU tensor of the segment's length")
            s.bf16_mirror = mi.data_ptr()
        s.a, s.b, s.n = x.data_ptr(), y.data_ptr(), x.numel()
    if S == 0:
        return
    _launch(_device(*a, *b, *[mi for mi in mirrors if mi is not None]), lib.ldit_swap_multi_f32, segs, S)


def requant_train_mirror(flat_state, opt_state: Optional[torch.Tensor] = None) -> None:
    """The MX operands of a quantisation-aware encoder's training mirror re-made from its fp32 master in ONE launch
    (``ldit_requant_train_mirror``): every layer's four matrices (codes, scales, dequantised bf16 copies) and fused bias, nothing else.
    ``flat_state``: the encoder's :class:`~layoutdit_amd.training.FlatState` (mxfp8 with ``qat=True``).  ``opt_state``: the step's
    ``ldit_opt_state`` block; with its ``skip`` set nothing is written.  No synchronisation."""
    lib = _lib.load()
    if not getattr(flat_state, "mx", False):
        raise ValueError("requant_train_mirror: the flat state is not the quantisation-aware mxfp8 build's (DiTEncoder(compute_dtype='mxfp8', qat=True))")
    if opt_state is not None:
        opt_state = _req_opt_state(opt_state)
    params, mirror = _req(flat_state.params, "flat_state.params"), flat_state.packed
    _launch(_device(params, mirror, opt_state), lib.ldit_requant_train_mirror, C.byref(flat_state.lcfg), _ptr(params), _ptr(mirror),
            mirror.numel(), _ptr(opt_state))


# ---- COCO box evaluation (include/ldit.h "COCO box evaluation"; csrc/coco_eval.hip) -----------------------------------------------------
COCO_MAX_DETS, COCO_MAX_GT, COCO_MAX_CLASSES = 128, 128, 64      # per image: detection slots, GT boxes; categories
COCO_MAX_SLOTS = 1 << 24                                         # capacity * slots per image the total-order key has room for


def _req_form(t, name: str, dtype: torch.dtype, shape) -> torch.Tensor:
    """The tensor's form only (dtype, contiguity, shape): where it lives is _device's check, after every form check."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _coco_caps(D: int, G: int, K: int) -> None:
    if D > COCO_MAX_DETS or G > COCO_MAX_GT or K > COCO_MAX_CLASSES:
        raise ValueError(f"coco: D={D} G={G} K={K}: at most {COCO_MAX_DETS} detections and {COCO_MAX_GT} GT boxes per image and "
                         f"{COCO_MAX_CLASSES} categories are handled")
    if D < 1 or G < 1 or K < 1:
        raise ValueError(f"coco: D={D} G={G} K={K}: empty problem (pad to at least one row)")


def _coco_store(code, rank, npig, scores_out, labels_out, K: int):
    """The evaluator's store: ``code`` uint8 [N, Ds, 4, 10], ``rank`` int32 [N, Ds], ``npig`` int32 [N, K, 4], ``scores_out`` fp32 and
    ``labels_out`` int32 [N, Ds].  Returns ``(N, Ds)``."""
    if not isinstance(rank, torch.Tensor) or rank.dim() != 2:
        raise ValueError("coco: rank: expected an int32 [N, D] tensor")
    N, Ds = rank.shape
    _req_form(code, "code", torch.uint8, (N, Ds, 4, 10))
    _req_form(rank, "rank", torch.int32, (N, Ds))
    _req_form(npig, "npig", torch.int32, (N, K, 4))
    _req_form(scores_out, "scores_out", torch.float32, (N, Ds))
    _req_form(labels_out, "labels_out", torch.int32, (N, Ds))
    if N < 1 or N * Ds > COCO_MAX_SLOTS:
        raise ValueError(f"coco: a store of {N} x {Ds} slots: between 1 and 2^24 are handled")
    return N, Ds


def coco_match(boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, count: torch.Tensor, gt_boxes: torch.Tensor,
               gt_labels: torch.Tensor, gt_count: torch.Tensor, gt_crowd: Optional[torch.Tensor], gt_area: Optional[torch.Tensor],
               num_classes: int, code: torch.Tensor, rank: torch.Tensor, npig: torch.Tensor, scores_out: torch.Tensor,
               labels_out: torch.Tensor, image_offset: int, iou_thrs: Sequence[float], area_rng: Sequence[Sequence[float]]) -> None:
    """COCO's per-image matching for a padded batch, written into rows ``[image_offset, image_offset + B)`` of the caller's store
    (``ldit_coco_match``).  ``boxes`` [B, D, 4], ``scores`` [B, D], ``labels`` int32 [B, D], ``count`` int32 [B]; ``gt_boxes`` [B, G, 4],
    ``gt_labels`` int32 [B, G], ``gt_count`` int32 [B], ``gt_crowd`` uint8 [B, G] or None, ``gt_area`` fp32 [B, G] or None.  ``iou_thrs``:
    10 doubles, ``area_rng``: 4 ``(lo, hi)`` pairs - they reach the kernel bit for bit.  No synchronisation, no allocation."""
    lib = _lib.load()
    K = int(num_classes)
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2 or not isinstance(gt_labels, torch.Tensor) or gt_labels.dim() != 2:
        raise ValueError("coco_match: scores / gt_labels: expected [B, D] / [B, G] tensors")
    (B, D), G = scores.shape, gt_labels.shape[1]
    _coco_caps(D, G, K)
    _req_form(boxes, "boxes", torch.float32, (B, D, 4)), _req_form(scores, "scores", torch.float32, (B, D))
    _req_form(labels, "labels", torch.int32, (B, D)), _req_form(count, "count", torch.int32, (B,))
    _req_form(gt_boxes, "gt_boxes", torch.float32, (B, G, 4)), _req_form(gt_labels, "gt_labels", torch.int32, (B, G))
    _req_form(gt_count, "gt_count", torch.int32, (B,))
    if gt_crowd is not None:
        _req_form(gt_crowd, "gt_crowd", torch.uint8, (B, G))
    if gt_area is not None:
        _req_form(gt_area, "gt_area", torch.float32, (B, G))
    N, Ds = _coco_store(code, rank, npig, scores_out, labels_out, K)
    if B < 1 or Ds < D:
        raise ValueError(f"coco_match: a batch of {B} images x {D} detections does not fit rows of {Ds} slots")
    if image_offset < 0 or image_offset + B > N:
        raise ValueError(f"coco_match: images [{image_offset}, {image_offset + B}) do not fit a store of {N}")
    thr = [float(x) for x in iou_thrs]
    rng = [float(x) for pair in area_rng for x in pair]
    if len(thr) != 10 or len(rng) != 8:
        raise ValueError("coco_match: 10 IoU thresholds and 4 (lo, hi) area ranges are expected")
    _launch(_device(boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_crowd, gt_area, code, rank, npig, scores_out, labels_out),
            lib.ldit_coco_match, _ptr(boxes), _ptr(scores), _ptr(labels), _ptr(count), _ptr(gt_boxes), _ptr(gt_labels), _ptr(gt_crowd),
            _ptr(gt_area), _ptr(gt_count), B, D, G, K, (C.c_double * 10)(*thr), (C.c_double * 8)(*rng), _ptr(code), _ptr(rank), _ptr(npig),
            _ptr(scores_out), _ptr(labels_out), N, Ds, int(image_offset))


def coco_accumulate(code: torch.Tensor, rank: torch.Tensor, npig: torch.Tensor, scores_out: torch.Tensor, labels_out: torch.Tensor,
                    n_images: int, num_classes: int, rec_thrs: Sequence[float], max_dets: Sequence[int] = (1, 10, 100),
                    precision: Optional[torch.Tensor] = None, recall: Optional[torch.Tensor] = None):
    """COCO's accumulation over the first ``n_images`` rows of the store :func:`coco_match` filled: one total-order key per stored
    detection (``ldit_coco_keys``), ``torch.sort`` of the keys (the device-wide sort is plumbing), then ``ldit_coco_accumulate``.
    Returns ``precision`` fp64 [10, 101, K, 4, 3] and ``recall`` fp64 [10, K, 4, 3] (``-1`` where a cell has no GT).  No synchronisation."""
    lib = _lib.load()
    K = int(num_classes)
    _coco_caps(1, 1, K)
    N, Ds = _coco_store(code, rank, npig, scores_out, labels_out, K)
    n = int(n_images)
    if n < 0 or n > N:
        raise ValueError(f"coco_accumulate: {n} images in a store of {N}")
    rec = [float(x) for x in rec_thrs]
    md = [int(m) for m in max_dets]
    if len(rec) != 101 or len(md) != 3:
        raise ValueError("coco_accumulate: 101 recall thresholds and 3 maxDets are expected")
    dev = _device(code, rank, npig, scores_out, labels_out, precision, recall)
    if precision is None:
        precision = torch.empty((10, 101, K, 4, 3), device=dev, dtype=torch.float64)
    if recall is None:
        recall = torch.empty((10, K, 4, 3), device=dev, dtype=torch.float64)
    _req_form(precision, "precision", torch.float64, (10, 101, K, 4, 3)), _req_form(recall, "recall", torch.float64, (10, K, 4, 3))
    keys = index = None
    if n:
        keys = torch.empty(n * Ds, device=dev, dtype=torch.int64)
        _launch(_device(rank, scores_out, labels_out, keys), lib.ldit_coco_keys, _ptr(rank), _ptr(scores_out), _ptr(labels_out), n, Ds, _ptr(keys))
        with torch.cuda.device(dev):
            keys, index = torch.sort(keys)
    _launch(_device(code, rank, npig, precision, recall, keys, index), lib.ldit_coco_accumulate, _ptr(keys), _ptr(index), _ptr(code), _ptr(rank),
            _ptr(npig), n, Ds, K, (C.c_double * 101)(*rec), (C.c_int32 * 3)(*md), _ptr(precision), _ptr(recall))
    return precision, recall


# ---- train-time augmentation of the targets (include/ldit.h "train-time augmentation"; csrc/augment.hip) ------------------------------
def augment_targets(gt_boxes: torch.Tensor, gt_labels: Optional[torch.Tensor], gt_count: torch.Tensor, windows, size,
                    min_visibility: float = 0.3, min_size: float = 1.0):
    """The padded targets of a batch through the windows :func:`preprocess` cut from its pages: ``gt_boxes`` [B, Gmax, 4] in the pages'
    pixels, ``gt_labels`` int32 [B, Gmax] or None, ``gt_count`` int32 [B], ``windows`` as for :func:`window_args`, ``size`` the batch's
    ``(out_h, out_w)`` (or one int).  A box is clipped to its window and kept if its clipped area is positive and at least
    ``min_visibility`` of its own; it is shifted to the window, mirrored under ``flip`` and scaled to the batch, and kept if both sides
    are then at least ``min_size``.  Returns ``(out_boxes [B, Gmax, 4], out_labels int32 [B, Gmax] or None, out_count int32 [B])``: the
    kept rows in their original order, zeros behind them - the triple ``RoIHeads`` takes, its first and last member the pair of the
    RPN.  Rows at or beyond ``gt_count`` are never read.  ``Gmax <= RPN_TARGETS_MAX_GT``.  One launch per 48 images, no
    synchronisation."""
    lib = _lib.load()
    if not isinstance(gt_boxes, torch.Tensor) or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise ValueError(f"augment_targets: gt_boxes {tuple(getattr(gt_boxes, 'shape', ()))} is not [B, Gmax, 4]")
    B, Gmax = gt_boxes.shape[:2]
    wins = window_args(windows, B)                       # host checks first: they need no GPU
    out_h, out_w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if out_h <= 0 or out_w <= 0 or not float(min_visibility) >= 0.0 or not float(min_size) >= 0.0:
        raise ValueError("augment_targets: need a positive size and non-negative min_visibility and min_size")
    gt_boxes, gt_count = _req(gt_boxes, "gt_boxes"), _req_i32(gt_count, "gt_count")
    if gt_labels is not None:
        gt_labels = _req_i32(gt_labels, "gt_labels")
    if tuple(gt_count.shape) != (B,) or (gt_labels is not None and tuple(gt_labels.shape) != (B, Gmax)):
        raise ValueError(f"augment_targets: gt_count {tuple(gt_count.shape)} / gt_labels "
                         f"{None if gt_labels is None else tuple(gt_labels.shape)} are not [{B}] / [{B}, {Gmax}]")
    if B == 0 or Gmax == 0:
        raise ValueError("augment_targets: empty problem (pad gt_boxes to at least one row)")
    if Gmax > RPN_TARGETS_MAX_GT:
        raise ValueError(f"augment_targets: Gmax = {Gmax}, at most {RPN_TARGETS_MAX_GT} boxes per image are handled")
    dev = gt_boxes.device
    out_boxes = torch.empty((B, Gmax, 4), device=dev, dtype=torch.float32)
    out_labels = None if gt_labels is None else torch.empty((B, Gmax), device=dev, dtype=torch.int32)
    out_count = torch.empty((B,), device=dev, dtype=torch.int32)
    _launch(_device(gt_boxes, gt_labels, gt_count), lib.ldit_augment_targets_f32, _ptr(gt_boxes), _ptr(gt_labels), _ptr(gt_count), wins, B,
            Gmax, out_h, out_w, float(min_visibility), float(min_size), _ptr(out_boxes), _ptr(out_labels), _ptr(out_count))
    return out_boxes, out_labels, out_count


# ---- test-time augmentation, the merge (include/ldit.h "test-time augmentation"; csrc/tta_merge.hip) ----------------------------------
TTA_MAX_VIEWS = 16


def _tta_views(views, view_specs, original_sizes, who: str):
    """Host checks of the merge's arguments (they need no GPU): ``(V, B, D, specs, pages)`` with the two HOST int32 arrays of the C ABI."""
    views, specs_in = list(views), list(view_specs)
    V = len(views)
    if V < 1 or V > TTA_MAX_VIEWS:
        raise ValueError(f"{who}: {V} views, between 1 and {TTA_MAX_VIEWS} are handled")
    if len(specs_in) != V:
        raise ValueError(f"{who}: {len(specs_in)} view specs for {V} views")
    if any(not isinstance(v, (tuple, list)) or len(v) != 4 for v in views):
        raise ValueError(f"{who}: every view is the tuple (boxes, scores, labels, count) of forward_padded")
    if not isinstance(views[0][1], torch.Tensor) or views[0][1].dim() != 2:
        raise ValueError(f"{who}: views[0]: scores: expected a [B, D] tensor")
    B, D = views[0][1].shape
    if B < 1 or D < 1:
        raise ValueError(f"{who}: empty problem (B={B}, D={D})")
    if V * D > NMS_MAX_CANDIDATES:
        raise ValueError(f"{who}: {V} views x {D} detections = {V * D} pool entries per image, at most NMS_MAX_CANDIDATES = "
                         f"{NMS_MAX_CANDIDATES} are handled (fewer views, or a smaller detections_per_img)")
    for v, (boxes, scores, labels, count) in enumerate(views):
        _req_form(boxes, f"views[{v}]: boxes", torch.float32, (B, D, 4)), _req_form(scores, f"views[{v}]: scores", torch.float32, (B, D))
        _req_form(labels, f"views[{v}]: labels", torch.int32, (B, D)), _req_form(count, f"views[{v}]: count", torch.int32, (B,))
    flat = []
    for v, s in enumerate(specs_in):
        try:
            s = [operator.index(x) for x in s]
        except TypeError:
            s = None
        if s is None or len(s) != 3 or s[0] < 1 or s[1] < 1 or s[2] not in (0, 1) or max(s[:2]) >= 2 ** 31:
            raise ValueError(f"{who}: view_specs[{v}] must be (width >= 1, height >= 1, flip 0 or 1), got {specs_in[v]!r}")
        flat.extend(s)
    pages = [(operator.index(hw[0]), operator.index(hw[1])) for hw in original_sizes]
    if len(pages) != B:
        raise ValueError(f"{who}: {len(pages)} original sizes for {B} images")
    if any(h < 1 or w < 1 or max(h, w) >= 2 ** 31 for h, w in pages):
        raise ValueError(f"{who}: original_sizes are the pages' (height, width), each at least 1")
    return V, B, D, (C.c_int32 * (3 * V))(*flat), (C.c_int32 * (2 * B))(*[x for h, w in pages for x in (w, h)])


def tta_pool(views, view_specs, original_sizes):
    """The padded detections of ``V`` views of one batch as one pool per image, in the pages' coordinates (``ldit_tta_pool_f32``).
    ``views``: ``V`` tuples ``(boxes [B, D, 4], scores [B, D], labels int32 [B, D], count int32 [B])`` as ``forward_padded`` returns
    them, each in its view's coordinates; ``view_specs``: ``V`` triples ``(width, height, flip)``; ``original_sizes``: the pages'
    ``(height, width)`` as ``img.shape[-2:]`` gives them.  Returns ``(pool_boxes [B, V * D, 4], pool_scores [B, V * D], pool_labels int32
    [B, V * D])``, entry ``v * D + d`` from detection ``d`` of view ``v``: unmirrored where ``flip`` is 1, then times ``(rw, rh, rw, rh)``
    formed as ``resize_boxes`` forms them; an entry at or beyond its view's count has score ``-inf``, label 0 and a zero box, whatever
    the input's padding row holds.  The host integers travel in the kernel arguments: no copy, no synchronisation."""
    lib = _lib.load()
    V, B, D, specs, pages = _tta_views(views, view_specs, original_sizes, "tta_pool")
    tensors = [t for view in views for t in view]
    dev = _device(*tensors)
    pool_boxes = torch.empty((B, V * D, 4), device=dev, dtype=torch.float32)
    pool_scores = torch.empty((B, V * D), device=dev, dtype=torch.float32)
    pool_labels = torch.empty((B, V * D), device=dev, dtype=torch.int32)
    ptrs = [(C.c_void_p * V)(*[view[m].data_ptr() for view in views]) for m in range(4)]
    _launch(_device(*tensors), lib.ldit_tta_pool_f32, ptrs[0], ptrs[1], ptrs[2], ptrs[3], specs, pages, V, B, D, _ptr(pool_boxes),
            _ptr(pool_scores), _ptr(pool_labels))
    return pool_boxes, pool_scores, pool_labels


def box_vote(pool_boxes: torch.Tensor, pool_scores: torch.Tensor, pool_labels: torch.Tensor, keep: torch.Tensor, kept: torch.Tensor,
             vote_thresh: Optional[float] = None):
    """Behind :func:`batched_nms_padded` on a pool (``keep`` int32 [B, D_out], ``kept`` int32 [B]): ``(boxes [B, D_out, 4] or None, labels
    int32 [B, D_out])`` (``ldit_box_vote_f32``).  The labels are the kept entries' own.  The box of a kept entry is the score-weighted
    mean of every pool entry of its image with its label, a score ``> -inf`` and an IoU with it ``>= vote_thresh`` (the NMS's fp32
    IoU; the entry itself always) - sums and quotient in double, rounded to fp32 once, in a fixed order, so two runs agree bit for
    bit.  Rows at or beyond ``kept`` are zero.  ``vote_thresh=None``: no arithmetic, boxes ``None`` (the NMS's own stand), only the
    labels are gathered.  One launch, no synchronisation."""
    lib = _lib.load()
    if not isinstance(pool_scores, torch.Tensor) or pool_scores.dim() != 2 or not isinstance(keep, torch.Tensor) or keep.dim() != 2:
        raise ValueError("box_vote: pool_scores / keep: expected [B, N] / [B, D_out] tensors")
    (B, N), Dout = pool_scores.shape, keep.shape[1]
    if B < 1 or N < 1 or Dout < 1:
        raise ValueError("box_vote: empty problem")
    if N > NMS_MAX_CANDIDATES:
        raise ValueError(f"box_vote: {N} pool entries per image, at most NMS_MAX_CANDIDATES = {NMS_MAX_CANDIDATES} are handled")
    if vote_thresh is not None and not 0.0 <= float(vote_thresh) <= 1.0:
        raise ValueError(f"box_vote: vote_thresh = {vote_thresh} is outside [0, 1]")
    _req_form(pool_boxes, "pool_boxes", torch.float32, (B, N, 4)), _req_form(pool_scores, "pool_scores", torch.float32, (B, N))
    _req_form(pool_labels, "pool_labels", torch.int32, (B, N)), _req_form(keep, "keep", torch.int32, (B, Dout))
    _req_form(kept, "kept", torch.int32, (B,))
    dev = _device(pool_boxes, pool_scores, pool_labels, keep, kept)
    boxes = None if vote_thresh is None else torch.empty((B, Dout, 4), device=dev, dtype=torch.float32)
    labels = torch.empty((B, Dout), device=dev, dtype=torch.int32)
    _launch(_device(pool_boxes, pool_scores, pool_labels, keep, kept), lib.ldit_box_vote_f32, _ptr(pool_boxes), _ptr(pool_scores),
            _ptr(pool_labels), _ptr(keep), _ptr(kept), B, N, Dout, 0.0 if vote_thresh is None else float(vote_thresh), _ptr(boxes), _ptr(labels))
    return boxes, labels


def tta_merge(views, view_specs, original_sizes, nms_thresh: float = 0.5, detections_per_img: int = 100,
              vote_thresh: Optional[float] = None):
    """Test-time augmentation's merge: :func:`tta_pool`, one class-wise :func:`batched_nms_padded` over each image's pool (the NMS
    of the box head: same kernel, same IoU arithmetic), :func:`box_vote`.  Arguments as for :func:`tta_pool`; ``V * D`` must not
    exceed ``NMS_MAX_CANDIDATES``.  Returns ``(boxes [B, D_out, 4] in page coordinates, scores [B, D_out], labels int32 [B, D_out], count
    int32 [B])`` with ``D_out = detections_per_img``, zero padding, in the NMS's order: descending score, ties by pool index (plain
    views first, in the order given).  ``vote_thresh=None``: the boxes are the kept pool entries' own bits.  Three launches, no
    synchronisation, capturable."""
    Dout = int(detections_per_img)
    if Dout < 1:
        raise ValueError("tta_merge: detections_per_img must be positive")
    if not 0.0 <= float(nms_thresh) <= 1.0:
        raise ValueError(f"tta_merge: nms_thresh = {nms_thresh} is outside [0, 1]")
    if vote_thresh is not None and not 0.0 <= float(vote_thresh) <= 1.0:
        raise ValueError(f"tta_merge: vote_thresh = {vote_thresh} is outside [0, 1]")
    _tta_views(views, view_specs, original_sizes, "tta_merge")         # every host check before the first launch
    pool_boxes, pool_scores, pool_labels = tta_pool(views, view_specs, original_sizes)
    keep, count, boxes, scores = batched_nms_padded(pool_boxes, pool_scores, pool_labels, float(nms_thresh), Dout)
    voted, labels = box_vote(pool_boxes, pool_scores, pool_labels, keep, count, vote_thresh)
    return (boxes if voted is None else voted), scores, labels, count
