#!/usr/bin/env python3
"""Getting 64 decoded pages of 612 x 792 into the detector's 224 x 224 batch: fp32 planar pages (what ToTensor() leaves) against uint8
interleaved pages (what the decoder leaves; layoutdit_amd.data.stage_images + ldit_preprocess_u8), in one process on one device.

  (a) one copy of the pinned fp32 planar pages + ldit_preprocess_f32
  (b) one copy of the pinned uint8 interleaved pages + ldit_preprocess_u8; and stage_images() as a whole, its host-side packing included
  (c) each kernel alone on resident pages: ldit_preprocess_f32 / _u8 planar / _u8 interleaved, and ldit_embed_bf16_images with the
      same three sources (the fused im2col pass TOGETHER with its patch GEMM: no entry runs the pass alone, so the difference between
      two sources is the pass's)
  (d) what (b) no longer asks of the CPU per page: float().div(255) and the transpose to planar

Medians of --runs runs after --warmup.  Stated beforehand: each uint8 kernel alone should take no longer than its fp32 sibling (it
reads a quarter of the bytes and writes the same); "u8_not_slower" in the output says whether that held in this run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import _lib, ops                         # noqa: E402
from layoutdit_amd.data import StagingBuffer, stage_images  # noqa: E402

DEV = torch.device("cuda:0")


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def gpu_ms(fn, runs, warmup, inner=1):
    """HIP events around `inner` back-to-back calls, per call."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return stats(out)


def wall_ms(fn, runs, warmup):
    """Host clock around a call that ends in a device synchronise."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--height", type=int, default=792)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ingest_bench: no GPU (nothing here can be timed on a CPU)")
    lib = _lib.load()
    B, h, w, S = a.pages, a.height, a.width, a.size
    rng = np.random.default_rng(0)
    pages = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]          # as a decoder leaves them
    n = 3 * h * w
    stream = lambda: torch.cuda.current_stream(DEV).cuda_stream                            # noqa: E731
    out = torch.empty((B, 3, S, S), device=DEV, dtype=torch.float32)

    # (d) the CPU work per page that the uint8 path drops
    def to_tensor(p):
        return torch.from_numpy(p).float().div(255).permute(2, 0, 1).contiguous()
    cpu = []
    for p in pages[:max(a.runs, 20)]:
        t0 = time.perf_counter()
        to_tensor(p)
        cpu.append((time.perf_counter() - t0) * 1e3)

    # (a) pinned fp32 planar, one copy, ldit_preprocess_f32
    host32 = torch.empty(B * n, dtype=torch.float32, pin_memory=True)
    for i, p in enumerate(pages):
        host32[i * n:(i + 1) * n].view(3, h, w).copy_(to_tensor(p))
    dev32 = torch.empty(B * n, dtype=torch.float32, device=DEV)
    f32 = [dev32[i * n:(i + 1) * n].view(3, h, w) for i in range(B)]
    _, p32, hs, ws, _, _ = ops.image_list_args(f32)

    def pre_f32():
        _lib.check(lib.ldit_preprocess_f32(p32, hs, ws, B, 3, 0.5, 0.5, S, S, out.data_ptr(), stream()))

    def a_path():
        dev32.copy_(host32, non_blocking=True)
        pre_f32()

    # (b) pinned uint8 interleaved, one copy, ldit_preprocess_u8
    buf = StagingBuffer()
    hwc = stage_images(pages, DEV, buf, layout="hwc")
    torch.cuda.synchronize()
    host8 = buf.host[:B * n]
    dev8 = torch.empty(B * n, dtype=torch.uint8, device=DEV)
    dev8.copy_(host8)
    u8i = [dev8[i * n:(i + 1) * n].view(h, w, 3).permute(2, 0, 1) for i in range(B)]
    u8p = [t.contiguous() for t in u8i]
    _, p8i, _, _, fmt_i, _ = ops.image_list_args(u8i)
    _, p8p, _, _, fmt_p, _ = ops.image_list_args(u8p)
    assert (fmt_i, fmt_p) == (ops.IMG_U8_HWC, ops.IMG_U8)

    def pre_u8(ptrs, inter):
        _lib.check(lib.ldit_preprocess_u8(ptrs, hs, ws, inter, B, 3, 0.5, 0.5, S, S, out.data_ptr(), stream()))

    def b_path():
        dev8.copy_(host8, non_blocking=True)
        pre_u8(p8i, 1)

    def b_whole():
        ops.preprocess(stage_images(pages, DEV, buf, layout="hwc"), size=S)

    # the three sources give one batch, bit for bit
    a_path()
    ref = ops.preprocess(f32, size=S)
    assert torch.equal(out, ref)
    assert torch.equal(ops.preprocess(u8i, size=S), ref) and torch.equal(ops.preprocess(u8p, size=S), ref) and torch.equal(ops.preprocess(hwc, size=S), ref)

    # the fused bf16 patch pass (+ its GEMM), ViT-B's embedding
    Cc, P = 768, (S // 16) ** 2
    g = torch.Generator(device=DEV).manual_seed(1)
    pw16 = (torch.randn(Cc, 768, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    pb, cls = torch.randn(Cc, device=DEV, generator=g) * 0.02, torch.randn(Cc, device=DEV, generator=g) * 0.02
    pos = torch.randn(P + 1, Cc, device=DEV, generator=g) * 0.02
    emb = torch.empty((B, P + 1, Cc), device=DEV, dtype=torch.float32)
    scratch = torch.empty((B * P, 768), device=DEV, dtype=torch.bfloat16)
    tail = (pw16.data_ptr(), pb.data_ptr(), cls.data_ptr(), pos.data_ptr(), emb.data_ptr(), scratch.data_ptr(), B, 3, S, S, 16, Cc)

    def embed_f32():
        _lib.check(lib.ldit_embed_bf16_images(p32, hs, ws, 0, 0.5, 0.5, *tail, stream()))

    def embed_u8(ptrs, inter):
        _lib.check(lib.ldit_embed_bf16_images_u8(ptrs, hs, ws, inter, 0.5, 0.5, *tail, stream()))

    embed_f32()
    want = emb.clone()
    for ptrs, inter in ((p8p, 0), (p8i, 1)):
        embed_u8(ptrs, inter)
        assert torch.equal(emb, want)

    R, W = a.runs, a.warmup
    ms = {}
    for _ in range(2):                      # the same order twice; the second pass is kept (every code object loaded, clocks settled)
        ms = {
            "a/copy_fp32_planar+preprocess_f32": gpu_ms(a_path, R, W),
            "b/copy_u8_interleaved+preprocess_u8": gpu_ms(b_path, R, W),
            "b/stage_images+preprocess_u8 (host packing included, wall clock)": wall_ms(b_whole, R, W),
            "c/preprocess_f32": gpu_ms(pre_f32, R, W, inner=10),
            "c/preprocess_u8_planar": gpu_ms(lambda: pre_u8(p8p, 0), R, W, inner=10),
            "c/preprocess_u8_interleaved": gpu_ms(lambda: pre_u8(p8i, 1), R, W, inner=10),
            "c/embed_bf16_images_f32 (im2col pass + patch GEMM)": gpu_ms(embed_f32, R, W, inner=10),
            "c/embed_bf16_images_u8_planar (im2col pass + patch GEMM)": gpu_ms(lambda: embed_u8(p8p, 0), R, W, inner=10),
            "c/embed_bf16_images_u8_interleaved (im2col pass + patch GEMM)": gpu_ms(lambda: embed_u8(p8i, 1), R, W, inner=10),
        }
    med = lambda k: ms[k]["median_ms"]                                                     # noqa: E731
    result = {
        "note": "one run's numbers on one device, every variant timed in the same process; the copies are one packed transfer each",
        "workload": {"pages": B, "page": [h, w], "target": [S, S], "fp32_planar_mb": round(B * n * 4 / 1e6, 1), "uint8_mb": round(B * n / 1e6, 1),
                     "batch_out_mb": round(out.numel() * 4 / 1e6, 1)},
        "runs": R, "warmup": W,
        "timer": "HIP events on the stream (c: around 10 back-to-back launches, per launch); wall clock ending in a synchronise where stated",
        "ms": ms,
        "d/cpu_per_page_float_div255_transpose": stats(cpu),
        "d/cpu_per_batch_ms": round(statistics.median(cpu) * B, 2),
        "fp32_over_u8": {"copy+preprocess": round(med("a/copy_fp32_planar+preprocess_f32") / med("b/copy_u8_interleaved+preprocess_u8"), 3)},
        "u8_not_slower": {
            "preprocess_u8_planar": med("c/preprocess_u8_planar") <= med("c/preprocess_f32"),
            "preprocess_u8_interleaved": med("c/preprocess_u8_interleaved") <= med("c/preprocess_f32"),
            "embed_bf16_images_u8_planar": med("c/embed_bf16_images_u8_planar (im2col pass + patch GEMM)") <= med("c/embed_bf16_images_f32 (im2col pass + patch GEMM)"),
            "embed_bf16_images_u8_interleaved": med("c/embed_bf16_images_u8_interleaved (im2col pass + patch GEMM)") <= med("c/embed_bf16_images_f32 (im2col pass + patch GEMM)"),
        },
        "agreement": "ldit_preprocess_f32, _u8 planar and _u8 interleaved: torch.equal; the three ldit_embed_bf16_images sources: torch.equal",
        "device": torch.cuda.get_device_name(DEV),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
