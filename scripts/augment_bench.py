#!/usr/bin/env python3
"""Train-time augmentation inside the input transform: 64 pages of 792 x 612 to 224 x 224, each image format, one
process on one device, every pair timed alternately (one window of each member in turn, so clock drift falls on both):

  (a) the windowed transform on WHOLE-PAGE windows against the existing transform on the same pages - what the window arguments cost
      when they change nothing (ldit_preprocess_win_* against ldit_preprocess_*): through ops.preprocess, whose host-side window
      checks are Python, and as the two C entries on prepared descriptor arrays (the launches alone);
  (b) the windowed transform on random crop / flip windows against what a user did before: torch crop / flip copies of every page,
      then the existing transform on the copies (both produce the same batch, bit for bit - asserted);
  (c) ops.augment_targets against a torch version with boolean indexing per image (which synchronises once per image).

Nothing here is a gate: the file records what one run showed, with its ranges."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import _lib, ops                          # noqa: E402
from layoutdit_amd.augment import DetectorAugment, whole_page_windows   # noqa: E402

DEV = torch.device("cuda:0")


def window(fn, inner):
    """Milliseconds per call of `inner` back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def alternate(pair, runs, warmup, inner):
    for _ in range(warmup):
        for _, fn in pair:
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _ in pair}
    for _ in range(runs):                                    # alternating: one window of each in turn
        for name, fn in pair:
            samples[name].append(window(fn, inner))
    out = {name: spread(v) for name, v in samples.items()}
    (na, a), (nb, b) = out.items()
    out["ratio_first_over_second"] = round(a["median_ms"] / b["median_ms"], 3)
    out["separated"] = bool(a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"])
    return out


def torch_augment_targets(gt_boxes, gt_labels, gt_count, windows, size, min_visibility, min_size):
    """What a user wrote before: per image clip, filter with a boolean index, shift, flip, scale, pad again."""
    B, Gmax = gt_boxes.shape[:2]
    out_boxes, out_labels = torch.zeros_like(gt_boxes), torch.zeros_like(gt_labels)
    counts = []
    for i, (x0, y0, cw, ch, flip) in enumerate(windows):
        n = int(gt_count[i])                                 # a synchronisation per image
        b, lab = gt_boxes[i, :n], gt_labels[i, :n]
        lo = torch.tensor([x0, y0, x0, y0], device=b.device, dtype=b.dtype)
        hi = torch.tensor([x0 + cw, y0 + ch, x0 + cw, y0 + ch], device=b.device, dtype=b.dtype)
        c = torch.minimum(torch.maximum(b, lo), hi)
        iw, ih = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
        keep = (iw > 0) & (ih > 0) & (iw * ih >= min_visibility * ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])))
        c = c - lo
        if flip:
            c = torch.stack([cw - c[:, 2], c[:, 1], cw - c[:, 0], c[:, 3]], dim=1)
        c = c * torch.tensor([size[1] / cw, size[0] / ch, size[1] / cw, size[0] / ch], device=b.device, dtype=b.dtype)
        keep &= ((c[:, 2] - c[:, 0]) >= min_size) & ((c[:, 3] - c[:, 1]) >= min_size)
        c, lab = c[keep], lab[keep]                          # boolean indexing: another synchronisation
        out_boxes[i, :c.shape[0]] = c
        out_labels[i, :c.shape[0]] = lab
        counts.append(c.shape[0])
    return out_boxes, out_labels, torch.tensor(counts, dtype=torch.int32, device=gt_boxes.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--height", type=int, default=792)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--boxes", type=int, default=40, help="padded boxes per page for (c)")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "augment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench: no GPU (nothing here can be timed on a CPU)")
    B, h, w, S = a.pages, a.height, a.width, a.size
    rng = np.random.default_rng(0)
    codes = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for _ in range(B)]      # as a decoder leaves them
    lists = {
        "u8_interleaved": [c.permute(2, 0, 1) for c in codes],
        "u8_planar": [c.permute(2, 0, 1).contiguous() for c in codes],
        "f32": [c.permute(2, 0, 1).float().div(255).contiguous() for c in codes],
        "f16": [c.permute(2, 0, 1).float().div(255).half().contiguous() for c in codes],
    }
    sizes = [(h, w)] * B
    whole = whole_page_windows(sizes)
    crops = DetectorAugment(seed=0, flip_prob=0.5).sample(sizes)

    def copies(images, fmt):
        out = []
        for img, (x0, y0, cw, ch, flip) in zip(images, crops):
            c = img[:, y0:y0 + ch, x0:x0 + cw]
            c = c.flip(-1) if flip else c
            out.append(c.permute(1, 2, 0).contiguous().permute(2, 0, 1) if fmt == "u8_interleaved" else c.contiguous())
        return out

    lib = _lib.load()
    out = torch.empty((B, 3, S, S), device=DEV, dtype=torch.float32)
    stream = lambda: torch.cuda.current_stream(DEV).cuda_stream                            # noqa: E731

    def entries(images, wins):
        """(windowed, existing): the two C entries on prepared descriptor arrays - the launches alone, no Python checks, no allocation."""
        _, ptrs, hs, ws, code, _ = ops.image_list_args(images)
        tail = (B, 3, 0.5, 0.5, S, S, out.data_ptr())
        if code in (ops.IMG_U8, ops.IMG_U8_HWC):
            inter = int(code == ops.IMG_U8_HWC)
            return (lambda: _lib.check(lib.ldit_preprocess_win_u8(ptrs, hs, ws, wins, inter, *tail, stream())),
                    lambda: _lib.check(lib.ldit_preprocess_u8(ptrs, hs, ws, inter, *tail, stream())))
        new, old = ((lib.ldit_preprocess_win_f16, lib.ldit_preprocess_f16) if code == ops.IMG_F16 else
                    (lib.ldit_preprocess_win_f32, lib.ldit_preprocess_f32))
        return (lambda: _lib.check(new(ptrs, hs, ws, wins, *tail, stream())), lambda: _lib.check(old(ptrs, hs, ws, *tail, stream())))

    whole_c, crops_c = ops.window_args(whole, B, sizes), ops.window_args(crops, B, sizes)
    ms = {}
    for fmt, images in lists.items():
        assert torch.equal(ops.preprocess(images, size=S, windows=whole), ops.preprocess(images, size=S))
        assert torch.equal(ops.preprocess(images, size=S, windows=crops), ops.preprocess(copies(images, fmt), size=S))
        win_whole, old_whole = entries(images, whole_c)
        win_crops, _ = entries(images, crops_c)
        ms[fmt] = {
            "a/whole_pages, C entries on prepared descriptors": alternate((("windowed_entry", win_whole), ("existing_entry", old_whole)),
                                                                          a.runs, a.warmup, a.inner),
            "a/crop_windows against whole pages, C entries": alternate((("windowed_entry_on_crops", win_crops), ("existing_entry_on_whole_pages", old_whole)),
                                                                       a.runs, a.warmup, a.inner),
            "a/whole_pages": alternate((("windowed_transform", lambda: ops.preprocess(images, size=S, windows=whole)),
                                        ("existing_transform", lambda: ops.preprocess(images, size=S))), a.runs, a.warmup, a.inner),
            "b/crop_and_flip": alternate((("windowed_transform", lambda: ops.preprocess(images, size=S, windows=crops)),
                                          ("torch_copies_then_existing_transform", lambda: ops.preprocess(copies(images, fmt), size=S))),
                                         a.runs, a.warmup, a.inner),
        }

    # (c) the targets: G random boxes per page, some outside their window
    G = a.boxes
    x = np.sort(rng.uniform(0, w, (B, G, 2)), axis=2)
    y = np.sort(rng.uniform(0, h, (B, G, 2)), axis=2)
    gt_boxes = torch.from_numpy(np.stack([x[..., 0], y[..., 0], x[..., 1], y[..., 1]], axis=-1).astype(np.float32)).to(DEV)
    gt_labels = torch.from_numpy(rng.integers(1, 6, (B, G)).astype(np.int32)).to(DEV)
    gt_count = torch.from_numpy(rng.integers(G // 2, G + 1, B).astype(np.int32)).to(DEV)
    ob, ol, oc = ops.augment_targets(gt_boxes, gt_labels, gt_count, crops, (S, S))
    tb, tl, tc = torch_augment_targets(gt_boxes, gt_labels, gt_count, crops, (S, S), 0.3, 1.0)
    agree = bool(torch.equal(oc, tc) and torch.equal(ol, tl) and torch.allclose(ob, tb, rtol=1e-5, atol=1e-4))
    ms["c/targets"] = alternate((("augment_targets_one_launch", lambda: ops.augment_targets(gt_boxes, gt_labels, gt_count, crops, (S, S))),
                                 ("torch_boolean_indexing", lambda: torch_augment_targets(gt_boxes, gt_labels, gt_count, crops, (S, S), 0.3, 1.0))),
                                a.runs, a.warmup, 1)
    kept = int(oc.sum())
    result = {
        "note": "one run's numbers on one device, every pair timed alternately in one process; no gate on any of them",
        "workload": {"pages": B, "page": [h, w], "target": [S, S], "boxes_per_page": G, "boxes_kept": kept, "boxes_valid": int(gt_count.sum()),
                     "mean_window_share_of_page": round(float(np.mean([cw * ch / (h * w) for _, _, cw, ch, _ in crops])), 3),
                     "flipped": int(sum(f for *_, f in crops))},
        "runs": a.runs, "warmup": a.warmup, "inner_calls_per_window": {"a": a.inner, "b": a.inner, "c": 1},
        "order": "alternating, one window of each of a pair in turn, one process",
        "timer": "HIP events around each window, host work of the calls included (descriptor checks, output allocation, the torch copies)",
        "ms": ms,
        "agreement": {"windowed == existing on whole pages": True, "windowed == existing on torch copies": True,
                      "augment_targets vs torch version (counts, labels equal; boxes allclose)": agree},
        "device": torch.cuda.get_device_name(DEV), "repeats": "one run",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
