#!/usr/bin/env python3
"""Test-time augmentation, one process on one device, every pair timed alternately (one window of each member in
turn, so clock drift falls on both):

  (a) the merge - ops.tta_merge: pool, class-wise NMS, box voting; three launches, no synchronisation - at B = 64 images, D = 100
      detections per view, V = 2, 4 and 8 views, against the torch composition on the same tensors: per image unmirror / scale, mask
      by the count, ``cat``, the repository's own ``ops.batched_nms`` (torchvision is absent), gather.  The torch side has no voting,
      so the merge is timed without it for the pair and with it on its own;
  (b) ``forward_padded_tta`` on the ViT-B detector at 224 x 224 against the same V views run one by one (``ops.preprocess`` +
      ``forward_padded``, no merge) and against one plain view: the expectation is about V times one view plus the merge.

Nothing here is a gate: the file records what one run showed, with its ranges."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import TestTimeAugment, ops              # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel     # noqa: E402

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


def alternate(group, runs, warmup, inner):
    for _ in range(warmup):
        for _, fn in group:
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _ in group}
    for _ in range(runs):                                    # alternating: one window of each in turn
        for name, fn in group:
            samples[name].append(window(fn, inner))
    return {name: spread(v) for name, v in samples.items()}


def synthetic_views(rng, V, B, D, size=224, objects=12):
    """V views of B pages: each view sees the page's objects a few times with jitter, sorted by score, ragged counts."""
    pages = [(792, 612)] * B
    specs = [(size, size, int(v >= (V + 1) // 2)) for v in range(V)]
    centres = rng.uniform(30, size - 30, (B, objects, 2))
    extent = rng.uniform(16, 60, (B, objects, 2))
    labels_of = rng.integers(1, 6, (B, objects))
    views = []
    for _, _, flip in specs:
        which = rng.integers(0, objects, (B, D))
        c = np.take_along_axis(centres, which[..., None], 1) + rng.normal(0, 2.0, (B, D, 2))
        e = np.take_along_axis(extent, which[..., None], 1) * np.exp(rng.normal(0, 0.1, (B, D, 2)))
        bx = np.clip(np.concatenate([c - e / 2, c + e / 2], -1), 0, size)
        if flip:
            bx = np.stack([size - bx[..., 2], bx[..., 1], size - bx[..., 0], bx[..., 3]], -1)
        scores = -np.sort(-rng.uniform(0.05, 1, (B, D)), axis=1)
        count = rng.integers(D // 2, D + 1, B)
        views.append((torch.from_numpy(bx.astype(np.float32)).to(DEV), torch.from_numpy(scores.astype(np.float32)).to(DEV),
                      torch.from_numpy(np.take_along_axis(labels_of, which, 1).astype(np.int32)).to(DEV),
                      torch.from_numpy(count.astype(np.int32)).to(DEV)))
    return views, specs, pages


def torch_merge(views, specs, pages, nms_thresh, d_out):
    """What a user wrote before: a per-image loop of masking, ``cat`` and ``ops.batched_nms`` (which synchronises)."""
    B, D = views[0][1].shape
    slots = torch.arange(D, device=DEV)
    out = []
    for b, (oh, ow) in enumerate(pages):
        bs, ss, ls = [], [], []
        for (boxes, scores, labels, count), (W, H, flip) in zip(views, specs):
            m = slots < count[b]
            bx = boxes[b][m]                                 # boolean indexing: a synchronisation
            if flip:
                bx = torch.stack([W - bx[:, 2], bx[:, 1], W - bx[:, 0], bx[:, 3]], dim=1)
            rw, rh = float(ow) / float(W), float(oh) / float(H)
            bs.append(bx * torch.tensor([rw, rh, rw, rh], device=DEV))
            ss.append(scores[b][m])
            ls.append(labels[b][m])
        bx, sc, lb = torch.cat(bs), torch.cat(ss), torch.cat(ls)
        keep = ops.batched_nms(bx, sc, lb, nms_thresh)[:d_out]
        out.append((bx[keep], sc[keep], lb[keep]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64, help="images of the merge benchmark")
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--pages", type=int, default=16, help="pages of the model benchmark")
    ap.add_argument("--dtype", default="bf16", help="compute_dtype of the ViT-B detector")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tta_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_bench: no GPU (nothing here can be timed on a CPU)")
    rng = np.random.default_rng(0)
    B, D = a.images, a.dets
    merge, agreement = {}, {}
    for V in (2, 4, 8):
        views, specs, pages = synthetic_views(rng, V, B, D)
        ours = ops.tta_merge(views, specs, pages, 0.5, D, None)
        theirs = torch_merge(views, specs, pages, 0.5, D)
        agreement[f"V={V}"] = all(int(ours[3][b]) == t[1].shape[0] and torch.equal(ours[1][b, :t[1].shape[0]], t[1])
                                  and torch.equal(ours[0][b, :t[1].shape[0]], t[0]) for b, t in enumerate(theirs))
        merge[f"V={V}"] = alternate((("tta_merge_three_launches", lambda: ops.tta_merge(views, specs, pages, 0.5, D, None)),
                                     ("tta_merge_with_voting", lambda: ops.tta_merge(views, specs, pages, 0.5, D, 0.7)),
                                     ("torch_loop_cat_mask_batched_nms", lambda: torch_merge(views, specs, pages, 0.5, D))),
                                    a.runs, a.warmup, a.inner)
        merge[f"V={V}"]["kept_per_image_mean"] = round(float(ours[3].float().mean()), 1)

    torch.manual_seed(0)
    model = LayoutDetectionModel(compute_dtype=a.dtype).to(DEV).eval()
    codes = [torch.from_numpy(rng.integers(0, 256, (792, 612, 3), dtype=np.uint8)).to(DEV).permute(2, 0, 1) for _ in range(a.pages)]
    t = model.model.transform
    mirror = [(0, 0, 612, 792, 1)] * a.pages
    fwd = {}
    with torch.no_grad():
        for name, tta in (("V=2", TestTimeAugment(flip=True)), ("V=4", TestTimeAugment(sizes=[(224, 224), (224, 224)], flip=True))):
            views = tta.views(model)

            def separate():
                for v in views:
                    model.forward_padded(ops.preprocess(codes, size=(v.height, v.width), mean=t.mean, std=t.std, windows=mirror if v.flip else None))

            fwd[name] = alternate((("forward_padded_tta", lambda: model.forward_padded_tta(codes, tta)),
                                   ("views_one_by_one_without_merge", separate),
                                   ("one_plain_view", lambda: model.forward_padded(ops.preprocess(codes, size=(224, 224), mean=t.mean, std=t.std)))),
                                  a.runs, a.warmup, 1)
            fwd[name]["kept_per_image_mean"] = round(float(model.forward_padded_tta(codes, tta)[3].float().mean()), 1)
    result = {
        "note": "one run's numbers on one device, every group timed alternately in one process; no gate on any of them",
        "runs": a.runs, "warmup": a.warmup, "inner_calls_per_window": {"merge": a.inner, "model": 1},
        "order": "alternating, one window of each member of a group in turn, one process",
        "timer": "HIP events around each window, host work of the calls included (argument checks, output allocation, the torch loop's synchronisations)",
        "merge": {"workload": {"images": B, "detections_per_view": D, "page": [792, 612], "view": [224, 224], "nms_thresh": 0.5,
                               "vote_thresh": 0.7, "torch side": "no voting: compare with tta_merge_three_launches"}, "ms": merge,
                  "same kept boxes and scores as the torch loop": agreement},
        "model": {"workload": {"detector": "ViT-B, random weights", "compute_dtype": a.dtype, "pages": a.pages, "page": [792, 612],
                               "format": "uint8 interleaved", "views": "224 x 224, plain then mirrored (V=4: each twice)"}, "ms": fwd},
        "accuracy": "not measured: there are no trained weights",
        "device": torch.cuda.get_device_name(DEV), "repeats": "one run",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
