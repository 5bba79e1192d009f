#!/usr/bin/env python3
"""Time of the padded region-proposal stage (csrc/proposals.hip) at the reference workload: bs=64, 224x224, 5 levels x 3
anchors (9408 + 2352 + 588 + 147 + 48 = 12543 anchors per image), pre / post NMS top-n 1000 / 1000, NMS threshold 0.7.
Each of the three launches is bracketed by HIP events on its own (median of --runs after --warmup); the input is what an RPN
head delivers on smooth feature maps: spatially correlated logits and small deltas, so neighbouring anchors overlap and NMS
has work to do.  ``--size H W`` moves the geometry off 224 x 224 (the five levels at strides 4, 8, 16, 32 and the pooled one): at
512 x 512 (p2 = 49 152 anchors, 65 472 per image) and 640 x 640 (76 800 / 102 300) ``rpn_topk`` and ``rpn_targets`` run their
chunked kernels, one workgroup per level or image - the two figures nobody has recorded yet.  ``rpn_targets`` (16 GT boxes per
image, sampler (256, 0.5)) is timed at every size.  Writes one JSON object (--out, default profiles/rpn_bench.json, or
profiles/rpn_bench_HxW.json with --size)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import ops  # noqa: E402
from layoutdit_amd.modeling import AnchorGenerator, RegionProposalNetwork, RPNHead  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--size", type=int, nargs=2, default=[224, 224], metavar=("H", "W"), help="image size, multiples of 32")
ap.add_argument("--out", default=None)
args = ap.parse_args()
H, W = args.size
if H % 32 or W % 32 or H <= 0 or W <= 0:
    ap.error("--size: H and W must be positive multiples of 32")
if args.out is None:
    name = "rpn_bench.json" if (H, W) == (224, 224) else f"rpn_bench_{H}x{W}.json"
    args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", name)

dev = "cuda:0"
B, PRE, POST, THR = args.batch, 1000, 1000, 0.7
grids = [(H // 4, W // 4), (H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32), ((H // 32 + 1) // 2, (W // 32 + 1) // 2)]
gen = AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)
rpn = RegionProposalNetwork(gen, RPNHead(256, 3), PRE, POST, THR).to(dev).eval()
anchors, sizes = gen(grids, (H, W), dev)
ntot = sum(sizes)

rng = np.random.RandomState(0)
parts = []
for gh, gw in grids:                                      # smooth objectness per level: a coarse random field, upsampled, + noise
    coarse = torch.from_numpy(rng.normal(0, 2.0, size=(B, 3, max(gh // 4, 1), max(gw // 4, 1))).astype(np.float32))
    field = torch.nn.functional.interpolate(coarse, size=(gh, gw), mode="bilinear", align_corners=False)
    field = field + torch.from_numpy(rng.normal(0, 0.3, size=(B, 3, gh, gw)).astype(np.float32))
    parts.append(field.permute(0, 2, 3, 1).reshape(B, -1))
logits = torch.cat(parts, dim=1).contiguous().to(dev)
deltas = torch.from_numpy(rng.normal(0, 0.15, size=(B, ntot, 4)).astype(np.float32)).to(dev)
groups = rpn._level_ids(sizes, B, dev)
G = 16                                                    # GT boxes per image for rpn_targets: anywhere in the image, 16 px to half of it
wh = rng.uniform(16.0, 0.5 * min(H, W), size=(B, G, 2))
xy = rng.uniform(0.0, 1.0, size=(B, G, 2)) * (np.asarray([W, H]) - wh)
gt_boxes = torch.from_numpy(np.concatenate([xy, xy + wh], axis=2).astype(np.float32)).to(dev)
gt_count = torch.full((B,), G, dtype=torch.int32, device=dev)
keys = torch.randint(0, 2 ** 31 - 1, (B, ntot), device=dev, dtype=torch.int32)


def stage():
    idx = ops.rpn_topk(logits, sizes, PRE)
    boxes, scores = ops.rpn_decode(logits, deltas, anchors, idx, (H, W), 1e-3, 0.0)
    return idx, boxes, scores, ops.batched_nms_padded(boxes, scores, groups, THR, POST)


idx, boxes, scores, (keep, count, _, _) = stage()
steps = {
    "rpn_topk": lambda: ops.rpn_topk(logits, sizes, PRE),
    "rpn_decode": lambda: ops.rpn_decode(logits, deltas, anchors, idx, (H, W), 1e-3, 0.0),
    "nms_batched": lambda: ops.batched_nms_padded(boxes, scores, groups, THR, POST),
    "stage": stage,
    "rpn_targets": lambda: ops.rpn_targets(anchors, gt_boxes, gt_count, keys),
}
ms = {}
for name, fn in steps.items():
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b))
    ms[name] = {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

cnt = count.cpu().numpy()
res = {
    "workload": {"batch": B, "image": [H, W], "levels": list(sizes), "anchors_per_image": ntot, "pre_nms_top_n": PRE,
                 "post_nms_top_n": POST, "nms_thresh": THR, "candidates_per_image": int(idx.shape[1]), "gt_per_image": G,
                 "chunked_topk": max(sizes) > ops.RPN_SORT_SLOTS, "chunked_targets": ntot > ops.RPN_SORT_SLOTS},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call (allocation of the outputs included)",
    "ms": ms,
    "kept_per_image": {"min": int(cnt.min()), "median": float(np.median(cnt)), "max": int(cnt.max())},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
