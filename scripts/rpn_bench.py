#!/usr/bin/env python3
"""Time of the padded region-proposal stage (csrc/proposals.hip) at the reference workload: bs=64, 224x224, 5 levels x 3
anchors (9408 + 2352 + 588 + 147 + 48 = 12543 anchors per image), pre / post NMS top-n 1000 / 1000, NMS threshold 0.7.
Each of the three launches is bracketed by HIP events on its own (median of --runs after --warmup); the input is what an RPN
head delivers on smooth feature maps: spatially correlated logits and small deltas, so neighbouring anchors overlap and NMS
has work to do.  Writes one JSON object (--out, default profiles/rpn_bench.json)."""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rpn_bench.json"))
args = ap.parse_args()

dev = "cuda:0"
B, PRE, POST, THR = args.batch, 1000, 1000, 0.7
grids = [(56, 56), (28, 28), (14, 14), (7, 7), (4, 4)]
gen = AnchorGenerator(sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5)
rpn = RegionProposalNetwork(gen, RPNHead(256, 3), PRE, POST, THR).to(dev).eval()
anchors, sizes = gen(grids, (224, 224), dev)
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


def stage():
    idx = ops.rpn_topk(logits, sizes, PRE)
    boxes, scores = ops.rpn_decode(logits, deltas, anchors, idx, (224, 224), 1e-3, 0.0)
    return idx, boxes, scores, ops.batched_nms_padded(boxes, scores, groups, THR, POST)


idx, boxes, scores, (keep, count, _, _) = stage()
steps = {
    "rpn_topk": lambda: ops.rpn_topk(logits, sizes, PRE),
    "rpn_decode": lambda: ops.rpn_decode(logits, deltas, anchors, idx, (224, 224), 1e-3, 0.0),
    "nms_batched": lambda: ops.batched_nms_padded(boxes, scores, groups, THR, POST),
    "stage": stage,
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
    "workload": {"batch": B, "image": [224, 224], "levels": list(sizes), "anchors_per_image": ntot, "pre_nms_top_n": PRE,
                 "post_nms_top_n": POST, "nms_thresh": THR, "candidates_per_image": int(idx.shape[1])},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call (allocation of the outputs included)",
    "ms": ms,
    "kept_per_image": {"min": int(cnt.min()), "median": float(np.median(cnt)), "max": int(cnt.max())},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
