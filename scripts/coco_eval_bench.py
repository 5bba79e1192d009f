#!/usr/bin/env python3
"""Time of the on-device COCO box evaluation (csrc/coco_eval.hip through CocoBoxEvaluator) on synthetic detections at validation-set
scale: --images images (default 11 000) x 100 detection slots, K = 5 categories, fed in batches of --batch.  Two figures: every
update() of one pass over the data in total, and compute() (keys, torch.sort, accumulation, the 12 means).  HIP events around each,
host work included, median of --runs after --warmup, as scripts/roi_bench.py.  pycocotools is timed on the same data only where it
happens to be importable (loadRes + evaluate + accumulate; the per-box host copies and the JSON file of the reference's loop are not
included).  Writes one JSON object (--out, default profiles/coco_eval_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import CocoBoxEvaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=11000)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coco_eval_bench.json"))
args = ap.parse_args()

dev, N, D, G, K = "cuda:0", args.images, 100, 32, 5
rng = np.random.RandomState(0)


def rand_boxes(*shape):
    side = np.exp(rng.uniform(np.log(8.0), np.log(300.0), size=shape + (2,)))
    xy = rng.uniform(0, 700, size=shape + (2,))
    return np.concatenate([xy, xy + side], axis=-1).astype(np.float32)


# a page has 4 .. 32 GT boxes; 60 % of the 100 detections are jittered copies of one of them with its label, the rest are random
gt_count = rng.randint(4, G + 1, size=N).astype(np.int32)
gt_boxes, gt_labels = rand_boxes(N, G), rng.randint(1, K + 1, size=(N, G)).astype(np.int32)
pick = (rng.uniform(size=(N, D)) * gt_count[:, None]).astype(np.int64)
src = np.take_along_axis(gt_boxes, pick[:, :, None], axis=1)
wh = np.concatenate([src[..., 2:] - src[..., :2]] * 2, axis=-1)
boxes = np.where(rng.uniform(size=(N, D, 1)) < 0.6, src + rng.normal(0, 0.08, size=(N, D, 4)).astype(np.float32) * wh, rand_boxes(N, D))
boxes[..., 2:] = np.maximum(boxes[..., 2:], boxes[..., :2] + 1)
labels = np.take_along_axis(gt_labels, pick, axis=1)
scores = np.sort(rng.uniform(0.05, 1, size=(N, D)).astype(np.float32), axis=1)[:, ::-1].copy()
count = rng.randint(20, D + 1, size=N).astype(np.int32)
host = (boxes.astype(np.float32), scores, labels, count, gt_boxes, gt_labels, gt_count)
data = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
batches = [[x[lo:lo + args.batch] for x in data] for lo in range(0, N, args.batch)]
ev = CocoBoxEvaluator(K, N, max_dets=D, max_gt=G, device=dev)


def update_all():
    ev.reset()
    for b in batches:
        ev.update(*b)


def compute():
    return ev.compute()


ms = {}
for name, fn in (("update_total", update_all), ("compute", compute)):
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

summary = ev.summary()
res = {
    "workload": {"images": N, "detection_slots": D, "detections": int(count.sum()), "gt_boxes": int(gt_count.sum()), "categories": K,
                 "batch": args.batch, "update_launches": len(batches)},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call, host work of the call included",
    "ms": ms, "summary": {k: round(v, 6) for k, v in summary.items()},
    "device": torch.cuda.get_device_name(0),
}

try:                                                             # only where it happens to be installed
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
except ImportError:
    res["pycocotools"] = "not importable on this box: not timed"
else:
    import contextlib
    import io
    anns, dets, aid = [], [], 0
    for i in range(N):
        for g in range(gt_count[i]):
            x1, y1, x2, y2 = (float(v) for v in gt_boxes[i, g])
            aid += 1
            anns.append({"id": aid, "image_id": i, "category_id": int(gt_labels[i, g]), "bbox": [x1, y1, x2 - x1, y2 - y1],
                         "area": (x2 - x1) * (y2 - y1), "iscrowd": 0})
        for d in range(count[i]):
            x1, y1, x2, y2 = (float(v) for v in host[0][i, d])
            dets.append({"image_id": i, "category_id": int(labels[i, d]), "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(scores[i, d])})
    with contextlib.redirect_stdout(io.StringIO()):
        gt = COCO()
        gt.dataset = {"images": [{"id": i} for i in range(N)], "annotations": anns, "categories": [{"id": k} for k in range(1, K + 1)]}
        gt.createIndex()
        t0 = time.perf_counter()
        e = COCOeval(gt, gt.loadRes(dets), iouType="bbox")
        e.evaluate()
        e.accumulate()
        t1 = time.perf_counter()
        e.summarize()
    res["pycocotools"] = {"loadRes_evaluate_accumulate_ms": round((t1 - t0) * 1e3, 1), "runs": 1, "timer": "time.perf_counter",
                          "max_abs_stats_difference": float(np.abs(np.asarray(e.stats) - np.asarray(list(summary.values()))).max())}

print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
