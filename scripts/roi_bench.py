#!/usr/bin/env python3
"""Time of the padded box head (csrc/roi_heads.hip and the head's GEMMs) at the reference workload: bs=64, 224x224, 1000 proposals
per image, five maps of 256 channels (56 / 28 / 14 / 7 and the strided 4 x 4 view of the 7 x 7), 5 + 1 classes, score threshold
0.05, NMS threshold 0.5, 100 detections.  Every launch is bracketed by HIP events on its own (median of --runs after --warmup).
In the same file, on the same box: a plain-torch restatement of the RoIAlign (per level F.grid_sample on the level's map plus a
2 x 2 mean) as the comparison - it is what one would write without the kernel, not torchvision's own implementation.
--head-dtype f32 | bf16 | both (default): the fp32 head (fp32 pooled rows, fp32 GEMMs, relu_ launches), the bf16 head (bf16 pooled
rows, bf16 GEMMs with the ReLU epilogue, fp32 predictor output) or both in this one process, step by step under the same brackets.
Writes one JSON object (--out, default profiles/roi_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import _lib, ops  # noqa: E402
from layoutdit_amd.modeling import FastRCNNPredictor, TwoMLPHead  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--proposals", type=int, default=1000)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--head-dtype", choices=["f32", "bf16", "both"], default="both")
ap.add_argument("--no-torch-roi-align", action="store_true", help="skip the plain-torch RoIAlign comparison")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "roi_bench.json"))
args = ap.parse_args()

dev = "cuda:0"
B, R, NC, P, S = args.batch, args.proposals, 6, 7, 2
rng = np.random.RandomState(0)
torch.manual_seed(0)
feats = [torch.randn(B, g, g, 256, device=dev).permute(0, 3, 1, 2) for g in (56, 28, 14, 7)]
feats.append(feats[3][:, :, ::2, ::2])
# proposals as an RPN leaves them: log-uniform sizes from 8 to 224 pixels, clipped to the image, a ragged count per image
ctr = rng.uniform(0, 224, size=(B, R, 2))
size = np.exp(rng.uniform(np.log(8.0), np.log(224.0), size=(B, R, 2)))
boxes = torch.from_numpy(np.clip(np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=-1), 0, 224).astype(np.float32)).to(dev)
count = torch.from_numpy(rng.randint(R // 2, R + 1, size=B).astype(np.int32)).to(dev)
head, pred = TwoMLPHead(256 * P * P, 1024).to(dev).eval(), FastRCNNPredictor(1024, NC).to(dev).eval()
with torch.no_grad():
    pred.cls_score.bias[0] = 3.0                          # most candidates are background, as behind a trained head


def torch_roi_align(chunk=8):
    """The same function in plain torch, without a synchronisation: levels with torchvision's formula; per level one F.grid_sample
    per chunk of images over ALL proposal rows (the rows of other levels are computed and discarded by a torch.where - gathering only
    a level's rows needs a nonzero, i.e. the host round trip this stage exists to avoid), then the 2 x 2 mean.  Samples outside
    [-1, h] are zeroed and the rest clamped to [0, h - 1] first (roi_align's border rule), so align_corners=True sampling reproduces
    the kernel's values.  Returns [B R, P, P, C] like the kernel."""
    scales = ops.infer_scales(feats, (224, 224))
    valid = torch.arange(R, device=dev)[None, :] < count[:, None]
    area = (boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1])
    k = torch.floor(4 + torch.log2(torch.sqrt(area) / 224) + 1e-6).clamp(2, 6).long() - 2
    k = torch.where(valid, k, torch.full_like(k, -1))
    out = torch.zeros(B, 256, R, P, P, device=dev)
    steps_p = (torch.arange(P * S, device=dev) // S).float()
    steps_i = ((torch.arange(P * S, device=dev) % S).float() + 0.5) / S
    for l, (f, s) in enumerate(zip(feats, scales)):
        bx = boxes * s
        h, w = f.shape[-2:]
        coords, inside = [], []
        for lo, hi, n in ((bx[..., 0], bx[..., 2], w), (bx[..., 1], bx[..., 3], h)):
            bin_ = (hi - lo).clamp(min=1.0) / P
            c = lo[..., None] + steps_p * bin_[..., None] + steps_i * bin_[..., None]              # [B, R, P S]
            inside.append((c >= -1) & (c <= n))
            coords.append(2 * c.clamp(0, n - 1) / max(n - 1, 1) - 1)
        for i in range(0, B, chunk):
            j = min(i + chunk, B)
            gx = coords[0][i:j, :, None, :].expand(-1, -1, P * S, -1)
            gy = coords[1][i:j, :, :, None].expand(-1, -1, -1, P * S)
            grid = torch.stack([gx, gy], dim=-1).reshape(j - i, R * P * S, P * S, 2)
            mask = (inside[1][i:j, :, :, None] & inside[0][i:j, :, None, :]).float()
            val = F.grid_sample(f[i:j], grid, mode="bilinear", padding_mode="border", align_corners=True)
            val = val.reshape(j - i, 256, R, P * S, P * S) * mask[:, None]
            val = val.reshape(j - i, 256, R, P, S, P, S).mean(dim=(4, 6))
            out[i:j] = torch.where((k[i:j] == l)[:, None, :, None, None], val, out[i:j])
    return out.permute(0, 2, 3, 4, 1).reshape(B * R, P, P, 256)


do32, do16 = args.head_dtype in ("f32", "both"), args.head_dtype in ("bf16", "both")
with torch.no_grad():
    steps, agree, pooled_bytes = {}, None, {}
    b6, b7 = head.fc6.bias.detach(), head.fc7.bias.detach()
    if do32:
        pooled = ops.roi_align_levels(feats, boxes, count, (224, 224))
        pooled_bytes["f32"] = int(pooled.numel() * 4)
        if not args.no_torch_roi_align:
            agree = float((pooled - torch_roi_align()).abs().max())
        w6 = head.fc6_weight_hwc(256, P, P)
        x6 = ops.linear(pooled.reshape(B * R, -1), w6, b6)
        x7 = head(pooled)
        y = pred.forward_stacked(x7)
        cand = ops.box_postprocess(y, boxes, count, (224, 224), NC)
        det = ops.box_detections_padded(y, boxes, count, (224, 224), NC)

        def whole():
            return ops.box_detections_padded(pred.forward_stacked(head(ops.roi_align_levels(feats, boxes, count, (224, 224)))), boxes, count,
                                             (224, 224), NC)

        steps.update({
            "roi_align_levels": lambda: ops.roi_align_levels(feats, boxes, count, (224, 224)),
            "fc6": lambda: ops.linear(pooled.reshape(B * R, -1), w6, b6),
            "relu_": lambda: torch.relu_(x6),
            "fc7": lambda: ops.linear(x6, head.fc7.weight.detach(), b7),
            "predictor": lambda: pred.forward_stacked(x7),
            "box_postprocess": lambda: ops.box_postprocess(y, boxes, count, (224, 224), NC),
            "nms_batched": lambda: ops.batched_nms_padded(cand[0], cand[1], cand[2], 0.5, 100),
            "box_head_whole": whole,
        })
    if do16:
        pooled16 = ops.roi_align_levels(feats, boxes, count, (224, 224), out_dtype=torch.bfloat16)
        pooled_bytes["bf16"] = int(pooled16.numel() * 2)
        w6h, w7h = head.operands_bf16(256, P, P)
        x6h = ops.linear_bf16(pooled16.reshape(B * R, -1), w6h, b6, _lib.EPI_BIAS_RELU)
        x7h = head.forward_bf16(pooled16)
        yh = pred.forward_stacked_bf16(x7h)
        candh = ops.box_postprocess(yh, boxes, count, (224, 224), NC)
        deth = ops.box_detections_padded(yh, boxes, count, (224, 224), NC)

        def whole_bf16():
            rows = ops.roi_align_levels(feats, boxes, count, (224, 224), out_dtype=torch.bfloat16)
            return ops.box_detections_padded(pred.forward_stacked_bf16(head.forward_bf16(rows)), boxes, count, (224, 224), NC)

        steps.update({
            "bf16/roi_align_levels": lambda: ops.roi_align_levels(feats, boxes, count, (224, 224), out_dtype=torch.bfloat16),
            "bf16/fc6_relu": lambda: ops.linear_bf16(pooled16.reshape(B * R, -1), w6h, b6, _lib.EPI_BIAS_RELU),
            "bf16/fc7_relu": lambda: ops.linear_bf16(x6h, w7h, b7, _lib.EPI_BIAS_RELU),
            "bf16/predictor": lambda: pred.forward_stacked_bf16(x7h),
            "bf16/box_postprocess": lambda: ops.box_postprocess(yh, boxes, count, (224, 224), NC),
            "bf16/nms_batched": lambda: ops.batched_nms_padded(candh[0], candh[1], candh[2], 0.5, 100),
            "bf16/box_head_whole": whole_bf16,
        })
    if do32 and not args.no_torch_roi_align:
        steps["torch_roi_align"] = torch_roi_align
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


def _kept(d):
    k = d[3].cpu().numpy()
    return {"min": int(k.min()), "median": float(np.median(k)), "max": int(k.max())}


res = {
    "workload": {"batch": B, "image": [224, 224], "proposals_per_image": R, "valid_proposals": int(count.sum()), "channels": 256,
                 "maps": [list(f.shape[-2:]) for f in feats], "output_size": P, "sampling_ratio": S, "num_classes": NC,
                 "pooled_bytes": pooled_bytes, "score_thresh": 0.05, "nms_thresh": 0.5, "detections_per_img": 100},
    "head_dtype": args.head_dtype,
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call (allocation of the outputs included)",
    "ms": ms,
    "torch_roi_align_max_abs_diff": agree,
    "detections_per_image": {k: _kept(d) for k, d in (("f32", det if do32 else None), ("bf16", deth if do16 else None)) if d is not None},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
