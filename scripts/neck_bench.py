#!/usr/bin/env python3
"""Time of the detector's neck - the FPN's four 3x3 output convolutions and the RPN head on p2..p5 and pool - at the reference
workload: ViT-B/16, 224x224, bs=64, 256 channels, maps of 56 / 28 / 14 / 7 and the strided 4 x 4 view of the 7 x 7.  The fp32 path
(neck_dtype="f32": the parent's code, still the default) and the bf16 path (neck_dtype="bf16") are timed in this one process, step
by step under the same brackets: every step is bracketed by HIP events on its own (median of --runs after --warmup), as
scripts/roi_bench.py does it.  Steps: the FPN's 3x3 stage on the four merged maps; the RPN head on the five maps; the bf16 path's
pad launches alone; the whole neck from the encoder's taps (laterals, merges, 3x3s, head); forward_padded with the bf16 encoder and
the bf16 box head under both neck settings.  Writes one JSON object (--out, default profiles/neck_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import _lib, config as cfgs, ops, synth  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel  # noqa: E402
from layoutdit_amd.modeling.dit_fpn import _f32c, _fpn_forward  # noqa: E402
from layoutdit_amd.modeling.grad_ops import conv3x3_fwd_bf16  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "neck_bench.json"))
args = ap.parse_args()

dev = "cuda:0"
B = args.batch
cfg = cfgs.vit_base()
torch.manual_seed(0)
model = LayoutDetectionModel(config=cfg, compute_dtype="bf16", head_dtype="bf16")
model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=1))
with torch.no_grad():                                      # the FPN's biases and the RPN head's weights as a trained detector has them: not zero
    for blk in list(model.model.backbone.fpn.inner_blocks) + list(model.model.backbone.fpn.layer_blocks):
        blk[0].bias.normal_(0, 0.1)
    for p in model.model.rpn.head.parameters():
        p.normal_(0, 0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2)
model = model.to(dev).eval()
fpn, head = model.model.backbone, model.model.rpn.head
bb = fpn.backbone
batch = torch.from_numpy(synth.synth_images(B, 224, 224, seed=7)).to(dev)
gh = gw = 224 // cfg.patch_size


def neck(toks, bf16):
    """The not-wants-grad branch of DiTWithFPN.forward behind the encoder, then the RPN head on the five maps."""
    lat = [fpn.fpn.inner_blocks[i][0] for i in range(4)]
    conv = [fpn.fpn.layer_blocks[i][0] for i in range(4)]
    outs, _ = _fpn_forward(bb.scales, gh, gw, toks, [m.weight.detach().reshape(256, bb.hidden_size) for m in lat],
                           [m.bias.detach() for m in lat], [fpn._ohwi_bf16(i) if bf16 else fpn._ohwi(i) for i in range(4)],
                           [m.bias.detach() for m in conv], keep_inner=False)   # a bf16 weight copy selects the bf16 3x3
    maps = [o.permute(0, 3, 1, 2) for o in outs]
    maps.append(maps[3][:, :, ::2, ::2])
    return head(maps)


with torch.no_grad():
    hs = bb.dit(batch, taps=bb.layer_idxs).hidden_states
    toks = [_f32c(hs[i].detach()) for i in bb.layer_idxs]
    lat = [fpn.fpn.inner_blocks[i][0] for i in range(4)]
    conv = [fpn.fpn.layer_blocks[i][0] for i in range(4)]
    cb = [m.bias.detach() for m in conv]
    _, inners = _fpn_forward(bb.scales, gh, gw, toks, [m.weight.detach().reshape(256, bb.hidden_size) for m in lat],
                             [m.bias.detach() for m in lat], [fpn._ohwi(i) for i in range(4)], cb, keep_inner=True)
    w32, w16 = [fpn._ohwi(i) for i in range(4)], [fpn._ohwi_bf16(i) for i in range(4)]
    maps = [ops.conv3x3_nhwc(inners[i], w32[i], cb[i]).permute(0, 3, 1, 2) for i in range(4)]
    maps.append(maps[3][:, :, ::2, ::2])
    nhwc = [m.permute(0, 2, 3, 1).contiguous() for m in maps]                    # what the head's levels pad (pool: a copy, p2..p5: free)

    def set_neck(d):
        model.set_neck_dtype(d)

    def with_neck(d, fn):
        def run():
            set_neck(d)
            return fn()
        return run

    steps = {
        "fpn_conv3x3": lambda: [ops.conv3x3_nhwc(inners[i], w32[i], cb[i]) for i in range(4)],
        "bf16/fpn_conv3x3": lambda: [conv3x3_fwd_bf16(inners[i], w16[i], cb[i], _lib.EPI_F32)[0] for i in range(4)],
        "bf16/fpn_pad_only": lambda: [ops.pad_nhwc_bf16(inners[i]) for i in range(4)],
        "rpn_head": with_neck("f32", lambda: head(maps)),
        "bf16/rpn_head": with_neck("bf16", lambda: head(maps)),
        "bf16/rpn_pad_only": lambda: [ops.pad_nhwc_bf16(x) for x in nhwc],
        "neck_whole": with_neck("f32", lambda: neck(toks, False)),
        "bf16/neck_whole": with_neck("bf16", lambda: neck(toks, True)),
        "forward_padded": with_neck("f32", lambda: model.forward_padded(batch)),
        "bf16/forward_padded": with_neck("bf16", lambda: model.forward_padded(batch)),
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
    set_neck("f32")
    # agreement of the two paths on this input (rel-L2 of the bf16 path against the fp32 one)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())     # noqa: E731
    l32, d32 = neck(toks, False)
    set_neck("bf16")
    l16, d16 = neck(toks, True)
    set_neck("f32")
    agree = {"rpn_logits_rel_l2": rel(l16, l32), "rpn_deltas_rel_l2": rel(d16, d32)}

flops_fpn = sum(2 * B * s * s * 256 * 9 * 256 for s in (56, 28, 14, 7))
flops_rpn = sum(2 * B * s * s * 256 * 9 * 256 for s in (56, 28, 14, 7, 4))
faster = {k: round(ms[k]["median_ms"] / ms["bf16/" + k]["median_ms"], 3) for k in ("fpn_conv3x3", "rpn_head", "neck_whole", "forward_padded")}
res = {
    "note": "one run's numbers on one device; fp32 and bf16 timed in the same process (the fp32 path is the parent commit's code)",
    "workload": {"batch": B, "image": [224, 224], "encoder": "ViT-B/16 bf16", "head_dtype": "bf16", "channels": 256,
                 "maps": [list(m.shape[-2:]) for m in maps], "fpn_3x3_gflop": round(flops_fpn / 1e9, 1),
                 "rpn_3x3_gflop": round(flops_rpn / 1e9, 1)},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each step (allocation of the outputs included)",
    "ms": ms,
    "fp32_over_bf16": faster,
    "tflops": {"fpn_conv3x3": round(flops_fpn / ms["fpn_conv3x3"]["median_ms"] / 1e9, 1),
               "bf16/fpn_conv3x3": round(flops_fpn / ms["bf16/fpn_conv3x3"]["median_ms"] / 1e9, 1)},
    "agreement": agree,
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
