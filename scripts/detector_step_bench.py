#!/usr/bin/env python3
"""Time of the detector's optimizer step (csrc/optim_multi.hip through DetectorTrainStep.apply(): non-finite check, state machine,
one AdamW over every parameter) against torch.optim.AdamW(foreach=True) + torch.amp.GradScaler (unscale_, step, update) on the same
parameters and the same gradients, on the same box.  The gradients come from one losses() + backward() of the detector on two
synthetic images; both sides then update a model of their own.  HIP events around each call, median of --runs after --warmup, as
scripts/roi_bench.py.  The loss scale is 1 on both sides, so the repeated in-place unscale of GradScaler leaves its gradients as they are.
Writes one JSON object (--out, default profiles/detector_step_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import config as cfgs, synth  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel  # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="vit_base", choices=["vit_micro", "vit_tiny", "vit_base"])
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "detector_step_bench.json"))
args = ap.parse_args()

dev = "cuda:0"
cfg = getattr(cfgs, args.config)()
cfg.drop_path_rate = 0.0


def build():
    torch.manual_seed(0)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    return model.to(dev).train()


images = [torch.from_numpy(synth.synth_images(1, 224, 224, seed=21 + i, kind="uniform")[0]).to(dev) for i in range(2)]
targets = [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [100.0, 30.0, 190.0, 110.0]], device=dev), "labels": torch.tensor([1, 3], device=dev)},
           {"boxes": torch.tensor([[30.0, 40.0, 200.0, 180.0]], device=dev), "labels": torch.tensor([2], device=dev)}]


def with_grads(model):
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    sum(model.losses(images, targets, generator=gen).values()).backward()
    return model


ours, theirs = with_grads(build()), with_grads(build())
step = DetectorTrainStep(ours, lr=1e-4, weight_decay=0.01, loss_scaling=False)
with_grad = [p for p in theirs.parameters() if p.grad is not None]
opt = torch.optim.AdamW(with_grad, lr=1e-4, weight_decay=0.01, foreach=True)
scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)
scaler.scale(torch.zeros((), device=dev))                      # GradScaler makes its scale tensor on first use


def torch_step():
    scaler.step(opt)                                           # unscale_ (found_inf per device), the host reads found_inf, AdamW
    scaler.update()


def fused_step():
    step.apply()


ms = {}
for name, fn in (("detector_train_step_apply", fused_step), ("torch_adamw_foreach_grad_scaler", torch_step)):
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

params, grads, _, _, _, _, _ = step._segments()
res = {
    "workload": {"config": args.config, "tensors_with_gradient": len(with_grad), "elements": int(sum(p.numel() for p in with_grad)),
                 "segments": len(params), "launches_per_apply": 1 + 2 * -(-len(params) // 64), "weight_decay": 0.01, "loss_scale": 1.0},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call, host work of the call included",
    "ms": ms,
    "steps_taken": {"fused": step.steps, "torch": int(opt.state[with_grad[0]]["step"])},
    "device": torch.cuda.get_device_name(0),
}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
