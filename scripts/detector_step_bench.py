#!/usr/bin/env python3
"""Time of the detector's optimizer step (csrc/optim_multi.hip through DetectorTrainStep.apply(): non-finite check, state machine,
one AdamW over every parameter) against torch.optim.AdamW(foreach=True) + torch.amp.GradScaler (unscale_, step, update) on the same
parameters and the same gradients, on the same box.  The gradients come from one losses() + backward() of the detector on two
synthetic images; both sides then update a model of their own.  HIP events around each call, median of --runs after --warmup, as
scripts/roi_bench.py.  The loss scale is 1 on both sides, so the repeated in-place unscale of GradScaler leaves its gradients as they are.
With --clip the same four-way comparison with global-norm clipping and parameter groups: (a) the default
apply(), (b) max_grad_norm set, one group, (c) detector_param_groups(layer_decay=0.75) + clipping, (d) clip_grad_norm_(foreach=True)
+ AdamW with the same groups + GradScaler; (b) and (c) are reported beside (d) as ratios of this one run.
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
from layoutdit_amd import training  # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="vit_base", choices=["vit_micro", "vit_tiny", "vit_base"])
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--clip", action="store_true", help="also time clipping and parameter groups against clip_grad_norm_ + AdamW(groups)")
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


cases = [("detector_train_step_apply", fused_step), ("torch_adamw_foreach_grad_scaler", torch_step)]
MAX_NORM, LAYER_DECAY = 1.0, 0.75
if args.clip:
    m_clip, m_groups, m_torch = with_grads(build()), with_grads(build()), with_grads(build())
    step_clip = DetectorTrainStep(m_clip, lr=1e-4, weight_decay=0.01, loss_scaling=False, max_grad_norm=MAX_NORM)
    step_groups = DetectorTrainStep(m_groups, lr=1e-4, weight_decay=0.01, loss_scaling=False, max_grad_norm=MAX_NORM,
                                    param_groups=training.detector_param_groups(m_groups, layer_decay=LAYER_DECAY, weight_decay=0.01))
    named = dict(m_torch.named_parameters())
    torch_groups = [{"params": [named[n] for n in g["params"] if named[n].grad is not None], "lr": 1e-4 * g["lr_scale"], "weight_decay": g["weight_decay"]}
                    for g in training.detector_param_groups(m_torch, layer_decay=LAYER_DECAY, weight_decay=0.01)]
    torch_groups = [g for g in torch_groups if g["params"]]
    clipped = [p for g in torch_groups for p in g["params"]]
    opt_groups = torch.optim.AdamW(torch_groups, lr=1e-4, foreach=True)
    scaler_groups = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)
    scaler_groups.scale(torch.zeros((), device=dev))

    def torch_clip_step():
        scaler_groups.unscale_(opt_groups)
        torch.nn.utils.clip_grad_norm_(clipped, MAX_NORM, foreach=True)
        scaler_groups.step(opt_groups)
        scaler_groups.update()

    # the gradients are clipped in place on the torch side, so after the first call its clip is inactive: the same launches run
    cases += [("detector_train_step_apply_clip", step_clip.apply), ("detector_train_step_apply_clip_groups", step_groups.apply),
              ("torch_clip_grad_norm_adamw_groups_grad_scaler", torch_clip_step)]

ms = {}
for name, fn in cases:
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

params = step._segments()[0]
res = {
    "workload": {"config": args.config, "tensors_with_gradient": len(with_grad), "elements": int(sum(p.numel() for p in with_grad)),
                 "segments": len(params), "launches_per_apply": 1 + 2 * -(-len(params) // 64), "weight_decay": 0.01, "loss_scale": 1.0},
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call, host work of the call included",
    "ms": ms,
    "steps_taken": {"fused": step.steps, "torch": int(opt.state[with_grad[0]]["step"])},
    "device": torch.cuda.get_device_name(0),
}
if args.clip:
    ref = ms["torch_clip_grad_norm_adamw_groups_grad_scaler"]["median_ms"]
    res["clip"] = {"max_grad_norm": MAX_NORM, "layer_decay": LAYER_DECAY,
                   "segments_clip": len(step_clip._segments()[0]), "segments_clip_groups": len(step_groups._segments()[0]),
                   "torch_groups": len(torch_groups),
                   "torch_over_clip": round(ref / ms["detector_train_step_apply_clip"]["median_ms"], 2),
                   "torch_over_clip_groups": round(ref / ms["detector_train_step_apply_clip_groups"]["median_ms"], 2)}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
