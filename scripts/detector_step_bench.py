#!/usr/bin/env python3
"""Time of the detector's optimizer step (csrc/optim_multi.hip through DetectorTrainStep.apply(): non-finite check, state machine,
one AdamW over every parameter) against torch.optim.AdamW(foreach=True) + torch.amp.GradScaler (unscale_, step, update) on the same
parameters and the same gradients, on the same box.  The gradients come from one losses() + backward() of the detector on two
synthetic images; both sides then update a model of their own.  HIP events around each call, median of --runs after --warmup, as
scripts/roi_bench.py.  The loss scale is 1 on both sides, so the repeated in-place unscale of GradScaler leaves its gradients as they are.
With --clip the same four-way comparison with global-norm clipping and parameter groups: (a) the default
apply(), (b) max_grad_norm set, one group, (c) detector_param_groups(layer_decay=0.75) + clipping, (d) clip_grad_norm_(foreach=True)
+ AdamW with the same groups + GradScaler; (b) and (c) are reported beside (d) as ratios of this one run.
With --qat nothing of the above runs; instead, alternating in one process: apply() of the detector on the bf16
encoder against apply() of the detector on the quantisation-aware mxfp8 encoder (the same launches plus ldit_requant_train_mirror),
and that one launch alone against ldit_pack_train on the same master (the cast pass plus one launch per layer: what mark_dirty()
would cost at the next forward), --inner calls per timed window; the file is profiles/detector_step_bench_qat.json.
With --ema nothing of the above runs either; instead, alternating in one process on the detector with the bf16
encoder: apply() without a moving average, apply() with ema_decay (the same launches, the update's one reading and writing a shadow
element as well), and apply() without followed by torch._foreach_lerp_ over the same tensors; then ops.swap_multi (weights <-> shadows,
one launch) against three torch._foreach_copy_ through a temporary, --inner calls per timed window; profiles/detector_step_bench_ema.json.
Writes one JSON object (--out, default profiles/detector_step_bench.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layoutdit_amd import _lib, config as cfgs, ops, synth  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel  # noqa: E402
from layoutdit_amd import training  # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="vit_base", choices=["vit_micro", "vit_tiny", "vit_base"])
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--clip", action="store_true", help="also time clipping and parameter groups against clip_grad_norm_ + AdamW(groups)")
ap.add_argument("--qat", action="store_true", help="time the qat detector's apply() beside the bf16-encoder detector's, and the re-quantise launch beside ldit_pack_train")
ap.add_argument("--ema", action="store_true", help="time apply() with the moving average beside apply() and apply() + torch._foreach_lerp_, and the swap launch")
ap.add_argument("--inner", type=int, default=20, help="--qat / --ema: calls of the launch / the pack / the exchange per timed window")
ap.add_argument("--commit", default=None, help="--ema: recorded as the commit the tree was measured at")
ap.add_argument("--out", default=None)
args = ap.parse_args()
args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "detector_step_bench_qat.json" if args.qat else "detector_step_bench_ema.json" if args.ema else
                                    "detector_step_bench.json")

dev = "cuda:0"
cfg = getattr(cfgs, args.config)()
cfg.drop_path_rate = 0.0


def build(compute_dtype="f32"):
    torch.manual_seed(0)
    model = LayoutDetectionModel(config=cfg, compute_dtype=compute_dtype, qat=compute_dtype == "mxfp8")
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


def window(fn, inner=1):
    """Milliseconds per call of `inner` back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def spread(v, digits=4):
    return {"median_ms": round(statistics.median(v), digits), "min_ms": round(min(v), digits), "max_ms": round(max(v), digits)}


if args.qat:
    m_bf16, m_qat = with_grads(build("bf16")), with_grads(build("mxfp8"))
    s_bf16 = DetectorTrainStep(m_bf16, lr=1e-6, weight_decay=0.01, loss_scaling=False)
    s_qat = DetectorTrainStep(m_qat, lr=1e-6, weight_decay=0.01, loss_scaling=False)
    st = m_qat.model.backbone.backbone.dit._flat_state
    pairs = {"apply": (("bf16_encoder", s_bf16.apply, 1), ("qat_mxfp8_encoder", s_qat.apply, 1)),
             "requantise": (("requant_train_mirror_one_launch", lambda: ops.requant_train_mirror(st), args.inner),
                            ("pack_train_cast_plus_launch_per_layer", lambda: st.repack(force=True), args.inner))}
    ms = {}
    for what, pair in pairs.items():
        for _ in range(args.warmup):
            for _, fn, _ in pair:
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _, _ in pair}
        for _ in range(args.runs):                             # alternating: one window of each in turn
            for name, fn, inner in pair:
                samples[name].append(window(fn, inner))
        ms[what] = {name: spread(v, 5) for name, v in samples.items()}
    L, Cc, F = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size
    matrix = L * (4 * Cc * Cc + 2 * Cc * F)
    a, q = ms["apply"]["bf16_encoder"], ms["apply"]["qat_mxfp8_encoder"]
    r, p = ms["requantise"]["requant_train_mirror_one_launch"], ms["requantise"]["pack_train_cast_plus_launch_per_layer"]
    res = {
        "workload": {"config": args.config, "encoder_elements": int(st.numel), "matrix_elements": int(matrix),
                     "requantise_bytes": {"read": 4 * matrix, "written": matrix + matrix // 32 + 2 * matrix},
                     "mirror_bytes": int(_lib.load().ldit_train_mirror_bytes(ctypes.byref(st.lcfg))),
                     "segments": {"bf16_encoder": len(s_bf16._segments()[0]), "qat_mxfp8_encoder": len(s_qat._segments()[0])},
                     "launches_per_apply": {"bf16_encoder": 1 + 2 * -(-len(s_bf16._segments()[0]) // 64),
                                            "qat_mxfp8_encoder": 2 + 2 * -(-len(s_qat._segments()[0]) // 64)},
                     "launches": {"requant_train_mirror": 1, "pack_train": 1 + L}, "weight_decay": 0.01, "loss_scale": 1.0},
        "runs": args.runs, "warmup": args.warmup, "inner_calls_per_window": args.inner,
        "order": "alternating, one window of each of a pair in turn, one process",
        "timer": "HIP events around each window, host work of the calls included",
        "ms": ms,
        "apply_difference": {"median_ms": round(q["median_ms"] - a["median_ms"], 5), "ratio": round(q["median_ms"] / a["median_ms"], 3),
                             "separated": bool(a["max_ms"] < q["min_ms"] or q["max_ms"] < a["min_ms"])},
        "one_launch_over_pack_train": {"ratio": round(r["median_ms"] / p["median_ms"], 3),
                                       "separated": bool(r["max_ms"] < p["min_ms"] or p["max_ms"] < r["min_ms"])},
        "steps_taken": {"bf16_encoder": s_bf16.steps, "qat_mxfp8_encoder": s_qat.steps},
        "device": torch.cuda.get_device_name(0), "box": "one MI355X box", "repeats": "one run",
    }
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    sys.exit(0)

if args.ema:
    m_plain, m_ema, m_lerp = with_grads(build("bf16")), with_grads(build("bf16")), with_grads(build("bf16"))
    s_plain = DetectorTrainStep(m_plain, lr=1e-6, weight_decay=0.01, loss_scaling=False)
    s_ema = DetectorTrainStep(m_ema, lr=1e-6, weight_decay=0.01, loss_scaling=False, ema_decay=0.9999)
    s_lerp = DetectorTrainStep(m_lerp, lr=1e-6, weight_decay=0.01, loss_scaling=False)
    # what a user without the option runs after every step(): torch._foreach_lerp_ over the tensors the update touched (the encoder's
    # flat block as the one tensor it is to the update - 238 separate parameters would only add launches on that side)
    lerp_params = [p.detach() for p in s_lerp._segments()[0]]
    lerp_shadows = [p.clone() for p in lerp_params]

    def apply_then_lerp():
        s_lerp.apply()
        torch._foreach_lerp_(lerp_shadows, lerp_params, 1.0 - 0.9999)

    s_ema.apply()                                              # makes the shadows the swap exchanges
    swap_a, swap_b, swap_mirrors, _ = s_ema._swap_lists()
    copy_a, copy_b = [t.clone() for t in swap_a], [t.clone() for t in swap_b]
    copy_tmp = [torch.empty_like(t) for t in copy_a]

    def copy_swap():
        torch._foreach_copy_(copy_tmp, copy_a)
        torch._foreach_copy_(copy_a, copy_b)
        torch._foreach_copy_(copy_b, copy_tmp)

    pairs = {"apply": (("apply_without_ema", s_plain.apply, 1), ("apply_with_ema", s_ema.apply, 1), ("apply_without_ema_then_foreach_lerp", apply_then_lerp, 1)),
             "swap": (("swap_multi_one_exchange", lambda: ops.swap_multi(swap_a, swap_b, swap_mirrors), args.inner),
                      ("foreach_copy_through_a_temporary", copy_swap, args.inner))}
    ms = {}
    for what, group in pairs.items():
        for _ in range(args.warmup):
            for _, fn, _ in group:
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _, _ in group}
        for _ in range(args.runs):                             # alternating: one window of each in turn
            for name, fn, inner in group:
                samples[name].append(window(fn, inner))
        ms[what] = {name: spread(v, 5) for name, v in samples.items()}
    if (args.warmup + args.runs * args.inner) % 2:
        ops.swap_multi(swap_a, swap_b, swap_mirrors)           # an even number of exchanges: the weights are where they were
    segs = s_ema._segments()[0]
    elements = int(sum(p.numel() for p in segs))

    def apart(x, y):
        return bool(x["max_ms"] < y["min_ms"] or y["max_ms"] < x["min_ms"])

    plain, fused, lerp = (ms["apply"][k] for k in ("apply_without_ema", "apply_with_ema", "apply_without_ema_then_foreach_lerp"))
    sw, cp = ms["swap"]["swap_multi_one_exchange"], ms["swap"]["foreach_copy_through_a_temporary"]
    res = {
        "workload": {"config": args.config, "encoder": "bf16", "elements": elements, "segments": len(segs),
                     "launches_per_apply": {"without_ema": 1 + 2 * -(-len(segs) // ops.OPT_MAX_SEGMENTS),
                                            "with_ema": 1 + -(-len(segs) // ops.OPT_MAX_SEGMENTS) + -(-len(segs) // ops.EMA_MAX_SEGMENTS)},
                     "update_bytes_per_element": {"without_ema": 4 * 7 + 2, "with_ema": 4 * 9 + 2},
                     "swap": {"pairs": len(swap_a), "elements": int(sum(t.numel() for t in swap_a)),
                              "launches": -(-len(swap_a) // ops.SWAP_MAX_SEGMENTS), "foreach_copies": 3},
                     "ema_decay": 0.9999, "weight_decay": 0.01, "loss_scale": 1.0},
        "runs": args.runs, "warmup": args.warmup, "inner_calls_per_window": {"apply": 1, "swap": args.inner},
        "order": "alternating, one window of each of a group in turn, one process",
        "timer": "HIP events around each window, host work of the calls included",
        "ms": ms,
        "ema_over_plain": {"median_ms": round(fused["median_ms"] - plain["median_ms"], 5), "ratio": round(fused["median_ms"] / plain["median_ms"], 3),
                           "separated": apart(plain, fused)},
        "ema_over_apply_then_lerp": {"ratio": round(fused["median_ms"] / lerp["median_ms"], 3), "separated": apart(fused, lerp)},
        "swap_over_foreach_copy": {"ratio": round(sw["median_ms"] / cp["median_ms"], 3), "separated": apart(sw, cp)},
        "steps_taken": {"without_ema": s_plain.steps, "with_ema": s_ema.steps, "then_lerp": s_lerp.steps},
        "device": torch.cuda.get_device_name(0), "commit": args.commit, "box": "one MI355X box", "repeats": "one run",
    }
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    sys.exit(0)

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
