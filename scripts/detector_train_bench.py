#!/usr/bin/env python3
"""Time of the detector's training iteration, split into its three calls - LayoutDetectionModel.losses(), backward() of the summed
loss, DetectorTrainStep.apply() - for grad_dtype "f32" and "bf16" (DESIGN section 30), alternating in ONE process on ONE set of
weights: ViT-B/16 detector, bf16 encoder, 224 x 224, bs=64, synthetic pages and targets from a seed, drop_path_rate = 0.  HIP events
around each call (host work of the call included), every shape warmed up in both settings first, median / min / max of --runs
iterations per setting.  The weights move by one AdamW step per timed iteration (lr 1e-6), for both settings alike.
--count N [--phases losses|iteration]: no timing and no file - N iterations (or their losses() alone) in the FIRST setting, for a
kernel trace of the process from outside: launches per call are differences between two such traces (scripts/README.md).
--train-dtype f32,bf16: the settings that alternate are train_dtype's instead, under one --grad-dtype (default
bf16); peak allocated memory of an iteration is recorded per setting, and the file is profiles/detector_train_bench_train_bf16.json.
--compute-dtype bf16,mxfp8: the settings that alternate are ENCODER builds - "mxfp8" is the quantisation-aware
build (qat=True), whose apply() ends with the one re-quantise launch - each a detector of its own from the same initial weights,
under one --grad-dtype; the file is profiles/detector_train_bench_qat.json.
--accumulate A: one detector under DetectorTrainStep(accumulate=A), --grad-dtype as given.  Timed per call of
step(): the A - 1 calls of an update that only fold their gradients into the bucket, and the one that also applies it.  Then, on
the gradients and the bucket's slices the last call left, the fold launches alone in both modes (ops.grads_accumulate_multi) beside
torch._foreach_copy_ / torch._foreach_add_ over the same tensor lists, the four alternating; the file is
profiles/detector_train_bench_accum.json.
Needs a GPU: without one it fails.  Writes one JSON object (--out, default profiles/detector_train_bench.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from layoutdit_amd import config as cfgs, synth  # noqa: E402
from layoutdit_amd.modeling import LayoutDetectionModel  # noqa: E402
from layoutdit_amd.training import DetectorTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="vit_base", choices=["vit_micro", "vit_tiny", "vit_base"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--settings", default="f32,bf16", help="comma-separated grad_dtype settings, timed alternately in this order")
ap.add_argument("--train-dtype", default=None, help="comma-separated train_dtype settings: these alternate instead, under --grad-dtype")
ap.add_argument("--compute-dtype", default=None, help="comma-separated encoder builds (bf16, mxfp8 = qat): these alternate instead, under --grad-dtype")
ap.add_argument("--grad-dtype", default="bf16", help="the one grad_dtype of a --train-dtype or --compute-dtype run")
ap.add_argument("--accumulate", type=int, default=0, help="micro-batches per update: time step() per call and the fold launches (see above)")
ap.add_argument("--count", type=int, default=0, help="no timing, nothing written: this many iterations of --phases in the first setting")
ap.add_argument("--phases", default="iteration", choices=["losses", "iteration"])
ap.add_argument("--commit", default=None, help="recorded as the tree's commit (default: git rev-parse of the checkout, if it is one)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.train_dtype and args.compute_dtype:
    ap.error("--train-dtype and --compute-dtype: one option alternates per run")
if args.accumulate and (args.train_dtype or args.compute_dtype or args.count or args.accumulate < 2):
    ap.error("--accumulate: at least 2, and on its own (no --train-dtype, --compute-dtype or --count)")
args.out = args.out or os.path.join(ROOT, "profiles", "detector_train_bench_accum.json" if args.accumulate else
                                    "detector_train_bench_qat.json" if args.compute_dtype else
                                    "detector_train_bench_train_bf16.json" if args.train_dtype else "detector_train_bench.json")
if args.runs < 20 and not args.count:
    ap.error("--runs: at least 20 iterations per setting")
if not torch.cuda.is_available():
    sys.exit("detector_train_bench: no GPU found (the detector has no CPU path)")

dev = "cuda:0"
settings = (args.compute_dtype or args.train_dtype or args.settings).split(",")
if args.compute_dtype and any(s not in ("bf16", "mxfp8") for s in settings):
    ap.error("--compute-dtype: bf16 and mxfp8 (the quantisation-aware build) are the encoders this comparison covers")
cfg = getattr(cfgs, args.config)()
cfg.drop_path_rate = 0.0


def build(compute_dtype: str):
    torch.manual_seed(0)
    m = LayoutDetectionModel(config=cfg, compute_dtype=compute_dtype, qat=compute_dtype == "mxfp8")
    m.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    m = m.to(dev).train()
    return m, DetectorTrainStep(m, lr=1e-6, accumulate=max(args.accumulate, 1))


# one detector whose options alternate, or (--compute-dtype) one detector per encoder build
built = {s: build(s) for s in settings} if args.compute_dtype else {None: build("bf16")}
model, step = next(iter(built.values()))

pages = synth.synth_images(args.batch, 224, 224, seed=args.seed, kind="doc")
images = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pages]
rng = np.random.RandomState(args.seed)
targets = []
for _ in range(args.batch):
    n = int(rng.randint(1, 9))
    x0, y0 = rng.uniform(0, 150, size=n), rng.uniform(0, 150, size=n)
    w, h = rng.uniform(16, 72, size=n), rng.uniform(16, 72, size=n)
    boxes = np.stack([x0, y0, np.minimum(x0 + w, 223.0), np.minimum(y0 + h, 223.0)], axis=1).astype(np.float32)
    targets.append({"boxes": torch.from_numpy(boxes).to(dev), "labels": torch.from_numpy(rng.randint(1, 6, size=n).astype(np.int64)).to(dev)})


def iteration(setting: str, timed: bool, losses_only: bool = False):
    model, step = built[setting] if args.compute_dtype else built[None]
    if args.compute_dtype:
        model.set_grad_dtype(args.grad_dtype)
    elif args.train_dtype:
        model.set_grad_dtype(args.grad_dtype).set_train_dtype(setting)
    else:
        model.set_grad_dtype(setting)
    for p in model.parameters():
        p.grad = None
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timed else None
    if timed:
        ev[0].record()
    losses = model.losses(images, targets, generator=gen)
    total = sum(losses.values())
    if losses_only:
        return None, float(total.detach())
    if timed:
        ev[1].record()
    total.backward()
    if timed:
        ev[2].record()
    step.apply()
    if timed:
        ev[3].record()
        ev[3].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)], float(total.detach())
    return None, float(total.detach())


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def head_commit():
    try:
        return args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or None
    except (OSError, subprocess.SubprocessError):
        return args.commit


def timed_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


if args.accumulate:
    from layoutdit_amd import ops  # noqa: E402
    model.set_grad_dtype(args.grad_dtype)
    A = args.accumulate

    def micro_batch():
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        return step.step(images, targets, generator=gen)

    for _ in range(args.warmup * A):                # whole updates: every shape, every cache, every moment and the bucket
        micro_batch()
    torch.cuda.synchronize()
    calls = {"fold_only": [], "fold_and_apply": []}
    finite = True
    for _ in range(args.runs):                      # the two kinds of call alternate by construction: A - 1 folds, then the update
        for k in range(A):
            t, losses = timed_call(micro_batch)
            calls["fold_and_apply" if k == A - 1 else "fold_only"].append(t)
            finite = finite and all(bool(torch.isfinite(v)) for v in losses.values())
    assert step.pending_micro_batches == 0
    # the fold alone, on what the last call left: the parameters' gradients and the bucket's slices (rewritten by the next fold)
    grads, slices = [g.reshape(-1) for g in step._segments()[1]], step._bucket_slices
    assert len(grads) == len(slices) and all(g.numel() == s.numel() for g, s in zip(grads, slices))
    folds = {"ldit_overwrite": lambda: ops.grads_accumulate_multi(slices, grads, True),
             "ldit_add": lambda: ops.grads_accumulate_multi(slices, grads, False),
             "torch_foreach_copy_": lambda: torch._foreach_copy_(slices, grads),
             "torch_foreach_add_": lambda: torch._foreach_add_(slices, grads)}
    step.bucket.zero_()                             # finite sums whatever the folds above left
    for _ in range(args.warmup):
        for fn in folds.values():
            fn()
    torch.cuda.synchronize()
    fold_ms = {k: [] for k in folds}
    for _ in range(args.runs):
        for k, fn in folds.items():
            fold_ms[k].append(timed_call(fn)[0])
    elements = int(sum(g.numel() for g in grads))
    res = {
        "workload": {"config": args.config, "encoder": "bf16", "batch": args.batch, "image": [224, 224], "seed": args.seed, "drop_path_rate": 0.0,
                     "grad_dtype": args.grad_dtype, "optimizer": f"DetectorTrainStep(lr=1e-6, accumulate={A}), every call one micro-batch of the whole batch"},
        "accumulate": A, "order": "alternating in one process: the calls of an update in turn; the four folds in turn",
        "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call, host work of the call included",
        "step_call_ms": {k: stats(v) for k, v in calls.items()},
        "apply_share_ms": round(statistics.median(calls["fold_and_apply"]) - statistics.median(calls["fold_only"]), 3),
        "fold": {"segments": len(grads), "elements": elements, "launches": -(-sum(1 for g in grads if g.numel()) // ops.ACC_MAX_SEGMENTS),
                 "bytes_moved": {"overwrite": 8 * elements, "add": 12 * elements}, "ms": {k: stats(v) for k, v in fold_ms.items()}},
        "all_losses_finite": finite, "steps": step.steps, "skipped_steps": step.skipped_steps,
        "device": torch.cuda.get_device_name(0), "commit": head_commit(), "box": "one MI355X box", "repeats": "one run",
    }
    for mode, nbytes in (("overwrite", 8), ("add", 12)):
        res["fold"]["ldit_" + mode + "_gb_per_s"] = round(nbytes * elements / (res["fold"]["ms"]["ldit_" + mode]["median_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    sys.exit(0)

if args.count:
    for _ in range(args.count):
        iteration(settings[0], False, losses_only=args.phases == "losses")
    torch.cuda.synchronize()
    sys.exit(0)
for _ in range(args.warmup):                       # every shape, every cache and every moment, in both settings
    for s in settings:
        iteration(s, False)
torch.cuda.synchronize()
samples = {s: [] for s in settings}
peak = {s: 0 for s in settings}
finite = True
for _ in range(args.runs):
    for s in settings:
        if args.train_dtype or args.compute_dtype:
            torch.cuda.reset_peak_memory_stats()
        t, total = iteration(s, True)
        peak[s] = max(peak[s], torch.cuda.max_memory_allocated())
        samples[s].append(t)
        finite = finite and bool(np.isfinite(total))
torch.cuda.synchronize()


ms = {s: {name: stats([t[i] for t in samples[s]]) for i, name in enumerate(("losses", "backward", "apply"))} for s in settings}
commit = head_commit()
res = {
    "workload": {"config": args.config, "encoder": "per setting (mxfp8 = qat)" if args.compute_dtype else "bf16", "batch": args.batch, "image": [224, 224], "seed": args.seed, "drop_path_rate": 0.0,
                 "gt_boxes": int(sum(len(t["labels"]) for t in targets)), "sampled_rows_per_image": model.model.roi_heads.batch_size_per_image,
                 "optimizer": "DetectorTrainStep(lr=1e-6), one step per timed iteration"},
    "settings": settings, "order": "alternating, one iteration of each setting in turn, one process, " +
                                   ("one detector per encoder build, equal initial weights" if args.compute_dtype else "one set of weights"),
    "runs": args.runs, "warmup": args.warmup, "timer": "HIP events around each call, host work of the call included",
    "ms": ms, "all_losses_finite": finite,
    "steps": {s: b[1].steps for s, b in built.items()} if args.compute_dtype else step.steps,
    "skipped_steps": {s: b[1].skipped_steps for s, b in built.items()} if args.compute_dtype else step.skipped_steps,
    "launches": None,                                  # from kernel traces of --count runs, where they were made (scripts/README.md)
    "device": torch.cuda.get_device_name(0), "commit": commit, "box": "one MI355X box", "repeats": "one run",
}
if len(settings) == 2:
    a, b = (ms[s]["backward"] for s in settings)
    res["backward_difference"] = {"median_ms": round(a["median_ms"] - b["median_ms"], 3),
                                  "spread_ms": {s: round(ms[s]["backward"]["max_ms"] - ms[s]["backward"]["min_ms"], 3) for s in settings},
                                  "separated": bool(b["max_ms"] < a["min_ms"])}
if args.compute_dtype:
    res["option"], res["grad_dtype"] = "compute_dtype", args.grad_dtype
    res["peak_allocated_mb"] = {s: round(peak[s] / 2 ** 20, 1) for s in settings}
    res["apply_launches"] = "the bf16 encoder's, plus one for mxfp8 (ldit_requant_train_mirror)"
    if len(settings) == 2:
        for phase in ("losses", "apply"):
            a, b = (ms[s][phase] for s in settings)
            res[phase + "_difference"] = {"median_ms": round(a["median_ms"] - b["median_ms"], 3),
                                          "spread_ms": {s: round(ms[s][phase]["max_ms"] - ms[s][phase]["min_ms"], 3) for s in settings},
                                          "separated": bool(b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"])}
if args.train_dtype:
    res["option"], res["grad_dtype"] = "train_dtype", args.grad_dtype
    res["peak_allocated_mb"] = {s: round(peak[s] / 2 ** 20, 1) for s in settings}
    if len(settings) == 2:
        a, b = (ms[s]["losses"] for s in settings)
        res["losses_difference"] = {"median_ms": round(a["median_ms"] - b["median_ms"], 3),
                                    "spread_ms": {s: round(ms[s]["losses"]["max_ms"] - ms[s]["losses"]["min_ms"], 3) for s in settings},
                                    "separated": bool(b["max_ms"] < a["min_ms"])}
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
