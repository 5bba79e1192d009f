#!/usr/bin/env python3
"""The mxfp8 inference build beside the fp8 build, one process, BASELINE configs[4] geometry (ViT-B/16 224^2, bs=32, synthetic
weights): the fp8 model is calibrated (untimed), both are warmed up and then timed back to back with bench.py's method (HIP events
around each forward, median over the steps).  Prints one JSON line.  bench.py has no mxfp8 choice on purpose (its yardstick stays
put); this script is where the build is measured.

    python scripts/mxfp8_bench.py [--steps 20] [--warmup 5] [--batch 32] [--rounds 3] [--out FILE]
    python scripts/mxfp8_bench.py --only mxfp8 --steps 5       # e.g. under rocprofv3 --kernel-trace --stats -- python ...

--rounds alternates the two builds (fp8, mxfp8, fp8, mxfp8, ...) so that clock drift falls on both."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["fp8", "mxfp8"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from layoutdit_amd import config as cfgs, synth
    from layoutdit_amd.modeling import DiTEncoder

    dev = torch.device("cuda", 0)
    cfg = cfgs.vit_base()
    w = synth.synth_weights(cfg, seed=0)
    x = torch.from_numpy(synth.synth_images(args.batch, 224, 224, seed=1234)).to(dev)
    builds = [args.only] if args.only else ["fp8", "mxfp8"]
    models = {}
    for b in builds:
        m = DiTEncoder(cfg, compute_dtype=b).load_numpy(w).to(dev).eval()
        if b == "fp8":
            m.calibrate_fp8(x)                          # untimed set-up, as in bench.py
        models[b] = m
    ms = {b: [] for b in builds}
    with torch.no_grad():
        for _ in range(args.rounds):
            for b, m in models.items():
                for _ in range(max(args.warmup, 1)):
                    out = m(x)
                torch.cuda.synchronize(dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
                ev[0].record()
                for i in range(args.steps):
                    out = m(x)
                    ev[i + 1].record()
                torch.cuda.synchronize(dev)
                ms[b] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]
                assert all(bool(torch.isfinite(h).all()) for h in out.hidden_states if h is not None)
    line = {"geometry": "vit_base 224x224", "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "device": torch.cuda.get_device_name(dev)}
    for b in builds:
        med = statistics.median(ms[b])
        line[b] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(ms[b]), 4), "ms_max": round(max(ms[b]), 4),
                   "images_per_sec": round(args.batch / med * 1e3, 1)}
    if len(builds) == 2:
        line["mxfp8_over_fp8_time"] = round(line["mxfp8"]["ms_per_step_median"] / line["fp8"]["ms_per_step_median"], 4)
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
