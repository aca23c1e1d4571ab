#!/usr/bin/env python
"""Step-time cost of the DenseNet encoder's dropout (drop_rate > 0, DenseNet.py:50-55), and its per-kernel deltas.

Two regression trainers at cfg2 (B=64, 240x320 crops, 128 anchors; RegressionTrainer.step: encoder forward, Sinkhorn loss,
backward, Adam), identical weights, one with drop_rate 0 and one with drop_rate 0.2, stepped alternately in one process on
one box after a warm-up.  Each figure is device-event milliseconds of one step, median / min / max over `--steps` steps.

The kernels' own times come from a separate profiler run (`--rates 0,0.2 --steps 3` under `rocprofv3 --kernel-trace
--stats`); `--stats CSV` then reads that run's kernel-stats file (no GPU needed) and pairs each conv3x3 kernel's DROP
instantiation with the plain one: average microseconds per call and the ratio.

    python tools/bench_dense_dropout.py [--steps 20] [--warmup 5] [--rates 0,0.2] [--out FILE.json]
    python tools/bench_dense_dropout.py --stats DIR_OR_CSV
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, CROP, ANCHORS = 64, (240, 320), 128
KERNELS = ("conv3x3_fwd_kernel", "conv3x3_fwd_tp_kernel", "conv3x3_bwd_data_kernel", "conv3x3_bwd_fused_tp_kernel")


def timed(steps, warmup, rates):
    import torch
    import oracle
    from emlight_amd.RegressionNetwork.data import synthetic_batch
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    dev = "cuda:0"
    sd = oracle.deterministic_state_dict(oracle.OracleDenseNet(anchors=ANCHORS, crop_hw=CROP).state_dict(), seed=2)
    trainers = []
    for r in rates:
        tr = RegressionTrainer(anchors=ANCHORS, crop_hw=CROP, device=dev, drop_rate=r)
        tr.model.load_state_dict(sd)
        trainers.append(tr)
    batch = synthetic_batch(B, ANCHORS, CROP, seed=1234, device=dev)
    times = {r: [] for r in rates}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(warmup + steps):
        for r, tr in zip(rates, trainers):   # alternate: the box's drift lands on both alike
            e0.record()
            loss, _ = tr.step(batch)
            e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(loss).all()
            if it >= warmup:
                times[r].append(e0.elapsed_time(e1))
    res = {"config": "cfg2 B=%d %dx%d anchors=%d, RegressionTrainer.step" % ((B,) + CROP + (ANCHORS,)),
           "steps": steps, "warmup": warmup, "drop_rate": {}}
    base = float(np.median(times[rates[0]]))
    for r in rates:
        t = times[r]
        res["drop_rate"][str(r)] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(min(t)), 3),
                                    "ms_max": round(float(max(t)), 3), "vs_first": round(float(np.median(t)) / base, 4)}
    return res


def from_stats(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % path)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    res = {}
    for k in KERNELS:
        acc = {}
        for r in rows:
            name = r["Name"]
            m = re.search(r"\b%s(<[^(]*>)?\(" % k, name)
            if not m:
                continue
            drop = (m.group(1) or "").strip("<>").replace(" ", "").split(",")[-1] == "true"   # DROP is the last argument
            c, t = acc.get(drop, (0, 0.0))
            acc[drop] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]))
        if acc:
            res[k] = {("drop" if d else "plain"): {"calls": c, "avg_us": round(t / c / 1e3, 2)} for d, (c, t) in acc.items()}
            if len(acc) == 2:
                res[k]["drop_vs_plain"] = round(res[k]["drop"]["avg_us"] / res[k]["plain"]["avg_us"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rates", default="0,0.2")
    ap.add_argument("--stats", default=None, help="rocprofv3 --stats output (directory or kernel_stats.csv): no GPU run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = from_stats(a.stats) if a.stats else timed(a.steps, a.warmup, [float(r) for r in a.rates.split(",")])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
