#!/usr/bin/env python
"""Step-time cost of the DenseNet encoder's input gradient, and the bytes its kernel moves.

Three requests of one train-mode forward + backward of the encoder at cfg2 (B=64, 240x320 crops, 128 anchors), alternated in
one process after a warm-up:
  * params  -- every parameter, x without a gradient (the training step);
  * params+x -- every parameter and x;
  * x       -- x only, every parameter frozen (a lighting-consistency loss, test-time optimisation).
Each figure is device-event milliseconds of one step (forward + backward), median / min / max over `--steps` timed steps.

The kernel's own time comes from a separate profiler run (`--modes x --steps 3` under `rocprofv3 --kernel-trace --stats`);
`--stats CSV` then reads that run's kernel-stats file (no GPU needed) and divides the kernel's algorithmic bytes -- computed
from the shapes below -- by its average duration, as a fraction of the 8 TB/s HBM peak.

    python tools/bench_dense_input_grad.py [--steps 20] [--warmup 5] [--modes params,params+x,x] [--out FILE.json]
    python tools/bench_dense_input_grad.py --stats DIR_OR_CSV [--norm0-fused 1]
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, CROP, ANCHORS, C0 = 64, (240, 320), 128, 24
HBM_PEAK = 8.0e12
KERNEL = "conv0_bwd_data_kernel"


def algorithmic_bytes(B=B, H=CROP[0], W=CROP[1], fused=True):
    """What conv0's data gradient must move: per pixel G's first 24 columns and Y0 (24 floats each), X1's 24 on the
    materialised path, and the 3 output floats.  The halo re-reads and the 2.6 KB of W0 are not counted."""
    per_pixel = 4 * (C0 + C0 + (0 if fused else C0) + 3)
    return B * H * W * per_pixel


def _model():
    import torch
    import oracle
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    net = DenseNet(anchors=ANCHORS, crop_hw=CROP).cuda().train()
    ref = oracle.OracleDenseNet(anchors=ANCHORS, crop_hw=CROP)
    net.load_state_dict(oracle.deterministic_state_dict(ref.state_dict(), seed=2))
    return net


def timed(steps, warmup, modes):
    import torch
    net = _model()
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.rand(B, 3, *CROP, device="cuda", generator=g)
    w = {k: torch.randn(B, n, device="cuda", generator=g) for k, n in
         (("distribution", ANCHORS), ("intensity", 1), ("rgb_ratio", 3), ("ambient", 3))}
    params = list(net.parameters())

    def step(mode):
        for q in params:
            q.requires_grad_(mode != "x")
            q.grad = None
        x = x0.clone().requires_grad_(mode != "params")
        out = net(x)
        sum((out[k] * w[k]).sum() for k in w).backward()

    times = {m: [] for m in modes}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in modes]
    for it in range(warmup + steps):
        for m, (e0, e1) in zip(modes, ev):   # alternate the requests: the box's drift lands on all of them alike
            e0.record()
            step(m)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[m].append(e0.elapsed_time(e1))
    res = {"config": "cfg2 B=%d %dx%d anchors=%d, train-mode forward+backward of the encoder" % ((B,) + CROP + (ANCHORS,)),
           "steps": steps, "warmup": warmup, "modes": {}}
    base = float(np.median(times[modes[0]]))
    for m in modes:
        t = times[m]
        res["modes"][m] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(min(t)), 3),
                           "ms_max": round(float(max(t)), 3), "vs_first": round(float(np.median(t)) / base, 4)}
    return res


def from_stats(path, fused):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % path)
    rows = [r for f in files for r in csv.DictReader(open(f)) if KERNEL in r["Name"]]
    if not rows:
        raise SystemExit("%s not in %s" % (KERNEL, files))
    calls = sum(int(r["Calls"]) for r in rows)
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    avg_s = total_ns / calls * 1e-9
    nbytes = algorithmic_bytes(fused=fused)
    return {"kernel": KERNEL, "calls": calls, "avg_us": round(avg_s * 1e6, 2), "algorithmic_bytes": nbytes,
            "achieved_TBps": round(nbytes / avg_s / 1e12, 3), "fraction_of_8TBps": round(nbytes / avg_s / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="params,params+x,x")
    ap.add_argument("--stats", default=None, help="rocprofv3 --stats output (directory or kernel_stats.csv): no GPU run")
    ap.add_argument("--norm0-fused", type=int, default=1, help="path the profiled run took (EML_NORM0_FUSED)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stats:
        res = from_stats(a.stats, bool(a.norm0_fused))
    else:
        modes = a.modes.split(",")
        if any(m not in ("params", "params+x", "x") for m in modes):
            raise SystemExit("--modes: params, params+x, x")
        res = timed(a.steps, a.warmup, modes)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
