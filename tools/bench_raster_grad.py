#!/usr/bin/env python
"""GPU microseconds of the SG rasteriser's three launches: the forward (eml_sg_rasterise_f32), the colour-only backward
(eml_sg_rasterise_bwd_colors_ex_f32: what convert_to_panorama's backward runs when only colours need a gradient) and the full
backward (eml_sg_rasterise_bwd_f32: dirs, sizes and colours).

Each launch goes through the C ABI into pre-allocated outputs, back to back between two HIP events on torch's current stream,
after a warm-up; a figure is the median over `--windows` windows of `--reps` launches.  Shapes: cfg3 (B=32, N=128, 128x256,
Fibonacci anchors at .0025), cfg5 per GPU (B=16, N=256, 256x512, the same anchors) and wide random lobes (B=32, N=128,
128x256, sizes .02-.3: almost nothing is culled).

    python tools/bench_raster_grad.py [--reps 200] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("cfg3", 32, 128, 128, "anchors"), ("cfg5_per_gpu", 16, 256, 256, "anchors"), ("wide_random", 32, 128, 128, "wide")]


def _us(fn, reps, windows, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(windows):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster_grad.py needs the MI355X")
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.util import sphere_points
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream
    dev = torch.device("cuda:0")
    rows = []
    for name, B, n, H, kind in SHAPES:
        W = 2 * H
        g = np.random.default_rng([1, B, n, H])
        if kind == "anchors":
            dirs = np.tile(sphere_points(n).reshape(1, 3 * n), (B, 1))
            sizes = np.full((B, n), 0.0025)
        else:
            d = g.standard_normal((B, n, 3))
            dirs = (d / np.linalg.norm(d, axis=2, keepdims=True)).reshape(B, 3 * n)
            sizes = g.uniform(0.02, 0.3, (B, n))
        colors = g.uniform(0, 3, (B, 3 * n))
        dirs, sizes, colors = (torch.tensor(x, dtype=torch.float32, device=dev) for x in (dirs, sizes, colors))
        gout = torch.tensor(g.standard_normal((B, 3, H, W)), dtype=torch.float32, device=dev)
        pano = torch.empty(B, 3, H, W, device=dev)
        gd, gs, gc = torch.empty(B, 3 * n, device=dev), torch.empty(B, n, device=dev), torch.empty(B, 3 * n, device=dev)
        work_c = torch.empty(L.eml_sg_rasterise_bwd_work_floats(B, n, H, W), device=dev)
        work_f = torch.empty(L.eml_sg_rasterise_bwd_full_work_floats(B, n, H, W), device=dev)

        def fwd():
            _lib.check(L.eml_sg_rasterise_f32(p(dirs), p(sizes), p(colors), p(pano), B, n, H, W, st()), "eml_sg_rasterise_f32")

        def bwd_colors():
            _lib.check(L.eml_sg_rasterise_bwd_colors_ex_f32(p(dirs), p(sizes), p(gout), p(gc), p(work_c), B, n, H, W, 0, st()),
                       "eml_sg_rasterise_bwd_colors_ex_f32")

        def bwd_full():
            _lib.check(L.eml_sg_rasterise_bwd_f32(p(dirs), p(sizes), p(colors), p(gout), p(gd), p(gs), p(gc), p(work_f), B, n, H,
                                                  W, 0, st()), "eml_sg_rasterise_bwd_f32")

        r = {"shape": name, "B": B, "N": n, "H": H, "W": W}
        for leg, fn in (("fwd", fwd), ("bwd_colors", bwd_colors), ("bwd_full", bwd_full)):
            med, lo, hi = _us(fn, a.reps, a.windows)
            r["us_" + leg] = round(med, 2)
            r["us_" + leg + "_range"] = [round(lo, 2), round(hi, 2)]
        r["full_over_colors"] = round(r["us_bwd_full"] / r["us_bwd_colors"], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
