#!/usr/bin/env python
"""GPU milliseconds of needlet analysis and synthesis (eml_needlet_analysis_f32 / eml_needlet_synthesis_f32 through
emlight_amd.needlets.NeedletBasis) at B = 32, 128 x 256, jmax = 3 and 4.

The method of tools/bench_env_prefilter.py: back to back between two HIP events on torch's current stream, after a warm-up; a
figure is the median over `--windows` windows of `--reps` calls.  No stock formulation is timed beside them and no threshold
rests on these times.

    python tools/bench_needlets.py [--reps 20] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(fn, reps, windows, warmup=3):
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
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_needlets.py needs the MI355X")
    from emlight_amd.needlets import NeedletBasis
    dev = torch.device("cuda:0")
    B, H, W = a.batch, 128, 256
    g = np.random.default_rng([1, B])
    pano = torch.tensor(g.random((B, 3, H, W)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    r = {"B": B, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows}
    for jmax in (3, 4):
        nb = NeedletBasis(jmax, H, W, device=dev)
        coeffs = nb.analysis(pano)
        for key, fn in (("analysis", lambda: nb.analysis(pano)), ("synthesis", lambda: nb.synthesis(coeffs))):
            med, lo, hi = _ms(fn, a.reps, a.windows)
            name = "ms_%s_jmax%d" % (key, jmax)
            r[name], r[name + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        # P x K x 3B multiply-adds either way; the Legendre sums that make Psi are not counted
        r["tflops_analysis_jmax%d" % jmax] = round(2.0 * nb.P * nb.K * 3 * B / (r["ms_analysis_jmax%d" % jmax] * 1e-3) / 1e12, 2)
        r["tflops_synthesis_jmax%d" % jmax] = round(2.0 * nb.P * nb.K * 3 * B / (r["ms_synthesis_jmax%d" % jmax] * 1e-3) / 1e12, 2)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
