#!/usr/bin/env python
"""GPU microseconds per Sinkhorn loss call (SamplesLoss.forward_raw: loop kernel + finishing kernel, forward and both unit
gradients), balanced and with a ``--reach`` (unbalanced OT, eml_sinkhorn_fwd_rho_f32).

Outputs are pre-allocated once, so a window is back-to-back launches between two HIP events on torch's current stream; the
balanced and the damped call alternate window by window in the same process, and a figure is the median over `--windows`
windows of `--reps` calls.  Shapes: cfg2 (B=64, N=128, the register-resident kernel) and cfg5 per GPU (B=16, N=256, the
split kernel), blur .05, the inputs of bench.py's Sinkhorn leg.

    python tools/bench_sinkhorn.py [--reach .1] [--reps 200] [--windows 7] [--out FILE.json]

``--dim``: instead of balanced vs damped, balanced calls on (B, N, D) samples for D in {1, 2, 4, 8} (eml_sinkhorn_fwd_dim_f32
for D > 1), alternating window by window the same way.

``--per_sample``: one shared (N, N) chord matrix (eml_sinkhorn_fwd_ex_f32) against one matrix per sample (B, N, N)
(eml_sinkhorn_fwd_cost_f32, stride N*N; the matrices of depths U(.5, 3) as gmloss.SamplesLoss builds them), and the batched
builder eml_gm_anchor_cost_f32 on its own, alternating the same way.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("cfg2", 64, 128), ("cfg5_per_gpu", 16, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reach", type=float, default=.1, help="reach of the damped calls (SamplesLoss(reach=...))")
    ap.add_argument("--blur", type=float, default=.05)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dim", action="store_true", help="time D = 1, 2, 4, 8 samples instead of balanced vs damped")
    ap.add_argument("--per_sample", action="store_true",
                    help="time a shared chord matrix against one per sample, and the batched cost builder")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinkhorn.py needs the MI355X")
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_outputs
    dev = torch.device("cuda:0")
    rows = []
    for name, B, N in SHAPES:
        g = torch.Generator().manual_seed(7)
        x = torch.softmax(torch.randn(B, N, generator=g), 1).view(B, N, 1).to(dev)
        y = torch.softmax(3 * torch.randn(B, N, generator=g), 1).view(B, N, 1).to(dev)
        calls = {}
        if a.per_sample:
            from emlight_amd import _lib
            from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_raw
            crit = SamplesLoss("sinkhorn", p=2, blur=a.blur, anchors=N)
            M1, _ = crit.cost_matrix(dev)
            depth = torch.empty(B, N).uniform_(.5, 3., generator=g).to(dev)
            anchors, Mb = torch.empty(B, N, 3, device=dev), torch.empty(B, N, N, device=dev)

            def build():
                _lib.check(_lib.lib().eml_gm_anchor_cost_f32(_lib.ptr(depth), 0, B, N, _lib.ptr(anchors), _lib.ptr(Mb),
                                                             _lib.current_stream()), "eml_gm_anchor_cost_f32")
                return None
            build()
            xr, yr = x.view(B, N).contiguous(), y.view(B, N).contiguous()
            for label, M in (("shared", M1), ("per_sample", Mb)):
                out = sinkhorn_outputs(B, N, dev, True, True)
                calls[label] = (lambda M=M, out=out: sinkhorn_raw(xr, yr, None, None, M, M, 2, a.blur, .5, None, True, True,
                                                                  out=out))
        elif a.dim:
            crit = SamplesLoss("sinkhorn", p=2, blur=a.blur, anchors=N)
            for D in (1, 2, 4, 8):
                # component 0 is the 1-D input; the others are further draws of the same recipe
                xd = torch.cat([x] + [torch.softmax(torch.randn(B, N, generator=g), 1).view(B, N, 1).to(dev)
                                      for _ in range(D - 1)], 2).contiguous()
                yd = torch.cat([y] + [torch.softmax(3 * torch.randn(B, N, generator=g), 1).view(B, N, 1).to(dev)
                                      for _ in range(D - 1)], 2).contiguous()
                out = sinkhorn_outputs(B, N, dev, True, True, D=D)
                calls["D%d" % D] = (lambda xd=xd, yd=yd, out=out: crit.forward_raw(xd, yd, out=out))
        else:
            for label, reach in (("balanced", None), ("reach", a.reach)):
                crit = SamplesLoss("sinkhorn", p=2, blur=a.blur, reach=reach, anchors=N)
                out = sinkhorn_outputs(B, N, dev, True, True)
                calls[label] = (lambda crit=crit, out=out: crit.forward_raw(x, y, out=out))
        n_eps = int(next(iter(calls.values()))()["n_eps"].item())
        if a.per_sample:
            calls["builder"] = build
        for fn in calls.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = {k: [] for k in calls}
        for _ in range(a.windows):
            for k, fn in calls.items():
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.reps)
        row = {"shape": name, "B": B, "N": N, "n_eps": n_eps}
        if not a.dim and not a.per_sample:
            row["reach"] = a.reach
        for k, v in us.items():
            row[k + "_us"] = round(float(np.median(v)), 2)
            row[k + "_us_min_max"] = [round(float(min(v)), 2), round(float(max(v)), 2)]
        if a.per_sample:
            row["per_sample_over_shared"] = round(row["per_sample_us"] / row["shared_us"], 4)
        elif a.dim:
            for D in (2, 4, 8):
                row["D%d_over_D1" % D] = round(row["D%d_us" % D] / row["D1_us"], 4)
        else:
            row["reach_over_balanced"] = round(row["reach_us"] / row["balanced_us"], 4)
        rows.append(row)
        print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
