#!/usr/bin/env python
"""GPU milliseconds of the gradients of object insertion, in one process on one box:

* the prefilter adjoint (eml_env_prefilter_bwd_f32) at B = 32, 128 x 256, Ho = 64, the diffuse lobe plus one Phong lobe
  (m = 50), next to the forward (eml_env_prefilter_f32) on the same shapes;
* the stock formulation of that adjoint: the (texels x directions) TRANSPOSED weight tables of both lobes stored in device
  memory, then torch.matmul per lobe against the gradient planes and one add.  The table build is not timed;
* the shading backward (eml_gbuffer_shade_bwd_f32) at 192 x 256 with a sphere G-buffer, three terms, the three coefficient
  gradients and the two map gradients, with and without dpano (the mirror scatter into the 128 x 256 panorama).

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls, with the smallest and the largest window beside it.  No test and no threshold rests on these times.

    python tools/bench_insert_grad.py [--reps 20] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_env_prefilter import _ms, weight_tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_insert_grad.py needs the MI355X")
    from emlight_amd.insert import gbuffer_sphere, prefilter_environment
    from emlight_amd.insert_grad import prefilter_environment_bwd_raw, shade_gbuffer_bwd_raw
    dev = torch.device("cuda:0")
    B, H, Ho, m = a.batch, 128, a.height, 50.0
    W, D, T = 2 * H, 2 * Ho * Ho, 2 * H * H
    rng = np.random.default_rng([2, B, Ho])
    pano = torch.tensor(rng.random((B, 3, H, W)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    g = torch.tensor(rng.standard_normal((B, 2, 3, Ho, 2 * Ho)), dtype=torch.float32, device=dev)
    r = {"B": B, "H": H, "W": W, "Ho": Ho, "directions": D, "lobes": ["diffuse", m], "device": torch.cuda.get_device_name(0),
         "reps": a.reps, "windows": a.windows}

    def record(key, fn):
        med, lo, hi = _ms(fn, a.reps, a.windows)
        r["ms_" + key], r["ms_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        return med

    record("forward_diffuse_phong", lambda: prefilter_environment(pano, Ho, ("diffuse", m)))
    med = record("adjoint_diffuse_phong", lambda: prefilter_environment_bwd_raw(g, H, ("diffuse", m)))
    r["adjoint_tflops"] = round(2 * 2.0 * D * T * 3 * B / (med * 1e-3) / 1e12, 2)     # 2 lobes x D x T x 3B multiply-adds
    record("adjoint_diffuse", lambda: prefilter_environment_bwd_raw(g[:, :1].contiguous(), H, ("diffuse",)))
    four = torch.cat([g, g], 1)
    record("adjoint_four_lobes", lambda: prefilter_environment_bwd_raw(four, H, ("diffuse", m, 10.0, 200.0)))

    Kd, Kg = weight_tables(H, Ho, m, dev)
    KdT, KgT = Kd.t().contiguous(), Kg.t().contiguous()                # (T, D): stored transposed, made once
    del Kd, Kg
    planes = g.permute(1, 3, 4, 0, 2).reshape(2, D, 3 * B).contiguous()   # (lobe, D, 3B): the GEMMs' B operands, made once
    out_d, out_g = torch.empty(T, 3 * B, device=dev), torch.empty(T, 3 * B, device=dev)

    def stock():
        torch.matmul(KdT, planes[0], out=out_d)
        torch.matmul(KgT, planes[1], out=out_g)
        out_d.add_(out_g)

    med = record("stock_matmul", stock)
    r["stock_tflops"] = round(2 * 2.0 * D * T * 3 * B / (med * 1e-3) / 1e12, 2)
    r["stock_table_bytes"] = int(KdT.numel() * 4 + KgT.numel() * 4)
    mine = prefilter_environment_bwd_raw(g, H, ("diffuse", m)).reshape(3 * B, T)
    stock()
    r["max_rel_difference_to_stock"] = float((mine - out_d.t()).abs().max() / out_d.abs().max())
    del KdT, KgT

    # the shading backward: 192 x 256, a sphere, three terms, maps made earlier
    h, w = 192, 256
    normal, cov = gbuffer_sphere(h, w, (128.0, 96.0), 80.0, device=dev, batch=B)
    maps = prefilter_environment(pano, 32, ("diffuse",))[:, 0], prefilter_environment(pano, 64, (m,))[:, 0]
    kd, ks, km = (torch.full((B, 3, h, w), v, device=dev) for v in (0.7, 0.2, 0.05))
    gs = torch.randn(B, 3, h, w, device=dev)
    ex = torch.full((B,), 0.05, device=dev)
    base = ("kd", "ks", "km", "e_diffuse", "e_phong")

    def shade(want, exposure=None):
        return shade_gbuffer_bwd_raw(gs, pano, maps, normal, cov, kd, ks, km, exposure=exposure, want=want)

    record("shade_bwd_192x256", lambda: shade(base))
    record("shade_bwd_192x256_with_dpano", lambda: shade(base + ("pano",)))
    record("shade_bwd_192x256_coefficients_only", lambda: shade(("kd", "ks", "km")))
    record("insert_object_bwd_192x256_with_dpano", lambda: shade(base + ("pano",), ex))
    r["covered_pixels"] = int(cov[0].sum())
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
