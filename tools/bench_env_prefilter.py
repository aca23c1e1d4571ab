#!/usr/bin/env python
"""GPU milliseconds of the environment prefilter (eml_env_prefilter_f32 through emlight_amd.insert.prefilter_environment) at
B = 32, 128 x 256, Ho = 64, the diffuse lobe plus one Phong lobe (m = 50), and of the stock formulation of the same two
integrals on the same box in the same process: the (directions x texels) weight tables of both lobes materialised once in
device memory, then one torch.matmul per lobe against the panorama planes.  The table build is not timed; the tables' bytes
are reported.  Also timed: the shading call of a 192 x 256 G-buffer (three terms plus the composite) on maps made earlier.

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls.  No threshold rests on these times: the product path is the HIP kernel either way.

    python tools/bench_env_prefilter.py [--reps 20] [--windows 5] [--out FILE.json]
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


def grid(G, dev):
    """omega (2 G^2, 3) and dOmega (2 G^2,) of the grid of height G, float64 on the device."""
    f64 = dict(dtype=torch.float64, device=dev)
    th = (torch.arange(G, **f64) + 0.5) * np.pi / G
    ph = (torch.arange(2 * G, **f64) + 0.5) * 2 * np.pi / (2 * G)
    om = torch.stack([th.sin()[:, None] * ph.cos()[None, :], th.sin()[:, None] * ph.sin()[None, :],
                      th.cos()[:, None].expand(G, 2 * G)], -1).reshape(2 * G * G, 3)
    return om, (th.sin()[:, None].expand(G, 2 * G) * (np.pi / G) * (2 * np.pi / (2 * G))).reshape(2 * G * G)


def weight_tables(H, Ho, m, dev):
    """The definition's weights as two (2 Ho^2, 2 H^2) float32 tables, built in float64 on the device."""
    om_t, dom = grid(H, dev)
    om_d, _ = grid(Ho, dev)
    x = (om_d @ om_t.T).clamp_min(0)
    return (x * dom / np.pi).float(), (x ** m * dom * ((m + 1) / (2 * np.pi))).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_env_prefilter.py needs the MI355X")
    from emlight_amd.insert import gbuffer_sphere, insert_object, prefilter_environment
    dev = torch.device("cuda:0")
    B, H, Ho, m = a.batch, 128, a.height, 50.0
    W, D, T = 2 * H, 2 * Ho * Ho, 2 * H * H
    g = np.random.default_rng([1, B, Ho])
    pano = torch.tensor(g.random((B, 3, H, W)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    r = {"B": B, "H": H, "W": W, "Ho": Ho, "directions": D, "lobes": ["diffuse", m], "device": torch.cuda.get_device_name(0),
         "reps": a.reps, "windows": a.windows}

    for key, lobes in (("hip_diffuse_phong", ("diffuse", m)), ("hip_diffuse", ("diffuse",)), ("hip_phong", (m,)),
                       ("hip_four_lobes", ("diffuse", m, 10.0, 200.0))):
        med, lo, hi = _ms(lambda: prefilter_environment(pano, Ho, lobes), a.reps, a.windows)
        r["ms_" + key], r["ms_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    # 2 lobes x D x T x 3B multiply-adds
    r["hip_tflops"] = round(2 * 2.0 * D * T * 3 * B / (r["ms_hip_diffuse_phong"] * 1e-3) / 1e12, 2)

    Kd, Kg = weight_tables(H, Ho, m, dev)
    planes = pano.reshape(3 * B, T).t().contiguous()                   # (T, 3B): the GEMM's B operand, made once
    out_d, out_g = torch.empty(D, 3 * B, device=dev), torch.empty(D, 3 * B, device=dev)

    def stock():
        torch.matmul(Kd, planes, out=out_d)
        torch.matmul(Kg, planes, out=out_g)

    med, lo, hi = _ms(stock, a.reps, a.windows)
    r["ms_stock_matmul"], r["ms_stock_matmul_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    r["stock_tflops"] = round(2 * 2.0 * D * T * 3 * B / (med * 1e-3) / 1e12, 2)
    r["stock_table_bytes"] = int(Kd.numel() * 4 + Kg.numel() * 4)
    # the two formulations compute the same numbers
    mine = prefilter_environment(pano, Ho, ("diffuse", m)).reshape(B, 2, 3, D)
    want = torch.stack([out_d, out_g], 0).reshape(2, D, B, 3).permute(2, 0, 3, 1)
    r["max_rel_difference_to_stock"] = float(((mine - want).abs().amax((2, 3)) / want.abs().amax((2, 3))).max())

    # the shading call: 192 x 256, three terms and the composite, maps made earlier
    h, w = 192, 256
    normal, cov = gbuffer_sphere(h, w, (128.0, 96.0), 80.0, device=dev, batch=B)
    maps = prefilter_environment(pano, 32, ("diffuse",))[:, 0], prefilter_environment(pano, 64, (m,))[:, 0]
    bg = torch.rand(B, 3, h, w, device=dev)
    ex = torch.full((B,), 0.05, device=dev)
    kd, ks, km = (torch.full((B, 3, h, w), v, device=dev) for v in (0.7, 0.2, 0.05))
    med, lo, hi = _ms(lambda: insert_object(pano, normal, cov, bg, ex, kd, ks, km, maps=maps), a.reps, a.windows)
    r["ms_insert_object_192x256"], r["ms_insert_object_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    r["covered_pixels"] = int(cov[0].sum())
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
