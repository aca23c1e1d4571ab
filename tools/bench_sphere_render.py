#!/usr/bin/env python
"""GPU milliseconds of the lighting evaluation's sphere renders (eml_sphere_render_f32 through
emlight_amd.evaluate.render_spheres) at B = 32, 128 x 256, S = 64, three materials, and of the stock formulation of the
same two integrals on the same box: the (pixels x texels) weight tables of the diffuse and the glossy sphere materialised
once in device memory, then one torch.matmul per material against the panorama planes.  The table build is not timed; the
tables' bytes are reported.  The stock mirror is not built: the figure that matters is the integrals'.

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls.  No threshold rests on these times: the product path is the HIP kernel either way.

    python tools/bench_sphere_render.py [--reps 20] [--windows 5] [--out FILE.json]
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


def weight_tables(H, W, S, view_azimuth_deg, m, dev):
    """The definition's weights as two (P, H W) float32 tables, built in float64 on the device."""
    f64 = dict(dtype=torch.float64, device=dev)
    th = (torch.arange(H, **f64) + 0.5) * np.pi / H
    ph = (torch.arange(W, **f64) + 0.5) * 2 * np.pi / W
    om = torch.stack([th.sin()[:, None] * ph.cos()[None, :], th.sin()[:, None] * ph.sin()[None, :],
                      th.cos()[:, None].expand(H, W)], -1).reshape(H * W, 3)
    dom = (th.sin()[:, None].expand(H, W) * (np.pi / H) * (2 * np.pi / W)).reshape(H * W)
    pc = np.deg2rad(view_azimuth_deg)
    r = torch.tensor([-np.sin(pc), np.cos(pc), 0.0], **f64)
    u = torch.tensor([0.0, 0.0, 1.0], **f64)
    v = torch.tensor([-np.cos(pc), -np.sin(pc), 0.0], **f64)
    k = torch.arange(S, device=dev)
    X, Y = 2 * k + 1 - S, S - 1 - 2 * k
    ii, jj = torch.nonzero((X * X)[None, :] + (Y * Y)[:, None] < S * S, as_tuple=True)
    px, py = X[jj].double() / S, Y[ii].double() / S
    nz = (1 - px * px - py * py).sqrt()
    n = px[:, None] * r + py[:, None] * u + nz[:, None] * v
    R = 2 * nz[:, None] * n - v
    Kd = ((n @ om.T).clamp_min(0) * dom / np.pi).float()
    Kg = ((R @ om.T).clamp_min(0) ** m * dom * ((m + 1) / (2 * np.pi))).float()
    return Kd, Kg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sphere_render.py needs the MI355X")
    from emlight_amd.evaluate import MATERIALS, render_spheres, sphere_mask
    dev = torch.device("cuda:0")
    B, H, W, S = a.batch, 128, 256, a.size
    g = np.random.default_rng([1, B, S])
    pano = torch.tensor(g.random((B, 3, H, W)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    P = int(sphere_mask(S).sum())
    r = {"B": B, "H": H, "W": W, "S": S, "inside_pixels": P, "device": torch.cuda.get_device_name(0), "reps": a.reps,
         "windows": a.windows}

    for key, mats in (("hip_three_materials", MATERIALS), ("hip_diffuse_glossy", MATERIALS[:2]), ("hip_mirror", MATERIALS[2:])):
        med, lo, hi = _ms(lambda: render_spheres(pano, size=S, materials=mats), a.reps, a.windows)
        r["ms_" + key], r["ms_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    # 2 materials x P x (H W) x 3B multiply-adds
    r["hip_integral_tflops"] = round(2 * 2.0 * P * H * W * 3 * B / (r["ms_hip_diffuse_glossy"] * 1e-3) / 1e12, 2)

    Kd, Kg = weight_tables(H, W, S, 180.0, 50.0, dev)
    planes = pano.reshape(3 * B, H * W).t().contiguous()               # (H W, 3B): the GEMM's B operand, made once
    out_d, out_g = torch.empty(P, 3 * B, device=dev), torch.empty(P, 3 * B, device=dev)

    def stock():
        torch.matmul(Kd, planes, out=out_d)
        torch.matmul(Kg, planes, out=out_g)

    med, lo, hi = _ms(stock, a.reps, a.windows)
    r["ms_stock_matmul_diffuse_glossy"], r["ms_stock_matmul_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    r["stock_table_bytes"] = int(Kd.numel() * 4 + Kg.numel() * 4)
    # the two formulations compute the same numbers
    mine = render_spheres(pano, size=S, materials=MATERIALS[:2])
    inside = sphere_mask(S, device=dev)
    got = mine[:, :, :, inside]                                         # (B, 2, 3, P)
    want = torch.stack([out_d, out_g], 0).reshape(2, P, B, 3).permute(2, 0, 3, 1)
    r["max_rel_difference_to_stock"] = float(((got - want).abs().amax((2, 3)) / want.abs().amax((2, 3))).max())
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
