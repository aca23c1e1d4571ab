#!/usr/bin/env python
"""GPU milliseconds of the render loss's backward call (eml_sphere_render_bwd_f32 through emlight_amd.evaluate: the adjoint of
the sphere renders) at B = 32, 128 x 256, S = 64 and S = 32, diffuse + glossy (RenderLoss's default materials; the three
materials are timed too), against two baselines on the same box in the same process:

(a) the forward call of the same shape and materials at this commit (eml_sphere_render_f32);
(b) the stock formulation: both (pixels x texels) weight tables materialised once in device memory, then one torch.matmul
    per material against the gradient operand (3B x P), the second accumulating into the first's result.  The table build
    is not timed; the tables' bytes are reported.

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls.  No threshold rests on these times: the product path is the HIP kernel either way.

    python tools/bench_sphere_render_bwd.py [--reps 20] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sphere_render import _ms, weight_tables  # noqa: E402


def one_size(B, H, W, S, reps, windows, dev):
    from emlight_amd import evaluate
    from emlight_amd.evaluate import MATERIALS, sphere_mask
    P = int(sphere_mask(S).sum())
    g = np.random.default_rng([2, B, S])
    pano = torch.tensor(g.random((B, 3, H, W)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    r = {"S": S, "inside_pixels": P}
    inside = sphere_mask(S, device=dev)
    for key, mats in (("diffuse_glossy", MATERIALS[:2]), ("three_materials", MATERIALS)):
        M = len(mats)
        mask = sum(evaluate._BIT[n] for n in mats)
        grad = torch.tensor(g.standard_normal((B, M, 3, S, S)), dtype=torch.float32, device=dev)
        args = (S, mask, M, 180.0, 50.0)
        evaluate._render_adjoint(grad, B, H, W, S, mask, 180.0, 50.0)            # the mirror's tap table, once
        med, lo, hi = _ms(lambda: evaluate._render_adjoint(grad, B, H, W, S, mask, 180.0, 50.0), reps, windows)
        r["ms_hip_backward_" + key], r["ms_hip_backward_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        med, lo, hi = _ms(lambda: evaluate._render(pano, *args), reps, windows)
        r["ms_hip_forward_" + key], r["ms_hip_forward_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    # 2 materials x P x (H W) x 3B multiply-adds
    r["hip_backward_tflops"] = round(2 * 2.0 * P * H * W * 3 * B / (r["ms_hip_backward_diffuse_glossy"] * 1e-3) / 1e12, 2)

    Kd, Kg = weight_tables(H, W, S, 180.0, 50.0, dev)
    grad = torch.tensor(g.standard_normal((B, 2, 3, S, S)), dtype=torch.float32, device=dev)
    gd = grad[:, 0][:, :, inside].reshape(3 * B, P).contiguous()                  # (3B, P): the GEMM's A operand, made once
    gg = grad[:, 1][:, :, inside].reshape(3 * B, P).contiguous()
    out = torch.empty(3 * B, H * W, device=dev)

    def stock():
        torch.matmul(gd, Kd, out=out)
        out.addmm_(gg, Kg)

    med, lo, hi = _ms(stock, reps, windows)
    r["ms_stock_matmul_diffuse_glossy"], r["ms_stock_matmul_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    r["stock_table_bytes"] = int(Kd.numel() * 4 + Kg.numel() * 4)
    # the two formulations compute the same numbers
    mine = evaluate._render_adjoint(grad, B, H, W, S, 3, 180.0, 50.0).reshape(B, 3 * H * W)
    want = out.reshape(B, 3 * H * W)
    r["max_rel_difference_to_stock"] = float(((mine - want).abs().amax(1) / want.abs().amax(1)).max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sphere_render_bwd.py needs the MI355X")
    dev = torch.device("cuda:0")
    B, H, W = a.batch, 128, 256
    r = {"B": B, "H": H, "W": W, "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows,
         "sizes": [one_size(B, H, W, S, a.reps, a.windows, dev) for S in a.sizes]}
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
