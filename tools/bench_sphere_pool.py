"""SphereMaxPool2D (csrc/sphere_pool.hip) against the stock formulation -- grid_sample into the (B, C, 3H', 3W') tensor, then
max_pool2d(3, 3) -- in one process on one GPU: forward (the HIP forward with its index bytes written) and forward plus backward,
timed with HIP events after warm-up, the two variants alternating over several rounds (median and minimum per call).  Also the
effective rate on the operator's algorithmic bytes: x once, y once, one index byte per output element (forward); plus dy, the
index bytes again and dx once (forward plus backward).  One JSON line per shape.     python tools/bench_sphere_pool.py [rounds]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emlight_amd import _runtime  # noqa: E402
_runtime.entry_point_defaults()
from emlight_amd.GenProjector.spherenet import sphere_max_pool, sphere_sampling_grid  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SHAPES = [(32, 64, 128, 256, 2), (32, 128, 64, 128, 1)]    # B, C, H, W, stride


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    for B, C, H, W, stride in SHAPES:
        x = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
        grid = sphere_sampling_grid(H, W, stride).cuda().expand(B, -1, -1, -1)
        ho, wo = -(-H // stride), -(-W // stride)
        gy = torch.randn(B, C, ho, wo, device="cuda").contiguous(memory_format=torch.channels_last)

        def hip_fwd():
            with torch.no_grad():
                return sphere_max_pool(x, stride, return_indices=True)

        def stock_fwd():
            with torch.no_grad():
                return F.max_pool2d(F.grid_sample(x, grid, mode="bilinear", align_corners=False), 3, 3)

        def hip_both():
            xi = x.detach().requires_grad_(True)
            return torch.autograd.grad(sphere_max_pool(xi, stride), xi, gy)

        def stock_both():
            xi = x.detach().requires_grad_(True)
            return torch.autograd.grad(F.max_pool2d(F.grid_sample(xi, grid, mode="bilinear", align_corners=False), 3, 3), xi, gy)

        fns = {"hip_fwd": hip_fwd, "stock_fwd": stock_fwd, "hip_fwd_bwd": hip_both, "stock_fwd_bwd": stock_both}
        # results first: the two must agree before their times are compared
        err = float((hip_fwd()[0] - stock_fwd()).abs().max())
        gerr = float((hip_both()[0] - stock_both()[0]).norm() / stock_both()[0].norm())
        for fn in fns.values():      # warm-up: code objects, the geometry, the allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k].append(events(fn, 10))
        n_in, n_out = B * C * H * W, B * C * ho * wo
        bytes_fwd = 4 * n_in + 4 * n_out + n_out
        bytes_both = bytes_fwd + 4 * n_out + n_out + 4 * n_in
        row = {"shape": [B, C, H, W, stride], "rounds": ROUNDS, "max_abs_diff_y": err, "rel_l2_diff_dx": gerr,
               "algorithmic_MB": {"fwd": round(bytes_fwd / 1e6, 1), "fwd_bwd": round(bytes_both / 1e6, 1)}}
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4)}
            if k.startswith("hip"):
                row[k]["algorithmic_GB_per_s"] = round((bytes_fwd if k == "hip_fwd" else bytes_both) / med / 1e6, 1)
        row["speedup_fwd"] = round(statistics.median(times["stock_fwd"]) / statistics.median(times["hip_fwd"]), 2)
        row["speedup_fwd_bwd"] = round(statistics.median(times["stock_fwd_bwd"]) / statistics.median(times["hip_fwd_bwd"]), 2)
        print(json.dumps(row), flush=True)
        del x, gy, grid
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
