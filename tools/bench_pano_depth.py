#!/usr/bin/env python
"""GPU milliseconds of the depth-aware panorama warp, in one process on one box:

* eml_pano_warp_depth_f32 at (B, H, W) = (32, 128, 256) -> (128, 256), steps 32, bisections 24, one (theta, phi, move) per sample,
  on a box room with per-sample depth scales, panorama and depth out, and depth alone.  (The section's comparison with a kernel
  that kept the depth map in LDS was made with this tool on a library that still had both; EML_LIB_PATH selects a library.);
* eml_pano_warp_f32 at the same shape and parameters: one position and one lookup per pixel, the yardstick per lookup;
* a PanoramaBatcher call on 256 x 512 sources at the same batch, without and with depth panoramas, without and with a warp: what
  the depth path adds to a training batch.

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls, with the smallest and the largest window beside it.  No test and no threshold rests on these times.

    python tools/bench_pano_depth.py [--reps 20] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_env_prefilter import _ms  # noqa: E402


def room_depth(H, W, lo=(-1.5, -2.0, -2.5), hi=(1.2, 3.0, 2.0)):
    """The distance from the origin to the walls of an axis-aligned box along the pixel directions of the warp's grid."""
    lat = (np.arange(H) * np.pi / H - np.pi / 2)[:, None]
    lon = (np.arange(W) * 2 * np.pi / W)[None, :]
    d = np.stack([np.sin(lat) + 0 * lon, np.sin(lon) * np.cos(lat), -np.cos(lon) * np.cos(lat)], -1)
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, np.array(hi) / d, np.where(d < 0, np.array(lo) / d, np.inf))
    return t.min(-1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--bisections", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pano_depth.py needs the MI355X")
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    dev = torch.device("cuda:0")
    B, H, W = a.batch, 128, 256
    rng = np.random.default_rng([3, B])
    scale = torch.tensor(rng.uniform(0.8, 1.6, B), dtype=torch.float32, device=dev)
    depth = torch.from_numpy(room_depth(H, W)).to(dev)[None] * scale[:, None, None]
    pano = torch.tensor(rng.random((B, H, W, 3)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    prm = torch.tensor(np.stack([rng.uniform(-20, 20, B), rng.uniform(-180, 180, B), rng.uniform(-0.8, 0.0, B)], 1),
                       dtype=torch.float64, device=dev)
    kw = dict(theta=prm[:, 0], phi=prm[:, 1], move=prm[:, 2])
    r = {"B": B, "H": H, "W": W, "steps": a.steps, "bisections": a.bisections, "device": torch.cuda.get_device_name(0),
         "reps": a.reps, "windows": a.windows, "lib": os.environ.get("EML_LIB_PATH", "")}

    def record(key, fn):
        med, lo, hi = _ms(fn, a.reps, a.windows)
        r["ms_" + key], r["ms_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        return med

    def depth_warp(with_pano=True):
        return PanoramaHandler.warp_panorama_depth(pano if with_pano else None, depth, None, steps=a.steps, bisections=a.bisections,
                                                   **kw)

    r["valid_samples"] = int(torch.isfinite(depth_warp()[1]).all(dim=(1, 2)).sum())
    record("depth_warp", depth_warp)
    record("unit_sphere_warp", lambda: PanoramaHandler.warp_panorama(pano, None, **kw))
    record("depth_warp_again", depth_warp)                             # the spread between two looks at the same kernel
    record("depth_warp_depth_only", lambda: depth_warp(False))

    # a batcher call: 256 x 512 sources
    big = torch.tensor(rng.random((B, 256, 512, 3)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    big_d = torch.from_numpy(room_depth(256, 512)).to(dev)[None] * scale[:, None, None]
    bt = PanoramaBatcher(anchors=96, crop_hw=(192, 256), fov_deg=60.0, device=dev)
    deg = torch.tensor(rng.uniform(0, 360, B), dtype=torch.float64, device=dev)
    warp = torch.stack([torch.zeros_like(prm[:, 2]), torch.zeros_like(prm[:, 2]), prm[:, 2]], 1)
    record("batcher", lambda: bt(big, deg=deg))
    record("batcher_unit_sphere_warp", lambda: bt(big, deg=deg, warp=warp))
    record("batcher_depth", lambda: bt(big, deg=deg, depth_panos=big_d))
    record("batcher_depth_warp", lambda: bt(big, deg=deg, warp=warp, depth_panos=big_d))
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
