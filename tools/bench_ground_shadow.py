#!/usr/bin/env python
"""GPU milliseconds of the ground-plane shadow (eml_ground_shadow_f32: three launches) at the workload's
size, in one process on one box: a 240 x 320 photograph, a 128 x 256 panorama, a level camera one unit above the floor,

* K = 1: the sphere of ``--sphere 160 150 60 --depth 3`` (``sphere_occluder``), resting a little above the floor;
* K = 16: a cluster of sixteen overlapping spheres of mixed sizes standing on the floor about three units away.

Beside each time: the ray-sphere tests a kernel without culling would execute (pixels x texels x K), that count per second
of the measured time -- a lower bound of the rate such a kernel would need to be as fast.  With a library built with
-DEML_GROUND_SHADOW_COUNTS (its waves count the texels they walk, 64 lanes each, behind the sums in the scratch buffer) also the
tests the kernel did execute and the share of tests culling skipped; the times are then that build's:

    tools/exp_build.sh counts -DEML_GROUND_SHADOW_COUNTS && EML_LIB_PATH=build_exp/lib_counts.so python tools/bench_ground_shadow.py

Back to back between two HIP events on torch's current stream, after a warm-up; a figure is the median over `--windows`
windows of `--reps` calls, with the smallest and the largest window beside it.  No test and no threshold rests on these times.

    python tools/bench_ground_shadow.py [--reps 20] [--windows 5] [--batch 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_env_prefilter import _ms  # noqa: E402


def cluster(K, seed=3):
    """K overlapping spheres standing on the floor y = -1 about (0, ., -3): an object's sphere-set proxy."""
    g = np.random.default_rng(seed)
    r = 0.12 + 0.2 * g.random(K)
    x, z = 0.45 * (g.random(K) - 0.5), -3.0 + 0.45 * (g.random(K) - 0.5)
    y = -1.0 + r + 0.5 * g.random(K) * (np.arange(K) % 2)                    # every other one stacked higher
    return np.stack([x, y, z, r], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ground_shadow.py needs the MI355X")
    from emlight_amd import _lib
    from emlight_amd.insert import ground_shadow, sphere_occluder
    dev = torch.device("cuda:0")
    B, H, h, w = a.batch, 128, 240, 320
    rng = np.random.default_rng([4, B])
    pano = torch.tensor(rng.random((B, 3, H, 2 * H)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
    image = torch.tensor(rng.random((B, 3, h, w)) ** 4 * 20 + 0.01, dtype=torch.float32, device=dev)
    plane = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * B, dtype=torch.float32, device=dev)
    scenes = {1: sphere_occluder(h, w, (160.0, 150.0), 60.0, 3.0, 60.0, device=dev).expand(B, 1, 4).contiguous(),
              16: torch.from_numpy(cluster(16)).to(dev)[None].expand(B, 16, 4).contiguous()}
    r = {"B": B, "H": H, "h": h, "w": w, "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows}
    L = _lib.lib()
    for K, occ in scenes.items():
        med, lo, hi = _ms(lambda: ground_shadow(pano, occ, plane, image=image), a.reps, a.windows)
        # the executed tests: one call of the entry point on a scratch buffer that is read back
        floats = L.eml_ground_shadow_work_floats(B, H, h, w, K)
        work = torch.zeros(floats // 2, dtype=torch.float64, device=dev)
        ratio = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
        _lib.check(L.eml_ground_shadow_f32(_lib.ptr(pano), B, H, 2 * H, _lib.ptr(plane), 4, _lib.ptr(occ), K, h, w, 60.0, 180.0, None,
                                           _lib.ptr(ratio), None, _lib.ptr(work), _lib.current_stream()), "eml_ground_shadow_f32")
        waves = B * ((h + 15) // 16) * ((w + 15) // 16) * 4
        counted = floats // 2 == B * 3 * (1 + (2 * H * H + 255) // 256 + 2 * H * H) + waves    # a counting build asks for more
        executed = int(work[-waves:].view(torch.int64).sum()) if counted else None
        full = B * h * w * 2 * H * H * K
        key = "K%d" % K
        r["ms_" + key], r["ms_" + key + "_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        r["tests_no_culling_" + key], r["tests_executed_" + key] = full, executed
        r["no_culling_tests_per_s_" + key] = float("%.4g" % (full / (med * 1e-3)))
        r["share_skipped_" + key] = round(1.0 - executed / full, 4) if counted else None
        r["shadowed_pixels_" + key] = int((ratio[:, 0] < 0.999).sum())
        r["smallest_ratio_" + key] = round(float(ratio.min()), 4)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
