#!/usr/bin/env python
"""GPU milliseconds of the ground-plane shadow's forward plus backward (eml_ground_shadow_bwd_f32) at
section 28's four configurations, in one process on one box: a 240 x 320 photograph, a 128 x 256 panorama, a level camera one
unit above the floor, K = 1 and K = 16 occluder spheres (``tools/bench_ground_shadow.py``'s two scenes), B = 1 and B = 8.

Per configuration, each a median over `--windows` windows of `--reps` back-to-back calls between two HIP events on torch's
current stream, after a warm-up, the variants taking turns window by window so that they share whatever else the box does:

* ``forward``: ``insert.ground_shadow`` with the image (ratio and shadowed);
* ``backward``: ``insert_grad.ground_shadow_bwd_raw`` with both gradients, for the panorama and the image;
* ``backward_walk``: the same call for the image alone -- the forward's walk without the transpose, the scale pass and dpano:
  ``backward - backward_walk`` is what the adjoint proper costs;
* ``forward_backward``: ``insert_grad.ground_shadow`` and ``backward()`` through autograd;
* ``forward_entry`` and, with ``--parent_lib FILE.so`` (a libemlight_hip.so built from another commit, loaded beside this
  one), ``parent_forward_entry``: ``eml_ground_shadow_f32`` called directly on preallocated buffers through either library,
  the same host path for both.

No test and no threshold rests on these times.

    python tools/bench_ground_shadow_grad.py [--reps 20] [--windows 5] [--parent_lib FILE.so] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_ground_shadow import cluster  # noqa: E402


def _turns(fns, reps, windows, warmup=3):
    """name -> (median, smallest, largest) ms per call; the variants take turns, one window each."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps)
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in out.items()}


def _forward_entry(handle, pano, plane, occ, image, h, w):
    """eml_ground_shadow_f32 through `handle` on buffers made once."""
    from emlight_amd import _lib
    B, _, H, W = pano.shape
    K = occ.shape[1]
    for name in ("eml_ground_shadow_work_floats", "eml_ground_shadow_f32"):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _lib.EXT_SIGNATURES[name]
    work = torch.empty(handle.eml_ground_shadow_work_floats(B, H, h, w, K) // 2 + 1, dtype=torch.float64, device=pano.device)
    ratio, shadowed = torch.empty_like(image), torch.empty_like(image)

    def call():
        rc = handle.eml_ground_shadow_f32(_lib.ptr(pano), B, H, W, _lib.ptr(plane), 4, _lib.ptr(occ), K, h, w, 60.0, 180.0,
                                          _lib.ptr(image), _lib.ptr(ratio), _lib.ptr(shadowed), _lib.ptr(work), _lib.current_stream())
        if rc != 0:
            raise RuntimeError("eml_ground_shadow_f32 returned %d" % rc)
    return call, ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ground_shadow_grad.py needs the MI355X")
    from emlight_amd import _lib, insert, insert_grad
    dev = torch.device("cuda:0")
    H, h, w = 128, 240, 320
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    r = {"H": H, "h": h, "w": w, "device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows,
         "parent_lib": a.parent_lib, "ms": {}}
    for B in (1, 8):
        rng = np.random.default_rng([4, B])
        pano = torch.tensor(rng.random((B, 3, H, 2 * H)) ** 4 * 50 + 0.01, dtype=torch.float32, device=dev)
        image = torch.tensor(rng.random((B, 3, h, w)) ** 4 * 20 + 0.01, dtype=torch.float32, device=dev)
        g_ratio = torch.tensor(rng.standard_normal((B, 3, h, w)), dtype=torch.float32, device=dev)
        g_shadowed = torch.tensor(rng.standard_normal((B, 3, h, w)), dtype=torch.float32, device=dev)
        plane = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * B, dtype=torch.float32, device=dev)
        scenes = {1: insert.sphere_occluder(h, w, (160.0, 150.0), 60.0, 3.0, 60.0, device=dev).expand(B, 1, 4).contiguous(),
                  16: torch.from_numpy(cluster(16)).to(dev)[None].expand(B, 16, 4).contiguous()}
        for K, occ in scenes.items():
            pg, ig = pano.clone().requires_grad_(True), image.clone().requires_grad_(True)

            def both():
                pg.grad = ig.grad = None
                ratio, shadowed = insert_grad.ground_shadow(pg, occ, plane, image=ig)
                torch.autograd.backward([ratio, shadowed], [g_ratio, g_shadowed])
            entry, ratio = _forward_entry(_lib.lib(), pano, plane, occ, image, h, w)
            fns = {"forward_entry": entry}
            if parent is not None:
                fns["parent_forward_entry"], parent_ratio = _forward_entry(parent, pano, plane, occ, image, h, w)
            fns.update({
                "forward": lambda: insert.ground_shadow(pano, occ, plane, image=image),
                "backward": lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, plane, image=image, g_ratio=g_ratio,
                                                                      g_shadowed=g_shadowed, want=("pano", "image")),
                "backward_walk": lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, plane, image=image, g_shadowed=g_shadowed,
                                                                           want=("image",)),
                "forward_backward": both})
            got = _turns(fns, a.reps, a.windows)
            key = "B%d_K%d" % (B, K)
            r["ms"][key] = {name: {"median": round(m, 4), "range": [round(lo, 4), round(hi, 4)]} for name, (m, lo, hi) in got.items()}
            r["ms"][key]["shadowed_pixels"] = int((ratio[:, 0] < 0.999).sum())
            if parent is not None:
                r["ms"][key]["forward_bits_equal_parent"] = bool(torch.equal(ratio, parent_ratio))
            print(key, json.dumps(r["ms"][key]), flush=True)
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
