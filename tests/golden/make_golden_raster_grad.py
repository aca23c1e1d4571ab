#!/usr/bin/env python
"""Generate tests/golden/rasteriser_grad.npz: the REFERENCE's gradients of convert_to_panorama wrt all three inputs (CPU, f32).

Run only in the build container, where the reference checkout exists (see make_golden.py):

    python tests/golden/make_golden_raster_grad.py

The reference's ``convert_to_panorama`` (``RegressionNetwork/util.py:222-245``; ``GenProjector/util.py`` holds an identical
copy and is the one make_golden.py's ``gen_rasteriser`` loads, by file path, with the I/O modules stubbed and ``.cuda()`` a
no-op) is plain torch arithmetic: its f32 autograd gives d/d dirs, d/d sizes and d/d colors of ``(pano * w).sum()`` for a
fixed random weight map ``w``.  The reference hard-codes 128 x 256, so every case is at that size.  Stored: the inputs, ``w``
(as int8 quarter steps: ``w = w_q / 4``) and the three gradients; arrays only.  The GPU tests read only the ``.npz``.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference location, shims and the rasteriser's input recipe)


def ref_convert_to_panorama():
    mg.stub_io_modules()
    spec = importlib.util.spec_from_file_location("ref_gp_util", os.path.join(mg.REF, "GenProjector", "util.py"))
    gp_util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp_util)
    return gp_util.convert_to_panorama


def gen_rasteriser_grad():
    convert = ref_convert_to_panorama()
    _, gutils = mg.ref_geomloss()
    out = {}
    for name, B, n in [("anchors_b2_n128", 2, 128), ("random_b3_n42", 3, 42)]:
        dirs, sizes, colors = mg.raster_inputs(B, n, 21, gutils.sphere_points(n))
        if name.startswith("random"):   # varied lobe widths + off-anchor directions
            g = mg.rng(22)
            sizes = g.uniform(0.002, 0.3, sizes.shape).astype(np.float32)
            d = g.standard_normal((B, n, 3))
            dirs = (d / np.linalg.norm(d, axis=2, keepdims=True)).reshape(B, 3 * n).astype(np.float32)
        w_q = mg.rng(23, B, n).integers(-8, 9, (B, 3, 128, 256)).astype(np.int8)
        w = torch.from_numpy(w_q.astype(np.float32) / 4)
        t = [torch.from_numpy(v).requires_grad_(True) for v in (dirs, sizes, colors)]
        (convert(*t) * w).sum().backward()
        out[name + "/dirs"], out[name + "/sizes"], out[name + "/colors"] = dirs, sizes, colors
        out[name + "/w_q"] = w_q
        out[name + "/gdirs"], out[name + "/gsizes"], out[name + "/gcolors"] = (v.grad.numpy() for v in t)
        print("raster grad", name, " ".join("|g%s| max %.4g" % (k, float(v.grad.abs().max()))
                                             for k, v in zip(("dirs", "sizes", "colors"), t)))
    np.savez_compressed(os.path.join(HERE, "rasteriser_grad.npz"), **out)


if __name__ == "__main__":
    mg.install_shims()
    gen_rasteriser_grad()
