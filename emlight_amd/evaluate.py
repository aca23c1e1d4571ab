"""Lighting evaluation as in the EMLight papers: light three spheres (diffuse, matte silver, mirror) with a predicted
panorama and with the true one, compare the renders by RMSE, scale-invariant RMSE and RGB angular error.  The reference
tree has no such code; DESIGN.md section 15 is the definition (``csrc/sphere_render.hip``).

    python -m emlight_amd.evaluate --pano_dir DIR --results_dir results [--fov 60] [--size 64] [--batchSize 8] [--out metrics.json]

reads ``results/pred_<name>.npy`` as ``GenProjector.test --pano_dir`` writes them and scores each against the projector's
target for that panorama (``ProjectorPanoramaBatcher(...)(pano, deg=0.0)["warped"]``: the panorama times the tonemap alpha).
"""
import argparse
import json
import os

import numpy as np
import torch

from . import _lib

MATERIALS = ("diffuse", "glossy", "mirror")
_BIT = {"diffuse": 1, "glossy": 2, "mirror": 4}     # EML_SPHERE_* of include/emlight_hip.h
METRICS = ("rmse", "si_rmse", "angular", "used")


def _materials(materials):
    if isinstance(materials, str):
        materials = (materials,)
    names = tuple(materials)
    if not names or len(set(names)) != len(names) or any(n not in _BIT for n in names):
        raise ValueError("materials: expected distinct names out of %s, got %r" % (MATERIALS, materials))
    return names


def _size(size):
    if int(size) != size or int(size) < 2:
        raise ValueError("size: expected an integer >= 2, got %r" % (size,))
    return int(size)


def sphere_mask(size, device=None):
    """``(S, S)`` bool: pixel (row i, column j) is inside the sphere's disc iff ``(2j + 1 - S)^2 + (S - 1 - 2i)^2 < S^2`` --
    an integer test, so the mask is exact; the kernels evaluate the same one."""
    S = _size(size)
    k = torch.arange(S, dtype=torch.int64, device=device)
    X, Y = 2 * k + 1 - S, S - 1 - 2 * k
    return (X * X)[None, :] + (Y * Y)[:, None] < S * S


def render_spheres(pano, size=64, materials=MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0):
    """``pano`` ``(B, 3, H, W)`` float32 on the device (``W == 2H``, the rasteriser's grid) -> ``(B, M, 3, S, S)``: the sphere
    under each of ``materials`` seen by an orthographic camera that looks towards ``view_azimuth_deg`` (180: the panorama's
    centre column); pixels outside the disc are 0.  ``eml_sphere_render_f32``; only enqueues work, run-to-run exact, and an
    image's render does not depend on the batch it is in."""
    names = _materials(materials)
    S = _size(size)
    x = _lib.require_gpu_tensor(pano, "pano")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] != 2 * x.shape[2]:
        raise ValueError("pano: expected (B, 3, H, 2H), got %s" % (tuple(x.shape),))
    if not float(phong_exponent) >= 0.0:
        raise ValueError("phong_exponent must be >= 0, got %r" % (phong_exponent,))
    B, _, H, W = x.shape
    canon = [n for n in MATERIALS if n in names]                  # the kernel's order
    mask = sum(_BIT[n] for n in canon)
    out = torch.empty(B, len(canon), 3, S, S, dtype=torch.float32, device=x.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, L.eml_sphere_render_work_floats(B, H, W, S)), dtype=torch.float32, device=x.device)
        _lib.check(L.eml_sphere_render_f32(_lib.ptr(x), B, H, W, S, float(view_azimuth_deg), mask, float(phong_exponent),
                                           _lib.ptr(out), _lib.ptr(work), _lib.current_stream()), "eml_sphere_render_f32")
    if list(names) != canon:
        out = torch.stack([out[:, canon.index(n)] for n in names], 1)     # slices, not an index tensor: no host-to-device copy
    return out


def render_metrics(pred_render, true_render):
    """Two ``(B, M, 3, S, S)`` render tensors -> ``(B, M, 4)`` float64: rmse, si_rmse, angular (degrees), used
    (``eml_sphere_render_metrics_f64``; sums in float64 over the inside pixels, fixed order)."""
    a = _lib.require_gpu_tensor(pred_render, "pred_render")
    b = _lib.require_gpu_tensor(true_render, "true_render")
    if a.dim() != 5 or a.shape[2] != 3 or a.shape[3] != a.shape[4] or not 1 <= a.shape[1] <= 3 or a.shape[3] < 2:
        raise ValueError("pred_render: expected (B, M, 3, S, S) with M in 1..3, got %s" % (tuple(a.shape),))
    if a.shape != b.shape:
        raise ValueError("pred_render %s and true_render %s differ in shape" % (tuple(a.shape), tuple(b.shape)))
    B, M, _, S, _ = a.shape
    out = torch.empty(B, M, 4, dtype=torch.float64, device=a.device)
    if B > 0:
        _lib.check(_lib.lib().eml_sphere_render_metrics_f64(_lib.ptr(a), _lib.ptr(b), B, M, S, _lib.ptr(out),
                                                            _lib.current_stream()), "eml_sphere_render_metrics_f64")
    return out


def lighting_metrics(pred, true, size=64, materials=MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0):
    """Predicted and true panoramas ``(B, 3, H, W)`` -> ``{"<material>/rmse" | "/si_rmse" | "/angular" | "/used": (B,) float64
    device tensors}``.  Both batches go through one render call (the weights of a pixel row are built once for both); no
    host synchronisation."""
    names = _materials(materials)
    p = _lib.require_gpu_tensor(pred, "pred")
    t = _lib.require_gpu_tensor(true, "true")
    if p.shape != t.shape:
        raise ValueError("pred %s and true %s differ in shape" % (tuple(p.shape), tuple(t.shape)))
    B = p.shape[0] if p.dim() == 4 else 0
    r = render_spheres(torch.cat([p, t], 0), size, names, view_azimuth_deg, phong_exponent)
    m = render_metrics(r[:B], r[B:])
    return {"%s/%s" % (n, k): m[:, i, j] for i, n in enumerate(names) for j, k in enumerate(METRICS)}


# ------------------------------------------------------------------------------------------------ command line
def _batcher(fov, device):
    from .GenProjector.data import ProjectorPanoramaBatcher
    return ProjectorPanoramaBatcher(fov_deg=fov, device=device)


def evaluate_directory(pano_dir, results_dir, fov=60.0, size=64, batch_size=8, device="cuda:0"):
    """Every panorama of ``pano_dir`` in name order (as ``GenProjector.test.run_panoramas`` walks them) against
    ``results_dir/pred_<name>.npy``; a missing prediction is reported by name and skipped."""
    from torch.utils.data import DataLoader
    from .RegressionNetwork.data import PanoramaDataset
    loader = DataLoader(PanoramaDataset(pano_dir), batch_size=batch_size, shuffle=False, drop_last=False)
    batcher = _batcher(fov, device)
    images, skipped = {}, []
    for para in loader:
        truth = batcher(para["pano"].to(device), deg=0.0)["warped"]
        keep, preds = [], []
        for j, name in enumerate(para["name"]):
            path = os.path.join(results_dir, "pred_%s.npy" % name)
            if not os.path.exists(path):
                print("missing prediction, skipped: %s" % path)
                skipped.append(name)
                continue
            a = np.asarray(np.load(path), dtype=np.float32)
            a = a.reshape((-1,) + a.shape[-3:]) if a.ndim in (3, 4) else a
            if a.shape != (1,) + tuple(truth.shape[1:]):
                raise ValueError("%s: expected %s, got %s" % (path, (1,) + tuple(truth.shape[1:]), a.shape))
            keep.append(j)
            preds.append(a)
        if not keep:
            continue
        pred = torch.from_numpy(np.concatenate(preds, 0)).to(device)
        met = lighting_metrics(pred, truth[keep].contiguous(), size=size)
        host = {k: v.cpu().numpy() for k, v in met.items()}
        for q, j in enumerate(keep):
            images[para["name"][j]] = {k: float(v[q]) for k, v in host.items()}
    keys = ["%s/%s" % (n, k) for n in MATERIALS for k in METRICS]
    means = {k: (float(np.mean([im[k] for im in images.values()])) if images else None) for k in keys}
    return {"pano_dir": pano_dir, "results_dir": results_dir, "fov": fov, "size": size, "materials": list(MATERIALS),
            "evaluated": len(images), "skipped": len(skipped), "skipped_names": skipped, "images": images, "means": means}


def print_table(result):
    print("%-8s %12s %12s %12s" % ("", "rmse", "si_rmse", "angular/deg"))
    for n in result["materials"]:
        row = [result["means"]["%s/%s" % (n, k)] for k in METRICS[:3]]
        print("%-8s %s" % (n, " ".join("%12s" % ("-" if v is None else "%.6g" % v) for v in row)))
    print("%d images evaluated, %d skipped" % (result["evaluated"], result["skipped"]))


def main(argv=None, device=None):
    ap = argparse.ArgumentParser(description="sphere-render lighting metrics of pred_<name>.npy against a panorama directory")
    ap.add_argument("--pano_dir", required=True)
    ap.add_argument("--results_dir", default="results")
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batchSize", type=int, default=8)
    ap.add_argument("--out", default=None, help="write the per-image values and the means as JSON")
    args = ap.parse_args(argv)
    from . import _runtime
    _runtime.entry_point_defaults()
    result = evaluate_directory(args.pano_dir, args.results_dir, args.fov, args.size, args.batchSize, device or "cuda:0")
    print_table(result)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
