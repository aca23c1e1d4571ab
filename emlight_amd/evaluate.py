"""Lighting evaluation as in the EMLight papers: light three spheres (diffuse, matte silver, mirror) with a predicted
panorama and with the true one, compare the renders by RMSE, scale-invariant RMSE and RGB angular error.  The reference
tree has no such code; DESIGN.md section 15 is the definition (``csrc/sphere_render.hip``).

    python -m emlight_amd.evaluate --pano_dir DIR --results_dir results [--fov 60] [--size 64] [--batchSize 8] [--out metrics.json]

reads ``results/pred_<name>.npy`` as ``GenProjector.test --pano_dir`` writes them and scores each against the projector's
target for that panorama (``ProjectorPanoramaBatcher(...)(pano, deg=0.0)["warped"]``: the panorama times the tonemap alpha).

``render_spheres`` is differentiable in the panorama (the renders are linear in it; the gradient is the adjoint,
``eml_sphere_render_bwd_f32``), and ``RenderLoss`` is the squared rmse of the renders as a training term: the projector and
joint trainers add it with ``--lambda_render L [--render_size S]``.
"""
import argparse
import functools
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


def _pano_arg(pano, name, phong_exponent):
    x = _lib.require_gpu_tensor(pano, name)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] != 2 * x.shape[2]:
        raise ValueError("%s: expected (B, 3, H, 2H), got %s" % (name, tuple(x.shape)))
    if not float(phong_exponent) >= 0.0:
        raise ValueError("phong_exponent must be >= 0, got %r" % (phong_exponent,))
    return x


def _canonical(names):
    canon = [n for n in MATERIALS if n in names]                  # the kernel's order
    return canon, sum(_BIT[n] for n in canon)


def _render(x, S, mask, M, az, m):
    """The forward's two calls: ``(B, 3, H, W)`` -> ``(B, M, 3, S, S)`` in the kernel's material order."""
    B, _, H, W = x.shape
    out = torch.empty(B, M, 3, S, S, dtype=torch.float32, device=x.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, L.eml_sphere_render_work_floats(B, H, W, S)), dtype=torch.float32, device=x.device)
        _lib.check(L.eml_sphere_render_f32(_lib.ptr(x), B, H, W, S, az, mask, m, _lib.ptr(out), _lib.ptr(work),
                                           _lib.current_stream()), "eml_sphere_render_f32")
    return out


@functools.lru_cache(maxsize=None)
def _inside_count(S):
    return int(sphere_mask(S).sum())                              # on the host: no device synchronisation


_MIRROR_CSR = {}


def _mirror_csr(H, W, S, az, device):
    """The mirror's taps (``eml_sphere_mirror_taps_f32``: four per inside pixel) sorted by texel, as ``SphereGeometry`` sorts
    its ``csr_*``: ``ptr (H W + 1)`` int32, ``src (4P)`` int32 linear pixel indices ``i S + j``, ``w (4P)`` float32.  A stable
    sort, so a texel's entries keep the pixel order and the adjoint adds them in a fixed order.  Built once per geometry."""
    key = (H, W, S, az, device)
    got = _MIRROR_CSR.get(key)
    if got is None:
        P = _inside_count(S)
        idx = torch.zeros(P, 4, dtype=torch.int32, device=device)
        wgt = torch.zeros(P, 4, dtype=torch.float32, device=device)
        _lib.check(_lib.lib().eml_sphere_mirror_taps_f32(H, W, S, az, _lib.ptr(idx), _lib.ptr(wgt), _lib.current_stream()),
                   "eml_sphere_mirror_taps_f32")
        flat = idx.reshape(-1).long()
        order = torch.argsort(flat, stable=True)
        pix = torch.nonzero(sphere_mask(S, device=device).reshape(-1)).reshape(-1)      # row-major: the kernels' pixel list
        ptr = torch.zeros(H * W + 1, dtype=torch.int32, device=device)
        ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=H * W)[:H * W], 0)
        got = _MIRROR_CSR[key] = (ptr, pix[order // 4].to(torch.int32).contiguous(), wgt.reshape(-1)[order].contiguous())
    return got


def _render_adjoint(g, B, H, W, S, mask, az, m):
    """``eml_sphere_render_bwd_f32``: ``g (B, M, 3, S, S)`` in the kernel's material order -> ``(B, 3, H, W)``."""
    g = _lib.require_gpu_tensor(g, "grad_out")
    dpano = torch.empty(B, 3, H, W, dtype=torch.float32, device=g.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, L.eml_sphere_render_bwd_work_floats(B, H, W, S)), dtype=torch.float32, device=g.device)
        csr = _mirror_csr(H, W, S, az, g.device) if mask & _BIT["mirror"] else (None, None, None)
        _lib.check(L.eml_sphere_render_bwd_f32(_lib.ptr(g), B, H, W, S, az, mask, m, _lib.ptr(csr[0]), _lib.ptr(csr[1]),
                                               _lib.ptr(csr[2]), _lib.ptr(dpano), _lib.ptr(work), _lib.current_stream()),
                   "eml_sphere_render_bwd_f32")
    return dpano


class _RenderSpheres(torch.autograd.Function):
    """The renders of ``pano`` and, in the same forward call, of ``truth`` (or None).  The operator is linear, so nothing is
    saved but the geometry; ``truth``'s renders are not differentiable and the adjoint runs over ``pano``'s columns only."""

    @staticmethod
    def forward(ctx, pano, truth, S, mask, M, az, m):
        B, _, H, W = pano.shape
        ctx.geometry = (B, H, W, S, mask, az, m)
        out = _render(pano if truth is None else torch.cat([pano, truth], 0), S, mask, M, az, m)
        if truth is None:
            return out
        a, b = out[:B], out[B:]
        ctx.mark_non_differentiable(b)
        return a, b

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        return (_render_adjoint(g, *ctx.geometry),) + (None,) * 6


def render_spheres(pano, size=64, materials=MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0):
    """``pano`` ``(B, 3, H, W)`` float32 on the device (``W == 2H``, the rasteriser's grid) -> ``(B, M, 3, S, S)``: the sphere
    under each of ``materials`` seen by an orthographic camera that looks towards ``view_azimuth_deg`` (180: the panorama's
    centre column); pixels outside the disc are 0.  ``eml_sphere_render_f32``; only enqueues work, run-to-run exact, and an
    image's render does not depend on the batch it is in.  Differentiable in ``pano`` (``eml_sphere_render_bwd_f32``: the
    adjoint, with the same two properties); an input that does not require grad makes the forward's calls and nothing else."""
    names = _materials(materials)
    S = _size(size)
    x = _pano_arg(pano, "pano", phong_exponent)
    canon, mask = _canonical(names)
    args = (S, mask, len(canon), float(view_azimuth_deg), float(phong_exponent))
    if torch.is_grad_enabled() and x.requires_grad:
        out = _RenderSpheres.apply(x, None, *args)
    else:
        out = _render(x, *args)
    if list(names) != canon:
        out = torch.stack([out[:, canon.index(n)] for n in names], 1)     # slices, not an index tensor: no host-to-device copy
    return out


class RenderLoss(torch.nn.Module):
    """What the evaluation scores, as a training term: the mean over images and ``materials`` of ``sum (a - b)^2 / 3P`` with
    ``a``, ``b`` the sphere renders of the prediction and of the truth and ``P`` the inside pixels -- the square of
    ``render_metrics``' rmse.  Both batches go through ONE render call of ``2B`` images; the truth gets no gradient and the
    adjoint kernel runs over the prediction's ``3B`` columns only.  After the first call of a geometry (the mirror's tap
    table) a forward plus backward only enqueues work."""

    def __init__(self, size=32, materials=("diffuse", "glossy"), view_azimuth_deg=180.0, phong_exponent=50.0):
        super().__init__()
        self.size, self.materials = _size(size), _materials(materials)
        self.view_azimuth_deg, self.phong_exponent = float(view_azimuth_deg), float(phong_exponent)
        if not self.phong_exponent >= 0.0:
            raise ValueError("phong_exponent must be >= 0, got %r" % (phong_exponent,))

    def forward(self, pred, true):
        p = _pano_arg(pred, "pred", self.phong_exponent)
        t = _pano_arg(true, "true", self.phong_exponent)
        if p.shape != t.shape or p.shape[0] < 1:
            raise ValueError("pred %s and true %s: expected two equal shapes (B, 3, H, 2H) with B >= 1"
                             % (tuple(p.shape), tuple(t.shape)))
        canon, mask = _canonical(self.materials)
        B, M = p.shape[0], len(canon)
        args = (self.size, mask, M, self.view_azimuth_deg, self.phong_exponent)
        if torch.is_grad_enabled() and p.requires_grad:
            a, b = _RenderSpheres.apply(p, t.detach(), *args)
        else:
            r = _render(torch.cat([p, t], 0), *args)
            a, b = r[:B], r[B:]
        d = a - b                                                         # 0 outside the disc: both renders are
        return (d * d).sum() / (3.0 * _inside_count(self.size) * B * M)


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
    with torch.no_grad():                                             # scores, not a training term: see RenderLoss
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
