"""Object insertion: light a virtual object with a (predicted) panorama and put it into the photograph -- what lighting
estimation is for (the reference's README; its tree has no code for the step).  DESIGN.md section 22 is the definition,
``tests/insert_oracle.py`` restates it in float64.

* ``prefilter_environment``: the panorama integrated against cosine and Phong lobes on an output grid
  (``csrc/env_prefilter.hip``: an implicit GEMM on the f32 MFMA).  The maps are a product of their own: an irradiance map
  and specular maps are what a real-time renderer takes.
* ``shade_gbuffer`` / ``composite`` / ``insert_object``: every covered pixel of a G-buffer (camera-space normals, coverage,
  ``kd``, ``ks``, ``km``) lit by three lookups and composited over the photograph (``csrc/gbuffer_shade.hip``).
* ``gbuffer_sphere``: the G-buffer of a sphere drawn as section 15 draws it, at a pixel position.
* ``ground_shadow``: the shadow the object, given as a few occluder spheres, casts on a ground plane: per pixel of the
  plane the panorama's irradiance with the spheres in the way over the irradiance without them (``csrc/ground_shadow.hip``,
  DESIGN.md section 28; ``tests/shadow_oracle.py``).  ``sphere_occluder`` is the occluder that goes with ``gbuffer_sphere``.

Forward only: a tensor that requires grad is refused (``emlight_amd.insert_grad`` is the differentiable interface).
Everything only enqueues work.

    python -m emlight_amd.insert --pano pred.npy --image crop.npy --gbuffer DIR --fov 60 [--exposure A] [--out out.npy]
    python -m emlight_amd.insert --pano pred.npy --image crop.npy --sphere CX CY RADIUS [--kd 0.8 --ks 0.2 --km 0]
    python -m emlight_amd.insert ... --ground HEIGHT [--ground_normal NX NY NZ] [--depth Z] [--occluders FILE.npy]

``DIR`` holds ``normal.npy`` (3, h, w), ``coverage.npy`` (h, w) or (1, h, w) and any of ``kd.npy``, ``ks.npy``, ``km.npy``
(3, h, w); the image is the HDR crop (3, h, w).  Without ``--exposure`` the scale is ``TonemapHDR``'s alpha of the image,
raised to gamma so that the object is tonemapped exactly as the photograph is.  ``--ground HEIGHT`` puts a ground plane
``HEIGHT`` below the camera (normal ``--ground_normal``, default straight up) and multiplies the HDR image by the shadow ratio
before it is tonemapped; the exposure is still the unshadowed image's.  The occluder is the sphere itself, ``--depth Z`` away
along its centre's ray (``--sphere``), or the ``(K, 4)`` camera-space spheres of ``--occluders`` (``--gbuffer``).
"""
import argparse
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

DIFFUSE = "diffuse"
MAX_LOBES = 8
MAX_OCCLUDERS = 16


def _forward_only(t, name):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise ValueError("%s requires grad: emlight_amd.insert is forward only (emlight_amd.insert_grad has the gradients of "
                         "pano, maps, kd, ks, km and shaded); pass %s.detach()" % (name, name))
    return t


def _lobes(lobes):
    if isinstance(lobes, (str, int, float)):
        lobes = (lobes,)
    vals = []
    for lb in tuple(lobes):
        if isinstance(lb, str):
            if lb != DIFFUSE:
                raise ValueError("lobes: a lobe is %r or a Phong exponent >= 0, got %r" % (DIFFUSE, lb))
            vals.append(-1.0)
        else:
            m = float(lb)
            if not (0.0 <= m <= 1e6):
                raise ValueError("lobes: a lobe is %r or a Phong exponent in [0, 1e6], got %r" % (DIFFUSE, lb))
            vals.append(m)
    if not 1 <= len(vals) <= MAX_LOBES:
        raise ValueError("lobes: expected 1..%d lobes, got %d" % (MAX_LOBES, len(vals)))
    return vals


def _height(v, name):
    if int(v) != v or not 1 <= int(v) <= 1024:
        raise ValueError("%s: expected an integer in 1..1024, got %r" % (name, v))
    return int(v)


def _pano_arg(pano):
    x = _lib.require_gpu_tensor(_forward_only(pano, "pano"), "pano")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] != 2 * x.shape[2]:
        raise ValueError("pano: expected (B, 3, H, 2H), got %s" % (tuple(x.shape),))
    return x


def prefilter_environment(pano, height=32, lobes=(DIFFUSE,)):
    """``pano`` ``(B, 3, H, 2H)`` float32 on the device -> ``(B, L, 3, height, 2 height)``: map ``l`` at texel direction ``d`` is
    ``c_l sum_t pano[t] k_l(omega_d . omega_t) dOmega_t`` for the lobe ``lobes[l]``: ``"diffuse"`` (``max(0, x) / pi``: the
    irradiance map over pi) or a Phong exponent ``m >= 0`` (``(m + 1) / 2 pi max(0, x)^m``).  ``eml_env_prefilter_f32``; only
    enqueues work, run-to-run exact; an image's maps do not depend on the batch, a lobe's map not on the other lobes."""
    vals = _lobes(lobes)
    Ho = _height(height, "height")
    x = _pano_arg(pano)
    B, _, H, W = x.shape
    out = torch.empty(B, len(vals), 3, Ho, 2 * Ho, dtype=torch.float32, device=x.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, L.eml_env_prefilter_work_floats(B, H, W, Ho, len(vals))), dtype=torch.float32,
                           device=x.device)
        arr = (ctypes.c_double * len(vals))(*vals)                    # a host array: read before the call returns
        _lib.check(L.eml_env_prefilter_f32(_lib.ptr(x), B, H, W, Ho, len(vals), arr, _lib.ptr(out), _lib.ptr(work),
                                           _lib.current_stream()), "eml_env_prefilter_f32")
    return out


def _coefficient(k, name, B, h, w, device):
    """None, a number, an RGB triple or a ``(B, 3, h, w)`` tensor -> None or a contiguous ``(B, 3, h, w)`` device tensor."""
    if k is None:
        return None
    if isinstance(k, torch.Tensor):
        t = _lib.require_gpu_tensor(_forward_only(k, name), name)
        if tuple(t.shape) != (B, 3, h, w):
            raise ValueError("%s: expected a number, an RGB triple or a tensor %s, got %s" % (name, (B, 3, h, w), tuple(t.shape)))
        return t
    if isinstance(k, (int, float)):
        return torch.full((B, 3, h, w), float(k), dtype=torch.float32, device=device)
    rgb = [float(v) for v in k]
    if len(rgb) != 3:
        raise ValueError("%s: expected a number, an RGB triple or a tensor, got %r" % (name, k))
    t = torch.empty(B, 3, h, w, dtype=torch.float32, device=device)
    for ch in range(3):                                               # fills, not a host-to-device copy
        t[:, ch].fill_(rgb[ch])
    return t


def _gbuffer(normal, coverage):
    n = _lib.require_gpu_tensor(_forward_only(normal, "normal"), "normal")
    c = _lib.require_gpu_tensor(_forward_only(coverage, "coverage"), "coverage")
    if n.dim() != 4 or n.shape[1] != 3 or n.shape[2] < 2 or n.shape[3] < 2:
        raise ValueError("normal: expected (B, 3, h, w) with h, w >= 2, got %s" % (tuple(n.shape),))
    B, _, h, w = n.shape
    if tuple(c.shape) != (B, 1, h, w):
        raise ValueError("coverage: expected %s, got %s" % ((B, 1, h, w), tuple(c.shape)))
    return n, c


def _map_arg(t, name, B):
    """A map ``(B, 3, G, 2G)``, possibly a slice ``maps[:, l]`` of ``prefilter_environment``'s output: -> (tensor, G, stride)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.EmlightHipError("%s must be a float32 tensor on the MI355X; there is no CPU path" % name)
    _lib.require_gpu_tensor(t.new_empty(0), name)                     # device and dtype, without require's contiguous copy
    _forward_only(t, name)
    if t.dim() != 4 or t.shape[0] != B or t.shape[1] != 3 or t.shape[2] < 1 or t.shape[3] != 2 * t.shape[2]:
        raise ValueError("%s: expected (%d, 3, G, 2G), got %s" % (name, B, tuple(t.shape)))
    G = t.shape[2]
    if t.stride()[1:] != (2 * G * G, 2 * G, 1) or (B > 1 and t.stride(0) < 6 * G * G):
        t = t.contiguous()
    return t, G, (t.stride(0) if B > 1 else 6 * G * G)


def _camera(fov_deg, view_azimuth_deg):
    fov, az = float(fov_deg), float(view_azimuth_deg)
    if not (0.0 <= fov < 180.0) or not math.isfinite(az):
        raise ValueError("fov_deg must be in [0, 180) (0: orthographic) and view_azimuth_deg finite, got %r, %r"
                         % (fov_deg, view_azimuth_deg))
    return fov, az


def _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height, glossy_height, maps,
           background=None, exposure=None, gamma=2.4, want_shaded=True):
    """One ``eml_gbuffer_shade_f32`` call (after the prefilter calls it needs): -> (shaded or None, composite or None)."""
    fov, az = _camera(fov_deg, view_azimuth_deg)
    x = _pano_arg(pano)
    n, c = _gbuffer(normal, coverage)
    B, _, h, w = n.shape
    if x.shape[0] != B:
        raise ValueError("pano has %d images, the G-buffer %d" % (x.shape[0], B))
    kd, ks, km = (_coefficient(k, nm, B, h, w, n.device) for k, nm in ((kd, "kd"), (ks, "ks"), (km, "km")))
    if kd is None and ks is None and km is None:
        raise ValueError("at least one of kd, ks, km must be given")
    ed = eg = None
    if maps is not None:
        ed, eg = maps
        if (kd is not None and ed is None) or (ks is not None and eg is None):
            raise ValueError("maps=(E_diffuse, E_phong): kd needs E_diffuse and ks needs E_phong")
    else:
        if kd is not None:
            ed = prefilter_environment(x, diffuse_height, (DIFFUSE,))[:, 0]
        if ks is not None:
            eg = prefilter_environment(x, glossy_height, (float(phong_exponent),))[:, 0]
    ed, Hd, d_stride = _map_arg(ed, "E_diffuse", B) if kd is not None else (None, 0, 0)
    eg, Hg, g_stride = _map_arg(eg, "E_phong", B) if ks is not None else (None, 0, 0)
    bg = ex = comp = None
    if background is not None:
        bg, ex, g = _composite_args(background, exposure, gamma, B, h, w)
        comp = torch.empty(B, 3, h, w, dtype=torch.float32, device=n.device)
    else:
        g = 1.0
    shaded = torch.empty(B, 3, h, w, dtype=torch.float32, device=n.device) if want_shaded or comp is None else None
    if B > 0:
        _lib.check(_lib.lib().eml_gbuffer_shade_f32(
            _lib.ptr(x), x.shape[2], _lib.ptr(ed), Hd, d_stride, _lib.ptr(eg), Hg, g_stride, _lib.ptr(n), _lib.ptr(c),
            _lib.ptr(kd), _lib.ptr(ks), _lib.ptr(km), B, h, w, fov, az, _lib.ptr(shaded), _lib.ptr(bg), _lib.ptr(ex), g,
            _lib.ptr(comp), _lib.current_stream()), "eml_gbuffer_shade_f32")
    return shaded, comp


def _composite_args(background, exposure, gamma, B, h, w):
    bg = _lib.require_gpu_tensor(_forward_only(background, "background"), "background")
    if tuple(bg.shape) != (B, 3, h, w):
        raise ValueError("background: expected %s, got %s" % ((B, 3, h, w), tuple(bg.shape)))
    if isinstance(exposure, torch.Tensor):
        ex = _lib.require_gpu_tensor(_forward_only(exposure, "exposure"), "exposure")
        if ex.dim() == 0:
            ex = ex.expand(B).contiguous()
    elif exposure is None:
        raise ValueError("exposure: a number or a (B,) device tensor (TonemapHDR's alpha of the crop) is required")
    else:
        ex = torch.full((B,), float(exposure), dtype=torch.float32, device=bg.device)
    if tuple(ex.shape) != (B,):
        raise ValueError("exposure: expected (%d,), got %s" % (B, tuple(ex.shape)))
    g = float(gamma)
    if not (0.0 < g <= 1e6):
        raise ValueError("gamma must be in (0, 1e6], got %r" % (gamma,))
    return bg, ex, g


def shade_gbuffer(pano, normal, coverage, kd=None, ks=None, km=None, *, fov_deg=60.0, view_azimuth_deg=180.0,
                  phong_exponent=50.0, diffuse_height=32, glossy_height=64, maps=None):
    """``shaded (B, 3, h, w) = kd lookup(E_diffuse, n) + ks lookup(E_phong, R) + km lookup(pano, R)`` for the G-buffer
    ``normal (B, 3, h, w)`` (camera space: x image right, y image up, z towards the camera, any length) and
    ``coverage (B, 1, h, w)``, seen by ``crop_panorama``'s camera of ``fov_deg`` (0: orthographic) looking towards
    ``view_azimuth_deg``.  A coefficient is None (its term is not evaluated, its map not made), a number, an RGB triple or a
    ``(B, 3, h, w)`` tensor.  Prefilters the lobes it needs (``diffuse_height``, ``glossy_height``, ``phong_exponent``) or takes
    ``maps=(E_diffuse, E_phong)`` made earlier by ``prefilter_environment`` (slices ``[:, l]`` are taken as they are).
    ``shaded`` is 0 where ``coverage == 0`` or the normal has zero length; nothing else of such a pixel is read."""
    return _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height,
                  glossy_height, maps)[0]


def composite(shaded, coverage, background, exposure, gamma=2.4):
    """``coverage * clamp(exposure_b * shaded, 0, 1)^(1/gamma) + (1 - coverage) * background``: ``(B, 3, h, w)``.  ``exposure`` is
    a number or a ``(B,)`` device tensor; ``gamma == 1`` skips the power.  The epilogue of ``eml_gbuffer_shade_f32`` alone."""
    s = _lib.require_gpu_tensor(_forward_only(shaded, "shaded"), "shaded")
    if s.dim() != 4 or s.shape[1] != 3 or s.shape[2] < 2 or s.shape[3] < 2:
        raise ValueError("shaded: expected (B, 3, h, w) with h, w >= 2, got %s" % (tuple(s.shape),))
    B, _, h, w = s.shape
    c = _lib.require_gpu_tensor(_forward_only(coverage, "coverage"), "coverage")
    if tuple(c.shape) != (B, 1, h, w):
        raise ValueError("coverage: expected %s, got %s" % ((B, 1, h, w), tuple(c.shape)))
    bg, ex, g = _composite_args(background, exposure, gamma, B, h, w)
    out = torch.empty(B, 3, h, w, dtype=torch.float32, device=s.device)
    if B > 0:
        _lib.check(_lib.lib().eml_gbuffer_shade_f32(
            None, 0, None, 0, 0, None, 0, 0, None, _lib.ptr(c), None, None, None, B, h, w, 0.0, 0.0, _lib.ptr(s), _lib.ptr(bg),
            _lib.ptr(ex), g, _lib.ptr(out), _lib.current_stream()), "eml_gbuffer_shade_f32")
    return out


def insert_object(pano, normal, coverage, background, exposure, kd=None, ks=None, km=None, *, gamma=2.4, fov_deg=60.0,
                  view_azimuth_deg=180.0, phong_exponent=50.0, diffuse_height=32, glossy_height=64, maps=None):
    """``composite(shade_gbuffer(...), coverage, background, exposure, gamma)`` in ONE shading call: the shaded image is never
    written.  -> ``(B, 3, h, w)``, the photograph with the object in it, tonemapped."""
    return _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height,
                  glossy_height, maps, background, exposure, gamma, want_shaded=False)[1]


def gbuffer_sphere(h, w, centre, radius, device="cuda", batch=1):
    """Normals ``(batch, 3, h, w)`` and coverage ``(batch, 1, h, w)`` of a sphere drawn as DESIGN section 15 draws it: pixel
    (row i, column j) has ``px = (j - cx) / radius``, ``py = (cy - i) / radius`` with ``centre = (cx, cy)`` in pixel
    coordinates (column, row); it is covered iff ``px^2 + py^2 < 1``, and its normal is ``(px, py, sqrt(1 - px^2 - py^2))``.
    ``centre = ((S - 1) / 2, (S - 1) / 2)``, ``radius = S / 2`` on an ``S x S`` image is section 15's sphere.  Uncovered pixels
    have a zero normal.  Evaluated in float64 on ``device``, rounded to float32 once."""
    h, w = int(h), int(w)
    cx, cy = (float(v) for v in centre)
    rad = float(radius)
    if h < 2 or w < 2 or not rad > 0.0 or not (math.isfinite(cx) and math.isfinite(cy) and math.isfinite(rad)):
        raise ValueError("gbuffer_sphere: h, w >= 2, a finite centre and a radius > 0, got %r" % ((h, w, centre, radius),))
    px = ((torch.arange(w, dtype=torch.float64, device=device) - cx) / rad)[None, :].expand(h, w)
    py = ((cy - torch.arange(h, dtype=torch.float64, device=device)) / rad)[:, None].expand(h, w)
    rr = px * px + py * py
    inside = rr < 1.0
    nz = (1.0 - rr).clamp_min(0.0).sqrt()
    normal = (torch.stack([px, py, nz], 0) * inside).to(torch.float32)
    cov = inside.to(torch.float32)[None]
    return normal[None].expand(batch, 3, h, w).contiguous(), cov[None].expand(batch, 1, h, w).contiguous()


def _filled(values, device):
    """A 1-d float32 device tensor of a few numbers.  One tiny fill kernel per number instead of ``torch.tensor(values,
    device=...)``: that would be a copy from pageable host memory, which synchronises the stream; fills only enqueue."""
    t = torch.empty(len(values), dtype=torch.float32, device=device)
    for k, v in enumerate(values):
        t[k].fill_(float(v))
    return t


def _plane_arg(plane, B, device):
    """A 4-tuple ``(nx, ny, nz, d)`` or a ``(B, 4)`` device tensor -> (tensor, stride in floats)."""
    if isinstance(plane, torch.Tensor):
        t = _lib.require_gpu_tensor(_forward_only(plane, "plane"), "plane")
        if tuple(t.shape) != (B, 4):
            raise ValueError("plane: expected (nx, ny, nz, d) or a tensor %s, got %s" % ((B, 4), tuple(t.shape)))
        return t, 4
    vals = [float(v) for v in plane]
    if len(vals) != 4 or not all(math.isfinite(v) for v in vals):
        raise ValueError("plane: expected four finite numbers (nx, ny, nz, d), got %r" % (plane,))
    if vals[0] == 0.0 and vals[1] == 0.0 and vals[2] == 0.0:
        raise ValueError("plane: the normal is zero, got %r" % (plane,))
    if not vals[3] > 0.0:
        raise ValueError("plane: d > 0 is required (the camera is on the lit side: n.q + d = 0 on the plane), got %r" % (plane,))
    return _filled(vals, device), 0


def _shadow_args(pano, occluders, plane, fov_deg, view_azimuth_deg, size, image):
    """The checked arguments of ``ground_shadow`` (and of its adjoint in ``insert_grad``):
    -> (pano, occluders, K, plane tensor, plane stride, image or None, h, w, fov, azimuth)."""
    fov, az = _camera(fov_deg, view_azimuth_deg)
    if fov == 0.0:
        raise ValueError("fov_deg must be in (0, 180): the rays of an orthographic camera would need origins, got %r" % (fov_deg,))
    x = _pano_arg(pano)
    B = x.shape[0]
    occ = _lib.require_gpu_tensor(_forward_only(occluders, "occluders"), "occluders")
    if occ.dim() != 3 or occ.shape[0] != B or occ.shape[2] != 4 or occ.shape[1] > MAX_OCCLUDERS:
        raise ValueError("occluders: expected (%d, K, 4) with K <= %d, got %s" % (B, MAX_OCCLUDERS, tuple(occ.shape)))
    K = occ.shape[1]
    img = None
    if image is not None:
        img = _lib.require_gpu_tensor(_forward_only(image, "image"), "image")
        if img.dim() != 4 or img.shape[0] != B or img.shape[1] != 3:
            raise ValueError("image: expected (%d, 3, h, w), got %s" % (B, tuple(img.shape)))
        if size is not None and tuple(int(v) for v in size) != tuple(img.shape[2:]):
            raise ValueError("size %r does not match the image's %s" % (size, tuple(img.shape[2:])))
        h, w = img.shape[2:]
    elif size is None:
        raise ValueError("size=(h, w) is required without image")
    else:
        h, w = (int(v) for v in size)
    if h < 2 or w < 2:
        raise ValueError("the image size: expected h, w >= 2, got %s" % ((h, w),))
    pl, stride = _plane_arg(plane, B, x.device)
    return x, occ, K, pl, stride, img, h, w, fov, az


def ground_shadow(pano, occluders, plane=(0.0, 1.0, 0.0, 1.0), *, fov_deg=60.0, view_azimuth_deg=180.0, size=None, image=None):
    """The shadow ``occluders (B, K, 4)`` -- spheres ``(cx, cy, cz, r)`` in camera space (x image right, y image up, z towards
    the camera), ``0 <= K <= 16``, ``r <= 0`` or NaN ignored, ``r = inf`` holds every point -- cast on the ground plane
    ``n.q + d = 0`` (``plane = (nx, ny, nz, d)`` in camera space, one for the batch or a ``(B, 4)`` device tensor; the four numbers are the equation's coefficients, the
    normal is normalised here and ``d`` with it, so with a unit normal ``d`` is the camera's distance; ``d > 0``; the default
    is a floor one unit below a level camera) under the panorama ``pano (B, 3, H, 2H)``, seen by ``shade_gbuffer``'s camera.
    -> ``ratio (B, 3, h, w)`` in [0, 1]: per pixel that shows the plane and per channel, the cosine-weighted irradiance with
    the spheres in the way over the irradiance without them; exactly 1 where the pixel misses the plane or the channel's
    irradiance is 0, exactly 0 where the plane's point is inside a sphere.  ``size=(h, w)`` is required without ``image``;
    with ``image (B, 3, h, w)`` (the HDR photograph) -> ``(ratio, shadowed)`` with ``shadowed = image * ratio``, what
    ``composite`` takes as the background once tonemapped.  ``ratio`` does not look at the object's coverage: the composite
    overwrites those pixels.  A plane given as a device tensor cannot be checked here: a zero normal or ``d <= 0`` makes that
    image NaN.  ``eml_ground_shadow_f32``; only enqueues work, run-to-run exact, an image's result does not depend on the
    batch.  The unit of length is arbitrary, shared by plane and spheres."""
    x, occ, K, pl, stride, img, h, w, fov, az = _shadow_args(pano, occluders, plane, fov_deg, view_azimuth_deg, size, image)
    B, _, H, W = x.shape
    ratio = torch.empty(B, 3, h, w, dtype=torch.float32, device=x.device)
    shadowed = torch.empty_like(ratio) if img is not None else None
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, (L.eml_ground_shadow_work_floats(B, H, h, w, K) + 1) // 2), dtype=torch.float64,
                           device=x.device)                          # doubles: 8-byte aligned
        _lib.check(L.eml_ground_shadow_f32(_lib.ptr(x), B, H, W, _lib.ptr(pl), stride, _lib.ptr(occ) if K > 0 else None, K,
                                           h, w, fov, az, _lib.ptr(img), _lib.ptr(ratio), _lib.ptr(shadowed), _lib.ptr(work),
                                           _lib.current_stream()), "eml_ground_shadow_f32")
    return ratio if img is None else (ratio, shadowed)


def sphere_occluder(h, w, centre, radius, depth, fov_deg=60.0, device="cuda"):
    """The ``(1, 1, 4)`` camera-space occluder of the sphere ``gbuffer_sphere(h, w, centre, radius)`` draws, ``depth`` away from
    the camera: its centre lies at distance ``depth`` along the ray of pixel ``centre = (cx, cy)`` (column, row; fractions are
    fine), its radius is ``radius * 2 tan(fov / 2) / (w - 1) * depth``, the width of ``radius`` pixels at that distance.  A
    sphere's perspective image is only approximately that disc (it is an ellipse away from the image centre, and the disc's
    rim is seen at the tangent cone, slightly in front of the centre): occluder and drawing agree to first order in
    ``radius / depth``."""
    h, w = int(h), int(w)
    cx, cy = (float(v) for v in centre)
    rad, dep, fov = float(radius), float(depth), float(fov_deg)
    if (h < 2 or w < 2 or not (rad > 0.0 and dep > 0.0 and 0.0 < fov < 180.0)
            or not all(math.isfinite(v) for v in (cx, cy, rad, dep))):
        raise ValueError("sphere_occluder: h, w >= 2, a finite centre, radius > 0, depth > 0 and fov_deg in (0, 180), got %r"
                         % ((h, w, centre, radius, depth, fov_deg),))
    scl = math.tan(math.radians(fov) / 2.0)
    sx = scl * (2.0 * cx / (w - 1) - 1.0)
    sy = (scl * h / w) * (2.0 * cy / (h - 1) - 1.0)
    t = dep / math.sqrt(sx * sx + sy * sy + 1.0)                      # the ray is (sx, -sy, -1) in camera space
    return _filled((t * sx, -t * sy, -t, rad * 2.0 * scl / (w - 1) * dep), device).view(1, 1, 4)


# ------------------------------------------------------------------------------------------------ command line
def _load(path, shapes, name):
    a = np.asarray(np.load(path), dtype=np.float32)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] not in shapes:
        raise SystemExit("%s (%s): expected %s leading channels on (h, w), got %s" % (name, path, " or ".join(map(str, shapes)),
                                                                                  a.shape))
    return a


def build_parser():
    ap = argparse.ArgumentParser(description="insert a virtual object, lit by a panorama, into a photograph (.npy in and out)")
    ap.add_argument("--pano", required=True, help="(3, H, 2H) or (1, 3, H, 2H) HDR panorama, e.g. pred_<name>.npy")
    ap.add_argument("--image", required=True, help="(3, h, w) HDR crop the object goes into")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--gbuffer", default=None, help="directory with normal.npy, coverage.npy and any of kd.npy, ks.npy, km.npy")
    src.add_argument("--sphere", nargs=3, type=float, metavar=("CX", "CY", "RADIUS"), default=None)
    ap.add_argument("--kd", type=float, default=0.8, help="with --sphere")
    ap.add_argument("--ks", type=float, default=0.2, help="with --sphere")
    ap.add_argument("--km", type=float, default=0.0, help="with --sphere")
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--azimuth", type=float, default=180.0)
    ap.add_argument("--phong", type=float, default=50.0)
    ap.add_argument("--gamma", type=float, default=2.4)
    ap.add_argument("--exposure", type=float, default=None, help="default: TonemapHDR's alpha of the image, raised to gamma")
    ap.add_argument("--ground", type=float, default=None, metavar="HEIGHT",
                    help="cast the object's shadow on a ground plane HEIGHT below the camera (in the units of --depth / --occluders)")
    ap.add_argument("--ground_normal", nargs=3, type=float, default=(0.0, 1.0, 0.0), metavar=("NX", "NY", "NZ"),
                    help="the plane's normal in camera space (x right, y up, z towards the camera); default: straight up")
    ap.add_argument("--depth", type=float, default=None, help="with --sphere and --ground: the distance of the sphere's centre")
    ap.add_argument("--occluders", default=None, help="with --gbuffer and --ground: (K, 4) camera-space spheres (cx, cy, cz, r), K <= 16")
    ap.add_argument("--out", default="inserted.npy")
    return ap


def main(argv=None, device=None):
    args = build_parser().parse_args(argv)
    for p in (args.pano, args.image, args.out) + ((args.occluders,) if args.occluders else ()):
        if not p.endswith(".npy"):
            raise SystemExit("%s: the format is .npy only" % p)
    if args.ground is None and (args.depth is not None or args.occluders is not None):
        raise SystemExit("--depth and --occluders describe the shadow's occluder: they need --ground HEIGHT")
    if args.ground is not None:
        if args.sphere is not None and (args.depth is None or args.occluders is not None):
            raise SystemExit("--ground with --sphere needs --depth Z (the occluder is the sphere itself, not --occluders)")
        if args.gbuffer is not None and (args.occluders is None or args.depth is not None):
            raise SystemExit("--ground with --gbuffer needs --occluders FILE.npy (a G-buffer carries no geometry; --depth goes with --sphere)")
    from . import _runtime
    from .RegressionNetwork.util import TonemapHDR
    _runtime.entry_point_defaults()
    dev = device or "cuda:0"
    pano = torch.from_numpy(_load(args.pano, (3,), "--pano")[None]).to(dev)
    image = torch.from_numpy(_load(args.image, (3,), "--image")[None]).to(dev)
    h, w = image.shape[2:]
    if args.gbuffer is not None:
        def part(name, shapes, required=False):
            path = os.path.join(args.gbuffer, name + ".npy")
            if not os.path.exists(path):
                if required:
                    raise SystemExit("missing %s" % path)
                return None
            a = _load(path, shapes, name)
            if a.shape[1:] != (h, w):
                raise SystemExit("%s: %s does not match the image's %s" % (path, a.shape[1:], (h, w)))
            return torch.from_numpy(a[None]).to(dev)
        normal, coverage = part("normal", (3,), True), part("coverage", (1,), True)
        kd, ks, km = part("kd", (3,)), part("ks", (3,)), part("km", (3,))
        if kd is None and ks is None and km is None:
            raise SystemExit("%s holds none of kd.npy, ks.npy, km.npy" % args.gbuffer)
    else:
        normal, coverage = gbuffer_sphere(h, w, args.sphere[:2], args.sphere[2], device=dev)
        kd, ks, km = (v if v != 0.0 else None for v in (args.kd, args.ks, args.km))
        if kd is None and ks is None and km is None:
            raise SystemExit("--sphere: at least one of --kd, --ks, --km must be non-zero")
    if args.exposure is None:
        alpha = TonemapHDR(gamma=args.gamma)(image, clip=True)[1]     # maps the median of I^(1/gamma) to 0.5
        exposure = alpha.to(torch.float32) ** args.gamma              # clamp(alpha^gamma I)^(1/gamma) = clamp(alpha I^(1/gamma))
    else:
        exposure = torch.full((1,), float(args.exposure), dtype=torch.float32, device=dev)
    if args.ground is not None:                                       # the shadow goes onto the HDR image; the exposure stays
        if args.sphere is not None:
            try:
                occ = sphere_occluder(h, w, args.sphere[:2], args.sphere[2], args.depth, args.fov, device=dev)
            except ValueError as e:
                raise SystemExit(str(e))
        else:
            a = np.asarray(np.load(args.occluders), dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] > MAX_OCCLUDERS:
                raise SystemExit("--occluders (%s): expected (K, 4) with K <= %d, got %s" % (args.occluders, MAX_OCCLUDERS, a.shape))
            occ = torch.from_numpy(a[None]).to(dev)
        ln = math.sqrt(sum(float(v) ** 2 for v in args.ground_normal))
        if not (ln > 0.0 and math.isfinite(ln)):
            raise SystemExit("--ground_normal: the normal is zero or not finite")
        try:                                                          # a unit normal: HEIGHT is then the camera's distance
            image = ground_shadow(pano, occ, tuple(float(v) / ln for v in args.ground_normal) + (args.ground,), fov_deg=args.fov,
                                  view_azimuth_deg=args.azimuth, image=image)[1]
        except ValueError as e:
            raise SystemExit(str(e))
    background = (image * exposure.view(1, 1, 1, 1)).clamp(0.0, 1.0) ** (1.0 / args.gamma)
    out = insert_object(pano, normal, coverage, background, exposure, kd, ks, km, gamma=args.gamma, fov_deg=args.fov,
                        view_azimuth_deg=args.azimuth, phong_exponent=args.phong)
    np.save(args.out, out[0].cpu().numpy())
    print("wrote %s %s" % (args.out, tuple(out.shape[1:])))
    return out


if __name__ == "__main__":
    main()
