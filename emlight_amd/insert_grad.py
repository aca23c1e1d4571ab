"""Object insertion with gradients: ``emlight_amd.insert``'s four operators, differentiable (DESIGN.md section 23;
``tests/insert_grad_oracle.py`` restates the adjoints in float64).

* ``prefilter_environment`` is linear in the panorama; its gradient is the adjoint (``csrc/env_prefilter_bwd.hip``: the
  forward's implicit GEMM on the f32 MFMA, exchanged).
* ``shade_gbuffer`` / ``composite`` / ``insert_object`` (``csrc/gbuffer_shade_bwd.hip``): gradients for ``pano``, for
  ``maps=(E_diffuse, E_phong)`` (slices of a prefilter output included), for tensor ``kd`` / ``ks`` / ``km`` and for
  ``shaded``.  The map gradients are a data-dependent bilinear scatter, added in 64-bit fixed point: run-to-run exact, and a
  sample's bits do not depend on its batch or on what else was asked for.  ``dpano`` of ``shade_gbuffer`` is autograd's sum of
  the mirror scatter and the prefilter adjoints of the two map gradients.
* ``InsertionLoss``: "the inserted object looks right" for an arbitrary G-buffer, as a training term.
* ``ground_shadow`` (``csrc/ground_shadow_bwd.hip``; ``tests/shadow_grad_oracle.py``): gradients for
  ``pano`` and ``image``.  The ratio is ``1 - D / E0``, two linear functionals of the panorama, so the gradient is closed
  form; its hot path, the scatter over the binary visibility, reruns the forward's walk and adds in 64-bit fixed point.  The
  gradient is that of the unclamped ratio: a non-negative panorama never reaches the clamp to [0, 1]; where negative texels
  make it bind, it is passed straight through.  ``ShadowLoss``: "the shadow falls right", as a training term.

Numbers and RGB triples get no gradient.  ``normal``, ``coverage``, ``background`` and ``exposure`` have no gradient defined,
nor have the shadow's ``plane`` and ``occluders`` (visibility is binary: its derivative is zero almost everywhere and a
distribution on the silhouettes): one that requires grad is refused by name.  When nothing requires grad, or grad mode is
off, every call here makes exactly the launches of ``emlight_amd.insert`` and returns the same bits.  Everything only
enqueues work.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import insert as _insert
from .insert import DIFFUSE, MAX_LOBES, gbuffer_sphere  # noqa: F401  (the same names as emlight_amd.insert)


def _no_gradient(t, name):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise ValueError("%s requires grad: no gradient is defined for %s (DESIGN section 23 differentiates pano, maps, kd, "
                         "ks, km and shaded); pass %s.detach()" % (name, name, name))
    return t


def _needs(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


# ------------------------------------------------------------------------------------------------ the entry points, raw
def prefilter_environment_bwd_raw(grad_out, pano_height, lobes):
    """``eml_env_prefilter_bwd_f32`` without autograd: ``grad_out (B, L, 3, Ho, 2Ho)`` -> ``dpano (B, 3, H, 2H)`` with
    ``H = pano_height`` and ``lobes`` as ``prefilter_environment`` takes them."""
    vals = _insert._lobes(lobes)
    g = _lib.require_gpu_tensor(grad_out, "grad_out")
    if g.dim() != 5 or g.shape[1] != len(vals) or g.shape[2] != 3 or g.shape[3] < 1 or g.shape[4] != 2 * g.shape[3]:
        raise ValueError("grad_out: expected (B, %d, 3, Ho, 2Ho), got %s" % (len(vals), tuple(g.shape)))
    H = int(pano_height)
    if H != pano_height or H < 1:
        raise ValueError("pano_height: expected an integer >= 1, got %r" % (pano_height,))
    B, Ho = g.shape[0], _insert._height(g.shape[3], "grad_out's height")
    dpano = torch.empty(B, 3, H, 2 * H, dtype=torch.float32, device=g.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, L.eml_env_prefilter_bwd_work_floats(B, H, 2 * H, Ho, len(vals))), dtype=torch.float32,
                           device=g.device)
        arr = (ctypes.c_double * len(vals))(*vals)                    # a host array: read before the call returns
        _lib.check(L.eml_env_prefilter_bwd_f32(_lib.ptr(g), B, H, 2 * H, Ho, len(vals), arr, _lib.ptr(dpano), _lib.ptr(work),
                                               _lib.current_stream()), "eml_env_prefilter_bwd_f32")
    return dpano


WANTS = ("kd", "ks", "km", "e_diffuse", "e_phong", "pano", "shaded")


def shade_gbuffer_bwd_raw(grad_out, pano=None, maps=(None, None), normal=None, coverage=None, kd=None, ks=None, km=None, *,
                          fov_deg=60.0, view_azimuth_deg=180.0, exposure=None, gamma=2.4, shaded=None, want=()):
    """``eml_gbuffer_shade_bwd_f32`` without autograd.  ``grad_out (B, 3, h, w)`` is the gradient of ``shaded`` or, with
    ``exposure (B,)``, of the composite.  ``kd`` / ``ks`` / ``km`` are ``(B, 3, h, w)`` tensors or None (a term that was not
    evaluated); all None is the composite alone, which reads ``shaded``.  ``want``: names out of ``WANTS``; what is not named is
    passed as NULL and not computed.  -> dict name -> tensor."""
    want = tuple(want)
    bad = [n for n in want if n not in WANTS]
    if bad or not want:
        raise ValueError("want: expected some of %s, got %r" % (WANTS, want))
    g = _lib.require_gpu_tensor(grad_out, "grad_out")
    if g.dim() != 4 or g.shape[1] != 3 or g.shape[2] < 2 or g.shape[3] < 2:
        raise ValueError("grad_out: expected (B, 3, h, w) with h, w >= 2, got %s" % (tuple(g.shape),))
    B, _, h, w = g.shape
    fov, az = _insert._camera(fov_deg, view_azimuth_deg)
    c = _lib.require_gpu_tensor(coverage, "coverage")
    if tuple(c.shape) != (B, 1, h, w):
        raise ValueError("coverage: expected %s, got %s" % ((B, 1, h, w), tuple(c.shape)))
    given = kd is None and ks is None and km is None
    n = x = s = ex = None
    H = 0
    if not given:
        n = _lib.require_gpu_tensor(normal, "normal")
        if tuple(n.shape) != (B, 3, h, w):
            raise ValueError("normal: expected %s, got %s" % ((B, 3, h, w), tuple(n.shape)))
    else:
        s = _lib.require_gpu_tensor(shaded, "shaded")
        if tuple(s.shape) != (B, 3, h, w):
            raise ValueError("shaded: expected %s, got %s" % ((B, 3, h, w), tuple(s.shape)))
    kd, ks, km = (_insert._coefficient(k, nm, B, h, w, g.device) for k, nm in ((kd, "kd"), (ks, "ks"), (km, "km")))
    if km is not None:
        x = _insert._pano_arg(pano)
        if x.shape[0] != B:
            raise ValueError("pano has %d images, the G-buffer %d" % (x.shape[0], B))
        H = x.shape[2]
    ed, Hd, d_stride = _insert._map_arg(maps[0], "E_diffuse", B) if kd is not None else (None, 0, 0)
    eg, Hg, g_stride = _insert._map_arg(maps[1], "E_phong", B) if ks is not None else (None, 0, 0)
    if exposure is not None:
        ex = _lib.require_gpu_tensor(exposure, "exposure")
        if tuple(ex.shape) != (B,):
            raise ValueError("exposure: expected (%d,), got %s" % (B, tuple(ex.shape)))
    shapes = {"kd": (B, 3, h, w), "ks": (B, 3, h, w), "km": (B, 3, h, w), "e_diffuse": (B, 3, Hd, 2 * Hd),
              "e_phong": (B, 3, Hg, 2 * Hg), "pano": (B, 3, H, 2 * H), "shaded": (B, 3, h, w)}
    out = {nm: torch.empty(shapes[nm], dtype=torch.float32, device=g.device) for nm in want}
    if B > 0:
        L = _lib.lib()
        flags = tuple(int(nm in want) for nm in ("pano", "e_diffuse", "e_phong"))
        work = None
        if any(flags):
            work = torch.empty(max(2, L.eml_gbuffer_shade_bwd_work_floats(B, H, Hd, Hg, h, w, *flags)), dtype=torch.float32,
                               device=g.device)
        _lib.check(L.eml_gbuffer_shade_bwd_f32(
            _lib.ptr(g), _lib.ptr(x), H, _lib.ptr(ed), Hd, d_stride, _lib.ptr(eg), Hg, g_stride, _lib.ptr(n), _lib.ptr(c),
            _lib.ptr(kd), _lib.ptr(ks), _lib.ptr(km), B, h, w, fov, az, _lib.ptr(s), _lib.ptr(ex), float(gamma),
            _lib.ptr(out.get("kd")), _lib.ptr(out.get("ks")), _lib.ptr(out.get("km")), _lib.ptr(out.get("e_diffuse")),
            _lib.ptr(out.get("e_phong")), _lib.ptr(out.get("pano")), _lib.ptr(out.get("shaded")), _lib.ptr(work),
            _lib.current_stream()), "eml_gbuffer_shade_bwd_f32")
    return out


def _no_shadow_gradient(t, name):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise ValueError("%s requires grad: no gradient is defined for %s (visibility is binary; DESIGN section 29 "
                         "differentiates pano and image); pass %s.detach()" % (name, name, name))
    return t


def ground_shadow_bwd_raw(pano, occluders, plane=(0.0, 1.0, 0.0, 1.0), *, fov_deg=60.0, view_azimuth_deg=180.0, size=None,
                          image=None, g_ratio=None, g_shadowed=None, want=("pano",)):
    """``eml_ground_shadow_bwd_f32`` without autograd.  The scene as ``ground_shadow`` takes it; ``g_ratio`` and ``g_shadowed``
    ``(B, 3, h, w)`` are the gradients of its two outputs, either may be None, ``g_shadowed`` needs ``image``.  ``want``: some of
    ``"pano"`` and ``"image"`` (which needs ``g_shadowed``); what is not named is passed as NULL and not computed.
    -> dict name -> tensor: ``pano (B, 3, H, 2H)``, ``image (B, 3, h, w)``."""
    want = tuple(want)
    if not want or any(n not in ("pano", "image") for n in want):
        raise ValueError("want: expected some of ('pano', 'image'), got %r" % (want,))
    if g_ratio is None and g_shadowed is None:
        raise ValueError("g_ratio and g_shadowed: at least one gradient is required")
    if g_shadowed is not None and image is None:
        raise ValueError("g_shadowed needs image (shadowed = image * ratio)")
    if "image" in want and g_shadowed is None:
        raise ValueError("want 'image' needs g_shadowed (dimage = g_shadowed * ratio)")
    if size is None and image is None:
        size = tuple((g_ratio if g_ratio is not None else g_shadowed).shape[2:])
    x, occ, K, pl, stride, img, h, w, fov, az = _insert._shadow_args(pano, occluders, plane, fov_deg, view_azimuth_deg, size,
                                                                     image)
    B, _, H, W = x.shape
    grads = []
    for t, nm in ((g_ratio, "g_ratio"), (g_shadowed, "g_shadowed")):
        if t is not None:
            t = _lib.require_gpu_tensor(t, nm)
            if tuple(t.shape) != (B, 3, h, w):
                raise ValueError("%s: expected %s, got %s" % (nm, (B, 3, h, w), tuple(t.shape)))
        grads.append(t)
    out = {}
    if "pano" in want:
        out["pano"] = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    if "image" in want:
        out["image"] = torch.empty(B, 3, h, w, dtype=torch.float32, device=x.device)
    if B > 0:
        L = _lib.lib()
        work = torch.empty(max(1, (L.eml_ground_shadow_bwd_work_floats(B, H, h, w, K) + 1) // 2), dtype=torch.float64,
                           device=x.device)                          # doubles: 8-byte aligned
        _lib.check(L.eml_ground_shadow_bwd_f32(_lib.ptr(x), B, H, W, _lib.ptr(pl), stride, _lib.ptr(occ) if K > 0 else None, K,
                                               h, w, fov, az, _lib.ptr(img) if grads[1] is not None else None,
                                               _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(out.get("pano")),
                                               _lib.ptr(out.get("image")), _lib.ptr(work), _lib.current_stream()),
                   "eml_ground_shadow_bwd_f32")
    return out


# ------------------------------------------------------------------------------------------------ autograd
class _Prefilter(torch.autograd.Function):
    """Linear in the panorama: nothing is saved but the geometry."""

    @staticmethod
    def forward(ctx, pano, height, lobes):
        ctx.geometry = (pano.shape[2], lobes)
        return _insert.prefilter_environment(pano, height, lobes)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return prefilter_environment_bwd_raw(g, *ctx.geometry), None, None


def prefilter_environment(pano, height=32, lobes=(DIFFUSE,)):
    """``emlight_amd.insert.prefilter_environment``, differentiable in ``pano`` (``eml_env_prefilter_bwd_f32``)."""
    if not _needs(pano):
        return _insert.prefilter_environment(pano, height, lobes)
    _insert._lobes(lobes), _insert._height(height, "height")
    lobes = (lobes,) if isinstance(lobes, (str, int, float)) else tuple(lobes)
    return _Prefilter.apply(pano, height, lobes)


class _Shade(torch.autograd.Function):
    """One shading call (with the composite as its epilogue when ``background`` is given) and its adjoint.  The tensor inputs
    that may take a gradient come first: pano (the mirror term), E_diffuse, E_phong, kd, ks, km."""

    @staticmethod
    def forward(ctx, pano, ed, eg, kd, ks, km, normal, coverage, background, exposure, gamma, fov, az):
        shaded, comp = _insert._shade(pano, normal, coverage, kd, ks, km, fov, az, 0.0, 1, 1, (ed, eg), background, exposure,
                                      gamma, want_shaded=background is None)
        ctx.save_for_backward(pano, ed, eg, kd, ks, km, normal, coverage, exposure)
        ctx.camera = (fov, az, gamma)
        return shaded if background is None else comp

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pano, ed, eg, kd, ks, km, normal, coverage, exposure = ctx.saved_tensors
        fov, az, gamma = ctx.camera
        names = ("pano", "e_diffuse", "e_phong", "kd", "ks", "km")
        term = {"pano": km, "e_diffuse": kd, "e_phong": ks, "kd": kd, "ks": ks, "km": km}      # a term that was not evaluated
        want = tuple(nm for nm, need in zip(names, ctx.needs_input_grad) if need and term[nm] is not None)   # has no gradient
        if not want:
            return (None,) * 13
        got = shade_gbuffer_bwd_raw(g, pano, (ed, eg), normal, coverage, kd, ks, km, fov_deg=fov, view_azimuth_deg=az,
                                    exposure=exposure, gamma=gamma, want=want)
        return tuple(got.get(nm) for nm in names) + (None,) * 7


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shaded, coverage, background, exposure, gamma):
        ctx.save_for_backward(shaded, coverage, exposure)
        ctx.gamma = gamma
        return _insert.composite(shaded, coverage, background, exposure, gamma)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        shaded, coverage, exposure = ctx.saved_tensors
        got = shade_gbuffer_bwd_raw(g, coverage=coverage, exposure=exposure, gamma=ctx.gamma, shaded=shaded, want=("shaded",))
        return got["shaded"], None, None, None, None


def _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height, glossy_height, maps,
           background=None, exposure=None, gamma=2.4):
    for t, nm in ((normal, "normal"), (coverage, "coverage"), (background, "background"), (exposure, "exposure")):
        _no_gradient(t, nm)
    given = tuple(maps) if maps is not None else (None, None)
    if not _needs(pano, kd, ks, km, *given):
        return _insert._shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height,
                              glossy_height, maps, background, exposure, gamma, want_shaded=background is None)[background is not None]
    fov, az = _insert._camera(fov_deg, view_azimuth_deg)
    n, c = _insert._gbuffer(normal, coverage)
    B, _, h, w = n.shape
    if not isinstance(pano, torch.Tensor) or pano.dim() != 4 or pano.shape[0] != B:
        raise ValueError("pano: expected (%d, 3, H, 2H) for this G-buffer, got %s" % (B, tuple(getattr(pano, "shape", ()))))
    with torch.no_grad():                                             # numbers and triples become constant tensors; a tensor stays
        kd, ks, km = (k if isinstance(k, torch.Tensor) else _insert._coefficient(k, nm, B, h, w, n.device)
                      for k, nm in ((kd, "kd"), (ks, "ks"), (km, "km")))
    if kd is None and ks is None and km is None:
        raise ValueError("at least one of kd, ks, km must be given")
    ed, eg = given
    if maps is not None:
        if (kd is not None and ed is None) or (ks is not None and eg is None):
            raise ValueError("maps=(E_diffuse, E_phong): kd needs E_diffuse and ks needs E_phong")
    else:
        if kd is not None:
            ed = prefilter_environment(pano, diffuse_height, (DIFFUSE,))[:, 0]
        if ks is not None:
            eg = prefilter_environment(pano, glossy_height, (float(phong_exponent),))[:, 0]
    ed, eg = (ed if kd is not None else None), (eg if ks is not None else None)
    bg = ex = None
    if background is not None:
        bg, ex, gamma = _insert._composite_args(background, exposure, gamma, B, h, w)
    return _Shade.apply(pano, ed, eg, kd, ks, km, n, c, bg, ex, float(gamma), fov, az)


def shade_gbuffer(pano, normal, coverage, kd=None, ks=None, km=None, *, fov_deg=60.0, view_azimuth_deg=180.0,
                  phong_exponent=50.0, diffuse_height=32, glossy_height=64, maps=None):
    """``emlight_amd.insert.shade_gbuffer``, differentiable in ``pano``, in ``maps`` and in tensor ``kd`` / ``ks`` / ``km``.
    Without ``maps`` the gradient of ``pano`` is the sum of the mirror scatter and of the prefilter adjoints of the two map
    gradients; with ``maps`` each map gets its own gradient and ``pano`` the mirror term alone."""
    return _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height,
                  glossy_height, maps)


def composite(shaded, coverage, background, exposure, gamma=2.4):
    """``emlight_amd.insert.composite``, differentiable in ``shaded``: ``coverage (1/gamma) exposure (exposure shaded)^(1/gamma - 1)``
    times the upstream gradient where ``0 < exposure shaded < 1``, and 0 elsewhere (both clamps, and the boundaries)."""
    for t, nm in ((coverage, "coverage"), (background, "background"), (exposure, "exposure")):
        _no_gradient(t, nm)
    if not _needs(shaded):
        return _insert.composite(shaded, coverage, background, exposure, gamma)
    if not isinstance(shaded, torch.Tensor) or shaded.dim() != 4:
        raise ValueError("shaded: expected (B, 3, h, w), got %r" % (getattr(shaded, "shape", shaded),))
    B, _, h, w = shaded.shape
    bg, ex, g = _insert._composite_args(background, exposure, gamma, B, h, w)
    return _Composite.apply(shaded, coverage, bg, ex, g)


def insert_object(pano, normal, coverage, background, exposure, kd=None, ks=None, km=None, *, gamma=2.4, fov_deg=60.0,
                  view_azimuth_deg=180.0, phong_exponent=50.0, diffuse_height=32, glossy_height=64, maps=None):
    """``emlight_amd.insert.insert_object``, differentiable as ``shade_gbuffer`` is: ONE shading call forward, and the adjoint
    recomputes the shaded value with the forward's own instruction sequence."""
    if background is None:
        raise ValueError("background: a (B, 3, h, w) device tensor is required")
    return _shade(pano, normal, coverage, kd, ks, km, fov_deg, view_azimuth_deg, phong_exponent, diffuse_height,
                  glossy_height, maps, background, exposure, gamma)


class _Shadow(torch.autograd.Function):
    """One forward call; the adjoint reruns the forward's walk from the forward's inputs, nothing else is saved."""

    @staticmethod
    def forward(ctx, pano, image, occluders, plane, fov, az, size):
        out = _insert.ground_shadow(pano, occluders, plane, fov_deg=fov, view_azimuth_deg=az, size=size, image=image)
        tensors = [pano, occluders] + [t for t in (image, plane) if isinstance(t, torch.Tensor)]
        ctx.save_for_backward(*tensors)
        ctx.scene = (image is not None, plane if not isinstance(plane, torch.Tensor) else None, fov, az, tuple(out[0].shape[2:])
                     if image is not None else tuple(out.shape[2:]))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ratio, g_shadowed=None):
        saved = list(ctx.saved_tensors)
        has_image, plane, fov, az, size = ctx.scene
        pano, occluders = saved[0].detach(), saved[1].detach()
        image = saved[2].detach() if has_image else None
        if plane is None:
            plane = saved[-1].detach()
        want = tuple(nm for nm, need in zip(("pano", "image"), ctx.needs_input_grad)
                     if need and (nm == "pano" or g_shadowed is not None))
        if not want or (g_ratio is None and g_shadowed is None):
            return (None,) * 7
        got = ground_shadow_bwd_raw(pano, occluders, plane, fov_deg=fov, view_azimuth_deg=az, size=size,
                                    image=image if g_shadowed is not None else None, g_ratio=g_ratio, g_shadowed=g_shadowed,
                                    want=want)
        return (got.get("pano"), got.get("image")) + (None,) * 5


def ground_shadow(pano, occluders, plane=(0.0, 1.0, 0.0, 1.0), *, fov_deg=60.0, view_azimuth_deg=180.0, size=None, image=None):
    """``emlight_amd.insert.ground_shadow``, differentiable in ``pano`` and in ``image`` (``eml_ground_shadow_bwd_f32``): the
    same arguments, the same returns, the same bits.  ``dpano = wgt / E0 (S - G)`` with ``S = sum_p g (1 - v)`` and
    ``G[t] = sum_p g blocked(p, t)`` over the pixels that hit the plane outside every sphere, ``g = g_ratio + g_shadowed image``;
    ``dimage = g_shadowed ratio``.  The gradient is that of the unclamped ratio: a non-negative panorama never reaches the
    clamp, and where negative texels make it bind it is passed straight through.  ``plane`` and ``occluders`` have no
    gradient (visibility is binary): one that requires grad is refused by name."""
    _no_shadow_gradient(plane, "plane"), _no_shadow_gradient(occluders, "occluders")
    if not _needs(pano, image):
        return _insert.ground_shadow(pano, occluders, plane, fov_deg=fov_deg, view_azimuth_deg=view_azimuth_deg, size=size,
                                     image=image)
    with torch.no_grad():                                             # every refusal of the forward, before anything is recorded
        _, _, _, _, _, _, h, w, fov, az = _insert._shadow_args(pano, occluders, plane, fov_deg, view_azimuth_deg, size, image)
    return _Shadow.apply(pano, image, occluders, plane, fov, az, (h, w))


# ------------------------------------------------------------------------------------------------ a training term
def _shade_pair(loss, pred, true):
    """The shaded images of ``pred`` and ``true`` from one prefilter call per lobe and one shading call over ``2B`` images:
    -> (shaded (2B, 3, h, w), E_diffuse or None, E_phong or None)."""
    x = torch.cat([pred, true], 0)
    ed = eg = None
    if loss.kd is not None:
        ed = _insert.prefilter_environment(x, loss.diffuse_height, (DIFFUSE,))[:, 0]
    if loss.ks is not None:
        eg = _insert.prefilter_environment(x, loss.glossy_height, (loss.phong_exponent,))[:, 0]
    out = _insert.shade_gbuffer(x, loss.normal2, loss.coverage2, loss.kd2, loss.ks2, loss.km2, fov_deg=loss.fov_deg,
                                view_azimuth_deg=loss.view_azimuth_deg, maps=(ed, eg))
    return out, ed, eg


class _ShadePair(torch.autograd.Function):
    """``_shade_pair`` for a ``pred`` that requires grad.  ``true``'s images are not differentiable and the adjoints run over
    ``pred``'s images only."""

    @staticmethod
    def forward(ctx, pred, true, loss):
        B = pred.shape[0]
        out, ed, eg = _shade_pair(loss, pred, true)
        ctx.save_for_backward(pred, ed, eg)
        ctx.loss = loss
        a, b = out[:B], out[B:]
        ctx.mark_non_differentiable(b)
        return a, b

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        pred, ed, eg = ctx.saved_tensors
        loss, B, H = ctx.loss, pred.shape[0], pred.shape[2]
        want = tuple(nm for nm, k in (("e_diffuse", loss.kd), ("e_phong", loss.ks), ("pano", loss.km)) if k is not None)
        got = shade_gbuffer_bwd_raw(g, pred, (None if ed is None else ed[:B], None if eg is None else eg[:B]), loss.normal,
                                    loss.coverage, loss.kd, loss.ks, loss.km, fov_deg=loss.fov_deg,
                                    view_azimuth_deg=loss.view_azimuth_deg, want=want)
        dpano = got.get("pano")                                       # the mirror term, then the two adjoints, in this order
        for nm, lobe in (("e_diffuse", DIFFUSE), ("e_phong", loss.phong_exponent)):
            if nm in got:
                term = prefilter_environment_bwd_raw(got[nm].unsqueeze(1), H, (lobe,))
                dpano = term if dpano is None else dpano + term
        return dpano, None, None


class InsertionLoss(torch.nn.Module):
    """"The inserted object looks right", as a training term: the mean over images of
    ``sum coverage (a - b)^2 / (3 sum coverage)`` with ``a``, ``b`` the shaded images of the G-buffer ``normal (B, 3, h, w)``,
    ``coverage (B, 1, h, w)``, ``kd`` / ``ks`` / ``km`` (None, a number, an RGB triple or a tensor, as ``shade_gbuffer`` takes
    them) under the predicted and the true panorama.  Both batches go through ONE forward over ``2B`` images; the truth gets
    no gradient and the adjoint kernels run over the prediction's images only.  A forward plus backward only enqueues work."""

    def __init__(self, normal, coverage, kd=None, ks=None, km=None, *, fov_deg=60.0, view_azimuth_deg=180.0,
                 phong_exponent=50.0, diffuse_height=32, glossy_height=64):
        super().__init__()
        for t, nm in ((normal, "normal"), (coverage, "coverage"), (kd, "kd"), (ks, "ks"), (km, "km")):
            _no_gradient(t, nm)
        self.fov_deg, self.view_azimuth_deg = _insert._camera(fov_deg, view_azimuth_deg)
        self.phong_exponent = float(phong_exponent)
        _insert._lobes((self.phong_exponent,))
        self.diffuse_height = _insert._height(diffuse_height, "diffuse_height")
        self.glossy_height = _insert._height(glossy_height, "glossy_height")
        with torch.no_grad():
            n, c = _insert._gbuffer(normal, coverage)
            B, _, h, w = n.shape
            if B < 1:
                raise ValueError("normal: expected at least one image, got %s" % (tuple(n.shape),))
            ks3 = [_insert._coefficient(k, nm, B, h, w, n.device) for k, nm in ((kd, "kd"), (ks, "ks"), (km, "km"))]
            if all(k is None for k in ks3):
                raise ValueError("at least one of kd, ks, km must be given")
            pairs = [("normal", n.detach()), ("coverage", c.detach())] + [(nm, None if k is None else k.detach())
                                                                          for nm, k in zip(("kd", "ks", "km"), ks3)]
            for nm, t in pairs:                                       # and the same G-buffer twice, for the forward over 2B images
                self.register_buffer(nm, t, persistent=False)
                self.register_buffer(nm + "2", None if t is None else torch.cat([t, t], 0), persistent=False)
            self.register_buffer("denominator", 3.0 * c.sum((1, 2, 3)), persistent=False)

    def forward(self, pred, true):
        p = _insert._pano_arg(pred.detach() if isinstance(pred, torch.Tensor) else pred)
        t = _insert._pano_arg(true.detach() if isinstance(true, torch.Tensor) else true)
        B = self.normal.shape[0]
        if p.shape != t.shape or p.shape[0] != B:
            raise ValueError("pred %s and true %s: expected two equal shapes (%d, 3, H, 2H)" % (tuple(p.shape), tuple(t.shape), B))
        if _needs(pred):
            a, b = _ShadePair.apply(pred, t, self)
        else:
            with torch.no_grad():
                out = _shade_pair(self, p, t)[0]
            a, b = out[:B], out[B:]
        d = a - b
        return ((self.coverage * d * d).sum((1, 2, 3)) / self.denominator).mean()


class _ShadowPair(torch.autograd.Function):
    """The shadow ratios of ``pred`` and ``true`` from one forward over ``2B`` images, for a ``pred`` that requires grad.
    ``true``'s images are not differentiable and the adjoint runs over ``pred``'s images only."""

    @staticmethod
    def forward(ctx, pred, true, loss):
        B = pred.shape[0]
        out = loss.ratios(pred, true)
        ctx.save_for_backward(pred)
        ctx.loss = loss
        a, b = out[:B], out[B:]
        ctx.mark_non_differentiable(b)
        return a, b

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        loss = ctx.loss
        got = ground_shadow_bwd_raw(ctx.saved_tensors[0].detach(), loss.occluders, loss.plane, fov_deg=loss.fov_deg,
                                    view_azimuth_deg=loss.view_azimuth_deg, size=loss.size, g_ratio=g.contiguous())
        return got["pano"], None, None


class ShadowLoss(torch.nn.Module):
    """"The shadow falls right", as a training term: the mean over images of ``sum weight (a - b)^2 / (3 sum weight)`` with
    ``a``, ``b`` the shadow ratios (``ground_shadow``: ``occluders (B, K, 4)``, ``plane`` four numbers or a ``(B, 4)`` tensor,
    ``size=(h, w)``) under the predicted and the true panorama.  ``weight (B, 1, h, w)`` defaults to all ones; pass
    ``1 - coverage`` to ignore the pixels the object hides.  Both panoramas go through ONE forward over ``2B`` images; the
    truth gets no gradient and the adjoint runs over the prediction's images only.  A misplaced or over-blurred light gives a
    wrong or missing shadow where the shaded object still looks plausible: this term sees it.  Only enqueues work."""

    def __init__(self, occluders, plane=(0.0, 1.0, 0.0, 1.0), *, size, fov_deg=60.0, view_azimuth_deg=180.0, weight=None):
        super().__init__()
        _no_shadow_gradient(occluders, "occluders"), _no_shadow_gradient(plane, "plane"), _no_gradient(weight, "weight")
        self.fov_deg, self.view_azimuth_deg = _insert._camera(fov_deg, view_azimuth_deg)
        self.size = tuple(int(v) for v in size)
        with torch.no_grad():
            occ = _lib.require_gpu_tensor(occluders, "occluders")
            if occ.dim() != 3 or occ.shape[0] < 1 or occ.shape[2] != 4 or occ.shape[1] > _insert.MAX_OCCLUDERS:
                raise ValueError("occluders: expected (B, K, 4) with B >= 1 and K <= %d, got %s"
                                 % (_insert.MAX_OCCLUDERS, tuple(occ.shape)))
            B, (h, w) = occ.shape[0], self.size
            if h < 2 or w < 2:
                raise ValueError("size: expected h, w >= 2, got %s" % (self.size,))
            if weight is None:
                wt = torch.ones(B, 1, h, w, dtype=torch.float32, device=occ.device)
            else:
                wt = _lib.require_gpu_tensor(weight, "weight")
                if tuple(wt.shape) != (B, 1, h, w):
                    raise ValueError("weight: expected %s, got %s" % ((B, 1, h, w), tuple(wt.shape)))
            self.register_buffer("occluders", occ.detach(), persistent=False)
            self.register_buffer("occluders2", torch.cat([occ, occ], 0).detach(), persistent=False)
            self.register_buffer("weight", wt.detach(), persistent=False)
            self.register_buffer("denominator", 3.0 * wt.sum((1, 2, 3)), persistent=False)
            if isinstance(plane, torch.Tensor):
                pl, _ = _insert._plane_arg(plane, B, occ.device)
                self.register_buffer("plane", pl.detach(), persistent=False)
                self.register_buffer("plane2", torch.cat([pl, pl], 0).detach(), persistent=False)
            else:
                _insert._plane_arg(plane, B, occ.device)              # its refusals, now
                self.plane = self.plane2 = tuple(float(v) for v in plane)

    def ratios(self, pred, true):
        """ratio (2B, 3, h, w): the prediction's images, then the truth's, from one forward call."""
        return _insert.ground_shadow(torch.cat([pred, true], 0), self.occluders2, self.plane2, fov_deg=self.fov_deg,
                                     view_azimuth_deg=self.view_azimuth_deg, size=self.size)

    def forward(self, pred, true):
        p = _insert._pano_arg(pred.detach() if isinstance(pred, torch.Tensor) else pred)
        t = _insert._pano_arg(true.detach() if isinstance(true, torch.Tensor) else true)
        B = self.occluders.shape[0]
        if p.shape != t.shape or p.shape[0] != B:
            raise ValueError("pred %s and true %s: expected two equal shapes (%d, 3, H, 2H)" % (tuple(p.shape), tuple(t.shape), B))
        if _needs(pred):
            a, b = _ShadowPair.apply(pred, t, self)
        else:
            with torch.no_grad():
                out = self.ratios(p, t)
            a, b = out[:B], out[B:]
        d = a - b
        return ((self.weight * d * d).sum((1, 2, 3)) / self.denominator).mean()
