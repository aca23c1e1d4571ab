"""Mirror of the hot-path parts of the reference's ``RegressionNetwork/util.py``.

``convert_to_panorama`` (reference ``util.py:222-245``) runs as one HIP kernel each way;
``sphere_points`` (``util.py:286-299``) is the small host helper the kept entry points need.
``PanoramaHandler`` (``util.py:69-185``: crop, rotate, resize) and ``TonemapHDR`` (``util.py:36-66``) run on device
tensors, batched (csrc/pano_prep.hip); ``PanoramaHandler.warp_panorama`` is the panorama warp of ``GenProjector/util.py:279-343``
(csrc/pano_warp.hip, gradients: csrc/pano_warp_bwd.hip), ``PanoramaHandler.warp_panorama_depth`` the same warp with the scene
where its depth panorama puts it (csrc/pano_warp_depth.hip, forward only); ``TonemapHDR`` keeps the reference's numpy form for numpy input.
EXR/vtk/cv2 I/O is out of scope.
"""
import functools

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib


def sphere_points(n=128):
    """Fibonacci-sphere anchors (n, 3), float64 -- reference ``util.py:286-299``."""
    idx = np.arange(n)
    ang = idx * (np.pi * (3.0 - np.sqrt(5.0)))
    z = np.linspace(1.0 - 1.0 / n, 1.0 / n - 1.0, n)
    rad = np.sqrt(1.0 - z * z)
    pts = np.empty((n, 3))
    pts[:, 0], pts[:, 1], pts[:, 2] = rad * np.cos(ang), rad * np.sin(ang), z
    return pts


class _Rasterise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, sizes, colors, H, W):
        B, N = sizes.shape
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dirs.device)
        _lib.check(_lib.lib().eml_sg_rasterise_f32(_lib.ptr(dirs), _lib.ptr(sizes), _lib.ptr(colors),
                                                   _lib.ptr(out), B, N, H, W, _lib.current_stream()),
                   "eml_sg_rasterise_f32")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(dirs, sizes, colors)   # q = gout . colors enters d/d dirs and d/d sizes
        else:
            ctx.save_for_backward(dirs, sizes)
        ctx.hw = (H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        need = ctx.needs_input_grad[:3]
        H, W = ctx.hw
        if not (need[0] or need[1]):
            dirs, sizes = ctx.saved_tensors
            return None, None, rasterise_bwd_colors_raw(dirs, sizes, gout, (H, W)), None, None
        dirs, sizes, colors = ctx.saved_tensors
        gd, gs, gc = rasterise_bwd_raw(dirs, sizes, colors, gout, (H, W), need=need)
        return gd, gs, gc, None, None


def rasterise_bwd_raw(dirs, sizes, colors, gout, pano_hw, exhaustive=False, need=(True, True, True)):
    """d loss / d (dirs (B, 3N), sizes (B, N), colors (B, 3N)) in one ``eml_sg_rasterise_bwd_f32`` launch (+ its tile-order
    reduce): the colours-only kernel's light lists and tiles with four more sums per light.  ``need``: which of the three to
    return (the others are ``None`` and not written); the colour gradient is bit for bit ``rasterise_bwd_colors_raw``'s.
    ``exhaustive``: every light for every tile (what the culled launch equals bit for bit)."""
    H, W = pano_hw
    B, N = sizes.shape
    if not any(need):
        raise ValueError("rasterise_bwd_raw: no gradient requested")
    L = _lib.lib()
    gout = gout.contiguous()
    dev = gout.device
    gd = torch.empty(B, 3 * N, dtype=torch.float32, device=dev) if need[0] else None
    gs = torch.empty(B, N, dtype=torch.float32, device=dev) if need[1] else None
    gc = torch.empty(B, 3 * N, dtype=torch.float32, device=dev) if need[2] else None
    work = torch.empty(max(1, L.eml_sg_rasterise_bwd_full_work_floats(B, N, int(H), int(W))), dtype=torch.float32, device=dev)
    _lib.check(L.eml_sg_rasterise_bwd_f32(_lib.ptr(dirs), _lib.ptr(sizes), _lib.ptr(colors), _lib.ptr(gout), _lib.ptr(gd),
                                          _lib.ptr(gs), _lib.ptr(gc), _lib.ptr(work), B, N, int(H), int(W), 1 if exhaustive else 0,
                                          _lib.current_stream()),
               "eml_sg_rasterise_bwd_f32")
    return gd, gs, gc


def rasterise_bwd_colors_raw(dirs, sizes, gout, pano_hw, exhaustive=False, legacy=False):
    """d loss / d colors (B, 3N) through ``eml_sg_rasterise_bwd_colors_ex_f32``: the forward's per-patch light lists, per-tile
    partial sums added in tile order.  ``exhaustive``: every light for every tile (what the culled launch equals bit for bit);
    ``legacy``: the round-1 kernel (one workgroup per 8 lights sweeping the whole panorama) -- the independent check."""
    H, W = pano_hw
    B, N = sizes.shape
    L = _lib.lib()
    gout = gout.contiguous()
    gcol = torch.empty(B, 3 * N, dtype=torch.float32, device=gout.device)
    if legacy:
        _lib.check(L.eml_sg_rasterise_bwd_colors_f32(_lib.ptr(dirs), _lib.ptr(sizes), _lib.ptr(gout), _lib.ptr(gcol), B, N, int(H),
                                                     int(W), _lib.current_stream()), "eml_sg_rasterise_bwd_colors_f32")
        return gcol
    work = torch.empty(max(1, L.eml_sg_rasterise_bwd_work_floats(B, N, int(H), int(W))), dtype=torch.float32, device=gout.device)
    _lib.check(L.eml_sg_rasterise_bwd_colors_ex_f32(_lib.ptr(dirs), _lib.ptr(sizes), _lib.ptr(gout), _lib.ptr(gcol), _lib.ptr(work),
                                                    B, N, int(H), int(W), 1 if exhaustive else 0, _lib.current_stream()),
               "eml_sg_rasterise_bwd_colors_ex_f32")
    return gcol


def rasterise_raw(dirs, sizes, colors, pano_hw=(128, 256), exhaustive=False, count=False):
    """``eml_sg_rasterise_ex_f32`` (no autograd): the panorama and, with ``count``, the number of exponentials the launch
    evaluated.  ``exhaustive``: every light for every pixel, in the reference's order (util.py:239-244) -- what the
    hierarchically culled default must equal bit for bit (tests); the bench reports both counts."""
    H, W = pano_hw
    d = _lib.require_gpu_tensor(dirs, "dirs")
    s = _lib.require_gpu_tensor(sizes, "sizes")
    c = _lib.require_gpu_tensor(colors, "colors")
    B, N = s.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=d.device)
    n = torch.zeros(1, dtype=torch.int64, device=d.device) if count else None
    _lib.check(_lib.lib().eml_sg_rasterise_ex_f32(_lib.ptr(d), _lib.ptr(s), _lib.ptr(c), _lib.ptr(out), B, N, int(H), int(W),
                                                  1 if exhaustive else 0, _lib.ptr(n), _lib.current_stream()),
               "eml_sg_rasterise_ex_f32")
    return (out, int(n.item())) if count else out


def convert_to_panorama(dirs, sizes, colors, pano_hw=(128, 256)):
    """SG lobes -> equirect panorama ``(B, 3, H, W)``; reference ``util.py:222-245``.

    dirs ``(B, 3N)``, sizes ``(B, N)``, colors ``(B, 3N)``.  ``pano_hw`` defaults to the
    reference's hard-coded 128 x 256 (``W`` must be ``2H``).  Differentiable in all three inputs, like the reference's
    torch arithmetic (once: the backward is not itself differentiable).  A backward that needs only ``colors`` runs the
    colour-gradient kernel alone; one that needs ``dirs`` or ``sizes`` runs the full-gradient kernel.
    """
    H, W = pano_hw
    d = _lib.require_gpu_tensor(dirs, "dirs")
    s = _lib.require_gpu_tensor(sizes, "sizes")
    c = _lib.require_gpu_tensor(colors, "colors")
    B, N = s.shape
    if d.shape != (B, 3 * N) or c.shape != (B, 3 * N):
        raise ValueError("expected dirs (B,3N), sizes (B,N), colors (B,3N); got %s %s %s"
                         % (tuple(d.shape), tuple(s.shape), tuple(c.shape)))
    if B == 0:
        return c.new_zeros(0, 3, int(H), int(W))
    return _Rasterise.apply(d, s, c, int(H), int(W))


def _per_sample(value, B, name):
    """A Python number goes by value and holds for the batch; a device tensor ((B,) or 0-d) gives one f64 value per sample.
    Returns (by-value float, device tensor or None)."""
    if isinstance(value, torch.Tensor):
        if not value.is_cuda:
            raise _lib.EmlightHipError("%s must be a Python number or a tensor on the MI355X (got %s)" % (name, value.device))
        if value.dim() == 0:
            value = value.expand(B)
        if value.shape != (B,):
            raise ValueError("%s: expected one value per sample, shape (%d,), got %s" % (name, B, tuple(value.shape)))
        return 0.0, value.to(torch.float64).contiguous()
    return float(value), None


def _warp_arguments(what, bhw, device, new_shape, theta, phi, move):
    """The argument handling that ``warp_panorama`` and ``warp_panorama_depth`` share: the output size from ``new_shape``
    (``(w, h)``, an int ``h`` meaning ``(2h, h)``, ``None`` for the source's) and the three parameters, each a Python number or
    a ``(B,)`` device tensor.  Returns ``(h, w, params, vals)``: ``params`` is the packed ``(B, 3)`` float64 device array if any
    parameter is a tensor (then ``vals`` is zeros), else ``None`` and ``vals`` the three finite by-value numbers."""
    B, H, W = bhw
    if new_shape is None:
        w, h = W, H
    elif isinstance(new_shape, tuple) and len(new_shape) == 2:
        w, h = int(new_shape[0]), int(new_shape[1])
    elif isinstance(new_shape, int):
        w, h = 2 * new_shape, new_shape
    else:
        raise ValueError("new_shape must be (w, h), an int h or None, got %r" % (new_shape,))
    if h < 1 or w < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty image, %d x %d -> %d x %d" % (what, H, W, h, w))
    vals = [_per_sample(v, B, n) for v, n in ((theta, "theta"), (phi, "phi"), (move, "move"))]
    params = None
    if any(t is not None for _, t in vals):
        params = torch.stack([t if t is not None else torch.full((B,), v, dtype=torch.float64, device=device)
                              for v, t in vals], dim=1).contiguous()
        vals = [(0.0, None)] * 3
    elif not all(np.isfinite(v) for v, _ in vals):
        raise ValueError("%s: theta, phi and move must be finite, got %r" % (what, [v for v, _ in vals]))
    return h, w, params, tuple(v for v, _ in vals)


def _forward_only(t, name, what):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise ValueError("%s requires grad: %s is forward only; pass %s.detach()" % (name, what, name))
    return t


def _warp_forward(x, params, vals, hw, return_coords):
    """The one ``eml_pano_warp_f32`` call of ``PanoramaHandler.warp_panorama``: ``x`` (B, H, W, 3), ``params`` (B, 3) float64 or
    ``None`` (then ``vals`` = (theta, phi, move) hold for the batch) -> ``(out, coords or None)``."""
    B, H, W, _ = x.shape
    h, w = hw
    n_sets = B if params is not None else 1
    out = torch.empty(B, h, w, 3, dtype=torch.float32, device=x.device)
    coords = torch.empty(n_sets, h, w, 2, dtype=torch.float64, device=x.device) if return_coords else None
    if B > 0:       # an empty batch has no storage to point at
        _lib.check(_lib.lib().eml_pano_warp_f32(_lib.ptr(x), B, H, W, h, w, vals[0], vals[1], vals[2],
                                                _lib.ptr(params), _lib.ptr(out), _lib.ptr(coords), _lib.current_stream()),
                   "eml_pano_warp_f32")
    return out, coords


def warp_panorama_bwd_raw(grad_out, pano, pano_hw, theta=0.0, phi=0.0, move=0.0, params=None, want_dpano=True,
                          want_dparams=True):
    """``eml_pano_warp_bwd_f32`` (no autograd): the gradients of the warp for ``grad_out`` (B, h, w, 3) float32.  ``pano``
    (B, H, W, 3) float32 is read for ``dparams`` only and may be ``None`` otherwise; ``pano_hw`` = (H, W).  ``params``: the
    (B, 3) float64 device array of per-sample (theta, phi, move), or ``None`` for the three by-value numbers.  Returns
    ``(dpano (B, H, W, 3) float32 or None, dparams (B, 3) float64 or None)``; ``dparams`` has one row per sample also with
    by-value parameters."""
    g = _lib.require_gpu_tensor(grad_out, "grad_out")
    if g.dim() != 4 or g.shape[-1] != 3:
        raise ValueError("grad_out: expected (B, h, w, 3), got %s" % (tuple(g.shape),))
    B, h, w, _ = g.shape
    H, W = int(pano_hw[0]), int(pano_hw[1])
    if not (want_dpano or want_dparams):
        raise ValueError("warp_panorama_bwd_raw: no gradient requested")
    x = None
    if want_dparams:
        x = _lib.require_gpu_tensor(pano, "pano")
        if x.shape != (B, H, W, 3):
            raise ValueError("pano: expected %s, got %s" % ((B, H, W, 3), tuple(x.shape)))
    if params is not None:
        params = _lib.require_gpu_tensor(params, "params", torch.float64)
        if params.shape != (B, 3):
            raise ValueError("params: expected (%d, 3), got %s" % (B, tuple(params.shape)))
    dpano = torch.empty(B, H, W, 3, dtype=torch.float32, device=g.device) if want_dpano else None
    dparams = torch.empty(B, 3, dtype=torch.float64, device=g.device) if want_dparams else None
    if B > 0:
        L = _lib.lib()
        n = L.eml_pano_warp_bwd_work_floats(B, H, W, h, w, 1 if want_dpano else 0, 1 if want_dparams else 0)
        work = torch.empty(max(1, (n + 1) // 2), dtype=torch.float64, device=g.device)      # float64: 8-byte aligned
        _lib.check(L.eml_pano_warp_bwd_f32(_lib.ptr(g), _lib.ptr(x), B, H, W, h, w, float(theta), float(phi), float(move),
                                           _lib.ptr(params), _lib.ptr(dpano), _lib.ptr(dparams), _lib.ptr(work),
                                           _lib.current_stream()), "eml_pano_warp_bwd_f32")
    return dpano, dparams


class _WarpPanorama(torch.autograd.Function):
    """``warp_panorama`` for autograd: inputs ``x`` (B, H, W, 3) and the packed ``params`` (B, 3) float64 or ``None``.  The
    packing (``torch.stack`` of the ``(B,)`` tensors cast to float64) is autograd's, so each parameter tensor receives its
    column in its own dtype and Python numbers get nothing."""

    @staticmethod
    def forward(ctx, x, params, vals, hw, return_coords):
        out, coords = _warp_forward(x, params, vals, hw, return_coords)
        need_params = params is not None and ctx.needs_input_grad[1]
        ctx.save_for_backward(x if need_params else None, params)    # the panorama enters d / d(theta, phi, move) only
        ctx.pano_hw, ctx.vals = (x.shape[1], x.shape[2]), vals
        if not return_coords:
            return out
        ctx.mark_non_differentiable(coords)
        return out, coords

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, *_):
        x, params = ctx.saved_tensors
        need_x, need_params = ctx.needs_input_grad[0], x is not None
        dpano, dparams = warp_panorama_bwd_raw(gout, x, ctx.pano_hw, *ctx.vals, params=params, want_dpano=need_x,
                                               want_dparams=need_params)
        return dpano, dparams, None, None, None


def parse_aspect_ratio(text):
    """``"a:b"`` -> a / b (``util.py:152-153``); anything else is a ``ValueError``."""
    try:
        num, den = [int(x) for x in str(text).split(":")]
        ratio = num / den
    except (ValueError, ZeroDivisionError) as e:
        raise ValueError("crop_image_aspect_ratio must look like '4:3', got %r" % (text,)) from e
    if not ratio > 0:
        raise ValueError("crop_image_aspect_ratio must be positive, got %r" % (text,))
    return ratio


@functools.lru_cache(maxsize=64)
def crop_sample_extent(fov_deg, h, w, ratio):
    """The range of the crop's sample positions, as fractions of the panorama's width and height:
    ``(x_min, x_max, y_min, y_max)`` with position = fraction * W (or H), from the formula of ``util.py:157-174`` in
    float64.  The azimuth depends on the column alone and the elevation is monotonic in the row, so the extremes lie on
    the crop's border (its corners and edge midpoints); only the border is evaluated."""
    scl = np.tan(np.deg2rad(fov_deg) / 2)
    xs, ys = np.linspace(-scl, scl, w), np.linspace(-scl / ratio, scl / ratio, h)
    bx = np.concatenate([xs, xs, np.full(h, xs[0]), np.full(h, xs[-1])])
    by = np.concatenate([np.full(w, ys[0]), np.full(w, ys[-1]), ys, ys])
    r = np.sqrt(by * by + bx * bx + 1)
    bx, by = bx / r, by / r
    bz = np.sqrt(1 - by * by - bx * bx)
    x = (1 + np.arctan2(bx, bz) / np.pi) / 2
    y = (1 + np.arcsin(by) / (np.pi / 2)) / 2
    return float(x.min()), float(x.max()), float(y.min()), float(y.max())


def _check_crop_inside(fov_deg, h, w, ratio, H, W):
    """The reference's interpolator raises ``ValueError`` for a sample outside ``[0, H-1] x [0, W-1]``; so does this,
    on the host, before any launch."""
    if not 0.0 < fov_deg < 180.0:
        raise ValueError("fov_deg must lie in (0, 180), got %r" % (fov_deg,))
    x0, x1, y0, y1 = crop_sample_extent(float(fov_deg), int(h), int(w), float(ratio))
    if x0 * W < 0 or x1 * W > W - 1 or y0 * H < 0 or y1 * H > H - 1:
        raise ValueError("One of the requested xi is out of bounds: a %g degree crop of %d x %d samples rows [%.3f, %.3f] "
                         "and columns [%.3f, %.3f] of a %d x %d panorama" % (fov_deg, h, w, y0 * H, y1 * H, x0 * W, x1 * W, H, W))


class PanoramaHandler(object):
    """The reference's ``PanoramaHandler`` static methods (``util.py:69-185``) on device tensors, one image
    ``(H, W, 3)`` or a batch ``(B, H, W, 3)``."""

    @staticmethod
    def _batched(hdr, name, dtypes=(torch.float32,)):
        if not isinstance(hdr, torch.Tensor) or hdr.dim() not in (3, 4) or hdr.shape[-1] != 3:
            raise ValueError("%s: expected a (H, W, 3) or (B, H, W, 3) tensor, got %s"
                             % (name, tuple(getattr(hdr, "shape", ())) or type(hdr)))
        single = hdr.dim() == 3
        dtype = hdr.dtype if hdr.dtype in dtypes else dtypes[0]
        return _lib.require_gpu_tensor(hdr.unsqueeze(0) if single else hdr, name, dtype), single

    @staticmethod
    def horizontal_rotate_panorama(hdr_img, deg):
        """``util.py:102-105``: a plain ``torch.roll`` along the width by ``int(deg / 360 * W)`` columns.  ``crop_panorama``
        and ``resize_panorama`` fold the same shift into their gathers (``deg=``) and need no rolled copy."""
        return torch.roll(hdr_img, shifts=int(deg / 360.0 * hdr_img.shape[-2]), dims=-2)

    @staticmethod
    def crop_panorama(hdr_img, fov_deg, crop_image_h=720, crop_image_aspect_ratio="4:3", deg=0.0):
        """Perspective crop of an equirect panorama (``util.py:147-185``), rotated by ``deg`` first (``:102-105``):
        ``(B, H, W, 3)`` float32 or uint8 (divided by 255) -> ``(B, 3, h, w)`` float32, channel-first as ``ToTensor``
        hands it to the network (``data.py:64``).  ``fov_deg`` and ``deg``: a Python number for the whole batch (passed by
        value; a shared field of view evaluates each pixel's position once for a run of images) or a ``(B,)`` device
        tensor, one value per sample.  A by-value ``fov_deg`` whose samples leave ``[0, H-1] x [0, W-1]`` raises
        ``ValueError`` before any launch, like the reference's interpolator; a per-sample tensor cannot be checked
        without a host synchronisation, there such pixels come out as NaN.  Nothing is clamped."""
        x, single = PanoramaHandler._batched(hdr_img, "hdr_img", (torch.float32, torch.uint8))
        ratio = parse_aspect_ratio(crop_image_aspect_ratio)
        h = int(crop_image_h)
        w = int(h * ratio)
        if h < 1 or w < 1:
            raise ValueError("empty crop: crop_image_h=%r, aspect %r" % (crop_image_h, crop_image_aspect_ratio))
        B, H, W, _ = x.shape
        fov, fov_t = _per_sample(fov_deg, B, "fov_deg")
        dg, deg_t = _per_sample(deg, B, "deg")
        if fov_t is None:
            _check_crop_inside(fov, h, w, ratio, H, W)
        out = torch.empty(B, 3, h, w, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().eml_pano_crop_f32(_lib.ptr(x), 1 if x.dtype == torch.uint8 else 0, B, H, W, h, w, ratio, fov,
                                                _lib.ptr(fov_t), dg, _lib.ptr(deg_t), _lib.ptr(out), _lib.current_stream()),
                   "eml_pano_crop_f32")
        return out[0] if single else out

    @staticmethod
    def resize_panorama(hdr_img, new_shape, deg=0.0):
        """``util.py:139-144`` with the rotation folded in: ``new_shape`` is ``(w, h)`` or an int ``h`` meaning
        ``(2h, h)``; ``(B, H, W, 3)`` float32 -> ``(B, h, w, 3)``.  The operation is DEFINED here as the box mean: output
        pixel ``(i, j)`` is the mean of its ``(H/h) x (W/w)`` box of source pixels, summed in float64 in a fixed order.
        Only integer factors are accepted (``ValueError`` otherwise).  The reference calls ``cv2.resize(...,
        INTER_AREA)``; cv2 was not available to compare against, so parity with it is neither tested nor claimed."""
        x, single = PanoramaHandler._batched(hdr_img, "hdr_img")
        if isinstance(new_shape, tuple) and len(new_shape) == 2:
            w, h = int(new_shape[0]), int(new_shape[1])
        elif isinstance(new_shape, int):
            w, h = 2 * new_shape, new_shape
        else:
            raise ValueError("new_shape must be (w, h) or an int h, got %r" % (new_shape,))
        B, H, W, _ = x.shape
        if h < 1 or w < 1 or H % h != 0 or W % w != 0:
            raise ValueError("resize_panorama takes integer factors only: %d x %d -> %d x %d" % (H, W, h, w))
        dg, deg_t = _per_sample(deg, B, "deg")
        out = torch.empty(B, h, w, 3, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().eml_pano_resize_area_f32(_lib.ptr(x), B, H, W, h, w, dg, _lib.ptr(deg_t), _lib.ptr(out),
                                                       _lib.current_stream()), "eml_pano_resize_area_f32")
        return out[0] if single else out

    @staticmethod
    def warp_panorama(hdr_img, new_shape=None, theta=0.0, phi=0.0, move=0.0, return_coords=False):
        """The reference's ``resize_exr`` (``GenProjector/util.py:279-343``) with its three constants as arguments
        (``eml_pano_warp_f32``): the panorama as seen after rotating the frame by ``theta`` (about x) and ``phi`` (about the
        rotated y axis), both in degrees, and stepping ``move`` sphere radii along the rotated -z axis -- the crop looks
        along +z, so a negative ``move`` steps toward what the crop shows.  ``(B, H, W, 3)`` float32 -> ``(B, h, w, 3)``,
        bilinear with wrap-around on both axes; ``new_shape`` is ``(w, h)`` or an int ``h`` meaning ``(2h, h)`` as for
        ``resize_panorama``, ``None`` keeps the source's size.  Each parameter: a Python number for the whole batch or a
        ``(B,)`` device tensor; if any is a tensor the three are packed into a ``(B, 3)`` float64 device array (no host
        synchronisation) and every sample is evaluated on its own.  By-value parameters that are not finite raise
        ``ValueError``; a per-sample value that gives no finite position (NaN; ``|move| == 1`` at the one direction that
        falls on the new viewpoint) gives NaN pixels.  ``return_coords``: also the float64 source positions ``(row, col)``,
        ``(n, h, w, 2)`` with ``n = B`` for per-sample parameters, else 1 (``(h, w, 2)`` for a single image); they carry no
        gradient.  With grad mode on and a panorama or a parameter tensor that requires grad, the result is differentiable
        (once; ``eml_pano_warp_bwd_f32``): the panorama's gradient has the panorama's shape, each ``(B,)``
        parameter tensor receives its gradient in its own dtype, Python numbers get none; a position that is an integer
        differentiates in its right-hand cell, a pixel within 0.06 degrees of the source's pole adds nothing to the parameters'
        gradients.  Otherwise the call is the one forward launch, bit for bit."""
        x, single = PanoramaHandler._batched(hdr_img, "hdr_img")
        h, w, params, vals = _warp_arguments("warp_panorama", x.shape[:3], x.device, new_shape, theta, phi, move)
        if torch.is_grad_enabled() and (x.requires_grad or (params is not None and params.requires_grad)):
            res = _WarpPanorama.apply(x, params, vals, (h, w), bool(return_coords))
            out, coords = res if return_coords else (res, None)
        else:
            out, coords = _warp_forward(x, params, vals, (h, w), return_coords)
        if single:
            out = out[0]
            coords = coords[0] if return_coords else None
        return (out, coords) if return_coords else out

    @staticmethod
    def warp_panorama_depth(hdr_img, depth, new_shape=None, theta=0.0, phi=0.0, move=0.0, steps=32, bisections=24,
                            return_hit=False):
        """``warp_panorama`` with the scene's own geometry (``eml_pano_warp_depth_f32``): the panorama AND its depth as seen
        after rotating the frame by ``theta``, ``phi`` (degrees, as ``warp_panorama``) and stepping ``move`` along the rotated -z
        axis, in the UNITS OF ``depth``.  ``depth`` ``(H, W)`` or ``(B, H, W)`` float32 is the distance from the viewpoint to
        the scene along each pixel's direction, finite and > 0.  Every output pixel's ray from the new viewpoint is marched
        (``steps`` equal steps over the interval that must hold the surface) to the first crossing of the depth map, which
        ``bisections`` halvings refine: a light that is close grows and shifts more than one that is far.  Returns
        ``(pano, depth)`` -- ``(B, h, w, 3)`` and ``(B, h, w)`` float32, without the batch axis for a single image; ``pano`` is
        ``None`` for ``hdr_img=None`` (depth only) -- and with ``return_hit`` also the float64 ``(B, h, w, 3)`` array of
        ``(t, row, col)``: the distance along the ray and the source position the pixel was sampled at.  Sampling is bilinear
        with wrapping columns and CLAMPED rows.  ``new_shape`` and the number-or-``(B,)``-tensor parameters are
        ``warp_panorama``'s.  A sample whose depth has a value that is not finite or not > 0, whose parameters are not finite,
        or whose new viewpoint lies on or behind the surface comes out as NaN, all of it.  The depth map is treated as one
        connected surface: regions the source viewpoint never saw are not filled, the surface is stretched across them.
        Forward only: an input that requires grad raises ``ValueError``."""
        what = "warp_panorama_depth"
        for t, name in ((hdr_img, "hdr_img"), (depth, "depth"), (theta, "theta"), (phi, "phi"), (move, "move")):
            _forward_only(t, name, what)
        if not isinstance(depth, torch.Tensor) or depth.dim() not in (2, 3):
            raise ValueError("depth: expected a (H, W) or (B, H, W) tensor, got %s"
                             % (tuple(getattr(depth, "shape", ())) or type(depth),))
        single = depth.dim() == 2
        d = _lib.require_gpu_tensor(depth.unsqueeze(0) if single else depth, "depth")
        B, H, W = d.shape
        x = None
        if hdr_img is not None:
            x, x_single = PanoramaHandler._batched(hdr_img, "hdr_img")
            if x_single != single or x.shape != (B, H, W, 3):
                raise ValueError("hdr_img %s and depth %s do not match" % (tuple(hdr_img.shape), tuple(depth.shape)))
        steps, bisections = int(steps), int(bisections)
        if not 1 <= steps <= 1024 or not 0 <= bisections <= 60:
            raise ValueError("%s: steps in 1..1024 and bisections in 0..60, got %r, %r" % (what, steps, bisections))
        h, w, params, vals = _warp_arguments(what, (B, H, W), d.device, new_shape, theta, phi, move)
        out = torch.empty(B, h, w, 3, dtype=torch.float32, device=d.device) if x is not None else None
        out_d = torch.empty(B, h, w, dtype=torch.float32, device=d.device)
        hit = torch.empty(B, h, w, 3, dtype=torch.float64, device=d.device) if return_hit else None
        if B > 0:
            L = _lib.lib()
            work = torch.empty(max(1, L.eml_pano_warp_depth_work_floats(B, H, W)), dtype=torch.float32, device=d.device)
            _lib.check(L.eml_pano_warp_depth_f32(_lib.ptr(x), _lib.ptr(d), B, H, W, h, w, vals[0], vals[1], vals[2],
                                                 _lib.ptr(params), steps, bisections, _lib.ptr(out), _lib.ptr(out_d),
                                                 _lib.ptr(hit), _lib.ptr(work), _lib.current_stream()),
                       "eml_pano_warp_depth_f32")
        if single:
            out, out_d, hit = (None if out is None else out[0]), out_d[0], (None if hit is None else hit[0])
        return (out, out_d, hit) if return_hit else (out, out_d)


def tonemap_raw(img, gamma=2.4, percentile=50, max_mapping=0.5, clip=True, alpha=None, use_gamma=True, apply=True):
    """``eml_tonemap_f32`` on a batch ``(B, ...)`` of images, with its raw per-image outputs: dict of ``out`` (like ``img``;
    ``None`` without ``apply``), ``P`` = img^(1/gamma), ``n`` (B,) int32 = number of positive values, ``lo`` / ``hi`` (B,) =
    the order statistics at floor / floor + 1 of the virtual index ``(n - 1) * percentile / 100``, ``r`` (B,) the
    percentile, ``alpha`` (B,).  ``alpha``: a Python number or a (B,) device tensor to use instead of the computed one."""
    x = _lib.require_gpu_tensor(img, "img")
    B = x.shape[0]
    n = x[0].numel() if B else 1
    if isinstance(alpha, torch.Tensor):
        alpha_t = _lib.require_gpu_tensor(alpha.expand(B) if alpha.dim() == 0 else alpha, "alpha")
        if alpha_t.shape != (B,):
            raise ValueError("alpha: expected shape (%d,), got %s" % (B, tuple(alpha_t.shape)))
    elif alpha is not None:
        alpha_t = torch.full((B,), float(alpha), dtype=torch.float32, device=x.device)
    else:
        alpha_t = None
    L = _lib.lib()
    P = torch.empty_like(x)
    out = torch.empty_like(x) if apply else None
    cnt = torch.empty(B, dtype=torch.int32, device=x.device)
    stats = torch.empty(B, 4, dtype=torch.float32, device=x.device)
    work = torch.empty(max(1, L.eml_tonemap_work_floats(B)), dtype=torch.int32, device=x.device)
    _lib.check(L.eml_tonemap_f32(_lib.ptr(x), B, n, 1 if use_gamma else 0, float(gamma) if use_gamma else 1.0, float(percentile),
                                 float(max_mapping), _lib.ptr(alpha_t), 1 if clip else 0, _lib.ptr(P), _lib.ptr(out),
                                 _lib.ptr(cnt), _lib.ptr(stats), _lib.ptr(work), _lib.current_stream()), "eml_tonemap_f32")
    return {"out": out, "P": P, "n": cnt, "lo": stats[:, 0], "hi": stats[:, 1], "r": stats[:, 2], "alpha": stats[:, 3]}


class TonemapHDR(object):
    """Global tonemap: alpha maps the ``percentile`` of I^(1/gamma) to ``max_mapping``
    (reference ``util.py:36-66``).  numpy input: numpy, host side (visualisation).  A device tensor ``(3, h, w)`` or a
    batch ``(B, 3, h, w)``: the HIP kernels, one alpha per image, no host round trip; returns ``(tensor, alpha tensor)``."""

    def __init__(self, gamma=2.4, percentile=50, max_mapping=0.5):
        self.gamma, self.percentile, self.max_mapping = gamma, percentile, max_mapping

    def __call__(self, numpy_img, clip=True, alpha=None, gamma=True):
        if isinstance(numpy_img, torch.Tensor):
            return self._tensor(numpy_img, clip, alpha, gamma)
        img = np.power(numpy_img, 1 / self.gamma) if gamma else numpy_img
        pos = img > 0
        ref = np.percentile(img[pos], self.percentile) if pos.any() else np.percentile(img, self.percentile)
        if alpha is None:
            alpha = self.max_mapping / (ref + 1e-10)
        out = np.multiply(alpha, img)
        if clip:
            out = np.clip(out, 0, 1)
        return out.astype("float32"), alpha

    def _tensor(self, img, clip, alpha, gamma):
        if img.dim() not in (3, 4):
            raise ValueError("expected a (3, h, w) image or a (B, 3, h, w) batch, got %s" % (tuple(img.shape),))
        single = img.dim() == 3
        raw = tonemap_raw(img.unsqueeze(0) if single else img, self.gamma, self.percentile, self.max_mapping, clip=clip,
                          alpha=alpha, use_gamma=bool(gamma))
        return (raw["out"][0], raw["alpha"][0]) if single else (raw["out"], raw["alpha"])
