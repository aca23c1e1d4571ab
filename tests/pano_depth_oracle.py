"""Float64 numpy restatement of the depth-aware panorama warp (csrc/pano_warp_depth.hip, ``eml_pano_warp_depth_f32``) and of the
per-anchor depth (``eml_gt_anchor_depth_f64``), with an analytic scene to pin the restatement to.

The algorithm, as ``include/emlight_hip_ext.h`` states it.  For output pixel ``(i, j)``: ``e = Rp Rt d(i, j)``,
``m = Rp Rt (0, 0, -1)`` (``tests/warp_oracle.py``'s frame), viewpoint ``c = move * m``, ray ``P(t) = c + t e``.  The position of
a point is ``warp_oracle``'s last step with the kernel's 2^-28 px snap; the depth there is bilinear with wrapping columns
and CLAMPED rows.  ``g(t) = |P(t)| - D(P(t))`` (``|P| == 0`` counts as inside); bracket ``t_lo = max(0, dmin - |c|)``,
``t_hi = dmax + |c|``; march ``t_k = t_lo + (t_hi - t_lo) k / steps`` to the first ``g(t_k) >= 0`` (``k = steps`` closes the
bracket unasked), then ``bisections`` halvings; ``t`` is the midpoint of what is left.

The scene: an axis-aligned box room ``[-1.5, 1.2] x [-2, 3] x [-2.5, 2]`` around the origin, optionally with a sphere of radius
0.45 at ``(0.3, 1.2, -0.9)``, and a smooth procedural colour at the hit point.  The source panorama and depth are the scene seen
from the origin at the pixel directions; the truth from any other viewpoint is the closed-form ray hit."""
import math

import numpy as np

from tests import warp_oracle

SNAP = 1.0 / (1 << 28)
BOX_LO = np.array([-1.5, -2.0, -2.5])
BOX_HI = np.array([1.2, 3.0, 2.0])
SPHERE_C = np.array([0.3, 1.2, -0.9])
SPHERE_R = 0.45
# what test_gpu_pano_depth.py runs the kernel on, and test_pano_depth_abi.py probes the oracle's stability on: (H, W, h, w) and
# one (theta, phi, move) per sample.  |move| <= 0.8 keeps every viewpoint inside the room (nearest wall 1.2) and outside the
# sphere (nearest point 1.08).
GPU_SHAPES = [(16, 32, 8, 16), (32, 64, 16, 32), (12, 40, 7, 9)]
GPU_PARAMS = [(0.0, 0.0, -0.8), (20.0, -35.0, 0.6), (-15.0, 130.0, -0.5)]


# ------------------------------------------------------------------------------------------------ the algorithm
def pixel_directions(h, w):
    """``d(i, j)``, ``(h * w, 3)``: ``lat = i pi / h - pi / 2``, ``lon = j 2 pi / w``, no half-pixel offset."""
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    lat = i * math.pi / h - math.pi / 2 + 0 * j
    lon = j * (2 * math.pi) / w + 0 * i
    return np.stack([np.sin(lat), np.sin(lon) * np.cos(lat), -np.cos(lon) * np.cos(lat)], axis=-1).reshape(-1, 3)


def frame(h, w, theta_deg=0.0, phi_deg=0.0):
    """``(e (h * w, 3), m (3,))``."""
    Rt, Rp = warp_oracle.rotations(theta_deg, phi_deg)
    e = (Rp @ (Rt @ pixel_directions(h, w).T)).T
    return e, Rp @ (Rt @ np.array([0.0, 0.0, -1.0]))


def _snap(x):
    n = np.rint(x)
    return np.where(np.abs(x - n) < SNAP, n, x)


def position(P, H, W):
    """``(row, col, |P|, ok)`` of points ``(n, 3)``; no position (NaN, ``ok`` false) where ``|P|`` is 0 or not finite."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2])
        ok = np.isfinite(n) & (n > 0)
        s = P / np.where(ok, n, 1.0)[:, None]
        az = np.arctan2(s[:, 1], -s[:, 2])
        az = np.where(az < 0, az + 2 * math.pi, az)
        row = _snap((np.arcsin(np.clip(s[:, 0], -1.0, 1.0)) + math.pi / 2) / math.pi * H)
        col = _snap(az / (2 * math.pi) * W)
    ok = ok & np.isfinite(row) & np.isfinite(col)
    return np.where(ok, row, np.nan), np.where(ok, col, np.nan), n, ok


def taps(row, col, H, W):
    """Clamped rows, wrapping columns: ``(i0, i1, j0, j1, yd, xd)`` of finite positions."""
    fr, fc = np.floor(row), np.floor(col)
    i0 = np.minimum(fr.astype(np.int64), H - 1)
    i1 = np.minimum(i0 + 1, H - 1)
    j0 = fc.astype(np.int64) % W
    j1 = (j0 + 1) % W
    return i0, i1, j0, j1, row - fr, col - fc


def lookup(depth, row, col):
    """The bilinear depth at finite positions, float64, products summed in the order 00, 01, 10, 11."""
    H, W = depth.shape
    D = depth.astype(np.float64)
    i0, i1, j0, j1, yd, xd = taps(row, col, H, W)
    v = D[i0, j0] * ((1 - yd) * (1 - xd))
    v = v + D[i0, j1] * ((1 - yd) * xd)
    v = v + D[i1, j0] * (yd * (1 - xd))
    v = v + D[i1, j1] * (yd * xd)
    return v


def sample(img, row, col):
    """The clamped-row bilinear sample of ``img`` ``(H, W, 3)``, summed in float64, rounded to float32 once; NaN positions
    give NaN."""
    H, W, _ = img.shape
    row, col = np.asarray(row, dtype=np.float64), np.asarray(col, dtype=np.float64)
    ok = np.isfinite(row) & np.isfinite(col)
    i0, i1, j0, j1, yd, xd = taps(np.where(ok, row, 0.0), np.where(ok, col, 0.0), H, W)
    yd, xd = yd[..., None], xd[..., None]
    x = img.astype(np.float64)
    v = x[i0, j0] * ((1 - yd) * (1 - xd))
    v = v + x[i0, j1] * ((1 - yd) * xd)
    v = v + x[i1, j0] * (yd * (1 - xd))
    v = v + x[i1, j1] * (yd * xd)
    out = v.astype(np.float32)
    out[~ok] = np.nan
    return out


def search_rays(depth, e, c, steps=32, bisections=24, scale=1.0):
    """The ray search for directions ``e`` ``(n, 3)`` from the viewpoint ``c`` ``(3,)``.  Returns a dict: ``t``, ``row``, ``col``
    ``(n,)`` (NaN for an invalid sample or a hit without a position), ``t_lo``, ``t_hi``, ``valid``.  ``scale`` multiplies
    ``|P|`` inside ``g`` (the stability probe of the tests; 1.0 is the algorithm)."""
    H, W = depth.shape
    e = np.asarray(e, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(c, dtype=np.float64)
    n = e.shape[0]
    nan = np.full(n, np.nan)
    out = {"t": nan, "row": nan.copy(), "col": nan.copy(), "t_lo": np.nan, "t_hi": np.nan, "valid": False}
    if not (np.isfinite(depth).all() and (depth > 0).all() and np.isfinite(c).all()):
        return out
    crow, ccol, clen, cok = position(c[None, :], H, W)
    clen = float(clen[0])
    if clen > 0 and (not cok[0] or clen >= float(lookup(depth, crow, ccol)[0])):
        return out
    t_lo, t_hi = max(0.0, float(depth.min()) - clen), float(depth.max()) + clen

    def outside(t, idx):
        row, col, length, ok = position(c[None, :] + t[:, None] * e[idx], H, W)
        res = np.zeros(len(idx), dtype=bool)
        res[ok] = length[ok] * scale - lookup(depth, row[ok], col[ok]) >= 0.0
        return res

    a, b = np.full(n, t_lo), np.full(n, t_hi)
    active = np.arange(n)
    for k in range(1, steps):
        if active.size == 0:
            break
        tk = np.full(active.size, t_lo + (t_hi - t_lo) * float(k) / float(steps))
        out_k = outside(tk, active)
        b[active[out_k]] = tk[out_k]
        a[active[~out_k]] = tk[~out_k]
        active = active[~out_k]
    everyone = np.arange(n)
    for _ in range(bisections):
        mid = 0.5 * (a + b)
        o = outside(mid, everyone)
        b = np.where(o, mid, b)
        a = np.where(o, a, mid)
    t = 0.5 * (a + b)
    row, col, _, ok = position(c[None, :] + t[:, None] * e, H, W)
    out.update(t=np.where(ok, t, np.nan), row=row, col=col, t_lo=t_lo, t_hi=t_hi, valid=True)
    return out


def warp(depth, h, w, theta_deg=0.0, phi_deg=0.0, move=0.0, steps=32, bisections=24, scale=1.0):
    """``search_rays`` in the frame of ``(theta, phi, move)``; arrays come back ``(h, w)``."""
    if not all(math.isfinite(v) for v in (theta_deg, phi_deg, move)):
        nan = np.full((h, w), np.nan)
        return {"t": nan, "row": nan.copy(), "col": nan.copy(), "t_lo": np.nan, "t_hi": np.nan, "valid": False}
    e, m = frame(h, w, theta_deg, phi_deg)
    r = search_rays(depth, e, move * m, steps, bisections, scale)
    for k in ("t", "row", "col"):
        r[k] = r[k].reshape(h, w)
    return r


def tolerance(r, steps=32, bisections=24):
    """Twice the width of the interval the search ends with."""
    return 2.0 * (r["t_hi"] - r["t_lo"]) / (steps * 2.0 ** bisections)


def anchor_depth(depth, idx, N):
    """``sum w D / sum w`` over each anchor's cell, ``w = sin((row + 0.5) / H pi)``; pixels that are not finite are left out."""
    H, W = depth.shape
    wgt = np.repeat(np.sin((np.arange(H) + 0.5) / H * math.pi), W)
    d = depth.reshape(-1).astype(np.float64)
    ok = np.isfinite(d)
    idx = np.asarray(idx).reshape(-1)
    num = np.bincount(idx[ok], weights=(wgt * np.where(ok, d, 0.0))[ok], minlength=N)
    den = np.bincount(idx[ok], weights=wgt[ok], minlength=N)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


# ------------------------------------------------------------------------------------------------ the analytic scene
def ray_hit(origin, dirs, sphere=False):
    """Distance along unit ``dirs`` ``(n, 3)`` from ``origin`` (inside the room, outside the sphere) to the nearest surface."""
    origin = np.asarray(origin, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        tb = np.where(dirs > 0, (BOX_HI - origin) / dirs, np.where(dirs < 0, (BOX_LO - origin) / dirs, np.inf))
    t = tb.min(axis=1)
    if sphere:
        oc = origin - SPHERE_C
        bq = dirs @ oc
        disc = bq * bq - (oc @ oc - SPHERE_R ** 2)
        with np.errstate(invalid="ignore"):
            ts = -bq - np.sqrt(disc)
        t = np.where((disc > 0) & (ts > 0) & (ts < t), ts, t)
    return t


def colour(points):
    """A smooth positive colour field, ``(n, 3)``."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    return np.stack([1.5 + np.sin(1.3 * x + 0.4 * y) * np.cos(0.7 * z),
                     1.2 + 0.8 * np.cos(0.9 * y - 0.5 * z),
                     2.0 + np.sin(0.6 * x * z + 0.3) * np.sin(1.1 * y)], axis=-1)


def source(H, W, sphere=False):
    """``(pano (H, W, 3) float32, depth (H, W) float32)``: the scene from the origin at the pixel directions."""
    d = pixel_directions(H, W)
    t = ray_hit(np.zeros(3), d, sphere)
    return colour(t[:, None] * d).astype(np.float32).reshape(H, W, 3), t.astype(np.float32).reshape(H, W)


def truth(c, e, sphere=False):
    """``(t_true, visible)``: the closed-form hit distance of the rays ``c + t e`` and whether the hit point is seen from the
    origin (nothing nearer on the segment from the origin to it)."""
    e = np.asarray(e, dtype=np.float64).reshape(-1, 3)
    unit = e / np.linalg.norm(e, axis=1, keepdims=True)
    t = ray_hit(c, unit, sphere)
    hit = np.asarray(c, dtype=np.float64)[None, :] + t[:, None] * unit
    dist = np.linalg.norm(hit, axis=1)
    seen = ray_hit(np.zeros(3), hit / dist[:, None], sphere)
    return t, seen >= dist * (1 - 1e-9)
