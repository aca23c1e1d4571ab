"""Float64 numpy restatement of the panorama warp (reference ``GenProjector/util.py:279-343``, ``resize_exr``) and of
bilinear sampling with wrap-around on both axes (what ``cv2.remap(..., INTER_LINEAR, borderMode=BORDER_WRAP)`` computes,
without cv2's quantisation of the weights to 1/32 px).  The reference forms its rotation matrices and its index grids in
float32; everything here is float64, so the two agree to float32 accuracy only (``tests/golden/warp.npz`` stores by how much).

Conventions: ``theta``, ``phi`` in degrees, ``move`` in sphere radii; the source is ``(H, W, 3)``, the output grid ``h x w``;
positions are ``(row, col)`` in source pixels, ``row`` in [0, H], ``col`` in [0, W] (both ends occur)."""
import math

import numpy as np

# (theta, phi, move) and (H, W, h, w) of tests/golden/warp.npz
PARAMS = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.4), (25.0, 0.0, 0.0), (0.0, 77.3, 0.0), (-30.0, 130.0, 0.6), (10.0, -200.0, -0.5),
          (90.0, 45.0, 0.9), (5.0, 5.0, 1.5)]
SHAPES = [(64, 128, 24, 40), (32, 64, 48, 80)]


def case_name(k, shape):
    return "p%d/%dx%d_%dx%d" % ((k,) + tuple(shape))


def rotations(theta_deg, phi_deg):
    """``(Rt, Rp)``: the rotation about x by theta, and Rodrigues' rotation about ``(0, cos theta, sin theta)`` whose sine is
    ``-sin(phi)`` (the reference negates it, ``util.py:301``)."""
    t, p = theta_deg / 180 * math.pi, phi_deg / 180 * math.pi
    ct, st = math.cos(t), math.sin(t)
    c, s = math.cos(p), -math.sin(p)
    ay, az = ct, st
    Rt = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]], dtype=np.float64)
    Rp = np.array([[c, -az * s, ay * s],
                   [az * s, c + ay * ay * (1 - c), ay * az * (1 - c)],
                   [-ay * s, az * ay * (1 - c), c + az * az * (1 - c)]], dtype=np.float64)
    return Rt, Rp


def positions(H, W, h, w, theta_deg=0.0, phi_deg=0.0, move=0.0):
    """``(row, col)``, each ``(h, w)`` float64.  A pixel whose shifted direction has no length (``|move| == 1`` only) or is
    not finite gives NaN."""
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    lat = i * math.pi / h - math.pi / 2 + 0 * j
    lon = j * (2 * math.pi) / w + 0 * i
    d = np.stack([np.sin(lat), np.sin(lon) * np.cos(lat), -np.cos(lon) * np.cos(lat)]).reshape(3, -1)
    Rt, Rp = rotations(theta_deg, phi_deg)
    m = Rp @ (Rt @ np.array([0.0, 0.0, -1.0]))
    v = Rp @ (Rt @ d) + move * m[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt((v * v).sum(axis=0))
        ok = np.isfinite(n) & (n > 0)
        s = v / np.where(ok, n, 1.0)
        row = (np.arcsin(np.clip(s[0], -1.0, 1.0)) + math.pi / 2) / math.pi * H
        col = np.arctan2(s[1], -s[2]) % (2 * math.pi) / (2 * math.pi) * W
    row[~ok], col[~ok] = np.nan, np.nan
    return row.reshape(h, w), col.reshape(h, w)


def unit_vectors(row, col, H, W):
    """The directions that source positions stand for, ``(..., 3)``: the inverse of the last step of ``positions``."""
    lat = np.asarray(row, dtype=np.float64) / H * math.pi - math.pi / 2
    lon = np.asarray(col, dtype=np.float64) / W * (2 * math.pi)
    return np.stack([np.sin(lat), np.sin(lon) * np.cos(lat), -np.cos(lon) * np.cos(lat)], axis=-1)


def chord(row_a, col_a, row_b, col_b, H, W):
    """The worst Euclidean distance between the unit vectors of two position maps.  Well conditioned at the poles, where the
    column alone is not (every column is the same point there)."""
    diff = unit_vectors(row_a, col_a, H, W) - unit_vectors(row_b, col_b, H, W)
    return float(np.sqrt((diff * diff).sum(axis=-1)).max())


def sample(img, row, col):
    """Bilinear taps of ``img`` ``(H, W, 3)`` at ``(row, col)`` with wrap-around on both axes: the taps are ``floor`` modulo the
    size and their ``+1`` neighbours, also modulo; the weights are the float64 fractions; the four products are summed in
    float64 in the order 00, 01, 10, 11 and rounded to float32 once.  A NaN position gives NaN."""
    H, W, _ = img.shape
    row, col = np.asarray(row, dtype=np.float64), np.asarray(col, dtype=np.float64)
    ok = np.isfinite(row) & np.isfinite(col)
    r, c = np.where(ok, row, 0.0), np.where(ok, col, 0.0)
    fr, fc = np.floor(r), np.floor(c)
    yd, xd = (r - fr)[..., None], (c - fc)[..., None]
    i0, j0 = fr.astype(np.int64) % H, fc.astype(np.int64) % W
    i1, j1 = (i0 + 1) % H, (j0 + 1) % W
    x = img.astype(np.float64)
    v = x[i0, j0] * ((1 - yd) * (1 - xd))
    v = v + x[i0, j1] * ((1 - yd) * xd)
    v = v + x[i1, j0] * (yd * (1 - xd))
    v = v + x[i1, j1] * (yd * xd)
    out = v.astype(np.float32)
    out[~ok] = np.nan
    return out


def warp(img, h, w, theta_deg=0.0, phi_deg=0.0, move=0.0):
    row, col = positions(img.shape[0], img.shape[1], h, w, theta_deg, phi_deg, move)
    return sample(img, row, col)
