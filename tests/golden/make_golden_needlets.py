#!/usr/bin/env python
"""Generate tests/golden/needlets.npz by running the REAL reference ``Needlets/sphere_needlets.py`` on the CPU (f64).

Run only where the reference checkout exists (see ``make_golden.py``); about a minute:

    python tests/golden/make_golden_needlets.py

The reference imports ``healpy`` (not installed) and its own ``utils`` (needs OpenEXR and cv2).  Two stand-ins are placed in
``sys.modules`` before the import: an empty ``utils``, and a ``healpy`` with ``pix2ang``, ``pix2vec`` and ``ringinfo`` of the
RING scheme written from the published formulae (Gorski et al. 2005, section 4.1).  Only ``spneedlet_eval``, ``fun_b`` and
``spharmonic_eval`` are called; ``SNvertex`` / ``spneedlet_pair`` pass generators to ``np.hstack`` and fail under numpy 2, so
``[Y_00, beta_0 ... beta_jmax]`` (``sphere_needlets.py:236``) is stacked here.

No point is ever placed at ``theta = pi`` exactly: ``scipy.special.lpmn(.., -1.0)`` returns ``P_l(-1) = 1`` instead of
``(-1)^l``, so the reference's row there is wrong.  The grid images' last row (``theta = pi``) is zero
and that row is left out of the reference-made matrix.

Contents (arrays only):
  a/j<jmax>/{theta,phi,matrix}        scattered points: 24 for jmax 1, 2, 3 and 6 for jmax 4; (n, K) matrix rows
  b/window                            fun_b(l / 2^j, 2) for j = 0..4, l = 1..32: (5, 32), entry [j, l - 1]
  c/<H>x<W>_j<jmax>/{image,coeffs}    image (2, 3, H, W) f32; coeffs (2, K, 3) f64 = sum im * SN_Matrix * solidAngle
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EMLIGHT_REFERENCE", "/root/reference")


# ---------------------------------------------------------------------------------------------- the healpy stand-in
def _ring_table(nside):
    """(z, count, shift) of ring 1 .. 4 nside - 1."""
    n, out = nside, []
    for i in range(1, 4 * n):
        if i < n:
            out.append((1.0 - i * i / (3.0 * n * n), 4 * i, 0.5))
        elif i <= 3 * n:
            out.append((4.0 / 3.0 - 2.0 * i / (3.0 * n), 4 * n, 0.5 * ((i - n + 1) % 2)))
        else:
            m = 4 * n - i
            out.append((-(1.0 - m * m / (3.0 * n * n)), 4 * m, 0.5))
    return out


def _all_pixels(nside):
    z, phi = [], []
    for zr, m, shift in _ring_table(nside):
        z.append(np.full(m, zr))
        phi.append((np.arange(m) + shift) * (2.0 * np.pi / m))
    return np.concatenate(z), np.concatenate(phi)


def _pix2ang(nside, ipix):
    z, phi = _all_pixels(nside)
    ipix = np.asarray(list(ipix) if not isinstance(ipix, np.ndarray) else ipix, dtype=np.int64)
    return np.arccos(z[ipix]), phi[ipix]


def _pix2vec(nside, ipix):
    theta, phi = _pix2ang(nside, ipix)
    return np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)


def _ringinfo(nside, ring):
    tab = _ring_table(nside)
    counts = np.array([m for _, m, _ in tab], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    z = np.array([t[0] for t in tab])
    r = np.asarray(ring, dtype=np.int64) - 1
    return start[r], counts[r], z[r], np.sqrt(1.0 - z[r] ** 2), np.array([t[2] == 0.5 for t in tab])[r]


def load_reference():
    hp = types.ModuleType("healpy")
    hp.pix2ang, hp.pix2vec, hp.ringinfo = _pix2ang, _pix2vec, _ringinfo
    sys.modules["healpy"] = hp
    sys.modules["utils"] = types.ModuleType("utils")
    sys.path.insert(0, os.path.join(REF, "Needlets"))
    import sphere_harmonics
    import sphere_needlets
    return sphere_needlets, sphere_harmonics


def sn_row(sn, sh, theta, phi, jmax):
    """One row of SN_matrix (sphere_needlets.py:213-236, without the symmetrised halves)."""
    beta = sn.spneedlet_eval(theta, phi, jmax)
    y00 = sh.spharmonic_eval(0, 0, theta, phi).real
    return np.concatenate([[y00]] + [np.asarray(beta[j], dtype=np.float64) for j in range(jmax + 1)])


def solid_angles(H, W):
    """getSolidAngleMap (Needlets/utils.py:35-50; that module does not import here), flattened."""
    y = np.arange(0, H)
    theta = (1.0 - ((y + 0.5) / H)) * np.pi
    row = ((np.pi * 2) / W) * (np.cos(theta - ((np.pi / H) / 2.0)) - np.cos(theta + ((np.pi / H) / 2.0)))
    return np.repeat(row[:, np.newaxis], W, axis=1).reshape((-1))


def main():
    warnings.simplefilter("ignore")
    sn, sh = load_reference()
    out = {}
    # (a) scattered points: both poles' neighbourhoods and the seam of phi
    special = [(0.0, 0.3), (np.pi - 1e-6, 1.0), (1.0, 0.0), (2.0, 2.0 * np.pi)]
    for jmax, n in ((1, 24), (2, 24), (3, 24), (4, 6)):
        g = np.random.default_rng([7, jmax])
        theta = np.concatenate([[s[0] for s in special], np.arccos(g.uniform(-1.0, 1.0, n - 4))])
        phi = np.concatenate([[s[1] for s in special], g.uniform(0.0, 2.0 * np.pi, n - 4)])
        assert np.all(theta < np.pi)
        out["a/j%d/theta" % jmax], out["a/j%d/phi" % jmax] = theta, phi
        out["a/j%d/matrix" % jmax] = np.stack([sn_row(sn, sh, t, p, jmax) for t, p in zip(theta, phi)])
        print("a: jmax %d done" % jmax, flush=True)
    # (b) the window
    out["b/window"] = np.array([[sn.fun_b(l / 2.0 ** j, 2.0) for l in range(1, 33)] for j in range(5)])
    # (c) grid coefficients on the reference grid of mat_gen2.py:22-25, the theta = pi row left out
    for H, W, jmax in ((12, 24, 1), (12, 24, 2), (16, 32, 3)):
        g = np.random.default_rng([11, H, W, jmax])
        im = (g.random((2, 3, H, W)) ** 4 * 50.0 + 0.01).astype(np.float32)
        im[:, :, -1, :] = 0.0
        pix1, pix2 = np.linspace(0, 1, H) * np.pi, np.linspace(0, 2, W) * np.pi
        X, Y = np.meshgrid(pix2, pix1)
        X, Y = X.reshape(-1)[:-W], Y.reshape(-1)[:-W]
        M = np.stack([sn_row(sn, sh, t, p, jmax) for t, p in zip(Y, X)])                # (P - W, K)
        flat = im.astype(np.float64).reshape(2, 3, H * W)[:, :, :-W] * solid_angles(H, W)[:-W]
        out["c/%dx%d_j%d/image" % (H, W, jmax)] = im
        out["c/%dx%d_j%d/coeffs" % (H, W, jmax)] = np.einsum("bcp,pk->bkc", flat, M)
        print("c: %dx%d jmax %d done" % (H, W, jmax), flush=True)
    path = os.path.join(HERE, "needlets.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
