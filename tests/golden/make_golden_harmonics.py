#!/usr/bin/env python
"""Generate tests/golden/harmonics.npz by running the REAL reference ``Needlets/sphere_harmonics.py`` on the CPU (f64).

Run only where the reference checkout exists (see ``make_golden.py``) and scipy still has ``lpmn``; a few seconds:

    python tests/golden/make_golden_harmonics.py

No point is ever placed at ``theta = pi`` exactly: ``scipy.special.lpmn(.., -1.0)`` is wrong there.
The grid images' last row (``theta = pi``) is zero and that row is left out of the reference-made matrix.  Every stored
value is checked against ``tests/harmonic_oracle.py`` to 1e-9 of the largest entry before the file is written.

Contents (arrays only):
  a/theta, a/phi                      24 scattered points, among them theta = 0, theta = pi - 1e-6, phi = 0 and phi = 2 pi
  a/symmetrised_l<lmax>               spharmonic (sphere_harmonics.py:94-115) at those points, lmax 1, 4, 32: (24, K)
  a/graphics_l<lmax>                  shEvaluate (:60-70) at the same points, lmax 4, 8: (24, K)
  c/<H>x<W>_l<lmax>/{image,coeffs}    image (2, 3, H, W) f32; coeffs (2, K, 3) f64 = sum im * SH_matrix * solidAngle on the
                                      grid of mat_gen2.py:22-25: 12x24 at lmax 4 with spharmonic, 16x32 at lmax 8 with shEvaluate
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EMLIGHT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def solid_angles(H, W):
    """getSolidAngleMap (Needlets/utils.py:35-50; that module needs OpenEXR and cv2 to import), flattened."""
    y = np.arange(0, H)
    theta = (1.0 - ((y + 0.5) / H)) * np.pi
    row = ((np.pi * 2) / W) * (np.cos(theta - ((np.pi / H) / 2.0)) - np.cos(theta + ((np.pi / H) / 2.0)))
    return np.repeat(row[:, np.newaxis], W, axis=1).reshape((-1))


def reference_matrix(sh, theta, phi, lmax, convention):
    if convention == "symmetrised":
        return sh.spharmonic(theta, phi, lmax)
    return np.stack([sh.shEvaluate(float(t), float(p), lmax)[0, 0] for t, p in zip(theta, phi)])


def main():
    warnings.simplefilter("ignore")
    sys.path.insert(0, os.path.join(REF, "Needlets"))
    import sphere_harmonics as sh
    from tests import harmonic_oracle as oracle

    def checked(got, want, what):
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("%s: reference vs oracle %.2e" % (what, err), flush=True)
        assert err <= 1e-9, what
        return got

    out = {}
    special = [(0.0, 0.3), (np.pi - 1e-6, 1.0), (1.0, 0.0), (2.0, 2.0 * np.pi)]
    g = np.random.default_rng([13, 24])
    theta = np.concatenate([[s[0] for s in special], np.arccos(g.uniform(-1.0, 1.0, 20))])
    phi = np.concatenate([[s[1] for s in special], g.uniform(0.0, 2.0 * np.pi, 20)])
    assert np.all(theta < np.pi)
    out["a/theta"], out["a/phi"] = theta, phi
    for convention, lmaxes in oracle.GOLDEN_POINTS.items():
        for lmax in lmaxes:
            name = "a/%s_l%d" % (convention, lmax)
            out[name] = checked(reference_matrix(sh, theta, phi, lmax, convention), oracle.matrix(theta, phi, lmax, convention), name)
    for H, W, lmax, convention in oracle.GOLDEN_GRIDS:
        g = np.random.default_rng([17, H, W, lmax])
        im = (g.random((2, 3, H, W)) ** 4 * 50.0 + 0.01).astype(np.float32)
        im[:, :, -1, :] = 0.0
        pix1, pix2 = np.linspace(0, 1, H) * np.pi, np.linspace(0, 2, W) * np.pi
        X, Y = np.meshgrid(pix2, pix1)
        X, Y = X.reshape(-1)[:-W], Y.reshape(-1)[:-W]
        M = reference_matrix(sh, Y, X, lmax, convention)                                  # (P - W, K)
        flat = im.astype(np.float64).reshape(2, 3, H * W)[:, :, :-W] * solid_angles(H, W)[:-W]
        name = "c/%dx%d_l%d" % (H, W, lmax)
        want = oracle.analysis(im, oracle.matrix(*oracle.grid_angles(H, W), lmax, convention), oracle.solid_angles(H, W))
        out[name + "/image"] = im
        out[name + "/coeffs"] = checked(np.einsum("bcp,pk->bkc", flat, M), want, name)
    path = os.path.join(HERE, "harmonics.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 449008


if __name__ == "__main__":
    main()
