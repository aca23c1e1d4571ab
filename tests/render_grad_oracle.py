"""The gradient of the sphere renders with respect to the panorama ("Render loss"), restated in numpy
float64 on top of ``sphere_render_oracle``.  A helper of ``test_render_loss_abi.py`` / ``test_gpu_render_loss.py``, not a test.
Nothing here looks at the product code.

The renders are linear in the panorama, so the gradient is the adjoint:

    dpano[b,ch,t] = sum_p Kd[p,t] g_d[b,ch,p] + sum_p Kg[p,t] g_g[b,ch,p] + sum over mirror taps (p,k) on t of w[p,k] g_m[b,ch,p]

with ``p`` over the inside pixels only.  The mirror's four taps per pixel: coordinates in f64 as ``sphere_render_oracle.mirror``
forms them, ``wx``, ``wy`` rounded to f32, then ``(1-wx)(1-wy)``, ``wx(1-wy)``, ``(1-wx)wy``, ``wx wy``.  Here the four products
are exact (float64 products of the f32-rounded fractions): that makes ``vjp`` the adjoint of ``sphere_render_oracle.render`` to
the last bits of a float64.  The device forms them in f32 (``eml_sphere_mirror_taps_f32``): three roundings per weight, a
relative 3 * 2^-24 at most, inside the tolerance of the GPU tests (``taps(..., f32=True)`` restates the device's values)."""
import numpy as np

from tests import sphere_render_oracle as oracle


def taps(H, W, S, view_azimuth_deg=180.0, f32=False):
    """idx (P, 4) int64 texel indices ``r W + c`` for (r0,c0), (r0,c1), (r1,c0), (r1,c1); w (P, 4) float64: the exact products
    of the f32-rounded fractions.  ``f32=True``: the products in float32 arithmetic, as the device's tap table holds them."""
    _, _, R = oracle.frames(S, view_azimuth_deg)
    th = np.arctan2(np.sqrt(R[:, 0] ** 2 + R[:, 1] ** 2), R[:, 2])
    ph = np.mod(np.arctan2(R[:, 1], R[:, 0]), 2.0 * np.pi)
    v = np.clip(th * H / np.pi - 0.5, 0.0, H - 1.0)                   # rows clamp
    u = ph * W / (2.0 * np.pi) - 0.5
    fv, fu = np.floor(v), np.floor(u)
    r0 = fv.astype(np.int64)
    r1 = np.minimum(r0 + 1, H - 1)
    c0 = np.mod(fu.astype(np.int64), W)                               # columns wrap
    c1 = np.mod(c0 + 1, W)
    wy, wx = (v - fv).astype(np.float32), (u - fu).astype(np.float32)
    if not f32:
        wy, wx = wy.astype(np.float64), wx.astype(np.float64)
    one = wx.dtype.type(1.0)
    ux, uy = one - wx, one - wy
    w = np.stack([ux * uy, wx * uy, ux * wy, wx * wy], 1)
    assert w.dtype == wx.dtype
    idx = np.stack([r0 * W + c0, r0 * W + c1, r1 * W + c0, r1 * W + c1], 1)
    return idx, w.astype(np.float64)


def max_taps_on_a_texel(H, W, S, view_azimuth_deg=180.0):
    return int(np.bincount(taps(H, W, S, view_azimuth_deg)[0].ravel(), minlength=H * W).max())


def _vjp(g, H, W, S, materials, view_azimuth_deg, phong_exponent, K, absolute):
    g = np.asarray(g, dtype=np.float64)
    B = g.shape[0]
    assert g.shape == (B, len(materials), 3, S, S)
    inside = oracle.mask(S)
    if K is None and ("diffuse" in materials or "glossy" in materials):
        K = oracle.weights(H, W, S, view_azimuth_deg, phong_exponent)
    out = np.zeros((B, 3, H * W))
    for i, name in enumerate(materials):
        gi = g[:, i][:, :, inside]                                    # (B, 3, P): values outside the disc are ignored
        if absolute:
            gi = np.abs(gi)
        if name == "mirror":
            idx, w = taps(H, W, S, view_azimuth_deg)
            for k in range(4):
                contrib = gi * (np.abs(w[:, k]) if absolute else w[:, k])
                for b in range(B):
                    for ch in range(3):
                        np.add.at(out[b, ch], idx[:, k], contrib[b, ch])
        else:
            Ki = K[0 if name == "diffuse" else 1]
            out += gi @ (np.abs(Ki) if absolute else Ki)
    return out.reshape(B, 3, H, W)


def vjp(g, H, W, S, materials=oracle.MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0, K=None):
    """g (B, M, 3, S, S) in the order of ``materials`` -> (B, 3, H, W) float64.  ``K``: the pair of
    ``sphere_render_oracle.weights`` of this geometry, when the caller keeps them."""
    return _vjp(g, H, W, S, materials, view_azimuth_deg, phong_exponent, K, False)


def abs_vjp(g, H, W, S, materials=oracle.MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0, K=None):
    """The same with ``|K|``, ``|w|``, ``|g|``: the scale an f32 evaluation's rounding errors are relative to."""
    return _vjp(g, H, W, S, materials, view_azimuth_deg, phong_exponent, K, True)
