"""The definition of the sphere renders and their metrics, restated in numpy float64.  A helper of
``test_gpu_sphere_render.py`` / ``test_sphere_render_abi.py``, not a test.  Nothing here looks at the product code."""
import numpy as np

MATERIALS = ("diffuse", "glossy", "mirror")


def mask(S):
    k = np.arange(S, dtype=np.int64)
    X, Y = 2 * k + 1 - S, S - 1 - 2 * k
    return (X * X)[None, :] + (Y * Y)[:, None] < S * S


def texel_grid(H, W):
    """omega (H*W, 3) and dOmega (H*W,) of the rasteriser's grid."""
    th = (np.arange(H) + 0.5) * np.pi / H
    ph = (np.arange(W) + 0.5) * 2.0 * np.pi / W
    st = np.sin(th)[:, None] * np.ones(W)[None, :]
    om = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                   np.cos(th)[:, None] * np.ones(W)[None, :]], -1).reshape(H * W, 3)
    return om, (st * (np.pi / H) * (2.0 * np.pi / W)).reshape(H * W)


def frames(S, view_azimuth_deg=180.0):
    """inside (S, S) bool, n (P, 3), R (P, 3) for the inside pixels in row-major order."""
    pc = np.deg2rad(float(view_azimuth_deg))
    f = np.array([np.cos(pc), np.sin(pc), 0.0])
    r = np.array([-np.sin(pc), np.cos(pc), 0.0])
    u = np.array([0.0, 0.0, 1.0])
    v = -f
    inside = mask(S)
    ii, jj = np.nonzero(inside)
    px, py = (2 * jj + 1 - S) / S, (S - 1 - 2 * ii) / S
    nz = np.sqrt(1.0 - px * px - py * py)
    n = px[:, None] * r + py[:, None] * u + nz[:, None] * v
    R = 2.0 * nz[:, None] * n - v
    return inside, n, R


def weights(H, W, S, view_azimuth_deg=180.0, phong_exponent=50.0):
    """The (P, H*W) weight matrices of the two integrals, normalisation included."""
    om, dom = texel_grid(H, W)
    _, n, R = frames(S, view_azimuth_deg)
    m = float(phong_exponent)
    Kd = np.maximum(n @ om.T, 0.0) * dom[None, :] / np.pi
    Kg = np.maximum(R @ om.T, 0.0) ** m * dom[None, :] * ((m + 1.0) / (2.0 * np.pi))
    return Kd, Kg


def mirror(pano, S, view_azimuth_deg=180.0):
    """pano (B, 3, H, W) -> (B, 3, P): bilinear lookup at R; coordinates in f64, weights rounded to f32."""
    pano = np.asarray(pano, dtype=np.float64)
    B, _, H, W = pano.shape
    _, _, R = frames(S, view_azimuth_deg)
    th = np.arctan2(np.sqrt(R[:, 0] ** 2 + R[:, 1] ** 2), R[:, 2])
    ph = np.mod(np.arctan2(R[:, 1], R[:, 0]), 2.0 * np.pi)
    v = np.clip(th * H / np.pi - 0.5, 0.0, H - 1.0)                   # rows clamp
    u = ph * W / (2.0 * np.pi) - 0.5
    fv, fu = np.floor(v), np.floor(u)
    r0 = fv.astype(np.int64)
    r1 = np.minimum(r0 + 1, H - 1)
    c0 = np.mod(fu.astype(np.int64), W)                               # columns wrap
    c1 = np.mod(c0 + 1, W)
    wy = (v - fv).astype(np.float32).astype(np.float64)
    wx = (u - fu).astype(np.float32).astype(np.float64)
    top = pano[:, :, r0, c0] * (1.0 - wx) + pano[:, :, r0, c1] * wx
    bot = pano[:, :, r1, c0] * (1.0 - wx) + pano[:, :, r1, c1] * wx
    return top * (1.0 - wy) + bot * wy


def render(pano, S, materials=MATERIALS, view_azimuth_deg=180.0, phong_exponent=50.0):
    """pano (B, 3, H, W) -> (B, M, 3, S, S) float64, 0 outside the disc."""
    pano = np.asarray(pano, dtype=np.float64)
    B, _, H, W = pano.shape
    inside = mask(S)
    flat = pano.reshape(B, 3, H * W)
    out = np.zeros((B, len(materials), 3, S, S))
    K = weights(H, W, S, view_azimuth_deg, phong_exponent) if ("diffuse" in materials or "glossy" in materials) else None
    for i, name in enumerate(materials):
        if name == "mirror":
            vals = mirror(pano, S, view_azimuth_deg)
        else:
            vals = flat @ K[0 if name == "diffuse" else 1].T          # (B, 3, P)
        out[:, i][:, :, inside] = vals
    return out


def metrics(a, b):
    """Two (B, M, 3, S, S) render arrays -> (B, M, 4): rmse, si_rmse, angular in degrees, used."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, M, _, S, _ = a.shape
    inside = mask(S)
    P = int(inside.sum())
    out = np.zeros((B, M, 4))
    for i in range(B):
        for j in range(M):
            x, y = a[i, j][:, inside], b[i, j][:, inside]             # (3, P)
            aa = np.sum(x * x)
            s = np.sum(x * y) / aa if aa != 0.0 else 0.0
            use = np.linalg.norm(x, axis=0) * np.linalg.norm(y, axis=0) != 0.0
            ang = np.arctan2(np.linalg.norm(np.cross(x.T, y.T), axis=1), np.sum(x * y, axis=0))
            n_used = int(use.sum())
            out[i, j] = (np.sqrt(np.sum((x - y) ** 2) / (3 * P)), np.sqrt(np.sum((s * x - y) ** 2) / (3 * P)),
                         np.degrees(np.mean(ang[use])) if n_used else 0.0, n_used)
    return out
