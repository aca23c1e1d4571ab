"""The definition of object insertion restated in numpy float64: prefiltered environment maps, the
direction lookup, the crop's camera, G-buffer shading and the composite.  A helper of ``test_insert_abi.py``,
``test_gpu_env_prefilter.py`` and ``test_gpu_gbuffer_shade.py``, not a test.  Nothing here looks at the product code; the
grid and the frame are those of ``sphere_render_oracle.py``."""
import numpy as np

from tests import sphere_render_oracle as sro

DIFFUSE = "diffuse"


def lobe_kernel(lobe, x):
    """``c_l k_l(x)`` of a lobe: ``"diffuse"`` or a Phong exponent ``m >= 0`` (``0^0 = 1``, numpy's rule)."""
    xp = np.maximum(x, 0.0)
    if lobe == DIFFUSE:
        return xp / np.pi
    m = float(lobe)
    return xp ** m * ((m + 1.0) / (2.0 * np.pi))


def lobe_weights(H, Ho, lobe):
    """The ``(2 Ho^2, 2 H^2)`` weight matrix of one lobe, normalisation and solid angle included."""
    om_t, dom = sro.texel_grid(H, 2 * H)
    om_d, _ = sro.texel_grid(Ho, 2 * Ho)
    return lobe_kernel(lobe, om_d @ om_t.T) * dom[None, :]


def prefilter(pano, Ho, lobes, weights=lobe_weights):
    """pano (B, 3, H, 2H) -> (B, L, 3, Ho, 2Ho) float64."""
    pano = np.asarray(pano, dtype=np.float64)
    B, _, H, W = pano.shape
    flat = pano.reshape(B, 3, H * W)
    return np.stack([(flat @ weights(H, Ho, lb).T).reshape(B, 3, Ho, 2 * Ho) for lb in lobes], 1)


def lookup(maps, dirs):
    """maps (B, 3, G, 2G), dirs (B, ..., 3) -> (B, 3, ...): bilinear, rows clamp, columns wrap; coordinates in f64, the
    fractions rounded to f32 (``sphere_render_oracle.mirror``'s rule from a direction).  A zero component counts as +0, so
    that the azimuth of the exact poles does not hang on the sign of a zero."""
    maps = np.asarray(maps, dtype=np.float64)
    B, _, G, W = maps.shape
    x, y, z = dirs[..., 0] + 0.0, dirs[..., 1] + 0.0, dirs[..., 2]              # -0 is 0: the poles themselves have phi = 0
    th = np.arctan2(np.hypot(x, y), z)
    ph = np.mod(np.arctan2(y, x), 2.0 * np.pi)
    v = np.clip(th * G / np.pi - 0.5, 0.0, G - 1.0)
    u = ph * W / (2.0 * np.pi) - 0.5
    fv, fu = np.floor(v), np.floor(u)
    r0 = fv.astype(np.int64)
    r1 = np.minimum(r0 + 1, G - 1)
    c0 = np.mod(fu.astype(np.int64), W)
    c1 = np.mod(c0 + 1, W)
    wy = (v - fv).astype(np.float32).astype(np.float64)
    wx = (u - fu).astype(np.float32).astype(np.float64)
    out = np.empty((B, 3) + x.shape[1:])
    for b in range(B):
        m = maps[b]
        top = m[:, r0[b], c0[b]] * (1.0 - wx[b]) + m[:, r0[b], c1[b]] * wx[b]
        bot = m[:, r1[b], c0[b]] * (1.0 - wx[b]) + m[:, r1[b], c1[b]] * wx[b]
        out[b] = top * (1.0 - wy[b]) + bot * wy[b]
    return out


def basis(view_azimuth_deg=180.0):
    pc = np.deg2rad(float(view_azimuth_deg))
    f = np.array([np.cos(pc), np.sin(pc), 0.0])
    r = np.array([-np.sin(pc), np.cos(pc), 0.0])
    u = np.array([0.0, 0.0, 1.0])
    return f, r, u, -f


def pixel_rays(h, w, fov_deg, view_azimuth_deg=180.0):
    """(h, w, 3) unit rays of ``crop_panorama``'s camera in the panorama's frame; ``fov_deg == 0``: all ``f``."""
    f, r, u, _ = basis(view_azimuth_deg)
    if fov_deg == 0:
        return np.broadcast_to(f, (h, w, 3)).copy()
    scl = np.tan(np.deg2rad(float(fov_deg)) / 2.0)
    sx = scl * (2.0 * np.arange(w) / (w - 1) - 1.0)
    sy = (scl * h / w) * (2.0 * np.arange(h) / (h - 1) - 1.0)
    ray = f[None, None, :] + sx[None, :, None] * r - sy[:, None, None] * u
    return ray / np.linalg.norm(ray, axis=-1, keepdims=True)


def frames(normal, coverage, fov_deg, view_azimuth_deg=180.0):
    """normal (B, 3, h, w), coverage (B, 1, h, w) -> valid (B, h, w) bool, n (B, h, w, 3), R (B, h, w, 3); rows of invalid
    pixels (coverage 0 or a zero normal; their inputs may be NaN) are (0, 0, 1)."""
    normal = np.asarray(normal, dtype=np.float64)
    cov = np.asarray(coverage, dtype=np.float64)[:, 0]
    B, _, h, w = normal.shape
    _, r, u, v = basis(view_azimuth_deg)
    nc = np.where(cov[:, None] != 0.0, normal, 0.0)
    n = nc[:, 0, ..., None] * r + nc[:, 1, ..., None] * u + nc[:, 2, ..., None] * v
    ln = np.linalg.norm(n, axis=-1)
    valid = (cov != 0.0) & (ln > 0.0)
    n = np.where(valid[..., None], n / np.where(valid, ln, 1.0)[..., None], np.array([0.0, 0.0, 1.0]))
    vp = -pixel_rays(h, w, fov_deg, view_azimuth_deg)[None]
    R = 2.0 * np.sum(n * vp, -1, keepdims=True) * n - vp
    R = np.where(valid[..., None], R, np.array([0.0, 0.0, 1.0]))
    return valid, n, R


def shade(pano, e_diffuse, e_phong, normal, coverage, kd=None, ks=None, km=None, fov_deg=60.0, view_azimuth_deg=180.0):
    """-> shaded (B, 3, h, w) float64 and the list of the evaluated terms' (|k|, map maximum, |term|) for the bounds."""
    valid, n, R = frames(normal, coverage, fov_deg, view_azimuth_deg)
    shaded = np.zeros(np.asarray(normal).shape)
    terms = []
    for k, mp, d in ((kd, e_diffuse, n), (ks, e_phong, R), (km, pano, R)):
        if k is None:
            continue
        kk = np.where(valid[:, None], np.asarray(k, dtype=np.float64), 0.0)
        term = kk * lookup(mp, d)
        shaded = shaded + term
        terms.append((np.abs(kk), np.abs(np.asarray(mp, dtype=np.float64)).reshape(len(kk), -1).max(1), np.abs(term)))
    return shaded, terms


def composite(shaded, coverage, background, exposure, gamma=2.4):
    shaded = np.asarray(shaded, dtype=np.float64)
    cov = np.asarray(coverage, dtype=np.float64)
    ldr = np.clip(np.asarray(exposure, dtype=np.float64)[:, None, None, None] * shaded, 0.0, 1.0)
    if gamma != 1:
        ldr = ldr ** (1.0 / gamma)
    return cov * ldr + (1.0 - cov) * np.asarray(background, dtype=np.float64)


def gbuffer_sphere(h, w, centre, radius):
    """normal (3, h, w), coverage (1, h, w) float64 of section 15's sphere at a pixel position."""
    px = ((np.arange(w) - centre[0]) / radius)[None, :] * np.ones((h, 1))
    py = ((centre[1] - np.arange(h)) / radius)[:, None] * np.ones((1, w))
    rr = px * px + py * py
    inside = rr < 1.0
    nz = np.sqrt(np.where(inside, 1.0 - rr, 0.0))
    return np.stack([px, py, nz], 0) * inside, inside[None].astype(np.float64)
