"""The definition of the ground-plane shadow restated in numpy float64.  A helper of
``test_ground_shadow_abi.py`` and ``test_gpu_ground_shadow.py``, not a test.  Nothing here looks at the product code; the
camera is ``insert_oracle``'s (``basis``, ``pixel_rays``), the grid ``sphere_render_oracle.texel_grid``.

Per image ``b`` and channel ``c``, with ``n`` the plane's unit normal in the panorama's frame:

    E0[b,c]      = sum_t pano[b,c,t] max(n . omega_t, 0) dOmega_t
    pixel (i, j) hits the plane iff n . ray < 0, at p = (-d / (n . ray)) ray
    blocked(p,t) = for some sphere k with r_k > 0, oc = c_k - p, s = oc . omega_t:
                   |oc|^2 < r_k^2   or   (s > 0 and |oc|^2 - s^2 < r_k^2)
    D[b,c,i,j]   = sum_t pano[b,c,t] max(n . omega_t, 0) dOmega_t blocked(p_ij, t)
    ratio        = clamp(1 - D / E0, 0, 1) where the pixel hits and E0[b,c] > 0, exactly 1 elsewhere

The *margin* of a pixel says how far its binary tests are from flipping: the minimum over the texels of non-zero weight
``max(n . omega_t, 0) dOmega_t`` and the spheres of ``| |oc|^2 - s^2 - r^2 | / r^2``, of ``|s| / |oc|`` where the first test is
within ``MARGIN`` of deciding or decides for the sphere (``|oc|^2 - s^2 <= r^2 (1 + MARGIN)``: only then does the sign of
``s`` matter), and, per sphere, of ``| |oc|^2 - r^2 | / r^2``.  Below ``MARGIN`` float64 rounding may legitimately flip a texel."""
import numpy as np

from tests import insert_oracle as io
from tests import sphere_render_oracle as sro

MARGIN = 1e-9


def to_panorama_frame(v, view_azimuth_deg):
    """camera-space vectors (..., 3) (x image right, y image up, z towards the camera) -> the panorama's frame."""
    _, r, u, back = io.basis(view_azimuth_deg)
    v = np.asarray(v, dtype=np.float64)
    return v[..., 0:1] * r + v[..., 1:2] * u + v[..., 2:3] * back


def evaluate(pano, plane, occluders, h, w, fov_deg=60.0, view_azimuth_deg=180.0):
    """pano (B, 3, H, 2H); plane (4,) or (B, 4); occluders (B, K, 4) -> a dict: ``ratio`` (B, 3, h, w), ``E0`` (B, 3),
    ``margin`` (B, h, w) (inf where the pixel misses the plane or no sphere counts), ``hit`` (B, h, w), ``n_ray`` (B, h, w),
    ``inside`` (B, h, w), ``blocked`` (B, h w, H 2H) bool and ``largest_term`` (B, 3): the largest single texel term / E0."""
    pano = np.asarray(pano, dtype=np.float64)
    B, _, H, W = pano.shape
    assert W == 2 * H and 0.0 < fov_deg < 180.0
    plane = np.broadcast_to(np.asarray(plane, dtype=np.float64), (B, 4))
    occ = np.asarray(occluders, dtype=np.float64).reshape(B, -1, 4)
    om, dom = sro.texel_grid(H, W)
    rays = io.pixel_rays(h, w, fov_deg, view_azimuth_deg).reshape(h * w, 3)
    T, P = H * W, h * w
    out = {"ratio": np.ones((B, 3, h, w)), "E0": np.zeros((B, 3)), "margin": np.full((B, h, w), np.inf),
           "hit": np.zeros((B, h, w), dtype=bool), "n_ray": np.zeros((B, h, w)), "inside": np.zeros((B, h, w), dtype=bool),
           "blocked": np.zeros((B, P, T), dtype=bool), "largest_term": np.zeros((B, 3))}
    for b in range(B):
        ln = np.linalg.norm(plane[b, :3])
        assert ln > 0.0 and plane[b, 3] > 0.0, "the plane needs a normal and d > 0"
        n = to_panorama_frame(plane[b, :3] / ln, view_azimuth_deg)
        d = plane[b, 3] / ln
        wgt = np.maximum(om @ n, 0.0) * dom                                          # (T,)
        terms = pano[b].reshape(3, T) * wgt                                          # (3, T)
        E0 = terms.sum(1)
        nr = rays @ n
        hit = nr < 0.0
        p = (-d / np.where(hit, nr, -1.0))[:, None] * rays                           # (P, 3); rows of missing pixels are unused
        blocked = np.zeros((P, T), dtype=bool)
        inside = np.zeros(P, dtype=bool)
        margin = np.full(P, np.inf)
        lit = wgt > 0.0
        for k in range(occ.shape[1]):
            r = occ[b, k, 3]
            if not r > 0.0:
                continue
            oc = to_panorama_frame(occ[b, k, :3], view_azimuth_deg)[None, :] - p     # (P, 3)
            oc2 = np.sum(oc * oc, 1)
            s = oc @ om.T                                                            # (P, T)
            q = oc2[:, None] - s * s
            blocked |= (oc2 < r * r)[:, None] | ((s > 0.0) & (q < r * r))
            inside |= oc2 < r * r
            m = np.abs(oc2 - r * r) / (r * r)
            if lit.any():
                m = np.minimum(m, (np.abs(q[:, lit] - r * r) / (r * r)).min(1))
                near = q[:, lit] <= r * r * (1.0 + MARGIN)
                ms = np.where(near, np.abs(s[:, lit]) / np.sqrt(oc2)[:, None], np.inf).min(1)
                m = np.minimum(m, ms)
            margin = np.minimum(margin, m)
        blocked &= hit[:, None]
        D = terms @ blocked.T.astype(np.float64)                                     # (3, P)
        for c in range(3):
            if E0[c] > 0.0:
                out["ratio"][b, c] = np.where(hit, np.clip(1.0 - D[c] / E0[c], 0.0, 1.0), 1.0).reshape(h, w)
                out["largest_term"][b, c] = terms[c].max() / E0[c]
        out["E0"][b] = E0
        out["margin"][b] = np.where(hit, margin, np.inf).reshape(h, w)
        out["hit"][b], out["n_ray"][b], out["inside"][b] = hit.reshape(h, w), nr.reshape(h, w), (inside & hit).reshape(h, w)
        out["blocked"][b] = blocked
    return out


def ground_shadow(pano, plane, occluders, h, w, fov_deg=60.0, view_azimuth_deg=180.0):
    """-> ratio (B, 3, h, w), E0 (B, 3), margin (B, h, w)."""
    r = evaluate(pano, plane, occluders, h, w, fov_deg, view_azimuth_deg)
    return r["ratio"], r["E0"], r["margin"]


def sphere_occluder(h, w, centre, radius, depth, fov_deg):
    """(cx, cy, cz, r) in camera space: the centre ``depth`` along pixel ``centre``'s ray, ``radius`` pixels wide there."""
    scl = np.tan(np.deg2rad(float(fov_deg)) / 2.0)
    sx = scl * (2.0 * centre[0] / (w - 1) - 1.0)
    sy = (scl * h / w) * (2.0 * centre[1] / (h - 1) - 1.0)
    ray = np.array([sx, -sy, -1.0])
    return np.append(depth * ray / np.linalg.norm(ray), radius * 2.0 * scl / (w - 1) * depth)
