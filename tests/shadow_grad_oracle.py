"""The adjoint of the ground-plane shadow restated in numpy float64, on top of
``shadow_oracle.evaluate``.  A helper of ``test_ground_shadow_grad_abi.py`` and ``test_gpu_ground_shadow_grad.py``, not a
test.  Nothing here looks at the product code.

Per image ``b`` and channel ``c``, with ``wgt[t] = max(n . omega_t, 0) dOmega_t``, ``E0 = sum_t pano wgt``,
``D[p] = sum_t pano wgt blocked(p, t)`` and the unclamped ``v = 1 - D / E0``: a pixel is *active* when it hits the plane, is
not inside a sphere and ``E0 > 0``.  With the upstream gradients ``g_ratio`` and ``g_shadowed`` (``shadowed = image ratio``):

    g      = g_ratio + g_shadowed * image
    S      = sum over active p of g (1 - v)
    G[t]   = sum over active p of g blocked(p, t)
    dpano  = wgt / E0 (S - G)            (0 for the whole channel where E0 <= 0)
    dimage = g_shadowed * ratio

The bound of the GPU tests, per texel: ``2^-23 |want| + 2^-40 (wgt / E0) sum_p |g|``: the single rounding to f32, doubled; and
the f64 sums of at most ``h w + 2 H^2`` terms plus the 2^-61 fixed-point unit, against the cancellation bound ``sum |g|``.

The scenes are restated, not imported: the eight of ``test_gpu_ground_shadow.py`` and "tiles", the only one whose image
spans more than one 16 x 16 block (the adjoint is the first code with state shared across blocks)."""
import functools

import numpy as np

from tests import shadow_oracle as so
from tests import sphere_render_oracle as sro

FLOOR = (0.0, 1.0, 0.0, 1.0)

# name -> H, (h, w), view azimuth, planes (one 4-tuple for the batch or one per image), occluders (B = 2, K, 4)
SCENES = {
    "resting": (16, (12, 16), 180.0, [FLOOR, (0.1, 1.0, -0.05, 1.3)],
                [[(0.2, -0.6, -3.0, 0.4)], [(-0.3, -0.7, -2.8, 0.5)]]),
    "overlap": (8, (7, 9), 37.0, FLOOR,
                [[(0.0, -0.6, -3.0, 0.4), (0.3, -0.5, -3.1, 0.35), (0.1, -0.3, -2.9, 0.3)],
                 [(-0.4, -0.5, -3.4, 0.5), (-0.1, -0.4, -3.3, 0.45), (0.2, -0.7, -2.6, 0.3)]]),
    "seam": (16, (7, 9), 180.0, FLOOR, [[(0.0, 0.0, -1.5, 0.5)], [(0.2, 0.1, -1.2, 0.4)]]),
    "zenith": (8, (12, 16), 180.0, FLOOR, [[(0.0, 0.5, -3.0, 0.4)], [(0.5, 0.2, -3.5, 0.6)]]),
    "tilted": (16, (12, 16), 37.0, [(0.3, 1.0, 0.25, 1.0), (-0.2, 1.0, 0.3, 0.8)],
               [[(0.084, -0.006, -2.787, 0.28)], [(-0.3, 0.3, -2.5, 0.3)]]),
    "inside": (8, (7, 9), 180.0, FLOOR, [[(0.0, -1.0, -3.5, 1.5)], [(0.5, -0.8, -4.0, 1.2)]]),
    "chunks": (64, (7, 9), 180.0, FLOOR, [[(0.0, 0.0, -1.5, 0.5), (0.1, -0.6, -3.6, 0.4)],
                                          [(0.2, 0.6, -2.6, 0.5), (-0.3, -0.5, -4.0, 0.6)]]),
    "below": (8, (7, 9), 37.0, FLOOR, [[(0.0, -2.0, -3.0, 0.5)], [(0.4, -1.8, -2.5, 0.6)]]),
    # 2 x 2 blocks of 16 x 16 pixels, the last row and column of blocks partly filled; shadowed pixels in all four
    "tiles": (8, (20, 24), 180.0, [FLOOR, (0.1, 1.0, -0.05, 1.3)],
              [[(0.2, -0.6, -3.0, 0.4)], [(-0.3, -0.7, -2.8, 0.5)]]),
}


def hdr(B, H, seed):
    g = np.random.default_rng([seed, B, H])
    pano = (g.random((B, 3, H, 2 * H)) ** 4 * 50.0 + 0.01).astype(np.float32)
    pano[:, :, 1, (5 * H) // 4] = 2000.0                                             # one bright texel, high in the sky
    return pano


def texel_weights(plane, B, H, view_azimuth_deg):
    """wgt (B, H 2H) in float64."""
    plane = np.broadcast_to(np.asarray(plane, dtype=np.float64), (B, 4))
    om, dom = sro.texel_grid(H, 2 * H)
    out = np.zeros((B, 2 * H * H))
    for b in range(B):
        n = so.to_panorama_frame(plane[b, :3] / np.linalg.norm(plane[b, :3]), view_azimuth_deg)
        out[b] = np.maximum(om @ n, 0.0) * dom
    return out


def gradients(pano, plane, occluders, h, w, fov_deg=60.0, view_azimuth_deg=180.0, g_ratio=None, g_shadowed=None, image=None,
              forward=None):
    """-> a dict: ``dpano`` (B, 3, H, 2H), ``dimage`` (B, 3, h, w) or None, ``tol`` (B, 3, H, 2H) (the bound of the module
    docstring), ``wgt`` (B, H, 2H), ``v`` (B, 3, h, w) unclamped (1 where not active), ``active`` (B, 3, h, w), ``g``
    (B, 3, h, w) and ``forward``, what ``shadow_oracle.evaluate`` returned (pass one to reuse it)."""
    pano = np.asarray(pano, dtype=np.float64)
    B, _, H, W = pano.shape
    T, P = H * W, h * w
    res = forward if forward is not None else so.evaluate(pano, plane, occluders, h, w, fov_deg, view_azimuth_deg)
    g = np.zeros((B, 3, h, w))
    if g_ratio is not None:
        g = g + np.asarray(g_ratio, dtype=np.float64)
    if g_shadowed is not None:
        g = g + np.asarray(g_shadowed, dtype=np.float64) * np.asarray(image, dtype=np.float64)
    wgt = texel_weights(plane, B, H, view_azimuth_deg)
    dpano, tol = np.zeros((B, 3, T)), np.zeros((B, 3, T))
    v, active = np.ones((B, 3, P)), np.zeros((B, 3, P), dtype=bool)
    for b in range(B):
        terms = pano[b].reshape(3, T) * wgt[b]
        E0 = terms.sum(1)
        assert np.allclose(E0, res["E0"][b], rtol=1e-14, atol=0.0)
        live = (res["hit"][b] & ~res["inside"][b]).reshape(P)
        blocked = res["blocked"][b].astype(np.float64)                               # (P, T)
        D = terms @ blocked.T                                                        # (3, P)
        for c in range(3):
            if not E0[c] > 0.0:
                continue
            active[b, c] = live
            v[b, c] = np.where(live, 1.0 - D[c] / E0[c], 1.0)
            ga = np.where(live, g[b, c].reshape(P), 0.0)
            S = np.sum(ga * (1.0 - v[b, c]))
            G = ga @ blocked
            dpano[b, c] = wgt[b] / E0[c] * (S - G)
            tol[b, c] = 2.0 ** -23 * np.abs(dpano[b, c]) + 2.0 ** -40 * (wgt[b] / E0[c]) * np.abs(g[b, c]).sum()
    dimage = None
    if g_shadowed is not None:
        dimage = np.asarray(g_shadowed, dtype=np.float64) * res["ratio"]
    return {"dpano": dpano.reshape(B, 3, H, W), "dimage": dimage, "tol": tol.reshape(B, 3, H, W), "wgt": wgt.reshape(B, H, W),
            "v": v.reshape(B, 3, h, w), "active": active.reshape(B, 3, h, w), "g": g, "forward": res}


def shadow_loss(pred, true, plane, occluders, h, w, fov_deg=60.0, view_azimuth_deg=180.0, weight=None):
    """``ShadowLoss`` and its chain in float64: -> (loss, dpred (B, 3, H, 2H), g_ratio (B, 3, h, w), the dict of ``gradients``
    for the prediction, a - b)."""
    B = np.asarray(pred).shape[0]
    wt = np.ones((B, 1, h, w)) if weight is None else np.asarray(weight, dtype=np.float64)
    fp = so.evaluate(pred, plane, occluders, h, w, fov_deg, view_azimuth_deg)
    ft = so.evaluate(true, plane, occluders, h, w, fov_deg, view_azimuth_deg)
    d = fp["ratio"] - ft["ratio"]
    den = 3.0 * wt.sum((1, 2, 3))
    loss = np.mean((wt * d * d).sum((1, 2, 3)) / den)
    g_ratio = 2.0 * wt * d / den[:, None, None, None] / B
    got = gradients(pred, plane, occluders, h, w, fov_deg, view_azimuth_deg, g_ratio=g_ratio, forward=fp)
    return loss, got["dpano"], g_ratio, got, d


@functools.lru_cache(maxsize=None)
def scene(name):
    """The inputs of a scene (float32, as the device gets them), random upstream gradients of mixed signs and an image, and
    the oracle's answer on exactly those values, made once and read-only."""
    H, (h, w), az, planes, occ = SCENES[name]
    pano = hdr(2, H, 51)
    planes = np.asarray(planes, dtype=np.float32)
    occ = np.asarray(occ, dtype=np.float32)
    r = np.random.default_rng([61, H, h, w])
    g_ratio = r.standard_normal((2, 3, h, w)).astype(np.float32)
    g_shadowed = r.standard_normal((2, 3, h, w)).astype(np.float32)
    image = (r.random((2, 3, h, w)) ** 4 * 20.0 + 0.01).astype(np.float32)
    want = gradients(pano, planes, occ, h, w, 60.0, az, g_ratio=g_ratio, g_shadowed=g_shadowed, image=image)
    out = {"pano": pano, "planes": planes, "occ": occ, "h": h, "w": w, "az": az, "g_ratio": g_ratio, "g_shadowed": g_shadowed,
           "image": image, "want": want}
    for v in list(out.values()) + list(want.values()) + list(want["forward"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
