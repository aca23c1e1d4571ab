"""The adjoints of object insertion restated in float64 on top of ``tests/insert_oracle.py``.  A helper of
``test_insert_grad_abi.py``, ``test_gpu_env_prefilter_bwd.py`` and ``test_gpu_gbuffer_shade_bwd.py``, not a test.  Nothing here
looks at the product code.

* ``prefilter_adjoint``: the transposed weight matrices of ``insert_oracle.lobe_weights``.
* ``shade`` / ``composite``: a torch float64 restatement of ``insert_oracle.shade`` / ``composite`` through which autograd
  gives every gradient: the taps (``floor``) are constants, the fractions are rounded to float32 as the definition says, and
  the clamp has derivative 0 outside the OPEN interval ``0 < e s < 1``.
* ``scatter``: the map gradient written out (``np.add.at``), used for the bounds' ``A = scatter(|k g|)``."""
import numpy as np
import torch

from tests import insert_oracle as oracle


def prefilter_adjoint(g, H, lobes, weights=oracle.lobe_weights):
    """g (B, L, 3, Ho, 2Ho) -> (B, 3, H, 2H) float64: ``sum_l g_l @ lobe_weights(H, Ho, l)``."""
    g = np.asarray(g, dtype=np.float64)
    B, L, _, Ho, _ = g.shape
    assert L == len(lobes)
    out = np.zeros((B, 3, 2 * H * H))
    for l, lb in enumerate(lobes):
        out += g[:, l].reshape(B, 3, 2 * Ho * Ho) @ weights(H, Ho, lb)
    return out.reshape(B, 3, H, 2 * H)


def taps(G, dirs):
    """dirs (B, ..., 3) -> r0, r1, c0, c1 (int64) and wx, wy (float64 values of the float32-rounded fractions):
    ``insert_oracle.lookup``'s rule."""
    W = 2 * G
    x, y, z = dirs[..., 0] + 0.0, dirs[..., 1] + 0.0, dirs[..., 2]
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
    return r0, r1, c0, c1, wx, wy


def lookup(maps, dirs):
    """maps: torch float64 (B, 3, G, 2G), dirs: numpy (B, h, w, 3) -> torch (B, 3, h, w), differentiable in ``maps``."""
    B, _, G, W = maps.shape
    r0, r1, c0, c1, wx, wy = taps(G, dirs)
    flat = maps.reshape(B, 3, G * W)
    wx, wy = torch.from_numpy(wx)[:, None], torch.from_numpy(wy)[:, None]

    def tap(r, c):
        idx = torch.from_numpy(r * W + c).reshape(B, 1, -1).expand(B, 3, -1)
        return torch.gather(flat, 2, idx).reshape(B, 3, *dirs.shape[1:-1])
    top = tap(r0, c0) * (1.0 - wx) + tap(r0, c1) * wx
    bot = tap(r1, c0) * (1.0 - wx) + tap(r1, c1) * wx
    return top * (1.0 - wy) + bot * wy


def _t(a):
    return a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def shade(pano, e_diffuse, e_phong, normal, coverage, kd=None, ks=None, km=None, fov_deg=60.0, view_azimuth_deg=180.0):
    """``insert_oracle.shade`` in torch float64; ``pano``, the maps and the coefficients may require grad.  ``normal`` and
    ``coverage`` are numpy: no gradient is defined for them.  Coefficients of invalid pixels (NaN is allowed there) count as 0."""
    valid, n, R = oracle.frames(normal, coverage, fov_deg, view_azimuth_deg)
    vt = torch.from_numpy(valid)[:, None]
    shaded = None
    for k, mp, d in ((kd, e_diffuse, n), (ks, e_phong, R), (km, pano, R)):
        if k is None:
            continue
        kk = torch.where(vt, _t(k).to(torch.float64), torch.zeros((), dtype=torch.float64))
        term = kk * lookup(_t(mp).to(torch.float64), d)
        shaded = term if shaded is None else shaded + term
    return shaded


def composite(shaded, coverage, background, exposure, gamma=2.4):
    """``insert_oracle.composite`` in torch float64, differentiable in ``shaded`` with the open-interval rule."""
    s = _t(shaded).to(torch.float64)
    cov, bg = _t(coverage).to(torch.float64), _t(background).to(torch.float64)
    x = _t(exposure).to(torch.float64)[:, None, None, None] * s
    inside = (x > 0.0) & (x < 1.0)
    safe = torch.where(inside, x, torch.full((), 0.5, dtype=torch.float64))
    ldr = torch.where(inside, safe if gamma == 1 else safe ** (1.0 / gamma), (x.detach() >= 1.0).to(torch.float64))
    return cov * ldr + (1.0 - cov) * bg


def scatter(G, dirs, values):
    """The map gradient written out: values (B, 3, h, w) float64 (``k g_s``, 0 at invalid pixels) at directions
    dirs (B, h, w, 3) -> (B, 3, G, 2G).  Two taps of a pixel on one texel both add."""
    values = np.asarray(values, dtype=np.float64)
    B, W = values.shape[0], 2 * G
    r0, r1, c0, c1, wx, wy = taps(G, dirs)
    out = np.zeros((B, 3, G * W))
    for b in range(B):
        for ch in range(3):
            for r, c, wgt in ((r0, c0, (1 - wx) * (1 - wy)), (r0, c1, wx * (1 - wy)), (r1, c0, (1 - wx) * wy), (r1, c1, wx * wy)):
                np.add.at(out[b, ch], (r[b] * W + c[b]).reshape(-1), (wgt[b] * values[b, ch]).reshape(-1))
    return out.reshape(B, 3, G, W)
