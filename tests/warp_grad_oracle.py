"""The panorama warp restated in torch float64 on the CPU, differentiable: the yardstick for the gradients of
``csrc/pano_warp_bwd.hip``.  ``tests/warp_oracle.py`` (numpy) is the forward's oracle and is pinned to the reference's own
maps; ``tests/test_warp_grad_oracle.py`` pins this file to it and to finite differences of itself.

What is differentiated, as DESIGN.md section 20 defines it:

* the position VALUE is the snapped one (closer than 2^-28 px to an integer: that integer), its DERIVATIVE that of the
  unsnapped formula; the clamp of ``s0`` and the ``mod 2 pi`` are the identity; ``floor`` is detached, so the bilinear slopes
  are those of the cell the forward used (the right-hand cell at an integer position);
* a pixel with ``s1^2 + s2^2 < 2^-20`` (the pole rule) or without a finite position has a constant position: its direction
  is replaced by a fixed one BEFORE ``asin`` / ``atan2`` (masking afterwards would still give ``0 * inf``);
* a pixel without a finite position is left out of both gradients.
"""
import math

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

POLE = 2.0 ** -20
SNAP = 2.0 ** -28


def _positions(H, W, h, w, theta_deg, phi_deg, move):
    """``theta_deg, phi_deg, move``: 0-d float64 tensors.  Returns ``row, col`` (unsnapped values, derivative masked as
    described above), ``ok`` (a finite position exists), ``rho2`` = ``s1^2 + s2^2``."""
    f8 = torch.float64
    i = torch.arange(h, dtype=f8)[:, None]
    j = torch.arange(w, dtype=f8)[None, :]
    lat = i * math.pi / h - math.pi / 2 + 0 * j
    lon = j * (2 * math.pi) / w + 0 * i
    d0, d1, d2 = torch.sin(lat), torch.sin(lon) * torch.cos(lat), -torch.cos(lon) * torch.cos(lat)
    t, p = theta_deg / 180 * math.pi, phi_deg / 180 * math.pi
    ct, st, c, s = torch.cos(t), torch.sin(t), torch.cos(p), -torch.sin(p)
    k = 1 - c
    ay, az = ct, st
    e0, e1, e2 = d0, ct * d1 - st * d2, st * d1 + ct * d2
    n1, n2 = st, -ct
    R = ((c, -az * s, ay * s), (az * s, c + ay * ay * k, ay * az * k), (-ay * s, az * ay * k, c + az * az * k))
    v = [R[a][0] * e0 + R[a][1] * e1 + R[a][2] * e2 + move * (R[a][1] * n1 + R[a][2] * n2) for a in range(3)]
    vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    n_val = torch.sqrt(vv.detach())
    ok = torch.isfinite(n_val) & (n_val > 0)
    n = torch.sqrt(torch.where(ok, vv, torch.ones_like(vv)))
    s0, s1, s2 = v[0] / n, v[1] / n, v[2] / n
    rho2 = (s1 * s1 + s2 * s2).detach()
    # the value, from plain numbers
    with torch.no_grad():
        s0v, s1v, s2v = s0.detach(), s1.detach(), s2.detach()
        row_v = (torch.asin(torch.clamp(s0v, -1.0, 1.0)) + math.pi / 2) / math.pi * H
        az_v = torch.atan2(s1v, -s2v)
        az_v = torch.where(az_v < 0, az_v + 2 * math.pi, az_v)
        col_v = az_v / (2 * math.pi) * W
    # the derivative, from directions that are constant where the pixel must not contribute
    live = ok & (rho2 >= POLE)
    zero, one = torch.zeros_like(rho2), torch.ones_like(rho2)
    m0, m1, m2 = torch.where(live, s0, zero), torch.where(live, s1, zero), torch.where(live, s2, -one)
    row_d = (torch.asin(m0) + math.pi / 2) / math.pi * H
    col_d = torch.atan2(m1, -m2) / (2 * math.pi) * W
    row = row_v + (row_d - row_d.detach())
    col = col_v + (col_d - col_d.detach())
    return row, col, ok, rho2


def _snap(x):
    n = torch.round(x.detach())
    return x + torch.where((x.detach() - n).abs() < SNAP, n - x.detach(), torch.zeros_like(n))


def _sample(img, row, col, ok):
    """Wrap-bilinear of ``img`` (H, W, 3) float64 at the snapped positions; pixels that are not ``ok`` give 0."""
    H, W, _ = img.shape
    r = _snap(torch.where(ok, row, torch.zeros_like(row)))
    c = _snap(torch.where(ok, col, torch.zeros_like(col)))
    fr, fc = torch.floor(r.detach()), torch.floor(c.detach())
    yd, xd = (r - fr)[..., None], (c - fc)[..., None]
    i0, j0 = fr.long() % H, fc.long() % W
    i1, j1 = (i0 + 1) % H, (j0 + 1) % W
    v = img[i0, j0] * ((1 - yd) * (1 - xd))
    v = v + img[i0, j1] * ((1 - yd) * xd)
    v = v + img[i1, j0] * (yd * (1 - xd))
    v = v + img[i1, j1] * (yd * xd)
    return torch.where(ok[..., None], v, torch.zeros_like(v))


def _scalars(theta, phi, move):
    return [torch.tensor(float(x), dtype=torch.float64) for x in (theta, phi, move)]


def forward(pano, h, w, theta=0.0, phi=0.0, move=0.0):
    """numpy: ``(image (h, w, 3) float64, NaN where there is no position; row, col (h, w) UNSNAPPED, NaN likewise)``."""
    img = torch.from_numpy(np.asarray(pano, dtype=np.float64))
    with torch.no_grad():
        row, col, ok, _ = _positions(img.shape[0], img.shape[1], h, w, *_scalars(theta, phi, move))
        out = _sample(img, row, col, ok)
    nan = torch.full_like(row, float("nan"))
    out = torch.where(ok[..., None], out, nan[..., None])
    return out.numpy(), torch.where(ok, row, nan).numpy(), torch.where(ok, col, nan).numpy()


def classify(H, W, h, w, theta=0.0, phi=0.0, move=0.0):
    """numpy: ``rho2`` = ``s1^2 + s2^2`` per pixel, the distances of the unsnapped ``row`` and ``col`` to the nearest integer,
    and ``ok``: what the pole rule and the snap decide on."""
    with torch.no_grad():
        row, col, ok, rho2 = _positions(H, W, h, w, *_scalars(theta, phi, move))
    dist = torch.minimum((row - torch.round(row)).abs(), (col - torch.round(col)).abs())
    return rho2.numpy(), dist.numpy(), ok.numpy()


def gradients(pano, grad_out, theta=0.0, phi=0.0, move=0.0):
    """``pano`` (H, W, 3), ``grad_out`` (h, w, 3), numpy.  Returns numpy float64
    ``dpano`` (H, W, 3), ``dparams`` (3,), ``A`` (H, W, 3) = the ``dpano`` of ``|grad_out|``, ``S_abs`` (3,) = the sum over
    pixels and channels of ``|grad_out * d out / d q|``.  ``dparams`` is autograd's (reverse mode); forward mode, which gives
    the per-pixel terms of ``S_abs``, must give the same number to 2^-30 ``S_abs``, a quarter of what the kernel is held to."""
    dpano, dparams, A, S_abs, fwd = gradients_both_modes(pano, grad_out, theta, phi, move)
    assert (np.abs(dparams - fwd) <= 2.0 ** -30 * S_abs).all(), (dparams, fwd, S_abs)
    return dpano, dparams, A, S_abs


def gradients_both_modes(pano, grad_out, theta=0.0, phi=0.0, move=0.0):
    """``gradients`` and, fifth, ``dparams`` by forward mode, without the assertion that the two modes agree: where a pixel's
    ``|v|`` is tiny but not 0 (``move = 1``: 1.2e-16) its term is a product of 1 / |v| and a difference that cancels, and
    float64 cannot say what the sum is."""
    img = torch.from_numpy(np.asarray(pano, dtype=np.float64)).requires_grad_(True)
    g = torch.from_numpy(np.asarray(grad_out, dtype=np.float64))
    h, w, _ = g.shape
    H, W, _ = img.shape
    prm = [x.requires_grad_(True) for x in _scalars(theta, phi, move)]
    row, col, ok, _ = _positions(H, W, h, w, *prm)
    out = _sample(img, row, col, ok)
    grads = torch.autograd.grad((out * g).sum(), [img] + prm, retain_graph=True, allow_unused=True)
    dpano = grads[0]
    dparams = torch.stack([x if x is not None else torch.zeros((), dtype=torch.float64) for x in grads[1:]])
    A = torch.autograd.grad((out * g.abs()).sum(), img)[0]
    # per-pixel terms by forward mode, one tangent at a time
    S_abs, fwd = [], []
    img_c = img.detach()
    for q in range(3):
        with fwAD.dual_level():
            duals = [fwAD.make_dual(x.detach(), torch.ones_like(x) if k == q else torch.zeros_like(x)) for k, x in enumerate(prm)]
            r2, c2, ok2, _ = _positions(H, W, h, w, *duals)
            tangent = fwAD.unpack_dual(_sample(img_c, r2, c2, ok2)).tangent
            tangent = torch.zeros_like(g) if tangent is None else tangent
        S_abs.append((g * tangent).abs().sum())
        fwd.append((g * tangent).sum())
    S_abs, fwd = torch.stack(S_abs), torch.stack(fwd)
    return dpano.numpy(), dparams.numpy(), A.numpy(), S_abs.numpy(), fwd.numpy()


# ------------------------------------------------------------------------------------------------ the cases of the tests
GENERIC = [(25.0, -40.0, -0.6), (-70.0, 130.0, 0.45), (5.0, 3.0, 0.9)]
PARAMS = [(0.0, 0.0, 0.0)] + GENERIC + [(0.0, 0.0, -0.6)]
FD_SIZES = [(16, 32, 16, 32), (12, 20, 24, 48), (16, 32, 6, 10)]                          # (H, W, h, w)
SIZES = [(8, 16, 6, 10), (8, 16, 8, 16), (16, 32, 16, 32), (12, 20, 24, 48), (64, 128, 64, 128), (1, 4, 3, 5)]
# per-sample |move| = 1 with theta = phi = 0: the direction that falls on the new viewpoint has no position where |v| == 0
# exactly in float64 (move = -1: pixel (h / 2, 0); move = +1: lon = pi has a sine of 1.2e-16, so the oracle decides)
UNIT_MOVES = [(16, 32, 8, 16, (0.0, 0.0, 1.0)), (16, 32, 8, 16, (0.0, 0.0, -1.0))]


def panoramas(B, H, W, seed):
    """Heavy-tailed panoramas (B, H, W, 3) float32, ``pano_inputs`` of ``make_golden_panorama`` (which needs H, W >= 2)."""
    from tests.golden.make_golden_panorama import pano_inputs
    return np.ascontiguousarray(pano_inputs(B, max(H, 2), max(W, 2), seed)[:, :H, :W])


def grad_outputs(B, h, w, seed):
    """(B, h, w, 3) float32: a normal variate times exp of a normal variate with sigma 3 -- about six decades."""
    g = np.random.default_rng([seed, B, h, w])
    return (g.standard_normal((B, h, w, 3)) * np.exp(3.0 * g.standard_normal((B, h, w, 3)))).astype(np.float32)
