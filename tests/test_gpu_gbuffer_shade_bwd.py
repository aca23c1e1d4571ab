"""GPU: the adjoint of G-buffer shading and of the composite (csrc/gbuffer_shade_bwd.hip through
``emlight_amd.insert_grad``) against autograd on the float64 restatement (``insert_grad_oracle.py``).  The oracle is fed the
DEVICE's own maps, so that the prefilter's error does not compound; the end-to-end test adds it explicitly.

Bounds, derived (``EPS = 2^-24``).  ``g_s`` is the upstream gradient of the shaded value, ``k`` a coefficient.

* shaded mode, ``g_s = grad_out`` exactly.
  - ``dk = fl(g_s lookup)``: the forward's lookup bound ``32 EPS max|map|`` times ``|g_s|``, plus the product's rounding and
    slack, ``8 EPS |dk|``.
  - map gradients: DESIGN section 20's bound of the 64-bit fixed-point scatter, ``2^-22 A[t] + 2^-40 S`` with
    ``A = scatter(|k g_s|)`` and ``S`` its total per sample and map: the weights come from the forward's float32 fractions
    exactly, every contribution is rounded once to a multiple of ``2^-61 S`` at most (``2^-40 S`` covers 2^21 taps on a
    texel), and the int64 -> f32 conversion and the float32 inputs of the products are within ``2^-22`` of ``A``.
* composite mode.  The kernel recomputes ``s`` in float32 (the forward's bits), forms ``x = fl(e s)`` and
  ``g_s = fl(g c (1/gamma) e x^(1/gamma - 1))`` with the power in float64; the oracle has ``x* = e s*`` with ``s*`` the float64
  shading of the same maps.  ``|s - s*| <= ds``, the forward's shading bound, so ``x`` is within ``rho = ds / s* + EPS`` of ``x*``
  relatively (``ds`` takes the maximum of a map with lamps in it, so ``rho`` reaches some 1e-3 at dark pixels); the power
  ``a = 1/gamma - 1`` in ``[-1, 0]`` amplifies a small relative change by ``|a|``: by the mean value theorem
  ``|(1 + t)^a - 1| = |a| |t| (1 + xi)^(a - 1) <= 1.03 |a| rho`` for ``|t| <= rho < 0.01`` (asserted; ``0.99^-2 < 1.03``);
  ``log2`` and ``exp2`` are float64 here (2^-52, not a term), the final rounding to float32 and the products add ``2 EPS``:

      |g_s - g_s*| <= dg = |g_s*| (1.03 |1/gamma - 1| (ds / s* + EPS) + 2 EPS)

  It is carried through the two bounds above: ``dk`` gets ``dg |lookup|`` and the bounds with ``|g_s*| + dg`` for ``|g_s|``;
  a map gradient gets ``scatter(|k| dg)`` and the scatter's bound with ``A``, ``S`` of ``|k| (|g_s*| + dg)``.
  So that kernel and oracle cannot classify a pixel differently, the test asserts ON THE ORACLE that no covered value of
  ``e s`` lies within ``2^-8`` of 1 or in ``(0, 0.02)``, that at least 40 % of the covered pixel-channels are inside ``(0, 1)``
  and at least 10 % above 1.  Outside the open interval the gradients are exactly 0.
* end to end (``InsertionLoss``): see ``test_insertion_loss_end_to_end``.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import insert_grad_oracle as grad_oracle
from tests import insert_oracle as oracle
from tests import sphere_render_oracle as sro

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
HD, HG, PHONG = 4, 6, 20.0
PANO_SEED = 51       # of the panorama; with it the composite cases below meet the oracle's conditions for both seeds (checked in float64)
D = oracle.DIFFUSE
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(("kd", "ks", "km"), n)]      # the seven non-empty subsets
#         h  w  B  H   fov
SHAPES = [(6, 8, 3, 16, 60.0), (7, 9, 1, 12, 0.0), (2, 2, 2, 8, 100.0)]
MAP_OF = {"kd": "e_diffuse", "ks": "e_phong", "km": "pano"}


def hdr(B, H, seed):
    """``test_gpu_env_prefilter.py``'s panorama: U[0,1)^4 * 50 + 0.01 with a few texels multiplied by 1e3 (lamps)."""
    g = np.random.default_rng([seed, B, H])
    x = g.random((B, 3, H, 2 * H)) ** 4 * 50.0 + 0.01
    for b in range(B):
        for _ in range(3):
            x[b, :, g.integers(H), g.integers(2 * H)] *= 1e3
    return x.astype(np.float32)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def normal_towards(target, h, w, i, j, fov, az):
    """The camera-space normal of pixel (i, j) whose reflection direction is ``target``: the half vector of target and v_p."""
    _, r, u, v = oracle.basis(az)
    vp = -oracle.pixel_rays(h, w, fov, az)[i, j]
    n = np.asarray(target, dtype=np.float64) / np.linalg.norm(target) + vp
    return np.array([n @ r, n @ u, n @ v])


def direction(theta, phi):
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


@functools.lru_cache(maxsize=None)
def scene(seed, h, w, B, H, fov, az):
    """Everything a case needs, made once: the inputs on both sides and the DEVICE's maps (slices of prefilter outputs)."""
    from emlight_amd.insert import prefilter_environment
    g = np.random.default_rng([seed, h, w])
    normal = g.standard_normal((B, 3, h, w))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.2
    cov = g.random((B, 1, h, w)) * 0.9 + 0.1
    coef = {"kd": g.random((B, 3, h, w)) * 0.8 + 0.1, "ks": g.random((B, 3, h, w)) * 0.3 + 0.05,
            "km": g.random((B, 3, h, w)) * 0.1 + 0.01}
    gout = g.standard_normal((B, 3, h, w))
    row = np.pi / H
    # planted, as in the forward's test: a back-facing normal, reflections on and next to the column seam, directions beyond
    # the first and the last row centre; then a zero normal, coverage 0 with NaN everywhere else, and a negative kd
    back = (0.3, 0.2, -0.8)
    targets = [direction(1.0, 0.0), direction(2.0, 1e-3), direction(0.3 * row / 2, 1.0), direction(np.pi - 0.3 * row / 2, 4.0)]
    npix = h * w
    negative = []
    for b in range(B):
        if npix > 8:
            for k in range(5):
                i, j = divmod((k + 3 * b) % npix, w)
                normal[b, :, i, j] = back if k == 0 else normal_towards(targets[k - 1], h, w, i, j, fov, az)
        slots = [divmod((p + b) % npix, w) for p in (npix - 1, npix - 2, npix - 3)]
        if npix > 8 or b == 0:                                                        # 2 x 2: the first image has these two ...
            cov[b, 0, slots[0][0], slots[0][1]] = 0.0
            coef["kd"][b, :, slots[2][0], slots[2][1]] = -3.0                           # and no positive term: below 0 for any light
            coef["ks"][b, :, slots[2][0], slots[2][1]] *= -1.0
            coef["km"][b, :, slots[2][0], slots[2][1]] *= -1.0
            negative.append((b,) + slots[2])
        if npix > 8 or b == 1:                                                        # ... the second the zero normal
            normal[b, :, slots[1][0], slots[1][1]] = 0.0
    normal, cov, gout = normal.astype(np.float32), cov.astype(np.float32), gout.astype(np.float32)
    dead = (cov[:, 0] == 0.0) | (np.abs(normal).sum(1) == 0.0)                        # NaN wherever nothing may be read ...
    for k in coef:
        coef[k] = coef[k].astype(np.float32)
        coef[k][np.broadcast_to(dead[:, None], coef[k].shape)] = np.nan
    gout[np.broadcast_to(dead[:, None], gout.shape)] = np.nan
    normal[np.broadcast_to((cov[:, 0] == 0.0)[:, None], normal.shape)] = np.nan        # ... the normal where coverage is 0
    pano = hdr(B, H, PANO_SEED)
    dev = cuda(pano)
    low, high = prefilter_environment(dev, HD, (D, PHONG)), prefilter_environment(dev, HG, (D, PHONG))
    sc = {"pano": pano, "pano_dev": dev, "ed_dev": low[:, 0], "eg_dev": high[:, 1], "ed": low[:, 0].cpu().numpy(),
          "eg": high[:, 1].cpu().numpy(), "normal": normal, "cov": cov, "coef": coef, "gout": gout, "dead": dead,
          "negative": negative, "gout0": np.where(np.isnan(gout), 0.0, gout).astype(np.float64)}
    valid, n, R = oracle.frames(normal, cov, fov, az)
    assert np.array_equal(valid, ~dead)
    sc["dirs"] = {"kd": n, "ks": R, "km": R}
    sc["maps"] = {"kd": sc["ed"], "ks": sc["eg"], "km": pano}
    sc["k0"] = {k: np.where(dead[:, None], 0.0, coef[k]).astype(np.float64) for k in coef}
    shaded, terms = oracle.shade(pano, sc["ed"], sc["eg"], normal, cov, coef["kd"], coef["ks"], coef["km"], fov, az)
    sc["shaded"], sc["ds"] = shaded, shading_bound(terms)
    med = np.array([np.median(shaded[b][np.broadcast_to(~dead[b], shaded[b].shape)]) for b in range(B)])    # of the lit values
    sc["exposure"] = (0.5 / med).astype(np.float32)
    sc["bg"] = g.random((B, 3, h, w)).astype(np.float32)
    return sc


def shading_bound(terms):
    """The forward's: per value, sum over the terms of 32 EPS |k| max|map| plus 8 EPS of the terms' magnitudes."""
    return sum(32 * EPS * ak * mx[:, None, None, None] for ak, mx, _ in terms) + 8 * EPS * sum(t for _, _, t in terms)


def oracle_gradients(sc, subset, fov, az, exposure=None, gamma=2.4):
    """Autograd on the float64 restatement -> gradients by name, the looked-up values and ``g_s*``."""
    leaves = {nm: torch.from_numpy(np.asarray(sc["maps"][k], dtype=np.float64)).requires_grad_(True) for k, nm in MAP_OF.items()}
    ks = {k: (torch.from_numpy(sc["k0"][k]).requires_grad_(True) if k in subset else None) for k in ("kd", "ks", "km")}
    sh = grad_oracle.shade(leaves["pano"], leaves["e_diffuse"], leaves["e_phong"], sc["normal"], sc["cov"], ks["kd"], ks["ks"],
                           ks["km"], fov, az)
    sh.retain_grad()
    out = sh if exposure is None else grad_oracle.composite(sh, sc["cov"], sc["bg"], exposure, gamma)
    (out * torch.from_numpy(sc["gout0"])).sum().backward()
    got = {k: ks[k].grad.numpy() for k in subset}
    got.update({MAP_OF[k]: leaves[MAP_OF[k]].grad.numpy() for k in subset})
    look = {k: grad_oracle.lookup(torch.from_numpy(np.asarray(sc["maps"][k], dtype=np.float64)), sc["dirs"][k]).numpy()
            for k in subset}
    return got, look, sh.grad.numpy(), sh.detach().numpy()


def device_gradients(sc, subset, fov, az, want, exposure=None, gamma=2.4):
    from emlight_amd.insert_grad import shade_gbuffer_bwd_raw
    ks = {k: (cuda(sc["coef"][k]) if k in subset else None) for k in ("kd", "ks", "km")}
    return shade_gbuffer_bwd_raw(cuda(sc["gout"]), sc["pano_dev"], (sc["ed_dev"], sc["eg_dev"]), cuda(sc["normal"]),
                                 cuda(sc["cov"]), ks["kd"], ks["ks"], ks["km"], fov_deg=fov, view_azimuth_deg=az,
                                 exposure=cuda(exposure), gamma=gamma, want=want)


def check(sc, subset, got, want, look, gs, dg, what):
    """The two bounds of the module docstring with ``|g_s| <= |gs| + dg``; ``dg = 0`` in the shaded mode."""
    dead3 = np.broadcast_to(sc["dead"][:, None], gs.shape)
    worst = 0.0
    G = np.abs(gs) + dg
    for k in subset:
        mx = np.abs(sc["maps"][k].astype(np.float64)).reshape(len(gs), -1).max(1)[:, None, None, None]
        dk = got[k].cpu().numpy().astype(np.float64)
        assert np.isfinite(dk).all() and np.all(dk[dead3] == 0.0), (what, k)
        tol = 32 * EPS * G * mx + 8 * EPS * np.abs(want[k]) + dg * np.abs(look[k])
        err = np.abs(dk - want[k])
        assert np.all(err <= tol), (what, k, float((err - tol).max()))
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
        nm = MAP_OF[k]
        dm = got[nm].cpu().numpy().astype(np.float64)
        Gm = sc["maps"][k].shape[2]
        A = grad_oracle.scatter(Gm, sc["dirs"][k], np.abs(sc["k0"][k]) * G)
        S = A.reshape(len(gs), -1).sum(1)[:, None, None, None]
        tol = 2.0 ** -22 * A + 2.0 ** -40 * S + grad_oracle.scatter(Gm, sc["dirs"][k], np.abs(sc["k0"][k]) * dg)
        err = np.abs(dm - want[nm])
        assert np.isfinite(dm).all() and np.all(err <= tol), (what, nm, float((err - tol).max()))
        assert np.all(dm[A == 0.0] == 0.0), (what, nm, "a texel nothing lands on is exactly 0")
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    return worst


@pytest.mark.parametrize("az", [180.0, 77.3])
@pytest.mark.parametrize("h,w,B,H,fov", SHAPES)
@pytest.mark.parametrize("seed", [60, 65])
def test_shaded_mode_against_the_oracle(seed, h, w, B, H, fov, az):
    sc = scene(seed, h, w, B, H, fov, az)
    worst = 0.0
    for subset in SUBSETS:
        names = tuple(subset) + tuple(MAP_OF[k] for k in subset)
        got = device_gradients(sc, subset, fov, az, names)
        want, look, gs, _ = oracle_gradients(sc, subset, fov, az)
        worst = max(worst, check(sc, subset, got, want, look, gs, 0.0, (subset, "shaded")))
        for nm in names:                                                   # asked for alone: the same bits
            assert torch.equal(device_gradients(sc, subset, fov, az, (nm,))[nm], got[nm]), (subset, nm)
    print("%dx%d B %d fov %g az %g seed %d: largest error / bound %.3e" % (h, w, B, fov, az, seed, worst))


def composite_case(sc, gamma):
    """The oracle's classification must be safe from rounding: asserted here, on the oracle."""
    B = len(sc["shaded"])
    e = sc["exposure"].astype(np.float64)[:, None, None, None]
    x = e * sc["shaded"]
    live = ~np.broadcast_to(sc["dead"][:, None], x.shape)
    xs = x[live]
    assert not np.any(np.abs(xs - 1.0) < 2.0 ** -8) and not np.any((xs > 0.0) & (xs < 0.02))
    assert ((xs > 0) & (xs < 1)).mean() >= 0.4 and (xs > 1).mean() >= 0.1
    for b, i, j in sc["negative"]:
        assert np.all(x[b, :, i, j] < 0.0)                                 # the planted negative kd reaches the lower clamp
    return x, live


@pytest.mark.parametrize("gamma", [2.4, 1.0])
@pytest.mark.parametrize("h,w,B,H,fov,az", [s + (a,) for s, a in zip(SHAPES, (180.0, 180.0, 77.3))])
@pytest.mark.parametrize("seed", [60, 65])
def test_composite_mode_against_the_oracle(seed, h, w, B, H, fov, az, gamma):
    sc = scene(seed, h, w, B, H, fov, az)
    x, live = composite_case(sc, gamma)
    subset = ("kd", "ks", "km")
    names = subset + tuple(MAP_OF[k] for k in subset)
    got = device_gradients(sc, subset, fov, az, names, sc["exposure"], gamma)
    want, look, gs, sh = oracle_gradients(sc, subset, fov, az, sc["exposure"], gamma)
    inside = (x > 0) & (x < 1)
    rho = np.where(inside, sc["ds"] / np.where(inside, sh, 1.0) + EPS, 0.0)
    assert rho.max() < 0.01 and 1.0 <= gamma
    dg = np.abs(gs) * (1.03 * abs(1.0 / gamma - 1.0) * rho + 2 * EPS)
    assert np.all(gs[~inside] == 0.0)
    worst = check(sc, subset, got, want, look, gs, dg, ("composite", gamma))
    for k in subset:                                                       # both clamps: exactly 0
        assert np.all(got[k].cpu().numpy()[~inside] == 0.0)
    for b, i, j in sc["negative"]:
        assert all(np.all(got[k][b, :, i, j].cpu().numpy() == 0.0) for k in subset)
    for nm in names:
        assert torch.equal(device_gradients(sc, subset, fov, az, (nm,), sc["exposure"], gamma)[nm], got[nm]), nm
    print("composite %dx%d gamma %g seed %d: largest error / bound %.3e; inside %.0f %%, above %.0f %%, smallest e s %.3f"
          % (h, w, gamma, seed, worst, 100 * inside[live].mean(), 100 * (x[live] > 1).mean(), x[live][x[live] > 0].min()))


@pytest.mark.parametrize("gamma", [2.4, 1.0])
def test_composite_alone(gamma):
    """``composite``'s gradient for ``shaded``: the device's own float32 ``shaded`` on both sides, so ``ds = 0``."""
    from emlight_amd import insert, insert_grad
    h, w, B, H, fov = SHAPES[0]
    sc = scene(65, h, w, B, H, fov, 180.0)
    composite_case(sc, gamma)
    shaded = np.where(sc["dead"][:, None], np.nan, sc["shaded"]).astype(np.float32)
    s = cuda(shaded).requires_grad_(True)
    out = insert_grad.composite(s, cuda(sc["cov"]), cuda(sc["bg"]), cuda(sc["exposure"]), gamma)
    assert torch.equal(out.detach(), insert.composite(s.detach(), cuda(sc["cov"]), cuda(sc["bg"]), cuda(sc["exposure"]), gamma))
    out.backward(cuda(sc["gout"]))
    got = s.grad.cpu().numpy().astype(np.float64)
    leaf = torch.from_numpy(np.where(sc["dead"][:, None], 0.0, shaded).astype(np.float64)).requires_grad_(True)
    cov0 = sc["cov"].astype(np.float64)
    (grad_oracle.composite(leaf, cov0, sc["bg"], sc["exposure"], gamma) * torch.from_numpy(sc["gout0"])).sum().backward()
    want = leaf.grad.numpy()
    tol = np.abs(want) * (1.03 * abs(1.0 / gamma - 1.0) * EPS + 2 * EPS)
    dead3 = np.broadcast_to(sc["dead"][:, None], got.shape)
    assert np.isfinite(got).all() and np.all(got[np.broadcast_to(sc["cov"] == 0, got.shape)] == 0.0)
    live = ~dead3
    assert np.all(np.abs(got - want)[live] <= tol[live]) and np.all(got[live & (want == 0.0)] == 0.0)
    print("composite alone gamma %g: largest error / bound %.3e" % (gamma, float((np.abs(got - want)[live & (tol > 0)] / tol[live & (tol > 0)]).max())))


@functools.lru_cache(maxsize=None)
def weights(H, Ho, lobe):
    return oracle.lobe_weights(H, Ho, lobe)


def test_insertion_loss_end_to_end():
    """``InsertionLoss`` backward against autograd on the oracle's whole chain (float64 maps, shading, loss).  Three bounds are
    carried to ``dpred``.  (1) The upstream gradient ``g = 2 c (a - b) / (3 sum c) / B`` is formed from the device's shaded
    images: ``|a - a*| <= da`` = the prefilter's forward bound scaled by ``|k|`` plus the shading bound (as in
    ``test_gpu_gbuffer_shade.py``), likewise ``b``, and float32's few roundings: ``dg = 2 c (da + db) / (3 sum c) / B + 8 EPS |g*|``.
    Every operator behind it has non-negative weights, so ``dg`` is carried by the oracle's adjoint chain on ``|k| dg``.
    (2) The scatter's bound ``2^-22 A + 2^-40 S`` per map with ``A = scatter(|k| (|g*| + dg))``, carried through the prefilter
    adjoint for the two lobes.  (3) The prefilter adjoint's own bound (``test_gpu_env_prefilter_bwd.py``) on an input of
    magnitude ``A``.  The float32 sum of the three terms adds ``4 EPS`` of their magnitudes."""
    from emlight_amd import insert_grad
    h, w, B, H, fov = SHAPES[0]
    az = 77.3
    sc = scene(60, h, w, B, H, fov, az)
    pred, true = sc["pano"], hdr(B, H, 61)
    k0, cov, dead = sc["k0"], sc["cov"].astype(np.float64), sc["dead"]
    coefs = {k: cuda(np.where(dead[:, None], 0.0, sc["coef"][k]).astype(np.float32)) for k in ("kd", "ks", "km")}
    normal = cuda(np.where(np.isnan(sc["normal"]), 0.0, sc["normal"]).astype(np.float32))
    loss = insert_grad.InsertionLoss(normal, cuda(sc["cov"]), coefs["kd"], coefs["ks"], coefs["km"], fov_deg=fov,
                                     view_azimuth_deg=az, phong_exponent=PHONG, diffuse_height=HD, glossy_height=HG)
    p, t = cuda(pred).requires_grad_(True), cuda(true).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        value = loss(p, t)
        value.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert t.grad is None
    got = p.grad.cpu().numpy().astype(np.float64)
    # the oracle's chain
    Wd, Wg = torch.from_numpy(weights(H, HD, D)), torch.from_numpy(weights(H, HG, PHONG))
    normal0 = np.where(np.isnan(sc["normal"]), 0.0, sc["normal"])

    def shaded_of(x):
        flat = x.reshape(B, 3, -1)
        ed, eg = (flat @ Wd.T).reshape(B, 3, HD, 2 * HD), (flat @ Wg.T).reshape(B, 3, HG, 2 * HG)
        return grad_oracle.shade(x, ed, eg, normal0, cov, k0["kd"], k0["ks"], k0["km"], fov, az), ed, eg
    leaf = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    a, ed, eg = shaded_of(leaf)
    a.retain_grad()
    with torch.no_grad():
        b, edb, egb = shaded_of(torch.from_numpy(true.astype(np.float64)))
    den = 3.0 * cov.sum((1, 2, 3))
    want_value = ((torch.from_numpy(cov) * (a - b) ** 2).sum((1, 2, 3)) / torch.from_numpy(den)).mean()
    want_value.backward()
    want, gstar = leaf.grad.numpy(), a.grad.numpy()
    assert abs(float(value.detach()) - float(want_value.detach())) <= 1e-4 * float(want_value.detach())

    def forward_bound(x, e_d, e_g):
        _, terms = oracle.shade(x, e_d, e_g, normal0, cov, k0["kd"], k0["ks"], k0["km"], fov, az)
        pre = [(H * 2 * H + 4 * m + 64) * EPS * np.abs(mp).reshape(B, -1).max(1) for m, mp in ((1.0, e_d), (PHONG, e_g))]
        return np.abs(k0["kd"]) * pre[0][:, None, None, None] + np.abs(k0["ks"]) * pre[1][:, None, None, None] + shading_bound(terms)
    da = forward_bound(pred, ed.detach().numpy(), eg.detach().numpy())
    db = forward_bound(true, edb.numpy(), egb.numpy())
    dg = 2.0 * cov * (da + db) / den[:, None, None, None] / B + 8 * EPS * np.abs(gstar)
    G = np.abs(gstar) + dg
    dirs = sc["dirs"]
    dom = sro.texel_grid(H, 2 * H)[1].reshape(H, 2 * H)
    tol, magnitude = np.zeros_like(want), np.zeros_like(want)
    for k, Gm, lobe, m, c in (("km", H, None, 0.0, 0.0), ("kd", HD, D, 1.0, 1.0 / np.pi), ("ks", HG, PHONG, PHONG, (PHONG + 1) / (2 * np.pi))):
        A = grad_oracle.scatter(Gm, dirs[k], np.abs(k0[k]) * G)
        S = A.reshape(B, -1).sum(1)[:, None, None, None]
        dmap = grad_oracle.scatter(Gm, dirs[k], np.abs(k0[k]) * dg) + 2.0 ** -22 * A + 2.0 ** -40 * S
        if lobe is None:
            tol, magnitude = tol + dmap, magnitude + A
            continue
        adj = grad_oracle.prefilter_adjoint(A[:, None], H, (lobe,), weights)
        own = EPS * (2 * Gm * Gm * adj + (4 * m + 64) * dom * c * A.sum((2, 3))[:, :, None, None])
        tol = tol + grad_oracle.prefilter_adjoint(dmap[:, None], H, (lobe,), weights) + own
        magnitude = magnitude + adj
    tol = tol + 4 * EPS * magnitude
    err = np.abs(got - want)
    print("InsertionLoss: dpred largest error / bound %.3e (loss %.6e)" % (float((err[tol > 0] / tol[tol > 0]).max()), float(value.detach())))
    assert np.isfinite(got).all() and np.all(err <= tol), float((err - tol).max())


def test_forward_bits_autograd_requests_and_only_enqueues():
    from emlight_amd import insert, insert_grad
    h, w, B, H, fov = SHAPES[0]
    az = 180.0
    sc = scene(65, h, w, B, H, fov, az)
    n, c, bg, ex = cuda(sc["normal"]), cuda(sc["cov"]), cuda(sc["bg"]), cuda(sc["exposure"])
    coef = {k: cuda(sc["coef"][k]) for k in sc["coef"]}
    g = cuda(sc["gout"])
    kw = dict(fov_deg=fov, view_azimuth_deg=az, phong_exponent=PHONG, diffuse_height=HD, glossy_height=HG)

    def run():
        leaves = {k: v.clone().requires_grad_(True) for k, v in coef.items()}
        p = sc["pano_dev"].clone().requires_grad_(True)
        out = insert_grad.shade_gbuffer(p, n, c, leaves["kd"], leaves["ks"], leaves["km"], **kw)
        out.backward(g)
        p2 = sc["pano_dev"].clone().requires_grad_(True)
        comp = insert_grad.insert_object(p2, n, c, bg, ex, coef["kd"], coef["ks"], coef["km"], gamma=2.4, **kw)
        comp.backward(g)
        return out.detach(), comp.detach(), p.grad, p2.grad, leaves["kd"].grad, leaves["ks"].grad, leaves["km"].grad
    first = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(first, second))                     # run to run: the same bits
    assert all(bool(torch.isfinite(a).all()) for a in first[2:])
    # the forward of insert_grad is insert's, bit for bit
    assert torch.equal(first[0], insert.shade_gbuffer(sc["pano_dev"], n, c, coef["kd"], coef["ks"], coef["km"], **kw))
    assert torch.equal(first[1], insert.insert_object(sc["pano_dev"], n, c, bg, ex, coef["kd"], coef["ks"], coef["km"], gamma=2.4, **kw))
    # dpano is the mirror scatter plus the prefilter adjoints of the two map gradients
    maps = (insert.prefilter_environment(sc["pano_dev"], HD, (D,))[:, 0], insert.prefilter_environment(sc["pano_dev"], HG, (PHONG,))[:, 0])
    raw = insert_grad.shade_gbuffer_bwd_raw(g, sc["pano_dev"], maps, n, c, coef["kd"], coef["ks"], coef["km"], fov_deg=fov,
                                            view_azimuth_deg=az, want=("pano", "e_diffuse", "e_phong", "kd"))
    parts = [raw["pano"], insert_grad.prefilter_environment_bwd_raw(raw["e_diffuse"].unsqueeze(1), H, (D,)),
             insert_grad.prefilter_environment_bwd_raw(raw["e_phong"].unsqueeze(1), H, (PHONG,))]
    total = first[2].double()
    assert float((total - sum(x.double() for x in parts)).abs().max()) <= 4 * EPS * float(sum(x.double().abs() for x in parts).max())
    assert torch.equal(raw["kd"], first[4])
    # batch independence: the first image alone
    one = insert_grad.shade_gbuffer_bwd_raw(g[:1], sc["pano_dev"][:1], (maps[0][:1], maps[1][:1]), n[:1], c[:1], coef["kd"][:1],
                                            coef["ks"][:1], coef["km"][:1], fov_deg=fov, view_azimuth_deg=az,
                                            want=("pano", "e_diffuse", "e_phong", "kd"))
    assert all(torch.equal(one[nm], raw[nm][:1]) for nm in one)
    # what has no gradient is refused by name
    for name, args in (("normal", (n.clone().requires_grad_(True), c)), ("coverage", (n, c.clone().requires_grad_(True)))):
        with pytest.raises(ValueError, match="no gradient is defined for %s" % name):
            insert_grad.shade_gbuffer(sc["pano_dev"], *args, km=coef["km"], **kw)
