"""GPU: the adjoint of the ground-plane shadow (csrc/ground_shadow_bwd.hip through ``emlight_amd.insert_grad``) against the
float64 restatement of its definition (``shadow_grad_oracle.py``).

Device and oracle add the same texels for every pixel (no scene has a pixel within ``MARGIN`` of a flipping test, and no
active pixel's unclamped ratio leaves [0, 1]: ``test_ground_shadow_grad_abi.py`` checks both on the CPU, so no pixel is left
out), and per texel

    |dpano - want| <= 2^-23 |want| + 2^-40 (wgt[t] / E0) sum_p |g[p]|:

the single rounding to f32 (2^-24), doubled; and the f64 sums of at most h w + 2 H^2 terms plus the fixed-point unit
(2^-61 sum |g| per pixel), against the cancellation bound sum |g|, with some 2^13 headroom.  ``dimage`` is one f32 product
of the forward's f32 ratio: exact.

The scenes are ``shadow_grad_oracle.SCENES``: the forward's eight and "tiles", 20 x 24 pixels in 2 x 2 blocks -- the
fixed-point accumulators and the partials of S are the first state shared across blocks."""
import numpy as np
import pytest
import torch

from tests import shadow_grad_oracle as go

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()                            # the scenes' arrays are read-only


def plane_arg(planes):
    return tuple(float(v) for v in planes) if planes.ndim == 1 else cuda(planes)


def raw(c, want=("pano", "image"), g_ratio=True, g_shadowed=True, **kw):
    """``ground_shadow_bwd_raw`` on a scene; ``g_ratio`` / ``g_shadowed``: True (the scene's), None or an array."""
    from emlight_amd.insert_grad import ground_shadow_bwd_raw
    c = dict(c, **kw)
    gr = c["g_ratio"] if g_ratio is True else g_ratio
    gs = c["g_shadowed"] if g_shadowed is True else g_shadowed
    return ground_shadow_bwd_raw(cuda(c["pano"]), cuda(c["occ"]), plane_arg(c["planes"]), fov_deg=60.0, view_azimuth_deg=c["az"],
                                 size=(c["h"], c["w"]), image=None if gs is None else cuda(c["image"]),
                                 g_ratio=None if gr is None else cuda(gr), g_shadowed=None if gs is None else cuda(gs), want=want)


def forward(c, **kw):
    from emlight_amd.insert import ground_shadow
    return ground_shadow(cuda(c["pano"]), cuda(c["occ"]), plane_arg(c["planes"]), fov_deg=60.0, view_azimuth_deg=c["az"],
                         size=(c["h"], c["w"]), **kw)


def within(name, got, want, tol):
    """The elementwise check; prints the largest error over its bound before it asserts."""
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    over = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err > 0.0, np.inf, 0.0))
    print("%s: largest |dpano| %.3e, largest error %.3e, largest error over its bound %.3e" % (name, np.abs(want).max(), err.max(),
                                                                                              over.max()))
    assert np.all(err <= tol), name
    return got


@pytest.mark.parametrize("name", sorted(go.SCENES))
def test_against_the_oracle(name):
    c = go.scene(name)
    want = c["want"]
    got = raw(c)
    H = c["pano"].shape[2]
    assert got["pano"].shape == (2, 3, H, 2 * H) and got["pano"].dtype == torch.float32
    dpano = within(name, got["pano"], want["dpano"], want["tol"])
    dark = np.broadcast_to((want["wgt"] == 0.0)[:, None], dpano.shape)
    assert dark.any() and np.all(dpano[dark] == 0.0), "a texel behind the plane gets exactly 0"
    if name == "below":
        assert np.all(dpano == 0.0)
    else:
        assert np.abs(dpano).max() > 0.0
    # Euler: the ratio is homogeneous of degree 0 in each channel of the panorama
    pano = c["pano"].astype(np.float64)
    euler, bound = np.abs((pano * dpano).sum((2, 3))), (pano * want["tol"]).sum((2, 3))
    print("%s: Euler's identity, largest |sum pano dpano| over its bound %.3e" % (name, (euler / np.maximum(bound, 1e-300)).max()))
    assert np.all(euler <= bound)
    # dimage: one f32 product of the forward's ratio
    ratio = forward(c)
    assert torch.equal(got["image"], cuda(c["g_shadowed"]) * ratio)


def test_black_channel_no_occluder_and_spheres_below_give_exact_zeros():
    c = go.scene("resting")
    pano = c["pano"].copy()
    pano[:, 1] = 0.0
    got = raw(dict(c, pano=pano))["pano"]
    full = raw(c)["pano"]
    assert torch.all(got[:, 1] == 0.0) and torch.equal(got[:, 0], full[:, 0]) and torch.equal(got[:, 2], full[:, 2])
    assert float(got[:, 0].abs().max()) > 0.0
    # K = 0, and spheres entirely below the plane in image 1 only: that image is exactly 0, the other untouched
    assert torch.all(raw(dict(c, occ=np.zeros((2, 0, 4), dtype=np.float32)))["pano"] == 0.0)
    occ = c["occ"].copy()
    occ[1, 0] = (0.4, -3.0, -2.5, 0.6)
    got = raw(dict(c, occ=occ))["pano"]
    assert torch.all(got[1] == 0.0) and torch.equal(got[0], full[0])


@pytest.mark.parametrize("name", ["tiles", "chunks"])
def test_exactness(name):
    c = go.scene(name)
    got = raw(c)
    again = raw(c)
    assert torch.equal(again["pano"], got["pano"]) and torch.equal(again["image"], got["image"])
    # image 0 does not depend on the batch
    one = {k: (v[:1] if isinstance(v, np.ndarray) and v.shape[:1] == (2,) else v) for k, v in c.items()}
    assert one["pano"].shape[0] == 1 and one["occ"].shape[0] == 1 and one["g_ratio"].shape[0] == 1
    alone = raw(one)
    assert torch.equal(alone["pano"][0], got["pano"][0]) and torch.equal(alone["image"][0], got["image"][0])
    # a padded (r = 0, NaN) or hidden sphere changes no bit, nor does the order of the spheres
    pad = np.array([[5.0, 5.0, 5.0, 0.0]] * 2, dtype=np.float32)[:, None]
    nan = np.array([[0.0, -0.6, -3.0, np.nan]] * 2, dtype=np.float32)[:, None]
    inner = c["occ"][:, :1].copy()
    inner[:, :, 3] *= 0.5
    for occ in (np.concatenate([c["occ"], pad], 1), np.concatenate([nan, c["occ"], pad], 1), np.concatenate([c["occ"], inner], 1),
                np.concatenate([inner, c["occ"][:, ::-1]], 1)):
        assert torch.equal(raw(dict(c, occ=occ), want=("pano",))["pano"], got["pano"])


def test_request_subsets():
    c = go.scene("tiles")
    zero = np.zeros_like(c["g_ratio"])
    # g_ratio alone against the full call with g_shadowed = 0; g_shadowed alone against the full call with g_ratio = 0
    full = raw(c, g_shadowed=zero)
    assert torch.equal(raw(c, want=("pano",), g_shadowed=None)["pano"], full["pano"]) and torch.all(full["image"] == 0.0)
    full = raw(c, g_ratio=zero)
    alone = raw(c, g_ratio=None)
    assert torch.equal(alone["pano"], full["pano"]) and torch.equal(alone["image"], full["image"])
    assert float(full["pano"].abs().max()) > 0.0
    # dimage alone, dpano alone: the bits of the full call's outputs
    full = raw(c)
    assert torch.equal(raw(c, want=("image",))["image"], full["image"])
    assert torch.equal(raw(c, want=("image",), g_ratio=None)["image"], full["image"])
    assert torch.equal(raw(c, want=("pano",))["pano"], full["pano"])


def test_through_autograd():
    from emlight_amd import insert, insert_grad
    c = go.scene("tiles")
    occ, planes = cuda(c["occ"]), plane_arg(c["planes"])
    args = dict(fov_deg=60.0, view_azimuth_deg=c["az"])
    pano, image = cuda(c["pano"]).requires_grad_(True), cuda(c["image"]).requires_grad_(True)
    ratio, shadowed = insert_grad.ground_shadow(pano, occ, planes, image=image, **args)
    want_ratio, want_shadowed = insert.ground_shadow(pano.detach(), occ, planes, image=image.detach(), **args)
    assert ratio.requires_grad and shadowed.requires_grad
    assert torch.equal(ratio, want_ratio) and torch.equal(shadowed, want_shadowed)
    torch.autograd.backward([ratio, shadowed], [cuda(c["g_ratio"]), cuda(c["g_shadowed"])])
    want = raw(c)
    assert torch.equal(pano.grad, want["pano"]) and torch.equal(image.grad, want["image"])
    with torch.no_grad():
        quiet = insert_grad.ground_shadow(pano, occ, planes, image=image, **args)
    assert not quiet[0].requires_grad and torch.equal(quiet[0], want_ratio) and torch.equal(quiet[1], want_shadowed)
    # the ratio alone, by size
    pano.grad = None
    alone = insert_grad.ground_shadow(pano, occ, planes, size=(c["h"], c["w"]), **args)
    assert torch.equal(alone, want_ratio)
    alone.backward(cuda(c["g_ratio"]))
    assert torch.equal(pano.grad, raw(c, want=("pano",), g_shadowed=None)["pano"])
    # a forward plus backward only enqueues work
    g1, g2 = cuda(c["g_ratio"]), cuda(c["g_shadowed"])
    pano.grad = image.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = insert_grad.ground_shadow(pano, occ, planes, image=image, **args)
        torch.autograd.backward([a, b], [g1, g2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(pano.grad, want["pano"]) and torch.equal(image.grad, want["image"])


def moved_light(pano, H):
    """The truth with its bright texel moved four columns: what a misplaced light looks like."""
    pred = pano.copy()
    col = (5 * H) // 4
    pred[:, :, 1, col + 4], pred[:, :, 1, col] = pano[:, :, 1, col], pano[:, :, 1, col + 4]
    return pred


def test_shadow_loss():
    """Value and gradient against the oracle's chain.  The device forms g = 2 weight (a - b) / (3 sum weight B) in f32 from
    f32 ratios that are each within 2^-23 of the oracle's: |delta d| <= 2^-22, and the subtraction and three products round
    once each (4 x 2^-24 relative, taken as 2^-21 with the f32 weight and denominator).  dpano is linear in g with
    |d dpano[t] / d g[p]| = (wgt / E0) |(1 - v) - blocked| <= wgt / E0, so the bound grows by (wgt / E0) sum_p |delta g[p]|.  The
    value: the same |delta d| through d^2, four f32 roundings per term, and an f32 sum of 3 h w non-negative terms and the
    mean (at most 3 h w + 4 more roundings)."""
    from emlight_amd.insert_grad import ShadowLoss
    c = go.scene("resting")
    H, h, w = 16, c["h"], c["w"]
    true = c["pano"]
    pred = moved_light(true, H)
    wt = (np.random.default_rng(71).random((2, 1, h, w)) * 0.75 + 0.25).astype(np.float32)
    loss = ShadowLoss(cuda(c["occ"]), cuda(c["planes"]), size=(h, w), view_azimuth_deg=c["az"], weight=cuda(wt))
    p = cuda(pred).requires_grad_(True)
    value = loss(p, cuda(true))
    value.backward()
    want_value, want_grad, g, chain, d = go.shadow_loss(pred, true, c["planes"], c["occ"], h, w, 60.0, c["az"], weight=wt)
    coeff = 2.0 * wt.astype(np.float64) / (3.0 * wt.astype(np.float64).sum((1, 2, 3)))[:, None, None, None] / 2.0
    dg = coeff * (2.0 ** -22 + 2.0 ** -21 * np.abs(d))                                   # (B, 3, h, w)
    E0 = chain["forward"]["E0"]
    scale = np.where(E0 > 0.0, 1.0 / np.where(E0 > 0.0, E0, 1.0), 0.0)[:, :, None, None] * chain["wgt"][:, None]
    tol = chain["tol"] + scale * dg.sum((2, 3))[:, :, None, None]
    tol_value = float(np.sum(0.5 * coeff * (2.0 * np.abs(d) * 2.0 ** -22 + 2.0 ** -44)) + (3 * h * w + 8) * 2.0 ** -24 * want_value)
    print("ShadowLoss: value %.6e, oracle %.6e, |difference| %.3e (bound %.3e)" % (float(value.detach()), want_value,
                                                                                   abs(float(value.detach()) - want_value), tol_value))
    assert want_value > 0.0 and abs(float(value.detach()) - want_value) <= tol_value
    within("ShadowLoss", p.grad, want_grad, tol)
    # pred is true: exactly zero, with a zero gradient
    t = cuda(true).requires_grad_(True)
    zero = loss(t, t)
    zero.backward()
    assert float(zero) == 0.0 and torch.all(t.grad == 0.0)
    # one descent step in the right direction lowers the loss (a sign check, not a convergence claim)
    with torch.no_grad():
        lr = 0.1 * value / (p.grad * p.grad).sum()
        after = loss(p - lr * p.grad, cuda(true))
    print("ShadowLoss: one step of size %.3e: %.6e -> %.6e" % (float(lr), float(value.detach()), float(after)))
    assert float(after) < float(value.detach())
