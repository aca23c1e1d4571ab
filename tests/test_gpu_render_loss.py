"""GPU: the gradient of the sphere renders with respect to the panorama (``eml_sphere_render_bwd_f32`` through
``emlight_amd.evaluate.render_spheres`` / ``RenderLoss``) against the float64 restatement of its definition
(``render_grad_oracle.py``), and the render loss as a term of the projector's generator step.

The tolerance is derived, not measured.  For one image, with ``abs_vjp`` the definition evaluated on ``|K|``, ``|w|``, ``|g|``:

    tol_b = (M_int * P + C_max + 4 m + 64) * 2^-24 * max_t abs_vjp_b[t]

``M_int`` the number of integral materials and ``P`` the inside pixels (the worst case of an f32 summation of ``M_int P`` terms
into one accumulator), ``C_max`` the largest number of mirror taps on one texel (their summation), ``4 m`` the rounding of
``x^m`` (``m`` times the 4 roundings behind ``x``), 64 for the weights' own roundings (``dOmega`` times the normalisation, the
tap weights' three) with a margin -- the forward's bound (``test_gpu_sphere_render.py``) with the roles exchanged."""
import functools

import numpy as np
import pytest
import torch

from tests import render_grad_oracle as grad_oracle
from tests import sphere_render_oracle as oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ALL = oracle.MATERIALS


def hdr(B, H, W, seed):
    """U[0,1)^4 * 50 + 0.01: strictly positive, a dynamic range of a few thousand (as ``test_gpu_sphere_render.py``)."""
    g = np.random.default_rng([seed, B, H, W])
    return (g.random((B, 3, H, W)) ** 4 * 50.0 + 0.01).astype(np.float32)


def grads(B, M, S, seed):
    """Signed, a few decades of magnitude, and LARGE outside the disc: those values must never be read."""
    g = np.random.default_rng([seed, B, M, S])
    v = (g.standard_normal((B, M, 3, S, S)) * 10.0 ** g.uniform(-2, 1, (B, M, 3, S, S))).astype(np.float32)
    v[..., ~oracle.mask(S)] = 1e30
    return v


@functools.lru_cache(maxsize=None)
def weights(H, W, S, az, m):
    return oracle.weights(H, W, S, az, m)


@functools.lru_cache(maxsize=None)
def c_max(H, W, S, az):
    return grad_oracle.max_taps_on_a_texel(H, W, S, az)


def want_and_tol(g, H, S, materials, az, m):
    """The oracle's gradient (B, 3, H, W) and tol_b (B,) for ``g`` in the order of ``materials``."""
    W = 2 * H
    K = weights(H, W, S, az, m) if set(materials) - {"mirror"} else None
    want = grad_oracle.vjp(g, H, W, S, materials, az, m, K=K)
    scale = grad_oracle.abs_vjp(g, H, W, S, materials, az, m, K=K).reshape(g.shape[0], -1).max(1)
    m_int = len(set(materials) - {"mirror"})
    c = c_max(H, W, S, az) if "mirror" in materials else 0
    P = int(oracle.mask(S).sum())
    return want, (m_int * P + c + 4 * m + 64) * EPS * scale


def check_grad(got, g, H, S, materials, az, m, what):
    want, tol = want_and_tol(g, H, S, materials, az, m)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    for b in range(got.shape[0]):
        err = float(np.abs(got[b] - want[b]).max())
        print("%s %s image %d: err %.3e tol %.3e" % (what, "+".join(materials), b, err, tol[b]))
        assert err <= tol[b], (what, materials, b, err, tol[b])


def device_grad(x, g, S, materials=ALL, az=180.0, m=50.0):
    """x (B, 3, H, W), g (B, M, 3, S, S) numpy -> x.grad after (render_spheres(x) * g).sum().backward()."""
    from emlight_amd.evaluate import render_spheres
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    out = render_spheres(xt, size=S, materials=materials, view_azimuth_deg=az, phong_exponent=m)
    assert out.requires_grad
    (out * torch.from_numpy(g).cuda()).sum().backward()
    assert xt.grad is not None and xt.grad.shape == xt.shape
    return xt.grad


# ------------------------------------------------------------------------------------------------ 1. against the oracle
SHAPES = [(16, 8, 3, 50.0, 180.0),       # P = 52, less than one 64-pixel chunk; 9 columns
          (16, 9, 11, 50.0, 180.0),      # P = 69 crosses a chunk; 33 columns cross a 32-column tile
          (16, 9, 33, 1.0, 0.0),         # 99 columns cross a 96-column group
          (12, 33, 2, 50.0, 180.0),      # 288 texels, a ragged 128-texel group; 861 pixels; up to 25 mirror taps on one texel
          (16, 8, 2, 200.0, 77.3),       # Phong exponent 200, azimuth 77.3
          (128, 16, 2, 50.0, 180.0),     # the real texel extent
          (16, 33, 9, 50.0, 180.0)]      # 861 pixels with 27 columns


@pytest.mark.parametrize("H,S,B,m,az", SHAPES)
def test_gradient_against_the_oracle(H, S, B, m, az):
    x = hdr(B, H, 2 * H, 31)
    for materials in (ALL, ("diffuse",), ("glossy",), ("mirror",), ("mirror", "diffuse")):
        g = grads(B, len(materials), S, 32)
        check_grad(device_grad(x, g, S, materials, az, m), g, H, S, materials, az, m, "H %d S %d B %d" % (H, S, B))


# ------------------------------------------------------------------------------------------------ 2. one row of K
def _pixel_list(S):
    return np.flatnonzero(oracle.mask(S).ravel())


def _one_hot(S, M, slot, ch, pix):
    g = np.zeros((1, M, 3, S, S), dtype=np.float32)
    g[0, slot, ch].reshape(-1)[pix] = 1.0
    return g


@pytest.mark.parametrize("S", [8, 9])
@pytest.mark.parametrize("name", ["diffuse", "glossy"])
def test_one_hot_gradient_is_a_row_of_the_weights(S, name):
    """g = 1 at one inside pixel, one channel, one material: the gradient is that pixel's row of K, no summation to hide
    behind; the other channels and the other material's slot contribute exactly nothing."""
    H, W = 16, 32
    x = hdr(1, H, W, 33)
    pixels = _pixel_list(S)
    slot = ALL.index(name)
    for q, ch in ((0, 0), (len(pixels) // 2, 1), (len(pixels) - 1, 2)):           # top rim, centre row, bottom rim
        g = _one_hot(S, 3, slot, ch, pixels[q])
        got = device_grad(x, g, S)
        check_grad(got, g, H, S, ALL, 180.0, 50.0, "one-hot %s pixel %d" % (name, q))
        row = weights(H, W, S, 180.0, 50.0)[slot][q].reshape(H, W)
        tol = (int(oracle.mask(S).sum()) + 4 * 50 + 64) * EPS * float(row.max())
        host = got.cpu().numpy()
        assert np.abs(host[0, ch] - row).max() <= tol
        assert np.all(np.delete(host[0], ch, 0) == 0.0)


def test_one_hot_gradient_of_the_mirror_wrap_clamp_and_ordinary():
    H, W = 16, 32
    picks = []
    # the centre pixel at azimuth 180 looks back at azimuth 0: c0 = W - 1, c1 = 0 (the column wrap)
    idx, w = grad_oracle.taps(H, W, 9)
    centre = int(np.flatnonzero(_pixel_list(9) == 4 * 9 + 4)[0])
    assert idx[centre, 0] % W == W - 1 and idx[centre, 1] % W == 0
    picks.append((9, centre))
    # an ordinary one: four distinct texels, no wrap
    ordinary = int(np.flatnonzero((idx[:, 1] == idx[:, 0] + 1) & (idx[:, 2] == idx[:, 0] + W) & (w.min(1) > 0.01))[0])
    picks.append((9, ordinary))
    # a pixel whose row coordinate clamps: r0 == r1, two taps fall on one texel and add
    idx33, _ = grad_oracle.taps(H, W, 33)
    clamped = np.flatnonzero(idx33[:, 0] == idx33[:, 2])
    assert len(clamped) >= 1
    picks.append((33, int(clamped[0])))
    for S, q in picks:
        x = hdr(1, H, W, 34)
        ti, tw = grad_oracle.taps(H, W, S)
        for materials in (("mirror",), ALL):
            g = _one_hot(S, len(materials), len(materials) - 1, 1, _pixel_list(S)[q])
            got = device_grad(x, g, S, materials)
            check_grad(got, g, H, S, materials, 180.0, 50.0, "one-hot mirror S %d pixel %d" % (S, q))
            host = got.cpu().numpy()[0, 1].reshape(-1)
            want = np.zeros(H * W)
            np.add.at(want, ti[q], tw[q])
            assert np.array_equal(host != 0, want != 0) and np.abs(host - want).max() <= 8 * EPS     # at most 4 weights of <= 1
            assert abs(float(host.sum()) - 1.0) <= 8 * EPS


# ------------------------------------------------------------------------------------------------ 3. adjoint on the device
def test_adjoint_identity_on_the_device():
    """<render(x), g> and <x, grad> accumulated in f64 on the host: both are <K x, g> up to the forward's bound on the render
    (``test_gpu_sphere_render.py``) weighed by |g| and tol_b weighed by |x|, each summed over the outputs."""
    from emlight_amd.evaluate import render_spheres
    H, W, S, B, m, az = 128, 256, 16, 2, 50.0, 180.0
    x = hdr(B, H, W, 35)
    g = grads(B, 3, S, 36)
    inside = oracle.mask(S)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    out = render_spheres(xt, size=S)
    (out * torch.from_numpy(g).cuda()).sum().backward()
    r = out.detach().cpu().numpy().astype(np.float64)[..., inside]                # (B, 3, 3, P)
    gi = g.astype(np.float64)[..., inside]
    lhs = float(np.sum(r * gi))
    rhs = float(np.sum(x.astype(np.float64) * xt.grad.cpu().numpy().astype(np.float64)))
    Kd, Kg = weights(H, W, S, az, m)
    flat = x.astype(np.float64).reshape(B, 3, H * W)
    bound = 0.0
    for b in range(B):
        for i, name in enumerate(ALL):
            if name == "mirror":
                tol_f = 32 * EPS * float(np.abs(x).max())
            else:
                tol_f = (H * W + 4 * m + 64) * EPS * float(np.abs(flat[b] @ (Kd if i == 0 else Kg).T).max())
            bound += tol_f * float(np.abs(gi[b, i]).sum())
    _, tol_b = want_and_tol(g, H, S, ALL, az, m)
    for b in range(B):
        bound += tol_b[b] * float(np.abs(x[b]).astype(np.float64).sum())
    print("<render(x), g> %.10g  <x, grad> %.10g  difference %.3e  bound %.3e" % (lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------------------ 4. bit reproducibility
@pytest.mark.parametrize("H,S", [(16, 9), (128, 16)])
def test_gradient_is_bit_reproducible_and_independent_of_the_batch(H, S):
    x = hdr(3, H, 2 * H, 37)
    g = grads(3, 3, S, 38)
    a, b = device_grad(x, g, S), device_grad(x, g, S)
    assert torch.equal(a, b)
    # no split of the sum over the pixels and an MFMA adds its k terms in order: the same bits in any batch
    assert torch.equal(device_grad(x[:1], g[:1], S), a[:1])


# ------------------------------------------------------------------------------------------------ 5. RenderLoss
@pytest.mark.parametrize("materials", [("diffuse", "glossy"), ALL])
def test_render_loss_value_gradient_and_no_host_sync(materials):
    from emlight_amd.evaluate import RenderLoss, render_spheres
    H, W, S, B = 16, 32, 9, 3
    M = len(materials)
    P = int(oracle.mask(S).sum())
    pred = torch.from_numpy(hdr(B, H, W, 39)).cuda().requires_grad_(True)
    true = torch.from_numpy(hdr(B, H, W, 40)).cuda().requires_grad_(True)
    crit = RenderLoss(size=S, materials=materials)
    loss = crit(pred, true)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    assert true.grad is None and pred.grad is not None
    with torch.no_grad():
        a = render_spheres(pred, size=S, materials=materials).cpu().numpy().astype(np.float64)
        b = render_spheres(true, size=S, materials=materials).cpu().numpy().astype(np.float64)
    inside = oracle.mask(S)
    rmse2 = ((a - b)[..., inside] ** 2).sum((2, 3)) / (3 * P)                      # (B, M): the square of render_metrics' rmse
    want = float(rmse2.mean())
    value = float(loss.detach())
    rel = abs(value - want) / want
    print("loss %.9g want %.9g rel %.3e bound %.3e" % (value, want, rel, (3 * S * S * M + 8) * EPS))
    assert rel <= (3 * S * S * M + 8) * EPS
    g = (2.0 * (a - b) / (3.0 * P * B * M)).astype(np.float32)
    check_grad(pred.grad, g, H, S, materials, 180.0, 50.0, "RenderLoss")
    # the value in a no-grad call is the same number
    assert float(crit(pred.detach(), true.detach())) == value
    # after the first call of a geometry a forward plus backward only enqueues work
    first = pred.grad.clone()
    pred.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        crit(pred, true).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(pred.grad, first)


# ------------------------------------------------------------------------------------------------ 6. training
def _generator_step(seed, **kw):
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.model_trainer import Trainer
    torch.manual_seed(seed)
    opt = networks.default_options(ngf=4, ndf=4, **{k: v for k, v in kw.items() if v is not None})
    for k, v in kw.items():
        if v is None:
            delattr(opt, k)
    tr = Trainer(opt, device="cuda")
    tr.run_generator_one_step(data.projector_batch(2, "cuda", seed=3))
    return tr


def test_training_step_with_the_render_term():
    tr = _generator_step(0, lambda_render=1.0, render_size=8)
    assert set(tr.g_losses) == {"GAN", "GAN_Feat", "COS", "Render"}
    render = tr.g_losses["Render"]
    assert render.shape == () and bool(torch.isfinite(render)) and float(render) > 0
    for name, q in tr.model.netG.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
    # off (0, the default) and absent (an options object from before the switch): today's terms, bit for bit
    off, absent = _generator_step(0, lambda_render=0.0), _generator_step(0, lambda_render=None, render_size=None)
    assert not hasattr(absent.opt, "lambda_render")
    assert set(off.g_losses) == set(absent.g_losses) == {"GAN", "GAN_Feat", "COS"}
    assert all(torch.equal(off.g_losses[k], absent.g_losses[k]) for k in off.g_losses)
    # and the render term changed the step: it is part of the objective, not a reported number
    assert any(not torch.equal(p.grad, q.grad) for p, q in zip(tr.model.netG.parameters(), off.model.netG.parameters()))
