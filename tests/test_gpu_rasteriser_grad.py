"""GPU: convert_to_panorama's gradients wrt dirs, sizes and colors (eml_sg_rasterise_bwd_f32) against f64 autograd of the
oracle, the reference's own f32 autograd (rasteriser_grad.npz), the exhaustive loop, the colour-only launch, and a fit of
SG lobes to a panorama by gradient descent."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KINDS = [(32, 128, 128, "anchors"), (16, 256, 256, "anchors"), (3, 130, 128, "random"), (2, 600, 64, "random"),
         (2, 128, 128, "odd"), (2, 96, 72, "anchors")]


def _lobes(B, n, kind, g):
    """The inputs of test_gpu_rasteriser.py's cull test: Fibonacci anchors at size .0025, random directions with wide and
    narrow lobes, and "odd" ones (non-unit directions, zero / negative / huge sizes: never culled)."""
    if kind == "anchors":
        dirs = np.tile(oracle.sphere_points(n).reshape(1, 3 * n), (B, 1)).astype(np.float32)
        sizes = np.full((B, n), 0.0025, np.float32)
    else:
        d = g.standard_normal((B, n, 3))
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        sizes = g.uniform(0.0005, 0.3, (B, n)).astype(np.float32)
        if kind == "odd":
            d *= g.uniform(0.2, 3.0, (B, n, 1))
            sizes[:, ::7] = 0.0
            sizes[:, 1::7] = -0.01
            sizes[:, 2::7] = 1e30
        dirs = d.reshape(B, 3 * n).astype(np.float32)
    colors = g.uniform(0, 3, (B, 3 * n)).astype(np.float32)
    return dirs, sizes, colors


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grads_ours(dirs, sizes, colors, w, H):
    from emlight_amd.RegressionNetwork.util import convert_to_panorama
    t = [x.requires_grad_(True) for x in _cuda(dirs, sizes, colors)]
    (convert_to_panorama(*t, pano_hw=(H, 2 * H)) * _cuda(w)[0]).sum().backward()
    return [x.grad.double().cpu().numpy() for x in t]


def _grads_oracle(dirs, sizes, colors, w, H, dtype):
    t = [torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (dirs, sizes, colors)]
    (oracle.convert_to_panorama(*t, height=H) * torch.from_numpy(w).to(dtype)).sum().backward()
    return [x.grad.double().numpy() for x in t]


@pytest.mark.parametrize("B,n,H,kind", [(3, 128, 128, "anchors"), (4, 7, 128, "random"), (2, 600, 64, "random"),
                                        (1, 256, 256, "cfg5"), (3, 130, 72, "random")])
def test_gradients_against_f64_autograd_of_the_oracle(B, n, H, kind):
    """No worse than the reference's own f32 arithmetic: for each gradient, the max abs error against f64 autograd of the
    oracle is at most 4x the f32 oracle's own (or 1e-5 of the gradient's largest magnitude, whichever is larger)."""
    g = np.random.default_rng([7, B, n, H])
    if kind == "cfg5":   # BASELINE cfg5's lobes: 256 Fibonacci anchors at size .0025, 256 x 512 (B kept small: the oracle's
        dirs, sizes, colors = _lobes(B, n, "anchors", g)   # per-light autograd graph costs ~1 GB per sample in f64)
    else:
        dirs, sizes, colors = _lobes(B, n, kind, g)
        if kind == "random":
            sizes = g.uniform(0.002, 0.3, (B, n)).astype(np.float32)
    w = g.standard_normal((B, 3, H, 2 * H)).astype(np.float32)
    want = _grads_oracle(dirs, sizes, colors, w, H, torch.float64)
    f32 = _grads_oracle(dirs, sizes, colors, w, H, torch.float32)
    got = _grads_ours(dirs, sizes, colors, w, H)
    for name, a, ref, o32 in zip(("dirs", "sizes", "colors"), got, want, f32):
        scale = float(np.abs(ref).max())
        err, err32 = float(np.abs(a - ref).max()), float(np.abs(o32 - ref).max())
        bound = max(4.0 * err32, 1e-5 * scale)
        print("d/d %-6s max|g| %.4g  err %.3g  f32 oracle err %.3g  ratio %.2f  (bound %.3g)"
              % (name, scale, err, err32, err / err32 if err32 else float("inf"), bound))
        assert err <= bound, (name, err, err32, scale)


@pytest.mark.parametrize("case", ["anchors_b2_n128", "random_b3_n42"])
def test_gradients_against_the_reference_fixture(case):
    """The reference's f32 autograd of (pano * w).sum() (tests/golden/make_golden_raster_grad.py), 128 x 256."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rasteriser_grad.npz"))
    c = {k: z[case + "/" + k] for k in ("dirs", "sizes", "colors", "w_q", "gdirs", "gsizes", "gcolors")}
    w = c["w_q"].astype(np.float32) / 4
    got = _grads_ours(c["dirs"], c["sizes"], c["colors"], w, 128)
    for name, a in zip(("gdirs", "gsizes", "gcolors"), got):
        want = c[name].astype(np.float64)
        np.testing.assert_allclose(a, want, rtol=1e-3, atol=1e-4 * np.abs(want).max(), err_msg=name)


@pytest.mark.parametrize("B,n,H,kind", KINDS)
def test_culled_gradients_are_bit_identical_to_the_exhaustive_loop(B, n, H, kind):
    """A culled light's exp2 underflows to exactly 0 on the whole patch, and every per-pixel term of the seven sums is that
    exponential times a finite factor: all three gradients equal the every-light-every-tile launch bit for bit (NaNs of the
    odd inputs included), and a second run of the same launch gives the same bits (no atomics)."""
    from emlight_amd.RegressionNetwork.util import rasterise_bwd_raw
    g = np.random.default_rng([8, B, n])
    dirs, sizes, colors = _lobes(B, n, kind, g)
    gout = g.standard_normal((B, 3, H, 2 * H)).astype(np.float32)
    a = _cuda(dirs, sizes, colors, gout)
    fast = rasterise_bwd_raw(*a, (H, 2 * H))
    full = rasterise_bwd_raw(*a, (H, 2 * H), exhaustive=True)
    again = rasterise_bwd_raw(*a, (H, 2 * H))
    for name, x, y, z in zip(("dirs", "sizes", "colors"), fast, full, again):
        assert torch.equal(_bits(x), _bits(y)), name
        assert torch.equal(_bits(x), _bits(z)), name
    if kind != "odd":
        assert all(bool(torch.isfinite(x).all()) for x in fast)


@pytest.mark.parametrize("B,n,H,kind", KINDS)
def test_colour_gradient_of_the_full_launch_is_the_colour_launch(B, n, H, kind):
    from emlight_amd.RegressionNetwork.util import rasterise_bwd_colors_raw, rasterise_bwd_raw
    g = np.random.default_rng([9, B, n])
    dirs, sizes, colors = _lobes(B, n, kind, g)
    gout = g.standard_normal((B, 3, H, 2 * H)).astype(np.float32)
    d, s, c, go = _cuda(dirs, sizes, colors, gout)
    for exhaustive in (False, True):
        _, _, gc = rasterise_bwd_raw(d, s, c, go, (H, 2 * H), exhaustive=exhaustive)
        assert torch.equal(_bits(gc), _bits(rasterise_bwd_colors_raw(d, s, go, (H, 2 * H), exhaustive=exhaustive)))


def test_partial_requests_match_the_full_launch():
    from emlight_amd.RegressionNetwork.util import convert_to_panorama, rasterise_bwd_raw
    B, n, H = 3, 130, 72
    g = np.random.default_rng(10)
    dirs, sizes, colors = _lobes(B, n, "random", g)
    gout = g.standard_normal((B, 3, H, 2 * H)).astype(np.float32)
    a = _cuda(dirs, sizes, colors, gout)
    all3 = rasterise_bwd_raw(*a, (H, 2 * H))
    for mask in range(1, 8):
        need = tuple(bool(mask >> k & 1) for k in range(3))
        part = rasterise_bwd_raw(*a, (H, 2 * H), need=need)
        for k in range(3):
            if need[k]:
                assert torch.equal(_bits(part[k]), _bits(all3[k])), (need, k)
            else:
                assert part[k] is None
        # autograd: a gradient for exactly the inputs that require one, equal to the raw launch's
        t = [x.clone().requires_grad_(r) for x, r in zip(a[:3], need)]
        convert_to_panorama(*t, pano_hw=(H, 2 * H)).backward(a[3])
        for k in range(3):
            if need[k]:
                assert torch.equal(_bits(t[k].grad), _bits(all3[k])), (need, k)
            else:
                assert t[k].grad is None


def _fit_problem():
    """16 known lobes (Fibonacci directions, sizes .02-.05) on a 64 x 128 panorama; the start: every direction turned by
    10 degrees, sizes x 1.5, colours off by up to 30 %."""
    g = np.random.default_rng(31)
    n = 16
    d = oracle.sphere_points(n)
    sizes = g.uniform(0.02, 0.05, n)
    colors = g.uniform(0.5, 2.0, (n, 3))
    r = g.standard_normal(d.shape)
    r -= (r * d).sum(1, keepdims=True) * d
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    a = np.deg2rad(10.0)
    d0 = np.cos(a) * d + np.sin(a) * r
    c0 = colors * g.uniform(0.7, 1.3, colors.shape)
    return (d, sizes, colors), (d0, 1.5 * sizes, c0)


def _fit(render, true, start, dtype, device, steps=100):
    T = lambda x: torch.tensor(x.reshape(1, -1), dtype=dtype, device=device)   # noqa: E731
    target = render(T(true[0]), T(true[1]), T(true[2])).detach()
    P = [T(x).requires_grad_(True) for x in start]
    opt = torch.optim.Adam([{"params": [P[0]], "lr": 0.01}, {"params": [P[1]], "lr": 0.002}, {"params": [P[2]], "lr": 0.03}])
    with torch.no_grad():
        mse0 = float(((render(*P) - target) ** 2).mean())
    for _ in range(steps):
        opt.zero_grad()
        ((render(*P) - target) ** 2).mean().backward()
        opt.step()
    with torch.no_grad():
        mse = float(((render(*P) - target) ** 2).mean())
    got = P[0].detach().double().cpu().numpy().reshape(-1, 3)
    got /= np.linalg.norm(got, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((got * true[0]).sum(1), -1.0, 1.0)))
    return mse0, mse, float(ang.max())


def test_fitting_lobes_to_a_panorama_by_gradient_descent():
    """Directions, sizes and colours of 16 SG lobes recovered with Adam through convert_to_panorama: the MSE falls by at least
    100x and every direction ends within 2 degrees of the true one -- as the same loop does on the f64 oracle."""
    from emlight_amd.RegressionNetwork.util import convert_to_panorama
    true, start = _fit_problem()
    for label, render, dtype, device in [
            ("f64 oracle", lambda d, s, c: oracle.convert_to_panorama(d, s, c, height=64), torch.float64, "cpu"),
            ("HIP", lambda d, s, c: convert_to_panorama(d, s, c, pano_hw=(64, 128)), torch.float32, "cuda")]:
        mse0, mse, ang = _fit(render, true, start, dtype, device)
        print("%s: MSE %.4g -> %.4g (x%.0f), worst direction %.3f deg" % (label, mse0, mse, mse0 / mse, ang))
        assert mse <= mse0 / 100, (label, mse0, mse)
        assert ang <= 2.0, (label, ang)
