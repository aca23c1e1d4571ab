"""GPU: ``SamplesLoss`` on D-dimensional samples, (B, N, D) (eml_sinkhorn_fwd_dim_f32), and the gradients of the weights
(eml_sinkhorn_bwd_weights_f32), against the reference's vectors (tests/golden/sinkhorn_dim.npz), an f64 restatement of the
fork's loop with autograd, and the D = 1 launch they must leave alone."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle
from tests.conftest import Golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_ATOL = 1e-6      # the bounds of test_gpu_sinkhorn.py::test_golden_cases
GRAD_RTOL = 1e-4

# (B, N, D) on every loop kernel D > 1 dispatches to: register-resident (N <= 128), LDS-tiled (128 < N <= 512, N % 4 == 0,
# the small batches the split kernel takes at D = 1 included), streaming (N % 4 != 0 or N > 512); D = 2..8 covers the three
# instantiations (2, 4, 8 components) with and without zero tail components
SHAPES = [(5, 128, 3), (3, 96, 2), (4, 33, 5), (2, 128, 8), (3, 200, 4), (16, 256, 3), (2, 384, 6), (2, 512, 2),
          (2, 202, 3), (2, 516, 2), (2, 202, 8)]


def _crit(n, blur=.05, reach=None, diameter=None, **kw):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    return SamplesLoss("sinkhorn", p=2, blur=blur, reach=reach, diameter=diameter, anchors=n, **kw)


def _inputs(B, n, D, seed=1234):
    g = torch.Generator().manual_seed(seed)
    x = torch.softmax(torch.randn(B, n, D, generator=g), 1)
    y = torch.softmax(3 * torch.randn(B, n, D, generator=g), 1)
    return x, y


def _weights(B, n, seed=7):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, n, generator=g)
    a[:, ::7] = 0
    b = torch.rand(B, n, generator=g)
    b[:, 3::11] = 0
    return a / a.sum(1, keepdim=True), b / b.sum(1, keepdim=True)


def loss_f64(x, y, M, blur, reach=None, a=None, b=None, p=2, scaling=.5, dtype=torch.float64, aux=None):
    """The fork's Sinkhorn loss in f64 with autograd (sinkhorn_divergence.py:9-109): the cost of ``oracle.spherical_cost``
    (any D), softmins damped by lam = 1 / (1 + eps / reach**p) when a reach is given, the duals detached into the last
    extrapolation, loss <a, b_x - a_x> + <b, a_y - b_y>.  The diameter is that of the f32 inputs, as the kernel sees them.
    ``dtype``: the precision of ``x, y`` (and of ``a, b`` when given) -- torch.float32 restates the reference's own
    arithmetic; ``aux``: a dict that receives ``eps_s``, ``diameter`` and the four final ``duals`` (4, B, N)."""
    B, N, _ = x.shape
    diameter = oracle.max_diameter(x.detach().float(), y.detach().float())
    eps_s = oracle.epsilon_schedule(p, diameter, blur, scaling)
    lam = (lambda e: 1.0) if reach is None else (lambda e: 1.0 / (1.0 + e / reach ** p))
    M = M.to(dtype)
    a = torch.full((B, N), 1.0 / N, dtype=dtype) if a is None else a
    b = torch.full((B, N), 1.0 / N, dtype=dtype) if b is None else b
    la, lb = oracle.log_weights(a.detach()), oracle.log_weights(b.detach())
    C = lambda u, v: oracle.spherical_cost(u, v, M)   # noqa: E731
    C_xx, C_yy, C_xy, C_yx = C(x, x.detach()), C(y, y.detach()), C(x, y.detach()), C(y, x.detach())
    sm = oracle.softmin
    with torch.no_grad():
        e = eps_s[0]
        a_x, b_y, a_y, b_x = (lam(e) * sm(e, C_xx, la), lam(e) * sm(e, C_yy, lb),
                              lam(e) * sm(e, C_yx, la), lam(e) * sm(e, C_xy, lb))
        for e in eps_s:
            at_x, bt_y = lam(e) * sm(e, C_xx, la + a_x / e), lam(e) * sm(e, C_yy, lb + b_y / e)
            at_y, bt_x = lam(e) * sm(e, C_yx, la + b_x / e), lam(e) * sm(e, C_xy, lb + a_y / e)
            a_x, b_y, a_y, b_x = .5 * (a_x + at_x), .5 * (b_y + bt_y), .5 * (a_y + at_y), .5 * (b_x + bt_x)
    a_x, b_y = lam(e) * sm(e, C_xx, (la + a_x / e).detach()), lam(e) * sm(e, C_yy, (lb + b_y / e).detach())
    a_y, b_x = lam(e) * sm(e, C_yx, (la + b_x / e).detach()), lam(e) * sm(e, C_xy, (lb + a_y / e).detach())
    if aux is not None:
        aux.update(eps_s=eps_s, diameter=diameter, duals=torch.stack([a_x, b_y, a_y, b_x]).detach())
    return oracle.sinkhorn_cost(a, b, a_x, b_y, a_y, b_x)


def _loss_close(got, want, what):
    want = np.asarray(want)
    np.testing.assert_allclose(got, want, rtol=0, atol=LOSS_ATOL * max(1.0, np.abs(want).max() / 1e-4), err_msg=what)


def _grad_close(got, want, what):
    want = np.asarray(want)
    np.testing.assert_allclose(got, want, rtol=GRAD_RTOL, atol=GRAD_RTOL * np.abs(want).max(), err_msg=what)


_G = Golden("sinkhorn_dim")
CASES = sorted({k.split("/")[0] for k in _G.z.files})


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(case):
    """The reference's own loss, gradients, duals, schedule and diameter on (B, N, D) samples; the weighted cases also the
    weights' gradients from its autograd."""
    c = _G.case(case)
    B, n, D = c["x"].shape
    reach = float(c["reach"]) or None
    x = torch.from_numpy(c["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(c["y"]).cuda()
    crit = _crit(n, float(c["blur"]), reach)
    if "alpha" in c:
        a = torch.from_numpy(c["alpha"]).cuda().requires_grad_(True)
        b = torch.from_numpy(c["beta"]).cuda().requires_grad_(True)
        loss = crit(a, x, b, y)
    else:
        loss = crit(x, y)
    loss.sum().backward()
    _loss_close(loss.detach().cpu().numpy(), c["loss"], case + " loss")
    assert x.grad.shape == (B, n, D)
    _grad_close(x.grad.cpu().numpy(), c["grad_x"], case + " grad_x")
    if "alpha" in c:
        _grad_close(a.grad.cpu().numpy(), c["grad_alpha"], case + " grad_alpha")
        _grad_close(b.grad.cpu().numpy(), c["grad_beta"], case + " grad_beta")
    raw = crit.forward_raw(x.detach(), y) if "alpha" not in c else None
    if raw is not None:
        duals = raw["duals"].cpu().numpy()
        np.testing.assert_allclose(duals, c["duals"], rtol=0, atol=2e-6 * max(1.0, np.abs(c["duals"]).max()))
        n_eps = int(raw["n_eps"].item())
        np.testing.assert_allclose(raw["eps_s"][:n_eps].cpu().numpy(), c["eps_s"], rtol=1e-6)
        assert float(raw["diameter"].item()) == pytest.approx(float(c["diameter"]), rel=1e-6)
        assert raw["gx"].shape == (B, n, D) and raw["gy"].shape == (B, n, D)


@pytest.mark.parametrize("B,n,D", SHAPES)
def test_autograd_vs_f64_oracle(B, n, D):
    """Loss and d loss / d x on every loop variant, against f64 autograd of the fork's loss (balanced)."""
    x, y = _inputs(B, n, D)
    M = oracle.anchor_cost_matrix(n)
    xo = x.double().requires_grad_(True)
    want = loss_f64(xo, y.double(), M, .05)
    want.sum().backward()
    xg = x.cuda().requires_grad_(True)
    got = _crit(n)(xg, y.cuda())
    got.sum().backward()
    _loss_close(got.detach().cpu().numpy(), want.detach().numpy(), "loss")
    _grad_close(xg.grad.cpu().numpy(), xo.grad.numpy(), "grad_x")


@pytest.mark.parametrize("B,n,D,reach", [(3, 96, 3, .1), (2, 256, 4, .3), (2, 202, 2, .1), (3, 128, 6, None),
                                         (16, 256, 2, None), (2, 516, 3, .2)])
def test_weights_reach_and_weight_gradients_vs_f64_oracle(B, n, D, reach):
    """Weights with zeros, a reach, and the gradients of x, y, alpha and beta on every loop variant, against f64 autograd;
    the weights' gradients have the caller's shape."""
    x, y = _inputs(B, n, D, seed=99)
    a, b = _weights(B, n)
    M = oracle.anchor_cost_matrix(n)
    xo, yo = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ao, bo = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = loss_f64(xo, yo, M, .05, reach, ao, bo)
    (want * torch.linspace(.5, 1.5, B, dtype=torch.float64)).sum().backward()
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    ag = a.cuda().view(B, n, 1).requires_grad_(True)   # the caller's shape is kept
    bg = b.cuda().requires_grad_(True)
    got = _crit(n, reach=reach)(ag, xg, bg, yg)
    (got * torch.linspace(.5, 1.5, B, device="cuda")).sum().backward()
    _loss_close(got.detach().cpu().numpy(), want.detach().numpy(), "loss")
    _grad_close(xg.grad.cpu().numpy(), xo.grad.numpy(), "grad_x")
    _grad_close(yg.grad.cpu().numpy(), yo.grad.numpy(), "grad_y")
    assert ag.grad.shape == (B, n, 1) and bg.grad.shape == (B, n)
    _grad_close(ag.grad.view(B, n).cpu().numpy(), ao.grad.numpy(), "grad_alpha")
    _grad_close(bg.grad.cpu().numpy(), bo.grad.numpy(), "grad_beta")


def test_weight_gradients_at_d1_vs_f64_oracle():
    """The weights' gradients on 1-D samples too (they were dropped before): register-resident and split kernels."""
    for B, n in ((4, 96), (3, 256)):
        x, y = _inputs(B, n, 1, seed=5)
        a, b = _weights(B, n)
        ao, bo = a.double().requires_grad_(True), b.double().requires_grad_(True)
        loss_f64(x.double(), y.double(), oracle.anchor_cost_matrix(n), .05, None, ao, bo).sum().backward()
        ag, bg = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        _crit(n)(ag, x.cuda(), bg, y.cuda()).sum().backward()
        _grad_close(ag.grad.cpu().numpy(), ao.grad.numpy(), "grad_alpha")
        _grad_close(bg.grad.cpu().numpy(), bo.grad.numpy(), "grad_beta")


def _fwd_dim_d1_args(x, y, crit, o, rho):
    from emlight_amd import _lib
    M, Mt = crit.cost_matrix(x.device)
    B, N = x.shape[:2]
    return (_lib.ptr(x), _lib.ptr(y), _lib.ptr(M), _lib.ptr(Mt), None, None, .05, .5, 2, -1.0, None, _lib.ptr(o["eps_s"]),
            _lib.ptr(o["n_eps"]), _lib.ptr(o["diameter"]), _lib.ptr(o["loss"]), _lib.ptr(o["gx"]), _lib.ptr(o["gy"]),
            _lib.ptr(o["work"]), B, N)


@pytest.mark.parametrize("B,n", [(4, 128), (40, 256), (16, 256), (2, 202)])
@pytest.mark.parametrize("rho", [0.0, .01])
def test_dim_entry_at_d1_is_bit_identical_to_the_rho_entry(B, n, rho):
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_outputs
    L = _lib.lib()
    x, y = _inputs(B, n, 1, seed=3)
    x, y = x.cuda().contiguous(), y.cuda().contiguous()
    crit = _crit(n)
    outs = []
    for entry in ("rho", "dim"):
        o = sinkhorn_outputs(B, n, x.device, True, True)
        args = _fwd_dim_d1_args(x, y, crit, o, rho)
        if entry == "rho":
            rc = L.eml_sinkhorn_fwd_rho_f32(*args, 0, rho, None, _lib.current_stream())
        else:
            rc = L.eml_sinkhorn_fwd_dim_f32(*args, 1, 0, rho, None, _lib.current_stream())
        assert rc == 0
        n_eps = int(o["n_eps"].item())   # a loss call writes the schedule buffer up to n_eps only
        outs.append({k: o[k].clone() for k in ("loss", "gx", "gy", "n_eps", "diameter")}
                    | {"eps_s": o["eps_s"][:n_eps].clone(), "duals": o["work"][:8 * B * n].clone()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("B,n", [(4, 128), (3, 96), (3, 256), (2, 202)])
def test_zero_padded_components_reproduce_the_1d_result(B, n):
    """(B, N, 1) samples padded with zero components: the loss and the first gradient component of the 1-D launch, the
    padded components' gradients exactly zero.  Not bit for bit: the D-term cost rounds |p|^2, p.q and |q|^2 separately
    where the 1-D cost's products are contracted into fmas, and the loss -- a difference of duals some 1e3 times its size
    -- shows those ulp-level cost differences at up to ~1e-5 of itself (measured: 4.7e-10 absolute on losses of 1e-4,
    three orders of magnitude inside the golden tests' 1e-6 bound)."""
    x, y = _inputs(B, n, 1, seed=11)
    crit = _crit(n)
    x1, y1 = x.cuda().requires_grad_(True), y.cuda()
    l1 = crit(x1, y1)
    l1.sum().backward()
    for D in (2, 3, 8):
        pad = torch.zeros(B, n, D - 1)
        xd = torch.cat([x, pad], 2).cuda().requires_grad_(True)
        yd = torch.cat([y, pad], 2).cuda()
        ld = crit(xd, yd)
        ld.sum().backward()
        np.testing.assert_allclose(ld.detach().cpu().numpy(), l1.detach().cpu().numpy(), rtol=5e-5, atol=0, err_msg="D=%d" % D)
        np.testing.assert_allclose(xd.grad[..., :1].cpu().numpy(), x1.grad.cpu().numpy(), rtol=1e-4,
                                   atol=1e-5 * float(x1.grad.abs().max()), err_msg="D=%d" % D)
        assert float(xd.grad[..., 1:].abs().max()) == 0.0


def test_properties_at_full_size():
    """S(x, x) = 0, symmetry and run-to-run bits at B = 256, D = 3."""
    B, n = 256, 128
    x, y = _inputs(B, n, 3, seed=9)
    x, y = x.cuda(), y.cuda()
    crit = _crit(n, diameter=1.0)
    assert float(crit(x, x).abs().max()) <= 2e-7
    sxy, syx = crit(x, y), crit(y, x)
    np.testing.assert_allclose(sxy.cpu().numpy(), syx.cpu().numpy(), rtol=0, atol=1e-6)
    assert float(sxy.min()) > 0
    assert torch.equal(crit(x, y), sxy)
    r1, r2 = _crit(n).forward_raw(x, y), _crit(n).forward_raw(x, y)
    for k in ("loss", "gx", "gy", "n_eps", "diameter", "duals"):
        assert torch.equal(r1[k], r2[k]), k
    k = int(r1["n_eps"].item())
    assert torch.equal(r1["eps_s"][:k], r2["eps_s"][:k])


def test_standalone_schedule_matches_the_loop_kernels():
    """eml_sinkhorn_schedule_dim_f32 derives the diameter and schedule the loss call derives, from 2*D range floats too."""
    from emlight_amd import _lib
    L = _lib.lib()
    B, n, D = 4, 128, 3
    x, y = _inputs(B, n, D, seed=2)
    x, y = x.cuda(), y.cuda()
    raw = _crit(n).forward_raw(x, y)
    eps, n_eps, diam = torch.empty(64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), \
        torch.empty(1, device="cuda")
    assert L.eml_sinkhorn_schedule_dim_f32(_lib.ptr(x), _lib.ptr(y), B * n, D, .05, .5, 2, -1.0, None, _lib.ptr(eps),
                                           _lib.ptr(n_eps), _lib.ptr(diam), _lib.current_stream()) == 0
    assert torch.equal(n_eps, raw["n_eps"]) and torch.equal(diam, raw["diameter"])
    k = int(n_eps.item())
    assert torch.equal(eps[:k], raw["eps_s"][:k]) and float(eps[k:].abs().max()) == 0.0
    assert float(diam.item()) == pytest.approx(oracle.max_diameter(x.cpu(), y.cpu()), rel=1e-6)
    # an outside range (the other ranks' shards) folded into every component: component 1 reaches down to -1
    rng = torch.tensor([0., -1., 0., 1., 1., 1.], device="cuda")
    assert L.eml_sinkhorn_schedule_dim_f32(_lib.ptr(x), _lib.ptr(y), B * n, D, .05, .5, 2, -1.0, _lib.ptr(rng),
                                           _lib.ptr(eps), _lib.ptr(n_eps), _lib.ptr(diam), _lib.current_stream()) == 0
    lo = torch.minimum(torch.minimum(x.reshape(-1, D).amin(0), y.reshape(-1, D).amin(0)), rng[:D]).cpu().double()
    hi = torch.maximum(torch.maximum(x.reshape(-1, D).amax(0), y.reshape(-1, D).amax(0)), rng[D:]).cpu().double()
    assert float(lo[1]) == -1.0
    assert float(diam.item()) == pytest.approx(float((hi - lo).norm()), rel=1e-6)


def _diameter_case():
    g = torch.Generator().manual_seed(5)
    B, N, D = 8, 128, 3
    x = torch.softmax(torch.randn(B, N, D, generator=g), 1)
    y = torch.softmax(3 * torch.randn(B, N, D, generator=g), 1)
    y[B // 2:, :, 1] = torch.softmax(8 * torch.randn(B // 2, N, generator=g), 1)   # rank 1's shard has the peaks
    return x, y


def _diameter_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK="0",
                      WORLD_SIZE=str(world), EML_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from emlight_amd.RegressionNetwork.engine import init_distributed
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    init_distributed()
    x, y = _diameter_case()
    h = x.shape[0] // world
    xs, ys = x[rank * h:(rank + 1) * h].cuda(), y[rank * h:(rank + 1) * h].cuda()
    out = {}
    for name, sync in (("synced", True), ("local", False)):
        r = SamplesLoss("sinkhorn", p=2, blur=.05, anchors=x.shape[1], sync_diameter=sync).forward_raw(xs, ys)
        out[name + "_loss"] = r["loss"].cpu().numpy()
        out[name + "_eps"] = r["eps_s"][:int(r["n_eps"].item())].cpu().numpy()
        out[name + "_gx"] = r["gx"].cpu().numpy()
    np.savez(os.path.join(out_dir, "diam%d.npz" % rank), **out)
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sync_diameter_two_ranks_at_d3(tmp_path):
    """Two ranks x B/2 with ``sync_diameter`` all-reduce the 2*D component ranges and reproduce the one-process schedule,
    loss and gradient of the whole batch at D = 3; without it rank 0 runs another schedule."""
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_diameter_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    x, y = _diameter_case()
    w = SamplesLoss("sinkhorn", p=2, blur=.05, anchors=x.shape[1]).forward_raw(x.cuda(), y.cuda())
    eps = w["eps_s"][:int(w["n_eps"].item())].cpu().numpy()
    d = [np.load(tmp_path / ("diam%d.npz" % k)) for k in range(2)]
    for k in range(2):
        np.testing.assert_array_equal(d[k]["synced_eps"], eps)
    np.testing.assert_allclose(np.concatenate([d[0]["synced_loss"], d[1]["synced_loss"]]), w["loss"].cpu().numpy(),
                               rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.concatenate([d[0]["synced_gx"], d[1]["synced_gx"]]), w["gx"].cpu().numpy(),
                               rtol=1e-6, atol=1e-10)
    assert len(d[0]["local_eps"]) != len(eps) or not np.array_equal(d[0]["local_eps"], eps)


def test_adam_fit_of_points_and_of_weights_lowers_the_loss():
    """A short Adam fit of learnable (B, N, 3) points, and of learnable weights (a predicted distribution on fixed anchors:
    alpha = softmax(logits)), each towards a fixed target: the loss goes down."""
    B, n = 4, 128
    x0, y = _inputs(B, n, 3, seed=21)
    y = y.cuda()
    crit = _crit(n)
    x = x0.cuda().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=2e-3)
    first = None
    for _ in range(30):
        opt.zero_grad()
        loss = crit(x, y).sum()
        loss.backward()
        first = loss.item() if first is None else first
        opt.step()
    assert crit(x, y).sum().item() < 0.8 * first

    pos = torch.from_numpy(oracle.sphere_points(n)).float().cuda().expand(B, n, 3).contiguous()
    target = torch.softmax(4 * torch.randn(B, n, generator=torch.Generator().manual_seed(3)), 1).cuda()
    logits = torch.zeros(B, n, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([logits], lr=5e-2)
    first = None
    for _ in range(30):
        opt.zero_grad()
        loss = crit(torch.softmax(logits, 1), pos, target, pos).sum()
        loss.backward()
        assert logits.grad is not None and float(logits.grad.abs().max()) > 0
        first = loss.item() if first is None else first
        opt.step()
    assert crit(torch.softmax(logits, 1), pos, target, pos).sum().item() < 0.8 * first
