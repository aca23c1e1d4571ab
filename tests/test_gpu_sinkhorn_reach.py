"""GPU: unbalanced Sinkhorn, ``SamplesLoss(reach=...)`` (eml_sinkhorn_fwd_rho_f32), against the reference's vectors
(tests/golden/sinkhorn_reach.npz), an f64 restatement of the fork's damped loop, and the balanced launch it must leave
alone."""
import math

import numpy as np
import pytest
import torch

import oracle
from tests.conftest import Golden

pytestmark = pytest.mark.gpu

LOSS_ATOL = 1e-6      # the bounds of test_gpu_sinkhorn.py
GRAD_RTOL = 1e-4

# every loop kernel: register-resident (N <= 128), split (small batch, N % 64 == 0 in [192, 512]), LDS-tiled (larger batches,
# N % 4 == 0, N <= 512), streaming (N % 4 != 0 or N > 512) -- the shapes of test_gpu_sinkhorn.py::test_autograd_vs_oracle
SHAPES = [(64, 128, .05), (7, 96, .025), (5, 33, .05), (3, 200, .05), (16, 256, .05), (4, 132, .05), (3, 384, .05),
          (2, 512, .025), (2, 202, .05), (2, 516, .05), (24, 256, .05), (40, 256, .05), (20, 384, .05), (3, 192, .05)]
# one shape per kernel, for the bitwise checks
VARIANTS = [(4, 128), (40, 256), (16, 256), (2, 202)]


def _crit(n, blur, reach=None, diameter=None):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    return SamplesLoss("sinkhorn", p=2, blur=blur, reach=reach, diameter=diameter, anchors=n)


def _inputs(B, n, seed=1234):
    g = torch.Generator().manual_seed(seed)
    x = torch.softmax(torch.randn(B, n, generator=g), 1).view(B, n, 1)
    y = torch.softmax(3 * torch.randn(B, n, generator=g), 1).view(B, n, 1)
    return x, y


def damped_loss_f64(x, y, M, blur, reach, a=None, b=None, p=2, scaling=.5):
    """The fork's unbalanced Sinkhorn in f64 (sinkhorn_divergence.py:35, 43-44, 65-109): every softmin times
    lam = 1 / (1 + eps / reach**p), the symmetrised averages unchanged, the loss <a, b_x - a_x> + <b, a_y - b_y> of the damped
    duals.  The diameter is the f32 range of the f32 inputs, as the kernel (and the reference's f32 run) sees it."""
    B, N, _ = x.shape
    eps_s = oracle.epsilon_schedule(p, oracle.max_diameter(x.detach().float(), y.detach().float()), blur, scaling)
    rho = reach ** p

    def lam(e):
        return 1.0 / (1.0 + e / rho)

    x, y, M = x.double(), y.double(), M.double()
    a = torch.full((B, N), 1.0 / N, dtype=torch.float64) if a is None else a.double()
    b = torch.full((B, N), 1.0 / N, dtype=torch.float64) if b is None else b.double()
    la, lb = oracle.log_weights(a), oracle.log_weights(b)
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
    return oracle.sinkhorn_cost(a, b, a_x, b_y, a_y, b_x)


def _close(got, want, what, atol):
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, err_msg=what)


def _grad_close(got, want, what):
    want = np.asarray(want)
    np.testing.assert_allclose(got, want, rtol=GRAD_RTOL, atol=GRAD_RTOL * np.abs(want).max(), err_msg=what)


_G = Golden("sinkhorn_reach")
CASES = sorted({k.split("/")[0] for k in _G.z.files})


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("gmloss")])
def test_golden_reach_cases(case):
    """The reference's own run with ``reach`` set: schedule, dampening schedule, loss, final duals and d/dx, at the bounds of
    test_gpu_sinkhorn.py::test_golden_cases (the fixture asserts that balanced numbers miss one of them by > 10x)."""
    c = _G.case(case)
    B, n = c["x"].shape
    crit = _crit(n, float(c["blur"]), float(c["reach"]))
    r = crit.forward_raw(torch.from_numpy(c["x"]).cuda().view(B, n, 1), torch.from_numpy(c["y"]).cuda().view(B, n, 1),
                         want_lam=True)
    n_eps = int(r["n_eps"].item())
    assert n_eps == len(c["eps_s"]) == len(c["lam"])
    np.testing.assert_allclose(r["eps_s"][:n_eps].cpu().numpy(), c["eps_s"].astype(np.float32), rtol=2e-7)
    np.testing.assert_allclose(r["lam"][:n_eps].cpu().numpy(), c["lam"].astype(np.float32), rtol=2e-7)
    assert abs(float(r["diameter"].item()) - float(c["diameter"])) <= 1e-7 * max(1.0, float(c["diameter"]))
    scale = max(1.0, float(np.abs(c["loss"]).max()) / 1e-4)
    _close(r["loss"].cpu().numpy(), c["loss"], "loss", LOSS_ATOL * scale)
    _close(r["duals"].cpu().numpy(), c["duals"], "duals", 2e-6 * max(1.0, np.abs(c["duals"]).max()))
    _grad_close(r["gx"].cpu().numpy(), c["grad_x"], "grad_x")


def test_gmloss_reach_matches_reference_golden():
    """gmloss.SamplesLoss(reach=...).forward(x, y, geometry): the parent's reach reaches the kernel through inheritance."""
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    c = _G.case("gmloss_b3_r1")
    B, n = c["x"].shape
    crit = SamplesLoss("sinkhorn", p=2, blur=float(c["blur"]), reach=float(c["reach"]), batchsize=B)
    x = torch.from_numpy(c["x"]).view(B, n, 1).cuda().requires_grad_(True)
    y = torch.from_numpy(c["y"]).view(B, n, 1).cuda()
    loss = crit(x, y, c["depth"])
    _close(loss.detach().cpu().numpy(), c["loss"], "loss", LOSS_ATOL)
    loss.sum().backward()
    _grad_close(x.grad.cpu().numpy().reshape(B, n), c["grad_x"], "grad_x")


@pytest.mark.parametrize("B,n,blur", SHAPES)
def test_autograd_vs_f64_restatement(B, n, blur):
    """Loss, d/dx and d/dy through autograd against autograd of the f64 damped loop, on every loop kernel, reach .1."""
    reach = .1
    x_c, y_c = _inputs(B, n)
    w = torch.rand(B, generator=torch.Generator().manual_seed(4)) + 0.5
    xo, yo = x_c.clone().requires_grad_(True), y_c.clone().requires_grad_(True)
    lo = damped_loss_f64(xo, yo, oracle.anchor_cost_matrix(n), blur, reach)
    (lo * w.double()).sum().backward()
    xg, yg = x_c.cuda().requires_grad_(True), y_c.cuda().requires_grad_(True)
    lg = _crit(n, blur, reach)(xg, yg)
    (lg * w.cuda()).sum().backward()
    scale = max(1.0, float(lo.detach().abs().max()) / 1e-4)
    _close(lg.detach().cpu().numpy(), lo.detach().numpy(), "loss", LOSS_ATOL * scale)
    _grad_close(xg.grad.cpu().numpy(), xo.grad.numpy(), "d/dx")
    _grad_close(yg.grad.cpu().numpy(), yo.grad.numpy(), "d/dy")


@pytest.mark.parametrize("B,n", [(3, 96), (3, 256), (40, 256), (2, 384), (2, 202)])
def test_weighted_four_argument_form_with_zero_weights(B, n):
    """(alpha, x, beta, y) with zero-mass anchors (log-weight -1e5) -- the case reach is for -- on every loop kernel."""
    g = torch.Generator().manual_seed(5)
    x = torch.softmax(torch.randn(B, n, generator=g), 1).view(B, n, 1)
    y = torch.softmax(torch.randn(B, n, generator=g), 1).view(B, n, 1)
    a = torch.rand(B, n, generator=g)
    a[:, ::7] = 0
    a = a / a.sum(1, keepdim=True)
    b = torch.rand(B, n, generator=g)
    b[:, 3::5] = 0
    b = b / b.sum(1, keepdim=True)
    want = damped_loss_f64(x, y, oracle.anchor_cost_matrix(n), .05, .1, a, b).numpy()
    got = _crit(n, .05, .1)(a.cuda(), x.cuda(), b.cuda(), y.cuda()).cpu().numpy()
    _close(got, want, "loss", LOSS_ATOL * max(1.0, np.abs(want).max() / 1e-4))
    bal = _crit(n, .05)(a.cuda(), x.cuda(), b.cuda(), y.cuda()).cpu().numpy()
    assert np.abs(bal - want).max() > 10 * LOSS_ATOL * max(1.0, np.abs(want).max() / 1e-4)   # the case tells them apart


def _all(r):
    n_eps = int(r["n_eps"].item())   # (eps_s past the schedule is not written)
    return ([r[k] for k in ("loss", "gx", "gy", "duals", "n_eps", "diameter")] + [r["eps_s"][:n_eps]]
            + [r["work"][:8 * r["gx"].numel()]])


@pytest.mark.parametrize("B,n", VARIANTS)
def test_balanced_outputs_are_bit_identical(B, n):
    """reach=inf and reach=None give the same bits, and the new entry point with rho <= 0 is eml_sinkhorn_fwd_ex_f32's
    launch, bit for bit (duals, expectation rows, loss, both gradients, schedule), on every loop kernel."""
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_raw
    x, y = _inputs(B, n, seed=99)
    xc, yc = x.cuda(), y.cuda()
    ref = _crit(n, .05).forward_raw(xc, yc)
    inf = _crit(n, .05, math.inf).forward_raw(xc, yc, want_lam=True)
    assert torch.equal(inf["lam"][:int(inf["n_eps"].item())], torch.ones(int(inf["n_eps"].item()), device="cuda"))
    crit = _crit(n, .05)
    M, Mt = crit.cost_matrix(xc.device)
    for r in [inf] + [sinkhorn_raw(xc.view(B, n), yc.view(B, n), None, None, M, Mt, 2, .05, .5, None, True, True, rho=rho)
                      for rho in (0.0, -1.0)]:
        for got, want in zip(_all(r), _all(ref)):
            assert torch.equal(got, want)


@pytest.mark.parametrize("B,n", [(16, 256), (3, 192), (2, 512)])
def test_split_and_tiled_kernels_agree_with_reach(B, n):
    """The split kernel exchanges the damped dual vector between its slices: forced split vs forced tiled, within the
    tolerance of the balanced split tests."""
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import EML_SINKHORN_FORCE_SPLIT, EML_SINKHORN_NO_SPLIT
    x, y = _inputs(B, n, seed=77)
    crit = _crit(n, .05, .1)
    xc, yc = x.cuda(), y.cuda()
    tiled = crit.forward_raw(xc, yc, flags=EML_SINKHORN_NO_SPLIT)
    split = crit.forward_raw(xc, yc, flags=EML_SINKHORN_FORCE_SPLIT)
    assert int(split["work"][24 * B * n:24 * B * n + 1].view(torch.int32).item()) == 0
    _close(split["loss"].cpu().numpy(), tiled["loss"].cpu().numpy(), "loss", LOSS_ATOL)
    _grad_close(split["gx"].cpu().numpy(), tiled["gx"].cpu().numpy(), "d/dx")
    bal = _crit(n, .05).forward_raw(xc, yc, flags=EML_SINKHORN_FORCE_SPLIT)
    assert not torch.allclose(bal["gx"], split["gx"], rtol=1e-2, atol=0)


def test_rescue_launch_honours_reach():
    """One give-up of the split kernel (EML_SINKHORN_TEST_STALL: a slice withholds its granules, the partners time out after
    50 ms -- no fault): the tiled rescue launch behind it must recompute the DAMPED batch, i.e. give the tiled kernel's
    own numbers for this reach, not the balanced ones."""
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import (EML_SINKHORN_FORCE_SPLIT, EML_SINKHORN_NO_SPLIT,
                                                                     EML_SINKHORN_TEST_STALL)
    B, n = 16, 256
    x, y = _inputs(B, n, seed=77)
    crit = _crit(n, .05, .1)
    xc, yc = x.cuda(), y.cuda()
    ref = crit.forward_raw(xc, yc, flags=EML_SINKHORN_NO_SPLIT)
    r = crit.forward_raw(xc, yc, flags=EML_SINKHORN_FORCE_SPLIT | EML_SINKHORN_TEST_STALL)
    torch.cuda.synchronize()
    assert int(r["work"][24 * B * n:24 * B * n + 1].view(torch.int32).item()) == 1, "the rescue did not run"
    assert torch.equal(r["loss"], ref["loss"]) and torch.equal(r["gx"], ref["gx"]) and torch.equal(r["duals"], ref["duals"])
    bal = _crit(n, .05).forward_raw(xc, yc, flags=EML_SINKHORN_NO_SPLIT)
    assert not torch.equal(r["loss"], bal["loss"])


def test_regression_trainer_with_reach_trains():
    """A short run of the regression trainer with reach .1 (train.py --reach .1) on one fixed synthetic batch: every term
    finite, the Sinkhorn term and the total going down (lr 1e-5: at 1e-4 the first Adam steps of a fresh encoder on one small
    batch overshoot before they descend).  Not a benchmark."""
    from emlight_amd.RegressionNetwork.data import synthetic_batch
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    torch.manual_seed(0)
    tr = RegressionTrainer(anchors=96, crop_hw=(192, 256), blur=.025, reach=.1, lr=1e-5, device="cuda")
    assert tr.sam_loss.reach == .1 and tr.sam_loss.rho == pytest.approx(.01)
    batch = synthetic_batch(8, 96, (192, 256), seed=1234, device="cuda")
    total, em = [], []
    for _ in range(20):
        loss, terms = tr.step(batch)
        total.append(float(loss))
        em.append(float(terms["dist_emloss"]))
    assert all(math.isfinite(v) for v in total + em)
    for h in (total, em):
        assert np.mean(h[-5:]) < 0.5 * np.mean(h[:5]) and h[-1] < 0.5 * h[0], h
