"""GPU: per-sample scene geometry in the Sinkhorn kernels -- the batched cost builder (``eml_gm_anchor_cost_f32``), the cost
stride of every loop kernel (``eml_sinkhorn_fwd_cost_f32``), ``gmloss.SamplesLoss`` on a ``(B, N)`` geometry and the trainer.

At EMLight's operating point (blur .05, values ~ 1/N) the chords are far larger than eps = blur^2, the transport plan is the
identity and neither the loss nor the gradient depends on the matrix: a kernel that read sample 0's matrix for every sample
would pass there.  Every value test below therefore runs where the matrix matters -- blur .5, p 2, scaling .5, samples
30 * softmax, depths U(.05, 3) drawn per sample, the diameter taken over the whole batch -- and first asserts, on the
oracle, that reading the NEXT sample's matrix moves every sample's gradient and duals by at least 100 times the tolerance
the test then uses (``_regime``).

Shapes (B = 3): N = 5, 128 the register-resident kernel; 132, 260 the tiled kernel with two lanes and one lane per row;
192, 256 the split kernel (EML_SINKHORN_FORCE_SPLIT); 130, 516 the streaming kernel; D = 3 at N = 128, 132, 130."""
import functools

import numpy as np
import pytest
import torch

import oracle
from tests.golden.make_golden_gmloss_batched import SEED, batch_diameter, batched_inputs

pytestmark = pytest.mark.gpu

LOSS_ATOL = 1e-6      # the bounds of test_gpu_sinkhorn.py
GRAD_RTOL = 1e-4
DUAL_RTOL = 2e-6
B = 3
BLUR, P, SCALING = .5, 2, .5
NO_SPLIT, FORCE_SPLIT = 1, 2

# (N, D, flags): every kernel path
PATHS = [(5, 1, 0), (128, 1, 0), (132, 1, NO_SPLIT), (260, 1, NO_SPLIT), (192, 1, FORCE_SPLIT), (256, 1, FORCE_SPLIT),
         (130, 1, 0), (516, 1, 0), (128, 3, 0), (132, 3, 0), (130, 3, 0)]
PATH_IDS = ["N%d_D%d" % (n, d) for n, d, _ in PATHS]
# The inputs' seed per N.  N = 5 with the common seed misses the precondition of ``_regime`` on the oracle (sample 2's
# gradient moves by 13 x the tolerance under the neighbour's matrix, 100 x is asked): its samples and depths are another
# draw of the same distributions, seed 26 (2755 x).  The factor of 100 and the tolerances are unchanged.
SEEDS = {5: 26}


# ------------------------------------------------------------------------------------------------ inputs and the oracle
@functools.lru_cache(maxsize=None)
def _inputs(n, D):
    """x, y (B, n, D) f32, depth (B, n) f64, the oracle's matrices (B, n, n) f32 and the batch's diameter."""
    x, y, depth = batched_inputs(B, n, SEEDS.get(n, SEED), D)
    M = torch.stack([oracle.cost_matrix_of(oracle.geometric_points(n, depth[b])) for b in range(B)])
    return (torch.from_numpy(x).view(B, n, D), torch.from_numpy(y).view(B, n, D), torch.from_numpy(depth), M,
            batch_diameter(x, y))


def _oracle_batch(x, y, M, diameter):
    """``oracle.samples_loss`` per sample with its own matrix: loss (B,), d/dx, d/dy (B, n, D), duals (4, B, n)."""
    loss, gx, gy, duals = [], [], [], []
    for b in range(x.shape[0]):
        xb, yb = x[b:b + 1].clone().requires_grad_(True), y[b:b + 1].clone().requires_grad_(True)
        lb, aux = oracle.samples_loss(xb, yb, M[b], blur=BLUR, scaling=SCALING, p=P, diameter=diameter, return_aux=True)
        lb.sum().backward()
        loss.append(lb.detach()[0])
        gx.append(xb.grad[0])
        gy.append(yb.grad[0])
        duals.append(torch.stack([d.detach()[0] for d in aux["duals"]]))
    return {"loss": torch.stack(loss).numpy(), "gx": torch.stack(gx).numpy(), "gy": torch.stack(gy).numpy(),
            "duals": torch.stack(duals, 1).numpy()}


@functools.lru_cache(maxsize=None)
def _regime(n, D):
    """The oracle's outputs for the batch, computed once per shape, behind the precondition: with the next sample's matrix
    every sample's gradient and duals move by >= 100 x the tolerance the value tests use."""
    x, y, _, M, diameter = _inputs(n, D)
    want = _oracle_batch(x, y, M, diameter)
    wrong = _oracle_batch(x, y, torch.roll(M, -1, 0), diameter)
    dual_tol = DUAL_RTOL * max(1.0, float(np.abs(want["duals"]).max()))
    for b in range(B):
        g_tol = GRAD_RTOL * float(np.abs(want["gx"][b]).max())
        g_move = float(np.abs(wrong["gx"][b] - want["gx"][b]).max())
        d_move = float(np.abs(wrong["duals"][:, b] - want["duals"][:, b]).max())
        print("regime N=%d D=%d sample %d: gradient moves %.3e (tolerance %.3e), duals move %.3e (tolerance %.3e)"
              % (n, D, b, g_move, g_tol, d_move, dual_tol))
        assert g_move >= 100 * g_tol, "N=%d D=%d sample %d: the neighbour's matrix moves the gradient by only %.3e" % (n, D, b, g_move)
        assert d_move >= 100 * dual_tol, "N=%d D=%d sample %d: the neighbour's matrix moves the duals by only %.3e" % (n, D, b, d_move)
    return want


def _dev(n, D):
    """The batch on the device: x, y as the kernels read them ((B, n) for D = 1), depth, the oracle's matrices."""
    x, y, depth, M, diameter = _inputs(n, D)
    if D == 1:
        x, y = x.view(B, n), y.view(B, n)
    return x.cuda().contiguous(), y.cuda().contiguous(), depth.cuda(), M.cuda().contiguous(), diameter


def _raw(x, y, M, diameter=None, flags=0, alpha=None, beta=None, rho=None):
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_raw
    Mt = M.transpose(-1, -2).contiguous()
    r = sinkhorn_raw(x, y, alpha, beta, M, Mt, P, BLUR, SCALING, diameter, True, True, flags=flags, rho=rho, want_lam=True)
    torch.cuda.synchronize()
    return r


OUTPUTS = ("loss", "gx", "gy", "duals", "eps_s", "n_eps", "diameter", "lam")


def _assert_same_bits(got, want, what, rows=slice(None)):
    for k in OUTPUTS:
        g, w = got[k], want[k]
        if k in ("loss", "gx", "gy"):
            w = w[rows]
        elif k == "duals":
            w = w[:, rows]
        elif k in ("eps_s", "lam"):   # the entries past n_eps are never written
            n = int(want["n_eps"].item())
            g, w = g[:n], w[:n]
        assert torch.equal(g, w), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------------ 1. the builder
@pytest.mark.parametrize("n", [5, 128, 516])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_builder_matches_the_oracle(n, f64):
    from emlight_amd import _lib
    depth = _inputs(n, 1)[2]
    depth = depth if f64 else depth.float()
    d = depth.cuda().contiguous()
    a = torch.full((B, n, 3), float("nan"), device="cuda")
    M = torch.full((B, n, n), float("nan"), device="cuda")
    _lib.check(_lib.lib().eml_gm_anchor_cost_f32(_lib.ptr(d), int(f64), B, n, _lib.ptr(a), _lib.ptr(M),
                                                 _lib.current_stream()), "eml_gm_anchor_cost_f32")
    M2 = torch.full((B, n, n), float("nan"), device="cuda")   # anchors_out = NULL: the same matrices
    _lib.check(_lib.lib().eml_gm_anchor_cost_f32(_lib.ptr(d), int(f64), B, n, None, _lib.ptr(M2),
                                                 _lib.current_stream()), "eml_gm_anchor_cost_f32")
    a, M, M2 = a.cpu(), M.cpu(), M2.cpu()
    assert torch.equal(M, M2)
    for b in range(B):
        pts = oracle.geometric_points(n, depth[b].double().numpy())   # an f32 depth is promoted exactly
        ulp = float(np.spacing(np.float32(np.abs(pts).max())))
        np.testing.assert_allclose(a[b].numpy(), pts.astype(np.float32), rtol=0, atol=ulp)
        np.testing.assert_allclose(M[b].numpy(), oracle.cost_matrix_of(pts).numpy(), rtol=0, atol=2e-6)
        assert torch.equal(M[b].diagonal(), torch.zeros(n)) and not bool(torch.signbit(M[b].diagonal()).any())
        assert torch.equal(M[b], M[b].t())   # bit for bit


# ------------------------------------------------------------------------------------------------ 2. stride 0 = the old entry
def _entry(name, x, y, M, Mt, alpha=None, beta=None, diameter=-1.0, D=1, flags=0, rho=0.0, stride=None):
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import sinkhorn_outputs
    n = x.shape[1]
    o = sinkhorn_outputs(B, n, x.device, True, True, D=D)
    o["eps_s"].zero_()
    lam = torch.zeros(64, device=x.device)
    p = _lib.ptr
    args = [p(x), p(y), p(M), p(Mt), p(alpha), p(beta), BLUR, SCALING, P, diameter, None, p(o["eps_s"]), p(o["n_eps"]),
            p(o["diameter"]), p(o["loss"]), p(o["gx"]), p(o["gy"]), p(o["work"]), B, n, D, flags, rho, p(lam)]
    if stride is not None:
        args.append(stride)
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream()), name)
    torch.cuda.synchronize()
    return {"loss": o["loss"], "gx": o["gx"], "gy": o["gy"], "duals": o["work"][:4 * B * n].view(4, B, n),
            "eps_s": o["eps_s"], "n_eps": o["n_eps"], "diameter": o["diameter"], "lam": lam}


@pytest.mark.parametrize("n,D,flags", PATHS, ids=PATH_IDS)
def test_stride_zero_is_the_old_entry(n, D, flags):
    x, y, _, M, _ = _dev(n, D)
    M0, Mt0 = M[0].contiguous(), M[0].t().contiguous()
    old = _entry("eml_sinkhorn_fwd_dim_f32", x, y, M0, Mt0, D=D, flags=flags)
    new = _entry("eml_sinkhorn_fwd_cost_f32", x, y, M0, Mt0, D=D, flags=flags, stride=0)
    assert bool(torch.isfinite(old["loss"]).all()) and int(old["n_eps"].item()) > 2
    _assert_same_bits(new, old, "stride 0, N=%d D=%d" % (n, D))


@pytest.mark.parametrize("kind", ["reach", "weights"])
def test_stride_zero_is_the_old_entry_with_reach_and_with_weights(kind):
    n = 128
    x, y, _, M, _ = _dev(n, 1)
    g = torch.Generator().manual_seed(3)
    kw = {"rho": 2.0 ** P} if kind == "reach" else \
        {"alpha": torch.softmax(torch.randn(B, n, generator=g), 1).cuda(), "beta": torch.softmax(torch.randn(B, n, generator=g), 1).cuda()}
    M0 = M[0].contiguous()
    old = _entry("eml_sinkhorn_fwd_dim_f32", x, y, M0, M0, **kw)
    new = _entry("eml_sinkhorn_fwd_cost_f32", x, y, M0, M0, stride=0, **kw)
    plain = _entry("eml_sinkhorn_fwd_dim_f32", x, y, M0, M0)
    assert not torch.equal(old["loss"], plain["loss"])   # the reach / the weights took effect
    _assert_same_bits(new, old, "stride 0 with " + kind)


# ------------------------------------------------------------------------------------------------ 3. B copies = the shared matrix
@pytest.mark.parametrize("n,D,flags", PATHS, ids=PATH_IDS)
def test_copies_of_one_matrix_equal_the_shared_matrix(n, D, flags):
    """Only the address differs between the two calls: no tolerance."""
    x, y, _, M, _ = _dev(n, D)
    M1 = M[1].contiguous()
    shared = _raw(x, y, M1, flags=flags)
    copies = _raw(x, y, M1.unsqueeze(0).repeat(B, 1, 1).contiguous(), flags=flags)
    assert bool(torch.isfinite(shared["loss"]).all())
    _assert_same_bits(copies, shared, "B copies, N=%d D=%d" % (n, D))


# ------------------------------------------------------------------------------------------------ 4. distinct matrices = single-sample calls
@pytest.mark.parametrize("n,D,flags", PATHS, ids=PATH_IDS)
def test_distinct_matrices_equal_single_sample_calls(n, D, flags):
    """At a fixed diameter a sample's numbers do not depend on its batch (checked first, with a shared matrix: the parent
    commit's code path); then sample b of the per-sample call is the B = 1 call on sample b with matrix b, bit for bit."""
    x, y, _, M, diameter = _dev(n, D)
    M1 = M[1].contiguous()
    shared = _raw(x, y, M1, diameter=diameter, flags=flags)
    batched = _raw(x, y, M, diameter=diameter, flags=flags)
    assert not torch.equal(batched["gx"], shared["gx"])
    for b in range(B):
        xb, yb = x[b:b + 1].clone(), y[b:b + 1].clone()
        _assert_same_bits(_raw(xb, yb, M1, diameter=diameter, flags=flags), shared, "batch invariance, N=%d sample %d" % (n, b),
                          rows=slice(b, b + 1))
        one = _raw(xb, yb, M[b].contiguous(), diameter=diameter, flags=flags)
        _assert_same_bits(one, batched, "N=%d D=%d sample %d" % (n, D, b), rows=slice(b, b + 1))
        _assert_same_bits(_raw(xb, yb, M[b:b + 1].clone(), diameter=diameter, flags=flags), one, "one-sample stack, N=%d" % n)


# ------------------------------------------------------------------------------------------------ 5. value against the oracle
def _check_values(got_loss, got_gx, got_gy, got_duals, want, what):
    scale = max(1.0, float(np.abs(want["loss"]).max()) / 1e-4)
    dual_tol = DUAL_RTOL * max(1.0, float(np.abs(want["duals"]).max()))
    print("%s: loss err %.3e (bound %.3e)" % (what, np.abs(got_loss - want["loss"]).max(), LOSS_ATOL * scale))
    for name, got, ref in (("gx", got_gx, want["gx"]), ("gy", got_gy, want["gy"])):
        if got is not None:
            print("%s: %s err %.3e (bound %.3e of max %.3e)" % (what, name, np.abs(got - ref).max(), GRAD_RTOL * np.abs(ref).max(),
                                                                np.abs(ref).max()))
    if got_duals is not None:
        print("%s: duals err %.3e (bound %.3e)" % (what, np.abs(got_duals - want["duals"]).max(), dual_tol))
    np.testing.assert_allclose(got_loss, want["loss"], rtol=0, atol=LOSS_ATOL * scale)
    for got, ref in ((got_gx, want["gx"]), (got_gy, want["gy"])):
        if got is not None:
            np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_RTOL * np.abs(ref).max())
    if got_duals is not None:
        np.testing.assert_allclose(got_duals, want["duals"], rtol=0, atol=dual_tol)


@pytest.mark.parametrize("n,D,flags", PATHS, ids=PATH_IDS)
def test_per_sample_cost_matches_the_oracle(n, D, flags):
    want = _regime(n, D)
    x, y, _, M, diameter = _dev(n, D)
    r = _raw(x, y, M, flags=flags)   # the diameter from the data, over the whole batch
    assert abs(float(r["diameter"].item()) - diameter) <= 1e-6 * diameter
    _check_values(r["loss"].cpu().numpy(), r["gx"].cpu().numpy().reshape(B, n, D), r["gy"].cpu().numpy().reshape(B, n, D),
                  r["duals"].cpu().numpy(), want, "oracle N=%d D=%d" % (n, D))


# ------------------------------------------------------------------------------------------------ 6. value against the reference
def test_per_sample_geometry_matches_the_reference_golden():
    """``gmloss.SamplesLoss`` of the REAL reference, run once per sample with that sample's depth and the batch's diameter
    (tests/golden/make_golden_gmloss_batched.py), against one call on the batch."""
    from tests.conftest import Golden
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    g = Golden("gmloss_batched")
    n = 128
    x_np, y_np, depth = batched_inputs(B, n, SEED)
    x = torch.from_numpy(x_np).view(B, n, 1).cuda().requires_grad_(True)
    y = torch.from_numpy(y_np).view(B, n, 1).cuda()
    crit = SamplesLoss("sinkhorn", p=2, blur=float(g["blur"]), diameter=float(g["diameter"]), batchsize=B)
    loss = crit(x, y, torch.from_numpy(depth).cuda())
    np.testing.assert_allclose(crit.anchors.cpu().numpy(), g["anchors"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(crit.M[:, ::8].cpu().numpy(), g["M_rows8"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), g["loss"], rtol=0, atol=1e-6)
    loss.sum().backward()
    np.testing.assert_allclose(x.grad.cpu().numpy().reshape(B, n), g["grad_x"], rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 7. the module
def test_module_on_a_batched_geometry_with_autograd_and_no_host_sync():
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    n = 128
    want = _regime(n, 1)
    x, y, depth, _, _ = _inputs(n, 1)
    xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    dg = depth.cuda()
    crit = SamplesLoss("sinkhorn", p=2, blur=BLUR, scaling=SCALING)
    w = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    loss = crit(xg, yg, dg)
    (loss * w).sum().backward()   # the warm-up call
    assert crit.M.shape == (B, n, n) and crit.anchors.shape == (B, n, 3)
    _check_values(loss.detach().cpu().numpy(), xg.grad.cpu().numpy(), yg.grad.cpu().numpy(), None, want, "module")
    with pytest.raises(ValueError):
        crit(xg, yg, dg[:2])
    cpu_loss = crit(xg, yg, depth.float())   # a CPU tensor: moved to the device
    assert crit.M.is_cuda and torch.isfinite(cpu_loss).all()
    xg.grad = yg.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = crit(xg, yg, dg)
        (again * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(again.detach(), loss.detach())


# ------------------------------------------------------------------------------------------------ 8. the trainer
def test_trainer_with_geometry():
    from emlight_amd.RegressionNetwork.data import synthetic_batch
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    batch = synthetic_batch(2, anchors=8, crop_hw=(32, 32), with_depth=True, device="cuda")
    torch.manual_seed(0)
    tr = RegressionTrainer(anchors=8, crop_hw=(32, 32), geometry=True)
    assert isinstance(tr.sam_loss, SamplesLoss)
    for _ in range(2):
        loss, terms = tr.step(batch)
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in terms.values())
    M = tr.sam_loss.M.cpu()
    assert M.shape == (2, 8, 8)
    for b in range(2):
        want = oracle.cost_matrix_of(oracle.geometric_points(8, batch["depth"][b].double().cpu().numpy()))
        np.testing.assert_allclose(M[b].numpy(), want.numpy(), rtol=0, atol=2e-6)
    no_depth = {k: v for k, v in batch.items() if k != "depth"}
    with pytest.raises(ValueError, match="depth"):
        tr.step(no_depth)
    plain = RegressionTrainer(anchors=8, crop_hw=(32, 32), geometry=False)
    loss, _ = plain.step(batch)   # the same batch, depth ignored
    assert bool(torch.isfinite(loss)) and not isinstance(plain.sam_loss, SamplesLoss)
