"""GPU: SphereMaxPool2D (csrc/sphere_pool.hip) against the reference's CPU outputs (``tests/golden/sphere_pool.npz``), the
float64 restatement of ``tests/sphere_pool_oracle.py`` and the stock ops on the same device.

Tolerances are derived, not tuned (u = 2^-24):
* forward: a tap value is at most 4 products and 3 additions of weights that sum to 1 -> ``|y - want| <= 16 u max|x|``
  (7 roundings on each side, rounded up);
* backward, for a FIXED routing: the kernel and the oracle differ in summation order and product rounding only ->
  ``|gx[q] - want[q]| <= 2 M u S[q] + 1e-30`` with M the longest CSR row and S[q] = sum |w * gy| of the routed terms.
Two routings are compared only outside the near-tie window (top-two tap gap in (1e-12, 1e-5 max|x|)), whose cells the test
counts and holds to the generator's cap of 0.5 %."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as stock
from tests import sphere_pool_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "sphere_pool.npz"))


@functools.lru_cache(None)
def _table(H, W, stride):
    idx, wgt = oracle.tap_table(H, W, stride)
    return idx, wgt, oracle.longest_row(idx, H * W)


def _flat(t):
    return t.detach().cpu().reshape(t.shape[0], t.shape[1], -1)


def _run(x, gy, stride):
    """The operator on the device: (y, arg, gx) on the CPU, flattened to (B, C, pixels)."""
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    xg = x.cuda().requires_grad_(True)
    y, arg = sphere_max_pool(xg, stride, return_indices=True)
    assert y.is_contiguous(memory_format=torch.channels_last) and arg.dtype == torch.uint8 and not arg.requires_grad
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return _flat(y).double(), _flat(arg).long(), _flat(xg.grad).double()


@functools.lru_cache(None)
def _golden_run(case):
    """One device run per golden case, shared by the four tests that read it (nothing below modifies it)."""
    z, name = _golden(), oracle.case_name(case)
    x, gy = torch.from_numpy(z[name + "/x"]), torch.from_numpy(z[name + "/gy"])
    H, W, stride, B, C = case
    idx, wgt, M = _table(H, W, stride)
    y, arg, gx = _run(x, gy, stride)
    return dict(x=x, gy=gy, y=y, arg=arg, gx=gx, vals=oracle.tap_values(x, idx, wgt), xmax=float(x.abs().max()),
                ref_y=_flat(torch.from_numpy(z[name + "/y"])).double(), ref_gx=_flat(torch.from_numpy(z[name + "/gx"])).double(),
                ref_arg=_flat(torch.from_numpy(z[name + "/arg"])).long())


def _check_forward(y, want, xmax, what):
    err = float((y - want).abs().max())
    print("%s: forward error %.3e, bound %.3e" % (what, err, oracle.forward_bound(xmax)))
    assert err <= oracle.forward_bound(xmax), what


def _check_indices(arg, vals, xmax, what):
    """The float64 value of the chosen tap is within the forward bound of the float64 maximum: no exclusions, pole ties may
    fall either way."""
    assert int(arg.min()) >= 0 and int(arg.max()) <= 8, what
    chosen = vals.gather(3, arg.unsqueeze(-1)).squeeze(-1)
    short = float((vals.max(-1).values - chosen).max())
    print("%s: chosen tap short of the maximum by %.3e, bound %.3e" % (what, short, oracle.forward_bound(xmax)))
    assert short <= oracle.forward_bound(xmax), what


def _check_grad(gx, want, M, S, what, skip=None):
    ratio = (gx - want).abs() / oracle.grad_bound(M, S)
    if skip is not None:
        ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
    print("%s: gradient at %.3f of its bound (M = %d)" % (what, float(ratio.max()), M))
    assert float(ratio.max()) <= 1.0, what


# ------------------------------------------------------------------------------------------------ the reference's cases
@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.case_name)
def test_forward_against_the_reference(case):
    r = _golden_run(case)
    _check_forward(r["y"], r["ref_y"], r["xmax"], oracle.case_name(case))


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.case_name)
def test_indices_are_legitimate(case):
    r = _golden_run(case)
    _check_indices(r["arg"], r["vals"], r["xmax"], oracle.case_name(case))


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.case_name)
def test_backward_for_the_kernels_own_routing(case):
    H, W, stride, B, C = case
    r = _golden_run(case)
    idx, wgt, M = _table(H, W, stride)
    want, S = oracle.routed_grad(_flat(r["gy"]), r["arg"], idx, wgt, H * W)
    _check_grad(r["gx"], want, M, S, oracle.case_name(case))


@pytest.mark.parametrize("case", oracle.CASES, ids=oracle.case_name)
def test_backward_against_the_reference(case):
    """The reference's gradient under the reference's routing.  Skipped: only input pixels fed by a cell in the near-tie window,
    and those cells are within the cap."""
    H, W, stride, B, C = case
    r = _golden_run(case)
    idx, wgt, M = _table(H, W, stride)
    _, S = oracle.routed_grad(_flat(r["gy"]), r["ref_arg"], idx, wgt, H * W)
    window = oracle.near_tie_cells(r["vals"], r["xmax"])
    share = float(window.double().mean())
    differ = int((r["arg"] != r["ref_arg"]).sum())
    print("%s: %d of %d cells in the near-tie window, %d routings differ from the reference's"
          % (oracle.case_name(case), int(window.sum()), window.numel(), differ))
    assert share <= oracle.NEAR_TIE_CAP
    _check_grad(r["gx"], r["ref_gx"], M, S, oracle.case_name(case), skip=oracle.fed_pixels(window, idx, H * W))


# ------------------------------------------------------------------------------------------------ shapes
GEOMETRIES = [(8, 16, 1), (8, 16, 2), (5, 12, 2), (10, 20, 3)]
CHANNELS = [1, 3, 5, 8, 68, 260]     # scalar path with several pixels per wave; vector path; 17 vector lanes; a second trip
SHAPES = [(H, W, s, 1 + 2 * ((i + j) % 2), C) for i, (H, W, s) in enumerate(GEOMETRIES) for j, C in enumerate(CHANNELS)]


def test_shape_list_covers_every_value_with_every_stride():
    for s in (1, 2, 3):
        assert {C for (_, _, st, _, C) in SHAPES if st == s} == set(CHANNELS)
        assert {B for (_, _, st, B, _) in SHAPES if st == s} == {1, 3}


@pytest.mark.parametrize("shape", SHAPES, ids=oracle.case_name)
def test_shapes_against_the_oracle(shape):
    H, W, stride, B, C = shape
    ho, wo = oracle.out_size(H, W, stride)
    g = torch.Generator().manual_seed(1000 * H + 10 * C + B)
    x, gy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, ho, wo, generator=g)
    idx, wgt, M = _table(H, W, stride)
    y, arg, gx = _run(x, gy, stride)
    assert y.shape == (B, C, ho * wo) and gx.shape == (B, C, H * W)
    vals, xmax, what = oracle.tap_values(x, idx, wgt), float(x.abs().max()), oracle.case_name(shape)
    _check_forward(y, vals.max(-1).values, xmax, what)
    _check_indices(arg, vals, xmax, what)
    want, S = oracle.routed_grad(_flat(gy), arg, idx, wgt, H * W)
    _check_grad(gx, want, M, S, what)


def test_device_table_is_the_oracles():
    """The geometry the pool shares with SphereConv2D holds the table the oracle builds on the CPU, bit for bit."""
    from emlight_amd.GenProjector.spherenet import sphere_geometry
    for H, W, stride in GEOMETRIES + [(9, 18, 3), (6, 12, 1), (16, 32, 2)]:
        geo = sphere_geometry(H, W, stride, torch.device("cuda", torch.cuda.current_device()), "sphere")
        idx, wgt, M = _table(H, W, stride)
        assert (geo.ho, geo.wo) == oracle.out_size(H, W, stride)
        assert torch.equal(geo.idx.cpu().long(), idx), (H, W, stride)
        differ = int((geo.wgt.cpu() != wgt).sum())
        print("%dx%d stride %d: %d of %d weights differ" % (H, W, stride, differ, wgt.numel()))
        assert differ == 0, (H, W, stride)
        assert int((geo.csr_ptr[1:] - geo.csr_ptr[:-1]).max()) == M


# ------------------------------------------------------------------------------------------------ properties
def test_layouts_give_the_same_bits():
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    torch.manual_seed(3)
    x = torch.randn(2, 12, 8, 16, device="cuda")
    gy = torch.randn(2, 12, 4, 8, device="cuda")
    outs = []
    for xi in (x.contiguous(), x.contiguous(memory_format=torch.channels_last), x.transpose(2, 3).contiguous().transpose(2, 3)):
        xi = xi.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y, arg = sphere_max_pool(xi, 2, return_indices=True)
        assert y.is_contiguous(memory_format=torch.channels_last) and arg.is_contiguous(memory_format=torch.channels_last)
        y.backward(gy)
        outs.append((y.detach(), arg, xi.grad))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    # a contiguous view that starts inside a storage (16-byte accesses need their own start)
    big = torch.randn(2 * 12 * 8 * 16 + 1, device="cuda")
    big[1:] = x.permute(0, 2, 3, 1).reshape(-1)
    view = big[1:].view(2, 8, 16, 12).permute(0, 3, 1, 2)
    assert view.data_ptr() % 16 and view.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(sphere_max_pool(view, 2), outs[0][0])


def test_every_gradient_element_is_written():
    """Stride 3: input pixels that no tap samples (an empty CSR row) and pixels whose cells all chose other taps get exactly 0,
    whatever the allocation held before."""
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    H, W, stride, B, C = 10, 20, 3, 2, 8
    idx, wgt, M = _table(H, W, stride)
    torch.manual_seed(5)
    x = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y, arg = sphere_max_pool(x, stride, return_indices=True)
    gy = torch.randn_like(y)
    poison = torch.full((B, H, W, C), float("nan"), device="cuda")      # the block the gradient is likely to be carved from
    del poison
    (gx,) = torch.autograd.grad(y, x, gy)
    _, S = oracle.routed_grad(_flat(gy), _flat(arg).long(), idx, wgt, H * W)
    gx = _flat(gx)
    empty = torch.bincount(idx[idx >= 0], minlength=H * W) == 0
    print("empty CSR rows: %.0f %% of the input; no routed term: %.0f %%" % (100 * float(empty.double().mean()),
                                                                            100 * float((S == 0).double().mean())))
    assert int(empty.sum()) > 0 and float((S == 0).double().mean()) > 0.5
    assert bool(torch.isfinite(gx).all())
    assert bool((gx[:, :, empty] == 0).all()) and bool((gx[S == 0] == 0).all())
    assert bool((gx[S > 0] != 0).any())


def test_backward_is_deterministic():
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    torch.manual_seed(6)
    x = torch.randn(3, 20, 16, 32, device="cuda", requires_grad=True)
    y = sphere_max_pool(x, 1)
    gy = torch.randn_like(y)
    a, = torch.autograd.grad(y, x, gy, retain_graph=True)
    b, = torch.autograd.grad(y, x, gy)
    assert torch.equal(a, b)
    assert torch.equal(sphere_max_pool(x.detach(), 1), y.detach())


def test_element_offsets_past_2_to_the_31():
    """B * pixels * C = 1025 * 8192 * 256 > 2^31 on both sides (stride 1): every sample of a batch of copies gives the bits the
    one sample gives alone -- output, indices and gradient, first, middle and last sample."""
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    B, C, H, W = 1025, 256, 64, 128
    assert B * C * H * W > 2 ** 31
    torch.manual_seed(11)
    xs = torch.randn(1, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    gys = torch.randn(1, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    x1 = xs.clone().requires_grad_(True)
    y1, a1 = sphere_max_pool(x1, 1, return_indices=True)
    (g1,) = torch.autograd.grad(y1, x1, gys)
    x = xs.expand(B, C, H, W).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y, a = sphere_max_pool(x, 1, return_indices=True)
    (g,) = torch.autograd.grad(y, x, gys.expand(B, C, H, W))
    assert y.numel() > 2 ** 31 and g.numel() > 2 ** 31
    for b in (0, B // 2, B - 1):
        assert torch.equal(y[b], y1[0].detach()) and torch.equal(a[b], a1[0]) and torch.equal(g[b], g1[0]), b


def _stock_pool(x, stride):
    from emlight_amd.GenProjector.spherenet import sphere_sampling_grid
    grid = sphere_sampling_grid(x.shape[2], x.shape[3], stride).to(x.device).expand(x.shape[0], -1, -1, -1)
    return F.max_pool2d(F.grid_sample(x, grid, mode="bilinear", align_corners=False), 3, 3)


@pytest.mark.parametrize("C", [3, 8])
def test_nan_propagates_like_the_stock_ops(C):
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    torch.manual_seed(7)
    x = torch.randn(2, C, 8, 16, device="cuda")
    clean = sphere_max_pool(x, 1)
    x[1, C - 1, 3, 5] = float("nan")
    y, want = sphere_max_pool(x, 1), _stock_pool(x, 1)
    mask = torch.isnan(y)
    assert torch.equal(mask, torch.isnan(want)) and 0 < int(mask.sum()) < 8 * 16
    assert not bool(mask[0].any()) and not bool(mask[1, :C - 1].any())
    assert torch.equal(y[~mask], clean[~mask])


def test_against_the_stock_ops_on_the_same_device():
    from emlight_amd.GenProjector.spherenet import sphere_max_pool
    torch.manual_seed(8)
    x = torch.randn(2, 8, 16, 32, device="cuda")
    y, want = sphere_max_pool(x, 1), _stock_pool(x, 1)
    assert y.shape == want.shape == (2, 8, 16, 32)
    _check_forward(y.double().cpu(), want.double().cpu(), float(x.abs().max()), "2x8x16x32 stride 1 vs grid_sample + max_pool2d")


def test_conv_pool_conv_against_the_stock_chain():
    """SphereConv2D(4, 8) -> SphereMaxPool2D(2) -> SphereConv2D(8, 4) on 16x32: output and every gradient against the same chain
    in stock ops on the device, in relative L2 per tensor at the bound of the small SphereConv chains,
    tests/test_gpu_projector.py:888 (``err < 2e-3``).  Nothing in between changes layout."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D, SphereMaxPool2D
    torch.manual_seed(9)
    c1, pool, c2 = SphereConv2D(4, 8).cuda(), SphereMaxPool2D(2).cuda(), SphereConv2D(8, 4).cuda()
    with torch.no_grad():
        c1.bias.uniform_(-0.5, 0.5)
        c2.bias.uniform_(-0.5, 0.5)
    params = [c1.weight, c1.bias, c2.weight, c2.bias]
    x = torch.randn(2, 4, 16, 32, device="cuda")
    gy = torch.randn(2, 4, 8, 16, device="cuda")
    results = []
    for kind in ("hip", "stock"):
        xi = x.clone().requires_grad_(True)
        if kind == "hip":
            h1 = c1(xi)
            h2 = pool(h1)
            y = c2(h2)
            for t in (h1, h2, y):
                assert t.is_contiguous(memory_format=torch.channels_last)
            assert h2.shape == (2, 8, 8, 16)
            # the pool reads the convolution's rows where they are, and the second convolution the pool's
            assert h1.permute(0, 2, 3, 1).is_contiguous() and h2.permute(0, 2, 3, 1).is_contiguous()
        else:
            h1 = stock.sphere_conv(xi, c1.weight, c1.bias, 1)
            y = stock.sphere_conv(_stock_pool(h1, 2), c2.weight, c2.bias, 1)
        grads = torch.autograd.grad(y, [xi] + params, gy)
        results.append([y.detach()] + [g.detach() for g in grads])
    for name, a, b in zip(("y", "dx", "dW1", "db1", "dW2", "db2"), *results):
        err = float((a - b).double().norm() / b.double().norm().clamp_min(1e-20))
        print("%s: relative L2 %.2e" % (name, err))
        assert err < 2e-3, (name, err)
