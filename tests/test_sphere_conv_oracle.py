"""CPU: the float64 SphereConv restatement of ``tests/sphere_conv_oracle.py`` against the stock ops.

The helper is what the GPU request matrix (``tests/test_gpu_sphere_conv_requests.py``) holds the HIP kernels to, so its own tap
order (t = a*3 + b, rows p*9 + t) and weight layout ((O, tap, c) columns) are guarded here against ``oracle.sphere_conv``
(grid_sample + conv2d(stride 3), float32, CPU): output, d/dx, d/dweight, d/dbias, with the project's bound for this comparison
(``test_sphere_conv_ngf64_layer_shapes_natural_dispatch``: rtol 1e-4, atol 1e-4 of the reference's largest entry)."""
import numpy as np
import pytest
import torch

import oracle as stock
from tests import sphere_conv_oracle as oracle

# (B, Cin, Cout, H, W, stride, residual, slope): an odd channel count on each side, a non-power-of-two grid with stride 3, an
# odd height with stride 2; the residual + LeakyReLU epilogue on the first shape
CASES = [(2, 5, 7, 8, 16, 1, False, 1.0), (1, 3, 4, 9, 18, 3, False, 1.0), (2, 6, 4, 5, 12, 2, False, 1.0),
         (2, 5, 7, 8, 16, 1, True, 0.2)]


def _inputs(B, Cin, Cout, H, W, stride, with_res, seed):
    g = torch.Generator().manual_seed(seed)
    ho, wo = -(-H // stride), -(-W // stride)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    b = torch.rand(Cout, generator=g) - 0.5
    r = torch.randn(B, Cout, ho, wo, generator=g) if with_res else None
    gy = torch.randn(B, Cout, ho, wo, generator=g)
    return x, w, b, r, gy


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride,with_res,slope", CASES)
def test_float64_restatement_vs_stock_ops(B, Cin, Cout, H, W, stride, with_res, slope):
    x, w, b, r, gy = _inputs(B, Cin, Cout, H, W, stride, with_res, seed=Cin * 100 + H)
    ins = [t.clone().requires_grad_(True) for t in (x, w, b)] + ([r.clone().requires_grad_(True)] if with_res else [])
    yr = stock.sphere_conv(ins[0], ins[1], ins[2], stride, ins[3] if with_res else None, slope)
    gr = torch.autograd.grad(yr, ins, gy)
    want = dict(zip(("x", "weight", "bias", "residual"), gr), y=yr.detach())
    got = oracle.grads("sphere", x, w, b, stride, r, slope, gy)
    # for the stock output's OWN mask: an output within rounding of zero may take the other branch in float32
    masked = oracle.grads_masked("sphere", x, w, b, stride, r, slope, gy, yr.detach())
    assert got["y"].dtype == torch.float64 and got["y"].shape == yr.shape == (B, Cout, -(-H // stride), -(-W // stride))
    np.testing.assert_array_equal(oracle.conv("sphere", x, w, b, stride, r, slope).numpy(), got["y"].numpy())
    flipped = (got["y"] > 0) != (yr.detach() > 0)
    print("mask: %d of %d outputs on the other side of zero" % (int(flipped.sum()), flipped.numel()))
    if not bool(flipped.any()):   # same mask: the two entries are the same linear backward
        for name in want:
            np.testing.assert_allclose(masked[name].numpy(), got[name].numpy(), rtol=1e-12, atol=0, err_msg=name)
    assert set(masked) == set(want)
    for name, ref in want.items():
        rtol, atol = oracle.bound(ref)
        print("%s: %.3f of the bound" % (name, oracle.ratio_to_bound(masked[name], ref)))
        np.testing.assert_allclose(masked[name].numpy(), ref.double().numpy(), rtol=rtol, atol=atol, err_msg=name)


def test_planar_kind_is_conv2d_with_zero_padding():
    x, w, b, _, gy = _inputs(2, 4, 6, 7, 9, 1, False, seed=3)
    got = oracle.grads("planar", x, w, b, 1, None, 0.0, gy)
    ins = [t.double().requires_grad_(True) for t in (x, w, b)]
    y = torch.relu(torch.nn.functional.conv2d(*ins, padding=1))
    want = dict(zip(("x", "weight", "bias"), torch.autograd.grad(y, ins, gy.double())), y=y.detach())
    for name, ref in want.items():
        np.testing.assert_allclose(got[name].numpy(), ref.numpy(), rtol=1e-12, atol=1e-12, err_msg=name)
    # a mask taken from another output changes the gradients exactly where the signs differ
    other = oracle.grads_masked("planar", x, w, b, 1, None, 0.0, gy, torch.ones_like(y))
    np.testing.assert_allclose(other["bias"].numpy(), gy.double().sum((0, 2, 3)).numpy(), rtol=1e-12, atol=1e-12)
