"""SphereConv2D (and the planar 3x3 convolution that shares its kernels) restated in float64 -- a helper of the SphereConv
tests, not a test.

The operator (reference ``spherenet/sphere_cnn.py:111-124``: ``conv2d(grid_sample(x, grid), weight, bias, stride=3)``) seen
through the bilinear tap table ``(idx, wgt)`` of ``tests/sphere_pool_oracle.tap_table`` (held bit-identical to the device's by
``test_device_table_is_the_oracles``): output pixel p, tap t = a*3 + b, corner k samples input pixel ``idx[p*9 + t, k]``
(-1: off the map, contributes 0) with weight ``wgt[p*9 + t, k]``.

    A9[b, p, (t, c)] = sum_k wgt[p*9 + t, k] * x[b, c, idx[p*9 + t, k]]
    y = leaky_relu(A9 @ W2^T + bias (+ residual), slope),   W2 = weight.permute(0, 2, 3, 1) as (O, (t, c))

* ``operand``       A9 (B, P, 9C), float64
* ``linear``        the convolution before its activation: A9 @ W2^T + bias (+ residual) -- ``F.conv2d(padding=1)`` for "planar"
* ``conv``          ``leaky_relu(linear, slope)`` (slope 1: none, 0: ReLU)
* ``grads``         output and gradients by float64 autograd of that expression
* ``grads_masked``  the gradients of the LINEAR part under a given activation mask (the sign of a given output): what a backward
                    that takes the activation's derivative from that output computes, whatever the sign of the exact output

Pure torch; every tensor lives on the CPU.  Inputs of any float dtype are taken at their own values and promoted to float64.
"""
import torch
import torch.nn.functional as F

from tests import sphere_pool_oracle

NAMES = ("x", "weight", "bias", "residual")


def operand(x, idx, wgt):
    """x (B, C, H, W) float64 -> A9 (B, P, 9C) float64, columns ordered (tap, c); differentiable in x."""
    B, C = x.shape[:2]
    xf = x.reshape(B, C, -1)
    idx, wgt = idx.long(), wgt.double()
    v = None
    for k in range(4):
        ok = (idx[:, k] >= 0).double()
        term = xf[:, :, idx[:, k].clamp(min=0)] * (wgt[:, k] * ok)      # (B, C, P*9)
        v = term if v is None else v + term
    P = idx.shape[0] // 9
    return v.view(B, C, P, 9).permute(0, 2, 3, 1).reshape(B, P, 9 * C)


def linear(kind, x, weight, bias, stride, residual=None):
    """The convolution before its activation, (B, O, H', W') float64."""
    B, C, H, W = x.shape
    O = weight.shape[0]
    if kind == "planar":
        y = F.conv2d(x, weight, bias, stride=stride, padding=1)
    else:
        idx, wgt = sphere_pool_oracle.tap_table(H, W, stride)
        ho, wo = sphere_pool_oracle.out_size(H, W, stride)
        w2 = weight.permute(0, 2, 3, 1).reshape(O, 9 * C)
        y = operand(x, idx, wgt) @ w2.t()                                # (B, P, O)
        if bias is not None:
            y = y + bias
        y = y.view(B, ho, wo, O).permute(0, 3, 1, 2)
    return y if residual is None else y + residual


def _activate(z, slope):
    return z if slope == 1.0 else F.leaky_relu(z, slope)


def conv(kind, x, weight, bias, stride=1, residual=None, slope=1.0):
    with torch.no_grad():
        x, weight, bias, residual = _f64(x, weight, bias, residual)
        return _activate(linear(kind, x, weight, bias, stride, residual), float(slope))


def _f64(*ts):
    return [None if t is None else t.detach().double().clone() for t in ts]


def _backward(kind, x, weight, bias, stride, residual, slope, gy, mask):
    ins = _f64(x, weight, bias, residual)
    for t in ins:
        if t is not None:
            t.requires_grad_(True)
    z = linear(kind, *ins[:3], stride, ins[3])
    if mask is None:
        y = _activate(z, float(slope))
        g = gy.detach().double()
    else:
        # the derivative of leaky_relu taken from the GIVEN output: 1 where it is positive, ``slope`` elsewhere (zero included)
        y = z
        one = torch.ones((), dtype=torch.float64)
        g = gy.detach().double() * torch.where(mask.detach().cpu() > 0, one, one * float(slope))
    present = [(n, t) for n, t in zip(NAMES, ins) if t is not None]
    gs = torch.autograd.grad(y, [t for _, t in present], g)
    out = {n: g_ for (n, _), g_ in zip(present, gs)}
    out["y"] = _activate(z.detach(), float(slope))
    return out


def grads(kind, x, weight, bias, stride, residual, slope, gy):
    """{"y", "x", "weight"[, "bias"][, "residual"]}: the output and the gradients of sum(y * gy), float64 autograd."""
    return _backward(kind, x, weight, bias, stride, residual, slope, gy, None)


def grads_masked(kind, x, weight, bias, stride, residual, slope, gy, y_mask):
    """The same, with the activation's derivative taken from ``y_mask``'s sign instead of the exact output's."""
    return _backward(kind, x, weight, bias, stride, residual, slope, gy, y_mask)


def bound(ref):
    """(rtol, atol) of the project's comparison of a SphereConv quantity with a reference: 1e-4 relative + 1e-4 of the
    reference's largest entry (``test_sphere_conv_ngf64_layer_shapes_natural_dispatch``)."""
    return 1e-4, 1e-4 * float(ref.abs().max()) if ref.numel() else 0.0


def ratio_to_bound(got, ref):
    """max |got - ref| / (atol + rtol |ref|), elementwise; 0 for empty tensors."""
    if ref.numel() == 0:
        return 0.0
    rtol, atol = bound(ref)
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float(((got - ref).abs() / (atol + rtol * ref.abs()).clamp(min=1e-300)).max())
