"""GPU: the adjoint of the prefiltered environment maps (csrc/env_prefilter_bwd.hip through
``emlight_amd.insert_grad``) against the float64 restatement (``insert_grad_oracle.prefilter_adjoint``).

The bound, per texel, is derived the way the forward's was (DESIGN sections 15 and 23).  A texel's value is a float32 sum of
``n = L 2 Ho^2`` terms ``c_l k_l(x) g`` of mixed sign: sequential float32 accumulation (inside an MFMA, across chunks, across
the splits) is off by at most ``n EPS`` times the sum of the terms' magnitudes, which is ``A = prefilter_adjoint(|g|)``; each
weight ``k_l(x)`` carries the 4 roundings behind ``x`` amplified by the exponent ``m`` and the roundings of ``log2``, ``exp2``,
``c_l``, the staging product and ``dOmega_t`` (the forward's ``4 m + 64``), relative to a weight that is at most 1:

    |got - want| <= EPS (n A[b, ch, t] + (4 m_max + 64) dOmega_t sum_l c_l sum_d |g[b, l, ch, d]|)

with ``m_max`` the largest exponent (1 for the diffuse lobe).  The shapes are the smallest that reach every kernel path (see
``CASES``).  Bit-exactness is asserted with ``torch.equal``."""
import functools

import numpy as np
import pytest
import torch

from tests import insert_grad_oracle as grad_oracle
from tests import insert_oracle as oracle
from tests import sphere_render_oracle as sro

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
D = oracle.DIFFUSE

#        H   Ho  B   lobes
CASES = [(16, 8, 3, (D, 50.0)),              # baseline: 512 texels, 128 directions of two lobes, 9 columns
         (16, 5, 1, (1.0,)),                 # 50 directions: a partial k chunk; no diffuse lobe
         (16, 8, 33, (D,)),                  # 99 columns: a second column group, partial
         (12, 7, 2, (D, 0.0, 200.0, 50.0)),  # 288 texels: a partial row tile; four lobes in one pass; 0^0 = 1
         (4, 64, 2, (D, 50.0))]              # one row group, 128 chunks per lobe over 64 splits: the split over k


def grad(B, L, Ho, seed):
    """normal * exp(normal): mixed signs and a wide range."""
    g = np.random.default_rng([seed, B, L, Ho])
    return (g.standard_normal((B, L, 3, Ho, 2 * Ho)) * np.exp(g.standard_normal((B, L, 3, Ho, 2 * Ho)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(H, Ho, lobe):
    return oracle.lobe_weights(H, Ho, lobe)


def scale(lobe):
    return 1.0 / np.pi if lobe == D else (float(lobe) + 1.0) / (2.0 * np.pi)


def bound(g, H, lobes, n=None):
    g = np.abs(np.asarray(g, dtype=np.float64))
    B, L, _, Ho, _ = g.shape
    n = L * 2 * Ho * Ho if n is None else n
    m_max = max(1.0 if lb == D else float(lb) for lb in lobes)
    dom = sro.texel_grid(H, 2 * H)[1].reshape(H, 2 * H)
    mass = sum(scale(lb) * g[:, l].sum((2, 3)) for l, lb in enumerate(lobes))                      # (B, 3)
    return EPS * (n * grad_oracle.prefilter_adjoint(g, H, lobes, weights) + (4 * m_max + 64) * dom * mass[:, :, None, None])


def adjoint(g, H, lobes):
    from emlight_amd.insert_grad import prefilter_environment_bwd_raw
    return prefilter_environment_bwd_raw(torch.from_numpy(g).cuda(), H, lobes)


def check(got, g, H, lobes, what, n=None):
    got = got.cpu().numpy().astype(np.float64)
    want = grad_oracle.prefilter_adjoint(g, H, lobes, weights)
    assert got.shape == want.shape == (g.shape[0], 3, H, 2 * H)
    tol = bound(g, H, lobes, n)
    err = np.abs(got - want)
    print("%s: largest error / bound %.3e; the bound is below |want| on %.1f %% of the texels"
          % (what, float((err[tol > 0] / tol[tol > 0]).max()), 100.0 * float((tol < np.abs(want)).mean())))
    assert np.all(err <= tol), (what, float((err - tol).max()))


@pytest.mark.parametrize("H,Ho,B,lobes", CASES)
def test_against_the_oracle(H, Ho, B, lobes):
    g = grad(B, len(lobes), Ho, 51)
    check(adjoint(g, H, lobes), g, H, lobes, "H %d Ho %d B %d lobes %s" % (H, Ho, B, lobes))


@pytest.mark.parametrize("direction", [(0, 3), (4, 0), (7, 15), (3, 8)], ids=["pole", "seam", "last", "middle"])
def test_one_hot_direction(direction):
    """One direction of one lobe: every texel is the value times ONE weight -- no summation to hide behind (the zeros of
    the other directions add exactly), so the bound holds with n = 1."""
    H, Ho, lobes = 16, 8, (D, 50.0)
    for l, lb in enumerate(lobes):
        g = np.zeros((1, 2, 3, Ho, 2 * Ho), dtype=np.float32)
        g[0, l, :, direction[0], direction[1]] = (100.0, -1.0, 0.01)
        got = adjoint(g, H, lobes)
        check(got, g, H, lobes, "one-hot %s lobe %s" % (direction, lb), n=1)
        row = weights(H, Ho, lb)[direction[0] * 2 * Ho + direction[1]].reshape(H, 2 * H)
        for ch, v in enumerate((100.0, -1.0, 0.01)):
            want = np.float64(np.float32(v)) * row
            assert np.all(np.abs(got[0, ch].cpu().numpy() - want) <= bound(g, H, lobes, 1)[0, ch])


def test_adjoint_identity_between_the_two_kernels():
    """``<E(p), g> = <p, E^T(g)>`` in float64 from the device outputs of both kernels, within the sum of their bounds."""
    from emlight_amd.insert import prefilter_environment
    H, Ho, B, lobes = 12, 7, 2, (D, 0.0, 200.0, 50.0)
    rng = np.random.default_rng(52)
    p = (rng.random((B, 3, H, 2 * H)) ** 4 * 50.0 + 0.01).astype(np.float32)
    g = grad(B, len(lobes), Ho, 53)
    fwd = prefilter_environment(torch.from_numpy(p).cuda(), Ho, lobes).cpu().numpy().astype(np.float64)
    bwd = adjoint(g, H, lobes).cpu().numpy().astype(np.float64)
    want = oracle.prefilter(p, Ho, lobes, weights)
    tol_f = np.stack([(H * 2 * H + 4 * (1.0 if lb == D else lb) + 64) * EPS * np.abs(want[:, l]).reshape(B, -1).max(1)
                      for l, lb in enumerate(lobes)], 1)                                           # (B, L): the forward's bound
    slack = float((np.abs(g.astype(np.float64)).sum((2, 3, 4)) * tol_f).sum()) + float((np.abs(p) * bound(g, H, lobes)).sum())
    lhs, rhs = float((fwd * g).sum()), float((p.astype(np.float64) * bwd).sum())
    print("adjoint identity: |lhs - rhs| / slack %.3e (lhs %.6e)" % (abs(lhs - rhs) / slack, lhs))
    assert abs(lhs - rhs) <= slack


def test_run_to_run_and_batch_independence():
    H, Ho, four = 12, 7, (D, 0.0, 200.0, 50.0)
    g = grad(3, 4, Ho, 54)
    a = adjoint(g, H, four)
    assert torch.equal(a, adjoint(g, H, four))                                         # no atomics: the same bits again
    assert torch.equal(adjoint(g[:1], H, four), a[:1])                                 # an image does not see its batch
    many = grad(33, 1, 8, 55)                                                          # a second column group
    b = adjoint(many, 16, (D,))
    assert torch.equal(adjoint(many[32:], 16, (D,)), b[32:]) and torch.equal(adjoint(many[:3], 16, (D,)), b[:3])
    split = grad(2, 2, 64, 56)                                                         # with the split over k
    c = adjoint(split, 4, (D, 50.0))
    assert torch.equal(adjoint(split[1:], 4, (D, 50.0)), c[1:]) and torch.equal(c, adjoint(split, 4, (D, 50.0)))


def test_autograd_is_the_raw_call_and_only_enqueues():
    from emlight_amd import insert, insert_grad
    H, Ho, lobes = 16, 5, (D, 20.0, 3.0)
    pano = torch.rand(2, 3, H, 2 * H, device="cuda")
    g = torch.from_numpy(grad(2, 3, Ho, 57)).cuda()
    want = insert_grad.prefilter_environment_bwd_raw(g, H, lobes)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x = pano.clone().requires_grad_(True)
        out = insert_grad.prefilter_environment(x, Ho, lobes)
        out.backward(g)
        plain = insert_grad.prefilter_environment(pano, Ho, lobes)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(x.grad, want)
    assert torch.equal(out.detach(), insert.prefilter_environment(pano, Ho, lobes)) and torch.equal(plain, out.detach())
    assert not plain.requires_grad
    # one lobe's slice: autograd places the contiguous gradient, the other lobes get zeros
    x = pano.clone().requires_grad_(True)
    insert_grad.prefilter_environment(x, Ho, lobes)[:, 1].backward(g[:, 1])
    only = torch.zeros_like(g)
    only[:, 1] = g[:, 1]
    assert torch.equal(x.grad, insert_grad.prefilter_environment_bwd_raw(only, H, lobes))
