"""GPU: the spherical needlets (csrc/needlets.hip through ``emlight_amd.needlets``) against the reference-made golden file
(``tests/golden/needlets.npz``) and the float64 restatement of the closed form (``needlet_oracle.py``).

Every error is ``max|got - want| / max|want|`` over the compared array.  The tolerances are not guessed: ``FLOOR`` below is
what ``needlet_oracle.float32_floors`` measures on the CPU -- the kernels' arithmetic in numpy float32 (float32 directions,
centres, coefficient table and solid angles; the same forward Legendre recurrence; float32 products and sums) against the
float64 golden (a) and (c) -- and each GPU tolerance is ``4 x`` its floor, the margin for the MFMA's split summation order
(``test_needlets_abi.py`` recomputes the floors and compares them with these constants).  The error of ``P_l(t)`` at a
float32 ``t`` grows with ``l^2``, so the floors are kept per ``jmax`` (matrix) or per shape (analysis, synthesis):

    matrix      jmax 1: 4.6e-7   jmax 2: 1.3e-6   jmax 3: 6.0e-6   jmax 4: 1.9e-5     (tolerance 1.8e-6 ... 7.6e-5)
    analysis    12x24 j1: 3.3e-7   12x24 j2: 3.6e-7   16x32 j3: 1.1e-6   32x64 j2: 1.0e-6
    synthesis   12x24 j1: 2.0e-7   12x24 j2: 2.6e-7   16x32 j3: 1.3e-6   32x64 j2: 3.8e-7

(32 x 64 is not in the golden file: its floors are against the float64 oracle, which equals the golden to 1e-9.)  A gradient
is the other operation, so it takes the other operation's tolerance.  Two comparisons carry a term that is not rounding:
the ``theta = pi`` row against the values at ``pi - 1e-6`` moves the point by 1e-6 rad, which changes a function of degree
``L = 2^(jmax+1)`` by at most ``L * 1e-6 * max|psi|`` (Bernstein's inequality), added to the tolerance there; and the adjoint
identity compares two inner products whose errors are bounded by the operations' tolerances times the sums of the other
factor's magnitudes.  Exact claims (run-to-run, batch independence, sparsify) are ``torch.equal`` / ``array_equal``.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import needlet_oracle as oracle

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR = {"matrix": {1: 4.6e-7, 2: 1.3e-6, 3: 6.0e-6, 4: 1.9e-5},
         "analysis": {"12x24_j1": 3.3e-7, "12x24_j2": 3.6e-7, "16x32_j3": 1.1e-6, "32x64_j2": 1.0e-6},
         "synthesis": {"12x24_j1": 2.0e-7, "12x24_j2": 2.6e-7, "16x32_j3": 1.3e-6, "32x64_j2": 3.8e-7}}
SHAPES = [(12, 24, 1), (16, 32, 3), (32, 64, 2)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key(H, W, jmax):
    return "%dx%d_j%d" % (H, W, jmax)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "needlets.npz"))


@functools.lru_cache(maxsize=None)
def want_matrix(H, W, jmax, grid="reference"):
    return oracle.matrix(*oracle.grid_angles(H, W, grid), jmax)


@functools.lru_cache(maxsize=None)
def basis(H, W, jmax, grid="reference"):
    from emlight_amd.needlets import NeedletBasis
    return NeedletBasis(jmax=jmax, height=H, width=W, grid=grid, device="cuda")


@functools.lru_cache(maxsize=None)
def image(B, H, W, seed=0):
    return oracle.hdr_image(B, H, W, seed)


@functools.lru_cache(maxsize=None)
def want_coeffs(B, H, W, jmax, seed=0):
    """Coefficients the oracle gives the seeded image: the tests' coefficient-like data."""
    return oracle.analysis(image(B, H, W, seed), want_matrix(H, W, jmax), oracle.solid_angles(H, W))


def check(got, want, floor, what, extra=0.0):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, tol = oracle.rel_err(got, want), MARGIN * floor + extra
    print("%s: err %.3e floor %.3e tol %.3e" % (what, err, floor, tol))
    assert err <= tol, (what, err, tol)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the basis matrix
@pytest.mark.parametrize("jmax", [1, 2, 3, 4])
def test_matrix_against_the_reference_rows(jmax):
    g = golden()
    got = basis(4, 8, jmax).matrix(g["a/j%d/theta" % jmax], g["a/j%d/phi" % jmax])
    check(got, g["a/j%d/matrix" % jmax], FLOOR["matrix"][jmax], "matrix jmax %d" % jmax)


@pytest.mark.parametrize("grid", ["reference", "centres"])
@pytest.mark.parametrize("H,W,jmax", SHAPES)
def test_matrix_on_the_grids(H, W, jmax, grid):
    got = basis(H, W, jmax, grid).matrix()
    want = want_matrix(H, W, jmax, grid)
    check(got, want, FLOOR["matrix"][jmax], "matrix %s %s" % (key(H, W, jmax), grid))
    if grid == "reference":                                               # the last row is theta = pi, where the reference is wrong
        south = got[-W:]
        check(south, want[-W:], FLOOR["matrix"][jmax] * float(np.abs(want).max() / np.abs(want[-W:]).max()), "theta = pi row")
        assert all(torch.equal(south[0], south[i]) for i in range(1, W)), "the pole's row must not depend on phi"
        near = oracle.matrix(np.full(W, np.pi - 1e-6), oracle.grid_angles(H, W)[1][-W:], jmax)
        shift = 2 ** (jmax + 1) * 1e-6 * float(np.abs(want).max() / np.abs(near).max())
        check(south, near, FLOOR["matrix"][jmax] * float(np.abs(want).max() / np.abs(near).max()), "theta = pi vs pi - 1e-6", shift)


def test_one_hot_panorama_gives_the_matrix_row_times_the_solid_angle():
    H, W, jmax = 12, 24, 1
    nb, M, w = basis(H, W, jmax), want_matrix(H, W, jmax), oracle.solid_angles(H, W)
    pixels = [(0, 0, 5), (1, 2, H * W - W - 3), (0, 1, 4 * W + 7)]          # the pole, the ragged last chunk, the first chunk
    pano = np.zeros((2, 3, H * W), dtype=np.float32)
    for b, c, p in pixels:
        pano[b, c, p] = 3.0
    got = nb.analysis(dev(pano.reshape(2, 3, H, W))).cpu().numpy()
    scale = float(np.abs(M).max())
    for b, c, p in pixels:
        want = 3.0 * M[p] * w[p]
        check(got[b, :, c], want, FLOOR["matrix"][jmax] * scale * 3.0 * w[p] / float(np.abs(want).max()), "one-hot pixel %d" % p)
    assert np.all(got[1, :, 0] == 0) and np.all(got[1, :, 1] == 0)


# ------------------------------------------------------------------------------------------------ 2. analysis
@pytest.mark.parametrize("H,W,jmax", [(12, 24, 1), (12, 24, 2), (16, 32, 3)])
def test_analysis_against_the_reference_coefficients(H, W, jmax):
    g = golden()
    got = basis(H, W, jmax).analysis(dev(g["c/%s/image" % key(H, W, jmax)]))
    check(got, g["c/%s/coeffs" % key(H, W, jmax)], FLOOR["analysis"][key(H, W, jmax)], "analysis " + key(H, W, jmax))


@pytest.mark.parametrize("H,W,jmax,B", [(12, 24, 1, 2), (16, 32, 3, 1), (32, 64, 2, 11)])
def test_analysis_against_the_oracle(H, W, jmax, B):
    x = image(B, H, W)
    check(basis(H, W, jmax).analysis(dev(x)), want_coeffs(B, H, W, jmax), FLOOR["analysis"][key(H, W, jmax)],
          "analysis %s B %d" % (key(H, W, jmax), B))
    got = basis(H, W, jmax, "centres").analysis(dev(x), weighted=False)
    check(got, oracle.analysis(x, want_matrix(H, W, jmax, "centres")), FLOOR["analysis"][key(H, W, jmax)],
          "analysis %s B %d centres unweighted" % (key(H, W, jmax), B))


# ------------------------------------------------------------------------------------------------ 3. synthesis
@pytest.mark.parametrize("H,W,jmax,B", [(12, 24, 1, 1), (16, 32, 3, 11), (32, 64, 2, 2)])
def test_synthesis_against_the_oracle(H, W, jmax, B):
    co = want_coeffs(B, H, W, jmax).astype(np.float32)
    nb, M = basis(H, W, jmax), want_matrix(H, W, jmax)
    check(nb.synthesis(dev(co)), oracle.synthesis(co, M, H, W), FLOOR["synthesis"][key(H, W, jmax)],
          "synthesis %s B %d" % (key(H, W, jmax), B))
    check(nb.synthesis(dev(co), weighted=True), oracle.synthesis(co, M, H, W, oracle.solid_angles(H, W)),
          FLOOR["synthesis"][key(H, W, jmax)], "weighted synthesis %s B %d" % (key(H, W, jmax), B))


# ------------------------------------------------------------------------------------------------ 4. adjoints and gradients
@pytest.mark.parametrize("H,W,jmax,B", [(12, 24, 1, 2), (16, 32, 3, 2)])
def test_adjoint_identity_and_autograd(H, W, jmax, B):
    nb, M, w = basis(H, W, jmax), want_matrix(H, W, jmax), oracle.solid_angles(H, W)
    k = key(H, W, jmax)
    x, g = image(B, H, W, seed=1), want_coeffs(B, H, W, jmax, seed=2).astype(np.float32)
    xt, gt = dev(x).requires_grad_(True), dev(g)
    c = nb.analysis(xt)
    (c * gt).sum().backward()
    want_dx = oracle.synthesis(g, M, H, W, w)                              # d<A x, g>/dx = A^T g: the weighted synthesis
    check(xt.grad, want_dx, FLOOR["synthesis"][k], "d analysis / d pano " + k)
    c64, dx64 = c.detach().cpu().numpy().astype(np.float64), xt.grad.cpu().numpy().astype(np.float64)
    lhs, rhs = float((c64 * g).sum()), float((x.astype(np.float64) * dx64).sum())
    bound = MARGIN * (FLOOR["analysis"][k] * np.abs(c64).max() * np.abs(g).sum() + FLOOR["synthesis"][k] * np.abs(dx64).max() * np.abs(x).sum())
    print("adjoint %s: <Ax, g> %.9e <x, A^T g> %.9e diff %.3e bound %.3e" % (k, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    # synthesis (unweighted): its gradient is the unweighted analysis of the upstream gradient
    ct, up = dev(g).requires_grad_(True), image(B, H, W, seed=3)
    (nb.synthesis(ct) * dev(up)).sum().backward()
    check(ct.grad, oracle.analysis(up, M), FLOOR["analysis"][k], "d synthesis / d coeffs " + k)
    ct2 = dev(g).requires_grad_(True)
    (nb.synthesis(ct2, weighted=True) * dev(up)).sum().backward()
    check(ct2.grad, oracle.analysis(up, M, w), FLOOR["analysis"][k], "d weighted synthesis / d coeffs " + k)


# ------------------------------------------------------------------------------------------------ 5. exactness
def test_an_image_is_treated_the_same_in_any_batch_and_run():
    H, W, jmax = 16, 32, 3
    nb = basis(H, W, jmax)
    x = dev(image(11, H, W, seed=4))
    c11 = nb.analysis(x)
    assert torch.equal(c11, nb.analysis(x)), "two runs differ"
    assert torch.equal(c11[4:5], nb.analysis(x[4:5].contiguous())), "alone"
    perm = torch.tensor([7, 4, 0, 10], device="cuda")
    assert torch.equal(c11[perm], nb.analysis(x[perm].contiguous())), "at another batch position"
    nb2 = basis(32, 64, 2)                                                # more than one pixel split
    y = dev(image(3, 32, 64, seed=4))
    assert torch.equal(nb2.analysis(y)[2:3], nb2.analysis(y[2:3].contiguous())) and torch.equal(nb2.analysis(y), nb2.analysis(y))
    r11 = nb.synthesis(c11)
    assert torch.equal(r11, nb.synthesis(c11)) and torch.equal(r11[4:5], nb.synthesis(c11[4:5].contiguous()))
    assert torch.equal(r11[perm], nb.synthesis(c11[perm].contiguous()))


@pytest.mark.parametrize("levels,ratio", [((2, 3), 0.1), ((0,), 0.5), ((), 0.1), ((0, 1, 2, 3), 1.0), ((1, 3), 0.0)])
def test_sparsify_equals_the_oracle(levels, ratio):
    jmax = 3
    nb = basis(16, 32, jmax)
    c = want_coeffs(3, 16, 32, jmax, seed=5).astype(np.float32)
    c[1, 700:, :] = 0.0                                                   # a level whose maximum is 0 in part of the batch
    c[2, 253:] = 0.0
    got, kept = nb.sparsify(dev(c), ratio=ratio, levels=levels)
    want, want_kept = oracle.sparsify(c, jmax, ratio, levels)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(kept.cpu().numpy(), want_kept)
    sl = oracle.level_slices(jmax)
    for j in range(-1, jmax + 1):
        if j not in levels:
            assert np.array_equal(got.cpu().numpy()[:, sl[j + 1]], c[:, sl[j + 1]]), "level %d must pass through" % j


def test_sparsify_drops_a_planted_tie():
    jmax = 3
    nb = basis(16, 32, jmax)
    c = np.clip(want_coeffs(2, 16, 32, jmax, seed=6), -7.0, 7.0).astype(np.float32)
    s = oracle.level_slices(jmax)[3]                                      # level 2
    c[0, s.start + 5, 1] = -8.0                                           # the level's maximum: threshold 0.25 * 8 = 2 exactly
    c[0, s.start + 9, 0] = 2.0                                            # the tie: |c| > 2 is false
    c[0, s.start + 11, 2] = -2.0
    c[0, s.start + 13, 0] = np.nextafter(np.float32(2.0), np.float32(3.0))
    got, kept = nb.sparsify(dev(c), ratio=0.25, levels=(2,))
    got = got.cpu().numpy()
    want, want_kept = oracle.sparsify(c, jmax, 0.25, (2,))
    assert got[0, s.start + 9, 0] == 0.0 and got[0, s.start + 11, 2] == 0.0 and got[0, s.start + 13, 0] == c[0, s.start + 13, 0]
    assert got[0, s.start + 5, 1] == -8.0
    assert np.array_equal(got, want) and np.array_equal(kept.cpu().numpy(), want_kept)
    assert int(kept[0, 2]) == int((np.abs(c[0, s]) > 2.0).sum()) and int(kept[0, 3]) == 3 * 768
