"""GPU: the spherical needlets (csrc/needlets.hip through ``emlight_amd.needlets``) against the reference-made golden file
(``tests/golden/needlets.npz``) and the float64 restatement of the closed form (``needlet_oracle.py``).

Every error is ``max|got - want| / max|want|`` over the compared array.  The tolerances are not guessed: ``FLOOR`` below is
what ``needlet_oracle.float32_floors`` measures on the CPU -- the kernels' arithmetic in numpy float32 (float32 directions,
centres, coefficient table and solid angles; the same forward Legendre recurrence; float32 products and sums) against the
float64 golden (a) and (c) -- and each GPU tolerance is ``4 x`` its floor, the margin for the MFMA's split summation order
(``test_needlets_abi.py`` recomputes the floors and compares them with these constants).  The error of ``P_l(t)`` at a
float32 ``t`` grows with ``l^2`` and the error of a sum depends on its terms, so the matrix floors are kept per ``jmax`` and
every analysis or synthesis floor is measured on the very input its test feeds in: the key names the shape, ``jmax``, the
batch size and the seed of ``needlet_oracle.hdr_image`` (which seeds itself with the batch size too), or the golden file's
image, or all ones.  The lists of cases live in ``needlet_oracle.py``, where ``float32_floors`` reads them as well.  Only the
golden images are held against the golden (c); everything else is against the float64 oracle, which equals the golden to 1e-9.

The shapes are chosen by what ``make_plan`` and the kernels' tiling do with them: 25 x 47 at ``jmax`` 4, 50 x 100 at 1 and
48 x 96 at 0 give an analysis split two chunks of 64 pixels (the prefetch inside the chunk loop, a last split of one chunk or a
full one, ragged last chunks of 23 and 8 pixels); 4 x 8 and 3 x 5 have a single chunk of fewer than 64 pixels; ``jmax`` 0 has
K = 13 < 64 basis rows, one ragged reduction chunk of the synthesis; batches of 32, 33 and 65 make 96, 96 + 3 and 96 + 96 + 3
image planes, that is one full column group of a workgroup, a second group of 3 and a third.  ``jmax`` 0 and 4 are the
shortest and the longest Legendre recurrence (L = 2 and 32).

A gradient is the other operation, so it takes the other operation's tolerance, measured on the upstream gradient it is given.
Two comparisons carry a term that is not rounding:
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
FLOOR = {"matrix": {0: 6.7e-8, 1: 4.6e-7, 2: 1.3e-6, 3: 6.0e-6, 4: 1.9e-5},
         "analysis": {"12x24_j1_b2_golden": 3.3e-7, "12x24_j2_b2_golden": 3.6e-7, "16x32_j3_b2_golden": 1.1e-6,
                      "12x24_j1_b2": 3.7e-7, "16x32_j3_b1": 5.9e-7, "32x64_j2_b11": 1.4e-6,
                      "25x47_j4_b2": 1.8e-6, "50x100_j1_b2": 3.0e-6, "48x96_j0_b1": 1.5e-6, "4x8_j0_b3": 1.5e-7, "3x5_j2_b2": 5.5e-7,
                      "12x24_j1_b32": 6.8e-7, "12x24_j1_b33": 7.7e-7, "12x24_j1_b65": 6.9e-7,
                      "12x24_j1_b2_s1": 4.2e-7, "12x24_j1_b2_s3": 3.5e-7, "16x32_j3_b2_s1": 6.5e-7, "16x32_j3_b2_s3": 1.1e-6,
                      "25x47_j4_b2_s1": 1.53e-6, "25x47_j4_b2_s3": 1.54e-6, "50x100_j1_b33_s1": 4.4e-6, "50x100_j1_b33_s3": 2.9e-6,
                      "12x24_j1_b2_ones": 3.8e-7},
         "synthesis": {"12x24_j1_b1": 2.7e-7, "16x32_j3_b11": 1.31e-6, "32x64_j2_b2": 3.8e-7,
                       "25x47_j4_b2": 4.2e-6, "4x8_j0_b3": 1.02e-7, "3x5_j2_b2": 3.0e-7, "48x96_j0_b1": 3.3e-7,
                       "12x24_j1_b32": 2.7e-7, "12x24_j1_b33": 2.5e-7, "12x24_j1_b65": 2.7e-7,
                       "12x24_j1_b2_s2": 2.3e-7, "16x32_j3_b2_s2": 9.3e-7, "25x47_j4_b2_s2": 5.1e-6, "50x100_j1_b33_s2": 4.0e-7,
                       "12x24_j1_b2_ones": 1.91e-6}}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key(H, W, jmax):
    return "%dx%d_j%d" % (H, W, jmax)


def floor_of(quantity, H, W, jmax, B, source=0):
    return FLOOR[quantity][oracle.floor_key(H, W, jmax, B, source)]


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


def poison(nb, B):
    """NaN into what the next analysis or synthesis of ``B`` images writes to: the basis' scratch, and freed blocks of the
    sizes of both outputs, which the caching allocator hands to the next ``empty`` of that size.  A plane that a kernel fails
    to store must not pass on the correct values an earlier call of the same shape left in that memory."""
    from emlight_amd import _lib
    nan = float("nan")
    nb._scratch(_lib.lib(), B).fill_(nan)
    for shape in ((B, nb.K, 3), (B, 3, nb.height, nb.width)):
        torch.full(shape, nan, dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the basis matrix
@pytest.mark.parametrize("jmax", [1, 2, 3, 4])
def test_matrix_against_the_reference_rows(jmax):
    g = golden()
    got = basis(4, 8, jmax).matrix(g["a/j%d/theta" % jmax], g["a/j%d/phi" % jmax])
    check(got, g["a/j%d/matrix" % jmax], FLOOR["matrix"][jmax], "matrix jmax %d" % jmax)


@pytest.mark.parametrize("grid", ["reference", "centres"])
@pytest.mark.parametrize("H,W,jmax", oracle.GRID_SHAPES)
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
@pytest.mark.parametrize("H,W,jmax", oracle.GOLDEN_SHAPES)
def test_analysis_against_the_reference_coefficients(H, W, jmax):
    g = golden()
    got = basis(H, W, jmax).analysis(dev(g["c/%s/image" % key(H, W, jmax)]))
    check(got, g["c/%s/coeffs" % key(H, W, jmax)], floor_of("analysis", H, W, jmax, 2, "golden"), "analysis golden " + key(H, W, jmax))


def analysis_both_ways(H, W, jmax, B):
    """The reference grid with the solid angles and the centres grid without them, against the oracle.  The second comparison
    borrows the first one's floor, as it always has: the same image and the same sum over the pixels, but other directions and
    no solid angles, so that floor is not measured on exactly these summands."""
    x, xd = image(B, H, W), dev(image(B, H, W))
    poison(basis(H, W, jmax), B)
    check(basis(H, W, jmax).analysis(xd), want_coeffs(B, H, W, jmax), floor_of("analysis", H, W, jmax, B),
          "analysis %s B %d" % (key(H, W, jmax), B))
    poison(basis(H, W, jmax, "centres"), B)
    got = basis(H, W, jmax, "centres").analysis(xd, weighted=False)
    check(got, oracle.analysis(x, want_matrix(H, W, jmax, "centres")), floor_of("analysis", H, W, jmax, B),
          "analysis %s B %d centres unweighted" % (key(H, W, jmax), B))


@pytest.mark.parametrize("H,W,jmax,B", oracle.ANALYSIS_CASES)
def test_analysis_against_the_oracle(H, W, jmax, B):
    analysis_both_ways(H, W, jmax, B)


# ------------------------------------------------------------------------------------------------ 3. synthesis
def synthesis_both_ways(H, W, jmax, B):
    co = want_coeffs(B, H, W, jmax).astype(np.float32)
    nb, M, cd = basis(H, W, jmax), want_matrix(H, W, jmax), dev(co)
    poison(nb, B)
    check(nb.synthesis(cd), oracle.synthesis(co, M, H, W), floor_of("synthesis", H, W, jmax, B),
          "synthesis %s B %d" % (key(H, W, jmax), B))
    poison(nb, B)
    check(nb.synthesis(cd, weighted=True), oracle.synthesis(co, M, H, W, oracle.solid_angles(H, W)),
          floor_of("synthesis", H, W, jmax, B), "weighted synthesis %s B %d" % (key(H, W, jmax), B))


@pytest.mark.parametrize("H,W,jmax,B", oracle.SYNTHESIS_CASES)
def test_synthesis_against_the_oracle(H, W, jmax, B):
    synthesis_both_ways(H, W, jmax, B)


@pytest.mark.parametrize("H,W,jmax,B", oracle.COLUMN_GROUP_CASES)
def test_column_groups_against_the_oracle(H, W, jmax, B):
    """3B = 96 planes fill one workgroup's columns exactly; 99 and 195 need a second and a third (``blockIdx.y`` > 0), the last
    of 3 planes: the plane -> (image, channel) addressing beyond plane 96, in both GEMMs and in the analysis' reduction."""
    analysis_both_ways(H, W, jmax, B)
    synthesis_both_ways(H, W, jmax, B)


# ------------------------------------------------------------------------------------------------ 4. adjoints and gradients
@pytest.mark.parametrize("H,W,jmax,B", oracle.ADJOINT_CASES)
def test_adjoint_identity_and_autograd(H, W, jmax, B):
    """Each operation's backward is the other's kernel: 25 x 47 at jmax 4 and 50 x 100 at jmax 1 with 99 planes put the chunk
    loop of the analysis and the column groups through the transposed instance as well."""
    nb, M, w = basis(H, W, jmax), want_matrix(H, W, jmax), oracle.solid_angles(H, W)
    k, seeds = "%s B %d" % (key(H, W, jmax), B), oracle.ADJOINT_SEEDS
    f_x, f_up = floor_of("analysis", H, W, jmax, B, seeds["x"]), floor_of("analysis", H, W, jmax, B, seeds["up"])
    f_g = floor_of("synthesis", H, W, jmax, B, seeds["g"])
    x, g = image(B, H, W, seed=seeds["x"]), want_coeffs(B, H, W, jmax, seed=seeds["g"]).astype(np.float32)
    xt, gt = dev(x).requires_grad_(True), dev(g)
    c = nb.analysis(xt)
    (c * gt).sum().backward()
    want_dx = oracle.synthesis(g, M, H, W, w)                              # d<A x, g>/dx = A^T g: the weighted synthesis
    check(xt.grad, want_dx, f_g, "d analysis / d pano " + k)
    c64, dx64 = c.detach().cpu().numpy().astype(np.float64), xt.grad.cpu().numpy().astype(np.float64)
    lhs, rhs = float((c64 * g).sum()), float((x.astype(np.float64) * dx64).sum())
    bound = MARGIN * (f_x * np.abs(c64).max() * np.abs(g).sum() + f_g * np.abs(dx64).max() * np.abs(x).sum())
    print("adjoint %s: <Ax, g> %.9e <x, A^T g> %.9e diff %.3e bound %.3e" % (k, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    # synthesis (unweighted): its gradient is the unweighted analysis of the upstream gradient
    ct, up = dev(g).requires_grad_(True), image(B, H, W, seed=seeds["up"])
    (nb.synthesis(ct) * dev(up)).sum().backward()
    check(ct.grad, oracle.analysis(up, M), f_up, "d synthesis / d coeffs " + k)
    ct2 = dev(g).requires_grad_(True)
    (nb.synthesis(ct2, weighted=True) * dev(up)).sum().backward()
    check(ct2.grad, oracle.analysis(up, M, w), f_up, "d weighted synthesis / d coeffs " + k)


def test_backward_of_a_sum_takes_a_stride_0_gradient():
    """``.sum().backward()`` hands the other operation an all-ones gradient expanded with stride 0 (a hook on the output sees
    the strides; the second gradient is expanded by hand, so that one does not depend on how ``sum`` builds it); the wrapper
    makes it contiguous before the kernel reads it.  The unweighted analysis' gradient is the unweighted synthesis of ones, the weighted
    synthesis' gradient the weighted analysis of ones: the two quantities the "ones" floors are measured on."""
    H, W, jmax, B = oracle.SUM_BACKWARD_CASE
    nb, M, w = basis(H, W, jmax), want_matrix(H, W, jmax), oracle.solid_angles(H, W)
    seen = []
    xt = dev(image(B, H, W)).requires_grad_(True)
    out = nb.analysis(xt, weighted=False)
    out.register_hook(lambda g: seen.append(g.stride()))
    out.sum().backward()
    check(xt.grad, oracle.synthesis(np.ones((B, nb.K, 3)), M, H, W), floor_of("synthesis", H, W, jmax, B, "ones"),
          "d sum(analysis) / d pano " + key(H, W, jmax))
    ct = dev(want_coeffs(B, H, W, jmax)).requires_grad_(True)
    out = nb.synthesis(ct, weighted=True)
    out.register_hook(lambda g: seen.append(g.stride()))
    out.backward(torch.ones((), device="cuda").expand_as(out))             # expanded by hand: stride 0 whatever sum() does
    check(ct.grad, oracle.analysis(np.ones((B, 3, H, W)), M, w), floor_of("analysis", H, W, jmax, B, "ones"),
          "d sum(weighted synthesis) / d coeffs " + key(H, W, jmax))
    assert seen == [(0, 0, 0), (0, 0, 0, 0)], "the gradients handed to the backward passes were not stride-0: %s" % (seen,)


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


def test_an_image_is_treated_the_same_in_any_column_group():
    """The same claim across ``blockIdx.y``: image 40 of a batch of 65 lies in the second column group (planes 120..122); it
    must come out as it does alone and at position 2 of a batch of 5, where it lies in the first.  The claim rests on the
    split depending on (P, jmax) only, so one shape whose splits hold two chunks is held to it as well."""
    H, W, jmax = 12, 24, 1
    nb = basis(H, W, jmax)
    x = dev(image(65, H, W, seed=4))
    five = torch.tensor([0, 64, 40, 33, 31], device="cuda")
    poison(nb, 65)
    c65 = nb.analysis(x)
    assert bool(torch.isfinite(c65).all()), "a plane of the batch of 65 was never stored"
    assert torch.equal(c65[40:41], nb.analysis(x[40:41].contiguous())), "analysis, alone"
    assert torch.equal(c65[five], nb.analysis(x[five].contiguous())), "analysis, in a batch of 5"
    poison(nb, 65)
    r65 = nb.synthesis(c65)
    assert bool(torch.isfinite(r65).all()), "a plane of the batch of 65 was never stored"
    assert torch.equal(r65[40:41], nb.synthesis(c65[40:41].contiguous())), "synthesis, alone"
    assert torch.equal(r65[five], nb.synthesis(c65[five].contiguous())), "synthesis, in a batch of 5"
    nb2 = basis(50, 100, 1)                                               # two chunks per split
    y = dev(image(3, 50, 100, seed=4))
    c3 = nb2.analysis(y)
    assert torch.equal(c3, nb2.analysis(y)) and torch.equal(c3[1:2], nb2.analysis(y[1:2].contiguous()))
    r3 = nb2.synthesis(c3)
    assert torch.equal(r3, nb2.synthesis(c3)) and torch.equal(r3[1:2], nb2.synthesis(c3[1:2].contiguous()))


def sparsify_equals_the_oracle(H, W, jmax, levels, ratio):
    nb = basis(H, W, jmax)
    c = want_coeffs(3, H, W, jmax, seed=5).astype(np.float32)
    c[1, 700:, :] = 0.0                                                   # a level whose maximum is 0 in part of the batch
    c[2, 253:] = 0.0
    if jmax == 0:                                                         # K = 13: both slices above are empty.  Image 1 loses
        c[1, nb.K // 2:, :] = 0.0                                         # half of level 0, image 2 keeps Y_00 alone: its only
        c[2, 1:] = 0.0                                                    # level is all zero (threshold 0, nothing kept)
    got, kept = nb.sparsify(dev(c), ratio=ratio, levels=levels)
    want, want_kept = oracle.sparsify(c, jmax, ratio, levels)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(kept.cpu().numpy(), want_kept)
    sl = oracle.level_slices(jmax)
    for j in range(-1, jmax + 1):
        if j not in levels:
            assert np.array_equal(got.cpu().numpy()[:, sl[j + 1]], c[:, sl[j + 1]]), "level %d must pass through" % j


@pytest.mark.parametrize("levels,ratio", [((2, 3), 0.1), ((0,), 0.5), ((), 0.1), ((0, 1, 2, 3), 1.0), ((1, 3), 0.0)])
def test_sparsify_equals_the_oracle(levels, ratio):
    sparsify_equals_the_oracle(16, 32, 3, levels, ratio)


@pytest.mark.parametrize("H,W,jmax,levels", [(4, 8, 0, (0,)), (25, 47, 4, (2, 3, 4))])
def test_sparsify_at_the_smallest_and_largest_jmax(H, W, jmax, levels):
    """K = 13 (a level of 36 values in one workgroup of 256 threads) and K = 4093 (level 4: 9216 values, 36 per thread)."""
    sparsify_equals_the_oracle(H, W, jmax, levels, 0.1)


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


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_command_line_on_the_device(tmp_path):
    """``python -m emlight_amd.needlets`` over three 8 x 16 panoramas at ``--height 4`` (the resize halves them; a 60 degree
    crop stays inside 8 rows), ``--batchSize 2``: a full batch and a ragged one.  The batcher is tested elsewhere; what is
    expected here is the float64 analysis of the batcher's own output -- ``small``, times the ``tone`` alpha -- which pins the
    permute to channel-first, the alpha's broadcast over the image, the order of the names and ``drop_last=False``.  The
    tolerance is the float32 floor of exactly that input, measured here as ``float32_floors`` measures the others.  The expected
    alpha is taken from one batch of three, the program takes it from batches of two and one: ``tone`` treats every image on
    its own (``test_gpu_panorama_prep.py`` holds it to that bit for bit), and a last-bit difference would be 6e-8 of the value
    against a tolerance of a few 1e-7 or more."""
    from emlight_amd import needlets
    H, W, jmax, fov = 4, 8, 2, 60.0
    panos, names = tmp_path / "panos", ["a", "b", "c"]
    panos.mkdir()
    raw = oracle.hdr_image(3, 2 * H, 2 * W, seed=7).transpose(0, 2, 3, 1)          # (3, 8, 16, 3), channel-last as on disk
    for name, p in zip(reversed(names), raw):                                        # written c, b, a: read back sorted
        np.save(str(panos / (name + ".npy")), p)
    batcher = needlets._batcher(fov, "cuda")
    batcher.PANO_HW = (H, W)
    on_dev = torch.from_numpy(np.ascontiguousarray(raw[::-1])).cuda()               # in name order
    small = batcher.small(on_dev, 0.0).permute(0, 3, 1, 2).contiguous()
    alpha = batcher.tone(batcher.crop(on_dev, 0.0, fov))[1]
    assert small.shape == (3, 3, H, W) and alpha.shape == (3,) and len(set(alpha.tolist())) == 3
    M, w = want_matrix(H, W, jmax), oracle.solid_angles(H, W)
    common = ["--pano_dir", str(panos), "--jmax", str(jmax), "--height", str(H), "--fov", str(fov), "--batchSize", "2"]
    for tag, extra, x in (("no alpha", ["--no_alpha"], small), ("alpha", [], small * alpha.reshape(-1, 1, 1, 1))):
        out = tmp_path / tag.replace(" ", "_")
        assert needlets.main(common + ["--out_dir", str(out)] + extra) == names
        got = np.stack([np.load(str(out / (n + ".npy"))) for n in names])
        assert got.dtype == np.float32
        x = x.cpu().numpy()
        check(got, oracle.analysis(x, M, w), oracle.analysis_floor(x, H, W, jmax), "command line, %s" % tag)
    sparse = tmp_path / "sparse"
    assert needlets.main(common + ["--out_dir", str(sparse), "--sparsify", "0.1"]) == names
    want = oracle.sparsify(got, jmax, 0.1, (2,))[0]                                  # of the files written with alpha
    assert np.array_equal(np.stack([np.load(str(sparse / (n + ".npy"))) for n in names]), want)
    assert (want == 0).sum() > (got == 0).sum(), "the threshold dropped nothing: the comparison would be empty"
