"""GPU: the real spherical harmonics (csrc/harmonics.hip through ``emlight_amd.harmonics``) against the reference-made golden
file (``tests/golden/harmonics.npz``) and the float64 restatement (``harmonic_oracle.py``).

Every error is ``max|got - want| / max|want|`` over the compared array.  The tolerances follow the rule of
``test_gpu_needlets.py``: ``FLOOR`` below is what ``harmonic_oracle.float32_floors`` measures on the CPU -- the kernels'
arithmetic in numpy float32 (the same tables, the same recurrence, the same two-stage order of the sums) against the float64
golden (a) and (c) or the float64 oracle -- and each GPU tolerance is ``4 x`` its floor (``test_harmonics_abi.py`` recomputes the
floors and compares them with these constants).  The matrix floors are kept per convention and ``lmax``; every analysis or
synthesis floor is measured on the very input its test feeds in (shape, ``lmax``, batch size and seed of
``needlet_oracle.hdr_image``, or the golden file's image) and for the very operation: ``harmonic_oracle.QUANTITIES`` names
the grid and whether the solid angles are in.  A case runs in ``harmonic_oracle.convention_of(lmax)``.

The shapes, by what the kernels' tiling (8 rows x 8 planes per workgroup, 128 columns per staged chunk and 32 per wave, the
orders held in registers: 4, 8, 16 or 32) does with them:
  3 x 5   lmax 4   B 2: one ragged row block (3 of 8 rows), 5 columns: only wave 0 has any; 6 of 8 planes
  4 x 8   lmax 1   B 1: 3 of 8 planes, the smallest register bucket with a single m > 0
  12 x 24 lmax 4   B 2: two row blocks, the second of 4 rows; the partial coefficients of two blocks are added
  25 x 47 lmax 8   B 2: four row blocks, the last of one row; an odd width, wave 1 ragged (15 of 32 columns); bucket 8
  64 x 128 lmax 32 B 1: eight full row blocks, exactly one full chunk of 128 columns, all four waves; bucket 32, K = 1089
  12 x 24 lmax 0   B 3: K = 1; 9 planes: a second plane group of one plane, image 2 split over two groups
  12 x 24 lmax 4   B 11 / 33: 33 and 99 planes: 5 and 13 plane groups, the last of one and of three planes
  9 x 133 lmax 16  B 3: a second chunk of 5 columns after a full one; a second row block of one row; bucket 16
  16 x 32 lmax 12: (the exactness test) bucket 16 with lmax below it: orders 13..16 are summed and never used

A gradient is the other operation, so it takes the other operation's tolerance, measured on the upstream gradient it is given.
The adjoint identity compares two inner products whose errors are bounded by the operations' tolerances times the sums of the
other factor's magnitudes.  Exact claims (run-to-run, batch independence, the poles' zeros) are ``torch.equal`` / ``== 0``.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import harmonic_oracle as oracle
from tests import needlet_oracle

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR = {"matrix": {"graphics": {0: 5.22e-08, 1: 6.43e-08, 4: 1.7e-07, 8: 4.86e-07, 32: 1.94e-06},
                    "symmetrised": {0: 5.22e-08, 1: 6.43e-08, 4: 1.7e-07, 8: 4.86e-07, 32: 1.94e-06}},
         "analysis": {"12x24_l4_b2_golden": 8.1e-08, "16x32_l8_b2_golden": 1.48e-07, "3x5_l4_b2": 1.03e-07, "4x8_l1_b1": 6.04e-08,
                      "12x24_l4_b2": 9.65e-08, "25x47_l8_b2": 2.03e-07, "64x128_l32_b1": 4.69e-07, "12x24_l0_b3": 1.02e-07,
                      "12x24_l4_b11": 1.09e-07, "12x24_l4_b33": 1.26e-07, "9x133_l16_b3": 3.44e-07, "12x24_l4_b2_s1": 8.32e-08,
                      "12x24_l4_b2_s3": 1.07e-07, "25x47_l8_b3_s1": 1.95e-07, "25x47_l8_b3_s3": 2.02e-07, "9x133_l16_b3_s1": 3.32e-07,
                      "9x133_l16_b3_s3": 3.35e-07},
         "analysis_unweighted": {"12x24_l4_b2_s3": 1.6e-07, "25x47_l8_b3_s3": 5.16e-07, "9x133_l16_b3_s3": 5.17e-07},
         "analysis_centres": {"3x5_l4_b2": 1.31e-07, "4x8_l1_b1": 6.45e-08, "12x24_l4_b2": 1.56e-07, "25x47_l8_b2": 2.07e-07,
                              "64x128_l32_b1": 2.26e-06, "12x24_l0_b3": 1.41e-07, "12x24_l4_b11": 2.11e-07, "12x24_l4_b33": 2.17e-07,
                              "9x133_l16_b3": 1.43e-06},
         "synthesis": {"3x5_l4_b2": 3.87e-08, "4x8_l1_b1": 1.2e-07, "12x24_l4_b2": 1.77e-07, "25x47_l8_b2": 5.53e-07,
                       "64x128_l32_b1": 2.6e-06, "12x24_l0_b3": 7.05e-08, "12x24_l4_b11": 2.5e-07, "12x24_l4_b33": 2.54e-07,
                       "9x133_l16_b3": 6e-07},
         "synthesis_weighted": {"3x5_l4_b2": 8.01e-08, "4x8_l1_b1": 1.44e-07, "12x24_l4_b2": 1.57e-07, "25x47_l8_b2": 2.13e-07,
                                "64x128_l32_b1": 5.26e-07, "12x24_l0_b3": 4.38e-08, "12x24_l4_b11": 1.78e-07, "12x24_l4_b33": 1.63e-07,
                                "9x133_l16_b3": 3.37e-07, "12x24_l4_b2_s2": 1.2e-07, "25x47_l8_b3_s2": 2.7e-07,
                                "9x133_l16_b3_s2": 3.63e-07},
         "synthesis_centres": {"3x5_l4_b2": 1.29e-07, "4x8_l1_b1": 9.46e-08, "12x24_l4_b2": 2.82e-07, "25x47_l8_b2": 3.52e-07,
                               "64x128_l32_b1": 1.82e-06, "12x24_l0_b3": 7.05e-08, "12x24_l4_b11": 2.8e-07, "12x24_l4_b33": 3e-07,
                               "9x133_l16_b3": 1.47e-06}}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key(H, W, lmax):
    return "%dx%d_l%d" % (H, W, lmax)


def floor_of(quantity, H, W, lmax, B, source=0):
    return FLOOR[quantity][oracle.floor_key(H, W, lmax, B, source)]


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "harmonics.npz"))


@functools.lru_cache(maxsize=None)
def basis(H, W, lmax, grid="reference", convention=None):
    from emlight_amd.harmonics import HarmonicBasis
    return HarmonicBasis(lmax=lmax, height=H, width=W, grid=grid, convention=convention or oracle.convention_of(lmax), device="cuda")


def want_matrix(H, W, lmax, grid="reference", convention=None):
    return oracle.grid_matrix(H, W, lmax, grid, convention or oracle.convention_of(lmax))


@functools.lru_cache(maxsize=None)
def image(B, H, W, seed=0):
    return oracle.hdr_image(B, H, W, seed)


@functools.lru_cache(maxsize=None)
def want_coeffs(B, H, W, lmax, seed=0):
    return oracle.coefficients_of(H, W, lmax, B, seed)


def check(got, want, floor, what, extra=0.0):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, tol = oracle.rel_err(got, want), MARGIN * floor + extra
    print("%s: err %.3e floor %.3e tol %.3e" % (what, err, floor, tol))
    assert err <= tol, (what, err, tol)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def poison(hb, B):
    """NaN into what the next analysis or synthesis of ``B`` images writes to (see ``test_gpu_needlets.poison``)."""
    from emlight_amd import _lib
    nan = float("nan")
    hb._scratch(_lib.lib(), B).fill_(nan)
    for shape in ((B, hb.K, 3), (B, 3, hb.height, hb.width)):
        torch.full(shape, nan, dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the basis matrix
@pytest.mark.parametrize("convention", oracle.CONVENTIONS)
@pytest.mark.parametrize("lmax", oracle.MATRIX_LMAX)
def test_matrix_at_the_golden_points(lmax, convention):
    g = golden()
    th, ph = oracle.golden_points(g)
    name = "a/%s_l%d" % (convention, lmax)
    want = g[name] if name in g else oracle.matrix(th, ph, lmax, convention)
    got = basis(4, 8, lmax, "reference", convention).matrix(th, ph)
    assert bool(torch.isfinite(got).all())
    check(got, want, FLOOR["matrix"][convention][lmax], "matrix %s lmax %d" % (convention, lmax))


@pytest.mark.parametrize("convention", oracle.CONVENTIONS)
def test_matrix_on_the_reference_grid_and_its_poles(convention):
    """12 x 24 at lmax 32: 7 points per workgroup, 42 workgroups, the last with one point; every entry finite (the
    unnormalised form would leave float32 at m = 32); the rows of theta = 0 and theta = pi hold exact zeros in every m != 0
    column and one value along phi in the m = 0 columns."""
    H, W, lmax = 12, 24, 32
    got = basis(H, W, lmax, "reference", convention).matrix()
    assert got.shape == (H * W, 1089) and bool(torch.isfinite(got).all())
    check(got, want_matrix(H, W, lmax, "reference", convention), FLOOR["matrix"][convention][lmax], "grid matrix " + convention)
    zonal = torch.tensor([l * l + l for l in range(lmax + 1)], device="cuda")
    other = torch.tensor([k for k in range(1089) if k not in set(zonal.tolist())], device="cuda")
    for pole in (got[:W], got[-W:]):
        assert bool((pole[:, other] == 0).all()), "an m != 0 column is not exactly zero at a pole"
        assert all(torch.equal(pole[0, zonal], pole[i, zonal]) for i in range(1, W)), "an m = 0 column varies along phi at a pole"
        assert bool((pole[:, zonal] != 0).all())


# ------------------------------------------------------------------------------------------------ 2. analysis, 3. synthesis
@pytest.mark.parametrize("H,W,lmax,convention", oracle.GOLDEN_GRIDS)
def test_analysis_against_the_reference_coefficients(H, W, lmax, convention):
    g = golden()
    got = basis(H, W, lmax, "reference", convention).analysis(dev(g["c/%s/image" % key(H, W, lmax)]))
    check(got, g["c/%s/coeffs" % key(H, W, lmax)], floor_of("analysis", H, W, lmax, 2, "golden"), "analysis golden " + key(H, W, lmax))


@pytest.mark.parametrize("H,W,lmax,B", oracle.CASES)
def test_analysis_against_the_oracle(H, W, lmax, B):
    """The reference grid with the solid angles and the centres grid without them, each against its own floor."""
    x, xd = image(B, H, W), dev(image(B, H, W))
    poison(basis(H, W, lmax), B)
    check(basis(H, W, lmax).analysis(xd), want_coeffs(B, H, W, lmax), floor_of("analysis", H, W, lmax, B),
          "analysis %s B %d" % (key(H, W, lmax), B))
    poison(basis(H, W, lmax, "centres"), B)
    got = basis(H, W, lmax, "centres").analysis(xd, weighted=False)
    check(got, oracle.analysis(x, want_matrix(H, W, lmax, "centres")), floor_of("analysis_centres", H, W, lmax, B),
          "analysis %s B %d centres unweighted" % (key(H, W, lmax), B))


@pytest.mark.parametrize("H,W,lmax,B", oracle.CASES)
def test_synthesis_against_the_oracle(H, W, lmax, B):
    co = want_coeffs(B, H, W, lmax).astype(np.float32)
    hb, M, cd = basis(H, W, lmax), want_matrix(H, W, lmax), dev(co)
    poison(hb, B)
    check(hb.synthesis(cd), oracle.synthesis(co, M, H, W), floor_of("synthesis", H, W, lmax, B),
          "synthesis %s B %d" % (key(H, W, lmax), B))
    poison(hb, B)
    check(hb.synthesis(cd, weighted=True), oracle.synthesis(co, M, H, W, oracle.solid_angles(H, W)),
          floor_of("synthesis_weighted", H, W, lmax, B), "weighted synthesis %s B %d" % (key(H, W, lmax), B))
    hc = basis(H, W, lmax, "centres")
    poison(hc, B)
    check(hc.synthesis(cd), oracle.synthesis(co, want_matrix(H, W, lmax, "centres"), H, W), floor_of("synthesis_centres", H, W, lmax, B),
          "synthesis %s B %d centres" % (key(H, W, lmax), B))


# ------------------------------------------------------------------------------------------------ 4. adjoints and gradients
@pytest.mark.parametrize("H,W,lmax,B", oracle.ADJOINT_CASES)
def test_adjoint_identity_and_autograd(H, W, lmax, B):
    hb, M, w = basis(H, W, lmax), want_matrix(H, W, lmax), oracle.solid_angles(H, W)
    k, seeds = "%s B %d" % (key(H, W, lmax), B), oracle.ADJOINT_SEEDS
    f_x, f_up = floor_of("analysis", H, W, lmax, B, seeds["x"]), floor_of("analysis", H, W, lmax, B, seeds["up"])
    f_up_plain = floor_of("analysis_unweighted", H, W, lmax, B, seeds["up"])
    f_g = floor_of("synthesis_weighted", H, W, lmax, B, seeds["g"])
    x, g = image(B, H, W, seed=seeds["x"]), want_coeffs(B, H, W, lmax, seed=seeds["g"]).astype(np.float32)
    xt, gt = dev(x).requires_grad_(True), dev(g)
    c = hb.analysis(xt)
    (c * gt).sum().backward()
    check(xt.grad, oracle.synthesis(g, M, H, W, w), f_g, "d analysis / d pano " + k)       # A^T g: the weighted synthesis
    c64, dx64 = c.detach().cpu().numpy().astype(np.float64), xt.grad.cpu().numpy().astype(np.float64)
    lhs, rhs = float((c64 * g).sum()), float((x.astype(np.float64) * dx64).sum())
    bound = MARGIN * (f_x * np.abs(c64).max() * np.abs(g).sum() + f_g * np.abs(dx64).max() * np.abs(x).sum())
    print("adjoint %s: <Ax, g> %.9e <x, A^T g> %.9e diff %.3e bound %.3e" % (k, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    ct, up = dev(g).requires_grad_(True), image(B, H, W, seed=seeds["up"])
    (hb.synthesis(ct) * dev(up)).sum().backward()
    check(ct.grad, oracle.analysis(up, M), f_up_plain, "d synthesis / d coeffs " + k)
    ct2 = dev(g).requires_grad_(True)
    (hb.synthesis(ct2, weighted=True) * dev(up)).sum().backward()
    check(ct2.grad, oracle.analysis(up, M, w), f_up, "d weighted synthesis / d coeffs " + k)


# ------------------------------------------------------------------------------------------------ 5. exactness
def test_an_image_is_treated_the_same_in_any_batch_and_run():
    """Image 5 of a batch of 11 has its planes 15..17 in plane groups 1 and 2 (groups of 8); alone it lies in group 0, and in the
    batch of four at position 1 in group 0 as well, at other lanes."""
    for H, W, lmax in ((16, 32, 12), (9, 133, 16)):
        hb = basis(H, W, lmax)
        x = dev(image(11, H, W, seed=4))
        poison(hb, 11)
        c11 = hb.analysis(x)
        assert bool(torch.isfinite(c11).all())
        assert torch.equal(c11, hb.analysis(x)), "two runs differ"
        assert torch.equal(c11[5:6], hb.analysis(x[5:6].contiguous())), "alone"
        perm = torch.tensor([7, 5, 0, 10], device="cuda")
        assert torch.equal(c11[perm], hb.analysis(x[perm].contiguous())), "at another batch position"
        poison(hb, 11)
        r11 = hb.synthesis(c11)
        assert bool(torch.isfinite(r11).all())
        assert torch.equal(r11, hb.synthesis(c11)) and torch.equal(r11[5:6], hb.synthesis(c11[5:6].contiguous()))
        assert torch.equal(r11[perm], hb.synthesis(c11[perm].contiguous()))


# ------------------------------------------------------------------------------------------------ 6. cross-checks
@pytest.mark.parametrize("H,W,lmax,B", [(12, 24, 4, 2), (25, 47, 8, 2)])
def test_the_matrix_path_and_the_separable_path_agree(H, W, lmax, B):
    """``analysis`` against ``matrix()^T (w * pano)`` taken in float64 of the float32 matrix: the two paths differ by the
    matrix tolerance (relative to the largest entry, carried through a sum of nonnegative terms) plus the analysis one."""
    hb, w = basis(H, W, lmax), oracle.solid_angles(H, W)
    x = image(B, H, W)
    via_matrix = oracle.analysis(x, hb.matrix().cpu().numpy().astype(np.float64), w)
    conv = oracle.convention_of(lmax)
    carried = FLOOR["matrix"][conv][lmax] * float(np.abs(want_matrix(H, W, lmax)).max() * (x.reshape(B, 3, -1) * w).sum(2).max()
                                                  / np.abs(via_matrix).max())
    check(hb.analysis(dev(x)), via_matrix, floor_of("analysis", H, W, lmax, B), "separable vs matrix " + key(H, W, lmax),
          MARGIN * carried)


def test_round_trip_on_the_centres_grid_equals_the_oracles():
    """synthesis(analysis(x)) on "centres" against the oracle's round trip, not against x: the quadrature error is not rounding.
    Both floors are measured here, on this grid and this input."""
    H, W, lmax, B = oracle.ROUND_TRIP_CASE
    hb, M, w = basis(H, W, lmax, "centres"), want_matrix(H, W, lmax, "centres"), oracle.solid_angles(H, W)
    x = image(B, H, W)
    c64 = oracle.analysis(x, M, w)
    c = hb.analysis(dev(x))
    conv = oracle.convention_of(lmax)
    f_a = oracle.analysis_floor(x, lmax, conv, grid="centres")
    f_s = oracle.synthesis_floor(c64.astype(np.float32), H, W, lmax, conv, grid="centres")
    check(c, c64, f_a, "round trip: analysis")
    # the synthesis is linear: the analysis' error reaches the image through at most sum_k |Y_k| per pixel
    carried = MARGIN * f_a * float(np.abs(c64).max() * np.abs(M).sum(1).max() / np.abs(oracle.synthesis(c64, M, H, W)).max())
    check(hb.synthesis(c), oracle.synthesis(c64, M, H, W), f_s, "round trip: synthesis", carried)


def transform_tolerance(lmax, jmax, conv):
    """(T, dT): the float64 transform and the largest error an entry of the product's may have: an entry is a matrix entry
    (within ``4 x`` the matrix floor of the largest entry of Y at the centres) times a scale of at most sqrt(4 pi / 12), the
    scale rounded to float32 and the product rounded once more."""
    T = oracle.needlet_transform(lmax, jmax, conv)
    cen = needlet_oracle.centres(jmax)[1:]
    Y = oracle.matrix(np.arccos(np.clip(cen[:, 2], -1.0, 1.0)), np.arctan2(cen[:, 1], cen[:, 0]), lmax, conv)
    dT = MARGIN * FLOOR["matrix"][conv][lmax] * float(np.abs(Y).max()) * np.sqrt(4 * np.pi / 12) + 2.0 ** -23 * float(np.abs(T).max())
    return T, dT


@pytest.mark.parametrize("lmax,jmax", [(4, 1), (8, 1), (32, 4)])
def test_to_needlets_against_the_oracle(lmax, jmax):
    """Degrees beyond 2^(jmax+1) = 4 are dropped at lmax 8.  The result's error is the transform's, carried through the sum
    over the K columns, plus the float32 matmul's own rounding (K terms)."""
    H, W, B = 12, 24, 2
    conv = oracle.convention_of(lmax)
    hb = basis(H, W, lmax)
    co = want_coeffs(B, H, W, lmax).astype(np.float32)
    T, dT = transform_tolerance(lmax, jmax, conv)
    got_T = hb.needlet_transform(jmax)
    assert float(got_T[0, 0]) == 1.0 and bool((got_T[0, 1:] == 0).all())
    check(got_T, T, 0.0, "needlet transform lmax %d jmax %d" % (lmax, jmax), dT / float(np.abs(T).max()))
    want = oracle.to_needlets(co, lmax, jmax, conv)
    bound = (dT + hb.K * 2.0 ** -24 * float(np.abs(T).max())) * float(np.abs(co).sum(1).max() / np.abs(want).max())
    got = hb.to_needlets(dev(co), jmax)
    assert got.shape == (B, needlet_oracle.rows(jmax), 3)
    check(got, want, 0.0, "to_needlets lmax %d jmax %d" % (lmax, jmax), bound)


@pytest.mark.parametrize("jmax", [1, 4])
def test_the_needlet_matrix_through_the_harmonics(jmax):
    """``Y(x) T^T`` with ``lmax = 2^(jmax+1)`` is ``NeedletBasis.matrix``: two float32 evaluations of one function.  The product
    (taken in float64 of the float32 factors) errs by at most ``dY max_n sum_k |T_nk| + dT max_p sum_k |Y_pk|``; the needlet
    side keeps its own tolerance (the floors of ``test_gpu_needlets.py``)."""
    from emlight_amd.needlets import NeedletBasis
    from tests.test_gpu_needlets import FLOOR as NEEDLET_FLOOR
    H, W, L = 6, 12, 2 ** (jmax + 1)
    hb = basis(H, W, L, "centres", "graphics")
    got = (hb.matrix().double() @ hb.needlet_transform(jmax).double().T).cpu().numpy()
    nb = NeedletBasis(jmax=jmax, height=H, width=W, grid="centres", device="cuda").matrix().cpu().numpy()
    want = needlet_oracle.matrix(*needlet_oracle.grid_angles(H, W, "centres"), jmax)
    Y64 = want_matrix(H, W, L, "centres", "graphics")
    T64, dT = transform_tolerance(L, jmax, "graphics")
    dY = MARGIN * FLOOR["matrix"]["graphics"][L] * float(np.abs(Y64).max())
    carried = (dY * float(np.abs(T64).sum(1).max()) + dT * float(np.abs(Y64).sum(1).max())) / float(np.abs(want).max())
    check(got, want, 0.0, "harmonic route vs needlet oracle jmax %d" % jmax, carried)
    check(got, nb.astype(np.float64), NEEDLET_FLOOR["matrix"][jmax], "harmonic route vs NeedletBasis jmax %d" % jmax, carried)


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_command_line_on_the_device(tmp_path):
    """``python -m emlight_amd.harmonics`` over three 8 x 16 panoramas at ``--height 4``, ``--batchSize 2`` (a full batch and a
    ragged one), in both conventions, against the direct call on the batcher's own output (``torch.equal``: the same kernel
    on the same input, whatever the batch) and against the float64 oracle of that input.  The exact comparison holds with
    the alpha too: the test takes it from one batch of three, the program from batches of two and one, and ``tone`` treats
    every image on its own (``test_gpu_panorama_prep.py`` holds it to that bit for bit)."""
    from emlight_amd import harmonics, needlets
    H, W, lmax, fov = 4, 8, 4, 60.0
    panos, names = tmp_path / "panos", ["a", "b", "c"]
    panos.mkdir()
    raw = oracle.hdr_image(3, 2 * H, 2 * W, seed=7).transpose(0, 2, 3, 1)
    for name, p in zip(reversed(names), raw):                                        # written c, b, a: read back sorted
        np.save(str(panos / (name + ".npy")), p)
    batcher = needlets._batcher(fov, "cuda")
    batcher.PANO_HW = (H, W)
    on_dev = torch.from_numpy(np.ascontiguousarray(raw[::-1])).cuda()
    small = batcher.small(on_dev, 0.0).permute(0, 3, 1, 2).contiguous()
    alpha = batcher.tone(batcher.crop(on_dev, 0.0, fov))[1]
    common = ["--pano_dir", str(panos), "--lmax", str(lmax), "--height", str(H), "--fov", str(fov), "--batchSize", "2"]
    for tag, extra, conv, x in (("no_alpha", ["--no_alpha"], "graphics", small),
                                ("alpha", ["--convention", "symmetrised"], "symmetrised", small * alpha.reshape(-1, 1, 1, 1))):
        out = tmp_path / tag
        assert harmonics.main(common + ["--out_dir", str(out)] + extra) == names
        got = np.stack([np.load(str(out / (n + ".npy"))) for n in names])
        assert got.dtype == np.float32 and got.shape == (3, 25, 3)
        direct = basis(H, W, lmax, "reference", conv).analysis(x.contiguous())
        assert np.array_equal(got, direct.cpu().numpy()), tag
        xn = x.cpu().numpy()
        check(got, oracle.analysis(xn, want_matrix(H, W, lmax, "reference", conv), oracle.solid_angles(H, W)),
              oracle.analysis_floor(xn, lmax, conv), "command line, %s" % tag)
