"""The definition of the real spherical harmonics in the reference's two conventions, their analysis / synthesis and the
change of basis to the needlets, restated in numpy float64.  A helper of ``test_gpu_harmonics.py`` /
``test_harmonics_abi.py``, not a test.  Nothing here looks at the product code: the Legendre functions carry their
``sin^m`` factor through the sectoral seed, and the azimuth is ``cos(m phi)`` / ``sin(m phi)`` of the angle itself rather than
a power of ``x + i y``.  ``float32_floors`` is the other thing: the kernels' own arithmetic, rounded to float32 step by step."""
import functools

import numpy as np

from tests import needlet_oracle as nd

CONVENTIONS = ("graphics", "symmetrised")
grid_angles, solid_angles, hdr_image, rel_err = nd.grid_angles, nd.solid_angles, nd.hdr_image, nd.rel_err
analysis, synthesis = nd.analysis, nd.synthesis


def terms(lmax):
    return (lmax + 1) ** 2


def legendre(theta, lmax):
    """Ybar[..., l, m]: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(cos theta) with the Condon-Shortley phase, 0 <= m <= l."""
    theta = np.asarray(theta, dtype=np.float64)
    z, s = np.cos(theta), np.sin(theta)
    out = np.zeros(theta.shape + (lmax + 1, lmax + 1))
    out[..., 0, 0] = 1.0 / np.sqrt(4.0 * np.pi)
    for m in range(1, lmax + 1):
        out[..., m, m] = -np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * out[..., m - 1, m - 1]
    for m in range(lmax + 1):
        for l in range(m + 1, lmax + 1):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            out[..., l, m] = a * (z * out[..., l - 1, m] - (b * out[..., l - 2, m] if l >= m + 2 else 0.0))
    return out


def column_table(lmax, convention):
    """Per column k = l^2 + l + mm: (l, |mm|, 0 for the cos part / 1 for the sin part, signed scale)."""
    assert convention in CONVENTIONS
    out = []
    for l in range(lmax + 1):
        for mm in range(-l, l + 1):
            m = abs(mm)
            if mm == 0:
                out.append((l, 0, 0, 1.0))
            elif convention == "graphics":                   # shEvaluate: m > 0 sqrt(2) cos, m < 0 sqrt(2) sin
                out.append((l, m, 0 if mm > 0 else 1, np.sqrt(2.0)))
            else:                                            # spharmonic: m < 0 sqrt(2) cos, m > 0 (-1)^m sqrt(2) sin
                out.append((l, m, 0, np.sqrt(2.0)) if mm < 0 else (l, m, 1, (-1.0) ** m * np.sqrt(2.0)))
    return out


def matrix(theta, phi, lmax, convention="graphics"):
    """(P, K) at the given angles."""
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    Y = legendre(theta, lmax)
    out = np.empty((theta.shape[0], terms(lmax)))
    for k, (l, m, part, scale) in enumerate(column_table(lmax, convention)):
        out[:, k] = scale * Y[:, l, m] * (np.sin(m * phi) if part else np.cos(m * phi))
    return out


def conversion(lmax):
    """(perm, sign): ``matrix(.., "symmetrised") == matrix(.., "graphics")[:, perm] * sign`` -- column (l, m) of the one is
    column (l, -m) of the other, times (-1)^m for m > 0."""
    perm, sign = [], []
    for l in range(lmax + 1):
        for mm in range(-l, l + 1):
            perm.append(l * l + l - mm)
            sign.append((-1.0) ** mm if mm > 0 else 1.0)
    return np.array(perm), np.array(sign)


def needlet_transform(lmax, jmax, convention="graphics"):
    """(K_needlets, K): row 0 passes Y_00 through; the row of needlet jk is sqrt(lambda_j) b(l / 2^j) Y_lm(xi_jk)."""
    cen, win = nd.centres(jmax), nd.window(jmax)               # win[j, l - 1] = b(l / 2^j), l = 1..2^(jmax+1)
    T = np.zeros((nd.rows(jmax), terms(lmax)))
    T[0, 0] = 1.0
    theta, phi = np.arccos(np.clip(cen[1:, 2], -1.0, 1.0)), np.arctan2(cen[1:, 1], cen[1:, 0])
    Y = matrix(theta, phi, lmax, convention)
    for j, sl in enumerate(nd.level_slices(jmax)[1:]):
        scale = np.zeros(terms(lmax))
        lam = 4.0 * np.pi / (sl.stop - sl.start)               # equal weights over the needlet oracle's own centres
        for l in range(1, min(lmax, win.shape[1]) + 1):
            scale[l * l:(l + 1) ** 2] = np.sqrt(lam) * win[j, l - 1]
        T[sl] = Y[sl.start - 1:sl.stop - 1] * scale
    return T


def to_needlets(coeffs, lmax, jmax, convention="graphics"):
    return np.einsum("nk,bkc->bnc", needlet_transform(lmax, jmax, convention), np.asarray(coeffs, dtype=np.float64))


def needlet_matrix_through_harmonics(theta, phi, jmax):
    """The link between the two representations: [Y_00, Y(x) diag(sqrt(lambda_j) b(l / 2^j)) Y(xi_j)^T] is the needlet matrix
    (the addition theorem; any one convention on both sides)."""
    L = 2 ** (jmax + 1)
    return matrix(theta, phi, L) @ needlet_transform(L, jmax).T


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic, float32
F = np.float32
ROWS, PLANES, CHUNK, WAVES = 8, 8, 128, 4                      # the kernels' tiling: see csrc/harmonics.hip


def fma(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def tables_f32(convention):
    d = np.empty(33)
    d[0] = 1.0 / np.sqrt(4.0 * np.pi)
    for m in range(1, 33):
        d[m] = -np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * d[m - 1]
    a, b = np.zeros((33, 33)), np.zeros((33, 33))
    for m in range(33):
        for l in range(m + 1, 33):
            a[m, l] = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b[m, l] = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
    sc, ss = np.full(33, np.sqrt(2.0)), np.full(33, np.sqrt(2.0))
    sc[0], ss[0] = 1.0, 0.0
    if convention == "symmetrised":
        ss[1:] *= (-1.0) ** np.arange(1, 33)
    return d.astype(F), a.astype(F), b.astype(F), sc.astype(F), ss.astype(F), (1 if convention == "graphics" else -1)


def _recurrence(z, m, lmax, d, a, b):
    """[q_m .. q_lmax] of the kernels' recurrence for Ybar_l^m / sin^m, float32 arrays shaped like z."""
    q0, q1, out = np.zeros_like(z), np.full_like(z, d[m]), []
    for l in range(m, lmax + 1):
        if l > m:
            q0, q1 = q1, a[m, l] * fma(z, q1, -(b[m, l] * q0))
        out.append(q1)
    return out


def directions_f32(theta, phi):
    """Unit vectors as the product makes them: the sine of the distance to the nearer pole, then rounded to float32."""
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    s = np.sin(np.minimum(theta, np.pi - theta))
    return np.stack([s * np.cos(phi), s * np.sin(phi), np.cos(theta)], -1).astype(F)


def matrix_f32(theta, phi, lmax, convention="graphics"):
    """eml_sh_basis_f32 in numpy float32."""
    d, a, b, sc, ss, dr = tables_f32(convention)
    x, y, z = directions_f32(theta, phi).T
    out = np.zeros((x.shape[0], terms(lmax)), dtype=F)
    re, im = np.ones_like(x), np.zeros_like(x)
    for m in range(lmax + 1):
        if m:
            re, im = fma(re, x, -(im * y)), fma(re, y, im * x)
        fc, fs = re * sc[m], im * ss[m]
        for l, q in zip(range(m, lmax + 1), _recurrence(z, m, lmax, d, a, b)):
            out[:, l * l + l + dr * m] = q * fc
            if m:
                out[:, l * l + l - dr * m] = q * fs
    return out


def grid_tables_f32(H, W, grid):
    th, ph = grid_angles(H, W, grid)
    th, ph = th[::W], ph[:W]
    arg = ph[:, None] * np.arange(33)[None, :]
    four = np.stack([np.cos(arg), np.sin(arg)], 2).astype(F)
    return np.cos(th).astype(F), np.sin(np.minimum(th, np.pi - th)).astype(F), four, solid_angles(H, W)[::W].astype(F)


def _row_factors(H, W, lmax, grid, convention, weighted):
    """lam (H, K) and, per column, (order, part): the kernels' ``row_factors``."""
    d, a, b, sc, ss, dr = tables_f32(convention)
    z, s, _, w = grid_tables_f32(H, W, grid)
    if not weighted:
        w = np.ones_like(w)
    lam = np.zeros((H, terms(lmax)), dtype=F)
    order, part = np.zeros(terms(lmax), dtype=int), np.zeros(terms(lmax), dtype=int)
    sm = np.ones_like(s)
    for m in range(lmax + 1):
        if m:
            sm = sm * s
        fc, fs = sm * sc[m] * w, sm * ss[m] * w
        for l, q in zip(range(m, lmax + 1), _recurrence(z, m, lmax, d, a, b)):
            kc, ks = l * l + l + dr * m, l * l + l - dr * m
            lam[:, kc], order[kc], part[kc] = q * fc, m, 0
            if m:
                lam[:, ks], order[ks], part[ks] = q * fs, m, 1
    return lam, order, part


def analysis_f32(im, lmax, grid="reference", convention="graphics", weighted=True):
    """eml_sh_analysis_f32 in numpy float32: each wave's Fourier sums over its 32 columns of every chunk of 128, the four
    waves added in order, times the rows' factors and summed over the 8 rows of a block, the blocks added in order."""
    im = np.asarray(im, dtype=F)
    B, _, H, W = im.shape
    px = im.reshape(3 * B, H, W)
    four = grid_tables_f32(H, W, grid)[2]
    Fsum = None
    for q in range(WAVES):
        acc = np.zeros((3 * B, H, 33, 2), dtype=F)
        for x0 in range(0, W, CHUNK):
            for x in range(x0 + q * 32, min(x0 + q * 32 + 32, W)):
                acc = fma(px[:, :, x, None, None], four[x], acc)
        Fsum = acc if Fsum is None else Fsum + acc
    lam, order, part = _row_factors(H, W, lmax, grid, convention, weighted)
    Fk = Fsum[:, :, order, part]                                # (N, H, K)
    total = np.zeros((3 * B, terms(lmax)), dtype=F)
    for y0 in range(0, H, ROWS):
        s = np.zeros_like(total)
        for y in range(y0, min(y0 + ROWS, H)):
            s = fma(lam[y], Fk[:, y], s)
        total = total + s
    return total.reshape(B, 3, -1).transpose(0, 2, 1)


def synthesis_f32(co, H, W, lmax, grid="reference", convention="graphics", weighted=False):
    """eml_sh_synthesis_f32 in numpy float32: the Legendre sums in order of l, then the Fourier sum in order of m."""
    co = np.asarray(co, dtype=F)
    B = co.shape[0]
    c = co.transpose(0, 2, 1).reshape(3 * B, -1)                # (N, K)
    dr = 1 if convention == "graphics" else -1
    four = grid_tables_f32(H, W, grid)[2]
    lam = _row_factors(H, W, lmax, grid, convention, weighted)[0]
    rec = None
    for m in range(lmax + 1):
        for sn in ((0,) if m == 0 else (0, 1)):
            g = np.zeros((3 * B, H), dtype=F)
            for l in range(m, lmax + 1):
                k = l * l + l + (-dr * m if sn else dr * m)
                g = fma(lam[None, :, k], c[:, None, k], g)
            if rec is None:
                rec = g[:, :, None] * four[None, None, :, 0, 0]
            else:
                rec = fma(g[:, :, None], four[None, None, :, m, sn], rec)
    return rec.reshape(B, 3, H, W)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# A case is (H, W, lmax, B); test_gpu_harmonics.py says which boundary of the kernels' tiling each shape hits.
GOLDEN_POINTS = {"symmetrised": (1, 4, 32), "graphics": (4, 8)}         # (a): lmax per convention
GOLDEN_GRIDS = [(12, 24, 4, "symmetrised"), (16, 32, 8, "graphics")]    # (c): B = 2
MATRIX_LMAX = [0, 1, 4, 8, 32]
CASES = [(3, 5, 4, 2), (4, 8, 1, 1), (12, 24, 4, 2), (25, 47, 8, 2), (64, 128, 32, 1), (12, 24, 0, 3), (12, 24, 4, 11),
         (12, 24, 4, 33), (9, 133, 16, 3)]
ADJOINT_CASES = [(12, 24, 4, 2), (25, 47, 8, 3), (9, 133, 16, 3)]
ADJOINT_SEEDS = {"x": 1, "g": 2, "up": 3}
ROUND_TRIP_CASE = (16, 32, 4, 2)                                         # on "centres"


def convention_of(lmax):
    """The convention the analysis / synthesis cases of degree ``lmax`` run in (the matrix tests run both at every degree)."""
    return "symmetrised" if lmax in (1, 8) else "graphics"


def floor_key(H, W, lmax, B, source=0):
    tail = "_" + source if isinstance(source, str) else ("" if source == 0 else "_s%d" % source)
    return "%dx%d_l%d_b%d%s" % (H, W, lmax, B, tail)


# quantity -> (operation, grid, with the solid angles)
QUANTITIES = {"analysis": ("analysis", "reference", True), "analysis_unweighted": ("analysis", "reference", False),
              "analysis_centres": ("analysis", "centres", False), "synthesis": ("synthesis", "reference", False),
              "synthesis_weighted": ("synthesis", "reference", True), "synthesis_centres": ("synthesis", "centres", False)}


def floor_cases():
    """Every input a GPU test holds against an analysis or a synthesis tolerance, per quantity of ``QUANTITIES``:
    (H, W, lmax, B, source).  A gradient is the other operation on the upstream gradient: the weighted synthesis of the
    coefficient-like ``g``, the unweighted and the weighted analysis of the image-like ``up``."""
    cases = [c + (0,) for c in CASES]
    out = {"analysis": [(H, W, l, 2, "golden") for H, W, l, _ in GOLDEN_GRIDS] + cases, "analysis_unweighted": [],
           "analysis_centres": list(cases), "synthesis": list(cases), "synthesis_weighted": list(cases),
           "synthesis_centres": list(cases)}
    for c in ADJOINT_CASES:
        out["analysis"] += [c + (ADJOINT_SEEDS["x"],), c + (ADJOINT_SEEDS["up"],)]
        out["analysis_unweighted"] += [c + (ADJOINT_SEEDS["up"],)]
        out["synthesis_weighted"] += [c + (ADJOINT_SEEDS["g"],)]
    return out


@functools.lru_cache(maxsize=None)
def grid_matrix(H, W, lmax, grid="reference", convention="graphics"):
    return matrix(*grid_angles(H, W, grid), lmax, convention)


def coefficients_of(H, W, lmax, B, seed=0):
    """The float64 weighted analysis of the seeded image on the reference grid: the tests' coefficient-like data."""
    return analysis(hdr_image(B, H, W, seed), grid_matrix(H, W, lmax, "reference", convention_of(lmax)), solid_angles(H, W))


def analysis_floor(im, lmax, convention, want=None, grid="reference", weighted=True):
    """``analysis_f32`` of ``im`` (B, 3, H, W) against ``want`` (default: the float64 analysis of the same image)."""
    H, W = im.shape[2:]
    if want is None:
        want = analysis(im, grid_matrix(H, W, lmax, grid, convention), solid_angles(H, W) if weighted else None)
    return rel_err(analysis_f32(im, lmax, grid, convention, weighted), want)


def synthesis_floor(co, H, W, lmax, convention, grid="reference", weighted=False):
    """``synthesis_f32`` of float32 coefficients ``co`` (B, K, 3) against the float64 one."""
    return rel_err(synthesis_f32(co, H, W, lmax, grid, convention, weighted),
                   synthesis(co, grid_matrix(H, W, lmax, grid, convention), H, W, solid_angles(H, W) if weighted else None))


def golden_points(golden):
    return golden["a/theta"], golden["a/phi"]


def float32_floors(golden):
    """The float32 floors behind the GPU tolerances (test_gpu_harmonics.py), as max|error| / max|value|:
    * matrix[convention][lmax]: ``matrix_f32`` at the golden file's points against the golden (a) where the file holds that
      (convention, lmax), against this file's float64 (which equals the golden to 1e-9) elsewhere;
    * the analysis quantities: ``analysis_f32`` of the golden image against golden (c), of every other image against this
      file's float64, on the grid and with or without the solid angles as ``QUANTITIES`` says;
    * the synthesis quantities: ``synthesis_f32`` of the float32-rounded float64 coefficients of that image (its weighted
      analysis on the reference grid) against this file's float64."""
    floors = {"matrix": {c: {} for c in CONVENTIONS}}
    th, ph = golden_points(golden)
    for conv in CONVENTIONS:
        for lmax in MATRIX_LMAX:
            name = "a/%s_l%d" % (conv, lmax)
            want = golden[name] if name in golden else matrix(th, ph, lmax, conv)
            floors["matrix"][conv][lmax] = rel_err(matrix_f32(th, ph, lmax, conv), want)
    conv_of_golden = {(H, W, l): c for H, W, l, c in GOLDEN_GRIDS}
    for quantity, cases in floor_cases().items():
        operation, grid, weighted = QUANTITIES[quantity]
        table = floors[quantity] = {}
        for H, W, lmax, B, source in cases:
            if source == "golden":
                name = "c/%dx%d_l%d" % (H, W, lmax)
                v = analysis_floor(golden[name + "/image"], lmax, conv_of_golden[(H, W, lmax)], golden[name + "/coeffs"])
            elif operation == "analysis":
                v = analysis_floor(hdr_image(B, H, W, source), lmax, convention_of(lmax), None, grid, weighted)
            else:
                v = synthesis_floor(coefficients_of(H, W, lmax, B, source).astype(F), H, W, lmax, convention_of(lmax), grid, weighted)
            table[floor_key(H, W, lmax, B, source)] = v
    return floors
