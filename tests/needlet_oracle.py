"""The definition of the needlet basis, its analysis / synthesis and the sparsify rule, restated in
numpy float64.  A helper of ``test_gpu_needlets.py`` / ``test_needlets_abi.py``, not a test.  Nothing here looks at the
product code: HEALPix comes from the pixel-index formulae (Gorski et al. 2005, eqs. 2-9) rather than ring by ring, and the
zonal sum is numpy's Clenshaw ``legval`` rather than the kernels' forward recurrence."""
import functools

import numpy as np
from numpy.polynomial import legendre


def rows(jmax):
    return 4 ** (jmax + 2) - 3


def level_slices(jmax):
    out, s = [slice(0, 1)], 1
    for j in range(jmax + 1):
        out.append(slice(s, s + 12 * 4 ** j))
        s += 12 * 4 ** j
    return out


def pix2zphi(nside, p):
    """z and phi of RING pixel p (one pixel; the published index formulae)."""
    n, npix = nside, 12 * nside * nside
    ncap = 2 * n * (n - 1)
    if p < ncap:                                               # north cap
        i = int((1 + np.sqrt(1 + 2 * p)) / 2)
        while 2 * i * (i - 1) > p:
            i -= 1
        while 2 * i * (i + 1) <= p:
            i += 1
        k = p - 2 * i * (i - 1)
        return 1.0 - i * i / (3.0 * n * n), (k + 0.5) * np.pi / (2.0 * i)
    if p < npix - ncap:                                        # belt
        q = p - ncap
        i, k = q // (4 * n) + n, q % (4 * n)
        s = (i - n + 1) % 2
        return 4.0 / 3.0 - 2.0 * i / (3.0 * n), (k + 0.5 * s) * np.pi / (2.0 * n)
    z, phi = pix2zphi(nside, npix - 1 - p)                     # south cap: the point mirror of the north cap, read backwards
    return -z, 2.0 * np.pi - phi


def ring_centres(nside):
    zp = np.array([pix2zphi(nside, p) for p in range(12 * nside * nside)])
    s = np.sqrt(1.0 - zp[:, 0] ** 2)
    return np.stack([s * np.cos(zp[:, 1]), s * np.sin(zp[:, 1]), zp[:, 0]], 1)


def centres(jmax):
    """(K, 3): row 0 (Y_00) has no centre (zeros), then the levels' pixel centres."""
    return np.concatenate([np.zeros((1, 3))] + [ring_centres(2 ** j) for j in range(jmax + 1)], 0)


def f2(u, nodes=240):
    x, w = legendre.leggauss(nodes)

    def integral(hi):
        t = -1.0 + (x + 1.0) * (hi + 1.0) / 2.0
        return (hi + 1.0) / 2.0 * np.sum(w * np.exp(-1.0 / (1.0 - t * t)))
    return integral(min(u + 1e-10, 1.0)) / integral(1.0)


def f3(x):
    return 1.0 if x <= 0.5 else (f2(1.0 - 4.0 * (x - 0.5)) if x <= 1.0 else 0.0)


def window(jmax):
    """b_vector of sphere_needlets.py:40-43 with lmax = 2^(jmax+1): (jmax + 1, lmax), entry [j, l - 1] = b(l / 2^j)."""
    L = 2 ** (jmax + 1)
    return np.array([[np.sqrt(max(f3(l / 2.0 ** j / 2.0) - f3(l / 2.0 ** j), 0.0)) for l in range(1, L + 1)]
                     for j in range(jmax + 1)])


def zonal_coefficients(jmax):
    """One Legendre series per table row: Y_00, then sqrt(lambda_j) b(l / 2^j) (2l + 1) / 4 pi."""
    b = window(jmax)
    L = b.shape[1]
    out = np.zeros((jmax + 2, L + 1))
    out[0, 0] = 1.0 / np.sqrt(4.0 * np.pi)
    l = np.arange(1, L + 1)
    for j in range(jmax + 1):
        out[j + 1, 1:] = np.sqrt(4.0 * np.pi / (12 * 4 ** j)) * b[j] * (2 * l + 1) / (4.0 * np.pi)
    return out


def directions(theta, phi):
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)


def matrix(theta, phi, jmax):
    """(P, K): [Y_00, psi_0., ..., psi_jmax.] at the given angles."""
    x = directions(theta, phi)
    c, cen = zonal_coefficients(jmax), centres(jmax)
    out = np.empty((x.shape[0], rows(jmax)))
    for row, sl in enumerate(level_slices(jmax)):
        out[:, sl] = legendre.legval(np.clip(x @ cen[sl].T, -1.0, 1.0), c[row])
    return out


def grid_angles(H, W, grid="reference"):
    if grid == "reference":                                    # mat_gen2.py:22-25
        th, ph = np.linspace(0, 1, H) * np.pi, np.linspace(0, 2, W) * np.pi
    else:
        th, ph = (np.arange(H) + 0.5) * np.pi / H, (np.arange(W) + 0.5) * 2 * np.pi / W
    X, Y = np.meshgrid(ph, th)
    return Y.reshape(-1), X.reshape(-1)


def solid_angles(H, W):
    """getSolidAngleMap (Needlets/utils.py:35-50), flattened; its height is W / 2 there, H here."""
    y = np.arange(H)
    theta = (1.0 - ((y + 0.5) / H)) * np.pi
    row = (np.pi * 2 / W) * (np.cos(theta - (np.pi / H / 2.0)) - np.cos(theta + (np.pi / H / 2.0)))
    return np.repeat(row[:, None], W, axis=1).reshape(-1)


def analysis(pano, M, weights=None):
    """pano (B, 3, H, W), M (P, K) -> (B, K, 3)."""
    B = pano.shape[0]
    flat = np.asarray(pano, dtype=np.float64).reshape(B, 3, -1)
    if weights is not None:
        flat = flat * weights
    return np.einsum("bcp,pk->bkc", flat, M)


def synthesis(coeffs, M, H, W, weights=None):
    """coeffs (B, K, 3), M (P, K) -> (B, 3, H, W)."""
    rec = np.einsum("pk,bkc->bcp", M, np.asarray(coeffs, dtype=np.float64))
    if weights is not None:
        rec = rec * weights
    return rec.reshape(coeffs.shape[0], 3, H, W)


def matrix_f32(theta, phi, jmax):
    """The kernels' arithmetic in numpy float32 (float32 directions, centres and table; forward three-term recurrence with
    float32 constants; every operation rounded to float32): the floor a float32 evaluation of the basis can reach."""
    f = np.float32
    x = directions(theta, phi).astype(f)
    c, cen = zonal_coefficients(jmax).astype(f), centres(jmax).astype(f)
    cen[0] = (0, 0, 1)
    L = c.shape[1] - 1
    out = np.empty((x.shape[0], rows(jmax)), dtype=f)
    for row, sl in enumerate(level_slices(jmax)):
        t = (x[:, 0:1] * cen[sl, 0] + x[:, 1:2] * cen[sl, 1]) + x[:, 2:3] * cen[sl, 2]
        p0, p1 = np.ones_like(t), t
        s = c[row, 0] + c[row, 1] * t
        for l in range(2, L + 1):
            a, b = f((2.0 * l - 1.0) / l), f((l - 1.0) / l)
            p = (a * t) * p1 - b * p0
            s = s + c[row, l] * p
            p0, p1 = p1, p
        out[:, sl] = s
    return out


def rel_err(got, want):
    """max|got - want| / max|want|: the measure of every needlet tolerance."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def hdr_image(B, H, W, seed=0):
    """U[0,1)^4 * 50 + 0.01 (the golden images' recipe): float32, a dynamic range of a few thousand."""
    g = np.random.default_rng([seed, B, H, W])
    return (g.random((B, 3, H, W)) ** 4 * 50.0 + 0.01).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
# The cases of test_gpu_needlets.py, kept here so that the floors below are measured on exactly the arrays the tests feed in
# (hdr_image seeds itself with B, so another batch size is another image).  A case is (H, W, jmax, B).
GOLDEN_SHAPES = [(12, 24, 1), (12, 24, 2), (16, 32, 3)]                    # images and coefficients of the golden file (B = 2)
GRID_SHAPES = [(12, 24, 1), (16, 32, 3), (32, 64, 2), (4, 8, 0)]           # the matrix on both grids
# analysis with more than one chunk per split (make_plan: per >= 2): K, chunks, per, splits, chunks in the last split, tail
#   25 x 47 jmax 4: 4093, 19, 2, 10, 1, 23      50 x 100 jmax 1: 61, 79, 2, 40, 1, 8      48 x 96 jmax 0: 13, 72, 2, 36, 2, 64
PER2_SHAPES = [(25, 47, 4), (50, 100, 1), (48, 96, 0)]
ONE_CHUNK_SHAPES = [(4, 8, 0), (3, 5, 2)]                                  # P < 64: a single ragged chunk
ANALYSIS_CASES = [(12, 24, 1, 2), (16, 32, 3, 1), (32, 64, 2, 11),
                  (25, 47, 4, 2), (50, 100, 1, 2), (48, 96, 0, 1), (4, 8, 0, 3), (3, 5, 2, 2)]
SYNTHESIS_CASES = [(12, 24, 1, 1), (16, 32, 3, 11), (32, 64, 2, 2),
                   (25, 47, 4, 2), (4, 8, 0, 3), (3, 5, 2, 2), (48, 96, 0, 1)]
COLUMN_GROUP_CASES = [(12, 24, 1, 32), (12, 24, 1, 33), (12, 24, 1, 65)]   # 3B = 96, 96 + 3, 96 + 96 + 3 planes
ADJOINT_CASES = [(12, 24, 1, 2), (16, 32, 3, 2), (25, 47, 4, 2), (50, 100, 1, 33)]
ADJOINT_SEEDS = {"x": 1, "g": 2, "up": 3}                                  # the panorama, the coefficients, the upstream image
SUM_BACKWARD_CASE = (12, 24, 1, 2)                                         # gradients of .sum(): all-ones upstream


def floor_key(H, W, jmax, B, source=0):
    """The name of a floor.  ``source``: the seed of ``hdr_image`` (0 is not written), "golden" or "ones"."""
    if isinstance(source, str):
        tail = "_" + source
    elif source == 0:
        tail = ""
    else:
        tail = "_s%d" % source
    return "%dx%d_j%d_b%d%s" % (H, W, jmax, B, tail)


def floor_cases():
    """{"analysis": [(H, W, jmax, B, source)], "synthesis": [...]}: every input a GPU test holds against an analysis or a
    synthesis tolerance."""
    ana = [(H, W, j, 2, "golden") for H, W, j in GOLDEN_SHAPES] + [c + (0,) for c in ANALYSIS_CASES + COLUMN_GROUP_CASES]
    syn = [c + (0,) for c in SYNTHESIS_CASES + COLUMN_GROUP_CASES]
    for c in ADJOINT_CASES:
        ana += [c + (ADJOINT_SEEDS["x"],), c + (ADJOINT_SEEDS["up"],)]
        syn += [c + (ADJOINT_SEEDS["g"],)]
    ana.append(SUM_BACKWARD_CASE + ("ones",))
    syn.append(SUM_BACKWARD_CASE + ("ones",))
    return {"analysis": ana, "synthesis": syn}


@functools.lru_cache(maxsize=None)
def _grid_matrices(H, W, jmax):
    """(M32, M64) on the reference grid: the float32 restatement and the float64 definition."""
    th, ph = grid_angles(H, W)
    return matrix_f32(th, ph, jmax), matrix(th, ph, jmax)


def analysis_floor(im, H, W, jmax, want=None):
    """The float32 restatement's weighted analysis of ``im`` (B, 3, H, W) on the reference grid against ``want`` (default:
    the float64 analysis of the same image), as max|error| / max|value|."""
    f = np.float32
    M32, M64 = _grid_matrices(H, W, jmax)
    B = im.shape[0]
    if want is None:
        want = analysis(im, M64, solid_angles(H, W))
    flat = np.asarray(im, dtype=f).reshape(3 * B, H * W) * solid_angles(H, W).astype(f)
    got = np.stack([np.sum(M32 * flat[n][:, None], axis=0, dtype=f) for n in range(3 * B)]).reshape(B, 3, -1).transpose(0, 2, 1)
    return rel_err(got, want)


def synthesis_floor(co, H, W, jmax):
    """The float32 restatement's (unweighted) synthesis of float32 coefficients ``co`` (B, K, 3) against the float64 one."""
    f = np.float32
    M32, M64 = _grid_matrices(H, W, jmax)
    B = co.shape[0]
    rec = np.stack([np.sum(M32 * co[b, :, c][None, :], axis=1, dtype=f) for b in range(B) for c in range(3)])
    return rel_err(rec, synthesis(co, M64, H, W).reshape(3 * B, -1))


def float32_floors(golden):
    """The float32 floors behind the GPU tolerances (test_gpu_needlets.py): what the kernels' arithmetic reaches in numpy
    float32 -- float32 directions, centres, table and solid angles, every product and (pairwise) sum rounded to float32 --
    as max|error| / max|value|.  The error of P_l(t) for a float32 t grows with l^2 and a sum's error depends on its terms,
    hence one floor per jmax (matrix) or per input (analysis, synthesis; ``floor_cases`` lists them, ``floor_key`` names them):
    * matrix[jmax]: against the reference-made golden (a); jmax 0 is not in that file: the same points, against this file's
      float64, which equals the golden to 1e-9 where they overlap;
    * analysis[key]: the golden image against golden (c); every other image against this file's float64;
    * synthesis[key]: of the float32-rounded float64 coefficients of that image, against this file's float64 (the reference
      writes no reconstruction).
    "ones" is the all-ones panorama, and the all-ones coefficients: the upstream gradient of a ``.sum()``."""
    f = np.float32
    floors = {"matrix": {}, "analysis": {}, "synthesis": {}}
    th, ph = golden["a/j1/theta"], golden["a/j1/phi"]
    floors["matrix"][0] = rel_err(matrix_f32(th, ph, 0), matrix(th, ph, 0))
    for jmax in (1, 2, 3, 4):
        th, ph = golden["a/j%d/theta" % jmax], golden["a/j%d/phi" % jmax]
        floors["matrix"][jmax] = rel_err(matrix_f32(th, ph, jmax), golden["a/j%d/matrix" % jmax])
    for H, W, jmax, B, source in floor_cases()["analysis"]:
        if source == "golden":
            name = "%dx%d_j%d" % (H, W, jmax)
            im, want = golden["c/%s/image" % name], golden["c/%s/coeffs" % name]
        else:
            im, want = np.ones((B, 3, H, W), dtype=f) if source == "ones" else hdr_image(B, H, W, source), None
        floors["analysis"][floor_key(H, W, jmax, B, source)] = analysis_floor(im, H, W, jmax, want)
    for H, W, jmax, B, source in floor_cases()["synthesis"]:
        if source == "ones":
            co = np.ones((B, rows(jmax), 3), dtype=f)
        else:
            co = analysis(hdr_image(B, H, W, source), _grid_matrices(H, W, jmax)[1], solid_angles(H, W)).astype(f)
        floors["synthesis"][floor_key(H, W, jmax, B, source)] = synthesis_floor(co, H, W, jmax)
    return floors


def sparsify(coeffs, jmax, ratio=0.1, levels=(2, 3)):
    """mat_gen2.py:43-51 on float32 coefficients (B, K, 3), in float32: (new coefficients, kept (B, jmax + 1) int32)."""
    c = np.array(coeffs, dtype=np.float32)
    sl = level_slices(jmax)
    kept = np.empty((c.shape[0], jmax + 1), dtype=np.int32)
    for b in range(c.shape[0]):
        for j in range(jmax + 1):
            blk = c[b, sl[j + 1]]
            if j in levels:
                mask = np.abs(blk) > np.float32(np.float32(ratio) * np.abs(blk).max())
                c[b, sl[j + 1]] = blk * mask
                kept[b, j] = mask.sum()
            else:
                kept[b, j] = blk.size
    return c, kept
