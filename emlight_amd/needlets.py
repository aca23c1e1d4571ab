"""Spherical needlets on the GPU (NeedleLight; the reference's ``Needlets/`` folder): the basis matrix ``SN_matrix`` of
``sphere_needlets.py:236``, the coefficients of a panorama (``gt_gen_j3.py:39-43``), the reconstruction
(``mat_gen2.py:55``) and the per-level hard threshold (``mat_gen2.py:43-51``).  ``csrc/needlets.hip`` holds the kernels,
DESIGN.md section 16 the closed form they evaluate.  No ``healpy``, no stored matrix, no CPU path.

    python -m emlight_amd.needlets --pano_dir DIR --out_dir DIR [--jmax 3] [--height 128] [--fov 60] [--no_alpha]
                                   [--sparsify RATIO] [--batchSize 8]

is ``gt_gen_j3.py`` over a directory of ``(H, W, 3)`` float32 ``.npy`` panoramas: one ``<name>.npy`` of shape ``(K, 3)`` each.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib

JMAX_LIMIT = 4            # the kernels' Legendre recurrence runs to 2^(jmax+1) <= 32
TABLE_ROW = 33            # coefficients l = 0..32 of one table row
GRIDS = ("reference", "centres")


def _jmax(jmax):
    if isinstance(jmax, bool) or int(jmax) != jmax or not 0 <= int(jmax) <= JMAX_LIMIT:
        raise ValueError("jmax: expected an integer in 0..%d, got %r" % (JMAX_LIMIT, jmax))
    return int(jmax)


# ------------------------------------------------------------------------------------------------ HEALPix, RING scheme
def _rings(nside):
    """For each ring i = 1..4 nside - 1: (z, number of pixels, phi of pixel 0 in units of the ring's step)."""
    n = int(nside)
    if n < 1 or n & (n - 1):
        raise ValueError("nside: expected a power of two >= 1, got %r" % (nside,))
    out = []
    for i in range(1, 4 * n):
        if i < n:                                   # north polar cap
            out.append((1.0 - i * i / (3.0 * n * n), 4 * i, 0.5))
        elif i <= 3 * n:                            # equatorial belt
            out.append((4.0 / 3.0 - 2.0 * i / (3.0 * n), 4 * n, 0.5 * ((i - n + 1) % 2)))
        else:                                       # south polar cap: the mirror image of the north one
            m = 4 * n - i
            out.append((-(1.0 - m * m / (3.0 * n * n)), 4 * m, 0.5))
    return out


def healpix_ring_centres(nside):
    """``(12 nside^2, 3)`` float64 unit vectors of the HEALPix pixel centres in RING order (Gorski et al. 2005, section 4.1;
    what ``healpy.pix2vec(nside, range(npix))`` returns)."""
    parts = []
    for z, m, shift in _rings(nside):
        phi = (np.arange(m) + shift) * (2.0 * np.pi / m)
        s = np.sqrt((1.0 - z) * (1.0 + z))
        parts.append(np.stack([s * np.cos(phi), s * np.sin(phi), np.full(m, z)], 1))
    return np.concatenate(parts, 0)


def _antipodes(nside):
    """Index of the pixel at ``-xi`` for every pixel: ring i <-> ring 4 nside - i, half a turn along the ring."""
    rings = _rings(nside)
    counts = np.array([m for _, m, _ in rings])
    start = np.concatenate([[0], np.cumsum(counts)])
    out = np.empty(start[-1], dtype=np.int64)
    R = len(rings)
    for r, (_, m, _) in enumerate(rings):
        out[start[r]:start[r + 1]] = start[R - 1 - r] + (np.arange(m) + m // 2) % m
    return out


def cubature(jmax):
    """All needlet centres ``xi_jk`` stacked by level, ``(K - 1, 3)`` float64: level j uses Nside = 2^j
    (``sphere_needlets.py:48`` with B = 2)."""
    return np.concatenate([healpix_ring_centres(2 ** j) for j in range(_jmax(jmax) + 1)], 0)


def cubature_weights(jmax):
    """``lambda_j = 4 pi / Npix_j`` for the levels 0..jmax, ``(jmax + 1,)`` float64: the equal weight of a level's centres
    (``sphere_needlets.py:50-52``)."""
    return np.array([4.0 * np.pi / (12.0 * 4 ** j) for j in range(_jmax(jmax) + 1)])


def antipodal_pairs(jmax):
    """``(cubature_pair, cubature_use)`` of ``spneedlet_pair`` (``sphere_needlets.py:107-128``) as int64 arrays over the
    stacked centres: ``cubature()[pair[i]] == -cubature()[i]``, and ``use`` lists the ``i`` with ``pair[i] > i`` -- the
    columns of the symmetrised basis ``(psi_i + psi_pair[i]) / 2``."""
    pair, base = [], 0
    for j in range(_jmax(jmax) + 1):
        a = _antipodes(2 ** j)
        pair.append(base + a)
        base += len(a)
    pair = np.concatenate(pair)
    return pair, np.nonzero(pair > np.arange(len(pair)))[0]


def level_slices(jmax):
    """Rows of the basis per level: ``[slice(0, 1)]`` for Y_00, then one slice per level 0..jmax."""
    out, start = [slice(0, 1)], 1
    for j in range(_jmax(jmax) + 1):
        out.append(slice(start, start + 12 * 4 ** j))
        start += 12 * 4 ** j
    return out


# ------------------------------------------------------------------------------------------------ window and coefficients
def _f2(u, nodes=200):
    """``compute_f2`` (``sphere_needlets.py:10-12``) by Gauss-Legendre quadrature (the integrand is smooth and flat at +-1)."""
    x, w = np.polynomial.legendre.leggauss(nodes)

    def integral(hi):
        hi = min(hi, 1.0)
        t = -1.0 + (x + 1.0) * (hi + 1.0) * 0.5
        return (hi + 1.0) * 0.5 * float(np.dot(w, np.exp(-1.0 / ((1.0 - t) * (1.0 + t)))))
    return integral(u + 1e-10) / integral(1.0)


def _f3(x):
    if x <= 0.5:
        return 1.0
    return _f2(1.0 - 4.0 * (x - 0.5)) if x <= 1.0 else 0.0


def needlet_window(jmax):
    """``b(l / 2^j)`` (``fun_b``, ``sphere_needlets.py:10-29``, B = 2) as ``(jmax + 1, 2^(jmax+1) + 1)`` float64, column l;
    column 0 and the columns beyond ``2^(j+1)`` are 0."""
    jmax = _jmax(jmax)
    L = 2 ** (jmax + 1)
    out = np.zeros((jmax + 1, L + 1))
    for j in range(jmax + 1):
        for l in range(1, L + 1):
            x = l / 2.0 ** j
            out[j, l] = np.sqrt(max(_f3(x / 2.0) - _f3(x), 0.0))
    return out


def coefficient_table(jmax):
    """``(jmax + 2, 33)`` float64: row 0 is Y_00 (``1 / sqrt(4 pi)`` at l = 0), row j + 1 is
    ``sqrt(4 pi / Npix_j) b(l / 2^j) (2l + 1) / (4 pi)``."""
    jmax = _jmax(jmax)
    b = needlet_window(jmax)
    out = np.zeros((jmax + 2, TABLE_ROW))
    out[0, 0] = 1.0 / np.sqrt(4.0 * np.pi)
    l = np.arange(b.shape[1])
    lam = cubature_weights(jmax)
    for j in range(jmax + 1):
        out[j + 1, :b.shape[1]] = np.sqrt(lam[j]) * b[j] * (2.0 * l + 1.0) / (4.0 * np.pi)
    return out


def directions(theta, phi):
    """Unit vectors ``(P, 3)`` float64 of colatitude / azimuth arrays.  ``sin(theta)`` is taken of the distance to the nearer
    pole, so that ``theta = pi`` gives the pole itself (``sin(np.pi)`` is 1.2e-16, not 0)."""
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    s = np.sin(np.minimum(theta, np.pi - theta))
    return np.stack([s * np.cos(phi), s * np.sin(phi), np.cos(theta)], -1)


def solid_angles(height, width):
    """``getSolidAngleMap`` (``Needlets/utils.py:35-50``) flattened, ``(height * width,)`` float64."""
    y = np.arange(height)
    th = (1.0 - (y + 0.5) / height) * np.pi
    row = (2.0 * np.pi / width) * (np.cos(th - np.pi / height / 2.0) - np.cos(th + np.pi / height / 2.0))
    return np.repeat(row[:, None], width, 1).reshape(-1)


def grid_angles(height, width, grid="reference"):
    """``(theta, phi)`` of every pixel, flattened row-major.  "reference": ``linspace(0, pi, H)`` x ``linspace(0, 2 pi, W)``,
    both inclusive (``mat_gen2.py:22-25``); "centres": the pixel centres, the quadrature ``solid_angles`` belongs to."""
    if grid == "reference":
        th, ph = np.linspace(0.0, 1.0, height) * np.pi, np.linspace(0.0, 2.0, width) * np.pi
    elif grid == "centres":
        th, ph = (np.arange(height) + 0.5) * np.pi / height, (np.arange(width) + 0.5) * 2.0 * np.pi / width
    else:
        raise ValueError("grid: expected one of %s, got %r" % (GRIDS, grid))
    return np.repeat(th, width), np.tile(ph, height)


# ------------------------------------------------------------------------------------------------ the basis object
class _Analysis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pano, basis, weighted):
        ctx.basis, ctx.weighted = basis, weighted
        return basis._analysis(pano, weighted)

    @staticmethod
    def backward(ctx, g):
        return _Synthesis.apply(g, ctx.basis, ctx.weighted), None, None


class _Synthesis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coeffs, basis, weighted):
        ctx.basis, ctx.weighted = basis, weighted
        return basis._synthesis(coeffs, weighted)

    @staticmethod
    def backward(ctx, g):
        return _Analysis.apply(g, ctx.basis, ctx.weighted), None, None


class NeedletBasis:
    """The needlet basis up to level ``jmax`` on an equirectangular ``height x width`` grid.

    * ``K``: the number of basis functions (13, 61, 253, 1021, 4093 for jmax 0..4); ``level_slices``: their rows per level;
    * ``matrix(theta=None, phi=None)``: ``(P, K)``, the reference's ``SN_matrix`` on the grid or at the given angles;
    * ``analysis(pano, weighted=True)``: ``(B, 3, H, W) -> (B, K, 3)``, ``sum_p psi_k(x_p) dOmega_p pano[b, c, p]``
      (``weighted=False``: without the solid angles);
    * ``synthesis(coeffs, weighted=False)``: ``(B, K, 3) -> (B, 3, H, W)``, ``np.dot(SN_Matrix, SN_Coeffs)``
      (``weighted=True``: times the solid angles, the adjoint of ``analysis``);
    * ``sparsify(coeffs, ratio=0.1, levels=(2, 3))``: ``(coeffs, kept)``.

    ``analysis`` and ``synthesis`` are differentiable; each one's backward is the other's kernel.  Only device tensors are
    taken; every call only enqueues work, is run-to-run exact and treats an image the same in any batch."""

    def __init__(self, jmax=3, height=128, width=256, grid="reference", device="cuda"):
        self.jmax = _jmax(jmax)
        if int(height) != height or int(width) != width or height < 1 or width < 1 or height * width > 1 << 24:
            raise ValueError("height, width: expected positive integers with height * width <= 2^24, got %r, %r" % (height, width))
        if grid not in GRIDS:
            raise ValueError("grid: expected one of %s, got %r" % (GRIDS, grid))
        self.height, self.width, self.grid, self.device = int(height), int(width), grid, torch.device(device)
        self.level_slices = level_slices(self.jmax)
        self.K = self.level_slices[-1].stop
        self.P = self.height * self.width
        cen = np.zeros((self.K, 4))
        cen[0, :3] = (0.0, 0.0, 1.0)                       # Y_00 is constant: any centre
        cen[1:, :3] = cubature(self.jmax)
        for row, sl in enumerate(self.level_slices):
            cen[sl, 3] = row
        self._centres = self._upload(cen)
        self._ctab = self._upload(coefficient_table(self.jmax))
        self._dirs = self._upload(directions(*grid_angles(self.height, self.width, grid)))
        self._weights = self._upload(solid_angles(self.height, self.width))
        self._work = None

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _scratch(self, L, B):
        need = max(1, L.eml_needlet_work_floats(self.P, self.jmax, B))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._work

    def matrix(self, theta=None, phi=None):
        if (theta is None) != (phi is None):
            raise ValueError("theta and phi go together")
        if theta is None:
            dirs = self._dirs
        else:
            th, ph = (np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float64) for v in (theta, phi))
            if th.ndim != 1 or th.shape != ph.shape or th.size < 1:
                raise ValueError("theta, phi: expected two 1-D arrays of one length >= 1, got %s and %s" % (th.shape, ph.shape))
            dirs = self._upload(directions(th, ph))
        dirs = _lib.require_gpu_tensor(dirs, "dirs")
        out = torch.empty(dirs.shape[0], self.K, dtype=torch.float32, device=dirs.device)
        _lib.check(_lib.lib().eml_needlet_basis_f32(_lib.ptr(dirs), dirs.shape[0], _lib.ptr(self._centres), _lib.ptr(self._ctab),
                                                    self.jmax, _lib.ptr(out), _lib.current_stream()), "eml_needlet_basis_f32")
        return out

    def _analysis(self, pano, weighted):
        x = _lib.require_gpu_tensor(pano, "pano")
        B = x.shape[0]
        out = torch.empty(B, self.K, 3, dtype=torch.float32, device=x.device)
        if B > 0:
            L = _lib.lib()
            _lib.check(L.eml_needlet_analysis_f32(_lib.ptr(x), _lib.ptr(self._dirs), _lib.ptr(self._weights if weighted else None),
                                                  B, self.P, _lib.ptr(self._centres), _lib.ptr(self._ctab), self.jmax,
                                                  _lib.ptr(out), _lib.ptr(self._scratch(L, B)), _lib.current_stream()),
                       "eml_needlet_analysis_f32")
        return out

    def _synthesis(self, coeffs, weighted):
        c = _lib.require_gpu_tensor(coeffs, "coeffs")
        B = c.shape[0]
        out = torch.empty(B, 3, self.height, self.width, dtype=torch.float32, device=c.device)
        if B > 0:
            _lib.check(_lib.lib().eml_needlet_synthesis_f32(_lib.ptr(c), _lib.ptr(self._dirs),
                                                            _lib.ptr(self._weights if weighted else None), B, self.P,
                                                            _lib.ptr(self._centres), _lib.ptr(self._ctab), self.jmax,
                                                            _lib.ptr(out), _lib.current_stream()), "eml_needlet_synthesis_f32")
        return out

    def _check_pano(self, pano):
        if not isinstance(pano, torch.Tensor) or pano.dim() != 4 or tuple(pano.shape[1:]) != (3, self.height, self.width):
            raise ValueError("pano: expected (B, 3, %d, %d), got %s" % (self.height, self.width, tuple(getattr(pano, "shape", ()))))

    def _check_coeffs(self, coeffs):
        if not isinstance(coeffs, torch.Tensor) or coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (self.K, 3):
            raise ValueError("coeffs: expected (B, %d, 3), got %s" % (self.K, tuple(getattr(coeffs, "shape", ()))))

    def analysis(self, pano, weighted=True):
        self._check_pano(pano)
        return _Analysis.apply(pano, self, bool(weighted))

    def synthesis(self, coeffs, weighted=False):
        self._check_coeffs(coeffs)
        return _Synthesis.apply(coeffs, self, bool(weighted))

    def sparsify(self, coeffs, ratio=0.1, levels=(2, 3)):
        """Per image and per level of ``levels``: keep ``|c| > float32(ratio) * max|c|`` (the maximum over the level's rows and
        the three channels), zero the rest; other rows pass through.  Returns the new coefficients and ``kept (B, jmax + 1)``
        int32, the entries kept per level.  Not differentiable."""
        self._check_coeffs(coeffs)
        if not 0.0 <= float(ratio) <= 1.0:
            raise ValueError("ratio: expected a number in [0, 1], got %r" % (ratio,))
        lv = tuple(levels)
        if len(set(lv)) != len(lv) or any(isinstance(v, bool) or int(v) != v or not 0 <= v <= self.jmax for v in lv):
            raise ValueError("levels: expected distinct integers in 0..%d, got %r" % (self.jmax, levels))
        c = _lib.require_gpu_tensor(coeffs.detach(), "coeffs")
        B = c.shape[0]
        out = torch.empty_like(c)
        kept = torch.empty(B, self.jmax + 1, dtype=torch.int32, device=c.device)
        if B > 0:
            _lib.check(_lib.lib().eml_needlet_sparsify_f32(_lib.ptr(c), B, self.jmax, sum(1 << int(v) for v in lv), float(ratio),
                                                           _lib.ptr(out), _lib.ptr(kept), _lib.current_stream()),
                       "eml_needlet_sparsify_f32")
        return out, kept


# ------------------------------------------------------------------------------------------------ command line
def _batcher(fov, device):
    from .RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(fov_deg=fov, device=device)


def prepared_batches(pano_dir, height, width, fov=60.0, alpha=True, batch_size=8, device="cuda:0"):
    """The input side of ``gt_gen_j3.py`` over ``pano_dir/*.npy``: yields ``(names, x)`` per batch, ``x`` ``(B, 3, height,
    width)`` contiguous -- the panoramas area-resized (``:31``) and, unless ``alpha`` is false, multiplied by the tonemap
    alpha of the crop at azimuth 0 (``:34-37``)."""
    from torch.utils.data import DataLoader
    from .RegressionNetwork.data import PanoramaDataset
    loader = DataLoader(PanoramaDataset(pano_dir), batch_size=batch_size, shuffle=False, drop_last=False)
    batcher = _batcher(fov, device)
    batcher.PANO_HW = (height, width)
    for para in loader:
        panos = para["pano"].to(device)
        x = batcher.small(panos, 0.0).permute(0, 3, 1, 2)
        if alpha:
            x = x * batcher.tone(batcher.crop(panos, 0.0, fov))[1].reshape(-1, 1, 1, 1)
        yield list(para["name"]), x.contiguous()


def coefficients_of_directory(pano_dir, out_dir, jmax=3, height=128, fov=60.0, alpha=True, sparsify=None, batch_size=8,
                              device="cuda:0"):
    """``gt_gen_j3.py`` over ``pano_dir/*.npy``: area-resize to ``height x 2 height`` (``:31``), multiply by the tonemap alpha
    of the crop at azimuth 0 (``:34-37``) unless ``alpha`` is false, project (``:39-43``), optionally threshold levels 2 and 3
    (``mat_gen2.py:43-51``), write ``out_dir/<name>.npy`` ``(K, 3)`` float32 (``:45``).  Returns the names written."""
    basis = NeedletBasis(jmax=jmax, height=height, width=2 * height, device=device)
    levels = tuple(v for v in (2, 3) if v <= basis.jmax)
    if sparsify is not None and not levels:
        raise ValueError("--sparsify thresholds levels 2 and 3; jmax = %d has neither" % basis.jmax)
    os.makedirs(out_dir, exist_ok=True)
    names = []
    for batch_names, x in prepared_batches(pano_dir, basis.height, basis.width, fov, alpha, batch_size, device):
        coeffs = basis.analysis(x)
        if sparsify is not None:
            coeffs = basis.sparsify(coeffs, ratio=sparsify, levels=levels)[0]
        host = coeffs.cpu().numpy()
        for q, name in enumerate(batch_names):
            np.save(os.path.join(out_dir, name + ".npy"), host[q])
            names.append(name)
    return names


def main(argv=None, device=None):
    ap = argparse.ArgumentParser(description="needlet coefficients of a directory of HDR panoramas")
    ap.add_argument("--pano_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--jmax", type=int, default=3)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--no_alpha", action="store_true", help="do not multiply by the crop's tonemap alpha")
    ap.add_argument("--sparsify", type=float, default=None, metavar="RATIO", help="hard-threshold levels 2 and 3")
    ap.add_argument("--batchSize", type=int, default=8)
    args = ap.parse_args(argv)
    from . import _runtime
    _runtime.entry_point_defaults()
    names = coefficients_of_directory(args.pano_dir, args.out_dir, args.jmax, args.height, args.fov, not args.no_alpha,
                                      args.sparsify, args.batchSize, device or "cuda:0")
    print("%d panoramas -> %s" % (len(names), args.out_dir))
    return names


if __name__ == "__main__":
    main()
