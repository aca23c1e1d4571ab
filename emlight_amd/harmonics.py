"""Real spherical harmonics on the GPU (the reference's ``Needlets/sphere_harmonics.py``): the basis matrix in both of its
conventions (``shEvaluate`` / ``SH``, ``:48-70``, and ``spharmonic``, ``:94-115``), the coefficients of a panorama and the
reconstruction as a separable transform on the equirectangular grid, and the change of basis to the needlets
(``Ctran_asymm``, ``sphere_needlets.py:254-277``).  ``csrc/harmonics.hip`` holds the kernels, DESIGN.md section 17 the
definitions.  No scipy, no stored ``(P, K)`` matrix on the grid path, no CPU path.

    python -m emlight_amd.harmonics --pano_dir DIR --out_dir DIR [--lmax 8] [--height 128] [--convention graphics]
                                    [--fov 60] [--no_alpha] [--batchSize 8]

writes one ``<name>.npy`` of shape ``(K, 3)`` per ``(H, W, 3)`` float32 ``.npy`` panorama of the directory.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, needlets

LMAX_LIMIT = 32           # the needlets' L at jmax = 4; the kernels hold 33 orders
ORDERS = LMAX_LIMIT + 1
CONVENTIONS = ("graphics", "symmetrised")
GRIDS = needlets.GRIDS


def _lmax(lmax):
    if isinstance(lmax, bool) or int(lmax) != lmax or not 0 <= int(lmax) <= LMAX_LIMIT:
        raise ValueError("lmax: expected an integer in 0..%d, got %r" % (LMAX_LIMIT, lmax))
    return int(lmax)


def _convention(convention):
    if convention not in CONVENTIONS:
        raise ValueError("convention: expected one of %s, got %r" % (CONVENTIONS, convention))
    return convention


def band_slices(lmax):
    """Columns of the basis per degree: ``slice(l^2, (l + 1)^2)`` for l = 0..lmax (column ``l^2 + l + m``)."""
    return [slice(l * l, (l + 1) * (l + 1)) for l in range(_lmax(lmax) + 1)]


def recurrence_table():
    """``(d, a, b)`` float64: ``d[m]`` is ``Ybar_m^m / sin^m(theta)``, ``a[m, l]`` and ``b[m, l]`` the coefficients of
    ``Ybar_l^m = a_lm (z Ybar_{l-1}^m - b_lm Ybar_{l-2}^m)``, zero where ``l <= m``."""
    d = np.empty(ORDERS)
    d[0] = 1.0 / np.sqrt(4.0 * np.pi)
    for m in range(1, ORDERS):
        d[m] = -np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * d[m - 1]
    a, b = np.zeros((ORDERS, ORDERS)), np.zeros((ORDERS, ORDERS))
    for m in range(ORDERS):
        for l in range(m + 1, ORDERS):
            a[m, l] = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b[m, l] = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
    return d, a, b


def convention_table(convention):
    """``(33, 4)`` float64, per order m: ``+1`` if the ``cos(m phi)`` part is column ``+m`` and the ``sin`` part ``-m``, ``-1``
    the other way round; the scale of the cos part; the scale of the sin part; 0."""
    out = np.zeros((ORDERS, 4))
    m = np.arange(1, ORDERS)
    out[0] = (1.0, 1.0, 0.0, 0.0)
    out[1:, 1] = np.sqrt(2.0)
    if _convention(convention) == "graphics":                # m > 0: sqrt(2) cos, m < 0: sqrt(2) sin
        out[1:, 0], out[1:, 2] = 1.0, np.sqrt(2.0)
    else:                                                    # m < 0: sqrt(2) cos, m > 0: (-1)^m sqrt(2) sin
        out[1:, 0], out[1:, 2] = -1.0, np.sqrt(2.0) * (-1.0) ** m
    return out


def device_table(convention):
    """The kernels' ``tab``: ``d``, ``a``, ``b`` and the convention, one flat float64 array of 2343."""
    d, a, b = recurrence_table()
    return np.concatenate([d, a.reshape(-1), b.reshape(-1), convention_table(convention).reshape(-1)])


def grid_tables(height, width, grid="reference"):
    """``(rows (H, 2), fourier (W, 33, 2), weights (H,))`` float64 of the product grid: ``cos`` and ``sin`` of the rows'
    colatitude (the sine of the distance to the nearer pole, as ``needlets.directions`` takes it), ``cos(m phi_x)`` and
    ``sin(m phi_x)`` for m = 0..32, and the rows' solid angle per pixel."""
    th, ph = needlets.grid_angles(height, width, grid)
    th, ph = th[::width], ph[:width]
    rows = np.stack([np.cos(th), np.sin(np.minimum(th, np.pi - th))], 1)
    arg = ph[:, None] * np.arange(ORDERS)[None, :]
    return rows, np.stack([np.cos(arg), np.sin(arg)], 2), needlets.solid_angles(height, width)[::width]


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


class HarmonicBasis:
    """The real spherical harmonics up to degree ``lmax`` on an equirectangular ``height x width`` grid.

    * ``K = (lmax + 1)^2``: the number of basis functions, column ``l^2 + l + m``; ``band_slices``: their columns per degree;
    * ``matrix(theta=None, phi=None)``: ``(P, K)``, ``spharmonic`` / ``shEvaluate`` on the grid or at the given angles;
    * ``analysis(pano, weighted=True)``: ``(B, 3, H, W) -> (B, K, 3)``, ``sum_p Y_k(x_p) dOmega_p pano[b, c, p]``
      (``weighted=False``: without the solid angles);
    * ``synthesis(coeffs, weighted=False)``: ``(B, K, 3) -> (B, 3, H, W)``, ``np.dot(SH_matrix, coeffs)``
      (``weighted=True``: times the solid angles, the adjoint of ``analysis``);
    * ``to_needlets(coeffs, jmax)``: ``(B, K, 3) -> (B, K_needlets, 3)``, the needlet coefficients of the band-limited
      function the harmonic coefficients describe.

    ``analysis`` and ``synthesis`` are differentiable; each one's backward is the other's kernel.  Only device tensors are
    taken; every call only enqueues work, is run-to-run exact and treats an image the same in any batch.

    A basis owns one scratch buffer for the analysis' partial sums, shared by all its calls (backward calls included), as
    ``NeedletBasis`` does: calls on one stream are ordered and safe, calls of one basis on different streams race on it --
    use a basis per stream."""

    def __init__(self, lmax=8, height=128, width=256, grid="reference", convention="graphics", device="cuda"):
        self.lmax, self.convention = _lmax(lmax), _convention(convention)
        if int(height) != height or int(width) != width or height < 1 or width < 1 or height * width > 1 << 24:
            raise ValueError("height, width: expected positive integers with height * width <= 2^24, got %r, %r" % (height, width))
        if grid not in GRIDS:
            raise ValueError("grid: expected one of %s, got %r" % (GRIDS, grid))
        self.height, self.width, self.grid, self.device = int(height), int(width), grid, torch.device(device)
        self.band_slices = band_slices(self.lmax)
        self.K = self.band_slices[-1].stop
        self.P = self.height * self.width
        rows, fourier, weights = grid_tables(self.height, self.width, grid)
        self._tab = self._upload(device_table(self.convention))
        self._rows, self._fourier, self._weights = self._upload(rows), self._upload(fourier), self._upload(weights)
        self._dirs = self._upload(needlets.directions(*needlets.grid_angles(self.height, self.width, grid)))
        self._work = None
        self._to_needlets = {}

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _scratch(self, L, B):
        need = max(1, L.eml_sh_work_floats(self.height, self.width, self.lmax, B))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._work

    def _matrix_at(self, dirs):
        dirs = _lib.require_gpu_tensor(dirs, "dirs")
        out = torch.empty(dirs.shape[0], self.K, dtype=torch.float32, device=dirs.device)
        _lib.check(_lib.lib().eml_sh_basis_f32(_lib.ptr(dirs), dirs.shape[0], _lib.ptr(self._tab), self.lmax, _lib.ptr(out),
                                               _lib.current_stream()), "eml_sh_basis_f32")
        return out

    def matrix(self, theta=None, phi=None):
        if (theta is None) != (phi is None):
            raise ValueError("theta and phi go together")
        if theta is None:
            return self._matrix_at(self._dirs)
        th, ph = (np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float64) for v in (theta, phi))
        if th.ndim != 1 or th.shape != ph.shape or th.size < 1:
            raise ValueError("theta, phi: expected two 1-D arrays of one length >= 1, got %s and %s" % (th.shape, ph.shape))
        return self._matrix_at(self._upload(needlets.directions(th, ph)))

    def _analysis(self, pano, weighted):
        x = _lib.require_gpu_tensor(pano, "pano")
        B = x.shape[0]
        out = torch.empty(B, self.K, 3, dtype=torch.float32, device=x.device)
        if B > 0:
            L = _lib.lib()
            _lib.check(L.eml_sh_analysis_f32(_lib.ptr(x), _lib.ptr(self._rows), _lib.ptr(self._weights if weighted else None),
                                             _lib.ptr(self._fourier), _lib.ptr(self._tab), B, self.height, self.width, self.lmax,
                                             _lib.ptr(out), _lib.ptr(self._scratch(L, B)), _lib.current_stream()),
                       "eml_sh_analysis_f32")
        return out

    def _synthesis(self, coeffs, weighted):
        c = _lib.require_gpu_tensor(coeffs, "coeffs")
        B = c.shape[0]
        out = torch.empty(B, 3, self.height, self.width, dtype=torch.float32, device=c.device)
        if B > 0:
            _lib.check(_lib.lib().eml_sh_synthesis_f32(_lib.ptr(c), _lib.ptr(self._rows),
                                                       _lib.ptr(self._weights if weighted else None), _lib.ptr(self._fourier),
                                                       _lib.ptr(self._tab), B, self.height, self.width, self.lmax, _lib.ptr(out),
                                                       _lib.current_stream()), "eml_sh_synthesis_f32")
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

    def needlet_transform(self, jmax):
        """``(K_needlets, K)``: row 0 passes ``Y_00`` through, the row of needlet ``jk`` is
        ``sqrt(lambda_j) b(l / 2^j) Y_lm(xi_jk)`` (``spneedlet``, ``sphere_needlets.py:76-101``, for the real basis of this
        convention).  Built once per ``jmax`` from the basis kernel at the needlets' centres."""
        jmax = needlets._jmax(jmax)
        if jmax not in self._to_needlets:
            window = needlets.needlet_window(jmax)                         # (jmax + 1, 2^(jmax+1) + 1), column l
            lam = needlets.cubature_weights(jmax)                          # the needlets' own lambda_j
            scale = np.zeros((needlets.level_slices(jmax)[-1].stop, self.K))
            for j, rows in enumerate(needlets.level_slices(jmax)[1:]):
                for l, cols in enumerate(self.band_slices):
                    if l < window.shape[1]:
                        scale[rows, cols] = np.sqrt(lam[j]) * window[j, l]
            centres = np.concatenate([[[0.0, 0.0, 1.0]], needlets.cubature(jmax)], 0)
            T = self._matrix_at(self._upload(centres)) * self._upload(scale)
            T[0] = 0.0                                                     # row 0 of the needlet basis is Y_00 itself: set, not
            T[0, 0] = 1.0                                                  # left to 0 * (whatever the basis kernel wrote there)
            self._to_needlets[jmax] = T
        return self._to_needlets[jmax]

    def to_needlets(self, coeffs, jmax):
        """``Ctran_asymm`` (``sphere_needlets.py:254-277``) applied: ``(B, K, 3) -> (B, 4^(jmax+2) - 3, 3)``, the coefficients
        ``NeedletBasis(jmax)`` would give the function ``sum_k coeffs[k] Y_k``.  Degrees beyond ``2^(jmax+1)`` fall outside
        every window and are dropped."""
        self._check_coeffs(coeffs)
        return torch.matmul(self.needlet_transform(jmax), coeffs)


# ------------------------------------------------------------------------------------------------ command line
def coefficients_of_directory(pano_dir, out_dir, lmax=8, height=128, convention="graphics", fov=60.0, alpha=True, batch_size=8,
                              device="cuda:0"):
    """The harmonic coefficients of ``pano_dir/*.npy``, prepared as the needlet command line prepares them (area-resize to
    ``height x 2 height``, times the tonemap alpha of the crop at azimuth 0 unless ``alpha`` is false): writes
    ``out_dir/<name>.npy`` ``(K, 3)`` float32.  Returns the names written."""
    basis = HarmonicBasis(lmax=lmax, height=height, width=2 * height, convention=convention, device=device)
    os.makedirs(out_dir, exist_ok=True)
    names = []
    for batch_names, x in needlets.prepared_batches(pano_dir, basis.height, basis.width, fov, alpha, batch_size, device):
        host = basis.analysis(x).cpu().numpy()
        for q, name in enumerate(batch_names):
            np.save(os.path.join(out_dir, name + ".npy"), host[q])
            names.append(name)
    return names


def main(argv=None, device=None):
    ap = argparse.ArgumentParser(description="spherical-harmonic coefficients of a directory of HDR panoramas")
    ap.add_argument("--pano_dir", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--lmax", type=int, default=8)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--convention", choices=CONVENTIONS, default="graphics")
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--no_alpha", action="store_true", help="do not multiply by the crop's tonemap alpha")
    ap.add_argument("--batchSize", type=int, default=8)
    args = ap.parse_args(argv)
    from . import _runtime
    _runtime.entry_point_defaults()
    names = coefficients_of_directory(args.pano_dir, args.out_dir, args.lmax, args.height, args.convention, args.fov,
                                      not args.no_alpha, args.batchSize, device or "cuda:0")
    print("%d panoramas -> %s" % (len(names), args.out_dir))
    return names


if __name__ == "__main__":
    main()
