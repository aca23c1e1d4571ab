"""CPU: the spherical harmonics (csrc/harmonics.hip, ``emlight_amd.harmonics``) reach their C ABI entry points with arguments
that convert to the bound signatures -- WITHOUT a GPU; the launchers validate before touching a device; the float64 oracle of
the GPU tests equals the reference-made golden file in both conventions; the product's host-made tables, evaluated in float64
as the kernels evaluate them, give the oracle's matrix; the harmonics and the needlets are linked by the addition theorem.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_needlets_abi.py``, restated here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import harmonic_oracle as oracle
from tests import needlet_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"eml_sh_basis_f32": 6, "eml_sh_work_floats": 4, "eml_sh_analysis_f32": 12, "eml_sh_synthesis_f32": 11}


class _Recorder:
    def __init__(self, signatures):
        self.signatures, self.calls, self.args = signatures, [], []

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        restype, argtypes = self.signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, call site passes %d" % (name, len(argtypes), len(args))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s" % (name, k, a, t.__name__)) from e
            self.calls.append(name)
            self.args.append((name, args))
            return 64 if restype is ctypes.c_size_t else 0
        return call

    def of(self, name):
        return [a for n, a in self.args if n == name]


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib

    def require(t, name, dtype=None):      # the dtype check stays, the device check goes
        if t.dtype != (dtype or torch.float32):
            raise _lib.EmlightHipError("%s must be %s" % (name, dtype or torch.float32))
        return t.contiguous()
    rec = _Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", require)
    return rec


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "harmonics.npz"))


def close(got, want, tol=1e-9):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) <= tol * max(1.0, float(np.abs(want).max()))


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                 # the comments name the entry points too
    for name, nargs in NEW.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().eml_abi_version() == 31
    assert len(_lib.SIGNATURES) == 131
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme
    assert "harmonics.hip" in readme and "emlight_amd/harmonics.py" in readme and "python -m emlight_amd.harmonics" in readme
    # every section of the header cites the reference: one file:line per new entry point
    section = header[header.index("real spherical harmonics"):]
    assert len(re.findall(r"sphere_harmonics\.py:\d+", section)) >= 4


def test_a_library_without_the_new_symbols_is_refused(built_lib, monkeypatch):
    """Bound by name: a library from before this header fails at load, not at the first call."""
    from emlight_amd import _lib

    class Old:
        def __getattr__(self, name):
            if name in NEW:
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol eml_sh_"):
        _lib.lib()


# ------------------------------------------------------------------------------------------------ call paths
# eml_sh_basis_f32(dirs, P, tab, lmax, out, stream)
def test_matrix_call(recorder):
    from emlight_amd.harmonics import HarmonicBasis
    hb = HarmonicBasis(lmax=2, height=4, width=8, device="cpu")
    assert hb.K == 9 and hb.band_slices == [slice(0, 1), slice(1, 4), slice(4, 9)]
    m = hb.matrix()
    assert m.shape == (32, 9) and m.dtype == torch.float32 and recorder.calls == ["eml_sh_basis_f32"]
    a = recorder.of("eml_sh_basis_f32")[0]
    assert a[1] == 32 and a[3] == 2 and all(a[i] is not None for i in (0, 2, 4))
    assert hb.matrix(np.array([0.1, 0.2, 3.0]), [0.0, 1.0, 6.0]).shape == (3, 9)
    assert recorder.of("eml_sh_basis_f32")[1][1] == 3
    assert HarmonicBasis(device="cpu").K == 81 and HarmonicBasis(lmax=32, height=4, width=8, device="cpu").K == 1089


# eml_sh_analysis_f32(pano, rows, weights, fourier, tab, B, H, W, lmax, coeffs, work, stream)
# eml_sh_synthesis_f32(coeffs, rows, weights, fourier, tab, B, H, W, lmax, rec, stream)
def test_analysis_and_synthesis_calls_and_their_backward(recorder):
    from emlight_amd.harmonics import HarmonicBasis
    hb = HarmonicBasis(lmax=3, height=4, width=8, convention="symmetrised", device="cpu")
    x = torch.rand(3, 3, 4, 8, requires_grad=True)
    c = hb.analysis(x)
    assert c.shape == (3, 16, 3) and recorder.calls == ["eml_sh_work_floats", "eml_sh_analysis_f32"]
    assert recorder.of("eml_sh_work_floats")[0] == (4, 8, 3, 3)
    a = recorder.of("eml_sh_analysis_f32")[0]
    assert a[5:9] == (3, 4, 8, 3) and a[2] is not None and all(a[i] is not None for i in (0, 1, 3, 4, 9, 10))
    c.sum().backward()                                                   # the backward of the analysis is the weighted synthesis
    assert recorder.calls[-1] == "eml_sh_synthesis_f32" and x.grad.shape == x.shape
    s = recorder.of("eml_sh_synthesis_f32")[0]
    assert s[5:9] == (3, 4, 8, 3) and s[2] is not None
    hb.analysis(x.detach(), weighted=False)
    assert recorder.of("eml_sh_analysis_f32")[-1][2] is None              # a null weight pointer: w = 1
    co = torch.rand(2, 16, 3, requires_grad=True)
    r = hb.synthesis(co)
    assert r.shape == (2, 3, 4, 8) and recorder.of("eml_sh_synthesis_f32")[-1][2] is None
    r.sum().backward()                                                   # ... and the other way round, unweighted
    assert recorder.calls[-1] == "eml_sh_analysis_f32" and recorder.of("eml_sh_analysis_f32")[-1][2] is None
    assert co.grad.shape == co.shape
    assert hb.synthesis(co.detach(), weighted=True).shape == (2, 3, 4, 8)
    assert recorder.of("eml_sh_synthesis_f32")[-1][2] is not None
    n = len(recorder.calls)
    assert hb.analysis(torch.rand(0, 3, 4, 8)).shape == (0, 16, 3) and hb.synthesis(torch.rand(0, 16, 3)).shape == (0, 3, 4, 8)
    assert len(recorder.calls) == n                                      # B = 0: nothing to launch


def test_to_needlets_call(recorder):
    """The transform is built once per jmax from one call of the basis kernel at the 1 + 60 centres, then a matmul."""
    from emlight_amd.harmonics import HarmonicBasis
    hb = HarmonicBasis(lmax=4, height=4, width=8, device="cpu")
    out = hb.to_needlets(torch.rand(2, 25, 3), 1)
    assert out.shape == (2, 61, 3) and recorder.calls == ["eml_sh_basis_f32"] and recorder.of("eml_sh_basis_f32")[0][1] == 61
    T = hb.needlet_transform(1)
    assert T.shape == (61, 25) and float(T[0, 0]) == 1.0 and bool((T[0, 1:] == 0).all())
    hb.to_needlets(torch.rand(1, 25, 3), 1)
    assert recorder.calls == ["eml_sh_basis_f32"]
    assert hb.to_needlets(torch.rand(1, 25, 3), 0).shape == (1, 13, 3) and len(recorder.calls) == 2


def test_bad_arguments_raise_value_error(recorder):
    from emlight_amd.harmonics import HarmonicBasis, band_slices, convention_table
    for kw in ({"lmax": 33}, {"lmax": -1}, {"lmax": 1.5}, {"lmax": True}, {"grid": "healpix"}, {"convention": "complex"}, {"height": 0},
               {"width": 2.5}, {"height": 8192, "width": 4096}):
        with pytest.raises(ValueError):
            HarmonicBasis(**{"lmax": 2, "height": 4, "width": 8, "device": "cpu", **kw})
    with pytest.raises(ValueError):
        band_slices(33)
    with pytest.raises(ValueError):
        convention_table("complex")
    hb = HarmonicBasis(lmax=2, height=4, width=8, device="cpu")
    for bad in (torch.rand(3, 4, 8), torch.rand(1, 3, 4, 9), torch.rand(1, 4, 4, 8), np.zeros((1, 3, 4, 8))):
        with pytest.raises(ValueError):
            hb.analysis(bad)
    for bad in (torch.rand(9, 3), torch.rand(1, 8, 3), torch.rand(1, 9, 4)):
        with pytest.raises(ValueError):
            hb.synthesis(bad)
        with pytest.raises(ValueError):
            hb.to_needlets(bad, 1)
    with pytest.raises(ValueError):
        hb.to_needlets(torch.rand(1, 9, 3), 5)
    with pytest.raises(ValueError):
        hb.matrix(theta=[0.1])
    with pytest.raises(ValueError):
        hb.matrix([0.1, 0.2], [0.1])
    assert recorder.calls == []


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.harmonics import HarmonicBasis
    hb = HarmonicBasis(lmax=2, height=4, width=8, device="cpu")
    for call in (lambda: hb.matrix(), lambda: hb.analysis(torch.rand(1, 3, 4, 8)), lambda: hb.synthesis(torch.rand(1, 9, 3)),
                 lambda: hb.to_needlets(torch.rand(1, 9, 3), 1)):
        with pytest.raises(_lib.EmlightHipError):
            call()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def basis(dirs=one, P=8, tab=one, lmax=2, out=one):
        return L.eml_sh_basis_f32(dirs, P, tab, lmax, out, None)

    def analysis(pano=one, rows=one, w=None, four=one, tab=one, B=1, H=2, W=4, lmax=2, out=one, work=one):
        return L.eml_sh_analysis_f32(pano, rows, w, four, tab, B, H, W, lmax, out, work, None)

    def synthesis(co=one, rows=one, w=None, four=one, tab=one, B=1, H=2, W=4, lmax=2, out=one):
        return L.eml_sh_synthesis_f32(co, rows, w, four, tab, B, H, W, lmax, out, None)

    for fn, ptrs in ((basis, ("dirs", "tab", "out")), (analysis, ("pano", "rows", "four", "tab", "out", "work")),
                     (synthesis, ("co", "rows", "four", "tab", "out"))):
        for p in ptrs:
            assert fn(**{p: None}) == -1 and b"null" in L.eml_last_error(), (fn.__name__, p)
        for lmax in (-1, 33):
            assert fn(lmax=lmax) == -1 and b"lmax" in L.eml_last_error(), (fn.__name__, lmax)
    for P in (0, (1 << 24) + 1):
        assert basis(P=P) == -1 and b"P must be" in L.eml_last_error()
    for fn in (analysis, synthesis):
        for H, W in ((0, 4), (2, 0), (-1, -1), (4097, 4096), (1 << 24, 2)):
            assert fn(H=H, W=W) == -1 and b"P must be" in L.eml_last_error(), (fn.__name__, H, W)
        for B in (-1, 65536):
            assert fn(B=B) == -1 and b"grid limits" in L.eml_last_error(), (fn.__name__, B)
        assert fn(B=0) == 0                                               # empty batch: nothing to launch
        assert fn(B=0, lmax=33) == -1                                     # ... but still validated
    # scratch: (row blocks of 8) * K * 3B floats, a function of (H, W, lmax) per image
    wf = L.eml_sh_work_floats
    assert wf(0, 4, 2, 1) == 0 and wf(4, 0, 2, 1) == 0 and wf(4, 8, 33, 1) == 0 and wf(4, 8, -1, 1) == 0
    assert wf(4, 8, 2, 0) == 0 and wf(4, 8, 2, 65536) == 0 and wf(4097, 4096, 2, 1) == 0
    assert wf(4, 8, 2, 1) == 1 * 9 * 3 and wf(8, 8, 2, 1) == 27 and wf(9, 8, 2, 1) == 54
    assert wf(128, 256, 32, 8) == 8 * wf(128, 256, 32, 1) == 16 * 1089 * 24 and wf(128, 999, 32, 1) == wf(128, 256, 32, 1)


def test_the_gpu_cases_cross_the_tiling_boundaries(built_lib):
    """What the docstring of ``test_gpu_harmonics.py`` says of its shapes, from the constants the oracle's float32 restatement
    shares with the kernels (8 rows, 8 planes, chunks of 128 columns, 4 waves) and the scratch size the library reports."""
    wf = built_lib.eml_sh_work_floats
    assert (oracle.ROWS, oracle.PLANES, oracle.CHUNK, oracle.WAVES) == (8, 8, 128, 4)
    blocks = {c: wf(c[0], c[1], c[2], c[3]) // (3 * c[3] * (c[2] + 1) ** 2) for c in oracle.CASES}
    assert blocks == {c: -(-c[0] // 8) for c in oracle.CASES}
    assert {1, 2, 4, 8} <= set(blocks.values())                          # one ragged block ... eight full ones
    assert any(c[0] % 8 == 1 for c in oracle.CASES)                      # a last block of one row
    widths = {c[1] for c in oracle.CASES}
    assert min(widths) < 32 and 128 in widths and any(w > 128 for w in widths) and any(w % 2 for w in widths)
    planes = {3 * c[3] for c in oracle.CASES}
    assert {3, 6, 9, 33, 99} <= planes
    buckets = {min(b for b in (4, 8, 16, 32) if c[2] <= b) for c in oracle.CASES}
    assert buckets == {4, 8, 16, 32} and {0, 1, 32} <= {c[2] for c in oracle.CASES}
    assert set(oracle.ADJOINT_CASES) <= {c[:3] + (c[3],) for c in oracle.CASES} | {(25, 47, 8, 3)}


# ------------------------------------------------------------------------------------------------ the definition
def test_oracle_equals_the_reference_made_golden(golden):
    th, ph = oracle.golden_points(golden)
    assert th.shape == (24,) and th.min() == 0.0 and th.max() < np.pi and th.max() > np.pi - 2e-6
    assert ph.min() == 0.0 and ph.max() == 2 * np.pi
    seen = 0
    for conv, lmaxes in oracle.GOLDEN_POINTS.items():
        for lmax in lmaxes:
            want = golden["a/%s_l%d" % (conv, lmax)]
            assert want.shape == (24, (lmax + 1) ** 2) and close(oracle.matrix(th, ph, lmax, conv), want), (conv, lmax)
            seen += 1
    assert seen == 5 and 32 in oracle.GOLDEN_POINTS["symmetrised"]
    for H, W, lmax, conv in oracle.GOLDEN_GRIDS:
        im, want = golden["c/%dx%d_l%d/image" % (H, W, lmax)], golden["c/%dx%d_l%d/coeffs" % (H, W, lmax)]
        assert im.shape == (2, 3, H, W) and im.dtype == np.float32 and np.all(im[:, :, -1] == 0) and want.shape == (2, (lmax + 1) ** 2, 3)
        got = oracle.analysis(im, oracle.matrix(*oracle.grid_angles(H, W), lmax, conv), oracle.solid_angles(H, W))
        assert close(got, want), (H, W, lmax)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "harmonics.npz")) < 449008


def test_the_two_conventions_are_a_permutation_and_a_sign_of_each_other(golden):
    th, ph = oracle.golden_points(golden)
    for lmax in (1, 4, 32):
        perm, sign = oracle.conversion(lmax)
        assert sorted(perm) == list(range((lmax + 1) ** 2)) and set(sign) <= {1.0, -1.0}
        g, s = oracle.matrix(th, ph, lmax, "graphics"), oracle.matrix(th, ph, lmax, "symmetrised")
        assert np.array_equal(s, g[:, perm] * sign)
    # and so between the two reference-made files where both exist
    perm, sign = oracle.conversion(4)
    assert close(golden["a/symmetrised_l4"], golden["a/graphics_l4"][:, perm] * sign)
    # orthonormal: the Gram matrix of a Gauss-Legendre x uniform-phi quadrature that is exact to degree 2 lmax
    lmax, n = 8, 12
    x, w = np.polynomial.legendre.leggauss(n)
    phi = np.arange(2 * n) * np.pi / n
    T, P = np.meshgrid(np.arccos(x), phi, indexing="ij")
    for conv in oracle.CONVENTIONS:
        Y = oracle.matrix(T.reshape(-1), P.reshape(-1), lmax, conv)
        gram = Y.T @ (Y * np.repeat(w * np.pi / n, 2 * n)[:, None])
        assert np.abs(gram - np.eye(81)).max() < 1e-12, conv


def test_product_tables_evaluated_in_float64_give_the_oracle(golden):
    """The kernels' arithmetic on the product's own host-made tables, in float64: the basis kernel's route (powers of x + i y)
    at the golden points and the grid route (rows, Fourier table, convention table) on both grids."""
    from emlight_amd import harmonics as hm
    from emlight_amd import needlets as nd
    th, ph = oracle.golden_points(golden)

    def columns(tab, lmax, z, re_of, im_of):
        d, a, b, conv = tab[:33], tab[33:1122].reshape(33, 33), tab[1122:2211].reshape(33, 33), tab[2211:].reshape(33, 4)
        out = np.zeros((z.shape[0], (lmax + 1) ** 2))
        for m in range(lmax + 1):
            q0, q1 = np.zeros_like(z), np.full_like(z, d[m])
            for l in range(m, lmax + 1):
                if l > m:
                    q0, q1 = q1, a[m, l] * (z * q1 - b[m, l] * q0)
                out[:, l * l + l + int(conv[m, 0]) * m] = q1 * re_of(m) * conv[m, 1]
                if m:
                    out[:, l * l + l - int(conv[m, 0]) * m] = q1 * im_of(m) * conv[m, 2]
        return out

    for conv in hm.CONVENTIONS:
        tab = hm.device_table(conv)
        assert tab.shape == (2343,)
        x, y, z = nd.directions(th, ph).T
        power = [(x + 1j * y) ** m for m in range(33)]
        got = columns(tab, 32, z, lambda m: power[m].real, lambda m: power[m].imag)
        assert close(got, oracle.matrix(th, ph, 32, conv), 1e-11), conv
        for grid in hm.GRIDS:
            H, W, lmax = 7, 10, 9
            rows, four, w = hm.grid_tables(H, W, grid)
            assert rows.shape == (H, 2) and four.shape == (W, 33, 2) and w.shape == (H,)
            assert close(np.repeat(w, W), oracle.solid_angles(H, W), 1e-15)
            zz, ss = np.repeat(rows[:, 0], W), np.repeat(rows[:, 1], W)
            got = columns(tab, lmax, zz, lambda m: ss ** m * np.tile(four[:, m, 0], H), lambda m: ss ** m * np.tile(four[:, m, 1], H))
            assert close(got, oracle.matrix(*oracle.grid_angles(H, W, grid), lmax, conv), 1e-11), (conv, grid)
    rows = hm.grid_tables(5, 4, "reference")[0]
    assert np.array_equal(rows[0], [1.0, 0.0]) and np.array_equal(rows[-1], [-1.0, 0.0])     # the poles are the poles
    assert [(s.start, s.stop) for s in hm.band_slices(3)] == [(0, 1), (1, 4), (4, 9), (9, 16)]


def test_the_needlets_are_the_windowed_harmonics():
    """``[Y_00, Y(x) diag(sqrt(lambda_j) b(l / 2^j)) Y(xi_j)^T]`` is the needlet oracle's matrix (the addition theorem), in
    either convention; and ``to_needlets`` of the harmonic coefficients of a band-limited function gives its needlet
    coefficients.  This validates the two float64 oracles against each other, not the product: it runs no code of
    ``emlight_amd``.  The product is held to the same identity on the device, in
    ``test_gpu_harmonics.py::test_the_needlet_matrix_through_the_harmonics``."""
    g = np.random.default_rng(3)
    th, ph = np.arccos(g.uniform(-1, 1, 10)), g.uniform(0, 2 * np.pi, 10)
    for jmax in (1, 4):
        L = 2 ** (jmax + 1)
        want = needlet_oracle.matrix(th, ph, jmax)
        assert close(oracle.needlet_matrix_through_harmonics(th, ph, jmax), want, 1e-12), jmax
        sym = oracle.matrix(th, ph, L, "symmetrised") @ oracle.needlet_transform(L, jmax, "symmetrised").T
        assert close(sym, want, 1e-12), jmax
    T = oracle.needlet_transform(8, 1)
    assert T.shape == (61, 81) and T[0, 0] == 1.0 and np.all(T[0, 1:] == 0) and np.all(T[1:, 0] == 0)
    assert np.all(T[:, 25:] == 0) and np.abs(T[1:, 1:25]).max() > 0          # degrees beyond 2^(jmax+1) = 4 are dropped
    co = g.standard_normal((2, 81, 3))
    assert oracle.to_needlets(co, 8, 1).shape == (2, 61, 3) and np.array_equal(oracle.to_needlets(co, 8, 1)[:, 0], co[:, 0])


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_on_host_stand_ins(tmp_path, monkeypatch, capsys):
    from emlight_amd import harmonics, needlets
    panos, out = tmp_path / "panos", tmp_path / "coeffs"
    panos.mkdir()
    g = np.random.default_rng(5)
    for name in ("a", "b", "c"):
        np.save(str(panos / (name + ".npy")), g.random((8, 16, 3), dtype=np.float32))
    seen = {}

    class Batcher:
        PANO_HW = (128, 256)

        def small(self, pano, deg):
            assert deg == 0.0 and self.PANO_HW == (4, 8)
            return pano[:, ::2, ::2].contiguous()

        def crop(self, pano, deg, fov):
            assert deg == 0.0 and fov == 75.0
            return pano

        def tone(self, crop):
            return crop, torch.full((crop.shape[0],), 2.0)

    class Basis:
        def __init__(self, lmax, height, width, convention, device):
            seen["basis"] = (lmax, height, width, convention, device)
            self.height, self.width = height, width

        def analysis(self, x):
            assert x.is_contiguous() and x.shape[1:] == (3, 4, 8)
            return x.sum((2, 3))[:, None, :].repeat(1, 16, 1)

    monkeypatch.setattr(needlets, "_batcher", lambda fov, device: seen.setdefault("fov", fov) and Batcher())
    monkeypatch.setattr(harmonics, "HarmonicBasis", Basis)
    names = harmonics.main(["--pano_dir", str(panos), "--out_dir", str(out), "--lmax", "3", "--height", "4", "--fov", "75",
                            "--convention", "symmetrised", "--batchSize", "2"], device="cpu")
    assert names == ["a", "b", "c"] and "3 panoramas" in capsys.readouterr().out
    assert seen["basis"] == (3, 4, 8, "symmetrised", "cpu") and seen["fov"] == 75.0
    for name in names:
        got = np.load(str(out / (name + ".npy")))
        src = np.load(str(panos / (name + ".npy")))[::2, ::2]
        assert got.shape == (16, 3) and got.dtype == np.float32
        assert np.allclose(got[0], 2.0 * src.sum((0, 1)), rtol=1e-5)      # times the tonemap alpha
    harmonics.main(["--pano_dir", str(panos), "--out_dir", str(out), "--lmax", "3", "--height", "4", "--no_alpha", "--fov", "75"],
                   device="cpu")
    assert seen["basis"][3] == "graphics"
    src = np.load(str(panos / "a.npy"))[::2, ::2]
    assert np.allclose(np.load(str(out / "a.npy"))[0], src.sum((0, 1)), rtol=1e-5)
    with pytest.raises(SystemExit):
        harmonics.main(["--pano_dir", str(panos), "--out_dir", str(out), "--convention", "complex"], device="cpu")


def test_the_gpu_tolerances_are_the_measured_float32_floors(golden):
    """``FLOOR`` of test_gpu_harmonics.py is what the float32 restatement of the kernels' arithmetic reaches here, rounded up:
    one floor for every input the GPU file holds against a tolerance, measured on that input and for that operation."""
    from tests.test_gpu_harmonics import FLOOR, MARGIN
    measured = oracle.float32_floors(golden)
    cases = oracle.floor_cases()
    assert set(cases) == set(oracle.QUANTITIES) and all(len(set(v)) == len(v) for v in cases.values())
    assert MARGIN == 4.0 and set(FLOOR) == set(measured) == set(cases) | {"matrix"}
    assert {q: set(FLOOR[q]) for q in cases} == {q: {oracle.floor_key(*c) for c in v} for q, v in cases.items()}
    assert set(FLOOR["matrix"]) == set(oracle.CONVENTIONS)
    for conv in oracle.CONVENTIONS:
        assert set(FLOOR["matrix"][conv]) == set(oracle.MATRIX_LMAX) == {0, 1, 4, 8, 32}
        for lmax, v in measured["matrix"][conv].items():
            assert v <= FLOOR["matrix"][conv][lmax] <= 1.1 * v, (conv, lmax, v)
    for q in cases:
        for k, v in measured[q].items():
            assert v <= FLOOR[q][k] <= 1.1 * v, (q, k, v, FLOOR[q][k])
