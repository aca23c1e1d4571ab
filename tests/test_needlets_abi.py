"""CPU: the spherical needlets (csrc/needlets.hip, ``emlight_amd.needlets``) reach their C ABI entry points with arguments
that convert to the bound signatures -- WITHOUT a GPU; the launchers validate before touching a device; the float64 oracle of
the GPU tests equals the reference-made golden file; the HEALPix centres are what the published formulae say.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_sphere_render_abi.py``, restated here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import needlet_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"eml_needlet_basis_f32": 7, "eml_needlet_work_floats": 3, "eml_needlet_analysis_f32": 11,
       "eml_needlet_synthesis_f32": 10, "eml_needlet_sparsify_f32": 8}
KS = {0: 13, 1: 61, 2: 253, 3: 1021, 4: 4093}


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
    return np.load(os.path.join(ROOT, "tests", "golden", "needlets.npz"))


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
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "needlets.hip" in readme and "emlight_amd/needlets.py" in readme and "python -m emlight_amd.needlets" in readme


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
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol eml_needlet"):
        _lib.lib()


# ------------------------------------------------------------------------------------------------ call paths
# eml_needlet_basis_f32(dirs, P, centres, ctab, jmax, out, stream)
def test_matrix_call(recorder):
    from emlight_amd.needlets import NeedletBasis
    nb = NeedletBasis(jmax=1, height=4, width=8, device="cpu")
    assert nb.K == 61 and nb.level_slices == [slice(0, 1), slice(1, 13), slice(13, 61)]
    m = nb.matrix()
    assert m.shape == (32, 61) and m.dtype == torch.float32 and recorder.calls == ["eml_needlet_basis_f32"]
    a = recorder.of("eml_needlet_basis_f32")[0]
    assert a[1] == 32 and a[4] == 1 and all(a[i] is not None for i in (0, 2, 3, 5))
    assert nb.matrix(np.array([0.1, 0.2, 3.0]), [0.0, 1.0, 6.0]).shape == (3, 61)
    assert recorder.of("eml_needlet_basis_f32")[1][1] == 3


# eml_needlet_analysis_f32(pano, dirs, weights, B, P, centres, ctab, jmax, coeffs, work, stream)
# eml_needlet_synthesis_f32(coeffs, dirs, weights, B, P, centres, ctab, jmax, rec, stream)
def test_analysis_and_synthesis_calls_and_their_backward(recorder):
    from emlight_amd.needlets import NeedletBasis
    nb = NeedletBasis(jmax=2, height=4, width=8, device="cpu")
    x = torch.rand(3, 3, 4, 8, requires_grad=True)
    c = nb.analysis(x)
    assert c.shape == (3, 253, 3) and recorder.calls == ["eml_needlet_work_floats", "eml_needlet_analysis_f32"]
    assert recorder.of("eml_needlet_work_floats")[0] == (32, 2, 3)
    a = recorder.of("eml_needlet_analysis_f32")[0]
    assert a[3:5] == (3, 32) and a[7] == 2 and a[2] is not None and all(a[i] is not None for i in (0, 1, 5, 6, 8, 9))
    c.sum().backward()                                                   # the backward of the analysis is the weighted synthesis
    assert recorder.calls[-1] == "eml_needlet_synthesis_f32" and x.grad.shape == x.shape
    s = recorder.of("eml_needlet_synthesis_f32")[0]
    assert s[3:5] == (3, 32) and s[7] == 2 and s[2] is not None
    nb.analysis(x.detach(), weighted=False)
    assert recorder.of("eml_needlet_analysis_f32")[-1][2] is None         # a null weight pointer: w = 1
    n = len(recorder.of("eml_needlet_work_floats"))
    nb.analysis(x.detach())
    assert len(recorder.of("eml_needlet_work_floats")) == n + 1            # sized per call, the tensor itself is reused
    co = torch.rand(2, 253, 3, requires_grad=True)
    r = nb.synthesis(co)
    assert r.shape == (2, 3, 4, 8) and recorder.of("eml_needlet_synthesis_f32")[-1][2] is None
    r.sum().backward()                                                   # ... and the other way round, unweighted
    assert recorder.calls[-1] == "eml_needlet_analysis_f32" and recorder.of("eml_needlet_analysis_f32")[-1][2] is None
    assert co.grad.shape == co.shape
    assert nb.synthesis(co.detach(), weighted=True).shape == (2, 3, 4, 8)
    assert recorder.of("eml_needlet_synthesis_f32")[-1][2] is not None
    n = len(recorder.calls)
    assert nb.analysis(torch.rand(0, 3, 4, 8)).shape == (0, 253, 3) and nb.synthesis(torch.rand(0, 253, 3)).shape == (0, 3, 4, 8)
    assert len(recorder.calls) == n                                      # B = 0: nothing to launch


# eml_needlet_sparsify_f32(coeffs, B, jmax, levels_mask, ratio, out, kept, stream)
def test_sparsify_call(recorder):
    from emlight_amd.needlets import NeedletBasis
    nb = NeedletBasis(jmax=3, height=4, width=8, device="cpu")
    out, kept = nb.sparsify(torch.rand(2, 1021, 3))
    assert out.shape == (2, 1021, 3) and kept.shape == (2, 4) and kept.dtype == torch.int32
    a = recorder.of("eml_needlet_sparsify_f32")[0]
    assert a[1:5] == (2, 3, 12, 0.1) and isinstance(a[4], float)
    nb.sparsify(torch.rand(1, 1021, 3), ratio=1, levels=[0])
    assert recorder.of("eml_needlet_sparsify_f32")[1][1:5] == (1, 3, 1, 1.0)
    n = len(recorder.calls)
    assert nb.sparsify(torch.rand(0, 1021, 3))[1].shape == (0, 4) and len(recorder.calls) == n


def test_bad_arguments_raise_value_error(recorder):
    from emlight_amd.needlets import NeedletBasis, antipodal_pairs, cubature, healpix_ring_centres, needlet_window
    for kw in ({"jmax": 5}, {"jmax": -1}, {"jmax": 1.5}, {"grid": "healpix"}, {"height": 0}, {"width": 2.5}, {"height": 8192, "width": 4096}):
        with pytest.raises(ValueError):
            NeedletBasis(**{"jmax": 1, "height": 4, "width": 8, "device": "cpu", **kw})
    for fn in (needlet_window, cubature, antipodal_pairs):
        with pytest.raises(ValueError):
            fn(5)
    with pytest.raises(ValueError):
        healpix_ring_centres(3)
    nb = NeedletBasis(jmax=1, height=4, width=8, device="cpu")
    for bad in (torch.rand(3, 4, 8), torch.rand(1, 3, 4, 9), torch.rand(1, 4, 4, 8), np.zeros((1, 3, 4, 8))):
        with pytest.raises(ValueError):
            nb.analysis(bad)
    for bad in (torch.rand(61, 3), torch.rand(1, 60, 3), torch.rand(1, 61, 4)):
        with pytest.raises(ValueError):
            nb.synthesis(bad)
        with pytest.raises(ValueError):
            nb.sparsify(bad, levels=(1,))
    ok = torch.rand(1, 61, 3)
    for kw in ({"ratio": -0.1}, {"ratio": 1.5}, {"ratio": float("nan")}, {"levels": (2,)}, {"levels": (1, 1)}, {"levels": (0.5,)},
               {}):                                                      # the default levels (2, 3) do not exist at jmax = 1
        with pytest.raises(ValueError):
            nb.sparsify(ok, **kw)
    with pytest.raises(ValueError):
        nb.matrix(theta=[0.1])
    with pytest.raises(ValueError):
        nb.matrix([0.1, 0.2], [0.1])
    assert recorder.calls == []


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.needlets import NeedletBasis
    nb = NeedletBasis(jmax=1, height=4, width=8, device="cpu")
    for call in (lambda: nb.matrix(), lambda: nb.analysis(torch.rand(1, 3, 4, 8)), lambda: nb.synthesis(torch.rand(1, 61, 3)),
                 lambda: nb.sparsify(torch.rand(1, 61, 3), levels=(1,))):
        with pytest.raises(_lib.EmlightHipError):
            call()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(20)

    def basis(dirs=one, P=8, cen=one, tab=one, jmax=1, out=one):
        return L.eml_needlet_basis_f32(dirs, P, cen, tab, jmax, out, None)

    def analysis(pano=one, dirs=one, w=None, B=1, P=8, cen=one, tab=one, jmax=1, out=one, work=one):
        return L.eml_needlet_analysis_f32(pano, dirs, w, B, P, cen, tab, jmax, out, work, None)

    def synthesis(co=one, dirs=one, w=None, B=1, P=8, cen=one, tab=one, jmax=1, out=one):
        return L.eml_needlet_synthesis_f32(co, dirs, w, B, P, cen, tab, jmax, out, None)

    def sparsify(co=one, B=1, jmax=3, mask=12, ratio=0.1, out=one, kept=one):
        return L.eml_needlet_sparsify_f32(co, B, jmax, mask, ratio, out, kept, None)

    for fn, ptrs in ((basis, ("dirs", "cen", "tab", "out")), (analysis, ("pano", "dirs", "cen", "tab", "out", "work")),
                     (synthesis, ("co", "dirs", "cen", "tab", "out")), (sparsify, ("co", "out", "kept"))):
        for p in ptrs:
            assert fn(**{p: None}) == -1 and b"null" in L.eml_last_error(), (fn.__name__, p)
        for jmax in (-1, 5):
            assert fn(jmax=jmax) == -1 and b"jmax" in L.eml_last_error(), (fn.__name__, jmax)
    for fn in (basis, analysis, synthesis):
        assert fn(P=0) == -1 and b"P must be" in L.eml_last_error()
        assert fn(P=(1 << 24) + 1) == -1 and b"P must be" in L.eml_last_error()
        assert fn(cen=odd) == -1 and b"aligned" in L.eml_last_error()
    for fn in (analysis, synthesis, sparsify):
        for B in (-1, 65536):
            assert fn(B=B) == -1 and b"grid limits" in L.eml_last_error(), (fn.__name__, B)
        assert fn(B=0) == 0                                               # empty batch: nothing to launch
    assert analysis(work=odd) == -1 and b"aligned" in L.eml_last_error()
    for mask in (-1, 16):
        assert sparsify(mask=mask) == -1 and b"levels mask" in L.eml_last_error()
    assert sparsify(jmax=1, mask=4) == -1 and b"levels mask" in L.eml_last_error()
    for ratio in (-0.5, 1.5, float("nan")):
        assert sparsify(ratio=ratio) == -1 and b"ratio" in L.eml_last_error()
    # scratch: splits * K * 3B floats; the split depends on (P, jmax) only
    wf = L.eml_needlet_work_floats
    assert wf(0, 1, 1) == 0 and wf(8, 5, 1) == 0 and wf(8, 1, 0) == 0 and wf(8, 1, 65536) == 0
    assert wf(288, 1, 2) == 5 * 61 * 6                                    # 5 chunks of 64 pixels, the last ragged
    assert wf(512, 3, 1) == 8 * 1021 * 3 and wf(2048, 2, 11) == 32 * 253 * 33
    assert wf(128 * 256, 3, 5) == 5 * wf(128 * 256, 3, 1) == 5 * 64 * 1021 * 3


def test_the_gpu_cases_reach_the_chunk_loop_of_the_analysis(built_lib):
    """The analysis stages 64 pixels per chunk and gives each split ``per`` chunks.  Only with ``per >= 2`` does the kernel's
    chunk loop come round again (the prefetch of the next chunk, the barrier before the staging buffer is overwritten, a last
    split that is clipped).  The plan is not exported, its scratch size is: ``work_floats(P, jmax, 1) = splits * K * 3``, and
    ``per >= 2`` exactly when there are fewer splits than chunks.  If the plan's constants move, this says that the GPU cases
    of ``test_gpu_needlets.py`` no longer cover the loop."""
    wf = built_lib.eml_needlet_work_floats

    def splits_and_chunks(H, W, jmax):
        floats = wf(H * W, jmax, 1)
        assert floats > 0 and floats % (3 * KS[jmax]) == 0, (H, W, jmax, floats)
        return floats // (3 * KS[jmax]), -(-H * W // 64)

    assert oracle.PER2_SHAPES == [(25, 47, 4), (50, 100, 1), (48, 96, 0)]
    assert [splits_and_chunks(*c) for c in oracle.PER2_SHAPES] == [(10, 19), (40, 79), (36, 72)]      # each < its chunk count
    for H, W, jmax in oracle.PER2_SHAPES:
        assert (H, W, jmax) in {c[:3] for c in oracle.ANALYSIS_CASES}, "a per >= 2 shape no analysis test runs"
        splits, chunks = splits_and_chunks(H, W, jmax)
        assert splits < chunks, (H, W, jmax, splits, chunks)
    assert {c[:3] for c in oracle.ADJOINT_CASES} >= set(oracle.PER2_SHAPES[:2])
    one_chunk_per_split = [(12, 24, 1), (12, 24, 2), (16, 32, 3), (32, 64, 2)] + oracle.ONE_CHUNK_SHAPES
    for H, W, jmax in one_chunk_per_split:
        splits, chunks = splits_and_chunks(H, W, jmax)
        assert splits == chunks, (H, W, jmax, splits, chunks)
    assert [splits_and_chunks(*c)[1] for c in oracle.ONE_CHUNK_SHAPES] == [1, 1]
    every = {c[:3] for c in oracle.ANALYSIS_CASES + oracle.COLUMN_GROUP_CASES + oracle.ADJOINT_CASES} | set(oracle.GOLDEN_SHAPES)
    assert every == set(oracle.PER2_SHAPES) | set(one_chunk_per_split), "a shape of the GPU file this test does not classify"


# ------------------------------------------------------------------------------------------------ the definition
def test_oracle_equals_the_reference_made_golden(golden):
    for jmax in (1, 2, 3, 4):
        got = oracle.matrix(golden["a/j%d/theta" % jmax], golden["a/j%d/phi" % jmax], jmax)
        want = golden["a/j%d/matrix" % jmax]
        assert want.shape == (24 if jmax < 4 else 6, KS[jmax]) and close(got, want), jmax
        assert golden["a/j%d/theta" % jmax].max() < np.pi and golden["a/j%d/theta" % jmax].min() == 0.0
    assert close(oracle.window(4), golden["b/window"])
    for H, W, jmax in ((12, 24, 1), (12, 24, 2), (16, 32, 3)):
        im, want = golden["c/%dx%d_j%d/image" % (H, W, jmax)], golden["c/%dx%d_j%d/coeffs" % (H, W, jmax)]
        assert im.shape == (2, 3, H, W) and im.dtype == np.float32 and np.all(im[:, :, -1] == 0) and want.shape == (2, KS[jmax], 3)
        got = oracle.analysis(im, oracle.matrix(*oracle.grid_angles(H, W), jmax), oracle.solid_angles(H, W))
        assert close(got, want), (H, W, jmax)


def test_product_tables_equal_the_oracle(golden):
    from emlight_amd import needlets as nd
    for jmax in range(5):
        assert np.abs(nd.cubature(jmax) - oracle.centres(jmax)[1:]).max() < 1e-14
        tab = nd.coefficient_table(jmax)
        assert tab.shape == (jmax + 2, 33) and np.all(tab[:, 2 ** (jmax + 1) + 1:] == 0)
        assert close(tab[:, :2 ** (jmax + 1) + 1], oracle.zonal_coefficients(jmax), 1e-12)
        assert [(s.start, s.stop) for s in nd.level_slices(jmax)] == [(s.start, s.stop) for s in oracle.level_slices(jmax)]
        assert nd.level_slices(jmax)[-1].stop == KS[jmax] == oracle.rows(jmax)
    w = nd.needlet_window(4)
    assert w.shape == (5, 33) and np.all(w[:, 0] == 0) and close(w[:, 1:], golden["b/window"])
    assert w[0, 1] == 1.0 and np.all(w[0, 2:] == 0)                       # b(1) = 1, b(2) = 0
    for H, W in ((12, 24), (5, 7)):
        assert close(nd.solid_angles(H, W), oracle.solid_angles(H, W), 1e-15)
        assert abs(nd.solid_angles(H, W).sum() - 4 * np.pi) < 1e-12
        for grid in nd.GRIDS:
            th, ph = nd.grid_angles(H, W, grid)
            oth, oph = oracle.grid_angles(H, W, grid)
            assert np.array_equal(th, oth) and np.array_equal(ph, oph)
            assert np.abs(nd.directions(th, ph) - oracle.directions(oth, oph)).max() < 1e-15
    d = nd.directions(np.array([0.0, np.pi, np.pi]), np.array([0.3, 0.0, 5.0]))
    assert np.array_equal(d, [[0, 0, 1], [0, 0, -1], [0, 0, -1]])          # the poles themselves, whatever phi


def test_healpix_facts():
    from emlight_amd.needlets import antipodal_pairs, cubature, healpix_ring_centres
    k = np.arange(4)

    def zphi(v):
        return v[:, 2], np.mod(np.arctan2(v[:, 1], v[:, 0]), 2 * np.pi)

    z, phi = zphi(healpix_ring_centres(1))
    assert np.allclose(z, np.repeat([2 / 3, 0, -2 / 3], 4), atol=1e-15)
    assert np.allclose(phi[:4], np.pi / 4 + k * np.pi / 2) and np.allclose(phi[4:8], k * np.pi / 2, atol=1e-15)
    assert np.allclose(phi[8:], np.pi / 4 + k * np.pi / 2)
    z, phi = zphi(healpix_ring_centres(2))
    k8 = np.arange(8)
    assert np.allclose(z[:4], 11 / 12) and np.allclose(z[4:12], 2 / 3) and np.allclose(z[12:20], 1 / 3)
    assert np.allclose(phi[4:12], (k8 + 0.5) * np.pi / 4) and np.allclose(phi[12:20], k8 * np.pi / 4, atol=1e-15)
    for nside in (1, 2, 4, 8, 16):
        v = healpix_ring_centres(nside)
        assert v.shape == (12 * nside * nside, 3) and np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-15)
        assert np.abs(v - oracle.ring_centres(nside)).max() < 1e-14
        assert np.abs(v.sum(0)).max() < 1e-11
        corr = v @ v.T
        anti = corr + 1 < 1e-10                                           # the reference's test, sphere_needlets.py:123
        assert np.all(anti.sum(1) == 1)
    for jmax in (0, 1, 3):
        pair, use = antipodal_pairs(jmax)
        xi = cubature(jmax)
        assert pair.shape == (KS[jmax] - 1,) and np.array_equal(pair[pair], np.arange(len(pair)))
        assert np.abs(xi[pair] + xi).max() < 1e-14
        assert np.array_equal(use, [i for i in range(len(pair)) if pair[i] > i]) and 2 * len(use) == len(pair)
        # the reference's own search (sphere_needlets.py:119-126)
        corr = xi @ xi.T
        assert np.array_equal(pair, [np.where(corr[i] + 1 < 1e-10)[0][0] for i in range(len(xi))])


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_on_host_stand_ins(tmp_path, monkeypatch, capsys):
    from emlight_amd import needlets
    panos, out = tmp_path / "panos", tmp_path / "coeffs"
    panos.mkdir()
    g = np.random.default_rng(5)
    for name in ("a", "b", "c"):
        np.save(str(panos / (name + ".npy")), g.random((8, 16, 3), dtype=np.float32))
    seen = {"sparsify": []}

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
        def __init__(self, jmax, height, width, device):
            seen["basis"] = (jmax, height, width, device)
            self.jmax, self.height, self.width = jmax, height, width

        def analysis(self, x):
            assert x.is_contiguous() and x.shape[1:] == (3, 4, 8)
            return x.sum((2, 3))[:, None, :].repeat(1, 253, 1)

        def sparsify(self, coeffs, ratio, levels):
            seen["sparsify"].append((ratio, levels))
            return coeffs * 0, None

    monkeypatch.setattr(needlets, "_batcher", lambda fov, device: seen.setdefault("fov", fov) and Batcher())
    monkeypatch.setattr(needlets, "NeedletBasis", Basis)
    names = needlets.main(["--pano_dir", str(panos), "--out_dir", str(out), "--jmax", "2", "--height", "4", "--fov", "75",
                           "--batchSize", "2"], device="cpu")
    assert names == ["a", "b", "c"] and "3 panoramas" in capsys.readouterr().out
    assert seen["basis"] == (2, 4, 8, "cpu") and seen["fov"] == 75.0 and seen["sparsify"] == []
    for name in names:
        got = np.load(str(out / (name + ".npy")))
        src = np.load(str(panos / (name + ".npy")))[::2, ::2]
        assert got.shape == (253, 3) and got.dtype == np.float32
        assert np.allclose(got[0], 2.0 * src.sum((0, 1)), rtol=1e-5)      # times the tonemap alpha
    needlets.main(["--pano_dir", str(panos), "--out_dir", str(out), "--jmax", "2", "--height", "4", "--no_alpha", "--sparsify",
                   "0.25", "--fov", "75"], device="cpu")
    assert seen["sparsify"] == [(0.25, (2,))] and np.all(np.load(str(out / "a.npy")) == 0)
    with pytest.raises(ValueError, match="sparsify"):
        needlets.main(["--pano_dir", str(panos), "--out_dir", str(out), "--jmax", "1", "--height", "4", "--sparsify", "0.1"],
                      device="cpu")


def test_the_gpu_tolerances_are_the_measured_float32_floors(golden):
    """``FLOOR`` of test_gpu_needlets.py is what the float32 restatement of the kernels' arithmetic reaches here, rounded up:
    one floor for every input the GPU file holds against an analysis or a synthesis tolerance, measured on that input."""
    from tests.test_gpu_needlets import FLOOR, MARGIN
    measured = oracle.float32_floors(golden)
    cases = oracle.floor_cases()
    assert all(len(set(v)) == len(v) for v in cases.values())
    assert {q: set(FLOOR[q]) for q in cases} == {q: {oracle.floor_key(*c) for c in v} for q, v in cases.items()}
    assert set(FLOOR["matrix"]) == {0, 1, 2, 3, 4}
    assert MARGIN == 4.0 and {q: set(v) for q, v in FLOOR.items()} == {q: set(v) for q, v in measured.items()}
    for q, table in measured.items():
        for k, v in table.items():
            assert v <= FLOOR[q][k] <= 1.1 * v, (q, k, v, FLOOR[q][k])
