"""CPU: the lighting evaluation (csrc/sphere_render.hip, ``emlight_amd.evaluate``) reaches its C ABI entry points with
arguments that convert to the bound signatures -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_projector_pano_abi.py``, restated here).  The
launchers' own argument validation is checked against the built library (it returns before anything touches a device), and
the float64 oracle of the GPU tests is checked against the closed forms a constant panorama has."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import sphere_render_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"eml_sphere_render_work_floats": 4, "eml_sphere_render_f32": 11, "eml_sphere_render_metrics_f64": 7}


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
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib().eml_abi_version()
    bits = {n: int(re.search(r"#define EML_SPHERE_%s (\d+)" % n.upper(), header).group(1)) for n in oracle.MATERIALS}
    from emlight_amd import evaluate
    assert bits == evaluate._BIT and evaluate.MATERIALS == oracle.MATERIALS
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "sphere_render" in readme and "emlight_amd/evaluate.py" in readme


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
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol eml_sphere_render"):
        _lib.lib()


# eml_sphere_render_f32(pano, B, H, W, S, view_azimuth_deg, materials_mask, phong_m, out, work, stream)
def test_render_spheres_call(recorder):
    from emlight_amd.evaluate import render_spheres
    out = render_spheres(torch.rand(3, 3, 16, 32), size=9)
    assert out.shape == (3, 3, 3, 9, 9) and out.dtype == torch.float32
    assert recorder.calls == ["eml_sphere_render_work_floats", "eml_sphere_render_f32"]
    assert recorder.of("eml_sphere_render_work_floats")[0] == (3, 16, 32, 9)
    a = recorder.of("eml_sphere_render_f32")[0]
    assert a[1:8] == (3, 16, 32, 9, 180.0, 7, 50.0) and a[8] is not None and a[9] is not None
    for names, bits in ((("diffuse",), 1), (("glossy",), 2), (("mirror",), 4), (("mirror", "diffuse"), 5), ("glossy", 2),
                        (("glossy", "mirror"), 6)):
        out = render_spheres(torch.rand(1, 3, 4, 8), size=4, materials=names, view_azimuth_deg=77, phong_exponent=3)
        assert out.shape == (1, 1 if isinstance(names, str) else len(names), 3, 4, 4)
        b = recorder.of("eml_sphere_render_f32")[-1]
        assert b[6] == bits and b[5] == 77.0 and b[7] == 3.0 and isinstance(b[5], float) and isinstance(b[7], float)
    n = len(recorder.calls)
    assert render_spheres(torch.rand(0, 3, 4, 8), size=4).shape == (0, 3, 3, 4, 4) and len(recorder.calls) == n   # nothing to launch


# eml_sphere_render_metrics_f64(pred_render, true_render, B, M, S, out, stream)
def test_lighting_metrics_call(recorder):
    from emlight_amd.evaluate import METRICS, lighting_metrics
    got = lighting_metrics(torch.rand(2, 3, 16, 32), torch.rand(2, 3, 16, 32), size=8, materials=("mirror", "glossy"))
    assert recorder.calls == ["eml_sphere_render_work_floats", "eml_sphere_render_f32", "eml_sphere_render_metrics_f64"]
    assert recorder.of("eml_sphere_render_f32")[0][1:8] == (4, 16, 32, 8, 180.0, 6, 50.0)      # both batches in one render call
    assert recorder.of("eml_sphere_render_metrics_f64")[0][2:5] == (2, 2, 8)
    assert list(got) == ["%s/%s" % (n, k) for n in ("mirror", "glossy") for k in METRICS]
    assert all(v.shape == (2,) and v.dtype == torch.float64 for v in got.values())
    assert set(lighting_metrics(torch.rand(1, 3, 4, 8), torch.rand(1, 3, 4, 8), size=4)) == {
        "%s/%s" % (n, k) for n in oracle.MATERIALS for k in ("rmse", "si_rmse", "angular", "used")}


def test_bad_shapes_and_names_raise_value_error(recorder):
    from emlight_amd.evaluate import lighting_metrics, render_metrics, render_spheres, sphere_mask
    ok = torch.rand(1, 3, 4, 8)
    for bad in (torch.rand(3, 4, 8), torch.rand(1, 4, 4, 8), torch.rand(1, 3, 4, 9), torch.rand(1, 3, 0, 0)):
        with pytest.raises(ValueError):
            render_spheres(bad, size=4)
    for kw in ({"size": 1}, {"size": 4.5}, {"materials": ()}, {"materials": ("diffuse", "chrome")}, {"materials": ("mirror", "mirror")},
               {"phong_exponent": -1.0}, {"phong_exponent": float("nan")}):
        with pytest.raises(ValueError):
            render_spheres(ok, **{"size": 4, **kw})
    with pytest.raises(ValueError):
        lighting_metrics(ok, torch.rand(2, 3, 4, 8), size=4)
    with pytest.raises(ValueError):
        lighting_metrics(ok, ok, size=4, materials=("silver",))
    with pytest.raises(ValueError):
        render_metrics(torch.rand(1, 3, 3, 4, 4), torch.rand(1, 2, 3, 4, 4))
    with pytest.raises(ValueError):
        render_metrics(torch.rand(1, 4, 3, 4, 4), torch.rand(1, 4, 3, 4, 4))
    with pytest.raises(ValueError):
        sphere_mask(1)
    assert recorder.calls == []


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.evaluate import lighting_metrics, render_metrics, render_spheres
    x = torch.rand(1, 3, 4, 8)
    with pytest.raises(_lib.EmlightHipError):
        render_spheres(x, size=4)
    with pytest.raises(_lib.EmlightHipError):
        lighting_metrics(x, x, size=4)
    with pytest.raises(_lib.EmlightHipError):
        render_metrics(torch.rand(1, 3, 3, 4, 4), torch.rand(1, 3, 3, 4, 4))


def test_sphere_mask_is_the_integer_test():
    from emlight_amd.evaluate import sphere_mask
    for S in (2, 3, 8, 9, 33, 64):
        m = sphere_mask(S)
        assert m.dtype == torch.bool and m.shape == (S, S) and np.array_equal(m.numpy(), oracle.mask(S))
    assert int(oracle.mask(64).sum()) == 3228 and int(oracle.mask(33).sum()) == 861 and int(oracle.mask(2).sum()) == 4


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def render(pano=one, B=1, H=16, W=32, S=8, az=180.0, mask=7, m=50.0, out=one, work=one):
        return L.eml_sphere_render_f32(pano, B, H, W, S, az, mask, m, out, work, None)

    for kw in ({"pano": None}, {"out": None}, {"work": None}):
        assert render(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert render(W=33) == -1 and b"W == 2H" in L.eml_last_error()
    assert render(H=0, W=0) == -1 and b"W == 2H" in L.eml_last_error()
    assert render(S=1) == -1 and b"S must be" in L.eml_last_error()
    for mask in (0, 8, -1):
        assert render(mask=mask) == -1 and b"materials mask" in L.eml_last_error(), mask
    assert render(m=-0.5) == -1 and b"phong" in L.eml_last_error()
    assert render(m=float("nan")) == -1 and b"phong" in L.eml_last_error()
    for kw in ({"B": -1}, {"B": 4097}, {"S": 1025}, {"H": 4097, "W": 8194}):
        assert render(**kw) == -1 and b"grid limits" in L.eml_last_error(), kw
    assert render(work=ctypes.c_void_p(20)) == -1 and b"aligned" in L.eml_last_error()
    assert render(B=0) == 0                                                 # empty batch: nothing to launch
    # texel table (4 H W) + pixel records (8 P) + the split's partial tiles (splits * 2 materials * P * 3B)
    assert L.eml_sphere_render_work_floats(0, 16, 32, 8) == 0 and L.eml_sphere_render_work_floats(1, 16, 33, 8) == 0
    assert L.eml_sphere_render_work_floats(1, 16, 32, 1) == 0
    P8, P33 = int(oracle.mask(8).sum()), int(oracle.mask(33).sum())
    assert L.eml_sphere_render_work_floats(3, 16, 32, 8) == 4 * 512 + 8 * P8 + 8 * 2 * P8 * 9          # 8 chunks of 64 texels
    assert L.eml_sphere_render_work_floats(2, 12, 24, 33) == 4 * 288 + 8 * P33 + 5 * 2 * P33 * 6       # 5 chunks, the last ragged
    # the split does not depend on the batch
    w1, w5 = L.eml_sphere_render_work_floats(1, 128, 256, 16), L.eml_sphere_render_work_floats(5, 128, 256, 16)
    fixed = 4 * 128 * 256 + 8 * int(oracle.mask(16).sum())
    assert (w5 - fixed) == 5 * (w1 - fixed)

    def metrics(a=one, b=one, B=1, M=3, S=8, out=one):
        return L.eml_sphere_render_metrics_f64(a, b, B, M, S, out, None)

    for kw in ({"a": None}, {"b": None}, {"out": None}):
        assert metrics(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert metrics(M=0) == -1 and metrics(M=4) == -1 and b"materials" in L.eml_last_error()
    assert metrics(S=1) == -1 and b"S must be" in L.eml_last_error()
    assert metrics(B=-1) == -1 and metrics(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    assert metrics(B=0) == 0


def test_the_oracle_has_the_closed_forms_of_a_constant_panorama():
    """A constant panorama renders to that constant under every material (both integrals are normalised to 1 over the
    sphere up to the quadrature's error), and the metrics of hand-made renders are what the formulas say."""
    pano = np.full((1, 3, 16, 32), 2.5)
    r = oracle.render(pano, 8)
    inside = oracle.mask(8)
    assert r.shape == (1, 3, 3, 8, 8) and np.all(r[..., ~inside] == 0)
    assert np.abs(r[0, 0][:, inside] / 2.5 - 1).max() < 5e-3 and np.abs(r[0, 1][:, inside] / 2.5 - 1).max() < 3e-2
    assert np.abs(r[0, 2][:, inside] - 2.5).max() < 1e-12
    # the mirror at the disc's centre looks back at the camera: azimuth 0 when the camera looks towards 180
    g = np.zeros((1, 3, 16, 32))
    g[0, :, :, 0] = g[0, :, :, 31] = 7.0
    centre = oracle.render(g, 9, ("mirror",))[0, 0, :, 4, 4]
    assert np.allclose(centre, 7.0)
    assert np.allclose(oracle.render(g, 9, ("mirror",), view_azimuth_deg=0.0)[0, 0, :, 4, 4], 0.0)
    a = np.zeros((1, 1, 3, 2, 2))
    b = np.zeros((1, 1, 3, 2, 2))
    a[0, 0, 0], b[0, 0, 1] = 1.0, 2.0                                   # red against green: orthogonal everywhere
    m = oracle.metrics(a, b)[0, 0]
    assert np.allclose(m, [np.sqrt(5 / 3), np.sqrt(4 / 3), 90.0, 4])
    assert np.allclose(oracle.metrics(3 * b, b)[0, 0], [np.sqrt(16 / 3), 0.0, 0.0, 4])
    assert np.allclose(oracle.metrics(0 * b, b)[0, 0], [np.sqrt(4 / 3), np.sqrt(4 / 3), 0.0, 0])


def test_command_line_on_host_stand_ins(tmp_path, monkeypatch, capsys):
    """Three panoramas, one prediction missing: the JSON has the keys, the per-image entries and a skipped count of 1."""
    from emlight_amd import evaluate
    panos, results = tmp_path / "panos", tmp_path / "results"
    panos.mkdir(), results.mkdir()
    g = np.random.default_rng(3)
    for name in ("a", "b", "c"):
        np.save(str(panos / (name + ".npy")), g.random((8, 16, 3), dtype=np.float32))
        if name != "b":
            np.save(str(results / ("pred_%s.npy" % name)), g.random((1, 3, 4, 8), dtype=np.float32))
    seen = {}

    class Batcher:
        def __call__(self, pano, deg=None):
            assert deg == 0.0
            return {"warped": pano.permute(0, 3, 1, 2)[:, :, ::2, ::2].contiguous()}

    def fake_metrics(pred, true, size=64, **kw):
        seen.setdefault("sizes", []).append((tuple(pred.shape), tuple(true.shape), size))
        v = (pred - true).abs().mean((1, 2, 3)).double()
        return {"%s/%s" % (n, k): v + i for i, n in enumerate(evaluate.MATERIALS) for k in evaluate.METRICS}

    monkeypatch.setattr(evaluate, "_batcher", lambda fov, device: seen.setdefault("fov", fov) and Batcher())
    monkeypatch.setattr(evaluate, "lighting_metrics", fake_metrics)
    out = str(tmp_path / "metrics.json")
    res = evaluate.main(["--pano_dir", str(panos), "--results_dir", str(results), "--fov", "75", "--size", "12", "--batchSize", "2",
                         "--out", out], device="cpu")
    said = capsys.readouterr().out
    assert "pred_b.npy" in said and "2 images evaluated, 1 skipped" in said and "si_rmse" in said
    disk = json.load(open(out))
    assert disk == json.loads(json.dumps(res))
    assert seen["fov"] == 75.0 and seen["sizes"] == [((1, 3, 4, 8), (1, 3, 4, 8), 12), ((1, 3, 4, 8), (1, 3, 4, 8), 12)]
    assert disk["skipped"] == 1 and disk["skipped_names"] == ["b"] and disk["evaluated"] == 2 and sorted(disk["images"]) == ["a", "c"]
    keys = {"%s/%s" % (n, k) for n in oracle.MATERIALS for k in ("rmse", "si_rmse", "angular", "used")}
    assert set(disk["means"]) == keys and all(set(v) == keys for v in disk["images"].values())
    for k in keys:
        assert disk["means"][k] == pytest.approx((disk["images"]["a"][k] + disk["images"]["c"][k]) / 2)
    assert disk["images"]["a"]["glossy/rmse"] == pytest.approx(disk["images"]["a"]["diffuse/rmse"] + 1)
    # a prediction of another shape is an error, not a silent resize
    np.save(str(results / "pred_b.npy"), np.zeros((1, 3, 8, 16), dtype=np.float32))
    with pytest.raises(ValueError, match="pred_b.npy"):
        evaluate.main(["--pano_dir", str(panos), "--results_dir", str(results)], device="cpu")
