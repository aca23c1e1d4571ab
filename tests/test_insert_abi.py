"""CPU: object insertion (csrc/env_prefilter.hip, csrc/gbuffer_shade.hip, ``emlight_amd/insert.py``) WITHOUT a GPU.

* The three entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported; the
  first header and its 131 names are untouched.
* Every refusal of the launchers runs against the built library (they return before anything touches a device).
* The Python layer reaches the entry points with arguments that convert to the bound signatures (the recorder of
  ``test_pano_warp_abi.py``, restated here), and the command line is parsed and dispatched against it.
* ``tests/insert_oracle.py``, the yardstick of the GPU tests, is pinned to what exists: section 15's sphere frames,
  ``crop_panorama``'s rays, quadrature sums computed independently, texel centres."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import insert_oracle as oracle
from tests import sphere_render_oracle as sro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK, PREFILTER, SHADE = "eml_env_prefilter_work_floats", "eml_env_prefilter_f32", "eml_gbuffer_shade_f32"
NARGS = {WORK: 5, PREFILTER: 10, SHADE: 24}


# ------------------------------------------------------------------------------------------------ where the symbols live
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_in_the_extension_header_bound_and_exported(built_lib):
    from emlight_amd import _lib
    ext = open(os.path.join(ROOT, "include", "emlight_hip_ext.h")).read()
    first = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    declared = sorted(set(re.findall(r"\b(eml_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(_lib.EXT_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in NARGS.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == n, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES[WORK][0] is ctypes.c_size_t
    # the declarations cite the DESIGN section and the reference lines they generalise
    assert "DESIGN.md section 22" in ext and "RegressionNetwork/util.py:157-174" in ext
    # the first header, its table and the ABI version are untouched
    assert not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 131
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme and "env_prefilter.hip" in readme and "gbuffer_shade.hip" in readme
    assert "emlight_amd/insert.py" in readme and "python -m emlight_amd.insert" in readme
    assert all(n in readme for n in (PREFILTER, SHADE))


def test_a_library_without_a_symbol_is_refused(built_lib, monkeypatch):
    from emlight_amd import _lib

    class Old:
        def __getattr__(self, name):
            if name == SHADE:
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EmlightHipError, match="lacks symbol %s" % SHADE):
        _lib.lib()


def test_prefilter_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    diffuse_phong = (ctypes.c_double * 2)(-1.0, 50.0)

    def pre(pano=one, B=1, H=4, W=8, Ho=2, nl=2, lobes=diffuse_phong, out=one, work=one):
        return L.eml_env_prefilter_f32(pano, B, H, W, Ho, nl, lobes, out, work, None)

    for kw in ({"pano": None}, {"lobes": None}, {"out": None}, {"work": None}):
        assert pre(**kw) == -1 and b"null" in L.eml_last_error(), kw
    for kw in ({"W": 9}, {"H": 0, "W": 0}):
        assert pre(**kw) == -1 and b"W == 2H" in L.eml_last_error(), kw
    for kw in ({"nl": 0}, {"nl": 9}):
        assert pre(**kw) == -1 and b"lobes" in L.eml_last_error(), kw
    for kw in ({"B": -1}, {"B": 4097}, {"H": 4097, "W": 8194}, {"Ho": 0}, {"Ho": 1025}):
        assert pre(**kw) == -1 and b"limits" in L.eml_last_error(), kw
    for bad in (math.nan, 1e7, math.inf):
        assert pre(lobes=(ctypes.c_double * 2)(-1.0, bad)) == -1 and b"lobe 1" in L.eml_last_error(), bad
    assert pre(work=ctypes.c_void_p(20)) == -1 and b"16-byte" in L.eml_last_error()
    assert pre(B=0) == 0                                       # empty batch: nothing to launch
    # the scratch size: tables of both grids and two slots per split; 0 for a refused size
    w = L.eml_env_prefilter_work_floats
    assert w(0, 4, 8, 2, 2) == 0 and w(1, 4, 9, 2, 2) == 0 and w(1, 4, 8, 0, 2) == 0 and w(1, 4, 8, 2, 9) == 0
    assert w(1, 4, 8, 2, 1) == 4 * 32 + 4 * 8 + 1 * 2 * 8 * 3          # 32 texels: one chunk, one split
    assert w(2, 4, 8, 2, 1) - w(1, 4, 8, 2, 1) == 2 * 8 * 3 and w(1, 4, 8, 2, 8) == w(1, 4, 8, 2, 1)   # passes reuse it
    # the split is a function of (H, Ho) alone: the per-image scratch is the same for every batch and lobe count
    per_image = [(w(B, 128, 256, 4, nl) - 4 * 32768 - 4 * 32) // (2 * 32 * 3 * B) for B in (1, 2, 33) for nl in (1, 2, 5)]
    assert len(set(per_image)) == 1 and per_image[0] > 1


def test_shade_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    base = dict(pano=one, H=4, ed=one, Hd=2, ds=24, eg=one, Hg=2, gs=24, normal=one, coverage=one, kd=one, ks=one, km=one, B=1,
                h=4, w=6, fov=60.0, az=180.0, shaded=one, bg=None, ex=None, gamma=2.4, comp=None)

    def shade(**kw):
        a = dict(base, **kw)
        return L.eml_gbuffer_shade_f32(a["pano"], a["H"], a["ed"], a["Hd"], a["ds"], a["eg"], a["Hg"], a["gs"], a["normal"],
                                       a["coverage"], a["kd"], a["ks"], a["km"], a["B"], a["h"], a["w"], a["fov"], a["az"],
                                       a["shaded"], a["bg"], a["ex"], a["gamma"], a["comp"], None)

    def refused(word, **kw):
        assert shade(**kw) == -1 and word in L.eml_last_error(), (kw, L.eml_last_error())

    refused(b"null normal or coverage", normal=None)
    refused(b"null normal or coverage", coverage=None)
    refused(b"null outputs", shaded=None)
    refused(b"no coefficient", kd=None, ks=None, km=None)                       # composite alone needs both tensors
    refused(b"no coefficient", kd=None, ks=None, km=None, shaded=None, comp=one, bg=one, ex=one)
    for kw in ({"ed": None}, {"Hd": 0}, {"Hd": 4097}, {"ds": 23}):
        refused(b"kd needs e_diffuse", **kw)
    for kw in ({"eg": None}, {"Hg": 0}, {"gs": 23}):
        refused(b"ks needs e_phong", **kw)
    for kw in ({"pano": None}, {"H": 0}, {"H": 4097}):
        refused(b"km needs pano", **kw)
    refused(b"composite needs", comp=one, bg=one)
    refused(b"composite needs", comp=one, ex=one)
    refused(b"need the composite output", bg=one)
    refused(b"need the composite output", ex=one)
    for g in (0.0, -1.0, math.nan, math.inf):
        refused(b"gamma", comp=one, bg=one, ex=one, gamma=g)
    for kw in ({"fov": -1.0}, {"fov": 180.0}, {"fov": math.nan}, {"az": math.nan}, {"az": math.inf}):
        refused(b"fov_deg", **kw)
    refused(b"grid.y", B=-1)
    refused(b"grid.y", B=65536)
    for kw in ({"h": 1}, {"w": 1}, {"h": 1 << 15, "w": (1 << 14) + 1}):
        refused(b"image size", **kw)
    # consistent sets that are fine, on an empty batch: nothing to launch
    assert shade(B=0) == 0
    assert shade(B=0, kd=None, ed=None, Hd=0, ds=0) == 0 and shade(B=0, ks=None, km=None, eg=None, pano=None) == 0
    assert shade(B=0, comp=one, bg=one, ex=one, shaded=None) == 0
    assert shade(B=0, kd=None, ks=None, km=None, normal=None, comp=one, bg=one, ex=one, gamma=1.0) == 0   # composite alone
    assert shade(B=0, gamma=math.nan) == 0                                      # unused without the composite


# ------------------------------------------------------------------------------------------------ recorder
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
    rec = _Recorder({**_lib.SIGNATURES, **_lib.EXT_SIGNATURES})
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", require)
    return rec


def _val(p):
    return None if p is None else p.value


def test_prefilter_environment_call(recorder):
    from emlight_amd import insert
    pano = torch.rand(3, 3, 8, 16)
    out = insert.prefilter_environment(pano, height=4, lobes=("diffuse", 50, 0.0))
    assert out.shape == (3, 3, 3, 4, 8) and out.dtype == torch.float32
    assert recorder.calls == [WORK, PREFILTER]
    assert recorder.of(WORK)[0] == (3, 8, 16, 4, 3)
    a = recorder.of(PREFILTER)[0]
    assert a[0].value == pano.data_ptr() and a[1:6] == (3, 8, 16, 4, 3) and a[7].value == out.data_ptr()
    assert list(a[6]) == [-1.0, 50.0, 0.0]                                       # the host array of doubles
    assert insert.prefilter_environment(pano).shape == (3, 1, 3, 32, 64)          # defaults: the irradiance map at 32
    assert list(recorder.of(PREFILTER)[1][6]) == [-1.0]
    assert insert.prefilter_environment(pano, 4, 7.5).shape == (3, 1, 3, 4, 8)    # a single lobe, not in a tuple
    n = len(recorder.calls)
    assert insert.prefilter_environment(torch.rand(0, 3, 8, 16), 4).shape == (0, 1, 3, 4, 8) and len(recorder.calls) == n
    for kw in ({"lobes": ()}, {"lobes": ("glossy",)}, {"lobes": (-1.0,)}, {"lobes": (math.nan,)}, {"lobes": (1,) * 9},
               {"height": 0}, {"height": 2.5}, {"height": 1025}):
        with pytest.raises(ValueError):
            insert.prefilter_environment(pano, **{"height": 4, **kw})
    for bad in (torch.rand(3, 8, 16), torch.rand(1, 3, 8, 15), torch.rand(1, 4, 8, 16)):
        with pytest.raises(ValueError):
            insert.prefilter_environment(bad)
    with pytest.raises(_lib_error()):
        insert.prefilter_environment(pano.double())
    with pytest.raises(ValueError, match="forward only"):
        insert.prefilter_environment(pano.clone().requires_grad_(True))
    assert len(recorder.calls) == n


def _lib_error():
    from emlight_amd import _lib
    return _lib.EmlightHipError


# eml_gbuffer_shade_f32(pano, H, e_diffuse, Hd, d_stride, e_phong, Hg, g_stride, normal, coverage, kd, ks, km, B, h, w, fov_deg,
#                       view_azimuth_deg, shaded, background, exposure, gamma, composite, stream)
def test_shade_gbuffer_prefilters_only_the_lobes_it_needs(recorder):
    from emlight_amd import insert
    pano = torch.rand(2, 3, 8, 16)
    normal, cov = torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7)
    out = insert.shade_gbuffer(pano, normal, cov, kd=0.5, ks=(0.1, 0.2, 0.3), km=torch.rand(2, 3, 5, 7), fov_deg=50.0,
                               view_azimuth_deg=77.3, phong_exponent=20.0, diffuse_height=4, glossy_height=6)
    assert out.shape == (2, 3, 5, 7)
    assert recorder.calls == [WORK, PREFILTER, WORK, PREFILTER, SHADE]
    pd, pg = recorder.of(PREFILTER)
    assert pd[4:6] == (4, 1) and list(pd[6]) == [-1.0] and pg[4:6] == (6, 1) and list(pg[6]) == [20.0]
    a = recorder.of(SHADE)[0]
    assert a[0].value == pano.data_ptr() and a[1] == 8
    assert (a[2].value, a[3], a[4]) == (pd[7].value, 4, 3 * 4 * 8) and (a[5].value, a[6], a[7]) == (pg[7].value, 6, 3 * 6 * 12)
    assert a[8].value == normal.data_ptr() and a[9].value == cov.data_ptr() and all(p is not None for p in a[10:13])
    assert a[13:18] == (2, 5, 7, 50.0, 77.3) and a[18].value == out.data_ptr()
    assert a[19] is None and a[20] is None and a[22] is None
    # an absent coefficient: no map, no pointer
    recorder.calls.clear(), recorder.args.clear()
    insert.shade_gbuffer(pano, normal, cov, km=1.0)
    assert recorder.calls == [SHADE]
    a = recorder.of(SHADE)[0]
    assert a[2] is None and a[5] is None and a[10] is None and a[11] is None and a[12] is not None and a[16:18] == (60.0, 180.0)
    recorder.calls.clear(), recorder.args.clear()
    insert.shade_gbuffer(pano, normal, cov, ks=1.0)
    assert recorder.calls == [WORK, PREFILTER, SHADE] and recorder.of(PREFILTER)[0][4] == 64 and list(recorder.of(PREFILTER)[0][6]) == [50.0]
    # maps made earlier: slices of one prefilter output are taken as they are, with the batch stride of the whole
    recorder.calls.clear(), recorder.args.clear()
    maps = insert.prefilter_environment(pano, 4, ("diffuse", 50.0))
    recorder.calls.clear(), recorder.args.clear()
    insert.shade_gbuffer(pano, normal, cov, kd=1.0, ks=1.0, maps=(maps[:, 0], maps[:, 1]))
    assert recorder.calls == [SHADE]
    a = recorder.of(SHADE)[0]
    assert (a[2].value, a[3], a[4]) == (maps.data_ptr(), 4, 2 * 3 * 32)
    assert (a[5].value, a[6], a[7]) == (maps.data_ptr() + 4 * 3 * 32, 4, 2 * 3 * 32)


def test_composite_and_insert_object_calls(recorder):
    from emlight_amd import insert
    pano = torch.rand(2, 3, 8, 16)
    normal, cov, bg = torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7), torch.rand(2, 3, 5, 7)
    ex = torch.tensor([0.5, 2.0])
    out = insert.insert_object(pano, normal, cov, bg, ex, kd=0.7, diffuse_height=4, fov_deg=0.0)
    assert out.shape == (2, 3, 5, 7) and recorder.calls == [WORK, PREFILTER, SHADE]
    a = recorder.of(SHADE)[0]
    assert a[18] is None and a[19].value == bg.data_ptr() and a[20].value == ex.data_ptr() and a[21] == 2.4
    assert a[22].value == out.data_ptr() and a[16] == 0.0
    # composite alone: no coefficient, no normal, shaded is the input
    recorder.calls.clear(), recorder.args.clear()
    shaded = torch.rand(2, 3, 5, 7)
    out = insert.composite(shaded, cov, bg, 1.5, gamma=1)
    assert recorder.calls == [SHADE]
    a = recorder.of(SHADE)[0]
    assert all(a[k] is None for k in (0, 2, 5, 8, 10, 11, 12)) and a[9].value == cov.data_ptr()
    assert a[18].value == shaded.data_ptr() and a[19].value == bg.data_ptr() and a[20] is not None and a[21] == 1.0
    assert a[22].value == out.data_ptr()
    n = len(recorder.calls)
    for call in (lambda: insert.composite(shaded, cov, bg, None), lambda: insert.composite(shaded, cov, bg, 1.0, gamma=0),
                 lambda: insert.composite(shaded, cov, bg[:1], 1.0), lambda: insert.composite(shaded, cov, bg, torch.ones(3)),
                 lambda: insert.composite(shaded, cov[:, :, :4], bg, 1.0)):
        with pytest.raises(ValueError):
            call()
    assert len(recorder.calls) == n


def test_python_layer_refuses_bad_arguments(recorder):
    from emlight_amd import insert
    pano = torch.rand(2, 3, 8, 16)
    normal, cov = torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7)
    bad_calls = [
        lambda: insert.shade_gbuffer(pano, normal, cov),                                   # no coefficient
        lambda: insert.shade_gbuffer(pano, normal, cov, kd=(1.0, 2.0)),
        lambda: insert.shade_gbuffer(pano, normal, cov, kd=torch.rand(2, 3, 5, 6)),
        lambda: insert.shade_gbuffer(pano, normal, torch.ones(2, 5, 7), km=1.0),
        lambda: insert.shade_gbuffer(pano, torch.rand(2, 3, 1, 7), torch.ones(2, 1, 1, 7), km=1.0),
        lambda: insert.shade_gbuffer(pano[:1], normal, cov, km=1.0),
        lambda: insert.shade_gbuffer(pano, normal, cov, km=1.0, fov_deg=180.0),
        lambda: insert.shade_gbuffer(pano, normal, cov, km=1.0, fov_deg=-5.0),
        lambda: insert.shade_gbuffer(pano, normal, cov, km=1.0, view_azimuth_deg=math.nan),
        lambda: insert.shade_gbuffer(pano, normal, cov, kd=1.0, maps=(None, torch.rand(2, 3, 4, 8))),
        lambda: insert.shade_gbuffer(pano, normal, cov, kd=1.0, maps=(torch.rand(2, 3, 4, 7), None)),
        lambda: insert.gbuffer_sphere(1, 8, (0, 0), 2.0, device="cpu"),
        lambda: insert.gbuffer_sphere(8, 8, (0, 0), 0.0, device="cpu"),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert SHADE not in recorder.calls, k
    # forward only: every tensor input that requires grad is refused by name
    for name in ("pano", "normal", "coverage", "km"):
        args = {"pano": pano, "normal": normal, "coverage": cov, "km": torch.rand(2, 3, 5, 7)}
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="%s requires grad.*forward only" % name):
            insert.shade_gbuffer(**args)
    with torch.no_grad():                                                                   # nothing to detach silently
        insert.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov, km=1.0)


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib, insert
    with pytest.raises(_lib.EmlightHipError):
        insert.prefilter_environment(torch.rand(1, 3, 4, 8))
    with pytest.raises(_lib.EmlightHipError):
        insert.shade_gbuffer(torch.rand(1, 3, 4, 8), torch.rand(1, 3, 4, 4), torch.ones(1, 1, 4, 4), km=1.0)
    with pytest.raises(_lib.EmlightHipError):
        insert.composite(torch.rand(1, 3, 4, 4), torch.ones(1, 1, 4, 4), torch.rand(1, 3, 4, 4), 1.0)


# ------------------------------------------------------------------------------------------------ oracle properties
@pytest.mark.parametrize("S", [8, 9])
@pytest.mark.parametrize("az", [180.0, 77.3])
def test_oracle_frames_equal_the_sphere_renders(S, az):
    """fov 0 and a sphere that fills the image: section 15's normals and reflections, pixel for pixel."""
    from emlight_amd import insert
    normal, cov = oracle.gbuffer_sphere(S, S, ((S - 1) / 2, (S - 1) / 2), S / 2)
    inside, n_want, R_want = sro.frames(S, az)
    assert np.array_equal(cov[0] != 0, inside)
    valid, n, R = oracle.frames(normal[None], cov[None], 0.0, az)
    assert np.array_equal(valid[0], inside)
    assert np.abs(n[0][inside] - n_want).max() <= 1e-12 and np.abs(R[0][inside] - R_want).max() <= 1e-12
    # the product's sphere is the oracle's, rounded to float32 once
    got_n, got_c = insert.gbuffer_sphere(S, S, ((S - 1) / 2, (S - 1) / 2), S / 2, device="cpu", batch=2)
    assert got_n.shape == (2, 3, S, S) and got_c.shape == (2, 1, S, S) and got_n.dtype == got_c.dtype == torch.float32
    assert np.array_equal(got_c[1].numpy(), cov.astype(np.float32))
    assert np.array_equal(got_n[0].numpy(), normal.astype(np.float32)) and torch.equal(got_n[0], got_n[1])
    # placed elsewhere: a shifted copy
    shifted, cov2 = oracle.gbuffer_sphere(S + 3, S + 5, ((S - 1) / 2 + 4, (S - 1) / 2 + 2), S / 2)
    assert np.array_equal(shifted[:, 2:2 + S, 4:4 + S], normal) and cov2.sum() == cov.sum()


@pytest.mark.parametrize("h,w,fov", [(6, 8, 60.0), (7, 9, 100.0), (2, 2, 60.0), (24, 32, 90.0)])
def test_oracle_rays_reproduce_crop_panorama(h, w, fov):
    """``crop_panorama``'s formulas (restated: scl, the two linspaces with ratio = w / h, the normalisation, azimuth =
    atan2(x, z), elevation = asin(y)): at view azimuth 180 the ray of pixel (i, j) has panorama azimuth pi + azimuth and
    polar angle pi / 2 + elevation -- the centre looks at the centre column, positive sample_y goes to lower rows."""
    ratio = w / h
    scl = np.tan(np.deg2rad(fov) / 2)
    sample_x, sample_y = np.meshgrid(np.linspace(-scl, scl, w), np.linspace(-scl / ratio, scl / ratio, h))
    r = np.sqrt(sample_y * sample_y + sample_x * sample_x + 1)
    sample_x, sample_y = sample_x / r, sample_y / r
    sample_z = np.sqrt(1 - sample_y * sample_y - sample_x * sample_x)
    azimuth, elevation = np.arctan2(sample_x, sample_z), np.arcsin(sample_y)
    ray = oracle.pixel_rays(h, w, fov, 180.0)
    assert np.abs(np.linalg.norm(ray, axis=-1) - 1).max() <= 1e-14
    phi = np.mod(np.arctan2(ray[..., 1], ray[..., 0]), 2 * np.pi)
    theta = np.arctan2(np.hypot(ray[..., 0], ray[..., 1]), ray[..., 2])
    assert np.abs(phi - (np.pi + azimuth)).max() <= 1e-12 and np.abs(theta - (np.pi / 2 + elevation)).max() <= 1e-12
    # another azimuth turns every ray about z; the orthographic camera looks along f
    turned = oracle.pixel_rays(h, w, fov, 77.3)
    phi2 = np.arctan2(turned[..., 1], turned[..., 0])
    assert np.abs(np.mod(phi2 - phi - np.deg2rad(77.3 - 180.0) + np.pi, 2 * np.pi) - np.pi).max() <= 1e-12
    assert np.abs(turned[..., 2] - ray[..., 2]).max() <= 1e-15
    assert np.abs(oracle.pixel_rays(h, w, 0.0, 180.0) - np.array([-1.0, 0.0, 0.0])).max() <= 1.3e-16


@pytest.mark.parametrize("lobe", ["diffuse", 0.0, 1.0, 50.0])
def test_oracle_constant_panorama_gives_the_quadrature_sum(lobe):
    """A constant panorama c: every lobe map is c times the lobe's quadrature sum at that direction, here summed with
    explicit loops over the texel rows and columns instead of the oracle's matrix product."""
    H, Ho, c = 6, 3, np.array([0.25, 1.0, 7.0])
    got = oracle.prefilter(np.broadcast_to(c[None, :, None, None], (1, 3, H, 2 * H)), Ho, (lobe,))
    assert got.shape == (1, 1, 3, Ho, 2 * Ho)
    for hd in range(Ho):
        for wd in range(2 * Ho):
            td, pd = (hd + 0.5) * math.pi / Ho, (wd + 0.5) * 2 * math.pi / (2 * Ho)
            od = (math.sin(td) * math.cos(pd), math.sin(td) * math.sin(pd), math.cos(td))
            q = 0.0
            for ht in range(H):
                for wt in range(2 * H):
                    tt, pt = (ht + 0.5) * math.pi / H, (wt + 0.5) * 2 * math.pi / (2 * H)
                    x = max(0.0, od[0] * math.sin(tt) * math.cos(pt) + od[1] * math.sin(tt) * math.sin(pt) + od[2] * math.cos(tt))
                    k = x / math.pi if lobe == "diffuse" else (1.0 if lobe == 0 else x ** lobe) * (lobe + 1) / (2 * math.pi)
                    q += k * math.sin(tt) * (math.pi / H) * (2 * math.pi / (2 * H))
            assert np.abs(got[0, 0, :, hd, wd] - c * q).max() <= 1e-12 * c.max() * max(q, 1.0)
    # the normalisations integrate to about 1 (a lobe map of a constant is that constant) where a 6 x 12 grid resolves the lobe
    # (m = 0 with 0^0 = 1 weighs the whole sphere, not a hemisphere: 2)
    if lobe != 50.0:
        assert np.abs(got[0, 0, 1] - (2.0 if lobe == 0.0 else 1.0)).max() < 0.05


def test_oracle_lookup_at_texel_centres_and_borders():
    G = 5
    g = np.random.default_rng(3)
    maps = g.random((2, 3, G, 2 * G))
    om, _ = sro.texel_grid(G, 2 * G)
    got = oracle.lookup(maps, np.broadcast_to(om, (2, 2 * G * G, 3)) * 3.0)       # any length
    assert np.abs(got - maps.reshape(2, 3, -1)).max() <= 1e-6                       # fractions are rounded to f32
    # the poles clamp to the first and last row; the seam blends the last column with the first
    top = oracle.lookup(maps, np.array([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]] * 2))
    assert np.abs(top[:, :, 0] - 0.5 * (maps[:, :, 0, -1] + maps[:, :, 0, 0])).max() <= 1e-15
    assert np.abs(top[:, :, 1] - 0.5 * (maps[:, :, -1, -1] + maps[:, :, -1, 0])).max() <= 1e-15
    mid = 0.5 * (maps[:, :, 2, -1] + maps[:, :, 2, 0])                              # theta = pi / 2 is the centre of row 2
    assert np.abs(top[:, :, 2] - mid).max() <= 1e-15


def test_oracle_shade_and_composite_rules():
    g = np.random.default_rng(4)
    pano, ed, eg = g.random((1, 3, 8, 16)), g.random((1, 3, 2, 4)), g.random((1, 3, 4, 8))
    normal = g.standard_normal((1, 3, 3, 4))
    cov = np.ones((1, 1, 3, 4))
    cov[0, 0, 0, 0], normal[0, :, 0, 0] = 0.0, np.nan
    normal[0, :, 1, 1] = 0.0
    kd = g.random((1, 3, 3, 4))
    kd[0, :, 0, 0] = np.nan
    sh, terms = oracle.shade(pano, ed, eg, normal, cov, kd=kd, km=kd, fov_deg=60.0)
    assert len(terms) == 2 and np.all(sh[0, :, 0, 0] == 0) and np.all(sh[0, :, 1, 1] == 0) and np.isfinite(sh).all()
    # the length of the normal is arbitrary; a mirror facing the orthographic camera shows what is behind the camera
    sh2, _ = oracle.shade(pano, ed, eg, normal * 3.0, cov, kd=kd, km=kd, fov_deg=60.0)
    assert np.abs(sh - sh2).max() <= 1e-12
    facing = np.zeros((1, 3, 2, 2))
    facing[:, 2] = 1.0
    one, _ = oracle.shade(pano, None, None, facing, np.ones((1, 1, 2, 2)), km=np.ones((1, 3, 2, 2)), fov_deg=0.0)
    want = oracle.lookup(pano, np.array([[[1.0, 0.0, 0.0]]]))[:, :, 0]                # v = -f = (1, 0, 0) at azimuth 180
    assert np.abs(one - want[:, :, None, None]).max() <= 1e-12
    out = oracle.composite(np.array([[[[4.0, 0.25], [-1.0, 0.5]]] * 3]), np.array([[[[1.0, 1.0], [1.0, 0.25]]]]),
                           np.full((1, 3, 2, 2), 0.8), np.array([0.5]), gamma=2.0)
    assert np.allclose(out[0, 0], [[1.0, math.sqrt(0.125)], [0.0, 0.25 * 0.5 + 0.75 * 0.8]], rtol=0, atol=1e-15)
    assert np.allclose(oracle.composite(np.full((1, 3, 2, 2), 0.5), np.ones((1, 1, 2, 2)), np.zeros((1, 3, 2, 2)),
                                        np.array([0.5]), gamma=1), 0.25, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_is_parsed_and_dispatched(recorder, tmp_path, capsys):
    from emlight_amd import insert
    g = np.random.default_rng(5)
    pano, image = str(tmp_path / "pred.npy"), str(tmp_path / "crop.npy")
    np.save(pano, g.random((1, 3, 8, 16)).astype(np.float32))                       # as GenProjector.test writes it
    np.save(image, g.random((3, 6, 8)).astype(np.float32))
    gb = tmp_path / "gbuffer"
    gb.mkdir()
    np.save(str(gb / "normal.npy"), g.random((3, 6, 8)).astype(np.float32))
    np.save(str(gb / "coverage.npy"), np.ones((6, 8), dtype=np.float32))
    np.save(str(gb / "ks.npy"), g.random((3, 6, 8)).astype(np.float32))
    out = str(tmp_path / "out.npy")
    res = insert.main(["--pano", pano, "--image", image, "--gbuffer", str(gb), "--fov", "50", "--out", out], device="cpu")
    # no --exposure: the project's tonemap gives the alpha; only ks is there: one prefilter (Phong at 64), one shading call
    assert recorder.calls == ["eml_tonemap_work_floats", "eml_tonemap_f32", WORK, PREFILTER, SHADE]
    a = recorder.of(SHADE)[0]
    assert a[10] is None and a[11] is not None and a[12] is None and a[13:17] == (1, 6, 8, 50.0) and a[18] is None
    assert all(a[k] is not None for k in (19, 20, 22)) and a[21] == 2.4
    assert res.shape == (1, 3, 6, 8) and np.load(out).shape == (3, 6, 8)
    # --sphere and --exposure: no tonemap call, kd and ks by default
    recorder.calls.clear(), recorder.args.clear()
    insert.main(["--pano", pano, "--image", image, "--sphere", "4", "3", "2.5", "--exposure", "0.7", "--out", out], device="cpu")
    assert recorder.calls == [WORK, PREFILTER, WORK, PREFILTER, SHADE]
    a = recorder.of(SHADE)[0]
    assert a[10] is not None and a[11] is not None and a[12] is None and a[16] == 60.0
    capsys.readouterr()
    args = insert.build_parser().parse_args(["--pano", "p.npy", "--image", "i.npy", "--sphere", "1", "2", "3"])
    assert args.sphere == [1.0, 2.0, 3.0] and args.gbuffer is None and args.exposure is None and args.fov == 60.0
    for argv in (["--pano", pano, "--image", image],                                           # neither source
                 ["--pano", pano, "--image", image, "--gbuffer", str(gb), "--sphere", "1", "2", "3"],
                 ["--pano", pano, "--image", image, "--sphere", "1", "2"],
                 ["--pano", pano, "--image", str(tmp_path / "crop.exr"), "--sphere", "1", "2", "3"],
                 ["--pano", pano, "--image", image, "--gbuffer", str(tmp_path)],                # no normal.npy
                 ["--pano", pano, "--image", image, "--sphere", "1", "2", "3", "--kd", "0", "--ks", "0"]):
        with pytest.raises(SystemExit):
            insert.main(argv, device="cpu")
    capsys.readouterr()
