"""CPU: the ground-plane shadow (csrc/ground_shadow.hip, ``emlight_amd.insert.ground_shadow``) WITHOUT a GPU.

* The two entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported, with
  matching argument counts; every refusal of the launcher runs against the built library (it returns before anything
  touches a device).
* ``ground_shadow``, ``sphere_occluder`` and the command line reach the entry points with arguments that convert to the bound
  signatures (the call recorder of ``test_insert_abi.py``, restated here): no shadow call without ``--ground``, one with it.
* ``tests/shadow_oracle.py``, the yardstick of the GPU tests, against a closed form, and the GPU tests' scenes against what
  they say they reach (a wrapped seam, a pole, a part of the image off the plane, points inside a sphere, no pixel near a
  flipping test)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import shadow_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK, SHADOW = "eml_ground_shadow_work_floats", "eml_ground_shadow_f32"
NARGS = {WORK: 5, SHADOW: 17}
INSERT = ["eml_env_prefilter_work_floats", "eml_env_prefilter_f32", "eml_env_prefilter_work_floats", "eml_env_prefilter_f32",
          "eml_gbuffer_shade_f32"]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(built_lib):
    from emlight_amd import _lib
    ext = open(os.path.join(ROOT, "include", "emlight_hip_ext.h")).read()
    first = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in NARGS.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == n, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES[WORK][0] is ctypes.c_size_t and _lib.EXT_SIGNATURES[SHADOW][0] is ctypes.c_int
    assert "DESIGN.md section 28" in ext
    assert len(_lib.SIGNATURES) == 131 and _lib.ABI_VERSION == 31
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ground_shadow.hip" in readme and SHADOW in readme and "--ground" in readme


def test_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    base = dict(pano=one, B=1, H=4, W=8, plane=one, stride=0, occ=one, K=1, h=4, w=6, fov=60.0, az=180.0, image=None, ratio=one,
                shadowed=None, work=one)

    def shadow(**kw):
        a = dict(base, **kw)
        return L.eml_ground_shadow_f32(a["pano"], a["B"], a["H"], a["W"], a["plane"], a["stride"], a["occ"], a["K"], a["h"], a["w"],
                                       a["fov"], a["az"], a["image"], a["ratio"], a["shadowed"], a["work"], None)

    def refused(word, **kw):
        assert shadow(**kw) == -1 and word in L.eml_last_error(), (kw, L.eml_last_error())

    for kw in ({"pano": None}, {"plane": None}, {"work": None}):
        refused(b"null pano, plane or work", **kw)
    refused(b"null occluders", occ=None)
    refused(b"null outputs", ratio=None)
    refused(b"go together", image=one)
    refused(b"go together", shadowed=one)
    for kw in ({"W": 9}, {"W": 4}, {"H": 0, "W": 0}, {"H": 1025, "W": 2050}):
        refused(b"W == 2H", **kw)
    for kw in ({"K": 17}, {"K": -1}):
        refused(b"0..16 occluder spheres", **kw)
    for kw in ({"h": 1}, {"w": 1}, {"h": 16385}, {"w": 16385}):
        refused(b"image size", **kw)
    for kw in ({"fov": 0.0}, {"fov": -1.0}, {"fov": 180.0}, {"fov": math.nan}, {"az": math.nan}, {"az": math.inf}):
        refused(b"fov_deg must be in (0, 180)", **kw)
    for kw in ({"stride": 3}, {"stride": -4}):
        refused(b"plane_stride", **kw)
    for kw in ({"B": -1}, {"B": 65536}):
        refused(b"grid.z", **kw)
    refused(b"8-byte", work=ctypes.c_void_p(20))
    # consistent sets on an empty batch: nothing to launch
    assert shadow(B=0) == 0 and shadow(B=0, K=0, occ=None) == 0 and shadow(B=0, stride=4) == 0
    assert shadow(B=0, image=one, shadowed=one) == 0 and shadow(B=0, image=one, shadowed=one, ratio=None) == 0
    # the scratch: E0, the 256-texel partials and the per-texel terms in doubles; 0 when refused
    wf = L.eml_ground_shadow_work_floats
    assert wf(0, 4, 4, 6, 1) == 0 and wf(1, 0, 4, 6, 1) == 0 and wf(1, 1025, 4, 6, 1) == 0 and wf(1, 4, 1, 6, 1) == 0
    assert wf(1, 4, 4, 6, 17) == 0
    assert wf(1, 4, 4, 6, 1) == 2 * 3 * (1 + 1 + 32) and wf(1, 4, 4, 6, 0) == wf(1, 4, 4, 6, 16)
    assert wf(3, 128, 240, 320, 16) == 2 * 3 * 3 * (1 + 128 + 32768) and wf(3, 128, 24, 32, 1) == wf(3, 128, 240, 320, 16)


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


# eml_ground_shadow_f32(pano, B, H, W, plane, plane_stride, occluders, K, h, w, fov_deg, view_azimuth_deg, image, ratio, shadowed,
#                       work, stream)
def test_ground_shadow_call(recorder):
    from emlight_amd import insert
    pano, occ = torch.rand(2, 3, 8, 16), torch.rand(2, 3, 4)
    out = insert.ground_shadow(pano, occ, size=(5, 7))
    assert out.shape == (2, 3, 5, 7) and out.dtype == torch.float32 and recorder.calls == [WORK, SHADOW]
    assert recorder.of(WORK)[0] == (2, 8, 5, 7, 3)
    a = recorder.of(SHADOW)[0]
    assert a[0].value == pano.data_ptr() and a[1:4] == (2, 8, 16) and a[5] == 0 and a[6].value == occ.data_ptr()
    assert a[7:12] == (3, 5, 7, 60.0, 180.0) and a[12] is None and a[13].value == out.data_ptr() and a[14] is None
    assert a[15].value % 8 == 0
    # with the image: both outputs, the size from the image; a plane per image travels with stride 4
    recorder.calls.clear(), recorder.args.clear()
    image, planes = torch.rand(2, 3, 5, 7), torch.tensor([[0.0, 1.0, 0.0, 1.0], [0.1, 1.0, 0.0, 2.0]])
    ratio, shadowed = insert.ground_shadow(pano, occ, planes, fov_deg=50.0, view_azimuth_deg=37.0, image=image)
    a = recorder.of(SHADOW)[0]
    assert a[4].value == planes.data_ptr() and a[5] == 4 and a[10:12] == (50.0, 37.0) and a[12].value == image.data_ptr()
    assert a[13].value == ratio.data_ptr() and a[14].value == shadowed.data_ptr() and shadowed.shape == (2, 3, 5, 7)
    # no sphere: no pointer; an empty batch: no call
    recorder.calls.clear(), recorder.args.clear()
    insert.ground_shadow(pano, torch.rand(2, 0, 4), (0.0, 2.0, 0.0, 3.0), size=(5, 7))
    a = recorder.of(SHADOW)[0]
    assert a[6] is None and a[7] == 0
    n = len(recorder.calls)
    assert insert.ground_shadow(torch.rand(0, 3, 8, 16), torch.rand(0, 1, 4), size=(5, 7)).shape == (0, 3, 5, 7)
    assert len(recorder.calls) == n


def test_python_layer_refusals(recorder):
    from emlight_amd import insert
    pano, occ, image = torch.rand(2, 3, 8, 16), torch.rand(2, 1, 4), torch.rand(2, 3, 5, 7)
    bad_calls = [
        lambda: insert.ground_shadow(pano, occ, size=(5, 7), fov_deg=0.0),                  # orthographic
        lambda: insert.ground_shadow(pano, occ, size=(5, 7), fov_deg=180.0),
        lambda: insert.ground_shadow(pano, occ, size=(5, 7), view_azimuth_deg=math.inf),
        lambda: insert.ground_shadow(pano, torch.rand(2, 17, 4), size=(5, 7)),              # K = 17
        lambda: insert.ground_shadow(pano, torch.rand(1, 1, 4), size=(5, 7)),
        lambda: insert.ground_shadow(pano, torch.rand(2, 1, 3), size=(5, 7)),
        lambda: insert.ground_shadow(pano, occ, (0.0, 1.0, 0.0, 0.0), size=(5, 7)),         # d <= 0
        lambda: insert.ground_shadow(pano, occ, (0.0, 1.0, 0.0, -1.0), size=(5, 7)),
        lambda: insert.ground_shadow(pano, occ, (0.0, 0.0, 0.0, 1.0), size=(5, 7)),         # a zero normal
        lambda: insert.ground_shadow(pano, occ, (0.0, 1.0, 0.0), size=(5, 7)),
        lambda: insert.ground_shadow(pano, occ, (0.0, math.nan, 0.0, 1.0), size=(5, 7)),
        lambda: insert.ground_shadow(pano, occ, torch.rand(3, 4), size=(5, 7)),
        lambda: insert.ground_shadow(pano, occ),                                            # neither size nor image
        lambda: insert.ground_shadow(pano, occ, size=(1, 7)),
        lambda: insert.ground_shadow(pano, occ, size=(5, 8), image=image),
        lambda: insert.ground_shadow(pano, occ, image=image[:1]),
        lambda: insert.ground_shadow(torch.rand(2, 3, 8, 15), occ, size=(5, 7)),
        lambda: insert.sphere_occluder(1, 8, (0, 0), 2.0, 3.0, 60.0, device="cpu"),
        lambda: insert.sphere_occluder(8, 8, (0, 0), 0.0, 3.0, 60.0, device="cpu"),
        lambda: insert.sphere_occluder(8, 8, (0, 0), 2.0, 0.0, 60.0, device="cpu"),
        lambda: insert.sphere_occluder(8, 8, (0, 0), 2.0, 3.0, 0.0, device="cpu"),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert recorder.calls == [], k
    for name in ("pano", "occluders", "plane", "image"):
        args = {"pano": pano, "occluders": occ, "plane": torch.tensor([[0.0, 1.0, 0.0, 1.0]] * 2), "image": image}
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="%s requires grad.*forward only" % name):
            insert.ground_shadow(**args)
    with pytest.raises(_lib_error()):
        insert.ground_shadow(pano.double(), occ, size=(5, 7))
    assert recorder.calls == []


def _lib_error():
    from emlight_amd import _lib
    return _lib.EmlightHipError


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib, insert
    with pytest.raises(_lib.EmlightHipError):
        insert.ground_shadow(torch.rand(1, 3, 4, 8), torch.rand(1, 1, 4), size=(4, 4))


def test_sphere_occluder_is_the_partner_of_gbuffer_sphere():
    from emlight_amd import insert
    h, w, fov = 12, 16, 70.0
    got = insert.sphere_occluder(h, w, (9.0, 6.5), 4.0, 3.0, fov, device="cpu")
    assert got.shape == (1, 1, 4) and got.dtype == torch.float32
    want = oracle.sphere_occluder(h, w, (9.0, 6.5), 4.0, 3.0, fov)
    assert np.allclose(got.numpy()[0, 0], want, rtol=2e-7, atol=0)
    # the centre is `depth` away along the centre pixel's ray (the camera's rays, turned into camera space) ...
    from tests import insert_oracle as io
    centre = want[:3]
    assert abs(np.linalg.norm(centre) - 3.0) <= 1e-12 and centre[2] < 0
    _, r, u, v = io.basis(180.0)
    rays = io.pixel_rays(h, w, fov, 180.0)
    lo, hi = rays[6, 9], rays[7, 9]                                                       # row 6.5 lies between rows 6 and 7
    mid = (lo + hi) / np.linalg.norm(lo + hi)
    cam = np.array([mid @ r, mid @ u, mid @ v])
    assert np.abs(centre / 3.0 - cam).max() <= 2e-3
    # ... and the radius is what `radius` pixels span at that distance
    assert abs(want[3] - 4.0 * 2.0 * math.tan(math.radians(fov) / 2.0) / (w - 1) * 3.0) <= 1e-12


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_calls_the_shadow_once_with_ground(recorder, tmp_path, capsys):
    from emlight_amd import insert
    g = np.random.default_rng(5)
    pano, image = str(tmp_path / "pred.npy"), str(tmp_path / "crop.npy")
    np.save(pano, g.random((1, 3, 8, 16)).astype(np.float32))
    np.save(image, g.random((3, 6, 8)).astype(np.float32))
    out = str(tmp_path / "out.npy")
    sphere = ["--pano", pano, "--image", image, "--sphere", "4", "3", "2.5", "--exposure", "0.7", "--out", out]
    insert.main(sphere, device="cpu")
    assert recorder.calls == INSERT                                                       # --ground absent: no shadow call
    recorder.calls.clear(), recorder.args.clear()
    insert.main(sphere + ["--ground", "1.5", "--depth", "3"], device="cpu")
    assert recorder.calls == [WORK, SHADOW] + INSERT                                      # present: one, before the tonemap
    a = recorder.of(SHADOW)[0]
    assert a[1:4] == (1, 8, 16) and a[5] == 0 and a[7:12] == (1, 6, 8, 60.0, 180.0) and all(a[k] is not None for k in (12, 13, 14))
    assert np.load(out).shape == (3, 6, 8)
    # a G-buffer carries no geometry: the spheres come from a file
    gb = tmp_path / "gbuffer"
    gb.mkdir()
    np.save(str(gb / "normal.npy"), g.random((3, 6, 8)).astype(np.float32))
    np.save(str(gb / "coverage.npy"), np.ones((6, 8), dtype=np.float32))
    np.save(str(gb / "kd.npy"), g.random((3, 6, 8)).astype(np.float32))
    occ = str(tmp_path / "occ.npy")
    np.save(occ, np.array([[0.0, -0.5, -3.0, 0.5], [0.3, -0.6, -3.2, 0.4]], dtype=np.float32))
    gbuf = ["--pano", pano, "--image", image, "--gbuffer", str(gb), "--exposure", "0.7", "--azimuth", "37", "--out", out]
    recorder.calls.clear(), recorder.args.clear()
    insert.main(gbuf + ["--ground", "1", "--ground_normal", "0", "2", "0", "--occluders", occ], device="cpu")
    assert recorder.calls == [WORK, SHADOW] + INSERT[2:]
    a = recorder.of(SHADOW)[0]
    assert a[7] == 2 and a[11] == 37.0
    recorder.calls.clear(), recorder.args.clear()
    np.save(str(tmp_path / "many.npy"), np.zeros((17, 4), dtype=np.float32))
    for argv in (sphere + ["--ground", "1.5"],                                            # --sphere needs --depth
                 sphere + ["--depth", "3"], sphere + ["--occluders", occ],                # both need --ground
                 sphere + ["--ground", "1.5", "--depth", "3", "--occluders", occ],
                 sphere + ["--ground", "0", "--depth", "3"], sphere + ["--ground", "1", "--depth", "-3"],
                 sphere + ["--ground", "1", "--depth", "3", "--ground_normal", "0", "0", "0"],
                 sphere + ["--ground", "1", "--depth", "3", "--fov", "0"],
                 gbuf + ["--ground", "1"], gbuf + ["--ground", "1", "--depth", "3"],
                 gbuf + ["--ground", "1", "--occluders", str(tmp_path / "occ.txt")],
                 gbuf + ["--ground", "1", "--occluders", str(tmp_path / "many.npy")]):
        with pytest.raises(SystemExit):
            insert.main(argv, device="cpu")
        assert SHADOW not in recorder.calls, argv
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_against_the_closed_form():
    """A uniform panorama over a horizontal floor, one sphere of radius r centred a > r straight above the hit point: the
    sphere fills the cap of half angle asin(r / a) about the zenith, whose cosine-weighted share of the hemisphere is
    (r / a)^2.  The quadrature error shrinks as the grid grows (DESIGN.md section 28 records the three values).  A cap about
    the pole cuts whole rows of the grid, so the error is a staircase: it is, to first order, the distance of the cap's edge
    to the nearest row boundary.  r / a = sin(4.3125 pi / 32) puts that edge 0.3125, 0.375 and 0.25 rows from a boundary at
    H = 32, 64, 128 -- 3.1e-2, 1.8e-2 and 6.1e-3 radians, times d sin^2 / d alpha = 0.75 -- so that the three errors shrink;
    a cap whose edge cuts the same rows at two heights (r / a = 0.4 does at 32 and 64) repeats its error exactly."""
    h = w = 3
    fov, a = 60.0, 2.0
    r = a * math.sin(4.3125 * math.pi / 32.0)
    occ_of = lambda p: np.array([[[p[0], p[1] + a, p[2], r]]])                             # noqa: E731
    from tests import insert_oracle as io
    sy = math.tan(math.radians(fov) / 2.0)                                                 # pixel (2, 1): straight ahead, down
    t = 1.0 / sy
    p = np.array([0.0, -1.0, -t])                                                          # where its ray meets y = -1
    errs = []
    for H in (32, 64, 128):
        res = oracle.evaluate(np.ones((1, 3, H, 2 * H)), (0.0, 1.0, 0.0, 1.0), occ_of(p), h, w, fov, 180.0)
        assert res["hit"][0, 2, 1] and not res["hit"][0, 1, 1] and not res["hit"][0, 0].any()
        assert abs(res["E0"][0, 0] - math.pi) < 1e-2                                       # the irradiance of a unit sky
        errs.append(abs((1.0 - res["ratio"][0, 0, 2, 1]) - (r / a) ** 2))
        assert np.all(res["ratio"][0, :, :2] == 1.0)
    print("closed form (r / a)^2 = %.4f: |error| at H = 32, 64, 128: %.3e %.3e %.3e" % ((r / a) ** 2, *errs))
    assert errs[0] > errs[1] > errs[2]
    # the hit point itself: the camera's ray in camera space is (0, -sy, -1) / norm
    ray = io.pixel_rays(h, w, fov, 180.0)[2, 1]
    _, rr, uu, vv = io.basis(180.0)
    assert np.abs(np.array([ray @ rr, ray @ uu, ray @ vv]) * math.hypot(1.0, sy) - np.array([0.0, -sy, -1.0])).max() <= 1e-15


def test_oracle_rules():
    g = np.random.default_rng(7)
    pano = g.random((1, 3, 8, 16))
    pano[0, 1] = 0.0
    occ = np.array([[[0.0, -0.6, -3.0, 0.4], [9.0, 9.0, 9.0, 0.0]]])
    ratio, E0, margin = oracle.ground_shadow(pano, (0.0, 1.0, 0.0, 1.0), occ, 6, 8)
    assert E0[0, 1] == 0.0 and np.all(ratio[0, 1] == 1.0) and ratio[0, 0].min() < 1.0 and np.all(ratio[0, :, :3] == 1.0)
    assert np.isinf(margin[0, :3]).all() and np.isfinite(margin[0, 3:]).all() and margin.min() > 0.0
    # the padded sphere, the order of the spheres and a sphere hidden in another change nothing
    real = occ[:, :1]
    assert np.array_equal(oracle.ground_shadow(pano, (0.0, 1.0, 0.0, 1.0), real, 6, 8)[0], ratio)
    inner = real.copy()
    inner[..., 3] = 0.2
    assert np.array_equal(oracle.ground_shadow(pano, (0.0, 1.0, 0.0, 1.0), np.concatenate([inner, real], 1), 6, 8)[0], ratio)
    # the plane's four numbers are an equation: a common factor changes nothing but rounding
    twice = oracle.ground_shadow(pano, (0.0, 2.0, 0.0, 2.0), occ, 6, 8)[0]
    assert np.abs(twice - ratio).max() <= 1e-12
    # a sphere that swallows the floor in view: 0 wherever the plane is hit
    big = oracle.evaluate(pano, (0.0, 1.0, 0.0, 1.0), np.array([[[0.0, -1.0, -3.0, 50.0]]]), 6, 8)
    assert big["inside"][0, 3:].all() and np.all(big["ratio"][0, 0][big["hit"][0]] == 0.0)


def test_the_gpu_scenes_reach_what_they_say_and_stay_off_the_margin():
    """The GPU tests' scenes, on the CPU: every property their names promise holds in the oracle, and with these seeds no
    plane-hitting pixel is within the margin of a flipping test (the bound there is 2 %)."""
    from tests import test_gpu_ground_shadow as scenes
    for name in sorted(scenes.CASES):
        c = scenes.case(name)
        want, H = c["want"], c["pano"].shape[2]
        hit = want["hit"]
        low = hit & (want["margin"] < oracle.MARGIN)
        assert hit[0].any() and hit[1].any() and low.sum() == 0, name
        graze = np.abs(want["n_ray"])                                                      # no pixel grazes the plane: a level
        assert graze[graze > 0.0].min() > 1e-6, name                                       # camera's middle row is exactly 0, a miss
        blocked = want["blocked"].reshape(2, c["h"] * c["w"], H, 2 * H)
        if name == "below":
            assert np.all(want["ratio"] == 1.0)
            continue
        assert want["ratio"].min() < 0.999 and not np.array_equal(want["ratio"][0], want["ratio"][1]), name
        if name == "seam":                                                                 # both edge columns, not all columns
            rows = blocked[:, :, :, 0] & blocked[:, :, :, -1] & ~blocked.all(3)
            assert rows.any(), name
        if name == "chunks":                                                               # W = 128: two 64-column chunks
            assert blocked.shape[3] == 128
            wrap = blocked[0, :, :, 0] & blocked[0, :, :, -1] & ~blocked[0].all(2)         # the seam, not all columns
            across = blocked[0, :, :, 63] & blocked[0, :, :, 64] & ~blocked[0, :, :, 0]    # the chunk boundary, off the seam
            assert wrap.any() and across.any() and blocked[1, :, 0, :].all(1).any(), name  # and a pole in the second image
        if name == "zenith":                                                               # row 0 in all columns
            assert blocked[:, :, 0, :].all(2).any(), name
        if name == "tilted":
            assert not hit[0].all() and not hit[1].all() and hit[0].sum() != hit[1].sum()
        if name == "inside":
            assert want["inside"][0].any() and want["inside"][1].any() and not want["inside"][0][hit[0]].all()
        if name == "overlap":                                                              # some texel is blocked by two spheres
            each = [oracle.evaluate(c["pano"], c["planes"], c["occ"][:, k:k + 1], c["h"], c["w"], 60.0, c["az"])["blocked"]
                    for k in range(3)]
            assert (each[0] & each[1]).any() or (each[0] & each[2]).any() or (each[1] & each[2]).any()
    assert {scenes.CASES[n][0] for n in scenes.CASES} == {8, 16, 64}
    assert {scenes.CASES[n][1] for n in scenes.CASES} == {(12, 16), (7, 9)}
    assert {scenes.CASES[n][2] for n in scenes.CASES} == {180.0, 37.0}
