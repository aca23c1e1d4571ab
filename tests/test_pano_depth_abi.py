"""CPU: depth panoramas -- the depth-aware warp (csrc/pano_warp_depth.hip, ``PanoramaHandler.warp_panorama_depth``), the
per-anchor depth (``extract_mesh.anchor_depth``), ``PanoramaDataset(depth_dir=)``, ``PanoramaBatcher(depth_panos=)`` and
``train.py --depth_dir`` WITHOUT a GPU.

* ``tests/pano_depth_oracle.py`` is pinned to an analytic scene: its hit distances converge to the closed-form ray hits at
  second order in the source's resolution, and it is stable against a 2^-50 perturbation of ``g`` (the condition behind the
  bound that ``test_gpu_pano_depth.py`` holds the kernel to).
* The entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported; the first
  header and its 131 names are untouched.
* The launcher's own argument validation runs against the built library (it returns before anything touches a device).
* The Python layers reach the entry points with arguments that convert to the bound signatures: the HIP library is replaced by
  a recorder (the pattern of ``test_pano_warp_abi.py``, restated here)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import pano_depth_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP, WORK, ANCHOR = "eml_pano_warp_depth_f32", "eml_pano_warp_depth_work_floats", "eml_gt_anchor_depth_f64"
VIEWPOINTS = [(0.0, 0.0, 0.8), (0.5, -0.7, -1.0), (-0.6, 0.9, -0.2)]


# ------------------------------------------------------------------------------------------------ oracle vs analytic scene
@pytest.mark.parametrize("c", VIEWPOINTS)
def test_oracle_converges_to_the_closed_form_hits_at_second_order(c):
    """Box room, output (16, 32), theta = phi = 0, defaults 32 / 24: the median relative error of t falls by a factor >= 3 per
    doubling of the source (second order predicts 4; a first-order or mis-indexed lookup gives about 2)."""
    e, _ = oracle.frame(16, 32)
    t_true, _ = oracle.truth(c, e)
    med = []
    for H, W in ((32, 64), (64, 128), (128, 256)):
        _, depth = oracle.source(H, W)
        r = oracle.search_rays(depth, e, c)
        assert r["valid"] and np.isfinite(r["t"]).all()
        med.append(float(np.median(np.abs(r["t"] - t_true) / t_true)))
    print("c = %s: median relative error %.3e, %.3e, %.3e; ratios %.2f, %.2f" % (c, med[0], med[1], med[2], med[0] / med[1],
                                                                                 med[1] / med[2]))
    assert med[0] / med[1] >= 3 and med[1] / med[2] >= 3


def test_oracle_returns_the_source_depth_from_the_source_viewpoint():
    """c = 0: every ray is a source direction; at matching pixels t is the stored depth, to float32 storage."""
    e, _ = oracle.frame(16, 32)
    for H, W in ((32, 64), (64, 128)):
        _, depth = oracle.source(H, W)
        r = oracle.search_rays(depth, e, (0.0, 0.0, 0.0))
        want = depth[::H // 16, ::W // 32].astype(np.float64).reshape(-1)
        rel = float(np.abs(r["t"] - want).max() / want.min())
        print("%dx%d: worst relative difference %.2e" % (H, W, rel))
        assert (np.abs(r["t"] - want) / want).max() <= 1e-6
        # and the positions are the matching pixels themselves
        assert np.abs(r["row"].reshape(16, 32) - np.arange(16)[:, None] * (H // 16)).max() < 1e-9


@pytest.mark.parametrize("c", VIEWPOINTS)
def test_oracle_with_an_occluder(c):
    """The sphere in the room, source (64, 128), output (32, 64), pixels whose true hit point the origin sees: at most 2 % are off
    by more than 5 % (silhouettes and box edges)."""
    e, _ = oracle.frame(32, 64)
    t_true, visible = oracle.truth(c, e, sphere=True)
    _, depth = oracle.source(64, 128, sphere=True)
    r = oracle.search_rays(depth, e, c)
    rel = np.abs(r["t"] - t_true) / t_true
    share = float((rel[visible] > 0.05).mean())
    print("c = %s: %d of %d pixels visible from the origin, %.2f %% of them off by more than 5 %%"
          % (c, int(visible.sum()), visible.size, 100 * share))
    assert visible.sum() > 0.5 * visible.size and share <= 0.02


def test_oracle_conventions():
    """Rows clamp (no blend of the last row with row 0), columns wrap, the 2^-28 px snap, NaN for an invalid sample."""
    depth = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    got = oracle.lookup(depth, np.array([2.5, 3.0, 0.0, 1.5]), np.array([0.0, 4.0, 3.5, 3.0]))
    np.testing.assert_array_equal(got, [9.0, 9.0, 0.5 * 4 + 0.5 * 1, 0.5 * 8 + 0.5 * 12])
    row, col, n, ok = oracle.position(np.array([[0.0, 0.0, -2.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]), 8, 16)
    assert (row[0], col[0], n[0]) == (4.0, 0.0, 2.0) and not ok[1] and np.isnan(row[1]) and row[2] == 8.0
    img = np.stack([depth, 2 * depth, 3 * depth], axis=-1)
    np.testing.assert_array_equal(oracle.sample(img, np.array([2.5, np.nan]), np.array([0.0, 1.0]))[0], [9.0, 18.0, 27.0])
    assert np.isnan(oracle.sample(img, np.array([np.nan]), np.array([1.0]))).all()
    _, room = oracle.source(16, 32)
    bad = room.copy()
    bad[3, 5] = 0.0
    assert not oracle.warp(bad, 4, 8)["valid"] and np.isnan(oracle.warp(bad, 4, 8)["t"]).all()
    assert not oracle.warp(room, 4, 8, move=-2.5)["valid"]           # the viewpoint is behind the wall at z = 2
    assert oracle.warp(room, 4, 8, move=-1.9)["valid"] and not oracle.warp(room, 4, 8, move=math.nan)["valid"]


@pytest.mark.parametrize("sphere", [False, True])
@pytest.mark.parametrize("steps", [8, 32])
def test_oracle_is_stable_against_the_rounding_of_g(sphere, steps):
    """|P| times 1 +- 2^-50 inside g: no pixel's t moves by more than twice the final interval.  This is the condition under
    which another libm (the device's) may differ in the last bits of g and still land within the bound of the GPU test.
    The viewpoints are those of ``test_gpu_pano_depth.py`` (its shapes and per-sample parameters)."""
    worst = 0.0
    for H, W, h, w in oracle.GPU_SHAPES:
        _, depth = oracle.source(H, W, sphere)
        for theta, phi, move in oracle.GPU_PARAMS:
            base = oracle.warp(depth, h, w, theta, phi, move, steps=steps)
            assert base["valid"]
            for s in (1 + 2.0 ** -50, 1 - 2.0 ** -50):
                moved = oracle.warp(depth, h, w, theta, phi, move, steps=steps, scale=s)
                d = float(np.abs(moved["t"] - base["t"]).max() / oracle.tolerance(base, steps))
                worst = max(worst, d)
                assert d <= 1.0, (sphere, steps, (H, W, h, w), (theta, phi, move), d)
    print("sphere %s, steps %d: the largest move is %.3f of the bound" % (sphere, steps, worst))


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
    for name, nargs in ((WARP, 18), (WORK, 3), (ANCHOR, 9)):
        assert name in declared
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == nargs, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES[WORK][0] is ctypes.c_size_t
    # the declarations cite the reference: the frame, and what depth means
    comment = ext[:ext.index("size_t %s(" % WORK)]
    comment = comment[comment.rindex("/*"):]
    assert "GenProjector/util.py:279-343" in comment and "gmloss/utils.py:63-73" in comment
    comment = ext[:ext.index("int %s(" % ANCHOR)]
    assert "gmloss/utils.py:63-73" in comment[comment.rindex("/*"):]
    # the first header, its table and the ABI version are untouched
    assert not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 131
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme and "pano_warp_depth.hip" in readme and "--depth_dir" in readme


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def warp(pano=one, depth=one, B=1, H=4, W=8, h=4, w=8, theta=0.0, phi=0.0, move=0.0, params=None, steps=32, bisections=24,
             out_pano=one, out_depth=one, hit=None, work=one):
        return L.eml_pano_warp_depth_f32(pano, depth, B, H, W, h, w, theta, phi, move, params, steps, bisections, out_pano,
                                         out_depth, hit, work, None)

    for kw in ({"depth": None}, {"work": None}):
        assert warp(**kw) == -1 and b"null" in L.eml_last_error(), kw
    assert warp(out_pano=None, out_depth=None) == -1 and b"no output" in L.eml_last_error()
    assert warp(out_pano=None, out_depth=None, hit=one) == -1           # the hit list alone is no output
    assert warp(pano=None) == -1 and b"without pano" in L.eml_last_error()
    assert warp(B=-1) == -1 and warp(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    for kw in ({"H": 0}, {"W": 0}, {"h": 0}, {"w": -3}, {"H": 1 << 15, "W": (1 << 14) + 1}, {"h": 1 << 15, "w": 1 << 15}):
        assert warp(**kw) == -1 and b"bad size" in L.eml_last_error(), kw
    for kw in ({"theta": math.nan}, {"phi": math.inf}, {"move": -math.inf}, {"move": math.nan}):
        assert warp(**kw) == -1 and b"not finite" in L.eml_last_error(), kw
    for kw in ({"steps": 0}, {"steps": 1025}, {"steps": -1}):
        assert warp(**kw) == -1 and b"steps" in L.eml_last_error(), kw
    for kw in ({"bisections": -1}, {"bisections": 61}):
        assert warp(**kw) == -1 and b"bisections" in L.eml_last_error(), kw
    # B == 0: nothing to launch; depth only and pano=None are fine; per-sample parameters leave the by-value ones unused
    assert warp(B=0) == 0 and warp(B=0, pano=None, out_pano=None) == 0 and warp(B=0, out_depth=None, hit=one) == 0
    assert warp(B=0, params=one, move=math.nan) == 0 and warp(B=0, steps=1, bisections=0) == 0 and warp(B=0, steps=1024, bisections=60) == 0
    assert L.eml_pano_warp_depth_work_floats(3, 16, 32) >= 3 and L.eml_pano_warp_depth_work_floats(0, 16, 32) == 0
    assert L.eml_pano_warp_depth_work_floats(1, 0, 32) == 0 and L.eml_pano_warp_depth_work_floats(-1, 4, 8) == 0

    def anchor(depth=one, ptr=one, pix=one, B=1, H=4, W=8, N=4, out=one):
        return L.eml_gt_anchor_depth_f64(depth, ptr, pix, B, H, W, N, out, None)

    for kw in ({"depth": None}, {"ptr": None}, {"pix": None}, {"out": None}, {"B": -1}, {"B": 65536}, {"H": 0}, {"W": 0}, {"N": 0}):
        assert anchor(**kw) == -1 and b"eml_gt_anchor_depth_f64" in L.eml_last_error(), kw
    assert anchor(B=0) == 0


def test_a_library_without_the_symbols_is_refused(built_lib, monkeypatch):
    from emlight_amd import _lib
    for missing in (WARP, WORK, ANCHOR):
        class Old:
            def __getattr__(self, name):
                if name == missing:
                    raise AttributeError(name)
                return lambda *a: _lib.ABI_VERSION

        monkeypatch.setattr(_lib, "_lib", None)
        monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Old())
        with pytest.raises(_lib.EmlightHipError, match="lacks symbol %s" % missing):
            _lib.lib()


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


class _FakeDeviceTensor(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _dev(values):
    return torch.tensor(values, dtype=torch.float32).as_subclass(_FakeDeviceTensor)


def _cpu_mesh(ln, h=128, w=256):
    """An ``extract_mesh`` whose tables live on the host (its constructor needs the device)."""
    from emlight_amd.RegressionNetwork.representation import extract_mesh as cls
    m = cls.__new__(cls)
    m.h, m.w, m.ln = h, w, ln
    m.csr_pix = torch.arange(h * w, dtype=torch.int32)
    m.csr_ptr = torch.zeros(ln + 1, dtype=torch.int32)
    m.lum = torch.tensor([0.3, 0.59, 0.11], dtype=torch.float64)
    return m


# eml_pano_warp_depth_f32(pano, depth, B, H, W, h, w, theta, phi, move, params, steps, bisections, out_pano, out_depth, hit,
#                         work, stream)
def test_warp_panorama_depth_call(recorder):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    warp = PanoramaHandler.warp_panorama_depth
    pano, depth = torch.rand(3, 8, 16, 3), torch.rand(3, 8, 16) + 1
    out, out_d = warp(pano, depth, (10, 6), theta=25.0, phi=-200, move=0.4)
    assert out.shape == (3, 6, 10, 3) and out_d.shape == (3, 6, 10) and out.dtype == out_d.dtype == torch.float32
    assert recorder.calls == [WORK, WARP] and recorder.of(WORK)[0] == (3, 8, 16)
    a = recorder.of(WARP)[0]
    assert a[0].value == pano.data_ptr() and a[1].value == depth.data_ptr()
    assert a[2:10] == (3, 8, 16, 6, 10, 25.0, -200.0, 0.4) and a[10] is None and a[11:13] == (32, 24)
    assert a[13].value == out.data_ptr() and a[14].value == out_d.data_ptr() and a[15] is None and a[16] is not None
    assert a[17] is None
    # an int is the height of a 2:1 panorama, None keeps the size; a single image comes back single; the hit list on request
    out, out_d, hit = warp(torch.rand(8, 16, 3), torch.rand(8, 16) + 1, 5, steps=8, bisections=0, return_hit=True)
    assert out.shape == (5, 10, 3) and out_d.shape == (5, 10) and hit.shape == (5, 10, 3) and hit.dtype == torch.float64
    b = recorder.of(WARP)[1]
    assert b[2:7] == (1, 8, 16, 5, 10) and b[11:13] == (8, 0) and b[15] is not None
    # hdr_img=None: depth only
    out, out_d = warp(None, depth)
    assert out is None and out_d.shape == (3, 8, 16)
    c = recorder.of(WARP)[2]
    assert c[0] is None and c[13] is None and c[14] is not None and c[2:7] == (3, 8, 16, 8, 16)
    n = len(recorder.calls)
    out, out_d = warp(torch.rand(0, 8, 16, 3), torch.rand(0, 8, 16), (4, 2))
    assert out.shape == (0, 2, 4, 3) and out_d.shape == (0, 2, 4) and len(recorder.calls) == n
    # any tensor parameter: the three travel as one (B, 3) float64 array, the by-value arguments are unused
    made, real = [], torch.stack

    def stack(tensors, dim=0):
        made.append(real(tensors, dim=dim))
        return made[-1]
    torch.stack = stack
    try:
        warp(torch.rand(2, 8, 16, 3), torch.rand(2, 8, 16) + 1, None, theta=5.0, move=_dev([0.25, -0.5]))
    finally:
        torch.stack = real
    d = recorder.of(WARP)[-1]
    assert d[7:10] == (0.0, 0.0, 0.0) and len(made) == 1 and d[10].value == made[0].data_ptr()
    assert made[0].dtype == torch.float64 and made[0].is_contiguous()
    assert torch.equal(made[0], torch.tensor([[5.0, 0.0, 0.25], [5.0, 0.0, -0.5]], dtype=torch.float64))


def test_warp_panorama_depth_refuses_bad_arguments(recorder):
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    warp = PanoramaHandler.warp_panorama_depth
    pano, depth = torch.rand(2, 8, 16, 3), torch.rand(2, 8, 16) + 1
    for kw in ({"theta": math.nan}, {"phi": math.inf}, {"move": -math.inf}):
        with pytest.raises(ValueError, match="finite"):
            warp(pano, depth, **kw)
    for shape in ((0, 4), (4, 0), (1, 2, 3), "8x16", 0, 2.5):
        with pytest.raises(ValueError):
            warp(pano, depth, shape)
    for kw in ({"steps": 0}, {"steps": 1025}, {"bisections": -1}, {"bisections": 61}):
        with pytest.raises(ValueError, match="steps"):
            warp(pano, depth, **kw)
    for bad_pano, bad_depth in ((pano, torch.rand(2, 8, 15)), (pano, torch.rand(8, 16)), (pano[0], depth), (pano, torch.rand(2, 8, 16, 1)),
                                (torch.rand(2, 8, 16, 4), depth), (pano, None)):
        with pytest.raises(ValueError):
            warp(bad_pano, bad_depth)
    with pytest.raises(ValueError, match="one value per sample"):
        warp(pano, depth, move=_dev([0.1, 0.2, 0.3]))
    with pytest.raises(_lib.EmlightHipError):
        warp(pano, depth.double())
    # forward only: the argument that requires grad is named
    for kw, name in (({"hdr_img": pano.clone().requires_grad_()}, "hdr_img"), ({"depth": depth.clone().requires_grad_()}, "depth"),
                     ({"move": _dev([0.1, 0.2]).requires_grad_()}, "move"), ({"theta": _dev([0.1, 0.2]).requires_grad_()}, "theta")):
        args = {"hdr_img": pano, "depth": depth, **kw}
        with pytest.raises(ValueError, match="^%s requires grad" % name):
            warp(**args)
        with torch.no_grad():
            warp(**args)                    # no graph is asked for: fine
    assert recorder.calls == [WORK, WARP] * 4


def test_cpu_tensors_are_refused():
    from emlight_amd import _lib
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    with pytest.raises(_lib.EmlightHipError):
        PanoramaHandler.warp_panorama_depth(torch.rand(1, 4, 8, 3), torch.rand(1, 4, 8))
    with pytest.raises(_lib.EmlightHipError):
        _cpu_mesh(4, 4, 8).anchor_depth(torch.rand(4, 8))


# eml_gt_anchor_depth_f64(depth, csr_ptr, csr_pix, B, H, W, N, out, stream)
def test_anchor_depth_call(recorder):
    mesh = _cpu_mesh(16)
    depth = torch.rand(2, 128, 256)
    out = mesh.anchor_depth(depth)
    assert out.shape == (2, 16) and out.dtype == torch.float64 and recorder.calls == [ANCHOR]
    a = recorder.of(ANCHOR)[0]
    assert a[0].value == depth.data_ptr() and a[1].value == mesh.csr_ptr.data_ptr() and a[2].value == mesh.csr_pix.data_ptr()
    assert a[3:7] == (2, 128, 256, 16) and a[7].value == out.data_ptr() and a[8] is None
    assert mesh.anchor_depth(depth[0]).shape == (16,) and recorder.of(ANCHOR)[1][3] == 1
    assert mesh.anchor_depth(depth[:0]).shape == (0, 16) and len(recorder.calls) == 2
    for bad in (torch.rand(2, 64, 128), torch.rand(2, 128, 256, 1), torch.rand(256), None):
        with pytest.raises(ValueError):
            mesh.anchor_depth(bad)


# ------------------------------------------------------------------------------------------------ batcher
TODAY = ["eml_pano_crop_f32", "eml_tonemap_work_floats", "eml_tonemap_f32", "eml_pano_resize_area_f32", "eml_gt_parametrise_f64"]
WITH_DEPTH = TODAY[:4] + ["eml_pano_resize_area_f32", "eml_gt_parametrise_f64", ANCHOR]
WITH_DEPTH_AND_WARP = TODAY[:4] + ["eml_pano_resize_area_f32", WORK, WARP, "eml_gt_parametrise_f64", ANCHOR]


def _batcher(**kw):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(anchors=16, crop_hw=(24, 32), device="cpu", mesh=_cpu_mesh(16), **kw)


def test_batcher_calls_with_and_without_depth_panoramas(recorder):
    panos, depths = torch.rand(2, 256, 512, 3), torch.rand(2, 256, 512) + 1
    plain = _batcher()(panos, deg=12.0)
    assert recorder.calls == TODAY and "depth" not in plain
    # depth_panos=None, passed or not: today's calls, also with a warp (the unit-sphere one)
    recorder.calls.clear()
    assert list(_batcher()(panos, deg=12.0, depth_panos=None)) == list(plain) and recorder.calls == TODAY
    recorder.calls.clear()
    _batcher()(panos, deg=12.0, warp=(10.0, -20.0, 0.5))
    assert recorder.calls == TODAY[:4] + ["eml_pano_warp_f32"] + TODAY[4:]
    # depth, no warp: a second resize (of the depth) and the per-anchor reduction
    recorder.calls.clear(), recorder.args.clear()
    out = _batcher()(panos, deg=12.0, depth_panos=depths)
    assert recorder.calls == WITH_DEPTH
    assert list(out) == ["crop", "distribution", "intensity", "rgb_ratio", "ambient", "depth", "alpha"]
    assert out["depth"].shape == (2, 16) and out["depth"].dtype == torch.float32
    r_pano, r_depth = recorder.of("eml_pano_resize_area_f32")
    assert r_pano[0].value == panos.data_ptr() and r_depth[1:6] == r_pano[1:6] == (2, 256, 512, 128, 256) and r_depth[6] == 12.0
    assert recorder.of("eml_gt_parametrise_f64")[0][0].value == r_pano[8].value
    assert recorder.of(ANCHOR)[0][3:7] == (2, 128, 256, 16)
    for k in plain:
        assert out[k].shape == plain[k].shape
    # depth and a warp: the depth-aware warp instead of the unit-sphere one
    recorder.calls.clear(), recorder.args.clear()
    out = _batcher()(panos, deg=12.0, warp=(10.0, -20.0, -0.5), depth_panos=depths)
    assert recorder.calls == WITH_DEPTH_AND_WARP
    a = recorder.of(WARP)[0]
    assert a[2:10] == (2, 128, 256, 128, 256, 10.0, -20.0, -0.5) and a[10] is None and a[11:13] == (32, 24) and a[15] is None
    # the warp reads what the resize wrote (the panorama directly, the depth as channel 0 of the resized three-channel view);
    # the targets and the per-anchor depth read what the warp wrote; the crop is made before all of it
    assert a[0].value == recorder.of("eml_pano_resize_area_f32")[0][8].value
    assert recorder.of("eml_gt_parametrise_f64")[0][0].value == a[13].value
    assert recorder.of(ANCHOR)[0][0].value == a[14].value
    assert out["depth"].shape == (2, 16)
    # per-sample warps and a drawn move reach it as (B, 3) parameters
    recorder.calls.clear(), recorder.args.clear()
    _batcher()(panos, deg=12.0, warp=_dev([[0.0, 0.0, 0.1], [5.0, 6.0, -0.2]]), depth_panos=depths)
    assert recorder.calls == WITH_DEPTH_AND_WARP and recorder.of(WARP)[0][10] is not None
    for bad in (depths[:1], depths[:, :128], torch.rand(2, 256, 512, 1), "depth"):
        with pytest.raises(ValueError, match="depth_panos"):
            _batcher()(panos, deg=12.0, depth_panos=bad)


def test_batcher_draws_the_move_for_the_depth_aware_warp(recorder, monkeypatch):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    draws = []

    def rand(self, B):
        draws.append(B)
        return _dev([0.25] * B).double().as_subclass(_FakeDeviceTensor)
    monkeypatch.setattr(PanoramaBatcher, "_rand", rand)
    panos, depths = torch.rand(2, 256, 512, 3), torch.rand(2, 256, 512) + 1
    _batcher(move_range=(-0.8, 0.0))(panos, depth_panos=depths)
    assert draws == [2, 2] and recorder.calls == WITH_DEPTH_AND_WARP and recorder.of(WARP)[0][10] is not None


# ------------------------------------------------------------------------------------------------ dataset
def test_panorama_dataset_with_depth_dir(tmp_path):
    from emlight_amd.RegressionNetwork.data import PanoramaDataset
    root, ddir = tmp_path / "panos", tmp_path / "depth"
    root.mkdir(), ddir.mkdir()
    rng = np.random.default_rng(5)
    for name in ("a", "b", "c"):
        np.save(root / (name + ".npy"), rng.random((8, 16, 3)).astype(np.float32))
    # without depth_dir: today's items
    item = PanoramaDataset(str(root))[0]
    assert sorted(item) == ["name", "pano"] and item["name"] == "a"
    np.save(ddir / "a.npy", rng.random((8, 16)) + 0.5)                    # float64 on disk: converted
    np.save(ddir / "c.npy", rng.random((8, 16)).astype(np.float32) + 0.5)
    with pytest.raises(FileNotFoundError, match=r"b\.npy"):
        PanoramaDataset(str(root), depth_dir=str(ddir))
    np.save(ddir / "b.npy", rng.random((4, 16)).astype(np.float32) + 0.5)
    ds = PanoramaDataset(str(root), depth_dir=str(ddir))
    item = ds[0]
    assert sorted(item) == ["depth_pano", "name", "pano"]
    assert item["depth_pano"].shape == (8, 16) and item["depth_pano"].dtype == torch.float32 and item["pano"].shape == (8, 16, 3)
    with pytest.raises(ValueError, match=r"depth.b\.npy.*shape"):
        ds[1]
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = rng.random((8, 16)).astype(np.float32) + 0.5
        d[3, 7] = bad
        np.save(ddir / "c.npy", d)
        with pytest.raises(ValueError, match=r"depth.c\.npy.*finite and > 0"):
            ds[2]
    # the default collate stacks the depth panoramas like the panoramas
    from torch.utils.data import DataLoader
    np.save(ddir / "b.npy", rng.random((8, 16)).astype(np.float32) + 0.5)
    batch = next(iter(DataLoader(ds, batch_size=2)))
    assert batch["pano"].shape == (2, 8, 16, 3) and batch["depth_pano"].shape == (2, 8, 16)


# ------------------------------------------------------------------------------------------------ command line
def test_depth_dir_flag_combinations(capsys):
    from emlight_amd.RegressionNetwork import train
    args = train.parse_args(["--geometry", "--pano_dir", "X", "--depth_dir", "Y", "--warp_move", "-0.8", "0"])
    assert args.geometry and args.pano_dir == "X" and args.depth_dir == "Y" and args.warp_move == [-0.8, 0.0]
    assert train.parse_args(["--pano_dir", "X", "--depth_dir", "Y"]).geometry is False       # depth without the loss is fine
    assert train.parse_args(["--pano_dir", "X"]).depth_dir is None
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--geometry", "--pano_dir", "X"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "no depth panoramas" in err and "--depth_dir" in err
    for argv in (["--depth_dir", "Y"], ["--synthetic", "--geometry", "--depth_dir", "Y"]):
        with pytest.raises(SystemExit) as e:
            train.parse_args(argv)
        assert e.value.code == 2 and "--pano_dir" in capsys.readouterr().err
    assert "depth" in [a for a in train.build_parser()._actions if a.dest == "warp_move"][0].help


def test_train_main_hands_the_depth_panoramas_to_the_batcher(monkeypatch, tmp_path):
    """``main`` builds ``PanoramaDataset(X, depth_dir=Y)`` and passes ``depth_pano`` to the batcher (everything that needs the
    device is replaced)."""
    from emlight_amd import _runtime
    from emlight_amd.RegressionNetwork import train
    seen = {}

    class Trainer:
        def __init__(self, **kw):
            seen["geometry"] = kw["geometry"]
            self.model = self.optimizer = None

        def step(self, batch):
            seen["batch"] = batch
            raise KeyboardInterrupt                     # one step is all this test looks at

    class Batcher:
        def __call__(self, panos, depth_panos=None):
            seen["panos"], seen["depth_panos"] = panos, depth_panos
            return {"made": True}

    root, ddir = tmp_path / "panos", tmp_path / "depth"
    root.mkdir(), ddir.mkdir()
    for name in ("a", "b"):
        np.save(root / (name + ".npy"), np.ones((8, 16, 3), dtype=np.float32))
        np.save(ddir / (name + ".npy"), np.full((8, 16), 2.0, dtype=np.float32))
    monkeypatch.setattr(_runtime, "entry_point_defaults", lambda: None)
    monkeypatch.setattr(train, "init_distributed", lambda: (1, 0, 1))           # rank 1: no printing, no checkpoints
    monkeypatch.setattr(train, "RegressionTrainer", Trainer)
    monkeypatch.setattr(train, "make_batcher", lambda args, device: Batcher())
    monkeypatch.setattr(train, "DataLoader", lambda ds, **kw: [torch.utils.data.default_collate([ds[0], ds[1]])])
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **kw: self)
    with pytest.raises(KeyboardInterrupt):
        train.main(["--geometry", "--pano_dir", str(root), "--depth_dir", str(ddir), "--batch_size", "2"])
    assert seen["geometry"] is True and seen["batch"] == {"made": True}
    assert seen["panos"].shape == (2, 8, 16, 3) and seen["depth_panos"].shape == (2, 8, 16) and float(seen["depth_panos"][0, 0, 0]) == 2.0
    # without --depth_dir the batcher gets no depth
    with pytest.raises(KeyboardInterrupt):
        train.main(["--pano_dir", str(root), "--batch_size", "2"])
    assert seen["depth_panos"] is None and seen["geometry"] is False
