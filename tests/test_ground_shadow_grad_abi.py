"""CPU: the adjoint of the ground-plane shadow (csrc/ground_shadow_bwd.hip, ``emlight_amd.insert_grad.ground_shadow``,
``ShadowLoss``) WITHOUT a GPU.

* The two entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported, with
  matching argument counts; the first header keeps its 131 names and ABI 31; every refusal of the launcher runs against the
  built library (it returns before anything touches a device).
* Under the call recorder (restated from ``test_ground_shadow_abi.py``): without grad the forward's call only; with a
  ``pano`` that requires grad one backward call whose arguments convert to the bound signature; ``plane`` and ``occluders``
  that require grad are refused by name; ``ShadowLoss`` makes one forward over ``2B`` and one backward over ``B``.
* ``tests/shadow_grad_oracle.py``, the yardstick of the GPU tests, against central differences of
  ``shadow_oracle.evaluate``'s ratio, and the GPU tests' scenes: no pixel below the margin, no active pixel whose unclamped
  ratio leaves [0, 1] (so the GPU tests leave no pixel out), and "tiles" shadowed in all four blocks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import shadow_grad_oracle as go
from tests import shadow_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWORK, FWD = "eml_ground_shadow_work_floats", "eml_ground_shadow_f32"
WORK, BWD = "eml_ground_shadow_bwd_work_floats", "eml_ground_shadow_bwd_f32"
NARGS = {WORK: 5, BWD: 19}


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
    assert _lib.EXT_SIGNATURES[WORK][0] is ctypes.c_size_t and _lib.EXT_SIGNATURES[BWD][0] is ctypes.c_int
    assert "DESIGN.md section 29" in ext
    assert len(_lib.SIGNATURES) == 131 and _lib.ABI_VERSION == 31
    assert len(re.findall(r"\beml_\w+\(", re.sub(r"/\*.*?\*/", "", first, flags=re.S))) == 131
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ground_shadow_bwd.hip" in readme and "ground_shadow_walk.h" in readme and BWD in readme and WORK in readme


def test_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    base = dict(pano=one, B=1, H=4, W=8, plane=one, stride=0, occ=one, K=1, h=4, w=6, fov=60.0, az=180.0, image=None, g_ratio=one,
                g_shadowed=None, dpano=one, dimage=None, work=one)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.eml_ground_shadow_bwd_f32(a["pano"], a["B"], a["H"], a["W"], a["plane"], a["stride"], a["occ"], a["K"], a["h"],
                                           a["w"], a["fov"], a["az"], a["image"], a["g_ratio"], a["g_shadowed"], a["dpano"],
                                           a["dimage"], a["work"], None)

    def refused(word, **kw):
        assert bwd(**kw) == -1 and word in L.eml_last_error(), (kw, L.eml_last_error())
        assert b"eml_ground_shadow_bwd_f32" in L.eml_last_error()

    # everything the forward refuses, under the same conditions
    for kw in ({"pano": None}, {"plane": None}, {"work": None}):
        refused(b"null pano, plane or work", **kw)
    refused(b"null occluders", occ=None)
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
    # and its own
    refused(b"null gradients", g_ratio=None)
    refused(b"null outputs", dpano=None)
    refused(b"g_shadowed needs image", g_shadowed=one)
    refused(b"dimage needs g_shadowed", dimage=one)
    refused(b"dimage needs g_shadowed", dimage=one, image=one)
    # consistent sets on an empty batch: nothing to launch
    assert bwd(B=0) == 0 and bwd(B=0, K=0, occ=None) == 0 and bwd(B=0, stride=4) == 0
    assert bwd(B=0, image=one, g_shadowed=one, dimage=one) == 0 and bwd(B=0, image=one, g_shadowed=one, g_ratio=None) == 0
    assert bwd(B=0, image=one, g_shadowed=one, dimage=one, dpano=None) == 0
    # the scratch: 0 when refused; the forward's doubles, then A, S, their partials and one 64-bit accumulator per texel value
    wf = L.eml_ground_shadow_bwd_work_floats
    assert wf(0, 4, 4, 6, 1) == 0 and wf(1, 0, 4, 6, 1) == 0 and wf(1, 1025, 4, 6, 1) == 0 and wf(1, 4, 1, 6, 1) == 0
    assert wf(1, 4, 4, 6, 17) == 0 and wf(1, 4, 4, 16385, 1) == 0 and wf(65536, 4, 4, 6, 1) == 0
    assert wf(1, 4, 4, 6, 1) == 2 * 3 * ((1 + 1 + 32) + 2 + 1 + 1 + 32) and wf(1, 4, 4, 6, 0) == wf(1, 4, 4, 6, 16)
    assert wf(3, 128, 240, 320, 16) == 2 * 3 * 3 * ((1 + 128 + 32768) + 2 + 300 + 300 + 32768)
    assert wf(1, 4, 4, 6, 1) >= L.eml_ground_shadow_work_floats(1, 4, 4, 6, 1)


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


# eml_ground_shadow_bwd_f32(pano, B, H, W, plane, plane_stride, occluders, K, h, w, fov_deg, view_azimuth_deg, image, g_ratio,
#                           g_shadowed, dpano, dimage, work, stream)
def test_without_grad_only_the_forward_is_called(recorder):
    from emlight_amd import insert_grad
    pano, occ, image = torch.rand(2, 3, 8, 16), torch.rand(2, 3, 4), torch.rand(2, 3, 5, 7)
    out = insert_grad.ground_shadow(pano, occ, size=(5, 7))
    assert out.shape == (2, 3, 5, 7) and not out.requires_grad and recorder.calls == [FWORK, FWD]
    recorder.calls.clear(), recorder.args.clear()
    ratio, shadowed = insert_grad.ground_shadow(pano, occ, fov_deg=50.0, image=image)
    assert recorder.calls == [FWORK, FWD] and not ratio.requires_grad and not shadowed.requires_grad
    # grad mode off: a tensor that requires grad changes nothing
    recorder.calls.clear(), recorder.args.clear()
    with torch.no_grad():
        out = insert_grad.ground_shadow(pano.clone().requires_grad_(True), occ, size=(5, 7))
    assert recorder.calls == [FWORK, FWD] and not out.requires_grad


def test_backward_call(recorder):
    from emlight_amd import insert_grad
    pano, occ = torch.rand(2, 3, 8, 16).requires_grad_(True), torch.rand(2, 3, 4)
    out = insert_grad.ground_shadow(pano, occ, fov_deg=50.0, view_azimuth_deg=37.0, size=(5, 7))
    assert out.requires_grad and recorder.calls == [FWORK, FWD]
    g = torch.rand(2, 3, 5, 7)
    out.backward(g)
    assert recorder.calls == [FWORK, FWD, WORK, BWD] and pano.grad.shape == pano.shape
    assert recorder.of(WORK)[0] == (2, 8, 5, 7, 3)
    a = recorder.of(BWD)[0]
    assert a[0].value == pano.data_ptr() and a[1:4] == (2, 8, 16) and a[5] == 0 and a[6].value == occ.data_ptr()
    assert a[7:12] == (3, 5, 7, 50.0, 37.0) and a[12] is None and a[13].value == g.data_ptr() and a[14] is None
    assert a[15] is not None and a[16] is None and a[17].value % 8 == 0
    # pano and image: both gradients, both outputs; a plane per image travels with stride 4
    recorder.calls.clear(), recorder.args.clear()
    image, planes = torch.rand(2, 3, 5, 7).requires_grad_(True), torch.tensor([[0.0, 1.0, 0.0, 1.0], [0.1, 1.0, 0.0, 2.0]])
    pano.grad = None
    ratio, shadowed = insert_grad.ground_shadow(pano, occ, planes, image=image)
    (ratio.sum() + 2.0 * shadowed.sum()).backward()
    assert recorder.calls == [FWORK, FWD, WORK, BWD]
    a = recorder.of(BWD)[0]
    assert a[4].value == planes.data_ptr() and a[5] == 4 and a[12].value == image.data_ptr()
    assert all(a[k] is not None for k in (13, 14, 15, 16)) and image.grad.shape == image.shape
    # the image alone: dimage without dpano; shadowed unused: its gradient is absent and the image gets none
    recorder.calls.clear(), recorder.args.clear()
    image.grad = None
    ratio, shadowed = insert_grad.ground_shadow(pano.detach(), occ, image=image)
    shadowed.sum().backward()
    a = recorder.of(BWD)[0]
    assert a[13] is None and a[14] is not None and a[15] is None and a[16] is not None
    recorder.calls.clear(), recorder.args.clear()
    pano.grad = None
    ratio, shadowed = insert_grad.ground_shadow(pano, occ, image=image)
    ratio.sum().backward()
    a = recorder.of(BWD)[0]
    assert a[12] is None and a[13] is not None and a[14] is None and a[15] is not None and a[16] is None
    # no sphere: no pointer
    recorder.calls.clear(), recorder.args.clear()
    insert_grad.ground_shadow(pano, torch.rand(2, 0, 4), (0.0, 2.0, 0.0, 3.0), size=(5, 7)).sum().backward()
    a = recorder.of(BWD)[0]
    assert a[6] is None and a[7] == 0


def test_raw_call_and_refusals(recorder):
    from emlight_amd import insert_grad
    pano, occ, image, g = torch.rand(2, 3, 8, 16), torch.rand(2, 1, 4), torch.rand(2, 3, 5, 7), torch.rand(2, 3, 5, 7)
    got = insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g)
    assert set(got) == {"pano"} and got["pano"].shape == (2, 3, 8, 16) and recorder.calls == [WORK, BWD]
    got = insert_grad.ground_shadow_bwd_raw(pano, occ, image=image, g_shadowed=g, want=("image",))
    assert set(got) == {"image"} and got["image"].shape == (2, 3, 5, 7)
    n = len(recorder.calls)
    assert insert_grad.ground_shadow_bwd_raw(torch.rand(0, 3, 8, 16), torch.rand(0, 1, 4), g_ratio=torch.rand(0, 3, 5, 7))[
        "pano"].shape == (0, 3, 8, 16) and len(recorder.calls) == n
    recorder.calls.clear()
    bad_calls = [
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, size=(5, 7)),                              # no gradient
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_shadowed=g),                             # without image
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g, image=image, want=("image",)),  # without g_shadowed
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g, want=()),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g, want=("plane",)),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g, size=(5, 8)),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g[:1]),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, g_ratio=g, fov_deg=0.0),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, occ, (0.0, 1.0, 0.0, 0.0), g_ratio=g),
        lambda: insert_grad.ground_shadow_bwd_raw(pano, torch.rand(2, 17, 4), g_ratio=g),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert recorder.calls == [], k


def test_plane_and_occluders_are_refused_by_name(recorder):
    from emlight_amd import insert_grad
    pano, occ, image = torch.rand(2, 3, 8, 16).requires_grad_(True), torch.rand(2, 1, 4), torch.rand(2, 3, 5, 7)
    planes = torch.tensor([[0.0, 1.0, 0.0, 1.0]] * 2)
    for name in ("plane", "occluders"):
        args = {"pano": pano, "occluders": occ, "plane": planes, "image": image}
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="%s requires grad: no gradient is defined for %s" % (name, name)):
            insert_grad.ground_shadow(**args)
        with pytest.raises(ValueError, match="%s requires grad: no gradient is defined for %s" % (name, name)):
            insert_grad.ShadowLoss(args["occluders"], args["plane"], size=(5, 7))
    # the forward's own refusals still hold on the differentiable path, before anything is called
    for call in (lambda: insert_grad.ground_shadow(pano, occ, size=(5, 7), fov_deg=0.0),
                 lambda: insert_grad.ground_shadow(pano, occ), lambda: insert_grad.ground_shadow(pano, occ[:1], size=(5, 7)),
                 lambda: insert_grad.ground_shadow(pano, occ, (0.0, 0.0, 0.0, 1.0), size=(5, 7))):
        with pytest.raises(ValueError):
            call()
    assert recorder.calls == []
    # emlight_amd.insert stays forward only
    from emlight_amd import insert
    with pytest.raises(ValueError, match="pano requires grad.*forward only"):
        insert.ground_shadow(pano, occ, size=(5, 7))


def test_shadow_loss_makes_one_forward_over_2b_and_one_backward_over_b(recorder):
    from emlight_amd import insert_grad
    occ = torch.rand(2, 3, 4)
    loss = insert_grad.ShadowLoss(occ, size=(5, 7), fov_deg=50.0, weight=torch.rand(2, 1, 5, 7))
    pred, true = torch.rand(2, 3, 8, 16).requires_grad_(True), torch.rand(2, 3, 8, 16)
    recorder.calls.clear(), recorder.args.clear()
    value = loss(pred, true)
    assert value.dim() == 0 and value.requires_grad and recorder.calls == [FWORK, FWD]
    a = recorder.of(FWD)[0]
    assert a[1:4] == (4, 8, 16) and a[7:11] == (3, 5, 7, 50.0) and a[12] is None and a[14] is None
    value.backward()
    assert recorder.calls == [FWORK, FWD, WORK, BWD] and pred.grad.shape == pred.shape
    a = recorder.of(BWD)[0]
    assert a[0].value == pred.data_ptr() and a[1:4] == (2, 8, 16) and a[6].value == loss.occluders.data_ptr() and a[7] == 3
    assert a[12] is None and a[13] is not None and a[14] is None and a[15] is not None and a[16] is None
    # no grad: the forward alone; a truth that requires grad gets none
    recorder.calls.clear(), recorder.args.clear()
    assert not loss(pred.detach(), true).requires_grad and recorder.calls == [FWORK, FWD]
    true_g = true.clone().requires_grad_(True)
    loss(pred, true_g).backward()
    assert true_g.grad is None
    # a plane per image is doubled for the forward and single for the adjoint
    planes = torch.tensor([[0.0, 1.0, 0.0, 1.0], [0.1, 1.0, 0.0, 2.0]])
    loss = insert_grad.ShadowLoss(occ, planes, size=(5, 7))
    recorder.calls.clear(), recorder.args.clear()
    loss(pred, true).backward()
    assert recorder.of(FWD)[0][4].value == loss.plane2.data_ptr() and recorder.of(FWD)[0][5] == 4
    assert recorder.of(BWD)[0][4].value == loss.plane.data_ptr() and recorder.of(BWD)[0][5] == 4
    for call in (lambda: insert_grad.ShadowLoss(occ, size=(1, 7)), lambda: insert_grad.ShadowLoss(occ, size=(5, 7), fov_deg=math.nan),
                 lambda: insert_grad.ShadowLoss(torch.rand(2, 17, 4), size=(5, 7)),
                 lambda: insert_grad.ShadowLoss(occ, (0.0, 1.0, 0.0, 0.0), size=(5, 7)),
                 lambda: insert_grad.ShadowLoss(occ, size=(5, 7), weight=torch.rand(2, 3, 5, 7)),
                 lambda: loss(pred[:1], true[:1]), lambda: loss(pred, true[:, :, :4, :8])):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ the oracle
def test_gradient_oracle_against_central_differences():
    """F(pano) = sum g_ratio ratio + sum g_shadowed image ratio is linear-fractional in every texel, so a central difference
    is exact up to its third-order term (step^2, some 1e-10 relative here) and rounding.  Every texel of image 0."""
    H, h, w = 4, 5, 6
    r = np.random.default_rng(29)
    pano = r.random((2, 3, H, 2 * H)) ** 2 * 5.0 + 0.05
    planes = np.array([go.FLOOR, (0.1, 1.0, -0.05, 1.3)])
    occ = np.array([[(0.2, -0.6, -3.0, 0.6)], [(-0.3, -0.7, -2.8, 0.5)]])
    g_ratio, g_shadowed = r.standard_normal((2, 3, h, w)), r.standard_normal((2, 3, h, w))
    image = r.random((2, 3, h, w)) + 0.1
    want = go.gradients(pano, planes, occ, h, w, 60.0, 180.0, g_ratio=g_ratio, g_shadowed=g_shadowed, image=image)
    assert want["forward"]["margin"].min() >= oracle.MARGIN and want["active"][0].any() and (want["v"][0] < 0.99).any()
    assert want["v"].min() >= 0.0 and want["v"].max() <= 1.0                              # the clamp binds nowhere
    assert np.array_equal(want["dimage"], g_shadowed * want["forward"]["ratio"])

    def F(x):
        ratio = oracle.evaluate(x, planes, occ, h, w, 60.0, 180.0)["ratio"]
        return np.sum((g_ratio + g_shadowed * image) * ratio)
    worst = 0.0
    for c in range(3):
        for t in range(2 * H * H):
            i, j = divmod(t, 2 * H)
            step = 1e-4 * pano[0, c, i, j]
            up, dn = pano.copy(), pano.copy()
            up[0, c, i, j] += step
            dn[0, c, i, j] -= step
            fd = (F(up) - F(dn)) / (up[0, c, i, j] - dn[0, c, i, j])
            an = want["dpano"][0, c, i, j]
            if want["wgt"][0, i, j] == 0.0:
                assert fd == 0.0 and an == 0.0
                continue
            worst = max(worst, abs(fd - an) / abs(an))
    print("central differences: largest relative difference %.3e" % worst)
    assert worst <= 1e-6
    # a black channel, a pixel inside a sphere and pixels off the plane contribute exactly nothing
    black = pano.copy()
    black[0, 1] = 0.0
    got = go.gradients(black, planes, occ, h, w, 60.0, 180.0, g_ratio=g_ratio)
    assert np.all(got["dpano"][0, 1] == 0.0) and not got["active"][0, 1].any() and got["dpano"][0, 0].any()
    big = np.array([[(0.0, -1.0, -3.0, 50.0)], [(0.0, -1.0, -3.0, 50.0)]])
    assert np.all(go.gradients(pano, planes, big, h, w, 60.0, 180.0, g_ratio=g_ratio)["dpano"] == 0.0)


def test_shadow_loss_oracle_against_central_differences():
    H, h, w = 4, 5, 6
    r = np.random.default_rng(31)
    pred, true = r.random((1, 3, H, 2 * H)) ** 2 * 5.0 + 0.05, r.random((1, 3, H, 2 * H)) ** 2 * 5.0 + 0.05
    occ = np.array([[(0.2, -0.6, -3.0, 0.6)]])
    wt = r.random((1, 1, h, w))
    loss, dpred = go.shadow_loss(pred, true, go.FLOOR, occ, h, w, weight=wt)[:2]
    assert loss > 0.0 and go.shadow_loss(true, true, go.FLOOR, occ, h, w, weight=wt)[0] == 0.0
    scale = np.abs(dpred).max()
    for c, i, j in ((0, 0, 1), (1, 1, 5), (2, 0, 6), (0, 1, 2)):
        step = 1e-4 * pred[0, c, i, j]
        up, dn = pred.copy(), pred.copy()
        up[0, c, i, j] += step
        dn[0, c, i, j] -= step
        fd = (go.shadow_loss(up, true, go.FLOOR, occ, h, w, weight=wt)[0]
              - go.shadow_loss(dn, true, go.FLOOR, occ, h, w, weight=wt)[0]) / (up[0, c, i, j] - dn[0, c, i, j])
        assert abs(fd - dpred[0, c, i, j]) <= 1e-6 * scale, (c, i, j, fd, dpred[0, c, i, j])


def test_the_gpu_scenes_leave_no_pixel_out():
    """Every scene of the GPU tests, on the CPU: no plane-hitting pixel within the margin of a flipping test, no active pixel
    whose unclamped ratio leaves [0, 1]: the cap on left-out pixels is zero.  The eight scenes of the forward are restated
    exactly, and "tiles" has shadowed pixels in all four 16 x 16 blocks of image 0."""
    from tests import test_gpu_ground_shadow as forward_scenes
    assert {k: v for k, v in go.SCENES.items() if k != "tiles"} == forward_scenes.CASES
    assert np.array_equal(go.hdr(2, 16, 51), forward_scenes.hdr(2, 16, 51))
    for name in sorted(go.SCENES):
        c = go.scene(name)
        want = c["want"]
        fwd = want["forward"]
        hit = fwd["hit"]
        assert hit[0].any() and hit[1].any() and (hit & (fwd["margin"] < oracle.MARGIN)).sum() == 0, name
        v = want["v"][want["active"]]
        assert v.min() >= 0.0 and v.max() <= 1.0, name
        print("%s: smallest margin %.2e, unclamped v in [%.4f, %.4f]" % (name, fwd["margin"].min(), v.min(), v.max()))
        assert np.array_equal(np.where(want["active"], want["v"], fwd["ratio"]), fwd["ratio"]), name   # no clamp, one forward
        if name == "below":
            assert np.all(want["dpano"] == 0.0)
        else:
            assert np.abs(want["dpano"]).max() > 0.0, name
    t = go.scene("tiles")
    assert (t["h"], t["w"]) == (20, 24)
    shadowed = t["want"]["forward"]["ratio"][0, 0] < 0.999
    assert all(shadowed[a, b].any() for a in (slice(0, 16), slice(16, 20)) for b in (slice(0, 16), slice(16, 24)))
