"""CPU: the gradients of object insertion (csrc/env_prefilter_bwd.hip, csrc/gbuffer_shade_bwd.hip,
``emlight_amd/insert_grad.py``) WITHOUT a GPU.

* The four entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` and exported.
* Every refusal of the launchers runs against the built library (they return before anything touches a device).
* The calls a forward plus backward make for each request subset, NULL for what is not needed, no backward call when
  nothing requires grad, and the named refusals (the recorder of ``test_insert_abi.py``, restated here).
* ``tests/insert_grad_oracle.py``, the yardstick of the GPU tests, is pinned: its forward is ``insert_oracle``'s, the
  prefilter adjoint satisfies the adjoint identity, its gradients agree with central differences."""
import ctypes
import functools
import itertools
import math
import os
import re
import threading

import numpy as np
import pytest
import torch

from tests import insert_grad_oracle as grad_oracle
from tests import insert_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PWORK, PRE, SWORK, SHADE = ("eml_env_prefilter_bwd_work_floats", "eml_env_prefilter_bwd_f32",
                            "eml_gbuffer_shade_bwd_work_floats", "eml_gbuffer_shade_bwd_f32")
FWORK, FPRE, FSHADE = "eml_env_prefilter_work_floats", "eml_env_prefilter_f32", "eml_gbuffer_shade_f32"
NARGS = {PWORK: 5, PRE: 10, SWORK: 9, SHADE: 31}
# eml_gbuffer_shade_bwd_f32(grad_out 0, pano 1, H 2, e_diffuse 3, Hd 4, d_stride 5, e_phong 6, Hg 7, g_stride 8, normal 9,
#   coverage 10, kd 11, ks 12, km 13, B 14, h 15, w 16, fov 17, az 18, shaded 19, exposure 20, gamma 21, dkd 22, dks 23, dkm 24,
#   d_e_diffuse 25, d_e_phong 26, dpano 27, dshaded 28, work 29, stream 30)
OUT = {"kd": 22, "ks": 23, "km": 24, "e_diffuse": 25, "e_phong": 26, "pano": 27, "shaded": 28}


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
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in NARGS.items():
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == n, name
        assert hasattr(handle, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES[PWORK][0] is ctypes.c_size_t and _lib.EXT_SIGNATURES[SWORK][0] is ctypes.c_size_t
    assert "DESIGN.md section 23" in ext
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("env_prefilter_bwd.hip", "gbuffer_shade_bwd.hip", "emlight_amd/insert_grad.py", PRE, SHADE, "env_lobes.h",
                 "gbuffer_lookup.h"):
        assert word in readme, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 23\. ", design, re.M)


def test_prefilter_bwd_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    diffuse_phong = (ctypes.c_double * 2)(-1.0, 50.0)

    def pre(g=one, B=1, H=4, W=8, Ho=2, nl=2, lobes=diffuse_phong, dpano=one, work=one):
        return L.eml_env_prefilter_bwd_f32(g, B, H, W, Ho, nl, lobes, dpano, work, None)

    for kw in ({"g": None}, {"lobes": None}, {"dpano": None}, {"work": None}):
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
    w = L.eml_env_prefilter_bwd_work_floats
    assert w(0, 4, 8, 2, 2) == 0 and w(1, 4, 9, 2, 2) == 0 and w(1, 4, 8, 0, 2) == 0 and w(1, 4, 8, 2, 9) == 0
    assert w(1, 4, 8, 2, 1) == 4 * 32 + 4 * 8 + 1 * 32 * 3              # 8 directions: one chunk, one split
    assert w(1, 4, 8, 2, 8) == w(1, 4, 8, 2, 1)                         # one pass for any number of lobes
    # the split is a function of (H, Ho) alone: the per-image scratch is the same for every batch and lobe count
    per_image = [(w(B, 4, 8, 64, nl) - 4 * 32 - 4 * 8192) // (32 * 3 * B) for B in (1, 2, 33) for nl in (1, 2, 5)]
    assert len(set(per_image)) == 1 and per_image[0] == 64


def test_shade_bwd_launcher_refusals_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)
    base = dict(g=one, pano=one, H=4, ed=one, Hd=2, ds=24, eg=one, Hg=2, gs=24, normal=one, coverage=one, kd=one, ks=one, km=one,
                B=1, h=4, w=6, fov=60.0, az=180.0, shaded=None, ex=None, gamma=2.4, dkd=one, dks=None, dkm=None, ded=None,
                deg=None, dpano=None, dshaded=None, work=one)
    order = ("g", "pano", "H", "ed", "Hd", "ds", "eg", "Hg", "gs", "normal", "coverage", "kd", "ks", "km", "B", "h", "w", "fov", "az",
             "shaded", "ex", "gamma", "dkd", "dks", "dkm", "ded", "deg", "dpano", "dshaded", "work")

    def shade(**kw):
        a = dict(base, **kw)
        return L.eml_gbuffer_shade_bwd_f32(*[a[k] for k in order], None)

    def refused(word, **kw):
        assert shade(**kw) == -1 and word in L.eml_last_error(), (kw, L.eml_last_error())

    refused(b"null grad_out", g=None)
    refused(b"null normal or coverage", normal=None)
    refused(b"null normal or coverage", coverage=None)
    refused(b"null outputs", dkd=None)
    alone = dict(kd=None, ks=None, km=None, dkd=None)
    refused(b"no coefficient", **alone, dshaded=one, ex=one)                       # the composite alone needs shaded, ...
    refused(b"no coefficient", **alone, dshaded=one, shaded=one)                   # ... exposure ...
    refused(b"no coefficient", **alone, dpano=one, shaded=one, ex=one)             # ... and the dshaded output
    refused(b"only dshaded", **alone, dshaded=one, shaded=one, ex=one, dpano=one)
    refused(b"composite alone", shaded=one)
    refused(b"composite alone", dshaded=one)
    for kw in ({"ed": None}, {"Hd": 0}, {"Hd": 4097}, {"ds": 23}):
        refused(b"kd needs e_diffuse", **kw)
    for kw in ({"eg": None}, {"Hg": 0}, {"gs": 23}):
        refused(b"ks needs e_phong", **kw)
    for kw in ({"pano": None}, {"H": 0}, {"H": 4097}):
        refused(b"km needs pano", **kw)
    # a term whose coefficient is NULL is not evaluated: asking for its gradient is refused
    refused(b"need kd", kd=None)
    refused(b"need kd", kd=None, dkd=None, ded=one)
    refused(b"need ks", ks=None, dks=one)
    refused(b"need ks", ks=None, deg=one)
    refused(b"need km", km=None, dkm=one)
    refused(b"need km", km=None, dpano=one)
    for g in (0.0, -1.0, math.nan, math.inf):
        refused(b"gamma", ex=one, gamma=g)
    for kw in ({"fov": -1.0}, {"fov": 180.0}, {"fov": math.nan}, {"az": math.nan}, {"az": math.inf}):
        refused(b"fov_deg", **kw)
    refused(b"grid.y", B=-1)
    refused(b"grid.y", B=65536)
    for kw in ({"h": 1}, {"w": 1}, {"h": 1 << 15, "w": (1 << 14) + 1}):
        refused(b"image size", **kw)
    refused(b"work is null", ded=one, work=None)
    refused(b"work is null", dpano=one, work=ctypes.c_void_p(20))
    # consistent sets that are fine, on an empty batch: nothing to launch
    assert shade(B=0) == 0 and shade(B=0, gamma=math.nan) == 0                      # gamma is unused without exposure
    assert shade(B=0, dkd=None, ded=one, deg=one, dpano=one, work=None) == 0
    assert shade(B=0, ex=one, dks=one, dkm=one) == 0
    assert shade(B=0, **alone, normal=None, dshaded=one, shaded=one, ex=one, gamma=1.0, work=None) == 0
    # the scratch: int64 accumulators of the wanted maps, the tiles' partial sums and S, in 8-byte words
    w = L.eml_gbuffer_shade_bwd_work_floats
    assert w(0, 4, 2, 2, 4, 6, 1, 1, 1) == 0 and w(1, 4, 2, 2, 1, 6, 1, 1, 1) == 0 and w(1, 0, 2, 2, 4, 6, 1, 0, 0) == 0
    assert w(1, 4, 2, 2, 4, 6, 0, 0, 0) == 0
    assert w(2, 4, 2, 3, 4, 6, 1, 0, 0) == 2 * (2 * 3 * 32 + 2 * 3 * 1 + 2 * 3)
    assert w(2, 4, 2, 3, 4, 6, 1, 1, 1) == 2 * (2 * 3 * (32 + 8 + 18) + 2 * 3 * 1 + 2 * 3)
    assert w(1, 0, 2, 0, 20, 30, 0, 1, 0) == 2 * (3 * 8 + 3 * 3 + 3)                # 600 pixels: three tiles


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

    def clear(self):
        self.calls.clear(), self.args.clear()


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


def _scene():
    return torch.rand(2, 3, 8, 16), torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7)


def test_prefilter_forward_and_backward_calls(recorder):
    from emlight_amd import insert_grad
    pano = torch.rand(3, 3, 8, 16, requires_grad=True)
    out = insert_grad.prefilter_environment(pano, height=4, lobes=("diffuse", 50, 0.0))
    assert out.shape == (3, 3, 3, 4, 8) and out.requires_grad and recorder.calls == [FWORK, FPRE]
    g = torch.rand(3, 3, 3, 4, 8)
    out.backward(g)
    assert recorder.calls == [FWORK, FPRE, PWORK, PRE] and pano.grad.shape == pano.shape
    assert recorder.of(PWORK)[0] == (3, 8, 16, 4, 3)
    a = recorder.of(PRE)[0]
    assert a[0].value == g.data_ptr() and a[1:6] == (3, 8, 16, 4, 3) and list(a[6]) == [-1.0, 50.0, 0.0] and a[7] is not None
    # a slice's backward: autograd places the contiguous gradient
    recorder.clear()
    insert_grad.prefilter_environment(pano, 4, 7.5)[:, 0].sum().backward()
    assert recorder.calls == [FWORK, FPRE, PWORK, PRE] and list(recorder.of(PRE)[0][6]) == [7.5]
    # nothing requires grad, or grad mode is off: the forward's calls and nothing else
    recorder.clear()
    assert not insert_grad.prefilter_environment(pano.detach(), 4).requires_grad
    with torch.no_grad():
        assert not insert_grad.prefilter_environment(pano, 4).requires_grad
    assert recorder.calls == [FWORK, FPRE] * 2
    for kw in ({"lobes": ()}, {"lobes": ("glossy",)}, {"height": 0}, {"height": 2.5}):
        with pytest.raises(ValueError):
            insert_grad.prefilter_environment(pano, **{"height": 4, **kw})
    # the raw entry point
    recorder.clear()
    assert insert_grad.prefilter_environment_bwd_raw(torch.rand(2, 1, 3, 4, 8), 8, 20.0).shape == (2, 3, 8, 16)
    assert recorder.calls == [PWORK, PRE]
    for bad in (lambda: insert_grad.prefilter_environment_bwd_raw(torch.rand(2, 2, 3, 4, 8), 8, 20.0),
                lambda: insert_grad.prefilter_environment_bwd_raw(torch.rand(2, 1, 3, 4, 7), 8, 20.0),
                lambda: insert_grad.prefilter_environment_bwd_raw(torch.rand(2, 1, 3, 4, 8), 0, 20.0)):
        with pytest.raises(ValueError):
            bad()
    assert insert_grad.prefilter_environment_bwd_raw(torch.rand(0, 1, 3, 4, 8), 8, 20.0).shape == (0, 3, 8, 16)
    assert recorder.calls == [PWORK, PRE]


REQUESTS = [s for n in (1, 2, 3, 4) for s in itertools.combinations(("pano", "kd", "ks", "km"), n)]


@pytest.mark.parametrize("request_set", REQUESTS, ids=["+".join(s) for s in REQUESTS])
def test_shade_gbuffer_backward_asks_for_what_is_needed(recorder, request_set):
    """All three terms, the maps made inside: ``pano``'s gradient is the mirror scatter plus the two prefilter adjoints."""
    from emlight_amd import insert_grad
    pano, normal, cov = _scene()
    t = {"pano": pano, "kd": torch.rand(2, 3, 5, 7), "ks": torch.rand(2, 3, 5, 7), "km": torch.rand(2, 3, 5, 7)}
    for nm in request_set:
        t[nm].requires_grad_(True)
    out = insert_grad.shade_gbuffer(t["pano"], normal, cov, t["kd"], t["ks"], t["km"], fov_deg=50.0, view_azimuth_deg=77.3,
                                    phong_exponent=20.0, diffuse_height=4, glossy_height=6)
    assert recorder.calls == [FWORK, FPRE, FWORK, FPRE, FSHADE]
    recorder.clear()
    g = torch.rand(2, 3, 5, 7)
    out.backward(g)
    with_pano = "pano" in request_set
    assert recorder.calls == ([SWORK, SHADE, PWORK, PRE, PWORK, PRE] if with_pano else [SHADE])
    a = recorder.of(SHADE)[0]
    assert a[0].value == g.data_ptr() and a[1].value == pano.data_ptr() and (a[2], a[4], a[7]) == (8, 4, 6)
    assert (a[5], a[8]) == (3 * 4 * 8, 3 * 6 * 12) and a[9].value == normal.data_ptr() and a[10].value == cov.data_ptr()
    assert a[14:19] == (2, 5, 7, 50.0, 77.3) and a[19] is None and a[20] is None and a[28] is None
    wanted = set(request_set) - {"pano"} | ({"pano", "e_diffuse", "e_phong"} if with_pano else set())
    for nm, k in OUT.items():
        assert (a[k] is not None) == (nm in wanted), (nm, request_set)
    assert (a[29] is not None) == with_pano                                     # scratch only for the scatter
    if with_pano:
        assert recorder.of(SWORK)[0] == (2, 8, 4, 6, 5, 7, 1, 1, 1)
        lobes = sorted(list(p[6])[0] for p in recorder.of(PRE))
        assert lobes == [-1.0, 20.0] and all(p[1:6] in ((2, 8, 16, 4, 1), (2, 8, 16, 6, 1)) for p in recorder.of(PRE))
    for nm in ("pano", "kd", "ks", "km"):
        assert (t[nm].grad is not None) == (nm in request_set)


def test_maps_given_as_slices_get_their_own_gradient(recorder):
    from emlight_amd import insert, insert_grad
    pano, normal, cov = _scene()
    maps = insert.prefilter_environment(pano, 4, ("diffuse", 50.0)).requires_grad_(True)
    recorder.clear()
    out = insert_grad.shade_gbuffer(pano, normal, cov, kd=0.5, ks=(0.1, 0.2, 0.3), maps=(maps[:, 0], maps[:, 1]))
    assert recorder.calls == [FSHADE]
    out.sum().backward()
    assert recorder.calls == [FSHADE, SWORK, SHADE] and maps.grad.shape == maps.shape
    a = recorder.of(SHADE)[0]
    assert (a[3].value, a[4], a[5]) == (maps.data_ptr(), 4, 2 * 3 * 32)           # the slices as they are, the batch stride of the whole
    assert (a[6].value, a[7], a[8]) == (maps.data_ptr() + 4 * 3 * 32, 4, 2 * 3 * 32)
    assert [nm for nm, k in OUT.items() if a[k] is not None] == ["e_diffuse", "e_phong"] and a[1] is None and a[13] is None
    assert recorder.of(SWORK)[0][6:] == (0, 1, 1)
    # only the diffuse map requires grad; km absent: pano takes no gradient and is not asked for
    recorder.clear()
    ed = maps.detach()[:, 0].clone().requires_grad_(True)
    insert_grad.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov, kd=1.0, ks=1.0, maps=(ed, maps.detach()[:, 1])).sum().backward()
    a = recorder.of(SHADE)[0]
    assert [nm for nm, k in OUT.items() if a[k] is not None] == ["e_diffuse"] and ed.grad.shape == ed.shape


def test_composite_and_insert_object_calls(recorder):
    from emlight_amd import insert_grad
    pano, normal, cov = _scene()
    bg, ex = torch.rand(2, 3, 5, 7), torch.tensor([0.5, 2.0])
    km = torch.rand(2, 3, 5, 7, requires_grad=True)
    out = insert_grad.insert_object(pano, normal, cov, bg, ex, kd=0.7, km=km, diffuse_height=4, fov_deg=0.0, gamma=2.0)
    assert recorder.calls == [FWORK, FPRE, FSHADE] and recorder.of(FSHADE)[0][18] is None      # the shaded image is never written
    out.sum().backward()
    assert recorder.calls == [FWORK, FPRE, FSHADE, SHADE]
    a = recorder.of(SHADE)[0]
    assert a[20].value == ex.data_ptr() and a[21] == 2.0 and a[17] == 0.0 and a[11] is not None and a[12] is None
    assert [nm for nm, k in OUT.items() if a[k] is not None] == ["km"] and a[29] is None
    # composite alone: no coefficient, no normal, shaded is read and dshaded written
    recorder.clear()
    shaded = torch.rand(2, 3, 5, 7, requires_grad=True)
    insert_grad.composite(shaded, cov, bg, 1.5, gamma=1).sum().backward()
    assert recorder.calls == [FSHADE, SHADE]
    a = recorder.of(SHADE)[0]
    assert all(a[k] is None for k in (1, 3, 6, 9, 11, 12, 13, 22, 23, 24, 25, 26, 27, 29)) and a[10].value == cov.data_ptr()
    assert a[19].value == shaded.data_ptr() and a[20] is not None and a[21] == 1.0 and a[28] is not None
    assert shaded.grad.shape == shaded.shape
    # nothing requires grad, or grad mode is off: exactly insert's calls
    recorder.clear()
    insert_grad.insert_object(pano, normal, cov, bg, ex, kd=0.7, diffuse_height=4)
    insert_grad.composite(shaded.detach(), cov, bg, 1.5)
    insert_grad.shade_gbuffer(pano, normal, cov, km=1.0)
    with torch.no_grad():
        insert_grad.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov, km=km)
    assert recorder.calls == [FWORK, FPRE, FSHADE, FSHADE, FSHADE, FSHADE]


def test_no_gradient_is_defined_for_the_gbuffer_and_the_photograph(recorder):
    from emlight_amd import insert_grad
    pano, normal, cov = _scene()
    bg, ex = torch.rand(2, 3, 5, 7), torch.tensor([0.5, 2.0])
    for name in ("normal", "coverage", "background", "exposure"):
        args = {"pano": pano.clone().requires_grad_(True), "normal": normal, "coverage": cov, "background": bg, "exposure": ex}
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="%s requires grad: no gradient is defined for %s" % (name, name)):
            insert_grad.insert_object(km=1.0, **args)
        if name in ("normal", "coverage"):
            with pytest.raises(ValueError, match="no gradient is defined for %s" % name):
                insert_grad.shade_gbuffer(args["pano"], args["normal"], args["coverage"], km=1.0)
            with pytest.raises(ValueError, match="no gradient is defined for %s" % name):
                insert_grad.InsertionLoss(args["normal"], args["coverage"], km=1.0)
        else:
            with pytest.raises(ValueError, match="no gradient is defined for %s" % name):
                insert_grad.composite(torch.rand(2, 3, 5, 7, requires_grad=True), cov, args["background"], args["exposure"])
    assert recorder.calls == []
    for bad in (lambda: insert_grad.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov),          # no coefficient
                lambda: insert_grad.shade_gbuffer(pano[:1].clone().requires_grad_(True), normal, cov, km=1.0),
                lambda: insert_grad.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov, kd=1.0, maps=(None, None)),
                lambda: insert_grad.shade_gbuffer_bwd_raw(torch.rand(2, 3, 5, 7), pano, (None, None), normal, cov, km=normal,
                                                          want=("normal",))):
        with pytest.raises(ValueError):
            bad()
    assert recorder.calls == []
    # emlight_amd.insert keeps refusing, and points here
    from emlight_amd import insert
    with pytest.raises(ValueError, match="forward only.*insert_grad"):
        insert.shade_gbuffer(pano.clone().requires_grad_(True), normal, cov, km=1.0)


def test_insertion_loss_calls(recorder):
    from emlight_amd import insert_grad
    pano, normal, cov = _scene()
    loss = insert_grad.InsertionLoss(normal, cov, kd=0.8, ks=(0.1, 0.2, 0.3), fov_deg=50.0, phong_exponent=20.0, diffuse_height=4,
                                     glossy_height=6)
    pred, true = pano.clone().requires_grad_(True), torch.rand(2, 3, 8, 16, requires_grad=True)
    value = loss(pred, true)
    assert value.dim() == 0 and recorder.calls == [FWORK, FPRE, FWORK, FPRE, FSHADE]
    assert [a[0] for a in recorder.of(FWORK)] == [4, 4] and recorder.of(FSHADE)[0][13] == 4          # ONE forward over 2B images
    recorder.clear()
    value.backward()
    assert recorder.calls == [SWORK, SHADE, PWORK, PRE, PWORK, PRE]                                   # over pred's images only
    a = recorder.of(SHADE)[0]
    assert a[14] == 2 and a[1] is None and a[13] is None and (a[5], a[8]) == (3 * 4 * 8, 3 * 6 * 12)
    assert [nm for nm, k in OUT.items() if a[k] is not None] == ["e_diffuse", "e_phong"]
    assert [p[1] for p in recorder.of(PRE)] == [2, 2] and pred.grad.shape == pred.shape and true.grad is None
    recorder.clear()
    loss(pred.detach(), true)                                                                         # nothing to differentiate
    assert recorder.calls == [FWORK, FPRE, FWORK, FPRE, FSHADE]
    with pytest.raises(ValueError):
        loss(pred[:1], true[:1])
    with pytest.raises(ValueError):
        insert_grad.InsertionLoss(normal, cov)


# ------------------------------------------------------------------------------------------------ the oracle, pinned
def off_the_main_heap(test):
    """Run a test body on a worker thread.  The oracle tests below go through megabytes of float64 temporaries.  Other
    modules' call-recorder tests look at ``torch.empty`` buffers that nothing writes, and float64 noise read as float32 is a NaN
    once in 256 words.  A thread allocates from its own malloc arena, so what these tests free is not handed to the main
    thread's later allocations."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        failure = []

        def body():
            try:
                test(*args, **kwargs)
            except BaseException as e:                                             # re-raised on the main thread
                failure.append(e)
        worker = threading.Thread(target=body)
        worker.start()
        worker.join()
        if failure:
            raise failure[0]
    return run


def _oracle_scene(seed=7, B=2, h=5, w=6):
    g = np.random.default_rng(seed)
    pano, ed, eg = g.random((B, 3, 8, 16)) + 0.1, g.random((B, 3, 3, 6)) + 0.1, g.random((B, 3, 4, 8)) + 0.1
    normal = g.standard_normal((B, 3, h, w))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.2
    cov = g.random((B, 1, h, w)) * 0.9 + 0.1
    cov[0, 0, 0, 0], normal[0, :, 0, 0] = 0.0, np.nan
    normal[1, :, 1, 1] = 0.0
    coef = [g.random((B, 3, h, w)) * s + 0.05 for s in (0.8, 0.3, 0.1)]
    return pano, ed, eg, normal, cov, coef


@off_the_main_heap
def test_oracle_forward_is_the_numpy_oracle():
    pano, ed, eg, normal, cov, (kd, ks, km) = _oracle_scene()
    for sub in itertools.product((False, True), repeat=3):
        if not any(sub):
            continue
        k = [c if s else None for c, s in zip((kd, ks, km), sub)]
        for fov, az in ((60.0, 180.0), (0.0, 77.3)):
            want, _ = oracle.shade(pano, ed, eg, normal, cov, *k, fov, az)
            got = grad_oracle.shade(pano, ed, eg, normal, cov, *k, fov, az).numpy()
            assert np.abs(got - want).max() <= 1e-12
    sh, _ = oracle.shade(pano, ed, eg, normal, cov, kd, ks, km)
    bg, ex = np.random.default_rng(8).random(sh.shape), np.array([0.4, 3.0])
    sh[0, :, 2, 2], sh[1, :, 2, 3] = -0.5, 0.0                                    # the lower clamp and its boundary
    for gamma in (2.4, 1):
        want = oracle.composite(sh, cov, bg, ex, gamma)
        assert np.abs(grad_oracle.composite(sh, cov, bg, ex, gamma).numpy() - want).max() <= 1e-12
    x = ex[:, None, None, None] * sh
    assert (x > 1).any() and (x < 0).any() and ((x > 0) & (x < 1)).any()


@pytest.mark.parametrize("lobes", [("diffuse",), ("diffuse", 0.0, 50.0), (1.0, 7.5)])
@off_the_main_heap
def test_oracle_prefilter_adjoint_identity(lobes):
    g = np.random.default_rng(9)
    H, Ho = 6, 4
    p, q = g.standard_normal((2, 3, H, 2 * H)), g.standard_normal((2, len(lobes), 3, Ho, 2 * Ho))
    lhs = float((oracle.prefilter(p, Ho, lobes) * q).sum())
    adj = grad_oracle.prefilter_adjoint(q, H, lobes)
    assert adj.shape == p.shape and abs(lhs - float((p * adj).sum())) <= 1e-12 * max(abs(lhs), 1.0)


@off_the_main_heap
def test_oracle_gradients_against_central_differences():
    """Inputs away from tap boundaries (the taps are constants of the differentiation) and from the clamp's ends."""
    pano, ed, eg, normal, cov, (kd, ks, km) = _oracle_scene(seed=11)
    bg = np.random.default_rng(12).random(kd.shape)
    sh0, _ = oracle.shade(pano, ed, eg, normal, cov, kd, ks, km)
    ex = 0.8 / np.median(sh0.reshape(2, -1), 1)
    x0 = ex[:, None, None, None] * sh0
    live = np.broadcast_to(cov != 0, x0.shape) & (x0 != 0)
    # a step of 1e-6 moves e s by about as much; the third derivative of x^(1/2.4) at 0.02 is 1e4: the difference quotient is good to 1e-8
    assert np.abs(x0[live] - 1.0).min() > 1e-4 and x0[live].min() > 0.02 and (x0 > 1).mean() > 0.1
    gout = np.random.default_rng(13).standard_normal(kd.shape)
    dead = ~np.broadcast_to(oracle.frames(normal, cov, 60.0)[0][:, None], kd.shape)

    def value(arrs, gamma):
        p, d, g_, a, b, c = arrs
        sh = grad_oracle.shade(p, d, g_, normal, cov, a, b, c)
        return (grad_oracle.composite(sh, cov, bg, ex, gamma) * torch.from_numpy(gout)).sum()

    for gamma in (2.4, 1):
        leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (pano, ed, eg, kd, ks, km)]
        value(leaves, gamma).backward()
        rng = np.random.default_rng(14)
        for i, (leaf, arr) in enumerate(zip(leaves, (pano, ed, eg, kd, ks, km))):
            grad = leaf.grad.numpy()
            assert np.isfinite(grad).all()
            if i >= 3:
                assert np.all(grad[dead] == 0.0)
            for _ in range(6):
                idx = tuple(rng.integers(s) for s in arr.shape)
                if i >= 3 and dead[idx]:
                    continue
                eps = 1e-6
                hi, lo = [a.copy() for a in (pano, ed, eg, kd, ks, km)], [a.copy() for a in (pano, ed, eg, kd, ks, km)]
                hi[i][idx] += eps
                lo[i][idx] -= eps
                with torch.no_grad():
                    fd = (float(value([torch.from_numpy(a) for a in hi], gamma))
                          - float(value([torch.from_numpy(a) for a in lo], gamma))) / (2 * eps)
                assert abs(fd - grad[idx]) <= 1e-6 * max(1.0, abs(grad[idx])), (gamma, i, idx, fd, grad[idx])
    # the written-out scatter is autograd's map gradient
    leaves = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (pano, ed, eg)]
    (grad_oracle.shade(*leaves, normal, cov, kd, ks, km) * torch.from_numpy(gout)).sum().backward()
    valid, n, R = oracle.frames(normal, cov, 60.0)
    for leaf, k, d in zip(leaves, (km, kd, ks), (R, n, R)):
        want = grad_oracle.scatter(leaf.shape[2], d, np.where(valid[:, None], k * gout, 0.0))
        assert np.abs(leaf.grad.numpy() - want).max() <= 1e-12
