"""CPU: the gradients of the panorama warp (csrc/pano_warp_bwd.hip, the ``torch.autograd.Function`` behind
``PanoramaHandler.warp_panorama`` / ``GenProjector.data.resize_exr``) WITHOUT a GPU -- the pattern of
``test_pano_warp_abi.py``, restated here.

* Both entry points are declared in ``include/emlight_hip_ext.h``, bound in ``_lib.EXT_SIGNATURES`` with matching argument
  counts and exported; the first header keeps its 131 names and ABI 31.
* The launcher's argument validation runs against the built library: every ``EML_EINVAL`` case returns before anything
  touches a device.
* With a call recorder in place of the library: inputs that do not require grad make exactly the one ``eml_pano_warp_f32``
  call; inputs that do make the same forward call and, in backward, one ``eml_pano_warp_bwd_f32`` call whose arguments
  convert to the bound signature, and save the panorama only when a parameter needs a gradient."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = "eml_pano_warp_f32"
WORK, BWD = "eml_pano_warp_bwd_work_floats", "eml_pano_warp_bwd_f32"
NARGS = {WORK: 7, BWD: 15}


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
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NARGS.items():
        assert name in declared
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == nargs, name
        assert hasattr(exported, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert name not in first and name not in _lib.SIGNATURES
    assert _lib.EXT_SIGNATURES[WORK][0] is ctypes.c_size_t
    # the comment of the declarations cites the reference
    comment = ext[:ext.index("size_t " + WORK)].rsplit("/*", 1)[1]
    assert "GenProjector/util.py:279-343" in comment
    # the first header, its table and the ABI version are untouched
    assert len(_lib.SIGNATURES) == 131 and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    assert "EML_ABI_VERSION" not in code
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme and "pano_warp_bwd.hip" in readme and BWD in readme


def test_a_library_without_the_symbols_is_refused(built_lib, monkeypatch):
    from emlight_amd import _lib
    for missing in (WORK, BWD):
        class Old:
            def __getattr__(self, name, missing=missing):
                if name == missing:
                    raise AttributeError(name)
                return lambda *a: _lib.ABI_VERSION

        monkeypatch.setattr(_lib, "_lib", None)
        monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path, Old=Old: Old())
        with pytest.raises(_lib.EmlightHipError, match="lacks symbol %s" % missing):
            _lib.lib()


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def bwd(g=one, pano=one, B=1, H=4, W=8, h=4, w=8, theta=0.0, phi=0.0, move=0.0, params=None, dpano=one, dparams=one,
            work=one):
        return L.eml_pano_warp_bwd_f32(g, pano, B, H, W, h, w, theta, phi, move, params, dpano, dparams, work, None)

    assert bwd(g=None) == -1 and b"null grad_out" in L.eml_last_error()
    assert bwd(dpano=None, dparams=None) == -1 and b"neither" in L.eml_last_error()
    assert bwd(pano=None) == -1 and b"needs the panorama" in L.eml_last_error()
    assert bwd(pano=None, dpano=None) == -1 and b"needs the panorama" in L.eml_last_error()
    assert bwd(B=-1) == -1 and bwd(B=65536) == -1 and b"grid.y" in L.eml_last_error()
    for kw in ({"H": 0}, {"W": 0}, {"h": 0}, {"w": -3}, {"H": 1 << 15, "W": (1 << 14) + 1}, {"h": 1 << 15, "w": 1 << 15}):
        assert bwd(**kw) == -1 and b"bad size" in L.eml_last_error(), kw
    for kw in ({"theta": math.nan}, {"phi": math.inf}, {"move": -math.inf}, {"move": math.nan}):
        assert bwd(**kw) == -1 and b"not finite" in L.eml_last_error(), kw
        assert bwd(dparams=None, pano=None, **kw) == -1 and b"not finite" in L.eml_last_error(), kw
    assert bwd(work=None) == -1 and bwd(work=ctypes.c_void_p(20)) == -1 and b"work" in L.eml_last_error()
    # an empty batch: nothing to launch, whatever the pointers; per-sample parameters: the by-value ones are unused
    assert bwd(B=0) == 0 and bwd(B=0, work=None) == 0 and bwd(B=0, params=one, move=math.nan) == 0
    # the work size: 8-byte words, so an even number of floats; 0 where nothing would run
    f = L.eml_pano_warp_bwd_work_floats
    assert f(0, 4, 8, 4, 8, 1, 1) == 0 and f(1, 0, 8, 4, 8, 1, 1) == 0 and f(1, 4, 8, 4, 8, 0, 0) == 0
    assert f(70000, 4, 8, 4, 8, 1, 1) == 0 and f(1, 1 << 15, 1 << 15, 4, 8, 1, 1) == 0
    both, only_pano, only_par = f(3, 4, 8, 16, 32, 1, 1), f(3, 4, 8, 16, 32, 1, 0), f(3, 4, 8, 16, 32, 0, 1)
    assert both == only_pano + only_par and both % 2 == 0
    assert only_pano >= 2 * 3 * 3 * 4 * 8                   # one 64-bit accumulator per element of dpano
    assert only_par == 2 * 3 * 3 * 2                        # two 256-pixel tiles, three parameters, per sample


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


def _per_sample(monkeypatch):
    """``(B,)`` host tensors as per-sample parameters: only the device check of ``_per_sample`` goes."""
    from emlight_amd.RegressionNetwork import util

    def per_sample(value, B, name):
        if isinstance(value, torch.Tensor):
            if value.dim() == 0:
                value = value.expand(B)
            if value.shape != (B,):
                raise ValueError("%s: expected one value per sample" % name)
            return 0.0, value.to(torch.float64).contiguous()
        return float(value), None
    monkeypatch.setattr(util, "_per_sample", per_sample)


def test_inputs_that_do_not_require_grad_make_the_one_forward_call(recorder, monkeypatch):
    from emlight_amd.GenProjector.data import resize_exr
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    _per_sample(monkeypatch)
    x = torch.rand(3, 8, 16, 3)
    out = PanoramaHandler.warp_panorama(x, (10, 6), theta=25.0, phi=-200, move=0.4)
    assert recorder.calls == [FWD] and out.grad_fn is None and not out.requires_grad
    out, coords = PanoramaHandler.warp_panorama(x, None, move=torch.tensor([0.1, 0.2, 0.3]), return_coords=True)
    assert recorder.calls == [FWD] * 2 and out.grad_fn is None and coords.grad_fn is None
    assert resize_exr(x[0], 6, 10).grad_fn is None and recorder.calls == [FWD] * 3
    # grad mode off: the plain call although the inputs require grad
    with torch.no_grad():
        out = PanoramaHandler.warp_panorama(x.clone().requires_grad_(True), move=torch.tensor([0.1, 0.2, 0.3], requires_grad=True))
    assert recorder.calls == [FWD] * 4 and out.grad_fn is None
    # the same arguments reach the forward with and without autograd
    recorder.calls.clear(), recorder.args.clear()
    PanoramaHandler.warp_panorama(x, (10, 6), theta=25.0, phi=-200, move=0.4)
    PanoramaHandler.warp_panorama(x.clone().requires_grad_(True), (10, 6), theta=25.0, phi=-200, move=0.4)
    a, b = recorder.of(FWD)
    assert a[1:9] == b[1:9] == (3, 8, 16, 6, 10, 25.0, -200.0, 0.4) and a[9] is None and b[9] is None and recorder.calls == [FWD] * 2


def test_autograd_calls_and_what_is_saved(recorder, monkeypatch):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    _per_sample(monkeypatch)
    # the panorama alone, by value: dpano only, no panorama passed or saved
    x = torch.rand(3, 8, 16, 3, requires_grad=True)
    out = PanoramaHandler.warp_panorama(x, (10, 6), theta=25.0, move=0.4)
    assert out.shape == (3, 6, 10, 3) and out.grad_fn is not None
    out.backward(torch.ones_like(out))
    assert recorder.calls == [FWD, WORK, BWD]
    assert recorder.of(WORK)[0] == (3, 8, 16, 6, 10, 1, 0)
    a = recorder.of(BWD)[0]
    assert a[1] is None and a[2:10] == (3, 8, 16, 6, 10, 25.0, 0.0, 0.4) and a[10] is None
    assert a[11] is not None and a[12] is None and a[13] is not None and a[13].value % 8 == 0
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32
    # a parameter alone: dparams only, the panorama is passed; Python numbers get nothing, the tensor its own dtype
    recorder.calls.clear(), recorder.args.clear()
    x = torch.rand(2, 8, 16, 3)
    move = torch.tensor([0.25, -0.5], dtype=torch.float32, requires_grad=True)
    out, coords = PanoramaHandler.warp_panorama(x, None, theta=5.0, move=move, return_coords=True)
    assert out.grad_fn is not None and not coords.requires_grad and coords.shape == (2, 8, 16, 2)
    out.sum().backward()
    assert recorder.calls == [FWD, WORK, BWD] and recorder.of(WORK)[0] == (2, 8, 16, 8, 16, 0, 1)
    a = recorder.of(BWD)[0]
    assert a[1].value == x.data_ptr() and a[7:10] == (0.0, 0.0, 0.0) and a[10] is not None
    assert a[11] is None and a[12] is not None
    assert move.grad.shape == (2,) and move.grad.dtype == torch.float32
    # everything, a single image: shapes and dtypes of the inputs
    recorder.calls.clear(), recorder.args.clear()
    x = torch.rand(8, 16, 3, requires_grad=True)
    t = torch.tensor([3.0], dtype=torch.float64, requires_grad=True)
    f = torch.tensor([4.0], dtype=torch.float32, requires_grad=True)
    out = PanoramaHandler.warp_panorama(x, 5, theta=t, phi=f, move=0.1)
    assert out.shape == (5, 10, 3)
    out.sum().backward()
    assert recorder.of(WORK)[0] == (1, 8, 16, 5, 10, 1, 1)
    assert x.grad.shape == (8, 16, 3) and t.grad.dtype == torch.float64 and f.grad.dtype == torch.float32
    assert t.grad.shape == f.grad.shape == (1,)
    # the backward is not differentiable a second time
    x = torch.rand(1, 8, 16, 3, requires_grad=True)
    out = PanoramaHandler.warp_panorama(x)
    (gx,) = torch.autograd.grad(out, x, torch.ones_like(out, requires_grad=True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
    # an empty batch: no call at all, empty gradients
    recorder.calls.clear()
    x = torch.rand(0, 8, 16, 3, requires_grad=True)
    PanoramaHandler.warp_panorama(x, (4, 2)).sum().backward()
    assert recorder.calls == [] and x.grad.shape == (0, 8, 16, 3)


def test_the_forward_saves_the_panorama_only_for_a_parameter_gradient(recorder, monkeypatch):
    from emlight_amd.RegressionNetwork import util
    _per_sample(monkeypatch)
    saved = []
    real = util._WarpPanorama.forward

    class Spy:
        def __init__(self, ctx):
            object.__setattr__(self, "ctx", ctx)

        def __getattr__(self, name):
            return getattr(self.ctx, name)

        def __setattr__(self, name, value):
            setattr(self.ctx, name, value)

        def save_for_backward(self, *tensors):
            saved.append(tensors)
            self.ctx.save_for_backward(*tensors)

    monkeypatch.setattr(util._WarpPanorama, "forward", staticmethod(lambda ctx, *a: real(Spy(ctx), *a)))
    x = torch.rand(2, 8, 16, 3, requires_grad=True)
    move = torch.tensor([0.25, -0.5], dtype=torch.float64)
    util.PanoramaHandler.warp_panorama(x, move=0.3)
    util.PanoramaHandler.warp_panorama(x, move=move)
    util.PanoramaHandler.warp_panorama(x, move=move.clone().requires_grad_(True))
    util.PanoramaHandler.warp_panorama(x.detach(), move=move.clone().requires_grad_(True))
    assert [s[0] is None for s in saved] == [True, True, False, False]
    assert [s[1] is None for s in saved] == [True, False, False, False]
