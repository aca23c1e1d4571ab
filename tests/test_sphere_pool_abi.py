"""CPU: SphereMaxPool2D (csrc/sphere_pool.hip, ``spherenet.sphere_max_pool``, ``spherenet.SphereMaxPool2D``) WITHOUT a GPU.

* The two entry points are declared in ``include/emlight_hip_ext.h`` (citing the reference's lines), bound in
  ``_lib.EXT_SIGNATURES`` with matching argument counts and exported; the first header keeps its 131 names and ABI 31.
* The launchers' own argument validation runs against the built library (it returns before anything touches a device).
* The Python layer reaches the entry points with arguments that convert to the bound signatures: the HIP library is replaced
  by a recorder (the pattern of ``test_pano_warp_abi.py``, restated here) whose tap-table call fills in the real table.
* ``tests/sphere_pool_oracle.py`` is pinned to the reference: it reproduces the outputs and gradients that the reference's own
  ``SphereMaxPool2D`` made on the CPU (``tests/golden/sphere_pool.npz``)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from emlight_amd.GenProjector.spherenet import SphereMaxPool2D, sphere_max_pool  # noqa: F401  (absent before this layer existed)
from tests import sphere_pool_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "eml_sphere_max_pool_fwd_f32", "eml_sphere_max_pool_bwd_f32"
NARGS = {FWD: 10, BWD: 11}


# ------------------------------------------------------------------------------------------------ oracle vs reference
def test_oracle_is_pinned_to_the_reference_outputs():
    path = os.path.join(ROOT, "tests", "golden", "sphere_pool.npz")
    assert os.path.getsize(path) < 200 * 1024
    z = np.load(path)
    assert len(z.files) == 6 * len(oracle.CASES)
    for case in oracle.CASES:
        H, W, stride, B, C = case
        name = oracle.case_name(case)
        ho, wo = oracle.out_size(H, W, stride)
        x, y, gy, gx, arg = (torch.from_numpy(z[name + "/" + k]) for k in ("x", "y", "gy", "gx", "arg"))
        assert x.shape == (B, C, H, W) and y.shape == gy.shape == arg.shape == (B, C, ho, wo) and gx.shape == x.shape
        assert x.dtype == y.dtype == gy.dtype == gx.dtype == torch.float32 and arg.dtype == torch.uint8 and int(arg.max()) <= 8
        idx, wgt = oracle.tap_table(H, W, stride)
        vals = oracle.tap_values(x, idx, wgt)
        want, mine = oracle.pool(vals)
        xmax = float(x.abs().max())
        err = float((want - y.double().view(B, C, -1)).abs().max())
        # the reference's tap is a maximal one (pole ties may fall either way)
        a = arg.long().view(B, C, -1)
        chosen = vals.gather(3, a.unsqueeze(-1)).squeeze(-1)
        short = float((want - chosen).max())
        M = oracle.longest_row(idx, H * W)
        g, S = oracle.routed_grad(gy.view(B, C, -1), a, idx, wgt, H * W)
        ratio = float(((g - gx.double().view(B, C, -1)).abs() / oracle.grad_bound(M, S)).max())
        window = oracle.near_tie_cells(vals, xmax)
        print("%-16s forward %.2e (bound %.2e), chosen tap short by %.2e, %d routings differ, M %d, gradient at %.3f of "
              "its bound, %d near ties" % (name, err, oracle.forward_bound(xmax), short, int((mine != a).sum()), M, ratio,
                                           int(window.sum())))
        assert err <= oracle.forward_bound(xmax), name
        assert short <= oracle.forward_bound(xmax), name
        assert ratio <= 1.0, name
        assert float(window.double().mean()) <= oracle.NEAR_TIE_CAP, name
        # where the routings differ the float64 taps tie (the pole rows)
        assert bool((oracle.top_two_gap(vals)[mine != a] <= oracle.NEAR_TIE_LO).all()), name


def test_oracle_conventions():
    """Ceiling output size, taps in the window's row-major order, first maximum, NaN wins, empty CSR rows at stride 3."""
    assert oracle.out_size(5, 12, 2) == (3, 6) and oracle.out_size(10, 20, 3) == (4, 7)
    idx, wgt = oracle.tap_table(8, 16, 1)
    assert idx.shape == wgt.shape == (8 * 16 * 9, 4) and wgt.dtype == torch.float32
    # the centre tap (t = 4) of cell (r, c) is the pixel itself: half-way between four texels in grid_sample's coordinates
    p = 3 * 16 + 5
    assert set(idx[p * 9 + 4].tolist()) == {2 * 16 + 4, 2 * 16 + 5, 3 * 16 + 4, 3 * 16 + 5}
    assert torch.equal(wgt[p * 9 + 4], torch.full((4,), 0.25))
    # tap 3 lies to the west of tap 5, tap 1 to the north of tap 7
    x = torch.arange(16.0).view(1, 1, 1, 16).expand(1, 1, 8, 16).contiguous()
    v = oracle.tap_values(x, idx, wgt)[0, 0, p]
    assert v[3] < v[4] < v[5]
    x = torch.arange(8.0).view(1, 1, 8, 1).expand(1, 1, 8, 16).contiguous()
    v = oracle.tap_values(x, idx, wgt)[0, 0, p]
    assert v[1] < v[4] < v[7]
    vals = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0], [1.0, float("nan"), 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                         [float("nan"), 0.0, 0.0, 0.0, float("nan"), 0.0, 0.0, 9.0, 0.0]], dtype=torch.float64).view(1, 1, 3, 9)
    y, arg = oracle.pool(vals)
    assert arg.view(-1).tolist() == [1, 1, 4] and float(y[0, 0, 0]) == 3.0 and bool(torch.isnan(y[0, 0, 1:]).all())
    # stride 3: some input pixels are sampled by no tap at all (an empty row of the CSR transpose: the last row of a 9-row map),
    # and under any one routing most of the others receive nothing either
    idx, wgt = oracle.tap_table(9, 18, 3)
    _, S = oracle.routed_grad(torch.ones(1, 1, 18), torch.full((1, 1, 18), 4, dtype=torch.int64), idx, wgt, 9 * 18)
    fed = torch.bincount(idx[idx >= 0], minlength=9 * 18) > 0
    assert 0.05 < float((~fed).double().mean()) < 0.5 and bool((S[0, 0][~fed] == 0).all())
    assert float((S == 0).double().mean()) > 0.6


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
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NARGS.items():
        assert name in declared
        decl = re.search(r"\b%s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.EXT_SIGNATURES[name][1]) == nargs, name
        assert hasattr(exported, name), "libemlight_hip.so does not export %s" % name
        assert getattr(built_lib, name).argtypes == _lib.EXT_SIGNATURES[name][1]
        assert _lib.EXT_SIGNATURES[name][0] is ctypes.c_int
        assert name not in first and name not in _lib.SIGNATURES
    # each declaration cites the reference
    assert len(re.findall(r"spherenet/sphere_cnn\.py:127-150", ext)) >= 2
    # the first header, its table and the ABI version are untouched
    assert len(_lib.SIGNATURES) == 131 and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    assert int(re.search(r"#define EML_ABI_VERSION (\d+)", first).group(1)) == _lib.ABI_VERSION == 31
    assert "EML_ABI_VERSION" not in code
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ABI 31, 131 symbols" in readme and "sphere_pool.hip" in readme and FWD in readme and BWD in readme


def test_launcher_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def fwd(x=one, idx=one, wgt=one, y=one, arg=one, B=1, n_src=128, n_dst=32, C=4):
        return L.eml_sphere_max_pool_fwd_f32(x, idx, wgt, y, arg, B, n_src, n_dst, C, None)

    def bwd(gy=one, arg=one, ptr=one, src=one, w=one, gx=one, B=1, n_src=128, n_dst=32, C=4):
        return L.eml_sphere_max_pool_bwd_f32(gy, arg, ptr, src, w, gx, B, n_src, n_dst, C, None)

    for key in ("x", "idx", "wgt", "y"):
        assert fwd(**{key: None}) == -1 and b"eml_sphere_max_pool_fwd_f32: null" in L.eml_last_error(), key
    for key in ("gy", "arg", "ptr", "src", "w", "gx"):
        assert bwd(**{key: None}) == -1 and b"eml_sphere_max_pool_bwd_f32: null" in L.eml_last_error(), key
    for call in (fwd, bwd):
        for kw in ({"C": 0}, {"C": -4}, {"n_dst": 0}, {"n_src": 0}, {"B": -1}):
            assert call(**kw) == -1 and b"bad size" in L.eml_last_error(), kw
        # rows are 32-bit
        for kw in ({"B": 1 << 16, "n_dst": 1 << 15}, {"B": 1 << 16, "n_src": 1 << 15}, {"n_dst": (1 << 31) // 9 + 1}):
            assert call(**kw) == -1 and b"2^31" in L.eml_last_error(), kw
        assert call(B=0) == 0                               # an empty batch: nothing to launch
    assert fwd(B=0, arg=None) == 0                          # the indices are optional ...
    assert bwd(B=0, arg=None) == -1                         # ... for the forward only


# ------------------------------------------------------------------------------------------------ recorder
class _Recorder:
    """Stands in for the library: checks every call against the bound signature.  The tap-table call writes the real table
    (the CSR transpose is built from it on the host side), everything else computes nothing."""

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
            if name == "eml_sphere_tap_table_f32":
                _, h, w, ho, wo, idx_p, wgt_p, _ = args
                stride = next(s for s in range(1, h + 1) if oracle.out_size(h, w, s) == (ho, wo))
                idx, wgt = oracle.tap_table(h, w, stride)
                idx = idx.to(torch.int32).contiguous()
                ctypes.memmove(idx_p.value, idx.data_ptr(), idx.numel() * 4)
                ctypes.memmove(wgt_p.value, wgt.data_ptr(), wgt.numel() * 4)
            return 64 if restype is ctypes.c_size_t else 0
        return call

    def of(self, name):
        return [a for n, a in self.args if n == name]


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    rec = _Recorder({**_lib.SIGNATURES, **_lib.EXT_SIGNATURES})
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(spherenet, "_GEOMETRY", {})          # geometries made here stay here
    return rec


class _FakeDeviceTensor(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _dev(t):
    return t.as_subclass(_FakeDeviceTensor)


# eml_sphere_max_pool_fwd_f32(x, idx, wgt, y, arg, B, n_src, n_dst, C, stream)
# eml_sphere_max_pool_bwd_f32(gy, arg, csr_ptr, csr_src, csr_w, gx, B, n_src, n_dst, C, stream)
def test_forward_and_backward_reach_the_entry_points(recorder):
    from emlight_amd.GenProjector import spherenet
    x = _dev(torch.randn(2, 4, 8, 16)).requires_grad_(True)
    y = spherenet.sphere_max_pool(x, 2)
    assert y.shape == (2, 4, 4, 8) and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
    geo = spherenet.sphere_geometry(8, 16, 2, x.device, "sphere")          # the table a SphereConv2D of this size uses
    f = recorder.of(FWD)[0]
    assert f[5:9] == (2, 128, 32, 4) and f[9] is None and f[4] is not None
    assert f[1].value == geo.idx.data_ptr() and f[2].value == geo.wgt.data_ptr() and f[0].value != x.data_ptr()
    assert recorder.calls.count("eml_sphere_tap_table_f32") == 1
    y.backward(torch.ones_like(y))
    b = recorder.of(BWD)[0]
    assert b[6:10] == (2, 128, 32, 4) and b[1].value == f[4].value
    assert (b[2].value, b[3].value, b[4].value) == (geo.csr_ptr.data_ptr(), geo.csr_src.data_ptr(), geo.csr_w.data_ptr())
    assert x.grad.shape == x.shape and b[5] is not None
    # the CSR the backward walks is the transpose of the real table: as many entries as taps on the map, M as the oracle's
    idx, _ = oracle.tap_table(8, 16, 2)
    assert geo.csr_src.numel() == int((idx >= 0).sum())
    assert int((geo.csr_ptr[1:] - geo.csr_ptr[:-1]).max()) == oracle.longest_row(idx, 128)
    # a channels-last input is used in place, odd sizes give a ceiling
    xc = _dev(torch.randn(1, 3, 5, 12).contiguous(memory_format=torch.channels_last))
    with torch.no_grad():
        y = spherenet.sphere_max_pool(xc, 2)
    f = recorder.of(FWD)[-1]
    assert y.shape == (1, 3, 3, 6) and f[0].value == xc.data_ptr() and f[5:9] == (1, 60, 18, 3)


def test_indices_are_kept_only_when_somebody_needs_them(recorder):
    from emlight_amd.GenProjector import spherenet
    x = _dev(torch.randn(1, 4, 8, 16))
    with torch.no_grad():
        spherenet.sphere_max_pool(_dev(torch.randn(1, 4, 8, 16)).requires_grad_(True))
    assert recorder.of(FWD)[-1][4] is None                   # no gradient, no return_indices: NULL
    spherenet.sphere_max_pool(x)
    assert recorder.of(FWD)[-1][4] is None                   # an input that takes no gradient
    with torch.no_grad():
        y, arg = spherenet.sphere_max_pool(x, 1, return_indices=True)
    assert recorder.of(FWD)[-1][4] is not None
    assert arg.shape == y.shape == (1, 4, 8, 16) and arg.dtype == torch.uint8 and not arg.requires_grad
    assert arg.is_contiguous(memory_format=torch.channels_last)
    xg = _dev(torch.randn(1, 4, 8, 16)).requires_grad_(True)
    y, arg = spherenet.sphere_max_pool(xg, return_indices=True)
    assert y.requires_grad and not arg.requires_grad
    n = len(recorder.of(BWD))
    y.sum().backward()
    assert len(recorder.of(BWD)) == n + 1


def test_backward_is_once_differentiable(recorder):
    from emlight_amd.GenProjector import spherenet
    x = _dev(torch.randn(1, 4, 8, 16)).requires_grad_(True)
    y = spherenet.sphere_max_pool(x)
    (gx,) = torch.autograd.grad((y * y).sum(), x, create_graph=True)     # an incoming gradient that itself has a graph
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        gx.sum().backward()


def test_cpu_tensors_and_other_dtypes_are_refused(recorder):
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    with pytest.raises(_lib.EmlightHipError, match="no CPU path"):
        spherenet.sphere_max_pool(torch.rand(1, 3, 8, 16))
    with pytest.raises(_lib.EmlightHipError, match="no CPU path"):
        spherenet.SphereMaxPool2D()(torch.rand(1, 3, 8, 16))
    with pytest.raises(_lib.EmlightHipError, match="float32"):
        spherenet.sphere_max_pool(_dev(torch.rand(1, 3, 8, 16).double()))
    with pytest.raises(ValueError):
        spherenet.sphere_max_pool(_dev(torch.rand(3, 8, 16)))
    assert FWD not in recorder.calls


def test_module_mirrors_the_reference_signature():
    from emlight_amd.GenProjector import networks, spherenet
    sig = inspect.signature(spherenet.SphereMaxPool2D.__init__)
    assert list(sig.parameters) == ["self", "stride", "mode"]
    assert sig.parameters["stride"].default == 1 and sig.parameters["mode"].default == "bilinear"
    m = spherenet.SphereMaxPool2D(stride=2)
    assert m.stride == 2 and m.mode == "bilinear"
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert list(inspect.signature(m.forward).parameters) == ["x"]
    with pytest.raises(NotImplementedError, match="half-way"):
        spherenet.SphereMaxPool2D(mode="nearest")
    with pytest.raises(NotImplementedError):
        spherenet.SphereMaxPool2D(2, "bicubic")
    # exported where SphereConv2D is
    assert networks.SphereMaxPool2D is spherenet.SphereMaxPool2D and networks.SphereConv2D is spherenet.SphereConv2D
    assert list(inspect.signature(spherenet.sphere_max_pool).parameters) == ["x", "stride", "return_indices"]


def test_module_forward_goes_through_sphere_max_pool(recorder):
    from emlight_amd.GenProjector import spherenet
    m = spherenet.SphereMaxPool2D(stride=2)
    y = m(_dev(torch.randn(1, 8, 16, 32)))
    assert y.shape == (1, 8, 8, 16) and recorder.of(FWD)[-1][5:9] == (1, 512, 128, 8)
