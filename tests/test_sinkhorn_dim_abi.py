"""CPU: SamplesLoss on (B, N, D) samples reaches eml_sinkhorn_fwd_dim_f32 with D and a 2*D range buffer, D = 1 keeps the
exact call it made before, weights that require grad reach eml_sinkhorn_bwd_weights_f32, D out of bounds is refused, and
the launchers validate their arguments -- WITHOUT a GPU.

The HIP library is replaced by the argument recorder of ``test_sinkhorn_reach_abi.py`` (restated here); the launchers'
own validation is checked against the built library (it returns before anything touches a device)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ARG, FLAGS_ARG, RHO_ARG = 20, 21, 22   # positions in eml_sinkhorn_fwd_dim_f32's argument list


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
            if name == "eml_sinkhorn_dim_work_floats":
                return (4 + 4 * args[2]) * args[0] * args[1]
            if name == "eml_sinkhorn_work_floats":
                return 24 * args[0] * args[1] + 4
            return 0
        return call

    def last(self, name):
        return [a for n, a in self.args if n == name][-1]


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib
    rec = _Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name, dtype=None: t.contiguous())
    return rec


@pytest.fixture
def ranges(monkeypatch):
    """Every range buffer global_range hands to a call."""
    from emlight_amd.RegressionNetwork.geomloss import samples_loss as sl
    seen, orig = [], sl.global_range

    def rec(x, y):
        r = orig(x, y)
        seen.append(r)
        return r
    monkeypatch.setattr(sl, "global_range", rec)
    return seen


def _xy(B=2, n=16, D=3):
    g = torch.Generator().manual_seed(0)
    return torch.softmax(torch.randn(B, n, D, generator=g), 1), torch.softmax(torch.randn(B, n, D, generator=g), 1)


@pytest.mark.parametrize("D", [2, 3, 4, 8])
def test_d_above_one_reaches_the_dim_entry_with_d_and_a_2d_range(recorder, ranges, D):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy(D=D)
    x.requires_grad_(True)
    loss = SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16, sync_diameter=True)(x, y)
    assert loss.shape == (2,)
    loss.sum().backward()
    assert "eml_sinkhorn_fwd_ex_f32" not in recorder.calls and "eml_sinkhorn_fwd_rho_f32" not in recorder.calls
    args = recorder.last("eml_sinkhorn_fwd_dim_f32")
    assert args[18:21] == (2, 16, D) and args[RHO_ARG] == 0.0
    assert ("eml_sinkhorn_dim_work_floats", (2, 16, D)) in recorder.args
    assert len(ranges) == 1 and ranges[0].shape == (2 * D,) and args[10].value == ranges[0].data_ptr()
    lo, hi = ranges[0][:D], ranges[0][D:]
    assert torch.equal(lo, torch.minimum(x.detach().reshape(-1, D).amin(0), y.reshape(-1, D).amin(0)))
    assert torch.equal(hi, torch.maximum(x.detach().reshape(-1, D).amax(0), y.reshape(-1, D).amax(0)))
    assert x.grad.shape == (2, 16, D)
    bwd = recorder.last("eml_sinkhorn_bwd_f32")
    assert bwd[3:5] == (2, 16 * D)   # the row scaling runs over the N * D gradient entries of a sample
    r = SamplesLoss("sinkhorn", p=2, blur=.05, reach=.1, anchors=16).forward_raw(x.detach(), y, want_lam=True)
    args = recorder.last("eml_sinkhorn_fwd_dim_f32")
    assert args[RHO_ARG] == pytest.approx(.01) and args[23].value == r["lam"].data_ptr()
    assert r["gx"].shape == (2, 16, D) and r["gy"].shape == (2, 16, D) and r["duals"].shape == (4, 2, 16)


def test_d1_keeps_the_exact_call(recorder, ranges):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy(D=1)
    x.requires_grad_(True)
    SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16, sync_diameter=True)(x, y).sum().backward()
    assert "eml_sinkhorn_fwd_dim_f32" not in recorder.calls and "eml_sinkhorn_bwd_weights_f32" not in recorder.calls
    args = recorder.last("eml_sinkhorn_fwd_ex_f32")
    assert len(args) == 22 and args[18:21] == (2, 16, 0)
    assert ranges[0].shape == (2,)
    assert recorder.last("eml_sinkhorn_bwd_f32")[3:5] == (2, 16)


@pytest.mark.parametrize("D", [1, 3])
def test_weights_that_require_grad_get_gradients_of_their_shape(recorder, D):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy(D=D)
    a = torch.full((2, 16, 1), 1 / 16, requires_grad=True)   # the caller's shape
    b = torch.full((2, 16), 1 / 16)
    SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16)(a, x, b, y).sum().backward()
    args = recorder.last("eml_sinkhorn_bwd_weights_f32")
    assert args[2] is not None and args[3] is None and args[4:6] == (2, 16)
    fwd = recorder.last("eml_sinkhorn_fwd_dim_f32" if D > 1 else "eml_sinkhorn_fwd_ex_f32")
    assert args[1].value == fwd[17].value   # the duals of that forward's scratch
    assert a.grad is not None and a.grad.shape == (2, 16, 1)
    b.requires_grad_(True)
    SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16)(a.detach(), x, b, y).sum().backward()
    args = recorder.last("eml_sinkhorn_bwd_weights_f32")
    assert args[2] is None and args[3] is not None and b.grad.shape == (2, 16)


def test_d_out_of_bounds_and_mismatched_shapes_raise_value_error():
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    from emlight_amd.RegressionNetwork.geomloss.samples_loss import MAX_DIM
    assert MAX_DIM == 8
    crit = SamplesLoss("sinkhorn", anchors=16)
    with pytest.raises(ValueError, match="D <= 8"):
        crit(torch.rand(2, 16, 9), torch.rand(2, 16, 9))
    with pytest.raises(ValueError, match="D <= 8"):
        crit(torch.rand(2, 16, 0), torch.rand(2, 16, 0))
    with pytest.raises(ValueError):
        crit(torch.rand(2, 16, 3), torch.rand(2, 16, 2))
    with pytest.raises(ValueError):
        crit(torch.rand(2, 16), torch.rand(2, 16))


def test_header_binding_and_bound_agree():
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    assert int(re.search(r"#define EML_SINKHORN_MAX_DIM (\d+)", header).group(1)) == 8
    decl = re.search(r"int eml_sinkhorn_fwd_dim_f32\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    _, argtypes = _lib.SIGNATURES["eml_sinkhorn_fwd_dim_f32"]
    assert len(params) == len(argtypes) == 25
    assert params[D_ARG] == "int D" and params[FLAGS_ARG] == "int flags" and params[RHO_ARG] == "double rho"
    rho = _lib.SIGNATURES["eml_sinkhorn_fwd_rho_f32"][1]
    assert argtypes[:D_ARG] + argtypes[D_ARG + 1:] == rho   # the rho entry's arguments + D after N
    for name in ("eml_sinkhorn_dim_work_floats", "eml_sinkhorn_schedule_dim_f32", "eml_sinkhorn_bwd_weights_f32"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_dim_entry_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def call(D=3, B=2, N=256, x=one, work=one, flags=0, rho=0.0):
        return L.eml_sinkhorn_fwd_dim_f32(x, one, one, one, None, None, .05, .5, 2, -1.0, None, None, None, None, one, None,
                                          None, work, B, N, D, flags, rho, None, None)

    assert call(D=0) == -1 and b"D <= 8" in L.eml_last_error()
    assert call(D=9) == -1 and b"D <= 8" in L.eml_last_error()
    assert call(x=None) == -1 and b"null" in L.eml_last_error()
    assert call(work=None) == -1 and b"null" in L.eml_last_error()
    assert call(N=0) == -1 and call(N=4096) == -1
    assert call(flags=8) == -1 and b"unknown flags" in L.eml_last_error()
    assert call(rho=float("nan")) == -1 and b"NaN" in L.eml_last_error()
    assert call(B=0) == 0 and call(B=0, D=8) == 0   # empty batch: nothing launched
    # work sizes: D = 1 is the 1-D scratch (split exchange buffer and status word included), D > 1 duals + D rows
    for B, N in ((2, 96), (16, 256), (3, 202)):
        assert L.eml_sinkhorn_dim_work_floats(B, N, 1) == L.eml_sinkhorn_work_floats(B, N)
        for D in range(2, 9):
            assert L.eml_sinkhorn_dim_work_floats(B, N, D) == (4 + 4 * D) * B * N
    assert L.eml_sinkhorn_dim_work_floats(2, 96, 0) == 0 and L.eml_sinkhorn_dim_work_floats(2, 96, 9) == 0
    assert L.eml_sinkhorn_schedule_dim_f32(one, one, 64, 9, .05, .5, 2, -1.0, None, one, one, one, None) == -1
    assert L.eml_sinkhorn_schedule_dim_f32(one, one, 64, 3, .05, .5, 2, -1.0, None, None, one, one, None) == -1
    assert L.eml_sinkhorn_bwd_weights_f32(one, one, None, None, 2, 16, None) == -1
    assert L.eml_sinkhorn_bwd_weights_f32(None, one, one, None, 2, 16, None) == -1
    assert L.eml_sinkhorn_bwd_weights_f32(one, one, one, None, 0, 16, None) == 0
