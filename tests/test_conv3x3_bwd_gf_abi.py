"""CPU: who gets the compact GF (P, 12) of the conv3x3 backward, and who may do without it.

The fused entry forms dW2 itself, so nobody reads the GF it used to store: the engine passes NULL and the kernel stores
nothing.  The unfused data entry still writes it for the separate weight-gradient launch and keeps requiring it.  Driven
through the recorder of ``tests/test_dry_run_abi.py`` (call sites against the bound C signatures, no GPU), then against the
built library's argument validation, which returns before any device work."""
import ctypes

import pytest
import torch

from tests.test_dry_run_abi import recorder  # noqa: F401  (the fixture)

FUSED = ("eml_dense_conv3x3_bwd_fused_f32", "eml_dense_conv3x3_bwd_fused_drop_f32")
DATA = ("eml_dense_conv3x3_bwd_data_f32", "eml_dense_conv3x3_bwd_data_drop_f32")
GF_ARG = 18   # G, ldg, c0, W2, Z, zmean, zistd, DZ, B, H, W, partials, grid, X, ldx, cx, sB, sC, GF


def _backward(recorder, drop_rate=0.0):
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    from emlight_amd.RegressionNetwork.dense_engine import HipDenseEncoder
    net = DenseNet(anchors=8, crop_hw=(32, 32), drop_rate=drop_rate).train()
    net._hip = HipDenseEncoder(net)
    net._hip._cu = 256
    sum(v.sum() for v in net(torch.rand(2, 3, 32, 32)).values()).backward()
    return net


@pytest.mark.parametrize("drop_rate", [0.0, 0.2])
def test_the_fused_entry_receives_no_gf(recorder, monkeypatch, drop_rate):  # noqa: F811
    monkeypatch.delenv("EML_C3_GF", raising=False)
    recorder.returns["eml_dense_conv3x3_bwd_fused_supported"] = 1
    _backward(recorder, drop_rate)
    fused = [a for n, a in recorder.args if n in FUSED]
    assert len(fused) == 48 and all(a[GF_ARG] is None for a in fused)
    assert all(n == FUSED[1 if drop_rate else 0] for n, _ in recorder.args if n in FUSED)
    assert not any(n in DATA or n == "eml_dense_conv3x3_bwd_weight_f32" for n in recorder.calls)


def test_no_gf_buffer_is_allocated_on_the_fused_path(recorder, monkeypatch):  # noqa: F811
    from emlight_amd.RegressionNetwork import dense_engine_bwd
    made = []
    init = dense_engine_bwd._BwdBuffers.__init__
    monkeypatch.setattr(dense_engine_bwd._BwdBuffers, "__init__", lambda self, *a: (init(self, *a), made.append(self))[0])
    monkeypatch.delenv("EML_C3_GF", raising=False)
    recorder.returns["eml_dense_conv3x3_bwd_fused_supported"] = 1
    _backward(recorder)
    assert made and all(t is None for b in made for t in b.GF12)
    # EML_C3_GF=1 (A/B): the buffer is handed over as before
    monkeypatch.setenv("EML_C3_GF", "1")
    n = len(recorder.args)
    _backward(recorder)
    fused = [a for nme, a in recorder.args[n:] if nme in FUSED]
    assert len(fused) == 48 and all(a[GF_ARG] is not None for a in fused)
    assert made[-1].GF12[0] is not None


@pytest.mark.parametrize("drop_rate", [0.0, 0.2])
def test_the_unfused_data_entry_always_receives_gf(recorder, monkeypatch, drop_rate):  # noqa: F811
    """The library's "not supported" (the stub's default 0) and EML_C3_FOLD=0 both take the two launches: the data entry writes
    the GF the weight-gradient entry then reads."""
    for fold, supported in (("1", 0), ("0", 1)):
        monkeypatch.setenv("EML_C3_FOLD", fold)
        recorder.returns["eml_dense_conv3x3_bwd_fused_supported"] = supported
        n = len(recorder.args)
        _backward(recorder, drop_rate)
        calls = recorder.args[n:]
        data = [a for nme, a in calls if nme in DATA]
        wgrad = [a for nme, a in calls if nme == "eml_dense_conv3x3_bwd_weight_f32"]
        assert len(data) == 48 and len(wgrad) == 48 and not any(nme in FUSED for nme, _ in calls)
        assert all(a[GF_ARG] is not None for a in data)
        assert all(ctypes.cast(d[GF_ARG], ctypes.c_void_p).value == ctypes.cast(w[0], ctypes.c_void_p).value
                   for d, w in zip(data, wgrad))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(256)
    data = lambda GF=one: L.eml_dense_conv3x3_bwd_data_f32(one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64, one, 224, 24,
                                                           one, one, GF, None)
    assert data(GF=None) == -1 and b"GF" in L.eml_last_error()
    data_drop = lambda GF=one: L.eml_dense_conv3x3_bwd_data_drop_f32(one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64, one,
                                                                     224, 24, one, one, GF, 5, 0, 0.2, None)
    assert data_drop(GF=None) == -1 and b"GF" in L.eml_last_error()
    # The fused entries accept GF == NULL: what they refuse next -- an argument checked AFTER the NULL test -- shows that the
    # NULL passed (a launch is never reached: no device is needed)
    fused = lambda GF=one, X=one: L.eml_dense_conv3x3_bwd_fused_f32(one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64, X, 224,
                                                                    24, one, one, GF, one, one, one, one, None)
    fused_drop = lambda GF=one, X=one: L.eml_dense_conv3x3_bwd_fused_drop_f32(one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64,
                                                                              X, 224, 24, one, one, GF, one, one, one, one, 5, 0,
                                                                              0.2, None)
    odd = ctypes.c_void_p(260)
    for f in (fused, fused_drop):
        assert f(GF=None, X=odd) == -1 and b"aligned" in L.eml_last_error()      # past "bad arguments"
        assert f(GF=one, X=odd) == -1 and b"aligned" in L.eml_last_error()
        assert f(GF=odd) == -1 and b"aligned" in L.eml_last_error()              # a buffer that IS given must be aligned
        assert f(GF=None, X=None) == -1 and b"bad arguments" in L.eml_last_error()
