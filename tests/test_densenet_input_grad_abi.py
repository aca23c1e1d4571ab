"""CPU: the DenseNet encoder's gradient with respect to its input image reaches the C ABI (eml_dense_conv0_bwd_data_f32)
with arguments that convert to the bound signature, exactly once and only when ``x`` asks for it, and frozen parameters get
neither a gradient nor a gradient-bucket slot -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_dry_run_abi.py``, restated here).  The launcher's own
argument validation is checked against the built library (it returns before anything touches a device)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "eml_dense_conv0_bwd_data_f32"


class _Recorder:
    def __init__(self, signatures):
        self.signatures, self.calls, self.args = signatures, [], []

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        _, argtypes = self.signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, call site passes %d" % (name, len(argtypes), len(args))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) does not convert to %s" % (name, k, a, t.__name__)) from e
            self.calls.append(name)
            self.args.append((name, args))
            return 0
        return call


@pytest.fixture
def recorder(monkeypatch):
    from emlight_amd import _lib
    rec = _Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name, dtype=None: t.contiguous())
    return rec


def _net(B=2, crop=(32, 32)):
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    from emlight_amd.RegressionNetwork.dense_engine import HipDenseEncoder
    net = DenseNet(anchors=8, crop_hw=crop).train()
    net._hip = HipDenseEncoder(net)
    net._hip._cu = 256
    return net, torch.rand(B, 3, *crop)


def _ptr(a):
    return a.value if isinstance(a, ctypes.c_void_p) else a


def _step(net, x):
    sum(v.sum() for v in net(x).values()).backward()


def test_header_declares_the_bound_signature():
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    decl = re.search(r"int %s\((.*?)\);" % ENTRY, header, re.S).group(1)
    params = [q.strip() for q in decl.split(",")]
    _, argtypes = _lib.SIGNATURES[ENTRY]
    assert len(params) == len(argtypes) == 19
    assert params[2] == "const float* X1" and params[13] == "const float* W0" and params[17] == "float* dX"
    for decl_, t in zip(params, argtypes):
        assert (t is ctypes.c_int) == decl_.startswith("int "), decl_
    assert "DenseNet.py:88-93" in header[header.index(ENTRY) - 1200:header.index(ENTRY)]   # the reference citation


@pytest.mark.parametrize("fused", ["1", "0"])
def test_input_gradient_launches_once_on_both_norm0_paths(recorder, monkeypatch, fused):
    monkeypatch.setenv("EML_NORM0_FUSED", fused)
    net, x = _net()
    x.requires_grad_(True)
    _step(net, x)
    launches = [a for n, a in recorder.args if n == ENTRY]
    assert len(launches) == 1
    a = launches[0]
    # after conv0's weight gradient, which reads the same G / Y0 / coefficient vectors
    wname = "eml_dense_conv0_bwd_weight_fused_f32" if fused == "1" else "eml_dense_conv0_bwd_weight_f32"
    assert recorder.calls.index(wname) < recorder.calls.index(ENTRY) == len(recorder.calls) - 1
    (w,) = [b for n, b in recorder.args if n == wname]
    assert _ptr(a[0]) == _ptr(w[1]) and a[1] == w[2]                        # G, ldg
    assert (a[2] is None) == (fused == "1")                                # X1 == NULL selects the fused form
    assert a[5] == 24 and a[14:17] == (2, 32, 32)                          # C0, B, H, W
    assert _ptr(a[13]) == net.features.conv0.weight.data_ptr()
    assert x.grad is not None and x.grad.shape == x.shape and _ptr(a[17]) == x.grad.data_ptr()
    assert all(q.grad is not None for q in net.parameters())


def test_parameters_only_backward_issues_todays_launches(recorder):
    net, x = _net()
    _step(net, x)                                        # (the first step also builds the workspace)
    recorder.calls.clear()
    net.zero_grad(set_to_none=True)
    _step(net, x)
    base = list(recorder.calls)
    assert ENTRY not in base and x.grad is None
    recorder.calls.clear()
    net.zero_grad(set_to_none=True)
    x.requires_grad_(True)
    _step(net, x)
    assert recorder.calls == base + [ENTRY]                                # the same sequence, then the data gradient


def test_frozen_parameters_get_no_grad_and_no_bucket_slot(recorder, monkeypatch):
    from emlight_amd import _dist
    asked = []
    monkeypatch.setattr(_dist, "grad_slot", lambda param=None, ptr=None: asked.append(id(param)))
    net, x = _net()
    for q in net.parameters():
        q.requires_grad_(False)
    x.requires_grad_(True)
    _step(net, x)                                        # x only: the forward keeps its activations, the backward runs
    assert x.grad is not None and recorder.calls.count(ENTRY) == 1
    assert asked == [] and all(q.grad is None for q in net.parameters())
    # partial freezing: conv0 and the first dense block frozen, the rest (heads included) trainable
    frozen = set(id(q) for q in [net.features.conv0.weight, net.features.norm0.weight]
                 + list(net.features.denseblock1.parameters()))
    for q in net.parameters():
        q.requires_grad_(id(q) not in frozen)
    x.grad = None
    n = len(recorder.calls)
    _step(net, x)
    assert recorder.calls[n:].count(ENTRY) == 1 and x.grad is not None
    assert asked and not frozen.intersection(asked)
    for q in net.parameters():
        assert (q.grad is None) == (id(q) in frozen)
    # without x: the same weight-gradient launches, no data gradient
    x.requires_grad_(False)
    n = len(recorder.calls)
    _step(net, x)
    assert ENTRY not in recorder.calls[n:] and "eml_dense_conv0_bwd_weight_fused_f32" in recorder.calls[n:]


def test_eval_mode_input_gradient_is_refused(recorder):
    """x alone now keeps the forward's activations, so the backward reaches the train-mode-only error, not "activations gone"."""
    net, x = _net()
    for q in net.parameters():
        q.requires_grad_(False)
    net.eval()
    x.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="train-mode"):
        _step(net, x)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)

    def call(G=one, ldg=224, X1=None, ldx=0, Y0=one, C0=24, s=one, cA=one, W0=one, B=1, H=8, W=8, dX=one):
        return L.eml_dense_conv0_bwd_data_f32(G, ldg, X1, ldx, Y0, C0, s, s, s, s, cA, cA, cA, W0, B, H, W, dX, None)

    assert call(G=None) == -1 and b"null" in L.eml_last_error()
    assert call(W0=None) == -1 and call(dX=None) == -1
    assert call(s=None) == -1 and b"null" in L.eml_last_error()          # the fused form needs scale0, shift0, sB, sC
    assert call(C0=12) == -1 and b"C0 == 24" in L.eml_last_error()
    assert call(ldg=226) == -1 and call(ldg=20) == -1 and call(B=0) == -1 and call(W=0) == -1
    assert call(X1=one, ldx=6) == -1 and b"bad shape" in L.eml_last_error()
    assert call(G=odd) == -1 and b"aligned" in L.eml_last_error()
    assert call(X1=odd, ldx=224) == -1 and b"aligned" in L.eml_last_error()
    assert call(B=2 ** 30, H=2 ** 12, W=2 ** 12) == -1 and b"tiles" in L.eml_last_error()
