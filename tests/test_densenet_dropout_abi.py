"""CPU: the DenseNet encoder's dropout (drop_rate > 0, DenseNet.py:50-55) reaches the C ABI -- the ``_drop_`` conv3x3 entry
points, once per dense layer in each direction, with the layer's global index, p and one key per forward -- WITHOUT a GPU;
drop_rate = 0 and eval mode issue exactly today's launches; the key follows torch's default CPU generator or a pinned value;
stream capture is refused.  The HIP library is replaced by the recorder of ``test_densenet_input_grad_abi.py`` (restated
here).  The new launchers' argument validation is checked against the built library (nothing touches a device)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("eml_dense_conv3x3_fwd_drop_f32", "eml_dense_conv3x3_fwd_tp_drop_f32")
BWD = ("eml_dense_conv3x3_bwd_data_drop_f32", "eml_dense_conv3x3_bwd_fused_drop_f32")
NEW = FWD + BWD + ("eml_dense_dropout_mask_u16",)


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


def _net(drop_rate, B=2, crop=(32, 32)):
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    from emlight_amd.RegressionNetwork.dense_engine import HipDenseEncoder
    torch.manual_seed(0)
    net = DenseNet(anchors=8, crop_hw=crop, drop_rate=drop_rate).train()
    net._hip = HipDenseEncoder(net)
    net._hip._cu = 256
    return net, torch.rand(B, 3, *crop)


def _step(net, x):
    sum(v.sum() for v in net(x).values()).backward()


def test_constructs_and_validates_drop_rate():
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    net = DenseNet(drop_rate=0.2)
    assert net.features.denseblock3.denselayer16.drop_rate == 0.2
    DenseNet(drop_rate=1)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="between 0 and 1"):
            DenseNet(drop_rate=bad)
    with pytest.raises(ValueError):
        net.set_dropout_key(-1)
    with pytest.raises(ValueError):
        net.set_dropout_key(2 ** 64)


def test_header_declares_the_bound_signatures():
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    for name in NEW:
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        params = [q.strip() for q in decl.split(",")]
        _, argtypes = _lib.SIGNATURES[name]
        assert len(params) == len(argtypes), name
        assert "unsigned long long seed" in params and "double p" in params
        assert argtypes[params.index("unsigned long long seed")] is ctypes.c_ulonglong
        assert argtypes[params.index("double p")] is ctypes.c_double
    i = header.index("int eml_dense_conv3x3_fwd_drop_f32")
    assert "DenseNet.py:50-55" in header[i - 1500:i]
    i = header.index("int eml_dense_conv3x3_bwd_data_drop_f32")
    assert "DenseNet.py:50-55" in header[i - 1000:i]


def test_train_step_calls_the_drop_entry_points_once_per_layer(recorder):
    net, x = _net(0.2)
    net.features.denseblock2.denselayer3.drop_rate = 0.5     # read per layer, at every forward
    net.set_dropout_key(12345)
    _step(net, x)
    fwd = [a for n, a in recorder.args if n in FWD]
    bwd = [a for n, a in recorder.args if n in BWD]
    assert len(fwd) == len(bwd) == 48
    assert "eml_dense_conv3x3_fwd_f32" not in recorder.calls and "eml_dense_conv3x3_bwd_data_f32" not in recorder.calls
    assert [a[-4] for a in fwd] == [12345] * 48 and [a[-4] for a in bwd] == [12345] * 48
    assert [a[-3] for a in fwd] == list(range(48)) and sorted(a[-3] for a in bwd) == list(range(48))
    ps = {a[-3]: a[-2] for a in fwd}
    assert ps[16 + 2] == 0.5 and all(v == 0.2 for k, v in ps.items() if k != 18)
    assert {a[-3]: a[-2] for a in bwd} == ps
    assert net._hip.last_dropout_key == 12345


def test_zero_rate_and_eval_mode_issue_todays_launches(recorder):
    base, x = _net(0.0)
    _step(base, x)
    recorder.calls.clear()
    _step(base, x)
    plain = list(recorder.calls)
    net, _ = _net(0.2)
    for L in net.modules():
        if hasattr(L, "drop_rate"):
            L.drop_rate = 0.0
    _step(net, x)
    recorder.calls.clear()
    _step(net, x)
    assert recorder.calls == plain and net._hip.last_dropout_key is None
    # eval mode: no dropout (forward only: eval-mode backward is refused)
    base.eval()
    with torch.no_grad():
        base(x)                               # (the first eval forward builds its workspace)
        recorder.calls.clear()
        base(x)
    plain_eval = list(recorder.calls)
    net, _ = _net(0.3)
    net.eval()
    with torch.no_grad():
        net(x)
        recorder.calls.clear()
        net(x)
    assert recorder.calls == plain_eval and not set(NEW).intersection(recorder.calls)
    # one layer back in training mode drops alone, also under no_grad
    net.features.denseblock1.denselayer4.train()
    recorder.calls.clear()
    with torch.no_grad():
        net(x)
    assert [a[-3] for n, a in recorder.args[-len(recorder.calls):] if n in FWD] == [3]


def test_key_follows_torch_default_generator_or_the_pinned_value(recorder):
    net, x = _net(0.2)
    keys = []
    for _ in range(2):
        torch.manual_seed(7)
        with torch.no_grad():
            net(x)
        keys.append(net._hip.last_dropout_key)
    with torch.no_grad():
        net(x)
    assert keys[0] == keys[1] != net._hip.last_dropout_key
    assert 0 <= keys[0] < 2 ** 64
    # p = 0 draws nothing: the generator is not advanced
    torch.manual_seed(7)
    before = torch.get_rng_state()
    base, _ = _net(0.0)
    torch.set_rng_state(before)
    with torch.no_grad():
        base(x)
    assert torch.equal(torch.get_rng_state(), before)
    net.set_dropout_key(2 ** 64 - 1)
    with torch.no_grad():
        net(x)
    assert net._hip.last_dropout_key == 2 ** 64 - 1
    assert [a[-4] for n, a in recorder.args if n in FWD][-1] == 2 ** 64 - 1


def test_invalid_rate_at_forward_raises(recorder):
    net, x = _net(0.2)
    net.features.denseblock3.denselayer2.drop_rate = 1.5
    with pytest.raises(ValueError, match="between 0 and 1"):
        net(x)
    assert not recorder.calls


def test_refused_under_stream_capture(recorder, monkeypatch):
    from emlight_amd.RegressionNetwork import dense_engine
    monkeypatch.setattr(dense_engine, "_capturing", lambda x: True)
    net, x = _net(0.2)
    with pytest.raises(RuntimeError, match="captured"):
        net(x)
    assert not recorder.calls
    base, _ = _net(0.0)
    base(x)                                  # drop_rate = 0 captures as before
    assert recorder.calls


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(256)
    fwd = lambda p=0.2, layer=0, B=1, X=one: L.eml_dense_conv3x3_fwd_drop_f32(one, one, one, one, X, 224, 24, B, 8, 8, one, 64, 5,
                                                                                 layer, p, None)
    assert fwd(X=None) == -1 and b"bad arguments" in L.eml_last_error()
    assert fwd(p=1.5) == -1 and b"p must be in [0, 1]" in L.eml_last_error()
    assert fwd(p=-0.1) == -1 and fwd(p=float("nan")) == -1 and fwd(layer=-1) == -1
    assert fwd(B=2 ** 26) == -1 and b"32-bit" in L.eml_last_error()
    tp = lambda p=0.2, W=64: L.eml_dense_conv3x3_fwd_tp_drop_f32(one, one, one, one, one, 224, 24, 1, 8, W, 4, one, 64, 5, 0, p,
                                                                  None)
    assert tp(p=2.0) == -1 and b"p must be" in L.eml_last_error()
    assert tp(W=96) == -1 and b"is not 16" in L.eml_last_error()
    bd = lambda X=one, p=0.2: L.eml_dense_conv3x3_bwd_data_drop_f32(one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64, X,
                                                                     224, 24, one, one, one, 5, 0, p, None)
    assert bd(X=None) == -1 and b"fused affine" in L.eml_last_error()
    assert bd(p=1.01) == -1 and b"p must be" in L.eml_last_error()
    bf = lambda X=one, p=0.2, layer=0: L.eml_dense_conv3x3_bwd_fused_drop_f32(
        one, 224, 24, one, one, one, one, one, 1, 8, 8, one, 64, X, 224, 24, one, one, one, one, one, one, one, 5, layer, p, None)
    assert bf(X=None) == -1 and b"bad arguments" in L.eml_last_error()
    assert bf(p=-1.0) == -1 and bf(layer=-3) == -1 and b"layer >= 0" in L.eml_last_error()
    assert bf(X=ctypes.c_void_p(260)) == -1 and b"aligned" in L.eml_last_error()
    mk = lambda P=64, mask=one, p=0.2: L.eml_dense_dropout_mask_u16(1, 0, p, P, mask, None)
    assert mk(mask=None) == -1 and mk(P=0) == -1 and mk(P=2 ** 31) == -1 and mk(p=1.5) == -1
    assert b"eml_dense_dropout_mask_u16" in L.eml_last_error()
