"""CPU: SamplesLoss(reach=...) reaches eml_sinkhorn_fwd_rho_f32 as rho = reach**p with arguments that convert to the bound
signature, reach=None keeps the balanced eml_sinkhorn_fwd_ex_f32 call, invalid reaches are refused, and the header, the
ctypes binding and the ABI version agree -- WITHOUT a GPU.

The HIP library is replaced by a recorder that validates each call's argument count and converts every argument with the
ctypes type declared in ``emlight_amd/_lib.py`` (the pattern of ``test_dry_run_abi.py``, restated here).  The launcher's own
argument validation is checked against the built library (it returns before anything touches a device)."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO_ARG, LAM_ARG, FLAGS_ARG = 21, 22, 20   # positions in eml_sinkhorn_fwd_rho_f32's argument list


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


def _xy(B=2, n=16):
    g = torch.Generator().manual_seed(0)
    x = torch.softmax(torch.randn(B, n, generator=g), 1).view(B, n, 1)
    y = torch.softmax(torch.randn(B, n, generator=g), 1).view(B, n, 1)
    return x, y


@pytest.mark.parametrize("reach,p", [(.3, 2), (.05, 2), (2.0, 1), (math.inf, 2)])
def test_reach_reaches_the_rho_entry_as_reach_to_the_p(recorder, reach, p):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy()
    x.requires_grad_(True)
    SamplesLoss("sinkhorn", p=p, blur=.05, reach=reach, anchors=16)(x, y).sum().backward()
    assert "eml_sinkhorn_fwd_ex_f32" not in recorder.calls
    args = recorder.last("eml_sinkhorn_fwd_rho_f32")
    assert args[RHO_ARG] == reach ** p and isinstance(args[RHO_ARG], float)
    assert args[LAM_ARG] is None                                  # the lam schedule is not asked for by forward()
    assert args[8] == p and args[18:20] == (2, 16)                # p, B, N
    assert "eml_sinkhorn_bwd_f32" in recorder.calls


def test_forward_raw_reports_the_lam_schedule_on_request(recorder):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy()
    r = SamplesLoss("sinkhorn", p=2, blur=.05, reach=.1, anchors=16).forward_raw(x, y, want_lam=True)
    args = recorder.last("eml_sinkhorn_fwd_rho_f32")
    assert r["lam"].shape == (64,) and args[LAM_ARG].value == r["lam"].data_ptr()
    assert args[RHO_ARG] == pytest.approx(.01, rel=1e-15)
    # balanced, but with the schedule requested: the rho entry with rho = 0 (lam = 1, the balanced launch)
    recorder.calls.clear()
    r = SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16).forward_raw(x, y, want_lam=True)
    assert recorder.calls[-1] == "eml_sinkhorn_fwd_rho_f32" and recorder.last("eml_sinkhorn_fwd_rho_f32")[RHO_ARG] == 0.0


def test_reach_none_keeps_the_balanced_call(recorder):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    x, y = _xy()
    x.requires_grad_(True)
    crit = SamplesLoss("sinkhorn", p=2, blur=.05, anchors=16)
    crit(x, y).sum().backward()
    crit.forward_raw(x.detach(), y)
    a = torch.full((2, 16), 1 / 16)
    crit(a, x.detach(), a, y)
    assert recorder.calls.count("eml_sinkhorn_fwd_ex_f32") == 3
    assert "eml_sinkhorn_fwd_rho_f32" not in recorder.calls
    assert len(recorder.last("eml_sinkhorn_fwd_ex_f32")) == 22


@pytest.mark.parametrize("reach", [0, 0.0, -1.0, -math.inf, float("nan"), "far", [1.0]])
def test_invalid_reach_raises_value_error(reach):
    from emlight_amd.RegressionNetwork.geomloss import SamplesLoss
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss as GMSamplesLoss
    with pytest.raises(ValueError):
        SamplesLoss("sinkhorn", reach=reach, anchors=16)
    with pytest.raises(ValueError):
        GMSamplesLoss("sinkhorn", reach=reach)


def test_gmloss_inherits_reach():
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    crit = SamplesLoss("sinkhorn", p=2, blur=.05, reach=.2, batchsize=3)
    assert crit.reach == .2 and crit.rho == pytest.approx(.04, rel=1e-15)
    assert SamplesLoss("sinkhorn").rho is None


def test_train_and_joint_mains_pass_reach_to_the_trainer(monkeypatch):
    """train.py / joint.py --reach: the trainers get it (default None: the balanced loss, nothing changes)."""
    from emlight_amd import joint
    from emlight_amd.RegressionNetwork import train
    seen = []

    class Stop(Exception):
        pass

    def stub(*a, **k):
        seen.append(k.get("reach"))
        raise Stop

    monkeypatch.setattr(train, "RegressionTrainer", stub)
    monkeypatch.setattr(joint, "JointTrainer", stub)
    for main, argv in ((train.main, ["--synthetic"]), (joint.main, [])):
        for extra, want in (([], None), (["--reach", ".1"], .1)):
            with pytest.raises(Stop):
                main(argv + extra)
            assert seen[-1] == want


def test_header_binding_and_abi_version_agree():
    from emlight_amd import _lib
    header = open(os.path.join(ROOT, "include", "emlight_hip.h")).read()
    assert _lib.ABI_VERSION == int(re.search(r"#define EML_ABI_VERSION (\d+)", header).group(1)) == 31
    decl = re.search(r"int eml_sinkhorn_fwd_rho_f32\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    _, argtypes = _lib.SIGNATURES["eml_sinkhorn_fwd_rho_f32"]
    assert len(params) == len(argtypes) == 24
    assert params[FLAGS_ARG] == "int flags" and params[RHO_ARG] == "double rho" and params[LAM_ARG] == "float* lam_out"
    assert argtypes[RHO_ARG] is ctypes.c_double
    ex = _lib.SIGNATURES["eml_sinkhorn_fwd_ex_f32"][1]
    assert argtypes[:FLAGS_ARG + 1] == ex[:FLAGS_ARG + 1] and argtypes[-1] == ex[-1]   # ex's arguments + rho, lam_out


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    from emlight_amd import _lib
    return _lib.lib()


def test_rho_entry_argument_validation_without_gpu(built_lib):
    L = built_lib
    one = ctypes.c_void_p(16)

    def call(rho=.01, flags=0, B=2, N=256, x=one):
        return L.eml_sinkhorn_fwd_rho_f32(x, one, one, one, None, None, .05, .5, 2, -1.0, None, None, None, None, one, None,
                                          None, one, B, N, flags, rho, None, None)

    assert call(rho=float("nan")) == -1 and b"NaN" in L.eml_last_error()
    assert call(flags=8) == -1 and b"unknown flags" in L.eml_last_error()
    assert call(x=None) == -1 and b"null" in L.eml_last_error()
    assert call(N=0) == -1
    assert call(B=0) == 0 and call(B=0, rho=-1.0) == 0 and call(B=0, rho=math.inf) == 0   # empty batch: nothing launched
