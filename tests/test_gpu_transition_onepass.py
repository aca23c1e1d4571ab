"""GPU: the passes over HBM that the step no longer makes leave every result BIT-IDENTICAL.

* ``EML_TRANS_ONEPASS`` (default 1): ``eml_dense_conv1x1_fwd_f32`` with Cout > 48, no pool and no mask -- the transition
  convs -- runs as many 48-channel chunks per dispatch as LDS holds the weights of (conv1x1_fwd_wide_kernel) instead of one
  dispatch per chunk.  The library reads the knob once, so each setting runs in a fresh child process; compared with
  ``torch.equal``: T, the f64 partials, dW of the transition conv and what ``eml_dense_bn_bwd_finalize_f32`` derives from it.
* ``GF == NULL`` on the fused conv3x3 backward (what the engine passes; ``EML_C3_GF=1`` hands the buffer over as before):
  DZ, the partials and dW2 against the same call with GF given, with and without dropout.
* One whole training step (predictions, loss, every gradient, every updated weight and buffer) between the knobs set to the
  old and to the new behaviour.

Run as a script (``python tests/test_gpu_transition_onepass.py CASE OUT``) it is the child: it writes CASE's tensors to OUT."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64
# (P, Cin, Cout): EMLight's three transitions at the golden fixture's resolution (B = 2, 192 x 256 crops: 24 x 32, 12 x 16 and
# 6 x 8 output pixels per image), then ragged ones: P not a multiple of 256, Cout not a multiple of 16 -- together they run
# every instantiation of the wide kernel (7 | 6 + 4 | 6 + 5 | 8 | 9 output tiles) and a lone last chunk (Kp = 320 holds two
# chunks' weights: 2 + 1)
TRANSITIONS = [(1536, 216, 108), (384, 300, 150), (96, 342, 171), (1000, 200, 123), (777, 100, 140), (200, 310, 130)]


def r16(v):
    return (v + 15) // 16 * 16


def _transition_case(P, Cin, Cout):
    from emlight_amd import _lib as lib
    L, p, st = lib.lib(), lib.ptr, lib.current_stream()
    g = torch.Generator(device=DEV).manual_seed(1000 * P + Cout)
    rnd = lambda *s, scale=1.0: torch.randn(*s, device=DEV, generator=g) * scale
    Kp, Ko = r16(Cin), r16(Cout)
    A = rnd(P, Kp)
    A[:, Cin:] = 0
    sc, sh = torch.zeros(Kp, device=DEV), torch.zeros(Kp, device=DEV)
    sc[:Cin], sh[:Cin] = torch.rand(Cin, device=DEV, generator=g) + 0.5, rnd(Cin, scale=0.3)
    Wt = rnd(Cout, Cin, scale=1.0 / np.sqrt(Cin))
    nch = (Cout + 47) // 48
    Wp = torch.empty(nch * Kp * 48, device=DEV)
    lib.check(L.eml_dense_permute_w1_f32(p(Wt), Cout, Cin, Kp, p(Wp), st), "permute")
    T = torch.full((P, Ko), 3.0, device=DEV)
    part = torch.full((nch * G * 96,), 7.0, dtype=torch.float64, device=DEV)
    lib.check(L.eml_dense_conv1x1_fwd_f32(p(A), Kp, P, 1, P, 0, Kp, p(sc), p(sh), p(Wp), Cout, p(T), Ko, p(part), G, None, st),
              "conv1x1 fwd")
    # the transition conv's weight gradient on the same operand, and the BatchNorm backward that takes S2 from it
    DY = rnd(P, Ko)
    cA, cB, cC = (torch.zeros(Ko, device=DEV) for _ in range(3))
    cA[:Cout], cB[:Cout], cC[:Cout] = rnd(Cout), rnd(Cout, scale=0.1), rnd(Cout, scale=0.1)
    partW = torch.empty(G * Kp * 48, device=DEV)
    dW = torch.empty(Cout, Cin, device=DEV)
    lib.check(L.eml_dense_conv1x1_bwd_weight_f32(p(A), Kp, P, 1, P, 0, Kp, Cin, p(sc), p(sh), p(DY), Ko, p(T), Ko, p(cA), p(cB),
                                                 p(cC), Cout, p(partW), p(dW), G, None, None, 0, None, 0, None, None, st), "wgrad")
    S = torch.randn(G * Kp * 2, device=DEV, generator=g, dtype=torch.float64)
    S.view(G, Kp, 2)[:, :, 1] = 0
    gamma, mean, istd, beta = torch.rand(Cin, device=DEV, generator=g) + 0.5, rnd(Cin, scale=0.1), \
        torch.rand(Cin, device=DEV, generator=g) + 0.5, rnd(Cin, scale=0.3)
    dg, db = torch.empty(Cin, device=DEV), torch.empty(Cin, device=DEV)
    lib.check(L.eml_dense_bn_bwd_finalize_f32(p(S), G, 2 * Kp, float(4 * P), p(gamma), p(mean), p(istd), Cin, Kp, 1, p(dg), p(db),
                                              None, None, None, None, None, 0, 0, Kp, p(beta), p(Wt), p(dW), Cout, None, None,
                                              st), "finalize from dW")
    torch.cuda.synchronize()
    return {"T": T, "partials": part, "dW": dW, "dgamma": dg, "dbeta": db}


def _train_step_case():
    import oracle
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    keys = ("distribution", "intensity", "rgb_ratio", "ambient")
    z = np.load(os.path.join(ROOT, "tests", "golden", "densenet.npz"))
    tr = RegressionTrainer(anchors=96, crop_hw=(192, 256), blur=.025, device="cuda:0")
    tr.model.load_state_dict(oracle.deterministic_state_dict(oracle.OracleDenseNet().state_dict(), seed=0))
    batch = {k: torch.from_numpy(z["train/gt_" + k]).cuda() for k in keys}
    batch["crop"] = torch.from_numpy(np.random.default_rng([0]).random((2, 3, 192, 256), dtype=np.float32)).cuda()
    loss, terms = tr.step(batch)
    out = {"loss": loss.detach()}
    out.update({"term/" + k: v.detach() for k, v in terms.items()})
    out.update({"pred/" + k: tr.last_pred[k].detach() for k in keys})
    out.update({"grad/" + n: q.grad for n, q in tr.model.named_parameters()})
    out.update({"state/" + n: v for n, v in tr.model.state_dict().items()})
    torch.cuda.synchronize()
    return out


def _child(case, env):
    """CASE in a fresh process under `env` (on top of this one's): the library parses its knobs once per process."""
    import tempfile
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case, path], env=e, cwd=ROOT, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, "child %s %s failed:\n%s\n%s" % (case, env, r.stdout[-2000:], r.stderr[-4000:])
        return torch.load(path, map_location="cpu")


def _assert_equal(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        a, b = new[k], old[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        same = torch.equal(a, b)
        print("%s %s: %s" % (what, k, "bit-identical" if same else "max |diff| %g" % float((a.double() - b.double()).abs().max())))
        assert same, (what, k)


@pytest.fixture(scope="module")
def transition_runs():
    return {knob: _child("transitions", {"EML_TRANS_ONEPASS": knob}) for knob in ("1", "0")}


@pytest.mark.parametrize("P,Cin,Cout", TRANSITIONS)
def test_transition_conv_is_bit_identical_to_the_chunk_loop(transition_runs, P, Cin, Cout):
    key = "%d_%d_%d" % (P, Cin, Cout)
    new, old = transition_runs["1"][key], transition_runs["0"][key]
    _assert_equal(new, old, "transition " + key)
    # ... and it is the conv: T against f64, every column past Cout untouched
    ref = _transition_case_reference(P, Cin, Cout)
    err = (new["T"][:, :Cout].double() - ref).abs().max()
    assert float(err) <= 2e-5 * float(ref.abs().max()), float(err)
    assert bool((new["T"][:, Cout:] == 3.0).all())


def _transition_case_reference(P, Cin, Cout):
    g = torch.Generator(device=DEV).manual_seed(1000 * P + Cout)
    rnd = lambda *s, scale=1.0: torch.randn(*s, device=DEV, generator=g) * scale
    A = rnd(P, r16(Cin))[:, :Cin].double()
    sc, sh = torch.rand(Cin, device=DEV, generator=g) + 0.5, rnd(Cin, scale=0.3)
    Wt = rnd(Cout, Cin, scale=1.0 / np.sqrt(Cin))
    return ((A * sc.double() + sh.double()).clamp_min(0) @ Wt.double().t()).cpu()


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("B,H,W,c0,ld,compact", [(2, 48, 64, 24, 224, False), (2, 24, 32, 120, 304, True), (2, 12, 16, 150, 352, False),
                                                   (3, 7, 9, 36, 64, True), (2, 17, 70, 162, 176, False)])
def test_fused_conv3x3_backward_without_gf(B, H, W, c0, ld, compact, drop):
    """GF == NULL against GF given, same call otherwise: DZ, the f64 partials and dW2 bit for bit.  The three block geometries
    of the golden fixture (16-byte and, in block 3, 8-byte staging loads) and ragged tiles."""
    from emlight_amd import _lib as lib
    L, p, st = lib.lib(), lib.ptr, lib.current_stream()
    g = torch.Generator(device=DEV).manual_seed(B * H * W + c0)
    rnd = lambda *s, scale=1.0: torch.randn(*s, device=DEV, generator=g) * scale
    P = B * H * W
    Gd, Z, X, N12 = rnd(P, ld), rnd(P, 48), rnd(P, ld), rnd(P, 12)
    W2 = rnd(12, 48, 3, 3, scale=0.05)
    s2, t2 = torch.rand(48, device=DEV, generator=g) + 0.5, rnd(48, scale=0.3)
    zmean, zistd = rnd(48, scale=0.1), torch.rand(48, device=DEV, generator=g) + 0.5
    sB, sC = rnd(ld, scale=0.3), rnd(ld, scale=0.3)
    gsrc = (N12, 12, 0) if compact else (Gd, ld, c0)
    assert L.eml_dense_conv3x3_bwd_fused_supported(gsrc[1], gsrc[2], ld, c0) == 1
    fn = "eml_dense_conv3x3_bwd_fused_drop_f32" if drop else "eml_dense_conv3x3_bwd_fused_f32"
    tail = (0xC0FFEE, 5, 0.3) if drop else ()
    out = {}
    for gf in (True, False):
        DZ = torch.full((P, 48), 3.0, device=DEV)
        GF = torch.full((P, 12), 7.0, device=DEV)
        part = torch.full((G * 96,), 5.0, dtype=torch.float64, device=DEV)
        partW = torch.zeros(2 * G * 27 * 256, device=DEV)
        dW2 = torch.empty(12, 48, 3, 3, device=DEV)
        lib.check(getattr(L, fn)(p(gsrc[0]), gsrc[1], gsrc[2], p(W2), p(Z), p(zmean), p(zistd), p(DZ), B, H, W, p(part), G, p(X),
                                 ld, c0, p(sB), p(sC), p(GF) if gf else None, p(s2), p(t2), p(partW), p(dW2), *tail, st), fn)
        torch.cuda.synchronize()
        out[gf] = {"DZ": DZ, "partials": part, "dW2": dW2}
        if gf:
            assert not bool((GF == 7.0).any())
        else:
            assert bool((GF == 7.0).all())       # (nothing strays into the buffer that was not passed)
    _assert_equal(out[False], out[True], "fused conv3x3 backward without GF")


def test_a_whole_train_step_is_bit_identical_between_the_old_and_the_new_passes():
    new = _child("train_step", {"EML_TRANS_ONEPASS": "1", "EML_C3_GF": "0"})
    old = _child("train_step", {"EML_TRANS_ONEPASS": "0", "EML_C3_GF": "1"})
    assert any(k.startswith("grad/") for k in new) and any(k.startswith("state/") for k in new)
    _assert_equal(new, old, "train step")


if __name__ == "__main__":
    from emlight_amd import _runtime
    _runtime.entry_point_defaults()
    case, path = sys.argv[1:3]
    if case == "transitions":
        res = {"%d_%d_%d" % t: {k: v.cpu() for k, v in _transition_case(*t).items()} for t in TRANSITIONS}
    elif case == "train_step":
        res = {k: v.detach().cpu() for k, v in _train_step_case().items()}
    else:
        raise SystemExit("unknown case " + case)
    torch.save(res, path)
