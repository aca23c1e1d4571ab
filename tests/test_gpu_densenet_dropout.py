"""GPU: the DenseNet encoder's dropout (drop_rate > 0, DenseNet.py:50-55) in the conv3x3 kernels.

* eml_dense_dropout_mask_u16 equals the numpy restatement of the hash (tests/dropout_hash.py) bit for bit; keep fractions and
  cross-layer / cross-key correlations are those of independent Bernoulli draws.
* Against the reference's f64 run with the same masks (densenet_dropout.npz): outputs within 1e-4; dX within 4x the f32
  reference's own relative L2 error against f64 (the rule of test_gpu_densenet_input_grad.py); the stored parameter
  gradients are those of the masked f64 oracle restatement below, and the whole network's parameter gradients follow the rule
  of test_gpu_densenet.py::test_gradient_error_is_f32_conditioning (median and worst tensor within 3x of the f32 oracle's,
  + 5e-4) against it.
* Against that f64 restatement of the oracle, which multiplies in the same masks: crops that take the tap-packed forward
  (W = 256, 320: four wavefronts side by side) and crops that do not; EML_C3_FOLD 0/1, EML_WGRAD_OVERLAP 0/1.  dX: 4x the f32
  oracle's error + 5e-4 (the parameter rule's floor).  At these toy batches the f32 oracle's own error moves by an order of
  magnitude from one mask to the next at B = 2 (a ReLU tie in the head that one f32 summation order flips and another does
  not: 48x80 B=2 dX 7.1e-4 against an f32 oracle's 1.4e-4, 2.0e-3 for both at p = 0), so these crops run B = 1 and 3, where
  the engine and the f32 oracle both land within ~1e-6 of f64 (measured on the MI355X: 32x64 B=3 dX 1.0e-6 against 1.1e-6,
  parameter medians 1.3e-6 against 1.2e-6).
* Same key: bitwise equal results; the dropped elements of the block buffer are the hash's on both forward kernels; p = 1
  zeroes the new channels and conv2's gradient; eval mode with p > 0 is bitwise p = 0; a cfg2-size step is finite and
  deterministic."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle.densenet import _bn
from tests.dropout_hash import draws, keep_mask, mask_words, scaled_mask_nchw

pytestmark = pytest.mark.gpu
KEYS = ("distribution", "intensity", "rgb_ratio", "ambient")
RATIO = 4.0


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _device_mask(key, layer, p, P):
    from emlight_amd import _lib
    out = torch.empty(P, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().eml_dense_dropout_mask_u16(key, layer, p, P, _lib.ptr(out), _lib.current_stream()),
               "eml_dense_dropout_mask_u16")
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("key,layer,p", [(0, 0, 0.2), (0x9E3779B97F4A7C15, 47, 0.1), (2 ** 64 - 1, 17, 0.5),
                                         (123456789, 3, 0.0), (5, 30, 1.0), (77, 9, 0.999)])
def test_mask_entry_point_equals_numpy_hash(key, layer, p):
    P = 70001
    got = _device_mask(key, layer, p, P)
    assert np.array_equal(got, mask_words(key, layer, p, P))
    if p == 0:
        assert (got == 0xFFF).all()
    if p == 1:
        assert (got == 0).all()


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_keep_fraction_and_independence(p):
    P = 100000                                             # 1.2e6 draws per layer
    n = 12 * P
    keep = [np.unpackbits(_device_mask(k, l, p, P).view(np.uint8)).reshape(P, 16) for k, l in ((11, 0), (11, 1), (12, 0))]
    bits = [k[:, [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12]].astype(np.float64).ravel() for k in keep]   # the 12 channel bits
    frac = bits[0].mean()
    sigma = np.sqrt(p * (1 - p) / n)
    print("p=%.1f: keep fraction %.5f (expected %.5f, %.2f sigma)" % (p, frac, 1 - p, (frac - (1 - p)) / sigma))
    assert abs(frac - (1 - p)) <= 6 * sigma
    for other in bits[1:]:                                 # another layer, another key: uncorrelated
        r = np.corrcoef(bits[0], other)[0, 1]
        assert abs(r) <= 5 / np.sqrt(n), r
    # neighbouring channels of one pixel and neighbouring pixels of one channel: uncorrelated
    b = bits[0].reshape(P, 12)
    assert abs(np.corrcoef(b[:, :-1].ravel(), b[:, 1:].ravel())[0, 1]) <= 5 / np.sqrt(11 * P)
    assert abs(np.corrcoef(b[:-1].ravel(), b[1:].ravel())[0, 1]) <= 5 / np.sqrt(12 * (P - 1))


class _MaskedOracle(oracle.OracleDenseNet):
    """OracleDenseNet.features_forward with each dense layer's new channels multiplied by the hash's mask / (1 - p)."""
    key, p = 0, 0.0

    def features_forward(self, x):
        f, tr = self.features, self.training
        x = F.relu(_bn(F.conv2d(x, f.conv0.weight, padding=1), f.norm0, tr))
        gl = 0
        for b, n_layers in enumerate(self.block_config, 1):
            blk = getattr(f, "denseblock%d" % b)
            for l in range(n_layers):
                L = getattr(blk, "denselayer%d" % (l + 1))
                z = F.conv2d(F.relu(_bn(x, L.norm1, tr)), L.conv1.weight)
                new = F.conv2d(_bn(z, L.norm2, tr), L.conv2.weight, padding=1)
                B, _, H, W = new.shape
                new = new * torch.from_numpy(scaled_mask_nchw(self.key, gl, self.p, B, H, W)).to(new)
                gl += 1
                x = torch.cat([x, new], 1)
            T = getattr(f, "transition%d" % b)
            x = F.avg_pool2d(F.conv2d(F.relu(_bn(x, T.norm, tr)), T.conv.weight), 2, 2)
            x = _bn(x, getattr(f, "last_norm%d" % b), tr)
        return x


def _net(anchors, crop, sd, p, key):
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    net = DenseNet(anchors=anchors, crop_hw=crop, drop_rate=p).cuda().train()
    net.load_state_dict(sd)
    net.set_dropout_key(key)
    return net


def _run(model, x, w):
    """(outputs, dX, {name: grad}) of sum_k <model(x)[k], w[k]>."""
    for q in model.parameters():
        q.requires_grad_(True)
        q.grad = None
    x = x.detach().clone().requires_grad_(True)
    out = model(x)
    sum((out[k] * w[k].to(out[k])).sum() for k in KEYS).backward()
    return ({k: v.detach().double().cpu().numpy() for k, v in out.items()}, x.grad.double().cpu().numpy(),
            {n: q.grad.double().cpu().numpy() for n, q in model.named_parameters()})


def test_reference_fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densenet_dropout.npz"))
    B, _, H, W = (int(v) for v in z["shape"])
    key, p = int(z["key"]), float(z["p"])
    x = torch.from_numpy(np.random.default_rng(int(z["x_seed"])).random((B, 3, H, W), dtype=np.float32)).cuda()
    w = {k: torch.from_numpy(z["w_" + k]).cuda() for k in KEYS}
    ref = oracle.OracleDenseNet(anchors=int(z["anchors"]), crop_hw=(H, W))
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=int(z["weight_seed"]))
    net = _net(int(z["anchors"]), (H, W), sd, p, key)
    out, gx, gp = _run(net, x, w)
    # the f32 yardstick: the larger of the reference's own f32 error (CPU, stored) and the masked f32 oracle's on the GPU
    # (same weights, same masks), as in test_gpu_densenet_input_grad.py
    o32 = _MaskedOracle(anchors=int(z["anchors"]), crop_hw=(H, W))
    o32.load_state_dict(sd)
    o32.key, o32.p = key, p
    _, gx32, gp32 = _run(o32.cuda().train(), x, w)
    for k in KEYS:
        err = np.abs(out[k] - z["out_" + k]).max()
        print("output %s: max abs err %.3g" % (k, err))
        assert err <= 1e-4, k
    e, e32 = _rel(gx[0], z["grad_x0"]), max(float(z["grad_x0_ref_f32_rel_l2"]), _rel(gx32[0], z["grad_x0"]))
    print("dX rel-L2 %.3g (f32 yardstick %.3g)" % (e, e32))
    assert e <= RATIO * e32
    # the masked f64 oracle restatement IS the reference with the shimmed dropout ...
    o64 = _MaskedOracle(anchors=int(z["anchors"]), crop_hw=(H, W))
    o64.load_state_dict(sd)
    o64.key, o64.p = key, p
    _, _, gp64 = _run(o64.double().cuda().train(), x.double(), {k: v.double() for k, v in w.items()})
    for n in [k[len("grad/"):] for k in z.files if k.startswith("grad/")]:
        assert _rel(gp64[n], z["grad/" + n]) <= 1e-6, n
        print("%s: rel-L2 HIP %.3g, f32 oracle %.3g, reference f32 %.3g" % (n, _rel(gp[n], z["grad/" + n]),
                                                                         _rel(gp32[n], z["grad/" + n]),
                                                                         float(z["ref_f32_rel_l2/" + n])))
    norms = np.array([np.linalg.norm(gp64[n]) for n in z["param_names"]])
    assert np.allclose(norms, z["param_grad_l2"], rtol=1e-5, atol=1e-9 * z["param_grad_l2"].max())
    # ... and the HIP engine's parameter gradients against it: the worst tensor by the whole-network rule.  (Not the median: at
    # B = 2 one ReLU tie in the head flips between f32 summation orders -- last_norm3.bias, which only the head feeds, is 2.3e-3
    # from f64 here against the f32 oracle's 3e-7 -- and moves every upstream tensor by ~1e-2 together.)
    _param_rule(gp, gp64, gp32, "fixture", median=False)


def _oracle_pair(anchors, crop, sd, p, key, x, w):
    """f64 and f32 runs of the masked oracle on the GPU, same weights."""
    res = []
    for dt in (torch.float64, torch.float32):
        ref = _MaskedOracle(anchors=anchors, crop_hw=crop)
        ref.load_state_dict(sd)
        ref.key, ref.p = key, p
        ref = ref.to(dtype=dt).cuda().train()
        res.append(_run(ref, x.to(dt), {k: v.to(dt) for k, v in w.items()}))
    return res


def _param_rule(gp, gp64, gp32, tag, median=True):
    """test_gpu_densenet.py::test_gradient_error_is_f32_conditioning: per-tensor relative L2 against f64, median and worst
    tensor within 3x of the f32 oracle's (+ 5e-4); last_norm{1,2}.bias are analytically zero (they feed train-mode BNs)."""
    names = [n for n in gp if n not in ("features.last_norm1.bias", "features.last_norm2.bias")]
    e_hip = [_rel(gp[n], gp64[n]) for n in names]
    e_o32 = [_rel(gp32[n], gp64[n]) for n in names]
    print("%s: parameter rel-L2 vs f64: HIP median %.2e max %.2e | f32 oracle median %.2e max %.2e"
          % (tag, np.median(e_hip), max(e_hip), np.median(e_o32), max(e_o32)))
    assert not median or np.median(e_hip) <= 3.0 * np.median(e_o32) + 5e-4, tag
    assert max(e_hip) <= 3.0 * max(e_o32) + 5e-4, tag


def _check(got, o64, o32, tag):
    out, gx, gp = got
    for k in KEYS:
        assert np.abs(out[k] - o64[0][k]).max() <= 1e-4 + 4 * np.abs(o32[0][k] - o64[0][k]).max(), (tag, k)
    e, e32 = _rel(gx, o64[1]), _rel(o32[1], o64[1])
    print("%s: dX rel-L2 vs f64: HIP %.3g, f32 oracle %.3g" % (tag, e, e32))
    assert e <= RATIO * e32 + 5e-4, tag
    _param_rule(gp, o64[2], o32[2], tag)


@pytest.mark.parametrize("crop,B", [((32, 256), 3), ((32, 320), 1), ((32, 64), 3), ((48, 80), 3), ((64, 96), 3)])
@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("overlap", ["0", "1"])
def test_against_masked_f64_oracle(monkeypatch, crop, B, fold, overlap):
    monkeypatch.setenv("EML_C3_FOLD", fold)
    monkeypatch.setenv("EML_WGRAD_OVERLAP", overlap)
    ref = oracle.OracleDenseNet(anchors=32, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=21)
    key = 0xC0FFEE + B
    net = _net(32, crop, sd, 0.3, key)
    g = np.random.default_rng([31, B])
    x = torch.from_numpy(g.random((B, 3) + crop, dtype=np.float32)).cuda()
    w = {k: torch.from_numpy(g.standard_normal((B, n)).astype(np.float32)).cuda() for k, n in zip(KEYS, (32, 1, 3, 3))}
    got = _run(net, x, w)
    o64, o32 = _oracle_pair(32, crop, sd, 0.3, key, x, w)
    tp = net._hip.tap_packed_plan(B, *crop, x.device) is not None
    assert tp == (crop[1] in (256, 320))
    _check(got, o64, o32, "crop %s B=%d fold=%s overlap=%s tap-packed=%s" % (crop, B, fold, overlap, tp))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_same_key_is_bitwise_reproducible_and_no_grad_drops_alike():
    crop, B = (64, 96), 2
    ref = oracle.OracleDenseNet(anchors=32, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=22)
    net = _net(32, crop, sd, 0.2, 99)
    x = torch.rand(B, 3, *crop, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    w = {k: torch.randn(B, n, device="cuda") for k, n in zip(KEYS, (32, 1, 3, 3))}
    a, b = _run(net, x, w), _run(net, x, w)
    for k in KEYS:
        assert np.array_equal(_bits(a[0][k]), _bits(b[0][k]))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert all(np.array_equal(_bits(a[2][n]), _bits(b[2][n])) for n in a[2])
    with torch.no_grad():
        out = net(x)
    assert all(np.array_equal(_bits(out[k].double().cpu().numpy()), _bits(a[0][k])) for k in KEYS)
    net.set_dropout_key(100)
    c = _run(net, x, w)
    assert not np.array_equal(c[1], a[1])
    # the default: a fresh key per forward from torch's CPU generator, reproduced by torch.manual_seed
    net.set_dropout_key(None)
    torch.manual_seed(5)
    d = _run(net, x, w)
    torch.manual_seed(5)
    e = _run(net, x, w)
    assert np.array_equal(_bits(d[1]), _bits(e[1])) and not np.array_equal(d[1], _run(net, x, w)[1])


@pytest.mark.parametrize("tp", ["auto", "off"])
def test_dropped_positions_are_the_hash_on_both_forward_kernels(monkeypatch, tp):
    monkeypatch.setenv("EML_C3_TP", tp)
    crop, B, key, p = (32, 256), 2, 4242, 0.3
    ref = oracle.OracleDenseNet(anchors=32, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=23)
    net = _net(32, crop, sd, p, key)
    x = torch.rand(B, 3, *crop, device="cuda")
    with torch.no_grad():
        net(x)
    enc = net._hip
    (ws,) = [w_ for pool in enc._ws.values() for w_ in pool]
    assert (ws.blocks[0]["tp"] is not None) == (tp == "auto")
    gl = 0
    for blk in ws.blocks:
        X = blk["X"].cpu().numpy()
        for lay in blk["layers"]:
            new = X[:, lay["Cin"]:lay["Cin"] + 12]
            keep = keep_mask(key, gl, p, blk["P"])
            assert np.array_equal(new != 0, keep), (gl, tp)
            gl += 1


def test_p_one_zeroes_new_channels_and_conv2_gradients():
    crop, B = (64, 64), 2
    ref = oracle.OracleDenseNet(anchors=32, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=24)
    net = _net(32, crop, sd, 1.0, 3)
    x = torch.rand(B, 3, *crop, device="cuda")
    w = {k: torch.randn(B, n, device="cuda") for k, n in zip(KEYS, (32, 1, 3, 3))}
    out, gx, gp = _run(net, x, w)
    assert all(np.isfinite(v).all() for v in out.values()) and np.isfinite(gx).all()
    (ws,) = [w_ for pool in net._hip._ws.values() for w_ in pool]
    for blk in ws.blocks:
        X = blk["X"].cpu().numpy()
        assert not X[:, blk["C0"]:blk["Ctot"]].any()
    for n, g in gp.items():
        assert np.isfinite(g).all(), n
        if n.endswith("conv2.weight") or n.endswith("conv1.weight") or ".norm2." in n:
            assert not g.any(), n


def test_eval_mode_is_bitwise_the_zero_rate_forward():
    crop, B = (64, 96), 2
    ref = oracle.OracleDenseNet(anchors=32, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=25)
    sd = {k: (v + 0.1 * torch.rand_like(v).abs() if k.endswith("running_var") else v) for k, v in sd.items()}
    x = torch.rand(B, 3, *crop, device="cuda")
    outs = []
    for p in (0.0, 0.4):
        net = _net(32, crop, sd, p, 8).eval()
        with torch.no_grad():
            outs.append({k: v.double().cpu().numpy() for k, v in net(x).items()})
    assert all(np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])) for k in KEYS)


def test_cfg2_step():
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    B, crop = 64, (240, 320)
    torch.manual_seed(0)
    net = DenseNet(anchors=128, crop_hw=crop, drop_rate=0.2).cuda().train()
    net.set_dropout_key(2024)
    x = torch.rand(B, 3, *crop, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    w = {k: torch.randn(B, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
         for k, n in zip(KEYS, (128, 1, 3, 3))}
    res = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        net.zero_grad(set_to_none=True)
        out = net(x)
        sum((out[k] * w[k]).sum() for k in KEYS).backward()
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t, {k: v.detach().clone() for k, v in out.items()},
                    [q.grad.clone() for q in net.parameters()]))
    print("cfg2 encoder step with drop_rate 0.2: %.1f ms (second run)" % (1e3 * res[1][0]))
    for (_, o1, g1), (_, o2, g2) in [(res[0], res[1])]:
        assert all(torch.isfinite(o1[k]).all() and torch.equal(o1[k], o2[k]) for k in KEYS)
        assert all(torch.isfinite(a).all() and torch.equal(a, b) for a, b in zip(g1, g2))
