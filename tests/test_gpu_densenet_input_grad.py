"""GPU: the DenseNet encoder's gradient with respect to its input image (eml_dense_conv0_bwd_data_f32) against the reference's
f64 autograd (densenet_input_grad.npz) and the oracle's f64 autograd, on both norm0 paths; bitwise agreement between request
combinations (x and/or parameters, partial freezing); determinism; test-time optimisation of the input; eval mode; cfg2 size.

Accuracy rule (the rasteriser-gradient tests'): the relative L2 error of dX against f64 is at most 4x the f32 stock-op
oracle's own error against the same f64 gradient at the same shape and weights.  Measured on the MI355X (HIP error / f32 oracle
error): fixture 192x256 B=1 0.67 and 64x96 B=2 0.60 (against the larger of the GPU oracle's and the stored CPU reference's f32
error); oracle crops 32x32 B=3 0.96, 64x96 B=2 1.63, 96x160 B=1 1.13, identical on both norm0 paths.  Test-time optimisation:
largest loss gap 3.3e-3 against a 2.42 start."""
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
KEYS = ("distribution", "intensity", "rgb_ratio", "ambient")
RATIO = 4.0


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _nets(anchors, crop, seed):
    from emlight_amd.RegressionNetwork.DenseNet import DenseNet
    ref = oracle.OracleDenseNet(anchors=anchors, crop_hw=crop)
    sd = oracle.deterministic_state_dict(ref.state_dict(), seed=seed)
    ref.load_state_dict(sd)
    net = DenseNet(anchors=anchors, crop_hw=crop).cuda().train()
    net.load_state_dict(sd)
    return ref, net


def _cotangents(B, anchors, seed):
    g = np.random.default_rng(seed)
    return {k: g.standard_normal((B, n)).astype(np.float32) for k, n in zip(KEYS, (anchors, 1, 3, 3))}


def _input_grad(model, x, w, params=True):
    """d/dx sum_k <model(x)[k], w[k]>; params: whether the parameters ask for gradients too."""
    for q in model.parameters():
        q.requires_grad_(params)
        q.grad = None
    x = x.detach().clone().requires_grad_(True)
    out = model(x)
    sum((out[k] * w[k].to(out[k])).sum() for k in KEYS).backward()
    return x.grad


def _oracle_grads(ref, x, w):
    """(f64, f32) input gradients of the stock-op oracle on the GPU, same weights and running statistics."""
    ref32 = ref.cuda().train()
    state = {k: v.clone() for k, v in ref32.state_dict().items()}
    g32 = _input_grad(ref32, x.cuda(), w).double().cpu().numpy()
    ref64 = oracle.OracleDenseNet(anchors=ref.fc_dist.out_features, crop_hw=tuple(x.shape[2:])).double().cuda().train()
    ref64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in state.items()})
    g64 = _input_grad(ref64, x.double().cuda(), w).cpu().numpy()
    return g64, g32


@pytest.mark.parametrize("case", ["ref_b1_192x256", "cfg2_b2_64x96"])
def test_reference_fixture(case):
    """The reference DenseNet's own f64 input gradient (train mode, random cotangents on the four heads)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densenet_input_grad.npz"))
    p = case + "/"
    B, _, H, W = (int(v) for v in z[p + "shape"])
    anchors = int(z[p + "anchors"])
    x = torch.from_numpy(np.random.default_rng(int(z[p + "x_seed"])).random((B, 3, H, W), dtype=np.float32))
    w = {k: torch.from_numpy(z[p + "w_" + k]).cuda() for k in KEYS}
    ref, net = _nets(anchors, (H, W), int(z[p + "weight_seed"]))
    got = _input_grad(net, x.cuda(), w).double().cpu().numpy()
    want = z[p + "grad_x"]
    g32 = _input_grad(ref.cuda().train(), x.cuda(), w).double().cpu().numpy()
    e_hip, e_o32, e_ref32 = _rel(got, want), _rel(g32, want), float(z[p + "ref_f32_rel_l2"])
    print("%s: dX rel-L2 vs reference f64: HIP %.3g | f32 oracle %.3g | reference f32 (CPU) %.3g -> ratio %.2f"
          % (case, e_hip, e_o32, e_ref32, e_hip / max(e_o32, e_ref32)))
    assert np.isfinite(got).all()
    assert e_hip <= RATIO * max(e_o32, e_ref32)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("crop,B", [((32, 32), 3), ((64, 96), 2), ((96, 160), 1)])
def test_against_f64_oracle(monkeypatch, crop, B, fused):
    monkeypatch.setenv("EML_NORM0_FUSED", fused)
    ref, net = _nets(32, crop, seed=11)
    x = torch.from_numpy(np.random.default_rng([7, B]).random((B, 3) + crop, dtype=np.float32))
    w = {k: torch.from_numpy(v).cuda() for k, v in _cotangents(B, 32, [8, B]).items()}
    got = _input_grad(net, x.cuda(), w).double().cpu().numpy()
    g64, g32 = _oracle_grads(ref, x, w)
    e_hip, e_o32 = _rel(got, g64), _rel(g32, g64)
    print("crop %s B=%d norm0_fused=%s: dX rel-L2 vs f64: HIP %.3g, f32 oracle %.3g, ratio %.2f"
          % (crop, B, fused, e_hip, e_o32, e_hip / e_o32))
    assert e_hip <= RATIO * e_o32


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_request_combinations_are_bitwise_consistent():
    _, net = _nets(32, (64, 96), seed=12)
    B = 2
    x = torch.rand(B, 3, 64, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    w = {k: torch.from_numpy(v).cuda() for k, v in _cotangents(B, 32, 13).items()}
    params = list(net.parameters())

    def run(need_x, trainable):
        for q in params:
            q.requires_grad_(trainable(q))
            q.grad = None
        xx = x.clone().requires_grad_(need_x)
        out = net(xx)
        sum((out[k] * w[k]).sum() for k in KEYS).backward()
        return xx.grad, [None if q.grad is None else q.grad.clone() for q in params]

    dx_all, g_all = run(True, lambda q: True)
    dx_only, g_none = run(True, lambda q: False)
    dx_none, g_params = run(False, lambda q: True)
    assert dx_none is None and all(g is None for g in g_none)
    assert torch.equal(_bits(dx_all), _bits(dx_only))
    for a, b in zip(g_all, g_params):
        assert torch.equal(_bits(a), _bits(b))
    # partial freezing: conv0 / norm0 and the first dense block frozen, the rest trainable (heads included)
    frozen = set(id(q) for q in [net.features.conv0.weight, net.features.norm0.weight, net.features.norm0.bias]
                 + list(net.features.denseblock1.parameters()))
    dx_part, g_part = run(True, lambda q: id(q) not in frozen)
    assert torch.equal(_bits(dx_part), _bits(dx_all))
    for q, a, b in zip(params, g_all, g_part):
        if id(q) in frozen:
            assert b is None
        else:
            assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_deterministic(monkeypatch, fused):
    monkeypatch.setenv("EML_NORM0_FUSED", fused)
    _, net = _nets(32, (96, 160), seed=14)
    x = torch.rand(2, 3, 96, 160, device="cuda")
    w = {k: torch.from_numpy(v).cuda() for k, v in _cotangents(2, 32, 15).items()}
    a, b = _input_grad(net, x, w), _input_grad(net, x, w)
    assert torch.equal(_bits(a), _bits(b))


def test_test_time_optimisation_tracks_the_oracle():
    """Frozen weights, Adam on the input image toward a target intensity and light distribution.  The loss falls and the
    HIP loop's loss stays within 2 % of the initial loss of the same loop run on the f32 stock-op oracle."""
    crop, B, anchors, steps = (32, 64), 2, 16, 8
    ref, net = _nets(anchors, crop, seed=16)
    ref = ref.cuda().train()
    g = np.random.default_rng(17)
    x0 = torch.from_numpy(g.random((B, 3) + crop, dtype=np.float32)).cuda()
    t_int = torch.from_numpy(g.uniform(0.5, 1.5, (B, 1)).astype(np.float32)).cuda()
    t_dist = torch.from_numpy(g.standard_normal((B, anchors)).astype(np.float32)).cuda()

    def loop(model):
        for q in model.parameters():
            q.requires_grad_(False)
        x = x0.clone().requires_grad_(True)
        opt = torch.optim.Adam([x], lr=1e-2)
        losses = []
        for _ in range(steps):
            out = model(x)
            loss = (torch.nn.functional.mse_loss(out["intensity"], t_int)
                    + torch.nn.functional.mse_loss(out["distribution"], t_dist))
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return np.array(losses)

    l_hip, l_ref = loop(net), loop(ref)
    print("test-time optimisation losses: HIP", np.round(l_hip, 5), "oracle", np.round(l_ref, 5))
    assert l_hip[-1] < 0.9 * l_hip[0]
    assert np.abs(l_hip - l_ref).max() <= 0.02 * l_ref[0]


def test_eval_mode_is_refused():
    _, net = _nets(32, (32, 32), seed=18)
    net.eval()
    for q in net.parameters():
        q.requires_grad_(False)
    x = torch.rand(2, 3, 32, 32, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        sum(v.sum() for v in net(x).values()).backward()


def test_full_size_cfg2():
    """BASELINE cfg2: B=64, 240x320, 128 anchors.  dX finite with the right shape; parameter gradients bitwise equal with and
    without x; the extra peak memory of an x-only step over a parameters-only step is printed and bounded by dX plus slack."""
    B, crop = 64, (240, 320)
    _, net = _nets(128, crop, seed=2)
    x = torch.rand(B, 3, *crop, device="cuda", generator=torch.Generator(device="cuda").manual_seed(19))
    w = {k: torch.from_numpy(v).cuda() for k, v in _cotangents(B, 128, 20).items()}
    params = list(net.parameters())

    def run(need_x, need_params):
        for q in params:
            q.requires_grad_(need_params)
            q.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        xx = x.clone().requires_grad_(need_x)
        out = net(xx)
        sum((out[k] * w[k]).sum() for k in KEYS).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return xx.grad, [q.grad for q in params] if need_params else None, peak

    run(False, True)   # warm-up: the workspace and backward buffers of this shape
    _, g_p, peak_p = run(False, True)
    dx, g_px, peak_px = run(True, True)
    dx_o, _, peak_x = run(True, False)
    assert dx.shape == x.shape and bool(torch.isfinite(dx).all())
    assert torch.equal(_bits(dx), _bits(dx_o))
    for a, b in zip(g_p, g_px):
        assert torch.equal(_bits(a), _bits(b))
    mb = 2.0 ** 20
    print("cfg2 peak memory above the step's start: params %.1f MB, params+x %.1f MB, x only %.1f MB (dX %.1f MB)"
          % (peak_p / mb, peak_px / mb, peak_x / mb, dx.numel() * 4 / mb))
    assert peak_x <= peak_p + dx.numel() * 4 + 64 * mb
