"""GPU: one projector iteration (G step + D step) with the ground-truth Gaussian map produced by the HIP
rasteriser, and the batched GT map against the oracle's per-sample recipe (GenProjector/data.py:86-102)."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


def test_gaussian_map_batched_vs_oracle():
    from emlight_amd.GenProjector.data import gaussian_map
    from emlight_amd.RegressionNetwork.data import synthetic_batch
    B, ln = 3, 128
    p = synthetic_batch(B, ln, (32, 32), seed=5)
    inten, amb = p["intensity"] * 300.0, p["ambient"] * 128 * 256
    got = gaussian_map(p["distribution"].cuda(), inten.cuda(), p["rgb_ratio"].cuda(), amb.cuda(), ln=ln).cpu()
    dirs = torch.from_numpy(oracle.sphere_points(ln)).float().view(1, ln * 3)
    size = torch.full((1, ln), 0.0025)
    for b in range(B):  # the reference's per-item code path
        light = (p["distribution"][b].view(1, ln, 1).repeat(1, 1, 3) * (inten[b] * 0.01).view(1, 1, 1).repeat(1, ln, 3)
                 * p["rgb_ratio"][b].view(1, 1, 3).repeat(1, ln, 1)).view(1, ln * 3)
        want = oracle.convert_to_panorama(dirs, size, light).view(3, 128, 256) + (amb[b] / (128 * 256)).view(3, 1, 1)
        np.testing.assert_allclose(got[b].numpy(), want.numpy(), rtol=1e-4, atol=1e-4 * float(want.max()))


def test_projector_iteration_on_gpu():
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.model_trainer import Trainer
    torch.manual_seed(0)
    tr = Trainer(networks.default_options(ngf=4, ndf=4), device="cuda")
    batch = data.projector_batch(2, "cuda", seed=3)
    assert batch["input"].shape == (2, 3, 128, 256) and batch["map"].shape == (2, 1, 128, 256)
    tr.step(batch)
    losses = tr.get_latest_losses()
    assert set(losses) == {"GAN", "GAN_Feat", "COS", "D_Fake", "D_real"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert tr.generated.shape == (2, 3, 128, 256)


# ------------------------------------------------------------------------------------------ SphereConv2D (HIP)
@pytest.mark.parametrize("B,Cin,Cout,H,W,stride,bias", [(2, 16, 8, 8, 16, 1, True), (3, 6, 12, 16, 32, 2, True),
                                                        (1, 3, 8, 4, 8, 1, False), (2, 128, 64, 32, 64, 1, True),
                                                        (0, 8, 8, 8, 16, 1, True)])
def test_sphere_conv_hip_vs_stock_ops(B, Cin, Cout, H, W, stride, bias):
    """im2col_sphere + GEMM + col2im_sphere against grid_sample + conv2d(stride 3) (sphere_cnn.py:121-124) in torch
    f32 on the same GPU: output, d/dx, d/dweight, d/dbias."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    torch.manual_seed(B * 100 + Cin)
    ref = SphereConv2D(Cin, Cout, stride=stride, bias=bias).cuda()   # parameters only; run through the oracle's ops
    hip = SphereConv2D(Cin, Cout, stride=stride, bias=bias).cuda()
    hip.load_state_dict(ref.state_dict())
    if bias:
        with torch.no_grad():
            ref.bias.uniform_(-0.5, 0.5)
            hip.bias.copy_(ref.bias)
    x = torch.randn(B, Cin, H, W, device="cuda")
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr, yh = oracle.sphere_conv(xr, ref.weight, ref.bias, stride), hip(xh)
    assert yh.shape == yr.shape == (B, Cout, H // stride, W // stride)
    if B == 0:
        return
    scale = float(yr.detach().abs().max())
    np.testing.assert_allclose(yh.detach().cpu().numpy(), yr.detach().cpu().numpy(), rtol=1e-4, atol=2e-5 * scale)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    yh.backward(gy)
    for name, a, b in [("dx", xh.grad, xr.grad), ("dW", hip.weight.grad, ref.weight.grad)] + \
            ([("db", hip.bias.grad, ref.bias.grad)] if bias else []):
        s = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=3e-5 * s, err_msg=name)


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride,bias", [(2, 32, 64, 8, 16, 1, True), (2, 64, 128, 16, 32, 1, True),
                                                        (3, 128, 64, 16, 32, 2, False), (1, 64, 192, 6, 10, 1, True),
                                                        (2, 256, 256, 8, 16, 1, True), (1, 96, 64, 12, 20, 1, True),
                                                        (1, 64, 64, 64, 128, 1, True), (2, 128, 64, 32, 64, 1, False)])
def test_sphere_conv_fused_kernels_vs_stock_ops(B, Cin, Cout, H, W, stride, bias, monkeypatch):
    """The fused implicit-GEMM kernels (taps gathered straight into the MFMA operand tile: forward, and the weight
    gradient where Cin % 64 == 0) against grid_sample + conv2d(stride 3) in torch f32 on the same GPU; pixel counts that
    are not a multiple of the 128-pixel tile, 64- and 128-wide channel tiles, strided geometry."""
    from emlight_amd.GenProjector import spherenet
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    monkeypatch.setattr(SphereConv2D, "fused_min_bytes", 0)   # every layer counts as large
    torch.manual_seed(B * 100 + Cin)
    ref = SphereConv2D(Cin, Cout, stride=stride, bias=bias).cuda()
    hip = SphereConv2D(Cin, Cout, stride=stride, bias=bias).cuda()
    hip.load_state_dict(ref.state_dict())
    if bias:
        with torch.no_grad():
            ref.bias.uniform_(-0.5, 0.5)
            hip.bias.copy_(ref.bias)
    x = torch.randn(B, Cin, H, W, device="cuda")
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = oracle.sphere_conv(xr, ref.weight, ref.bias, stride)
    from emlight_amd import _lib
    real = _lib.lib()
    seen = set()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                seen.add(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    yh = hip(xh)
    assert yh.shape == yr.shape == (B, Cout, H // stride, W // stride)
    scale = float(yr.detach().abs().max())
    np.testing.assert_allclose(yh.detach().cpu().numpy(), yr.detach().cpu().numpy(), rtol=1e-4, atol=2e-5 * scale)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    yh.backward(gy)
    assert "eml_sphere_conv_fwd_fused_ex_f32" in seen
    # the fused input gradient: stride-1 layers with Cout % 32 == 0 and Cin % 64 == 0 (else dY W2 + col2im)
    assert ("eml_sphere_conv_dgrad_fused_f32" in seen) == (stride == 1 and Cin % 64 == 0)
    assert ("eml_sphere_col2im_f32" in seen) != ("eml_sphere_conv_dgrad_fused_f32" in seen)
    assert ("eml_sphere_conv_wgrad_fused_f32" in seen) == (Cin % 64 == 0)
    assert ("eml_sphere_im2col_f32" in seen) == (Cin % 64 != 0)   # A9 is rebuilt only where the fused wgrad does not tile
    for name, a, b in [("dx", xh.grad, xr.grad), ("dW", hip.weight.grad, ref.weight.grad)] + \
            ([("db", hip.bias.grad, ref.bias.grad)] if bias else []):
        s_ = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=3e-5 * s_, err_msg=name)
    # bitwise run-to-run (split-K partials are summed in a fixed order)
    xh2 = x.clone().requires_grad_(True)
    gw1 = hip.weight.grad.clone()
    hip.zero_grad()
    y2 = hip(xh2)
    y2.backward(gy)
    assert torch.equal(y2, yh) and torch.equal(xh2.grad, xh.grad) and torch.equal(hip.weight.grad, gw1)


@pytest.mark.parametrize("B,Cin,Cout,H,W,bias,with_res,slope", [
    (2, 128, 128, 8, 16, True, False, 1.0),     # one tile per sample, footprint = the sample; split-K (few tiles)
    (3, 128, 256, 16, 32, True, True, 0.2),     # four tiles per sample, row-range footprints; residual + LeakyReLU epilogue
    (2, 64, 256, 32, 64, False, False, 1.0),    # 448-pixel footprints: the 512-thread variant (forward; C = 64: dX the old way)
    (5, 128, 128, 4, 8, True, False, 0.0),      # 32 pixels per sample: a tile spans four samples, the last tile one; ReLU
    (1, 96, 384, 16, 32, True, False, 1.0),     # three channel chunks, three 128-wide output tiles
    (2, 256, 256, 32, 64, True, False, 1.0),    # the 512-thread variant both ways
    (33, 32, 128, 8, 16, True, True, 1.0),      # more tiles than one round of workgroups
])
def test_sphere_conv_lowres_footprint_kernel_vs_stock_ops(B, Cin, Cout, H, W, bias, with_res, slope, monkeypatch):
    """Round 6, ``csrc/gather_gemm3.h`` (``eml_sphere_conv_lowres_f32``): the low-resolution wide layers with the source footprint
    in LDS -- forward (with the residual / activation epilogue) and the input gradient over the transposed table -- against
    grid_sample + conv2d(stride 3) (sphere_cnn.py:111-124) in torch f32 on the same GPU; neither sphere_im2col nor
    sphere_col2im may run for them; run-to-run bit equality (split-K partials are summed in a fixed order)."""
    from emlight_amd import _lib
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    monkeypatch.setattr(SphereConv2D, "lowres", "force")
    torch.manual_seed(B * 100 + Cin)
    hip = SphereConv2D(Cin, Cout, stride=1, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            hip.bias.uniform_(-0.5, 0.5)
    x = torch.randn(B, Cin, H, W, device="cuda")
    rs = torch.randn(B, Cout, H, W, device="cuda") if with_res else None
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wr = hip.weight.detach().clone().requires_grad_(True)
    br = hip.bias.detach().clone().requires_grad_(True) if bias else None
    rr, rh = (rs.clone().requires_grad_(True), rs.clone().requires_grad_(True)) if with_res else (None, None)
    yr = oracle.sphere_conv(xr, wr, br, 1)
    if with_res:
        yr = yr + rr
    if slope != 1.0:
        yr = torch.nn.functional.leaky_relu(yr, slope)
    real, seen = _lib.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                seen.append(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    yh = hip(xh, residual=rh, act_slope=slope)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    yh.backward(gy)
    # forward always; the input gradient (the same product over the transposed table: C and O swap roles) where C % 128 == 0
    assert seen.count("eml_sphere_conv_lowres_f32") == 1 + int(Cin % 128 == 0), seen
    assert "eml_sphere_conv_fwd_fused_ex_f32" not in seen and "eml_sphere_im2col_f32" not in seen[:seen.index("eml_sphere_conv_lowres_f32") + 1], seen
    scale = float(yr.detach().abs().max())
    np.testing.assert_allclose(yh.detach().cpu().numpy(), yr.detach().cpu().numpy(), rtol=1e-4, atol=3e-5 * scale)
    pairs = [("dx", xh.grad, xr.grad), ("dW", hip.weight.grad, wr.grad)] + ([("db", hip.bias.grad, br.grad)] if bias else []) + \
        ([("dres", rh.grad, rr.grad)] if with_res else [])
    for name, a, b in pairs:
        s_ = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=3e-5 * s_, err_msg=name)
    xh2 = x.clone().requires_grad_(True)
    y2 = hip(xh2, residual=rs, act_slope=slope)
    y2.backward(gy)
    assert torch.equal(y2, yh) and torch.equal(xh2.grad, xh.grad)


# Every distinct SphereConv geometry (B, Cin, Cout, H, W, stride) of the ngf = ndf = 64 projector at BASELINE configs[2]
# (B = 32; the discriminator sees fake + real = 64): the SPADE blocks' convs and their (gamma | beta) heads (one conv over the
# concatenated outputs), the 3 -> 128 guide-map convs at every resolution, the output layer, both PatchGAN scales.
# test_ngf64_shape_list_is_what_the_networks_run holds this list to the shapes the modules really call.
NGF64_SHAPES = [
    # generator: head_0 @ 4x8, G_middle_* @ 8x16
    (32, 3, 128, 4, 8, 1), (32, 128, 2048, 4, 8, 1), (32, 1024, 1024, 4, 8, 1),
    (32, 3, 128, 8, 16, 1), (32, 128, 2048, 8, 16, 1), (32, 1024, 1024, 8, 16, 1),
    # up_0 (1024 -> 512) @ 16x32
    (32, 3, 128, 16, 32, 1), (32, 128, 2048, 16, 32, 1), (32, 128, 1024, 16, 32, 1), (32, 1024, 512, 16, 32, 1),
    (32, 512, 512, 16, 32, 1),
    # up_1 (512 -> 256) @ 32x64
    (32, 3, 128, 32, 64, 1), (32, 128, 1024, 32, 64, 1), (32, 128, 512, 32, 64, 1), (32, 512, 256, 32, 64, 1),
    (32, 256, 256, 32, 64, 1),
    # up_2 (256 -> 128) @ 64x128
    (32, 3, 128, 64, 128, 1), (32, 128, 512, 64, 128, 1), (32, 128, 256, 64, 128, 1), (32, 256, 128, 64, 128, 1),
    (32, 128, 128, 64, 128, 1),
    # up_3 (128 -> 64) and the output layer @ 128x256
    (32, 3, 128, 128, 256, 1), (32, 128, 256, 128, 256, 1), (32, 128, 128, 128, 256, 1), (32, 128, 64, 128, 256, 1),
    (32, 64, 64, 128, 256, 1), (32, 64, 3, 128, 256, 1),
    # discriminator, scale 1 (128x256 input) and scale 2 (64x128)
    (64, 6, 64, 128, 256, 2), (64, 64, 128, 64, 128, 2), (64, 128, 256, 32, 64, 2), (64, 256, 512, 16, 32, 1),
    (64, 512, 3, 16, 32, 1),
    (64, 6, 64, 64, 128, 2), (64, 64, 128, 32, 64, 2), (64, 128, 256, 16, 32, 2), (64, 256, 512, 8, 16, 1),
    (64, 512, 3, 8, 16, 1),
]


def test_ngf64_shape_list_is_what_the_networks_run(monkeypatch):
    from emlight_amd.GenProjector import networks, spherenet
    from emlight_amd.GenProjector.data import projector_batch
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    seen = set()
    real = spherenet.sphere_conv

    def spy(x, weight, bias, stride=1, *more):
        seen.add((x.shape[0], x.shape[1], weight.shape[0], x.shape[2], x.shape[3], stride))
        return real(x, weight, bias, stride, *more)
    monkeypatch.setattr(spherenet, "sphere_conv", spy)
    real_spade = spherenet.spade_conv_modulate

    def spy_spade(x, actv, wg, *more):   # the gamma | beta SphereConvs that run with SPADE's modulation as their epilogue
        seen.add((actv.shape[0], actv.shape[1], 2 * wg.shape[0], actv.shape[2], actv.shape[3], 1))   # the two heads: O = 2 Cn
        return real_spade(x, actv, wg, *more)
    monkeypatch.setattr(spherenet, "spade_conv_modulate", spy_spade)
    torch.manual_seed(0)
    pm = Pix2PixModel(networks.default_options()).cuda()
    with torch.no_grad():
        pm(projector_batch(32, "cuda", seed=1), mode="generator")
    assert seen == set(NGF64_SHAPES), (sorted(seen - set(NGF64_SHAPES)), sorted(set(NGF64_SHAPES) - seen))


def _plan_entry_points(plan, Cin):
    """The SphereConv entry points a forward + backward under ``plan`` calls, with every gradient wanted, on a geometry that has
    a transposed tap table (all but the tiniest) and the default ``narrow_project``."""
    fwd = {"narrow": "conv_narrow_fwd2", "small": "conv_small_fwd", "fused": "conv_fwd_fused_ex", "library": "im2col"}[plan.fwd]
    dgrad = {"narrow": ["conv_narrow_dgrad2" if Cin <= 128 else "conv_narrow_dgrad"], "small": ["conv_small_da9", "col2im"],
             "fused": ["conv_dgrad_fused"], "library": ["col2im"]}[plan.dgrad]
    wgrad = {"narrow": "conv_narrow_wgrad2", "small": "conv_small_wgrad", "fused": "conv_wgrad_fused",
             "library": "im2col"}[plan.wgrad]     # (the library weight gradient: on the kept operand, or on a rebuilt one)
    assert plan.keep == (plan.fwd == "library" and plan.wgrad == "library")
    return {"eml_sphere_%s_f32" % n for n in [fwd, wgrad] + dgrad}


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", NGF64_SHAPES)
def test_sphere_conv_ngf64_layer_shapes_natural_dispatch(B, Cin, Cout, H, W, stride, monkeypatch):
    """The projector at its REAL size never met the oracle layer by layer: the reference golden is ngf = 8, and the per-shape
    dispatch rules (fused gather-GEMM kernels vs im2col + library GEMM, ``spherenet._conv_plan``) pick different kernels
    at ngf = 64.  Every distinct layer geometry of NGF64_SHAPES, at BASELINE's batch, with the dispatch left alone:
    output, d/dx, d/dweight, d/dbias against grid_sample + conv2d(stride 3) (sphere_cnn.py:111-124) in torch f32.
    Bounds: f32 sums over K = 9*Cin (forward), 9*Cout (d/dx), B*H'*W' (d/dweight) terms in two different orders agree to
    ~sqrt(K) * 6e-8 of the sum's scale -- 1e-4 relative + 1e-4 of the tensor's largest entry covers K up to 1e6.
    The convolution's entry points that ran are exactly those of the layer's plan (``_conv_plan``, pinned per shape on the CPU by
    tests/test_sphere_conv_plan.py)."""
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    torch.manual_seed(Cin * 7 + Cout + H)
    hip = SphereConv2D(Cin, Cout, stride=stride, bias=True).cuda()
    with torch.no_grad():
        hip.bias.uniform_(-0.5, 0.5)
    x = torch.randn(B, Cin, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wr, br = hip.weight.detach().clone().requires_grad_(True), hip.bias.detach().clone().requires_grad_(True)
    real, seen = _lib.lib(), set()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                seen.add(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    yh = hip(xh)
    gy = torch.randn_like(yh)
    yh.backward(gy)
    monkeypatch.undo()
    # The stock ops run in batch chunks (samples are independent; parameter gradients accumulate over the chunks): at
    # B = 32, C = 128, 128x256 the grid_sample output is 4.83 GB and ATen / MIOpen on ROCm address it with 32-bit byte
    # offsets -- measured on the MI355X: exactly the elements past 2^32 bytes (the last 11.1 % of the batch) come out
    # wrong in the STOCK forward.  The HIP kernels index with 64-bit pixel offsets and take the whole batch at once.
    per_sample = Cin * 9 * (H // stride) * (W // stride) * 4
    bs = max(1, min(B, (1 << 30) // per_sample))
    ys = []
    for i in range(0, B, bs):
        yc = oracle.sphere_conv(xr[i:i + bs], wr, br, stride)
        yc.backward(gy[i:i + bs])
        ys.append(yc.detach())
    yr = torch.cat(ys, 0)
    assert yh.shape == yr.shape == (B, Cout, H // stride, W // stride)
    print("dispatch", (B, Cin, Cout, H, W, stride), sorted(n.replace("eml_sphere_", "") for n in seen))
    # the convolution's own entry points are exactly the ones the layer's plan names (tests/test_sphere_conv_plan.py pins the plan)
    plan = spherenet._conv_plan("sphere", stride, B, Cin, Cout, H, W, False, 1.0, spherenet._Needs(True, True, True, False),
                                bool(real.eml_sphere_conv_small_supported(Cin, Cout)),
                                bool(real.eml_sphere_conv_narrow_supported(Cin, Cout)))
    ran = {n for n in seen if n.startswith("eml_sphere_") and not n.endswith(("_supported", "_floats", "tap_table_f32"))}
    assert ran == _plan_entry_points(plan, Cin), (plan, sorted(ran))
    for name, a, b in [("y", yh.detach(), yr.detach()), ("dx", xh.grad, xr.grad), ("dW", hip.weight.grad, wr.grad),
                       ("db", hip.bias.grad, br.grad)]:
        s_ = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4 * s_, err_msg=name)


def test_sphere_conv_hip_is_deterministic_and_has_no_cpu_path():
    from emlight_amd import _lib
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    m = SphereConv2D(8, 8).cuda()
    x = torch.randn(2, 8, 16, 32, device="cuda", requires_grad=True)
    g1 = torch.autograd.grad(m(x).square().sum(), x)[0]
    g2 = torch.autograd.grad(m(x).square().sum(), x)[0]
    assert torch.equal(g1, g2)  # gather backward: no atomics (grid_sampler_2d_backward is not run-to-run exact)
    with pytest.raises(_lib.EmlightHipError):
        SphereConv2D(8, 8)(torch.randn(1, 8, 16, 32))


@pytest.mark.parametrize("force_fused", [False, True])
def test_projector_matches_reference_golden_on_hip_sphereconv(force_fused, monkeypatch):
    """The golden vectors of the REAL reference networks (ngf = ndf = 8, tests/golden/projector.npz) through the
    HIP SphereConv2D path: generator output, losses, parameter-gradient samples, discriminator losses.  force_fused:
    every layer whose channel counts tile takes the fused gather-GEMM kernels (forward, weight and input gradient), which
    at this width would otherwise only serve the large layers."""
    from tests.conftest import Golden
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    if force_fused:
        monkeypatch.setattr(SphereConv2D, "fused_min_bytes", 0)
    from tests.golden.make_golden import projector_inputs
    from emlight_amd.GenProjector import networks
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    g = Golden("projector")
    m = Pix2PixModel(networks.default_options(ngf=8, ndf=8))
    m.netG.load_state_dict(oracle.deterministic_projector_state_dict(m.netG.state_dict(), seed=11))
    m.netD.load_state_dict(oracle.deterministic_projector_state_dict(m.netD.state_dict(), seed=12))
    m = m.cuda().train()
    inp, crop, warped, mask = (torch.from_numpy(a).cuda() for a in projector_inputs(2, 21))
    data = {"input": inp, "crop": crop, "warped": warped, "map": mask}
    losses, fake = m(data, "generator")
    fk = fake.detach().cpu()
    np.testing.assert_allclose(fk.reshape(-1)[torch.from_numpy(g["fake_idx"])].numpy(), g["fake_sample"], rtol=1e-4, atol=5e-4)
    assert abs(float(fk.double().mean()) - float(g["fake_mean"])) < 2e-4
    for k in ("GAN", "GAN_Feat", "COS"):
        np.testing.assert_allclose(float(losses[k].detach().mean()), float(g["g_loss/" + k]), rtol=5e-4, atol=2e-5)
    sum(v.mean() for v in losses.values()).backward()
    named = dict(m.netG.named_parameters())
    for key in [k[len("g_grad/"):] for k in g.z.files if k.startswith("g_grad/")]:
        got = named[key].grad.reshape(-1).cpu()[torch.from_numpy(g["g_grad_idx/" + key])].numpy()
        l2 = float(g["g_grad_l2/" + key])
        np.testing.assert_allclose(got, g["g_grad/" + key], rtol=5e-3, atol=5e-4 * l2 / np.sqrt(named[key].numel()) + 1e-8,
                                   err_msg=key)
    m2 = Pix2PixModel(networks.default_options(ngf=8, ndf=8))
    m2.netG.load_state_dict(oracle.deterministic_projector_state_dict(m2.netG.state_dict(), seed=11))
    m2.netD.load_state_dict(oracle.deterministic_projector_state_dict(m2.netD.state_dict(), seed=12))
    d = m2.cuda().train()(data, "discriminator")
    for k in ("D_Fake", "D_real"):
        np.testing.assert_allclose(float(d[k].detach()), float(g["d_loss/" + k]), rtol=5e-4, atol=2e-5)


@pytest.mark.parametrize("mode", [True, False])
@pytest.mark.parametrize("slope,B,C,H,W", [(1.0, 2, 16, 8, 16), (0.2, 2, 16, 8, 16), (0.2, 3, 1024, 4, 8), (0.2, 1, 64, 32, 64),
                                           (1.0, 2, 1280, 2, 4)])
def test_spade_norm_modulate_hip_vs_stock_ops(slope, B, C, H, W, mode):
    """Parameter-free BatchNorm (train: batch statistics + running update; eval: running statistics) folded into the
    fused gamma|beta SphereConv + modulation (+ LeakyReLU), against normalization.py:101-115 / architecture.py:56-57
    written with stock ops: output, running statistics, and the gradients w.r.t. x (through the statistics), actv and
    the four head parameters."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D, spade_norm_modulate
    torch.manual_seed(3)
    nh = 12
    bn_ref, bn_hip = torch.nn.BatchNorm2d(C, affine=False).cuda().train(mode), torch.nn.BatchNorm2d(C, affine=False).cuda().train(mode)
    with torch.no_grad():
        for bn in (bn_ref, bn_hip):
            bn.running_mean.copy_(torch.linspace(-0.2, 0.3, C))
            bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
    ref_g, ref_b = SphereConv2D(nh, C).cuda(), SphereConv2D(nh, C).cuda()   # parameter holders for the oracle's ops
    hip_g, hip_b = SphereConv2D(nh, C).cuda(), SphereConv2D(nh, C).cuda()
    for m in (ref_g, ref_b):
        with torch.no_grad():
            m.bias.uniform_(-0.3, 0.3)
    hip_g.load_state_dict(ref_g.state_dict())
    hip_b.load_state_dict(ref_b.state_dict())
    xn0, a0 = torch.randn(B, C, H, W, device="cuda") * 1.7 + 0.4, torch.randn(B, nh, H, W, device="cuda")
    outs = []
    for fn, bn, g_, b_ in ((oracle.spade_norm_modulate, bn_ref, ref_g, ref_b), (spade_norm_modulate, bn_hip, hip_g, hip_b)):
        xn, actv = xn0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        y = fn(xn, bn, actv, g_, b_, slope)
        (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
        outs.append([y.detach(), xn.grad, actv.grad, g_.weight.grad, g_.bias.grad, b_.weight.grad, b_.bias.grad])
    for name, r, h in zip(["y", "d_x", "d_actv", "dWg", "dbg", "dWb", "dbb"], outs[0], outs[1]):
        s = float(r.abs().max())
        np.testing.assert_allclose(h.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, atol=3e-5 * s, err_msg=name)
    np.testing.assert_allclose(bn_hip.running_mean.cpu().numpy(), bn_ref.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn_hip.running_var.cpu().numpy(), bn_ref.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert int(bn_hip.num_batches_tracked) == int(bn_ref.num_batches_tracked)


@pytest.mark.parametrize("project", [True, False])
@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", [(2, 64, 3, 16, 32, 1), (3, 128, 1, 10, 20, 1), (2, 512, 3, 8, 16, 1),
                                                    (1, 64, 4, 6, 12, 1), (2, 192, 2, 12, 24, 2), (1, 64, 3, 2, 4, 1),
                                                    (5, 64, 3, 9, 19, 1)])
def test_sphere_conv_few_output_channels_one_pass_kernels(B, Cin, Cout, H, W, stride, project, monkeypatch):
    """conv_img 64 -> 3 and the discriminators' final convolutions (csrc/sphere_conv_narrow.hip: forward, input gradient by the
    transposed tap table, weight gradient) against grid_sample + conv2d(stride 3) (sphere_cnn.py:111-124): pixel counts that do
    not fill a workgroup, several 64-channel groups, stride 2, and a geometry so small that a (pixel, tap) has more than 8
    sources (the input gradient then falls back to dA9 + col2im)."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    torch.manual_seed(Cin + Cout)
    # project = the round-6 form (csrc/sphere_conv_narrow2.hip: a (pixels, 36) projection, then 16-byte gathers; the weight
    # gradient through the transposed table) -- False: the one-pass kernels, which stay behind EML_NARROW_PROJECT=0
    monkeypatch.setattr(SphereConv2D, "narrow_project", project)
    hip = SphereConv2D(Cin, Cout, stride=stride, bias=True).cuda()
    with torch.no_grad():
        hip.bias.uniform_(-0.5, 0.5)
    x = torch.randn(B, Cin, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wr, br = hip.weight.detach().clone().requires_grad_(True), hip.bias.detach().clone().requires_grad_(True)
    seen = _spy_on_lib(monkeypatch)
    yh = hip(xh)
    yr = oracle.sphere_conv(xr, wr, br, stride)
    gy = torch.randn_like(yr)
    yh.backward(gy)
    yr.backward(gy)
    if project:
        assert "eml_sphere_conv_narrow_fwd2_f32" in seen and "eml_sphere_conv_narrow_fwd_f32" not in seen
        # (the 2 x 4 geometry has a (pixel, tap) with more than 8 sources: no transposed table, the one-pass weight gradient)
        assert ("eml_sphere_conv_narrow_wgrad2_f32" in seen) != ("eml_sphere_conv_narrow_wgrad_f32" in seen)
        narrow_dgrad = "eml_sphere_conv_narrow_dgrad2_f32" if Cin <= 128 else "eml_sphere_conv_narrow_dgrad_f32"   # (wide heads: one pass)
        assert ("eml_sphere_conv_narrow_wgrad2_f32" in seen) == (narrow_dgrad in seen)
        assert (narrow_dgrad in seen) != ("eml_sphere_col2im_f32" in seen)
    else:
        assert "eml_sphere_conv_narrow_fwd_f32" in seen and "eml_sphere_conv_narrow_wgrad_f32" in seen
        assert ("eml_sphere_conv_narrow_dgrad_f32" in seen) != ("eml_sphere_col2im_f32" in seen)
    assert "eml_sphere_im2col_f32" not in seen
    for name, h, r in (("y", yh, yr), ("dx", xh.grad, xr.grad), ("dW", hip.weight.grad, wr.grad), ("db", hip.bias.grad, br.grad)):
        np.testing.assert_allclose(h.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-4,
                                   atol=1e-4 * float(r.detach().abs().max()), err_msg=name)
    # run-to-run exact (fixed-order sums, no atomics)
    hip.zero_grad(set_to_none=True)
    x2 = x.clone().requires_grad_(True)
    y2 = hip(x2)
    y2.backward(gy)
    assert torch.equal(y2, yh) and torch.equal(x2.grad, xh.grad)
    # the input gradient on its own (frozen weights: the discriminators in the generator step) builds its own V: same values
    x3 = x.clone().requires_grad_(True)
    (gx3,) = torch.autograd.grad(hip(x3), x3, gy)
    assert torch.equal(gx3, xh.grad)


def _spy_on_lib(monkeypatch):
    """Route every C-ABI call through a recorder; returns the list of entry-point names in call order."""
    from emlight_amd import _lib
    real, seen = _lib.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                seen.append(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    return seen


@pytest.mark.parametrize("mode", [True, False])
@pytest.mark.parametrize("slope,B,C,nh,H,W,up2", [(0.2, 2, 64, 128, 16, 32, False), (1.0, 1, 128, 128, 8, 16, False),
                                                   (0.2, 2, 128, 64, 12, 24, True), (0.0, 3, 256, 128, 6, 12, True),
                                                   (0.2, 1, 64, 96, 10, 20, False)])
def test_spade_in_one_launch_vs_two_launches_and_stock_ops(slope, B, C, nh, H, W, up2, mode, monkeypatch):
    """The gamma | beta SphereConv with SPADE's modulation as its epilogue (eml_sphere_conv_spade_fwd_f32: the (B, 2C, H, W)
    tensor never exists; backward from gamma and the output's sign) against (a) the two-launch HIP path -- same conv kernel,
    same arithmetic: 1e-6 -- and (b) normalization.py:101-115 / architecture.py:56-57 on stock ops, incl. the folded nearest
    x2 upsample (generator.py:70-82), partial pixel tiles (B*H*W not a multiple of 128) and eval-mode statistics."""
    from emlight_amd.GenProjector import spherenet
    from emlight_amd.GenProjector.spherenet import SphereConv2D, spade_norm_modulate
    torch.manual_seed(5)
    monkeypatch.setattr(SphereConv2D, "fused_min_bytes", 0)       # every layer on the fused kernels, whatever its size
    seen = _spy_on_lib(monkeypatch)
    bns = [torch.nn.BatchNorm2d(C, affine=False).cuda().train(mode) for _ in range(3)]
    with torch.no_grad():
        for bn in bns:
            bn.running_mean.copy_(torch.linspace(-0.2, 0.3, C))
            bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
    heads = [(SphereConv2D(nh, C).cuda(), SphereConv2D(nh, C).cuda()) for _ in range(3)]
    with torch.no_grad():
        for m in heads[0]:
            m.bias.uniform_(-0.3, 0.3)
    for g_, b_ in heads[1:]:
        g_.load_state_dict(heads[0][0].state_dict())
        b_.load_state_dict(heads[0][1].state_dict())
    hx, wx = (H // 2, W // 2) if up2 else (H, W)
    xn0 = (torch.randn(B, C, hx, wx, device="cuda") * 1.7 + 0.4).contiguous(memory_format=torch.channels_last)
    a0 = torch.randn(B, nh, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    wy = torch.linspace(-1, 1, B * C * H * W, device="cuda").view(B, C, H, W)

    def stock(xn, bn, actv, g_, b_, slope):
        return oracle.spade_norm_modulate(torch.nn.functional.interpolate(xn, scale_factor=2) if up2 else xn, bn, actv, g_, b_, slope)

    def hip(xn, bn, actv, g_, b_, slope):
        return spade_norm_modulate(xn, bn, actv, g_, b_, slope, None, up2)

    outs = []
    for k, (fn, fuse) in enumerate(((stock, True), (hip, False), (hip, True))):
        monkeypatch.setattr(SphereConv2D, "fuse_spade", fuse)
        n0 = len(seen)
        xn, actv = xn0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        g_, b_ = heads[k]
        y = fn(xn, bns[k], actv, g_, b_, slope)
        (y * wy).sum().backward()
        outs.append([y.detach(), xn.grad, actv.grad, g_.weight.grad, g_.bias.grad, b_.weight.grad, b_.bias.grad])
        if k:
            assert ("eml_sphere_conv_spade_fwd_f32" in seen[n0:]) == fuse and ("eml_spade_norm_modulate_bwd_y_f32" in seen[n0:]) == fuse
    names = ["y", "d_x", "d_actv", "dWg", "dbg", "dWb", "dbb"]
    for name, r, two, one in zip(names, *outs):
        s_ = float(r.abs().max())
        np.testing.assert_allclose(one.cpu().numpy(), two.cpu().numpy(), rtol=1e-6, atol=1e-6 * s_, err_msg="one vs two launches: " + name)
        np.testing.assert_allclose(one.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, atol=3e-5 * s_, err_msg="vs stock ops: " + name)
    np.testing.assert_allclose(bns[2].running_mean.cpu().numpy(), bns[0].running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bns[2].running_var.cpu().numpy(), bns[0].running_var.cpu().numpy(), rtol=1e-5, atol=1e-6)
    # inference (the discriminator step's generator pass): gamma is not stored either
    monkeypatch.setattr(SphereConv2D, "fuse_spade", True)
    with torch.no_grad():
        y_ng = hip(xn0, bns[2].eval(), a0, *heads[2], slope)
        y_two = (monkeypatch.setattr(SphereConv2D, "fuse_spade", False), hip(xn0, bns[1].eval(), a0, *heads[1], slope))[1]
    np.testing.assert_allclose(y_ng.cpu().numpy(), y_two.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(y_two.abs().max()))


@pytest.mark.parametrize("C,H,W,up2", [(64, 128, 256, False), (128, 128, 256, True), (256, 64, 128, True), (128, 64, 128, False)])
def test_spade_in_one_launch_at_cfg3_size_natural_dispatch(C, H, W, up2, monkeypatch):
    """BASELINE configs[2] geometry (B = 32, ngf = 64: the SPADEs of up_2 / up_3), dispatch left alone: these layers take the
    one-launch path, and it agrees with the two-launch HIP path (which the per-layer and trainer-level tests pin to the
    reference's ops) to rounding -- output, d/dx through the batch statistics, d/dactv, the four head gradients."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D, spade_norm_modulate
    torch.manual_seed(C + H)
    B, nh = 32, 128
    seen = _spy_on_lib(monkeypatch)
    g_, b_ = SphereConv2D(nh, C).cuda(), SphereConv2D(nh, C).cuda()
    hx, wx = (H // 2, W // 2) if up2 else (H, W)
    xn0 = (torch.randn(B, C, hx, wx, device="cuda") * 1.3 - 0.2).contiguous(memory_format=torch.channels_last)
    a0 = torch.randn(B, nh, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    wy = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    outs = []
    for fuse in (False, True):
        monkeypatch.setattr(SphereConv2D, "fuse_spade", fuse)
        bn = torch.nn.BatchNorm2d(C, affine=False).cuda().train()
        n0 = len(seen)
        xn, actv = xn0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        for m in (g_, b_):
            m.zero_grad(set_to_none=True)
        y = spade_norm_modulate(xn, bn, actv, g_, b_, 0.2, None, up2)
        (y * wy).sum().backward()
        outs.append([y.detach(), xn.grad, actv.grad, g_.weight.grad.clone(), g_.bias.grad.clone(), b_.weight.grad.clone(),
                     b_.bias.grad.clone()])
        assert ("eml_sphere_conv_spade_fwd_f32" in seen[n0:]) == fuse, "natural dispatch must take the one-launch path here"
        assert ("eml_spade_norm_modulate_fwd_f32" in seen[n0:] or "eml_spade_norm_modulate_up2_fwd_f32" in seen[n0:]) != fuse
        del y, xn, actv
    # (256 @ 64x128: the two-launch path forms gamma | beta with the library GEMM, the one-launch path in the gather-GEMM --
    # rounding-level differences in the pre-activation flip the LeakyReLU's mask at a handful of near-zero pixels, so the
    # gradients are compared in the L2 norm; the output is continuous in gamma, beta and is compared entry by entry)
    for name, two, one in zip(["y", "d_x", "d_actv", "dWg", "dbg", "dWb", "dbb"], *outs):
        if name == "y":
            assert float((one - two).abs().max()) <= 2e-6 * float(two.abs().max()), name
        assert float((one - two).norm()) <= 1e-3 * float(two.norm()), name   # measured 1.3e-4 (three flipped pixels of 67 M)


def test_sphere_conv_properties_at_full_size():
    """cfg3 size (B=32, 128x256, 128 -> 64 channels) is checked through size-independent properties: exact linearity
    and determinism of the forward, and the adjoint identity <conv(x), y> == <x, conv^T(y)> that ties the deterministic
    col2im gather to the im2col gather it transposes."""
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    torch.manual_seed(9)
    m = SphereConv2D(128, 64, bias=False).cuda()
    x = torch.randn(32, 128, 128, 256, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y1 = m(x)
    with torch.no_grad():
        assert torch.equal(m(x), y1), "forward must be run-to-run exact"
        assert torch.equal(m(2.0 * x), 2.0 * y1), "forward must be exactly linear in x"
    gy = torch.randn_like(y1)
    (gx,) = torch.autograd.grad(y1, x, gy, retain_graph=True)
    (gx2,) = torch.autograd.grad(y1, x, gy)
    assert torch.equal(gx, gx2), "gather backward must be run-to-run exact"
    lhs = float((y1.detach().double() * gy.double()).sum())
    rhs = float((x.detach().double() * gx.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)


# ------------------------------------------------------------------------------------------ VGG19 perceptual term
@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", [(2, 3, 64, 16, 32, 1), (2, 64, 64, 32, 64, 1), (1, 128, 256, 16, 32, 1),
                                                   (32, 64, 128, 64, 128, 1), (2, 64, 64, 17, 30, 2), (1, 512, 512, 8, 16, 1)])
def test_planar_conv3x3_vs_conv2d(B, Cin, Cout, H, W, stride):
    """An ordinary zero-padded 3x3 convolution through the SphereConv gather-GEMM kernels (planar tap table) against
    F.conv2d(padding=1): output, d/dx, d/dweight, d/dbias; unfused (3 input channels, small layers) and fused dispatch."""
    from emlight_amd.GenProjector.spherenet import planar_conv3x3
    torch.manual_seed(Cin + Cout)
    w = (torch.randn(Cout, Cin, 3, 3, device="cuda") / np.sqrt(9 * Cin)).requires_grad_(True)
    b = torch.randn(Cout, device="cuda").requires_grad_(True)
    x = torch.randn(B, Cin, H, W, device="cuda")
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wr, br = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yh = planar_conv3x3(xh, w, b, stride)
    yr = torch.nn.functional.conv2d(xr, wr, br, stride=stride, padding=1)
    assert yh.shape == yr.shape
    gy = torch.randn_like(yr)
    yh.backward(gy)
    yr.backward(gy)
    for name, a, c in [("y", yh.detach(), yr.detach()), ("dx", xh.grad, xr.grad), ("dW", w.grad, wr.grad), ("db", b.grad, br.grad)]:
        np.testing.assert_allclose(a.cpu().numpy(), c.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(c.abs().max()), err_msg=name)


def test_vgg19_features_and_loss_vs_stock_ops():
    """The perceptual term's arithmetic (architecture.py:92-125, loss.py:102-114) with INJECTED weights: a torchvision-style
    ``vgg19`` state dict (seeded here; the ImageNet one cannot be obtained offline) is loaded into VGG19Features and into a
    stock nn.Sequential with torchvision's layer indices; the five feature maps, the loss and d loss / d fake agree."""
    from emlight_amd.GenProjector.vgg import VGG19Features, vgg_loss, _CFG
    torch.manual_seed(3)
    layers, sd = {}, {}
    for item in _CFG:
        if item != "M":
            idx, ci, co = item
            conv = torch.nn.Conv2d(ci, co, 3, padding=1)
            torch.nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            torch.nn.init.uniform_(conv.bias, -0.1, 0.1)
            layers[idx] = conv
            sd["features.%d.weight" % idx], sd["features.%d.bias" % idx] = conv.weight.detach().clone(), conv.bias.detach().clone()
    sd["classifier.0.weight"] = torch.zeros(4, 4)          # torchvision's dict also carries the classifier: ignored
    seq = []
    for i in range(30):
        seq.append(layers[i] if i in layers else (torch.nn.MaxPool2d(2, 2) if i in (4, 9, 18, 27) else torch.nn.ReLU()))
    stock = torch.nn.Sequential(*seq).cuda()

    def stock_feats(x):
        out = []
        for i, m in enumerate(stock):
            x = m(x)
            if i in (1, 6, 11, 20, 29):
                out.append(x)
        return out
    vgg = VGG19Features(state_dict=sd).cuda()
    assert vgg.pretrained and not any(q.requires_grad for q in vgg.parameters())
    B = 2
    fake = (torch.rand(B, 3, 128, 256, device="cuda") * 3).requires_grad_(True)
    fake_r = fake.detach().clone().requires_grad_(True)
    real = torch.rand(B, 3, 128, 256, device="cuda") * 3
    got, want = vgg(fake), stock_feats(fake_r)
    assert [tuple(t.shape) for t in got] == [(B, 64, 128, 256), (B, 128, 64, 128), (B, 256, 32, 64), (B, 512, 16, 32), (B, 512, 8, 16)]
    for a, c in zip(got, want):
        np.testing.assert_allclose(a.detach().cpu().numpy(), c.detach().cpu().numpy(), rtol=1e-4, atol=1e-4 * float(c.abs().max()))
    l_h = vgg_loss(vgg, fake, real) * 5
    w5 = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
    with torch.no_grad():
        fr = stock_feats(real)
    l_r = sum(w * torch.nn.functional.l1_loss(a, c) for w, a, c in zip(w5, stock_feats(fake_r), fr)) * 5
    np.testing.assert_allclose(float(l_h), float(l_r), rtol=1e-4)
    # the data gradient of the whole stack, first through a LINEAR functional of the five maps (no sign(.) in it: tight) ...
    proj = [torch.randn_like(c) for c in want]
    gh, = torch.autograd.grad(sum(w * (a * q).mean() for w, a, q in zip(w5, got, proj)), fake, retain_graph=True)
    gr, = torch.autograd.grad(sum(w * (c * q).mean() for w, c, q in zip(w5, want, proj)), fake_r, retain_graph=True)
    # Through 13 ReLU layers and 4 max-pools a unit whose pre-activation lies within the forward's rounding error of zero takes
    # the other branch.  Measured against the TRUTH (the same stack in f64 on the CPU), round 4, two boxes: the HIP stack
    # 1.56e-2 (deterministic: the same kernels everywhere), MIOpen's f32 stack 2.9e-3 on one box and ~1.6e-2 on another (the
    # library picks its algorithm per device; HIP vs MIOpen was 5.7e-3 / 1.6e-2 there).  The HIP convolutions accumulate
    # K = 9C <= 4608 products in ONE sequential f32 MFMA chain: relative error ~3.5e-7 * sqrt(K) ~ 2e-5 of the output scale
    # (cdna_hip_programming.md, FP32-input MFMA), i.e. a fraction ~6e-5 of the units flips over 13 layers and moves the
    # gradient by 2 * sqrt(6e-5) ~ 1.5e-2 in relative L2 -- the figure measured.  That is f32 arithmetic, not a defect: each
    # layer's own d/dx is held to 1e-4 by test_planar_conv3x3_vs_conv2d and the features below to 1e-4; a wrong kernel or a
    # wrong tap table is O(1).  Bound: 2.5e-2 (1.6x the measured, deterministic value).
    stock64 = oracle.StockVGG19(sd).double()
    fake64 = fake.detach().cpu().double().requires_grad_(True)
    want64 = stock64(fake64)
    g64, = torch.autograd.grad(sum(w * (c * q.cpu().double()).mean() for w, c, q in zip(w5, want64, proj)), fake64)
    rel = lambda g: float((g.detach().cpu().double() - g64).norm() / g64.norm())
    e_hip, e_stock = rel(gh), rel(gr)
    e_lin = float((gh - gr).double().norm() / gr.double().norm())
    print("VGG stack data gradient, linear functional: vs f64 HIP %.2e, stock f32 %.2e; HIP vs stock f32 %.2e" % (e_hip, e_stock, e_lin))
    assert e_hip < 2.5e-2
    # ... then through the L1 loss itself: sign(a - b) flips wherever two f32 evaluations of a feature difference straddle
    # zero (a fraction f of the elements moves the gradient by ~2 sqrt(f) in relative L2), so: relative L2, loose
    l_h.backward()
    l_r.backward()
    d = (fake.grad - fake_r.grad).double()
    e_l1 = float(d.norm() / fake_r.grad.double().norm())
    print("VGG stack data gradient, L1 loss: rel L2 %.2e" % e_l1)
    assert e_l1 < 2e-2
    with pytest.warns(UserWarning, match="RANDOM features"):
        VGG19Features()


def test_frozen_weight_layouts_are_remembered_and_follow_the_weight():
    """The (O, 9C) / (C, 9O) operands of a weight that takes no gradient (the VGG19 stack) are built once per (Parameter,
    version, storage) -- and again when the weight is rewritten."""
    from emlight_amd.GenProjector import spherenet
    from emlight_amd.GenProjector.vgg import PlanarConv3x3
    torch.manual_seed(0)
    conv = PlanarConv3x3(64, 64).cuda()
    for q in conv.parameters():
        q.requires_grad = False
    x = torch.randn(2, 64, 16, 32, device="cuda", requires_grad=True)
    spherenet._FROZEN.clear()
    y1 = conv(x)
    y1.sum().backward()
    held = {k[1]: v[2].data_ptr() for k, v in spherenet._FROZEN.items()}
    assert set(held) >= {"w2"}
    y2 = conv(x)
    assert torch.equal(y1, y2) and {k[1]: v[2].data_ptr() for k, v in spherenet._FROZEN.items()} == held   # no new copies
    want = torch.nn.functional.conv2d(x, conv.weight, conv.bias, padding=1)
    np.testing.assert_allclose(y2.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-4, atol=1e-4)
    with torch.no_grad():
        conv.weight.mul_(-0.5)
    y3 = conv(x)
    np.testing.assert_allclose(y3.detach().cpu().numpy(), (-0.5 * (want - conv.bias.view(1, -1, 1, 1)) + conv.bias.view(1, -1, 1, 1)).detach().cpu().numpy(),
                               rtol=1e-4, atol=1e-4)
    trainable = PlanarConv3x3(64, 64).cuda()
    n = len(spherenet._FROZEN)
    trainable(x)
    assert len(spherenet._FROZEN) == n                                   # a weight that takes a gradient is never remembered


def test_vgg_stack_construction_leaves_the_global_rng_alone():
    """building the (random) feature stack must not reseed the CPU or the CUDA generators."""
    from emlight_amd.GenProjector.vgg import VGG19Features
    torch.manual_seed(1234)
    torch.cuda.manual_seed(99)
    c0, g0 = torch.random.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    with pytest.warns(UserWarning, match="RANDOM features"):
        a = VGG19Features(seed=0)
    assert torch.equal(torch.random.get_rng_state(), c0) and torch.equal(torch.cuda.get_rng_state(), g0)
    with pytest.warns(UserWarning, match="RANDOM features"):
        b = VGG19Features(seed=0)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))   # still seeded


def test_random_vgg_features_need_an_explicit_opt_in():
    """with the term on, no weights and no ``vgg_random`` the model refuses to be built."""
    from emlight_amd.GenProjector import networks
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    with pytest.raises(ValueError, match="vgg_random"):
        Pix2PixModel(networks.default_options(ngf=4, ndf=4, no_vgg_loss=False))
    import argparse
    ap = argparse.ArgumentParser()
    networks.add_vgg_arguments(ap)
    assert networks.vgg_options(ap.parse_args([]), verbose=False)["no_vgg_loss"] is True          # default: OFF, said so
    assert networks.vgg_options(ap.parse_args(["--vgg_random"]), verbose=False)["no_vgg_loss"] is False
    assert networks.vgg_options(ap.parse_args(["--vgg_weights", "x.pth"]), verbose=False)["no_vgg_loss"] is False


def _rel_l2_report(named_got, named_want):
    """per-tensor relative L2 gradient errors (floor: 1e-3 of the median tensor RMS), largest first"""
    grads = {k: q.grad.detach().cpu().double() for k, q in named_want.items() if q.grad is not None}
    rms = lambda t: float(t.pow(2).mean().sqrt())
    floor = 1e-3 * float(np.median([rms(g) for g in grads.values()]))
    return sorted(((rms(named_got[k].grad.detach().cpu().double() - g) / max(rms(g), floor), k) for k, g in grads.items()),
                  reverse=True)


def test_generator_and_discriminator_step_with_the_vgg_term_vs_stock_ops():
    """the configuration that is TIMED (bench.py, the CLIs: VGG perceptual term on) pinned at trainer
    level.  The same seeded torchvision-style vgg19 state dict is injected into the HIP feature stack (gather-GEMM kernels)
    and into a stock nn.Sequential on the all-stock CPU side (oracle SphereConv / SPADE, ATen norms); one generator step and
    one discriminator step (pix2pix_model.py:92-141): every loss term incl. VGG <= 2e-3 rel, generator gradients <= 2e-2
    relative L2 per tensor (median 2e-3), discriminator gradients likewise."""
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.model_trainer import Trainer
    from emlight_amd.GenProjector.vgg import VGG19Features
    torch.manual_seed(5)
    sd = oracle.seeded_vgg19_state_dict(seed=3)
    opt = networks.default_options(ngf=8, ndf=8, no_vgg_loss=False)
    cpu = Trainer(opt, device="cpu", vgg_features=oracle.StockVGG19(sd))
    cpu.model.netG.load_state_dict(oracle.deterministic_projector_state_dict(cpu.model.netG.state_dict(), seed=11))
    cpu.model.netD.load_state_dict(oracle.deterministic_projector_state_dict(cpu.model.netD.state_dict(), seed=12))
    hip = Trainer(opt, device="cuda", vgg_features=VGG19Features(state_dict=sd))
    assert hip.model.vgg_variant == "pretrained"
    hip.model.netG.load_state_dict(cpu.model.netG.state_dict())
    hip.model.netD.load_state_dict(cpu.model.netD.state_dict())
    batch = data.projector_batch(2, "cuda", seed=31)
    batch_cpu = {k: v.cpu() for k, v in batch.items()}
    # generator half: losses + gradients BEFORE Adam (model_trainer.py:34-42 without the step)
    gl_h, fake_h = hip.model(batch, mode="generator")
    sum(gl_h.values()).mean().backward()
    with oracle.stock_sphere_ops():
        gl_c, fake_c = cpu.model(batch_cpu, mode="generator")
        sum(gl_c.values()).mean().backward()
    assert set(gl_h) == set(gl_c) == {"GAN", "GAN_Feat", "VGG", "COS"}
    for k in gl_c:
        a, b = float(gl_h[k].detach().mean()), float(gl_c[k].detach().mean())
        print("G loss %-8s hip %.6f  stock %.6f" % (k, a, b))
        assert abs(a - b) <= 2e-3 * abs(b) + 1e-6, (k, a, b)
    np.testing.assert_allclose(fake_h.detach().cpu().numpy(), fake_c.detach().numpy(), rtol=1e-3, atol=2e-3)
    errs = _rel_l2_report(dict(hip.model.netG.named_parameters()), dict(cpu.model.netG.named_parameters()))
    print("generator gradients with the VGG term: worst %s, median %.2e" % (errs[:3], np.median([e for e, _ in errs])))
    assert errs[0][0] < 2e-2 and np.median([e for e, _ in errs]) < 2e-3, errs[:6]
    # discriminator half from the same (un-updated) weights
    for tr in (hip, cpu):
        tr.optimizer_D.zero_grad()
    dl_h = hip.model(batch, mode="discriminator")
    sum(dl_h.values()).mean().backward()
    with oracle.stock_sphere_ops():
        dl_c = cpu.model(batch_cpu, mode="discriminator")
        sum(dl_c.values()).mean().backward()
    for k in dl_c:
        a, b = float(dl_h[k].detach().mean()), float(dl_c[k].detach().mean())
        assert abs(a - b) <= 2e-3 * abs(b) + 1e-6, (k, a, b)
    errs = _rel_l2_report(dict(hip.model.netD.named_parameters()), dict(cpu.model.netD.named_parameters()))
    print("discriminator gradients: worst %s, median %.2e" % (errs[:3], np.median([e for e, _ in errs])))
    assert errs[0][0] < 2e-2 and np.median([e for e, _ in errs]) < 2e-3, errs[:6]


def test_generator_step_includes_the_vgg_term():
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.model_trainer import Trainer
    torch.manual_seed(0)
    with pytest.warns(UserWarning, match="RANDOM features"):
        tr = Trainer(networks.default_options(ngf=4, ndf=4, no_vgg_loss=False, vgg_random=True), device="cuda")
    tr.step(data.projector_batch(2, "cuda", seed=3))
    losses = tr.get_latest_losses()
    assert set(losses) == {"GAN", "GAN_Feat", "VGG", "COS", "D_Fake", "D_real"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()) and float(losses["VGG"]) > 0
    assert not any("vgg" in k for k in tr.model.netG.state_dict())    # checkpoints hold G and D only, like the reference's


# ------------------------------------------------------------------------- epilogues folded into the convolution, InstanceNorm
@pytest.mark.parametrize("B,Cin,Cout,H,W,stride,slope,with_res", [
    (2, 64, 64, 16, 32, 1, 0.2, True), (2, 128, 128, 32, 64, 1, 1.0, True), (1, 64, 128, 16, 32, 1, 0.0, False),   # fused kernel
    (2, 6, 8, 8, 16, 1, 0.2, True), (2, 3, 16, 8, 16, 1, 0.0, False),                                               # library GEMM
    (2, 3, 128, 16, 32, 1, 0.0, False), (3, 6, 64, 16, 32, 2, 0.2, False), (2, 3, 64, 8, 16, 1, 0.0, False),        # 3-channel kernels (6 -> 64: general)
    (1, 3, 128, 5, 6, 1, 1.0, False), (2, 3, 128, 64, 128, 1, 0.0, False)])
def test_sphere_conv_epilogue_residual_and_activation(B, Cin, Cout, H, W, stride, slope, with_res):
    """``leaky_relu(conv(x) + residual, slope)`` in the kernel's epilogue (fused kernel: first three shapes with
    ``fused_min_bytes = 0``; library-GEMM path; the few-channel input-layer kernels of ``csrc/sphere_conv_small.hip``, whose
    weight gradient also folds the activation's backward and the bias gradient) against the separate stock ops of the
    reference (architecture.py:60, generator.py:84, normalization.py:92-96): value and d/dx, d/dW, d/db, d/dresidual."""
    from emlight_amd import _lib
    from emlight_amd.GenProjector.spherenet import SphereConv2D
    torch.manual_seed(Cin + Cout)
    conv = SphereConv2D(Cin, Cout, stride=stride).cuda()
    assert bool(_lib.lib().eml_sphere_conv_small_supported(Cin, Cout)) == ((Cin, Cout) in ((3, 64), (3, 128)))
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    x = torch.randn(B, Cin, H, W, device="cuda")
    res = (torch.randn(B, Cout, H // stride, W // stride, device="cuda").contiguous(memory_format=torch.channels_last)
           if with_res else None)
    leaves = []
    outs = []
    saved = SphereConv2D.fused_min_bytes
    SphereConv2D.fused_min_bytes = 0
    try:
        for fn in ("hip", "stock"):
            xi = x.clone().requires_grad_(True)
            ri = res.clone().requires_grad_(True) if with_res else None
            for q in conv.parameters():
                q.grad = None
            if fn == "hip":
                y = conv(xi, residual=ri, act_slope=slope)
            else:
                y = oracle.sphere_conv(xi, conv.weight, conv.bias, stride, ri, slope)
            gy = torch.randn(y.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            y.backward(gy)
            outs.append(y.detach())
            leaves.append([xi.grad, conv.weight.grad.clone(), conv.bias.grad.clone()] + ([ri.grad] if with_res else []))
    finally:
        SphereConv2D.fused_min_bytes = saved
    scale = float(outs[1].abs().max())
    np.testing.assert_allclose(outs[0].cpu().numpy(), outs[1].cpu().numpy(), rtol=1e-4, atol=3e-5 * scale)
    if slope == 0.0:
        assert float(outs[0].min()) >= 0.0
    for name, a, b in zip(("dx", "dW", "db", "dres"), leaves[0], leaves[1]):
        # an output within rounding of 0 may take the other branch of the activation: compare in RMS, not element-wise
        err = float((a - b).norm() / b.norm().clamp_min(1e-20))
        assert err < 2e-3, (name, err)


@pytest.mark.parametrize("B,C,H,W,cl,slope", [(4, 128, 32, 64, True, 0.2), (3, 36, 8, 16, True, 0.2), (2, 512, 8, 16, True, 1.0),
                                              (4, 64, 64, 64, False, 0.2), (2, 512, 4, 4, False, 0.2), (2, 6, 5, 7, False, 0.0)])
def test_instance_norm_act_vs_stock_ops(B, C, H, W, cl, slope):
    """``leaky_relu(InstanceNorm2d(affine=False)(x), slope)`` as one HIP launch each way (channels-last and NCHW) against
    ATen in f64: value and input gradient (normalization.py:44-45, discriminator.py:84-98)."""
    from emlight_amd.GenProjector.spherenet import instance_norm_act
    torch.manual_seed(C)
    x = (torch.randn(B, C, H, W, device="cuda") * 3 + 1.5)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    norm = torch.nn.InstanceNorm2d(C, affine=False)
    xh = x.clone().requires_grad_(True)
    if cl:
        xh.data = xh.data.contiguous(memory_format=torch.channels_last)
    yh = instance_norm_act(xh, norm, slope)
    assert yh.shape == x.shape and yh.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    xr = x.double().contiguous().requires_grad_(True)
    yr = norm(xr)
    yr = yr if slope == 1.0 else torch.nn.functional.leaky_relu(yr, slope)
    gy = torch.randn_like(x)
    yh.backward(gy)
    yr.backward(gy.double())
    np.testing.assert_allclose(yh.detach().cpu().numpy(), yr.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    err = float((xh.grad.double() - xr.grad).norm() / xr.grad.norm())
    assert err < 1e-4, err
    # not the HIP kernel: a norm with running statistics or an affine one falls back to the module itself
    aff = torch.nn.InstanceNorm2d(C, affine=True).cuda()
    torch.testing.assert_close(instance_norm_act(x, aff, 0.2), torch.nn.functional.leaky_relu(aff(x), 0.2))


@pytest.mark.parametrize("O,C", [(64, 32), (128, 1024), (1024, 128), (3, 64), (40, 6)])
def test_fused_spectral_norm_vs_torch_hook(O, C):
    """``csrc/spectral.hip`` against ``torch.nn.utils.spectral_norm`` on the same weight_orig / u / v: the normalised weight,
    the updated power-iteration buffers, the gradient w.r.t. weight_orig (u, v constants), a second training forward, and
    eval mode (no iteration) -- and the state_dict keys of the wrapped module are torch's."""
    import copy
    from emlight_amd.GenProjector.spherenet import SphereConv2D, fused_spectral_norm
    torch.manual_seed(O + C)
    base = SphereConv2D(C, O).cuda()
    with torch.no_grad():
        base.weight.normal_(0, 0.05)
    ref = torch.nn.utils.spectral_norm(copy.deepcopy(base))
    hip = fused_spectral_norm(copy.deepcopy(base))
    hip.load_state_dict(ref.state_dict())
    assert set(hip.state_dict()) == set(ref.state_dict()) == {"weight_orig", "weight_u", "weight_v", "bias"}
    pre_ref = next(iter(ref._forward_pre_hooks.values()))
    pre_hip = next(iter(hip._forward_pre_hooks.values()))
    gw = torch.randn(O, C, 3, 3, device="cuda")
    for mode in ("train", "train", "eval"):
        ref.train(mode == "train")
        hip.train(mode == "train")
        for m in (ref, hip):
            m.weight_orig.grad = None
        pre_ref(ref, None)
        pre_hip(hip, None)
        assert hip.weight.shape == ref.weight.shape == (O, C, 3, 3)
        s = float(ref.weight.abs().max())
        np.testing.assert_allclose(hip.weight.detach().cpu().numpy(), ref.weight.detach().cpu().numpy(), rtol=2e-5, atol=2e-6 * s)
        for name in ("weight_u", "weight_v"):
            np.testing.assert_allclose(getattr(hip, name).cpu().numpy(), getattr(ref, name).cpu().numpy(), rtol=1e-4, atol=1e-6)
        (ref.weight * gw).sum().backward()
        (hip.weight * gw).sum().backward()
        gs = float(ref.weight_orig.grad.abs().max())
        np.testing.assert_allclose(hip.weight_orig.grad.cpu().numpy(), ref.weight_orig.grad.cpu().numpy(), rtol=1e-4,
                                   atol=1e-5 * gs)
    # the (O, C, 3, 3) weight the hook hands to the convolution is a view of the kernels' (O, tap, c) operand: no re-layout copy
    w2 = hip.weight.permute(0, 2, 3, 1)
    assert w2.is_contiguous()


@pytest.mark.parametrize("iterate", [1, 0])
def test_batched_spectral_norm_is_bit_identical_to_single_calls(iterate):
    """``eml_spectral_norm_w2_batch_f32`` (round 5: every normalised weight of a network in five launches) against one
    ``eml_spectral_norm_w2_f32`` per weight on copies of the same operands: W2, sigma, the (u | v) record and the updated
    buffers, bit for bit -- 37 weights (two chunks of the 32-entry batch), wide, narrow, non-multiple-of-4 channel counts."""
    import ctypes
    from emlight_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    g = torch.Generator(device="cuda").manual_seed(17 + iterate)
    shapes = [(64, 64), (128, 256), (1024, 1024), (32, 3), (8, 5), (512, 1024), (3, 64)] + [(16 + 8 * i, 12 + 4 * i) for i in range(30)]

    def operands():
        out = []
        for O, C in shapes:
            out.append(dict(O=O, C=C, W=torch.randn(O, C, 3, 3, device="cuda", generator=g) * 0.05,
                            u=torch.nn.functional.normalize(torch.randn(O, device="cuda", generator=g), dim=0),
                            v=torch.nn.functional.normalize(torch.randn(9 * C, device="cuda", generator=g), dim=0)))
        return out
    ops = operands()
    res = {}
    for mode in ("single", "batch"):
        items = [dict(o, u=o["u"].clone(), v=o["v"].clone(), W2=torch.full((o["O"], 9 * o["C"]), float("nan"), device="cuda"),
                      sigma=torch.zeros(1, device="cuda"), uv=torch.zeros(o["O"] + 9 * o["C"], device="cuda"),
                      scratch=torch.empty(L.eml_spectral_norm_scratch_floats(o["O"], o["C"]), device="cuda")) for o in ops]
        if mode == "single":
            for it in items:
                _lib.check(L.eml_spectral_norm_w2_f32(p(it["W"]), p(it["u"]), p(it["v"]), iterate, 1e-12, p(it["W2"]), p(it["sigma"]),
                                                      p(it["uv"]), p(it["scratch"]), it["O"], it["C"], st), "single")
        else:
            n = len(items)
            arr = lambda key: (ctypes.c_void_p * n)(*[it[key].data_ptr() for it in items])
            ints = lambda key: (ctypes.c_int * n)(*[it[key] for it in items])
            _lib.check(L.eml_spectral_norm_w2_batch_f32(n, arr("W"), arr("u"), arr("v"), iterate, 1e-12, arr("W2"), arr("sigma"),
                                                        arr("uv"), arr("scratch"), ints("O"), ints("C"), st), "batch")
        torch.cuda.synchronize()
        res[mode] = items
    for a, b in zip(res["single"], res["batch"]):
        for key in ("W2", "sigma", "uv", "u", "v"):
            assert torch.equal(a[key], b[key]), (a["O"], a["C"], key)
        assert bool(torch.isfinite(b["W2"]).all())
    assert L.eml_spectral_norm_w2_batch_f32(0, None, None, None, 1, 1e-12, None, None, None, None, None, None, st) == 0   # empty batch


def test_generator_with_batched_spectral_norm_equals_per_module_hooks(monkeypatch):
    """The generator's forward + backward with ``spectral_precompute`` (default) and with every hook launching for itself
    (EML_SN_BATCH=0): the image, the power-iteration buffers and every parameter gradient of this repo's kernels, bit for bit."""
    import copy
    from emlight_amd.GenProjector import networks, spherenet
    torch.manual_seed(3)
    opt = networks.default_options()
    opt.ngf = 8
    a = networks.SPADEGenerator(opt).cuda()
    networks.init_weights(a, "xavier", 0.02)
    b = copy.deepcopy(a)
    guide = torch.rand(2, 3, 128, 256, device="cuda")
    crop = torch.rand(2, 3, 96, 128, device="cuda")
    outs = []
    for net, flag in ((a, True), (b, False)):
        monkeypatch.setattr(spherenet, "_sn_batch", flag)
        net.train()
        for _ in range(2):   # two passes: the second starts from the buffers the first one left
            net.zero_grad(set_to_none=True)
            y = net(guide, crop)
            y.square().mean().backward()
        with torch.no_grad():
            net.eval()
            ye = net(guide, crop)
        outs.append((y.detach(), ye, {n: q.grad for n, q in net.named_parameters()}, dict(net.named_buffers())))
    (ya, yea, ga, ba), (yb, yeb, gb, bb) = outs
    assert torch.equal(ya, yb) and torch.equal(yea, yeb)
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None), n
        if ga[n] is None:
            continue
        if n.startswith("netE."):   # the crop encoder's nn.Conv2d / Linear run on MIOpen / the BLAS library: their weight
            torch.testing.assert_close(ga[n], gb[n], rtol=1e-3, atol=1e-4 * float(gb[n].abs().max()))   # gradients are not run-to-run exact
        else:
            assert torch.equal(ga[n], gb[n]), n
    for n in ba:
        assert torch.equal(ba[n], bb[n]), n
    plan = spherenet._SN_PLANS[a]
    assert len(plan) == 23 and all(h.pre is None for _, h in plan)   # 18 SphereConvs of the blocks + the crop encoder's 5; all consumed
    assert "_eml_sn_plan" not in a.__dict__   # (kept beside the network: a pickled / copied one does not carry it)


@pytest.mark.parametrize("fin,fout,H,W,train", [(64, 32, 8, 16, True), (128, 64, 16, 32, True), (32, 16, 4, 8, False)])
def test_spade_block_with_the_upsample_folded_in(fin, fout, H, W, train):
    """``blk(x, seg, up2=True)`` (the nearest x2 upsample of generator.py:70-82 folded into the SPADE kernels: statistics from the
    low-resolution map, indexing in the modulation, the 4-children sum in BatchNorm's backward) against ``blk(up(x), seg)`` on
    the same HIP kernels: output, running statistics, d/dx and every parameter gradient."""
    import copy
    from emlight_amd.GenProjector import networks
    torch.manual_seed(fin)
    opt = networks.default_options()
    a = networks.SPADEResnetBlock(fin, fout, opt).cuda()
    networks.init_weights(a, "xavier", 0.02)
    b = copy.deepcopy(a)
    a.train(train)
    b.train(train)
    x = torch.randn(3, fin, H, W, device="cuda")
    seg = torch.rand(3, 3, 128, 256, device="cuda")
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = a(xa, seg, up2=True)
    yb = b(torch.nn.functional.interpolate(xb, scale_factor=2), seg)
    assert ya.shape == yb.shape == (3, fout, 2 * H, 2 * W)
    s = float(yb.detach().abs().max())
    np.testing.assert_allclose(ya.detach().cpu().numpy(), yb.detach().cpu().numpy(), rtol=1e-4, atol=1e-5 * s)
    gy = torch.randn_like(yb)
    ya.backward(gy)
    yb.backward(gy)
    err = float((xa.grad - xb.grad).norm() / xb.grad.norm())
    assert err < 1e-4, err
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        e = float((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-20))
        assert e < 2e-4, (k, e)
    for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6, msg=k)


def test_gamma_beta_bias_gradient_comes_from_the_modulation_backward(monkeypatch):
    """The bias gradient of SPADE's gamma | beta convolution is the column sum of dgb; the modulation's backward leaves it on
    the dgb tensor (f64-accumulated) and the convolution's backward must use that instead of reducing dgb again."""
    from emlight_amd.GenProjector import spherenet
    torch.manual_seed(3)
    C, nh = 64, 128
    bn = torch.nn.BatchNorm2d(C, affine=False).cuda().train()
    g_, b_ = spherenet.SphereConv2D(nh, C).cuda(), spherenet.SphereConv2D(nh, C).cuda()
    x = torch.randn(4, C, 16, 32, device="cuda", requires_grad=True)
    actv = torch.randn(4, nh, 16, 32, device="cuda")
    loss = (spherenet.spade_norm_modulate(x, bn, actv, g_, b_, 0.2) * torch.randn(4, C, 16, 32, device="cuda")).sum()
    calls = []
    real_sum = torch.Tensor.sum
    monkeypatch.setattr(torch.Tensor, "sum", lambda self, *a, **k: (calls.append(tuple(self.shape)), real_sum(self, *a, **k))[1])
    loss.backward()
    monkeypatch.undo()
    assert calls == [], calls
    assert g_.bias.grad is not None and float(g_.bias.grad.abs().max()) > 0 and float(b_.bias.grad.abs().max()) > 0


def test_stale_column_sums_are_not_used_for_the_bias_gradient(monkeypatch):
    """the column sums travel as an attribute of the dgb tensor.  If that tensor is written between the
    modulation's backward and the convolution's (autograd accumulating a second consumer's gradient in place, a hook), the
    sums are stale: the convolution's backward must notice (storage pointer + version counter) and reduce dgb itself.  Here a
    hook doubles dgb IN PLACE (same tensor object, attribute still attached): the bias gradients must double too."""
    from emlight_amd.GenProjector import spherenet
    C, nh = 64, 128

    def run(hook):
        torch.manual_seed(3)
        bn = torch.nn.BatchNorm2d(C, affine=False).cuda().train()
        g_, b_ = spherenet.SphereConv2D(nh, C).cuda(), spherenet.SphereConv2D(nh, C).cuda()
        x = torch.randn(4, C, 16, 32, device="cuda", requires_grad=True)
        actv = torch.randn(4, nh, 16, 32, device="cuda")
        wgt = torch.randn(4, C, 16, 32, device="cuda")
        real = spherenet.sphere_conv

        def hooked(*a, **k):
            out = real(*a, **k)
            if hook:
                out.register_hook(lambda g: g.mul_(2.0))
            return out
        monkeypatch.setattr(spherenet, "sphere_conv", hooked)
        (spherenet.spade_norm_modulate(x, bn, actv, g_, b_, 0.2) * wgt).sum().backward()
        monkeypatch.undo()
        return g_.bias.grad.clone(), b_.bias.grad.clone(), g_.weight.grad.clone()
    g0, b0, w0 = run(False)
    g1, b1, w1 = run(True)
    torch.testing.assert_close(w1, 2 * w0, rtol=1e-5, atol=1e-6)   # the hook took effect
    torch.testing.assert_close(g1, 2 * g0, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(b1, 2 * b0, rtol=1e-4, atol=1e-5)


def test_three_iterations_follow_the_stock_op_trajectory():
    """Three full projector iterations (G step + D step each, fresh batch each) on the HIP path against the same trainer on the
    CPU with every op stock (torch's spectral-norm hook, ATen instance norm, unfused Adam, the oracle's SphereConv / SPADE):
    what a single step cannot show -- the power-iteration buffers after six forwards, SPADE's running statistics, Adam's
    moments -- stays on the reference's trajectory.  Bounds from the measured distances (tools/debug_trajectory.py: losses
    <= 3e-4, buffers <= 1.4e-3, parameter UPDATES <= 0.11 of the update's norm), with a factor <= 2 of head room on the
    updates.  Adam's first
    updates are sign-like (|update| = lr whatever |grad|), so an element whose gradient is at round-off level may step the other
    way: updates are compared in norm; the bias of a convolution whose output only ever reaches the rest of the network through
    a parameter-free BatchNorm (conv_0 of every SPADE block; conv_1 / conv_s of every block but the last, whose sum is
    renormalised by the next block) has an exactly-zero gradient in exact arithmetic -- both sides walk on their own rounding
    noise there -- and is only held to the size of three steps."""
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.model_trainer import Trainer
    torch.manual_seed(5)
    opt = networks.default_options(ngf=8, ndf=8)
    cpu = Trainer(opt, device="cpu")
    cpu.model.netG.load_state_dict(oracle.deterministic_projector_state_dict(cpu.model.netG.state_dict(), seed=11))
    cpu.model.netD.load_state_dict(oracle.deterministic_projector_state_dict(cpu.model.netD.state_dict(), seed=12))
    hip = Trainer(opt, device="cuda")
    hip.model.netG.load_state_dict(cpu.model.netG.state_dict())
    hip.model.netD.load_state_dict(cpu.model.netD.state_dict())
    start = {n: {k: v.detach().clone().double() for k, v in net.state_dict().items()}
             for n, net in (("G", cpu.model.netG), ("D", cpu.model.netD))}
    for it in range(3):
        batch = data.projector_batch(2, "cuda", seed=30 + it)
        hip.step(batch)
        with oracle.stock_sphere_ops():
            cpu.step({k: v.cpu() for k, v in batch.items()})
        lh, lc = hip.get_latest_losses(), cpu.get_latest_losses()
        for k in lc:
            a, b = float(lh[k].detach().mean()), float(lc[k].detach().mean())
            assert abs(a - b) <= 2e-3 * abs(b) + 1e-6, (it, k, a, b)
    for net_h, net_c, name in ((hip.model.netG, cpu.model.netG, "G"), (hip.model.netD, cpu.model.netD, "D")):
        sh, sc = net_h.state_dict(), net_c.state_dict()
        assert set(sh) == set(sc)
        for k in sc:
            if not sc[k].dtype.is_floating_point:
                assert int(sh[k]) == int(sc[k]), k
                continue
            a, b, z = sh[k].detach().cpu().double(), sc[k].detach().double(), start[name][k]
            if k.endswith(("weight_u", "weight_v", "running_mean", "running_var")):
                assert float((a - b).norm()) <= 5e-3 * float(b.norm()) + 1e-7, (name, k)
            elif k.endswith(("conv_0.bias", "conv_1.bias", "conv_s.bias")) and not k.startswith("up_3.conv_1") \
                    and not k.startswith("up_3.conv_s"):
                # |Adam update| <= lr / sqrt(1 - beta2) (beta1 = 0, beta2 = 0.9); worst case: opposite directions on all 3 steps
                lr = (1e-4 if name == "G" else 4e-4) / np.sqrt(1 - 0.9)
                assert float((a - b).abs().max()) <= 2 * 3 * lr * 1.01, (name, k)
            else:
                upd = float((b - z).norm())
                assert float(((a - z) - (b - z)).norm()) <= 0.2 * upd + 1e-9, (name, k, upd)   # measured 0.11 (<= 2x)


def test_inference_in_eval_mode_matches_the_stock_ops():
    """``mode='inference'`` with the networks in eval(): running statistics in SPADE (each norm its own), no power iteration in
    the spectral norm (sigma from the stored u, v), the folded upsample and the fused epilogues -- against the all-stock CPU path."""
    from emlight_amd.GenProjector import data, networks
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    torch.manual_seed(9)
    opt = networks.default_options(ngf=8, ndf=8)
    cpu = Pix2PixModel(opt)
    cpu.netG.load_state_dict(oracle.deterministic_projector_state_dict(cpu.netG.state_dict(), seed=11))
    with torch.no_grad():   # running statistics that differ between the norms of a block, as after training
        for k, b in cpu.netG.named_buffers():
            if k.endswith("running_mean"):
                b.normal_(0, 0.2)
            elif k.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    hip = Pix2PixModel(opt)
    hip.netG.load_state_dict(cpu.netG.state_dict())
    hip = hip.cuda().eval()
    cpu = cpu.eval()
    batch = data.projector_batch(2, "cuda", seed=77)
    u_before = {k: v.clone() for k, v in hip.netG.state_dict().items() if k.endswith(("weight_u", "running_mean"))}
    got = hip(batch, "inference").cpu()
    with oracle.stock_sphere_ops():
        want = cpu({k: v.cpu() for k, v in batch.items()}, "inference")
    assert got.shape == want.shape == (2, 3, 128, 256)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-3 * float(want.abs().max()))
    for k, v in u_before.items():   # eval: no buffer moves
        assert torch.equal(hip.netG.state_dict()[k], v), k


def test_fused_l1_terms_vs_stock_formulas():
    """``csrc/losses.hip`` (feature matching over the maps of cat(fake, real) with the x50 off-light weight, and the VGG-style
    weighted L1 sum) against the literal reference formulas (pix2pix_model.py:101-117, loss.py:108-114) in f64: value,
    gradient (the real half of a feature map gets exactly 0), odd channel counts (scalar path), run-to-run bit equality."""
    from emlight_amd.GenProjector import l1_terms
    torch.manual_seed(11)
    B, num_D = 3, 2
    shapes = [(64, 16, 32), (128, 8, 16), (6, 8, 16), (512, 4, 8)]
    feats = [torch.randn(2 * B, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_()
             for c, h, w in shapes]
    with torch.no_grad():
        feats[1][:B, :, 0, 0] = feats[1][B:, :, 0, 0]   # exact ties: sign(0) = 0 like torch's abs backward
    masks = [(torch.rand(B, 1, h, w, device="cuda") > 0.7).float() for _, h, w in shapes]
    got = l1_terms.feature_matching(feats, masks, num_D)
    got.backward()
    again = l1_terms.feature_matching([t.detach() for t in feats], masks, num_D)
    assert torch.equal(got.detach(), again)
    refs = [t.detach().double().requires_grad_() for t in feats]
    want = 0
    for t, m in zip(refs, masks):
        f, r, m = t[:B], t[B:].detach(), m.double()
        want = want + torch.nn.functional.l1_loss(f * m + f * (1 - m) * 50, r * m + r * (1 - m) * 50) / num_D
    want.backward()
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    for t, rt in zip(feats, refs):
        assert float(t.grad[B:].abs().max()) == 0.0
        np.testing.assert_allclose(t.grad.cpu().numpy(), rt.grad.cpu().numpy(), rtol=1e-5, atol=1e-12)
    # VGG-style: sum_i w_i L1(a_i, b_i), gradient to a_i only; one NCHW-contiguous input (a stock feature stack)
    ws = (1 / 32, 1 / 16, 1.0)
    a = [torch.randn(B, c, h, w, device="cuda", requires_grad=True) for c, h, w in shapes[:3]]
    b = [torch.randn(B, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last) for c, h, w in shapes[:3]]
    got = l1_terms.l1_sum(zip(ws, a, b))
    got.backward()
    ar = [t.detach().double().requires_grad_() for t in a]
    want = sum(w * torch.nn.functional.l1_loss(x, y.double()) for w, x, y in zip(ws, ar, b))
    want.backward()
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    for t, rt in zip(a, ar):
        np.testing.assert_allclose(t.grad.cpu().numpy(), rt.grad.cpu().numpy(), rtol=1e-5, atol=1e-12)


@pytest.mark.gpu
def test_fused_l1_terms_with_more_pairs_than_one_launch_takes_and_with_none():
    """``--num_D 3 --n_layers_D 6`` makes 18 feature-matching pairs, ``--num_D 5`` 20 -- more than the
    16 a launch of ``eml_l1_pairs_*`` takes: they run as two launches whose sums add up; an empty list of pairs is
    the reference's zero loss (pix2pix_model.py:101-117), not an error.  Then the same through the model's own loss."""
    from emlight_amd.GenProjector import l1_terms
    torch.manual_seed(5)
    B, num_D = 2, 5
    shapes = [(8 + 4 * (i % 3), 4 + (i % 2) * 4, 8) for i in range(20)]
    feats = [torch.randn(2 * B, c, h, w, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_()
             for c, h, w in shapes]
    masks = [(torch.rand(B, 1, h, w, device="cuda") > 0.5).float() for _, h, w in shapes]
    got = l1_terms.feature_matching(feats, masks, num_D)
    got.backward()
    refs = [t.detach().double().requires_grad_() for t in feats]
    want = 0
    for t, m in zip(refs, masks):
        f, r, m = t[:B], t[B:].detach(), m.double()
        want = want + torch.nn.functional.l1_loss(f * m + f * (1 - m) * 50, r * m + r * (1 - m) * 50) / num_D
    want.backward()
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    for t, rt in zip(feats, refs):
        np.testing.assert_allclose(t.grad.cpu().numpy(), rt.grad.cpu().numpy(), rtol=1e-5, atol=1e-12)
    a = [torch.randn(B, 8, 4, 8, device="cuda", requires_grad=True) for _ in range(17)]
    b = [torch.randn(B, 8, 4, 8, device="cuda") for _ in range(17)]
    got = l1_terms.l1_sum((0.5 + i, x, y) for i, (x, y) in enumerate(zip(a, b)))
    want = sum((0.5 + i) * torch.nn.functional.l1_loss(x.double(), y.double()) for i, (x, y) in enumerate(zip(a, b)))
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    zero = l1_terms.feature_matching([], [], 2)
    assert zero.shape == () and float(zero) == 0.0 and zero.is_cuda
    # the model's generator loss at such settings: 18 pairs, and the smallest discriminators (one intermediate map each)
    from emlight_amd.GenProjector import networks
    from emlight_amd.GenProjector.data import projector_batch
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    for num_d, n_layers, pairs in ((3, 6, 18), (2, 1, 2)):
        model = Pix2PixModel(networks.default_options(ngf=4, ndf=4, num_D=num_d, n_layers_D=n_layers)).cuda()
        losses, _ = model(projector_batch(2, "cuda:0"), mode="generator")
        assert bool(torch.isfinite(losses["GAN_Feat"]).all()) and losses["GAN_Feat"].shape == (1,)
        assert float(losses["GAN_Feat"]) > 0.0
        sum(losses.values()).mean().backward()


@pytest.mark.parametrize("B,C,O,H,W", [(2, 64, 64, 16, 32), (3, 128, 128, 32, 64), (1, 128, 256, 8, 16), (2, 64, 128, 12, 20)])
def test_row_shared_corners_gather_is_bit_identical(B, C, O, H, W):
    """EML_TAP_ROWSHARE (include/emlight_hip.h): on a stride-1 sphere table a pixel's east corners are its right neighbour's
    west corners (sphere_cnn.py:31-58 shifts a whole row by the same amount), so the gather-GEMM fetches 10 lines per 4 pixels
    instead of 16.  The property is VERIFIED on the table (not assumed) -- here once more, independently -- and the kernel
    that uses it must reproduce the 16-load kernel bit for bit: forward (+ residual / activation epilogue), the SPADE epilogue,
    and the input gradient on the transposed table where that table has the property too."""
    from emlight_amd import _lib
    from emlight_amd.GenProjector import spherenet
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    torch.manual_seed(C + O + H)
    geo = spherenet.sphere_geometry(H, W, 1, torch.device("cuda"))
    po = H * W
    idx, wgt = geo.idx.view(po, 9, 4), geo.wgt.view(po, 9, 4)
    same_row = (torch.arange(po, device="cuda") % 4 != 3)[:-1]

    def shared(a, b):   # the same source pixel, or one side is grid_sample's zero-padded wrap-around column
        return (a == b) | (a < 0) | (b < 0)
    want = bool((shared(idx[:-1, :, 1], idx[1:, :, 0]) & shared(idx[:-1, :, 3], idx[1:, :, 2]))[same_row].all())
    assert want and bool((wgt[idx < 0] == 0).all()) and geo.rowshare == 1   # W % 4 == 0: 4 consecutive pixels share a row
    seams = int(((idx[:-1, :, 1] != idx[1:, :, 0]) & (idx[:-1, :, 1] >= 0) & (idx[1:, :, 0] >= 0))[same_row].sum())
    assert seams == 0
    assert spherenet.sphere_geometry(H, W, 2, torch.device("cuda")).rowshare == 0   # stride 2: neighbours sample 2 columns apart
    x = torch.randn(B * po, C, device="cuda")
    w2 = torch.randn(O, 9 * C, device="cuda") * 0.05
    bias = torch.randn(O, device="cuda")
    res = torch.randn(B * po, O, device="cuda")
    ys = []
    for flags in (0, 1):
        y = torch.full((B * po, O), float("nan"), device="cuda")
        _lib.check(L.eml_sphere_conv_fwd_fused_ex_f32(p(x), p(geo.idx), p(geo.wgt), p(w2), p(bias), p(y), B, po, po, C, O, 4, p(res),
                                                      0.2, flags, st), "fwd")
        ys.append(y)
    assert torch.equal(ys[0], ys[1])
    ref = oracle.sphere_conv(x.view(B, H, W, C).permute(0, 3, 1, 2), w2.view(O, 3, 3, C).permute(0, 3, 1, 2), bias, 1,
                             res.view(B, H, W, O).permute(0, 3, 1, 2), 0.2).permute(0, 2, 3, 1).reshape(B * po, O)
    np.testing.assert_allclose(ys[1].cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=3e-5 * float(ref.abs().max()))
    # the SPADE epilogue on the same gather (Cin = C -> 2 Cn = O rows of gamma | beta)
    if L.eml_sphere_conv_spade_supported(C, O // 2, po):
        Cn = O // 2
        xn = torch.randn(B * po, Cn, device="cuda")
        mean, istd = torch.randn(Cn, device="cuda"), torch.rand(Cn, device="cuda") + 0.5
        outs = []
        for flags in (0, 1):
            y = torch.full((B * po, Cn), float("nan"), device="cuda")
            g = torch.full((B * po, Cn), float("nan"), device="cuda")
            _lib.check(L.eml_sphere_conv_spade_fwd_f32(p(x), p(geo.idx), p(geo.wgt), p(w2), p(bias), p(xn), p(mean), p(istd), p(y),
                                                       p(g), B, H, W, C, Cn, 0, 0.2, flags, st), "spade")
            outs.append((y, g))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # input gradient: the forward kernel on the transposed table (roles of C and O swap)
    tt = geo.transposed_table()
    if tt is not None and tt[3] == 4:
        tidx, twgt, rowmax, ke = tt
        w2t = torch.randn(C, 9 * O, device="cuda") * 0.05
        gy = torch.randn(B * po, O, device="cuda")
        gs = []
        for flags in (0, geo.t_rowshare):
            gx = torch.full((B * po, C), float("nan"), device="cuda")
            _lib.check(L.eml_sphere_conv_dgrad_fused_f32(p(gy), p(tidx), p(twgt), p(rowmax), ke, p(w2t), p(gx), B, po, po, C, O,
                                                         flags, st), "dgrad")
            gs.append(gx)
        assert torch.equal(gs[0], gs[1])


@pytest.mark.parametrize("rows,cols", [(1048576, 3), (100003, 1), (4097, 8), (5, 64), (0, 3)])
def test_colsum_of_a_tall_skinny_matrix(rows, cols):
    """``eml_colsum_f32`` (the bias gradient of the few-output-channel layers) against an f64 column sum; run-to-run equal."""
    from emlight_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    x = torch.randn(max(rows, 1), cols, device="cuda")[:rows].contiguous()
    outs = []
    for _ in range(2):
        part = torch.empty(L.eml_colsum_partial_doubles(cols), dtype=torch.float64, device="cuda")
        out = torch.full((cols,), float("nan"), device="cuda")
        _lib.check(L.eml_colsum_f32(p(x) if rows else p(torch.empty(1, device="cuda")), rows, cols, p(part), p(out), st), "colsum")
        outs.append(out)
    want = x.double().sum(0)
    assert torch.equal(outs[0], outs[1])
    np.testing.assert_allclose(outs[0].cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=1e-6 * np.sqrt(max(rows, 1)))


@pytest.mark.parametrize("Cn,Cin", [(64, 128), (128, 128), (16, 64), (64, 6)])
def test_spade_heads_as_one_operand(Cn, Cin):
    """``eml_spade_heads_w2_f32``: cat(gamma head, beta head) in the (tap, c) column order of the gather-GEMM kernels, in cat
    order and -- for the one-launch SPADE -- in that kernel's row order: bitwise what cat + permute (+ row gather) produce."""
    from emlight_amd.GenProjector import spherenet
    torch.manual_seed(Cn + Cin)
    wg, wb = torch.randn(Cn, Cin, 3, 3, device="cuda"), torch.randn(Cn, Cin, 3, 3, device="cuda")
    bg, bb = torch.randn(Cn, device="cuda"), torch.randn(Cn, device="cuda")
    w_cat = torch.cat([wg, wb], 0).permute(0, 2, 3, 1).reshape(2 * Cn, 9 * Cin)
    b_cat = torch.cat([bg, bb], 0)
    w2, b2 = spherenet.spade_heads_w2(wg, wb, bg, bb, False)
    assert torch.equal(w2, w_cat) and torch.equal(b2, b_cat)
    if Cn % 64 == 0:
        order = spherenet.spade_row_order(Cn, wg.device)
        w2r, br = spherenet.spade_heads_w2(wg, wb, bg, bb, True)
        assert torch.equal(w2r, w_cat[order]) and torch.equal(br, b_cat[order])
    # through autograd: the (2 Cn, Cin, 3, 3) VIEW the convolutions take, gradients = the two halves
    wg.requires_grad_(), wb.requires_grad_(), bg.requires_grad_(), bb.requires_grad_()
    w, b = spherenet._SpadeHeadsFn.apply(wg, wb, bg, bb)
    assert w.shape == (2 * Cn, Cin, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()
    gw, gbias = torch.randn_like(w), torch.randn_like(b)
    ((w * gw).sum() + (b * gbias).sum()).backward()
    assert torch.equal(wg.grad, gw[:Cn]) and torch.equal(wb.grad, gw[Cn:]) and torch.equal(bg.grad, gbias[:Cn]) and torch.equal(bb.grad, gbias[Cn:])


@pytest.mark.parametrize("O,slope,M", [(128, 0.0, 4099), (64, 0.0, 512), (128, 1.0, 33), (64, 0.2, 70000)])
def test_small_layer_input_gradient_first_half(O, slope, M):
    """``eml_sphere_conv_small_da9_f32``: dA9 = (dY * act'(Y)) W2 for the 3-channel input layers, against the two stock steps."""
    from emlight_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    torch.manual_seed(O + M)
    gy, y = torch.randn(M, O, device="cuda"), torch.randn(M, O, device="cuda")
    w2 = torch.randn(O, 27, device="cuda") * 0.2
    da9 = torch.full((M, 27), float("nan"), device="cuda")
    _lib.check(L.eml_sphere_conv_small_da9_f32(p(gy), p(y) if slope != 1.0 else None, slope, p(w2), p(da9), M, 3, O, st), "da9")
    g = gy if slope == 1.0 else torch.where(y > 0, gy, gy * slope)
    want = g.double() @ w2.double()
    np.testing.assert_allclose(da9.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=2e-6 * float(want.abs().max()))


def test_discriminator_step_graph_equals_eager():
    """Round 6: the discriminator step's no-grad generator pass replayed from a captured HIP graph
    (``pix2pix_model._NoGradGraph``; captured on the second call per shape) against the same pass run eagerly on a copy of the
    model: the image bit for bit, over four calls with the parameters changed in place in between (as Adam does) and new inputs
    each time, then every buffer the pass updates (the power iteration's u / v, BatchNorm's running statistics); a new batch
    size starts over (eager, then captured); a deep copy of the model drops the graph."""
    import copy
    from emlight_amd.GenProjector import networks
    from emlight_amd.GenProjector.pix2pix_model import Pix2PixModel
    torch.manual_seed(11)
    opt = networks.default_options(no_vgg_loss=True)
    opt.ngf = opt.ndf = 8
    a = Pix2PixModel(opt).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(5)
    draw = lambda B: (torch.rand(B, 3, 128, 256, device="cuda", generator=g), torch.rand(B, 3, 128, 128, device="cuda", generator=g))
    b = copy.deepcopy(a)
    assert Pix2PixModel.graph_dstep, "EML_GRAPH_DSTEP=0 in the environment: nothing to test"
    for step in range(4):
        inp, crop = draw(2)
        with torch.no_grad():
            fa = a._fake_for_discriminator(inp, crop)
            fb = b.generate_fake(inp, crop)
        gr = a.__dict__["_dstep_graph"]
        assert not gr.failed, "the capture was refused"
        assert (gr.graph is not None) == (step >= 1), "eager first, captured from the second call on"
        assert torch.equal(fa, fb), "step %d" % step
        with torch.no_grad():
            for q, r in zip(a.netG.parameters(), b.netG.parameters()):   # an optimizer step's in-place update, on both
                q.mul_(1.0 + 1e-3 * (step + 1))
                r.mul_(1.0 + 1e-3 * (step + 1))
    for (n, x), (_, y) in zip(a.netG.named_buffers(), b.netG.named_buffers()):
        assert torch.equal(x, y), n
    for step in range(2):                      # another batch size: eager, then captured again
        inp, crop = draw(1)
        with torch.no_grad():
            assert torch.equal(a._fake_for_discriminator(inp, crop), b.generate_fake(inp, crop))
    assert a.__dict__["_dstep_graph"].key[0] == (1, 3, 128, 256) and a.__dict__["_dstep_graph"].graph is not None
    c = copy.deepcopy(a)
    assert c.__dict__.get("_dstep_graph") is None
    with torch.no_grad():
        inp, crop = draw(1)
        fc = c._fake_for_discriminator(inp, crop)
        assert torch.equal(fc, b.generate_fake(inp, crop)) and torch.equal(fc, a._fake_for_discriminator(inp, crop))
