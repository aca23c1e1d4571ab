"""GPU: the projector's inputs from HDR panoramas on the MI355X (csrc/projector_prep.hip) -- the light targets against their
float32 definition restated in numpy (exact), the bilinear resize against a float64 evaluation of its formula and against
``F.interpolate``, ``ProjectorPanoramaBatcher`` against the operators it chains, and the three entry points on a directory
of ``.npy`` panoramas.

Resize tolerance ``RESIZE_ATOL = 2e-6``: the result is a convex combination of four values of magnitude at most 1 with
float32 weights made from float64 positions -- at most 8 roundings of 2^-24, about 5e-7; the margin is x4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.make_golden_panorama import BATCHER, pano_inputs

pytestmark = pytest.mark.gpu

RESIZE_ATOL = 2e-6
f32 = np.float32


# ------------------------------------------------------------------------------------------------ light targets
def _expected_targets(small, alpha):
    """GenProjector/data.py:73-84 in float32, in the reference's association: every numpy operation below rounds to float32
    and nothing is contracted."""
    small = np.ascontiguousarray(small, dtype=np.float32)
    luma = (f32(.3) * small[..., 0] + f32(.59) * small[..., 1]) + f32(.11) * small[..., 2]
    assert luma.dtype == np.float32
    thr = (luma.reshape(len(luma), -1).max(axis=1) * f32(.05)).astype(np.float32)
    mask = (luma > thr[:, None, None]).astype(np.float32)[:, None]
    a = np.ones(len(small), dtype=np.float32) if alpha is None else np.asarray(alpha, dtype=np.float32)
    warped = (small * a[:, None, None, None]).transpose(0, 3, 1, 2)
    assert warped.dtype == np.float32
    return warped, mask


def _check_targets(small, alpha, name):
    from emlight_amd.GenProjector.data import light_targets
    x = torch.from_numpy(small).cuda()
    a = None if alpha is None else torch.from_numpy(alpha).cuda()
    warped, mask = light_targets(x, a)
    again_w, again_m = light_targets(x, a)
    B, h, w, _ = small.shape
    assert warped.shape == (B, 3, h, w) and mask.shape == (B, 1, h, w) and warped.dtype == mask.dtype == torch.float32
    assert torch.equal(warped, again_w) and torch.equal(mask, again_m), "%s: a second call is bit-identical" % name
    want_w, want_m = _expected_targets(small, alpha)
    got_m = mask.cpu().numpy()
    print("%s: %d of %d mask values differ, %.1f %% lit" % (name, int((got_m != want_m).sum()), want_m.size, 100 * want_m.mean()))
    np.testing.assert_array_equal(got_m, want_m, err_msg=name)
    assert np.array_equal(warped.cpu().numpy().view(np.int32), np.ascontiguousarray(want_w).view(np.int32)), name
    return warped, mask


@pytest.mark.parametrize("B,h,w", [(3, 6, 10), (2, 33, 7), (2, 128, 256)])
def test_light_targets_exact_on_uniform_images(B, h, w):
    """A pixel of 10 among U[0, 1) values: the threshold 0.5 sits at the median of the lumas, about half the mask is on.
    6 x 10: one ragged tile, 16-byte stores; 33 x 7 = 231 pixels: no multiple of 4, the dword paths and images whose base is
    not 16-byte aligned; 128 x 256: 32 tiles and 32 partial maxima per image."""
    g = np.random.default_rng([5, B, h, w])
    small = g.random((B, h, w, 3), dtype=np.float32)
    small[:, 0, 0] = 10.0
    alpha = g.uniform(0.1, 2.0, B).astype(np.float32)
    _, mask = _check_targets(small, alpha, "uniform %dx%dx%d" % (B, h, w))
    assert 0.3 < float(mask.mean()) < 0.7
    # alpha=None is alpha = 1
    from emlight_amd.GenProjector.data import light_targets
    x = torch.from_numpy(small).cuda()
    w_none, m_none = light_targets(x)
    w_ones, m_ones = light_targets(x, torch.ones(B, device="cuda"))
    assert torch.equal(w_none, w_ones) and torch.equal(m_none, m_ones) and torch.equal(m_none, mask)
    assert torch.equal(w_none, x.permute(0, 3, 1, 2))


def test_light_targets_exact_on_heavy_tailed_panoramas_and_edge_images():
    small = pano_inputs(3, 128, 256, 41)
    alpha = np.asarray([0.37, 1.0, 0.0123], dtype=np.float32)
    _check_targets(small, alpha, "heavy-tailed")
    _check_targets(small, None, "heavy-tailed, no alpha")
    # an all-zero image: nothing is above 0; a constant positive image: everything is above 5 % of itself; the images next to
    # them keep their own threshold
    edge = np.random.default_rng(6).random((4, 9, 13, 3), dtype=np.float32)
    edge[1] = 0.0
    edge[2] = 0.731
    _, mask = _check_targets(edge, np.asarray([1.5, 2.0, 0.5, 1.0], dtype=np.float32), "edge images")
    assert float(mask[1].max()) == 0.0 and float(mask[2].min()) == 1.0
    _, m1 = _check_targets(np.ascontiguousarray(edge[:1, :1, :1]), None, "a single pixel")
    assert m1.shape == (1, 1, 1, 1) and float(m1.min()) == 1.0
    from emlight_amd.GenProjector.data import light_targets
    empty_w, empty_m = light_targets(torch.empty(0, 4, 4, 3, device="cuda"))
    assert empty_w.shape == (0, 3, 4, 4) and empty_m.shape == (0, 1, 4, 4)


# ------------------------------------------------------------------------------------------------ resize
def _cell(n_in, n_out):
    pos = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(pos).astype(np.int64)
    wgt = pos - i0
    low, high = pos < 0, i0 >= n_in - 1
    i0[low], wgt[low] = 0, 0.0
    i0[high], wgt[high] = n_in - 1, 0.0
    return i0, np.minimum(i0 + 1, n_in - 1), wgt


def _bilinear_f64(x, oh, ow):
    """The formula of cv2 INTER_LINEAR / F.interpolate(align_corners=False) in float64: horizontal, then vertical."""
    x = x.astype(np.float64)
    r0, r1, wy = _cell(x.shape[2], oh)
    c0, c1, wx = _cell(x.shape[3], ow)
    top = x[:, :, r0][..., c0] * (1 - wx) + x[:, :, r0][..., c1] * wx
    bot = x[:, :, r1][..., c0] * (1 - wx) + x[:, :, r1][..., c1] * wx
    return top * (1 - wy)[:, None] + bot * wy[:, None]


@pytest.mark.parametrize("B,h,w,oh,ow", [(3, 24, 32, 128, 128), (2, 192, 256, 128, 128), (1, 7, 5, 4, 9)])
def test_resize_bilinear_matches_its_formula_and_interpolate(B, h, w, oh, ow):
    from emlight_amd.GenProjector.data import resize_bilinear
    x = np.random.default_rng([7, h, w]).random((B, 3, h, w), dtype=np.float32)
    xd = torch.from_numpy(x).cuda()
    got = resize_bilinear(xd, (oh, ow))
    assert got.shape == (B, 3, oh, ow) and got.dtype == torch.float32 and torch.equal(got, resize_bilinear(xd, (oh, ow)))
    want = _bilinear_f64(x, oh, ow)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    torch_err = float((got - F.interpolate(xd, size=(oh, ow), mode="bilinear", align_corners=False)).abs().max())
    print("resize %dx%d -> %dx%d: worst |error| %.3e vs float64, %.3e vs F.interpolate (bound %.1e)"
          % (h, w, oh, ow, err, torch_err, RESIZE_ATOL))
    assert err <= RESIZE_ATOL
    assert torch_err <= RESIZE_ATOL
    # the identity size returns the taps bit for bit (signed zeros and huge values included)
    y = xd.clone()
    y[0, 0, 0, :2] = torch.tensor([-0.0, 3.0e38], device="cuda")
    same = resize_bilinear(y, (h, w))
    assert torch.equal(same.view(torch.int32), y.view(torch.int32))


def test_resize_with_alpha_and_clip_is_the_resized_tonemap():
    """The 128 x 128 tonemapped crop from the tonemap's P and alpha, without the full-size tonemapped image."""
    from emlight_amd.GenProjector.data import resize_bilinear
    from emlight_amd.RegressionNetwork.util import TonemapHDR, tonemap_raw
    hdr = torch.from_numpy(np.ascontiguousarray(pano_inputs(2, 48, 64, 9).transpose(0, 3, 1, 2))).cuda()
    out, alpha = TonemapHDR(2.4, 50, 0.5)(hdr)
    assert float(out.max()) == 1.0 and float(out.min()) >= 0.0               # the clip bites on these images
    raw = tonemap_raw(hdr, 2.4, 50, 0.5, apply=False)
    assert raw["out"] is None and torch.equal(raw["alpha"], alpha)
    got = resize_bilinear(raw["P"], (128, 128), alpha=raw["alpha"], clip=True)
    want = resize_bilinear(out, (128, 128))
    err = float((got - want).abs().max())
    print("alpha + clip taps vs the resized tonemap: worst |difference| %.3e" % err)
    assert err <= RESIZE_ATOL
    assert torch.equal(resize_bilinear(raw["P"], (48, 64), alpha=raw["alpha"], clip=True), out)
    unclipped = resize_bilinear(raw["P"], (48, 64), alpha=raw["alpha"])
    assert torch.equal(unclipped, raw["P"] * raw["alpha"].view(2, 1, 1, 1)) and float(unclipped.max()) > 1.0
    assert resize_bilinear(torch.empty(0, 3, 4, 4, device="cuda"), (2, 2)).shape == (0, 3, 2, 2)


# ------------------------------------------------------------------------------------------------ batcher
def _batcher(regression=False, seed=1234):
    from emlight_amd.GenProjector.data import ProjectorPanoramaBatcher
    return ProjectorPanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], seed=seed,
                                    regression=regression)


@pytest.fixture(scope="module")
def recipe():
    cfg = BATCHER
    panos = torch.from_numpy(pano_inputs(cfg["B"], cfg["HW"][0], cfg["HW"][1], cfg["seed"])).cuda()
    deg = torch.tensor(cfg["deg"], device="cuda", dtype=torch.float64)
    return panos, deg, _batcher()(panos, deg=deg), _batcher(regression=True)(panos, deg=deg)


def test_batcher_outputs_are_the_chained_operators(recipe):
    from emlight_amd import joint
    from emlight_amd.GenProjector.data import resize_bilinear
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    from emlight_amd.RegressionNetwork.util import PanoramaHandler, TonemapHDR
    cfg = BATCHER
    panos, deg, out, full = recipe
    B = cfg["B"]
    assert {k: tuple(v.shape) for k, v in out.items()} == {
        "input": (B, 3, 128, 256), "crop": (B, 3, 128, 128), "warped": (B, 3, 128, 256), "map": (B, 1, 128, 256),
        "pano": (B, 128, 256, 3), "alpha": (B,)}
    reg = PanoramaBatcher(anchors=cfg["anchors"], crop_hw=cfg["crop_hw"], fov_deg=cfg["fov"])(panos, deg=deg)
    assert torch.equal(out["alpha"], reg["alpha"]), "alpha is PanoramaBatcher's, bit for bit"
    assert torch.equal(out["pano"], PanoramaHandler.resize_panorama(panos, (256, 128), deg=deg))
    want_w, want_m = _expected_targets(out["pano"].cpu().numpy(), out["alpha"].cpu().numpy())
    np.testing.assert_array_equal(out["map"].cpu().numpy(), want_m)
    assert np.array_equal(out["warped"].cpu().numpy().view(np.int32), np.ascontiguousarray(want_w).view(np.int32))
    assert 0 < float(out["map"].mean()) < 0.5                                 # the saturated patches, not the background
    raw_crop = PanoramaHandler.crop_panorama(panos, cfg["fov"], cfg["crop_hw"][0], "4:3", deg=deg)
    want_crop = resize_bilinear(TonemapHDR(2.4, 50, .5)(raw_crop)[0], (128, 128))
    err = float((out["crop"] - want_crop).abs().max())
    print("crop vs the resized tonemapped crop: worst |difference| %.3e" % err)
    assert err <= RESIZE_ATOL
    # regression=True: PanoramaBatcher's keys bit for bit, the encoder's crop under `crop`, the projector's under `crop128`
    for k in ("crop", "distribution", "intensity", "rgb_ratio", "ambient", "alpha"):
        assert torch.equal(full[k], reg[k]), k
    for k in ("input", "warped", "map", "pano"):
        assert torch.equal(full[k], out[k]), k
    assert torch.equal(full["crop128"], out["crop"])
    # the guide map of the ground-truth parameters is the joint step's map of the regression targets: the two differ by a
    # handful of float32 roundings of non-negative factors (<= 1e-6); the bound catches a wrong 0.01, 500 or 128 * 256
    want_in = joint.predicted_gaussian_map(full, cfg["anchors"])
    top = float(want_in.max())
    err = float((out["input"] - want_in).abs().max())
    print("input vs predicted_gaussian_map of the regression keys: worst |difference| %.3e, max %.3e" % (err, top))
    assert top > 0
    assert torch.allclose(out["input"], want_in, rtol=1e-5, atol=1e-5 * top)


def test_batcher_seeded_views_independent_images_and_no_host_sync():
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    B = 4
    panos = torch.from_numpy(pano_inputs(B, 256, 512, 33)).cuda()
    a, b = _batcher(seed=7), _batcher(seed=7)
    first, second = a(panos), a(panos)
    again = b(panos)
    for k in first:
        assert torch.equal(first[k], again[k]), "the same seed gives the same batch: %s" % k
    assert not torch.equal(first["crop"], second["crop"]), "a fresh view per step"
    # the views are PanoramaBatcher's: same generator, same seed, one azimuth per sample
    reg = PanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], seed=7)
    degs = reg.random_deg(B)
    assert torch.equal(_batcher(seed=7).random_deg(B), degs)
    assert torch.equal(first["alpha"], PanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"],
                                                       fov_deg=BATCHER["fov"], seed=7)(panos)["alpha"])
    for i in (0, 3):                                             # sample i of the batch is the same panorama run alone
        alone = _batcher()(panos[i:i + 1], deg=degs[i:i + 1])
        for k in first:
            assert torch.equal(alone[k][0], first[k][i]), k
    # the call only enqueues: with synchronising calls turned into errors it still runs (the probe shows the mode bites)
    bt, btr = _batcher(seed=9), _batcher(regression=True, seed=9)
    bt(panos)                                                    # allocator warm-up, generator and anchor-table creation
    btr(panos)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                  # the mode is effective on this build
        out = bt(panos)
        out2 = btr(panos, deg=12.5, fov_deg=90.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert all(bool(torch.isfinite(v).all()) for v in out2.values())


# ------------------------------------------------------------------------------------------------ entry points
@pytest.fixture(scope="module")
def pano_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("panos")
    for i, p in enumerate(pano_inputs(3, 256, 512, 55)):
        np.save(str(d / ("room%d.npy" % i)), p)
    return d


def test_projector_train_and_test_on_a_panorama_directory(pano_dir, tmp_path):
    from emlight_amd.GenProjector import test as gp_test
    from emlight_amd.GenProjector import train as gp_train
    ckpt, results = str(tmp_path / "ckpt"), str(tmp_path / "results")
    losses = gp_train.main(["--pano_dir", str(pano_dir), "--batchSize", "2", "--max_iters", "2", "--ngf", "8", "--ndf", "8",
                            "--checkpoints_dir", ckpt, "--name", "pano", "--dataset_mode", "lavalindoor", "--display_freq", "7"])
    assert losses and all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    print({k: round(float(v.detach().mean()), 4) for k, v in losses.items()})
    assert os.path.exists(os.path.join(ckpt, "pano", "latest_net_G.pth"))
    gp_test.main(["--pano_dir", str(pano_dir), "--batchSize", "2", "--ngf", "8", "--checkpoints_dir", ckpt, "--name", "pano",
                  "--results_dir", results])
    for i in range(3):
        pred = np.load(os.path.join(results, "pred_room%d.npy" % i))
        assert pred.shape == (1, 3, 128, 256) and pred.dtype == np.float32 and np.isfinite(pred).all()
    assert len(os.listdir(results)) == 3


def test_joint_step_on_the_batchers_output():
    from emlight_amd.GenProjector import networks
    from emlight_amd.GenProjector.data import ProjectorPanoramaBatcher
    from emlight_amd.joint import JointTrainer
    panos = torch.from_numpy(pano_inputs(2, 256, 512, 56)).cuda()
    batch = ProjectorPanoramaBatcher(regression=True, crop_hw=(32, 64), anchors=32)(panos)
    assert batch["crop"].shape == (2, 3, 32, 64) and batch["crop128"].shape == (2, 3, 128, 128)
    tr = JointTrainer(networks.default_options(ngf=8, ndf=8), anchors=32, crop_hw=(32, 64), device="cuda:0")
    losses = tr.step(batch)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    assert any(float(p.grad.abs().max()) > 0 for p in tr.reg.model.parameters() if p.grad is not None), "encoder"
    assert any(float(p.grad.abs().max()) > 0 for p in tr.proj.model.netG.parameters() if p.grad is not None), "generator"
