"""GPU: HDR panorama -> training batch on the MI355X (csrc/pano_prep.hip) -- the perspective crop with its folded rotation and
the tonemap against vectors of the REAL reference (``tests/golden/make_golden_panorama.py``), the area resize against its
float64 definition, the radix select against ``np.partition`` bit for bit, and the ``PanoramaBatcher`` end to end.

The device's ``powf`` is the one float32 operation here that is not correctly rounded.  The ROCm device-library
documentation that states its ulp bound is not shipped with the toolchain this was developed on, so the bound is taken
from a measurement: the worst distance between the device's ``P = I^(1/gamma)`` and ``np.power`` over the inputs of this
file (the golden tonemap inputs, the batcher's crops, 64 x 3 x 240 x 320 heavy-tailed values, gamma 2.4) was
POW_ULP_MEASURED ulp; ``POW_ULP`` is twice that.  The tolerance on alpha and on the tonemapped output is
``(2 * POW_ULP + 4) * 2^-23``."""
import numpy as np
import pytest
import torch

from tests.conftest import Golden
from tests.golden.make_golden_panorama import (BATCHER, CROP_CASES, TONE_CASES, TONE_SETTINGS, box_mean, pano_inputs,
                                               tone_inputs)

pytestmark = pytest.mark.gpu

POW_ULP_MEASURED = 2
POW_ULP = 2 * POW_ULP_MEASURED
TONE_RTOL = (2 * POW_ULP + 4) * 2.0 ** -23


def _ulp_distance(a, b):
    """Distance in float32 ulp between arrays of non-negative floats (their bit patterns order as the values)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def golden():
    return Golden("panorama_prep")


# ------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("case", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_crop_with_folded_rotation_matches_reference(golden, case):
    """rtol 1e-6, atol 0: the output is a convex combination of four non-negative float32 values with weights rounded
    from float64 -- no cancellation, a few float32 ulp of the result."""
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    name, (H, W), seed, fov, h, aspect, deg, u8 = case
    pano = torch.from_numpy(pano_inputs(1, H, W, seed, uint8=u8)[0]).cuda()
    got = PanoramaHandler.crop_panorama(pano, fov, h, aspect, deg=deg)
    want = golden["crop/%s" % name]
    assert got.shape == want.shape and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    print("crop %s: worst relative error %.3e" % (name, err[want != 0].max()))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=0)
    # the rotation folded into the gather is the rolled copy, bit for bit; so is a per-sample tensor of the same values
    rolled = PanoramaHandler.horizontal_rotate_panorama(pano, deg)
    assert torch.equal(rolled, torch.roll(pano, int(deg / 360.0 * W), dims=1))
    assert torch.equal(got, PanoramaHandler.crop_panorama(rolled, fov, h, aspect))
    per_sample = PanoramaHandler.crop_panorama(pano[None], torch.tensor([fov], device="cuda"), h, aspect,
                                               deg=torch.tensor([deg], device="cuda", dtype=torch.float64))
    assert torch.equal(per_sample[0], got)


def test_crop_batch_shared_and_per_sample_paths_agree():
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    B = 11                                          # more than one run of images per thread, and a ragged last run
    pano = torch.from_numpy(pano_inputs(B, 64, 128, 3)).cuda()
    degs = torch.linspace(-400.0, 800.0, B, dtype=torch.float64, device="cuda")
    shared = PanoramaHandler.crop_panorama(pano, 90.0, 24, "4:3", deg=degs)
    per = PanoramaHandler.crop_panorama(pano, torch.full((B,), 90.0, device="cuda"), 24, "4:3", deg=degs)
    assert torch.equal(shared, per)
    for b in (0, 4, 10):
        alone = PanoramaHandler.crop_panorama(pano[b], 90.0, 24, "4:3", deg=float(degs[b]))
        assert torch.equal(alone, shared[b])
    # a per-sample fov cannot be checked on the host: its out-of-range samples are NaN, the other image is untouched
    fovs = torch.tensor([170.0, 60.0], device="cuda")
    out = PanoramaHandler.crop_panorama(pano[:2], fovs, 26, "1:2")
    assert bool(torch.isnan(out[0]).any()) and not bool(torch.isnan(out[1]).any())
    assert torch.equal(out[1], PanoramaHandler.crop_panorama(pano[1], 60.0, 26, "1:2"))
    with pytest.raises(ValueError):
        PanoramaHandler.crop_panorama(pano[:2], 170.0, 26, "1:2")


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("H,W,h,w", [(256, 512, 128, 256), (64, 128, 16, 16), (48, 96, 48, 96), (60, 120, 20, 24), (30, 90, 10, 18),
                                     (512, 1024, 8, 16), (1024, 2048, 128, 256)])
def test_resize_is_the_box_mean_of_the_rolled_input(H, W, h, w):
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    B = 3
    x = torch.from_numpy(pano_inputs(B, H, W, 7)).cuda()
    degs = [0.0, 77.3, -45.0]
    got = PanoramaHandler.resize_panorama(x, (w, h), deg=torch.tensor(degs, device="cuda"))
    again = PanoramaHandler.resize_panorama(x, (w, h), deg=torch.tensor(degs, device="cuda"))
    assert torch.equal(got, again), "a fixed-order f64 sum is run-to-run exact"
    for b in range(B):
        rolled = torch.roll(x[b], int(degs[b] / 360.0 * W), dims=1)
        want = rolled.double().reshape(h, H // h, w, W // w, 3).mean(dim=(1, 3)).float()
        d = _ulp_distance(got[b].cpu().numpy(), want.cpu().numpy())
        print("resize %dx%d->%dx%d image %d: worst %d ulp" % (H, W, h, w, b, d.max()))
        assert d.max() <= 2
        assert torch.equal(got[b], PanoramaHandler.resize_panorama(x[b], (w, h), deg=degs[b]))
    np.testing.assert_array_equal(PanoramaHandler.resize_panorama(x[0], (w, h)).cpu().numpy()[:1, :1],
                                  box_mean(x[0].cpu().numpy(), h, w)[:1, :1])


# ------------------------------------------------------------------------------------------------ selection
def _selection_images(h=16, w=20, seed=5):
    """One batch whose images stress the select: heavy-tailed, n = 1, n = 2, all values equal, ties at every rank,
    all zero, mostly zero (a very different n), +a wide dynamic range."""
    g = np.random.default_rng(seed)
    n = 3 * h * w
    imgs = np.zeros((8, n), dtype=np.float32)
    imgs[0] = g.random(n) ** 8 * 50
    imgs[1, 17] = 3.25                                           # n = 1
    imgs[2, [5, 900]] = (0.5, 7.0)                               # n = 2
    imgs[3] = 0.731                                              # all equal
    imgs[4] = g.integers(1, 6, n).astype(np.float32) / 4         # five distinct values: ties at the selected rank
    imgs[6, g.choice(n, 37, replace=False)] = g.random(37) * 9   # n = 37 next to images with n = 960
    imgs[7] = np.exp(g.uniform(-80, 80, n)).astype(np.float32)   # every exponent bin
    return imgs.reshape(8, 3, h, w)


def _check_selection(raw, q):
    P = raw["P"].cpu().numpy()
    n_dev, lo, hi, r = (raw[k].cpu().numpy() for k in ("n", "lo", "hi", "r"))
    worst = 0
    for b in range(P.shape[0]):
        pos = P[b][P[b] > 0]
        assert n_dev[b] == pos.size, "image %d: n" % b
        if pos.size == 0:
            assert lo[b] == 0 and hi[b] == 0 and r[b] == 0
            continue
        # numpy forms the virtual index of an f32 array in f32: f32(n - 1) * (f32(q) / f32(100)); >= n - 1 takes the maximum
        vi = np.float32(pos.size - 1) * (np.float32(q) / np.float32(100))
        k = pos.size - 1 if vi >= np.float32(pos.size - 1) else int(np.floor(vi))
        k1 = min(k + 1, pos.size - 1)
        part = np.partition(pos, [k, k1])
        assert lo[b].view(np.int32) == part[k].view(np.int32), "image %d q %g: order statistic %d" % (b, q, k)
        assert hi[b].view(np.int32) == part[k1].view(np.int32), "image %d q %g: order statistic %d" % (b, q, k1)
        d = int(_ulp_distance(r[b:b + 1], np.asarray([np.percentile(pos, q)], dtype=np.float32))[0])
        worst = max(worst, d)
        assert d <= 2, "image %d q %g: r is %d ulp off np.percentile" % (b, q, d)
    return worst


@pytest.mark.parametrize("q", [50, 99, 90, 0, 100, 37.5])
@pytest.mark.parametrize("use_gamma", [True, False])
def test_selection_is_exact(q, use_gamma):
    from emlight_amd.RegressionNetwork.util import tonemap_raw
    x = torch.from_numpy(_selection_images()).cuda()
    raw = tonemap_raw(x, gamma=2.4, percentile=q, max_mapping=0.5, use_gamma=use_gamma)
    again = tonemap_raw(x, gamma=2.4, percentile=q, max_mapping=0.5, use_gamma=use_gamma)
    for k in ("out", "n", "lo", "hi", "r", "alpha"):
        assert torch.equal(raw[k], again[k]), "integer counts are order-free: %s must be bit-reproducible" % k
    print("q=%g gamma=%s: r worst %d ulp off np.percentile" % (q, use_gamma, _check_selection(raw, q)))
    # images of a batch do not touch each other: each one alone gives the same raw outputs
    for b in (1, 4, 5, 6):
        one = tonemap_raw(x[b:b + 1], gamma=2.4, percentile=q, max_mapping=0.5, use_gamma=use_gamma)
        for k in ("out", "n", "lo", "hi", "r", "alpha"):
            assert torch.equal(one[k][0], raw[k][b]), k


def test_selection_odd_sizes_and_unfriendly_values():
    """A size that is no multiple of 4 (the dword path), and negative / NaN / inf input: no fault, and the images next to
    it keep their results."""
    from emlight_amd.RegressionNetwork.util import tonemap_raw
    g = np.random.default_rng(8)
    x = (g.random((5, 3, 7, 11)) ** 6 * 20).astype(np.float32)
    raw = tonemap_raw(torch.from_numpy(x).cuda(), percentile=90, use_gamma=False)
    _check_selection(raw, 90)
    bad = x.copy()
    bad[2, 0, 0, :4] = (-1.0, np.nan, np.inf, -np.inf)
    rb = tonemap_raw(torch.from_numpy(bad).cuda(), percentile=90, use_gamma=False)
    for b in (0, 1, 3, 4):
        for k in ("out", "n", "lo", "hi", "r", "alpha"):
            assert torch.equal(rb[k][b], raw[k][b])
    assert int(rb["n"][2]) == int(raw["n"][2]) - 3               # -1, NaN and -inf are not positive; +inf is


def test_selection_batch_of_64_at_cfg2_size():
    from emlight_amd.RegressionNetwork.util import tonemap_raw
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(64, 3, 240, 320, generator=gen, device="cuda") ** 8 * 50
    x[5, :, 100:] = 0                                            # a very different n
    x[9] = 0
    for q in (50, 99):
        raw = tonemap_raw(x, gamma=2.4, percentile=q, max_mapping=0.5)
        print("64 x 3 x 240 x 320, q=%d: r worst %d ulp off np.percentile" % (q, _check_selection(raw, q)))
        host_pow = np.power(x.cpu().numpy(), np.float32(1 / 2.4))
        print("  device pow vs np.power: worst %d ulp" % _ulp_distance(raw["P"].cpu().numpy(), host_pow).max())
        assert _ulp_distance(raw["P"].cpu().numpy(), host_pow).max() <= POW_ULP


# ------------------------------------------------------------------------------------------------ tonemap
@pytest.mark.parametrize("case", TONE_CASES, ids=[c[0] for c in TONE_CASES])
def test_tonemap_matches_reference(golden, case):
    """alpha and the output within ``(2 U + 4) * 2^-23`` (relative): the one float32 difference beyond rounding is the
    device's pow (U ulp); an order statistic moves by at most the largest per-element perturbation, so another element
    at the selected rank is no failure."""
    from emlight_amd.RegressionNetwork.util import TonemapHDR
    name, kind, si, kw = case
    x = tone_inputs(kind)
    tone = TonemapHDR(*TONE_SETTINGS[si])
    out, alpha = tone(torch.from_numpy(x).cuda(), **kw)
    assert out.shape == x.shape and alpha.shape == ()
    want, walpha = golden["tone/%s/out" % name], float(golden["tone/%s/alpha" % name])
    got = out.cpu().numpy()
    nz = want != 0
    rel = np.abs(got[nz].astype(np.float64) - want[nz]) / want[nz] if nz.any() else np.zeros(1)
    print("tone %s: alpha %.9g vs %.9g (rel %.2e), output worst rel %.2e, bound %.2e"
          % (name, float(alpha), walpha, abs(float(alpha) - walpha) / walpha, rel.max(), TONE_RTOL))
    np.testing.assert_allclose(float(alpha), walpha, rtol=TONE_RTOL, atol=0)
    np.testing.assert_allclose(got, want, rtol=TONE_RTOL, atol=0)
    if kw.get("gamma", True) and tone.gamma != 1.0:
        P = np.power(x, np.float32(1 / tone.gamma))
        from emlight_amd.RegressionNetwork.util import tonemap_raw
        d = _ulp_distance(tonemap_raw(torch.from_numpy(x[None]).cuda(), gamma=tone.gamma)["P"][0].cpu().numpy(), P).max()
        print("  device pow vs np.power: worst %d ulp" % d)
        assert d <= POW_ULP
    # a batch holding the image twice gives it twice, and the numpy path still is the host's
    both, alphas = tone(torch.from_numpy(np.stack([x, x])).cuda(), **kw)
    assert torch.equal(both[0], out) and torch.equal(both[1], out) and torch.equal(alphas[0], alpha)
    host, halpha = tone(x, **kw)
    assert isinstance(host, np.ndarray) and np.array_equal(host, want) and float(halpha) == walpha


# ------------------------------------------------------------------------------------------------ batcher
def _batcher(seed=1234):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], seed=seed)


def test_batcher_matches_reference_chain(golden):
    """crop as the tonemap check.  distribution / rgb_ratio: extract_mesh's tolerances of ``test_gpu_gt_param.py`` (rtol
    1e-10, atol 1e-12) plus one float32 rounding (2^-23: the batcher returns the float32 the training step reads, the
    vectors hold float64).  intensity / ambient are those times alpha: alpha's tolerance on top, and one more float32
    rounding for each of the product and the quotient."""
    cfg = BATCHER
    panos = torch.from_numpy(pano_inputs(cfg["B"], cfg["HW"][0], cfg["HW"][1], cfg["seed"])).cuda()
    out = _batcher()(panos, deg=torch.tensor(cfg["deg"], device="cuda", dtype=torch.float64))
    f32 = 2.0 ** -23
    for b in range(cfg["B"]):
        g = golden.case("batch/%d" % b)
        np.testing.assert_allclose(float(out["alpha"][b]), float(g["alpha"]), rtol=TONE_RTOL, atol=0)
        np.testing.assert_allclose(out["crop"][b].cpu().numpy(), g["crop"], rtol=TONE_RTOL, atol=0)
        for k in ("distribution", "rgb_ratio"):
            np.testing.assert_allclose(out[k][b].cpu().numpy(), g[k], rtol=1e-10 + f32, atol=1e-12, err_msg=k)
        for k in ("intensity", "ambient"):
            got = out[k][b].cpu().numpy().reshape(-1)
            print("batch %d %s: %s vs %s" % (b, k, got, g[k].reshape(-1)))
            np.testing.assert_allclose(got, g[k].reshape(-1), rtol=TONE_RTOL + 1e-10 + 3 * f32, atol=1e-12, err_msg=k)
    # a Python number for the batch is the tensor of that number
    same = _batcher()(panos, deg=77.3)
    alone = _batcher()(panos[:1], deg=torch.tensor([77.3], device="cuda"))
    for k in out:
        assert torch.equal(same[k][0], out[k][0]) and torch.equal(alone[k][0], out[k][0]), k


def test_batcher_seeded_views_independent_images_and_no_host_sync():
    B = 6
    panos = torch.from_numpy(pano_inputs(B, 256, 512, 33)).cuda()
    a, b = _batcher(seed=7), _batcher(seed=7)
    first, second = a(panos), a(panos)
    again = b(panos)
    for k in first:
        assert torch.equal(first[k], again[k]), "the same seed gives the same views: %s" % k
    assert not torch.equal(first["crop"], second["crop"]), "a fresh view per step"
    degs = _batcher(seed=7).random_deg(B)
    assert degs.dtype == torch.float64 and degs.is_cuda and bool(((degs >= 0) & (degs < 360)).all())
    assert len(set(degs.tolist())) == B
    # images of a batch are independent: sample i of the batch is the same panorama run alone
    for i in (0, 3, 5):
        alone = _batcher()(panos[i:i + 1], deg=degs[i:i + 1])
        for k in first:
            assert torch.equal(alone[k][0], first[k][i]), k
    # the call only enqueues: with synchronising calls turned into errors it still runs (the probe shows the mode bites)
    bt = _batcher(seed=9)
    bt(panos)                                                    # allocator warm-up, generator creation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()                  # the mode is effective on this build
        out = bt(panos)
        out2 = bt(panos, deg=12.5, fov_deg=90.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out["crop"]).all()) and bool(torch.isfinite(out2["ambient"]).all())


def test_full_size_batch_feeds_one_engine_step():
    """B = 64 panoramas of 1024 x 2048 -> 240 x 320 crops and targets, then one training step on the result."""
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    B, anchors = 64, 96
    gen = torch.Generator(device="cuda").manual_seed(11)
    panos = torch.rand(B, 1024, 2048, 3, generator=gen, device="cuda") ** 8 * 50
    for b in range(B):
        y0, x0 = 37 * b % 900, 131 * b % 1900
        panos[b, y0:y0 + 48, x0:x0 + 96] = 1500.0 + 40.0 * b      # a saturated light
    batch = PanoramaBatcher(anchors=anchors, crop_hw=(240, 320), fov_deg=60.0)(panos)
    del panos
    for k, v in batch.items():
        assert bool(torch.isfinite(v).all()), k
    crop = batch["crop"]
    assert crop.shape == (B, 3, 240, 320) and float(crop.min()) >= 0 and float(crop.max()) <= 1
    worst = 0.0
    for b in range(B):
        c = crop[b].cpu().numpy()
        worst = max(worst, abs(float(np.percentile(c[c > 0], 50)) - 0.5))
    print("median of the positive crop values: worst |median - 0.5| = %.3e" % worst)
    # alpha = max_mapping / (r + 1e-10) with r the median of P: alpha * P keeps the order, so the median of the output is
    # alpha * r up to one float32 rounding per factor and the 1e-10 (r here is ~0.3)
    assert worst <= 0.5 * (4 * 2.0 ** -23 + 1e-9)
    assert torch.allclose(batch["distribution"].sum(1), torch.ones(B, device="cuda"), atol=1e-5)
    tr = RegressionTrainer(anchors=anchors, crop_hw=(240, 320))
    loss, terms = tr.step({k: v for k, v in batch.items() if k != "alpha"})
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in terms.values())
