"""GPU: the depth-aware panorama warp (csrc/pano_warp_depth.hip) and the per-anchor depth (csrc/gt_param.hip) on the MI355X
against ``tests/pano_depth_oracle.py``, the float64 restatement that ``test_pano_depth_abi.py`` pins to an analytic scene.

Bounds
* ``t``: the kernel and the oracle run the same march and the same bisection; they end in the same interval of width
  ``(t_hi - t_lo) / (steps 2^bisections)`` unless a rounding difference between the two libms flips a comparison
  ``g(mid) >= 0``, which happens only where ``g(mid)`` is within rounding of 0, i.e. the root is at ``mid`` itself; the two then
  end in the two intervals next to ``mid``.  So ``|t_gpu - t_oracle| <= 2 (t_hi - t_lo) / (steps 2^bisections)``, on all but at
  most 0.1 % of the pixels (``test_pano_depth_abi.py`` shows that the oracle itself moves by no more under a 2^-50 perturbation
  of ``g`` at these shapes and viewpoints).
* positions: chord distance on the sphere between the exported ``(row, col)`` and the oracle's position of ``c + t_gpu e``, at
  most ``1e-7``, the bound and the reasoning of ``test_gpu_pano_warp.py``.
* ``out_depth`` is ``float32(t)`` bit for bit; ``out_pano`` is the oracle's clamped-row bilinear sample AT THE EXPORTED
  POSITIONS to 1 float32 ulp (the same four float64 products in the same order, rounded once).
* everything about batches, parameters passed by value or per sample and absent outputs is bit for bit.
* ``anchor_depth``: relative error at most 1e-11 against the float64 restatement: a cell has at most 32768 positive terms and a
  tree or a sequential sum of n positive terms is off by at most n 2^-53 relative, 3.6e-12 for each of the two sums."""
import numpy as np
import pytest
import torch

from tests import pano_depth_oracle as oracle
from tests import warp_oracle

pytestmark = pytest.mark.gpu

SHAPES, PARAMS = oracle.GPU_SHAPES, oracle.GPU_PARAMS
CHORD_BOUND = 1e-7


def _handler():
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    return PanoramaHandler


def _ulps(a, b):
    ia, ib = np.ascontiguousarray(a).view(np.int32).astype(np.int64), np.ascontiguousarray(b).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def _bits_equal(a, b):
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _prm(params=PARAMS):
    return torch.tensor(params, dtype=torch.float64, device="cuda")


def _scene(H, W, sphere, B=3):
    """B copies of the scene with different brightness: a batch index that is off shows in the colours."""
    pano, depth = oracle.source(H, W, sphere)
    panos = np.stack([pano * (1.0 + 0.5 * b) for b in range(B)]).astype(np.float32)
    return panos, np.stack([depth] * B)


@pytest.fixture(scope="module")
def runs():
    """Every (scene, shape, steps) case once, per-sample parameters: the inputs, the kernel's three outputs, the oracle's search."""
    warp = _handler().warp_panorama_depth
    made = []
    for sphere in (False, True):
        for shape in SHAPES:
            H, W, h, w = shape
            panos, depths = _scene(H, W, sphere)
            for steps in (8, 32):
                p = _prm()
                out = warp(torch.from_numpy(panos).cuda(), torch.from_numpy(depths).cuda(), (w, h), theta=p[:, 0], phi=p[:, 1],
                           move=p[:, 2], steps=steps, return_hit=True)
                made.append((sphere, shape, steps, panos, depths, out))
    torch.cuda.synchronize()
    result = []
    for sphere, shape, steps, panos, depths, (out, out_d, hit) in made:
        H, W, h, w = shape
        assert out.shape == (3, h, w, 3) and out_d.shape == (3, h, w) and hit.shape == (3, h, w, 3)
        assert out.dtype == out_d.dtype == torch.float32 and hit.dtype == torch.float64
        want = [oracle.warp(depths[b], h, w, *PARAMS[b], steps=steps) for b in range(3)]
        result.append({"sphere": sphere, "shape": shape, "steps": steps, "panos": panos, "depths": depths, "out": out.cpu().numpy(),
                       "out_d": out_d.cpu().numpy(), "hit": hit.cpu().numpy(), "want": want})
    return result


def test_hit_against_the_oracle(runs):
    worst_t, worst_chord, missed = 0.0, 0.0, 0
    for r in runs:
        H, W, h, w = r["shape"]
        for b in range(3):
            want, hit = r["want"][b], r["hit"][b]
            assert want["valid"] and np.isfinite(hit).all(), (r["sphere"], r["shape"], b)
            tol = oracle.tolerance(want, r["steps"])
            err = np.abs(hit[..., 0] - want["t"])
            good = err <= tol
            missed += int((~good).sum())
            print("sphere %d %-16s steps %2d sample %d: worst |t - oracle| %.3e (bound %.3e), %d pixels beyond it"
                  % (r["sphere"], r["shape"], r["steps"], b, err.max(), tol, int((~good).sum())))
            assert (~good).sum() <= 0.001 * good.size, (r["sphere"], r["shape"], r["steps"], b)
            worst_t = max(worst_t, float(err[good].max() / tol))
            # the exported position is the position of c + t e, with the kernel's own t
            e, m = oracle.frame(h, w, PARAMS[b][0], PARAMS[b][1])
            row, col, _, ok = oracle.position(PARAMS[b][2] * m + hit[..., 0].reshape(-1, 1) * e, H, W)
            assert ok.all()
            g = good.reshape(-1)
            d = warp_oracle.chord(hit[..., 1].reshape(-1)[g], hit[..., 2].reshape(-1)[g], row[g], col[g], H, W)
            worst_chord = max(worst_chord, d)
            assert d <= CHORD_BOUND, (r["sphere"], r["shape"], r["steps"], b, d)
            assert hit[..., 1].min() >= 0 and hit[..., 1].max() <= H and hit[..., 2].min() >= 0 and hit[..., 2].max() <= W
    print("worst |t - oracle| %.3f of the bound, worst chord %.3e, %d pixels beyond the bound in all" % (worst_t, worst_chord, missed))
    # the three samples differ (their parameters do)
    assert not np.array_equal(runs[0]["hit"][0], runs[0]["hit"][1])


def test_outputs_against_the_hit_list(runs):
    worst = 0
    for r in runs:
        for b in range(3):
            hit = r["hit"][b]
            want_d = hit[..., 0].astype(np.float32)
            assert np.array_equal(r["out_d"][b].view(np.int32), want_d.view(np.int32)), (r["shape"], b)
            want = oracle.sample(r["panos"][b], hit[..., 1], hit[..., 2])
            assert np.isfinite(r["out"][b]).all()
            u = _ulps(r["out"][b], want)
            worst = max(worst, u)
            assert u <= 1, (r["sphere"], r["shape"], r["steps"], b, u)
    print("worst distance to the oracle's sample at the exported positions: %d ulp" % worst)
    # rows past H - 1 occur (the clamp is exercised) and the brightness tells the samples apart
    assert any((r["hit"][..., 1] > r["shape"][0] - 1).any() for r in runs)
    assert not np.array_equal(runs[0]["out"][0], runs[0]["out"][1])


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_and_parameter_independence(shape):
    warp = _handler().warp_panorama_depth
    H, W, h, w = shape
    panos, depths = _scene(H, W, True)
    x, d = torch.from_numpy(panos).cuda(), torch.from_numpy(depths).cuda()
    p = _prm()
    out, out_d, hit = warp(x, d, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2], return_hit=True)
    again = warp(x, d, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2])
    assert _bits_equal(out, again[0]) and _bits_equal(out_d, again[1]), "without the hit list / a second call"
    for b in range(3):
        theta, phi, move = PARAMS[b]
        # alone, by value
        o1, d1, h1 = warp(x[b], d[b], (w, h), theta=theta, phi=phi, move=move, return_hit=True)
        assert o1.shape == (h, w, 3) and d1.shape == (h, w) and h1.shape == (h, w, 3)
        assert _bits_equal(o1, out[b]) and _bits_equal(d1, out_d[b]) and _bits_equal(h1, hit[b]), b
        # a batch of three by value: every image of it
        o3, d3 = warp(x, d, (w, h), theta=theta, phi=phi, move=move)
        assert _bits_equal(o3[b], out[b]) and _bits_equal(d3[b], out_d[b]), b
    # depth only
    none, d0 = warp(None, d, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2])
    assert none is None and _bits_equal(d0, out_d)
    assert warp(x[:0], d[:0], (w, h))[1].shape == (0, h, w)


def test_move_zero_is_the_unit_sphere_warp_and_resamples_the_depth():
    handler = _handler()
    for H, W, h, w in SHAPES:
        panos, depths = _scene(H, W, True)
        x, d = torch.from_numpy(panos).cuda(), torch.from_numpy(depths).cuda()
        p = _prm([(t, f, 0.0) for t, f, _ in PARAMS])
        out, out_d, hit = handler.warp_panorama_depth(x, d, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2], return_hit=True)
        _, coords = handler.warp_panorama(x, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2], return_coords=True)
        hit, coords, out_d = hit.cpu().numpy(), coords.cpu().numpy(), out_d.cpu().numpy()
        dr = np.abs(hit[..., 1] - coords[..., 0])
        dc = np.abs((hit[..., 2] - coords[..., 1] + W / 2) % W - W / 2)
        print("%s: positions differ by at most %.2e rows, %.2e columns" % ((H, W, h, w), dr.max(), dc.max()))
        assert dr.max() <= 1e-9 and dc.max() <= 1e-9
        for b in range(3):
            want = oracle.lookup(depths[b], hit[b, ..., 1].reshape(-1), hit[b, ..., 2].reshape(-1)).reshape(h, w)
            tol = 2.0 * (depths[b].max() - depths[b].min()) / (32 * 2.0 ** 24) + np.spacing(want.astype(np.float32))
            assert (np.abs(out_d[b] - want) <= tol).all(), (H, W, b)


def test_invalid_samples_are_nan_and_touch_nothing_else():
    warp = _handler().warp_panorama_depth
    H, W, h, w = 16, 32, 8, 16
    panos, depths = _scene(H, W, False)
    depths = depths.copy()
    depths[0, 5, 7] = 0.0                                            # a depth that is not > 0
    params = [(0.0, 0.0, 0.3), (0.0, 0.0, -2.5), (20.0, -35.0, 0.6)]     # sample 1: the viewpoint is behind the wall at z = 2
    for b in range(2):
        assert not oracle.warp(depths[b], h, w, *params[b])["valid"]
    x, d, p = torch.from_numpy(panos).cuda(), torch.from_numpy(depths).cuda(), _prm(params)
    out, out_d, hit = warp(x, d, (w, h), theta=p[:, 0], phi=p[:, 1], move=p[:, 2], return_hit=True)
    for b in range(2):
        assert bool(torch.isnan(out[b]).all()) and bool(torch.isnan(out_d[b]).all()) and bool(torch.isnan(hit[b]).all()), b
    o1, d1, h1 = warp(x[2], d[2], (w, h), theta=params[2][0], phi=params[2][1], move=params[2][2], return_hit=True)
    assert _bits_equal(o1, out[2]) and _bits_equal(d1, out_d[2]) and _bits_equal(h1, hit[2])
    assert bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(hit[2]).all())
    # a NaN depth and a NaN parameter likewise
    depths[0, 5, 7] = np.nan
    p2 = _prm([(0.0, 0.0, 0.3), (float("nan"), 0.0, 0.1), (20.0, -35.0, 0.6)])
    out2, d2 = warp(x, torch.from_numpy(depths).cuda(), (w, h), theta=p2[:, 0], phi=p2[:, 1], move=p2[:, 2])
    assert bool(torch.isnan(out2[:2]).all()) and bool(torch.isnan(d2[:2]).all()) and _bits_equal(out2[2], out[2])
    with pytest.raises(ValueError):
        warp(x, d, (w, h), move=float("nan"))


def test_the_training_size_source():
    """(128, 256) -> (16, 32), the batcher's source size: the one kernel there is (the variant that kept the depth map in LDS
    was measured slower and is not in the library), against the oracle."""
    warp = _handler().warp_panorama_depth
    H, W, h, w = 128, 256, 16, 32
    _, depth = oracle.source(H, W, True)
    d = torch.from_numpy(depth).cuda()
    theta, phi, move = PARAMS[1]
    _, out_d, hit = warp(None, d, (w, h), theta=theta, phi=phi, move=move, return_hit=True)
    want = oracle.warp(depth, h, w, theta, phi, move)
    err = np.abs(hit.cpu().numpy()[..., 0] - want["t"])
    assert (err <= oracle.tolerance(want)).sum() >= 0.999 * err.size
    assert np.array_equal(out_d.cpu().numpy().view(np.int32), hit.cpu().numpy()[..., 0].astype(np.float32).view(np.int32))


@pytest.mark.parametrize("N", [16, 128])
def test_anchor_depth_against_float64(N):
    from emlight_amd.RegressionNetwork.representation import extract_mesh
    H, W = 128, 256
    mesh = extract_mesh(h=H, w=W, ln=N)
    idx = mesh.idx.cpu().numpy()
    _, room = oracle.source(H, W, True)
    rng = np.random.default_rng(N)
    depths = np.stack([room, (room * rng.uniform(0.5, 2.0, room.shape)).astype(np.float32), np.full_like(room, 2.75)])
    depths[1, 40, 100:140] = np.nan                       # left out of its cell
    depths[1, 90, 7] = np.inf
    got = mesh.anchor_depth(torch.from_numpy(depths).cuda())
    assert got.shape == (3, N) and got.dtype == torch.float64
    got = got.cpu().numpy()
    for b in range(3):
        want = oracle.anchor_depth(depths[b], idx, N)
        rel = np.abs(got[b] - want) / want
        print("N = %d, image %d: worst relative error %.2e" % (N, b, rel.max()))
        assert np.isfinite(want).all() and rel.max() <= 1e-11
    assert (np.abs(got[2] - 2.75) <= 1e-15 * 2.75).all()
    # a single image comes back single, bit for bit
    assert _bits_equal(mesh.anchor_depth(torch.from_numpy(depths[0]).cuda()), torch.from_numpy(got[0]).cuda())
    # a cell that is all NaN gives NaN
    hole = depths[0].copy().reshape(-1)
    hole[idx == 3] = np.nan
    out = mesh.anchor_depth(torch.from_numpy(hole.reshape(H, W)).cuda()).cpu().numpy()
    assert np.isnan(out[3]) and np.isfinite(np.delete(out, 3)).all()


# ------------------------------------------------------------------------------------------------ batcher and trainer
@pytest.fixture(scope="module")
def room_batch():
    pano, depth = oracle.source(256, 512)
    panos = np.stack([pano, pano[:, ::-1] * 1.5]).astype(np.float32)
    return torch.from_numpy(panos).cuda(), torch.from_numpy(np.stack([depth, depth[:, ::-1]]).copy()).cuda()


def _batcher(**kw):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(anchors=16, crop_hw=(32, 32), fov_deg=60.0, seed=3, **kw)


def test_batcher_end_to_end(room_batch):
    panos, depths = room_batch
    handler = _handler()
    deg = torch.tensor([30.0, 200.0], dtype=torch.float64, device="cuda")
    warp = (0.0, 0.0, -0.8)
    bt = _batcher()
    out = bt(panos, deg=deg, warp=warp, depth_panos=depths)
    assert out["depth"].shape == (2, 16) and out["depth"].dtype == torch.float32
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    # what it is made of
    small = handler.resize_panorama(panos, (256, 128), deg=deg)
    small_d = bt.small_depth(panos, depths, deg)
    mean = depths.view(2, 128, 2, 256, 2).double().mean(dim=(2, 4))
    shift = [int(float(v) / 360.0 * 256) for v in deg.cpu()]
    for b in range(2):
        rolled = torch.roll(mean[b], shifts=shift[b], dims=1)
        assert float((small_d[b].double() - rolled).abs().max()) <= 1e-6 * float(rolled.max()), "the depth is rotated and resized like the panorama"
    w_pano, w_depth = handler.warp_panorama_depth(small, small_d, None, *warp)
    para, _ = bt.mesh.compute(w_pano)
    assert _bits_equal(out["distribution"], para["distribution"].float())
    assert _bits_equal(out["depth"], bt.mesh.anchor_depth(w_depth).float())
    # without a warp the depth is that of the camera's own position: another one
    still = _batcher()(panos, deg=deg, depth_panos=depths)
    assert _bits_equal(still["depth"], bt.mesh.anchor_depth(small_d).float()) and not torch.equal(still["depth"], out["depth"])
    assert _bits_equal(still["distribution"], bt.mesh.compute(small)[0]["distribution"].float())
    # the unit-sphere warp at the same move gives other targets; the crop is the same
    sphere = _batcher()(panos, deg=deg, warp=warp)
    assert "depth" not in sphere and not torch.equal(sphere["distribution"], out["distribution"])
    assert _bits_equal(sphere["crop"], out["crop"]) and _bits_equal(sphere["alpha"], out["alpha"])
    # without depth_panos: bit for bit what a batcher that never heard of the argument gives
    new = _batcher()(panos, deg=deg, warp=warp, depth_panos=None)
    assert list(new) == list(sphere) == ["crop", "distribution", "intensity", "rgb_ratio", "ambient", "alpha"]
    for k in new:
        assert _bits_equal(new[k], sphere[k]), k
    para, _ = bt.mesh.compute(handler.warp_panorama(small, None, *warp))
    assert _bits_equal(sphere["distribution"], para["distribution"].float())
    # the call only enqueues work
    drawn = _batcher(move_range=(-0.8, 0.0))
    drawn(panos, depth_panos=depths)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = drawn(panos, depth_panos=depths)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v).all()) for v in res.values())


def test_trainer_step_with_geometry_on_a_panorama_batch(room_batch):
    from emlight_amd.RegressionNetwork.engine import RegressionTrainer
    from emlight_amd.RegressionNetwork.gmloss import SamplesLoss
    panos, depths = room_batch
    batch = _batcher()(panos, deg=45.0, warp=(0.0, 0.0, -0.8), depth_panos=depths)
    torch.manual_seed(0)
    tr = RegressionTrainer(anchors=16, crop_hw=(32, 32), geometry=True)
    assert isinstance(tr.sam_loss, SamplesLoss)
    loss, terms = tr.step(batch)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in terms.values())
    assert tr.sam_loss.M.shape == (2, 16, 16)
