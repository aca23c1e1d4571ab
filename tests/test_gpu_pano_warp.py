"""GPU: the panorama warp on the MI355X (csrc/pano_warp.hip) against ``tests/warp_oracle.py``, the float64 restatement of
the reference's ``resize_exr`` that ``test_pano_warp_abi.py`` pins to the reference's own maps.

Bounds
* positions: chord distance on the sphere between the kernel's exported ``(row, col)`` and the oracle's, at most ``1e-7``.
  ``asin`` at the pole turns a 1-ulp float64 error of its argument into at most ``sqrt(2^-51) ~ 2.1e-8`` rad; the bound
  leaves a factor of 5 for the device's libm.  (The kernel takes a position within 2^-28 px of an integer for that integer:
  at most ``pi / H * 2^-28 ~ 6e-9`` rad at H = 2, inside the same bound.)
* image: the oracle's wrap-bilinear evaluated AT THE KERNEL'S OWN exported positions, at most 1 float32 ulp (the kernel
  sums the same four float64 products in the same order and rounds once; the ulp is room for a fused multiply-add).
* everything about batches, runs, the coordinate output and repeated calls is bit for bit.

Inputs: ``pano_inputs`` of ``make_golden_panorama`` -- heavy-tailed, non-negative, saturated patches in the thousands next
to values near zero, so that a wrong tap or a stray weight shows."""
import os

import numpy as np
import pytest
import torch

from tests import warp_oracle as oracle
from tests.golden.make_golden_panorama import BATCHER, pano_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHORD_BOUND = 1e-7
EXTRA_SHAPES = [(2, 2, 3, 5), (7, 9, 23, 41)]          # odd sizes, a non-2:1 aspect, a ragged 256-pixel tile


def _handler():
    from emlight_amd.RegressionNetwork.util import PanoramaHandler
    return PanoramaHandler


def _ulps(a, b):
    """Largest distance in float32 steps between two arrays of finite values of equal sign pattern."""
    ia, ib = np.ascontiguousarray(a).view(np.int32).astype(np.int64), np.ascontiguousarray(b).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def cases():
    """Every (parameters, shape) case once: source (2 images), the kernel's image and positions, the oracle's positions."""
    handler = _handler()
    made = []
    for k, (theta, phi, move) in enumerate(oracle.PARAMS):
        for shape in oracle.SHAPES + EXTRA_SHAPES:
            H, W, h, w = shape
            src = pano_inputs(2, H, W, 70 + k)
            out, coords = handler.warp_panorama(torch.from_numpy(src).cuda(), (w, h), theta=theta, phi=phi, move=move,
                                                return_coords=True)
            made.append((k, shape, src, out, coords))
    torch.cuda.synchronize()
    result = []
    for k, shape, src, out, coords in made:
        H, W, h, w = shape
        assert out.shape == (2, h, w, 3) and out.dtype == torch.float32
        assert coords.shape == (1, h, w, 2) and coords.dtype == torch.float64
        c = coords[0].cpu().numpy()
        result.append({"k": k, "shape": shape, "params": oracle.PARAMS[k], "src": src, "out": out.cpu().numpy(),
                       "row": c[..., 0], "col": c[..., 1], "want": oracle.positions(H, W, h, w, *oracle.PARAMS[k])})
    return result


def test_positions_against_the_oracle_and_the_reference(cases):
    z = np.load(os.path.join(ROOT, "tests", "golden", "warp.npz"))
    worst = 0.0
    for c in cases:
        H, W, h, w = c["shape"]
        assert np.isfinite(c["row"]).all() and np.isfinite(c["col"]).all()
        assert c["row"].min() >= 0 and c["row"].max() <= H and c["col"].min() >= 0 and c["col"].max() <= W
        d = oracle.chord(c["row"], c["col"], c["want"][0], c["want"][1], H, W)
        worst = max(worst, d)
        line = "p%d %-18s chord to the oracle %.3e (bound %.1e)" % (c["k"], c["shape"], d, CHORD_BOUND)
        name = oracle.case_name(c["k"], c["shape"])
        if name + "/row" in z.files:
            d_ref = float(z[name + "/d_ref"])
            to_ref = oracle.chord(c["row"], c["col"], z[name + "/row"], z[name + "/col"], H, W)
            line += "; to the reference's maps %.3e (the oracle's own distance %.3e)" % (to_ref, d_ref)
            assert to_ref <= d_ref + CHORD_BOUND, name              # triangle inequality
        print(line)
        assert d <= CHORD_BOUND, (c["k"], c["shape"])
    print("worst chord %.3e" % worst)
    assert sum(1 for c in cases if oracle.case_name(c["k"], c["shape"]) + "/row" in z.files) == 16


def test_image_is_the_wrap_bilinear_sample_at_the_exported_positions(cases):
    # what the cases cover, asserted from the oracle: the last row blending with row 0, the last column with column 0, and a
    # position exactly at the size (`mod 2 pi` rounding up to 2 pi at the pole row of p1 and p3), which must land on index 0
    rows_past, cols_past, exact = 0, 0, 0
    for c in cases:
        H, W, _, _ = c["shape"]
        row, col = c["want"]
        rows_past += int((row > H - 1).sum())
        cols_past += int((col > W - 1).sum())
        exact += int(((col == W) | (row == H)).sum())
    print("oracle positions: %d with row > H - 1, %d with col > W - 1, %d exactly at H or W" % (rows_past, cols_past, exact))
    assert rows_past > 0 and cols_past > 0 and exact > 0
    worst, exact_kernel = 0, 0
    for c in cases:
        H, W, _, _ = c["shape"]
        exact_kernel += int(((c["col"] == W) | (c["row"] == H)).sum())
        for b in range(2):
            want = oracle.sample(c["src"][b], c["row"], c["col"])
            assert np.isfinite(c["out"][b]).all()
            u = _ulps(c["out"][b], want)
            worst = max(worst, u)
            assert u <= 1, (c["k"], c["shape"], b, u)
    print("worst distance to the oracle's sample: %d ulp; %d kernel positions exactly at H or W" % (worst, exact_kernel))
    assert exact_kernel >= exact
    # the two images of a case differ, so the check tells a batch index apart
    assert not np.array_equal(cases[0]["out"][0], cases[0]["out"][1])


def test_batches_runs_and_the_coordinate_output_are_bit_identical():
    """By value, B = 5: two runs (4 images + a ragged run of 1) share one evaluated position each; per sample, B = 3 with the
    same values: one evaluation per image; single images; with and without the coordinate output; a second call."""
    handler = _handler()
    theta, phi, move = -30.0, 130.0, 0.6
    src = torch.from_numpy(pano_inputs(5, 16, 32, 81)).cuda()
    size = (41, 23)
    five, coords = handler.warp_panorama(src, size, theta=theta, phi=phi, move=move, return_coords=True)
    assert coords.shape == (1, 23, 41, 2)
    assert _bits_equal(five, handler.warp_panorama(src, size, theta=theta, phi=phi, move=move)), "without coords"
    assert _bits_equal(five, handler.warp_panorama(src, size, theta=theta, phi=phi, move=move, return_coords=True)[0])
    full = lambda v: torch.full((3,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    three, coords3 = handler.warp_panorama(src[1:4], size, theta=full(theta), phi=full(phi), move=full(move), return_coords=True)
    assert coords3.shape == (3, 23, 41, 2)
    assert _bits_equal(three, five[1:4]), "per-sample parameters that repeat the by-value ones"
    assert all(_bits_equal(coords3[i], coords[0]) for i in range(3))
    assert _bits_equal(three, handler.warp_panorama(src[1:4], size, theta=full(theta), phi=phi, move=move)), "without coords"
    for b in (0, 3, 4):                                              # first run, its last image, the ragged run
        alone, c1 = handler.warp_panorama(src[b], size, theta=theta, phi=phi, move=move, return_coords=True)
        assert alone.shape == (23, 41, 3) and c1.shape == (23, 41, 2)
        assert _bits_equal(alone, five[b]) and _bits_equal(c1, coords[0]), b
    # per-sample values that differ: each image is what it is alone
    prm = torch.tensor([[0.0, 0.0, 0.4], [25.0, 0.0, 0.0], [10.0, -200.0, -0.5]], dtype=torch.float64, device="cuda")
    mixed = handler.warp_panorama(src[:3], size, theta=prm[:, 0], phi=prm[:, 1], move=prm[:, 2])
    for b in range(3):
        t, p, m = (float(v) for v in prm[b].cpu())
        assert _bits_equal(mixed[b], handler.warp_panorama(src[b], size, theta=t, phi=p, move=m)), b
    assert handler.warp_panorama(src[:0], size).shape == (0, 23, 41, 3)


@pytest.mark.parametrize("H,W", [(128, 256), (33, 47)])
def test_identity_returns_the_source_bit_for_bit(H, W):
    handler = _handler()
    src = torch.from_numpy(pano_inputs(2, H, W, 82)).cuda()
    out, coords = handler.warp_panorama(src, return_coords=True)
    rows = torch.arange(H, device="cuda", dtype=torch.float64)[:, None].expand(H, W)
    cols = torch.arange(W, device="cuda", dtype=torch.float64)[None, :].expand(H, W)
    print("identity %dx%d: %d of %d values differ" % (H, W, int((out.view(torch.int32) != src.view(torch.int32)).sum()), out.numel()))
    assert _bits_equal(out, src)
    assert torch.equal(coords[0, ..., 0], rows) and torch.equal(coords[0, ..., 1] % W, cols)
    from emlight_amd.GenProjector.data import resize_exr
    assert _bits_equal(resize_exr(src, H, W), src)


def test_positions_that_are_not_finite_give_nan_and_touch_nothing_else():
    """Per-sample parameters: a NaN move (no pixel has a position), move = 1.0 exactly (the direction that
    would fall on the new viewpoint is lon = pi, whose float64 sine is 1.2e-16, not 0 -- the oracle says which pixels, if
    any, have none) and move = -1.0 exactly (lon = 0: pixel (h / 2, 0) has |v| == 0 exactly)."""
    handler = _handler()
    H, W, h, w = 16, 32, 8, 16
    src = pano_inputs(5, H, W, 83)
    moves = [0.3, float("nan"), 1.0, -1.0, 0.3]
    prm = torch.tensor([[0.0, 0.0, m] for m in moves], dtype=torch.float64, device="cuda")
    x = torch.from_numpy(src).cuda()
    out, coords = handler.warp_panorama(x, (w, h), theta=prm[:, 0], phi=prm[:, 1], move=prm[:, 2], return_coords=True)
    out, coords = out.cpu().numpy(), coords.cpu().numpy()
    assert np.isnan(out[1]).all() and np.isnan(coords[1]).all()
    for b in (2, 3):
        row, col = oracle.positions(H, W, h, w, 0.0, 0.0, moves[b])
        bad = np.isnan(row)
        print("move %+.1f: %d pixels without a position" % (moves[b], int(bad.sum())))
        np.testing.assert_array_equal(np.isnan(out[b]).any(axis=-1), bad)
        np.testing.assert_array_equal(np.isnan(out[b]).all(axis=-1), bad)
        np.testing.assert_array_equal(np.isnan(coords[b]).any(axis=-1), bad)
        assert oracle.chord(coords[b][~bad][:, 0], coords[b][~bad][:, 1], row[~bad], col[~bad], H, W) <= CHORD_BOUND
        want = oracle.sample(src[b], coords[b][..., 0], coords[b][..., 1])
        assert _ulps(out[b][~bad], want[~bad]) <= 1
    assert np.isnan(out[3][h // 2, 0]).all() and int(np.isnan(out[3]).any(axis=-1).sum()) == 1
    # the images around them are what they are alone
    for b in (0, 4):
        alone = handler.warp_panorama(x[b], (w, h), move=0.3).cpu().numpy()
        assert np.array_equal(out[b].view(np.int32), alone.view(np.int32)) and np.isfinite(out[b]).all()
    # by value, such parameters never reach the kernel
    with pytest.raises(ValueError):
        handler.warp_panorama(x, (w, h), move=float("nan"))


# ------------------------------------------------------------------------------------------------ batchers
@pytest.fixture(scope="module")
def panos():
    cfg = BATCHER
    return torch.from_numpy(pano_inputs(cfg["B"], cfg["HW"][0], cfg["HW"][1], cfg["seed"])).cuda()


def _projector(**kw):
    from emlight_amd.GenProjector.data import ProjectorPanoramaBatcher
    return ProjectorPanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], **kw)


def _regression(**kw):
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    return PanoramaBatcher(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], **kw)


@pytest.mark.parametrize("warp", [(0.0, 0.0, -0.5), "per-sample"])
def test_batchers_derive_their_targets_from_the_warped_panorama(panos, warp):
    from emlight_amd.GenProjector.data import gaussian_map, light_targets
    handler = _handler()
    deg = torch.tensor(BATCHER["deg"], device="cuda", dtype=torch.float64)
    if warp == "per-sample":
        warp = torch.tensor([[10.0, -20.0, 0.4], [0.0, 5.0, -0.6]], dtype=torch.float64, device="cuda")
        kw = {"theta": warp[:, 0], "phi": warp[:, 1], "move": warp[:, 2]}
    else:
        kw = dict(zip(("theta", "phi", "move"), warp))
    plain = _projector(regression=True)(panos, deg=deg)
    out = _projector(regression=True)(panos, deg=deg, warp=warp)
    want_pano = handler.warp_panorama(handler.resize_panorama(panos, (256, 128), deg=deg), **kw)
    assert _bits_equal(out["pano"], want_pano) and not torch.equal(out["pano"], plain["pano"])
    warped, mask = light_targets(want_pano, out["alpha"])
    assert _bits_equal(out["warped"], warped) and torch.equal(out["map"], mask)
    bt = _regression()
    para, _ = bt.mesh.compute(want_pano)
    targets = bt.targets(para, out["alpha"])
    for k in ("distribution", "intensity", "rgb_ratio", "ambient"):
        assert _bits_equal(out[k], targets[k]), k
    assert _bits_equal(out["input"], gaussian_map(para["distribution"].float(), para["intensity"].float(), para["rgb_ratio"].float(),
                                                  para["ambient"].float(), out["alpha"], ln=BATCHER["anchors"]))
    # the crop is untouched
    for k in ("crop", "crop128", "alpha"):
        assert _bits_equal(out[k], plain[k]), k
    # PanoramaBatcher: the same targets from the same warped panorama
    reg = _regression()(panos, deg=deg, warp=warp)
    for k in reg:
        assert _bits_equal(reg[k], out[k]), k


def test_move_range_is_seeded_and_absent_arguments_change_nothing(panos):
    handler = _handler()
    a, b = _projector(seed=7, move_range=(-0.6, 0.0)), _projector(seed=7, move_range=(-0.6, 0.0))
    first, second, again = a(panos), a(panos), b(panos)
    for k in first:
        assert _bits_equal(first[k], again[k]), "the same seed gives the same batch: %s" % k
    assert not torch.equal(first["pano"], second["pano"])
    # the draws: the azimuths first, as without move_range, then the moves, uniform in [lo, hi)
    c = _projector(seed=7, move_range=(-0.6, 0.0))
    B = panos.shape[0]
    deg, move = c.random_deg(B), c.random_move(B)
    assert torch.equal(deg, _projector(seed=7).random_deg(B))
    assert bool((move >= -0.6).all()) and bool((move < 0.0).all()) and move.dtype == torch.float64
    small = handler.resize_panorama(panos, (256, 128), deg=deg)
    assert _bits_equal(first["pano"], handler.warp_panorama(small, move=move))
    assert _bits_equal(first["crop"], _projector(seed=7)(panos)["crop"]), "the crop is the one drawn without move_range"
    reg = _regression(seed=7, move_range=(-0.6, 0.0))(panos)
    assert _bits_equal(reg["alpha"], first["alpha"])
    # neither argument: what a batcher built without them gives (the two constructors' defaults are the old signatures')
    from emlight_amd.GenProjector.data import ProjectorPanoramaBatcher
    from emlight_amd.RegressionNetwork.data import PanoramaBatcher
    args = dict(anchors=BATCHER["anchors"], crop_hw=BATCHER["crop_hw"], fov_deg=BATCHER["fov"], seed=11)
    for cls, extra in ((ProjectorPanoramaBatcher, {"regression": True}), (PanoramaBatcher, {})):
        old, new = cls(**args, **extra), cls(**args, **extra, move_range=None)
        want, got = old(panos), new(panos, warp=None)
        assert list(want) == list(got)
        for k in want:
            assert torch.equal(want[k], got[k]), k
    # the call only enqueues work, drawn warp included
    bt = _projector(seed=9, move_range=(-0.5, 0.5))
    bt(panos)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bt(panos)
        out2 = bt(panos, deg=12.5, warp=(5.0, 5.0, 0.2))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and all(bool(torch.isfinite(v).all()) for v in out2.values())
