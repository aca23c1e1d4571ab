"""GPU: the ground-plane shadow (csrc/ground_shadow.hip through ``emlight_amd.insert.ground_shadow``) against the float64
restatement of its definition (``shadow_oracle.py``).

The sum is over binary visibility tests, in f64 on both sides.  Where every test of a pixel is at least ``MARGIN = 1e-9``
(relative, ``shadow_oracle``'s margin) from flipping, device and oracle add the same texels and

    |ratio - oracle| <= 2^-23:

the result lies in [0, 1] and is rounded to f32 once (at most 2^-25); the f64 sums of at most 8192 terms (H <= 64) and the
division contribute some 1e-12; the rest is margin.  Pixels below the margin are left out of that check; they may be at most
2 % of a case's plane-hitting pixels (the scenes below have none: ``test_ground_shadow_abi.py`` checks that on the CPU), must
lie in [0, 1] and may differ from the oracle by at most the largest single texel term over E0.

The scenes are the smallest that reach every path of the kernel: panoramas of H = 8 and 16 (non-negative random HDR values,
one bright texel), images of 12 x 16 and 7 x 9 (partly filled 16 x 16 tiles, partly filled waves), B = 2 with another plane
and other spheres in the second image, view azimuths 180 and 37 degrees -- and one scene at H = 64: the kernel walks a row 64
columns at a time, and only a panorama wider than 64 columns has a second chunk."""
import functools

import numpy as np
import pytest
import torch

from tests import shadow_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
FLOOR = (0.0, 1.0, 0.0, 1.0)

# name -> H, (h, w), view azimuth, planes (one 4-tuple for the batch or one per image), occluders (B = 2, K, 4)
CASES = {
    # one sphere resting on (b = 0) or hovering over (b = 1) the floor, in view; per-image planes
    "resting": (16, (12, 16), 180.0, [FLOOR, (0.1, 1.0, -0.05, 1.3)],
                [[(0.2, -0.6, -3.0, 0.4)], [(-0.3, -0.7, -2.8, 0.5)]]),
    # three overlapping spheres: a texel two of them block counts once
    "overlap": (8, (7, 9), 37.0, FLOOR,
                [[(0.0, -0.6, -3.0, 0.4), (0.3, -0.5, -3.1, 0.35), (0.1, -0.3, -2.9, 0.3)],
                 [(-0.4, -0.5, -3.4, 0.5), (-0.1, -0.4, -3.3, 0.45), (0.2, -0.7, -2.6, 0.3)]]),
    # between the camera and the floor it looks at, overhead: from the floor the sphere lies towards +z of the camera, where
    # the panorama's column seam is at azimuth 180
    "seam": (16, (7, 9), 180.0, FLOOR, [[(0.0, 0.0, -1.5, 0.5)], [(0.2, 0.1, -1.2, 0.4)]]),
    # straight above a part of the floor: the cone of those pixels holds the zenith, row 0 in all columns
    "zenith": (8, (12, 16), 180.0, FLOOR, [[(0.0, 0.5, -3.0, 0.4)], [(0.5, 0.2, -3.5, 0.6)]]),
    # planes that rise away from the camera and lean sideways: a part of the image misses them
    "tilted": (16, (12, 16), 37.0, [(0.3, 1.0, 0.25, 1.0), (-0.2, 1.0, 0.3, 0.8)],
               [[(0.084, -0.006, -2.787, 0.28)], [(-0.3, 0.3, -2.5, 0.3)]]),
    # spheres that reach through the floor: the floor's points inside them are exactly 0
    "inside": (8, (7, 9), 180.0, FLOOR, [[(0.0, -1.0, -3.5, 1.5)], [(0.5, -0.8, -4.0, 1.2)]]),
    # 128 columns, two 64-column chunks per row: an overhead sphere whose hull wraps the seam (walked as the head of the first
    # chunk and the tail of the last) and a sphere ahead on the floor whose cap lies across the chunk boundary (azimuth 180 is
    # column 64); in the second image the cap about the zenith takes all columns of both chunks
    "chunks": (64, (7, 9), 180.0, FLOOR, [[(0.0, 0.0, -1.5, 0.5), (0.1, -0.6, -3.6, 0.4)],
                                          [(0.2, 0.6, -2.6, 0.5), (-0.3, -0.5, -4.0, 0.6)]]),
    # entirely below the plane: nothing is lost
    "below": (8, (7, 9), 37.0, FLOOR, [[(0.0, -2.0, -3.0, 0.5)], [(0.4, -1.8, -2.5, 0.6)]]),
}


def hdr(B, H, seed):
    g = np.random.default_rng([seed, B, H])
    pano = (g.random((B, 3, H, 2 * H)) ** 4 * 50.0 + 0.01).astype(np.float32)
    pano[:, :, 1, (5 * H) // 4] = 2000.0                                             # one bright texel, high in the sky
    return pano


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case (float32, as the device gets them) and the oracle's answer on exactly those values, made once."""
    H, (h, w), az, planes, occ = CASES[name]
    pano = hdr(2, H, 51)
    planes = np.asarray(planes, dtype=np.float32)
    occ = np.asarray(occ, dtype=np.float32)
    want = oracle.evaluate(pano, planes, occ, h, w, 60.0, az)
    for v in want.values():
        v.setflags(write=False)
    return {"pano": pano, "planes": planes, "occ": occ, "h": h, "w": w, "az": az, "want": want}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plane_arg(planes):
    return tuple(float(v) for v in planes) if planes.ndim == 1 else cuda(planes)


def run(c, **kw):
    from emlight_amd.insert import ground_shadow
    args = dict(fov_deg=60.0, view_azimuth_deg=c["az"], size=(c["h"], c["w"]))
    args.update(kw)
    return ground_shadow(cuda(c["pano"]), cuda(c["occ"]), plane_arg(c["planes"]), **args)


def compare(name, got, want):
    """The elementwise check of the module docstring; prints each figure before it asserts."""
    got = got.cpu().numpy().astype(np.float64)
    hit, margin = want["hit"], want["margin"]
    firm = margin >= oracle.MARGIN                                                     # inf where the pixel misses the plane
    left = hit & ~firm
    err = np.abs(got - want["ratio"])
    firm3 = np.broadcast_to(firm[:, None], got.shape)
    print("%s: %d of %d pixels hit the plane, %d below the margin; largest error %.3e (bound %.3e); smallest ratio %.4f"
          % (name, hit.sum(), hit.size, left.sum(), err[firm3].max(), TOL, got.min()))
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert left.sum() <= 0.02 * hit.sum()
    assert err[firm3].max() <= TOL
    assert np.all(got[np.broadcast_to(~hit[:, None], got.shape)] == 1.0), "a pixel that misses the plane is exactly 1"
    assert np.all(got[np.broadcast_to(want["inside"][:, None], got.shape)] == 0.0), "a point inside a sphere is exactly 0"
    assert np.all(err <= np.where(firm3, TOL, want["largest_term"][:, :, None, None]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_oracle(name):
    c = case(name)
    got = run(c)
    assert got.shape == (2, 3, c["h"], c["w"]) and got.dtype == torch.float32
    compare(name, got, c["want"])
    want = c["want"]
    if name == "below":
        assert torch.all(got == 1.0)
    else:
        assert float(got.min()) < 0.999, "the case casts a shadow"
    if name == "tilted":
        assert want["hit"].any() and not want["hit"].all()
    if name == "inside":
        assert want["inside"][0].any() and want["inside"][1].any()
    # two runs are bit-identical, and image 0 does not depend on the batch
    assert torch.equal(run(c), got)
    one = dict(c, pano=c["pano"][:1], occ=c["occ"][:1], planes=c["planes"] if c["planes"].ndim == 1 else c["planes"][:1])
    assert torch.equal(run(one)[0], got[0])


def test_no_occluder_is_all_ones():
    c = case("resting")
    none = dict(c, occ=np.zeros((2, 0, 4), dtype=np.float32))
    assert torch.all(run(none) == 1.0)


def test_a_padded_sphere_changes_no_bit():
    c = case("overlap")
    got = run(c)
    pad = np.array([[5.0, 5.0, 5.0, 0.0]] * 2, dtype=np.float32)[:, None]              # r = 0: ignored wherever it stands
    neg = np.array([[0.0, -0.6, -3.0, -1.0]] * 2, dtype=np.float32)[:, None]            # r < 0 too, even on top of a real one
    for occ in (np.concatenate([c["occ"], pad], 1), np.concatenate([pad, c["occ"]], 1),
                np.concatenate([c["occ"][:, :1], neg, c["occ"][:, 1:], pad], 1)):
        assert torch.equal(run(dict(c, occ=occ)), got)
    nan = np.array([[0.0, -0.6, -3.0, np.nan]] * 2, dtype=np.float32)[:, None]          # a NaN radius is padding as well
    assert torch.equal(run(dict(c, occ=np.concatenate([nan, c["occ"]], 1))), got)
    # an infinite radius holds every point: 0 wherever the plane is hit, 1 elsewhere
    inf = np.array([[0.0, 0.0, 0.0, np.inf]] * 2, dtype=np.float32)[:, None]
    hit = torch.from_numpy(np.broadcast_to(c["want"]["hit"][:, None], got.shape).copy()).cuda()
    assert torch.equal(run(dict(c, occ=np.concatenate([c["occ"], inf], 1))), torch.where(hit, 0.0, 1.0))
    # and a sphere another one hides entirely changes nothing either: a texel counts once
    inner = c["occ"][:, :1].copy()
    inner[:, :, 3] *= 0.5
    assert torch.equal(run(dict(c, occ=np.concatenate([c["occ"], inner], 1))), got)


def test_a_black_channel_is_exactly_one():
    c = case("resting")
    pano = c["pano"].copy()
    pano[:, 1] = 0.0
    got = run(dict(c, pano=pano))
    assert torch.all(got[:, 1] == 1.0)
    assert torch.equal(got[:, 0], run(c)[:, 0]) and float(got[:, 2].min()) < 0.999     # the other channels are untouched


def test_plane_as_numbers_and_as_a_tensor():
    c = case("zenith")                                                                  # one plane for the batch
    got = run(c)
    assert torch.equal(run(dict(c, planes=np.broadcast_to(c["planes"], (2, 4)).copy())), got)
    # the four numbers are the plane equation's coefficients: a common factor changes nothing that matters
    scaled = run(dict(c, planes=(c["planes"] * 2.0).astype(np.float32)))
    assert float((scaled - got).abs().max()) <= TOL
    # a plane the host could not see: a zero normal or d <= 0 in a device tensor makes that image NaN, and only that image
    bad = np.array([FLOOR, (0.0, 0.0, 0.0, 1.0)], dtype=np.float32)
    out = run(dict(c, planes=bad))
    assert torch.equal(out[0], got[0]) and bool(torch.isnan(out[1]).all())


def test_outputs_do_not_depend_on_each_other():
    from emlight_amd import _lib
    c = case("resting")
    g = np.random.default_rng(52)
    image = cuda((g.random((2, 3, c["h"], c["w"])) ** 4 * 20.0 + 0.01).astype(np.float32))
    ratio = run(c)
    both = run(c, image=image, size=None)
    assert torch.equal(both[0], ratio) and torch.equal(both[1], image * ratio)          # one f32 multiply
    # shadowed alone: the entry point itself, without the ratio output
    L = _lib.lib()
    pano, occ, planes = cuda(c["pano"]), cuda(c["occ"]), cuda(c["planes"])
    work = torch.empty(L.eml_ground_shadow_work_floats(2, 16, c["h"], c["w"], 1) // 2 + 1, dtype=torch.float64, device="cuda")
    alone = torch.empty_like(ratio)
    _lib.check(L.eml_ground_shadow_f32(_lib.ptr(pano), 2, 16, 32, _lib.ptr(planes), 4, _lib.ptr(occ), 1, c["h"], c["w"], 60.0,
                                       c["az"], _lib.ptr(image), None, _lib.ptr(alone), _lib.ptr(work), _lib.current_stream()),
               "eml_ground_shadow_f32")
    assert torch.equal(alone, both[1])


def test_only_enqueues_work():
    c = case("seam")
    pano, occ = cuda(c["pano"]), cuda(c["occ"])
    from emlight_amd.insert import ground_shadow, sphere_occluder

    def go():
        o = sphere_occluder(7, 9, (4.0, 3.0), 1.5, 3.0, 60.0).expand(2, 1, 4).contiguous()
        return ground_shadow(pano, occ, FLOOR, size=(7, 9)), ground_shadow(pano, o, FLOOR, size=(7, 9))
    want = go()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = go()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # the occluder of a drawn sphere is the oracle's
    o = sphere_occluder(7, 9, (4.0, 3.0), 1.5, 3.0, 60.0)
    assert o.shape == (1, 1, 4) and np.allclose(o.cpu().numpy()[0, 0], oracle.sphere_occluder(7, 9, (4.0, 3.0), 1.5, 3.0, 60.0),
                                                rtol=1e-6, atol=0)


def test_command_line_casts_the_shadow(tmp_path):
    from emlight_amd import insert
    from emlight_amd.RegressionNetwork.util import TonemapHDR
    g = np.random.default_rng(53)
    pano, image = hdr(1, 16, 54), (g.random((3, 12, 16)) ** 4 * 20.0 + 0.01).astype(np.float32)
    np.save(str(tmp_path / "pred.npy"), pano)
    np.save(str(tmp_path / "crop.npy"), image)
    out = str(tmp_path / "out.npy")
    base = ["--pano", str(tmp_path / "pred.npy"), "--image", str(tmp_path / "crop.npy"), "--sphere", "9", "6.5", "3", "--out", out]
    insert.main(base + ["--ground", "1.0", "--depth", "3"])
    got = np.load(out)
    img = cuda(image[None])
    alpha = TonemapHDR(gamma=2.4)(img, clip=True)[1]
    exposure = alpha.to(torch.float32) ** 2.4                                          # of the unshadowed image
    normal, cov = insert.gbuffer_sphere(12, 16, (9.0, 6.5), 3.0)
    occ = insert.sphere_occluder(12, 16, (9.0, 6.5), 3.0, 3.0, 60.0)
    ratio = insert.ground_shadow(cuda(pano), occ, (0.0, 1.0, 0.0, 1.0), size=(12, 16))
    assert float(ratio.min()) < 0.99 and float(ratio.max()) == 1.0
    # the floor is darker under and beside the sphere, away from the light: the bright texel stands high, ahead and to the
    # right of the camera (azimuth 230 degrees against the view's 180), so the pixels that lose it lie below the sphere's
    # centre (row 6.5) and, on average, left of its column (9)
    rows, cols = np.nonzero(ratio[0, 0].cpu().numpy() < 0.6)
    assert rows.size >= 8 and rows.min() >= 9 and cols.mean() < 9.0

    def composite(hdr_image):
        background = (hdr_image * exposure.view(1, 1, 1, 1)).clamp(0.0, 1.0) ** (1.0 / 2.4)
        return insert.insert_object(cuda(pano), normal, cov, background, exposure, 0.8, 0.2, None)[0].cpu().numpy()
    assert np.array_equal(got, composite(img * ratio))
    # without --ground: today's output
    insert.main(base)
    plain = np.load(out)
    assert np.array_equal(plain, composite(img))
    assert (got <= plain).all() and (got < plain).any()                                # darker on the floor, equal elsewhere
