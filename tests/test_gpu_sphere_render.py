"""GPU: the sphere renders (csrc/sphere_render.hip through ``emlight_amd.evaluate``) against the float64 restatement of their
definition (``sphere_render_oracle.py``), and the metrics kernel against the same on the device's own renders.

Tolerances are derived, not measured:

* integrals: ``|got - want| <= (H W + 4 m + 64) 2^-24 max|want|`` per image and material -- the worst case of a float32
  summation of ``H W`` non-negative terms, the rounding of ``x^m`` (``m`` times the 4 roundings behind ``x``) and of the weight;
* mirror: ``|got - want| <= 32 * 2^-24 max|pano|`` -- at most 8 roundings with a x4 margin (``RESIZE_ATOL`` of
  ``test_gpu_projector_pano.py``);
* metrics: the sums are float64 over at most ``3 S^2`` terms of float32 data, so every term carries about ``1e-16`` of the data's
  scale and a sum about ``1e-12``.  rmse and si_rmse are therefore compared within ``1e-10`` of ``max(|want|, rms(b))`` (relative
  for any value that is not a cancelled zero) and angular within ``1e-10`` of ``max(|want|, 1 degree)``; ``used`` exactly.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import sphere_render_oracle as oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ALL = oracle.MATERIALS


def hdr(B, H, W, seed):
    """U[0,1)^4 * 50 + 0.01: strictly positive, a dynamic range of a few thousand."""
    g = np.random.default_rng([seed, B, H, W])
    return (g.random((B, 3, H, W)) ** 4 * 50.0 + 0.01).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(H, W, S, az, m):
    return oracle.weights(H, W, S, az, m)


def want_render(pano, S, materials=ALL, az=180.0, m=50.0):
    """The oracle's render with the weight matrices shared between the tests of one (grid, S, azimuth, m)."""
    B, _, H, W = pano.shape
    inside = oracle.mask(S)
    out = np.zeros((B, len(materials), 3, S, S))
    flat = pano.astype(np.float64).reshape(B, 3, H * W)
    for i, name in enumerate(materials):
        if name == "mirror":
            out[:, i][:, :, inside] = oracle.mirror(pano, S, az)
        else:
            out[:, i][:, :, inside] = flat @ weights(H, W, S, az, m)[0 if name == "diffuse" else 1].T
    return out


def check_render(got, pano, S, materials=ALL, az=180.0, m=50.0, what=""):
    B, _, H, W = pano.shape
    got = got.cpu().numpy().astype(np.float64)
    want = want_render(pano, S, materials, az, m)
    assert got.shape == want.shape
    inside = oracle.mask(S)
    assert np.all(got[..., ~inside] == 0.0), "pixels outside the disc must be exactly 0"
    for b in range(B):
        for i, name in enumerate(materials):
            if name == "mirror":
                tol = 32 * EPS * float(np.abs(pano).max())
            else:
                tol = (H * W + 4 * m + 64) * EPS * float(np.abs(want[b, i]).max())
            err = float(np.abs(got[b, i] - want[b, i]).max())
            print("%s %s image %d: err %.3e tol %.3e" % (what, name, b, err, tol))
            assert err <= tol, (what, name, b, err, tol)


def render(pano, S, materials=ALL, az=180.0, m=50.0):
    from emlight_amd.evaluate import render_spheres
    return render_spheres(torch.from_numpy(pano).cuda(), size=S, materials=materials, view_azimuth_deg=az, phong_exponent=m)


# ------------------------------------------------------------------------------------------------ 1. geometry
# 16 x 32, camera towards azimuth 180 (the centre column): near a pole, on the equator behind the sphere, in front of it
@pytest.mark.parametrize("S", [8, 9])
@pytest.mark.parametrize("texel", [(0, 5), (8, 16), (7, 0)], ids=["pole", "behind", "front"])
def test_one_hot_texel(S, texel):
    from emlight_amd.evaluate import sphere_mask
    H, W = 16, 32
    pano = np.zeros((1, 3, H, W), dtype=np.float32)
    pano[0, :, texel[0], texel[1]] = 100.0
    got = render(pano, S)
    check_render(got, pano, S, what="one-hot %s S=%d" % (texel, S))
    # each integral render is the texel's value times its weight: no summation to hide behind
    inside = oracle.mask(S)
    t = texel[0] * W + texel[1]
    for i in range(2):
        col = 100.0 * weights(H, W, S, 180.0, 50.0)[i][:, t]
        tol = (H * W + 4 * 50 + 64) * EPS * float(col.max()) if col.max() > 0 else 0.0
        for ch in range(3):
            assert np.abs(got[0, i, ch].cpu().numpy()[inside] - col).max() <= tol
    assert np.array_equal(sphere_mask(S).numpy(), inside)
    assert np.array_equal(sphere_mask(S, device="cuda").cpu().numpy(), inside)


# ------------------------------------------------------------------------------------------------ 2. ragged shapes
RAGGED = [(16, 8, 3, ("glossy",)),          # 9 columns
          (12, 33, 2, ("diffuse",)),        # 861 pixels, 288 texels: several row tiles with a ragged last one, 4.5 k chunks
          (16, 9, 11, ("mirror",))]         # 33 columns cross a 32-column tile


@pytest.mark.parametrize("H,S,B,single", RAGGED)
def test_ragged_shapes(H, S, B, single):
    pano = hdr(B, H, 2 * H, 11)
    check_render(render(pano, S), pano, S, what="ragged all")
    check_render(render(pano, S, single), pano, S, single, what="ragged single")


def test_two_materials_in_the_callers_order():
    pano = hdr(2, 16, 32, 12)
    got = render(pano, 9, ("mirror", "diffuse"))
    check_render(got, pano, 9, ("mirror", "diffuse"), what="reordered")
    check_render(render(pano, 9, ("diffuse", "glossy")), pano, 9, ("diffuse", "glossy"), what="pair")


# ------------------------------------------------------------------------------------------------ 3. full panorama size
def test_full_panorama_size():
    pano = hdr(2, 128, 256, 13)                                    # the real k extent and the k split
    check_render(render(pano, 16), pano, 16, what="128x256")


# ------------------------------------------------------------------------------------------------ 4. parameters
@pytest.mark.parametrize("az", [0.0, 77.3])
@pytest.mark.parametrize("m", [1.0, 200.0])
def test_view_azimuth_and_phong_exponent(az, m):
    pano = hdr(2, 16, 32, 14)
    check_render(render(pano, 8, ALL, az, m), pano, 8, ALL, az, m, what="az %g m %g" % (az, m))


# ------------------------------------------------------------------------------------------------ 5. bit reproducibility
def test_bit_reproducible_and_independent_of_the_batch():
    from emlight_amd.evaluate import lighting_metrics
    pano = hdr(3, 16, 32, 15)
    a, b = render(pano, 9), render(pano, 9)
    assert torch.equal(a, b)
    # the k split depends on (H, W, S) only and an MFMA adds its k terms in order: the same bits in any batch
    assert torch.equal(render(pano[:1], 9), a[:1])
    big = hdr(3, 128, 256, 16)
    assert torch.equal(render(big[:1], 16), render(big, 16)[:1])
    p, t = torch.from_numpy(pano).cuda(), torch.from_numpy(hdr(3, 16, 32, 17)).cuda()
    m1, m2 = lighting_metrics(p, t, size=9), lighting_metrics(p, t, size=9)
    assert all(torch.equal(m1[k], m2[k]) for k in m1)


def test_lighting_metrics_only_enqueues_work():
    from emlight_amd.evaluate import lighting_metrics
    p, t = torch.from_numpy(hdr(2, 16, 32, 22)).cuda(), torch.from_numpy(hdr(2, 16, 32, 23)).cuda()
    want = lighting_metrics(p, t, size=8, materials=("mirror", "diffuse"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = lighting_metrics(p, t, size=8, materials=("mirror", "diffuse"))       # the caller's order: no index tensor either
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in got)


# ------------------------------------------------------------------------------------------------ 6. metrics
def check_metrics(got, a, b, S):
    """got: the dict of lighting_metrics; a, b: the device's own renders (B, M, 3, S, S) on the host."""
    want = oracle.metrics(a, b)
    inside = oracle.mask(S)
    for i, name in enumerate(ALL):
        for bi in range(a.shape[0]):
            rms_b = float(np.sqrt(np.mean(b[bi, i][:, inside].astype(np.float64) ** 2)))
            for j, key in enumerate(("rmse", "si_rmse", "angular", "used")):
                g, w = float(got["%s/%s" % (name, key)][bi]), float(want[bi, i, j])
                print("%s/%s image %d: got %.17g want %.17g" % (name, key, bi, g, w))
                if key == "used":
                    assert g == w
                else:
                    scale = max(abs(w), rms_b if key != "angular" else 1.0)
                    assert abs(g - w) <= 1e-10 * scale, (name, key, bi, g, w)
    return want


def metrics_and_renders(pred, true, S):
    from emlight_amd.evaluate import lighting_metrics, render_spheres
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(true).cuda()
    got = {k: v.cpu().numpy() for k, v in lighting_metrics(p, t, size=S).items()}
    assert all(v.dtype == np.float64 and v.shape == (pred.shape[0],) for v in got.values())
    return got, render_spheres(p, size=S).cpu().numpy(), render_spheres(t, size=S).cpu().numpy()


def test_metrics_against_the_oracle_on_the_devices_renders():
    S = 9
    pred, true = hdr(3, 16, 32, 18), hdr(3, 16, 32, 19)            # independent, strictly positive
    got, a, b = metrics_and_renders(pred, true, S)
    want = check_metrics(got, a, b, S)
    P = int(oracle.mask(S).sum())
    assert np.all(want[:, :, 3] == P) and np.all(want[:, :, 0] > 0)


def test_metrics_of_equal_scaled_and_zero_predictions():
    S = 8
    true = hdr(2, 16, 32, 20)
    inside = oracle.mask(S)
    P = int(inside.sum())
    # pred == true: zeros, every pixel used
    got, a, b = metrics_and_renders(true, true, S)
    check_metrics(got, a, b, S)
    for name in ALL:
        assert np.all(got[name + "/rmse"] == 0) and np.all(got[name + "/si_rmse"] == 0) and np.all(got[name + "/used"] == P)
        assert np.all(got[name + "/angular"] <= 1e-10)
    # pred = 3 true: the scale is taken out (what is left is the float32 rounding of 3 x), rmse = 2 rms(b)
    got, a, b = metrics_and_renders(3.0 * true, true, S)
    check_metrics(got, a, b, S)
    # Each render is within its tolerance tb of the exact one (3 tb for the render of 3 x), and the exact ones are
    # proportional, so |a - 3 b| <= 6 tb per value: the residual at s = 1/3 is at most 2 tb and the least-squares s does no
    # worse; rms(a - b) is within rms(a - 3 b) of 2 rms(b); a_p = 3 b_p + e_p with |e_p| <= sqrt(3) 6 tb bounds the angle.
    for i, name in enumerate(ALL):
        for bi in range(2):
            bb, aa = b[bi, i][:, inside].astype(np.float64), a[bi, i][:, inside].astype(np.float64)
            rms_b = float(np.sqrt(np.mean(bb ** 2)))
            tb = 32 * EPS * float(true.max()) if name == "mirror" else (16 * 32 + 4 * 50 + 64) * EPS * float(np.abs(bb).max())
            ang = np.degrees(np.mean(np.arcsin(np.minimum(1.0, np.sqrt(3.0) * 6 * tb / np.linalg.norm(aa, axis=0)))))
            print("%s image %d: si_rmse %.3e <= %.3e, angular %.3e <= %.3e" % (name, bi, got[name + "/si_rmse"][bi], 2 * tb,
                                                                              got[name + "/angular"][bi], ang))
            assert got[name + "/si_rmse"][bi] <= 2 * tb
            assert got[name + "/angular"][bi] <= ang
            assert abs(got[name + "/rmse"][bi] - 2 * rms_b) <= 6 * tb
            assert got[name + "/used"][bi] == P
    # a zero prediction: s = 0, no pixel used
    got, a, b = metrics_and_renders(np.zeros_like(true), true, S)
    check_metrics(got, a, b, S)
    for i, name in enumerate(ALL):
        for bi in range(2):
            rms_b = float(np.sqrt(np.mean(b[bi, i][:, inside].astype(np.float64) ** 2)))
            assert got[name + "/used"][bi] == 0 and got[name + "/angular"][bi] == 0
            assert abs(got[name + "/si_rmse"][bi] - rms_b) <= 1e-10 * rms_b and abs(got[name + "/rmse"][bi] - rms_b) <= 1e-10 * rms_b


# ------------------------------------------------------------------------------------------------ 7. command line
def test_command_line_means_equal_the_direct_call(tmp_path):
    from emlight_amd import evaluate
    from emlight_amd.GenProjector.data import ProjectorPanoramaBatcher
    panos, results = tmp_path / "panos", tmp_path / "results"
    panos.mkdir(), results.mkdir()
    g = np.random.default_rng(21)
    src = (g.random((2, 128, 256, 3)) ** 4 * 50.0 + 0.01).astype(np.float32)   # the batcher's area resize takes integer factors
    preds = (g.random((2, 1, 3, 128, 256)) ** 4 * 20.0 + 0.01).astype(np.float32)
    for i in range(2):
        np.save(str(panos / ("room%d.npy" % i)), src[i])
        np.save(str(results / ("pred_room%d.npy" % i)), preds[i])
    out = str(tmp_path / "metrics.json")
    evaluate.main(["--pano_dir", str(panos), "--results_dir", str(results), "--size", "16", "--out", out])
    res = json.load(open(out))
    assert res["evaluated"] == 2 and res["skipped"] == 0 and sorted(res["images"]) == ["room0", "room1"]
    truth = ProjectorPanoramaBatcher(fov_deg=60.0, device="cuda:0")(torch.from_numpy(src).cuda(), deg=0.0)["warped"]
    direct = evaluate.lighting_metrics(torch.from_numpy(preds[:, 0]).cuda(), truth, size=16)
    assert set(res["means"]) == set(direct)
    for k, v in direct.items():
        assert res["means"][k] == pytest.approx(float(v.mean()), rel=1e-12, abs=0), k
        assert [res["images"]["room%d" % i][k] for i in range(2)] == [float(x) for x in v.cpu()]
