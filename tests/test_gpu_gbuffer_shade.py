"""GPU: G-buffer shading and the composite (csrc/gbuffer_shade.hip through ``emlight_amd.insert``) against the float64
restatement of their definition (``insert_oracle.py``).  The oracle is fed the DEVICE's own maps, so that the prefilter's
error (bounded in ``test_gpu_env_prefilter.py``) does not compound; the end-to-end test adds it explicitly.

Bounds, derived (``EPS = 2^-24``, the unit roundoff of float32):

* shading, per pixel: every lookup is within ``32 EPS max|map|`` of the oracle's (DESIGN section 15's bound for the mirror
  lookup, f32 blend included; geometry is f64 on both sides and the bilinear interpolant is continuous in it), scaled by its
  ``|k|``; the products and sums add at most ``8 EPS`` of the sum of the terms' magnitudes.
* composite, per value, on the device's own ``shaded``: ``x = fl(a s)`` (1 rounding), ``ldr = exp2(fl(log2(x) fl(1/gamma)))``.
  With ``log2`` and ``exp2`` good to 2 ulp (``4 EPS`` relative each; the hardware's are 1 ulp), the exponent ``log2(x) / gamma``
  carries a relative error of at most ``4 + 2 = 6 EPS`` plus ``1.45 EPS / gamma`` absolute from the rounding of ``x``, and an
  absolute error ``d`` of the exponent is a relative ``ln2 d`` of the result: ``ldr`` is within
  ``EPS (6 |log2 x| / gamma + 2 / gamma + 4) ldr``; the clamped ends (0 and 1) are exact.  The blend
  ``fl(fl(c ldr) + fl(fl(1 - c) bg))`` adds at most ``4 EPS (c ldr + (1 - c) |bg|)``.
* end to end (``insert_object`` against the oracle's whole chain): the shaded value is within ``ds`` = the prefilter's bound
  (section 15's ``(H W + 4 m + 64) EPS max|map|``, scaled by ``|k|``: a lookup is a convex combination) plus the shading
  bound; the composite is monotone in ``shaded``, so ``ds`` is carried through it by evaluating the oracle's composite at
  ``shaded +- ds``, and the composite's own bound is added: the sum of the three bounds, each carried to the output.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import insert_oracle as oracle
from tests import sphere_render_oracle as sro

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
H, HD, HG, PHONG = 16, 4, 8, 50.0
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(("kd", "ks", "km"), n)]      # the seven non-empty subsets


def hdr(B, Hh, seed):
    g = np.random.default_rng([seed, B, Hh])
    return (g.random((B, 3, Hh, 2 * Hh)) ** 4 * 50.0 + 0.01).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(B):
    """The panorama and the DEVICE's maps of it, made once per batch size: host copies and device tensors."""
    from emlight_amd.insert import prefilter_environment
    pano = hdr(B, H, 41)
    dev = torch.from_numpy(pano).cuda()
    ed = prefilter_environment(dev, HD, ("diffuse",))
    eg = prefilter_environment(dev, HG, (PHONG,))
    return {"pano": pano, "pano_dev": dev, "ed_dev": ed[:, 0], "eg_dev": eg[:, 0], "ed": ed[:, 0].cpu().numpy(),
            "eg": eg[:, 0].cpu().numpy()}


def normal_towards(target, h, w, i, j, fov, az):
    """The camera-space normal of pixel (i, j) whose reflection direction is ``target``: the half vector of target and v_p."""
    _, r, u, v = oracle.basis(az)
    vp = -oracle.pixel_rays(h, w, fov, az)[i, j]
    n = np.asarray(target, dtype=np.float64) / np.linalg.norm(target) + vp
    return np.array([n @ r, n @ u, n @ v])


def direction(theta, phi):
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


@functools.lru_cache(maxsize=None)
def gbuffer(B, h, w, fov, az):
    g = np.random.default_rng([42, B, h, w, int(fov), int(az)])
    normal = g.standard_normal((B, 3, h, w))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.05                                       # random, facing the camera
    row = np.pi / H                                                                  # one texel row of the panorama
    planted = [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.3, 0.2, -0.8),  # facing, up, down, back-facing
               (0.3, 0.0, 0.4), (1.0, -2.0, 2.0), (0.0, 0.0, 0.0)]             # lengths 0.5 and 3, zero length
    targets = [direction(1.0, 0.0), direction(2.0, 1e-3), direction(0.7, -1e-3),      # on and about the column seam
               direction(0.3 * row / 2, 1.0), direction(np.pi - 0.3 * row / 2, 4.0),  # beyond the first / last row centre
               direction(1e-3, 2.0), direction(np.pi - 1e-3, 5.0)]                    # next to the poles (AT a pole the azimuth of
    # a computed reflection is rounding noise and the clamped row makes the value depend on it: only the normals (0, +-1, 0) go there)
    npix = h * w
    for b in range(B):
        for k in range(min(npix, len(planted) + len(targets))):
            i, j = divmod((k + 3 * b) % npix, w)                                      # another pixel in every image
            normal[b, :, i, j] = planted[k] if k < len(planted) else normal_towards(targets[k - len(planted)], h, w, i, j,
                                                                                    fov, az)
    cov = g.random((B, 1, h, w)) * 0.9 + 0.1
    cov[g.random((B, 1, h, w)) < 0.3] = 1.0
    coef = {k: g.random((B, 3, h, w)) * s for k, s in (("kd", 1.0), ("ks", 0.5), ("km", 0.3))}
    coef["kd"][:, :, 0, :] *= -3.0                                                    # a negative coefficient
    if npix > 20:
        zero = (g.random((B, 1, npix)) < 0.25) & (np.arange(npix) >= 20)              # the planted pixels stay covered
        zero[:, :, -1] = True
        cov[zero.reshape(B, 1, h, w)] = 0.0
    normal = normal.astype(np.float32)
    dead = (cov[:, 0] == 0.0) | (np.abs(normal).sum(1) == 0.0)                        # NaN wherever nothing may be read ...
    for k in coef:
        coef[k] = coef[k].astype(np.float32)
        coef[k][np.broadcast_to(dead[:, None], coef[k].shape)] = np.nan
    normal[np.broadcast_to((cov[:, 0] == 0.0)[:, None], normal.shape)] = np.nan        # ... the normal where coverage is 0
    cov = cov.astype(np.float32)
    bg = g.random((B, 3, h, w)).astype(np.float32)
    return normal, cov, coef, bg, dead


def shading_bound(terms):
    """Per value: sum over the terms of 32 EPS |k| max|map| plus 8 EPS of the terms' magnitudes."""
    return sum(32 * EPS * ak * mx[:, None, None, None] for ak, mx, _ in terms) + 8 * EPS * sum(t for _, _, t in terms)


def cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


CAMERAS = [(60.0, 180.0), (100.0, 77.3), (0.0, 180.0), (0.0, 77.3), (60.0, 77.3), (100.0, 180.0)]


@pytest.mark.parametrize("fov,az", CAMERAS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", [(6, 8), (7, 9), (2, 2)])
def test_shading_against_the_oracle(h, w, B, fov, az):
    from emlight_amd.insert import shade_gbuffer
    sc = scene(B)
    normal, cov, coef, _, dead = gbuffer(B, h, w, fov, az)
    worst = 0.0
    for subset in SUBSETS:
        ks = {k: (coef[k] if k in subset else None) for k in ("kd", "ks", "km")}
        got = shade_gbuffer(sc["pano_dev"], cuda(normal), cuda(cov), cuda(ks["kd"]), cuda(ks["ks"]), cuda(ks["km"]), fov_deg=fov,
                            view_azimuth_deg=az, maps=(sc["ed_dev"], sc["eg_dev"])).cpu().numpy().astype(np.float64)
        want, terms = oracle.shade(sc["pano"], sc["ed"], sc["eg"], normal, cov, ks["kd"], ks["ks"], ks["km"], fov, az)
        assert len(terms) == len(subset) and np.isfinite(got).all()
        assert np.all(got[np.broadcast_to(dead[:, None], got.shape)] == 0.0), "uncovered pixels and zero normals: exactly 0"
        tol = shading_bound(terms)
        live = ~np.broadcast_to(dead[:, None], got.shape)
        assert np.all(np.abs(got - want) <= tol), (subset, float(np.abs(got - want).max()))
        worst = max(worst, float((np.abs(got - want)[live] / tol[live]).max()))
    print("%dx%d B %d fov %g az %g: largest error / bound %.3e" % (h, w, B, fov, az, worst))


def composite_bound(shaded, cov, bg, exposure, gamma):
    x = np.clip(exposure[:, None, None, None] * shaded, 0.0, 1.0)
    ldr = x ** (1.0 / gamma)
    l2 = np.abs(np.log2(np.where(x > 0, x, 1.0)))
    inner = EPS * (6.0 * l2 / gamma + 2.0 / gamma + 4.0) * ldr
    return cov * inner + 4 * EPS * (cov * ldr + (1.0 - cov) * np.abs(bg))


@pytest.mark.parametrize("gamma", [2.4, 1.0])
def test_composite_against_the_oracle_on_the_devices_shaded(gamma):
    from emlight_amd.insert import composite, insert_object, shade_gbuffer
    B, h, w, fov, az = 3, 6, 8, 60.0, 180.0
    sc = scene(B)
    normal, cov, coef, bg, dead = gbuffer(B, h, w, fov, az)
    exposure = np.array([1e-3, 0.05, 40.0], dtype=np.float32)                         # dark; mid-range; clamps at 1
    args = (sc["pano_dev"], cuda(normal), cuda(cov))
    kw = dict(kd=cuda(coef["kd"]), ks=cuda(coef["ks"]), km=cuda(coef["km"]), fov_deg=fov, view_azimuth_deg=az,
              maps=(sc["ed_dev"], sc["eg_dev"]))
    shaded = shade_gbuffer(*args, **kw)
    got = composite(shaded, cuda(cov), cuda(bg), cuda(exposure), gamma=gamma).cpu().numpy().astype(np.float64)
    sh = shaded.cpu().numpy().astype(np.float64)
    want = oracle.composite(sh, cov, bg, exposure, gamma)
    x = exposure[:, None, None, None].astype(np.float64) * sh
    assert (x < 0).any() and (x > 1).any() and ((x > 0) & (x < 1)).any()              # both ends clamp, and the middle is there
    tol = composite_bound(sh, cov.astype(np.float64), bg.astype(np.float64), exposure.astype(np.float64), gamma)
    err = np.abs(got - want)
    print("composite gamma %g: largest error / bound %.3e" % (gamma, float((err[tol > 0] / tol[tol > 0]).max())))
    assert np.all(err <= tol), float((err - tol).max())
    full = np.broadcast_to(cov == 0.0, got.shape)
    assert np.array_equal(got[full], bg.astype(np.float64)[np.broadcast_to(cov == 0.0, bg.shape)])   # uncovered: the photograph
    # the same epilogue inside the shading call: the bits of the two-step result, and a number for the exposure
    one = insert_object(*args, cuda(bg), cuda(exposure), gamma=gamma, **kw)
    assert torch.equal(one, torch.from_numpy(got.astype(np.float32)).cuda())
    flat = insert_object(*args, cuda(bg), 0.05, gamma=gamma, **kw)
    assert torch.equal(flat[1], one[1])


def test_insert_object_end_to_end():
    from emlight_amd.insert import insert_object
    B, h, w, fov, az, gamma = 3, 7, 9, 60.0, 77.3, 2.4
    pano = hdr(B, H, 43)
    normal, cov, coef, bg, dead = gbuffer(B, h, w, fov, az)
    exposure = np.array([0.01, 0.05, 2.0], dtype=np.float32)
    got = insert_object(cuda(pano), cuda(normal), cuda(cov), cuda(bg), cuda(exposure), cuda(coef["kd"]), cuda(coef["ks"]),
                        cuda(coef["km"]), gamma=gamma, fov_deg=fov, view_azimuth_deg=az, phong_exponent=PHONG,
                        diffuse_height=HD, glossy_height=HG).cpu().numpy().astype(np.float64)
    ed = oracle.prefilter(pano, HD, ("diffuse",))[:, 0]
    eg = oracle.prefilter(pano, HG, (PHONG,))[:, 0]
    sh, terms = oracle.shade(pano, ed, eg, normal, cov, coef["kd"], coef["ks"], coef["km"], fov, az)
    pre = [(H * 2 * H + 4 * m + 64) * EPS * np.abs(mp).reshape(B, -1).max(1) for m, mp in ((1.0, ed), (PHONG, eg))]
    ds = terms[0][0] * pre[0][:, None, None, None] + terms[1][0] * pre[1][:, None, None, None] + shading_bound(terms)
    c64, b64, e64 = cov.astype(np.float64), bg.astype(np.float64), exposure.astype(np.float64)
    want = oracle.composite(sh, c64, b64, e64, gamma)
    carried = np.maximum(np.abs(oracle.composite(sh + ds, c64, b64, e64, gamma) - want),
                         np.abs(oracle.composite(sh - ds, c64, b64, e64, gamma) - want))
    own = np.maximum(composite_bound(sh + ds, c64, b64, e64, gamma), composite_bound(sh - ds, c64, b64, e64, gamma))
    tol = carried + own
    err = np.abs(got - want)
    print("insert_object: largest error / bound %.3e" % float((err[tol > 0] / tol[tol > 0]).max()))
    assert np.isfinite(got).all() and np.all(err <= tol), float((err - tol).max())


def test_sphere_against_render_spheres():
    """A diffuse and a glossy sphere through ``gbuffer_sphere`` and the orthographic camera against ``render_spheres``.  The
    difference is mostly the interpolation error of looking maps up instead of integrating -- a property of the method,
    computed here per pixel as the difference of the two float64 oracles on the same input; the GPU results may differ by
    that plus the rounding bounds of the three kernels involved (prefilter, shading; the renders' own of section 15)."""
    from emlight_amd.evaluate import render_spheres
    from emlight_amd.insert import gbuffer_sphere, shade_gbuffer
    S, Hd, Hg = 16, 16, 32
    pano = hdr(2, H, 44)
    dev = cuda(pano)
    centre, radius = ((S - 1) / 2, (S - 1) / 2), S / 2
    normal, cov = gbuffer_sphere(S, S, centre, radius, batch=2)
    on, oc = oracle.gbuffer_sphere(S, S, centre, radius)
    assert np.array_equal(cov[0, 0].cpu().numpy() != 0, sro.mask(S)) and np.array_equal(normal[1].cpu().numpy(), on.astype(np.float32))
    renders = render_spheres(dev, size=S, materials=("diffuse", "glossy"), phong_exponent=PHONG).cpu().numpy().astype(np.float64)
    o_render = sro.render(pano, S, ("diffuse", "glossy"), 180.0, PHONG)
    one = np.ones((2, 3, S, S))
    n64, c64 = np.broadcast_to(on, (2, 3, S, S)), np.broadcast_to(oc, (2, 1, S, S))
    for i, (name, m, G) in enumerate((("diffuse", 1.0, Hd), ("glossy", PHONG, Hg))):
        emap = oracle.prefilter(pano, G, ("diffuse" if i == 0 else PHONG,))[:, 0]
        if i == 0:
            got = shade_gbuffer(dev, normal, cov, kd=1.0, fov_deg=0.0, diffuse_height=G)
            o_shade, terms = oracle.shade(pano, emap, None, n64, c64, kd=one, fov_deg=0.0)
        else:
            got = shade_gbuffer(dev, normal, cov, ks=(1.0, 1.0, 1.0), fov_deg=0.0, glossy_height=G, phong_exponent=PHONG)
            o_shade, terms = oracle.shade(pano, None, emap, n64, c64, ks=one, fov_deg=0.0)
        got = got.cpu().numpy().astype(np.float64)
        interp = np.abs(o_shade - o_render[:, i])
        integral = (H * 2 * H + 4 * m + 64) * EPS
        tol = (interp + integral * np.abs(emap).reshape(2, -1).max(1)[:, None, None, None] + shading_bound(terms)
               + integral * np.abs(o_render[:, i]).reshape(2, -1).max(1)[:, None, None, None])
        diff = np.abs(got - renders[:, i])
        print("%s sphere, map height %d: interpolation error %.3e of the maximum %.3e; GPU difference %.3e"
              % (name, G, float(interp.max()), float(np.abs(o_render[:, i]).max()), float(diff.max())))
        assert np.all(diff <= tol), (name, float((diff - tol).max()))
        assert np.all(got[:, :, ~sro.mask(S)] == 0.0)


def test_only_enqueues_work():
    from emlight_amd.insert import gbuffer_sphere, insert_object, shade_gbuffer
    B, h, w = 2, 6, 8
    pano, bg = cuda(hdr(B, H, 45)), torch.rand(B, 3, h, w, device="cuda")
    ex = torch.full((B,), 0.05, device="cuda")

    def run():
        normal, cov = gbuffer_sphere(h, w, (3.5, 2.5), 2.6, batch=B)
        a = shade_gbuffer(pano, normal, cov, kd=(0.8, 0.7, 0.6), ks=0.2, km=0.05, diffuse_height=4, glossy_height=8)
        return a, insert_object(pano, normal, cov, bg, ex, kd=0.8, ks=0.2, diffuse_height=4, glossy_height=8)
    want = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(g, w_) for g, w_ in zip(got, want))


def test_refusals_raise():
    from emlight_amd import _lib
    from emlight_amd.insert import composite, shade_gbuffer
    sc = scene(1)
    normal, cov = torch.rand(1, 3, 4, 5, device="cuda"), torch.ones(1, 1, 4, 5, device="cuda")
    with pytest.raises(ValueError):
        shade_gbuffer(sc["pano_dev"], normal, cov)
    with pytest.raises(ValueError):
        shade_gbuffer(sc["pano_dev"], normal, cov, km=1.0, fov_deg=180.0)
    with pytest.raises(ValueError, match="forward only"):
        shade_gbuffer(sc["pano_dev"], normal.clone().requires_grad_(True), cov, km=1.0)
    with pytest.raises(_lib.EmlightHipError):
        shade_gbuffer(sc["pano_dev"], normal.cpu(), cov, km=1.0)
    with pytest.raises(ValueError):
        composite(normal, cov, normal, 1.0, gamma=0.0)
    # the launcher itself refuses an inconsistent set with a message
    L = _lib.lib()
    out = torch.empty(1, 3, 4, 5, device="cuda")
    rc = L.eml_gbuffer_shade_f32(None, 16, None, 0, 0, None, 0, 0, _lib.ptr(normal), _lib.ptr(cov), None, None, _lib.ptr(normal),
                                 1, 4, 5, 60.0, 180.0, _lib.ptr(out), None, None, 2.4, None, _lib.current_stream())
    with pytest.raises(_lib.EmlightHipError, match="km needs pano"):
        _lib.check(rc, "eml_gbuffer_shade_f32")


def test_command_line_equals_the_direct_call(tmp_path):
    from emlight_amd import insert
    from emlight_amd.RegressionNetwork.util import TonemapHDR
    g = np.random.default_rng(47)
    pano, image = hdr(1, H, 48), (g.random((3, 12, 16)) ** 4 * 20.0 + 0.01).astype(np.float32)
    np.save(str(tmp_path / "pred.npy"), pano)                                         # (1, 3, H, 2H), as GenProjector.test writes it
    np.save(str(tmp_path / "crop.npy"), image)
    out = str(tmp_path / "out.npy")
    insert.main(["--pano", str(tmp_path / "pred.npy"), "--image", str(tmp_path / "crop.npy"), "--sphere", "9", "6.5", "4", "--fov", "70",
                 "--ks", "0.3", "--km", "0.1", "--out", out])
    got = np.load(out)
    img = cuda(image[None])
    alpha = TonemapHDR(gamma=2.4)(img, clip=True)[1]
    exposure = alpha.to(torch.float32) ** 2.4
    background = (img * exposure.view(1, 1, 1, 1)).clamp(0.0, 1.0) ** (1.0 / 2.4)
    normal, cov = insert.gbuffer_sphere(12, 16, (9.0, 6.5), 4.0)
    want = insert.insert_object(cuda(pano), normal, cov, background, exposure, 0.8, 0.3, 0.1, fov_deg=70.0)
    assert got.shape == (3, 12, 16) and np.array_equal(got, want[0].cpu().numpy())
    covered = cov[0, 0].cpu().numpy() != 0
    assert covered.sum() > 30 and np.array_equal(got[:, ~covered], background[0].cpu().numpy()[:, ~covered])
    assert np.isfinite(got).all() and (got[:, covered] != background[0].cpu().numpy()[:, covered]).any()
    # a G-buffer directory with the same sphere and coefficients gives the same image
    gb = tmp_path / "gbuffer"
    gb.mkdir()
    np.save(str(gb / "normal.npy"), normal[0].cpu().numpy())
    np.save(str(gb / "coverage.npy"), cov[0, 0].cpu().numpy())
    for name, v in (("kd", 0.8), ("ks", 0.3), ("km", 0.1)):
        np.save(str(gb / (name + ".npy")), np.full((3, 12, 16), v, dtype=np.float32))
    insert.main(["--pano", str(tmp_path / "pred.npy"), "--image", str(tmp_path / "crop.npy"), "--gbuffer", str(gb), "--fov", "70", "--out", out])
    assert np.array_equal(np.load(out), got)
