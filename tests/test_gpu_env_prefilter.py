"""GPU: the prefiltered environment maps (csrc/env_prefilter.hip through ``emlight_amd.insert.prefilter_environment``)
against the float64 restatement of their definition (``insert_oracle.py``).

The bound is the project's own for these integrals (Accuracy), per image and lobe:
``|got - want| <= (H W + 4 m + 64) 2^-24 max|want|`` with ``m = 1`` for the diffuse lobe -- the worst case of a float32
summation of ``H W`` non-negative terms, the rounding of ``x^m`` (``m`` times the 4 roundings behind ``x``) and of the weight.
The shapes are the smallest that reach every kernel path (see ``CASES``).  Bit-exactness is asserted with ``torch.equal``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import insert_oracle as oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
D = oracle.DIFFUSE

#        H   Ho  B   lobes
CASES = [(16, 8, 3, (D, 50.0)),              # baseline: one pass of two lobes, 128 directions, 9 columns
         (16, 5, 1, (1.0,)),                 # 50 directions: a partial 32-row tile; one lobe in a pass
         (16, 8, 33, (D,)),                  # 99 columns: a second column group, partial
         (12, 7, 2, (D, 0.0, 200.0, 50.0)),  # more lobes than one pass holds; 288 texels: 4.5 chunks; 0^0 = 1
         (128, 4, 2, (D, 50.0))]             # 512 chunks over 64 splits: the texel split


def hdr(B, H, seed):
    """U[0,1)^4 * 50 + 0.01, strictly positive, with a few texels multiplied by 1e3 (lamps)."""
    g = np.random.default_rng([seed, B, H])
    x = g.random((B, 3, H, 2 * H)) ** 4 * 50.0 + 0.01
    for b in range(B):
        for _ in range(3):
            x[b, :, g.integers(H), g.integers(2 * H)] *= 1e3
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def weights(H, Ho, lobe):
    return oracle.lobe_weights(H, Ho, lobe)


def tolerance(H, lobe, want_max):
    m = 1.0 if lobe == D else float(lobe)
    return (H * 2 * H + 4 * m + 64) * EPS * want_max


def prefilter(pano, Ho, lobes):
    from emlight_amd.insert import prefilter_environment
    return prefilter_environment(torch.from_numpy(pano).cuda(), Ho, lobes)


def check(got, pano, Ho, lobes, what):
    B, _, H, _ = pano.shape
    got = got.cpu().numpy().astype(np.float64)
    want = oracle.prefilter(pano, Ho, lobes, weights)
    assert got.shape == want.shape == (B, len(lobes), 3, Ho, 2 * Ho)
    worst = 0.0
    for b in range(B):
        for i, lb in enumerate(lobes):
            tol = tolerance(H, lb, float(np.abs(want[b, i]).max()))
            err = float(np.abs(got[b, i] - want[b, i]).max())
            worst = max(worst, err / tol)
            assert err <= tol, (what, b, lb, err, tol)
    print("%s: largest error / bound %.3e" % (what, worst))


@pytest.mark.parametrize("H,Ho,B,lobes", CASES)
def test_against_the_oracle(H, Ho, B, lobes):
    pano = hdr(B, H, 31)
    check(prefilter(pano, Ho, lobes), pano, Ho, lobes, "H %d Ho %d B %d lobes %s" % (H, Ho, B, lobes))


@pytest.mark.parametrize("texel", [(0, 5), (8, 0), (15, 31), (7, 16)], ids=["pole", "seam", "last", "middle"])
def test_one_hot_texel(texel):
    """One texel: each map is the texel's value times ONE weight per direction -- no summation to hide behind."""
    H, Ho, lobes = 16, 8, (D, 50.0)
    pano = np.zeros((1, 3, H, 2 * H), dtype=np.float32)
    pano[0, :, texel[0], texel[1]] = (100.0, 1.0, 0.01)
    got = prefilter(pano, Ho, lobes)
    check(got, pano, Ho, lobes, "one-hot %s" % (texel,))
    t = texel[0] * 2 * H + texel[1]
    for i, lb in enumerate(lobes):
        col = weights(H, Ho, lb)[:, t].reshape(Ho, 2 * Ho)
        for ch, v in enumerate((100.0, 1.0, 0.01)):
            want = np.float64(np.float32(v)) * col
            assert np.abs(got[0, i, ch].cpu().numpy() - want).max() <= tolerance(H, lb, float(want.max()))


def test_run_to_run_batch_and_lobe_independence():
    H, Ho = 12, 7
    pano = hdr(3, H, 32)
    four = (D, 0.0, 200.0, 50.0)
    a = prefilter(pano, Ho, four)
    assert torch.equal(a, prefilter(pano, Ho, four))                                   # no atomics: the same bits again
    assert torch.equal(prefilter(pano[:1], Ho, four), a[:1])                           # an image does not see its batch
    for i, lb in enumerate(four):                                                      # a lobe does not see the others
        assert torch.equal(prefilter(pano, Ho, (lb,))[:, 0], a[:, i]), lb
    shuffled = (50.0, D, 7.0, 0.0, 200.0)                                              # other partners, other slots, 3 passes
    b = prefilter(pano, Ho, shuffled)
    for i, lb in enumerate(shuffled):
        if lb in four:
            assert torch.equal(b[:, i], a[:, four.index(lb)]), lb
    assert torch.equal(prefilter(pano, Ho, (D, D))[:, 1], a[:, 0])
    # with the texel split and with a second column group
    big = hdr(2, 128, 33)
    c = prefilter(big, 4, (D, 50.0))
    assert torch.equal(prefilter(big[:1], 4, (50.0,))[:, 0], c[:1, 1]) and torch.equal(c, prefilter(big, 4, (D, 50.0)))
    many = hdr(33, 16, 34)
    d = prefilter(many, 8, (D,))
    assert torch.equal(prefilter(many[32:], 8, (D,)), d[32:]) and torch.equal(prefilter(many[:3], 8, (D,)), d[:3])


def test_only_enqueues_work():
    from emlight_amd.insert import prefilter_environment
    pano = torch.from_numpy(hdr(2, 16, 35)).cuda()
    want = prefilter_environment(pano, 5, (D, 20.0, 3.0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = prefilter_environment(pano, 5, (D, 20.0, 3.0))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want)


def test_refusals_raise():
    from emlight_amd import _lib
    from emlight_amd.insert import prefilter_environment
    pano = torch.from_numpy(hdr(1, 16, 36)).cuda()
    for kw in ({"height": 0}, {"height": 1025}, {"lobes": ()}, {"lobes": (1.0,) * 9}, {"lobes": (-2.0,)}, {"lobes": ("mirror",)}):
        with pytest.raises(ValueError):
            prefilter_environment(pano, **{"height": 4, **kw})
    with pytest.raises(ValueError):
        prefilter_environment(pano[:, :, :, :31].contiguous(), 4)
    with pytest.raises(_lib.EmlightHipError):
        prefilter_environment(pano.cpu(), 4)
    with pytest.raises(_lib.EmlightHipError):
        prefilter_environment(pano.double(), 4)
    with pytest.raises(ValueError, match="forward only"):
        prefilter_environment(pano.clone().requires_grad_(True), 4)
    # the launcher itself: a misaligned scratch pointer and a bad exponent are refused with a message, nothing is enqueued
    L = _lib.lib()
    out = torch.empty(1, 1, 3, 4, 8, device="cuda")
    work = torch.empty(L.eml_env_prefilter_work_floats(1, 16, 32, 4, 1) + 4, device="cuda")
    for wp, lobe, word in ((work.data_ptr() + 4, 50.0, "16-byte"), (work.data_ptr(), 2e6, "lobe 0")):
        rc = L.eml_env_prefilter_f32(_lib.ptr(pano), 1, 16, 32, 4, 1, (ctypes.c_double * 1)(lobe), _lib.ptr(out),
                                     ctypes.c_void_p(wp), _lib.current_stream())
        with pytest.raises(_lib.EmlightHipError, match=word):
            _lib.check(rc, "eml_env_prefilter_f32")
