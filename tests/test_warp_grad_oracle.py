"""CPU: ``tests/warp_grad_oracle.py``, the float64 torch restatement of the panorama warp that the GPU gradients
(``tests/test_gpu_pano_warp_grad.py``) are measured against, validated WITHOUT a GPU.

* Its positions equal ``tests/warp_oracle.positions`` (pinned to the reference's own maps by ``test_pano_warp_abi.py``) to
  1e-9 px and its image equals ``warp_oracle.warp`` to float32 rounding, on every case the GPU test uses.
* Its ``dparams`` agree with central finite differences (step 1e-6) of its own forward to 1e-6 relative, at generic
  parameters only: at the identity every position is an integer, a kink, where the right-hand-cell convention is the
  definition and a central difference does not apply.
* No case of the GPU test lets the kernel and the oracle classify a pixel differently: no pixel has ``s1^2 + s2^2`` in
  [2^-21, 2^-19] (the pole rule's threshold is 2^-20), no position lies at a distance in [2^-29, 2^-27] from an integer (the
  snap's threshold is 2^-28)."""
import numpy as np
import pytest

from tests import warp_grad_oracle as go
from tests import warp_oracle as oracle

CASES = [(s, p) for s in go.SIZES for p in go.PARAMS] + [(tuple(c[:4]), c[4]) for c in go.UNIT_MOVES]


def test_forward_is_the_numpy_oracle():
    worst_px, worst_img = 0.0, 0.0
    for (H, W, h, w), prm in CASES:
        src = go.panoramas(1, H, W, 90)[0]
        img, row, col = go.forward(src, h, w, *prm)
        want_row, want_col = oracle.positions(H, W, h, w, *prm)
        np.testing.assert_array_equal(np.isnan(row), np.isnan(want_row))
        ok = ~np.isnan(want_row)
        d_row = np.abs(row - want_row)[ok].max()
        d_col = np.abs((col - want_col + W / 2) % W - W / 2)[ok].max()
        worst_px = max(worst_px, d_row, d_col)
        assert d_row <= 1e-9 and d_col <= 1e-9, ((H, W, h, w), prm, d_row, d_col)
        # the image: the numpy oracle samples at ITS positions (unsnapped), this one at the snapped ones; a position within
        # 2^-28 px of an integer moves the value by at most 2^-28 * (the largest difference of neighbouring texels)
        want = oracle.warp(src, h, w, *prm).astype(np.float64)
        np.testing.assert_array_equal(np.isnan(img).any(axis=-1), ~ok)
        tol = 2.0 ** -23 * np.abs(want[ok]) + 2.0 ** -27 * float(np.abs(src).max())
        err = np.abs(img[ok] - want[ok])
        worst_img = max(worst_img, float((err / tol).max()))
        assert (err <= tol).all(), ((H, W, h, w), prm, float((err / tol).max()))
    print("worst position difference %.3e px; worst image error %.3f of its bound" % (worst_px, worst_img))


def test_no_case_sits_on_a_threshold():
    seen_pole, seen_snap, seen_none = 0, 0, 0
    for (H, W, h, w), prm in CASES:
        rho2, dist, ok = go.classify(H, W, h, w, *prm)
        near_pole = ok & (rho2 >= 2.0 ** -21) & (rho2 <= 2.0 ** -19)
        near_snap = ok & (dist >= 2.0 ** -29) & (dist <= 2.0 ** -27)
        assert not near_pole.any(), ((H, W, h, w), prm, rho2[near_pole])
        assert not near_snap.any(), ((H, W, h, w), prm, dist[near_snap])
        seen_pole += int((ok & (rho2 < 2.0 ** -20)).sum())
        seen_snap += int((ok & (dist < 2.0 ** -28)).sum())
        seen_none += int((~ok).sum())
    print("pole pixels %d, snapped positions %d, pixels without a position %d" % (seen_pole, seen_snap, seen_none))
    assert seen_pole > 0 and seen_snap > 0 and seen_none > 0          # the cases do exercise the three rules


@pytest.mark.parametrize("size", go.FD_SIZES)
@pytest.mark.parametrize("prm", go.GENERIC)
def test_dparams_agree_with_central_differences(size, prm):
    H, W, h, w = size
    src = go.panoramas(1, H, W, 91)[0]
    g = go.grad_outputs(1, h, w, 92)[0].astype(np.float64)
    _, dparams, _, S_abs = go.gradients(src, g, *prm)

    def loss(q):
        img, _, _ = go.forward(src, h, w, *q)
        assert np.isfinite(img).all()
        return float((img * g).sum())
    step = 1e-6
    for k in range(3):
        lo, hi = list(prm), list(prm)
        lo[k] -= step
        hi[k] += step
        fd = (loss(hi) - loss(lo)) / (2 * step)
        rel = abs(fd - dparams[k]) / abs(dparams[k])
        print("%s %s q=%d: autograd %.12e, differences %.12e, relative %.2e (S_abs %.3e)" % (size, prm, k, dparams[k], fd, rel, S_abs[k]))
        assert rel <= 1e-6, (size, prm, k)


def test_conventions_at_the_identity():
    """Row 0 is the pole: it adds nothing to dparams; dpano of the identity warp is grad_out itself; a texel nothing lands on
    is exactly 0 in dpano and in A."""
    H, W = 8, 16
    src = go.panoramas(1, H, W, 93)[0]
    g = go.grad_outputs(1, H, W, 94)[0]
    dpano, dparams, A, S_abs = go.gradients(src, g)
    np.testing.assert_array_equal(dpano, g.astype(np.float64))
    np.testing.assert_array_equal(A, np.abs(g).astype(np.float64))
    g2 = g.copy()
    g2[0] = 0
    _, dparams2, _, S_abs2 = go.gradients(src, g2)
    np.testing.assert_array_equal(dparams, dparams2)
    np.testing.assert_array_equal(S_abs, S_abs2)
    assert np.isfinite(dparams).all() and (S_abs > 0).all()
    # shrinking: most texels receive nothing
    dpano, _, A, _ = go.gradients(go.panoramas(1, 16, 32, 93)[0], go.grad_outputs(1, 3, 5, 94)[0], 25.0, -40.0, -0.6)
    assert (A == 0).sum() > 0 and (dpano[A == 0] == 0).all()
