"""No GPU: tests/norm_oracle.py against float64 ``F.batch_norm`` / ``F.instance_norm`` / ``F.leaky_relu`` autograd on the CPU, so
that the oracle of tests/test_gpu_norm_kernels.py cannot be wrong in the way the kernels are; the condition that test's inputs
must meet (at most 0.1 % of a case's pre-activations near zero); the coverage of its shape lists; and ``_rows_view``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_oracle as no

EPS = 1e-5


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(grad)


def _nchw(rows, B, H, W):   # (B*H*W, C) -> (B, C, H, W)
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):               # (B, C, H, W) -> (B*H*W, C) numpy
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _close(got, want, what, tol=1e-11):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    assert err <= tol * (1 + float(np.abs(want).max())), "%s: %.3e" % (what, err)


@pytest.mark.parametrize("B,H,W,C,ld", [(2, 3, 5, 4, 4), (1, 1, 1, 8, 12), (3, 4, 2, 12, 32)])
def test_statistics_against_batch_norm(B, H, W, C, ld):
    """bn_sums + bn_finalize: mean, istd, and the running buffers of a training step (n = 1 included: biased variance)."""
    r = np.random.RandomState(B * 100 + C)
    n = B * H * W
    buf = r.randn(n, ld).astype(np.float32)
    sums, mags = no.bn_sums(buf, C)
    x = buf[:, :C].astype(np.float64)
    _close(sums[:, 0], x.sum(0), "sum")
    _close(sums[:, 1], (x * x).sum(0), "sumsq")
    _close(mags[:, 0], np.abs(x).sum(0), "abs sum")
    rm, rv = r.randn(C), r.rand(C) + 0.5
    mom = np.float32(0.1)
    mean, istd, nrm, nrv = no.bn_finalize(sums, n, EPS, mom, rm, rv)
    trm, trv = _t(rm).clone(), _t(rv).clone()
    xt = _nchw(_t(x), B, H, W)
    if n > 1:
        out = F.batch_norm(xt, trm, trv, None, None, True, float(mom), EPS)
        _close(_rows(out), (x - mean) * istd, "normalised")
        _close(nrm, trm.numpy(), "running mean")
        _close(nrv, trv.numpy(), "running var")
    else:   # batch_norm refuses one value per channel; the guard: unbiased falls back to biased = 0
        _close(mean, x[0], "mean")
        _close(istd, np.full(C, EPS ** -0.5), "istd")
        _close(nrm, (1 - float(mom)) * rm + float(mom) * x[0], "running mean")
        _close(nrv, (1 - float(mom)) * rv, "running var")
    assert no.bn_finalize(sums, n, EPS, mom)[2:] == (None, None)
    tm, (lo, hi), _, _ = no.bn_finalize_tol(sums, n, EPS, mom, rm, rv)
    assert (lo <= istd).all() and (istd <= hi).all() and (tm >= 0).all()


@pytest.mark.parametrize("slope", no.SLOPES)
@pytest.mark.parametrize("B,H,W,C,up2", [(2, 2, 6, 4, False), (3, 2, 6, 8, True), (2, 6, 4, 12, True), (1, 3, 5, 4, False)])
def test_spade_chain_against_autograd(B, H, W, C, up2, slope):
    """leaky_relu(batch_norm(x) * (1 + gamma) + beta) in training mode, x upsampled first with ``up2``: the forward, dgb and dx
    of the oracle's three steps (norm_modulate_fwd, norm_modulate_bwd, bn_bwd_apply) and the four column sums."""
    r = np.random.RandomState(7 * B + C + int(up2))
    n = B * H * W
    nlo = n // 4 if up2 else n
    x, gb, gy = r.randn(nlo, C + 4), r.randn(n, 2 * C + 8), r.randn(n, C)
    bhw = (B, H, W) if up2 else None
    xl, gbl = _t(x[:, :C], True), _t(gb[:, :2 * C], True)     # the leaves, as rows
    xt = _nchw(xl, B, H // 2 if up2 else H, W // 2 if up2 else W)
    gbt = _nchw(gbl, B, H, W)
    xin = F.interpolate(xt, scale_factor=2, mode="nearest") if up2 else xt
    xn = F.batch_norm(xin, None, None, None, None, True, 0.1, EPS)
    y = F.leaky_relu(xn * (1 + gbt[:, :C]) + gbt[:, C:], slope)
    y.backward(_nchw(_t(gy), B, H, W))
    xfull = no.up2_rows(x, bhw, C) if up2 else x[:, :C]
    sums, _ = no.bn_sums(xfull)
    mean, istd, _, _ = no.bn_finalize(sums, n, EPS, 0.1)
    got, mag, t = no.norm_modulate_fwd(x, gb, C, slope, mean, istd, bhw)
    _close(got, _rows(y), "forward")
    assert (mag >= np.abs(t) - 1e-12).all()
    b = no.norm_modulate_bwd(gy, x, gb, C, slope, mean, istd, bhw)
    _close(np.concatenate([b["dgamma"][0], b["dbeta"][0]], 1), gbl.grad.numpy(), "dgb")
    dxn = b["dxn"][0]
    _close(b["sums"], np.stack([dxn.sum(0), (dxn * b["xhat"]).sum(0), b["dgamma"][0].sum(0), b["dbeta"][0].sum(0)], 1), "sums")
    dx, dmag = no.bn_bwd_apply(dxn, x, C, mean, istd, b["sums"][:, :2], n, bhw)
    _close(dx, xl.grad.numpy(), "dx")
    assert (dmag >= np.abs(dx) - 1e-12).all()
    # the mask from the stored output is the mask from the pre-activation
    if slope < 1:
        by = no.norm_modulate_bwd(gy, x, gb[:, :C], C, slope, mean, istd, bhw, y=got)
        for k in ("dxn", "dgamma", "dbeta"):
            assert np.array_equal(by[k][0], b[k][0]), k
    # eval mode: the statistics are constants
    ev, _ = no.bn_bwd_apply(dxn, x, C, mean, istd, None, n, bhw)
    xel = _t(x[:, :C], True)
    xe = _nchw(xel, B, H // 2 if up2 else H, W // 2 if up2 else W)
    xu = F.interpolate(xe, scale_factor=2, mode="nearest") if up2 else xe
    ((xu - _t(mean).view(1, C, 1, 1)) * _t(istd).view(1, C, 1, 1) * _nchw(_t(dxn), B, H, W)).sum().backward()
    _close(ev, xel.grad.numpy(), "eval dx")


@pytest.mark.parametrize("slope", no.SLOPES)
def test_plain_modulation_against_autograd(slope):
    r = np.random.RandomState(3)
    rows, C = 11, 8
    xn, gb, gy = r.randn(rows, C + 4), r.randn(rows, 2 * C), r.randn(rows, C + 8)
    a, g = _t(xn[:, :C], True), _t(gb, True)
    y = F.leaky_relu(a * (1 + g[:, :C]) + g[:, C:], slope)
    y.backward(_t(gy[:, :C]))
    _close(no.modulate_fwd(xn, gb, C, slope)[0], y.detach().numpy(), "forward")
    b = no.modulate_bwd(gy, xn, gb, C, slope)
    _close(b["dxn"][0], a.grad.numpy(), "dxn")
    _close(np.concatenate([b["dgamma"][0], b["dbeta"][0]], 1), g.grad.numpy(), "dgb")


@pytest.mark.parametrize("slope", no.SLOPES)
@pytest.mark.parametrize("case", [(1, (2, 4, 31)), (0, (2, 3, 63)), (1, (1, 8, 1)), (0, (1, 2, 5))], ids=no.in_name)
def test_instance_norm_against_autograd(case, slope):
    cl, (B, C, HW) = case
    x, gy = no.instance_inputs(case, 5)
    planes = lambda v: _t(np.transpose(v, (0, 2, 1)) if cl else v)
    xt = planes(x).clone().requires_grad_(True)
    if HW > 1:
        y = F.leaky_relu(F.instance_norm(xt, eps=EPS), slope)
    else:   # instance_norm refuses a single value per plane; the formula gives xhat = 0
        y = F.leaky_relu((xt - xt.mean(2, keepdim=True)) / torch.sqrt(xt.var(2, unbiased=False, keepdim=True) + EPS), slope)
    y.backward(planes(gy))
    back = lambda t: np.transpose(t.detach().numpy(), (0, 2, 1)) if cl else t.detach().numpy()
    got, mag, rec = no.instance_norm_act_fwd(x, EPS, slope, cl)
    _close(got, back(y), "forward")
    _close(rec[:, :, 0], x.astype(np.float64).mean(1 if cl else 2), "mean")
    dx, dmag, _ = no.instance_norm_act_bwd(gy, x, rec, slope, cl)
    _close(dx, back(xt.grad), "dx", 1e-9)
    assert got.shape == x.shape and dx.shape == x.shape and (dmag >= np.abs(dx) - 1e-9).all()
    rec2, tm, lo, hi = no.instance_norm_record(x, EPS, cl)
    assert (lo <= rec2[:, :, 1]).all() and (rec2[:, :, 1] <= hi).all()


# ------------------------------------------------------------------------------------------------ the GPU test's cases
def test_case_lists_cover_every_value_of_every_axis():
    for C in no.CHANNELS:
        mine = [c for c in no.FLAT_CASES if c[0] == C]
        assert {c[1] for c in mine} == set(no.ROW_KINDS)
        assert {c[2] for c in mine} == set(no.LD_KINDS)
        assert {c[3] for c in mine} == set(no.GRID_KINDS)
        assert {c[4] for c in mine} == set(no.SLOPES)
        up = [c for c in no.UP2_CASES if c[0] == C]
        assert {c[1] for c in up} == set(no.UP2_MAPS) and {c[3] for c in up} == set(no.SLOPES)
    assert {c[2] for c in no.UP2_CASES} == set(no.GRID_KINDS)
    assert set(no.CHANNELS) == {4, 12, 36, 100, 1020, 1024, 1028}
    assert {no.rows_of(k, 100) for k in no.ROW_KINDS} == {1, 3, 7, 9, 517}           # cvp = 32: 8 rows per pass
    assert {no.rows_of(k, 4) for k in no.ROW_KINDS} == {1, 3, 255, 257, 517}
    assert {no.ld_of(k, 12) for k in no.LD_KINDS} == {12, 16, 32}
    assert {R for R, _ in no.FOLD_CASES} == {1, 2, 15, 16, 17, 512}
    assert {nk for _, nk in no.FOLD_CASES} == {"1", "15", "16", "17", "2C", "4C+1"}
    assert {c[1] for c in no.IN_CASES if c[0]} == {(1, 4, 1), (2, 4, 31), (2, 36, 33), (3, 64, 32), (1, 32, 100)}
    assert {c[1] for c in no.IN_CASES if not c[0]} == {(1, 1, 1), (2, 3, 63), (2, 5, 65), (1, 2, 257), (3, 7, 1000)}
    for cl in (0, 1):
        assert {no.IN_SLOPES[i] for i, c in enumerate(no.IN_CASES) if c[0] == cl} == set(no.SLOPES)
    # B > 1 and H != W: a wrong source row of the upsample is invisible at B = 1 or on square maps
    assert any(B > 1 and H != W for B, H, W in no.UP2_MAPS)


def test_col_map_is_the_launchers():
    """The oracle's copy of the reducing kernels' layout and the grid the Python side picks from it."""
    from emlight_amd.GenProjector.spherenet import _stats_grid
    assert [no.col_map(C) for C in no.CHANNELS] == [(1, 256), (4, 64), (16, 16), (32, 8), (256, 1), (256, 1), (256, 1)]
    for C in no.CHANNELS:
        for rows in (1, 3, 255, 517, 10 ** 6):
            assert no.stats_grid(rows, C) == _stats_grid(rows, C)


def test_near_zero_share_of_every_case_is_within_the_cap():
    """A condition on the inputs, checked on the oracle alone: at most 0.1 % of a case's pre-activations lie within
    16 * 2^-24 magnitudes of zero (the only elements the GPU test may skip)."""
    worst = 0.0
    for case in no.FLAT_CASES:
        C, rk, _, _, slope = case
        rows = no.rows_of(rk, C)
        x, gb, gy, mean, istd = no.spade_inputs(rows, C, no.case_seed("flat", C, rk))
        for t, mag in (no.modulate_fwd(x, gb, C, slope)[1:][::-1], no.norm_modulate_fwd(x, gb, C, slope, mean, istd)[1:][::-1]):
            share = float(no.near_zero(t, mag).mean())
            worst = max(worst, share)
            assert share <= no.FLIP_CAP, (no.flat_name(case), share)
    for case in no.UP2_CASES:
        C, (B, H, W), _, slope = case
        x, gb, gy, mean, istd = no.spade_inputs(B * H * W, C, no.case_seed("up2", C, B, H, W), rows_x=B * H * W // 4)
        _, mag, t = no.norm_modulate_fwd(x, gb, C, slope, mean, istd, (B, H, W))
        share = float(no.near_zero(t, mag).mean())
        worst = max(worst, share)
        assert share <= no.FLIP_CAP, (no.up2_name(case), share)
    print("largest near-zero share: %.3e" % worst)


# ------------------------------------------------------------------------------------------------ _rows_view
def test_rows_view_keeps_aligned_views_and_copies_the_rest():
    """Pure stride logic, run on CPU tensors: a channels-last channel slice that starts on a 16-byte boundary is passed through
    with its row stride; one that starts at a channel that is no multiple of 4, or a tensor that is not channels-last, is copied."""
    from emlight_amd.GenProjector.spherenet import _rows_view
    base = torch.arange(2 * 16 * 3 * 5, dtype=torch.float32).view(2, 3, 5, 16).permute(0, 3, 1, 2)   # (2, 16, 3, 5) channels-last
    assert base.data_ptr() % 16 == 0
    v, ld = _rows_view(base)
    assert v.data_ptr() == base.data_ptr() and ld == 16
    for c0 in (0, 4, 8):                                    # aligned slices: kept as views
        s = base[:, c0:c0 + 8]
        v, ld = _rows_view(s)
        assert v.data_ptr() == s.data_ptr() and ld == 16 and v.data_ptr() % 16 == 0
    for c0 in (1, 2, 3, 6):                                 # 4, 8 or 12 bytes off a boundary: copied
        s = base[:, c0:c0 + 4]
        assert s.stride(3) % 4 == 0 and s.data_ptr() % 16 != 0
        v, ld = _rows_view(s)
        assert v.data_ptr() != s.data_ptr() and v.data_ptr() % 16 == 0 and ld == 4 and torch.equal(v, s)
        assert v.stride(1) == 1
    nchw = torch.randn(2, 8, 3, 5)                          # not channels-last: copied
    v, ld = _rows_view(nchw)
    assert v.data_ptr() != nchw.data_ptr() and ld == 8 and v.stride(1) == 1 and torch.equal(v, nchw)
    big = torch.randn(7, 3, 5, 8)                           # B = 1: the batch stride is never used
    one = big.permute(0, 3, 1, 2)[2:7:9]
    assert one.shape[0] == 1 and one.stride(0) != 3 * 5 * 8
    v, ld = _rows_view(one)
    assert v.data_ptr() == one.data_ptr() and ld == 8
    flat = torch.randn(2 * 3 * 5 * 8 + 2)                   # dense, but 8 bytes into its storage: a copy with its own start
    off = flat[2:].view(2, 3, 5, 8).permute(0, 3, 1, 2)
    v, ld = _rows_view(off)
    assert v.data_ptr() % 16 == 0 and ld == 8 and torch.equal(v, off)
