"""GPU: the thirteen entry points of csrc/spade.hip and csrc/instance_norm.hip through the C ABI, one launcher at a time, against
the float64 restatement of tests/norm_oracle.py (itself checked against float64 autograd in tests/test_norm_oracle.py).

What no other test does: channel counts whose 4-channel groups are not a power of two (idle column lanes), a second trip over the
channel groups with one live lane (C = 1028), row counts below and beside the rows a block covers per pass, grids larger than the
rows need (such a block must leave a zero partial row), leading dimensions above their minimum with the data a column slice of a
larger buffer (no other test hands these six entry points a padded ``ld``; inputs carry NaN and outputs a sentinel in the padding),
statistics of constant, far-offset, tiny and huge channels, one row, and the eval-mode ``sums == NULL`` branch at ragged shapes.

Bounds are derived, not tuned (u = 2^-24, v = 2^-53):
* elementwise: ``|got - want| <= k u magnitude`` with k = the f32 roundings of the formula + 2 (``norm_oracle.K``, counted in the
  oracle's docstrings: modulate forward 3 + 2, its dxn 3 + 2, dgamma 2 + 2, dbeta 1 + 2; with the normalisation inline forward
  5 + 2, dgamma 4 + 2; bn_bwd_apply 8 + 2, 1 + 2 in eval mode, 11 + 2 and 4 + 2 with the four children of the upsample;
  InstanceNorm forward 3 + 2, backward 13 + 2) and the magnitude the sum of the absolute terms the kernel rounds;
* sums accumulated in f64: ``|got - want| <= n v sum|term|`` for n terms, whatever the order; bit-identical run to run;
* mean / istd / running buffers / the InstanceNorm record: one f32 rounding of the float64 value computed from the SAME sums,
  plus what float64 leaves open in ``q/n - mean^2`` (``norm_oracle.stats_from_sums``), carried as an interval for istd;
* the only elements ever skipped: the SPADE backward (and the forward at slope 0) where the float64 pre-activation lies within
  16 u magnitudes of zero; their share is asserted <= 0.1 % per case (a condition on the inputs, checked on the CPU).
Every pointer handed to a kernel is 16-byte aligned and every size in range."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import norm_oracle as no

pytestmark = pytest.mark.gpu
DEV = "cuda"
EML_EINVAL = -1
SENT = -7.5          # outputs are pre-filled with it: padding columns must still hold it afterwards
EPS = 1e-5
U24, U53 = no.U24, no.U53
f = ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    from emlight_amd import _lib
    return _lib


class Buf:
    """A (rows, ld) f32 device buffer whose columns [off, off + width) are the tensor a kernel sees (off = 4 floats -- still
    16-byte aligned -- whenever the padding allows it).  Inputs: the data, NaN elsewhere.  Outputs: SENT everywhere."""

    def __init__(self, rows, width, ld, data=None):
        assert ld >= width and ld % 4 == 0
        self.rows, self.width, self.ld = rows, width, ld
        self.off = 4 if ld >= width + 4 else 0
        self.t = torch.full((rows, ld), float("nan") if data is not None else SENT, dtype=torch.float32, device=DEV)
        if data is not None:
            assert data.shape == (rows, width) and data.dtype == np.float32
            self.t[:, self.off:self.off + width] = torch.from_numpy(data).to(DEV)
        addr = self.t.data_ptr() + 4 * self.off
        assert addr % 16 == 0
        self.ptr = ctypes.c_void_p(addr)

    def host(self):
        """(rows, ld - off) view of what the kernel addresses: the first ``width`` columns count"""
        return self.t.cpu().numpy()[:, self.off:]

    def value(self):
        return self.host()[:, :self.width]

    def padding_holds(self, fill=SENT):
        h = self.t.cpu().numpy()
        pad = np.concatenate([h[:, :self.off], h[:, self.off + self.width:]], 1)
        return bool(np.isnan(pad).all()) if np.isnan(fill) else bool((pad == fill).all())


def _call(lib, name, *args):
    lib.check(getattr(lib.lib(), name)(*args, lib.current_stream()), name)
    torch.cuda.synchronize()


def _s32(slope):
    """the slope as the f32 a kernel is handed (0.2 is not one)"""
    return float(np.float32(slope))


def _lds(kind, n):
    """n leading-dimension kinds, rotated from the case's one: a case pads some of its tensors and leaves others dense"""
    i = no.LD_KINDS.index(kind)
    return [no.LD_KINDS[(i + k) % 3] for k in range(n)]


def _elementwise(name, kkey, got, want, mag, skip=None):
    """|got - want| <= K u magnitude everywhere outside ``skip``; prints the largest error as a fraction of the bound."""
    got = np.asarray(got, np.float64)
    bound = no.K[kkey] * U24 * mag
    err = np.abs(got - want)
    assert np.isfinite(got).all(), name
    keep = np.ones(err.shape, bool) if skip is None else ~skip
    ratio = float((err[keep] / np.maximum(bound[keep], 1e-300)).max()) if keep.any() else 0.0
    print("RATIO %s %.4f" % (name, ratio))
    bad = keep & (err > bound)
    assert not bad.any(), "%s: %d elements beyond %d u magnitude, worst ratio %.3f" % (name, int(bad.sum()), no.K[kkey], ratio)


def _skip_share(name, t, tmag):
    skip = no.near_zero(t, tmag)
    share = float(skip.mean())
    print("EXCLUDED %s %.3e" % (name, share))
    assert share <= no.FLIP_CAP, (name, share)
    return skip


def _f64_sums(name, got, want, mag, n):
    bound = n * U53 * mag
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("RATIO %s %.4f" % (name, ratio))
    assert np.isfinite(got).all() and (err <= bound).all(), "%s: worst ratio %.3f of %d v sum|term|" % (name, ratio, n)


def _idle_blocks_are_zero(partials, rows, C):
    """A block past the last row pass owns no row: its whole partial row is exactly 0 (and nothing is left unwritten)."""
    rpp = no.col_map(C)[1]
    owning = (rows + rpp - 1) // rpp
    assert not np.isnan(partials).any()
    assert (partials[owning:] == 0).all()


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ statistics
def _stats(lib, xb, rows, C, grid):
    """eml_bn_stats_f32 + eml_bn_fold_f64 -> (partials (grid, C, 2), sums (2C + 1) with the count in the last slot), on the host"""
    p = lib.ptr
    partials = torch.full((grid, C, 2), float("nan"), dtype=torch.float64, device=DEV)
    _call(lib, "eml_bn_stats_f32", xb.ptr, xb.ld, rows, C, p(partials), grid)
    sums = torch.full((2 * C + 1,), float(rows), dtype=torch.float64, device=DEV)
    _call(lib, "eml_bn_fold_f64", p(partials), grid, 2 * C, p(sums))
    return partials.cpu().numpy(), sums.cpu().numpy()


def _finalize_and_check(lib, name, sums, rows, C, eps=EPS, running=True, seed=0):
    p = lib.ptr
    r = np.random.RandomState(seed)
    rm, rv = r.randn(C).astype(np.float32), (r.rand(C) + 0.5).astype(np.float32)
    mom = np.float32(0.1)
    mean, istd = (torch.full((C + 4,), SENT, device=DEV) for _ in range(2))
    drm, drv, dsums = _dev32(rm), _dev32(rv), _dev64(sums)
    _call(lib, "eml_bn_finalize_f32", p(dsums), C, f(eps), f(mom), p(mean), p(istd), p(drm) if running else None,
          p(drv) if running else None)
    mean, istd = mean.cpu().numpy(), istd.cpu().numpy()
    assert (mean[C:] == SENT).all() and (istd[C:] == SENT).all()
    table = sums[:2 * C].reshape(C, 2)
    args = (table, rows, np.float32(eps), mom) + ((rm, rv) if running else ())
    wm, wi, wrm, wrv = no.bn_finalize(*args)
    tm, (lo, hi), trm, trv = no.bn_finalize_tol(*args)
    assert np.isfinite(mean[:C]).all() and np.isfinite(istd[:C]).all(), name
    assert (np.abs(mean[:C] - wm) <= tm).all(), "%s mean: %.3e" % (name, float(np.abs(mean[:C] - wm).max()))
    assert ((lo <= istd[:C]) & (istd[:C] <= hi)).all(), "%s istd: %s not in [%s, %s]" % (name, istd[:C], lo, hi)
    print("RATIO eml_bn_finalize_f32.mean %.4f" % float((np.abs(mean[:C] - wm) / np.maximum(tm, 1e-300)).max()))
    if running:
        grm, grv = drm.cpu().numpy(), drv.cpu().numpy()
        assert np.isfinite(grm).all() and np.isfinite(grv).all(), name
        assert (np.abs(grm - wrm) <= trm).all(), "%s running mean: %.3e" % (name, float(np.abs(grm - wrm).max()))
        assert (np.abs(grv - wrv) <= trv).all(), "%s running var: %.3e" % (name, float(np.abs(grv - wrv).max()))
    else:
        assert np.array_equal(drm.cpu().numpy(), rm) and np.array_equal(drv.cpu().numpy(), rv)
    return mean[:C], istd[:C]


@pytest.mark.parametrize("case", no.FLAT_CASES, ids=no.flat_name)
def test_batch_statistics(lib, case):
    """eml_bn_stats_f32 -> eml_bn_fold_f64 -> eml_bn_finalize_f32: the folded (sum, sum of squares) within rows * 2^-53 * sum|term|
    of the exact sums (f64 accumulation of f32 data, any order) and bit-identical run to run; blocks beyond the rows leave zeros;
    mean, istd and the running buffers one f32 rounding from the float64 values of those sums, with and without running buffers."""
    C, rk, ldk, gk, _ = case
    rows, ld, grid = no.rows_of(rk, C), no.ld_of(ldk, C), no.grid_of(gk, no.rows_of(rk, C), C)
    x = no.spade_inputs(rows, C, no.case_seed("flat", C, rk))[0]
    xb = Buf(rows, C, ld, x)
    partials, sums = _stats(lib, xb, rows, C, grid)
    _idle_blocks_are_zero(partials, rows, C)
    assert sums[2 * C] == rows                                   # the fold writes its n columns and nothing behind them
    want, mag = no.bn_sums(xb.host(), C)
    _f64_sums("eml_bn_stats_f32+fold", sums[:2 * C].reshape(C, 2), want, mag, rows)
    again = _stats(lib, xb, rows, C, grid)
    assert np.array_equal(again[0], partials) and np.array_equal(again[1], sums)
    _finalize_and_check(lib, no.flat_name(case), sums, rows, C, running=True, seed=C + rows)
    _finalize_and_check(lib, no.flat_name(case), sums, rows, C, running=False, seed=C + rows)


@pytest.mark.parametrize("R,nk", no.FOLD_CASES)
def test_fold_alone(lib, R, nk):
    """eml_bn_fold_f64 on its own: R partial rows of n columns around its 16-row slices and 16-column blocks, against the
    exact column sums within R * 2^-53 * sum|term|; nothing written behind column n."""
    C = 12
    n = {"1": 1, "15": 15, "16": 16, "17": 17, "2C": 2 * C, "4C+1": 4 * C + 1}[nk]
    r = np.random.RandomState(R * 100 + n)
    part = r.randn(R, n) * np.exp(3 * r.randn(R, n))
    sums = torch.full((n + 3,), SENT, dtype=torch.float64, device=DEV)
    dp = _dev64(part)
    _call(lib, "eml_bn_fold_f64", lib.ptr(dp), R, n, lib.ptr(sums))
    got = sums.cpu().numpy()
    assert (got[n:] == SENT).all()
    exact = part.astype(np.longdouble).sum(0).astype(np.float64)
    _f64_sums("eml_bn_fold_f64", got[:n], exact, np.abs(part).sum(0), R)
    _f64_sums("eml_bn_fold_f64.vs_numpy", got[:n], part.sum(axis=0), np.abs(part).sum(0), 2 * R)   # numpy's own sum rounds too


HARD = ("zero", "const1e3", "offset", "tiny", "huge", "one_row", "inexact_const")


@pytest.mark.parametrize("kind", HARD)
def test_hard_statistics(lib, kind):
    """One small shape each (67 rows, or 1, of C = 12 with ld = 16):
    * zero / const1e3: a constant channel -- the variance is 0, istd = 1/sqrt(eps); a variance formed from rounded means, or an
      istd without eps, shows here;
    * offset: mean 1e3, spread 1e-2 -- squares accumulated in f32 lose the variance entirely (1e6 against 1e-4);
    * tiny / huge: values near 1e-20 / 1e18 -- the squares are finite in f64 only: an f32 square is 0 / inf;
    * one_row: n = 1 -- a division by n - 1 = 0 for the unbiased variance makes the running variance NaN;
    * inexact_const: channels constant at values whose sums round (k * 0.1 + 1000) with eps = 1e-30 -- q/n - mean^2 is rounding
      noise of either sign around 0: without the clamp at 0 a negative one makes istd NaN."""
    rows, C, ld = (1 if kind == "one_row" else 67), 12, 16
    r = np.random.RandomState(HARD.index(kind))
    z = r.randn(rows, C)
    x = {"zero": 0 * z, "const1e3": 0 * z + 1e3, "offset": 1e3 + 1e-2 * z, "tiny": 1e-20 * (1 + 0.3 * z),
         "huge": 1e18 * (1 + 0.3 * z), "one_row": z, "inexact_const": 0 * z + 1000 + 0.1 * np.arange(1, C + 1)}[kind]
    x = x.astype(np.float32)
    xb = Buf(rows, C, ld, x)
    grid = no.stats_grid(rows, C)
    partials, sums = _stats(lib, xb, rows, C, grid)
    want, mag = no.bn_sums(x)
    _f64_sums("eml_bn_stats_f32+fold.%s" % kind, sums[:2 * C].reshape(C, 2), want, mag, rows)
    eps = 1e-30 if kind == "inexact_const" else EPS
    mean, istd = _finalize_and_check(lib, kind, sums, rows, C, eps=eps, running=True, seed=5)
    if kind in ("zero", "const1e3", "one_row"):
        assert np.array_equal(mean, x[0])
    if kind == "offset":   # the true variance is about 1e-4: far from the 0 an f32 accumulation leaves
        assert (np.abs(istd / (1 / np.sqrt(x.astype(np.float64).var(0) + EPS)) - 1) < 1e-3).all()


# ------------------------------------------------------------------------------------------------------------ flat elementwise
@functools.lru_cache(None)
def _flat_inputs(C, rk):
    return no.spade_inputs(no.rows_of(rk, C), C, no.case_seed("flat", C, rk))


@pytest.mark.parametrize("case", no.FLAT_CASES, ids=no.flat_name)
def test_modulate_forward_and_backward(lib, case):
    """eml_spade_modulate_{fwd,bwd}_f32 on an already normalised input, every tensor with a leading dimension of its own."""
    C, rk, ldk, _, slope = case
    rows, slope = no.rows_of(rk, C), _s32(slope)
    x, gb, gy, _, _ = _flat_inputs(C, rk)
    kx, kg, ky, ku, kd, kdg = _lds(ldk, 3) + _lds(ldk, 3)[::-1]
    xb, gbb, gyb = Buf(rows, C, no.ld_of(kx, C), x), Buf(rows, 2 * C, no.ld_of(kg, 2 * C), gb), Buf(rows, C, no.ld_of(ku, C), gy)
    yb, dxb, dgb = Buf(rows, C, no.ld_of(ky, C)), Buf(rows, C, no.ld_of(kd, C)), Buf(rows, 2 * C, no.ld_of(kdg, 2 * C))
    _call(lib, "eml_spade_modulate_fwd_f32", xb.ptr, xb.ld, gbb.ptr, gbb.ld, yb.ptr, yb.ld, rows, C, f(slope))
    want, mag, t = no.modulate_fwd(xb.host(), gbb.host(), C, slope)
    skip = _skip_share("modulate", t, mag)
    _elementwise("eml_spade_modulate_fwd_f32", "modulate_fwd", yb.value(), want, mag, skip if slope == 0 else None)
    assert yb.padding_holds() and xb.padding_holds(np.nan) and gbb.padding_holds(np.nan)
    _call(lib, "eml_spade_modulate_bwd_f32", gyb.ptr, gyb.ld, xb.ptr, xb.ld, gbb.ptr, gbb.ld, dxb.ptr, dxb.ld, dgb.ptr, dgb.ld,
          rows, C, f(slope))
    b = no.modulate_bwd(gyb.host(), xb.host(), gbb.host(), C, slope)
    _elementwise("eml_spade_modulate_bwd_f32.dxn", "modulate_bwd.dxn", dxb.value(), *b["dxn"], skip)
    _elementwise("eml_spade_modulate_bwd_f32.dgamma", "modulate_bwd.dgamma", dgb.value()[:, :C], *b["dgamma"], skip)
    _elementwise("eml_spade_modulate_bwd_f32.dbeta", "modulate_bwd.dbeta", dgb.value()[:, C:], *b["dbeta"], skip)
    assert dxb.padding_holds() and dgb.padding_holds()


@pytest.mark.parametrize("case", no.FLAT_CASES, ids=no.flat_name)
def test_norm_modulate_forward(lib, case):
    """eml_spade_norm_modulate_fwd_f32 with the f32 (mean, istd) it is handed."""
    C, rk, ldk, _, slope = case
    rows, slope = no.rows_of(rk, C), _s32(slope)
    x, gb, _, mean, istd = _flat_inputs(C, rk)
    kx, kg, ky = _lds(ldk, 3)
    xb, gbb, yb = Buf(rows, C, no.ld_of(kx, C), x), Buf(rows, 2 * C, no.ld_of(kg, 2 * C), gb), Buf(rows, C, no.ld_of(ky, C))
    dm, di = _dev32(mean), _dev32(istd)
    _call(lib, "eml_spade_norm_modulate_fwd_f32", xb.ptr, xb.ld, gbb.ptr, gbb.ld, yb.ptr, yb.ld, rows, C, f(slope), lib.ptr(dm),
          lib.ptr(di))
    want, mag, t = no.norm_modulate_fwd(xb.host(), gbb.host(), C, slope, mean, istd)
    skip = _skip_share("norm_modulate", t, mag)
    _elementwise("eml_spade_norm_modulate_fwd_f32", "norm_modulate_fwd", yb.value(), want, mag, skip if slope == 0 else None)
    assert yb.padding_holds()


@pytest.mark.parametrize("case", no.FLAT_CASES, ids=no.flat_name)
def test_bn_backward_apply(lib, case):
    """eml_bn_bwd_apply_f32 out of place, with dx aliasing dxn (how the trainer calls it) and in eval mode (sums == NULL)."""
    C, rk, ldk, _, _ = case
    rows = no.rows_of(rk, C)
    x, _, dxn, mean, istd = _flat_inputs(C, rk)
    r = np.random.RandomState(rows + C)
    sums = np.concatenate([(r.randn(2 * C) * np.sqrt(rows)), [float(rows)]])
    kd, kx, ko = _lds(ldk, 3)
    xb = Buf(rows, C, no.ld_of(kx, C), x)
    dm, di, ds = _dev32(mean), _dev32(istd), _dev64(sums)
    p = lib.ptr
    for mode in ("train", "alias", "eval"):
        db = Buf(rows, C, no.ld_of(kd, C), dxn)
        ob = db if mode == "alias" else Buf(rows, C, no.ld_of(ko, C))
        _call(lib, "eml_bn_bwd_apply_f32", db.ptr, db.ld, xb.ptr, xb.ld, rows, C, p(dm), p(di), None if mode == "eval" else p(ds),
              ob.ptr, ob.ld)
        table = None if mode == "eval" else sums[:2 * C].reshape(C, 2)
        want, mag = no.bn_bwd_apply(dxn, xb.host(), C, mean, istd, table, rows)
        _elementwise("eml_bn_bwd_apply_f32.%s" % mode, "bn_bwd_apply.eval" if mode == "eval" else "bn_bwd_apply", ob.value(), want, mag)
        assert ob.padding_holds(np.nan if mode == "alias" else SENT)
        if mode != "alias":
            assert np.array_equal(db.value(), dxn)


# ------------------------------------------------------------------------------------------------------------ the dense backward
def _dense_backward(lib, C, bhw, up2, slope, gk, inputs):
    """eml_spade_norm_modulate_bwd_cols_f32 and _bwd_y_f32 on one case (the forward that feeds _bwd_y its output is checked too),
    then BatchNorm's backward from the folded sums.  -> nothing; asserts."""
    p = lib.ptr
    B, H, W = bhw
    rows, slope = B * H * W, _s32(slope)
    rows_x = rows // 4 if up2 else rows
    x, gb, gy, mean, istd = inputs
    grid = no.grid_of(gk, rows, C)
    dx_, dgb_, dgy, dm, di = _dev32(x), _dev32(gb), _dev32(gy), _dev32(mean), _dev32(istd)
    o_up2 = bhw if up2 else None
    tag = "up2" if up2 else "flat"
    # forward (dense): the output whose sign _bwd_y reads
    y = torch.full((rows, C), SENT, device=DEV)
    if up2:
        _call(lib, "eml_spade_norm_modulate_up2_fwd_f32", p(dx_), p(dgb_), p(y), B, H, W, C, f(slope), p(dm), p(di))
    else:
        _call(lib, "eml_spade_norm_modulate_fwd_f32", p(dx_), C, p(dgb_), 2 * C, p(y), C, rows, C, f(slope), p(dm), p(di))
    want, mag, t = no.norm_modulate_fwd(x, gb, C, slope, mean, istd, o_up2)
    skip = _skip_share("norm_modulate.%s" % tag, t, mag)
    fwd = "eml_spade_norm_modulate_up2_fwd_f32" if up2 else "eml_spade_norm_modulate_fwd_f32.dense"
    _elementwise(fwd, "norm_modulate_fwd", y.cpu().numpy(), want, mag, skip if slope == 0 else None)

    def run(entry):
        dxn, dgb = torch.full((rows, C), SENT, device=DEV), torch.full((rows, 2 * C), SENT, device=DEV)
        partials = torch.full((grid, 4 * C + 1), float("nan"), dtype=torch.float64, device=DEV)
        if entry.endswith("_y_f32"):
            gamma = dgb_[:, :C].contiguous()
            _call(lib, entry, p(dgy), p(dx_), p(gamma), p(y), p(dxn), p(dgb), B, H, W, C, int(up2), f(slope), p(dm), p(di),
                  p(partials), grid)
        else:
            _call(lib, entry, p(dgy), p(dx_), p(dgb_), p(dxn), p(dgb), B, H, W, C, int(up2), f(slope), p(dm), p(di), p(partials), grid)
        folded = torch.full((4 * C + 1 + 3,), SENT, dtype=torch.float64, device=DEV)
        _call(lib, "eml_bn_fold_f64", p(partials), grid, 4 * C + 1, p(folded))
        return dxn, dgb.cpu().numpy(), partials.cpu().numpy(), folded.cpu().numpy()

    cols = "eml_spade_norm_modulate_bwd_cols_f32"
    dxn_dev, dgb, partials, folded = run(cols)
    dxn = dxn_dev.cpu().numpy()
    b = no.norm_modulate_bwd(gy, x, gb, C, slope, mean, istd, o_up2)
    _elementwise("%s.%s.dxn" % (cols, tag), "norm_modulate_bwd.dxn", dxn, *b["dxn"], skip)
    _elementwise("%s.%s.dgamma" % (cols, tag), "norm_modulate_bwd.dgamma", dgb[:, :C], *b["dgamma"], skip)
    _elementwise("%s.%s.dbeta" % (cols, tag), "norm_modulate_bwd.dbeta", dgb[:, C:], *b["dbeta"], skip)
    # partial rows: (C, 2) | the count's slot | (C, 2); blocks without rows are all zero; the fold keeps to its 4C + 1 columns
    _idle_blocks_are_zero(partials, rows, C)
    assert (partials[:, 2 * C] == 0).all() and folded[2 * C] == 0 and (folded[4 * C + 1:] == SENT).all()
    # the four column sums against sums of the device's OWN outputs, xhat recomputed in f32 as the kernel forms it (a subtraction
    # followed by a multiplication cannot be contracted): an activation flip cannot disturb this
    xs = no.up2_rows(x, bhw, C) if up2 else x
    xhat32 = ((xs - mean[None, :]) * istd[None, :]).astype(np.float32)
    assert xhat32.dtype == np.float32 and (xs - mean[None, :]).dtype == np.float32
    L = np.longdouble
    terms = [dxn.astype(L), dxn.astype(L) * xhat32.astype(L), dgb[:, :C].astype(L), dgb[:, C:].astype(L)]
    want4 = np.stack([v.sum(0) for v in terms], 1).astype(np.float64)
    mag4 = np.stack([np.abs(v).sum(0) for v in terms], 1).astype(np.float64)
    got4 = np.concatenate([folded[:2 * C].reshape(C, 2), folded[2 * C + 1:4 * C + 1].reshape(C, 2)], 1)
    _f64_sums("%s.%s.sums" % (cols, tag), got4, want4, mag4, rows)
    # the same pass with the mask taken from the stored output: bit for bit
    ydxn, ydgb, ypart, yfold = run("eml_spade_norm_modulate_bwd_y_f32")
    assert np.array_equal(ydxn.cpu().numpy(), dxn) and np.array_equal(ydgb, dgb), "bwd_y differs from bwd_cols (slope %g)" % slope
    assert np.array_equal(ypart, partials) and np.array_equal(yfold, folded)
    # BatchNorm's backward from those sums with the count in its slot, as the trainer calls it
    sums = folded[:2 * C + 1].copy()
    sums[2 * C] = rows
    ds = _dev64(sums)
    for mode in ("train", "eval"):
        if up2:
            out = torch.full((rows_x, C), SENT, device=DEV)
            _call(lib, "eml_bn_bwd_apply_up2_f32", p(dxn_dev), p(dx_), B, H, W, C, p(dm), p(di), p(ds) if mode == "train" else None, p(out))
            key, name = "bn_bwd_apply_up2", "eml_bn_bwd_apply_up2_f32"
        else:
            out = torch.full((rows, C), SENT, device=DEV)
            _call(lib, "eml_bn_bwd_apply_f32", p(dxn_dev), C, p(dx_), C, rows, C, p(dm), p(di), p(ds) if mode == "train" else None,
                  p(out), C)
            key, name = "bn_bwd_apply", "eml_bn_bwd_apply_f32.dense"
        table = sums[:2 * C].reshape(C, 2) if mode == "train" else None
        want, mag = no.bn_bwd_apply(dxn, x, C, mean, istd, table, rows, o_up2)
        _elementwise("%s.%s" % (name, mode), key + (".eval" if mode == "eval" else ""), out.cpu().numpy(), want, mag)


@pytest.mark.parametrize("case", no.FLAT_CASES, ids=no.flat_name)
def test_dense_backward_flat(lib, case):
    """bwd_cols / bwd_y without the upsample, (B, H, W) = (1, 1, rows): values against the oracle, the four per-channel sums
    against sums of the device's own outputs in f64, bwd_y bit-identical to bwd_cols, zero partial rows of idle blocks."""
    C, rk, _, gk, slope = case
    _dense_backward(lib, C, (1, 1, no.rows_of(rk, C)), False, slope, gk, _flat_inputs(C, rk))


@pytest.mark.parametrize("case", no.UP2_CASES, ids=no.up2_name)
def test_dense_backward_with_the_upsample_folded_in(lib, case):
    """The same with x the map BEFORE the nearest x2 upsample (eml_spade_norm_modulate_up2_fwd_f32, up2 = 1 in both backwards,
    eml_bn_bwd_apply_up2_f32).  B > 1 and H != W: a wrong source row is invisible at B = 1 or on square maps."""
    C, (B, H, W), gk, slope = case
    inputs = no.spade_inputs(B * H * W, C, no.case_seed("up2", C, B, H, W), rows_x=B * H * W // 4)
    _dense_backward(lib, C, (B, H, W), True, slope, gk, inputs)


# ------------------------------------------------------------------------------------------------------------ InstanceNorm
IN_RUNS = [(i, None) for i in range(len(no.IN_CASES))] + [(i, h) for i in (2, 7) for h in ("const", "offset")]


def _in_name(run):
    return no.in_name(no.IN_CASES[run[0]]) + ("-" + run[1] if run[1] else "")


@pytest.mark.parametrize("run", IN_RUNS, ids=_in_name)
def test_instance_norm(lib, run):
    """eml_instance_norm_act_{fwd,bwd}_f32 in both layouts: HW below, beside and at the 32 pixel lanes, one live channel group of
    eight (C = 4), HW = 1; a constant plane and one with mean 1e3 / spread 1e-2.  The record against the oracle's to one f32
    rounding; the output and dx against the oracle evaluated WITH the record the kernel wrote.  xhat = (x - mean) * istd keeps the
    sign of x - mean in f32 and in f64 alike, so no element is skipped."""
    i, hard = run
    case = no.IN_CASES[i]
    cl, (B, C, HW) = case
    slope = _s32(no.IN_SLOPES[i])
    p = lib.ptr
    x, gy = no.instance_inputs(case, no.case_seed("in", i), hard)
    dxv, dgy = _dev32(x), _dev32(gy)
    y, dx = (torch.full(x.shape, SENT, device=DEV) for _ in range(2))
    stats = torch.full((B * C * 2 + 4,), SENT, device=DEV)
    _call(lib, "eml_instance_norm_act_fwd_f32", p(dxv), p(y), p(stats), B, HW, C, cl, f(EPS), f(slope))
    sh = stats.cpu().numpy()
    assert (sh[B * C * 2:] == SENT).all()
    rec = sh[:B * C * 2].reshape(B, C, 2)
    want_rec, tm, lo, hi = no.instance_norm_record(x, EPS, cl)
    assert np.isfinite(rec).all()
    assert (np.abs(rec[:, :, 0] - want_rec[:, :, 0]) <= tm).all(), float(np.abs(rec[:, :, 0] - want_rec[:, :, 0]).max())
    assert ((lo <= rec[:, :, 1]) & (rec[:, :, 1] <= hi)).all(), (rec[:, :, 1], lo, hi)
    if hard == "const" or HW == 1:
        assert rec[0, 0, 0] == x[0, 0, 0]                         # a constant plane: its mean is the value, xhat = 0
    want, mag, _ = no.instance_norm_act_fwd(x, EPS, slope, cl, stats=rec)
    _elementwise("eml_instance_norm_act_fwd_f32.%s" % ("nhwc" if cl else "nchw"), "instance_norm_fwd", y.cpu().numpy(), want, mag)
    _call(lib, "eml_instance_norm_act_bwd_f32", p(dgy), p(dxv), p(stats), p(dx), B, HW, C, cl, f(slope))
    want, mag, _ = no.instance_norm_act_bwd(gy, x, rec, slope, cl)
    _elementwise("eml_instance_norm_act_bwd_f32.%s" % ("nhwc" if cl else "nchw"), "instance_norm_bwd", dx.cpu().numpy(), want, mag)
    assert np.array_equal(stats.cpu().numpy(), sh)                # the backward only reads the record


def test_instance_norm_refusals_and_the_empty_batch(lib):
    L, p = lib.lib(), lib.ptr
    st = lib.current_stream()
    x = torch.randn(2, 31, 8, device=DEV)
    y, dx, stats = torch.full_like(x, SENT), torch.full_like(x, SENT), torch.full((2 * 8 * 2,), SENT, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((y == SENT).all()) and bool((dx == SENT).all()) and bool((stats == SENT).all())

    assert L.eml_instance_norm_act_fwd_f32(p(x), p(y), p(stats), 0, 31, 8, 1, f(EPS), f(0.2), st) == 0 and untouched()      # B = 0
    assert L.eml_instance_norm_act_bwd_f32(p(x), p(x), p(stats), p(dx), 0, 31, 8, 0, f(0.2), st) == 0 and untouched()
    assert L.eml_instance_norm_act_fwd_f32(p(x), p(y), p(stats), 2, 31, 6, 1, f(EPS), f(0.2), st) == EML_EINVAL and untouched()   # C % 4
    assert L.eml_instance_norm_act_bwd_f32(p(x), p(x), p(stats), p(dx), 2, 31, 6, 1, f(0.2), st) == EML_EINVAL and untouched()
    for slope in (-0.1, 1.5, float("nan")):
        for cl in (0, 1):
            assert L.eml_instance_norm_act_fwd_f32(p(x), p(y), p(stats), 2, 31, 8, cl, f(EPS), f(slope), st) == EML_EINVAL
            assert L.eml_instance_norm_act_bwd_f32(p(x), p(x), p(stats), p(dx), 2, 31, 8, cl, f(slope), st) == EML_EINVAL
    assert untouched()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_spade_argument_refusals(lib):
    """EML_EINVAL, and every output still holds its sentinel: a leading dimension below its minimum or no multiple of 4, C = 2,
    odd H or W with the upsample, eps = 0 and a running mean without a running variance in finalize."""
    L, p = lib.lib(), lib.ptr
    st = lib.current_stream()
    C, rows, B, H, W = 8, 24, 1, 4, 6
    a = torch.randn(rows, 4 * C, device=DEV)                       # any input; wider than any leading dimension named below
    v = torch.rand(C, device=DEV) + 0.5
    sums = _dev64(np.concatenate([np.ones(2 * C), [rows]]))
    outs = [torch.full((rows, 4 * C), SENT, device=DEV) for _ in range(2)]
    part = torch.full((4, 4 * C + 1), SENT, dtype=torch.float64, device=DEV)
    vec = [torch.full((C,), SENT, device=DEV) for _ in range(4)]
    o0, o1 = outs
    calls = []
    for bad, bad2 in ((C - 4, 2 * C - 4), (C + 2, 2 * C + 2)):     # below the minimum; not a multiple of 4 (of C, of 2C)
        calls += [
            lambda bad=bad: L.eml_spade_modulate_fwd_f32(p(a), bad, p(a), 2 * C, p(o0), C, rows, C, f(0.2), st),
            lambda bad2=bad2: L.eml_spade_modulate_fwd_f32(p(a), C, p(a), bad2, p(o0), C, rows, C, f(0.2), st),
            lambda bad=bad: L.eml_spade_modulate_fwd_f32(p(a), C, p(a), 2 * C, p(o0), bad, rows, C, f(0.2), st),
            lambda bad=bad: L.eml_spade_modulate_bwd_f32(p(a), bad, p(a), C, p(a), 2 * C, p(o0), C, p(o1), 2 * C, rows, C, f(0.2), st),
            lambda bad=bad: L.eml_spade_modulate_bwd_f32(p(a), C, p(a), bad, p(a), 2 * C, p(o0), C, p(o1), 2 * C, rows, C, f(0.2), st),
            lambda bad2=bad2: L.eml_spade_modulate_bwd_f32(p(a), C, p(a), C, p(a), bad2, p(o0), C, p(o1), 2 * C, rows, C, f(0.2), st),
            lambda bad=bad: L.eml_spade_modulate_bwd_f32(p(a), C, p(a), C, p(a), 2 * C, p(o0), bad, p(o1), 2 * C, rows, C, f(0.2), st),
            lambda bad2=bad2: L.eml_spade_modulate_bwd_f32(p(a), C, p(a), C, p(a), 2 * C, p(o0), C, p(o1), bad2, rows, C, f(0.2), st),
            lambda bad=bad: L.eml_spade_norm_modulate_fwd_f32(p(a), bad, p(a), 2 * C, p(o0), C, rows, C, f(0.2), p(v), p(v), st),
            lambda bad2=bad2: L.eml_spade_norm_modulate_fwd_f32(p(a), C, p(a), bad2, p(o0), C, rows, C, f(0.2), p(v), p(v), st),
            lambda bad=bad: L.eml_spade_norm_modulate_fwd_f32(p(a), C, p(a), 2 * C, p(o0), bad, rows, C, f(0.2), p(v), p(v), st),
            lambda bad=bad: L.eml_bn_stats_f32(p(a), bad, rows, C, p(part), 4, st),
            lambda bad=bad: L.eml_bn_bwd_apply_f32(p(a), bad, p(a), C, rows, C, p(v), p(v), p(sums), p(o0), C, st),
            lambda bad=bad: L.eml_bn_bwd_apply_f32(p(a), C, p(a), bad, rows, C, p(v), p(v), p(sums), p(o0), C, st),
            lambda bad=bad: L.eml_bn_bwd_apply_f32(p(a), C, p(a), C, rows, C, p(v), p(v), p(sums), p(o0), bad, st),
        ]
    calls += [                                                      # C = 2
        lambda: L.eml_spade_modulate_fwd_f32(p(a), 4, p(a), 4, p(o0), 4, rows, 2, f(0.2), st),
        lambda: L.eml_spade_modulate_bwd_f32(p(a), 4, p(a), 4, p(a), 4, p(o0), 4, p(o1), 4, rows, 2, f(0.2), st),
        lambda: L.eml_spade_norm_modulate_fwd_f32(p(a), 4, p(a), 4, p(o0), 4, rows, 2, f(0.2), p(v), p(v), st),
        lambda: L.eml_bn_stats_f32(p(a), 4, rows, 2, p(part), 4, st),
        lambda: L.eml_bn_bwd_apply_f32(p(a), 4, p(a), 4, rows, 2, p(v), p(v), p(sums), p(o0), 4, st),
        lambda: L.eml_spade_norm_modulate_up2_fwd_f32(p(a), p(a), p(o0), B, H, W, 2, f(0.2), p(v), p(v), st),
        lambda: L.eml_spade_norm_modulate_bwd_cols_f32(p(a), p(a), p(a), p(o0), p(o1), B, H, W, 2, 0, f(0.2), p(v), p(v), p(part), 4, st),
        lambda: L.eml_spade_norm_modulate_bwd_y_f32(p(a), p(a), p(a), p(a), p(o0), p(o1), B, H, W, 2, 0, f(0.2), p(v), p(v), p(part), 4, st),
        lambda: L.eml_bn_bwd_apply_up2_f32(p(a), p(a), B, H, W, 2, p(v), p(v), p(sums), p(o0), st),
    ]
    for h, w in ((3, 6), (4, 5)):                                   # odd H, odd W with the upsample
        calls += [
            lambda h=h, w=w: L.eml_spade_norm_modulate_up2_fwd_f32(p(a), p(a), p(o0), B, h, w, C, f(0.2), p(v), p(v), st),
            lambda h=h, w=w: L.eml_spade_norm_modulate_bwd_cols_f32(p(a), p(a), p(a), p(o0), p(o1), B, h, w, C, 1, f(0.2), p(v), p(v),
                                                                    p(part), 4, st),
            lambda h=h, w=w: L.eml_spade_norm_modulate_bwd_y_f32(p(a), p(a), p(a), p(a), p(o0), p(o1), B, h, w, C, 1, f(0.2), p(v), p(v),
                                                                 p(part), 4, st),
            lambda h=h, w=w: L.eml_bn_bwd_apply_up2_f32(p(a), p(a), B, h, w, C, p(v), p(v), p(sums), p(o0), st),
        ]
    calls += [                                                      # finalize: eps = 0; a running mean without a running variance
        lambda: L.eml_bn_finalize_f32(p(sums), C, f(0.0), f(0.1), p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), st),
        lambda: L.eml_bn_finalize_f32(p(sums), C, f(EPS), f(0.1), p(vec[0]), p(vec[1]), p(vec[2]), None, st),
    ]
    for n, call in enumerate(calls):
        assert call() == EML_EINVAL, "call %d was not refused" % n
    torch.cuda.synchronize()
    for t in outs + [part] + vec:
        assert bool((t == SENT).all())
