"""Float64 restatement of the SPADE / BatchNorm / InstanceNorm kernels (csrc/spade.hip, csrc/instance_norm.hip), in plain numpy,
written from the formulas and not from the kernels' loops:

    SPADE        y  = leaky_relu(xhat * (1 + gamma) + beta, slope),  xhat = (x - mean) * istd        (gamma | beta = the halves of gb)
    its backward d  = gy * leaky_relu'(t),  dxn = d * (1 + gamma),  dgamma = d * xhat,  dbeta = d
    BatchNorm    dx = istd * (dxn - S1/n - xhat * S2/n),  S1 = sum dxn, S2 = sum dxn * xhat          (sums == None: istd * dxn)
    InstanceNorm the same per (sample, channel) plane, biased variance, with the activation applied to xhat itself.

Every function takes the arrays the entry point takes -- rows of ``ld >= C`` floats, of which the first C count -- and returns float64.
Next to each value comes its MAGNITUDE: the sum of the absolute values of the terms the kernel rounds in f32, so that a test can
state its bound as ``k * 2^-24 * magnitude`` with k counted from the formula.  ``mean`` / ``istd`` are taken AS GIVEN (the f32 the
kernel is handed): the statistics' own rounding is tested on its own and must not leak into the elementwise bounds.

The module also holds the shape lists and the input generators of tests/test_gpu_norm_kernels.py, so that the GPU-free
tests/test_norm_oracle.py can check the condition those inputs have to meet (the share of near-zero pre-activations)."""
import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53
FLIP_WINDOW = 16 * U24      # pre-activations within this many magnitudes of zero may take the other branch in f32
FLIP_CAP = 1e-3             # at most this share of a case's elements may be excluded for it

f64 = np.float64


def _d(a):
    return np.asarray(a, dtype=f64)


def lrelu(t, slope):
    return np.where(t > 0, t, slope * t)


def up2_rows(x, bhw, C):
    """Rows of the nearest x2 upsample of a (B * H/2 * W/2, >= C) map, H and W being the UPSAMPLED size: (B * H * W, C)."""
    B, H, W = bhw
    lo = np.asarray(x)[:, :C].reshape(B, H // 2, W // 2, C)
    return np.repeat(np.repeat(lo, 2, axis=1), 2, axis=2).reshape(B * H * W, C)


# ------------------------------------------------------------------------------------------------------------ statistics
def bn_sums(x, C=None):
    """Per-channel (sum x, sum x^2) of the first C columns of x (rows, ld): ((C, 2) sums, (C, 2) sums of the absolute terms).
    Accumulated in extended precision, so the result is the float64 nearest to the exact sum."""
    C = x.shape[1] if C is None else C
    v = np.asarray(x)[:, :C].astype(np.longdouble)
    s, q = v.sum(0), (v * v).sum(0)
    return np.stack([s, q], 1).astype(f64), np.stack([np.abs(v).sum(0), q], 1).astype(f64)


def stats_from_sums(s, q, n, eps, nacc=0):
    """mean, istd of the biased variance max(q/n - mean^2, 0), and what float64 arithmetic on (s, q) leaves open:
    -> (mean, istd, mean_slack, istd_lo, istd_hi, var, dvar).  ``nacc``: float64 additions behind s and q (0: they are given).
    q/n - mean^2 cancels: six float64 roundings (s/n twice over in the square, the square, q/n, the difference; + 2) and the
    accumulation move it by at most dvar = (3 nacc + 6) 2^-53 q/n  (mean^2 <= q/n), which the interval [istd_lo, istd_hi] carries."""
    s, q = np.asarray(s, np.longdouble), np.asarray(q, np.longdouble)
    mu = s / n
    var = np.maximum(q / n - mu * mu, 0)
    dvar = (3 * nacc + 6) * U53 * (q / n)
    e = np.longdouble(eps)
    istd = 1 / np.sqrt(var + e)
    lo, hi = 1 / np.sqrt(var + dvar + e), 1 / np.sqrt(np.maximum(var - dvar, 0) + e)
    mslack = (nacc + 2) * U53 * np.sqrt(q / n)
    return tuple(np.asarray(a, f64) for a in (mu, istd, mslack, lo, hi, var, dvar))


def bn_finalize(sums, n, eps, momentum, rmean=None, rvar=None):
    """nn.BatchNorm2d's training step from the (C, 2) sums over n rows: (mean, istd, new running mean, new running var); the
    running variance is the unbiased one, which falls back to the biased one at n = 1.  ``momentum`` and ``eps`` as the f32 handed
    to the kernel.  The running values are None without buffers."""
    sums = _d(sums).reshape(-1, 2)
    mu, istd, _, _, _, var, _ = stats_from_sums(sums[:, 0], sums[:, 1], n, eps)
    if rmean is None:
        return mu, istd, None, None
    m = float(np.float32(momentum))
    unb = var * n / (n - 1) if n > 1 else var
    return mu, istd, (1 - m) * _d(rmean) + m * mu, (1 - m) * _d(rvar) + m * unb


def bn_finalize_tol(sums, n, eps, momentum, rmean=None, rvar=None):
    """Absolute tolerances for the four results of ``bn_finalize`` against an f32 result: one f32 rounding of the value plus
    what float64 leaves open (``stats_from_sums``): -> (mean, (istd_lo, istd_hi), running mean, running var) with the istd entry
    an interval already widened by the f32 rounding."""
    sums = _d(sums).reshape(-1, 2)
    mu, istd, mslack, lo, hi, var, dvar = stats_from_sums(sums[:, 0], sums[:, 1], n, eps)
    tm = U24 * np.abs(mu) + mslack
    ti = (lo * (1 - U24) - 4 * U53 * lo, hi * (1 + U24) + 4 * U53 * hi)
    if rmean is None:
        return tm, ti, None, None
    m = float(np.float32(momentum))
    k = n / (n - 1) if n > 1 else 1.0
    wm = (1 - m) * np.abs(_d(rmean)) + m * np.abs(mu)
    wv = (1 - m) * np.abs(_d(rvar)) + m * k * var
    return tm, ti, U24 * wm + 4 * U53 * wm + m * mslack, U24 * wv + 6 * U53 * wv + m * k * dvar


# ------------------------------------------------------------------------------------------------------------ SPADE
def _gamma_beta(gb, C, gamma_only=False):
    gb = np.asarray(gb)
    return _d(gb[:, :C]), (None if gamma_only else _d(gb[:, C:2 * C]))


def modulate_fwd(xn, gb, C, slope):
    """-> (y, magnitude, pre-activation t) for an already normalised xn.  f32 roundings: 1 + gamma, the fma, slope * t: 3."""
    a = _d(np.asarray(xn)[:, :C])
    g, b = _gamma_beta(gb, C)
    t = a * (1 + g) + b
    return lrelu(t, slope), np.abs(a) * (1 + np.abs(g)) + np.abs(b), t


def _modulate_bwd(u, a, g, t, slope):
    d = np.where(t > 0, u, slope * u)
    au = np.abs(u)
    return {"dxn": (d * (1 + g), au * (1 + np.abs(g))), "dgamma": (d * a, au * np.abs(a)), "dbeta": (d, au)}


def modulate_bwd(gy, xn, gb, C, slope):
    """-> {"dxn" | "dgamma" | "dbeta": (value, magnitude), "t": pre-activation, "tmag": its magnitude}.
    f32 roundings: dxn 3 (slope * gy, 1 + gamma, the product), dgamma 2, dbeta 1."""
    a = _d(np.asarray(xn)[:, :C])
    g, b = _gamma_beta(gb, C)
    t = a * (1 + g) + b
    out = _modulate_bwd(_d(np.asarray(gy)[:, :C]), a, g, t, slope)
    out["t"], out["tmag"] = t, np.abs(a) * (1 + np.abs(g)) + np.abs(b)
    return out


def xhat_of(x, C, mean, istd, up2=None):
    xs = up2_rows(x, up2, C) if up2 else np.asarray(x)[:, :C]
    return (_d(xs) - _d(mean)[None, :C]) * _d(istd)[None, :C]


def norm_modulate_fwd(x, gb, C, slope, mean, istd, up2=None):
    """-> (y, magnitude, t).  ``up2`` = (B, H, W) of the OUTPUT: x is the (B * H/2 * W/2, ld) map before the nearest x2 upsample.
    f32 roundings: x - mean, * istd, 1 + gamma, the fma, slope * t: 5."""
    a = xhat_of(x, C, mean, istd, up2)
    g, b = _gamma_beta(gb, C)
    t = a * (1 + g) + b
    return lrelu(t, slope), np.abs(a) * (1 + np.abs(g)) + np.abs(b), t


def norm_modulate_bwd(gy, x, gb, C, slope, mean, istd, up2=None, y=None):
    """The modulation's backward with the normalisation inline.  ``y`` (from_y): gb holds gamma alone and the activation's mask
    is the sign of the stored output y instead of the pre-activation's.  -> as ``modulate_bwd``, plus "sums": the (C, 4) column
    sums (sum dxn, sum dxn * xhat, sum dgamma, sum dbeta), "xhat", and "t" / "tmag" (None with ``y``).
    f32 roundings: dxn 3, dgamma 4 (slope * gy, x - mean, * istd, the product), dbeta 1."""
    a = xhat_of(x, C, mean, istd, up2)
    g, b = _gamma_beta(gb, C, gamma_only=y is not None)
    u = _d(np.asarray(gy)[:, :C])
    if y is not None:
        t, tmag, sign = None, None, _d(np.asarray(y)[:, :C])
    else:
        t = a * (1 + g) + b
        tmag, sign = np.abs(a) * (1 + np.abs(g)) + np.abs(b), t
    out = _modulate_bwd(u, a, g, sign, slope)
    dxn, dg, db = out["dxn"][0], out["dgamma"][0], out["dbeta"][0]
    out["sums"] = np.stack([dxn.sum(0), (dxn * a).sum(0), dg.sum(0), db.sum(0)], 1)
    out["t"], out["tmag"], out["xhat"] = t, tmag, a
    return out


def bn_bwd_apply(dxn, x, C, mean, istd, sums, n, up2=None):
    """BatchNorm's backward from its folded sums ((C, 2) float64 as handed to the kernel, or None in eval mode) over n rows:
    dx = istd * (dxn - S1/n - xhat * S2/n).  ``up2`` = (B, H, W) of dxn: x and the result live on the (H/2, W/2) grid, the four
    children of a source pixel are summed, S1 and S2 count four times.  -> (dx, magnitude).
    f32 roundings, train: S1/n, S2/n, x - mean, * istd, * S2/n, dxn - S1/n, the difference, * istd: 8 (+ 3 additions of the
    children with up2: 11); eval: * istd: 1 (+ 3 with up2: 4)."""
    d = _d(np.asarray(dxn)[:, :C])
    dabs = np.abs(d)
    rep = 1.0
    if up2:
        B, H, W = up2
        fold = lambda v: v.reshape(B, H // 2, 2, W // 2, 2, C).sum((2, 4)).reshape(-1, C)
        d, dabs, rep = fold(d), fold(dabs), 4.0
    a = xhat_of(x, C, mean, istd)
    i = _d(istd)[None, :C]
    if sums is None:
        return i * d, np.abs(i) * dabs
    s = _d(sums).reshape(-1, 2)
    m1, m2 = rep * s[None, :, 0] / n, rep * s[None, :, 1] / n
    return i * (d - m1 - a * m2), np.abs(i) * (dabs + np.abs(m1) + np.abs(a * m2))


# ------------------------------------------------------------------------------------------------------------ InstanceNorm
def _planes(x, channels_last):
    """(B, HW, C) pixel-major or (B, C, HW) planar -> (B, C, HW) float64"""
    x = _d(x)
    return x.transpose(0, 2, 1) if channels_last else x


def _unplanes(v, channels_last):
    return np.ascontiguousarray(v.transpose(0, 2, 1)) if channels_last else v


def instance_norm_record(x, eps, channels_last):
    """The (mean, istd) record of every (sample, channel) plane, (B, C, 2), with its tolerance against an f32 record:
    -> (record, mean tolerance (B, C), istd_lo, istd_hi).  One f32 rounding plus float64 accumulation over the HW pixels."""
    p = _planes(x, channels_last).astype(np.longdouble)
    hw = p.shape[2]
    mu, istd, mslack, lo, hi, _, _ = stats_from_sums(p.sum(2), (p * p).sum(2), hw, eps, nacc=hw)
    return np.stack([mu, istd], 2), U24 * np.abs(mu) + mslack, lo * (1 - U24) - 4 * U53 * lo, hi * (1 + U24) + 4 * U53 * hi


def instance_norm_act_fwd(x, eps, slope, channels_last, stats=None):
    """y = leaky_relu((x - mean) * istd, slope) per plane, in x's layout: -> (y, magnitude, record (B, C, 2)).  ``stats``: evaluate
    with this record (the f32 one a kernel wrote) instead of the oracle's own.  f32 roundings: x - mean, * istd, slope *: 3."""
    rec = instance_norm_record(x, eps, channels_last)[0] if stats is None else _d(stats)
    h = (_planes(x, channels_last) - rec[:, :, :1]) * rec[:, :, 1:]
    return _unplanes(lrelu(h, slope), channels_last), _unplanes(np.abs(h), channels_last), rec


def instance_norm_act_bwd(gy, x, stats, slope, channels_last):
    """g' = gy * leaky_relu'(xhat),  dx = istd * (g' - mean(g') - xhat * mean(g' xhat)) per plane: -> (dx, magnitude, record).
    The kernel forms the two means from its f32 g' and xhat, so their magnitudes are means of absolute values.  f32 roundings:
    g' 1; mean(g'): its g' 1 + its own 1; mean(g' xhat): g' 1, xhat 2, its own 1; xhat 2; xhat * mean 1; g' - mean 1; the
    difference 1; * istd 1: 13."""
    rec = _d(stats)
    h = (_planes(x, channels_last) - rec[:, :, :1]) * rec[:, :, 1:]
    g = _planes(gy, channels_last)
    gp = np.where(h > 0, g, slope * g)
    i = rec[:, :, 1:]
    dx = i * (gp - gp.mean(2, keepdims=True) - h * (gp * h).mean(2, keepdims=True))
    mag = np.abs(i) * (np.abs(gp) + np.abs(gp).mean(2, keepdims=True) + np.abs(h) * np.abs(gp * h).mean(2, keepdims=True))
    return _unplanes(dx, channels_last), _unplanes(mag, channels_last), rec


# ------------------------------------------------------------------------------------------------------------ bounds
K = {  # f32 roundings of each formula (counted in the docstrings above) + 2
    "modulate_fwd": 3 + 2, "modulate_bwd.dxn": 3 + 2, "modulate_bwd.dgamma": 2 + 2, "modulate_bwd.dbeta": 1 + 2,
    "norm_modulate_fwd": 5 + 2, "norm_modulate_bwd.dxn": 3 + 2, "norm_modulate_bwd.dgamma": 4 + 2, "norm_modulate_bwd.dbeta": 1 + 2,
    "bn_bwd_apply": 8 + 2, "bn_bwd_apply.eval": 1 + 2, "bn_bwd_apply_up2": 11 + 2, "bn_bwd_apply_up2.eval": 4 + 2,
    "instance_norm_fwd": 3 + 2, "instance_norm_bwd": 13 + 2,
}


def near_zero(t, tmag):
    """Elements whose float64 pre-activation lies within FLIP_WINDOW magnitudes of zero: the only ones a test may skip."""
    return np.abs(t) <= FLIP_WINDOW * tmag


# ------------------------------------------------------------------------------------------------------------ shapes
def col_map(C):
    """(cvp, rpp) of the reducing kernels: 4-channel groups rounded up to a power of two (<= 256), rows per pass of a block."""
    cvp = 1
    while cvp < C // 4 and cvp < 256:
        cvp <<= 1
    return cvp, 256 // cvp


CHANNELS = (4, 12, 36, 100, 1020, 1024, 1028)
ROW_KINDS = ("1", "3", "rpp-1", "rpp+1", "517")
LD_KINDS = ("C", "C+4", "2C+8")
GRID_KINDS = ("1", "stats_grid", "3x")
SLOPES = (0.0, 0.2, 1.0)
UP2_MAPS = ((1, 2, 2), (3, 2, 6), (2, 6, 4))


def rows_of(kind, C):
    rpp = col_map(C)[1]
    return {"1": 1, "3": 3, "rpp-1": max(1, rpp - 1), "rpp+1": rpp + 1, "517": 517}[kind]


def ld_of(kind, need):
    return {"C": need, "C+4": need + 4, "2C+8": 2 * need + 8}[kind]


def stats_grid(rows, C):
    rpp = col_map(C)[1]
    return max(1, min(512, (rows + rpp - 1) // rpp))


def grid_of(kind, rows, C):
    return {"1": 1, "stats_grid": stats_grid(rows, C), "3x": 3 * stats_grid(rows, C)}[kind]


# one case per (C, row kind); the other axes cycle so that every value of each appears with every C
FLAT_CASES = [(C, rk, LD_KINDS[(i + j) % 3], GRID_KINDS[(2 * i + j) % 3], SLOPES[(i + 2 * j) % 3])
              for i, C in enumerate(CHANNELS) for j, rk in enumerate(ROW_KINDS)]
UP2_CASES = [(C, bhw, GRID_KINDS[(i + j) % 3], SLOPES[(2 * i + j) % 3]) for i, C in enumerate(CHANNELS)
             for j, bhw in enumerate(UP2_MAPS)]
FOLD_CASES = [(R, nk) for i, R in enumerate((1, 2, 15, 16, 17, 512)) for nk in ("1", "15", "16", "17", "2C", "4C+1")]
IN_CASES = [(1, (1, 4, 1)), (1, (2, 4, 31)), (1, (2, 36, 33)), (1, (3, 64, 32)), (1, (1, 32, 100)),
            (0, (1, 1, 1)), (0, (2, 3, 63)), (0, (2, 5, 65)), (0, (1, 2, 257)), (0, (3, 7, 1000))]
IN_SLOPES = {i: SLOPES[i % 3] for i in range(len(IN_CASES))}


def flat_name(case):
    return "C%d-rows_%s-ld_%s-grid_%s-slope%g" % case


def up2_name(case):
    return "C%d-B%dH%dW%d-grid_%s-slope%g" % ((case[0],) + case[1] + case[2:])


def in_name(case):
    return "%s-B%d-C%d-HW%d" % (("nhwc" if case[0] else "nchw",) + case[1])


def case_seed(*parts):
    s = 17
    for p in parts:
        s = (s * 1000003 + hash_int(p)) % (2 ** 31 - 1)
    return s


def hash_int(p):
    if isinstance(p, (tuple, list)):
        return sum((k + 1) * hash_int(v) for k, v in enumerate(p))
    if isinstance(p, str):
        return sum((k + 1) * ord(ch) for k, ch in enumerate(p))
    return int(round(float(p) * 10))


def spade_inputs(rows, C, seed, rows_x=None):
    """f32 inputs of one SPADE case: x (rows_x or rows, C) with a per-channel offset and scale, gb (rows, 2C), gy (rows, C), and
    (mean, istd) of x as f32 -- the numbers a kernel would be handed, not re-derived by the oracle."""
    r = np.random.RandomState(seed)
    rx = rows if rows_x is None else rows_x
    x = (r.randn(rx, C) * (0.5 + r.rand(1, C)) + r.randn(1, C)).astype(np.float32)
    gb = (0.5 * r.randn(rows, 2 * C)).astype(np.float32)
    gy = r.randn(rows, C).astype(np.float32)
    xd = x.astype(f64)
    mean = xd.mean(0).astype(np.float32)
    istd = (1 / np.sqrt(xd.var(0) + 1e-5)).astype(np.float32)
    return x, gb, gy, mean, istd


def instance_inputs(case, seed, hard=None):
    """x and gy of an InstanceNorm case in its layout.  ``hard``: "const" makes plane (0, 0) constant, "offset" gives it mean 1e3
    and spread 1e-2."""
    cl, (B, C, HW) = case
    r = np.random.RandomState(seed)
    x = (r.randn(B, C, HW) * (0.5 + r.rand(B, C, 1)) + r.randn(B, C, 1)).astype(np.float32)
    gy = r.randn(B, C, HW).astype(np.float32)
    if hard == "const":
        x[0, 0] = np.float32(1.7)
    elif hard == "offset":
        x[0, 0] = (1e3 + 1e-2 * r.randn(HW)).astype(np.float32)
    if cl:
        x, gy = np.ascontiguousarray(x.transpose(0, 2, 1)), np.ascontiguousarray(gy.transpose(0, 2, 1))
    return x, gy
