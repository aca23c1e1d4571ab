"""SphereMaxPool2D restated in float64 from a tap table -- a helper of the sphere-pool tests, not a test.

The operator (reference ``spherenet/sphere_cnn.py:127-150``: ``max_pool2d(grid_sample(x, grid), 3, 3)``) seen through the
bilinear tap table ``(idx, wgt)`` of ``eml_sphere_tap_table_f32``: output cell p, tap t = a*3 + b, corner k samples input
pixel ``idx[p*9 + t, k]`` (-1: off the map, contributes 0) with weight ``wgt[p*9 + t, k]``.

* ``tap_table``      the table on the CPU from ``sphere_sampling_grid`` with grid_sample's float32 arithmetic (the four lines
                     of ``sphere_tap_table_kernel``, csrc/sphere_conv.hip)
* ``tap_values``     the nine tap values of every cell, float64
* ``pool``           the pooled value and the winning tap under max_pool2d's rule (first maximum; a NaN wins)
* ``routed_grad``    the input gradient FOR A GIVEN ROUTING (an index tensor), and S[q] = sum |w * gy| of the routed terms
* ``longest_row``    M, the longest row of the table's CSR transpose
* ``top_two_gap``    per cell, the gap between the largest and the second largest tap value
* ``fed_pixels``     the input pixels that a set of cells can send gradient to

Pure torch and numpy; every tensor lives on the CPU.
"""
import numpy as np
import torch

from emlight_amd.GenProjector.spherenet import sphere_sampling_grid

# the cases of tests/golden/sphere_pool.npz: (H, W, stride, B, C)
CASES = [(8, 16, 1, 2, 5), (8, 16, 2, 2, 8), (9, 18, 3, 1, 3), (6, 12, 1, 1, 1), (16, 32, 2, 2, 4), (5, 12, 2, 1, 7)]
U = 2.0 ** -24                      # float32 unit roundoff
NEAR_TIE_LO, NEAR_TIE_REL = 1e-12, 1e-5   # a near tie: top-two gap in (1e-12, 1e-5 * max|x|); at most 0.5 % of the cells
NEAR_TIE_CAP = 0.005


def case_name(case):
    return "h%dw%ds%db%dc%d" % case


def out_size(H, W, stride):
    return -(-H // stride), -(-W // stride)


def tap_table(H, W, stride, contracted=True):
    """(idx (P*9, 4) int64, wgt (P*9, 4) float32) with P = H' * W', rows ordered p*9 + a*3 + b.

    ATen's ``grid_sampler_unnormalize`` for ``align_corners=False`` is ``((coord + 1) * size - 1) / 2`` in float32.  Its
    product and difference are ONE fused multiply-add, one rounding (``contracted=True``), in the table kernel as compiled
    (``v_pk_fma_f32``) and, judged by its results, in grid_sample on the CPU: against the reference's CPU outputs in
    ``tests/golden/sphere_pool.npz`` this table leaves 0.02 to 0.09 of the forward bound and at most 0.07 of the gradient bound,
    while two roundings (``contracted=False``) leave 0.26 and 1.03 at 6x12 and 5x12.  The two differ in the last bit of a
    coordinate, only where ``size`` is not a power of two (75 weights at 9x18 stride 3, 249 at 6x12, none at 8x16 or 16x32)."""
    g = sphere_sampling_grid(H, W, stride)[0].numpy()                    # (3H', 3W', 2) float32: (x, y)
    ho, wo = g.shape[0] // 3, g.shape[1] // 3
    g = g.reshape(ho, 3, wo, 3, 2).transpose(0, 2, 1, 3, 4).reshape(ho * wo * 9, 2)
    f32 = np.float32

    def unnormalize(coord, size):
        s = coord + f32(1)                                               # float32
        if contracted:
            return ((s.astype(np.float64) * size - 1.0).astype(f32)) / f32(2)    # exact in float64, rounded once
        return (s * f32(size) - f32(1)) / f32(2)
    ix, iy = unnormalize(g[:, 0], W), unnormalize(g[:, 1], H)
    fx, fy = np.floor(ix), np.floor(iy)
    xe, ye = fx + f32(1), fy + f32(1)
    w4 = np.stack([(xe - ix) * (ye - iy), (ix - fx) * (ye - iy), (xe - ix) * (iy - fy), (ix - fx) * (iy - fy)], 1)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xs = np.stack([x0, x0 + 1, x0, x0 + 1], 1)
    ys = np.stack([y0, y0, y0 + 1, y0 + 1], 1)
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    idx = np.where(ok, ys * W + xs, -1)
    wgt = np.where(ok, w4, f32(0)).astype(f32)
    assert w4.dtype == f32
    return torch.from_numpy(idx), torch.from_numpy(wgt)


def tap_values(x, idx, wgt):
    """x (B, C, H, W) -> (B, C, P, 9) float64: v_t = sum_k wgt * x[idx], an index of -1 contributing 0."""
    B, C = x.shape[:2]
    xf = x.detach().double().reshape(B, C, -1)
    idx, wgt = idx.long(), wgt.double()
    v = torch.zeros(B, C, idx.shape[0], dtype=torch.float64)
    for k in range(4):
        ok = idx[:, k] >= 0
        term = xf[:, :, idx[:, k].clamp(min=0)] * wgt[:, k]
        v = v + torch.where(ok, term, torch.zeros_like(term))
    return v.view(B, C, -1, 9)


def pool(vals):
    """(B, C, P, 9) -> (y (B, C, P), arg (B, C, P) int64): tap t replaces the running maximum when v_t > max or v_t is NaN."""
    best, arg = vals[..., 0].clone(), torch.zeros(vals.shape[:-1], dtype=torch.int64)
    for t in range(1, 9):
        v = vals[..., t]
        m = (v > best) | torch.isnan(v)
        best, arg = torch.where(m, v, best), torch.where(m, torch.full_like(arg, t), arg)
    return best, arg


def routed_grad(gy, arg, idx, wgt, n_src):
    """gy, arg (B, C, P) -> (gx, S) (B, C, n_src) float64: gx[q] = sum of wgt * gy over the (cell, tap, corner) entries that sample
    q and whose tap is the cell's ``arg``; S[q] the same sum of absolute values."""
    B, C, P = gy.shape
    gy, idx, wgt, arg = gy.detach().double(), idx.long().view(P, 9, 4), wgt.double().view(P, 9, 4), arg.long()
    gx = torch.zeros(B, C, n_src, dtype=torch.float64)
    S = torch.zeros_like(gx)
    for t in range(9):
        g = torch.where(arg == t, gy, torch.zeros_like(gy))
        for k in range(4):
            ok = idx[:, t, k] >= 0
            term = g[:, :, ok] * wgt[ok, t, k]
            gx.index_add_(2, idx[ok, t, k], term)
            S.index_add_(2, idx[ok, t, k], term.abs())
    return gx, S


def longest_row(idx, n_src):
    flat = idx.long().reshape(-1)
    return int(torch.bincount(flat[flat >= 0], minlength=n_src).max())


def top_two_gap(vals):
    top = torch.topk(vals, 2, dim=-1).values
    return top[..., 0] - top[..., 1]


def near_tie_cells(vals, x_absmax):
    """(B, C, P) bool: the cells whose top-two gap lies in the near-tie window.  Exact ties (gap <= 1e-12: the pole rows, where
    tap 1 or 7 has the centre tap's footprint) are not in it: either routing gives the same gradient."""
    gap = top_two_gap(vals)
    return (gap > NEAR_TIE_LO) & (gap < NEAR_TIE_REL * x_absmax)


def fed_pixels(cells, idx, n_src):
    """cells (B, C, P) bool -> (B, C, n_src) bool: input pixels sampled by any tap of a marked cell."""
    B, C, P = cells.shape
    idx = idx.long().view(P, 36)
    fed = torch.zeros(B, C, n_src + 1, dtype=torch.float64)
    c = cells.double()
    for j in range(36):
        fed.index_add_(2, torch.where(idx[:, j] >= 0, idx[:, j], torch.full_like(idx[:, j], n_src)), c)
    return fed[:, :, :n_src] > 0


def forward_bound(x_absmax):
    """|y - want| <= 16 u max|x|: a tap value is at most 4 products and 3 additions of weights that sum to 1, 7 roundings on each
    side, rounded up."""
    return 16 * U * x_absmax


def grad_bound(M, S):
    """|gx[q] - want[q]| <= 2 M u S[q] + 1e-30 for a fixed routing: summation order and product rounding only."""
    return 2 * M * U * S + 1e-30
