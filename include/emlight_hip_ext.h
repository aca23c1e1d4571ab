/*
 * emlight_hip_ext.h -- entry points of libemlight_hip.so added after the 131 of emlight_hip.h.
 *
 * Same library, same conventions (emlight_hip.h: caller-owned contiguous device buffers, launchers only enqueue on
 * `stream`, 0 or a negative EML_E* code or a positive hipError_t, eml_last_error() for the message).  emlight_hip.h and
 * EML_ABI_VERSION stay as they are; the ctypes binding keeps these names in a second table (EXT_SIGNATURES) and refuses a
 * library that lacks one of them by name, as it does for the first.  The reference file:line each entry point stands in
 * for is cited on its declaration.
 */
#ifndef EMLIGHT_HIP_EXT_H
#define EMLIGHT_HIP_EXT_H

#include "emlight_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- panorama warp (data preparation)
 * GenProjector/util.py:279-343 (`resize_exr`; copy: GenProjector/tools/util.py), the operator behind the
 * `warpedHDROutputs` files of GenProjector/data.py:73, with the three constants of util.py:281 as arguments.
 * pano (B,H,W,3) f32 -> out (B,h,w,3) f32 pixel-major (what eml_pano_resize_area_f32 writes and eml_gt_parametrise_f64 /
 * eml_projector_targets_f32 read).  For output pixel (i, j), all in f64:
 *   lat = i pi / h - pi / 2,  lon = j 2 pi / w  (no half-pixel offset),  d = (sin lat, sin lon cos lat, -cos lon cos lat)
 *   Rt = rotation about x by theta;  Rp = Rodrigues' rotation about (0, cos theta, sin theta), cosine cos(phi), sine -sin(phi)
 *   v = Rp Rt d + move * Rp Rt (0,0,-1),  s = v / |v|
 *   row = (asin(s0) + pi/2) / pi * H,  col = (atan2(s1, -s2) mod 2 pi) / (2 pi) * W
 * theta, phi in degrees, move in sphere radii.  A position closer than 2^-28 px to an integer is that integer (the
 * identity warp then returns the source bit for bit).  Sampling is bilinear with wrap-around on BOTH axes (BORDER_WRAP):
 * taps floor mod size and their +1 neighbours mod size, f64 fractions as weights, the four products summed in f64 in the
 * order 00, 01, 10, 11 and rounded to f32 once; row == H and col == W occur and land on index 0.  cv2's quantisation of
 * the weights to 1/32 px is not reproduced.
 * params_dev: (B,3) f64 device array of (theta, phi, move), one per sample, or NULL: then the three by-value arguments
 * hold for the batch, must be finite (EML_EINVAL otherwise), and every thread evaluates its position once for a run of
 * images.  With params_dev, a pixel whose position is not finite (|v| == 0, possible only at |move| == 1; a NaN or
 * infinite parameter) is written as NaN and loads nothing; tap indices are formed after that check and reduced modulo
 * the size, so no parameter value reads outside the image.
 * coords: NULL, or (n_sets,h,w,2) f64 receiving (row, col); n_sets = B with params_dev, else 1.  The image is the same
 * bits with and without it.  No atomics: run-to-run exact, and an image gives the same bits in any batch.
 * Limits: 0 <= B <= 65535 (grid.y); H, W, h, w >= 1; H * W and h * w <= 2^29 (pixel indices are 32-bit). */
int eml_pano_warp_f32(const float* pano, int B, int H, int W, int h, int w, double theta_deg, double phi_deg, double move,
                      const double* params_dev, float* out, double* coords, eml_stream_t stream);

/* GenProjector/util.py:279-343, the gradients of eml_pano_warp_f32 (the reference has none).  Per output
 * pixel p = (i, j) of sample b the forward has a source position (row, col) in f64, snapped to an integer when closer than
 * 2^-28 px; taps i0 = floor(row) mod H, i1 = i0 + 1 mod H, j0, j1 likewise; fractions yd, xd; and
 *   out = w00 I00 + w01 I01 + w10 I10 + w11 I11,  w00 = (1-yd)(1-xd), w01 = (1-yd) xd, w10 = yd (1-xd), w11 = yd xd.
 * A pixel whose position is not finite (NaN in the forward) contributes nothing to either gradient.
 * grad_out (B,h,w,3) f32 = g.
 * dpano (B,H,W,3) f32 or NULL, every element written:
 *   dpano[b,t,ch] = sum over (p, k) whose tap k lands on texel t of w_k(b,p) g[b,p,ch]
 * with the forward's own f64 weights, made from the snapped position.  Each product is formed in f64, rounded once to a
 * multiple of u_b = 2^(e_b - 61), where 2^e_b is the power of two above S_b = sum |g[b]| (taken in f64 in a fixed order by a
 * first pass), and added in 64-bit integers; the integer sum is exact and order-independent, and is rounded to f32 once.
 * |error before that rounding| <= n 2^-61 S_b for a texel that n taps land on.  Two taps of one pixel that name the same
 * texel (H == 1 or W == 1) both add; a texel that nothing lands on is exactly 0.
 * dparams (B,3) f64 or NULL, order theta_deg, phi_deg, move, one row per sample also with by-value parameters:
 *   dparams[b,q] = sum_p sum_ch g[b,p,ch] (dOut/dRow dRow/dq + dOut/dCol dCol/dq)
 *   dOut/dRow = (1-xd)(I10-I00) + xd (I11-I01),  dOut/dCol = (1-yd)(I01-I00) + yd (I11-I10)
 * in the cell the forward used (at an integer position the right-hand cell, grid_sample's convention), in f64 from the f32
 * texels.  dRow/dq, dCol/dq: the derivative of the unsnapped position formula (degree-to-radian factor, both rotations,
 * move * m, the normalisation, asin, atan2; the clamp of s0, the `mod 2 pi` and the snap are the identity), forward mode in
 * f64.  Pole rule: a pixel with s1^2 + s2^2 < 2^-20 (1 - s0^2 formed as that sum) contributes 0 to dparams; its
 * contribution to dpano is unaffected.  The sum over pixels is a fixed-order f64 reduction: a tree inside each 256-pixel
 * tile, the tiles' partials into `work`, then one fixed-order pass per sample.
 * Run-to-run exact; a sample's gradients have the same bits in any batch and with by-value and per-sample parameters.  Only
 * enqueues: no host synchronisation, no host work that depends on the parameters.  Non-finite values in grad_out leave that
 * sample's gradients unspecified; tap indices never depend on grad_out and are reduced modulo the size.
 * pano may be NULL when dparams is NULL.  work: eml_pano_warp_bwd_work_floats(...) floats (0 when a size is refused, B == 0
 * or nothing is wanted), 8-byte aligned.  Limits as eml_pano_warp_f32.  EML_EINVAL with nothing enqueued: a NULL grad_out;
 * both outputs NULL; dparams without pano; bad sizes; non-finite by-value parameters (params_dev == NULL); a NULL or
 * misaligned work with B > 0.  B == 0 returns 0. */
size_t eml_pano_warp_bwd_work_floats(int B, int H, int W, int h, int w, int want_dpano, int want_dparams);
int eml_pano_warp_bwd_f32(const float* grad_out, const float* pano, int B, int H, int W, int h, int w, double theta_deg,
                          double phi_deg, double move, const double* params_dev, float* dpano, double* dparams, float* work,
                          eml_stream_t stream);

/* ---------------------------------------------------------------- render loss: the adjoint of the sphere renders
 * The reference tree has no such code; DESIGN.md section 15 is the definition (as for eml_sphere_render_f32, whose
 * geometry, materials mask, material order and limits these share).  eml_sphere_render_f32 is linear in the panorama:
 * two integrals K . pano and one bilinear lookup.  Its gradient with respect to the panorama is the adjoint:
 *   dpano[b,ch,t] = sum_p Kd[p,t] g_d[b,ch,p] + sum_p Kg[p,t] g_g[b,ch,p] + sum over mirror taps (p,k) on t of w[p,k] g_m[b,ch,p]
 * with Kd, Kg the weights of the two integrals, normalisations 1/pi and (m+1)/2pi included, p over the INSIDE pixels only
 * (values of grad_out outside the disc are never read).
 * grad_out (B,M,3,S,S) f32 in the kernel's material order (diffuse, glossy, mirror; M = bits set in materials_mask) ->
 * dpano (B,3,H,W) f32, every element written.  K is never stored; no atomics: run-to-run exact; the summation is not split,
 * pixels are added in list order, so an image's gradient has the same bits in any batch.
 * With EML_SPHERE_MIRROR: the taps of eml_sphere_mirror_taps_f32 sorted by texel (stable) as a CSR over the H W texels:
 * mirror_csr_ptr (H W + 1) int32, mirror_csr_src (4P) int32 = the pixel's linear index i S + j in the S x S image,
 * mirror_csr_w (4P) f32; a texel's entries are added in CSR order after the integrals.  Entries outside [0, 4P) or
 * [0, S S) are skipped.  Without that bit the three pointers are not read (NULL is fine).
 * work: eml_sphere_render_bwd_work_floats(B, H, W, S) floats (0 when a size is refused or B == 0), 16-byte aligned. */
size_t eml_sphere_render_bwd_work_floats(int B, int H, int W, int S);
int eml_sphere_render_bwd_f32(const float* grad_out, int B, int H, int W, int S, double view_azimuth_deg, int materials_mask,
                              double phong_m, const int* mirror_csr_ptr, const int* mirror_csr_src, const float* mirror_csr_w,
                              float* dpano, float* work, eml_stream_t stream);

/* The mirror's four taps per inside pixel (pixels in row-major order, P of them): idx (P,4) int32
 * texel indices r W + c, wgt (P,4) f32.  Coordinates in f64 exactly as eml_sphere_render_f32 forms them (rows clamp,
 * columns wrap); wx, wy rounded to f32, then (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy in f32 for the taps (r0,c0), (r0,c1),
 * (r1,c0), (r1,c1).  Two taps of a pixel may name the same texel (a clamped row): they add. */
int eml_sphere_mirror_taps_f32(int H, int W, int S, double view_azimuth_deg, int* idx, float* wgt, eml_stream_t stream);

/* ---------------------------------------------------------------- GMLight loss: one scene geometry per sample
 * gmloss/utils.py:63-108 (`geometric_points` and `distance`, built once per sample instead of one geometry repeated
 * `batchsize` times, utils.py:89-93).  depth (B,N): the per-anchor depths, f32 or f64 (depth_is_f64 != 0), device ->
 *   anchors_out (B,N,3) f32 or NULL: (r cos theta, r sin theta, z) with theta = pi (3 - sqrt 5) k and
 *     z = linspace(1 - 1/N, 1/N - 1, N), evaluated in f64 as numpy does (an f32 depth is promoted exactly) and rounded to f32 once;
 *   M_out (B,N,N) f32: M_ij = sqrtf(dx^2 + dy^2 + dz^2) of the f32 anchors, eml_emd_anchor_cost_f32's arithmetic; the
 *     diagonal is exactly 0 and M is symmetric bit for bit.
 * One launch for the batch, no host work per sample, no atomics.  Limits: 1 <= N <= 2048, B >= 0 (B == 0 returns 0);
 * a NULL depth or M_out is EML_EINVAL before anything is enqueued. */
int eml_gm_anchor_cost_f32(const void* depth, int depth_is_f64, int B, int N, float* anchors_out, float* M_out,
                           eml_stream_t stream);

/* gmloss/samples_loss.py:69-84 (`sinkhorn_tensorized` with a `distance` per call) on a batch whose samples each have
 * their own ground cost: eml_sinkhorn_fwd_dim_f32, every argument and output as there, plus
 *   cost_stride   floats between the samples' matrices: sample b reads M + b * cost_stride and Mt + b * cost_stride
 *                 ((B,N,N) contiguous: N*N).  0: one (N,N) matrix for the batch -- the outputs of eml_sinkhorn_fwd_dim_f32
 *                 bit for bit.
 * EML_EINVAL, with nothing enqueued: cost_stride < 0; 0 < cost_stride < N*N; cost_stride % 4 != 0 when N % 4 == 0 (those
 * kernels load M as 16-byte vectors, so M itself must be 16-byte aligned as well).  The split kernel, its status word
 * and its rescue launch, rho, D > 1 and the weight gradients work as with one matrix. */
int eml_sinkhorn_fwd_cost_f32(const float* x, const float* y, const float* M, const float* Mt,
                              const float* alpha, const float* beta, double blur, double scaling, int p,
                              double diameter, const float* range_lo_hi, float* eps_out, int* n_eps_out,
                              float* diameter_out, float* loss, float* gx, float* gy, float* work, int B, int N,
                              int D, int flags, double rho, float* lam_out, long cost_stride, eml_stream_t stream);

/* ---------------------------------------------------------------- SphereMaxPool2D
 * spherenet/sphere_cnn.py:127-150 (`SphereMaxPool2D.forward`: grid_sample, then max_pool2d(3, 3)) in one pass over the tap
 * table of eml_sphere_tap_table_f32.  x (B*n_src, C) f32 pixel-major -> y (B*n_dst, C) f32:
 *   v_t = sum_k wgt[p*9 + t][k] * x[b][idx[p*9 + t][k]][c]   (corners in grid_sampler_2d's order; an index < 0 adds +0)
 *   y[b][p][c] = max_t v_t,   arg[b][p][c] = the winning tap t = a*3 + b (row-major in the 3x3 window)
 * max_pool2d's rule: tap t replaces the running maximum when v_t > max or v_t is NaN.  So the first maximal tap wins, a NaN
 * wins over every number and propagates, and of several NaN taps the last is recorded.
 * arg: (B*n_dst, C) uint8, or NULL when nobody needs the indices.  An index >= n_src is treated like one < 0.
 * Limits: B >= 0 (B == 0 returns 0 without a launch); C, n_src, n_dst >= 1; B * n_src, B * n_dst, 9 * n_dst < 2^31 (rows
 * are 32-bit, element offsets 64-bit); x and y 16-byte aligned when C % 4 == 0.  EML_EINVAL otherwise, nothing enqueued. */
int eml_sphere_max_pool_fwd_f32(const float* x, const int* idx, const float* wgt, float* y, unsigned char* arg, int B,
                                int n_src, int n_dst, int C, eml_stream_t stream);

/* spherenet/sphere_cnn.py:127-150, the gradient of the above with respect to x (autograd's max_pool2d backward followed by
 * grid_sampler's backward), as a gather over the CSR transpose of the tap table (csr_ptr (n_src + 1), csr_src, csr_w: entry
 * e of row q has output pixel csr_src[e] / 9, tap csr_src[e] % 9 and bilinear weight csr_w[e]):
 *   gx[b][q][c] = sum over e in row q with arg[b][csr_src[e] / 9][c] == csr_src[e] % 9 of csr_w[e] * gy[b][csr_src[e] / 9][c]
 * summed in CSR order with one fmaf per term; terms of taps that lost are skipped, not multiplied by 0.  No atomics: run-to-run
 * exact.  Every element of gx (B*n_src, C) is written; a pixel with an empty row gets 0.  Entries with csr_src / 9 >= n_dst
 * are skipped.  Limits and alignment as for the forward; gy, gx 16-byte and arg 4-byte aligned when C % 4 == 0. */
int eml_sphere_max_pool_bwd_f32(const float* gy, const unsigned char* arg, const int* csr_ptr, const int* csr_src,
                                const float* csr_w, float* gx, int B, int n_src, int n_dst, int C, eml_stream_t stream);

/* ---------------------------------------------------------------- SphereConv, 3-channel input layers: the bias gradient alone
 * spherenet/sphere_cnn.py:111-124 with the ReLU of normalization.py:92-96 folded in: the bias gradient of a 3 -> 64 / 3 -> 128
 * layer whose weight takes no gradient (eml_sphere_conv_small_wgrad_f32, emlight_hip.h, gives it together with dW2):
 *   db[o] = sum_m g'[m][o],   g' = dY * (Yact > 0 ? 1 : act_slope),   m < B * Po
 * one read of (dY, Yact) instead of an activation-backward pass and a column sum.  The result equals the db of
 * eml_sphere_conv_small_wgrad_f32 on the same (dY, Yact) BIT FOR BIT: the same MFMA sequence on the ones column alone, the
 * same grid, the same fixed-order sums (no atomics: run-to-run exact).
 * dY, Yact (B*Po, O) 16-byte aligned; Yact = the forward's output, NULL with act_slope = 1; act_slope in [0, 1]; (C, O) in
 * {(3, 64), (3, 128)}; partial: eml_sphere_conv_small_wgrad_partial_floats(B, Po, C, O) floats of scratch suffice (one per
 * workgroup and channel is used).  B == 0 zeroes db.  EML_EINVAL otherwise, nothing enqueued. */
int eml_sphere_conv_small_dbias_f32(const float* dY, const float* Yact, float act_slope, float* partial, float* db, int B,
                                    int Po, int C, int O, eml_stream_t stream);

/* ---------------------------------------------------------------- object insertion: prefiltered environment maps
 * The reference tree has no such code (its README describes the use: a virtual object lit by the predicted panorama);
 * DESIGN.md section 22 is the definition, and the lobes are section 15's two materials (eml_sphere_render_f32) evaluated at
 * the texel directions of an output grid instead of at a sphere's normals.  pano (B,3,H,W) f32, W == 2H ->
 * out (B,L,3,Ho,2Ho) f32, every element written:
 *   out[b,l,ch,d] = c_l sum_t pano[b,ch,t] k_l(omega_d . omega_t) dOmega_t
 * with omega, dOmega of the equirectangular grids of heights Ho (d) and H (t) as in section 15.  lobes: HOST array of L
 * doubles, read before the call returns: a value < 0 is the diffuse lobe (k = max(0, x), c = 1/pi), a value m >= 0 the Phong
 * lobe (k = max(0, x)^m, c = (m + 1) / 2 pi, 0^0 = 1).  An implicit GEMM on v_mfma_f32_32x32x2_f32 (rows: the 2 Ho^2
 * directions, k: the texels, columns: the 3B planes); the weights are never stored; two lobes share one read of the
 * panorama operand, L > 2 takes ceil(L / 2) passes.  No atomics: run-to-run exact.  The split over k is a function of (H, Ho)
 * alone and is added in split order, so an image's maps have the same bits in any batch; a lobe's arithmetic does not
 * depend on the lobe it shares a pass with, so its map has the same bits whatever else was asked for and in any position.
 * work: eml_env_prefilter_work_floats(B, H, W, Ho, L) floats (0 when a size is refused or B == 0), 16-byte aligned.
 * Limits: 0 <= B <= 4096 (B == 0 returns 0), 1 <= H <= 4096, W == 2H, 1 <= Ho <= 1024, 1 <= L <= 8, m <= 1e6 and not NaN.
 * EML_EINVAL otherwise, and for a NULL pointer, with nothing enqueued. */
size_t eml_env_prefilter_work_floats(int B, int H, int W, int Ho, int L);
int eml_env_prefilter_f32(const float* pano, int B, int H, int W, int Ho, int L, const double* lobes, float* out, float* work,
                          eml_stream_t stream);

/* ---------------------------------------------------------------- object insertion: G-buffer shading and composite
 * DESIGN.md section 22; the camera is RegressionNetwork/util.py:157-174 (`crop_panorama`'s ray of pixel (i, j), ratio = w / h)
 * written in the panorama's frame of section 15.  One thread per pixel of a (B, ., h, w) G-buffer, all geometry in f64:
 *   (c, s) = (cos, sin) of view_azimuth_deg;  f = (c, s, 0), r = (-s, c, 0), u = (0, 0, 1), v = -f
 *   fov_deg > 0: scl = tan(fov / 2), sx = scl (2j / (w-1) - 1), sy = (scl h / w)(2i / (h-1) - 1),
 *                v_p = -normalize(f + sx r - sy u);   fov_deg == 0 (orthographic): v_p = v
 *   n = normalize(nx r + ny u + nz v) from normal (B,3,h,w),  R = 2 (n . v_p) n - v_p  (no special case for back faces)
 *   shaded = kd * lookup(e_diffuse, n) + ks * lookup(e_phong, R) + km * lookup(pano, R)   products and sums in f32, in this order
 * lookup(map of height G, dir): theta = atan2(sqrt(x^2 + y^2), z), phi = atan2(y, x) mod 2 pi (x, y = -0 count as +0: the
 * poles themselves have phi = 0); continuous coordinates
 * theta G / pi - 1/2 clamped to [0, G - 1] and phi 2G / 2 pi - 1/2 with wrapping columns, in f64; fractions rounded to f32;
 * blend in f32, horizontal then vertical, a weight of 0 returns the tap (the mirror of eml_sphere_render_f32).
 * kd, ks, km (B,3,h,w) or NULL: a term whose coefficient is NULL is not evaluated and its map is not read.  Where
 * coverage (B,1,h,w) == 0 or the normal has length 0, shaded = 0 and neither the normal (at coverage 0) nor the coefficients
 * are read.  Maps: pano (B,3,H,2H); e_diffuse (.,3,Hd,2Hd) and e_phong (.,3,Hg,2Hg) with d_stride / g_stride floats between
 * the images' maps (a slice of eml_env_prefilter_f32's output: L 3 Hd 2Hd).
 * Composite (epilogue, optional): background (B,3,h,w), exposure (B,) on the device, gamma > 0:
 *   ldr = clamp(exposure[b] * shaded, 0, 1)^(1 / gamma)  (gamma == 1: no power),  composite = coverage ldr + (1 - coverage) background
 * shaded and composite may each be NULL, not both.  kd, ks and km all NULL is the composite alone: shaded is then READ, not
 * written, normal is not read (NULL is fine) and composite is required.
 * Limits: 0 <= B <= 65535 (grid.y; B == 0 returns 0), 2 <= h, w and h w <= 2^29, 0 <= fov_deg < 180, map heights 1..4096.
 * EML_EINVAL, with nothing enqueued: a NULL normal or coverage; kd, ks and km all NULL without shaded and composite; kd without e_diffuse, ks without
 * e_phong, km without pano; a stride below 3 G 2G; composite without background or exposure, either of those without
 * composite; gamma not > 0 with composite; non-finite angles; limits. */
int eml_gbuffer_shade_f32(const float* pano, int H, const float* e_diffuse, int Hd, long d_stride, const float* e_phong, int Hg,
                          long g_stride, const float* normal, const float* coverage, const float* kd, const float* ks,
                          const float* km, int B, int h, int w, double fov_deg, double view_azimuth_deg, float* shaded,
                          const float* background, const float* exposure, double gamma, float* composite,
                          eml_stream_t stream);

/* ---------------------------------------------------------------- object insertion: the adjoint of the prefilter
 * DESIGN.md section 23 (the reference tree has no such code).  eml_env_prefilter_f32 is linear in the panorama; its gradient
 * with respect to the panorama is the adjoint.  grad_out (B,L,3,Ho,2Ho) f32 -> dpano (B,3,H,W) f32, every element written:
 *   dpano[b,ch,t] = dOmega_t sum_l c_l sum_d k_l(omega_d . omega_t) grad_out[b,l,ch,d]
 * Grids, lobes (the same HOST array of L doubles, read before the call returns), c_l, 0^0 = 1 and the limits are those of
 * eml_env_prefilter_f32, and so are the weights: the same f32 grid tables, the same dot product, the same x^m.  The same
 * implicit GEMM on v_mfma_f32_32x32x2_f32, exchanged: rows are the 2 H^2 texels, k the (lobe, direction) pairs, columns the
 * 3B planes.  All L lobes add into the same accumulators: one pass over grad_out serves any L.  c_l is applied to the staged
 * grad_out, dOmega_t once per texel at the end.  No atomics: run-to-run exact.  The split over k is a function of (H, Ho)
 * alone and is added in split order, so an image's gradient has the same bits in any batch.
 * work: eml_env_prefilter_bwd_work_floats(B, H, W, Ho, L) floats (0 when a size is refused or B == 0), 16-byte aligned.
 * EML_EINVAL on the conditions of eml_env_prefilter_f32 and for a NULL grad_out or dpano, with nothing enqueued; B == 0
 * returns 0. */
size_t eml_env_prefilter_bwd_work_floats(int B, int H, int W, int Ho, int L);
int eml_env_prefilter_bwd_f32(const float* grad_out, int B, int H, int W, int Ho, int L, const double* lobes, float* dpano,
                              float* work, eml_stream_t stream);

/* ---------------------------------------------------------------- object insertion: the adjoint of shading and composite
 * DESIGN.md section 23.  The inputs of eml_gbuffer_shade_f32 (maps with their strides, normal, coverage, kd / ks / km or
 * NULL, the camera) and grad_out (B,3,h,w) f32.  Per pixel the frame, the taps, the fractions and the looked-up values are
 * the forward's, bit for bit.  exposure == NULL: grad_out is the gradient of `shaded`, g_s = grad_out.  exposure (B,) given
 * (with gamma): grad_out is the gradient of `composite`; the kernel recomputes s = shaded with the forward's f32 sequence,
 * x = fl(exposure[b] s), and
 *   g_s = grad_out coverage (1 / gamma) exposure[b] x^(1 / gamma - 1)   where 0 < x < 1,   g_s = 0 elsewhere
 * (both clamps and the two boundaries give 0: the gradient is always finite; gamma == 1: grad_out coverage exposure[b]).
 * The power is taken in f64 and g_s rounded to f32 once.  background takes no part.  Outputs, each may be NULL:
 *   dkd, dks, dkm (B,3,h,w): g_s * lookup(e_diffuse, n), g_s * lookup(e_phong, R), g_s * lookup(pano, R), products in f32
 *   d_e_diffuse (B,3,Hd,2Hd), d_e_phong (B,3,Hg,2Hg), dpano (B,3,H,2H; the mirror term only), contiguous, every element written:
 *     dmap[b,ch,t] = sum over the taps (p, q) on texel t of w_q(p) k[b,ch,p] g_s[b,ch,p]
 *     with (1-wx)(1-wy), wx (1-wy), (1-wx) wy, wx wy formed in f64 from the forward's f32 fractions
 *   dshaded (B,3,h,w): g_s itself, in the composite-only mode (kd, ks, km all NULL), which READS shaded (B,3,h,w)
 * A pixel with coverage 0 or a zero or non-finite normal gives exactly 0 everywhere and adds nothing; nothing of it but its
 * coverage (and, at coverage != 0, its normal) is read.  Two taps of a pixel on one texel (a clamped row) both add; a texel
 * nothing lands on is exactly 0.  The scatter is section 20's: per sample and map S = sum |k g_s| in f64 in a fixed order,
 * the unit u = 2^(e - 61) with 2^e the power of two above S; each contribution is formed in f64, rounded once to a multiple
 * of u and added with 64-bit integer atomics; one int64 -> f32 conversion.  |error before that rounding| <= n 2^-61 S for a
 * texel n taps land on.  The bits do not depend on the arrival order, the batch, or the set of outputs asked for.
 * Non-finite values in grad_out leave that sample's gradients unspecified; tap indices never depend on grad_out.  Only
 * enqueues.  work: eml_gbuffer_shade_bwd_work_floats(...) floats (0 when a size is refused, B == 0 or no map gradient is
 * wanted), 8-byte aligned; not read (NULL is fine) when no map gradient is wanted.  Limits as eml_gbuffer_shade_f32.
 * EML_EINVAL, with nothing enqueued: a NULL grad_out, coverage or (with a coefficient) normal; no output; a gradient of a
 * term whose coefficient is NULL; a coefficient without its map; shaded or dshaded with a coefficient, or the composite-only
 * mode without shaded, exposure and dshaded; gamma not > 0 with exposure; non-finite angles; limits; a NULL or misaligned
 * work when a map gradient is wanted and B > 0.  B == 0 returns 0. */
size_t eml_gbuffer_shade_bwd_work_floats(int B, int H, int Hd, int Hg, int h, int w, int want_dpano, int want_d_e_diffuse,
                                         int want_d_e_phong);
int eml_gbuffer_shade_bwd_f32(const float* grad_out, const float* pano, int H, const float* e_diffuse, int Hd, long d_stride,
                              const float* e_phong, int Hg, long g_stride, const float* normal, const float* coverage,
                              const float* kd, const float* ks, const float* km, int B, int h, int w, double fov_deg,
                              double view_azimuth_deg, const float* shaded, const float* exposure, double gamma, float* dkd,
                              float* dks, float* dkm, float* d_e_diffuse, float* d_e_phong, float* dpano, float* dshaded,
                              float* work, eml_stream_t stream);

/* ---------------------------------------------------------------- depth panoramas: the parallax-correct warp
 * GenProjector/util.py:279-343 gives the frame (`resize_exr`: the two rotations and the step along the rotated -z axis, as
 * eml_pano_warp_f32 forms them, from the same code); gmloss/utils.py:63-73 (`geometric_points`) says what depth means: the
 * distance from the viewpoint to the scene along a direction, the factor that scales a unit anchor.  The reference puts the
 * whole scene on the unit sphere; here it stands where its depth panorama says, and `move` is in the units of `depth`.
 * pano (B,H,W,3) f32 or NULL, depth (B,H,W) f32 -> out_pano (B,h,w,3) f32 or NULL, out_depth (B,h,w) f32 or NULL,
 * hit (B,h,w,3) f64 = (t, row, col) or NULL.  For output pixel (i, j), all in f64 without contraction:
 *   e = Rp Rt d(i, j),  m = Rp Rt (0,0,-1)  (eml_pano_warp_f32's two terms),  c = move * m,  P(t) = c + t e
 *   position(P): s = P / |P|, row = (asin(clamp(s0)) + pi/2) / pi * H, col = (atan2(s1, -s2) mod 2 pi) / (2 pi) * W, with the
 *     2^-28 px snap of eml_pano_warp_f32
 *   D(P): bilinear sample of depth at position(P), f64 weights, products summed in the order 00, 01, 10, 11; columns wrap,
 *     rows CLAMP: i0 = min(floor(row), H-1), i1 = min(i0+1, H-1) (eml_pano_warp_f32 blends the last row with row 0, the
 *     opposite pole; for a distance that would mix ceiling and floor)
 *   g(t) = |P(t)| - D(P(t)); a point with |P| == 0 counts as inside (g < 0)
 * Pre-pass per sample (fixed-order reduction into `work`): dmin, dmax, and a flag for a pixel that is not finite or not > 0.
 * A sample is INVALID when the flag is set, when one of its parameters is not finite, or when the viewpoint is on or outside
 * the surface (|c| > 0 and |c| >= D(c)): every pixel of its outputs and of its hit entries is NaN; nothing else is touched.
 * Bracket t_lo = max(0, dmin - |c|), t_hi = dmax + |c|; march t_k = t_lo + (t_hi - t_lo) k / steps, k = 1..steps, t_steps =
 * t_hi exactly; the first k with g(t_k) >= 0 (k = steps when none) gives a = t_(k-1), b = t_k: the nearest surface.  Then
 * `bisections` rounds mid = (a + b) / 2, g(mid) >= 0 ? b = mid : a = mid;  t = (a + b) / 2.  Fixed trip counts.
 * out_depth = (float)t; (row, col) = position(P(t)); out_pano = the clamped-row bilinear sample of pano there, summed in f64
 * and rounded once; a pixel whose P(t) has no position is NaN.  The depth map is treated as one connected surface: what the
 * source viewpoint never saw is not filled.
 * params_dev (B,3) f64 of (theta_deg, phi_deg, move) per sample, or NULL: the by-value three hold for the batch and must be
 * finite.  No atomics; an image gives the same bits in any batch and with either kind of parameters.  One thread per
 * output pixel, the depth gathered through the caches (a kernel that kept the map in LDS was slower: DESIGN.md section 26).
 * work: eml_pano_warp_depth_work_floats(B, H, W) floats (0 when a size is refused).
 * Limits: sizes as eml_pano_warp_f32; 1 <= steps <= 1024; 0 <= bisections <= 60.  EML_EINVAL, nothing enqueued: NULL depth
 * or work; both outputs NULL; out_pano without pano; bad sizes; non-finite by-value parameters; steps or bisections out of
 * range.  B == 0 returns 0. */
size_t eml_pano_warp_depth_work_floats(int B, int H, int W);
int eml_pano_warp_depth_f32(const float* pano, const float* depth, int B, int H, int W, int h, int w, double theta_deg,
                            double phi_deg, double move, const double* params_dev, int steps, int bisections, float* out_pano,
                            float* out_depth, double* hit, float* work, eml_stream_t stream);

/* RegressionNetwork/data.py:75 reads a per-anchor `depth` from the training pickles and gmloss/utils.py:63-73 scales the unit
 * anchors by it; nothing in the reference makes it.  Here: the steradian-weighted mean of a depth panorama over each anchor's
 * Voronoi cell, with the CSR tables that eml_gt_parametrise_f64 takes (csr_ptr (N+1), csr_pix (H W)) and its pixel weight:
 *   out[b,a] = sum_p w_p D[b,p] / sum_p w_p,   w_p = sin((row_p + 0.5) / H * pi),   p over the cell of anchor a
 * depth (B,H,W) f32 -> out (B,N) f64.  A pixel that is not finite has weight 0; a cell whose weights sum to 0 gives NaN.  f64,
 * one block per (anchor, image), fixed-order tree reduction: run-to-run exact.  0 <= B <= 65535 (B == 0 returns 0); EML_EINVAL
 * for a NULL pointer or a size < 1, nothing enqueued. */
int eml_gt_anchor_depth_f64(const float* depth, const int* csr_ptr, const int* csr_pix, int B, int H, int W, int N, double* out,
                            eml_stream_t stream);

/* ---------------------------------------------------------------- object insertion: the shadow on a ground plane
 * The reference tree has no such code; DESIGN.md section 28 is the definition (differential rendering with a diffuse shadow
 * catcher), the camera is eml_gbuffer_shade_f32's (RegressionNetwork/util.py:157-174), the grid section 15's.
 * pano (B,3,H,W) f32, W == 2H; plane: (nx, ny, nz, d) f32 on the device in CAMERA space (x image right, y image up, z towards
 * the camera), image b reads plane + b * plane_stride (0: one plane for the batch; else >= 4); occluders (B,K,4) f32: spheres
 * (cx, cy, cz, r) in camera space, 0 <= K <= 16, a sphere whose r is not > 0 (0, negative, NaN) is ignored (padding), one
 * with r = +inf holds every finite point.  All in f64:
 *   n = the plane's normal, normalised (d scaled with it), in the panorama's frame; the plane's points q have n.q + d = 0
 *   E0[b,ch] = sum_t pano[b,ch,t] max(n . omega_t, 0) dOmega_t
 *   pixel (i, j) with eml_gbuffer_shade_f32's unit ray hits the plane iff n . ray < 0, at p = (-d / (n . ray)) ray
 *   blocked(p, omega_t): for some sphere k with r_k > 0, oc = c_k - p, s = oc . omega_t:  |oc|^2 < r_k^2 (p inside the
 *     sphere), or s > 0 and |oc|^2 - s^2 < r_k^2
 *   D[b,ch,i,j] = sum over the blocked texels of pano[b,ch,t] max(n . omega_t, 0) dOmega_t  (a texel counts once)
 *   ratio = clamp(1 - D / E0, 0, 1) where the pixel hits the plane and E0[b,ch] > 0, exactly 1 elsewhere; a pixel inside a
 *   sphere is exactly 0; rounded to f32 once.  shadowed = image * ratio (one f32 product).
 * A plane with a zero or non-finite normal or with d not > 0 makes every value of that image NaN (the host cannot see a
 * device plane without a synchronisation; emlight_amd.insert refuses such a plane when it is given as numbers).
 * ratio (B,3,h,w) and shadowed (B,3,h,w) may each be NULL, not both; image (B,3,h,w) goes with shadowed.  The bits of either
 * output do not depend on the other being asked for.  Three launches: the per-texel terms and their 256-texel partial sums,
 * E0, the pixels (8 x 8 per wave).  The order of every sum is fixed (no atomics): run-to-run exact; a pixel adds its blocked
 * texels rows ascending, columns ascending, each texel once however many spheres block it, so an image's result does not
 * depend on the batch nor on the order of the spheres, and a padded or hidden sphere changes no bit.  Per wave and sphere only the hull of the 64 pixels' caps (asin(r / |oc|) about oc, as a row range
 * and a column interval that may wrap the seam; all columns when a cap holds a pole) is walked, less the rows under the
 * plane's horizon: culling skips only texels whose test is false or whose term is 0.
 * work: eml_ground_shadow_work_floats(B, H, h, w, K) floats (0 when a size is refused or B == 0), 8-byte aligned: the
 * 3 B (1 + ceil(2 H^2 / 256) + 2 H^2) doubles of the sums.  Only a library built with -DEML_GROUND_SHADOW_COUNTS (an
 * experiment build for tools/bench_ground_shadow.py) asks for more and writes, behind them, one uint64 per wave (4 per
 * 16 x 16 tile, tiles row-major per image): the texel tests that wave executed, 64 lanes per texel walked.
 * Limits: 0 <= B <= 65535 (B == 0 returns 0), 1 <= H <= 1024, 2 <= h, w <= 16384, 0 < fov_deg < 180 (an orthographic camera's
 * rays would need origins).  EML_EINVAL, with nothing enqueued: a NULL pano, plane or work; NULL occluders with K > 0; both
 * outputs NULL; image without shadowed or shadowed without image; W != 2H; K outside 0..16; a plane_stride of 1..3 or < 0;
 * fov_deg outside (0, 180) or a non-finite azimuth; limits; a misaligned work. */
size_t eml_ground_shadow_work_floats(int B, int H, int h, int w, int K);
int eml_ground_shadow_f32(const float* pano, int B, int H, int W, const float* plane, int plane_stride, const float* occluders,
                          int K, int h, int w, double fov_deg, double view_azimuth_deg, const float* image, float* ratio,
                          float* shadowed, float* work, eml_stream_t stream);

/* The adjoint of eml_ground_shadow_f32 (tests/shadow_grad_oracle.py): gradients for the panorama and
 * for the image.  With wgt[t] = max(n . omega_t, 0) dOmega_t, v = 1 - D / E0 and g = g_ratio + g_shadowed * image (in f64;
 * either gradient may be NULL, not both), over the active pixels (the pixel hits the plane, is not inside a sphere, E0 > 0):
 *   S[b,ch] = sum_p g (1 - v)      G[b,ch,t] = sum_p g blocked(p, t)
 *   dpano[b,ch,t]  = wgt[t] / E0[b,ch] (S - G)     (exactly 0 where wgt = 0 and for the whole of a channel with E0 <= 0)
 *   dimage[b,ch,p] = g_shadowed * ratio            (one f32 product of the forward's f32 ratio)
 * The gradient is that of the unclamped v: for a non-negative panorama 0 <= v <= 1 always holds; where negative texels make
 * the clamp bind, it is passed straight through.  Pixels inside a sphere, pixels off the plane and black channels add exactly
 * nothing.  plane and occluders get no gradient (visibility is binary).  Nothing is kept from the forward but its inputs: the
 * walk is the forward's own (csrc/ground_shadow_walk.h), every lane ends with the forward's D bit for bit.  G is a scatter,
 * added in 64-bit fixed point (units of 2^(e-61) with 2^e > sum_p |g| per image and channel) with integer atomics; every
 * other sum has a fixed order and there are no float atomics: run-to-run exact, an image's gradient does not depend on the
 * batch nor on the order of the spheres, a padded or hidden sphere changes no bit, and the bits of either output do not
 * depend on the other being asked for.
 * dpano (B,3,H,W) and dimage (B,3,h,w) may each be NULL, not both; g_shadowed needs image, dimage needs g_shadowed.
 * work: eml_ground_shadow_bwd_work_floats(B, H, h, w, K) floats (0 when a size is refused or B == 0), 8-byte aligned.
 * Limits and EML_EINVAL as eml_ground_shadow_f32, and: both gradients NULL; both outputs NULL; g_shadowed without image;
 * dimage without g_shadowed.  B == 0 returns 0. */
size_t eml_ground_shadow_bwd_work_floats(int B, int H, int h, int w, int K);
int eml_ground_shadow_bwd_f32(const float* pano, int B, int H, int W, const float* plane, int plane_stride,
                              const float* occluders, int K, int h, int w, double fov_deg, double view_azimuth_deg,
                              const float* image, const float* g_ratio, const float* g_shadowed, float* dpano, float* dimage,
                              float* work, eml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* EMLIGHT_HIP_EXT_H */
