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

#ifdef __cplusplus
}
#endif

#endif /* EMLIGHT_HIP_EXT_H */
