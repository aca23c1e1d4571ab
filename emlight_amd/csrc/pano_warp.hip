// Panorama warp on the device: the reference's resize_exr (GenProjector/util.py:279-343, copy in GenProjector/tools/util.py)
// for a batch.  The output frame is rotated about two axes, the viewpoint is shifted by `move` along the rotated -z axis,
// the direction is renormalised and the source is resampled bilinearly with wrap-around on both axes (BORDER_WRAP).
//
// One thread per output pixel evaluates the source position in f64, as pano_crop_kernel does:
//   lat = i pi / h - pi / 2, lon = j 2 pi / w (no half-pixel offset: the reference has none)
//   d   = (sin lat, sin lon cos lat, -cos lon cos lat)
//   Rt  = rotation about x by theta; Rp = Rodrigues' rotation about a = (0, cos theta, sin theta) with cosine cos(phi) and
//         sine -sin(phi) (the reference negates it, util.py:301)
//   v   = Rp Rt d + move * Rp Rt (0, 0, -1),  s = v / |v|
//   row = (asin(s0) + pi / 2) / pi * H,  col = (atan2(s1, -s2) mod 2 pi) / (2 pi) * W
// and gathers the four taps (floor mod size and their +1 neighbours mod size) for a run of images.  The weights are the f64
// fractions; the four products are summed in f64 in the order 00, 01, 10, 11 and rounded to f32 once.  row == H and
// col == W occur (s0 == 1; `mod 2 pi` rounding up to 2 pi) and land on index 0.  cv2 quantises the weights to 1/32 px; that
// is not reproduced.
//
// A position closer than 2^-28 px to an integer IS that integer: asin(sin(lat)) returns lat only to some 1e-13 px (more
// near the poles and for larger H), and a tap weight of 1e-13 on a neighbour 10^6 times brighter -- HDR panoramas have
// those -- changes the f32 result.  With the snap the identity warp (theta = phi = move = 0 at the source's size) returns
// the source bit for bit; 2^-28 px is far below the f32 accuracy of the reference's own maps.  The exported coordinates are
// the snapped ones, the ones the taps and weights are made from.
//
// No contraction into FMAs (the pragma below), no atomics: the arithmetic of a pixel is one fixed sequence of IEEE
// operations, the same with by-value and with per-sample parameters, so an image gives the same bits in any batch.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "pano_warp_pos.h"

#include <cmath>

namespace {

using namespace eml::warp;   // warp_position, wrap_index, kRun: pano_warp_pos.h, shared with pano_warp_bwd.hip

// grid (pixel tiles, runs): blockIdx.y covers images [y * per, (y + 1) * per); with params (one (theta, phi, move) per
// sample) per == 1.  out (B, h, w, 3); coords (n_sets, h, w, 2) or null, n_sets = B with params, else 1 (run 0 writes it).
__global__ __launch_bounds__(256) void pano_warp_kernel(const float* __restrict__ pano, int B, int H, int W, int h, int w,
                                                        double theta_deg, double phi_deg, double move,
                                                        const double* __restrict__ params, int per,
                                                        float* __restrict__ out, double* __restrict__ coords) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int b0 = blockIdx.y * per, b1 = min(B, b0 + per);
  const int i = p / w, j = p - i * w;
  if (params) {
    theta_deg = params[(size_t)b0 * 3];
    phi_deg = params[(size_t)b0 * 3 + 1];
    move = params[(size_t)b0 * 3 + 2];
  }
  double row, col;
  const bool ok = warp_position(i, j, h, w, H, W, theta_deg, phi_deg, move, row, col);
  const size_t plane = (size_t)h * w;
  if (coords && (params || blockIdx.y == 0)) {
    double* cd = coords + ((size_t)(params ? b0 : 0) * plane + p) * 2;
    cd[0] = row;
    cd[1] = col;
  }
  if (!ok) {                              // nothing is loaded
    for (int b = b0; b < b1; ++b) {
      float* o = out + ((size_t)b * plane + p) * 3;
      o[0] = o[1] = o[2] = __builtin_nanf("");
    }
    return;
  }
  // row in [0, H], col in [0, W]: finite, so the casts are defined; every index is reduced modulo the size
  const double fr = floor(row), fc = floor(col);
  const double yd = row - fr, xd = col - fc;
  const int i0 = wrap_index((long long)fr, H), j0 = wrap_index((long long)fc, W);
  const int i1 = i0 + 1 == H ? 0 : i0 + 1, j1 = j0 + 1 == W ? 0 : j0 + 1;
  const double w00 = (1.0 - yd) * (1.0 - xd), w01 = (1.0 - yd) * xd, w10 = yd * (1.0 - xd), w11 = yd * xd;
  const size_t o00 = ((size_t)i0 * W + j0) * 3, o01 = ((size_t)i0 * W + j1) * 3;
  const size_t o10 = ((size_t)i1 * W + j0) * 3, o11 = ((size_t)i1 * W + j1) * 3;
  for (int b = b0; b < b1; ++b) {
    const float* img = pano + (size_t)b * H * W * 3;
    float* o = out + ((size_t)b * plane + p) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double v = (double)img[o00 + ch] * w00;
      v = v + (double)img[o01 + ch] * w01;
      v = v + (double)img[o10 + ch] * w10;
      v = v + (double)img[o11 + ch] * w11;
      o[ch] = (float)v;
    }
  }
}

}  // namespace

// Index arithmetic: pixel indices are int (h * w, H * W <= 2^29, so 3 * H * W < 2^31 too); byte offsets are size_t.
extern "C" int eml_pano_warp_f32(const float* pano, int B, int H, int W, int h, int w, double theta_deg, double phi_deg,
                                 double move, const double* params_dev, float* out, double* coords, eml_stream_t stream) {
  if (!pano || !out) return eml::fail(EML_EINVAL, "eml_pano_warp_f32: null pointer");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_pano_warp_f32: B must be 0..65535 (grid.y)");
  if (H < 1 || W < 1 || h < 1 || w < 1 || (long)H * W > (1l << 29) || (long)h * w > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_pano_warp_f32: bad size (H, W, h, w >= 1; H * W, h * w <= 2^29)");
  if (!params_dev && !(std::isfinite(theta_deg) && std::isfinite(phi_deg) && std::isfinite(move)))
    return eml::fail(EML_EINVAL, "eml_pano_warp_f32: theta, phi or move is not finite");
  if (B == 0) return EML_OK;
  // shared parameters: every thread evaluates its position once for a run of kRun images
  const int per = params_dev ? 1 : kRun;
  const dim3 grid((h * w + 255) / 256, (B + per - 1) / per);
  hipLaunchKernelGGL(pano_warp_kernel, grid, dim3(256), 0, (hipStream_t)stream, pano, B, H, W, h, w, theta_deg, phi_deg, move,
                     params_dev, per, out, coords);
  return eml::check_launch("eml_pano_warp_f32");
}
