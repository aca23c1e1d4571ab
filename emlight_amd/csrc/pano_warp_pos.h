// The source position of the panorama warp (GenProjector/util.py:279-343), shared by the forward (pano_warp.hip) and its
// gradients (pano_warp_bwd.hip): both make their taps and weights from the SAME snapped f64 position, bit for bit.  The
// depth-aware warp (pano_warp_depth.hip) uses the two halves on their own: the frame of a pixel, the position of a point.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace eml {
namespace warp {

constexpr double kPi = 3.14159265358979323846;
constexpr double kSnap = 1.0 / (double)(1 << 28);   // px
constexpr int kRun = 4;                              // images per evaluated position with by-value parameters

__device__ __forceinline__ double snap_px(double x) {
  const double n = rint(x);
  return fabs(x - n) < kSnap ? n : x;
}

// The frame of output pixel (i, j): e = Rp Rt d(i, j) and m = Rp Rt (0, 0, -1), the two terms of the warp's v = e + move * m.
// pano_warp_depth.hip walks the ray c + t e from the viewpoint c = move * m with the same e and m, bit for bit.
__device__ __forceinline__ void warp_frame(int i, int j, int h, int w, double theta_deg, double phi_deg, double& E0, double& E1,
                                           double& E2, double& m0, double& m1, double& m2) {
#pragma clang fp contract(off)
  const double lat = (double)i * kPi / (double)h - kPi / 2.0, lon = (double)j * (2.0 * kPi) / (double)w;
  const double clat = cos(lat);
  const double d0 = sin(lat), d1 = sin(lon) * clat, d2 = -cos(lon) * clat;
  const double theta = theta_deg / 180.0 * kPi, phi = phi_deg / 180.0 * kPi;
  const double ct = cos(theta), st = sin(theta), c = cos(phi), s = -sin(phi), k = 1.0 - c;
  // Rt d and Rt (0, 0, -1)
  const double e0 = d0, e1 = ct * d1 - st * d2, e2 = st * d1 + ct * d2;
  const double n0 = 0.0, n1 = st, n2 = -ct;
  // Rp, axis (0, ay, az)
  const double ay = ct, az = st;
  const double r00 = c, r01 = -az * s, r02 = ay * s;
  const double r10 = az * s, r11 = c + ay * ay * k, r12 = ay * az * k;
  const double r20 = -ay * s, r21 = az * ay * k, r22 = c + az * az * k;
  m0 = r00 * n0 + r01 * n1 + r02 * n2, m1 = r10 * n0 + r11 * n1 + r12 * n2, m2 = r20 * n0 + r21 * n1 + r22 * n2;
  E0 = r00 * e0 + r01 * e1 + r02 * e2;
  E1 = r10 * e0 + r11 * e1 + r12 * e2;
  E2 = r20 * e0 + r21 * e1 + r22 * e2;
}

// (row, col) of the direction of v in an H x W source, and len = |v|; false (and NaN positions) where there is none:
// |v| == 0 or not finite.
__device__ __forceinline__ bool direction_position(double v0, double v1, double v2, int H, int W, double& row, double& col,
                                                   double& len) {
#pragma clang fp contract(off)
  len = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  row = col = __builtin_nan("");
  if (!(len > 0.0) || !isfinite(len)) return false;
  const double s0 = fmin(fmax(v0 / len, -1.0), 1.0), s1 = v1 / len, s2 = v2 / len;
  double az_s = atan2(s1, -s2);
  if (az_s < 0.0) az_s += 2.0 * kPi;      // numpy's `% (2 pi)` on [-pi, pi]; -tiny + 2 pi rounds to 2 pi: col == W
  if (az_s == 0.0) az_s = 0.0;            // -0 -> +0
  const double r = snap_px((asin(s0) + kPi / 2.0) / kPi * (double)H);
  const double q = snap_px(az_s / (2.0 * kPi) * (double)W);
  if (!isfinite(r) || !isfinite(q)) return false;
  row = r;
  col = q;
  return true;
}

// (row, col) of output pixel (i, j); false (and NaNs) where the position is not finite: |v| == 0, possible only at
// |move| == 1, a NaN or infinite parameter, an overflow of move * m.
__device__ __forceinline__ bool warp_position(int i, int j, int h, int w, int H, int W, double theta_deg, double phi_deg,
                                              double move, double& row, double& col) {
#pragma clang fp contract(off)
  double E0, E1, E2, m0, m1, m2, len;
  warp_frame(i, j, h, w, theta_deg, phi_deg, E0, E1, E2, m0, m1, m2);
  const double v0 = E0 + move * m0;
  const double v1 = E1 + move * m1;
  const double v2 = E2 + move * m2;
  return direction_position(v0, v1, v2, H, W, row, col, len);
}

__device__ __forceinline__ int wrap_index(long long k, int n) {
  const int m = (int)(k % (long long)n);
  return m < 0 ? m + n : m;
}

}  // namespace warp
}  // namespace eml
