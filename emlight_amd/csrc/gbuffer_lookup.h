// The geometry of G-buffer shading, shared by the forward (gbuffer_shade.hip) and its adjoint (gbuffer_shade_bwd.hip): the
// pixel's frame (normal and reflection direction in the panorama's frame), where a direction lands on a map and the f32
// bilinear lookup.  Both kernels get the SAME taps, fractions and looked-up values, bit for bit (DESIGN.md sections 22, 23).
#pragma once
#include <hip/hip_runtime.h>

namespace eml {
namespace gbuf {

constexpr double kPi = 3.14159265358979323846;
constexpr int kThreads = 256;
constexpr int kMaxG = 4096;

__device__ __forceinline__ float lerp_f32(float a, float b, float t) {
  return t == 0.f ? a : __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, t)), __fmul_rn(b, t));
}

// where a direction lands on the G x 2G grid: rows r0, r1 (clamped), columns c0, c1 (wrapped), fractions rounded to f32
struct Taps {
  int r0, r1, c0, c1;
  float wx, wy;
};
__device__ __forceinline__ Taps direction_taps(const double* d, int G) {
  const int W = 2 * G;
  const double x = d[0] == 0.0 ? 0.0 : d[0], y = d[1] == 0.0 ? 0.0 : d[1];  // -0 is 0: the poles themselves have phi = 0
  const double th = atan2(sqrt(x * x + y * y), d[2]);
  double ph = atan2(y, x);
  if (ph < 0.0) ph += 2.0 * kPi;
  double v = th * (double)G / kPi - 0.5, u = ph * (double)W / (2.0 * kPi) - 0.5;
  v = !(v > 0.0) ? 0.0 : (v > (double)(G - 1) ? (double)(G - 1) : v);     // rows clamp (a NaN lands on row 0, in bounds)
  const double fv = floor(v), fu = floor(u);
  Taps m;
  m.r0 = (int)fv, m.r1 = m.r0 + 1 < G ? m.r0 + 1 : G - 1;
  m.c0 = (((int)fu % W) + W) % W, m.c1 = (m.c0 + 1) % W;                 // columns wrap
  m.wy = (float)(v - fv), m.wx = (float)(u - fu);
  return m;
}
__device__ __forceinline__ float lookup(const float* __restrict__ img, int W, const Taps& q) {
  const float top = lerp_f32(img[(size_t)q.r0 * W + q.c0], img[(size_t)q.r0 * W + q.c1], q.wx);
  const float bot = lerp_f32(img[(size_t)q.r1 * W + q.c0], img[(size_t)q.r1 * W + q.c1], q.wx);
  return lerp_f32(top, bot, q.wy);
}

// The frame of pixel (i, j) whose normal starts at normal[base] (planes hw apart): n and R in the panorama's frame.
// false for a normal of zero length (and NaN, infinite): the pixel is not shaded.
__device__ __forceinline__ bool pixel_frame(const float* __restrict__ normal, size_t base, int hw, int i, int j, int h, int w,
                                            double scl, double c, double s, double* n, double* R) {
  const double nx = normal[base], ny = normal[base + hw], nz = normal[base + 2 * (size_t)hw];
  // n = nx r + ny u + nz v with r = (-s, c, 0), u = (0, 0, 1), v = (-c, -s, 0)
  n[0] = nx * -s + nz * -c, n[1] = nx * c + nz * -s, n[2] = ny;
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (!(len > 0.0 && len < 1e300)) return false;
  n[0] /= len, n[1] /= len, n[2] /= len;
  double vp[3] = {-c, -s, 0.0};                                      // orthographic: v
  if (scl > 0.0) {
    const double sx = scl * (2.0 * j / (double)(w - 1) - 1.0);
    const double sy = (scl * (double)h / (double)w) * (2.0 * i / (double)(h - 1) - 1.0);
    const double rx = c + sx * -s, ry = s + sx * c, rz = -sy;        // f + sx r - sy u
    const double rl = sqrt(rx * rx + ry * ry + rz * rz);
    vp[0] = -rx / rl, vp[1] = -ry / rl, vp[2] = -rz / rl;
  }
  const double nv = n[0] * vp[0] + n[1] * vp[1] + n[2] * vp[2];
  R[0] = 2.0 * nv * n[0] - vp[0], R[1] = 2.0 * nv * n[1] - vp[1], R[2] = 2.0 * nv * n[2] - vp[2];
  return true;
}

}  // namespace gbuf
}  // namespace eml
