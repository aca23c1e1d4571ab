// Depth-aware panorama warp: the panorama and its depth as seen from another position, with the scene's own geometry
// instead of the unit sphere of resize_exr (GenProjector/util.py:279-343).  depth (B,H,W) is the distance from the source
// viewpoint to the surface along each pixel's direction, in the units of gmloss/utils.py:63-73 (`geometric_points` scales the
// unit anchors by it); `move` is in the same units.
//
// Frame: that of pano_warp.hip, from the same code (pano_warp_pos.h).  For output pixel (i, j), e = Rp Rt d(i, j) and
// m = Rp Rt (0, 0, -1); the new viewpoint is c = move * m and a point on the pixel's ray is P(t) = c + t e.
// Position of a point P: s = P / |P|, row = (asin(clamp(s0)) + pi/2) / pi * H, col = (atan2(s1, -s2) mod 2 pi) / (2 pi) * W,
// snapped to an integer when closer than 2^-28 px (direction_position).  D(P): the bilinear sample of the depth map there,
// f64 weights, the four products summed in the order 00, 01, 10, 11; columns wrap, rows CLAMP (i0 = min(floor(row), H-1),
// i1 = min(i0 + 1, H-1)): blending the last row with row 0, as the colour warp does after cv2's BORDER_WRAP, would mix the
// distance to the floor with the distance to the ceiling.
//
// Pre-pass, one workgroup per sample, fixed-order tree: dmin, dmax and a flag (a pixel that is not finite or not > 0) into
// `work`.  A sample is invalid if the flag is set, if one of its three parameters is not finite, or if the viewpoint is on or
// outside the surface (|c| > 0 and |c| >= D(c)); every output pixel of an invalid sample is NaN, nothing else is touched.
//
// Root of g(t) = |P(t)| - D(P(t)); a point with |P| == 0 (the ray passes through the source viewpoint) counts as inside,
// g < 0.  Bracket t_lo = max(0, dmin - |c|), t_hi = dmax + |c|: g(t_lo) <= 0 <= g(t_hi) by the triangle inequality and the
// bounds of bilinear interpolation.  March t_k = t_lo + (t_hi - t_lo) k / steps, k = 1..steps (t_steps = t_hi exactly); the
// first k with g(t_k) >= 0 -- k = steps if rounding leaves none -- gives a = t_{k-1}, b = t_k: the NEAREST surface.  Then
// `bisections` rounds of mid = (a + b) / 2, g(mid) >= 0 ? b = mid : a = mid, and t = (a + b) / 2.  Both loops have fixed trip
// counts.  out_depth = (float)t, (row, col) = position of P(t), out_pano = the clamped-row bilinear sample of pano there
// (f64 sum, one rounding), hit = (t, row, col).  The search treats the depth map as one connected surface: what the source
// viewpoint never saw is not filled, the surface is stretched across it.
//
// One thread per output pixel; the up to steps + bisections dependent lookups of a pixel gather the depth map through the
// caches.  A variant that staged the sample's map into LDS once per workgroup was measured slower and is
// not kept.
//
// No contraction into FMAs, no atomics: a pixel is one fixed sequence of IEEE operations, so an image gives the same bits in
// any batch, with by-value and with per-sample parameters.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "pano_warp_pos.h"

#include <cmath>

namespace {

using namespace eml::warp;

constexpr int kWorkPerSample = 4;          // dmin, dmax, flag, unused

// fixed-order reduction of (min, max, any-bad) over a sample's depth map
__global__ __launch_bounds__(1024) void depth_range_kernel(const float* __restrict__ depth, int H, int W,
                                                           float* __restrict__ work) {
  __shared__ float lo[1024], hi[1024];
  __shared__ int bad[1024];
  const float* d = depth + (size_t)blockIdx.x * H * W;
  const int tid = threadIdx.x;
  float mn = __builtin_inff(), mx = 0.f;
  int b = 0;
  for (int p = tid; p < H * W; p += 1024) {
    const float v = d[p];
    if (!(isfinite(v) && v > 0.f)) {
      b = 1;
    } else {
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  lo[tid] = mn, hi[tid] = mx, bad[tid] = b;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) {
      lo[tid] = fminf(lo[tid], lo[tid + s]);
      hi[tid] = fmaxf(hi[tid], hi[tid + s]);
      bad[tid] |= bad[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* o = work + (size_t)blockIdx.x * kWorkPerSample;
    o[0] = lo[0];
    o[1] = hi[0];
    o[2] = bad[0] ? 1.f : 0.f;
    o[3] = 0.f;
  }
}

struct Taps {
  int o00, o01, o10, o11;
  double w00, w01, w10, w11;
};

// row in [0, H], col in [0, W], both finite (direction_position returned true); rows clamp, columns wrap
__device__ __forceinline__ Taps clamped_taps(double row, double col, int H, int W) {
#pragma clang fp contract(off)
  const double fr = floor(row), fc = floor(col);
  const double yd = row - fr, xd = col - fc;
  const int i0 = min(max((int)fr, 0), H - 1), i1 = min(i0 + 1, H - 1);
  const int j0 = wrap_index((long long)fc, W), j1 = j0 + 1 == W ? 0 : j0 + 1;
  Taps t;
  t.o00 = i0 * W + j0, t.o01 = i0 * W + j1, t.o10 = i1 * W + j0, t.o11 = i1 * W + j1;
  t.w00 = (1.0 - yd) * (1.0 - xd), t.w01 = (1.0 - yd) * xd, t.w10 = yd * (1.0 - xd), t.w11 = yd * xd;
  return t;
}

__device__ __forceinline__ double depth_at(const float* D, const Taps& t) {
#pragma clang fp contract(off)
  double v = (double)D[t.o00] * t.w00;
  v = v + (double)D[t.o01] * t.w01;
  v = v + (double)D[t.o10] * t.w10;
  v = v + (double)D[t.o11] * t.w11;
  return v;
}

// g(t) >= 0 ?  (outside or on the surface)
__device__ __forceinline__ bool outside(const float* D, int H, int W, double c0, double c1, double c2, double e0, double e1,
                                        double e2, double t) {
#pragma clang fp contract(off)
  double row, col, len;
  if (!direction_position(c0 + t * e0, c1 + t * e1, c2 + t * e2, H, W, row, col, len)) return false;
  return len - depth_at(D, clamped_taps(row, col, H, W)) >= 0.0;
}

// One output pixel.  D: the sample's depth map.
__device__ __forceinline__ void search_pixel(const float* __restrict__ D, const float* __restrict__ img, int H, int W, int h, int w, int p,
                                             double theta_deg, double phi_deg, double move, float dmin, float dmax, bool bad,
                                             int steps, int bisections, float* __restrict__ op, float* __restrict__ od,
                                             double* __restrict__ oh) {
#pragma clang fp contract(off)
  const int i = p / w, j = p - i * w;
  const double nan = __builtin_nan("");
  double t = nan, row = nan, col = nan;
  bool ok = !bad && isfinite(theta_deg) && isfinite(phi_deg) && isfinite(move);
  double e0, e1, e2, m0, m1, m2;
  if (ok) {
    warp_frame(i, j, h, w, theta_deg, phi_deg, e0, e1, e2, m0, m1, m2);
    const double c0 = move * m0, c1 = move * m1, c2 = move * m2;
    double crow, ccol, clen;
    const bool moved = direction_position(c0, c1, c2, H, W, crow, ccol, clen);     // false at c == 0: clen == 0
    if (!isfinite(clen) || (clen > 0.0 && !moved)) ok = false;
    if (ok && moved && clen >= depth_at(D, clamped_taps(crow, ccol, H, W))) ok = false;   // on or outside the surface
    if (ok) {
      const double t_lo = fmax(0.0, (double)dmin - clen), t_hi = (double)dmax + clen;
      const double span = t_hi - t_lo;
      double a = t_lo, b = t_hi;
      for (int k = 1; k < steps; ++k) {               // at most steps - 1 lookups: t_steps = t_hi closes the bracket unasked
        const double tk = t_lo + span * (double)k / (double)steps;
        if (outside(D, H, W, c0, c1, c2, e0, e1, e2, tk)) {
          b = tk;
          break;
        }
        a = tk;
      }
      for (int r = 0; r < bisections; ++r) {
        const double mid = 0.5 * (a + b);
        if (outside(D, H, W, c0, c1, c2, e0, e1, e2, mid)) b = mid;
        else a = mid;
      }
      t = 0.5 * (a + b);
      double len;
      if (!direction_position(c0 + t * e0, c1 + t * e1, c2 + t * e2, H, W, row, col, len)) {
        t = nan;
        ok = false;
      }
    }
  }
  if (oh) oh[0] = t, oh[1] = row, oh[2] = col;
  if (od) *od = (float)t;
  if (op) {
    if (!ok) {
      op[0] = op[1] = op[2] = __builtin_nanf("");
    } else {
      const Taps s = clamped_taps(row, col, H, W);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        double v = (double)img[(size_t)s.o00 * 3 + ch] * s.w00;
        v = v + (double)img[(size_t)s.o01 * 3 + ch] * s.w01;
        v = v + (double)img[(size_t)s.o10 * 3 + ch] * s.w10;
        v = v + (double)img[(size_t)s.o11 * 3 + ch] * s.w11;
        op[ch] = (float)v;
      }
    }
  }
}

struct Args {
  const float* pano;
  const float* depth;
  int H, W, h, w;
  double theta_deg, phi_deg, move;
  const double* params;
  int steps, bisections;
  float* out_pano;
  float* out_depth;
  double* hit;
  const float* work;
};

__device__ __forceinline__ void run_pixel(const Args& a, const float* D, int b, int p) {
  double theta = a.theta_deg, phi = a.phi_deg, move = a.move;
  if (a.params) {
    theta = a.params[(size_t)b * 3];
    phi = a.params[(size_t)b * 3 + 1];
    move = a.params[(size_t)b * 3 + 2];
  }
  const float* wk = a.work + (size_t)b * kWorkPerSample;
  const size_t q = (size_t)b * a.h * a.w + p;
  search_pixel(D, a.pano ? a.pano + (size_t)b * a.H * a.W * 3 : nullptr, a.H, a.W, a.h, a.w, p, theta, phi, move, wk[0], wk[1],
               wk[2] != 0.f, a.steps, a.bisections, a.out_pano ? a.out_pano + q * 3 : nullptr,
               a.out_depth ? a.out_depth + q : nullptr, a.hit ? a.hit + q * 3 : nullptr);
}

// grid (pixel tiles of 256, B)
__global__ __launch_bounds__(256) void pano_warp_depth_kernel(Args a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.h * a.w) return;
  const int b = blockIdx.y;
  run_pixel(a, a.depth + (size_t)b * a.H * a.W, b, p);
}

bool sizes_ok(int B, int H, int W) {
  return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W <= (1l << 29);
}

}  // namespace

extern "C" size_t eml_pano_warp_depth_work_floats(int B, int H, int W) {
  if (!sizes_ok(B, H, W)) return 0;
  return (size_t)B * kWorkPerSample;
}

// Index arithmetic: pixel indices are int (h * w, H * W <= 2^29, so 3 * H * W < 2^31 too); element offsets are size_t.
extern "C" int eml_pano_warp_depth_f32(const float* pano, const float* depth, int B, int H, int W, int h, int w, double theta_deg,
                                       double phi_deg, double move, const double* params_dev, int steps, int bisections,
                                       float* out_pano, float* out_depth, double* hit, float* work, eml_stream_t stream) {
  const char* me = "eml_pano_warp_depth_f32";
  if (!depth || !work) return eml::fail(EML_EINVAL, "%s: null depth or work", me);
  if (!out_pano && !out_depth) return eml::fail(EML_EINVAL, "%s: no output (out_pano and out_depth are both null)", me);
  if (out_pano && !pano) return eml::fail(EML_EINVAL, "%s: out_pano without pano", me);
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "%s: B must be 0..65535 (grid.y)", me);
  if (H < 1 || W < 1 || h < 1 || w < 1 || (long)H * W > (1l << 29) || (long)h * w > (1l << 29))
    return eml::fail(EML_EINVAL, "%s: bad size (H, W, h, w >= 1; H * W, h * w <= 2^29)", me);
  if (!params_dev && !(std::isfinite(theta_deg) && std::isfinite(phi_deg) && std::isfinite(move)))
    return eml::fail(EML_EINVAL, "%s: theta, phi or move is not finite", me);
  if (steps < 1 || steps > 1024) return eml::fail(EML_EINVAL, "%s: steps must be 1..1024, got %d", me, steps);
  if (bisections < 0 || bisections > 60) return eml::fail(EML_EINVAL, "%s: bisections must be 0..60, got %d", me, bisections);
  if (B == 0) return EML_OK;
  hipLaunchKernelGGL(depth_range_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, depth, H, W, work);
  int rc = eml::check_launch(me, "range");
  if (rc) return rc;
  const Args a{pano, depth, H, W, h, w, theta_deg, phi_deg, move, params_dev, steps, bisections, out_pano, out_depth, hit, work};
  hipLaunchKernelGGL(pano_warp_depth_kernel, dim3((h * w + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, a);
  return eml::check_launch(me, "search");
}
