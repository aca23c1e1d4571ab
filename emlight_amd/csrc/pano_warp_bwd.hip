// Gradients of the panorama warp (pano_warp.hip; the reference's resize_exr, GenProjector/util.py:279-343, has none: this is
// its adjoint with respect to the panorama and its derivative with respect to theta, phi, move).  DESIGN.md section 20 and
// include/emlight_hip_ext.h hold the definition.
//
// One thread per output pixel, as in the forward, evaluates the SAME snapped f64 position (pano_warp_pos.h), hence the same
// taps and the same f64 weights w00, w01, w10, w11.
//
// dpano: the contributions w_k g[ch] are a scatter whose pattern depends on the parameters.  They are accumulated in 64-bit
// integers: integer addition is associative, so the atomics give the same bits in any order, in any batch and on every run.
//   pass 1  S_b = sum |grad_out[b]| in f64 in a fixed order (kAbsChunks partials per image, each a fixed tree)
//   scale   e_b with S_b < 2^e_b (the exponent of S_b);  unit u_b = 2^(e_b - 61)
//   pass 2  q = rint(w_k g / u_b), |q| < 2^61, added into acc[b][ch][texel] (planar, so a wave's adds touch adjacent words)
//           A texel's exact sum is bounded by sum_p |g[b,p,ch]| <= S_b < 2^e_b, so |sum q| < 2^61 + (taps on the texel) / 2:
//           no overflow for any input that is finite.
//   pass 3  dpano = (float)acc * u_b: one correctly rounded int64 -> f32 conversion and an exact scaling
// Error: each contribution is rounded to a multiple of u_b once, |error| <= u_b / 2 <= 2^-61 S_b; a texel that n taps land on
// is off by at most n 2^-61 S_b before the single f32 rounding.  Zero contributions are not added; a texel nothing lands on
// stays at the 0 the accumulator was cleared to.
//
// dparams: forward-mode derivative of the unsnapped position with three tangents (theta_deg, phi_deg, move), all in f64,
// times the bilinear slopes in the cell the forward used; the per-pixel terms are reduced in a fixed order: a tree inside
// the 256-pixel tile, the tiles' partials in `work`, then one pass per image (as gt_param.hip does).  No atomics.
//
// The launcher only enqueues: one memset node, at most four kernels.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "pano_warp_pos.h"

#include <cmath>
#include <cstdint>

namespace {

using namespace eml::warp;

constexpr int kAbsChunks = 64;                            // partial sums of |grad_out| per image: one wave adds them
constexpr double kPole = 1.0 / (double)(1 << 20);         // s1^2 + s2^2 below this: the pixel adds nothing to dparams
constexpr int kUnitBits = 61;                             // |q| < 2^61

// value and the derivatives with respect to (theta_deg, phi_deg, move)
struct Dual {
  double v, t[3];
};
__device__ __forceinline__ Dual cst(double v) { return {v, {0.0, 0.0, 0.0}}; }
__device__ __forceinline__ Dual var(double v, int q) {
  Dual r = cst(v);
  r.t[q] = 1.0;
  return r;
}
__device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) {
  return {a.v + b.v, {a.t[0] + b.t[0], a.t[1] + b.t[1], a.t[2] + b.t[2]}};
}
__device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) {
  return {a.v - b.v, {a.t[0] - b.t[0], a.t[1] - b.t[1], a.t[2] - b.t[2]}};
}
__device__ __forceinline__ Dual operator-(const Dual& a) { return {-a.v, {-a.t[0], -a.t[1], -a.t[2]}}; }
__device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) {
  return {a.v * b.v, {a.t[0] * b.v + a.v * b.t[0], a.t[1] * b.v + a.v * b.t[1], a.t[2] * b.v + a.v * b.t[2]}};
}
__device__ __forceinline__ Dual operator*(const Dual& a, double b) { return {a.v * b, {a.t[0] * b, a.t[1] * b, a.t[2] * b}}; }
__device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) {
  const double q = a.v / b.v;
  return {q, {(a.t[0] - q * b.t[0]) / b.v, (a.t[1] - q * b.t[1]) / b.v, (a.t[2] - q * b.t[2]) / b.v}};
}
__device__ __forceinline__ Dual dsin(const Dual& a) {
  const double c = cos(a.v);
  return {sin(a.v), {c * a.t[0], c * a.t[1], c * a.t[2]}};
}
__device__ __forceinline__ Dual dcos(const Dual& a) {
  const double s = -sin(a.v);
  return {cos(a.v), {s * a.t[0], s * a.t[1], s * a.t[2]}};
}
__device__ __forceinline__ Dual dsqrt(const Dual& a) {
  const double r = sqrt(a.v), k = 0.5 / r;
  return {r, {k * a.t[0], k * a.t[1], k * a.t[2]}};
}

// d row / dq and d col / dq of the unsnapped position of pano_warp_pos.h (the clamp of s0, the `mod 2 pi` and the snap are
// the identity).  false where the pixel adds nothing: no finite direction, or the pole rule.  1 - s0^2 is s1^2 + s2^2.
__device__ __forceinline__ bool warp_tangents(int i, int j, int h, int w, int H, int W, double theta_deg, double phi_deg,
                                              double move, double* drow, double* dcol) {
#pragma clang fp contract(off)
  const double lat = (double)i * kPi / (double)h - kPi / 2.0, lon = (double)j * (2.0 * kPi) / (double)w;
  const double clat = cos(lat);
  const double d0 = sin(lat), d1 = sin(lon) * clat, d2 = -cos(lon) * clat;
  const Dual theta = var(theta_deg, 0) * (1.0 / 180.0) * kPi, phi = var(phi_deg, 1) * (1.0 / 180.0) * kPi, mv = var(move, 2);
  const Dual ct = dcos(theta), st = dsin(theta), c = dcos(phi), s = -dsin(phi), k = cst(1.0) - c;
  const Dual e0 = cst(d0), e1 = ct * d1 - st * d2, e2 = st * d1 + ct * d2;
  const Dual n1 = st, n2 = -ct;
  const Dual ay = ct, az = st;
  const Dual r00 = c, r01 = -(az * s), r02 = ay * s;
  const Dual r10 = az * s, r11 = c + ay * ay * k, r12 = ay * az * k;
  const Dual r20 = -(ay * s), r21 = az * ay * k, r22 = c + az * az * k;
  const Dual m0 = r01 * n1 + r02 * n2, m1 = r11 * n1 + r12 * n2, m2 = r21 * n1 + r22 * n2;
  const Dual v0 = (r00 * e0 + r01 * e1 + r02 * e2) + mv * m0;
  const Dual v1 = (r10 * e0 + r11 * e1 + r12 * e2) + mv * m1;
  const Dual v2 = (r20 * e0 + r21 * e1 + r22 * e2) + mv * m2;
  const Dual len = dsqrt(v0 * v0 + v1 * v1 + v2 * v2);
  if (!(len.v > 0.0) || !isfinite(len.v)) return false;
  const Dual s0 = v0 / len, s1 = v1 / len, s2 = v2 / len;
  const double rho2 = s1.v * s1.v + s2.v * s2.v;
  if (!(rho2 >= kPole)) return false;
  // asin'(s0) = 1 / sqrt(1 - s0^2);  atan2(y, x)' = (x dy - y dx) / (x^2 + y^2) with y = s1, x = -s2
  const double ka = (double)H / kPi / sqrt(rho2), kc = (double)W / (2.0 * kPi) / rho2;
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    drow[q] = ka * s0.t[q];
    dcol[q] = kc * (s1.v * s2.t[q] - s2.v * s1.t[q]);
    finite = finite && isfinite(drow[q]) && isfinite(dcol[q]);
  }
  return finite;
}

// sum over the wave, the same bits in every lane: each step adds a pair in both of its lanes (a + b == b + a)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = v + eml::shfl_xor_d(v, o);
  return v;
}

// the exponent e of an image's S = sum |grad_out|, S < 2^e, from its kAbsChunks partials; called by one whole wave
__device__ __forceinline__ int image_exponent(const double* __restrict__ part) {
  const double S = wave_sum_d(part[threadIdx.x & 63]);
  if (!(S > 0.0)) return 0;
  return (int)((__double_as_longlong(S) >> 52) & 0x7ff) - 1022;      // 1025 for an infinite S: still a valid scale
}

// grid (kAbsChunks, B): part[b][chunk] = sum of |g[b][k]| over k = chunk * 256 + tid (mod kAbsChunks * 256), n = 3 h w
__global__ __launch_bounds__(256) void pano_warp_abs_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sw[4];
  const float* gb = g + (size_t)blockIdx.y * n;
  double a = 0.0;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)kAbsChunks * 256) a = a + fabs((double)gb[k]);
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * kAbsChunks + blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

__device__ __forceinline__ void add_fixed(unsigned long long* p, double c) {
  if (!(fabs(c) < 0x1p62)) return;        // a non-finite grad_out: that image is unspecified, the conversion stays defined
  const long long q = (long long)rint(c);
  if (q != 0) atomicAdd(p, (unsigned long long)q);
}

// grid (pixel tiles, runs) as pano_warp_kernel.  acc (B, 3, H W) int64 or null; par_part (B, ntiles, 3) f64 or null.
__global__ __launch_bounds__(256) void pano_warp_bwd_kernel(const float* __restrict__ g, const float* __restrict__ pano, int B,
                                                            int H, int W, int h, int w, double theta_deg, double phi_deg,
                                                            double move, const double* __restrict__ params, int per,
                                                            const double* __restrict__ abs_part,
                                                            unsigned long long* __restrict__ acc, double* __restrict__ par_part) {
#pragma clang fp contract(off)
  __shared__ double s_inv[kRun];
  __shared__ double s_red[4][kRun * 3];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool inside = p < h * w;
  const int b0 = blockIdx.y * per, b1 = min(B, b0 + per), nb = b1 - b0;
  const int wave = threadIdx.x >> 6;
  if (acc) {                              // wave k: the unit of image b0 + k
    if (wave < nb) {
      const int e = image_exponent(abs_part + (size_t)(b0 + wave) * kAbsChunks);
      if ((threadIdx.x & 63) == 0) s_inv[wave] = ldexp(1.0, kUnitBits - e);
    }
    __syncthreads();
  }
  const int i = inside ? p / w : 0, j = inside ? p - i * w : 0;
  if (params) {
    theta_deg = params[(size_t)b0 * 3];
    phi_deg = params[(size_t)b0 * 3 + 1];
    move = params[(size_t)b0 * 3 + 2];
  }
  double row, col;
  const bool ok = warp_position(i, j, h, w, H, W, theta_deg, phi_deg, move, row, col) && inside;
  // row in [0, H], col in [0, W] where ok: finite, so the casts are defined; every index is reduced modulo the size
  const double fr = ok ? floor(row) : 0.0, fc = ok ? floor(col) : 0.0;
  const double yd = ok ? row - fr : 0.0, xd = ok ? col - fc : 0.0;
  const int i0 = wrap_index((long long)fr, H), j0 = wrap_index((long long)fc, W);
  const int i1 = i0 + 1 == H ? 0 : i0 + 1, j1 = j0 + 1 == W ? 0 : j0 + 1;
  const int t00 = i0 * W + j0, t01 = i0 * W + j1, t10 = i1 * W + j0, t11 = i1 * W + j1;
  const size_t plane = (size_t)h * w, HW = (size_t)H * W;
  if (acc && ok) {
    const double w00 = (1.0 - yd) * (1.0 - xd), w01 = (1.0 - yd) * xd, w10 = yd * (1.0 - xd), w11 = yd * xd;
    for (int b = b0; b < b1; ++b) {
      const float* gp = g + ((size_t)b * plane + p) * 3;
      const double inv = s_inv[b - b0];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double gv = (double)gp[ch];
        unsigned long long* a = acc + ((size_t)b * 3 + ch) * HW;
        add_fixed(a + t00, w00 * gv * inv);
        add_fixed(a + t01, w01 * gv * inv);
        add_fixed(a + t10, w10 * gv * inv);
        add_fixed(a + t11, w11 * gv * inv);
      }
    }
  }
  if (!par_part) return;
  double drow[3], dcol[3];
  const bool live = ok && warp_tangents(i, j, h, w, H, W, theta_deg, phi_deg, move, drow, dcol);
  double term[kRun * 3];
#pragma unroll
  for (int k = 0; k < kRun * 3; ++k) term[k] = 0.0;
  if (live) {
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      const int b = b0 + r;
      if (b >= b1) break;
      const float* img = pano + (size_t)b * HW * 3;
      const float* gp = g + ((size_t)b * plane + p) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double I00 = (double)img[(size_t)t00 * 3 + ch], I01 = (double)img[(size_t)t01 * 3 + ch];
        const double I10 = (double)img[(size_t)t10 * 3 + ch], I11 = (double)img[(size_t)t11 * 3 + ch];
        const double o_r = (1.0 - xd) * (I10 - I00) + xd * (I11 - I01);
        const double o_c = (1.0 - yd) * (I01 - I00) + yd * (I11 - I10);
        const double gv = (double)gp[ch];
#pragma unroll
        for (int q = 0; q < 3; ++q) term[r * 3 + q] = term[r * 3 + q] + gv * (o_r * drow[q] + o_c * dcol[q]);
      }
    }
  }
  // the tile's sum: a tree inside each wave, then the four waves in order
#pragma unroll
  for (int k = 0; k < kRun * 3; ++k) {
    const double v = wave_sum_d(term[k]);
    if ((threadIdx.x & 63) == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < nb * 3) {
    const int k = threadIdx.x, b = b0 + k / 3, q = k - (k / 3) * 3;
    par_part[((size_t)b * gridDim.x + blockIdx.x) * 3 + q] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
  }
}

// grid (ceil(3 H W / 256), B): dpano (B, H, W, 3) f32 from acc (B, 3, H W)
__global__ __launch_bounds__(256) void pano_warp_dpano_kernel(const unsigned long long* __restrict__ acc,
                                                              const double* __restrict__ abs_part, size_t HW,
                                                              float* __restrict__ dpano) {
  __shared__ int s_e;
  if (threadIdx.x < 64) {
    const int e = image_exponent(abs_part + (size_t)blockIdx.y * kAbsChunks);
    if (threadIdx.x == 0) s_e = e;
  }
  __syncthreads();
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= HW * 3) return;
  const size_t t = k / 3, ch = k - t * 3;
  const long long q = (long long)acc[((size_t)blockIdx.y * 3 + ch) * HW + t];
  dpano[(size_t)blockIdx.y * HW * 3 + k] = ldexpf((float)q, s_e - kUnitBits);
}

// grid (B): dparams[b][q] = the tiles' partials, thread t adding tiles t, t + 256, ... in order, then the tile tree
__global__ __launch_bounds__(256) void pano_warp_dparams_kernel(const double* __restrict__ par_part, int ntiles,
                                                                double* __restrict__ dparams) {
#pragma clang fp contract(off)
  __shared__ double s_red[4][3];
  const double* part = par_part + (size_t)blockIdx.x * ntiles * 3;
  double a[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < ntiles; t += 256)
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = a[q] + part[(size_t)t * 3 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double v = wave_sum_d(a[q]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    dparams[(size_t)blockIdx.x * 3 + q] = ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
  }
}

bool sizes_ok(int B, int H, int W, int h, int w) {
  return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && (long)H * W <= (1l << 29) && (long)h * w <= (1l << 29);
}

// `work` in 8-byte words: [acc B 3 H W][abs_part B kAbsChunks] when dpano is wanted, [par_part B ntiles 3] when dparams is
struct Layout {
  size_t acc, abs_part, par_part, total;
  int ntiles;
};
Layout layout(int B, int H, int W, int h, int w, bool want_dpano, bool want_dparams) {
  Layout L;
  L.ntiles = (h * w + 255) / 256;
  L.acc = 0;
  L.abs_part = want_dpano ? (size_t)B * 3 * H * W : 0;
  L.par_part = L.abs_part + (want_dpano ? (size_t)B * kAbsChunks : 0);
  L.total = L.par_part + (want_dparams ? (size_t)B * L.ntiles * 3 : 0);
  return L;
}

}  // namespace

extern "C" size_t eml_pano_warp_bwd_work_floats(int B, int H, int W, int h, int w, int want_dpano, int want_dparams) {
  if (!sizes_ok(B, H, W, h, w) || B == 0) return 0;
  return 2 * layout(B, H, W, h, w, want_dpano != 0, want_dparams != 0).total;
}

// Index arithmetic: pixel and texel indices are int (h * w, H * W <= 2^29); element offsets are size_t.
extern "C" int eml_pano_warp_bwd_f32(const float* grad_out, const float* pano, int B, int H, int W, int h, int w,
                                     double theta_deg, double phi_deg, double move, const double* params_dev, float* dpano,
                                     double* dparams, float* work, eml_stream_t stream) {
  if (!grad_out) return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: null grad_out");
  if (!dpano && !dparams) return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: neither dpano nor dparams is asked for");
  if (dparams && !pano) return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: dparams needs the panorama (null pano)");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: B must be 0..65535 (grid.y)");
  if (!sizes_ok(B, H, W, h, w))
    return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: bad size (H, W, h, w >= 1; H * W, h * w <= 2^29)");
  if (!params_dev && !(std::isfinite(theta_deg) && std::isfinite(phi_deg) && std::isfinite(move)))
    return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: theta, phi or move is not finite");
  if (B == 0) return EML_OK;
  if (!work || ((uintptr_t)work & 7)) return eml::fail(EML_EINVAL, "eml_pano_warp_bwd_f32: work is null or not 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const Layout L = layout(B, H, W, h, w, dpano != nullptr, dparams != nullptr);
  double* words = reinterpret_cast<double*>(work);
  unsigned long long* acc = dpano ? reinterpret_cast<unsigned long long*>(words + L.acc) : nullptr;
  double* abs_part = dpano ? words + L.abs_part : nullptr;
  double* par_part = dparams ? words + L.par_part : nullptr;
  const size_t HW = (size_t)H * W;
  if (dpano) {
    const hipError_t e = hipMemsetAsync(acc, 0, (size_t)B * 3 * HW * sizeof(unsigned long long), st);
    if (e != hipSuccess) return eml::fail((int)e > 0 ? (int)e : EML_ELAUNCH, "eml_pano_warp_bwd_f32(clear): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(pano_warp_abs_kernel, dim3(kAbsChunks, B), dim3(256), 0, st, grad_out, (size_t)h * w * 3, abs_part);
    if (int rc = eml::check_launch("eml_pano_warp_bwd_f32", "abs")) return rc;
  }
  // shared parameters: every thread evaluates its position once for a run of kRun images, as the forward does
  const int per = params_dev ? 1 : kRun;
  hipLaunchKernelGGL(pano_warp_bwd_kernel, dim3(L.ntiles, (B + per - 1) / per), dim3(256), 0, st, grad_out, pano, B, H, W, h, w,
                     theta_deg, phi_deg, move, params_dev, per, abs_part, acc, par_part);
  if (int rc = eml::check_launch("eml_pano_warp_bwd_f32", "scatter")) return rc;
  if (dpano) {
    hipLaunchKernelGGL(pano_warp_dpano_kernel, dim3((unsigned)((HW * 3 + 255) / 256), B), dim3(256), 0, st, acc, abs_part, HW,
                       dpano);
    if (int rc = eml::check_launch("eml_pano_warp_bwd_f32", "dpano")) return rc;
  }
  if (dparams) {
    hipLaunchKernelGGL(pano_warp_dparams_kernel, dim3(B), dim3(256), 0, st, par_part, L.ntiles, dparams);
    if (int rc = eml::check_launch("eml_pano_warp_bwd_f32", "dparams")) return rc;
  }
  return EML_OK;
}
