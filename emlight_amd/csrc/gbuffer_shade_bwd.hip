// Object insertion: the adjoint of G-buffer shading and of the composite (gbuffer_shade.hip; DESIGN.md section 23;
// tests/insert_grad_oracle.py restates the definition in float64).
//
// One thread per pixel, as in the forward, evaluates the SAME frame, taps and lookups (gbuffer_lookup.h) and, for the
// composite, the forward's own f32 sequence for `shaded`; from these the upstream gradient g_s of the shaded value.
//   pixel pass    dkd, dks, dkm (and dshaded in the composite-only mode); per map the tile's sum of |k g_s| in f64, a fixed tree
//   scale pass    S[b][map] = the tiles' partials in a fixed order
//   scatter pass  the pixel's state again; per map q = rint(w_tap k g_s / u) added into acc[b][ch][texel] with 64-bit integer
//                 atomics, u = 2^(e - 61) with 2^e the power of two above S.  Integer addition is associative: the bits do not
//                 depend on the arrival order, the batch, or which gradients were asked for together (section 20's design).
//                 A texel's exact sum is bounded by S < 2^e, so |sum q| < 2^61 + (taps on the texel) / 2: no overflow.
//   convert pass  dmap = (float)acc * u: one correctly rounded int64 -> f32 conversion and an exact scaling
// Zero contributions are not added; a texel nothing lands on stays at the 0 the accumulator was cleared to.
// The launcher only enqueues: one memset node, at most six kernels.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "gbuffer_lookup.h"

#include <cmath>
#include <cstdint>

namespace {

using namespace eml::gbuf;

constexpr int kUnitBits = 61;                             // |q| < 2^61
constexpr int kDiffuseMap = 0, kPhongMap = 1, kPanoMap = 2;

struct Args {
  const float *g, *pano, *ed, *eg, *normal, *coverage, *kd, *ks, *km, *shaded, *exposure;
  int H, Hd, Hg, h, w;
  long d_stride, g_stride;
  double scl, c, s, inv_gamma;
};

// what both passes know of a pixel: whether it is shaded, the taps of the evaluated terms, its coefficients and g_s
struct Pixel {
  bool valid;
  Taps qd, qg, qm;
  float k[3][3], look[3][3], gs[3];                       // [map][channel]
};

// the derivative of clamp(e s, 0, 1)^(1 / gamma) coverage with respect to s, times the upstream gradient: 0 outside the
// OPEN interval 0 < e s < 1, so always finite.  x = fl(e s) as the forward forms it; the power in f64, rounded once.
__device__ __forceinline__ float composite_gs(float g, float cov, float e, float sh, double inv_gamma) {
  const float x = __fmul_rn(e, sh);
  if (!(x > 0.f && x < 1.f)) return 0.f;
  const double up = (double)g * (double)cov * (double)e;
  return (float)(inv_gamma == 1.0 ? up : up * inv_gamma * exp2((inv_gamma - 1.0) * log2((double)x)));
}

// need_look: the looked-up values are wanted (a coefficient gradient, or the composite's recomputation of `shaded`)
__device__ __forceinline__ Pixel pixel_state(const Args& a, int b, int p, bool need_look) {
  Pixel px;
  px.valid = false;
  const int hw = a.h * a.w, i = p / a.w, j = p - i * a.w;
  const size_t base = (size_t)b * 3 * hw + p;
  const float cov = a.coverage[(size_t)b * hw + p];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) px.gs[ch] = 0.f;
  if (cov == 0.f) return px;                              // nothing else of this pixel is read
  double n[3], R[3];
  if (!pixel_frame(a.normal, base, hw, i, j, a.h, a.w, a.scl, a.c, a.s, n, R)) return px;
  px.valid = true;
  const bool look = need_look || a.exposure;
  float sh[3] = {0.f, 0.f, 0.f};
  if (a.kd) {
    px.qd = direction_taps(n, a.Hd);
    const float* img = a.ed + (size_t)b * (size_t)a.d_stride;
    const size_t T = 2 * (size_t)a.Hd * a.Hd;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      px.k[kDiffuseMap][ch] = a.kd[base + (size_t)ch * hw];
      if (look) {
        px.look[kDiffuseMap][ch] = lookup(img + ch * T, 2 * a.Hd, px.qd);
        sh[ch] = __fmul_rn(px.k[kDiffuseMap][ch], px.look[kDiffuseMap][ch]);
      }
    }
  }
  if (a.ks) {
    px.qg = direction_taps(R, a.Hg);
    const float* img = a.eg + (size_t)b * (size_t)a.g_stride;
    const size_t T = 2 * (size_t)a.Hg * a.Hg;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      px.k[kPhongMap][ch] = a.ks[base + (size_t)ch * hw];
      if (look) {
        px.look[kPhongMap][ch] = lookup(img + ch * T, 2 * a.Hg, px.qg);
        const float term = __fmul_rn(px.k[kPhongMap][ch], px.look[kPhongMap][ch]);
        sh[ch] = a.kd ? __fadd_rn(sh[ch], term) : term;
      }
    }
  }
  if (a.km) {
    px.qm = direction_taps(R, a.H);
    const size_t T = 2 * (size_t)a.H * a.H;
    const float* img = a.pano + (size_t)b * 3 * T;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      px.k[kPanoMap][ch] = a.km[base + (size_t)ch * hw];
      if (look) {
        px.look[kPanoMap][ch] = lookup(img + ch * T, 2 * a.H, px.qm);
        const float term = __fmul_rn(px.k[kPanoMap][ch], px.look[kPanoMap][ch]);
        sh[ch] = (a.kd || a.ks) ? __fadd_rn(sh[ch], term) : term;
      }
    }
  }
  const float e = a.exposure ? a.exposure[b] : 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float g = a.g[base + (size_t)ch * hw];
    px.gs[ch] = a.exposure ? composite_gs(g, cov, e, sh[ch], a.inv_gamma) : g;
  }
  return px;
}

// sum over the wave, the same bits in every lane: each step adds a pair in both of its lanes (a + b == b + a)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = v + eml::shfl_xor_d(v, o);
  return v;
}

// grid (tiles, B).  The composite-only mode (no coefficient): dshaded from `shaded`, nothing else.
// tile_part (B, 3 maps, tiles) f64 or null: the tile's sum of |k g_s| per map.
__global__ __launch_bounds__(kThreads) void shade_bwd_pixel_kernel(Args a, float* __restrict__ dkd, float* __restrict__ dks,
                                                                   float* __restrict__ dkm, float* __restrict__ dshaded,
                                                                   double* __restrict__ tile_part) {
#pragma clang fp contract(off)
  __shared__ double sw[3][4];
  const int p = blockIdx.x * kThreads + threadIdx.x, hw = a.h * a.w, b = blockIdx.y;
  const bool inside = p < hw;
  const size_t base = (size_t)b * 3 * hw + p;
  if (!a.kd && !a.ks && !a.km) {
    if (!inside) return;
    const float cov = a.coverage[(size_t)b * hw + p];
    const float e = a.exposure[b];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const size_t o = base + (size_t)ch * hw;
      dshaded[o] = cov == 0.f ? 0.f : composite_gs(a.g[o], cov, e, a.shaded[o], a.inv_gamma);
    }
    return;
  }
  Pixel px;
  px.valid = false;
  if (inside) px = pixel_state(a, b, p, dkd || dks || dkm);
  float* const dk[3] = {dkd, dks, dkm};
  const bool has[3] = {a.kd != nullptr, a.ks != nullptr, a.km != nullptr};
  double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int mp = 0; mp < 3; ++mp) {
    if (!has[mp]) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (dk[mp] && inside) dk[mp][base + (size_t)ch * hw] = px.valid ? __fmul_rn(px.gs[ch], px.look[mp][ch]) : 0.f;
      if (px.valid) sum[mp] = sum[mp] + fabs((double)px.k[mp][ch] * (double)px.gs[ch]);
    }
  }
  if (!tile_part) return;
  // the tile's sums: a tree inside each wave, then the four waves in order
#pragma unroll
  for (int mp = 0; mp < 3; ++mp) {
    const double v = wave_sum_d(sum[mp]);
    if ((threadIdx.x & 63) == 0) sw[mp][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int mp = threadIdx.x;
    tile_part[((size_t)b * 3 + mp) * gridDim.x + blockIdx.x] = ((sw[mp][0] + sw[mp][1]) + sw[mp][2]) + sw[mp][3];
  }
}

// grid (3, B): S[b][map] = the tiles' partials, thread t adding tiles t, t + 256, ... in order, then the tile tree
__global__ __launch_bounds__(kThreads) void shade_bwd_scale_kernel(const double* __restrict__ tile_part, int ntiles,
                                                                   double* __restrict__ S) {
#pragma clang fp contract(off)
  __shared__ double sw[4];
  const size_t row = (size_t)blockIdx.y * 3 + blockIdx.x;
  const double* part = tile_part + row * ntiles;
  double v = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += kThreads) v = v + part[t];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) S[row] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// the exponent e of S < 2^e (0 for S == 0; 1025 for an infinite or NaN S: still a valid scale)
__device__ __forceinline__ int exponent_of(double S) {
  if (S == 0.0) return 0;
  return (int)((__double_as_longlong(S) >> 52) & 0x7ff) - 1022;
}

__device__ __forceinline__ void add_fixed(unsigned long long* p, double c) {
  if (!(fabs(c) < 0x1p62)) return;        // a non-finite grad_out: that image is unspecified, the conversion stays defined
  const long long q = (long long)rint(c);
  if (q != 0) atomicAdd(p, (unsigned long long)q);
}

// one map's four taps of one pixel: planar accumulator acc (3, G 2G) of this image
__device__ __forceinline__ void scatter_map(unsigned long long* __restrict__ acc, int G, const Taps& q, const float* k,
                                            const float* gs, double inv) {
#pragma clang fp contract(off)
  const int W = 2 * G;
  const size_t T = (size_t)G * W;
  const double wx = (double)q.wx, wy = (double)q.wy;
  const double w00 = (1.0 - wx) * (1.0 - wy), w01 = wx * (1.0 - wy), w10 = (1.0 - wx) * wy, w11 = wx * wy;
  const size_t t00 = (size_t)q.r0 * W + q.c0, t01 = (size_t)q.r0 * W + q.c1, t10 = (size_t)q.r1 * W + q.c0,
               t11 = (size_t)q.r1 * W + q.c1;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double v = (double)k[ch] * (double)gs[ch] * inv;
    unsigned long long* a = acc + ch * T;
    add_fixed(a + t00, w00 * v);
    add_fixed(a + t01, w01 * v);
    add_fixed(a + t10, w10 * v);
    add_fixed(a + t11, w11 * v);
  }
}

// grid (tiles, B).  acc_d (B, 3, Hd 2Hd), acc_g, acc_p int64 or null; S (B, 3) f64
__global__ __launch_bounds__(kThreads) void shade_bwd_scatter_kernel(Args a, const double* __restrict__ S,
                                                                     unsigned long long* __restrict__ acc_d,
                                                                     unsigned long long* __restrict__ acc_g,
                                                                     unsigned long long* __restrict__ acc_p) {
  const int p = blockIdx.x * kThreads + threadIdx.x, hw = a.h * a.w, b = blockIdx.y;
  if (p >= hw) return;
  const Pixel px = pixel_state(a, b, p, false);
  if (!px.valid) return;
  if (acc_d)
    scatter_map(acc_d + (size_t)b * 6 * a.Hd * a.Hd, a.Hd, px.qd, px.k[kDiffuseMap], px.gs,
                ldexp(1.0, kUnitBits - exponent_of(S[(size_t)b * 3 + kDiffuseMap])));
  if (acc_g)
    scatter_map(acc_g + (size_t)b * 6 * a.Hg * a.Hg, a.Hg, px.qg, px.k[kPhongMap], px.gs,
                ldexp(1.0, kUnitBits - exponent_of(S[(size_t)b * 3 + kPhongMap])));
  if (acc_p)
    scatter_map(acc_p + (size_t)b * 6 * a.H * a.H, a.H, px.qm, px.k[kPanoMap], px.gs,
                ldexp(1.0, kUnitBits - exponent_of(S[(size_t)b * 3 + kPanoMap])));
}

// grid (ceil(n / 256), B): out (B, n) f32 from acc (B, n) int64, n = 3 G 2G
__global__ __launch_bounds__(kThreads) void shade_bwd_convert_kernel(const unsigned long long* __restrict__ acc,
                                                                     const double* __restrict__ S, int mp, size_t n,
                                                                     float* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int e = exponent_of(S[(size_t)blockIdx.y * 3 + mp]);
  out[(size_t)blockIdx.y * n + k] = ldexpf((float)(long long)acc[(size_t)blockIdx.y * n + k], e - kUnitBits);
}

bool sizes_ok(int B, int h, int w) { return B >= 0 && B <= 65535 && h >= 2 && w >= 2 && (long)h * w <= (1l << 29); }
bool height_ok(int G) { return G >= 1 && G <= kMaxG; }

// `work` in 8-byte words: [acc_d B 3 Hd 2Hd][acc_g B 3 Hg 2Hg][acc_p B 3 H 2H] as wanted, then [tile_part B 3 tiles][S B 3]
struct Layout {
  size_t acc_d, acc_g, acc_p, tile_part, S, total;
  int ntiles;
};
Layout layout(int B, int H, int Hd, int Hg, int h, int w, bool want_pano, bool want_d, bool want_g) {
  Layout L;
  L.ntiles = (h * w + kThreads - 1) / kThreads;
  L.acc_d = 0;
  L.acc_g = L.acc_d + (want_d ? (size_t)B * 6 * Hd * Hd : 0);
  L.acc_p = L.acc_g + (want_g ? (size_t)B * 6 * Hg * Hg : 0);
  L.tile_part = L.acc_p + (want_pano ? (size_t)B * 6 * H * H : 0);
  const bool any = want_pano || want_d || want_g;
  L.S = L.tile_part + (any ? (size_t)B * 3 * L.ntiles : 0);
  L.total = L.S + (any ? (size_t)B * 3 : 0);
  return L;
}

}  // namespace

extern "C" size_t eml_gbuffer_shade_bwd_work_floats(int B, int H, int Hd, int Hg, int h, int w, int want_dpano,
                                                    int want_d_e_diffuse, int want_d_e_phong) {
  if (!sizes_ok(B, h, w) || B == 0) return 0;
  if ((want_dpano && !height_ok(H)) || (want_d_e_diffuse && !height_ok(Hd)) || (want_d_e_phong && !height_ok(Hg))) return 0;
  return 2 * layout(B, H, Hd, Hg, h, w, want_dpano != 0, want_d_e_diffuse != 0, want_d_e_phong != 0).total;
}

// Index arithmetic: pixel indices are int (h * w <= 2^29); texel and element offsets are size_t.
extern "C" int eml_gbuffer_shade_bwd_f32(const float* grad_out, const float* pano, int H, const float* e_diffuse, int Hd,
                                         long d_stride, const float* e_phong, int Hg, long g_stride, const float* normal,
                                         const float* coverage, const float* kd, const float* ks, const float* km, int B,
                                         int h, int w, double fov_deg, double view_azimuth_deg, const float* shaded,
                                         const float* exposure, double gamma, float* dkd, float* dks, float* dkm,
                                         float* d_e_diffuse, float* d_e_phong, float* dpano, float* dshaded, float* work,
                                         eml_stream_t stream) {
  const bool given = !kd && !ks && !km;
  if (!grad_out) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: null grad_out");
  if (!coverage || (!normal && !given)) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: null normal or coverage");
  if (!dkd && !dks && !dkm && !d_e_diffuse && !d_e_phong && !dpano && !dshaded)
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: null outputs: no gradient is asked for");
  if (given && (!shaded || !exposure || !dshaded))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: no coefficient: kd, ks and km are all null (the composite alone "
                                 "needs shaded, exposure and the dshaded output)");
  if (given && (dkd || dks || dkm || d_e_diffuse || d_e_phong || dpano))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: no coefficient: only dshaded is defined for the composite alone");
  if (!given && (shaded || dshaded))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: shaded and dshaded belong to the composite alone (no coefficient)");
  if (kd && (!e_diffuse || Hd < 1 || Hd > kMaxG || d_stride < 6l * Hd * Hd))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: kd needs e_diffuse, 1 <= Hd <= %d and a stride of at least 3 Hd 2Hd",
                     kMaxG);
  if (ks && (!e_phong || Hg < 1 || Hg > kMaxG || g_stride < 6l * Hg * Hg))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: ks needs e_phong, 1 <= Hg <= %d and a stride of at least 3 Hg 2Hg",
                     kMaxG);
  if (km && (!pano || H < 1 || H > kMaxG))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: km needs pano and 1 <= H <= %d", kMaxG);
  if (!kd && (dkd || d_e_diffuse))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: dkd and d_e_diffuse need kd: a term without coefficient is not evaluated");
  if (!ks && (dks || d_e_phong))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: dks and d_e_phong need ks: a term without coefficient is not evaluated");
  if (!km && (dkm || dpano))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: dkm and dpano need km: a term without coefficient is not evaluated");
  if (exposure && !(gamma > 0.0 && gamma <= 1e6))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: gamma must be in (0, 1e6] for the composite");
  if (!(fov_deg >= 0.0 && fov_deg < 180.0) || !(view_azimuth_deg - view_azimuth_deg == 0.0))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: fov_deg must be in [0, 180) and the azimuth finite");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: B must be 0..65535 (grid.y)");
  if (h < 2 || w < 2 || (long)h * w > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: image size: h, w >= 2 and h w <= 2^29, got %d x %d", h, w);
  if (B == 0) return EML_OK;
  const bool scatter = d_e_diffuse || d_e_phong || dpano;
  if (scatter && (!work || ((uintptr_t)work & 7)))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_bwd_f32: work is null or not 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const double az = view_azimuth_deg * (kPi / 180.0);
  Args a;
  a.g = grad_out, a.pano = pano, a.ed = e_diffuse, a.eg = e_phong, a.normal = normal, a.coverage = coverage;
  a.kd = kd, a.ks = ks, a.km = km, a.shaded = shaded, a.exposure = exposure;
  a.H = H, a.Hd = Hd, a.Hg = Hg, a.h = h, a.w = w, a.d_stride = d_stride, a.g_stride = g_stride;
  a.scl = fov_deg > 0.0 ? tan(fov_deg * (kPi / 180.0) * 0.5) : 0.0;
  a.c = cos(az), a.s = sin(az), a.inv_gamma = exposure ? 1.0 / gamma : 1.0;
  const Layout L = layout(B, H, Hd, Hg, h, w, dpano != nullptr, d_e_diffuse != nullptr, d_e_phong != nullptr);
  double* words = reinterpret_cast<double*>(work);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(work);
  unsigned long long* acc_d = d_e_diffuse ? acc + L.acc_d : nullptr;
  unsigned long long* acc_g = d_e_phong ? acc + L.acc_g : nullptr;
  unsigned long long* acc_p = dpano ? acc + L.acc_p : nullptr;
  double* tile_part = scatter ? words + L.tile_part : nullptr;
  double* S = scatter ? words + L.S : nullptr;
  const dim3 grid(L.ntiles, B);
  if (scatter) {
    const hipError_t e = hipMemsetAsync(acc, 0, L.tile_part * sizeof(unsigned long long), st);
    if (e != hipSuccess)
      return eml::fail((int)e > 0 ? (int)e : EML_ELAUNCH, "eml_gbuffer_shade_bwd_f32(clear): %s", hipGetErrorString(e));
  }
  if (scatter || dkd || dks || dkm || dshaded) {
    hipLaunchKernelGGL(shade_bwd_pixel_kernel, grid, dim3(kThreads), 0, st, a, dkd, dks, dkm, dshaded, tile_part);
    if (int rc = eml::check_launch("eml_gbuffer_shade_bwd_f32", "pixels")) return rc;
  }
  if (!scatter) return EML_OK;
  hipLaunchKernelGGL(shade_bwd_scale_kernel, dim3(3, B), dim3(kThreads), 0, st, (const double*)tile_part, L.ntiles, S);
  hipLaunchKernelGGL(shade_bwd_scatter_kernel, grid, dim3(kThreads), 0, st, a, (const double*)S, acc_d, acc_g, acc_p);
  if (int rc = eml::check_launch("eml_gbuffer_shade_bwd_f32", "scatter")) return rc;
  const struct {
    unsigned long long* acc;
    int G, mp;
    float* out;
  } maps[3] = {{acc_d, Hd, kDiffuseMap, d_e_diffuse}, {acc_g, Hg, kPhongMap, d_e_phong}, {acc_p, H, kPanoMap, dpano}};
  for (const auto& m : maps) {
    if (!m.out) continue;
    const size_t n = 6 * (size_t)m.G * m.G;
    hipLaunchKernelGGL(shade_bwd_convert_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads), B), dim3(kThreads), 0, st,
                       (const unsigned long long*)m.acc, (const double*)S, m.mp, n, m.out);
  }
  return eml::check_launch("eml_gbuffer_shade_bwd_f32", "convert");
}
