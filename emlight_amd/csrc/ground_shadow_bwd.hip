// Object insertion: the adjoint of the ground-plane shadow (tests/shadow_grad_oracle.py restates it in
// float64).  The ratio is v = 1 - D / E0 with E0 = sum_t pano wgt and D = sum_t pano wgt blocked(p, t), two linear
// functionals of the panorama.  With g = g_ratio + g_shadowed * image (f64), over the active pixels (the pixel hits the plane,
// is not inside a sphere, E0 > 0):
//   S[b,ch]    = sum_p g (1 - v)          G[b,ch,t] = sum_p g blocked(p, t)
//   dpano      = wgt / E0 (S - G)         dimage    = g_shadowed * ratio (one f32 product of the forward's f32 ratio)
// The gradient is that of the unclamped v: a non-negative panorama never reaches the clamp, and where negative texels do, the
// clamp is passed straight through.  Visibility is binary: plane and occluders get no gradient.
// G is the transpose of the forward's add under the bits, a scatter.  It is added in 64-bit fixed point: per image and channel
// A = sum_p |g| (fixed tree), 2^e > A, every pixel's g is rounded ONCE to units of 2^(e - 61) and the integers are added
// (associative: run-to-run exact, independent of the batch, of the order of the spheres and of padded or hidden spheres).
// Launches: weight_kernel and e0_kernel as the forward (ground_shadow_walk.h); [clear G]; the sums of |g| (abs_kernel, then
// e0_kernel over its partials); shadow_bwd_kernel: the forward's walk, so every lane ends with the forward's D, and per chunk
// the transpose: lane q owns column cb + q and adds the fixed-point g of the lanes whose word has bit q set, then issues at
// most one integer atomic per (wave, column, channel); after the walk g (1 - v) goes through the block tree to a per-tile
// partial of S and dimage is written; e0_kernel over the S partials; dpano_kernel, one thread per texel.  No float atomics.
#include "ground_shadow_walk.h"
#include "../../include/emlight_hip_ext.h"

namespace {

using namespace shadow;

constexpr int kUnitBits = 61;          // |g| <= A < 2^e: a pixel's integer is below 2^61 and the sum of all of them below 2^62

// g[b,ch,p] in f64; the product of two floats is exact in a double
__device__ __forceinline__ double upstream(const float* __restrict__ g_ratio, const float* __restrict__ g_shadowed,
                                           const float* __restrict__ image, size_t k) {
#pragma clang fp contract(off)
  const double a = g_ratio ? (double)g_ratio[k] : 0.0;
  const double m = g_shadowed ? (double)g_shadowed[k] * (double)image[k] : 0.0;
  return a + m;
}

// e with 2^e > A; 0 for A = 0, 1025 for a non-finite A (still a valid scale), no less than -900 so that 2^(61 - e) is finite
__device__ __forceinline__ int fixed_exponent(double A) {
  if (!(A > 0.0)) return 0;
  return max((int)((__double_as_longlong(A) >> 52) & 0x7ff) - 1022, -900);
}

__device__ __forceinline__ long long to_fixed(double c) {
  if (!(fabs(c) < 0x1p62)) return 0;     // a non-finite gradient: that image is unspecified, the conversion stays defined
  return (long long)rint(c);
}

__device__ __forceinline__ long long readlane_i64(long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffull), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// grid (ceil(h w / 256), B): part[b][block][ch] = sum of |g| over the block's 256 pixels, fixed tree
__global__ __launch_bounds__(kThreads) void abs_kernel(const float* __restrict__ g_ratio, const float* __restrict__ g_shadowed,
                                                       const float* __restrict__ image, size_t hw, double* __restrict__ part) {
  __shared__ double red[3 * kThreads];
  const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (p < hw) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = fabs(upstream(g_ratio, g_shadowed, image, ((size_t)blockIdx.y * 3 + ch) * hw + p));
  }
  block_sum3(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + ch] = v[ch];
  }
}

// grid (ceil(w / 16), ceil(h / 16), B) and dynamic LDS as shadow_kernel.  acc (B, 3, H W) int64, cleared, or null (dimage
// alone: the walk only finds the ratio); s_part (B, tiles, 3); dimage (B, 3, h, w) or null
__global__ __launch_bounds__(kThreads) void shadow_bwd_kernel(const double* __restrict__ wp, const double* __restrict__ e0, int H,
                                                              const float* __restrict__ plane, int plane_stride,
                                                              const float* __restrict__ occluders, int K, int h, int w, double scl,
                                                              double c, double s, const float* __restrict__ image,
                                                              const float* __restrict__ g_ratio, const float* __restrict__ g_shadowed,
                                                              const double* __restrict__ gabs, unsigned long long* __restrict__ acc,
                                                              double* __restrict__ s_part, float* __restrict__ dimage) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  __shared__ int box[kThreads / 64][kMaxK][4];
  __shared__ double stage[kThreads / 64][3 * 64];                          // after the walk: the tree of block_sum3
  static_assert(sizeof(stage) == 3 * kThreads * sizeof(double), "stage doubles as block_sum3's scratch");
  const int b = blockIdx.z, lane = threadIdx.x & 63, W = 2 * H;
  const size_t HW = (size_t)H * W, hw = (size_t)h * w;
  int i, j;
  pixel_of_thread(&i, &j);
  const bool in_image = i < h && j < w;
  const size_t base = (size_t)b * 3 * hw + (size_t)i * w + j;
  double g[3] = {0.0, 0.0, 0.0};
  long long q[3] = {0, 0, 0};                                              // g in units of 2^(e - 61); 0 for a black channel
  if (acc && in_image) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      g[ch] = upstream(g_ratio, g_shadowed, image, base + ch * hw);
      if (e0[b * 3 + ch] > 0.0) q[ch] = to_fixed(g[ch] * ldexp(1.0, kUnitBits - fixed_exponent(gabs[b * 3 + ch])));
    }
  }
  const bool carries = (q[0] | q[1] | q[2]) != 0;

  const Pixel p = walk(wp, H, plane, plane_stride, occluders, K, h, w, scl, c, s, lds, box, stage, nullptr,
                       [&](int r, int cb, int ce, unsigned long long bits) {
    if (!acc) return;
    // the transpose of the add: a pixel that is not active has no bit set, so only active pixels are ever added
    long long sum[3] = {0, 0, 0};
    for (unsigned long long who = __ballot(bits != 0 && carries); who; who &= who - 1) {
      const int l = __builtin_ctzll(who);
      const bool on = ((unsigned long long)readlane_i64((long long)bits, l) >> lane) & 1ull;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sum[ch] += on ? readlane_i64(q[ch], l) : 0ll;
    }
    if (lane < ce - cb) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        if (sum[ch] != 0) atomicAdd(acc + ((size_t)b * 3 + ch) * HW + (size_t)r * W + cb + lane, (unsigned long long)sum[ch]);
    }
  });

  double sv[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double E = e0[b * 3 + ch];
    if (p.hit && !p.inside && E > 0.0) sv[ch] = g[ch] * (p.acc[ch] / E);  // g (1 - v) of the unclamped v
    if (dimage && in_image) dimage[base + ch * hw] = __fmul_rn(g_shadowed[base + ch * hw], (float)ratio_value(p, ch, E));
  }
  if (!acc) return;
  __syncthreads();                                                         // every wave is done with its slot of stage
  block_sum3(sv, &stage[0][0]);
  if (threadIdx.x == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, ntiles = (size_t)gridDim.y * gridDim.x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s_part[((size_t)b * ntiles + tile) * 3 + ch] = sv[ch];
  }
}

// grid (ceil(H W / 256), B): dpano = wgt / E0 (S - G); exactly 0 where wgt = 0 and for the whole of a black channel
__global__ __launch_bounds__(kThreads) void dpano_kernel(int H, const float* __restrict__ plane, int plane_stride, double c, double s,
                                                         const double* __restrict__ e0, const double* __restrict__ gabs,
                                                         const double* __restrict__ ssum,
                                                         const unsigned long long* __restrict__ acc, float* __restrict__ dpano) {
#pragma clang fp contract(off)
  const int W = 2 * H, HW = H * W, b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= HW) return;
  double n[3] = {0.0, 0.0, 0.0}, d = 0.0;
  const bool ok = plane_frame(plane + (size_t)b * plane_stride, c, s, n, &d);
  const double wgt = ok ? texel_weight(n, H, W, t) : 0.0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const size_t k = ((size_t)b * 3 + ch) * HW + t;
    const double E = e0[b * 3 + ch];
    float out = 0.f;
    if (E > 0.0 && wgt > 0.0) {
      const double G = (double)(long long)acc[k] * ldexp(1.0, fixed_exponent(gabs[b * 3 + ch]) - kUnitBits);
      out = (float)(wgt / E * (ssum[b * 3 + ch] - G));
    }
    dpano[k] = out;
  }
}

inline size_t pixel_blocks(int h, int w) { return ((size_t)h * w + kThreads - 1) / kThreads; }

}  // namespace

// doubles: the forward's E0, partials and wp; then A and S (3 B each), the partials of A (3 B pixel blocks) and of S
// (3 B tiles), and the 3 B H W 64-bit accumulators of G
extern "C" size_t eml_ground_shadow_bwd_work_floats(int B, int H, int h, int w, int K) {
  if (!sizes_ok(B, H, h, w, K) || B == 0) return 0;
  const size_t HW = (size_t)2 * H * H;
  return 2 * (size_t)B * 3 * (1 + weight_blocks(H) + HW + 2 + pixel_blocks(h, w) + tiles(h, w) + HW);
}

extern "C" int eml_ground_shadow_bwd_f32(const float* pano, int B, int H, int W, const float* plane, int plane_stride,
                                         const float* occluders, int K, int h, int w, double fov_deg, double view_azimuth_deg,
                                         const float* image, const float* g_ratio, const float* g_shadowed, float* dpano,
                                         float* dimage, float* work, eml_stream_t stream) {
  const char* who = "eml_ground_shadow_bwd_f32";
  if (!pano || !plane || !work) return eml::fail(EML_EINVAL, "%s: null pano, plane or work", who);
  if (!g_ratio && !g_shadowed) return eml::fail(EML_EINVAL, "%s: null gradients: g_ratio and g_shadowed", who);
  if (!dpano && !dimage) return eml::fail(EML_EINVAL, "%s: null outputs: dpano and dimage", who);
  if (g_shadowed && !image) return eml::fail(EML_EINVAL, "%s: g_shadowed needs image (shadowed = image * ratio)", who);
  if (dimage && !g_shadowed) return eml::fail(EML_EINVAL, "%s: dimage needs g_shadowed (dimage = g_shadowed * ratio)", who);
  if (int rc = refuse_geometry(who, work, B, H, W, plane_stride, occluders, K, h, w, fov_deg, view_azimuth_deg)) return rc;
  if (B == 0) return EML_OK;
  const size_t nblk = weight_blocks(H), HW = (size_t)2 * H * H, pblk = pixel_blocks(h, w), ntiles = tiles(h, w);
  double* e0 = reinterpret_cast<double*>(work);
  double* partial = e0 + (size_t)3 * B;
  double* wp = partial + (size_t)3 * B * nblk;
  double* gabs = wp + (size_t)3 * B * HW;
  double* ssum = gabs + (size_t)3 * B;
  double* a_part = ssum + (size_t)3 * B;
  double* s_part = a_part + (size_t)3 * B * pblk;
  unsigned long long* acc = dpano ? reinterpret_cast<unsigned long long*>(s_part + (size_t)3 * B * ntiles) : nullptr;
  const double az = view_azimuth_deg * (kPi / 180.0), scl = tan(fov_deg * (kPi / 180.0) * 0.5);
  const double c = cos(az), s = sin(az);
  hipStream_t q = (hipStream_t)stream;
  if (int rc = enqueue_e0(who, pano, B, H, plane, plane_stride, c, s, e0, partial, wp, q)) return rc;
  if (acc) {
    const hipError_t e = hipMemsetAsync(acc, 0, (size_t)3 * B * HW * sizeof(unsigned long long), q);
    if (e != hipSuccess) return eml::fail((int)e > 0 ? (int)e : EML_ELAUNCH, "%s(clear): %s", who, hipGetErrorString(e));
    hipLaunchKernelGGL(abs_kernel, dim3((unsigned)pblk, B), dim3(kThreads), 0, q, g_ratio, g_shadowed, image, (size_t)h * w, a_part);
    if (int rc = eml::check_launch(who, "abs")) return rc;
    hipLaunchKernelGGL(e0_kernel, dim3(B), dim3(kThreads), 0, q, a_part, (int)pblk, gabs);
    if (int rc = eml::check_launch(who, "scale")) return rc;
  }
  hipLaunchKernelGGL(shadow_bwd_kernel, dim3((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, B), dim3(kThreads), walk_lds_bytes(H),
                     q, wp, e0, H, plane, plane_stride, occluders, K, h, w, scl, c, s, image, g_ratio, g_shadowed, gabs, acc, s_part,
                     dimage);
  if (int rc = eml::check_launch(who, "pixels")) return rc;
  if (!acc) return EML_OK;
  hipLaunchKernelGGL(e0_kernel, dim3(B), dim3(kThreads), 0, q, s_part, (int)ntiles, ssum);
  if (int rc = eml::check_launch(who, "S")) return rc;
  hipLaunchKernelGGL(dpano_kernel, dim3((unsigned)nblk, B), dim3(kThreads), 0, q, H, plane, plane_stride, c, s, e0, gabs, ssum, acc,
                     dpano);
  return eml::check_launch(who, "dpano");
}
