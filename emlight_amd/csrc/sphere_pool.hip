// SphereMaxPool2D (reference models/networks/spherenet/sphere_cnn.py:127-150):
//     x -> grid_sample(x, fixed tangent-plane grid) -> (B, C, 3H', 3W') -> max_pool2d(3, 3)
// in one pass each way over the tap table of sphere_conv.hip and its CSR transpose: the 9x blown-up tensor never exists and
// the backward is a gather, not grid_sample's atomicAdd scatter.
//
//   forward  : v_t = sum_k wgt[p*9 + t][k] * X[b][idx[p*9 + t][k]][c]  (corner order nw, ne, sw, se as grid_sampler_2d; a
//              corner off the map adds +0);  Y[b][p][c] = max_t v_t,  ARG[b][p][c] = the winning t = a*3 + b
//              max_pool2d's rule: tap t replaces the running maximum when v_t > max or v_t is NaN -- the first maximal tap wins,
//              a NaN wins over every number and the last NaN tap is the one recorded
//   backward : dX[b][q][c] = sum over the entries e of row q of the CSR transpose with ARG[b][src_e / 9][c] == src_e % 9 of
//              w_e * dY[b][src_e / 9][c], in CSR order (no atomics: run-to-run exact); every element of dX is written
//
// Both are HBM-streaming kernels in the thread layout of sphere_conv.hip's gather kernels: TPR (a power of two, at most one
// wave) consecutive threads share one pixel and stride over its channels, 16-byte accesses when C % 4 == 0 (4 index bytes as one
// 32-bit access), a scalar path otherwise; a wave covers 64 / TPR pixels, so C = 1 and C = 3 images fill their waves.  Rows
// (b, pixel) are 32-bit (the launchers refuse B * pixels >= 2^31), element offsets are size_t.
#include <algorithm>

#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"

namespace {

constexpr int kTaps = 9;

__device__ __forceinline__ bool replaces(float v, float best) { return v > best || v != v; }

template <int VEC, int TPR>
__global__ __launch_bounds__(256) void sphere_max_pool_fwd_kernel(const float* __restrict__ X, const int* __restrict__ idx,
                                                                  const float* __restrict__ wgt, float* __restrict__ Y,
                                                                  unsigned char* __restrict__ ARG, unsigned rows,
                                                                  unsigned n_src, unsigned n_dst, int C) {
  constexpr unsigned RPB = 256 / TPR;  // pixels per block per pass
  const int cv = C / VEC;
  const unsigned rl = threadIdx.x / TPR;
  const int cl = threadIdx.x % TPR;
  for (unsigned row = blockIdx.x * RPB + rl; row < rows; row += gridDim.x * RPB) {   // rows < 2^31: no wrap-around
    const unsigned b = row / n_dst, p = row - b * n_dst;
    const float* xb = X + (size_t)b * n_src * C;
    const int* ip = idx + (size_t)p * (kTaps * 4);
    const float* wp = wgt + (size_t)p * (kTaps * 4);
    for (int c = cl; c < cv; c += TPR) {
      if constexpr (VEC == 4) {
        float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned arg = 0;   // one byte per channel, channel 4c in the low byte (the order a little-endian 32-bit store writes)
        // a window row (3 taps, 12 corner loads) per step: the nine taps unrolled kept 36 loads and the pixel's whole table in
        // registers -- 306 of them, one wave per SIMD
#pragma unroll 1
        for (int t3 = 0; t3 < kTaps; t3 += 3) {
#pragma unroll
        for (int t = t3; t < t3 + 3; ++t) {
          const int4 id = *reinterpret_cast<const int4*>(ip + 4 * t);
          const float4 w = *reinterpret_cast<const float4*>(wp + 4 * t);
          const int ids[4] = {id.x, id.y, id.z, id.w};
          const float ws[4] = {w.x, w.y, w.z, w.w};
          // the four corner loads are issued together, a corner off the map at a clamped address (sphere_im2col_kernel);
          // an index past the input is treated like one off the map: nothing is read outside the sample
          float4 v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            v[k] = *reinterpret_cast<const float4*>(xb + (size_t)min((unsigned)max(ids[k], 0), n_src - 1) * C + 4 * c);
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool in = (unsigned)ids[k] < n_src;     // exactly +0 whatever the clamped address holds (0 * Inf would be NaN)
            const float wk = in ? ws[k] : 0.f;
            acc.x += (in ? v[k].x : 0.f) * wk;
            acc.y += (in ? v[k].y : 0.f) * wk;
            acc.z += (in ? v[k].z : 0.f) * wk;
            acc.w += (in ? v[k].w : 0.f) * wk;
          }
          if (t == 0) {
            best = acc;
          } else {
            if (replaces(acc.x, best.x)) { best.x = acc.x; arg = (arg & 0xffffff00u) | (unsigned)t; }
            if (replaces(acc.y, best.y)) { best.y = acc.y; arg = (arg & 0xffff00ffu) | ((unsigned)t << 8); }
            if (replaces(acc.z, best.z)) { best.z = acc.z; arg = (arg & 0xff00ffffu) | ((unsigned)t << 16); }
            if (replaces(acc.w, best.w)) { best.w = acc.w; arg = (arg & 0x00ffffffu) | ((unsigned)t << 24); }
          }
        }
        }
        const size_t o = (size_t)row * C + 4 * c;
        *reinterpret_cast<float4*>(Y + o) = best;
        if (ARG) *reinterpret_cast<unsigned*>(ARG + o) = arg;   // o % 4 == 0
      } else {
        float best = 0.f;
        int arg = 0;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
          float acc = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int id = ip[4 * t + k];
            if ((unsigned)id < n_src) acc += xb[(size_t)id * C + c] * wp[4 * t + k];
          }
          if (t == 0 || replaces(acc, best)) { best = acc; arg = t; }
        }
        const size_t o = (size_t)row * C + c;
        Y[o] = best;
        if (ARG) ARG[o] = (unsigned char)arg;
      }
    }
  }
}

template <int VEC, int TPR>
__global__ __launch_bounds__(256) void sphere_max_pool_bwd_kernel(const float* __restrict__ dY,
                                                                  const unsigned char* __restrict__ ARG,
                                                                  const int* __restrict__ ptr, const int* __restrict__ src,
                                                                  const float* __restrict__ w, float* __restrict__ dX,
                                                                  unsigned rows, unsigned n_src, unsigned n_dst, int C) {
  constexpr unsigned RPB = 256 / TPR;
  const int cv = C / VEC;
  const unsigned rl = threadIdx.x / TPR;
  const int cl = threadIdx.x % TPR;
  for (unsigned row = blockIdx.x * RPB + rl; row < rows; row += gridDim.x * RPB) {
    const unsigned b = row / n_src, q = row - b * n_src;
    const float* gb = dY + (size_t)b * n_dst * C;
    const unsigned char* ab = ARG + (size_t)b * n_dst * C;
    const int k0 = ptr[q], k1 = ptr[q + 1];
    for (int c = cl; c < cv; c += TPR) {
      if constexpr (VEC == 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // two entries per step: their (source, weight) loads first, then the row reads, then the sums in CSR order
        // (sphere_col2im_kernel's scheme; a term that lost its cell's maximum is skipped, not multiplied by 0: 0 * Inf)
        int k = k0;
        for (; k + 2 <= k1; k += 2) {
          const int s0 = src[k], s1 = src[k + 1];
          const float w0 = w[k], w1 = w[k + 1];
          const unsigned p0 = (unsigned)s0 / kTaps, t0 = (unsigned)s0 - p0 * kTaps;
          const unsigned p1 = (unsigned)s1 / kTaps, t1 = (unsigned)s1 - p1 * kTaps;
          // (a source past the output -- a table of another geometry -- matches no tap: read at pixel 0, never added)
          const size_t o0 = (size_t)(p0 < n_dst ? p0 : 0u) * C + 4 * c, o1 = (size_t)(p1 < n_dst ? p1 : 0u) * C + 4 * c;
          const unsigned a0 = p0 < n_dst ? *reinterpret_cast<const unsigned*>(ab + o0) : 0xffffffffu;
          const unsigned a1 = p1 < n_dst ? *reinterpret_cast<const unsigned*>(ab + o1) : 0xffffffffu;
          const float4 g0 = *reinterpret_cast<const float4*>(gb + o0), g1 = *reinterpret_cast<const float4*>(gb + o1);
          if ((a0 & 0xffu) == t0) acc.x = fmaf(w0, g0.x, acc.x);
          if (((a0 >> 8) & 0xffu) == t0) acc.y = fmaf(w0, g0.y, acc.y);
          if (((a0 >> 16) & 0xffu) == t0) acc.z = fmaf(w0, g0.z, acc.z);
          if ((a0 >> 24) == t0) acc.w = fmaf(w0, g0.w, acc.w);
          if ((a1 & 0xffu) == t1) acc.x = fmaf(w1, g1.x, acc.x);
          if (((a1 >> 8) & 0xffu) == t1) acc.y = fmaf(w1, g1.y, acc.y);
          if (((a1 >> 16) & 0xffu) == t1) acc.z = fmaf(w1, g1.z, acc.z);
          if ((a1 >> 24) == t1) acc.w = fmaf(w1, g1.w, acc.w);
        }
        for (; k < k1; ++k) {
          const int s0 = src[k];
          const float w0 = w[k];
          const unsigned p0 = (unsigned)s0 / kTaps, t0 = (unsigned)s0 - p0 * kTaps;
          const size_t o0 = (size_t)(p0 < n_dst ? p0 : 0u) * C + 4 * c;
          const unsigned a0 = p0 < n_dst ? *reinterpret_cast<const unsigned*>(ab + o0) : 0xffffffffu;
          const float4 g0 = *reinterpret_cast<const float4*>(gb + o0);
          if ((a0 & 0xffu) == t0) acc.x = fmaf(w0, g0.x, acc.x);
          if (((a0 >> 8) & 0xffu) == t0) acc.y = fmaf(w0, g0.y, acc.y);
          if (((a0 >> 16) & 0xffu) == t0) acc.z = fmaf(w0, g0.z, acc.z);
          if ((a0 >> 24) == t0) acc.w = fmaf(w0, g0.w, acc.w);
        }
        *reinterpret_cast<float4*>(dX + (size_t)row * C + 4 * c) = acc;   // an empty CSR row: 0
      } else {
        float acc = 0.f;
        for (int k = k0; k < k1; ++k) {
          const int s0 = src[k];
          const unsigned p0 = (unsigned)s0 / kTaps, t0 = (unsigned)s0 - p0 * kTaps;
          const size_t o0 = (size_t)p0 * C + c;
          if (p0 < n_dst && ab[o0] == t0) acc = fmaf(w[k], gb[o0], acc);
        }
        dX[(size_t)row * C + c] = acc;
      }
    }
  }
}

// threads per pixel = the smallest power of two >= C / VEC, at most one wave; a block of 256 threads covers 256 / TPR pixels
#define EML_POOL_CASE(KERNEL, V, T, ...) \
  case T: hipLaunchKernelGGL((KERNEL<V, T>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;
#define EML_POOL_CASES(KERNEL, V, ...)     \
  switch (tpr) {                           \
    EML_POOL_CASE(KERNEL, V, 1, __VA_ARGS__)  \
    EML_POOL_CASE(KERNEL, V, 2, __VA_ARGS__)  \
    EML_POOL_CASE(KERNEL, V, 4, __VA_ARGS__)  \
    EML_POOL_CASE(KERNEL, V, 8, __VA_ARGS__)  \
    EML_POOL_CASE(KERNEL, V, 16, __VA_ARGS__) \
    EML_POOL_CASE(KERNEL, V, 32, __VA_ARGS__) \
    EML_POOL_CASE(KERNEL, V, 64, __VA_ARGS__) \
  }
#define EML_POOL_LAUNCH(KERNEL, rows, ...)                                                          \
  do {                                                                                             \
    const int cv = (C % 4 == 0) ? C / 4 : C;                                                       \
    int tpr = 1;                                                                                   \
    while (tpr < cv && tpr < 64) tpr <<= 1;                                                        \
    const size_t rpb = 256 / tpr;                                                                  \
    const dim3 grid((unsigned)std::min<size_t>(((size_t)(rows) + rpb - 1) / rpb, (size_t)16384)); \
    if (C % 4 == 0) {                                                                              \
      EML_POOL_CASES(KERNEL, 4, __VA_ARGS__)                                                       \
    } else {                                                                                       \
      EML_POOL_CASES(KERNEL, 1, __VA_ARGS__)                                                       \
    }                                                                                              \
  } while (0)

// shared argument checks: sizes, and rows = B * pixels of either side below 2^31
int pool_sizes_ok(const char* what, int B, int n_src, int n_dst, int C) {
  if (B < 0 || C < 1 || n_src < 1 || n_dst < 1)
    return eml::fail(EML_EINVAL, "%s: bad size (B >= 0; C, n_src, n_dst >= 1)", what);
  const size_t lim = (size_t)1 << 31;
  if ((size_t)B * (size_t)n_src >= lim || (size_t)B * (size_t)n_dst >= lim || (size_t)n_dst * kTaps >= lim)
    return eml::fail(EML_EINVAL, "%s: B * n_src, B * n_dst and 9 * n_dst must be below 2^31", what);
  return EML_OK;
}

}  // namespace

extern "C" int eml_sphere_max_pool_fwd_f32(const float* x, const int* idx, const float* wgt, float* y, unsigned char* arg, int B,
                                           int n_src, int n_dst, int C, eml_stream_t stream) {
  if (!x || !idx || !wgt || !y) return eml::fail(EML_EINVAL, "eml_sphere_max_pool_fwd_f32: null pointer");
  if (const int rc = pool_sizes_ok("eml_sphere_max_pool_fwd_f32", B, n_src, n_dst, C)) return rc;
  if (B == 0) return EML_OK;
  const unsigned rows = (unsigned)B * (unsigned)n_dst;
  EML_POOL_LAUNCH(sphere_max_pool_fwd_kernel, rows, x, idx, wgt, y, arg, rows, (unsigned)n_src, (unsigned)n_dst, C);
  return eml::check_launch("eml_sphere_max_pool_fwd_f32");
}

extern "C" int eml_sphere_max_pool_bwd_f32(const float* gy, const unsigned char* arg, const int* csr_ptr, const int* csr_src,
                                           const float* csr_w, float* gx, int B, int n_src, int n_dst, int C,
                                           eml_stream_t stream) {
  if (!gy || !arg || !csr_ptr || !csr_src || !csr_w || !gx)
    return eml::fail(EML_EINVAL, "eml_sphere_max_pool_bwd_f32: null pointer");
  if (const int rc = pool_sizes_ok("eml_sphere_max_pool_bwd_f32", B, n_src, n_dst, C)) return rc;
  if (B == 0) return EML_OK;
  const unsigned rows = (unsigned)B * (unsigned)n_src;
  EML_POOL_LAUNCH(sphere_max_pool_bwd_kernel, rows, gy, arg, csr_ptr, csr_src, csr_w, gx, rows, (unsigned)n_src, (unsigned)n_dst,
                  C);
  return eml::check_launch("eml_sphere_max_pool_bwd_f32");
}
