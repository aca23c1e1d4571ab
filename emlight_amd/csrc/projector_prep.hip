// Projector inputs from a panorama on the device (reference GenProjector/data.py:58-108, numpy / cv2 on the host, one
// sample at a time): the real panorama times the crop's tonemap alpha and the light mask of its luma (:73-84), and the
// bilinear resize of the tonemapped crop (:70).
//
// Targets: the input is pixel-major (R, G, B interleaved), the outputs are planes.  A workgroup stages a tile of 1024 pixels
// (3072 floats) in LDS with 16-byte loads that are contiguous across the wave, then every thread takes four pixels from LDS
// and writes 16 bytes per plane.  The light threshold needs the image's maximum luma first: launch 1 leaves one partial
// maximum per (image, slice), launch 2 re-reduces the image's partials (at most 64, one wave) and writes.  A maximum does
// not depend on the order of its operands and the luma is formed by the same function in both launches, so the result is
// run-to-run exact without atomics.
// Resize: one thread per four output columns of a row of one plane; positions in f64, weights in f32, 16-byte stores.
// The gathers' addresses depend on the scale, so they stay dword loads.
#include "eml_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTilePix = 4 * kThreads;      // pixels per staged tile
constexpr int kTileFloats = 3 * kTilePix;
constexpr int kMaxSlices = 64;              // partial maxima per image: one wave re-reduces them

// (f32(.3) R + f32(.59) G) + f32(.11) B, every operation rounded to f32 (data.py:75); hipcc would contract a * b + c
__device__ __forceinline__ float luma_f32(float r, float g, float b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.3f, r), __fmul_rn(0.59f, g)), __fmul_rn(0.11f, b));
}

__host__ __device__ __forceinline__ int tiles_of(long n) { return (int)((n + kTilePix - 1) / kTilePix); }
__host__ __device__ __forceinline__ int slices_of(long n) {
  const int t = tiles_of(n);
  return t < kMaxSlices ? t : kMaxSlices;
}

// Pixels [p0, p0 + kTilePix) of an image of n pixels -> tile (interleaved, as in memory).  img: the image's first float.
// vec: img + 3 p0 is 16-byte aligned (p0 is a multiple of kTilePix, so that is a property of the image's base).
__device__ __forceinline__ void stage_tile(const float* __restrict__ img, long p0, long n, bool vec, float* tile) {
  const long rest = n - p0;
  const int nfl = 3 * (int)(rest < kTilePix ? rest : kTilePix);
  const float* src = img + 3 * p0;
  if (vec) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = (k * kThreads + threadIdx.x) * 4;
      if (i + 4 <= nfl) {
        *reinterpret_cast<float4*>(tile + i) = *reinterpret_cast<const float4*>(src + i);
      } else {
        for (int e = i; e < nfl; ++e) tile[e] = src[e];      // at most three floats of the image's last tile
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const int i = k * kThreads + threadIdx.x;
      if (i < nfl) tile[i] = src[i];
    }
  }
}

// grid (slices, B): slice s takes tiles s, s + slices, ...; work[b * slices + s] = max luma of those tiles
__global__ __launch_bounds__(kThreads) void targets_max_kernel(const float* __restrict__ small, long n, int slices,
                                                               float* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  __shared__ float wave_part[kThreads / 64];
  const int b = blockIdx.y;
  const float* img = small + (size_t)b * 3 * (size_t)n;
  const bool vec = (((size_t)img) & 15) == 0;
  const int tiles = tiles_of(n);
  float m = -INFINITY;
  for (int t = blockIdx.x; t < tiles; t += slices) {
    const long p0 = (long)t * kTilePix;
    stage_tile(img, p0, n, vec, tile);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = j * kThreads + threadIdx.x;              // stride 3 floats across the wave: no bank conflict
      if (p0 + q < n) m = fmaxf(m, luma_f32(tile[3 * q], tile[3 * q + 1], tile[3 * q + 2]));
    }
    __syncthreads();
  }
  m = eml::wave_max(m);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / 64; ++k) m = fmaxf(m, wave_part[k]);
    work[(size_t)b * slices + blockIdx.x] = m;
  }
}

// grid (tiles, B): threshold from the image's partial maxima, then warped and map of one tile
__global__ __launch_bounds__(kThreads) void targets_write_kernel(const float* __restrict__ small,
                                                                 const float* __restrict__ alpha, long n, int slices,
                                                                 const float* __restrict__ work, float* __restrict__ warped,
                                                                 float* __restrict__ map) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  const int b = blockIdx.y;
  const float* img = small + (size_t)b * 3 * (size_t)n;
  const long p0 = (long)blockIdx.x * kTilePix;
  stage_tile(img, p0, n, (((size_t)img) & 15) == 0, tile);
  const int lane = threadIdx.x & 63;
  const float mx = eml::wave_max(lane < slices ? work[(size_t)b * slices + lane] : -INFINITY);   // every wave: the same value
  const float thr = __fmul_rn(mx, 0.05f);
  const float a = alpha ? alpha[b] : 1.f;
  float* wr = warped + (size_t)b * 3 * (size_t)n;
  float* mp = map + (size_t)b * (size_t)n;
  __syncthreads();
  // 16-byte stores when every plane's base allows them: n % 4 == 0 and aligned buffers
  if ((n & 3) == 0 && ((((size_t)warped) | ((size_t)map)) & 15) == 0) {
    const long p = p0 + 4 * (long)threadIdx.x;
    if (p >= n) return;                                      // n % 4 == 0: a thread's four pixels are inside or outside together
    const float* px = tile + 12 * threadIdx.x;
    float v[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(px + 4 * k);
      v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
    }
    float o[4][4];                                           // R, G, B planes and the mask
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float r = v[3 * j], g = v[3 * j + 1], bl = v[3 * j + 2];
      o[0][j] = alpha ? __fmul_rn(r, a) : r;
      o[1][j] = alpha ? __fmul_rn(g, a) : g;
      o[2][j] = alpha ? __fmul_rn(bl, a) : bl;
      o[3][j] = luma_f32(r, g, bl) > thr ? 1.f : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(wr + (size_t)c * (size_t)n + p) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    *reinterpret_cast<float4*>(mp + p) = make_float4(o[3][0], o[3][1], o[3][2], o[3][3]);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = j * kThreads + threadIdx.x;
    const long p = p0 + q;
    if (p >= n) continue;
    const float r = tile[3 * q], g = tile[3 * q + 1], bl = tile[3 * q + 2];
    wr[p] = alpha ? __fmul_rn(r, a) : r;
    wr[(size_t)n + p] = alpha ? __fmul_rn(g, a) : g;
    wr[2 * (size_t)n + p] = alpha ? __fmul_rn(bl, a) : bl;
    mp[p] = luma_f32(r, g, bl) > thr ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ bilinear resize
// cv2 INTER_LINEAR / F.interpolate(align_corners=False): position (d + .5) * scale - .5 in f64; i0, i1 in [0, n_in - 1]
__device__ __forceinline__ void source_cell(int d, double scale, int n_in, int& i0, int& i1, float& wgt) {
  const double pos = ((double)d + 0.5) * scale - 0.5;
  if (pos < 0.0) {
    i0 = 0, wgt = 0.f;
  } else {
    const double fl = floor(pos);
    if (fl >= (double)(n_in - 1)) {
      i0 = n_in - 1, wgt = 0.f;
    } else {
      i0 = (int)fl, wgt = (float)(pos - fl);
    }
  }
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
}

__device__ __forceinline__ float tap(const float* __restrict__ p, bool scale, float a, int clip) {
  float v = *p;
  if (scale) v = __fmul_rn(a, v);
  return clip ? fminf(fmaxf(v, 0.f), 1.f) : v;
}

// a (1 - t) + b t, each operation rounded to f32; t == 0 is the tap itself (signed zeros, an infinite neighbour)
__device__ __forceinline__ float lerp_f32(float a, float b, float t) {
  return t == 0.f ? a : __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, t)), __fmul_rn(b, t));
}

// grid (ceil(oh * ceil(ow / 4) / 256), B * C): a thread makes four consecutive columns of one output row
__global__ __launch_bounds__(kThreads) void resize_bilinear_kernel(const float* __restrict__ src,
                                                                   const float* __restrict__ alpha, int clip, int C, int h,
                                                                   int w, int oh, int ow, double sy, double sx,
                                                                   float* __restrict__ out) {
  const int groups = (ow + 3) >> 2;
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)oh * groups) return;
  const int y = (int)(t / groups), x0 = 4 * (int)(t - (long)y * groups);
  const int plane = blockIdx.y;
  const bool scale = alpha != nullptr;
  const float a = scale ? alpha[plane / C] : 1.f;
  const float* img = src + (size_t)plane * (size_t)h * (size_t)w;
  int r0, r1;
  float wy;
  source_cell(y, sy, h, r0, r1, wy);
  const float* row0 = img + (size_t)r0 * w;
  const float* row1 = img + (size_t)r1 * w;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    if (x >= ow) break;
    int c0, c1;
    float wx;
    source_cell(x, sx, w, c0, c1, wx);
    const float top = lerp_f32(tap(row0 + c0, scale, a, clip), tap(row0 + c1, scale, a, clip), wx);
    const float bot = lerp_f32(tap(row1 + c0, scale, a, clip), tap(row1 + c1, scale, a, clip), wx);
    o[j] = lerp_f32(top, bot, wy);
  }
  float* dst = out + ((size_t)plane * oh + y) * (size_t)ow + x0;
  if ((ow & 3) == 0 && (((size_t)out) & 15) == 0) {          // every row then starts on 16 bytes and x0 + 4 <= ow
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < ow) dst[j] = o[j];
  }
}

bool targets_size_ok(int B, int h, int w) {
  return B >= 0 && B <= 65535 && h >= 1 && w >= 1 && (long)h * w <= (1l << 29);
}

}  // namespace

extern "C" size_t eml_projector_targets_work_floats(int B, int h, int w) {
  if (!targets_size_ok(B, h, w)) return 0;
  return (size_t)B * slices_of((long)h * w);
}

extern "C" int eml_projector_targets_f32(const float* small, const float* alpha, int B, int h, int w, float* warped,
                                         float* map, float* work, eml_stream_t stream) {
  if (!small || !warped || !map || !work) return eml::fail(EML_EINVAL, "eml_projector_targets_f32: null pointer");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_projector_targets_f32: B must be 0..65535 (grid.y)");
  if (!targets_size_ok(B, h, w)) return eml::fail(EML_EINVAL, "eml_projector_targets_f32: bad size (h, w >= 1, h * w <= 2^29)");
  if (B == 0) return EML_OK;
  const long n = (long)h * w;
  const int slices = slices_of(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(targets_max_kernel, dim3(slices, B), dim3(kThreads), 0, s, small, n, slices, work);
  hipLaunchKernelGGL(targets_write_kernel, dim3(tiles_of(n), B), dim3(kThreads), 0, s, small, alpha, n, slices,
                     (const float*)work, warped, map);
  return eml::check_launch("eml_projector_targets_f32");
}

extern "C" int eml_resize_bilinear_f32(const float* src, const float* alpha, int clip, int B, int C, int h, int w, int oh,
                                       int ow, float* out, eml_stream_t stream) {
  if (!src || !out) return eml::fail(EML_EINVAL, "eml_resize_bilinear_f32: null pointer");
  if (B < 0 || C < 1 || (long)B * C > 65535)
    return eml::fail(EML_EINVAL, "eml_resize_bilinear_f32: B >= 0, C >= 1 and B * C <= 65535 (grid.y)");
  if (h < 1 || w < 1 || oh < 1 || ow < 1 || (long)h * w > (1l << 29) || (long)oh * ow > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_resize_bilinear_f32: bad size (h, w, oh, ow >= 1, planes of at most 2^29 values)");
  if (B == 0) return EML_OK;
  const long threads = (long)oh * ((ow + 3) / 4);
  const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads), B * C);
  hipLaunchKernelGGL(resize_bilinear_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, src, alpha, clip ? 1 : 0, C, h, w,
                     oh, ow, (double)h / (double)oh, (double)w / (double)ow, out);
  return eml::check_launch("eml_resize_bilinear_f32");
}
