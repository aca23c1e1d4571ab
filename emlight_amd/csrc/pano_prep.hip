// HDR panorama -> training batch on the device: perspective crop with a folded horizontal rotation
// (reference RegressionNetwork/util.py:147-185 + :102-105), integer-factor area resize (:139-144) and the global
// tonemap (:36-66) of a batch.  The reference is numpy / scipy on the host, one image at a time.
//
// Crop: one thread per crop pixel evaluates the reference's sample position in f64 (tangent-plane grid -> azimuth /
// elevation -> equirect position) once and gathers the four bilinear neighbours for a run of batch images; the
// rotation is not a copy, it is the column index (j - shift) mod W of the gather.
// Resize: one thread per output pixel sums its fy x fx box in f64 in a fixed order (run-to-run exact).
// Tonemap: P = I^(1/gamma), then an exact k-th order statistic per image WITHOUT a sort: positive f32 values order
// as their bit patterns, so three histogram passes (11 + 11 + 9 bits of the 31-bit key) narrow the selected rank to
// one exact value.  Counts are integers (LDS histograms per workgroup, wave-level pre-aggregation of equal bins,
// integer atomics into the per-image histogram), so the result does not depend on the order of arrival.  The
// (k+1)-th statistic is the next occupied bin of the last histogram, or the smallest key above the selected 22-bit
// prefix (an integer atomic min gathered by the last pass).
#include "eml_common.h"

#include <cmath>

namespace {

constexpr double kPi = 3.14159265358979323846;

// numpy.linspace(-s, s, n)[i]: i * step + (-s) with step = 2s / (n - 1), last element exactly s
__device__ __forceinline__ double linspace_sym(int i, int n, double s) {
  if (n <= 1) return -s;
  if (i == n - 1) return s;
  return (double)i * ((s + s) / (double)(n - 1)) + (-s);
}

// int(deg / 360.0 * W) truncated toward zero, reduced to (-W, W); the gather takes column (j - shift) mod W
__device__ __forceinline__ int column_shift(double deg, int W) {
  const double t = trunc(deg / 360.0 * (double)W);
  if (!isfinite(t)) return 0;
  return (int)fmod(t, (double)W);
}
__device__ __forceinline__ int wrap_col(int j, int W) {
  j %= W;
  return j < 0 ? j + W : j;
}

__device__ __forceinline__ double px_value(const float* p) { return (double)*p; }
__device__ __forceinline__ double px_value(const unsigned char* p) { return (double)*p / 255.0; }   // util.py:149-150

// grid (pixel tiles, batch runs): blockIdx.y covers images [y * per, (y + 1) * per); with fov_dev (one field of view
// per sample) per == 1.  A position outside [0, H-1] x [0, W-1] (the reference raises there; the host refuses a
// by-value fov before the launch) writes NaN: nothing is clamped and nothing is read out of bounds.
template <typename T>
__global__ __launch_bounds__(256) void pano_crop_kernel(const T* __restrict__ pano, int B, int H, int W, int h, int w,
                                                        double ratio, double fov_deg, const double* __restrict__ fov_dev,
                                                        double deg, const double* __restrict__ deg_dev, int per,
                                                        float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int b0 = blockIdx.y * per, b1 = min(B, b0 + per);
  const int r = p / w, c = p - r * w;
  const double fov = fov_dev ? fov_dev[b0] : fov_deg;
  const double scl = tan(fov * (kPi / 180.0) / 2.0);
  double sx = linspace_sym(c, w, scl), sy = linspace_sym(r, h, scl / ratio);
  const double rr = sqrt(sy * sy + sx * sx + 1.0);
  sx /= rr;
  sy /= rr;
  const double sz = sqrt(1.0 - sy * sy - sx * sx);
  const double az = atan2(sx, sz), el = asin(sy);
  const double x = (1.0 + az / kPi) / 2.0 * (double)W, y = (1.0 + el / (kPi / 2.0)) / 2.0 * (double)H;
  const bool inside = x >= -1e-9 && x <= (double)(W - 1) + 1e-9 && y >= -1e-9 && y <= (double)(H - 1) + 1e-9;
  const size_t plane = (size_t)h * w;
  if (!inside) {
    for (int b = b0; b < b1; ++b)
      for (int ch = 0; ch < 3; ++ch) out[((size_t)b * 3 + ch) * plane + p] = __builtin_nanf("");
    return;
  }
  // the interpolator's cell: index clipped to [0, n - 2], weight = distance inside the cell
  const int i0 = min(max((int)floor(y), 0), H - 2), j0 = min(max((int)floor(x), 0), W - 2);
  const double yd = y - (double)i0, xd = x - (double)j0;
  const double w00 = (1.0 - yd) * (1.0 - xd), w01 = (1.0 - yd) * xd, w10 = yd * (1.0 - xd), w11 = yd * xd;
  for (int b = b0; b < b1; ++b) {
    const int s = column_shift(deg_dev ? deg_dev[b] : deg, W);
    const int ja = wrap_col(j0 - s, W), jb = wrap_col(j0 + 1 - s, W);
    const T* img = pano + (size_t)b * H * W * 3;
    const T* r0a = img + ((size_t)i0 * W + ja) * 3;
    const T* r0b = img + ((size_t)i0 * W + jb) * 3;
    const T* r1a = r0a + (size_t)W * 3;
    const T* r1b = r0b + (size_t)W * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double v = 0.0;
      v += px_value(r0a + ch) * w00;
      v += px_value(r0b + ch) * w01;
      v += px_value(r1a + ch) * w10;
      v += px_value(r1b + ch) * w11;
      out[((size_t)b * 3 + ch) * plane + p] = (float)v;
    }
  }
}

// out (B, h, w, 3): mean of the fy x fx box of the rotated panorama, f64 sum in row-major box order
__global__ __launch_bounds__(256) void pano_resize_kernel(const float* __restrict__ pano, int H, int W, int h, int w,
                                                          double deg, const double* __restrict__ deg_dev,
                                                          float* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int b = blockIdx.y;
  const int i = p / w, j = p - i * w;
  const int fy = H / h, fx = W / w;
  const int s = column_shift(deg_dev ? deg_dev[b] : deg, W);
  const int jstart = wrap_col(j * fx - s, W);
  const float* img = pano + (size_t)b * H * W * 3;
  double sr = 0.0, sg = 0.0, sb = 0.0;
  for (int dy = 0; dy < fy; ++dy) {
    const float* row = img + (size_t)(i * fy + dy) * W * 3;
    int col = jstart;
    for (int dx = 0; dx < fx; ++dx) {
      const float* px = row + (size_t)col * 3;
      sr += (double)px[0];
      sg += (double)px[1];
      sb += (double)px[2];
      if (++col == W) col = 0;
    }
  }
  const double inv = (double)fy * (double)fx;
  float* o = out + ((size_t)b * h * w + p) * 3;
  o[0] = (float)(sr / inv);
  o[1] = (float)(sg / inv);
  o[2] = (float)(sb / inv);
}

// ------------------------------------------------------------------------------------------------ tonemap
constexpr int kBins0 = 2048, kBins1 = 2048, kBins2 = 512;      // key bits 30..20, 19..9, 8..0
constexpr int kStateWords = 16;
constexpr int kWorkWords = kBins0 + kBins1 + kBins2 + kStateWords;   // per image, 32-bit words
enum { ST_N = 0, ST_KLO, ST_KREM, ST_PREFIX, ST_MINABOVE, ST_EMPTY, ST_GAMMA };
constexpr int kTmThreads = 256, kTmPerThread = 32;              // values per thread and pass

__device__ __forceinline__ unsigned* work_of(unsigned* work, int b) { return work + (size_t)b * kWorkWords; }

// Adds one count per valid lane.  Lanes of a wave that hit the bin of the first pending lane are counted with one
// LDS atomic (two rounds: images with few distinct values, e.g. a dominant exponent bin, collapse to 1-2 atomics per
// wave); what is left goes lane by lane.  Called in wave-uniform control flow only.
__device__ __forceinline__ void hist_add(unsigned* hist, bool valid, unsigned bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(valid);
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    if (!pending) break;
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const unsigned lb = (unsigned)__shfl((int)bin, leader, 64);
    const bool same = valid && bin == lb;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(m));
    valid = valid && !same;
    pending &= ~m;
  }
  if (valid) atomicAdd(&hist[bin], 1u);
}

__device__ __forceinline__ void flush_hist(const unsigned* lds, unsigned* glob, int bins) {
  for (int i = threadIdx.x; i < bins; i += kTmThreads) {
    const unsigned v = lds[i];
    if (v) atomicAdd(&glob[i], v);
  }
}

// LEVEL 0: P = I^e (or I), store P, histogram of key bits 30..20 of the positive values.
// LEVEL 1: histogram of bits 19..9 of the values whose bits 30..20 are the selected prefix.
// LEVEL 2: histogram of bits 8..0 under the selected 22-bit prefix, and the smallest key above that prefix.
template <int LEVEL>
__global__ __launch_bounds__(kTmThreads) void tonemap_hist_kernel(const float* __restrict__ src, float* __restrict__ P,
                                                                  long n, int use_pow, float expo,
                                                                  unsigned* __restrict__ work) {
  constexpr int BINS = LEVEL == 0 ? kBins0 : (LEVEL == 1 ? kBins1 : kBins2);
  __shared__ unsigned hist[BINS];
  __shared__ unsigned wave_min[kTmThreads / 64];
  const int b = blockIdx.y;
  unsigned* wk = work_of(work, b);
  const unsigned* st = wk + kBins0 + kBins1 + kBins2;
  unsigned prefix = 0;
  if (LEVEL > 0) {
    if (st[ST_EMPTY]) return;          // no positive value: nothing to select (block-uniform)
    prefix = st[ST_PREFIX];
  }
  for (int i = threadIdx.x; i < BINS; i += kTmThreads) hist[i] = 0;
  __syncthreads();
  const size_t base = (size_t)b * (size_t)n;
  const long chunk = (long)kTmThreads * kTmPerThread;
  const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  unsigned above = 0xFFFFFFFFu;
  // uniform trip count (hist_add holds wave-wide ballots); the tail is masked
  // 16-byte loads and stores where the image's base allows them (n % 4 == 0 or image 0), else dword ones
  const bool vec = ((base | (size_t)lo) & 3) == 0 && ((((size_t)src) | ((size_t)P)) & 15) == 0;
  for (long off = lo; off < lo + chunk; off += kTmThreads * 4) {
    const long i = off + (long)threadIdx.x * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const bool full = vec && i + 4 <= hi;
    if (full) {
      const float4 t = *reinterpret_cast<const float4*>(src + base + i);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < hi) v[e] = src[base + i + e];
    }
    if (LEVEL == 0) {
      if (use_pow) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = powf(v[e], expo);
      }
      if (full) {
        *reinterpret_cast<float4*>(P + base + i) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < hi) P[base + i + e] = v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned key = __float_as_uint(v[e]);
      const bool pos = i + e < hi && v[e] > 0.f;    // false for NaN; +inf counts, key 0x7f800000
      if (LEVEL == 0) {
        hist_add(hist, pos, key >> 20);
      } else if (LEVEL == 1) {
        hist_add(hist, pos && (key >> 20) == prefix, (key >> 9) & 0x7FFu);
      } else {
        hist_add(hist, pos && (key >> 9) == prefix, key & 0x1FFu);
        if (pos && (key >> 9) > prefix) above = min(above, key);
      }
    }
  }
  __syncthreads();
  flush_hist(hist, wk + (LEVEL == 0 ? 0 : (LEVEL == 1 ? kBins0 : kBins0 + kBins1)), BINS);
  if (LEVEL == 2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above = min(above, (unsigned)__shfl_xor((int)above, o, 64));
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = above;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned m = wave_min[0];
      for (int k = 1; k < kTmThreads / 64; ++k) m = min(m, wave_min[k]);
      if (m != 0xFFFFFFFFu) atomicMin(&wk[kBins0 + kBins1 + kBins2 + ST_MINABOVE], m);
    }
  }
}

// Bin of `hist` (global, `bins` counts) that holds rank k: hist[0..bin) sums to `before` <= k < before + hist[bin]; `total`
// is the sum of all counts.  All 256 threads call; the result is valid in thread 0.  `part` is 256 words of LDS.
__device__ __forceinline__ void find_bin(const unsigned* __restrict__ hist, int bins, unsigned k, unsigned* part,
                                         unsigned& bin, unsigned& before, unsigned& total) {
  const int per = bins / 256;
  unsigned s = 0;
  for (int i = 0; i < per; ++i) s += hist[threadIdx.x * per + i];
  part[threadIdx.x] = s;
  __syncthreads();
  bin = before = total = 0;
  if (threadIdx.x == 0) {
    unsigned cum = 0;
    int g = 0;
    for (; g < 256; ++g) {
      if (cum + part[g] > k) break;
      cum += part[g];
    }
    unsigned t = cum;
    for (int q = g; q < 256; ++q) t += part[q];
    total = t;
    if (g == 256) {                    // k >= total: cannot happen for k < n; stay in bounds
      bin = bins - 1;
      before = cum;
    } else {
      int i = g * per;
      for (; i < g * per + per - 1; ++i) {
        if (cum + hist[i] > k) break;
        cum += hist[i];
      }
      bin = (unsigned)i;
      before = cum;
    }
  }
  __syncthreads();
}

// LEVEL 0: n, the virtual index, the first prefix.  LEVEL 1: the 22-bit prefix.
// LEVEL 2: both order statistics, r, alpha; writes the per-image raw outputs.
// numpy (2.x) forms the percentile of an f32 array in f32 throughout: q32 = f32(q) / f32(100), the virtual index
// f32(n - 1) * q32, its floor and fraction t, and lerp = t >= .5 ? hi - (hi - lo) * (1 - t) : lo + (hi - lo) * t; a
// virtual index >= n - 1 takes the maximum.  Restated here operation by operation (no contraction), so r is numpy's.
template <int LEVEL>
__global__ __launch_bounds__(256) void tonemap_scan_kernel(unsigned* __restrict__ work, float q32, float max_mapping,
                                                           const float* __restrict__ alpha_in, int* __restrict__ n_out,
                                                           float* __restrict__ stats) {
  __shared__ unsigned part[256];
  const int b = blockIdx.x;
  unsigned* wk = work_of(work, b);
  unsigned* st = wk + kBins0 + kBins1 + kBins2;
  unsigned bin, before, total;
  if (LEVEL == 0) {
    find_bin(wk, kBins0, 0xFFFFFFFFu, part, bin, before, total);   // total only
    unsigned n = 0, klo = 0;
    float gamma = 0.f;
    if (threadIdx.x == 0) {
      n = total;
      st[ST_N] = n;
      st[ST_EMPTY] = n == 0 ? 1u : 0u;
      st[ST_MINABOVE] = 0xFFFFFFFFu;
      if (n > 0) {
        const float top = (float)(n - 1), vi = __fmul_rn(top, q32);
        if (vi >= top) {
          klo = n - 1;
        } else {
          const float fl = floorf(fmaxf(vi, 0.f));
          klo = min((unsigned)fl, n - 1);
          gamma = __fsub_rn(vi, fl);
        }
      }
      st[ST_KLO] = klo;
      st[ST_GAMMA] = __float_as_uint(gamma);
      part[0] = klo;
      part[1] = n;
    }
    __syncthreads();
    klo = part[0];
    n = part[1];
    __syncthreads();
    if (n == 0) return;
    find_bin(wk, kBins0, klo, part, bin, before, total);
    if (threadIdx.x == 0) {
      st[ST_PREFIX] = bin;
      st[ST_KREM] = klo - before;
    }
    return;
  }
  const bool empty = st[ST_EMPTY] != 0;
  if (LEVEL == 1) {
    if (empty) return;
    find_bin(wk + kBins0, kBins1, st[ST_KREM], part, bin, before, total);
    if (threadIdx.x == 0) {
      st[ST_PREFIX] = (st[ST_PREFIX] << 11) | bin;
      st[ST_KREM] = st[ST_KREM] - before;
    }
    return;
  }
  float vlo = 0.f, vhi = 0.f, r = 0.f;
  if (!empty) {
    const unsigned* h2 = wk + kBins0 + kBins1;
    find_bin(h2, kBins2, st[ST_KREM], part, bin, before, total);
    if (threadIdx.x == 0) {
      const unsigned n = st[ST_N], klo = st[ST_KLO], krem = st[ST_KREM] - before;
      const unsigned key_lo = (st[ST_PREFIX] << 9) | bin;
      unsigned key_hi = key_lo;
      if (klo + 1 < n && krem + 1 >= h2[bin]) {       // the next rank is a larger value
        unsigned nb = bin + 1;
        while (nb < (unsigned)kBins2 && h2[nb] == 0) ++nb;
        key_hi = nb < (unsigned)kBins2 ? ((st[ST_PREFIX] << 9) | nb) : st[ST_MINABOVE];
        if (key_hi == 0xFFFFFFFFu) key_hi = key_lo;   // cannot happen for klo + 1 < n; stay defined
      }
      vlo = __uint_as_float(key_lo);
      vhi = __uint_as_float(key_hi);
      const float t = __uint_as_float(st[ST_GAMMA]), d = __fsub_rn(vhi, vlo);
      r = t >= 0.5f ? __fsub_rn(vhi, __fmul_rn(d, __fsub_rn(1.f, t))) : __fadd_rn(vlo, __fmul_rn(d, t));
    }
  }
  if (threadIdx.x == 0) {
    n_out[b] = empty ? 0 : (int)st[ST_N];
    float* o = stats + (size_t)b * 4;
    o[0] = vlo;
    o[1] = vhi;
    o[2] = r;
    o[3] = alpha_in ? alpha_in[b] : max_mapping / __fadd_rn(r, 1e-10f);
  }
}

__global__ __launch_bounds__(256) void tonemap_apply_kernel(const float* __restrict__ P, const float* __restrict__ stats,
                                                            long n, int clip, float* __restrict__ out) {
  const int b = blockIdx.y;
  const float alpha = stats[(size_t)b * 4 + 3];
  const size_t base = (size_t)b * (size_t)n;
  const long chunk = (long)kTmThreads * kTmPerThread;
  const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  if (((base | (size_t)lo) & 3) == 0 && ((((size_t)P) | ((size_t)out)) & 15) == 0) {
    for (long i = lo + (long)threadIdx.x * 4; i < hi; i += kTmThreads * 4) {
      if (i + 4 <= hi) {
        float4 v = *reinterpret_cast<const float4*>(P + base + i);
        v.x = __fmul_rn(alpha, v.x);
        v.y = __fmul_rn(alpha, v.y);
        v.z = __fmul_rn(alpha, v.z);
        v.w = __fmul_rn(alpha, v.w);
        if (clip) {
          v.x = fminf(fmaxf(v.x, 0.f), 1.f);
          v.y = fminf(fmaxf(v.y, 0.f), 1.f);
          v.z = fminf(fmaxf(v.z, 0.f), 1.f);
          v.w = fminf(fmaxf(v.w, 0.f), 1.f);
        }
        *reinterpret_cast<float4*>(out + base + i) = v;
      } else {
        for (long k = i; k < hi; ++k) {
          float v = __fmul_rn(alpha, P[base + k]);
          out[base + k] = clip ? fminf(fmaxf(v, 0.f), 1.f) : v;
        }
      }
    }
    return;
  }
  for (long i = lo + threadIdx.x; i < hi; i += kTmThreads) {
    float v = __fmul_rn(alpha, P[base + i]);
    out[base + i] = clip ? fminf(fmaxf(v, 0.f), 1.f) : v;
  }
}

}  // namespace

extern "C" int eml_pano_crop_f32(const void* pano, int is_u8, int B, int H, int W, int h, int w, double ratio,
                                 double fov_deg, const double* fov_dev, double deg, const double* deg_dev, float* out,
                                 eml_stream_t stream) {
  if (!pano || !out) return eml::fail(EML_EINVAL, "eml_pano_crop_f32: null pointer");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_pano_crop_f32: B must be 0..65535 (grid.y)");
  if (H < 2 || W < 2 || h < 1 || w < 1 || (long)H * W > (1l << 29) || (long)h * w > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_pano_crop_f32: bad size (H, W >= 2; h, w >= 1)");
  if (!(ratio > 0.0) || !std::isfinite(ratio)) return eml::fail(EML_EINVAL, "eml_pano_crop_f32: bad aspect ratio");
  if (!fov_dev && !(fov_deg > 0.0 && fov_deg < 180.0))
    return eml::fail(EML_EINVAL, "eml_pano_crop_f32: fov must lie in (0, 180) degrees");
  if (!deg_dev && !std::isfinite(deg)) return eml::fail(EML_EINVAL, "eml_pano_crop_f32: deg is not finite");
  if (B == 0) return EML_OK;
  // a shared field of view: every thread evaluates its position once for a run of `per` images
  const int runs = fov_dev ? B : (B < 8 ? B : 8);
  const int per = (B + runs - 1) / runs;
  const dim3 grid((h * w + 255) / 256, (B + per - 1) / per);
  if (is_u8)
    hipLaunchKernelGGL(pano_crop_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)pano, B, H, W, h, w, ratio, fov_deg, fov_dev, deg, deg_dev, per, out);
  else
    hipLaunchKernelGGL(pano_crop_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)pano, B, H, W, h, w,
                       ratio, fov_deg, fov_dev, deg, deg_dev, per, out);
  return eml::check_launch("eml_pano_crop_f32");
}

extern "C" int eml_pano_resize_area_f32(const float* pano, int B, int H, int W, int h, int w, double deg,
                                        const double* deg_dev, float* out, eml_stream_t stream) {
  if (!pano || !out) return eml::fail(EML_EINVAL, "eml_pano_resize_area_f32: null pointer");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_pano_resize_area_f32: B must be 0..65535 (grid.y)");
  if (H < 1 || W < 1 || h < 1 || w < 1 || (long)H * W > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_pano_resize_area_f32: bad size");
  if (H % h != 0 || W % w != 0) return eml::fail(EML_EINVAL, "eml_pano_resize_area_f32: integer factors only (H %% h, W %% w)");
  if (!deg_dev && !std::isfinite(deg)) return eml::fail(EML_EINVAL, "eml_pano_resize_area_f32: deg is not finite");
  if (B == 0) return EML_OK;
  hipLaunchKernelGGL(pano_resize_kernel, dim3((h * w + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, pano, H, W, h, w,
                     deg, deg_dev, out);
  return eml::check_launch("eml_pano_resize_area_f32");
}

extern "C" size_t eml_tonemap_work_floats(int B) { return B > 0 ? (size_t)B * kWorkWords : 0; }

extern "C" int eml_tonemap_f32(const float* img, int B, long n, int use_gamma, double gamma, double percentile,
                               double max_mapping, const float* alpha_in, int clip, float* P, float* out, int* n_out,
                               float* stats, void* work, eml_stream_t stream) {
  if (!img || !P || !n_out || !stats || !work) return eml::fail(EML_EINVAL, "eml_tonemap_f32: null pointer");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_tonemap_f32: B must be 0..65535 (grid.y)");
  if (n < 1 || n > (1l << 31) - 1) return eml::fail(EML_EINVAL, "eml_tonemap_f32: values per image must be 1..2^31-1");
  if (!(percentile >= 0.0 && percentile <= 100.0)) return eml::fail(EML_EINVAL, "eml_tonemap_f32: percentile outside [0, 100]");
  if (use_gamma && !(gamma > 0.0)) return eml::fail(EML_EINVAL, "eml_tonemap_f32: gamma must be positive");
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  unsigned* wk = (unsigned*)work;
  if (hipMemsetAsync(wk, 0, (size_t)B * kWorkWords * sizeof(unsigned), s) != hipSuccess)
    return eml::fail(EML_ELAUNCH, "eml_tonemap_f32: clearing the histograms failed");
  const long chunk = (long)kTmThreads * kTmPerThread;
  const dim3 grid((unsigned)((n + chunk - 1) / chunk), B), blk(kTmThreads);
  const float expo = use_gamma ? (float)(1.0 / gamma) : 1.f;   // np.power(f32 array, python float) stays f32
  const float q32 = (float)percentile / 100.f;   // np.percentile: q / f32(100) for an f32 array
  hipLaunchKernelGGL(tonemap_hist_kernel<0>, grid, blk, 0, s, img, P, n, use_gamma ? 1 : 0, expo, wk);
  hipLaunchKernelGGL(tonemap_scan_kernel<0>, dim3(B), dim3(256), 0, s, wk, q32, (float)max_mapping, alpha_in, n_out, stats);
  hipLaunchKernelGGL(tonemap_hist_kernel<1>, grid, blk, 0, s, (const float*)P, (float*)nullptr, n, 0, 1.f, wk);
  hipLaunchKernelGGL(tonemap_scan_kernel<1>, dim3(B), dim3(256), 0, s, wk, q32, (float)max_mapping, alpha_in, n_out, stats);
  hipLaunchKernelGGL(tonemap_hist_kernel<2>, grid, blk, 0, s, (const float*)P, (float*)nullptr, n, 0, 1.f, wk);
  hipLaunchKernelGGL(tonemap_scan_kernel<2>, dim3(B), dim3(256), 0, s, wk, q32, (float)max_mapping, alpha_in, n_out, stats);
  if (out) hipLaunchKernelGGL(tonemap_apply_kernel, grid, blk, 0, s, (const float*)P, (const float*)stats, n, clip ? 1 : 0, out);
  return eml::check_launch("eml_tonemap_f32");
}
