// The ground-plane shadow's walk, shared by the forward (ground_shadow.hip) and its adjoint (ground_shadow_bwd.hip): the
// plane's frame, the per-texel weight and the E0 sums, the pixel's ray and hit point, the phase-A hull, the chunked phase-B
// bit building and the add under the bits.  Both directions take the SAME decisions (which texels are tested, which are
// blocked) and end with the same D, bit for bit, because they run this one instruction sequence (DESIGN.md sections 28, 29).
// The adjoint hooks in per chunk, after the forward's add, with the lane's 64-bit word of blocked texels.
#pragma once
#include "eml_common.h"

namespace {
namespace shadow {

constexpr double kPi = 3.14159265358979323846;
constexpr int kThreads = 256, kTile = 16, kMaxK = 16, kMaxH = 1024, kMaxSide = 16384;
constexpr double kPad = 1e-6;          // radians added to every cap: the rounding of asin / atan2 is ten orders below it

// the plane of image b in the panorama's frame: unit normal n, offset d.  false: a zero or non-finite normal, d not > 0
__device__ __forceinline__ bool plane_frame(const float* __restrict__ plane, double c, double s, double* n, double* d) {
  const double nx = plane[0], ny = plane[1], nz = plane[2], dd = plane[3];
  const double len = sqrt(nx * nx + ny * ny + nz * nz);
  if (!(len > 0.0 && len < 1e300) || !(dd > 0.0 && dd < 1e300)) return false;
  // n = nx r + ny u + nz v with r = (-s, c, 0), u = (0, 0, 1), v = (-c, -s, 0)
  n[0] = (nx * -s + nz * -c) / len, n[1] = (nx * c + nz * -s) / len, n[2] = ny / len;
  *d = dd / len;
  return true;
}

// fixed-order tree over the block's 256 values of three channels; the totals land in thread 0's v
__device__ __forceinline__ void block_sum3(double* v, double* red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) red[ch * kThreads + tid] = v[ch];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) red[ch * kThreads + tid] += red[ch * kThreads + tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) v[ch] = red[ch * kThreads];
}

// wgt[t] = max(n . omega_t, 0) dOmega_t of texel t = r W + col, W = 2 H
__device__ __forceinline__ double texel_weight(const double* n, int H, int W, int t) {
  const int r = t / W, col = t - r * W;
  double st, ct, sp, cp;
  sincos((r + 0.5) * kPi / H, &st, &ct);
  sincos((col + 0.5) * 2.0 * kPi / W, &sp, &cp);
  const double nw = n[0] * (st * cp) + n[1] * (st * sp) + n[2] * ct;
  return nw > 0.0 ? nw * (st * (kPi / H) * (2.0 * kPi / W)) : 0.0;
}

// grid (ceil(H W / 256), B)
__global__ __launch_bounds__(kThreads) void weight_kernel(const float* __restrict__ pano, int H, const float* __restrict__ plane,
                                                          int plane_stride, double c, double s, double* __restrict__ wp,
                                                          double* __restrict__ partial) {
  __shared__ double red[3 * kThreads];
  const int W = 2 * H, HW = H * W, b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x;
  double n[3] = {0.0, 0.0, 0.0}, d = 0.0;
  const bool ok = plane_frame(plane + (size_t)b * plane_stride, c, s, n, &d);
  double v[3] = {0.0, 0.0, 0.0};
  if (t < HW) {
    if (ok) {
      const double wgt = texel_weight(n, H, W, t);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) v[ch] = (double)pano[((size_t)b * 3 + ch) * HW + t] * wgt;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) wp[((size_t)b * HW + t) * 3 + ch] = v[ch];
  }
  block_sum3(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) partial[((size_t)b * gridDim.x + blockIdx.x) * 3 + ch] = v[ch];
  }
}

// grid (B): total[b][ch] = the sum of partial[b][0 .. nblk)[ch], fixed order (E0 from the weight kernel's partials; the
// adjoint's sums of |g| and of g (1 - v) from theirs)
__global__ __launch_bounds__(kThreads) void e0_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ e0) {
  __shared__ double red[3 * kThreads];
  const int b = blockIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < nblk; k += kThreads) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] += partial[((size_t)b * nblk + k) * 3 + ch];
  }
  block_sum3(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) e0[b * 3 + ch] = v[ch];
  }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, eml::shfl_xor_d(v, o));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, eml::shfl_xor_d(v, o));
  return v;
}

// the second half of the definition's test (the first, p inside the sphere, is settled per pixel); ox * st and its like are
// invariant along a row and leave the column loop
__device__ __forceinline__ bool blocked(double ox, double oy, double oz, double o2, double r2, double st, double ct, double cp,
                                        double sp) {
  const double s = fma(ox * st, cp, fma(oy * st, sp, oz * ct));
  return s > 0.0 && fma(-s, s, o2) < r2;
}

// what the walk leaves in a lane: its pixel, what became of the pixel's ray, and D = the sum of wp over the blocked texels
struct Pixel {
  int i, j;
  bool ok, in_image, hit, inside;
  double acc[3];
};

// the forward's value of channel ch's ratio before the rounding to f32
__device__ __forceinline__ double ratio_value(const Pixel& p, int ch, double E) {
  double v = 1.0;
  if (!p.ok) v = __builtin_nan("");
  else if (p.hit && E > 0.0) v = p.inside ? 0.0 : fmin(fmax(1.0 - p.acc[ch] / E, 0.0), 1.0);
  return v;
}

// the pixel of this thread: 8 x 8 per wave, the block's four waves as 2 x 2
__device__ __forceinline__ void pixel_of_thread(int* i, int* j) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  *i = blockIdx.y * kTile + (wv >> 1) * 8 + (lane >> 3), *j = blockIdx.x * kTile + (wv & 1) * 8 + (lane & 7);
}

inline size_t walk_lds_bytes(int H) { return (size_t)(6 * H + 4 * kMaxK) * sizeof(double); }

// One thread per pixel, 8 x 8 pixels per wave, 16 x 16 per block; grid (ceil(w / 16), ceil(h / 16), B), called by all 256
// threads.  lds: walk_lds_bytes(H) of dynamic LDS; box: per wave and sphere R0, R1, c0, nc; stage: per wave the terms of the
// chunk being added.  on_chunk(r, cb, ce, bits) runs once per chunk in which some lane of the wave has a blocked texel, after
// the add, wave-uniformly: bit q of a lane's bits is texel (r, cb + q), set only for cb + q < ce.
template <class OnChunk>
__device__ __forceinline__ Pixel walk(const double* __restrict__ wp, int H, const float* __restrict__ plane, int plane_stride,
                                      const float* __restrict__ occluders, int K, int h, int w, double scl, double c, double s,
                                      double* lds, int (*box)[kMaxK][4], double (*stage)[3 * 64],
                                      unsigned long long* __restrict__ counts, OnChunk&& on_chunk) {
  const int W = 2 * H, HW = H * W, b = blockIdx.z, tid = threadIdx.x;
  double* st = lds;
  double* ct = st + H;
  double* cp = ct + H;
  double* sp = cp + W;
  double* sph = sp + W;                                                    // (K, 4): centre in the panorama's frame, radius or 0
  for (int i = tid; i < H; i += kThreads) sincos((i + 0.5) * kPi / H, &st[i], &ct[i]);
  for (int i = tid; i < W; i += kThreads) sincos((i + 0.5) * 2.0 * kPi / W, &sp[i], &cp[i]);
  if (tid < K) {
    const float* o = occluders + ((size_t)b * K + tid) * 4;
    const double x = o[0], y = o[1], z = o[2], r = o[3];
    sph[4 * tid + 0] = x * -s + z * -c, sph[4 * tid + 1] = x * c + z * -s, sph[4 * tid + 2] = y;
    sph[4 * tid + 3] = r > 0.0 ? r : 0.0;                                  // NaN counts as padding; +inf holds every point
  }
  __syncthreads();

  double n[3] = {0.0, 0.0, 0.0}, d = 0.0;
  const bool ok = plane_frame(plane + (size_t)b * plane_stride, c, s, n, &d);
  const int wv = tid >> 6, lane = tid & 63;
  int i, j;
  pixel_of_thread(&i, &j);
  const bool in_image = i < h && j < w;
  // the ray of pixel (i, j): crop_panorama's, in the panorama's frame (gbuffer_lookup.h forms the same one)
  const double sx = scl * (2.0 * j / (double)(w - 1) - 1.0);
  const double sy = (scl * (double)h / (double)w) * (2.0 * i / (double)(h - 1) - 1.0);
  double rx = c + sx * -s, ry = s + sx * c, rz = -sy;
  const double rl = sqrt(rx * rx + ry * ry + rz * rz);
  rx /= rl, ry /= rl, rz /= rl;
  const double nr = n[0] * rx + n[1] * ry + n[2] * rz;
  const bool hit = in_image && ok && nr < 0.0;
  const double tp = hit ? -d / nr : 0.0;
  const double px = tp * rx, py = tp * ry, pz = tp * rz;

  bool inside = false;
  for (int k = 0; k < K; ++k) {
    const double R = sph[4 * k + 3];
    const double ox = sph[4 * k] - px, oy = sph[4 * k + 1] - py, oz = sph[4 * k + 2] - pz;
    inside = inside || (R > 0.0 && ox * ox + oy * oy + oz * oz < R * R);
  }
  const bool live = hit && !inside;
  const double nxy = sqrt(n[0] * n[0] + n[1] * n[1]);

  // Phase A: per sphere, the hull of the wave's 64 caps as rows [R0, R1] and columns [c0, c0 + nc) mod W, kept in LDS
  unsigned amask = 0;                                                      // the spheres some lane of this wave can lose light to
  int RA = H, RB = -1;
  for (int k = 0; k < K; ++k) {
    const double R = sph[4 * k + 3];
    if (!(R > 0.0)) continue;
    const double ox = sph[4 * k] - px, oy = sph[4 * k + 1] - py, oz = sph[4 * k + 2] - pz;
    const double o2 = ox * ox + oy * oy + oz * oz;
    const bool act = live && o2 - o2 == 0.0;                              // a non-finite offset fails every test: no box
    // this lane's cap as rows [rlo, rhi] and the azimuth interval phd +- dph (or all columns)
    int rlo = H, rhi = -1;
    double phd = 0.0, dph = 0.0;
    bool allc = false;
    if (act) {
      const double al = asin(fmin(R / sqrt(o2), 1.0)) + kPad;
      const double thd = atan2(sqrt(ox * ox + oy * oy), oz);
      phd = atan2(oy, ox);
      const double tlo = thd - al, thi = thd + al;
      rlo = max(0, (int)floor(tlo * H / kPi - 0.5));
      rhi = min(H - 1, (int)ceil(thi * H / kPi - 0.5));
      if (tlo <= 0.0 || thi >= kPi) {
        allc = true;                                                       // the cap holds a pole
      } else {
        const double q = sin(al) / sin(thd);                               // sin(dph) of a cap that holds no pole
        if (q >= 1.0 - 1e-9) allc = true;
        else dph = asin(q) + kPad;
      }
    }
    const unsigned long long who = __ballot(act);
    if (who == 0) continue;
    const double phref = __shfl(phd, __builtin_ctzll(who), 64);           // intervals are measured from one lane's azimuth
    double lo = 1e300, hi = -1e300;
    if (act && !allc) {
      double dl = phd - phref;
      dl -= 2.0 * kPi * rint(dl / (2.0 * kPi));
      lo = dl - dph, hi = dl + dph;
    }
    const int R0 = wave_min_i(rlo), R1 = wave_max_i(rhi);
    lo = wave_min_d(lo), hi = wave_max_d(hi);
    int c0 = 0, nc = W;
    if (__ballot(allc) == 0 && hi - lo < 2.0 * kPi * (1.0 - 2.0 / W)) {
      const int cs = (int)floor((phref + lo) * W / (2.0 * kPi) - 0.5), ce = (int)ceil((phref + hi) * W / (2.0 * kPi) - 0.5);
      if (ce - cs + 1 < W) nc = ce - cs + 1, c0 = ((cs % W) + W) % W;
    }
    if (lane == 0) box[wv][k][0] = R0, box[wv][k][1] = R1, box[wv][k][2] = c0, box[wv][k][3] = nc;
    amask |= 1u << k, RA = min(RA, R0), RB = max(RB, R1);
  }
  __syncthreads();
  amask = __builtin_amdgcn_readfirstlane(amask), RA = __builtin_amdgcn_readfirstlane(RA), RB = __builtin_amdgcn_readfirstlane(RB);

  // Phase B: rows ascending, 64 columns at a time: every sphere whose box meets the chunk sets the bits of the texels it
  // blocks (a texel two spheres block is one bit), then the chunk's terms are added under the bits, columns ascending
  double acc[3] = {0.0, 0.0, 0.0};
#ifdef EML_GROUND_SHADOW_COUNTS
  unsigned long long visited = 0;                                          // texel tests this wave walked, over all spheres
#endif
  for (int r = RA; r <= RB; ++r) {
    const double str = st[r], ctr = ct[r];
    if (!(fma(n[2], ctr, nxy * str) > -1e-9)) continue;                    // the whole row is under the horizon: terms are 0
    unsigned rmask = 0;
    for (unsigned m = amask; m; m &= m - 1) {
      const int k = __builtin_ctz(m);
      if (box[wv][k][0] <= r && r <= box[wv][k][1]) rmask |= 1u << k;
    }
    rmask = __builtin_amdgcn_readfirstlane(rmask);
    if (rmask == 0) continue;
    const double* __restrict__ wrow = wp + ((size_t)b * HW + (size_t)r * W) * 3;
    for (int cb = 0; cb < W; cb += 64) {
      const int ce = min(cb + 64, W);
      bool meets = false;                                                  // does any sphere's box of this row reach the chunk?
      for (unsigned m = rmask; m && !meets; m &= m - 1) {
        const int k = __builtin_ctz(m);
        const int c0 = __builtin_amdgcn_readfirstlane(box[wv][k][2]), nc = __builtin_amdgcn_readfirstlane(box[wv][k][3]);
        meets = c0 + nc > W ? (cb < c0 + nc - W || ce > c0) : (cb < c0 + nc && ce > c0);
      }
      if (!meets) continue;
      // the chunk's 3 x 64 terms, one coalesced load that is in flight while the tests run
      double pre[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) pre[q] = 64 * q + lane < 3 * (ce - cb) ? wrow[3 * cb + 64 * q + lane] : 0.0;
      unsigned long long bits = 0;
      int tlo = W, thi = 0;
      for (unsigned m = rmask; m; m &= m - 1) {
        const int k = __builtin_ctz(m);
        const int c0 = __builtin_amdgcn_readfirstlane(box[wv][k][2]), nc = __builtin_amdgcn_readfirstlane(box[wv][k][3]);
        // ascending columns: a hull that wraps the seam is [0, c0 + nc - W) and [c0, W)
        const bool wraps = c0 + nc > W;
        const int l0 = max(cb, wraps ? 0 : c0), h0 = min(ce, wraps ? c0 + nc - W : c0 + nc);
        const int l1 = max(cb, wraps ? c0 : W), h1 = min(ce, W);
        if (l0 >= h0 && l1 >= h1) continue;
        const double R = sph[4 * k + 3];
        const double ox = sph[4 * k] - px, oy = sph[4 * k + 1] - py, oz = sph[4 * k + 2] - pz;
        const double o2 = ox * ox + oy * oy + oz * oz, r2 = R * R;
        const bool act = live && o2 - o2 == 0.0;
#pragma unroll 4
        for (int col = l0; col < h0; ++col)
          bits |= (unsigned long long)(act && blocked(ox, oy, oz, o2, r2, str, ctr, cp[col], sp[col])) << (col - cb);
#pragma unroll 4
        for (int col = l1; col < h1; ++col)
          bits |= (unsigned long long)(act && blocked(ox, oy, oz, o2, r2, str, ctr, cp[col], sp[col])) << (col - cb);
        if (l0 < h0) tlo = min(tlo, l0), thi = max(thi, h0);
        if (l1 < h1) tlo = min(tlo, l1), thi = max(thi, h1);
#ifdef EML_GROUND_SHADOW_COUNTS
        visited += (unsigned)(max(h0 - l0, 0) + max(h1 - l1, 0));
#endif
      }
      if (__ballot(bits != 0) == 0) continue;
      // through the wave's LDS slot to every lane; a wave's LDS operations execute in program order
#pragma unroll
      for (int q = 0; q < 3; ++q) stage[wv][64 * q + lane] = pre[q];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
      for (int col = tlo; col < thi; ++col) {
        const bool on = (bits >> (col - cb)) & 1ull;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += on ? stage[wv][3 * (col - cb) + ch] : 0.0;
      }
      on_chunk(r, cb, ce, bits);
      __builtin_amdgcn_wave_barrier();                                     // the slot is rewritten by the next chunk
    }
  }
#ifdef EML_GROUND_SHADOW_COUNTS
  if (counts && lane == 0)
    counts[((size_t)b * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wv] = visited * 64ull;
#endif
  Pixel p;
  p.i = i, p.j = j, p.ok = ok, p.in_image = in_image, p.hit = hit, p.inside = inside;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) p.acc[ch] = acc[ch];
  return p;
}

inline bool sizes_ok(int B, int H, int h, int w, int K) {
  return B >= 0 && B <= 65535 && H >= 1 && H <= kMaxH && h >= 2 && w >= 2 && h <= kMaxSide && w <= kMaxSide && K >= 0 && K <= kMaxK;
}
inline size_t weight_blocks(int H) { return ((size_t)2 * H * H + kThreads - 1) / kThreads; }
inline size_t tiles(int h, int w) { return (size_t)((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile); }

// launches 1 and 2 of either direction: wp (B, H W, 3), the 256-texel partials (B, weight_blocks(H), 3) and E0 (B, 3), in f64
inline int enqueue_e0(const char* who, const float* pano, int B, int H, const float* plane, int plane_stride, double c, double s,
                      double* e0, double* partial, double* wp, hipStream_t q) {
  const size_t nblk = weight_blocks(H);
  hipLaunchKernelGGL(weight_kernel, dim3((unsigned)nblk, B), dim3(kThreads), 0, q, pano, H, plane, plane_stride, c, s, wp, partial);
  if (int rc = eml::check_launch(who, "weights")) return rc;
  hipLaunchKernelGGL(e0_kernel, dim3(B), dim3(kThreads), 0, q, partial, (int)nblk, e0);
  return eml::check_launch(who, "E0");
}

// what both entry points refuse of the scene and the sizes, under `who`'s name, in eml_ground_shadow_f32's order (each checks
// its own pointers first); EML_OK when acceptable
inline int refuse_geometry(const char* who, const void* work, int B, int H, int W, int plane_stride, const void* occluders, int K,
                           int h, int w, double fov_deg, double view_azimuth_deg) {
  if (K < 0 || K > kMaxK) return eml::fail(EML_EINVAL, "%s: K must be 0..%d occluder spheres, got %d", who, kMaxK, K);
  if (K > 0 && !occluders) return eml::fail(EML_EINVAL, "%s: null occluders with K = %d", who, K);
  if (H < 1 || H > kMaxH || W != 2 * H)
    return eml::fail(EML_EINVAL, "%s: panorama size: 1 <= H <= %d and W == 2H, got %d x %d", who, kMaxH, H, W);
  if (h < 2 || w < 2 || h > kMaxSide || w > kMaxSide)
    return eml::fail(EML_EINVAL, "%s: image size: 2 <= h, w <= %d, got %d x %d", who, kMaxSide, h, w);
  if (!(fov_deg > 0.0 && fov_deg < 180.0) || !(view_azimuth_deg - view_azimuth_deg == 0.0))
    return eml::fail(EML_EINVAL, "%s: fov_deg must be in (0, 180) (the rays of an orthographic camera would need origins) and "
                                 "the azimuth finite", who);
  if (plane_stride != 0 && plane_stride < 4)
    return eml::fail(EML_EINVAL, "%s: plane_stride is 0 (one plane for the batch) or at least 4", who);
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "%s: B must be 0..65535 (grid.z)", who);
  if ((size_t)work % 8 != 0) return eml::fail(EML_EINVAL, "%s: work must be 8-byte aligned", who);
  return EML_OK;
}

}  // namespace shadow
}  // namespace
