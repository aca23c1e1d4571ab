// Lighting evaluation: three spheres (diffuse, matte silver, mirror) lit by an equirectangular panorama and seen by an
// orthographic camera, and the metrics that compare the renders of a predicted map with those of the true one (RMSE,
// scale-invariant RMSE, RGB angular error).  The reference tree has no such code (the papers describe it); DESIGN.md
// section 15 is the definition, tests/sphere_render_oracle.py restates it in float64.
//
// Diffuse and glossy are integrals over the panorama: render = K . pano with K (inside pixels x texels) the cosine /
// Phong-lobe weights times the texel's solid angle, pano (texels x 3B image planes), on the implicit GEMM of sphere_gemm.h:
// rows = inside pixels (a wave keeps its 32 n and R in registers), reduction = texels (table entry: omega, dOmega), split;
// the same chunk feeds both materials' accumulators.  Mirror is a bilinear gather at the reflection direction, coordinates
// in f64.  Metrics: one workgroup per (image, material), f64 tree reductions in a fixed order (as gt_param.hip), two passes
// so that si-RMSE is a sum of squares of residuals and not a difference of large sums.
//
// The renders are linear in the panorama; their gradient with respect to it (the render loss) is the adjoint: the same
// implicit GEMM with pixels and texels exchanged, plus the mirror's taps sorted by texel (see adjoint_kernel below).
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"

#include "env_lobes.h"

namespace {

using namespace eml::sgemm;
using eml::env::lobe;                   // the select form, shared with the prefilter

constexpr int kRec = 8;                 // floats per pixel record: n, R, linear pixel index, pad
constexpr int kMaxS = 1024, kMaxH = 4096, kMaxB = 4096;

// Row i of the S x S image: the inside pixels X^2 + Y^2 < S^2 (X = 2j + 1 - S, Y = S - 1 - 2i) are j0 .. S - 1 - j0
__host__ __device__ inline bool inside_px(int S, int i, int j) {
  const long long X = 2ll * j + 1 - S, Y = (long long)S - 1 - 2ll * i;
  return X * X + Y * Y < (long long)S * S;
}
__host__ __device__ inline int row_first(int S, int i) {
  const double Y = (double)S - 1.0 - 2.0 * i;
  int j0 = (int)ceil(((double)S - 1.0 - sqrt((double)S * S - Y * Y)) * 0.5);
  if (j0 < 0) j0 = 0;
  if (j0 > (S - 1) / 2) j0 = (S - 1) / 2;           // the centre column is inside for every row (S >= 2)
  while (j0 > 0 && inside_px(S, i, j0 - 1)) --j0;
  while (!inside_px(S, i, j0)) ++j0;
  return j0;
}
inline long inside_count(int S) {
  long P = 0;
  for (int i = 0; i < S; ++i) P += S - 2 * row_first(S, i);
  return P;
}

inline bool size_ok(int B, int H, int W, int S) {
  return B >= 0 && B <= kMaxB && H >= 1 && H <= kMaxH && W == 2 * H && S >= 2 && S <= kMaxS;
}

// ------------------------------------------------------------------------------------------------ tables
// n and R of pixel (i, j) in f64: r = (-s, c, 0), u = (0, 0, 1), v = (-c, -s, 0) with (c, s) = (cos, sin) of the azimuth
__device__ __forceinline__ void pixel_frame(int S, int i, int j, double c, double s, double* n, double* R) {
  const double px = (double)(2 * j + 1 - S) / (double)S, py = (double)(S - 1 - 2 * i) / (double)S;
  const double nz = sqrt(1.0 - px * px - py * py);
  n[0] = px * -s + nz * -c;
  n[1] = px * c + nz * -s;
  n[2] = py;
  R[0] = 2.0 * nz * n[0] + c;
  R[1] = 2.0 * nz * n[1] + s;
  R[2] = 2.0 * nz * n[2];
}

// one workgroup: the compact list of inside pixels in row-major order
__global__ __launch_bounds__(kThreads) void pixel_list_kernel(int S, double c, double s, float* __restrict__ rec) {
  __shared__ int start[kMaxS + 1];
  __shared__ int first[kMaxS];
  for (int i = threadIdx.x; i < S; i += kThreads) first[i] = row_first(S, i);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < S; ++i) {
      start[i] = acc;
      acc += S - 2 * first[i];
    }
    start[S] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S; i += kThreads) {
    const int j0 = first[i], cnt = S - 2 * j0;
    for (int q = 0; q < cnt; ++q) {
      double n[3], R[3];
      pixel_frame(S, i, j0 + q, c, s, n, R);
      float* o = rec + (size_t)(start[i] + q) * kRec;
      o[0] = (float)n[0], o[1] = (float)n[1], o[2] = (float)n[2];
      o[3] = (float)R[0], o[4] = (float)R[1], o[5] = (float)R[2];
      o[6] = __int_as_float(i * S + j0 + q);
      o[7] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------ integrals
// grid (rowgroups, colgroups, splits).  part[split][material 0..1][pixel][column].  Three column tiles under the guard
template <bool DIFF, bool GLOSS>
__global__ __launch_bounds__(kThreads) void integral_kernel(const float* __restrict__ pano, const float4* __restrict__ tab,
                                                            const float* __restrict__ rec, int P, int T, int N, int per,
                                                            int nchunks, float m, float* __restrict__ part) {
  constexpr int kMats = (int)DIFF + (int)GLOSS;
  __shared__ float sp[kColsWG * kStride];
  __shared__ float4 st[kKC];
  const Lanes ln = lanes();
  const int tid = ln.tid;
  float nx = 0.f, ny = 0.f, nz = 0.f, Rx = 0.f, Ry = 0.f, Rz = 0.f;      // a row beyond P weighs 0 and is never stored
  if (ln.row < P) {
    const float* q = rec + (size_t)ln.row * kRec;
    nx = q[0], ny = q[1], nz = q[2], Rx = q[3], Ry = q[4], Rz = q[5];
  }
  const int col0 = blockIdx.y * kColsWG;
  const int ncols = N - col0 < kColsWG ? N - col0 : kColsWG;             // > 0 by the grid
  f32x16 acc[kMats][3];                                                  // diffuse first
#pragma unroll
  for (int i = 0; i < kMats; ++i) zero(acc[i]);

  const ChunkRange cr = split_chunks(per, nchunks);
  float pre[kColsWG * kKC / kThreads];
  float4 pre_t;
  // a wave reads 64 consecutive texels of one plane
  auto fetch = [&](int step) {
    const int k0 = (cr.begin + step) * kKC;
    for_each_load<3>(tid, [&](int e, int cl, int k) {
      pre[e] = (cl < ncols && k0 + k < T) ? pano[(size_t)(col0 + cl) * (size_t)T + k0 + k] : 0.f;
    });
    pre_t = (tid < kKC && k0 + tid < T) ? tab[k0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage = [&]() {
    stage_plane<3>(sp, pre, tid);
    if (tid < kKC) st[tid] = pre_t;
  };
  auto weight = [&](int k, float (&w)[kMats]) {
    const float4 t = st[k];
    if (DIFF) w[0] = fmaxf(fmaf(nx, t.x, fmaf(ny, t.y, nz * t.z)), 0.f) * t.w;
    if (GLOSS) w[kMats - 1] = lobe(fmaf(Rx, t.x, fmaf(Ry, t.y, Rz * t.z)), m) * t.w;
  };
  pipeline(cr.end - cr.begin, fetch, stage, [&]() { chunk_mac<3, kMats, true, true, true>(sp, ncols, ln, weight, acc); });

  const size_t plane = (size_t)P * (size_t)N;
  float* pd = part + (size_t)blockIdx.z * 2 * plane;
  for_each_c<3>(ln, [&](int ct, int e, int i, int j) {
    const int row = ln.row0 + i, cl = ct * 32 + j;
    if (cl >= ncols || row >= P) return;
    const size_t o = (size_t)row * N + col0 + cl;
    if (DIFF) pd[o] = acc[0][ct][e];
    if (GLOSS) pd[plane + o] = acc[kMats - 1][ct][e];
  });
}

// out[b][slot][ch][pixel] = scale * the sum over the splits; mat 0: diffuse, 1: glossy
struct StoreRender {
  const float* rec;
  int S, M, slot_d, slot_g;
  float scale_d, scale_g;
  float* out;
  __device__ void operator()(int p, int col, int mat, float s) const {
    const int pix = __float_as_int(rec[(size_t)p * kRec + 6]);
    const int b = col / 3, ch = col - 3 * b;
    out[(((size_t)b * M + (mat == 0 ? slot_d : slot_g)) * 3 + ch) * (size_t)S * S + pix] = s * (mat == 0 ? scale_d : scale_g);
  }
};

// ------------------------------------------------------------------------------------------------ mirror
__device__ __forceinline__ float lerp_f32(float a, float b, float t) {
  return t == 0.f ? a : __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, t)), __fmul_rn(b, t));
}

// where pixel (i, j)'s reflection direction lands on the H x W grid: rows r0, r1 (clamped), columns c0, c1 (wrapped) and
// the fractions rounded to f32; coordinates in f64.  The forward's lookup and the adjoint's tap list both start here.
struct MirrorCoords {
  int r0, r1, c0, c1;
  float wx, wy;
};
__device__ __forceinline__ MirrorCoords mirror_coords(int S, int i, int j, int H, int W, double c, double s) {
  double n[3], R[3];
  pixel_frame(S, i, j, c, s, n, R);
  const double th = atan2(sqrt(R[0] * R[0] + R[1] * R[1]), R[2]);
  double ph = atan2(R[1], R[0]);
  if (ph < 0.0) ph += 2.0 * kPi;
  double v = th * (double)H / kPi - 0.5, u = ph * (double)W / (2.0 * kPi) - 0.5;
  v = v < 0.0 ? 0.0 : (v > (double)(H - 1) ? (double)(H - 1) : v);       // rows clamp
  const double fv = floor(v), fu = floor(u);
  MirrorCoords m;
  m.r0 = (int)fv, m.r1 = m.r0 + 1 < H ? m.r0 + 1 : H - 1;
  m.c0 = (((int)fu % W) + W) % W, m.c1 = (m.c0 + 1) % W;                 // columns wrap
  m.wy = (float)(v - fv), m.wx = (float)(u - fu);
  return m;
}

// grid (ceil(P / 256), B): a thread looks the panorama up at its pixel's reflection direction, three channels
__global__ __launch_bounds__(kThreads) void mirror_kernel(const float* __restrict__ pano, const float* __restrict__ rec, int P,
                                                          int H, int W, int S, int M, int slot, double c, double s,
                                                          float* __restrict__ out) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int b = blockIdx.y;
  const int pix = __float_as_int(rec[(size_t)p * kRec + 6]);
  const MirrorCoords q = mirror_coords(S, pix / S, pix % S, H, W, c, s);
  const int r0 = q.r0, r1 = q.r1, c0 = q.c0, c1 = q.c1;
  const float wx = q.wx, wy = q.wy;
  const size_t T = (size_t)H * W;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* img = pano + ((size_t)b * 3 + ch) * T;
    const float top = lerp_f32(img[(size_t)r0 * W + c0], img[(size_t)r0 * W + c1], wx);
    const float bot = lerp_f32(img[(size_t)r1 * W + c0], img[(size_t)r1 * W + c1], wx);
    out[(((size_t)b * M + slot) * 3 + ch) * (size_t)S * S + pix] = lerp_f32(top, bot, wy);
  }
}

// one workgroup (as pixel_list_kernel): the four taps of every inside pixel, row-major order
__global__ __launch_bounds__(kThreads) void mirror_taps_kernel(int H, int W, int S, double c, double s, int* __restrict__ idx,
                                                               float* __restrict__ wgt) {
  __shared__ int start[kMaxS + 1];
  __shared__ int first[kMaxS];
  for (int i = threadIdx.x; i < S; i += kThreads) first[i] = row_first(S, i);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < S; ++i) {
      start[i] = acc;
      acc += S - 2 * first[i];
    }
    start[S] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S; i += kThreads) {
    const int j0 = first[i], cnt = S - 2 * j0;
    for (int q = 0; q < cnt; ++q) {
      const MirrorCoords m = mirror_coords(S, i, j0 + q, H, W, c, s);
      const float ux = __fsub_rn(1.f, m.wx), uy = __fsub_rn(1.f, m.wy);
      const size_t o = (size_t)(start[i] + q) * 4;
      idx[o + 0] = m.r0 * W + m.c0, wgt[o + 0] = __fmul_rn(ux, uy);
      idx[o + 1] = m.r0 * W + m.c1, wgt[o + 1] = __fmul_rn(m.wx, uy);
      idx[o + 2] = m.r1 * W + m.c0, wgt[o + 2] = __fmul_rn(ux, m.wy);
      idx[o + 3] = m.r1 * W + m.c1, wgt[o + 3] = __fmul_rn(m.wx, m.wy);
    }
  }
}

// ------------------------------------------------------------------------------------------------ adjoint
// dpano = K^T . grad ("Render loss"): the implicit GEMM with the roles exchanged.  A workgroup owns
// 128 texels (32 per wave) x 96 columns (3B image planes) and reduces over ALL inside pixels in chunks of 64 -- no split, so
// the order of the sum is the pixel list's whatever the batch.  A wave keeps its 32 texels' omega in registers with each
// material's normalisation folded into dOmega; a chunk's pixel records and the gathered gradient operand sit in LDS.
// v_mfma_f32_32x32x2_f32 with the gradient as A (lane l: column l & 31, pixel k + (l >> 5)) and the weight as B (texel
// l & 31, same pixel): the C tile's lane & 31 is the texel, so a store row is 32 consecutive floats of one image plane.
// Both materials go into ONE accumulator set.  The mirror's taps on a texel (CSR, sorted by texel) are added in CSR order
// after the integrals by the lane that holds the texel.  grid (ceil(T / 128), colgroups)
// This kernel keeps its own chunk loop beside sphere_gemm.h's: written through the shared pipeline and multiply-accumulate it
// lost the register allocation of the tap loop below (205 -> 176 VGPRs, the 48 tap addresses recomputed per tap) and the
// backward with taps went 0.78 -> 0.90 ms.
template <bool DIFF, bool GLOSS>
__global__ __launch_bounds__(kThreads) void adjoint_kernel(const float* __restrict__ g, const float4* __restrict__ tab,
                                                           const float* __restrict__ rec, int P, int T, int N, int SS, int M,
                                                           int slot_d, int slot_g, int slot_m, float m, float scale_d,
                                                           float scale_g, const int* __restrict__ csr_ptr,
                                                           const int* __restrict__ csr_src, const float* __restrict__ csr_w,
                                                           float* __restrict__ dpano) {
  constexpr int kMats = (int)DIFF + (int)GLOSS;
  constexpr int kPlane = kColsWG * kStride;                              // one material's staged operand: [column][pixel]
  __shared__ float sg[(kMats ? kMats : 1) * kPlane];
  __shared__ float4 s0[kKC], s1[kKC];                                    // the chunk's records: (n, Rx), (Ry, Rz, pixel, -)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int t = blockIdx.x * kRowsWG + wave * 32 + r;
  float ox = 0.f, oy = 0.f, oz = 0.f, dd = 0.f, dg = 0.f;                // a texel beyond T weighs 0 and is never stored
  if (t < T) {
    const float4 q = tab[t];
    ox = q.x, oy = q.y, oz = q.z, dd = q.w * scale_d, dg = q.w * scale_g;
  }
  const int col0 = blockIdx.y * kColsWG;
  const int ncols = N - col0 < kColsWG ? N - col0 : kColsWG;             // > 0 by the grid
  f32x16 acc[3];
#pragma unroll
  for (int ct = 0; ct < 3; ++ct)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;

  if constexpr (kMats > 0) {
    const int nchunks = (P + kKC - 1) / kKC;
    constexpr int kLoads = kColsWG * kKC / kThreads;                     // 24 values per thread, material and chunk
    const size_t off_a = (size_t)(DIFF ? slot_d : slot_g) * 3 * (size_t)SS;
    const size_t off_b = (size_t)slot_g * 3 * (size_t)SS;                // used when both are on
    float pre_a[kLoads], pre_b[kMats == 2 ? kLoads : 1];
    float4 pre0, pre1;
    // chunk c -> registers.  A thread's loads are all of ONE pixel (256 is a multiple of 64): a wave reads the 64 pixels
    // of a chunk, consecutive in the image but for the row ends, in one column and material
    auto fetch = [&](int c) {
      const int p = c * kKC + (tid & (kKC - 1));
      const bool live = p < P;
      float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;              // a pixel beyond P: zero gradient, zero frame
      if (live) {
        const float4* q = reinterpret_cast<const float4*>(rec + (size_t)p * kRec);
        q0 = q[0], q1 = q[1];
      }
      const int pix = __float_as_int(q1.z);
#pragma unroll
      for (int e = 0; e < kLoads; ++e) {
        const int cl = e * (kThreads / kKC) + (tid >> 6);
        float va = 0.f, vb = 0.f;
        if (live && cl < ncols) {
          const int col = col0 + cl, b = col / 3, ch = col - 3 * b;
          const size_t o = ((size_t)b * M * 3 + ch) * (size_t)SS + pix;
          va = g[o + off_a];
          if constexpr (kMats == 2) vb = g[o + off_b];
        }
        pre_a[e] = va;
        if constexpr (kMats == 2) pre_b[e] = vb;
      }
      pre0 = q0, pre1 = q1;
    };
    fetch(0);                                                            // P >= 4: at least one chunk
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();                                                   // the previous chunk has been read
#pragma unroll
      for (int e = 0; e < kLoads; ++e) {
        const int o = (e * (kThreads / kKC) + (tid >> 6)) * kStride + (tid & (kKC - 1));
        sg[o] = pre_a[e];
        if constexpr (kMats == 2) sg[kPlane + o] = pre_b[e];
      }
      if (tid < kKC) s0[tid] = pre0, s1[tid] = pre1;
      __syncthreads();
      if (c + 1 < nchunks) fetch(c + 1);                                 // in flight while this chunk is computed
#pragma unroll 2
      for (int kk = 0; kk < kKC; kk += 2) {
        const float4 q0 = s0[kk + half], q1 = s1[kk + half];
        float wd = 0.f, wg = 0.f;
        if (DIFF) wd = fmaxf(fmaf(q0.x, ox, fmaf(q0.y, oy, q0.z * oz)), 0.f) * dd;
        if (GLOSS) wg = lobe(fmaf(q0.w, ox, fmaf(q1.x, oy, q1.y * oz)), m) * dg;
        if (DIFF) {
#pragma unroll
          for (int ct = 0; ct < 3; ++ct)
            if (ct * 32 < ncols)                                         // wave-uniform
              acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(sg[(ct * 32 + r) * kStride + kk + half], wd, acc[ct], 0, 0, 0);
        }
        if (GLOSS) {
#pragma unroll
          for (int ct = 0; ct < 3; ++ct)
            if (ct * 32 < ncols)
              acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(sg[(kMats - 1) * kPlane + (ct * 32 + r) * kStride + kk + half],
                                                             wg, acc[ct], 0, 0, 0);
        }
      }
    }
  }
  if (t >= T) return;
  // C/D of the 32x32 tile: column (texel) = lane & 31, row (image plane) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  if (csr_ptr) {
    const int ntaps = 4 * P;
    int q0 = csr_ptr[t], q1 = csr_ptr[t + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > ntaps) q1 = ntaps;
    const size_t off_m = (size_t)slot_m * 3 * (size_t)SS;
    for (int q = q0; q < q1; ++q) {
      const int src = csr_src[q];
      if ((unsigned)src >= (unsigned)SS) continue;                       // a malformed table reads nothing out of bounds
      const float w = csr_w[q];
#pragma unroll
      for (int ct = 0; ct < 3; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int cl = ct * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
          if (cl >= ncols) continue;
          const int col = col0 + cl, b = col / 3, ch = col - 3 * b;
          acc[ct][e] = fmaf(w, g[((size_t)b * M * 3 + ch) * (size_t)SS + off_m + src], acc[ct][e]);
        }
    }
  }
#pragma unroll
  for (int ct = 0; ct < 3; ++ct)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int cl = ct * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
      if (cl < ncols) dpano[(size_t)(col0 + cl) * (size_t)T + t] = acc[ct][e];
    }
}

// ------------------------------------------------------------------------------------------------ metrics
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kThreads >> 1; s > 0; s >>= 1) {      // fixed-order tree: deterministic
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// grid (M, B): out[b][m] = rmse, si_rmse, angular (degrees), used
__global__ __launch_bounds__(kThreads) void metrics_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                           int M, int S, double* __restrict__ out) {
  __shared__ double red[kThreads];
  const size_t SS = (size_t)S * S;
  const size_t base = ((size_t)blockIdx.y * M + blockIdx.x) * 3 * SS;
  const float* a = pred + base;
  const float* b = truth + base;
  double d2 = 0.0, ab = 0.0, aa = 0.0, ang = 0.0, used = 0.0, cnt = 0.0;
  for (int q = threadIdx.x; q < (int)SS; q += kThreads) {
    if (!inside_px(S, q / S, q % S)) continue;
    const double a0 = a[q], a1 = a[SS + q], a2 = a[2 * SS + q], b0 = b[q], b1 = b[SS + q], b2 = b[2 * SS + q];
    d2 += ((a0 - b0) * (a0 - b0) + (a1 - b1) * (a1 - b1)) + (a2 - b2) * (a2 - b2);
    const double dot = (a0 * b0 + a1 * b1) + a2 * b2;
    ab += dot;
    const double na = (a0 * a0 + a1 * a1) + a2 * a2, nb = (b0 * b0 + b1 * b1) + b2 * b2;
    aa += na;
    cnt += 1.0;
    if (sqrt(na) * sqrt(nb) != 0.0) {
      const double cx = a1 * b2 - a2 * b1, cy = a2 * b0 - a0 * b2, cz = a0 * b1 - a1 * b0;
      ang += atan2(sqrt((cx * cx + cy * cy) + cz * cz), dot);
      used += 1.0;
    }
  }
  d2 = block_sum(d2, red);
  ab = block_sum(ab, red);
  aa = block_sum(aa, red);
  ang = block_sum(ang, red);
  used = block_sum(used, red);
  cnt = block_sum(cnt, red);
  const double sc = aa == 0.0 ? 0.0 : ab / aa;
  double r2 = 0.0;
  for (int q = threadIdx.x; q < (int)SS; q += kThreads) {
    if (!inside_px(S, q / S, q % S)) continue;
    const double e0 = sc * (double)a[q] - (double)b[q], e1 = sc * (double)a[SS + q] - (double)b[SS + q],
                 e2 = sc * (double)a[2 * SS + q] - (double)b[2 * SS + q];
    r2 += (e0 * e0 + e1 * e1) + e2 * e2;
  }
  r2 = block_sum(r2, red);
  if (threadIdx.x == 0) {
    double* o = out + ((size_t)blockIdx.y * M + blockIdx.x) * 4;
    o[0] = sqrt(d2 / (3.0 * cnt));
    o[1] = sqrt(r2 / (3.0 * cnt));
    o[2] = used == 0.0 ? 0.0 : ang / used * (180.0 / kPi);
    o[3] = used;
  }
}

template <bool DIFF, bool GLOSS>
void launch_integral(dim3 grid, hipStream_t s, const float* pano, const float4* tab, const float* rec, int P, int T, int N,
                     int per, int nchunks, float m, float* part) {
  hipLaunchKernelGGL((integral_kernel<DIFF, GLOSS>), grid, dim3(kThreads), 0, s, pano, tab, rec, P, T, N, per, nchunks, m,
                     part);
}

}  // namespace

extern "C" size_t eml_sphere_render_work_floats(int B, int H, int W, int S) {
  if (!size_ok(B, H, W, S) || B == 0) return 0;
  const size_t T = (size_t)H * W, P = inside_count(S);
  return 4 * T + (size_t)kRec * P + (size_t)make_split_plan(P, T).splits * 2 * P * 3 * (size_t)B;
}

extern "C" int eml_sphere_render_f32(const float* pano, int B, int H, int W, int S, double view_azimuth_deg,
                                     int materials_mask, double phong_m, float* out, float* work, eml_stream_t stream) {
  if (!pano || !out || !work) return eml::fail(EML_EINVAL, "eml_sphere_render_f32: null pointer");
  if (W != 2 * H || H < 1) return eml::fail(EML_EINVAL, "eml_sphere_render_f32: W == 2H required (H >= 1), got %d x %d", H, W);
  if (S < 2) return eml::fail(EML_EINVAL, "eml_sphere_render_f32: S must be at least 2, got %d", S);
  if (materials_mask <= 0 || materials_mask > EML_SPHERE_ALL)
    return eml::fail(EML_EINVAL, "eml_sphere_render_f32: materials mask %d is empty or has unknown bits", materials_mask);
  if (!(phong_m >= 0.0) || !(phong_m <= 1e6) || !(view_azimuth_deg == view_azimuth_deg))
    return eml::fail(EML_EINVAL, "eml_sphere_render_f32: phong exponent must be in [0, 1e6] and the azimuth a number");
  if (!size_ok(B, H, W, S))
    return eml::fail(EML_EINVAL, "eml_sphere_render_f32: grid limits: 0 <= B <= %d, H <= %d, S <= %d", kMaxB, kMaxH, kMaxS);
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const int P = (int)inside_count(S), T = H * W, N = 3 * B;
  const SplitPlan pl = make_split_plan(P, T);               // of (H, W, S) alone: not of the batch
  const bool diff = materials_mask & EML_SPHERE_DIFFUSE, gloss = materials_mask & EML_SPHERE_GLOSSY,
             mirror = materials_mask & EML_SPHERE_MIRROR;
  const int M = (int)diff + (int)gloss + (int)mirror;
  const int slot_d = diff ? 0 : -1, slot_g = gloss ? (int)diff : -1, slot_m = (int)diff + (int)gloss;
  float4* tab = reinterpret_cast<float4*>(work);      // torch allocations are 16-byte aligned; 4 T floats keep rec aligned too
  float* rec = work + 4 * (size_t)T;
  float* part = rec + (size_t)kRec * P;
  if (((size_t)work) & 15) return eml::fail(EML_EINVAL, "eml_sphere_render_f32: work must be 16-byte aligned");
  const double az = view_azimuth_deg * (kPi / 180.0), c = cos(az), sn = sin(az);

  hipError_t e = hipMemsetAsync(out, 0, (size_t)B * M * 3 * (size_t)S * S * sizeof(float), s);   // outside the disc: 0
  if (e != hipSuccess) return eml::fail(EML_ELAUNCH, "eml_sphere_render_f32(zero): %s", hipGetErrorString(e));
  hipLaunchKernelGGL(pixel_list_kernel, dim3(1), dim3(kThreads), 0, s, S, c, sn, rec);
  if (diff || gloss) {
    hipLaunchKernelGGL(grid_table_kernel<>, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
    const dim3 grid(pl.rowgroups, (N + kColsWG - 1) / kColsWG, pl.splits);
    const float m = (float)phong_m;
    if (diff && gloss) launch_integral<true, true>(grid, s, pano, tab, rec, P, T, N, pl.per, pl.nchunks, m, part);
    else if (diff) launch_integral<true, false>(grid, s, pano, tab, rec, P, T, N, pl.per, pl.nchunks, m, part);
    else launch_integral<false, true>(grid, s, pano, tab, rec, P, T, N, pl.per, pl.nchunks, m, part);
    int rc = eml::check_launch("eml_sphere_render_f32(integral)");
    if (rc) return rc;
    launch_split_reduce(s, part, P, N, pl.splits, 2, diff ? 0 : 1, (int)diff + (int)gloss,
                        StoreRender{rec, S, M, slot_d, slot_g, (float)(1.0 / kPi), (float)((phong_m + 1.0) / (2.0 * kPi)), out});
  }
  if (mirror)
    hipLaunchKernelGGL(mirror_kernel, dim3((P + kThreads - 1) / kThreads, B), dim3(kThreads), 0, s, pano, (const float*)rec, P,
                       H, W, S, M, slot_m, c, sn, out);
  return eml::check_launch("eml_sphere_render_f32");
}

// texel table (4 T) and pixel records (8 P): the adjoint is not split, so nothing else
extern "C" size_t eml_sphere_render_bwd_work_floats(int B, int H, int W, int S) {
  if (!size_ok(B, H, W, S) || B == 0) return 0;
  return 4 * (size_t)H * W + (size_t)kRec * inside_count(S);
}

extern "C" int eml_sphere_render_bwd_f32(const float* grad_out, int B, int H, int W, int S, double view_azimuth_deg,
                                         int materials_mask, double phong_m, const int* mirror_csr_ptr,
                                         const int* mirror_csr_src, const float* mirror_csr_w, float* dpano, float* work,
                                         eml_stream_t stream) {
  if (!grad_out || !dpano || !work) return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: null pointer");
  if (W != 2 * H || H < 1)
    return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: W == 2H required (H >= 1), got %d x %d", H, W);
  if (S < 2) return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: S must be at least 2, got %d", S);
  if (materials_mask <= 0 || materials_mask > EML_SPHERE_ALL)
    return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: materials mask %d is empty or has unknown bits", materials_mask);
  const bool diff = materials_mask & EML_SPHERE_DIFFUSE, gloss = materials_mask & EML_SPHERE_GLOSSY,
             mirror = materials_mask & EML_SPHERE_MIRROR;
  if (mirror && (!mirror_csr_ptr || !mirror_csr_src || !mirror_csr_w))
    return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: the mirror bit needs the three mirror_csr pointers");
  if (!(phong_m >= 0.0) || !(phong_m <= 1e6) || !(view_azimuth_deg == view_azimuth_deg))
    return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: phong exponent must be in [0, 1e6] and the azimuth a number");
  if (!size_ok(B, H, W, S))
    return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: grid limits: 0 <= B <= %d, H <= %d, S <= %d", kMaxB, kMaxH, kMaxS);
  if (((size_t)work) & 15) return eml::fail(EML_EINVAL, "eml_sphere_render_bwd_f32: work must be 16-byte aligned");
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const int T = H * W, P = (int)inside_count(S), N = 3 * B;
  const int M = (int)diff + (int)gloss + (int)mirror;
  const int slot_d = 0, slot_g = (int)diff, slot_m = (int)diff + (int)gloss;
  float4* tab = reinterpret_cast<float4*>(work);
  float* rec = work + 4 * (size_t)T;
  const double az = view_azimuth_deg * (kPi / 180.0), c = cos(az), sn = sin(az);
  hipLaunchKernelGGL(pixel_list_kernel, dim3(1), dim3(kThreads), 0, s, S, c, sn, rec);
  hipLaunchKernelGGL(grid_table_kernel<>, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
  int rc = eml::check_launch("eml_sphere_render_bwd_f32(tables)");
  if (rc) return rc;
  const dim3 grid((T + kRowsWG - 1) / kRowsWG, (N + kColsWG - 1) / kColsWG);
  const float m = (float)phong_m, sd = (float)(1.0 / kPi), sg = (float)((phong_m + 1.0) / (2.0 * kPi));
  const int* cp = mirror ? mirror_csr_ptr : nullptr;
#define EML_ADJOINT(D, G)                                                                                                  \
  hipLaunchKernelGGL((adjoint_kernel<D, G>), grid, dim3(kThreads), 0, s, grad_out, (const float4*)tab, (const float*)rec, \
                     P, T, N, S * S, M, slot_d, slot_g, slot_m, m, sd, sg, cp, mirror_csr_src, mirror_csr_w, dpano)
  if (diff && gloss) EML_ADJOINT(true, true);
  else if (diff) EML_ADJOINT(true, false);
  else if (gloss) EML_ADJOINT(false, true);
  else EML_ADJOINT(false, false);
#undef EML_ADJOINT
  return eml::check_launch("eml_sphere_render_bwd_f32");
}

extern "C" int eml_sphere_mirror_taps_f32(int H, int W, int S, double view_azimuth_deg, int* idx, float* wgt,
                                          eml_stream_t stream) {
  if (!idx || !wgt) return eml::fail(EML_EINVAL, "eml_sphere_mirror_taps_f32: null pointer");
  if (W != 2 * H || H < 1)
    return eml::fail(EML_EINVAL, "eml_sphere_mirror_taps_f32: W == 2H required (H >= 1), got %d x %d", H, W);
  if (!(view_azimuth_deg == view_azimuth_deg) || !size_ok(1, H, W, S))
    return eml::fail(EML_EINVAL, "eml_sphere_mirror_taps_f32: grid limits: H <= %d, 2 <= S <= %d, the azimuth a number", kMaxH,
                     kMaxS);
  const double az = view_azimuth_deg * (kPi / 180.0);
  hipLaunchKernelGGL(mirror_taps_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, H, W, S, cos(az), sin(az), idx, wgt);
  return eml::check_launch("eml_sphere_mirror_taps_f32");
}

extern "C" int eml_sphere_render_metrics_f64(const float* pred_render, const float* true_render, int B, int M, int S,
                                             double* out, eml_stream_t stream) {
  if (!pred_render || !true_render || !out) return eml::fail(EML_EINVAL, "eml_sphere_render_metrics_f64: null pointer");
  if (M < 1 || M > 3) return eml::fail(EML_EINVAL, "eml_sphere_render_metrics_f64: M must be 1..3 materials, got %d", M);
  if (S < 2 || S > kMaxS) return eml::fail(EML_EINVAL, "eml_sphere_render_metrics_f64: S must be 2..%d, got %d", kMaxS, S);
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_sphere_render_metrics_f64: B must be 0..65535 (grid.y)");
  if (B == 0) return EML_OK;
  hipLaunchKernelGGL(metrics_kernel, dim3(M, B), dim3(kThreads), 0, (hipStream_t)stream, pred_render, true_render, M, S, out);
  return eml::check_launch("eml_sphere_render_metrics_f64");
}
