// Object insertion: the adjoint of the prefiltered environment maps (env_prefilter.hip; DESIGN.md section 23;
// tests/insert_grad_oracle.py restates the definition in float64).
//
// dpano = dOmega . K^T . grad_out: the forward's implicit GEMM, exchanged.  Rows: the 2 H^2 texels -- a wave owns 32 of
// them and keeps their omega in registers; k: the (lobe, direction) pairs; columns: the 3B planes.  The A fragment of
// v_mfma_f32_32x32x2_f32 (lane l: texel l & 31, direction k + (l >> 5)) is built from the direction table in LDS beside the
// staged chunk of grad_out, with the forward's dot product (direction first) and the forward's lobe().  Unlike the forward,
// every lobe adds into the SAME accumulators (3 column tiles x 16 registers): one pass serves any L.  The lobe loop is
// outside the chunk loop; the diffuse lobes come first and the Phong lobes second, each kind with its own instantiated
// inner loop, so the kind is a wave-uniform choice made once, not per element.  c_l is applied when a chunk is staged to
// LDS, dOmega_t once per row by the reduction.  The directions are split over grid.z; the partial tiles go to scratch and a
// second launch adds them in split order (no atomics: run-to-run exact).  The split depends on (H, Ho) only and an MFMA
// adds its k terms in order per output element: an image's gradient does not depend on the batch.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "env_lobes.h"

namespace {

using namespace eml::env;

constexpr int kKC = 64;                 // directions per staged chunk
constexpr int kColsWG = 96;             // image planes per workgroup: three 32-column MFMA tiles
constexpr int kRowsWG = 128;            // texels per workgroup: one 32-row tile per wave
constexpr int kStride = kKC + 1;        // LDS row of one plane's chunk, padded: the 32 lanes of a half hit 32 banks
constexpr int kMaxSplit = 64;
constexpr int kSlots = 512;             // 256 CUs x 2 resident workgroups

struct Plan {
  long T, D;
  int nchunks, per, splits, rowgroups;
};
// the k split is a function of (H, Ho) alone: an image's summation order must not depend on the batch
inline Plan make_plan(int H, int Ho) {
  Plan pl;
  pl.T = 2l * H * H;
  pl.D = 2l * Ho * Ho;
  pl.nchunks = (int)((pl.D + kKC - 1) / kKC);
  pl.rowgroups = (int)((pl.T + kRowsWG - 1) / kRowsWG);
  int want = kSlots / pl.rowgroups;                  // one column group's workgroups fit the part at once
  if (want > kMaxSplit) want = kMaxSplit;
  if (want > pl.nchunks) want = pl.nchunks;
  if (want < 1) want = 1;
  pl.per = (pl.nchunks + want - 1) / want;
  pl.splits = (pl.nchunks + pl.per - 1) / pl.per;
  return pl;
}

// the lobes in the order they are added: the diffuse ones first, then the Phong ones, each group in the caller's order
struct Lobes {
  int n, n_diffuse;
  int index[kMaxL];                     // the lobe's position in grad_out
  float m[kMaxL], c[kMaxL];
};

// one staged chunk: 64 directions against the wave's 32 texels.  No guard around an MFMA: columns beyond the batch hold zeros
template <int KIND, int NCT>
__device__ __forceinline__ void chunk_mac(const float* __restrict__ sp, const float4* __restrict__ st, float tx, float ty,
                                          float tz, float m, int half, int r, f32x16 (&acc)[NCT]) {
#pragma unroll 2
  for (int kk = 0; kk < kKC; kk += 2) {
    const float4 o = st[kk + half];
    const float x = fmaf(o.x, tx, fmaf(o.y, ty, o.z * tz));              // the forward's dot product: direction first
    const float wa = KIND == kDiffuse ? fmaxf(x, 0.f) : lobe(x, m);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const float b = sp[(ct * 32 + r) * kStride + kk + half];
      acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, b, acc[ct], 0, 0, 0);
    }
  }
}

// grid (rowgroups, column groups of this launch, splits).  part[split][texel][column].  g (B, L, 3, D).  NCT: the 32-column
// tiles of a workgroup, a compile-time constant (env_prefilter.hip has the measurement behind that).
template <int NCT>
__global__ __launch_bounds__(kThreads) void prefilter_bwd_kernel(const float* __restrict__ g, const float4* __restrict__ tab,
                                                                 const float4* __restrict__ dtab, int D, int T, int N,
                                                                 int col_base, int per, int nchunks, Lobes lb,
                                                                 float* __restrict__ part) {
  constexpr int kCols = NCT * 32;
  __shared__ float sp[kCols * kStride];
  __shared__ float4 st[kKC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int t = blockIdx.x * kRowsWG + wave * 32 + r;
  float tx = 0.f, ty = 0.f, tz = 0.f;                                    // a row beyond T is never stored
  if (t < T) {
    const float4 q = tab[t];
    tx = q.x, ty = q.y, tz = q.z;
  }
  const int col0 = col_base + blockIdx.y * kCols;
  const int ncols = N - col0 < kCols ? N - col0 : kCols;                 // > 0 by the grid
  f32x16 acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;

  const int c_begin = blockIdx.z * per;
  const int c_end = c_begin + per < nchunks ? c_begin + per : nchunks;   // > c_begin by the plan
  constexpr int kLoads = kCols * kKC / kThreads;                         // 8 values per thread, tile and chunk
  // this thread's columns: plane col = 3 b + ch of lobe l starts at ((b L + l) 3 + ch) D = (col + 3 b (L - 1) + 3 l) D
  size_t src[kLoads];
#pragma unroll
  for (int e = 0; e < kLoads; ++e) {
    const int cl = (e * kThreads + tid) >> 6, col = col0 + (cl < ncols ? cl : 0);
    src[e] = (size_t)(col + 3 * (col / 3) * (lb.n - 1)) * (size_t)D;
  }
  float pre[kLoads];
  float4 pre_t;
  // chunk c of lobe l -> registers; a wave reads 64 consecutive directions of one plane.  A direction beyond D: zero operand
  auto fetch = [&](int l, int c) {
    const int k0 = c * kKC;
    const size_t lobe_off = (size_t)(3 * l) * (size_t)D;
#pragma unroll
    for (int e = 0; e < kLoads; ++e) {
      const int idx = e * kThreads + tid, cl = idx >> 6, k = k0 + (idx & (kKC - 1));
      pre[e] = (cl < ncols && k < D) ? g[src[e] + lobe_off + k] : 0.f;
    }
    pre_t = (tid < kKC && k0 + tid < D) ? dtab[k0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  // the steps of this workgroup: lobe slot li (diffuse lobes first), chunk c; step + 1 is fetched while step is computed
  const int nc = c_end - c_begin, total = lb.n * nc;
  int li = 0, c = c_begin, step = 0;
  fetch(lb.index[0], c_begin);
  auto stage = [&]() {
    const float cl = lb.c[li];
    __syncthreads();                                                     // the previous chunk has been read
#pragma unroll
    for (int e = 0; e < kLoads; ++e) {
      const int idx = e * kThreads + tid;
      sp[(idx >> 6) * kStride + (idx & (kKC - 1))] = pre[e] * cl;        // c_l here: once per value, not per MFMA operand
    }
    if (tid < kKC) st[tid] = pre_t;
    __syncthreads();
    ++step, ++c;
    if (c == c_end) c = c_begin, ++li;
    if (step < total) fetch(lb.index[li], c);                            // in flight while this chunk is computed
  };
  // two loops, not a choice inside one: the accumulators stay where they are (a branch between two instantiated inner
  // loops per chunk made the compiler move all 48 registers in and out around it)
  const int diffuse_steps = lb.n_diffuse * nc;
  while (step < diffuse_steps) {
    stage();
    chunk_mac<kDiffuse, NCT>(sp, st, tx, ty, tz, 1.f, half, r, acc);
  }
  while (step < total) {
    const float m = lb.m[li];
    stage();
    chunk_mac<kPhong, NCT>(sp, st, tx, ty, tz, m, half, r, acc);
  }
  // C/D of the 32x32 tile: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float* pd = part + (size_t)blockIdx.z * (size_t)T * (size_t)N;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int cl = ct * 32 + r;
    if (cl >= ncols) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = blockIdx.x * kRowsWG + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
      if (row >= T) continue;
      pd[(size_t)row * N + col0 + cl] = acc[ct][e];
    }
  }
}

// dpano[col][texel] = dOmega_t * sum over the splits, in split order
__global__ __launch_bounds__(kThreads) void prefilter_bwd_reduce_kernel(const float* __restrict__ part,
                                                                        const float4* __restrict__ tab, int T, int N,
                                                                        int splits, float* __restrict__ dpano) {
  const size_t plane = (size_t)T * (size_t)N;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= plane) return;
  const int t = (int)(e / N), col = (int)(e - (size_t)t * N);
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[(size_t)k * plane + e];
  dpano[(size_t)col * (size_t)T + t] = s * tab[t].w;
}

}  // namespace

extern "C" size_t eml_env_prefilter_bwd_work_floats(int B, int H, int W, int Ho, int L) {
  if (!size_ok(B, H, W, Ho, L) || B == 0) return 0;
  const Plan pl = make_plan(H, Ho);
  return 4 * (size_t)pl.T + 4 * (size_t)pl.D + (size_t)pl.splits * pl.T * 3 * (size_t)B;
}

extern "C" int eml_env_prefilter_bwd_f32(const float* grad_out, int B, int H, int W, int Ho, int L, const double* lobes,
                                         float* dpano, float* work, eml_stream_t stream) {
  if (!grad_out || !lobes || !dpano || !work) return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: null pointer");
  if (W != 2 * H || H < 1)
    return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: W == 2H required (H >= 1), got %d x %d", H, W);
  if (L < 1 || L > kMaxL) return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: 1 <= L <= %d lobes, got %d", kMaxL, L);
  if (!size_ok(B, H, W, Ho, L))
    return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: grid limits: 0 <= B <= %d, H <= %d, 1 <= Ho <= %d", kMaxB, kMaxH,
                     kMaxHo);
  double lv[kMaxL];
  for (int l = 0; l < L; ++l) {
    lv[l] = lobes[l];
    if (!(lv[l] == lv[l]) || !(lv[l] <= 1e6))
      return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: lobe %d: a negative value (diffuse) or a Phong exponent in [0, 1e6]",
                       l);
  }
  Lobes lb;
  lb.n = 0;
  for (int l = 0; l < kMaxL; ++l) lb.index[l] = 0, lb.m[l] = 0.f, lb.c[l] = 0.f;
  for (int kind : {kDiffuse, kPhong}) {
    for (int l = 0; l < L; ++l)
      if (kind_of(lv[l]) == kind) lb.index[lb.n] = l, lb.m[lb.n] = (float)lv[l], lb.c[lb.n] = (float)scale_of(lv[l]), ++lb.n;
    if (kind == kDiffuse) lb.n_diffuse = lb.n;
  }
  if (((size_t)work) & 15) return eml::fail(EML_EINVAL, "eml_env_prefilter_bwd_f32: work must be 16-byte aligned");
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const Plan pl = make_plan(H, Ho);
  const int D = (int)pl.D, T = (int)pl.T, N = 3 * B;
  float4* tab = reinterpret_cast<float4*>(work);
  float4* dtab = tab + T;
  float* part = work + 4 * (size_t)T + 4 * (size_t)D;
  hipLaunchKernelGGL(grid_table_kernel, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
  hipLaunchKernelGGL(grid_table_kernel, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, Ho, dtab);
  int rc = eml::check_launch("eml_env_prefilter_bwd_f32(tables)");
  if (rc) return rc;
  // the full groups of 96 columns in one launch, the remaining 1..95 columns in a second with as many tiles as they need
  const int full = N / kColsWG, rest = N - full * kColsWG;
#define EML_TILES(NCT, groups, base)                                                                                        \
  hipLaunchKernelGGL((prefilter_bwd_kernel<NCT>), dim3(pl.rowgroups, groups, pl.splits), dim3(kThreads), 0, s, grad_out,    \
                     (const float4*)tab, (const float4*)dtab, D, T, N, base, pl.per, pl.nchunks, lb, part)
  if (full > 0) EML_TILES(3, full, 0);
  if (rest > 64) EML_TILES(3, 1, full * kColsWG);
  else if (rest > 32) EML_TILES(2, 1, full * kColsWG);
  else if (rest > 0) EML_TILES(1, 1, full * kColsWG);
#undef EML_TILES
  rc = eml::check_launch("eml_env_prefilter_bwd_f32(integral)");
  if (rc) return rc;
  const size_t plane = (size_t)T * N;
  hipLaunchKernelGGL(prefilter_bwd_reduce_kernel, dim3((unsigned)((plane + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     (const float*)part, (const float4*)tab, T, N, pl.splits, dpano);
  return eml::check_launch("eml_env_prefilter_bwd_f32");
}
