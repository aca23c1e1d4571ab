// Object insertion, first half: prefiltered environment maps.  The panorama integrated against cosine and Phong lobes at the
// texel directions of an output grid (the lobes are section 15's two materials, sphere_render.hip, at
// arbitrary directions; tests/insert_oracle.py restates the definition in float64).
//
// out = K . pano with K (2 Ho^2 output directions x H W texels) the lobe weights times the texel's solid angle and pano
// (texels x 3B image planes).  K is never stored (1 GB per lobe at Ho = 64, 128 x 256): a wave owns 32 directions, keeps
// their omega in registers and builds its A fragment of v_mfma_f32_32x32x2_f32 (lane l: direction l & 31, texel
// k + (l >> 5)) from a per-texel table (omega, dOmega) in LDS beside the staged panorama chunk.  Both lobes of a pass take
// the SAME dot product and the same operand read; a pass holds two lobes (2 x 3 column tiles x 16 accumulator registers,
// the budget of sphere_render.hip's integral kernel), more lobes are more passes.  The texels are split over grid.z; the
// partial tiles go to scratch and a second launch adds them in split order (no atomics: run-to-run exact).  The split
// depends on (H, Ho) only and an MFMA adds its k terms in order per output element: an image's maps do not depend on the
// batch.  A lobe's weight is the same instruction sequence in either slot of a pass and beside any partner, and its
// accumulators are its own: its map does not depend on what else was asked for.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"

#include "env_lobes.h"

namespace {

using namespace eml::env;                // the grid tables, lobe() and the limits: shared with env_prefilter_bwd.hip

constexpr int kKC = 64;                 // texels per staged chunk
constexpr int kColsWG = 96;             // image planes per workgroup: three 32-column MFMA tiles
constexpr int kRowsWG = 128;            // directions per workgroup: one 32-row tile per wave
constexpr int kStride = kKC + 1;        // LDS row of one plane's chunk, padded: the 32 lanes of a half hit 32 banks
constexpr int kMaxSplit = 64;
constexpr int kSlots = 512;             // 256 CUs x 2 resident workgroups

struct Plan {
  long T, D;
  int nchunks, per, splits, rowgroups;
};
// the k split is a function of (H, Ho) alone: an image's summation order must not depend on the batch or the lobes
inline Plan make_plan(int H, int Ho) {
  Plan pl;
  pl.T = 2l * H * H;
  pl.D = 2l * Ho * Ho;
  pl.nchunks = (int)((pl.T + kKC - 1) / kKC);
  pl.rowgroups = (int)((pl.D + kRowsWG - 1) / kRowsWG);
  int want = kSlots / pl.rowgroups;                  // one column group's workgroups fit the part at once
  if (want > kMaxSplit) want = kMaxSplit;
  if (want > pl.nchunks) want = pl.nchunks;
  if (want < 1) want = 1;
  pl.per = (pl.nchunks + want - 1) / want;
  pl.splits = (pl.nchunks + pl.per - 1) / pl.per;
  return pl;
}
// grid (rowgroups, column groups of this launch, splits).  part[split][slot 0..1][direction][column].  NCT: the 32-column
// tiles of a workgroup, a compile-time constant -- a guard around an MFMA inside the k loop makes the compiler carry that
// accumulator through VGPRs (16 reads, 16 writes and a drain of the matrix pipe per iteration: measured 1.13 ms against
// the figure in DESIGN 22).  The launcher sends the full groups of 96 columns through NCT = 3 and the rest through its own NCT.
template <int KA, int KB, int NCT>
__global__ __launch_bounds__(kThreads) void prefilter_kernel(const float* __restrict__ pano, const float4* __restrict__ tab,
                                                             const float4* __restrict__ dtab, int D, int T, int N, int col_base,
                                                             int per, int nchunks, float ma, float mb,
                                                             float* __restrict__ part) {
  constexpr int kCols = NCT * 32;
  __shared__ float sp[kCols * kStride];
  __shared__ float4 st[kKC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int d = blockIdx.x * kRowsWG + wave * 32 + r;
  float ox = 0.f, oy = 0.f, oz = 0.f;                                    // a row beyond D is never stored
  if (d < D) {
    const float4 q = dtab[d];
    ox = q.x, oy = q.y, oz = q.z;
  }
  const int col0 = col_base + blockIdx.y * kCols;
  const int ncols = N - col0 < kCols ? N - col0 : kCols;                 // > 0 by the grid
  f32x16 acca[NCT], accb[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int e = 0; e < 16; ++e) acca[ct][e] = 0.f, accb[ct][e] = 0.f;

  const int c_begin = blockIdx.z * per;
  const int c_end = c_begin + per < nchunks ? c_begin + per : nchunks;
  constexpr int kLoads = kCols * kKC / kThreads;                         // 8 values per thread, tile and chunk
  float pre[kLoads];
  float4 pre_t;
  // chunk c -> registers; a wave reads 64 consecutive texels of one plane.  A texel beyond T: zero operand, zero dOmega
  auto fetch = [&](int c) {
    const int k0 = c * kKC;
#pragma unroll
    for (int e = 0; e < kLoads; ++e) {
      const int idx = e * kThreads + tid, cl = idx >> 6, k = k0 + (idx & (kKC - 1));
      pre[e] = (cl < ncols && k < T) ? pano[(size_t)(col0 + cl) * (size_t)T + k] : 0.f;
    }
    pre_t = (tid < kKC && k0 + tid < T) ? tab[k0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  if (c_begin < c_end) fetch(c_begin);
  for (int c = c_begin; c < c_end; ++c) {
    __syncthreads();                                                     // the previous chunk has been read
#pragma unroll
    for (int e = 0; e < kLoads; ++e) {
      const int idx = e * kThreads + tid;
      sp[(idx >> 6) * kStride + (idx & (kKC - 1))] = pre[e];
    }
    if (tid < kKC) st[tid] = pre_t;
    __syncthreads();
    if (c + 1 < c_end) fetch(c + 1);                                     // in flight while this chunk is computed
#pragma unroll 2
    for (int kk = 0; kk < kKC; kk += 2) {
      const float4 t = st[kk + half];
      const float x = fmaf(ox, t.x, fmaf(oy, t.y, oz * t.z));            // one dot product for both lobes
      const float wa = lobe_weight<KA>(x, ma, t.w);
      float wb = 0.f;
      if (KB != kNone) wb = lobe_weight<KB>(x, mb, t.w);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {                                 // columns beyond ncols: a zero operand, no store
        const float b = sp[(ct * 32 + r) * kStride + kk + half];
        acca[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, b, acca[ct], 0, 0, 0);
        if (KB != kNone) accb[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb, b, accb[ct], 0, 0, 0);
      }
    }
  }
  // C/D of the 32x32 tile: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  const size_t plane = (size_t)D * (size_t)N;
  float* pd = part + (size_t)blockIdx.z * 2 * plane;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int cl = ct * 32 + r;
    if (cl >= ncols) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = blockIdx.x * kRowsWG + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
      if (row >= D) continue;
      const size_t o = (size_t)row * N + col0 + cl;
      pd[o] = acca[ct][e];
      if (KB != kNone) pd[plane + o] = accb[ct][e];
    }
  }
}

// out[b][lobe][ch][direction] = scale * sum over the splits, in split order.  grid (ceil(D N / 256), 2): y = the pass's slot
__global__ __launch_bounds__(kThreads) void prefilter_reduce_kernel(const float* __restrict__ part, int D, int N, int splits,
                                                                    int L, int lobe_a, int lobe_b, float scale_a,
                                                                    float scale_b, float* __restrict__ out) {
  const int slot = blockIdx.y;
  const int l = slot == 0 ? lobe_a : lobe_b;
  if (l < 0) return;
  const size_t plane = (size_t)D * (size_t)N;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= plane) return;
  const int d = (int)(e / N), col = (int)(e - (size_t)d * N);
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[((size_t)k * 2 + slot) * plane + e];
  const int b = col / 3, ch = col - 3 * b;
  out[(((size_t)b * L + l) * 3 + ch) * (size_t)D + d] = s * (slot == 0 ? scale_a : scale_b);
}

// the full groups of 96 columns in one launch, the remaining 1..95 columns in a second with as many tiles as they need
template <int KA, int KB>
void launch_pass(const Plan& pl, hipStream_t s, const float* pano, const float4* tab, const float4* dtab, int D, int T, int N,
                 float ma, float mb, float* part) {
  const int full = N / kColsWG, rest = N - full * kColsWG;
#define EML_TILES(NCT, groups, base)                                                                                  \
  hipLaunchKernelGGL((prefilter_kernel<KA, KB, NCT>), dim3(pl.rowgroups, groups, pl.splits), dim3(kThreads), 0, s, pano, tab, \
                     dtab, D, T, N, base, pl.per, pl.nchunks, ma, mb, part)
  if (full > 0) EML_TILES(3, full, 0);
  if (rest > 64) EML_TILES(3, 1, full * kColsWG);
  else if (rest > 32) EML_TILES(2, 1, full * kColsWG);
  else if (rest > 0) EML_TILES(1, 1, full * kColsWG);
#undef EML_TILES
}

}  // namespace

extern "C" size_t eml_env_prefilter_work_floats(int B, int H, int W, int Ho, int L) {
  if (!size_ok(B, H, W, Ho, L) || B == 0) return 0;
  const Plan pl = make_plan(H, Ho);
  return 4 * (size_t)pl.T + 4 * (size_t)pl.D + (size_t)pl.splits * 2 * pl.D * 3 * (size_t)B;
}

extern "C" int eml_env_prefilter_f32(const float* pano, int B, int H, int W, int Ho, int L, const double* lobes, float* out,
                                     float* work, eml_stream_t stream) {
  if (!pano || !lobes || !out || !work) return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: null pointer");
  if (W != 2 * H || H < 1) return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: W == 2H required (H >= 1), got %d x %d", H, W);
  if (L < 1 || L > kMaxL) return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: 1 <= L <= %d lobes, got %d", kMaxL, L);
  if (!size_ok(B, H, W, Ho, L))
    return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: grid limits: 0 <= B <= %d, H <= %d, 1 <= Ho <= %d", kMaxB, kMaxH,
                     kMaxHo);
  double lb[kMaxL];
  for (int l = 0; l < L; ++l) {
    lb[l] = lobes[l];
    if (!(lb[l] == lb[l]) || !(lb[l] <= 1e6))
      return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: lobe %d: a negative value (diffuse) or a Phong exponent in [0, 1e6]", l);
  }
  if (((size_t)work) & 15) return eml::fail(EML_EINVAL, "eml_env_prefilter_f32: work must be 16-byte aligned");
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const Plan pl = make_plan(H, Ho);
  const int D = (int)pl.D, T = (int)pl.T, N = 3 * B;
  float4* tab = reinterpret_cast<float4*>(work);
  float4* dtab = tab + T;
  float* part = work + 4 * (size_t)T + 4 * (size_t)D;
  hipLaunchKernelGGL(grid_table_kernel, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
  hipLaunchKernelGGL(grid_table_kernel, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, Ho, dtab);
  int rc = eml::check_launch("eml_env_prefilter_f32(tables)");
  if (rc) return rc;
  const size_t plane = (size_t)D * N;
  const dim3 rgrid((unsigned)((plane + kThreads - 1) / kThreads), 2);
  for (int l0 = 0; l0 < L; l0 += 2) {
    const bool two = l0 + 1 < L;
    const int ka = kind_of(lb[l0]), kb = two ? kind_of(lb[l0 + 1]) : kNone;
    const float ma = (float)lb[l0], mb = two ? (float)lb[l0 + 1] : 0.f;
#define EML_PASS(A, Bk) launch_pass<A, Bk>(pl, s, pano, (const float4*)tab, (const float4*)dtab, D, T, N, ma, mb, part)
    if (ka == kDiffuse && kb == kNone) EML_PASS(kDiffuse, kNone);
    else if (ka == kDiffuse && kb == kDiffuse) EML_PASS(kDiffuse, kDiffuse);
    else if (ka == kDiffuse) EML_PASS(kDiffuse, kPhong);
    else if (kb == kNone) EML_PASS(kPhong, kNone);
    else if (kb == kDiffuse) EML_PASS(kPhong, kDiffuse);
    else EML_PASS(kPhong, kPhong);
#undef EML_PASS
    rc = eml::check_launch("eml_env_prefilter_f32(integral)");
    if (rc) return rc;
    // the next pass overwrites `part`: stream order puts it behind this reduction
    hipLaunchKernelGGL(prefilter_reduce_kernel, rgrid, dim3(kThreads), 0, s, (const float*)part, D, N, pl.splits, L, l0,
                       two ? l0 + 1 : -1, (float)scale_of(lb[l0]), two ? (float)scale_of(lb[l0 + 1]) : 0.f, out);
  }
  return eml::check_launch("eml_env_prefilter_f32");
}
