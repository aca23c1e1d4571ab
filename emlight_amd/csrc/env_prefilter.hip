// Object insertion, first half: prefiltered environment maps.  The panorama integrated against cosine and Phong lobes at the
// texel directions of an output grid (the lobes are section 15's two materials, sphere_render.hip, at
// arbitrary directions; tests/insert_oracle.py restates the definition in float64).
//
// out = K . pano with K (2 Ho^2 output directions x H W texels) the lobe weights times the texel's solid angle and pano
// (texels x 3B image planes), on the implicit GEMM of sphere_gemm.h: rows = directions (a wave keeps its 32 omega in
// registers), reduction = texels (table entry: omega, dOmega), split.  Both lobes of a pass take the SAME dot product and
// the same operand read; a pass holds two lobes (2 x 3 column tiles x 16 accumulator registers), more lobes are more
// passes.  A lobe's weight is the same instruction sequence in either slot of a pass and beside any partner, and its
// accumulators are its own: its map does not depend on what else was asked for.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"

#include "env_lobes.h"

namespace {

using namespace eml::env;                // lobe() and the limits: shared with env_prefilter_bwd.hip
using namespace eml::sgemm;

// grid (rowgroups, column groups of this launch, splits).  part[split][slot 0..1][direction][column].  NCT: the 32-column
// tiles of a workgroup, a compile-time constant and no guard in the k loop (measured 1.13 ms with one against the figure in
// DESIGN 22).  The launcher sends the full groups of 96 columns through NCT = 3 and the rest through its own NCT.
template <int KA, int KB, int NCT>
__global__ __launch_bounds__(kThreads) void prefilter_kernel(const float* __restrict__ pano, const float4* __restrict__ tab,
                                                             const float4* __restrict__ dtab, int D, int T, int N, int col_base,
                                                             int per, int nchunks, float ma, float mb,
                                                             float* __restrict__ part) {
  constexpr int kCols = NCT * 32, kLobes = KB != kNone ? 2 : 1;
  __shared__ float sp[kCols * kStride];
  __shared__ float4 st[kKC];
  const Lanes ln = lanes();
  const int tid = ln.tid;
  float ox = 0.f, oy = 0.f, oz = 0.f;                                    // a row beyond D is never stored
  if (ln.row < D) {
    const float4 q = dtab[ln.row];
    ox = q.x, oy = q.y, oz = q.z;
  }
  const int col0 = col_base + blockIdx.y * kCols;
  const int ncols = N - col0 < kCols ? N - col0 : kCols;                 // > 0 by the grid
  f32x16 acc[kLobes][NCT];
#pragma unroll
  for (int i = 0; i < kLobes; ++i) zero(acc[i]);

  const ChunkRange cr = split_chunks(per, nchunks);
  float pre[kCols * kKC / kThreads];
  float4 pre_t;
  // a wave reads 64 consecutive texels of one plane.  A texel beyond T: zero operand, zero dOmega
  auto fetch = [&](int step) {
    const int k0 = (cr.begin + step) * kKC;
    for_each_load<NCT>(tid, [&](int e, int cl, int k) {
      pre[e] = (cl < ncols && k0 + k < T) ? pano[(size_t)(col0 + cl) * (size_t)T + k0 + k] : 0.f;
    });
    pre_t = (tid < kKC && k0 + tid < T) ? tab[k0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage = [&]() {
    stage_plane<NCT>(sp, pre, tid);
    if (tid < kKC) st[tid] = pre_t;
  };
  auto weight = [&](int k, float (&w)[kLobes]) {
    const float4 t = st[k];
    const float x = fmaf(ox, t.x, fmaf(oy, t.y, oz * t.z));              // one dot product for both lobes
    w[0] = lobe_weight<KA>(x, ma, t.w);
    if constexpr (kLobes == 2) w[1] = lobe_weight<KB>(x, mb, t.w);
  };
  pipeline(cr.end - cr.begin, fetch, stage,
           [&]() { chunk_mac<NCT, kLobes, true, false, true>(sp, ncols, ln, weight, acc); });

  const size_t plane = (size_t)D * (size_t)N;
  float* pd = part + (size_t)blockIdx.z * 2 * plane;
  for_each_c<NCT>(ln, [&](int ct, int e, int i, int j) {
    const int row = ln.row0 + i, cl = ct * 32 + j;
    if (cl >= ncols || row >= D) return;
    const size_t o = (size_t)row * N + col0 + cl;
#pragma unroll
    for (int l = 0; l < kLobes; ++l) pd[l * plane + o] = acc[l][ct][e];
  });
}

// out[b][lobe][ch][direction] = scale * the sum over the splits; slot = the pass's slot
struct StoreMaps {
  int D, L, lobe_a, lobe_b;
  float scale_a, scale_b;
  float* out;
  __device__ void operator()(int d, int col, int slot, float s) const {
    const int b = col / 3, ch = col - 3 * b;
    out[(((size_t)b * L + (slot == 0 ? lobe_a : lobe_b)) * 3 + ch) * (size_t)D + d] = s * (slot == 0 ? scale_a : scale_b);
  }
};

// the full groups of 96 columns in one launch, the remaining 1..95 columns in a second with as many tiles as they need
template <int KA, int KB>
void launch_pass(const SplitPlan& pl, hipStream_t s, const float* pano, const float4* tab, const float4* dtab, int D, int T, int N,
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
  const size_t T = 2 * (size_t)H * H, D = 2 * (size_t)Ho * Ho;
  return 4 * T + 4 * D + (size_t)make_split_plan(D, T).splits * 2 * D * 3 * (size_t)B;
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
  const int D = 2 * Ho * Ho, T = 2 * H * H, N = 3 * B;
  const SplitPlan pl = make_split_plan(D, T);               // of (H, Ho) alone: not of the batch, not of the lobes
  float4* tab = reinterpret_cast<float4*>(work);
  float4* dtab = tab + T;
  float* part = work + 4 * (size_t)T + 4 * (size_t)D;
  hipLaunchKernelGGL(grid_table_kernel<>, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
  hipLaunchKernelGGL(grid_table_kernel<>, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, Ho, dtab);
  int rc = eml::check_launch("eml_env_prefilter_f32(tables)");
  if (rc) return rc;
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
    launch_split_reduce(s, part, D, N, pl.splits, 2, 0, two ? 2 : 1,
                        StoreMaps{D, L, l0, l0 + 1, (float)scale_of(lb[l0]), two ? (float)scale_of(lb[l0 + 1]) : 0.f, out});
  }
  return eml::check_launch("eml_env_prefilter_f32");
}
