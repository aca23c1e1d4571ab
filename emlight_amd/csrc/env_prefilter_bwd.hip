// Object insertion: the adjoint of the prefiltered environment maps (env_prefilter.hip; DESIGN.md section 23;
// tests/insert_grad_oracle.py restates the definition in float64).
//
// dpano = dOmega . K^T . grad_out: the forward's implicit GEMM (sphere_gemm.h), exchanged.  Rows: the 2 H^2 texels -- a wave
// keeps its 32 omega in registers; reduction: the (lobe, direction) pairs, the directions split; columns: the 3B planes.
// The weight is made with the forward's dot product (direction first) and the forward's lobe().  Unlike the forward, every
// lobe adds into the SAME accumulators (3 column tiles x 16 registers): one pass serves any L.  The lobe loop is outside
// the chunk loop; the diffuse lobes come first and the Phong lobes second, each kind with its own instantiated inner loop,
// so the kind is a wave-uniform choice made once, not per element.  c_l is applied when a chunk is staged to LDS, dOmega_t
// once per row by the reduction.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include <type_traits>

#include "env_lobes.h"

namespace {

using namespace eml::env;
using namespace eml::sgemm;

// the lobes in the order they are added: the diffuse ones first, then the Phong ones, each group in the caller's order
struct Lobes {
  int n, n_diffuse;
  int index[kMaxL];                     // the lobe's position in grad_out
  float m[kMaxL], c[kMaxL];
};

// grid (rowgroups, column groups of this launch, splits).  part[split][texel][column].  g (B, L, 3, D).  NCT: the 32-column
// tiles of a workgroup, a compile-time constant and no guard in the k loop (env_prefilter.hip has the measurement behind
// that): columns beyond the batch hold zeros.
template <int NCT>
__global__ __launch_bounds__(kThreads) void prefilter_bwd_kernel(const float* __restrict__ g, const float4* __restrict__ tab,
                                                                 const float4* __restrict__ dtab, int D, int T, int N,
                                                                 int col_base, int per, int nchunks, Lobes lb,
                                                                 float* __restrict__ part) {
  constexpr int kCols = NCT * 32, kLoads = kCols * kKC / kThreads;
  __shared__ float sp[kCols * kStride];
  __shared__ float4 st[kKC];
  const Lanes ln = lanes();
  const int tid = ln.tid;
  float tx = 0.f, ty = 0.f, tz = 0.f;                                    // a row beyond T is never stored
  if (ln.row < T) {
    const float4 q = tab[ln.row];
    tx = q.x, ty = q.y, tz = q.z;
  }
  const int col0 = col_base + blockIdx.y * kCols;
  const int ncols = N - col0 < kCols ? N - col0 : kCols;                 // > 0 by the grid
  f32x16 acc[1][NCT];
  zero(acc[0]);

  const ChunkRange cr = split_chunks(per, nchunks);                      // end > begin by the plan
  // this thread's columns: plane col = 3 b + ch of lobe l starts at ((b L + l) 3 + ch) D = (col + 3 b (L - 1) + 3 l) D
  size_t src[kLoads];
  for_each_load<NCT>(tid, [&](int e, int cl, int) {
    const int col = col0 + (cl < ncols ? cl : 0);
    src[e] = (size_t)(col + 3 * (col / 3) * (lb.n - 1)) * (size_t)D;
  });
  float pre[kLoads];
  float4 pre_t;
  // The steps of this workgroup: lobe slot li (diffuse lobes first), chunk c.  (li, c) is a running cursor, not a function of
  // the step number (no division per chunk): stage() reads c_l and m of the step it stages and THEN moves the cursor to the
  // step that pipeline() fetches next, so fetch() takes the cursor as it finds it -- the call order is pipeline()'s contract.
  // A wave reads 64 consecutive directions of one plane; a direction beyond D: zero operand
  const int nc = cr.end - cr.begin, total = lb.n * nc, diffuse_steps = lb.n_diffuse * nc;
  int li = 0, c = cr.begin;
  float m_staged = 0.f;                                                  // the exponent of the step in LDS
  auto fetch = [&](int) {
    const int k0 = c * kKC;
    const size_t lobe_off = (size_t)(3 * lb.index[li]) * (size_t)D;
    for_each_load<NCT>(tid, [&](int e, int cl, int k) {
      pre[e] = (cl < ncols && k0 + k < D) ? g[src[e] + lobe_off + k0 + k] : 0.f;
    });
    pre_t = (tid < kKC && k0 + tid < D) ? dtab[k0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage = [&]() {
    const float cl = lb.c[li];
    m_staged = lb.m[li];
    stage_plane<NCT>(sp, pre, tid, cl);                                  // c_l here: once per value, not per MFMA operand
    if (tid < kKC) st[tid] = pre_t;
    if (++c == cr.end) c = cr.begin, ++li;                               // now the step that is fetched next
  };
  auto mac = [&](auto kind) {
    const float m = m_staged;                                            // by value: loop-invariant for the k loop
    chunk_mac<NCT, 1, true, false, true>(sp, ncols, ln, [&](int k, float (&w)[1]) {
      const float4 o = st[k];
      const float x = fmaf(o.x, tx, fmaf(o.y, ty, o.z * tz));            // the forward's dot product: direction first
      w[0] = decltype(kind)::value == kDiffuse ? fmaxf(x, 0.f) : lobe(x, m);
    }, acc);
  };
  // two loops, not a choice inside one: the accumulators stay where they are (a branch between two instantiated inner
  // loops per chunk made the compiler move all 48 registers in and out around it)
  fetch(0);
  pipeline(0, diffuse_steps, total, fetch, stage, [&]() { mac(std::integral_constant<int, kDiffuse>()); });
  pipeline(diffuse_steps, total, total, fetch, stage, [&]() { mac(std::integral_constant<int, kPhong>()); });

  float* pd = part + (size_t)blockIdx.z * (size_t)T * (size_t)N;
  for_each_c<NCT>(ln, [&](int ct, int e, int i, int j) {
    const int row = ln.row0 + i, cl = ct * 32 + j;
    if (cl < ncols && row < T) pd[(size_t)row * N + col0 + cl] = acc[0][ct][e];
  });
}

// dpano[col][texel] = dOmega_t * the sum over the splits
struct StoreGradient {
  const float4* tab;
  int T;
  float* dpano;
  __device__ void operator()(int t, int col, int, float s) const { dpano[(size_t)col * (size_t)T + t] = s * tab[t].w; }
};

}  // namespace

extern "C" size_t eml_env_prefilter_bwd_work_floats(int B, int H, int W, int Ho, int L) {
  if (!size_ok(B, H, W, Ho, L) || B == 0) return 0;
  const size_t T = 2 * (size_t)H * H, D = 2 * (size_t)Ho * Ho;
  return 4 * T + 4 * D + (size_t)make_split_plan(T, D).splits * T * 3 * (size_t)B;
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
  const int D = 2 * Ho * Ho, T = 2 * H * H, N = 3 * B;
  const SplitPlan pl = make_split_plan(T, D);               // of (H, Ho) alone: not of the batch
  float4* tab = reinterpret_cast<float4*>(work);
  float4* dtab = tab + T;
  float* part = work + 4 * (size_t)T + 4 * (size_t)D;
  hipLaunchKernelGGL(grid_table_kernel<>, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, s, H, tab);
  hipLaunchKernelGGL(grid_table_kernel<>, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, Ho, dtab);
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
  launch_split_reduce(s, part, T, N, pl.splits, 1, 0, 1, StoreGradient{tab, T, dpano});
  return eml::check_launch("eml_env_prefilter_bwd_f32");
}
