// Spherical needlets (NeedleLight; the reference's Needlets/ folder): basis matrix, analysis, synthesis, sparsify.
// DESIGN.md section 16 is the definition, tests/needlet_oracle.py restates it in float64.
//
// Row k of the basis is Y_00 (k = 0) or the needlet of level j centred at the HEALPix pixel centre xi_jk; by the addition
// theorem its value at direction x is a zonal sum  psi(x) = sum_{l <= L} c[level][l] P_l(xi . x),  L = 2^(jmax+1) <= 32, with
// c[level][l] = sqrt(lambda_j) b(l / 2^j) (2l+1) / 4pi made on the host in f64 (sphere_needlets.py:34-104 evaluates the same
// sum through the spherical harmonics of x).  A level's coefficients beyond its own 2^(j+1) are zero, so every row runs the
// same Legendre recurrence and the rows of one tile may span levels without a branch.
//
// Analysis (coeffs = Psi^T . (w * pano), gt_gen_j3.py:39-43) and synthesis (rec = w * Psi . coeffs, mat_gen2.py:55) are the
// implicit GEMM of sphere_gemm.h with Psi as the weight: a lane keeps its row's vector (a centre / a pixel direction), the
// reduction chunk (pixels / basis rows: vector, weight or level, and the 3B image planes) is staged in LDS.  Analysis
// splits the pixels; synthesis is not split.
#include "eml_common.h"
#include "sphere_gemm.h"

namespace {

using namespace eml::sgemm;

constexpr int kLmax = 32, kTabRow = kLmax + 1, kMaxLevels = 6;     // table rows: Y_00, levels 0..4
constexpr int kMaxB = 65535, kMaxP = 1 << 24;

inline int rows_of(int jmax) { return (1 << (2 * (jmax + 2))) - 3; }             // 1 + 12 (1 + 4 + ... + 4^jmax)
__host__ __device__ inline int level_start(int j) { return (1 << (2 * (j + 1))) - 3; }   // first row of level j

// sum_{l <= L} c[l] P_l(t): three-term recurrence l P_l = (2l-1) t P_{l-1} - (l-1) P_{l-2}
template <int L>
__device__ __forceinline__ float psi(const float* __restrict__ c, float t) {
  float p0 = 1.f, p1 = t, s = fmaf(c[1], t, c[0]);
#pragma unroll
  for (int l = 2; l <= L; ++l) {
    const float a = (float)((2.0 * l - 1.0) / l), b = (float)((l - 1.0) / l);
    const float p = fmaf(a * t, p1, -(b * p0));
    s = fmaf(c[l], p, s);
    p0 = p1, p1 = p;
  }
  return s;
}

// the coefficient table in LDS, with one more row of zeros (a reduction entry beyond K weighs 0)
__device__ __forceinline__ void load_table(const float* __restrict__ ctab, int nlev, float* sc) {
  for (int i = threadIdx.x; i < (kMaxLevels + 1) * kTabRow; i += kThreads) sc[i] = i < nlev * kTabRow ? ctab[i] : 0.f;
}

// ------------------------------------------------------------------------------------------------ basis matrix
// out[p][k] = psi_k(x_p): a thread per element, k fastest
template <int L>
__global__ __launch_bounds__(kThreads) void basis_kernel(const float* __restrict__ dirs, const float4* __restrict__ cen,
                                                         const float* __restrict__ ctab, int nlev, int P, int K,
                                                         float* __restrict__ out) {
  __shared__ float sc[(kMaxLevels + 1) * kTabRow];
  load_table(ctab, nlev, sc);
  __syncthreads();
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (size_t)P * (size_t)K) return;
  const size_t p = e / (size_t)K;
  const int k = (int)(e - p * (size_t)K);
  const float4 c = cen[k];
  const float* x = dirs + p * 3;
  const float t = fmaf(c.x, x[0], fmaf(c.y, x[1], c.z * x[2]));
  out[e] = psi<L>(sc + (int)c.w * kTabRow, t);
}

// ------------------------------------------------------------------------------------------------ the implicit GEMM
// SYNTH == false (analysis): rows = basis functions (R = K), reduction = pixels (T = P), src = pano (N, P);
//   grid (rowgroups, colgroups, splits), dst = part[split][k][column].
// SYNTH == true: rows = pixels (R = P), reduction = basis functions (T = K), src = coeffs (B, K, 3);
//   grid (rowgroups, colgroups, 1), dst = rec (N, P), written directly: the weight is the MFMA's B operand, C[plane][pixel],
//   so that a store runs along the pixels.
// Three column tiles under the guard; the entry loop is left to the compiler (psi<L> is long).
template <int L, bool SYNTH>
__global__ __launch_bounds__(kThreads) void gemm_kernel(const float* __restrict__ src, const float4* __restrict__ cen,
                                                        const float* __restrict__ dirs, const float* __restrict__ wts,
                                                        const float* __restrict__ ctab, int nlev, int K, int P, int N, int per,
                                                        int nchunks, float* __restrict__ dst) {
  __shared__ float sp[kColsWG * kStride];
  __shared__ float4 st[kKC];
  __shared__ float sc[(kMaxLevels + 1) * kTabRow];
  const Lanes ln = lanes();
  const int tid = ln.tid, row = ln.row;
  const int R = SYNTH ? P : K, T = SYNTH ? K : P;
  load_table(ctab, nlev, sc);
  __syncthreads();
  float vx = 0.f, vy = 0.f, vz = 0.f, wrow = 1.f;
  float cr[L + 1];                                                       // analysis: the row's own coefficients
#pragma unroll
  for (int l = 0; l <= L; ++l) cr[l] = 0.f;                              // a row beyond K weighs 0 and is never stored
  if (row < R) {
    if (SYNTH) {
      vx = dirs[(size_t)row * 3], vy = dirs[(size_t)row * 3 + 1], vz = dirs[(size_t)row * 3 + 2];
      if (wts) wrow = wts[row];
    } else {
      const float4 c = cen[row];
      vx = c.x, vy = c.y, vz = c.z;
      const float* q = sc + (int)c.w * kTabRow;
#pragma unroll
      for (int l = 0; l <= L; ++l) cr[l] = q[l];
    }
  }
  const int col0 = blockIdx.y * kColsWG;
  const int ncols = N - col0 < kColsWG ? N - col0 : kColsWG;             // > 0 by the grid
  f32x16 acc[1][3];
  zero(acc[0]);

  const ChunkRange chunks = split_chunks(per, nchunks);
  float pre[kColsWG * kKC / kThreads];
  float4 pre_t;
  auto fetch = [&](int step) {
    const int k0 = (chunks.begin + step) * kKC;
    for_each_load<3>(tid, [&](int e, int cl, int ko) {
      const int k = k0 + ko;
      float v = 0.f;
      if (cl < ncols && k < T) {
        const int col = col0 + cl;
        v = SYNTH ? src[((size_t)(col / 3) * K + k) * 3 + col % 3] : src[(size_t)col * (size_t)P + k];
      }
      pre[e] = v;
    });
    pre_t = make_float4(0.f, 0.f, 0.f, SYNTH ? (float)nlev : 0.f);        // beyond T: the zero row / weight 0
    if (tid < kKC && k0 + tid < T) {
      if (SYNTH) pre_t = cen[k0 + tid];
      else {
        const float* x = dirs + (size_t)(k0 + tid) * 3;
        pre_t = make_float4(x[0], x[1], x[2], wts ? wts[k0 + tid] : 1.f);
      }
    }
  };
  auto stage = [&]() {
    stage_plane<3>(sp, pre, tid);
    if (tid < kKC) st[tid] = pre_t;
  };
  auto weight = [&](int k, float (&w)[1]) {
    const float4 t = st[k];
    const float d = fmaf(vx, t.x, fmaf(vy, t.y, vz * t.z));
    w[0] = SYNTH ? psi<L>(sc + (int)t.w * kTabRow, d) : psi<L>(cr, d) * t.w;
  };
  pipeline(chunks.end - chunks.begin, fetch, stage,
           [&]() { chunk_mac<3, 1, !SYNTH, true, false>(sp, ncols, ln, weight, acc); });

  for_each_c<3>(ln, [&](int ct, int e, int i, int j) {
    if (SYNTH) {
      const int cl = ct * 32 + i;
      if (cl < ncols && row < P) dst[(size_t)(col0 + cl) * (size_t)P + row] = acc[0][ct][e] * wrow;
    } else {
      const int cl = ct * 32 + j, k = ln.row0 + i;
      if (cl < ncols && k < K) dst[((size_t)blockIdx.z * K + k) * (size_t)N + col0 + cl] = acc[0][ct][e];
    }
  });
}

// coeffs[b][k][ch] = the sum over the splits
struct StoreCoeffs {
  int K;
  float* out;
  __device__ void operator()(int k, int col, int, float s) const { out[((size_t)(col / 3) * K + k) * 3 + col % 3] = s; }
};

// ------------------------------------------------------------------------------------------------ sparsify
// grid (jmax + 2, B): block x = 0 copies row 0 (Y_00), block x = j + 1 owns level j of image y
__global__ __launch_bounds__(kThreads) void sparsify_kernel(const float* __restrict__ in, int K, int nlevels, int levels_mask,
                                                            float ratio, float* __restrict__ out, int* __restrict__ kept) {
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (blockIdx.x == 0) {
    if (tid < 3) out[(size_t)b * K * 3 + tid] = in[(size_t)b * K * 3 + tid];
    return;
  }
  const int j = blockIdx.x - 1;
  const int n = 3 * (level_start(j + 1) - level_start(j));
  const size_t base = ((size_t)b * K + level_start(j)) * 3;
  const float* x = in + base;
  float* y = out + base;
  if (!((levels_mask >> j) & 1)) {                                       // block-uniform
    for (int i = tid; i < n; i += kThreads) y[i] = x[i];
    if (tid == 0) kept[b * nlevels + j] = n;
    return;
  }
  float m = 0.f;
  for (int i = tid; i < n; i += kThreads) m = fmaxf(m, fabsf(x[i]));
  redf[tid] = m;
  __syncthreads();
  for (int s = kThreads >> 1; s > 0; s >>= 1) {
    if (tid < s) redf[tid] = fmaxf(redf[tid], redf[tid + s]);
    __syncthreads();
  }
  const float thr = __fmul_rn(ratio, redf[0]);
  int cnt = 0;
  for (int i = tid; i < n; i += kThreads) {
    const float v = x[i];
    const bool keep = fabsf(v) > thr;
    y[i] = keep ? v : 0.f;
    cnt += keep;
  }
  redi[tid] = cnt;
  __syncthreads();
  for (int s = kThreads >> 1; s > 0; s >>= 1) {
    if (tid < s) redi[tid] += redi[tid + s];
    __syncthreads();
  }
  if (tid == 0) kept[b * nlevels + j] = redi[0];
}

// ------------------------------------------------------------------------------------------------ launch helpers
template <int L>
void launch_basis(hipStream_t s, const float* dirs, const float4* cen, const float* ctab, int nlev, int P, int K, float* out) {
  const size_t total = (size_t)P * (size_t)K;
  hipLaunchKernelGGL((basis_kernel<L>), dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, dirs, cen, ctab,
                     nlev, P, K, out);
}
template <int L, bool SYNTH>
void launch_gemm(dim3 grid, hipStream_t s, const float* src, const float4* cen, const float* dirs, const float* wts,
                 const float* ctab, int nlev, int K, int P, int N, int per, int nchunks, float* dst) {
  hipLaunchKernelGGL((gemm_kernel<L, SYNTH>), grid, dim3(kThreads), 0, s, src, cen, dirs, wts, ctab, nlev, K, P, N, per, nchunks,
                     dst);
}
#define EML_NEEDLET_DISPATCH(jmax, CALL) \
  switch (jmax) {                        \
    case 0: CALL(2); break;              \
    case 1: CALL(4); break;              \
    case 2: CALL(8); break;              \
    case 3: CALL(16); break;             \
    default: CALL(32); break;            \
  }

inline bool jmax_ok(int jmax) { return jmax >= 0 && jmax <= 4; }

}  // namespace

extern "C" size_t eml_needlet_work_floats(int P, int jmax, int B) {
  if (!jmax_ok(jmax) || P < 1 || P > kMaxP || B < 1 || B > kMaxB) return 0;
  return (size_t)make_split_plan(rows_of(jmax), P).splits * rows_of(jmax) * 3 * (size_t)B;
}

extern "C" int eml_needlet_basis_f32(const float* dirs, int P, const float* centres, const float* ctab, int jmax, float* out,
                                     eml_stream_t stream) {
  if (!dirs || !centres || !ctab || !out) return eml::fail(EML_EINVAL, "eml_needlet_basis_f32: null pointer");
  if (!jmax_ok(jmax)) return eml::fail(EML_EINVAL, "eml_needlet_basis_f32: jmax must be 0..4, got %d", jmax);
  if (P < 1 || P > kMaxP) return eml::fail(EML_EINVAL, "eml_needlet_basis_f32: P must be 1..%d, got %d", kMaxP, P);
  if (((size_t)centres) & 15) return eml::fail(EML_EINVAL, "eml_needlet_basis_f32: centres must be 16-byte aligned");
  const int K = rows_of(jmax), nlev = jmax + 2;
  const float4* cen = reinterpret_cast<const float4*>(centres);
#define CALL(L) launch_basis<L>((hipStream_t)stream, dirs, cen, ctab, nlev, P, K, out)
  EML_NEEDLET_DISPATCH(jmax, CALL)
#undef CALL
  return eml::check_launch("eml_needlet_basis_f32");
}

extern "C" int eml_needlet_analysis_f32(const float* pano, const float* dirs, const float* weights, int B, int P,
                                        const float* centres, const float* ctab, int jmax, float* coeffs, float* work,
                                        eml_stream_t stream) {
  if (!pano || !dirs || !centres || !ctab || !coeffs || !work)
    return eml::fail(EML_EINVAL, "eml_needlet_analysis_f32: null pointer");
  if (!jmax_ok(jmax)) return eml::fail(EML_EINVAL, "eml_needlet_analysis_f32: jmax must be 0..4, got %d", jmax);
  if (P < 1 || P > kMaxP) return eml::fail(EML_EINVAL, "eml_needlet_analysis_f32: P must be 1..%d, got %d", kMaxP, P);
  if (B < 0 || B > kMaxB) return eml::fail(EML_EINVAL, "eml_needlet_analysis_f32: grid limits: 0 <= B <= %d, got %d", kMaxB, B);
  if ((((size_t)work) | ((size_t)centres)) & 15)
    return eml::fail(EML_EINVAL, "eml_needlet_analysis_f32: work and centres must be 16-byte aligned");
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const int K = rows_of(jmax), N = 3 * B, nlev = jmax + 2;
  const SplitPlan pl = make_split_plan(K, P);               // of (P, jmax) alone: not of the batch
  const float4* cen = reinterpret_cast<const float4*>(centres);
  const dim3 grid(pl.rowgroups, (N + kColsWG - 1) / kColsWG, pl.splits);
#define CALL(L) launch_gemm<L, false>(grid, s, pano, cen, dirs, weights, ctab, nlev, K, P, N, pl.per, pl.nchunks, work)
  EML_NEEDLET_DISPATCH(jmax, CALL)
#undef CALL
  int rc = eml::check_launch("eml_needlet_analysis_f32(partial)");
  if (rc) return rc;
  launch_split_reduce(s, work, K, N, pl.splits, 1, 0, 1, StoreCoeffs{K, coeffs});
  return eml::check_launch("eml_needlet_analysis_f32");
}

extern "C" int eml_needlet_synthesis_f32(const float* coeffs, const float* dirs, const float* weights, int B, int P,
                                         const float* centres, const float* ctab, int jmax, float* rec, eml_stream_t stream) {
  if (!coeffs || !dirs || !centres || !ctab || !rec) return eml::fail(EML_EINVAL, "eml_needlet_synthesis_f32: null pointer");
  if (!jmax_ok(jmax)) return eml::fail(EML_EINVAL, "eml_needlet_synthesis_f32: jmax must be 0..4, got %d", jmax);
  if (P < 1 || P > kMaxP) return eml::fail(EML_EINVAL, "eml_needlet_synthesis_f32: P must be 1..%d, got %d", kMaxP, P);
  if (B < 0 || B > kMaxB) return eml::fail(EML_EINVAL, "eml_needlet_synthesis_f32: grid limits: 0 <= B <= %d, got %d", kMaxB, B);
  if (((size_t)centres) & 15) return eml::fail(EML_EINVAL, "eml_needlet_synthesis_f32: centres must be 16-byte aligned");
  if (B == 0) return EML_OK;
  const int K = rows_of(jmax), N = 3 * B, nlev = jmax + 2;
  const float4* cen = reinterpret_cast<const float4*>(centres);
  const int nchunks = (K + kKC - 1) / kKC;
  const dim3 grid((P + kRowsWG - 1) / kRowsWG, (N + kColsWG - 1) / kColsWG, 1);
#define CALL(L) launch_gemm<L, true>(grid, (hipStream_t)stream, coeffs, cen, dirs, weights, ctab, nlev, K, P, N, nchunks, nchunks, rec)
  EML_NEEDLET_DISPATCH(jmax, CALL)
#undef CALL
  return eml::check_launch("eml_needlet_synthesis_f32");
}

extern "C" int eml_needlet_sparsify_f32(const float* coeffs, int B, int jmax, int levels_mask, double ratio, float* out,
                                        int* kept, eml_stream_t stream) {
  if (!coeffs || !out || !kept) return eml::fail(EML_EINVAL, "eml_needlet_sparsify_f32: null pointer");
  if (!jmax_ok(jmax)) return eml::fail(EML_EINVAL, "eml_needlet_sparsify_f32: jmax must be 0..4, got %d", jmax);
  if (levels_mask < 0 || levels_mask >= (1 << (jmax + 1)))
    return eml::fail(EML_EINVAL, "eml_needlet_sparsify_f32: levels mask %d names a level beyond jmax = %d", levels_mask, jmax);
  if (!(ratio >= 0.0) || !(ratio <= 1.0))
    return eml::fail(EML_EINVAL, "eml_needlet_sparsify_f32: ratio must be in [0, 1], got %g", ratio);
  if (B < 0 || B > kMaxB) return eml::fail(EML_EINVAL, "eml_needlet_sparsify_f32: grid limits: 0 <= B <= %d, got %d", kMaxB, B);
  if (B == 0) return EML_OK;
  hipLaunchKernelGGL(sparsify_kernel, dim3(jmax + 2, B), dim3(kThreads), 0, (hipStream_t)stream, coeffs, rows_of(jmax), jmax + 1,
                     levels_mask, (float)ratio, out, kept);
  return eml::check_launch("eml_needlet_sparsify_f32");
}
