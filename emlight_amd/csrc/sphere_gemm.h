// The implicit GEMM behind every sphere integral of the library:
//     C[row][column] = sum_k weight(row, k) * operand[k][column]
// with the weights made on the fly from a per-row vector in registers and a per-k table entry in LDS, never stored.  The
// integrals of the sphere renders (sphere_render.hip), the prefiltered environment maps and their adjoint (env_prefilter.hip,
// env_prefilter_bwd.hip) and needlet analysis and synthesis (needlets.hip) are this one program; each of them keeps how a row
// is loaded, how a chunk is fetched, its weight expression and its epilogue, and nothing else.  The adjoint of the renders
// (sphere_render.hip, adjoint_kernel: two operand planes into one accumulator set, then the mirror's taps) shares the
// constants, the grid table and lobe() but keeps its own loop: through this core it measured 16 % slower.
//
// A workgroup of 256 threads owns 128 rows (one 32-row tile of v_mfma_f32_32x32x2_f32 per wave) x up to 96 columns (NCT
// tiles of 32) and walks the reduction in chunks of 64 entries: the chunk's operand, [column][entry] with a padded row, and
// its table entries sit in LDS.  The reduction may be split over grid.z; the partial tiles then go to scratch and
// split_reduce_kernel adds them in split order (no atomics: run-to-run exact).
//
// Two invariants make an image's result independent of the batch it came in, and this header is the code that keeps them:
//   1. the split is a function of the row and reduction extents alone (make_split_plan takes nothing else);
//   2. an output element's terms are added in a fixed order: chunk by chunk (pipeline), entry pair by entry pair with the
//      lower half-wave's entry first (chunk_mac: an MFMA adds its two k terms in order), split by split from 0.f
//      (split_reduce_kernel).
#pragma once
#include <hip/hip_runtime.h>

namespace eml {
namespace sgemm {

constexpr double kPi = 3.14159265358979323846;
constexpr int kThreads = 256;
constexpr int kKC = 64;                 // reduction entries per staged chunk
constexpr int kColsWG = 96;             // columns per workgroup at most: three 32-column MFMA tiles
constexpr int kRowsWG = 128;            // rows per workgroup: one 32-row tile per wave
constexpr int kStride = kKC + 1;        // LDS row of one column's chunk, padded: the 32 lanes of a half hit 32 banks
constexpr int kMaxSplit = 64;
constexpr int kSlots = 512;             // 256 CUs x 2 resident workgroups (2 waves per SIMD)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------ the plan
struct SplitPlan {
  int nchunks, per, splits, rowgroups;  // chunks of the reduction, chunks per split, splits (grid.z), row groups (grid.x)
};
// The k split: one column group's workgroups fill the part at once (floor: no second round), at most 64 splits, at least
// one chunk per split.  A function of the two extents ALONE: a summation order must not depend on the batch.
inline SplitPlan make_split_plan(long rows, long k) {
  SplitPlan pl;
  pl.nchunks = (int)((k + kKC - 1) / kKC);
  pl.rowgroups = (int)((rows + kRowsWG - 1) / kRowsWG);
  int want = kSlots / pl.rowgroups;
  if (want > kMaxSplit) want = kMaxSplit;
  if (want > pl.nchunks) want = pl.nchunks;
  if (want < 1) want = 1;
  pl.per = (pl.nchunks + want - 1) / want;
  pl.splits = (pl.nchunks + pl.per - 1) / pl.per;
  return pl;
}

// ------------------------------------------------------------------------------------------------ lanes and tiles
// lane l of a wave holds, of an MFMA operand, row or column l & 31 at reduction entry k + (l >> 5)
struct Lanes {
  int tid, wave, half, r;
  int row0, row;                        // the wave's first row and this lane's row of the workgroup's 128
};
__device__ __forceinline__ Lanes lanes() {
  Lanes ln;
  ln.tid = threadIdx.x, ln.wave = ln.tid >> 6, ln.half = (ln.tid & 63) >> 5, ln.r = ln.tid & 31;
  ln.row0 = blockIdx.x * kRowsWG + ln.wave * 32, ln.row = ln.row0 + ln.r;
  return ln;
}

// the chunks [begin, end) of split blockIdx.z
struct ChunkRange {
  int begin, end;
};
__device__ __forceinline__ ChunkRange split_chunks(int per, int nchunks) {
  ChunkRange cr;
  cr.begin = blockIdx.z * per;
  cr.end = cr.begin + per < nchunks ? cr.begin + per : nchunks;
  return cr;
}

template <int N>
__device__ __forceinline__ void zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
}

// C/D of the 32x32 tile: lane l holds, as element e, column l & 31 of row c_row(e, l >> 5).  f(ct, e, tile row, tile column)
__device__ __forceinline__ int c_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }
template <int NCT, class F>
__device__ __forceinline__ void for_each_c(const Lanes& ln, F&& f) {
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int e = 0; e < 16; ++e) f(ct, e, c_row(e, ln.half), ln.r);
}

// ------------------------------------------------------------------------------------------------ staging
// The NCT * 8 operand values a thread moves per chunk: value e is column 4 e + (tid >> 6), entry tid & 63 of the chunk, so a
// wave moves 64 consecutive entries of one column.  f(e, column, entry)
template <int NCT, class F>
__device__ __forceinline__ void for_each_load(int tid, F&& f) {
#pragma unroll
  for (int e = 0; e < NCT * 32 * kKC / kThreads; ++e) {
    const int idx = e * kThreads + tid;
    f(e, idx >> 6, idx & (kKC - 1));
  }
}
// registers -> the chunk's operand plane in LDS
template <int NCT>
__device__ __forceinline__ void stage_plane(float* __restrict__ sp, const float (&pre)[NCT * 32 * kKC / kThreads], int tid) {
  for_each_load<NCT>(tid, [&](int e, int cl, int k) { sp[cl * kStride + k] = pre[e]; });
}
// the same with every value scaled on its way
template <int NCT>
__device__ __forceinline__ void stage_plane(float* __restrict__ sp, const float (&pre)[NCT * 32 * kKC / kThreads], int tid,
                                            float scale) {
  for_each_load<NCT>(tid, [&](int e, int cl, int k) { sp[cl * kStride + k] = pre[e] * scale; });
}

// ------------------------------------------------------------------------------------------------ the pipeline
// Steps [s0, s1) of `total`; step s0 is in registers already.  fetch(s): step s, global memory -> registers; stage():
// registers -> LDS; compute(): the step's multiply-accumulate.  Two barriers per step, and the fetch of step s + 1 is
// issued behind the second one so that it is in flight while step s is computed.  The order of the calls is part of the
// contract: stage() of step s runs before fetch(s + 1), which runs before compute() of step s, and the steps are fetched
// in order with none left out -- a caller may keep a running cursor between its callables instead of dividing by the step
// (env_prefilter_bwd.hip does).
template <class Fetch, class Stage, class Compute>
__device__ __forceinline__ void pipeline(int s0, int s1, int total, Fetch&& fetch, Stage&& stage, Compute&& compute) {
  for (int s = s0; s < s1; ++s) {
    __syncthreads();                    // the previous step has been read
    stage();
    __syncthreads();
    if (s + 1 < total) fetch(s + 1);
    compute();
  }
}
template <class Fetch, class Stage, class Compute>
__device__ __forceinline__ void pipeline(int total, Fetch&& fetch, Stage&& stage, Compute&& compute) {
  if (total > 0) fetch(0);
  pipeline(0, total, total, fetch, stage, compute);
}

// ------------------------------------------------------------------------------------------------ multiply-accumulate
// One staged chunk: 64 entries against the wave's 32 rows.  weight(k, w) makes this lane's NW weights of entry k from the
// staged table; the operand is read at sp[column][k].
// One operand read feeds NW accumulator sets (weight i -> acc[i]).
//   WEIGHT_IS_A: the weight is the MFMA's A operand, C[row][column]; otherwise B, C[column][row] (a store then runs
//                along the rows).
//   GUARD: a tile beyond ncols is skipped (wave-uniform).  The accumulators of a guarded MFMA travel through VGPRs in the
//          loop (16 v_accvgpr_read / write per iteration); unguarded, columns beyond ncols must hold zeros.
//   UNROLL2: `#pragma unroll 2` on the entry loop, or the compiler's own choice.
template <int NCT, int NW, bool WEIGHT_IS_A, bool GUARD, bool UNROLL2, class Weight>
__device__ __forceinline__ void chunk_mac(const float* __restrict__ sp, int ncols, const Lanes& ln, Weight&& weight,
                                          f32x16 (&acc)[NW][NCT]) {
  auto mma = [](float w, float b, f32x16 c) {
    return WEIGHT_IS_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(w, b, c, 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_32x32x2f32(b, w, c, 0, 0, 0);
  };
  auto entry_pair = [&](int kk) {
    float w[NW];
    weight(kk + ln.half, w);
    if constexpr (GUARD) {              // the weights are made in front of the guards: left alone the compiler moves the whole
#pragma unroll                          // weight computation under the first tile's test (measured slower)
      for (int i = 0; i < NW; ++i) asm volatile("" : "+v"(w[i]));
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      if (!GUARD || ct * 32 < ncols) {
        const float v = sp[(ct * 32 + ln.r) * kStride + kk + ln.half];
#pragma unroll
        for (int i = 0; i < NW; ++i) acc[i][ct] = mma(w[i], v, acc[i][ct]);
      }
  };
  if constexpr (UNROLL2) {
#pragma unroll 2
    for (int kk = 0; kk < kKC; kk += 2) entry_pair(kk);
  } else {
    for (int kk = 0; kk < kKC; kk += 2) entry_pair(kk);
  }
}

// ------------------------------------------------------------------------------------------------ the split reduction
// part[split][slot][row][column] -> epilogue(row, column, slot, sum over the splits in split order).  grid (ceil(rows N /
// 256), slots reduced), the first of them slot0; nslots: the slots `part` holds per split.
template <class Epilogue>
__global__ __launch_bounds__(kThreads) void split_reduce_kernel(const float* __restrict__ part, int rows, int N, int splits,
                                                                int nslots, int slot0, Epilogue epilogue) {
  const int slot = slot0 + blockIdx.y;
  const size_t plane = (size_t)rows * (size_t)N;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= plane) return;
  const int row = (int)(e / N), col = (int)(e - (size_t)row * N);
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[((size_t)k * nslots + slot) * plane + e];
  epilogue(row, col, slot, s);
}
template <class Epilogue>
inline void launch_split_reduce(hipStream_t s, const float* part, int rows, int N, int splits, int nslots, int slot0, int count,
                                Epilogue epilogue) {
  const size_t plane = (size_t)rows * (size_t)N;
  hipLaunchKernelGGL((split_reduce_kernel<Epilogue>), dim3((unsigned)((plane + kThreads - 1) / kThreads), count), dim3(kThreads),
                     0, s, part, rows, N, splits, nslots, slot0, epilogue);
}

// ------------------------------------------------------------------------------------------------ the grid table
// texel (h, w) of the equirectangular grid of height G (2 G wide): omega and dOmega in f64, rounded once.  A template so that
// only the files that launch it hold a copy
template <int BLOCK = kThreads>
__global__ __launch_bounds__(BLOCK) void grid_table_kernel(int G, float4* __restrict__ tab) {
  const int t = blockIdx.x * BLOCK + threadIdx.x, W = 2 * G;
  if (t >= G * W) return;
  const int h = t / W, w = t - h * W;
  const double th = ((double)h + 0.5) * kPi / (double)G, ph = ((double)w + 0.5) * (2.0 * kPi) / (double)W;
  const double st = sin(th);
  tab[t] = make_float4((float)(st * cos(ph)), (float)(st * sin(ph)), (float)cos(th),
                       (float)(st * (kPi / (double)G) * (2.0 * kPi / (double)W)));
}

}  // namespace sgemm
}  // namespace eml
