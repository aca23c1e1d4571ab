// Real spherical harmonics (the reference's Needlets/sphere_harmonics.py): the basis matrix at arbitrary directions and
// the separable analysis / synthesis on an equirectangular grid.  DESIGN.md section 17 is the definition,
// tests/harmonic_oracle.py restates it in float64.
//
// Column l^2 + l + m, |m| <= l <= lmax <= 32, K = (lmax+1)^2.  With Ybar_l^m the fully normalised associated Legendre function
// (Condon-Shortley phase) a column is  scale * Ybar_l^|m|(z) * s^|m| {cos, sin}(|m| phi):  which part a column takes and its
// signed scale is the convention ("graphics" = shEvaluate, :48-70; "symmetrised" = spharmonic, :94-115), a host-made table,
// never a branch here.  Ybar_l^m / s^m is a polynomial in z and follows the normalised three-term recurrence
//   q_m = d_m,   q_l = a_lm (z q_{l-1} - b_lm q_{l-2}),   d_m = -sqrt((2m+1)/(2m)) d_{m-1},  d_0 = 1/sqrt(4 pi)
// (the unnormalised (2m-1)!! of the reference leaves f32 at m = 32), s^m {cos, sin}(m phi) = {Re, Im} (x + i y)^m.
//
// tab (f32, made in f64 by the caller): d[33], a[33][33] and b[33][33] indexed [m][l], conv[33][4] = per order m
// {direction (+1: the cos part is column +m, the sin part -m; -1: the other way round), scale of the cos part, of the sin part, 0}.
//
// On the grid x_p = (theta_y, phi_x) the sum over the pixels is a product: stage 1, per image row, the 2 lmax + 1 Fourier sums
// against cos / sin (m phi_x) (table `four` (W, 33, 2), always 33 orders); stage 2, times w_y Ybar_l^m(z_y) s_y^m and summed
// over the rows.  A workgroup owns 8 rows of 8 image planes: its 64 (row, plane) pairs are the 64 lanes of every wave, so the
// Fourier table is read at a wave-uniform address and a pixel is one LDS read per 65 FMAs; the four waves split each staged
// chunk of 128 columns and add their sums in wave order.  The partial coefficients of a row block go to scratch and a second
// launch adds them in block order: no atomics, run-to-run exact, and the plan depends on (H, W, lmax) only.
#include "eml_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRB = 8;                   // image rows per workgroup
constexpr int kPG = 8;                   // image planes per workgroup
constexpr int kPairs = kRB * kPG;        // = one wave: lane = row * 8 + plane
constexpr int kWC = 128;                 // columns per staged chunk, 32 per wave
constexpr int kPxStride = kWC + 1;       // padded: the 64 lanes read 64 rows at one column
constexpr int kLmax = 32, kM = kLmax + 1, kKmax = kM * kM;
constexpr int kFS = 2 * kM + 1;          // a pair's Fourier sums [m][cos, sin], padded to an odd stride
constexpr int kFour = 2 * kM;            // floats per column of the Fourier table
constexpr int kTabD = 0, kTabA = kM, kTabB = kM + kKmax, kTabConv = kM + 2 * kKmax, kTabFloats = kTabConv + 4 * kM;
constexpr int kBuf = kRB * kKmax;        // 8712 floats: the staged pixels (64 x 129 = 8256), then the rows' Legendre factors
constexpr int kMaxB = 65535, kMaxP = 1 << 24;
static_assert(kPairs == 64 && kPairs * kPxStride <= kBuf && kWC * kPairs == 32 * kThreads && kTabFloats == 2343, "tiling");

// ------------------------------------------------------------------------------------------------ basis matrix
// out[p][k]: a thread per (point, m) runs the recurrence once and gives its 2 (lmax - m + 1) columns; a workgroup's points are
// consecutive, so their rows are one contiguous piece of `out`, assembled in LDS and stored along it.
__global__ __launch_bounds__(kThreads) void basis_kernel(const float* __restrict__ dirs, const float* __restrict__ tab, int P,
                                                         int lmax, float* __restrict__ out) {
  __shared__ float tile[kThreads * kM];                                  // PB * K <= 256 (lmax + 1)
  const int M1 = lmax + 1, K = M1 * M1, PB = kThreads / M1;
  const int tid = threadIdx.x, pl = tid / M1, m = tid - pl * M1;
  const size_t p0 = (size_t)blockIdx.x * PB;
  if (pl < PB && p0 + pl < (size_t)P) {
    const float* v = dirs + (p0 + pl) * 3;
    const float x = v[0], y = v[1], z = v[2];
    float re = 1.f, im = 0.f;                                            // (x + i y)^m
    for (int i = 0; i < m; ++i) {
      const float nr = fmaf(re, x, -(im * y)), ni = fmaf(re, y, im * x);
      re = nr, im = ni;
    }
    const float* cv = tab + kTabConv + 4 * m;
    const int dir = (int)cv[0];
    const float fc = re * cv[1], fs = im * cv[2];
    const float *a = tab + kTabA + m * kM, *b = tab + kTabB + m * kM;
    float* row = tile + pl * K;
    float q0 = 0.f, q1 = tab[kTabD + m];
    for (int l = m; l <= lmax; ++l) {
      if (l > m) {
        const float q = a[l] * fmaf(z, q1, -(b[l] * q0));
        q0 = q1, q1 = q;
      }
      const int c = l * l + l;
      row[c + dir * m] = q1 * fc;
      if (m) row[c - dir * m] = q1 * fs;
    }
  }
  __syncthreads();
  const size_t left = (size_t)P - p0;
  const int count = (int)(left < (size_t)PB ? left : (size_t)PB) * K;
  float* dst = out + p0 * (size_t)K;
  for (int i = tid; i < count; i += kThreads) dst[i] = tile[i];
}

// ------------------------------------------------------------------------------------------------ the rows' Legendre factors
// lam[r][k] = w_y * scale_k * Ybar_l^|m|(z_y) s_y^|m| for the rows y0 .. y0 + 7 (0 beyond H); fi[k] = 2 |m| + (sin part).
// sab: the recurrence's a and b in LDS (load_recurrence).  A thread takes the orders j and lmax - j of one row, lmax + 2
// steps whatever j: 8 x 17 threads at lmax = 32, one pass.
__device__ __forceinline__ void load_recurrence(const float* __restrict__ tab, float* sab) {
  for (int i = threadIdx.x; i < 2 * kKmax; i += kThreads) sab[i] = tab[kTabA + i];
}
__device__ __forceinline__ void row_factors(const float* __restrict__ rows, const float* __restrict__ wts,
                                            const float* __restrict__ tab, const float* sab, int H, int lmax, int y0,
                                            float* lam, unsigned char* fi) {
  const int M1 = lmax + 1, K = M1 * M1, half = (M1 + 1) / 2;
  for (int i = threadIdx.x; i < kRB * half; i += kThreads) {
    const int r = i / half, j = i - r * half, y = y0 + r;
    float z = 0.f, s = 0.f, w = 0.f;
    if (y < H) z = rows[2 * y], s = rows[2 * y + 1], w = wts ? wts[y] : 1.f;
    float* row = lam + r * K;
    for (int side = 0; side < 2; ++side) {
      const int m = side ? lmax - j : j;
      if (side && m <= j) break;                                         // the middle order once
      float sm = 1.f;
      for (int e = 0; e < m; ++e) sm *= s;
      const float* cv = tab + kTabConv + 4 * m;
      const int dir = (int)cv[0];
      const float fc = sm * cv[1] * w, fs = sm * cv[2] * w;
      const float *a = sab + m * kM, *b = sab + kKmax + m * kM;
      float q0 = 0.f, q1 = tab[kTabD + m];
      for (int l = m; l <= lmax; ++l) {
        if (l > m) {
          const float q = a[l] * fmaf(z, q1, -(b[l] * q0));
          q0 = q1, q1 = q;
        }
        const int c = l * l + l;
        row[c + dir * m] = q1 * fc;
        if (m) row[c - dir * m] = q1 * fs;
        if (fi && r == 0) {
          fi[c + dir * m] = (unsigned char)(2 * m);
          if (m) fi[c - dir * m] = (unsigned char)(2 * m + 1);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ analysis
// grid (row blocks, plane groups); part[row block][plane][k]
template <int LM>
__global__ __launch_bounds__(kThreads) void analysis_kernel(const float* __restrict__ pano, const float* __restrict__ rows,
                                                            const float* __restrict__ wts, const float* __restrict__ four,
                                                            const float* __restrict__ tab, int H, int W, int N, int lmax,
                                                            float* __restrict__ part) {
  __shared__ float sbuf[kBuf];
  __shared__ float sF[kPairs * kFS];
  __shared__ unsigned char sfi[kKmax];
  __shared__ float sab[2 * kKmax];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);            // uniform to the compiler: the table is read through the scalar cache
  const int y0 = blockIdx.x * kRB, n0 = blockIdx.y * kPG;
  float ac[LM + 1], as[LM + 1];
#pragma unroll
  for (int m = 0; m <= LM; ++m) ac[m] = 0.f, as[m] = 0.f;
  load_recurrence(tab, sab);                                             // read after the barriers below
  // stage 1: the Fourier sums of this lane's (row, plane) over the wave's 32 columns of every chunk
  for (int x0 = 0; x0 < W; x0 += kWC) {
    float px[kWC * kPairs / kThreads];                                   // all 32 loads in flight, then the barrier
#pragma unroll
    for (int e = 0; e < kWC * kPairs / kThreads; ++e) {
      const int idx = e * kThreads + tid, pr = idx >> 7, xx = idx & (kWC - 1);
      const int y = y0 + (pr >> 3), n = n0 + (pr & 7), x = x0 + xx;
      px[e] = (y < H && n < N && x < W) ? pano[((size_t)n * H + y) * (size_t)W + x] : 0.f;
    }
    __syncthreads();                                                     // the previous chunk has been read
#pragma unroll
    for (int e = 0; e < kWC * kPairs / kThreads; ++e) {
      const int idx = e * kThreads + tid;
      sbuf[(idx >> 7) * kPxStride + (idx & (kWC - 1))] = px[e];
    }
    __syncthreads();
    const int xb = wave * (kWC / 4);
    for (int j = 0; j < kWC / 4; ++j) {
      const int x = x0 + xb + j;
      if (x >= W) break;                                                 // wave-uniform
      const float v = sbuf[lane * kPxStride + xb + j];
      const float* t = four + (size_t)x * kFour;                         // wave-uniform address
      ac[0] = fmaf(v, t[0], ac[0]);
#pragma unroll
      for (int m = 1; m <= LM; ++m) {
        ac[m] = fmaf(v, t[2 * m], ac[m]);
        as[m] = fmaf(v, t[2 * m + 1], as[m]);
      }
    }
  }
  // the four waves' sums, added in wave order
  for (int q = 0; q < 4; ++q) {
    __syncthreads();
    if (wave == q) {
      float* f = sF + lane * kFS;
#pragma unroll
      for (int m = 0; m <= LM; ++m) {
        f[2 * m] = q ? f[2 * m] + ac[m] : ac[m];
        f[2 * m + 1] = q ? f[2 * m + 1] + as[m] : as[m];
      }
    }
  }
  row_factors(rows, wts, tab, sab, H, lmax, y0, sbuf, sfi);                   // the pixels in sbuf were last read before the barriers above
  __syncthreads();
  // stage 2: times the rows' factors, summed over the 8 rows in row order
  const int K = (lmax + 1) * (lmax + 1);
  for (int i = tid; i < kPG * K; i += kThreads) {
    const int nl = i / K, k = i - nl * K, n = n0 + nl;
    if (n >= N) break;                                                   // i grows with nl
    const int f = sfi[k];
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < kRB; ++r) s = fmaf(sbuf[r * K + k], sF[(r * kPG + nl) * kFS + f], s);
    part[((size_t)blockIdx.x * N + n) * (size_t)K + k] = s;
  }
}

// coeffs[b][k][ch] = sum over the row blocks, in block order
__global__ __launch_bounds__(kThreads) void analysis_reduce_kernel(const float* __restrict__ part, int K, int N, int blocks,
                                                                   float* __restrict__ out) {
  const size_t plane = (size_t)K * (size_t)N;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= plane) return;
  const int n = (int)(e / K), k = (int)(e - (size_t)n * K);
  float s = 0.f;
  for (int z = 0; z < blocks; ++z) s += part[(size_t)z * plane + e];
  out[((size_t)(n / 3) * K + k) * 3 + n % 3] = s;
}

// ------------------------------------------------------------------------------------------------ synthesis
// the transpose: per (row, plane) the Legendre sums to the 2 lmax + 1 ring coefficients, then the Fourier sum along the row
template <int LM>
__global__ __launch_bounds__(kThreads) void synthesis_kernel(const float* __restrict__ coeffs, const float* __restrict__ rows,
                                                             const float* __restrict__ wts, const float* __restrict__ four,
                                                             const float* __restrict__ tab, int H, int W, int N, int lmax,
                                                             float* __restrict__ rec) {
  __shared__ float sbuf[kBuf];
  __shared__ float sG[kPairs * kFS];
  __shared__ float sab[2 * kKmax];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);            // uniform to the compiler: the table is read through the scalar cache
  const int y0 = blockIdx.x * kRB, n0 = blockIdx.y * kPG;
  const int M1 = lmax + 1, K = M1 * M1;
  load_recurrence(tab, sab);
  __syncthreads();
  row_factors(rows, wts, tab, sab, H, lmax, y0, sbuf, nullptr);
  __syncthreads();
  // ring coefficients: an item is (m, part) for the wave and the 64 pairs for its lanes
  {
    const int r = lane >> 3, n = n0 + (lane & 7);
    const float* cf = coeffs + (size_t)(n < N ? n / 3 : 0) * K * 3 + (n < N ? n % 3 : 0);
    const float* lam = sbuf + r * K;
    for (int f = wave; f < 2 * M1; f += 4) {                             // wave-uniform
      const int m = f >> 1, sn = f & 1;
      float g = 0.f;
      if (n < N && !(sn && !m)) {
        const int dir = (int)tab[kTabConv + 4 * m], off = sn ? -dir * m : dir * m;
        for (int l = m; l <= lmax; ++l) {
          const int k = l * l + l + off;
          g = fmaf(lam[k], cf[(size_t)k * 3], g);
        }
      }
      sG[lane * kFS + f] = g;
    }
  }
  __syncthreads();
  float gc[LM + 1], gs[LM + 1];
#pragma unroll
  for (int m = 0; m <= LM; ++m) {
    gc[m] = m <= lmax ? sG[lane * kFS + 2 * m] : 0.f;
    gs[m] = m <= lmax ? sG[lane * kFS + 2 * m + 1] : 0.f;
  }
  for (int x0 = 0; x0 < W; x0 += kWC) {
    __syncthreads();                                                     // the factors / the previous chunk have been read
    const int xb = wave * (kWC / 4);
    for (int j = 0; j < kWC / 4; ++j) {
      const int x = x0 + xb + j;
      if (x >= W) break;                                                 // wave-uniform
      const float* t = four + (size_t)x * kFour;
      float v = gc[0] * t[0];
#pragma unroll
      for (int m = 1; m <= LM; ++m) {
        v = fmaf(gc[m], t[2 * m], v);
        v = fmaf(gs[m], t[2 * m + 1], v);
      }
      sbuf[lane * kPxStride + xb + j] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < kWC * kPairs / kThreads; ++e) {                  // stores run along the pixels
      const int idx = e * kThreads + tid, pr = idx >> 7, xx = idx & (kWC - 1);
      const int y = y0 + (pr >> 3), n = n0 + (pr & 7), x = x0 + xx;
      if (y < H && n < N && x < W) rec[((size_t)n * H + y) * (size_t)W + x] = sbuf[pr * kPxStride + xx];
    }
  }
}

// ------------------------------------------------------------------------------------------------ launch helpers
template <int LM>
void launch_analysis(dim3 grid, hipStream_t s, const float* pano, const float* rows, const float* wts, const float* four,
                     const float* tab, int H, int W, int N, int lmax, float* part) {
  hipLaunchKernelGGL((analysis_kernel<LM>), grid, dim3(kThreads), 0, s, pano, rows, wts, four, tab, H, W, N, lmax, part);
}
template <int LM>
void launch_synthesis(dim3 grid, hipStream_t s, const float* coeffs, const float* rows, const float* wts, const float* four,
                      const float* tab, int H, int W, int N, int lmax, float* rec) {
  hipLaunchKernelGGL((synthesis_kernel<LM>), grid, dim3(kThreads), 0, s, coeffs, rows, wts, four, tab, H, W, N, lmax, rec);
}
// the orders held in registers: the smallest of 4, 8, 16, 32 that holds lmax
#define EML_SH_DISPATCH(lmax, CALL) \
  if (lmax <= 4) CALL(4);           \
  else if (lmax <= 8) CALL(8);      \
  else if (lmax <= 16) CALL(16);    \
  else CALL(32)

inline bool lmax_ok(int lmax) { return lmax >= 0 && lmax <= kLmax; }
inline bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= kMaxP; }
inline int row_blocks(int H) { return (H + kRB - 1) / kRB; }

const char* check_grid_call(const char* who, bool ptrs, int lmax, int H, int W, int B) {
  static thread_local char msg[160];
  if (!ptrs) return snprintf(msg, sizeof msg, "%s: null pointer", who), msg;
  if (!lmax_ok(lmax)) return snprintf(msg, sizeof msg, "%s: lmax must be 0..%d, got %d", who, kLmax, lmax), msg;
  if (!grid_ok(H, W))
    return snprintf(msg, sizeof msg, "%s: P must be 1..%d, got H = %d, W = %d", who, kMaxP, H, W), msg;
  if (B < 0 || B > kMaxB) return snprintf(msg, sizeof msg, "%s: grid limits: 0 <= B <= %d, got %d", who, kMaxB, B), msg;
  return nullptr;
}

}  // namespace

extern "C" size_t eml_sh_work_floats(int H, int W, int lmax, int B) {
  if (!lmax_ok(lmax) || !grid_ok(H, W) || B < 1 || B > kMaxB) return 0;
  return (size_t)row_blocks(H) * (size_t)(lmax + 1) * (lmax + 1) * 3 * (size_t)B;
}

extern "C" int eml_sh_basis_f32(const float* dirs, int P, const float* tab, int lmax, float* out, eml_stream_t stream) {
  if (!dirs || !tab || !out) return eml::fail(EML_EINVAL, "eml_sh_basis_f32: null pointer");
  if (!lmax_ok(lmax)) return eml::fail(EML_EINVAL, "eml_sh_basis_f32: lmax must be 0..%d, got %d", kLmax, lmax);
  if (P < 1 || P > kMaxP) return eml::fail(EML_EINVAL, "eml_sh_basis_f32: P must be 1..%d, got %d", kMaxP, P);
  const int PB = kThreads / (lmax + 1);
  hipLaunchKernelGGL(basis_kernel, dim3((unsigned)((P + PB - 1) / PB)), dim3(kThreads), 0, (hipStream_t)stream, dirs, tab, P, lmax,
                     out);
  return eml::check_launch("eml_sh_basis_f32");
}

extern "C" int eml_sh_analysis_f32(const float* pano, const float* rows, const float* weights, const float* fourier,
                                   const float* tab, int B, int H, int W, int lmax, float* coeffs, float* work,
                                   eml_stream_t stream) {
  if (const char* e = check_grid_call("eml_sh_analysis_f32", pano && rows && fourier && tab && coeffs && work, lmax, H, W, B))
    return eml::fail(EML_EINVAL, "%s", e);
  if (B == 0) return EML_OK;
  hipStream_t s = (hipStream_t)stream;
  const int N = 3 * B, K = (lmax + 1) * (lmax + 1), blocks = row_blocks(H);
  const dim3 grid(blocks, (N + kPG - 1) / kPG);
#define CALL(LM) launch_analysis<LM>(grid, s, pano, rows, weights, fourier, tab, H, W, N, lmax, work)
  EML_SH_DISPATCH(lmax, CALL);
#undef CALL
  int rc = eml::check_launch("eml_sh_analysis_f32(partial)");
  if (rc) return rc;
  const size_t plane = (size_t)K * N;
  hipLaunchKernelGGL(analysis_reduce_kernel, dim3((unsigned)((plane + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     (const float*)work, K, N, blocks, coeffs);
  return eml::check_launch("eml_sh_analysis_f32");
}

extern "C" int eml_sh_synthesis_f32(const float* coeffs, const float* rows, const float* weights, const float* fourier,
                                    const float* tab, int B, int H, int W, int lmax, float* rec, eml_stream_t stream) {
  if (const char* e = check_grid_call("eml_sh_synthesis_f32", coeffs && rows && fourier && tab && rec, lmax, H, W, B))
    return eml::fail(EML_EINVAL, "%s", e);
  if (B == 0) return EML_OK;
  const int N = 3 * B;
  const dim3 grid(row_blocks(H), (N + kPG - 1) / kPG);
#define CALL(LM) launch_synthesis<LM>(grid, (hipStream_t)stream, coeffs, rows, weights, fourier, tab, H, W, N, lmax, rec)
  EML_SH_DISPATCH(lmax, CALL);
#undef CALL
  return eml::check_launch("eml_sh_synthesis_f32");
}
