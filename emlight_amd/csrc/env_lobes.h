// The lobe weights of the sphere renders (sphere_render.hip) and of the prefiltered environment maps, forward
// (env_prefilter.hip) and adjoint (env_prefilter_bwd.hip): all make k_l(omega_d . omega_t) from the SAME f32 grid tables
// (sphere_gemm.h), the same dot product and the same lobe(), bit for bit (DESIGN.md sections 15, 22 and 23).
#pragma once
#include "sphere_gemm.h"

namespace eml {
namespace env {

using sgemm::kPi;
constexpr int kMaxHo = 1024, kMaxH = 4096, kMaxB = 4096, kMaxL = 8;
constexpr int kNone = 0, kDiffuse = 1, kPhong = 2;

inline bool size_ok(int B, int H, int W, int Ho, int L) {
  return B >= 0 && B <= kMaxB && H >= 1 && H <= kMaxH && W == 2 * H && Ho >= 1 && Ho <= kMaxHo && L >= 1 && L <= kMaxL;
}

// x^m for x >= 0 (x = 0: 1 when m == 0, as numpy's 0.0 ** 0)
// Selects, not a branch: a divergent branch around the two transcendentals costs more than evaluating them on a safe argument
__device__ __forceinline__ float lobe(float x, float m) {
  const bool pos = x > 0.f;
  const float p = exp2f(m * log2f(pos ? x : 1.f));
  return pos ? p : (m == 0.f ? 1.f : 0.f);
}
template <int KIND>
__device__ __forceinline__ float lobe_weight(float x, float m, float dom) {
  return KIND == kDiffuse ? fmaxf(x, 0.f) * dom : lobe(x, m) * dom;
}

inline int kind_of(double v) { return v < 0.0 ? kDiffuse : kPhong; }
inline double scale_of(double v) { return v < 0.0 ? 1.0 / kPi : (v + 1.0) / (2.0 * kPi); }

}  // namespace env
}  // namespace eml
