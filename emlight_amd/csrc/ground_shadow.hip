// Object insertion: the shadow the inserted object casts on a ground plane (tests/shadow_oracle.py
// restates the definition in float64).  A diffuse shadow catcher: for every photograph pixel that shows the plane, the
// cosine-weighted irradiance from the panorama with the occluder spheres in the way, over the irradiance without them.
// Visibility is a binary test per (pixel, texel, sphere): no matrix unit takes this sum.  Three launches:
//   1. weight_kernel: wp[b,t,ch] = pano[b,ch,t] max(n.omega_t, 0) dOmega_t in f64 (the per-texel terms of E0, kept), and the
//      256-texel partial sums of them (fixed-order tree);
//   2. e0_kernel: E0[b,ch] from the partials, one block per image, fixed order;
//   3. shadow_kernel: one thread per pixel, 8 x 8 pixels per wave, 16 x 16 per block.  D = sum of wp over the blocked texels.
// Geometry, the blocked test and all sums in f64; one rounding to f32 at the end.  No atomics.  A pixel adds its blocked texels
// rows ascending, columns ascending, each texel once however many spheres block it: the order does not depend on the tile the
// pixel is in, on the order of the spheres, nor on the batch.
// Culling: from a hit point p, sphere k blocks only directions within asin(r / |oc|) of oc = c_k - p.  Each lane turns that cap
// into a row range and a column interval (all columns when the cap holds a pole); the wave takes the hull of its 64 lanes
// (phase A) and tests only the texels of that box, less the rows that lie wholly under the plane's horizon (their terms are
// exactly 0).  The box is padded, so it only ever skips texels whose test is false.  Phase B walks the rows 64 columns at a
// time: the spheres whose box meets the chunk set one bit per blocked texel in a 64-bit word per lane, branch-free (the sines
// and cosines come from LDS as broadcasts); the chunk's 192 terms are fetched by one coalesced load that is in flight
// meanwhile, go through a per-wave LDS slot, and are added under the bits.
#include "ground_shadow_walk.h"
#include "../../include/emlight_hip_ext.h"

namespace {

using namespace shadow;

// grid (ceil(w / 16), ceil(h / 16), B); dynamic LDS: walk_lds_bytes(H).  The walk itself is ground_shadow_walk.h's, shared
// with the adjoint.
__global__ __launch_bounds__(kThreads) void shadow_kernel(const double* __restrict__ wp, const double* __restrict__ e0, int H,
                                                          const float* __restrict__ plane, int plane_stride,
                                                          const float* __restrict__ occluders, int K, int h, int w, double scl,
                                                          double c, double s, const float* __restrict__ image,
                                                          float* __restrict__ ratio, float* __restrict__ shadowed,
                                                          unsigned long long* __restrict__ counts) {  // counts: EML_GROUND_SHADOW_COUNTS
  extern __shared__ double lds[];
  __shared__ int box[kThreads / 64][kMaxK][4];                             // per wave and sphere: R0, R1, c0, nc
  __shared__ double stage[kThreads / 64][3 * 64];                          // per wave: the terms of the chunk being added
  const Pixel p = walk(wp, H, plane, plane_stride, occluders, K, h, w, scl, c, s, lds, box, stage, counts,
                       [](int, int, int, unsigned long long) {});
  if (!p.in_image) return;
  const int b = blockIdx.z;
  const size_t hw = (size_t)h * w, base = (size_t)b * 3 * hw + (size_t)p.i * w + p.j;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float f = (float)ratio_value(p, ch, e0[b * 3 + ch]);
    if (ratio) ratio[base + ch * hw] = f;
    if (shadowed) shadowed[base + ch * hw] = __fmul_rn(image[base + ch * hw], f);
  }
}

}  // namespace

// doubles: E0 (3 B), the partials (3 B blocks), wp (3 B H W); a build with -DEML_GROUND_SHADOW_COUNTS (tools/bench_ground_shadow.py
// measures the culling with one) appends one 64-bit count of executed tests per wave (4 B tiles)
extern "C" size_t eml_ground_shadow_work_floats(int B, int H, int h, int w, int K) {
  if (!sizes_ok(B, H, h, w, K) || B == 0) return 0;
  size_t doubles = (size_t)B * 3 * (1 + weight_blocks(H) + (size_t)2 * H * H);
#ifdef EML_GROUND_SHADOW_COUNTS
  doubles += (size_t)B * tiles(h, w) * 4;
#endif
  return 2 * doubles;
}

extern "C" int eml_ground_shadow_f32(const float* pano, int B, int H, int W, const float* plane, int plane_stride,
                                     const float* occluders, int K, int h, int w, double fov_deg, double view_azimuth_deg,
                                     const float* image, float* ratio, float* shadowed, float* work, eml_stream_t stream) {
  if (!pano || !plane || !work) return eml::fail(EML_EINVAL, "eml_ground_shadow_f32: null pano, plane or work");
  if (!ratio && !shadowed) return eml::fail(EML_EINVAL, "eml_ground_shadow_f32: null outputs: ratio and shadowed");
  if ((image != nullptr) != (shadowed != nullptr))
    return eml::fail(EML_EINVAL, "eml_ground_shadow_f32: image and shadowed go together (shadowed = image * ratio)");
  if (int rc = refuse_geometry("eml_ground_shadow_f32", work, B, H, W, plane_stride, occluders, K, h, w, fov_deg, view_azimuth_deg))
    return rc;
  if (B == 0) return EML_OK;
  double* e0 = reinterpret_cast<double*>(work);
  double* partial = e0 + (size_t)3 * B;
  double* wp = partial + (size_t)3 * B * weight_blocks(H);
#ifdef EML_GROUND_SHADOW_COUNTS
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(wp + (size_t)3 * B * 2 * H * H);
#else
  unsigned long long* counts = nullptr;
#endif
  const double az = view_azimuth_deg * (kPi / 180.0), scl = tan(fov_deg * (kPi / 180.0) * 0.5);
  const double c = cos(az), s = sin(az);
  hipStream_t q = (hipStream_t)stream;
  if (int rc = enqueue_e0("eml_ground_shadow_f32", pano, B, H, plane, plane_stride, c, s, e0, partial, wp, q)) return rc;
  hipLaunchKernelGGL(shadow_kernel, dim3((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, B), dim3(kThreads), walk_lds_bytes(H), q,
                     wp, e0, H, plane, plane_stride, occluders, K, h, w, scl, c, s, image, ratio, shadowed, counts);
  return eml::check_launch("eml_ground_shadow_f32", "pixels");
}
