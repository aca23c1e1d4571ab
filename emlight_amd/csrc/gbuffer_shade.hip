// Object insertion, second half: light every covered pixel of a G-buffer by up to three lookups -- the irradiance map at the
// normal, the Phong map and the panorama itself at the reflection direction -- and composite the result over the photograph
// (tests/insert_oracle.py restates the definition in float64).  One thread per pixel, the three
// channels in registers; the camera ray (crop_panorama's, in the panorama's frame), the normal and the reflection in f64.
// The lookup is the mirror's of sphere_render.hip (rows clamp, columns wrap, f64 coordinates, f32 blend), started from a
// direction instead of a sphere pixel.
#include "eml_common.h"
#include "../../include/emlight_hip_ext.h"
#include "gbuffer_lookup.h"

namespace {

using namespace eml::gbuf;             // the frame, the taps and the lookup: shared with gbuffer_shade_bwd.hip

// grid (ceil(h w / 256), B)
__global__ __launch_bounds__(kThreads) void shade_kernel(const float* __restrict__ pano, int H, const float* __restrict__ ed,
                                                         int Hd, long d_stride, const float* __restrict__ eg, int Hg,
                                                         long g_stride, const float* __restrict__ normal,
                                                         const float* __restrict__ coverage, const float* __restrict__ kd,
                                                         const float* __restrict__ ks, const float* __restrict__ km, int h,
                                                         int w, double scl, double c, double s, float* __restrict__ shaded,
                                                         const float* __restrict__ background,
                                                         const float* __restrict__ exposure, float inv_gamma,
                                                         float* __restrict__ composite) {
  const int p = blockIdx.x * kThreads + threadIdx.x, hw = h * w;
  if (p >= hw) return;
  const int b = blockIdx.y, i = p / w, j = p - i * w;
  const size_t base = (size_t)b * 3 * hw + p;                            // channel 0 of this pixel in a (B, 3, h, w) tensor
  const float cov = coverage[(size_t)b * hw + p];
  float sh[3] = {0.f, 0.f, 0.f};
  const bool given = !kd && !ks && !km;                                  // composite only: shaded is the input
  if (given) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sh[ch] = shaded[base + (size_t)ch * hw];
  } else if (cov != 0.f) {
    double n[3], R[3];
    if (pixel_frame(normal, base, hw, i, j, h, w, scl, c, s, n, R)) {      // zero length (and NaN, infinite): shaded = 0
      if (kd) {
        const Taps q = direction_taps(n, Hd);
        const float* img = ed + (size_t)b * (size_t)d_stride;
        const size_t T = 2 * (size_t)Hd * Hd;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sh[ch] = __fmul_rn(kd[base + (size_t)ch * hw], lookup(img + ch * T, 2 * Hd, q));
      }
      if (ks) {
        const Taps q = direction_taps(R, Hg);
        const float* img = eg + (size_t)b * (size_t)g_stride;
        const size_t T = 2 * (size_t)Hg * Hg;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float term = __fmul_rn(ks[base + (size_t)ch * hw], lookup(img + ch * T, 2 * Hg, q));
          sh[ch] = kd ? __fadd_rn(sh[ch], term) : term;
        }
      }
      if (km) {
        const Taps q = direction_taps(R, H);
        const size_t T = 2 * (size_t)H * H;
        const float* img = pano + (size_t)b * 3 * T;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float term = __fmul_rn(km[base + (size_t)ch * hw], lookup(img + ch * T, 2 * H, q));
          sh[ch] = (kd || ks) ? __fadd_rn(sh[ch], term) : term;
        }
      }
    }
  }
  if (shaded && !given) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) shaded[base + (size_t)ch * hw] = sh[ch];
  }
  if (composite) {
    const float a = exposure[b], rest = __fsub_rn(1.f, cov);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float ldr = fminf(fmaxf(__fmul_rn(a, sh[ch]), 0.f), 1.f);          // a NaN product clamps to 0
      if (inv_gamma != 1.f) ldr = ldr > 0.f ? exp2f(__fmul_rn(log2f(ldr), inv_gamma)) : 0.f;
      const size_t o = base + (size_t)ch * hw;
      composite[o] = __fadd_rn(__fmul_rn(cov, ldr), __fmul_rn(rest, background[o]));
    }
  }
}

}  // namespace

extern "C" int eml_gbuffer_shade_f32(const float* pano, int H, const float* e_diffuse, int Hd, long d_stride,
                                     const float* e_phong, int Hg, long g_stride, const float* normal, const float* coverage,
                                     const float* kd, const float* ks, const float* km, int B, int h, int w, double fov_deg,
                                     double view_azimuth_deg, float* shaded, const float* background, const float* exposure,
                                     double gamma, float* composite, eml_stream_t stream) {
  const bool given = !kd && !ks && !km;
  if (!coverage || (!normal && !given)) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: null normal or coverage");
  if (!shaded && !composite) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: null outputs: shaded and composite");
  if (given && (!shaded || !composite))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: no coefficient: kd, ks and km are all null (composite only needs shaded "
                                 "as its input and the composite output)");
  if (kd && (!e_diffuse || Hd < 1 || Hd > kMaxG || d_stride < 6l * Hd * Hd))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: kd needs e_diffuse, 1 <= Hd <= %d and a stride of at least 3 Hd 2Hd", kMaxG);
  if (ks && (!e_phong || Hg < 1 || Hg > kMaxG || g_stride < 6l * Hg * Hg))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: ks needs e_phong, 1 <= Hg <= %d and a stride of at least 3 Hg 2Hg", kMaxG);
  if (km && (!pano || H < 1 || H > kMaxG))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: km needs pano and 1 <= H <= %d", kMaxG);
  if (composite && (!background || !exposure))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: composite needs background and exposure");
  if (!composite && (background || exposure))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: background and exposure need the composite output");
  if (composite && !(gamma > 0.0 && gamma <= 1e6))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: gamma must be in (0, 1e6] for the composite");
  if (!(fov_deg >= 0.0 && fov_deg < 180.0) || !(view_azimuth_deg - view_azimuth_deg == 0.0))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: fov_deg must be in [0, 180) and the azimuth finite");
  if (B < 0 || B > 65535) return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: B must be 0..65535 (grid.y)");
  if (h < 2 || w < 2 || (long)h * w > (1l << 29))
    return eml::fail(EML_EINVAL, "eml_gbuffer_shade_f32: image size: h, w >= 2 and h w <= 2^29, got %d x %d", h, w);
  if (B == 0) return EML_OK;
  const double az = view_azimuth_deg * (kPi / 180.0);
  const double scl = fov_deg > 0.0 ? tan(fov_deg * (kPi / 180.0) * 0.5) : 0.0;
  hipLaunchKernelGGL(shade_kernel, dim3((h * w + kThreads - 1) / kThreads, B), dim3(kThreads), 0, (hipStream_t)stream, pano, H,
                     e_diffuse, Hd, d_stride, e_phong, Hg, g_stride, normal, coverage, kd, ks, km, h, w, scl, cos(az), sin(az),
                     shaded, background, exposure, composite ? (float)(1.0 / gamma) : 1.f, composite);
  return eml::check_launch("eml_gbuffer_shade_f32");
}
