// Dropout of the dense layers' new channels (DenseNet.py:50-55, F.dropout after conv2): a stateless counter-based mask.
//
// The draw of output channel c (0..11) of global dense layer `layer` at the flat pixel (b*H + h)*W + w is word c % 4 of
//     Philox-4x32-10(counter = (pixel, c / 4, layer, 0), key = (seed low 32 bits, seed high 32 bits))
// and the element is kept iff draw >= floor(p * 2^32) (64-bit compare: p == 1 drops everything); kept values are scaled by
// 1 / (1 - p).  The mask is a function of (seed, layer, pixel, channel) only -- not of the grid, the tile, the band or the
// kernel variant -- so the forward kernels and every backward recompute the same bits from the same key: nothing is stored,
// nothing is written back.  Restated in numpy by tests/dropout_hash.py.
#pragma once

#include <hip/hip_runtime.h>

namespace eml {

struct DropKey {                // passed to the kernels by value
  unsigned k0, k1;              // 64-bit seed
  unsigned long long thr;       // floor(p * 2^32), 2^32 for p == 1
  unsigned layer;               // global dense-layer index (0..47 in EMLight)
  float scale;                  // 1 / (1 - p) (0 for p == 1)
};

// Random123's Philox-4x32 with 10 rounds (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments
// 0x9E3779B9 / 0xBB67AE85
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    if (i) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x, p1 = (unsigned long long)0xCD9E8D57u * c.z;
    c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
  }
  return c;
}

// the four draws of channels 4grp .. 4grp + 3 at `pixel`
__device__ __forceinline__ uint4 drop_draws(const DropKey& k, unsigned pixel, unsigned grp) {
  return philox4x32_10(make_uint4(pixel, grp, k.layer, 0u), k.k0, k.k1);
}

__device__ __forceinline__ float drop_apply(const DropKey& k, unsigned draw, float v) {
  return (unsigned long long)draw >= k.thr ? v * k.scale : 0.f;
}

__device__ __forceinline__ unsigned draw_word(const uint4& d, int w) {
  return w == 0 ? d.x : w == 1 ? d.y : w == 2 ? d.z : d.w;
}

// v holds channels 4grp .. 4grp + 3 of `pixel`
__device__ __forceinline__ float4 drop4(const DropKey& k, unsigned pixel, unsigned grp, float4 v) {
  const uint4 d = drop_draws(k, pixel, grp);
  return make_float4(drop_apply(k, d.x, v.x), drop_apply(k, d.y, v.y), drop_apply(k, d.z, v.z), drop_apply(k, d.w, v.w));
}

}  // namespace eml

// host side: the key of a launch (p validated by the caller)
inline eml::DropKey eml_drop_key(unsigned long long seed, int layer, double p) {
  eml::DropKey k;
  k.k0 = (unsigned)(seed & 0xFFFFFFFFull);
  k.k1 = (unsigned)(seed >> 32);
  k.thr = p >= 1.0 ? (1ull << 32) : (unsigned long long)(p * 4294967296.0);   // floor: p * 2^32 is exact in double
  k.layer = (unsigned)layer;
  k.scale = p >= 1.0 ? 0.f : (float)(1.0 / (1.0 - p));
  return k;
}
