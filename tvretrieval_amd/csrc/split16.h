// Per-element arithmetic of the split-f16 form (split16.hip's header comment), shared by the row / weight splitters
// (split16.hip) and the exact-rank update kernel (index_update_exact.hip): a slot written by xml_index_put_rows_exact holds
// bitwise what xml_split_f16_rows leaves for the same row because both run these functions.
#pragma once
#include "common.h"

__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }   // e in [-126, 127]

// power-of-two scale that maps a row / tensor maximum m into [2^13, 2^14); m == 0 or non-finite -> 1
__device__ __forceinline__ int scale_log2_of(float m) {
  if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
  int q;
  (void)frexpf(m, &q);                    // m = f 2^q, f in [0.5, 1)
  const int e = 14 - q;
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}

// 8 consecutive elements -> 8 hi halves + 8 lo halves (raw bits packed two per word), sum of squares of the hi residual
__device__ __forceinline__ float split8(const float* f, float s, uint4& hi, uint4& lo) {
  uint32_t h[8], l[8];
  float e2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float xs = f[i] * s;                        // exact (power of two) unless it over/underflows
    h[i] = f32_to_f16_bits_ftz(xs);
    const float r = xs - f16_bits_to_f32(h[i]);       // exact in f32: |r| <= ulp_f16(xs) / 2 (or xs itself when flushed)
    l[i] = f32_to_f16_bits_ftz(r);
    e2 += r * r;
  }
  hi = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  lo = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
  return e2;
}

__device__ __forceinline__ float row_absmax(const float* px, int k, int lane) {
  float m = 0.f;
  for (int c = lane * 8; c < k; c += 64 * 8) {
    float f[8];
    ld8<float>(px + c, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(f[i]));
  }
  return wave_max(m);
}
