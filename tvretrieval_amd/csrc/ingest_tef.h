// The temporal endpoint columns of the ingest launches (include/xmlhip_ingest_tef.h) and stores into rows whose pitch
// (D + 2) * size is not a multiple of 16 bytes.  Shared by ingest.hip and ingest_pool.hip.
#pragma once
#include "common.h"

// largest power of two <= 16 dividing both the base address and the row pitch
inline int tef_pow2_align(uintptr_t base, int64_t pitch_bytes) {
  const uint64_t x = (uint64_t)base | (uint64_t)pitch_bytes | 16u;
  return (int)(x & (~x + 1));
}

// (P, L) of item i: its place on the time axis.  Without the arrays, or with values that do not hold the item's len clips,
// the item is a whole video: P = 0, L = len.
__device__ __forceinline__ void tef_place(const int32_t* __restrict__ tef_pos, const int32_t* __restrict__ tef_len, int i, int len,
                                          int& P, int& L) {
  P = 0;
  L = len;
  if (tef_pos) {
    const int p = tef_pos[i], t = tef_len[i];
    if (p >= 0 && (int64_t)p + len <= (int64_t)t) { P = p; L = t; }
  }
}

// torch.arange(0, L, 1.0) / L and tef_st + 1.0 / L (xml/start_end_dataset.py:130-131, 331-332): an f32 division, and the f32
// sum with the DOUBLE quotient rounded to f32 -- the arithmetic of train_batch.hip
__device__ __forceinline__ void tef_values(int pos, int L, float& t_st, float& t_ed) {
  t_st = __fdiv_rn((float)pos, (float)L);
  t_ed = __fadd_rn(t_st, (float)(1.0 / (double)L));
}

// the two columns at p = row + D, in one store where `align` (wave-uniform; divides the row's address) and D allow it
template <typename D> __device__ __forceinline__ void tef_store(D* p, int d, float t_st, float t_ed, int align) {
  if constexpr (sizeof(D) == 4) {
    if (align >= 8 && (d & 1) == 0) {
      *reinterpret_cast<uint2*>(p) = make_uint2(__float_as_uint(t_st), __float_as_uint(t_ed));
      return;
    }
  } else {
    if (align >= 4 && (d & 1) == 0) {
      *reinterpret_cast<uint32_t*>(p) = f32x2_to_bf16x2(t_st, t_ed);
      return;
    }
  }
  DT<D>::st(p, t_st);
  DT<D>::st(p + 1, t_ed);
}

// N = 4 or 8 consecutive values at p, whose address is a multiple of min(align, N * sizeof(D)) bytes (align wave-uniform, a power
// of two <= 16): the widest stores that allows
template <typename D, int N> __device__ __forceinline__ void tef_stn(D* p, const float* v, int align) {
  if constexpr (sizeof(D) == 4) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    if (align >= 16) {
#pragma unroll
      for (int k = 0; k < N; k += 4)
        *reinterpret_cast<uint4*>(q + k) = make_uint4(__float_as_uint(v[k]), __float_as_uint(v[k + 1]), __float_as_uint(v[k + 2]),
                                                      __float_as_uint(v[k + 3]));
    } else if (align >= 8) {
#pragma unroll
      for (int k = 0; k < N; k += 2) *reinterpret_cast<uint2*>(q + k) = make_uint2(__float_as_uint(v[k]), __float_as_uint(v[k + 1]));
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) q[k] = __float_as_uint(v[k]);
    }
  } else {
    uint32_t w[N / 2];
#pragma unroll
    for (int k = 0; k < N / 2; ++k) w[k] = f32x2_to_bf16x2(v[2 * k], v[2 * k + 1]);
    if (N == 8 && align >= 16) {
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[N / 2 - 2], w[N / 2 - 1]);
    } else if (align >= 8) {
#pragma unroll
      for (int k = 0; k < N / 2; k += 2) *reinterpret_cast<uint2*>(p + 2 * k) = make_uint2(w[k], w[k + 1]);
    } else if (align >= 4) {
#pragma unroll
      for (int k = 0; k < N / 2; ++k) *reinterpret_cast<uint32_t*>(p + 2 * k) = w[k];
    } else {
#pragma unroll
      for (int k = 0; k < N / 2; ++k) { p[2 * k] = (bf16_t)(w[k] & 0xffffu); p[2 * k + 1] = (bf16_t)(w[k] >> 16); }
    }
  }
}
template <typename D> __device__ __forceinline__ void tef_st8(D* p, const float* v, int align) { tef_stn<D, 8>(p, v, align); }

// `bytes` zero bytes at p; p and bytes are multiples of `align`
__device__ __forceinline__ void tef_zero_row(char* p, int64_t bytes, int align, int lane) {
  if (align >= 16) {
    for (int64_t b = (int64_t)lane * 16; b < bytes; b += 64 * 16) *reinterpret_cast<uint4*>(p + b) = make_uint4(0u, 0u, 0u, 0u);
  } else if (align >= 8) {
    for (int64_t b = (int64_t)lane * 8; b < bytes; b += 64 * 8) *reinterpret_cast<uint2*>(p + b) = make_uint2(0u, 0u);
  } else if (align >= 4) {
    for (int64_t b = (int64_t)lane * 4; b < bytes; b += 64 * 4) *reinterpret_cast<uint32_t*>(p + b) = 0u;
  } else {
    for (int64_t b = (int64_t)lane * 2; b < bytes; b += 64 * 2) *reinterpret_cast<unsigned short*>(p + b) = 0;
  }
}
