// Training batches from a device-resident feature store: the dataset + collate half of the reference's training loop as
// one gather launch per stream (video, subtitle, query tokens).
//   reference: StartEndDataset.__getitem__            xml/start_end_dataset.py:94-145 (truncate to max_len, l2_normalize_np_array
//                                                      x / (||x||_2 + 1e-5), the temporal endpoint feature of lines 127-142)
//              start_end_collate / pad_sequences_1d   xml/start_end_dataset.py:346-359 (zero padding + float mask)
//              prepare_batch_inputs                   xml/start_end_dataset.py:362-370 (the host-to-device copy: gone, the rows
//                                                      already live on the device)
// The store's rows stay resident in the STORE's dtype; a step sends `n` example ids.  One wave per destination row (i, l):
// 16-byte loads of the source row into registers, the row's own sum of squares in a fixed order (lane-local in piece order,
// then the wave reduction), the scaled row stored as wide as the destination pitch allows.  HBM-bound: reads rows * d * 2 B,
// writes n * lmax * (d + 2 tef) * 4 B (f32) or * 2 B (bf16).
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

// VEC source elements per piece: 16 bytes on the vector path, one element on the scalar path
template <typename S, bool VECTOR> struct Piece { static constexpr int n = VECTOR ? (int)(16 / sizeof(S)) : 1; };

template <typename S, bool VECTOR> __device__ __forceinline__ void ld_piece(const S* p, float* v) {
  if constexpr (!VECTOR) {
    if constexpr (sizeof(S) == 2) v[0] = __half2float(*p); else v[0] = *p;
  } else if constexpr (sizeof(S) == 2) {
    const uint4 u = ld_global16(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = f16_bits_to_f32(w[k] & 0xffffu);
      v[2 * k + 1] = f16_bits_to_f32(w[k] >> 16);
    }
  } else {
    unpack16<float>(ld_global16(p), v);
  }
}

// N consecutive values at p, stored with the widest instruction that `align` (a power of two <= 16 dividing p's address and
// wave-uniform) and N * sizeof(D) allow
template <typename D, int N> __device__ __forceinline__ void st_piece(D* p, const float* v, int align) {
  if constexpr (N == 1) {
    DT<D>::st(p, v[0]);
  } else if constexpr (sizeof(D) == 4) {
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
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[(N / 2) > 2 ? 2 : 0], w[(N / 2) > 3 ? 3 : 0]);
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

// `bytes` zero bytes at p; p and bytes are multiples of `align`
__device__ __forceinline__ void zero_row(char* p, int64_t bytes, int align, int lane) {
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

// One wave per destination row r = i * lmax + l.  Lane `lane` owns pieces lane, lane + 64, ... (NP of them at most) of the
// source row and keeps them in registers between the norm and the store.
template <typename S, typename D, bool VECTOR, int NP>
__global__ __launch_bounds__(256) void gather_feature_rows_kernel(
    const S* __restrict__ src, const int64_t* __restrict__ row_start, int64_t n_items, const int32_t* __restrict__ ids, int n,
    const int32_t* __restrict__ item_of, int64_t n_examples, D* __restrict__ dst, float* __restrict__ mask,
    int32_t* __restrict__ len_out, int lmax, int d, int max_len, float eps, int normalize, int tef, int dst_align) {
  constexpr int VEC = Piece<S, VECTOR>::n;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (int64_t)n * lmax) return;
  const int i = (int)(r / lmax), l = (int)(r - (int64_t)i * lmax);
  // example -> item -> rows; anything out of range is an empty example (nothing here was ever seen by the host)
  int64_t item = ids[i];
  if (item_of) item = (item >= 0 && item < n_examples) ? (int64_t)item_of[item] : -1;
  int64_t first = 0;
  int len = 0;
  if (item >= 0 && item < n_items) {
    first = row_start[item];
    const int64_t have = row_start[item + 1] - first;
    len = (int)max((int64_t)0, min(have, (int64_t)min(max_len, lmax)));
  }
  const int64_t dd = (int64_t)d + 2 * tef;
  D* out = dst + r * dd;
  if (lane == 0) {
    if (mask) mask[r] = l < len ? 1.f : 0.f;
    if (len_out && l == 0) len_out[i] = len;
  }
  if (l >= len) {
    zero_row(reinterpret_cast<char*>(out), dd * (int64_t)sizeof(D), dst_align, lane);
    return;
  }
  const S* px = src + (first + l) * (int64_t)d;
  const int n_pieces = d / VEC;           // (vector path: d * sizeof(S) is a multiple of 16)
  float v[NP][VEC];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = lane + 64 * k;
    if (p < n_pieces) {
      ld_piece<S, VECTOR>(px + (int64_t)p * VEC, v[k]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += v[k][e] * v[k][e];
    }
  }
  if (normalize) s = sqrtf(wave_sum(s)) + eps;          // l2_normalize_np_array: x / (||x|| + eps)
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = lane + 64 * k;
    if (p < n_pieces) {
      if (normalize) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[k][e] = __fdiv_rn(v[k][e], s);
      }
      st_piece<D, VEC>(out + (int64_t)p * VEC, v[k], dst_align);
    }
  }
  if (tef && lane == 0) {
    // torch.arange(0, L, 1.0) / L and tef_st + 1.0 / L (start_end_dataset.py:130-131): an f32 division, and the f32 sum
    // with the DOUBLE quotient rounded to f32
    const float t_st = __fdiv_rn((float)l, (float)len);
    const float t_ed = __fadd_rn(t_st, (float)(1.0 / (double)len));
    DT<D>::st(out + d, t_st);
    DT<D>::st(out + d + 1, t_ed);
  }
}

__global__ __launch_bounds__(256) void gather_index_rows_kernel(const int64_t* __restrict__ src, int w, int64_t n_rows,
                                                                const int32_t* __restrict__ ids, int n, int64_t* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)n * w) return;
  const int i = (int)(t / w), c = (int)(t - (int64_t)i * w);
  const int64_t id = ids[i];
  dst[t] = (id >= 0 && id < n_rows) ? src[id * w + c] : 0;
}

// largest power of two <= 16 dividing both the base address and the row pitch
inline int pow2_align(uintptr_t base, int64_t pitch_bytes) {
  const uint64_t x = (uint64_t)base | (uint64_t)pitch_bytes | 16u;
  return (int)(x & (~x + 1));
}

}  // namespace

extern "C" int xml_gather_feature_rows(const void* src, int src_dt, const int64_t* row_start, int64_t n_items, const int32_t* ids,
                                       int n, const int32_t* item_of, int64_t n_examples, void* dst, int dst_dt, float* mask,
                                       int32_t* len_out, int lmax, int d, int max_len, float eps, int normalize, int tef,
                                       xml_stream_t stream) {
  XML_ENTER();
  if (!src || !row_start || !ids || !dst || n <= 0 || lmax <= 0 || d <= 0 || max_len <= 0 || n_items <= 0) return XML_ERR_BAD_ARG;
  if (item_of && n_examples <= 0) return XML_ERR_BAD_ARG;
  if ((src_dt != XML_F32 && src_dt != XML_F16) || (dst_dt != XML_F32 && dst_dt != XML_BF16)) return XML_ERR_BAD_ARG;
  if ((tef != 0 && tef != 1) || (normalize != 0 && normalize != 1) || eps != eps) return XML_ERR_BAD_ARG;
  if (d > 4096) return XML_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)n * lmax;
  if (rows > ((int64_t)1 << 31)) return XML_ERR_UNSUPPORTED;
  const size_t ssz = src_dt == XML_F32 ? 4 : 2, dsz = dst_dt == XML_F32 ? 4 : 2;
  const bool vector = ((uintptr_t)src & 15) == 0 && ((size_t)d * ssz) % 16 == 0;
  const int dst_align = pow2_align((uintptr_t)dst, ((int64_t)d + 2 * tef) * (int64_t)dsz);
  const int per_piece = vector ? (int)(16 / ssz) : 1;
  const int need = (d + 64 * per_piece - 1) / (64 * per_piece);       // pieces per lane
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define XML_GATHER(S, D, V, NP)                                                                                                 \
  hipLaunchKernelGGL((gather_feature_rows_kernel<S, D, V, NP>), grid, block, 0, st, (const S*)src, row_start, n_items, ids, n, \
                     item_of, n_examples, (D*)dst, mask, len_out, lmax, d, max_len, eps, normalize, tef, dst_align)
#define XML_GATHER_SD(S, D)                                      \
  do {                                                           \
    if (vector) {                                                \
      if (need <= 1) XML_GATHER(S, D, true, 1);                  \
      else if (need <= 2) XML_GATHER(S, D, true, 2);             \
      else if (need <= 4) XML_GATHER(S, D, true, 4);             \
      else if (need <= 8) XML_GATHER(S, D, true, 8);             \
      else XML_GATHER(S, D, true, (sizeof(S) == 4 ? 16 : 8));    \
    } else {                                                     \
      if (need <= 1) XML_GATHER(S, D, false, 1);                 \
      else if (need <= 4) XML_GATHER(S, D, false, 4);            \
      else if (need <= 16) XML_GATHER(S, D, false, 16);          \
      else XML_GATHER(S, D, false, 64);                          \
    }                                                            \
  } while (0)
  if (src_dt == XML_F32 && dst_dt == XML_F32) XML_GATHER_SD(float, float);
  else if (src_dt == XML_F32) XML_GATHER_SD(float, bf16_t);
  else if (dst_dt == XML_F32) XML_GATHER_SD(__half, float);
  else XML_GATHER_SD(__half, bf16_t);
#undef XML_GATHER_SD
#undef XML_GATHER
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_gather_index_rows(const int64_t* src, int w, int64_t n_rows, const int32_t* ids, int n, int64_t* dst,
                                     xml_stream_t stream) {
  XML_ENTER();
  if (!src || !ids || !dst || w <= 0 || n <= 0 || n_rows <= 0) return XML_ERR_BAD_ARG;
  if (w > 4096) return XML_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)n * w;
  hipLaunchKernelGGL(gather_index_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, w,
                     n_rows, ids, n, dst);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
