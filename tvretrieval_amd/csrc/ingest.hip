// Feature ingest on the device ("next" row 8f-3): the dataset-side half of the reference's context collate, applied to raw
// rows as they arrive from the host.
//   reference: StartEndEvalDataset._get_item_context  xml/start_end_dataset.py:297-321  (truncate to max_ctx_len, then
//                                                      l2_normalize_np_array: x / (||x||_2 + 1e-5), utils/basic_utils.py:82-84)
//              start_end_collate / pad_sequences_1d   xml/start_end_dataset.py:346-359, utils/tensor_utils.py:5-53
//                                                      (zero padding to the batch maximum + float mask)
// The host hands over the batch's rows back to back in the STORE's dtype (f16 on disk: half the bytes over PCIe, no
// host-side conversion, no per-video Python) plus a prefix array; one launch writes the padded (n, lmax, d) tensor the
// encoder reads -- converted, normalised, zero beyond each video's length -- and the (n, lmax) mask.  HBM-bound:
// reads rows * d * 2 B, writes n * lmax * d * 4 B (f32) or * 2 B (bf16).
#include <hip/hip_fp16.h>

#include "../../include/xmlhip_ingest_tef.h"
#include "common.h"
#include "ingest_tef.h"

namespace {

template <typename S> __device__ __forceinline__ float ing_ld(const S* p);
template <> __device__ __forceinline__ float ing_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ing_ld<__half>(const __half* p) { return __half2float(*p); }

// one wave per destination row (video i, clip l).  TEF: the row is d + 2 columns wide and ends in the temporal endpoint
// columns (xmlhip_ingest_tef.h); the d feature columns are computed by the same statements either way.
template <typename S, typename D, bool TEF>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const S* __restrict__ src, const int64_t* __restrict__ row_start,
                                                          D* __restrict__ dst, float* __restrict__ mask, int n, int lmax,
                                                          int d, int max_len, float eps, int normalize,
                                                          const int32_t* __restrict__ tef_pos, const int32_t* __restrict__ tef_len,
                                                          int dst_align) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (int64_t)n * lmax) return;
  const int i = (int)(r / lmax), l = (int)(r - (int64_t)i * lmax);
  const int64_t first = row_start[i];
  const int len = (int)min((int64_t)max_len, row_start[i + 1] - first);
  D* out = dst + r * (d + (TEF ? 2 : 0));
  if (lane == 0 && mask) mask[r] = l < len ? 1.f : 0.f;
  if (l >= len) {
    if constexpr (TEF) tef_zero_row(reinterpret_cast<char*>(out), (int64_t)(d + 2) * (int64_t)sizeof(D), dst_align, lane);
    else for (int c = lane; c < d; c += 64) DT<D>::st(out + c, 0.f);
    return;
  }
  const S* px = src + (first + l) * d;
  float s = 0.f;
  if (normalize) {
    for (int c = lane; c < d; c += 64) { const float v = ing_ld<S>(px + c); s += v * v; }
    s = sqrtf(wave_sum(s)) + eps;          // l2_normalize_np_array: x / (||x|| + eps)
  }
  for (int c = lane; c < d; c += 64) {
    const float v = ing_ld<S>(px + c);
    DT<D>::st(out + c, normalize ? v / s : v);
  }
  if constexpr (TEF) {
    if (lane == 0) {
      int P, L;
      float t_st, t_ed;
      tef_place(tef_pos, tef_len, i, len, P, L);
      tef_values(P + l, L, t_st, t_ed);
      tef_store<D>(out + d, d, t_st, t_ed, dst_align);
    }
  }
}

// The vector form of ingest_rows_kernel<S, D, true> for rows of whole 16-byte pieces (src 16-byte aligned, d * sizeof(S) a
// multiple of 16, d <= 4096): the row is read ONCE, in 16-byte pieces -- lane `lane` owns pieces lane, lane + 64, ... (NP at
// the most) of VEC = 16 / sizeof(S) columns and keeps them in registers --, and stored as wide as dst_align allows.  The sum
// of squares must be the one of the element-wise kernel bit for bit (the feature columns are those of xml_ingest_rows), and
// that kernel's lane j adds columns j, j + 64, ... in this order: each wave lays its raw row out in shared memory (d * sizeof(S)
// bytes per wave, only with `normalize`) and lane j reads exactly those columns back.
template <typename S, typename D, int NP>
__global__ __launch_bounds__(256) void ingest_rows_tef_vec_kernel(const S* __restrict__ src, const int64_t* __restrict__ row_start,
                                                                  D* __restrict__ dst, float* __restrict__ mask, int n, int lmax,
                                                                  int d, int max_len, float eps, int normalize,
                                                                  const int32_t* __restrict__ tef_pos,
                                                                  const int32_t* __restrict__ tef_len, int dst_align) {
  constexpr int VEC = (int)(16 / sizeof(S));
  extern __shared__ uint4 ing_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  const bool in_grid = r < (int64_t)n * lmax;
  int i = 0, l = 0, len = 0;
  int64_t first = 0;
  if (in_grid) {
    i = (int)(r / lmax);
    l = (int)(r - (int64_t)i * lmax);
    first = row_start[i];
    len = (int)min((int64_t)max_len, row_start[i + 1] - first);
  }
  const bool live = in_grid && l < len;
  D* out = dst + r * (d + 2);
  if (in_grid && lane == 0 && mask) mask[r] = live ? 1.f : 0.f;
  if (in_grid && !live) tef_zero_row(reinterpret_cast<char*>(out), (int64_t)(d + 2) * (int64_t)sizeof(D), dst_align, lane);
  const int n_pieces = d / VEC;
  const S* px = src + (first + l) * d;
  uint4 raw[NP];
  if (live) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int p = lane + 64 * k;
      if (p < n_pieces) raw[k] = ld_global16_as1(px + (int64_t)p * VEC);
    }
  }
  float s = 0.f;
  if (normalize) {                          // (uniform over the workgroup: every wave reaches the barrier)
    uint4* row16 = ing_smem + (size_t)wave * n_pieces;
    if (live) {
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int p = lane + 64 * k;
        if (p < n_pieces) row16[p] = raw[k];
      }
    }
    __syncthreads();
    if (live) {
      const S* row = reinterpret_cast<const S*>(row16);
      for (int c = lane; c < d; c += 64) { const float v = ing_ld<S>(row + c); s += v * v; }
      s = sqrtf(wave_sum(s)) + eps;          // l2_normalize_np_array: x / (||x|| + eps)
    }
  }
  if (!live) return;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int p = lane + 64 * k;
    if (p < n_pieces) {
      float v[VEC];
      if constexpr (sizeof(S) == 2) {
        const uint32_t w[4] = {raw[k].x, raw[k].y, raw[k].z, raw[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[2 * j] = f16_bits_to_f32(w[j] & 0xffffu);
          v[2 * j + 1] = f16_bits_to_f32(w[j] >> 16);
        }
      } else {
        unpack16<float>(raw[k], v);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = normalize ? v[e] / s : v[e];
      tef_stn<D, VEC>(out + (int64_t)p * VEC, v, dst_align);
    }
  }
  if (lane == 0) {
    int P, L;
    float t_st, t_ed;
    tef_place(tef_pos, tef_len, i, len, P, L);
    tef_values(P + l, L, t_st, t_ed);
    tef_store<D>(out + d, d, t_st, t_ed, dst_align);
  }
}

}  // namespace

extern "C" int xml_ingest_rows(const void* src, int src_dt, const int64_t* row_start, void* dst, int dst_dt, float* mask, int n,
                               int lmax, int d, int max_len, float eps, int normalize, xml_stream_t stream) {
  XML_ENTER();
  if (!src || !row_start || !dst || n <= 0 || lmax <= 0 || d <= 0 || max_len <= 0) return XML_ERR_BAD_ARG;
  if ((src_dt != XML_F32 && src_dt != XML_F16) || (dst_dt != XML_F32 && dst_dt != XML_BF16)) return XML_ERR_BAD_ARG;
  const int64_t rows = (int64_t)n * lmax;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define XML_INGEST(S, D) \
  hipLaunchKernelGGL((ingest_rows_kernel<S, D, false>), grid, block, 0, st, (const S*)src, row_start, (D*)dst, mask, n, lmax, d, \
                     max_len, eps, normalize, nullptr, nullptr, 0)
  if (src_dt == XML_F32 && dst_dt == XML_F32) XML_INGEST(float, float);
  else if (src_dt == XML_F32) XML_INGEST(float, bf16_t);
  else if (dst_dt == XML_F32) XML_INGEST(__half, float);
  else XML_INGEST(__half, bf16_t);
#undef XML_INGEST
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_ingest_rows_tef(const void* src, int src_dt, const int64_t* row_start, const int32_t* tef_pos,
                                   const int32_t* tef_len, void* dst, int dst_dt, float* mask, int n, int lmax, int d, int max_len,
                                   float eps, int normalize, xml_stream_t stream) {
  XML_ENTER();
  if (!src || !row_start || !dst || n <= 0 || lmax <= 0 || d <= 0 || max_len <= 0) return XML_ERR_BAD_ARG;
  if ((src_dt != XML_F32 && src_dt != XML_F16) || (dst_dt != XML_F32 && dst_dt != XML_BF16)) return XML_ERR_BAD_ARG;
  if ((tef_pos == nullptr) != (tef_len == nullptr)) return XML_ERR_BAD_ARG;
  if (d > 4096) return XML_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)n * lmax;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int dst_align = tef_pow2_align((uintptr_t)dst, ((int64_t)d + 2) * (dst_dt == XML_F32 ? 4 : 2));
  hipStream_t st = (hipStream_t)stream;
  // rows of whole 16-byte pieces on an aligned base: one 16-byte read per piece; any other shape: element by element
  const size_t ssz = src_dt == XML_F32 ? 4 : 2;
  const bool vector = ((uintptr_t)src & 15) == 0 && ((size_t)d * ssz) % 16 == 0;
  const int need = (int)(((size_t)d * ssz / 16 + 63) / 64);           // pieces per lane
  const size_t smem = normalize ? 4 * (size_t)d * ssz : 0;            // <= 64 KiB at d = 4096, f32
#define XML_INGEST_V(S, D, NP)                                                                                              \
  hipLaunchKernelGGL((ingest_rows_tef_vec_kernel<S, D, NP>), grid, block, smem, st, (const S*)src, row_start, (D*)dst, mask, n, \
                     lmax, d, max_len, eps, normalize, tef_pos, tef_len, dst_align)
#define XML_INGEST(S, D)                                                                                                            \
  do {                                                                                                                              \
    if (!vector)                                                                                                                    \
      hipLaunchKernelGGL((ingest_rows_kernel<S, D, true>), grid, block, 0, st, (const S*)src, row_start, (D*)dst, mask, n, lmax, d, \
                         max_len, eps, normalize, tef_pos, tef_len, dst_align);                                                     \
    else if (need <= 1) XML_INGEST_V(S, D, 1);                                                                                      \
    else if (need <= 2) XML_INGEST_V(S, D, 2);                                                                                      \
    else if (need <= 4) XML_INGEST_V(S, D, 4);                                                                                      \
    else if (need <= 8) XML_INGEST_V(S, D, 8);                                                                                      \
    else XML_INGEST_V(S, D, 16);                                                                                                    \
  } while (0)
  if (src_dt == XML_F32 && dst_dt == XML_F32) XML_INGEST(float, float);
  else if (src_dt == XML_F32) XML_INGEST(float, bf16_t);
  else if (dst_dt == XML_F32) XML_INGEST(__half, float);
  else XML_INGEST(__half, bf16_t);
#undef XML_INGEST
#undef XML_INGEST_V
  XML_CHECK_LAUNCH();
  return XML_OK;
}
