// Feature ingest from frame- and word-level stores (include/xmlhip_ingest_pool.h; tvretrieval_amd/ingest.py PooledStore;
// DESIGN.md section 23): xml_ingest_rows with a segmented reduction in front of it.  Replaces three offline numpy + h5py
// passes of the reference:
//   utils/video_feature/convert_feature_frm_to_clip.py:12-37        max / mean over the frames of a clip
//   utils/video_feature/normalize_and_concat.py:24-29               x / (||x|| + 1e-5) per source, ResNet || I3D
//   utils/text_feature/convert_sub_feature_word_to_clip.py:75-86    max / mean over the words of a clip's sentences, zero rows
// and then does what ingest.hip does: truncate to max_ctx_len, the dataset's x / (||x|| + 1e-5) over the whole row
// (xml/start_end_dataset.py:297-321), zero padding and the float mask (utils/tensor_utils.py:5-53).
//
// One wave per destination row (video i, clip l), grid-stride over the n * lmax rows.  The pooled row lives in REGISTERS: the
// row of up to 4096 columns is cut into chunks of 512, lane k of chunk c owns the 8 columns c * 512 + 8 k ..; a chunk is
// one 16-byte load per lane and source row for f16 (two for f32) and one 16-byte store (two for f32).  Every source row of a
// range is read once; the per-source norm, the row norm and the conversion work on the registers -- no second read, no
// intermediate in memory.  The loop over a clip's source rows issues the loads of all chunks of one row back to back (6
// independent KiB per wave at 2048 + 1024 columns).  Source offsets are 64-bit: a frame store is corpus-sized.  HBM-bound:
// reads (source rows named by the batch) * d * 2 B, writes n * lmax * (d_a + d_b) * 4 B (f32) or * 2 B (bf16).
#include <hip/hip_fp16.h>

#include "../../include/xmlhip_train_pool.h"
#include "common.h"
#include "ingest_tef.h"

namespace {

constexpr int POOL_CHUNK = 512;       // columns per chunk: 64 lanes x 8
constexpr int POOL_MAX_D = 4096;

// 8 consecutive source elements as floats; p is 16-byte aligned (the vector path only)
__device__ __forceinline__ void pool_ld8(const char* p, bool f16, float* v) {
  if (f16) {
    const uint4 u = ld_global16_as1(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = f16_bits_to_f32(w[j] & 0xffffu);
      v[2 * j + 1] = f16_bits_to_f32(w[j] >> 16);
    }
  } else {
    unpack16<float>(ld_global16_as1(p), v);
    unpack16<float>(ld_global16_as1(p + 16), v + 4);
  }
}
__device__ __forceinline__ float pool_ld1(const char* base, bool f16, int64_t elem) {
  return f16 ? __half2float(reinterpret_cast<const __half*>(base)[elem]) : reinterpret_cast<const float*>(base)[elem];
}

// the valid, non-empty range of clip row r in a source of `rows` rows: first row and row count (0: nothing is read)
__device__ __forceinline__ void pool_range(const int64_t* __restrict__ seg, int64_t r, int64_t rows, int64_t& lo, int& cnt) {
  lo = seg[2 * r];
  const int64_t hi = seg[2 * r + 1];
  const bool ok = lo >= 0 && lo < hi && hi <= rows && hi - lo <= (int64_t)0x7fffffff;
  cnt = ok ? (int)(hi - lo) : 0;
  if (!ok) lo = 0;
}

// NCH: chunks of 512 columns the row may span (d_a + d_b <= NCH * 512).  VEC: d_a % 8 == 0, d_b % 8 == 0 and all of src_a,
// src_b, dst 16-byte aligned -- a lane's 8 columns belong to one source and move as 16-byte pieces.  TEF
// (xmlhip_ingest_tef.h): the row is d_a + d_b + 2 columns wide and ends in the temporal endpoint columns; VEC then asks nothing of
// dst (its pitch is never a multiple of 16): the loads are the same 16-byte pieces, the stores as wide as dst_align allows.  The
// feature columns are computed by the same statements either way.  GATHER (xmlhip_train_pool.h): the training gather over a RESIDENT
// store -- row_start is the store's clip_start over n_items items and batch position i names its item through ids -> item_of;
// only how `first` and `len` are found differs (three dependent wave-uniform loads, as in train_batch.hip), the row body is the
// one below.  Without GATHER the five gather arguments are not read.
template <typename D, int NCH, bool VEC, bool TEF, bool GATHER>
__global__ __launch_bounds__(256) void ingest_pool_kernel(
    const char* __restrict__ src_a, int f16_a, int64_t rows_a, int d_a, const int64_t* __restrict__ seg_a, int norm_a,
    const char* __restrict__ src_b, int f16_b, int64_t rows_b, int d_b, const int64_t* __restrict__ seg_b, int norm_b,
    const int64_t* __restrict__ row_start, D* __restrict__ dst, float* __restrict__ mask, float* __restrict__ filled, int n,
    int lmax, int max_len, float eps, int normalize, int pool_mean, const int32_t* __restrict__ tef_pos,
    const int32_t* __restrict__ tef_len, int dst_align, int64_t n_items, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ item_of, int64_t n_examples, int32_t* __restrict__ len_out) {
  const int lane = threadIdx.x & 63;
  const int d = d_a + d_b;
  const int64_t total = (int64_t)n * lmax;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < total; r += (int64_t)gridDim.x * 4) {
    const int i = (int)(r / lmax), l = (int)(r - (int64_t)i * lmax);
    int64_t first;
    int len;
    if constexpr (GATHER) {
      // example -> item -> clip rows; anything out of range is an empty example (train_batch.hip)
      int64_t item = ids[i];
      if (item_of) item = (item >= 0 && item < n_examples) ? (int64_t)item_of[item] : -1;
      first = 0;
      len = 0;
      if (item >= 0 && item < n_items) {
        first = row_start[item];
        len = (int)max((int64_t)0, min(row_start[item + 1] - first, (int64_t)min(max_len, lmax)));
      }
      if (lane == 0 && l == 0 && len_out) len_out[i] = len;
    } else {
      first = row_start[i];
      len = (int)min((int64_t)max_len, row_start[i + 1] - first);
    }
    D* out = dst + r * (d + (TEF ? 2 : 0));
    if (l >= len) {
      if (lane == 0) {
        if (mask) mask[r] = 0.f;
        if (filled) filled[r] = 0.f;
      }
      if (TEF) {
        tef_zero_row(reinterpret_cast<char*>(out), (int64_t)(d + 2) * (int64_t)sizeof(D), dst_align, lane);
      } else if (VEC) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = lane * 8; c < d; c += POOL_CHUNK) st8<D>(out + c, z);
      } else {
        for (int c = lane; c < d; c += 64) DT<D>::st(out + c, 0.f);
      }
      continue;
    }
    int64_t lo_a, lo_b = 0;
    int cnt_a, cnt_b = 0;
    pool_range(seg_a, first + l, rows_a, lo_a, cnt_a);
    if (d_b > 0) pool_range(seg_b, first + l, rows_b, lo_b, cnt_b);
    if (lane == 0) {
      if (mask) mask[r] = 1.f;
      if (filled) filled[r] = (cnt_a > 0 || cnt_b > 0) ? 1.f : 0.f;
    }
    const int tmax = max(cnt_a, cnt_b);
    const float init_a = (pool_mean || cnt_a == 0) ? 0.f : -INFINITY, init_b = (pool_mean || cnt_b == 0) ? 0.f : -INFINITY;
    float acc[NCH][8];

    if (VEC) {
      // per chunk: this lane's 8 columns start at c0; they belong to source b when c0 >= d_a
      const char* p[NCH];
      int step[NCH], cnt[NCH];
      bool f16[NCH];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c0 = ch * POOL_CHUNK + lane * 8;
        const bool in_b = c0 >= d_a;
        const int es = (in_b ? f16_b : f16_a) ? 2 : 4;
        f16[ch] = in_b ? f16_b : f16_a;
        cnt[ch] = c0 < d ? (in_b ? cnt_b : cnt_a) : 0;
        step[ch] = (in_b ? d_b : d_a) * es;
        // 64-bit element offset: (first source row) * (row width) + (column inside the source)
        const int64_t e = in_b ? lo_b * d_b + (c0 - d_a) : lo_a * d_a + c0;
        p[ch] = (in_b ? src_b : src_a) + (cnt[ch] > 0 ? e * es : 0);
        const float init = in_b ? init_b : init_a;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ch][j] = cnt[ch] > 0 ? init : 0.f;
      }
      for (int t = 0; t < tmax; ++t) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (t < cnt[ch]) {
            float v[8];
            pool_ld8(p[ch], f16[ch], v);
            p[ch] += step[ch];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[ch][j] = pool_mean ? acc[ch][j] + v[j] : fmaxf(acc[ch][j], v[j]);
          }
        }
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = ch * POOL_CHUNK + lane * 8 + j;
          acc[ch][j] = c < d ? (c >= d_a ? init_b : init_a) : 0.f;
        }
      }
      for (int t = 0; t < tmax; ++t) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (ch * POOL_CHUNK < d) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int c = ch * POOL_CHUNK + lane * 8 + j;
              const bool in_b = c >= d_a;
              if (c < d && t < (in_b ? cnt_b : cnt_a)) {
                const float v = in_b ? pool_ld1(src_b, f16_b, (lo_b + t) * d_b + (c - d_a))
                                     : pool_ld1(src_a, f16_a, (lo_a + t) * d_a + c);
                acc[ch][j] = pool_mean ? acc[ch][j] + v : fmaxf(acc[ch][j], v);
              }
            }
          }
        }
      }
    }

    // mean: the f32 sum in row order over the count (an empty block stays zero)
    if (pool_mean) {
      const float na = (float)max(cnt_a, 1), nb = (float)max(cnt_b, 1);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = ch * POOL_CHUNK + lane * 8 + j;
          acc[ch][j] = acc[ch][j] / (c >= d_a ? nb : na);
        }
      }
    }
    // stage 2 of the reference: x / (||x|| + eps) per source (columns past d hold zeros and add nothing)
    if (norm_a || norm_b) {
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = ch * POOL_CHUNK + lane * 8 + j;
          const float q = acc[ch][j] * acc[ch][j];
          if (c >= d_a) sb += q; else sa += q;
        }
      }
      sa = norm_a ? sqrtf(wave_sum(sa)) + eps : 1.f;
      sb = norm_b ? sqrtf(wave_sum(sb)) + eps : 1.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = ch * POOL_CHUNK + lane * 8 + j;
          const bool in_b = c >= d_a;
          if (in_b ? norm_b : norm_a) acc[ch][j] = acc[ch][j] / (in_b ? sb : sa);
        }
      }
    }
    // the dataset's normalisation over the whole concatenated row (l2_normalize_np_array)
    if (normalize) {
      float s = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += acc[ch][j] * acc[ch][j];
      }
      s = sqrtf(wave_sum(s)) + eps;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[ch][j] = acc[ch][j] / s;
      }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = ch * POOL_CHUNK + lane * 8;
      if (VEC && TEF) {
        if (c0 < d) tef_st8<D>(out + c0, acc[ch], dst_align);
      } else if (VEC) {
        if (c0 < d) st8<D>(out + c0, acc[ch]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < d) DT<D>::st(out + c0 + j, acc[ch][j]);
      }
    }
    if (TEF && lane == 0) {
      int P, L;
      float t_st, t_ed;
      tef_place(tef_pos, tef_len, i, len, P, L);
      tef_values(P + l, L, t_st, t_ed);
      tef_store<D>(out + d, d, t_st, t_ed, dst_align);
    }
  }
}

template <typename D, int NCH, bool VEC, bool TEF, bool GATHER>
void launch_pool(dim3 grid, hipStream_t st, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a,
                 int norm_a, const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                 const int64_t* row_start, void* dst, float* mask, float* filled, int n, int lmax, int max_len, float eps,
                 int normalize, int pool, const int32_t* tef_pos, const int32_t* tef_len, int dst_align, int64_t n_items,
                 const int32_t* ids, const int32_t* item_of, int64_t n_examples, int32_t* len_out) {
  hipLaunchKernelGGL((ingest_pool_kernel<D, NCH, VEC, TEF, GATHER>), grid, dim3(256), 0, st, (const char*)src_a, (int)(src_dt_a == XML_F16),
                     rows_a, d_a, seg_a, norm_a, (const char*)src_b, (int)(src_dt_b == XML_F16), rows_b, d_b, seg_b, norm_b,
                     row_start, (D*)dst, mask, filled, n, lmax, max_len, eps, normalize, (int)(pool == XML_POOL_MEAN),
                     tef_pos, tef_len, dst_align, n_items, ids, item_of, n_examples, len_out);
}

// The launch both entries end in.  gather: row_start is clip_start over n_items items, ids / item_of / n_examples / len_out as in
// xml_gather_feature_rows; otherwise they are unused.
int pool_dispatch(bool tef, bool gather, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a, int norm_a,
                  const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                  const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled, int n, int lmax, int max_len, float eps,
                  int normalize, int pool, const int32_t* tef_pos, const int32_t* tef_len, int64_t n_items, const int32_t* ids,
                  const int32_t* item_of, int64_t n_examples, int32_t* len_out, xml_stream_t stream) {
  const int d = d_a + d_b;
  // with the endpoint columns the destination decides the store width only, never the load width
  const uintptr_t vec_ptrs = reinterpret_cast<uintptr_t>(src_a) | reinterpret_cast<uintptr_t>(src_b) |
                             (tef ? (uintptr_t)0 : reinterpret_cast<uintptr_t>(dst));
  const bool vec = d_a % 8 == 0 && d_b % 8 == 0 && (vec_ptrs & 15) == 0;
  const int dst_align = tef ? tef_pow2_align(reinterpret_cast<uintptr_t>(dst), ((int64_t)d + 2) * (dst_dt == XML_F32 ? 4 : 2)) : 0;
  // memory-bound: at most 256 CUs x 8 workgroups, the rest by grid stride
  const int64_t rows = (int64_t)n * lmax;
  const dim3 grid((unsigned)min((rows + 3) / 4, (int64_t)2048));
  hipStream_t st = (hipStream_t)stream;
#define XML_POOL(D, NCH, VEC, TEF, G) \
  launch_pool<D, NCH, VEC, TEF, G>(grid, st, src_a, src_dt_a, rows_a, d_a, seg_a, norm_a, src_b, src_dt_b, rows_b, d_b, seg_b, norm_b, \
                                   row_start, dst, mask, filled, n, lmax, max_len, eps, normalize, pool, tef_pos, tef_len, dst_align, \
                                   n_items, ids, item_of, n_examples, len_out)
#define XML_POOL_W(D, VEC, TEF, G)                 \
  do {                                     \
    if (d <= 2 * POOL_CHUNK) XML_POOL(D, 2, VEC, TEF, G); \
    else if (d <= 6 * POOL_CHUNK) XML_POOL(D, 6, VEC, TEF, G); \
    else XML_POOL(D, 8, VEC, TEF, G);              \
  } while (0)
#define XML_POOL_V(D, TEF, G) \
  do { if (vec) XML_POOL_W(D, true, TEF, G); else XML_POOL_W(D, false, TEF, G); } while (0)
#define XML_POOL_T(D, G) \
  do { if (tef) XML_POOL_V(D, true, G); else XML_POOL_V(D, false, G); } while (0)
  if (dst_dt == XML_F32) { if (gather) XML_POOL_T(float, true); else XML_POOL_T(float, false); }
  else { if (gather) XML_POOL_T(bf16_t, true); else XML_POOL_T(bf16_t, false); }
#undef XML_POOL_T
#undef XML_POOL_V
#undef XML_POOL_W
#undef XML_POOL
  XML_CHECK_LAUNCH();
  return XML_OK;
}

// tef: the entry with the endpoint columns (tef_pos / tef_len may still be NULL)
int ingest_pool_entry(bool tef, int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a, int norm_a,
                      const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                      const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled, int n, int lmax, int max_len,
                      float eps, int normalize, int pool, const int32_t* tef_pos, const int32_t* tef_len, xml_stream_t stream) {

  XML_ENTER();
  if (n_src != 1 && n_src != 2) return XML_ERR_BAD_ARG;
  if (!src_a || !seg_a || !row_start || !dst || n <= 0 || lmax <= 0 || max_len <= 0 || d_a <= 0 || rows_a <= 0) return XML_ERR_BAD_ARG;
  if (src_dt_a != XML_F32 && src_dt_a != XML_F16) return XML_ERR_BAD_ARG;
  if (n_src == 2) {
    if (!src_b || !seg_b || d_b <= 0 || rows_b <= 0) return XML_ERR_BAD_ARG;
    if (src_dt_b != XML_F32 && src_dt_b != XML_F16) return XML_ERR_BAD_ARG;
  } else {                            // one source: the _b arguments are ignored
    src_b = nullptr; seg_b = nullptr; d_b = 0; rows_b = 0; norm_b = 0; src_dt_b = src_dt_a;
  }
  if (dst_dt != XML_F32 && dst_dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (pool != XML_POOL_MAX && pool != XML_POOL_MEAN) return XML_ERR_BAD_ARG;
  if ((tef_pos == nullptr) != (tef_len == nullptr)) return XML_ERR_BAD_ARG;
  if ((int64_t)d_a + d_b > POOL_MAX_D) return XML_ERR_UNSUPPORTED;
  return pool_dispatch(tef, false, src_a, src_dt_a, rows_a, d_a, seg_a, norm_a, src_b, src_dt_b, rows_b, d_b, seg_b, norm_b, row_start,
                       dst, dst_dt, mask, filled, n, lmax, max_len, eps, normalize, pool, tef_pos, tef_len, 0, nullptr, nullptr, 0,
                       nullptr, stream);
}

}  // namespace

extern "C" int xml_ingest_pool_rows(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a,
                                    int norm_a, const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b,
                                    int norm_b, const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled,
                                    int n, int lmax, int max_len, float eps, int normalize, int pool, xml_stream_t stream) {
  return ingest_pool_entry(false, n_src, src_a, src_dt_a, rows_a, d_a, seg_a, norm_a, src_b, src_dt_b, rows_b, d_b, seg_b, norm_b,
                           row_start, dst, dst_dt, mask, filled, n, lmax, max_len, eps, normalize, pool, nullptr, nullptr, stream);
}

extern "C" int xml_ingest_pool_rows_tef(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a,
                                        int norm_a, const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b,
                                        int norm_b, const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled,
                                        int n, int lmax, int max_len, float eps, int normalize, int pool, const int32_t* tef_pos,
                                        const int32_t* tef_len, xml_stream_t stream) {
  return ingest_pool_entry(true, n_src, src_a, src_dt_a, rows_a, d_a, seg_a, norm_a, src_b, src_dt_b, rows_b, d_b, seg_b, norm_b,
                           row_start, dst, dst_dt, mask, filled, n, lmax, max_len, eps, normalize, pool, tef_pos, tef_len, stream);
}

// include/xmlhip_train_pool.h: the same launch over a resident store, the batch named by example ids
extern "C" int xml_gather_pool_feature_rows(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a,
                                            int norm_a, const void* src_b, int src_dt_b, int64_t rows_b, int d_b,
                                            const int64_t* seg_b, int norm_b, const int64_t* clip_start, int64_t n_items,
                                            const int32_t* ids, int n, const int32_t* item_of, int64_t n_examples, void* dst,
                                            int dst_dt, float* mask, int32_t* len_out, int lmax, int max_len, float eps,
                                            int normalize, int pool, int tef, xml_stream_t stream) {
  XML_ENTER();
  if (n_src != 1 && n_src != 2) return XML_ERR_BAD_ARG;
  if (!src_a || !seg_a || !clip_start || !ids || !dst || n <= 0 || lmax <= 0 || max_len <= 0 || d_a <= 0 || rows_a <= 0 || n_items <= 0)
    return XML_ERR_BAD_ARG;
  if (item_of && n_examples <= 0) return XML_ERR_BAD_ARG;
  if (src_dt_a != XML_F32 && src_dt_a != XML_F16) return XML_ERR_BAD_ARG;
  if (n_src == 2) {
    if (!src_b || !seg_b || d_b <= 0 || rows_b <= 0) return XML_ERR_BAD_ARG;
    if (src_dt_b != XML_F32 && src_dt_b != XML_F16) return XML_ERR_BAD_ARG;
  } else {                            // one source: the _b arguments are ignored
    src_b = nullptr; seg_b = nullptr; d_b = 0; rows_b = 0; norm_b = 0; src_dt_b = src_dt_a;
  }
  if (dst_dt != XML_F32 && dst_dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (pool != XML_POOL_MAX && pool != XML_POOL_MEAN) return XML_ERR_BAD_ARG;
  if ((tef != 0 && tef != 1) || (normalize != 0 && normalize != 1) || eps != eps) return XML_ERR_BAD_ARG;
  if ((int64_t)d_a + d_b > POOL_MAX_D) return XML_ERR_UNSUPPORTED;
  return pool_dispatch(tef != 0, true, src_a, src_dt_a, rows_a, d_a, seg_a, norm_a, src_b, src_dt_b, rows_b, d_b, seg_b, norm_b,
                       clip_start, dst, dst_dt, mask, nullptr, n, lmax, max_len, eps, normalize, pool, nullptr, nullptr, n_items, ids,
                       item_of, n_examples, len_out, stream);
}
