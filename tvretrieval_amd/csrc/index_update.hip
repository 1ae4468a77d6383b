// In-place updates of a resident corpus index with a fixed number of video SLOTS (inference.MutableCorpusIndex, DESIGN.md
// section 20).  xml_index_put_rows scatters one encoded context batch to its slots and leaves there what the one-shot build
// leaves for the same batch (inference._fill_index_rows + the packing pass of build_corpus_index(length_buckets=False)):
//   K6 operand   the L2-normalised feat1 rows (l2norm.h's arithmetic, bitwise), in K6's slice-major tile image
//                ([tile of 256 rows][64-byte K slice][row][64 B], index_build.hip: a tile holds two 128-clip slots) or
//                row-major where the tiled kernel does not take the shape; zero rows beyond the batch's padded width lb
//   feat2        the encoder's rows [0, lb) (padded positions included), zero rows [lb, lpad)
//   mask         the batch's f32 mask, 0 beyond lb; mask bits: 4 words per slot and modality (bit c = mask[c] != 0)
//   vlen         max over modalities of (last valid clip + 1), 0 -> l_ref, clamped to l_ref (CorpusIndex.set_valid_lengths)
//   slot_ids     the caller's id of the slot's video; live: the slot's bit set
// Every one of the slot's lpad rows is written, so nothing of a previous occupant survives a replace.
// xml_index_clear_rows frees slots: live bit cleared, mask rows and mask bits zeroed, vlen = l_ref (the feature rows stay).
// Pure streaming: half a wave per clip row, 16-byte loads and stores; one launch for both modalities.  Slots of one call are
// distinct (the host slot table guarantees it), several of them may share a live word: atomicOr / atomicAnd.
#include "l2norm.h"

namespace {

template <typename T, bool TILED>
__global__ __launch_bounds__(256) void index_put_rows_kernel(
    const T* __restrict__ f1_a, const T* __restrict__ f2_a, const float* __restrict__ mask_a,
    const T* __restrict__ f1_b, const T* __restrict__ f2_b, const float* __restrict__ mask_b,
    const int32_t* __restrict__ slots, const int32_t* __restrict__ ids,
    T* __restrict__ k6_a, T* __restrict__ feat2_a, float* __restrict__ imask_a, int32_t* __restrict__ bits_a,
    T* __restrict__ k6_b, T* __restrict__ feat2_b, float* __restrict__ imask_b, int32_t* __restrict__ bits_b,
    int32_t* __restrict__ vlen, int32_t* __restrict__ slot_ids, int32_t* __restrict__ live,
    int lb, int lpad, int l_ref, int capacity, int d, int n_mod) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int i = blockIdx.y;                               // video of the batch
  const bool second = blockIdx.z != 0;                    // modality (uniform per block)
  const int slot = slots[i];
  if (slot < 0 || slot >= capacity) return;               // (refused on the host; never a write outside the index)
  const T* f1 = second ? f1_b : f1_a;
  const T* f2 = second ? f2_b : f2_a;
  const float* bmask = second ? mask_b : mask_a;
  T* k6 = second ? k6_b : k6_a;
  T* feat2 = second ? feat2_b : feat2_a;

  // ---- the feature rows: half a wave per clip row
  const int l32 = threadIdx.x & 31;
  const int r = blockIdx.x * 8 + (threadIdx.x >> 5);      // clip row of the slot, < lpad (lpad % 8 == 0)
  const bool have = r < lb;
  const int64_t srow = (int64_t)i * lb + r;
  const int64_t drow = (int64_t)slot * lpad + r;
  uint4 v[L2N_MAXJ];
  const float nrm = l2n_load_row<T>(have ? f1 + srow * d : nullptr, d, l32, v);
  const int chunks = d / VEC;
  char* k6_row;
  if constexpr (TILED) {
    const int slices = chunks >> 2;                        // 64-byte slices per row
    k6_row = reinterpret_cast<char*>(k6) + (drow >> 8) * (int64_t)slices * (256 * 64) + (drow & 255) * 64;
  } else {
    k6_row = reinterpret_cast<char*>(k6 + drow * d);
  }
  const T* src2 = f2 + srow * d;
  T* dst2 = feat2 + drow * d;
#pragma unroll
  for (int j = 0; j < L2N_MAXJ; ++j) {
    const int c = l32 + 32 * j;
    if (c < chunks) {
      // a missing row: v is zero and 0 / max(0, 1e-12) = +0, the builder's value for the rows beyond lb
      const uint4 n = l2n_scale_chunk<T>(v[j], nrm);
      if constexpr (TILED) st_global16(k6_row + (int64_t)(c >> 2) * (256 * 64) + (c & 3) * 16, n);
      else st_global16(k6_row + (int64_t)c * 16, n);
      st_global16(dst2 + c * VEC, have ? ld_global16(src2 + c * VEC) : make_uint4(0u, 0u, 0u, 0u));
    }
  }
  if (blockIdx.x != 0) return;

  // ---- block 0 of (video, modality): the mask row, its bit words; of modality 0 also vlen, id and live bit.
  // threads 0..127 = waves 0 and 1 stand for clips 0..127 (lpad <= 128)
  __shared__ unsigned long long any_bits[2];
  const int t = threadIdx.x;
  const int w = t >> 6;
  if (w < 2) {
    const float mv = t < lb ? bmask[(int64_t)i * lb + t] : 0.f;
    float* imask = second ? imask_b : imask_a;
    int32_t* bits = second ? bits_b : bits_a;
    if (t < lpad) imask[(int64_t)slot * lpad + t] = mv;
    const unsigned long long mine = __ballot(mv != 0.f);
    if ((t & 63) == 0) {
      bits[(int64_t)slot * 4 + 2 * w] = (int32_t)(uint32_t)mine;
      bits[(int64_t)slot * 4 + 2 * w + 1] = (int32_t)(uint32_t)(mine >> 32);
    }
    if (!second) {      // valid length over BOTH modalities' masks
      float ov = 0.f;
      if (n_mod == 2 && t < lb) ov = mask_b[(int64_t)i * lb + t];
      const unsigned long long any = __ballot(mv != 0.f || ov != 0.f);
      if ((t & 63) == 0) any_bits[w] = any;
    }
  }
  if (second) return;
  __syncthreads();
  if (t == 0) {
    int pos = 0;                                           // last valid clip + 1
    if (any_bits[1]) pos = 128 - __clzll((long long)any_bits[1]);
    else if (any_bits[0]) pos = 64 - __clzll((long long)any_bits[0]);
    if (pos == 0) pos = l_ref;                             // no valid clip: the masked softmax is uniform, nothing is skipped
    vlen[slot] = pos < l_ref ? pos : l_ref;
    slot_ids[slot] = ids ? ids[i] : slot;
    atomicOr(reinterpret_cast<unsigned int*>(live) + (slot >> 5), 1u << (slot & 31));
  }
}

__global__ __launch_bounds__(128) void index_clear_rows_kernel(const int32_t* __restrict__ slots, float* __restrict__ imask_a,
                                                               int32_t* __restrict__ bits_a, float* __restrict__ imask_b,
                                                               int32_t* __restrict__ bits_b, int32_t* __restrict__ vlen,
                                                               int32_t* __restrict__ live, int lpad, int l_ref, int capacity) {
  const int slot = slots[blockIdx.x];
  if (slot < 0 || slot >= capacity) return;
  const int t = threadIdx.x;
  if (t < lpad) {
    imask_a[(int64_t)slot * lpad + t] = 0.f;
    if (imask_b) imask_b[(int64_t)slot * lpad + t] = 0.f;
  }
  if (t < 4) {
    bits_a[(int64_t)slot * 4 + t] = 0;
    if (bits_b) bits_b[(int64_t)slot * 4 + t] = 0;
  }
  if (t == 0) {
    vlen[slot] = l_ref;
    atomicAnd(reinterpret_cast<unsigned int*>(live) + (slot >> 5), ~(1u << (slot & 31)));
  }
}

template <typename T>
void launch_put(bool tiled, dim3 grid, hipStream_t st, const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b,
                const void* f2_b, const float* mask_b, const int32_t* slots, const int32_t* ids, void* k6_a, void* feat2_a,
                float* imask_a, int32_t* bits_a, void* k6_b, void* feat2_b, float* imask_b, int32_t* bits_b, int32_t* vlen,
                int32_t* slot_ids, int32_t* live, int lb, int lpad, int l_ref, int capacity, int d, int n_mod) {
  if (tiled)
    hipLaunchKernelGGL((index_put_rows_kernel<T, true>), grid, dim3(256), 0, st, (const T*)f1_a, (const T*)f2_a, mask_a,
                       (const T*)f1_b, (const T*)f2_b, mask_b, slots, ids, (T*)k6_a, (T*)feat2_a, imask_a, bits_a, (T*)k6_b,
                       (T*)feat2_b, imask_b, bits_b, vlen, slot_ids, live, lb, lpad, l_ref, capacity, d, n_mod);
  else
    hipLaunchKernelGGL((index_put_rows_kernel<T, false>), grid, dim3(256), 0, st, (const T*)f1_a, (const T*)f2_a, mask_a,
                       (const T*)f1_b, (const T*)f2_b, mask_b, slots, ids, (T*)k6_a, (T*)feat2_a, imask_a, bits_a, (T*)k6_b,
                       (T*)feat2_b, imask_b, bits_b, vlen, slot_ids, live, lb, lpad, l_ref, capacity, d, n_mod);
}

}  // namespace

extern "C" int xml_index_put_rows(int n_mod, const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b,
                                  const void* f2_b, const float* mask_b, const int32_t* slots, const int32_t* ids, int b,
                                  int lb, void* k6_a, void* feat2_a, float* imask_a, int32_t* bits_a, void* k6_b,
                                  void* feat2_b, float* imask_b, int32_t* bits_b, int32_t* vlen, int32_t* slot_ids,
                                  int32_t* live, int capacity, int lpad, int l_ref, int hidden, int dt, int tiled,
                                  xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!f1_a || !f2_a || !mask_a || !slots || !k6_a || !feat2_a || !imask_a || !bits_a || !vlen || !slot_ids || !live)
    return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!f1_b || !f2_b || !mask_b || !k6_b || !feat2_b || !imask_b || !bits_b)) return XML_ERR_BAD_ARG;
  if (b <= 0 || b > 65535 || capacity <= 0 || b > capacity || lb <= 0 || lpad <= 0 || lb > lpad || l_ref <= 0 || l_ref > lpad)
    return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_UNSUPPORTED;
  if ((lpad & 15) || lpad > 128 || (tiled && lpad != 128)) return XML_ERR_UNSUPPORTED;      // 4 mask words per slot
  if (!xml_q2c_tile_rows_l2norm_ok(hidden, dt)) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(lpad / 8), (unsigned)b, (unsigned)n_mod);
  hipStream_t st = (hipStream_t)stream;
  if (dt == XML_F32)
    launch_put<float>(tiled != 0, grid, st, f1_a, f2_a, mask_a, f1_b, f2_b, mask_b, slots, ids, k6_a, feat2_a, imask_a, bits_a,
                      k6_b, feat2_b, imask_b, bits_b, vlen, slot_ids, live, lb, lpad, l_ref, capacity, hidden, n_mod);
  else
    launch_put<bf16_t>(tiled != 0, grid, st, f1_a, f2_a, mask_a, f1_b, f2_b, mask_b, slots, ids, k6_a, feat2_a, imask_a, bits_a,
                       k6_b, feat2_b, imask_b, bits_b, vlen, slot_ids, live, lb, lpad, l_ref, capacity, hidden, n_mod);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_index_clear_rows(int n_mod, const int32_t* slots, int n, float* imask_a, int32_t* bits_a, float* imask_b,
                                    int32_t* bits_b, int32_t* vlen, int32_t* live, int capacity, int lpad, int l_ref,
                                    xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!slots || !imask_a || !bits_a || !vlen || !live) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!imask_b || !bits_b)) return XML_ERR_BAD_ARG;
  if (n <= 0 || capacity <= 0 || n > capacity || lpad <= 0 || l_ref <= 0 || l_ref > lpad) return XML_ERR_BAD_ARG;
  if ((lpad & 15) || lpad > 128) return XML_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(index_clear_rows_kernel, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, slots, imask_a, bits_a,
                     n_mod == 2 ? imask_b : nullptr, n_mod == 2 ? bits_b : nullptr, vlen, live, lpad, l_ref, capacity);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
