// In-place updates of a resident index whose K6 operand is the PACKED image (xml_q2c_scores_packed; DESIGN.md section 20,
// "packed form"; include/xmlhip_index.h).  A video occupies a RUN of nb = 1..8 consecutive 16-row blocks inside one 256-row
// tile of the image, at packed rows [first * 16, (first + nb) * 16), first = tile * 16 + block; the host's BlockTable
// (index_update.py) hands the runs out, this file keeps the three things K6 reads in step with them:
//   image   rows [0, 16 nb) of the video, L2-normalised (l2norm.h: bitwise the builder's), zero from the batch's width lb on
//   codes   (2 n_tiles, 8) = one int32 per block, flat index = the block number: -1 inside a run, the SLOT at its last block
//           (K6 writes out[q, slot]), -3 instead of -1 at block 7 of a tile when the run goes on into block 8, -2 unused
//   bits    (2 n_tiles, 4) words per modality, 16 bits per block: word = block >> 1, upper half for odd blocks
// and the per-slot state of xml_index_put_rows (feat2, f32 mask, vlen, slot_ids, live).  The EFFECTIVE mask of a video is
// its batch mask AND (clip < 16 nb): mask row, bits and vlen all follow it, so K6, K7 and K9 see one valid length.
// Invariants of the code table after every launch (the host never hands out overlapping runs): every run is -1 ... -1 slot
// within one tile; -3 stands only at block 7 of a tile and only when block 8 belongs to the same run -- the one case in
// which K6's eight waves take the straddle barrier; all other blocks are -2, and K6 skips those wherever they sit.
// A record that names a slot outside [0, capacity), nb outside 1..nb_max, a run outside the image or across a tile is
// dropped whole: nothing of it is written.
// Launch style of index_update.hip: half a wave per clip row, 16-byte loads and stores, one launch for both modalities.
// Two videos of one call can share a bits word (a block is half a word) or a live word: atomicAnd / atomicOr.
#include "../../include/xmlhip_index.h"
#include "l2norm.h"

namespace {

// a run record (first block, block count) the kernels act on: 1..nb_max blocks, inside the image, inside one tile
__device__ __forceinline__ bool run_ok(int first, int nb, int nb_max, int n_tiles) {
  return nb >= 1 && nb <= nb_max && first >= 0 && first <= n_tiles * 16 - nb && (first >> 4) == ((first + nb - 1) >> 4);
}

template <typename T>
__global__ __launch_bounds__(256) void index_put_rows_packed_kernel(
    const T* __restrict__ f1_a, const T* __restrict__ f2_a, const float* __restrict__ mask_a,
    const T* __restrict__ f1_b, const T* __restrict__ f2_b, const float* __restrict__ mask_b,
    const int32_t* __restrict__ slots, const int32_t* __restrict__ ids, const int32_t* __restrict__ runs,
    T* __restrict__ k6_a, T* __restrict__ feat2_a, float* __restrict__ imask_a, int32_t* __restrict__ bits_a,
    T* __restrict__ k6_b, T* __restrict__ feat2_b, float* __restrict__ imask_b, int32_t* __restrict__ bits_b,
    int32_t* __restrict__ codes, int32_t* __restrict__ vlen, int32_t* __restrict__ slot_ids, int32_t* __restrict__ live,
    int lb, int l_ref, int capacity, int n_tiles, int nb_max, int d, int n_mod) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int LPAD = 128;
  const int i = blockIdx.y;                               // video of the batch
  const bool second = blockIdx.z != 0;                    // modality (uniform per block)
  const int slot = slots[i];
  const int first = runs[2 * i], nb = runs[2 * i + 1];
  if (slot < 0 || slot >= capacity || !run_ok(first, nb, nb_max, n_tiles)) return;      // a bad record writes nothing
  const T* f1 = second ? f1_b : f1_a;
  const T* f2 = second ? f2_b : f2_a;
  const float* bmask = second ? mask_b : mask_a;
  T* k6 = second ? k6_b : k6_a;
  T* feat2 = second ? feat2_b : feat2_a;

  // ---- the feature rows: half a wave per clip row
  const int l32 = threadIdx.x & 31;
  const int r = blockIdx.x * 8 + (threadIdx.x >> 5);      // clip row of the slot, < 128
  const bool have = r < lb;
  const bool in_run = r < 16 * nb;                        // the image holds the run's rows only
  const int64_t srow = (int64_t)i * lb + r;
  uint4 v[L2N_MAXJ];
  const float nrm = l2n_load_row<T>(have && in_run ? f1 + srow * d : nullptr, d, l32, v);
  const int chunks = d / VEC;
  const int slices = chunks >> 2;                          // 64-byte slices per row
  const int64_t prow = (int64_t)first * 16 + r;            // packed row (in_run: < n_tiles * 256)
  char* k6_row = reinterpret_cast<char*>(k6) + (prow >> 8) * (int64_t)slices * (256 * 64) + (prow & 255) * 64;
  const T* src2 = f2 + srow * d;
  T* dst2 = feat2 + ((int64_t)slot * LPAD + r) * d;
#pragma unroll
  for (int j = 0; j < L2N_MAXJ; ++j) {
    const int c = l32 + 32 * j;
    if (c < chunks) {
      // a row beyond lb: v is zero and 0 / max(0, 1e-12) = +0, the builder's value
      if (in_run) st_global16(k6_row + (int64_t)(c >> 2) * (256 * 64) + (c & 3) * 16, l2n_scale_chunk<T>(v[j], nrm));
      st_global16(dst2 + c * VEC, have ? ld_global16(src2 + c * VEC) : make_uint4(0u, 0u, 0u, 0u));
    }
  }
  if (blockIdx.x != 0) return;

  // ---- block 0 of (video, modality): the mask row and the run's bits; of modality 0 also codes, vlen, id and live bit.
  // threads 0..127 = waves 0 and 1 stand for clips 0..127
  __shared__ unsigned long long any_bits[2];
  const int t = threadIdx.x;
  const int w = t >> 6;
  if (w < 2) {
    const bool mine_ok = t < lb && t < 16 * nb;            // the effective mask: nothing beyond the run
    const float mv = mine_ok ? bmask[(int64_t)i * lb + t] : 0.f;
    float* imask = second ? imask_b : imask_a;
    imask[(int64_t)slot * LPAD + t] = mv;
    const unsigned long long mine = __ballot(mv != 0.f);
    const int k = w * 4 + (t & 63);                        // lanes 0..3 of a wave: blocks 4 w .. 4 w + 3 of the run
    if ((t & 63) < 4 && k < nb) {
      unsigned int* word = reinterpret_cast<unsigned int*>(second ? bits_b : bits_a) + ((first + k) >> 1);
      const int sh = ((first + k) & 1) * 16;
      const unsigned int b16 = (unsigned int)(mine >> (16 * (t & 63))) & 0xffffu;
      atomicAnd(word, ~(0xffffu << sh));                   // (same thread, same address: the OR comes after the AND)
      atomicOr(word, b16 << sh);
    }
    if (!second) {      // valid length over BOTH modalities' effective masks
      float ov = 0.f;
      if (n_mod == 2 && mine_ok) ov = mask_b[(int64_t)i * lb + t];
      const unsigned long long any = __ballot(mv != 0.f || ov != 0.f);
      if ((t & 63) == 0) any_bits[w] = any;
      if (t < nb) codes[first + t] = t == nb - 1 ? slot : (((first + t) & 15) == 7 ? -3 : -1);
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

__global__ __launch_bounds__(128) void index_clear_rows_packed_kernel(
    const int32_t* __restrict__ slots, const int32_t* __restrict__ runs, float* __restrict__ imask_a,
    int32_t* __restrict__ bits_a, float* __restrict__ imask_b, int32_t* __restrict__ bits_b, int32_t* __restrict__ codes,
    int32_t* __restrict__ vlen, int32_t* __restrict__ live, int l_ref, int capacity, int n_tiles, int nb_max) {
  constexpr int LPAD = 128;
  const int slot = slots[blockIdx.x];
  const int first = runs[2 * blockIdx.x], nb = runs[2 * blockIdx.x + 1];
  if (slot < -1 || slot >= capacity || !run_ok(first, nb, nb_max, n_tiles)) return;     // a bad record writes nothing
  const int t = threadIdx.x;
  if (t < nb) {                                            // the run: unused blocks, no valid clip
    codes[first + t] = -2;
    const int sh = ((first + t) & 1) * 16;
    atomicAnd(reinterpret_cast<unsigned int*>(bits_a) + ((first + t) >> 1), ~(0xffffu << sh));
    if (bits_b) atomicAnd(reinterpret_cast<unsigned int*>(bits_b) + ((first + t) >> 1), ~(0xffffu << sh));
  }
  if (slot < 0) return;                                    // slot -1: the run alone (a replace that moves its video)
  imask_a[(int64_t)slot * LPAD + t] = 0.f;
  if (imask_b) imask_b[(int64_t)slot * LPAD + t] = 0.f;
  if (t == 0) {
    vlen[slot] = l_ref;
    atomicAnd(reinterpret_cast<unsigned int*>(live) + (slot >> 5), ~(1u << (slot & 31)));
  }
}

}  // namespace

extern "C" int xml_index_put_rows_packed(int n_mod, const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b,
                                         const void* f2_b, const float* mask_b, const int32_t* slots, const int32_t* ids,
                                         const int32_t* runs, int b, int lb, int nb_max, void* k6_a, void* feat2_a,
                                         float* imask_a, int32_t* bits_a, void* k6_b, void* feat2_b, float* imask_b,
                                         int32_t* bits_b, int32_t* codes, int32_t* vlen, int32_t* slot_ids, int32_t* live,
                                         int capacity, int n_tiles, int lpad, int l_ref, int hidden, int dt,
                                         xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!f1_a || !f2_a || !mask_a || !slots || !runs || !k6_a || !feat2_a || !imask_a || !bits_a || !codes || !vlen ||
      !slot_ids || !live)
    return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!f1_b || !f2_b || !mask_b || !k6_b || !feat2_b || !imask_b || !bits_b)) return XML_ERR_BAD_ARG;
  if (lpad != 128 || (dt != XML_F32 && dt != XML_BF16)) return XML_ERR_BAD_ARG;      // the packed image: 128-clip slots
  if (b <= 0 || b > 65535 || capacity <= 0 || b > capacity || lb <= 0 || lb > lpad || l_ref <= 0 || l_ref > lpad)
    return XML_ERR_BAD_ARG;
  if (nb_max < 1 || nb_max > 8 || n_tiles <= 0 || n_tiles > (1 << 26)) return XML_ERR_BAD_ARG;
  if (!xml_q2c_tile_rows_l2norm_ok(hidden, dt) || !xml_q2c_tiled_ok(lpad, hidden, dt)) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(lpad / 8), (unsigned)b, (unsigned)n_mod);
  hipStream_t st = (hipStream_t)stream;
  if (dt == XML_F32)
    hipLaunchKernelGGL((index_put_rows_packed_kernel<float>), grid, dim3(256), 0, st, (const float*)f1_a, (const float*)f2_a,
                       mask_a, (const float*)f1_b, (const float*)f2_b, mask_b, slots, ids, runs, (float*)k6_a,
                       (float*)feat2_a, imask_a, bits_a, (float*)k6_b, (float*)feat2_b, imask_b, bits_b, codes, vlen,
                       slot_ids, live, lb, l_ref, capacity, n_tiles, nb_max, hidden, n_mod);
  else
    hipLaunchKernelGGL((index_put_rows_packed_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)f1_a,
                       (const bf16_t*)f2_a, mask_a, (const bf16_t*)f1_b, (const bf16_t*)f2_b, mask_b, slots, ids, runs,
                       (bf16_t*)k6_a, (bf16_t*)feat2_a, imask_a, bits_a, (bf16_t*)k6_b, (bf16_t*)feat2_b, imask_b, bits_b,
                       codes, vlen, slot_ids, live, lb, l_ref, capacity, n_tiles, nb_max, hidden, n_mod);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_index_clear_rows_packed(int n_mod, const int32_t* slots, const int32_t* runs, int n, int nb_max,
                                           float* imask_a, int32_t* bits_a, float* imask_b, int32_t* bits_b, int32_t* codes, int32_t* vlen,
                                           int32_t* live, int capacity, int n_tiles, int lpad, int l_ref,
                                           xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!slots || !runs || !imask_a || !bits_a || !codes || !vlen || !live) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!imask_b || !bits_b)) return XML_ERR_BAD_ARG;
  if (lpad != 128) return XML_ERR_BAD_ARG;
  if (n <= 0 || n > 65535 || capacity <= 0 || n_tiles <= 0 || n_tiles > (1 << 26) || l_ref <= 0 || l_ref > lpad)
    return XML_ERR_BAD_ARG;
  if (nb_max < 1 || nb_max > 8) return XML_ERR_BAD_ARG;
  hipLaunchKernelGGL(index_clear_rows_packed_kernel, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, slots, runs, imask_a,
                     bits_a, n_mod == 2 ? imask_b : nullptr, n_mod == 2 ? bits_b : nullptr, codes, vlen, live, l_ref, capacity,
                     n_tiles, nb_max);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
