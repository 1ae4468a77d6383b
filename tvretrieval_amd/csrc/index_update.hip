// In-place updates of a resident corpus index with a fixed number of video SLOTS (inference.MutableCorpusIndex, DESIGN.md
// section 20).  xml_index_put_rows scatters one encoded context batch to its slots and leaves there what the one-shot build
// leaves for the same batch (inference._fill_index_rows + the packing pass of build_corpus_index(length_buckets=False)):
//   K6 operand   the L2-normalised feat1 rows (l2norm.h's arithmetic, bitwise), in K6's slice-major tile image
//                (index_rows.h: a tile holds two 128-clip slots) or row-major where the tiled kernel does not take the shape;
//                zero rows beyond the batch's padded width lb
//   feat2        the encoder's rows [0, lb) (padded positions included), zero rows [lb, lpad)
//   mask         the batch's f32 mask, 0 beyond lb; mask bits: 4 words per slot and modality (bit c = mask[c] != 0)
//   vlen         max over modalities of (last valid clip + 1), 0 -> l_ref, clamped to l_ref (CorpusIndex.set_valid_lengths)
//   slot_ids     the caller's id of the slot's video; live: the slot's bit set
// Every one of the slot's lpad rows is written, so nothing of a previous occupant survives a replace.
// xml_index_clear_rows frees slots: live bit cleared, mask rows and mask bits zeroed, vlen = l_ref (the feature rows stay).
//
// The PACKED form (xml_index_put_rows_packed / xml_index_clear_rows_packed; xml_q2c_scores_packed; DESIGN.md section 20,
// "packed form"; include/xmlhip_index.h).  A video occupies a RUN of nb = 1..8 consecutive 16-row blocks inside one 256-row
// tile of the image, at packed rows [first * 16, (first + nb) * 16), first = tile * 16 + block; the host's BlockTable
// (index_update.py) hands the runs out, the kernels keep the three things K6 reads in step with them:
//   image   rows [0, 16 nb) of the video, L2-normalised (l2norm.h: bitwise the builder's), zero from the batch's width lb on
//   codes   (2 n_tiles, 8) = one int32 per block, flat index = the block number: -1 inside a run, the SLOT at its last block
//           (K6 writes out[q, slot]), -3 instead of -1 at block 7 of a tile when the run goes on into block 8, -2 unused
//   bits    (2 n_tiles, 4) words per modality, 16 bits per block: word = block >> 1, upper half for odd blocks
// and the per-slot state above (feat2, f32 mask, vlen, slot_ids, live).  The EFFECTIVE mask of a video is its batch mask AND
// (clip < 16 nb): mask row, bits and vlen all follow it, so K6, K7 and K9 see one valid length.
// Invariants of the code table after every launch (the host never hands out overlapping runs): every run is -1 ... -1 slot
// within one tile; -3 stands only at block 7 of a tile and only when block 8 belongs to the same run -- the one case in
// which K6's eight waves take the straddle barrier; all other blocks are -2, and K6 skips those wherever they sit.
// A record that names a slot outside [0, capacity), nb outside 1..nb_max, a run outside the image or across a tile is
// dropped whole: nothing of it is written.
//
// Pure streaming: half a wave per clip row, 16-byte loads and stores; one launch for both modalities.  Slots of one call are
// distinct (the host slot table guarantees it), several of them may share a live word, two packed videos a bits word (a block
// is half a word): atomicOr / atomicAnd.
#include "../../include/xmlhip_index.h"
#include "index_rows.h"
#include "l2norm.h"

namespace {

// (ROW_MAJOR | TILED | PACKED, PackedRuns, run_ok and the bits-and-codes tail of a packed put: index_rows.h)
template <typename T, int FORM>
__global__ __launch_bounds__(256) void index_put_rows_kernel(Sides<BatchSide> batch, Sides<IndexSide> index,
                                                             const int32_t* __restrict__ slots,
                                                             const int32_t* __restrict__ ids, PackedRuns pk, SlotState st,
                                                             int lb, int lpad_arg, int l_ref, int capacity, int d, int n_mod) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int lpad = FORM == PACKED ? 128 : lpad_arg;        // (the packed image: 128-clip slots)
  const int i = blockIdx.y;                               // video of the batch
  const bool second = blockIdx.z != 0;                    // modality (uniform per block)
  const int slot = slots[i];
  int first = 0, nb = 0;
  if constexpr (FORM == PACKED) first = pk.runs[2 * i], nb = pk.runs[2 * i + 1];      // (fetched beside the slot, not behind it)
  // a slot outside the index (refused on the host), a bad run record: nothing is written
  if (slot < 0 || slot >= capacity || (FORM == PACKED && !run_ok(first, nb, pk.nb_max, pk.n_tiles))) return;
  const int keep = FORM == PACKED ? 16 * nb : lpad;        // the image holds the run's rows only
  const BatchSide& bs = batch.m[blockIdx.z];               // (references: the epilogue's operands are fetched by block 0 only)
  const IndexSide& ix = index.m[blockIdx.z];
  const T* __restrict__ f1 = static_cast<const T*>(bs.f1);
  const T* __restrict__ f2 = static_cast<const T*>(bs.f2);
  char* __restrict__ k6 = static_cast<char*>(ix.k6);
  T* __restrict__ feat2 = static_cast<T*>(ix.feat2);

  // ---- the feature rows: half a wave per clip row
  const int l32 = threadIdx.x & 31;
  const int r = blockIdx.x * 8 + (threadIdx.x >> 5);      // clip row of the slot, < lpad (lpad % 8 == 0)
  const bool have = r < lb;
  const bool in_run = r < keep;
  const int64_t srow = (int64_t)i * lb + r;
  const int64_t drow = (int64_t)slot * lpad + r;
  const int64_t krow = FORM == PACKED ? (int64_t)first * 16 + r : drow;      // row of the image (in_run: inside it)
  uint4 v[L2N_MAXJ];
  const float nrm = l2n_load_row<T>(have && in_run ? f1 + srow * d : nullptr, d, l32, v);
  const int chunks = d / VEC;
  const int slices = chunks >> 2;                          // 64-byte slices per row
  const T* src2 = f2 + srow * d;
  T* dst2 = feat2 + drow * d;
#pragma unroll
  for (int j = 0; j < L2N_MAXJ; ++j) {
    const int c = l32 + 32 * j;
    if (c < chunks) {
      // a missing row: v is zero and 0 / max(0, 1e-12) = +0, the builder's value for the rows beyond lb
      char* at = FORM == ROW_MAJOR ? k6 + krow * chunks * 16 + (int64_t)c * 16 : k6img::row_chunk(k6, krow, slices, c);
      if (in_run) st_global16(at, l2n_scale_chunk<T>(v[j], nrm));
      st_global16(dst2 + c * VEC, have ? ld_global16(src2 + c * VEC) : make_uint4(0u, 0u, 0u, 0u));
    }
  }
  if (blockIdx.x != 0) return;

  // ---- block 0 of (video, modality): the slot's state (index_rows.h) and the mask bits of the own modality
  const unsigned long long mine = put_slot_state(keep, lb, lpad, l_ref, i, slot, second, bs.mask,
                                                 n_mod == 2 ? batch.m[1].mask : nullptr, ix.imask, ids, st);
  const int t = threadIdx.x;
  const int w = t >> 6;
  if (w >= 2) return;
  if constexpr (FORM == PACKED) {
    put_run_bits_codes(mine, first, nb, slot, second, ix.bits, pk.codes);
  } else if ((t & 63) == 0) {                              // 4 words per slot
    ix.bits[(int64_t)slot * 4 + 2 * w] = (int32_t)(uint32_t)mine;
    ix.bits[(int64_t)slot * 4 + 2 * w + 1] = (int32_t)(uint32_t)(mine >> 32);
  }
}

// one workgroup of 128 threads per record.  PACKED: the record's run becomes unused blocks with no valid clip, and a slot of
// -1 names the run alone (a replace that moves its video).  The b side is NULL when there is one modality.
template <bool PACKED>
__global__ __launch_bounds__(128) void index_clear_rows_kernel(const int32_t* __restrict__ slots, Sides<IndexSide> index,
                                                               PackedRuns pk, SlotState st, int lpad, int l_ref, int capacity) {
  const int slot = slots[blockIdx.x];
  const int t = threadIdx.x;
  int32_t* bits_a = index.m[0].bits;
  int32_t* bits_b = index.m[1].bits;
  if constexpr (PACKED) {
    const int first = pk.runs[2 * blockIdx.x], nb = pk.runs[2 * blockIdx.x + 1];
    if (slot < -1 || slot >= capacity || !run_ok(first, nb, pk.nb_max, pk.n_tiles)) return;     // a bad record writes nothing
    if (t < nb) {
      pk.codes[first + t] = -2;
      const int sh = ((first + t) & 1) * 16;
      atomicAnd(reinterpret_cast<unsigned int*>(bits_a) + ((first + t) >> 1), ~(0xffffu << sh));
      if (bits_b) atomicAnd(reinterpret_cast<unsigned int*>(bits_b) + ((first + t) >> 1), ~(0xffffu << sh));
    }
    if (slot < 0) return;
  } else {
    if (slot < 0 || slot >= capacity) return;
    if (t < 4) {
      bits_a[(int64_t)slot * 4 + t] = 0;
      if (bits_b) bits_b[(int64_t)slot * 4 + t] = 0;
    }
  }
  free_slot_state(slot, t, lpad, l_ref, index.m[0].imask, index.m[1].imask, st);
}

// the per-modality operand structs of the C entries' _a / _b lists
Sides<BatchSide> batch_sides(const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b, const void* f2_b,
                             const float* mask_b) {
  return {{{f1_a, f2_a, mask_a}, {f1_b, f2_b, mask_b}}};
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
  const auto kernel = dt == XML_F32 ? (tiled ? index_put_rows_kernel<float, TILED> : index_put_rows_kernel<float, ROW_MAJOR>)
                                    : (tiled ? index_put_rows_kernel<bf16_t, TILED> : index_put_rows_kernel<bf16_t, ROW_MAJOR>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, batch_sides(f1_a, f2_a, mask_a, f1_b, f2_b, mask_b),
                     Sides<IndexSide>{{{k6_a, feat2_a, imask_a, bits_a}, {k6_b, feat2_b, imask_b, bits_b}}}, slots, ids,
                     PackedRuns{}, SlotState{vlen, slot_ids, live}, lb, lpad, l_ref, capacity, hidden, n_mod);
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
  Sides<IndexSide> index = {{{nullptr, nullptr, imask_a, bits_a}, {}}};
  if (n_mod == 2) index.m[1] = {nullptr, nullptr, imask_b, bits_b};
  hipLaunchKernelGGL(index_clear_rows_kernel<false>, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, slots, index,
                     PackedRuns{}, SlotState{vlen, nullptr, live}, lpad, l_ref, capacity);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

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
  const auto kernel = dt == XML_F32 ? index_put_rows_kernel<float, PACKED> : index_put_rows_kernel<bf16_t, PACKED>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, batch_sides(f1_a, f2_a, mask_a, f1_b, f2_b, mask_b),
                     Sides<IndexSide>{{{k6_a, feat2_a, imask_a, bits_a}, {k6_b, feat2_b, imask_b, bits_b}}}, slots, ids,
                     PackedRuns{runs, codes, n_tiles, nb_max}, SlotState{vlen, slot_ids, live}, lb, lpad, l_ref, capacity,
                     hidden, n_mod);
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
  Sides<IndexSide> index = {{{nullptr, nullptr, imask_a, bits_a}, {}}};
  if (n_mod == 2) index.m[1] = {nullptr, nullptr, imask_b, bits_b};
  hipLaunchKernelGGL(index_clear_rows_kernel<true>, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, slots, index,
                     PackedRuns{runs, codes, n_tiles, nb_max}, SlotState{vlen, nullptr, live}, lpad, l_ref, capacity);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
