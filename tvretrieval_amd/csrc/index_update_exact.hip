// Exact-rank mode on an index that takes updates (include/xmlhip_index_exact.h; index_update.MutableCorpusIndex.create(...,
// exact_rank=True)).  xml_index_put_rows_exact scatters one encoded f32 context batch to its slots and
// leaves there, in ONE launch, what the one-shot exact-rank build leaves after three or four passes over temporaries
// (inference._exact_filter_operands + _finish_index):
//   filter image   rne_bf16(F.normalize(f1 row))     l2norm.h's arithmetic, then round_bf16_rows_err_kernel's (exact.hip)
//   err row        || y - rne_bf16(y) ||_2            that kernel's reduction order: lane l sums its 8 elements per 512 in
//                                                     order, wave_sum, sqrtf -- hence one wave per clip row here
//   re-score rows  y (f32) or split-f16 at 2^14       split16.h, the functions xml_split_f16_rows runs
//   feat2          the f2 row (f32) or split-f16 at the row's own scale
//   mask row, mask-bit words, vlen, id, live bit     the slot-state epilogue of every put (index_rows.h)
// and raises the running bound ec[modality] by atomicMax on the bits of every err value.
// One wave per clip row, four rows per block.  The normalisation wants the row in l2norm.h's lane order (half a wave, chunk
// l, l + 32, ..: both halves of the wave load it), the rounding in lane order 8 l + 512 t: the row is fetched from memory once
// and walked a second time out of the cache.  Everything after the norm is elementwise on that second walk, 16 bytes per lane
// and store.  In the tiled image a row's 64-byte slices lie one 16 KiB chunk apart: four lanes fill one slice, and the four
// rows of a block are neighbours inside every slice column, so a block completes 256-byte runs.
// xml_index_put_rows_packed_exact (include/xmlhip_index_exact_packed.h; create(..., exact_rank=True, filter_tiles=N); DESIGN.md
// section 20f) is the same kernel with the FILTER rows in a run of the packed image (index_update.hip's header comment): only
// rows [0, 16 nb) of a video are stored there, with the run's codes and mask fields; every per-slot operand, the error norms and
// the bound are written and raised over all lpad rows as above, so they do not depend on the layout of the filter image.
// xml_index_exact_bound recomputes the bound over the live slots.  (xml_exact_certificate_dev: exact.hip.)
#include "../../include/xmlhip_index_exact.h"
#include "../../include/xmlhip_index_exact_packed.h"
#include "index_rows.h"
#include "l2norm.h"
#include "split16.h"

namespace {

constexpr int PUT_MAXT = (L2N_MAXJ * 4 + 15) / 16;        // trips of 512 elements per f32 row (l2n_vec_ok: <= 1024 elements)

// the order-preserving image of a non-negative norm: NaN -> +inf (safe: every certificate fails), <= 0 -> 0
__device__ __forceinline__ uint32_t bound_bits(float e) {
  if (!(e == e)) return 0x7f800000u;
  return e > 0.f ? __float_as_uint(e) : 0u;
}

// The operands stay plain _a / _b lists here, not index_rows.h's per-modality structs: with the structs this kernel measured
// 2 to 3 % slower (batches of 256 videos), with the lists it is level with what it was.
// FORM (index_rows.h): where the FILTER rows go.  PACKED (xml_index_put_rows_packed_exact): row r of the video is row
// first * 16 + r of its run and is stored only when r < keep = 16 nb; every other operand stays per slot and is written whole.
template <int MODE, int FORM>
__global__ __launch_bounds__(256) void index_put_rows_exact_kernel(
    const float* __restrict__ f1_a, const float* __restrict__ f2_a, const float* __restrict__ mask_a,
    const float* __restrict__ f1_b, const float* __restrict__ f2_b, const float* __restrict__ mask_b,
    const int32_t* __restrict__ slots, const int32_t* __restrict__ ids,
    char* __restrict__ k6_a, char* __restrict__ rs_a, float* __restrict__ rs_inv_a, char* __restrict__ feat2_a,
    float* __restrict__ f2_inv_a, float* __restrict__ err_a, float* __restrict__ imask_a, int32_t* __restrict__ bits_a,
    char* __restrict__ k6_b, char* __restrict__ rs_b, float* __restrict__ rs_inv_b, char* __restrict__ feat2_b,
    float* __restrict__ f2_inv_b, float* __restrict__ err_b, float* __restrict__ imask_b, int32_t* __restrict__ bits_b,
    uint32_t* __restrict__ ec, int32_t* __restrict__ vlen, int32_t* __restrict__ slot_ids, int32_t* __restrict__ live,
    int lb, int lpad, int l_ref, int capacity, int d, int n_mod, PackedRuns pk) {
  const int i = blockIdx.y;                               // video of the batch
  const bool second = blockIdx.z != 0;                    // modality (uniform per block)
  const int slot = slots[i];
  int first = 0, nb = 0;
  if constexpr (FORM == PACKED) first = pk.runs[2 * i], nb = pk.runs[2 * i + 1];
  // a slot outside the index (refused on the host), a bad run record: nothing is written
  if (slot < 0 || slot >= capacity || (FORM == PACKED && !run_ok(first, nb, pk.nb_max, pk.n_tiles))) return;
  const int keep = FORM == PACKED ? 16 * nb : lpad;        // the filter image holds the run's rows only
  const float* f1 = second ? f1_b : f1_a;
  const float* f2 = second ? f2_b : f2_a;
  const float* bmask = second ? mask_b : mask_a;
  char* k6 = second ? k6_b : k6_a;
  char* rs = second ? rs_b : rs_a;
  char* feat2 = second ? feat2_b : feat2_a;
  float* err = second ? err_b : err_a;

  // ---- the feature rows: one wave per clip row
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);      // clip row of the slot, < lpad (lpad % 4 == 0)
  const bool have = r < lb;
  const int64_t srow = (int64_t)i * lb + r;
  const int64_t drow = (int64_t)slot * lpad + r;
  const int64_t krow = FORM == PACKED ? (int64_t)first * 16 + r : drow;      // row of the filter image (r < keep: inside it)
  const float* px = f1 + srow * d;
  float nrm;
  {
    uint4 v[L2N_MAXJ];                                    // a missing row: zeros, nrm = 1e-12, y = 0 / 1e-12 = +0
    nrm = l2n_load_row<float>(have ? px : nullptr, d, lane & 31, v);
  }
  const int slices = d >> 5;                              // 64-byte slices per bf16 row
  char* rs_row = rs + drow * (int64_t)d * 4;
  const float unit = pow2f(XML_F16_UNIT_LOG2);
  float s = 0.f;
  for (int c = lane * 8; c < d; c += 64 * 8) {
    float f[8];
    if (have) {
      ld8<float>(px + c, f);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] / nrm;        // l2n_scale_chunk
    const uint4 packed = round_bf16_err8(f, s);           // round_bf16_rows_err_kernel's step (c >> 3: the 16-byte chunk)
    if (FORM != PACKED || r < keep)
      st_global16(FORM == ROW_MAJOR ? k6 + krow * (int64_t)d * 2 + c * 2 : k6img::row_chunk(k6, krow, slices, c >> 3), packed);
    if constexpr (MODE == XML_EXACT_F16S) {               // split_rows_kernel<0> at the fixed unit scale
      uint4 hi, lo;
      (void)split8(f, unit, hi, lo);
      char* gp = rs_row + (int64_t)(c >> 5) * 128 + (c & 31) * 2;
      st_global16(gp, hi);
      st_global16(gp + 64, lo);
    } else {
      st8<float>(reinterpret_cast<float*>(rs_row) + c, f);
    }
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float e = sqrtf(s);
    err[drow] = e;
    // the cell only rises: a row that cannot raise it (every padding row, most rows once the cell has settled) skips the
    // atomic; a stale read can only make us issue one that changes nothing
    uint32_t* cell = ec + (second ? 1 : 0);
    const uint32_t bits = bound_bits(e);
    if (bits > __atomic_load_n(cell, __ATOMIC_RELAXED)) atomicMax(cell, bits);
    if constexpr (MODE == XML_EXACT_F16S) (second ? rs_inv_b : rs_inv_a)[drow] = pow2f(-XML_F16_UNIT_LOG2);
  }

  // ---- feat2
  const float* p2 = f2 + srow * d;
  char* f2_row = feat2 + drow * (int64_t)d * 4;
  if constexpr (MODE == XML_EXACT_F16S) {                 // split_rows_kernel<0> at the row's own scale
    float g2[PUT_MAXT][8];
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < PUT_MAXT; ++t) {
      const int c = lane * 8 + t * 512;
#pragma unroll
      for (int e = 0; e < 8; ++e) g2[t][e] = 0.f;
      if (have && c < d) ld8<float>(p2 + c, g2[t]);
#pragma unroll
      for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(g2[t][e]));      // row_absmax
    }
    const int ex = scale_log2_of(wave_max(m));
    const float sc = pow2f(ex);
#pragma unroll
    for (int t = 0; t < PUT_MAXT; ++t) {
      const int c = lane * 8 + t * 512;
      if (c < d) {
        uint4 hi, lo;
        (void)split8(g2[t], sc, hi, lo);
        char* gp = f2_row + (int64_t)(c >> 5) * 128 + (c & 31) * 2;
        st_global16(gp, hi);
        st_global16(gp + 64, lo);
      }
    }
    if (lane == 0) (second ? f2_inv_b : f2_inv_a)[drow] = pow2f(-ex) * 1.f;
  } else {
    for (int c = lane * 4; c < d; c += 64 * 4)
      st_global16(f2_row + (int64_t)c * 4, have ? ld_global16(p2 + c) : make_uint4(0u, 0u, 0u, 0u));
  }
  if (blockIdx.x != 0) return;

  // ---- block 0 of (video, modality): the slot's state (index_rows.h) and the 4 mask words of the own modality
  const unsigned long long mine = put_slot_state(keep, lb, lpad, l_ref, i, slot, second, bmask, n_mod == 2 ? mask_b : nullptr,
                                                 second ? imask_b : imask_a, ids, SlotState{vlen, slot_ids, live});
  const int t = threadIdx.x;
  if constexpr (FORM == PACKED) {
    if (t < 128) put_run_bits_codes(mine, first, nb, slot, second, second ? bits_b : bits_a, pk.codes);
  } else if (t < 128 && (t & 63) == 0) {
    int32_t* bits = second ? bits_b : bits_a;
    bits[(int64_t)slot * 4 + 2 * (t >> 6)] = (int32_t)(uint32_t)mine;
    bits[(int64_t)slot * 4 + 2 * (t >> 6) + 1] = (int32_t)(uint32_t)(mine >> 32);
  }
}

// one workgroup of 16 waves per modality; a wave takes the slots w, w + 16, .. and skips the free ones
__global__ __launch_bounds__(1024) void index_exact_bound_kernel(const float* __restrict__ err_a, const float* __restrict__ err_b,
                                                                 const uint32_t* __restrict__ live, float* __restrict__ ec,
                                                                 int capacity, int lpad) {
  __shared__ uint32_t part[16];
  const float* err = blockIdx.x ? err_b : err_a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t best = 0u;
  for (int s = w; s < capacity; s += 16) {
    if (!((live[s >> 5] >> (s & 31)) & 1u)) continue;     // (uniform per wave)
    const float* row = err + (int64_t)s * lpad;
    for (int c = lane; c < lpad; c += 64) {
      const uint32_t b = bound_bits(row[c]);
      best = b > best ? b : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)best, o, 64);
    best = other > best ? other : best;
  }
  if (lane == 0) part[w] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 16; ++j) best = part[j] > best ? part[j] : best;
    ec[blockIdx.x] = __uint_as_float(best);
  }
}

}  // namespace

extern "C" int xml_index_put_rows_exact(int n_mod, int mode, const void* f1_a, const void* f2_a, const float* mask_a,
                                        const void* f1_b, const void* f2_b, const float* mask_b, const int32_t* slots,
                                        const int32_t* ids, int b, int lb, void* k6_a, void* rescore_a, float* rescore_inv_a,
                                        void* feat2_a, float* feat2_inv_a, float* err_a, float* imask_a, int32_t* bits_a,
                                        void* k6_b, void* rescore_b, float* rescore_inv_b, void* feat2_b, float* feat2_inv_b,
                                        float* err_b, float* imask_b, int32_t* bits_b, float* ec, int32_t* vlen,
                                        int32_t* slot_ids, int32_t* live, int capacity, int lpad, int l_ref, int hidden, int dt,
                                        int tiled, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (mode != XML_EXACT_F32 && mode != XML_EXACT_F16S) return XML_ERR_BAD_ARG;
  const bool split = mode == XML_EXACT_F16S;
  if (!f1_a || !f2_a || !mask_a || !slots || !k6_a || !rescore_a || !feat2_a || !err_a || !imask_a || !bits_a || !ec || !vlen ||
      !slot_ids || !live)
    return XML_ERR_BAD_ARG;
  if (split && (!rescore_inv_a || !feat2_inv_a)) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!f1_b || !f2_b || !mask_b || !k6_b || !rescore_b || !feat2_b || !err_b || !imask_b || !bits_b))
    return XML_ERR_BAD_ARG;
  if (n_mod == 2 && split && (!rescore_inv_b || !feat2_inv_b)) return XML_ERR_BAD_ARG;
  if (b <= 0 || b > 65535 || capacity <= 0 || b > capacity || lb <= 0 || lpad <= 0 || lb > lpad || l_ref <= 0 || l_ref > lpad)
    return XML_ERR_BAD_ARG;
  if (dt != XML_F32) return XML_ERR_UNSUPPORTED;
  if ((lpad & 15) || lpad > 128 || (tiled && lpad != 128)) return XML_ERR_UNSUPPORTED;      // 4 mask words per slot
  if (!xml_q2c_tile_rows_l2norm_ok(hidden, XML_F32)) return XML_ERR_UNSUPPORTED;
  if (tiled && !xml_q2c_tiled_ok(128, hidden, XML_BF16)) return XML_ERR_UNSUPPORTED;
  if (split && (hidden % 32)) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(lpad / 4), (unsigned)b, (unsigned)n_mod);
  const auto kernel = split ? (tiled ? index_put_rows_exact_kernel<XML_EXACT_F16S, TILED> : index_put_rows_exact_kernel<XML_EXACT_F16S, ROW_MAJOR>)
                            : (tiled ? index_put_rows_exact_kernel<XML_EXACT_F32, TILED> : index_put_rows_exact_kernel<XML_EXACT_F32, ROW_MAJOR>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)f1_a, (const float*)f2_a, mask_a,
                     (const float*)f1_b, (const float*)f2_b, mask_b, slots, ids, (char*)k6_a, (char*)rescore_a, rescore_inv_a,
                     (char*)feat2_a, feat2_inv_a, err_a, imask_a, bits_a, (char*)k6_b, (char*)rescore_b, rescore_inv_b,
                     (char*)feat2_b, feat2_inv_b, err_b, imask_b, bits_b, reinterpret_cast<uint32_t*>(ec), vlen, slot_ids, live,
                     lb, lpad, l_ref, capacity, hidden, n_mod, PackedRuns{});
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_index_put_rows_packed_exact(int n_mod, int mode, const void* f1_a, const void* f2_a, const float* mask_a,
                                               const void* f1_b, const void* f2_b, const float* mask_b, const int32_t* slots,
                                               const int32_t* ids, const int32_t* runs, int b, int lb, int nb_max, void* k6_a,
                                               void* rescore_a, float* rescore_inv_a, void* feat2_a, float* feat2_inv_a,
                                               float* err_a, float* imask_a, int32_t* bits_a, void* k6_b, void* rescore_b,
                                               float* rescore_inv_b, void* feat2_b, float* feat2_inv_b, float* err_b,
                                               float* imask_b, int32_t* bits_b, int32_t* codes, float* ec, int32_t* vlen,
                                               int32_t* slot_ids, int32_t* live, int capacity, int n_tiles, int lpad, int l_ref,
                                               int hidden, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (mode != XML_EXACT_F32 && mode != XML_EXACT_F16S) return XML_ERR_BAD_ARG;
  const bool split = mode == XML_EXACT_F16S;
  if (!f1_a || !f2_a || !mask_a || !slots || !runs || !k6_a || !rescore_a || !feat2_a || !err_a || !imask_a || !bits_a ||
      !codes || !ec || !vlen || !slot_ids || !live)
    return XML_ERR_BAD_ARG;
  if (split && (!rescore_inv_a || !feat2_inv_a)) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!f1_b || !f2_b || !mask_b || !k6_b || !rescore_b || !feat2_b || !err_b || !imask_b || !bits_b))
    return XML_ERR_BAD_ARG;
  if (n_mod == 2 && split && (!rescore_inv_b || !feat2_inv_b)) return XML_ERR_BAD_ARG;
  if (lpad != 128) return XML_ERR_BAD_ARG;                 // the packed image: 128-clip slots
  if (b <= 0 || b > 65535 || capacity <= 0 || b > capacity || lb <= 0 || lb > lpad || l_ref <= 0 || l_ref > lpad)
    return XML_ERR_BAD_ARG;
  if (nb_max < 1 || nb_max > 8 || n_tiles <= 0 || n_tiles > (1 << 26)) return XML_ERR_BAD_ARG;
  if (dt != XML_F32) return XML_ERR_UNSUPPORTED;
  if (!xml_q2c_tile_rows_l2norm_ok(hidden, XML_F32) || !xml_q2c_tiled_ok(128, hidden, XML_BF16)) return XML_ERR_UNSUPPORTED;
  if (split && (hidden % 32)) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(lpad / 4), (unsigned)b, (unsigned)n_mod);
  const auto kernel = split ? index_put_rows_exact_kernel<XML_EXACT_F16S, PACKED> : index_put_rows_exact_kernel<XML_EXACT_F32, PACKED>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)f1_a, (const float*)f2_a, mask_a,
                     (const float*)f1_b, (const float*)f2_b, mask_b, slots, ids, (char*)k6_a, (char*)rescore_a, rescore_inv_a,
                     (char*)feat2_a, feat2_inv_a, err_a, imask_a, bits_a, (char*)k6_b, (char*)rescore_b, rescore_inv_b,
                     (char*)feat2_b, feat2_inv_b, err_b, imask_b, bits_b, reinterpret_cast<uint32_t*>(ec), vlen, slot_ids, live,
                     lb, lpad, l_ref, capacity, hidden, n_mod, PackedRuns{runs, codes, n_tiles, nb_max});
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_index_exact_bound(int n_mod, const float* err_a, const float* err_b, const int32_t* live, float* ec,
                                     int capacity, int lpad, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!err_a || !live || !ec || (n_mod == 2 && !err_b)) return XML_ERR_BAD_ARG;
  if (capacity <= 0 || lpad <= 0) return XML_ERR_BAD_ARG;
  hipLaunchKernelGGL(index_exact_bound_kernel, dim3((unsigned)n_mod), dim3(1024), 0, (hipStream_t)stream, err_a,
                     n_mod == 2 ? err_b : err_a, reinterpret_cast<const uint32_t*>(live), ec, capacity, lpad);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
