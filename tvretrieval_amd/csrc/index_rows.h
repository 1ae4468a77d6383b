// What the kernels of a resident index share (index_build.hip, index_update.hip, index_update_exact.hip, index_compact.hip,
// index_view.hip, exact.hip): the geometry of K6's tile image, the per-modality operand structs of the
// update launches, the slot-state epilogue of a put, the run records and the bits-and-codes tail of a put into the packed
// image, the slot-freeing tail of a clear, and the round-to-bf16 step of the exact-rank filter image.
#pragma once
#include "common.h"

// ---- K6's slice-major tile image: [tile of 256 rows][64-byte K slice][row][64 B] (q2c_persist.hip).  A (tile, slice) CHUNK is
// 16 KiB; a BLOCK is 16 rows = 1 KiB of it, 16 blocks per tile.  All offsets are 64-bit: the image is corpus-sized.
namespace k6img {
constexpr int TILE_ROWS = 256;
constexpr int SLICE_BYTES = 64;
constexpr int CHUNK_BYTES = TILE_ROWS * SLICE_BYTES;
constexpr int BLOCK_ROWS = 16;
constexpr int BLOCK_BYTES = BLOCK_ROWS * SLICE_BYTES;

// address of the 16-byte chunk c (piece c & 3 of slice c >> 2) of image row `row`; `slices` = 64-byte slices per row
// (C: char or const char; the row's part first, so that it is formed once per row)
template <typename C>
__device__ __forceinline__ C* row_chunk(C* image, int64_t row, int slices, int c) {
  C* at = image + (row >> 8) * (int64_t)slices * CHUNK_BYTES + (row & 255) * SLICE_BYTES;
  return at + (int64_t)(c >> 2) * CHUNK_BYTES + (c & 3) * 16;
}

// address of the KiB that block `block` (global number: tile * 16 + block of the tile) has in slice `slice`
template <typename C>
__device__ __forceinline__ C* block_slice(C* image, int64_t block, int slices, int slice) {
  return image + (block >> 4) * (int64_t)slices * CHUNK_BYTES + (int64_t)slice * CHUNK_BYTES + (block & 15) * BLOCK_BYTES;
}

// The load phase of the block movers (index_compact.hip, index_view.hip): a workgroup of four waves owns one (tile, slice)
// chunk, wave w its blocks w + 4 i; src[i] = entry lane0 + w + 4 i of `word` (a source block, < 0: none), and a lane's four
// 16-byte loads are in flight together.
__device__ __forceinline__ void load_wave_blocks(const char* k6, int word, int lane0, int wave, int slices, int slice, int lane,
                                                 int (&src)[4], uint4 (&v)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) src[i] = __builtin_amdgcn_readlane(word, lane0 + wave + 4 * i);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (src[i] >= 0) v[i] = ld_global16(block_slice(k6, src[i], slices, slice) + lane * 16);
}
}  // namespace k6img

// ---- the operands of an update launch (index_update.hip): one struct per modality, passed by value as Sides<S> and indexed
// by blockIdx.z (kernel arguments live in the kernarg segment: a uniform index gives scalar loads)
struct BatchSide {         // the encoded batch
  const void* f1;
  const void* f2;
  const float* mask;
};
struct IndexSide {         // the index tensors of a modality
  void* k6;
  void* feat2;
  float* imask;
  int32_t* bits;
};
template <typename S>
struct Sides {
  S m[2];
};
struct SlotState {         // per slot, shared by the modalities
  int32_t* vlen;
  int32_t* slot_ids;       // (unused by a clear)
  int32_t* live;
};

// ---- the slot-state epilogue of a put: called by all 256 threads of the FIRST workgroup of (video i, modality).  Threads
// 0..127 = waves 0 and 1 stand for clips 0..127 (lpad <= 128).  The effective mask of the video is its batch mask AND
// (clip < keep): keep = lpad for a slot that holds all its rows, 16 nb for a run of the packed image.  Writes the slot's f32
// mask row and returns, in waves 0 and 1, the ballot of the caller's own effective mask (bit = lane), from which the caller
// writes its mask-bit words.  For modality 0 (second == false) it also finishes the slot: vlen = last valid clip + 1 over
// BOTH modalities' effective masks (mask_other: modality 1's batch mask, NULL when there is one modality), 0 -> l_ref, clamped
// to l_ref; slot_ids; the live bit (slots of one call may share a live word: atomicOr).
__device__ __forceinline__ unsigned long long put_slot_state(int keep, int lb, int lpad, int l_ref, int i, int slot, bool second,
                                                             const float* __restrict__ bmask,
                                                             const float* __restrict__ mask_other,
                                                             float* __restrict__ imask, const int32_t* __restrict__ ids,
                                                             const SlotState& st) {
  __shared__ unsigned long long any_bits[2];
  const int t = threadIdx.x;
  const int w = t >> 6;
  unsigned long long mine = 0ull;
  if (w < 2) {
    const bool mine_ok = t < lb && t < keep;
    const float mv = mine_ok ? bmask[(int64_t)i * lb + t] : 0.f;
    if (t < lpad) imask[(int64_t)slot * lpad + t] = mv;
    mine = __ballot(mv != 0.f);
    if (!second) {
      float ov = 0.f;
      if (mask_other && mine_ok) ov = mask_other[(int64_t)i * lb + t];
      const unsigned long long any = __ballot(mv != 0.f || ov != 0.f);
      if ((t & 63) == 0) any_bits[w] = any;
    }
  }
  if (second) return mine;
  __syncthreads();
  if (t == 0) {
    int pos = 0;                                           // last valid clip + 1
    if (any_bits[1]) pos = 128 - __clzll((long long)any_bits[1]);
    else if (any_bits[0]) pos = 64 - __clzll((long long)any_bits[0]);
    if (pos == 0) pos = l_ref;                             // no valid clip: the masked softmax is uniform, nothing is skipped
    st.vlen[slot] = pos < l_ref ? pos : l_ref;
    st.slot_ids[slot] = ids ? ids[i] : slot;
    atomicOr(reinterpret_cast<unsigned int*>(st.live) + (slot >> 5), 1u << (slot & 31));
  }
  return mine;
}

// ---- the PACKED form (index_update.hip's header comment; xml_q2c_scores_packed): where the K6 rows of a put go, the run
// records of the packed entries, and the tail of a put that keeps the run's mask fields and codes in step with its rows
enum { ROW_MAJOR, TILED, PACKED };

struct PackedRuns {        // the packed form's operands; unused by the others
  const int32_t* runs;     // (first block, blocks) per record
  int32_t* codes;
  int n_tiles, nb_max;
};

// a run record (first block, block count) the kernels act on: 1..nb_max blocks, inside the image, inside one tile
__device__ __forceinline__ bool run_ok(int first, int nb, int nb_max, int n_tiles) {
  return nb >= 1 && nb <= nb_max && first >= 0 && first <= n_tiles * 16 - nb && (first >> 4) == ((first + nb - 1) >> 4);
}

// called by waves 0 and 1 (threadIdx.x < 128) behind put_slot_state, `mine` its ballot: the 16-bit mask fields of the run's
// nb blocks (two videos may share a word: atomics) and, by modality 0, the run's codes
__device__ __forceinline__ void put_run_bits_codes(unsigned long long mine, int first, int nb, int slot, bool second,
                                                   int32_t* __restrict__ bits, int32_t* __restrict__ codes) {
  const int t = threadIdx.x;
  const int k = (t >> 6) * 4 + (t & 63);                   // lanes 0..3 of a wave: blocks 4 w .. 4 w + 3 of the run
  if ((t & 63) < 4 && k < nb) {
    unsigned int* word = reinterpret_cast<unsigned int*>(bits) + ((first + k) >> 1);
    const int sh = ((first + k) & 1) * 16;
    const unsigned int b16 = (unsigned int)(mine >> (16 * (t & 63))) & 0xffffu;
    atomicAnd(word, ~(0xffffu << sh));                     // (same thread, same address: the OR comes after the AND)
    atomicOr(word, b16 << sh);
  }
  if (!second && t < nb) codes[first + t] = t == nb - 1 ? slot : (((first + t) & 15) == 7 ? -3 : -1);
}

// ---- the slot-freeing tail of a clear (one workgroup of >= lpad threads per slot, thread t): mask rows zeroed, vlen = l_ref,
// live bit cleared; the feature rows stay.  imask_b: NULL when there is one modality.
__device__ __forceinline__ void free_slot_state(int slot, int t, int lpad, int l_ref, float* __restrict__ imask_a,
                                                float* __restrict__ imask_b, const SlotState& st) {
  if (t < lpad) {
    imask_a[(int64_t)slot * lpad + t] = 0.f;
    if (imask_b) imask_b[(int64_t)slot * lpad + t] = 0.f;
  }
  if (t == 0) {
    st.vlen[slot] = l_ref;
    atomicAnd(reinterpret_cast<unsigned int*>(st.live) + (slot >> 5), ~(1u << (slot & 31)));
  }
}

// ---- one trip of the exact-rank filter rows (round_bf16_rows_err_kernel, exact.hip; the exact put): the 8 values rounded to
// bf16 (returned packed) and s += sum of (f - rne_bf16(f))^2, elements in order.  The square and the sum are two roundings
// (contract off): with -ffp-contract=fast the compiler fuses them or not by the shape of the code around the call, and the
// callers' values are bitwise one another's.
__device__ __forceinline__ uint4 round_bf16_err8(const float (&f)[8], float& s) {
#pragma clang fp contract(off)
  const uint4 packed = pack16<bf16_t>(f);
  float g[8];
  unpack16<bf16_t>(packed, g);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float dlt = f[e] - g[e];          // exact in f32 (Sterbenz-like: g is f rounded to 8 significant bits)
    s += dlt * dlt;
  }
  return packed;
}
