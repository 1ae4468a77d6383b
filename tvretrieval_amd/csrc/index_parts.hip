// Long videos on an index that takes updates (include/xmlhip_index_parts.h): a video of more than
// l_ref clips is a CHAIN of slots, one overlapping part per slot, described by three per-slot tables
//   chain_head[s]    the slot of the first part (offset 0) of slot s's video
//   chain_next[s]    the slot of the next part in rising offset order, -1 at the end
//   chain_offset[s]  the first clip of slot s's part within its source video (read by xml_moments_decode_parts only)
// A free slot and a video of one part are in the SINGLE state: head == itself, next == -1, offset == 0.  A mutable index hands
// out slots lowest-free-first, so the parts of a video lie in scattered slots: the contiguous fold of parts.hip (a CSR over
// adjacent index rows) cannot serve it, the fold below walks the chain instead.
// Best part of a chain: the running best starts as (head, -inf); following `next`, a later part replaces it when its score is
// strictly greater -- ties go to the lowest offset, a NaN never wins, a chain of nothing but -inf / NaN keeps its head.  This
// is parts.hip's rule with row order replaced by chain order.
// THE WALK IS BOUNDED: every walk below visits at most max_parts slots (one `next` load per visited slot), stops at a `next`
// outside [0, capacity) and ignores a `head` outside that range -- a damaged table gives a wrong bit, never a kernel that does
// not end, and never an access outside the tables or the score row.
#include "../../include/xmlhip_index_parts.h"
#include "common.h"

namespace {

constexpr int FOLD_ROWS = 32;      // score rows per thread (parts.hip: the dependent table loads are paid once for all of them)
constexpr int CHAIN_REGS = 4;      // slot numbers of a chain kept in registers; a longer chain is re-walked behind them per row

__device__ __forceinline__ bool in_range(int s, int capacity) { return (unsigned)s < (unsigned)capacity; }

// One record {slot, head, next, offset} per thread (four int32 loads: the records need no 16-byte alignment).  The slot is
// checked again here (as xml_index_put_rows checks its slots): a record outside [0, capacity) writes nothing.
__global__ __launch_bounds__(256) void index_set_chains_kernel(const int32_t* __restrict__ records, int n,
                                                               int32_t* __restrict__ chain_head,
                                                               int32_t* __restrict__ chain_next,
                                                               int32_t* __restrict__ chain_offset, int capacity) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t* r = records + (int64_t)i * 4;
  const int slot = r[0];
  if (!in_range(slot, capacity)) return;
  chain_head[slot] = r[1];
  chain_next[slot] = r[2];
  chain_offset[slot] = r[3];
}

// grid (ceil(capacity / 256), ceil(rows / FOLD_ROWS)); one thread per slot and FOLD_ROWS score rows, one wave per two output
// words of each row (group_best_allow_kernel's shape).  The chain is chased ONCE per thread: its first CHAIN_REGS slot numbers
// stay in registers for all the rows, and only a chain longer than that is walked again, behind them, per row.  Every thread of
// a chain walks the whole chain and finds the same best part -- G^2 score loads per row for a chain of G parts, max_parts
// bounds G.  A chain of one slot is its own best part whatever it scores: its score is NOT READ (the packed K6 leaves the
// columns of free slots unspecified, and a free slot is in the single state).
__global__ __launch_bounds__(256) void chain_best_allow_kernel(
    const float* __restrict__ scores, int64_t ld, int rows, int capacity, const int32_t* __restrict__ chain_head,
    const int32_t* __restrict__ chain_next, int max_parts, const uint32_t* __restrict__ video_allow, int64_t allow_ld,
    int allow_rows, uint32_t* __restrict__ out_bits, int64_t out_ld) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int c[CHAIN_REGS];
  int n_reg = 0;             // slots of the chain held in c[]
  int rest = -1;             // the slot behind c[CHAIN_REGS - 1], -1: the chain ends inside c[]
  int h = -1;
  if (s < capacity) {
    h = chain_head[s];
    if (in_range(h, capacity)) {
      int j = h;
#pragma unroll
      for (int i = 0; i < CHAIN_REGS; ++i) {
        if (in_range(j, capacity) && i < max_parts) {
          c[i] = j;
          n_reg = i + 1;
          j = chain_next[j];
        } else {
          c[i] = 0;
          j = -1;
        }
      }
      if (in_range(j, capacity) && CHAIN_REGS < max_parts) rest = j;
    } else {
      h = -1;                                                // a head outside the table: the slot's bit is 0
    }
  }
  const bool single = n_reg == 1;
  const int row0 = blockIdx.y * FOLD_ROWS;
#pragma unroll 2
  for (int r = 0; r < FOLD_ROWS; ++r) {
    const int row = row0 + r;
    if (row >= rows) break;                                  // (uniform over the workgroup)
    bool set = false;
    if (h >= 0) {
      const uint32_t* a = video_allow + (allow_rows == 1 ? 0 : (int64_t)row * allow_ld);
      if ((a[h >> 5] >> (h & 31)) & 1u) {                    // the HEAD's bit: a caller's mask numbers a video by its head slot
        if (single) {
          set = s == h;
        } else {
          const float* __restrict__ sr = scores + (int64_t)row * ld;
          int best = h;
          float bv = -INFINITY;
#pragma unroll
          for (int i = 0; i < CHAIN_REGS; ++i) {
            if (i < n_reg) {
              const float v = sr[c[i]];
              if (v > bv) { bv = v; best = c[i]; }
            }
          }
          int j = rest;
          for (int seen = CHAIN_REGS; in_range(j, capacity) && seen < max_parts; ++seen) {
            const float v = sr[j];
            if (v > bv) { bv = v; best = j; }
            j = chain_next[j];
          }
          set = best == s;
        }
      }
    }
    const unsigned long long bal = __ballot(set);            // (every lane of the wave arrives here)
    if ((lane & 31) == 0 && s < capacity)                    // s is a multiple of 32: word s >> 5 exists; its padding bits are 0
      out_bits[(int64_t)row * out_ld + (s >> 5)] = (uint32_t)(bal >> lane);
  }
}

// one thread per row: the best part of the chain that video[row] (ANY slot of it) belongs to, -1 for a slot outside
// [0, capacity) or a head outside it
__global__ __launch_bounds__(256) void chain_best_rows_kernel(
    const float* __restrict__ scores, int64_t ld, int rows, int capacity, const int32_t* __restrict__ chain_head,
    const int32_t* __restrict__ chain_next, int max_parts, const int32_t* __restrict__ video, int32_t* __restrict__ out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int v = video[row];
  int best = -1;
  if (in_range(v, capacity)) {
    const int h = chain_head[v];
    if (in_range(h, capacity)) {
      best = h;
      int j = chain_next[h];
      if (in_range(j, capacity) && max_parts > 1) {          // (the score of a chain of one slot is not read)
        const float* __restrict__ sr = scores + (int64_t)row * ld;
        float bv = -INFINITY;
        const float v0 = sr[h];
        if (v0 > bv) bv = v0;
        for (int seen = 1; in_range(j, capacity) && seen < max_parts; ++seen) {
          const float x = sr[j];
          if (x > bv) { bv = x; best = j; }
          j = chain_next[j];
        }
      }
    }
  }
  out[row] = best;
}

}  // namespace

extern "C" int xml_index_set_chains(const int32_t* records, int n, int32_t* chain_head, int32_t* chain_next,
                                    int32_t* chain_offset, int capacity, xml_stream_t stream) {
  XML_ENTER();
  if (!records || !chain_head || !chain_next || !chain_offset) return XML_ERR_BAD_ARG;
  if (n < 0 || capacity <= 0) return XML_ERR_BAD_ARG;
  if (n == 0) return XML_OK;
  hipLaunchKernelGGL(index_set_chains_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     records, n, chain_head, chain_next, chain_offset, capacity);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_chain_best_allow(const float* scores, int64_t ld, int rows, int capacity, const int32_t* chain_head,
                                    const int32_t* chain_next, int max_parts, const uint32_t* video_allow, int64_t allow_ld,
                                    int allow_rows, uint32_t* out_bits, int64_t out_ld, xml_stream_t stream) {
  XML_ENTER();
  if (!scores || !chain_head || !chain_next || !video_allow || !out_bits) return XML_ERR_BAD_ARG;
  if (rows < 0 || capacity <= 0 || max_parts < 1 || ld < capacity) return XML_ERR_BAD_ARG;
  const int words = (capacity + 31) / 32;
  if (out_ld < words || allow_ld < words || (allow_rows != 1 && allow_rows != rows)) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  const int slice = 65535 * FOLD_ROWS;           // grid.y limit: slices of rows, same stream (one launch up to 2 097 120 rows)
  for (int r0 = 0; r0 < rows; r0 += slice) {
    const int nr = rows - r0 < slice ? rows - r0 : slice;
    hipLaunchKernelGGL(chain_best_allow_kernel, dim3((capacity + 255) / 256, (nr + FOLD_ROWS - 1) / FOLD_ROWS), dim3(256), 0,
                       (hipStream_t)stream, scores + (int64_t)r0 * ld, ld, nr, capacity, chain_head, chain_next, max_parts,
                       allow_rows != 1 ? video_allow + (int64_t)r0 * allow_ld : video_allow, allow_ld,
                       allow_rows == 1 ? 1 : nr, out_bits + (int64_t)r0 * out_ld, out_ld);
  }
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_chain_best_rows(const float* scores, int64_t ld, int rows, int capacity, const int32_t* chain_head,
                                   const int32_t* chain_next, int max_parts, const int32_t* video, int32_t* out,
                                   xml_stream_t stream) {
  XML_ENTER();
  if (!scores || !chain_head || !chain_next || !video || !out) return XML_ERR_BAD_ARG;
  if (rows < 0 || capacity <= 0 || max_parts < 1 || ld < capacity) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  hipLaunchKernelGGL(chain_best_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, ld, rows,
                     capacity, chain_head, chain_next, max_parts, video, out);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
