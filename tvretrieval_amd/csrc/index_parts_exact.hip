// Long videos on an EXACT-RANK index that takes updates (include/xmlhip_index_parts_exact.h).  The
// exact-rank chains never form the f32 (Nq, slots) matrix that index_parts.hip folds; they hold candidate lists -- per query m
// slots and their re-scored values -- and the fold of a video's parts runs on those:
//   xml_cand_best_part       each group of candidates (the parts of one video) reduced to its best member
//   xml_chain_spread_allow   a caller's head-bit mask made per-slot, for the selections that propose candidates
//   xml_chain_members        the slots of one video as a list, for SVMR
// The chain tables are those of index_parts.hip and nothing here trusts them either: every table value is range-checked before
// it is used as an index, and the one walk is bounded by max_parts.
#include "../../include/xmlhip_index_parts_exact.h"
#include "common.h"

namespace {

constexpr int CAND_MAX_M = 4096;   // inference.EXACT_TIER2_CAP: the widest list the exact-rank chains re-score
constexpr int CAND_THREADS = 256;

__device__ __forceinline__ bool in_range(int s, int n) { return (unsigned)s < (unsigned)n; }

__host__ __device__ inline int cand_table_size(int m) {        // slots of the hash table: a power of two >= 2 m
  int t = 64;
  while (t < 2 * m) t <<= 1;
  return t;
}

// One workgroup per row.  LDS (dynamic, 4 m + 4 T + 4 ceil(m / 32) bytes, T = cand_table_size(m); 48.5 KiB at m = 4096):
//   s_key[m]    the candidate's group: group[id] in [0, n); -1 an EMPTY candidate (id outside [0, n)); -2 - position a
//               candidate whose group value lies outside [0, n) -- a group of its own
//   s_tab[T]    phase 1: an open-addressing table group -> the position that claimed it (entries are POSITIONS; the key of an
//               entry is s_key[entry]).  A candidate that finds its group claimed marks the claimant and itself in s_multi.
//               phase 2: the same memory holds s_val[m] (v = isnan(s) ? -inf : s) and s_ord[m] (order[id]) -- T >= 2 m.
//   s_multi     one bit per position: the candidate shares its group with another one of the row
// Only a candidate with its s_multi bit scans the row (LDS broadcast reads of s_key, the few matches read s_val / s_ord); the
// others -- every one-part video, and every video of which one part was proposed -- are done after phase 1.
// Position i is read and written by thread i % 256 alone, and every read of a row's inputs precedes that thread's write: the
// fold may run in place.
__global__ __launch_bounds__(CAND_THREADS) void cand_best_part_kernel(
    const float* scores, const int32_t* ids, int64_t ld, int m, const int32_t* __restrict__ group,
    const int32_t* __restrict__ order, int n, float* out_scores, int32_t* out_ids, int64_t out_ld) {   // (out may be in)
  extern __shared__ __attribute__((aligned(16))) int32_t s_mem[];
  const int T = cand_table_size(m);
  int32_t* s_key = s_mem;
  int32_t* s_tab = s_mem + m;
  uint32_t* s_multi = (uint32_t*)(s_mem + m + T);
  float* s_val = (float*)s_tab;
  int32_t* s_ord = s_tab + m;
  const int tid = threadIdx.x;
  const float* sr = scores + (int64_t)blockIdx.x * ld;
  const int32_t* ir = ids + (int64_t)blockIdx.x * ld;

  for (int i = tid; i < m; i += CAND_THREADS) {
    const int id = ir[i];
    int key = -1;
    if (in_range(id, n)) {
      const int g = group[id];
      key = in_range(g, n) ? g : -2 - i;
    }
    s_key[i] = key;
  }
  for (int i = tid; i < T; i += CAND_THREADS) s_tab[i] = -1;
  for (int i = tid; i < (m + 31) / 32; i += CAND_THREADS) s_multi[i] = 0u;
  __syncthreads();

  // phase 1: who shares a group.  At most m <= T / 2 entries are ever claimed, so a probe meets a free entry within T steps.
  for (int i = tid; i < m; i += CAND_THREADS) {
    const int key = s_key[i];
    if (key < 0) continue;
    uint32_t h = ((uint32_t)key * 2654435761u) >> 7;
    for (int step = 0; step < T; ++step, ++h) {
      const int at = (int)(h & (uint32_t)(T - 1));
      const int old = atomicCAS(&s_tab[at], -1, i);
      if (old == -1) break;                                    // claimed: the first of its group so far
      if (in_range(old, m) && s_key[old] == key) {             // (s_key is not written after the barrier above)
        atomicOr(&s_multi[old >> 5], 1u << (old & 31));
        atomicOr(&s_multi[i >> 5], 1u << (i & 31));
        break;
      }
    }
  }
  __syncthreads();

  // phase 2: the table's memory becomes the values and orders of the row
  for (int i = tid; i < m; i += CAND_THREADS) {
    const float s = sr[i];
    const int key = s_key[i];
    s_val[i] = (s != s) ? -INFINITY : s;
    s_ord[i] = key == -1 ? 0 : order[ir[i]];                   // (key != -1: the id is in range)
  }
  __syncthreads();

  for (int i = tid; i < m; i += CAND_THREADS) {
    float s = sr[i];
    int id = ir[i];
    if ((s_multi[i >> 5] >> (i & 31)) & 1u) {
      const int key = s_key[i];
      const float vi = s_val[i];
      const int oi = s_ord[i];
      bool lose = false;
      for (int j = 0; j < m && !lose; ++j) {
        if (s_key[j] != key || j == i) continue;
        const float vj = s_val[j];
        const int oj = s_ord[j];
        lose = vj > vi || (vj == vi && (oj < oi || (oj == oi && j < i)));
      }
      if (lose) { s = -INFINITY; id = -1; }
    }
    out_scores[(int64_t)blockIdx.x * out_ld + i] = s;
    out_ids[(int64_t)blockIdx.x * out_ld + i] = id;
  }
}

// grid (ceil(capacity / 256), min(rows, 65535)): one thread per slot, one wave per two output words; the rows of a grid column
// are walked with the grid's y stride, the slot's head is loaded once for all of them.
__global__ __launch_bounds__(256) void chain_spread_allow_kernel(const uint32_t* __restrict__ video_allow, int64_t allow_ld,
                                                                 int allow_rows, int rows, int capacity,
                                                                 const int32_t* __restrict__ chain_head,
                                                                 uint32_t* __restrict__ out_bits, int64_t out_ld) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int h = -1;
  if (s < capacity) {
    h = chain_head[s];
    if (!in_range(h, capacity)) h = -1;                        // a head outside the table: the slot's bit is 0
  }
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    bool set = false;
    if (h >= 0) {
      const uint32_t* a = video_allow + (allow_rows == 1 ? 0 : (int64_t)row * allow_ld);
      set = (a[h >> 5] >> (h & 31)) & 1u;
    }
    const unsigned long long bal = __ballot(set);              // (every lane of the wave arrives here)
    if ((lane & 31) == 0 && s < capacity)                      // s is a multiple of 32: word s >> 5 exists; its padding bits are 0
      out_bits[(int64_t)row * out_ld + (s >> 5)] = (uint32_t)(bal >> lane);
  }
}

// one thread per row: the chain of video[row] from its head, at most max_parts slots, -1 behind its end
__global__ __launch_bounds__(256) void chain_members_kernel(const int32_t* __restrict__ video, int rows, int capacity,
                                                            const int32_t* __restrict__ chain_head,
                                                            const int32_t* __restrict__ chain_next, int max_parts,
                                                            int32_t* __restrict__ out, int64_t out_ld) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int v = video[row];
  int j = -1;
  if (in_range(v, capacity)) j = chain_head[v];
  int32_t* o = out + (int64_t)row * out_ld;
  for (int i = 0; i < max_parts; ++i) {
    const bool ok = in_range(j, capacity);
    o[i] = ok ? j : -1;
    j = ok ? chain_next[j] : -1;
  }
}

}  // namespace

extern "C" int xml_cand_best_part_max_m(void) { return CAND_MAX_M; }

extern "C" int xml_cand_best_part(const float* scores, const int32_t* ids, int64_t ld, int rows, int m, const int32_t* group,
                                  const int32_t* order, int n, float* out_scores, int32_t* out_ids, int64_t out_ld,
                                  xml_stream_t stream) {
  XML_ENTER();
  if (!scores || !ids || !group || !order || !out_scores || !out_ids) return XML_ERR_BAD_ARG;
  if (rows < 0 || m < 1 || m > xml_cand_best_part_max_m() || ld < m || out_ld < m || n <= 0) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  const size_t lds = 4u * ((size_t)m + (size_t)cand_table_size(m) + (size_t)((m + 31) / 32));   // <= 49 664 bytes
  hipLaunchKernelGGL(cand_best_part_kernel, dim3(rows), dim3(CAND_THREADS), lds, (hipStream_t)stream, scores, ids, ld, m,
                     group, order, n, out_scores, out_ids, out_ld);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_chain_spread_allow(const uint32_t* video_allow, int64_t allow_ld, int allow_rows, int rows, int capacity,
                                      const int32_t* chain_head, uint32_t* out_bits, int64_t out_ld, xml_stream_t stream) {
  XML_ENTER();
  if (!video_allow || !chain_head || !out_bits) return XML_ERR_BAD_ARG;
  if (rows < 0 || capacity <= 0) return XML_ERR_BAD_ARG;
  const int words = (capacity + 31) / 32;
  if (out_ld < words || allow_ld < words || (allow_rows != 1 && allow_rows != rows)) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  hipLaunchKernelGGL(chain_spread_allow_kernel, dim3((capacity + 255) / 256, rows < 65535 ? rows : 65535), dim3(256), 0,
                     (hipStream_t)stream, video_allow, allow_ld, allow_rows, rows, capacity, chain_head, out_bits, out_ld);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_chain_members(const int32_t* video, int rows, int capacity, const int32_t* chain_head,
                                 const int32_t* chain_next, int max_parts, int32_t* out, int64_t out_ld, xml_stream_t stream) {
  XML_ENTER();
  if (!video || !chain_head || !chain_next || !out) return XML_ERR_BAD_ARG;
  if (rows < 0 || capacity <= 0 || max_parts < 1 || out_ld < max_parts) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  hipLaunchKernelGGL(chain_members_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, video, rows, capacity,
                     chain_head, chain_next, max_parts, out, out_ld);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
