// K11: greedy temporal NMS of K10's records on the device -- one more launch behind xml_moments_decode.
//   reference: temporal_non_maximum_suppression   utils/temporal_nms.py:25-74
//              filter_vcmr_by_nms                 baselines/clip_alignment_with_language/inference.py:189-225
//              post_processing_svmr_nms           baselines/clip_alignment_with_language/inference.py:247-265
// The semantics are vcmr_row / svmr_row of postproc.hip (the host implementation, which stays the default): the result is a
// selection and an order of existing records, decided by f32 score comparisons and by `iou > thd` in float64 with one IEEE
// division -- the same operations on the same values as the host's, so the two agree bit for bit.
//
// One workgroup per query row (one wave up to 256 entries, four above), everything in LDS:
//   1. group id of an entry = position of the first entry with its video (the reference's dict by first appearance);
//   2. rank by counting on the 64-bit key (group, score descending, position): the groups become contiguous segments of one
//      sorted order, each in the order its greedy walk visits;
//   3. the walks of ALL groups advance together, one head per group and round: every pending entry takes one IoU against its
//      group's head, the survivors elect the next head with an LDS atomic min.  Rounds = the largest kept count of a group
//      (<= 100, the reference's per-video cap), not the number of entries;
//   4. rank by counting of the kept entries on (score descending, group, position) = the reference's stable sort of the
//      merged per-video lists; gather the records.
// No workspace, no host synchronisation; capturable.
#include "common.h"

#pragma clang fp contract(off)   // the IoU is min / max / subtract / divide on float64, one rounding per operation

namespace {

constexpr int NMS_GROUP_CAP = 100;        // temporal_non_maximum_suppression's default max_after_nms, which both callers keep
constexpr int NMS_NONE = 0x7fffffff;

enum { PENDING = 0, KEPT = 1, DEAD = 2 };

// f32 score -> 32-bit key, ascending key = DESCENDING score; -0 and +0 compare equal like the floats do.  (A NaN lands at one
// end instead of breaking the order: the ranks below are a permutation whatever the scores are.)
__device__ __forceinline__ uint32_t score_key_desc(float s) {
  if (s == 0.f) s = 0.f;
  const uint32_t b = __float_as_uint(s);
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;
}

// std::min / std::max of postproc.hip's tiou, operand order included
__device__ __forceinline__ double dmax(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double dmin(double a, double b) { return (b < a) ? b : a; }

__device__ __forceinline__ double tiou(double s0, double e0, double s1, double e1) {
  const double inter = dmax(0.0, dmin(e0, e1) - dmax(s0, s1));
  const double uni = dmax(e0, e1) - dmin(s0, s1);      // hull, as in the reference
  return uni == 0 ? 0.0 : inter / uni;
}

// LDS per entry of the row's capacity: two keys, st, ed (8 bytes each) + six int32 columns
constexpr int NMS_LDS_PER_ENTRY = 4 * 8 + 6 * 4;

__global__ __launch_bounds__(256) void nms_moments_kernel(
    const xml_moment* __restrict__ in, int64_t ld_in, const int32_t* __restrict__ count, int n, int cap, int by_video,
    double thd, double scale, int max_before, int max_after, xml_moment* __restrict__ out, int64_t ld_out,
    int32_t* __restrict__ out_index, int64_t ld_index, int32_t* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  uint64_t* s_key = reinterpret_cast<uint64_t*>(nms_lds);      // walk key (group, score desc, position) by input position
  uint64_t* s_fkey = s_key + cap;                              // by sorted position: output key (score desc, group, position)
  double* s_st = reinterpret_cast<double*>(s_fkey + cap);
  double* s_ed = s_st + cap;
  int* s_pos = reinterpret_cast<int*>(s_ed + cap);             // sorted position -> input position
  int* s_gs = s_pos + cap;                                     // sorted position -> first sorted position of its group
  int* s_state = s_gs + cap;
  int* s_head = s_state + cap;                                 // per group (indexed by its first sorted position): current head
  int* s_next = s_head + cap;                                  //   first survivor behind the head; the video ids in phase 1
  int* s_kept = s_next + cap;                                  //   kept so far
  int* s_vid = s_next;

  const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const xml_moment* row = in + (int64_t)q * ld_in;
  int m = count ? count[q] : n;
  m = min(min(max(m, 0), n), max_before);                      // <= cap = min(n, max_before)

  // 1. group = first position of the entry's video
  for (int i = tid; i < m; i += nt) s_vid[i] = row[i].vid;
  __syncthreads();
  for (int i = tid; i < m; i += nt) {
    int gf = 0;
    if (by_video) {
      const int v = s_vid[i];
      while (s_vid[gf] != v) ++gf;                             // ends at gf == i at the latest
    }
    s_key[i] = ((uint64_t)gf << 42) | ((uint64_t)score_key_desc(row[i].score) << 10) | (uint64_t)i;
  }
  __syncthreads();
  // 2. sorted position = number of smaller keys (the keys are distinct: they end in the position)
  for (int i = tid; i < m; i += nt) {
    const uint64_t k = s_key[i];
    const uint64_t g0 = k >> 42 << 42;
    int r = 0, gs = 0;
    for (int j = 0; j < m; ++j) {
      const uint64_t kj = s_key[j];                            // the same address in every lane: a broadcast
      r += kj < k;
      gs += kj < g0;
    }
    const xml_moment rec = row[i];
    s_st[r] = (double)rec.st * scale;
    s_ed[r] = (double)rec.ed * scale;
    s_pos[r] = i;
    s_fkey[r] = ((k >> 10 & 0xffffffffull) << 20) | (k >> 42 << 10) | (uint64_t)i;
    s_gs[r] = gs;
    s_state[r] = PENDING;
    s_head[r] = r;                                             // (read at group starts only, where r == gs)
    s_next[r] = NMS_NONE;
    s_kept[r] = 0;
  }
  __syncthreads();                                             // (also: every read of s_vid / s_key above is done)
  // 3. one head per group and round
  for (;;) {
    for (int p = tid; p < m; p += nt) {
      if (s_state[p] != PENDING) continue;
      const int g = s_gs[p], h = s_head[g];
      if (h < 0) {
        s_state[p] = DEAD;                                     // behind the per-group cap
      } else if (p == h) {
        s_state[p] = KEPT;                                     // one head per group: nobody else touches s_kept[g] here
        s_kept[g] += 1;
      } else if (tiou(s_st[h], s_ed[h], s_st[p], s_ed[p]) > thd) {
        s_state[p] = DEAD;
      } else {
        atomicMin(&s_next[g], p);
      }
    }
    __syncthreads();
    int active = 0;
    for (int p = tid; p < m; p += nt) {
      if (s_gs[p] != p || s_head[p] < 0) continue;
      const int nx = s_next[p];
      if (nx == NMS_NONE || s_kept[p] >= NMS_GROUP_CAP) {
        s_head[p] = -1;
      } else {
        s_head[p] = nx;
        active = 1;
      }
      s_next[p] = NMS_NONE;
    }
    if (!__syncthreads_or(active)) break;
  }
  // 4. output order: (score descending, group, position) over the kept entries
  int mine = 0;
  for (int p = tid; p < m; p += nt) {
    if (s_state[p] == KEPT) ++mine;
    else s_fkey[p] = ~0ull;
  }
  __syncthreads();
  for (int p = tid; p < m; p += nt) {
    const uint64_t f = s_fkey[p];
    if (f == ~0ull) continue;
    int r = 0;
    for (int j = 0; j < m; ++j) r += s_fkey[j] < f;
    if (r < max_after) {
      const int i = s_pos[p];
      if (out_index) out_index[(int64_t)q * ld_index + r] = i;
      if (out) *reinterpret_cast<uint4*>(&out[(int64_t)q * ld_out + r]) = *reinterpret_cast<const uint4*>(&row[i]);
    }
  }
  // total kept: block sum of `mine`
  __shared__ int s_total;
  if (tid == 0) s_total = 0;
  __syncthreads();
  if (mine) atomicAdd(&s_total, mine);
  __syncthreads();
  const int k_out = min(s_total, max_after);
  for (int r = k_out + tid; r < max_after; r += nt) {
    if (out_index) out_index[(int64_t)q * ld_index + r] = -1;
    if (out) *reinterpret_cast<uint4*>(&out[(int64_t)q * ld_out + r]) = make_uint4(0xffffffffu, 0u, 0u, 0u);
  }
  if (out_count && tid == 0) out_count[q] = k_out;
}

}  // namespace

extern "C" int xml_nms_moments(const xml_moment* in, int64_t ld_in, const int32_t* count, int nq, int n, int by_video,
                               double thd, double scale, int max_before, int max_after, xml_moment* out, int64_t ld_out,
                               int32_t* out_index, int64_t ld_index, int32_t* out_count, xml_stream_t stream) {
  XML_ENTER();
  static_assert(sizeof(xml_moment) == 16, "xml_moment is a 16-byte record");
  if (!in || (!out && !out_index && !out_count) || nq < 0 || n < 1 || n > 1024 || ld_in < n) return XML_ERR_BAD_ARG;
  if (max_before < 0 || max_after < 0 || thd != thd || scale != scale) return XML_ERR_BAD_ARG;
  if ((out && ld_out < max_after) || (out_index && ld_index < max_after)) return XML_ERR_BAD_ARG;
  if (((uintptr_t)in & 15) != 0 || ((uintptr_t)out & 15) != 0) return XML_ERR_BAD_ARG;
  if (nq == 0) return XML_OK;
  const int cap = n < max_before ? n : (max_before > 0 ? max_before : 1);
  const int threads = cap <= 256 ? 64 : 256;
  const size_t lds = (size_t)cap * NMS_LDS_PER_ENTRY;          // 56 KiB at cap = 1024
  hipLaunchKernelGGL(nms_moments_kernel, dim3(nq), dim3(threads), lds, (hipStream_t)stream, in, ld_in, count, n, cap,
                     by_video ? 1 : 0, thd, scale, max_before, max_after, out, ld_out, out_index, ld_index, out_count);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
