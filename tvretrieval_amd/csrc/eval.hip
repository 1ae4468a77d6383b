// K12: the retrieval metrics of K10 / K11 records on the device -- the first consumer of the final lists that is on the device
// too, so a validation pass can end in ~40 counters instead of a copy of every list.
//   reference: eval_by_task_type / eval_retrieval   standalone_eval/eval.py:83-276
//              compute_temporal_iou_batch           standalone_eval/eval.py:40-58
// The semantics are evaluate.eval_by_task_type on the array path (the host implementation, which stays the default): f32 IoU
// on the hull with one IEEE division, `>=` thresholds, the DiDeMo >= 2-of-n rule, the matched-rank rule of SVMR, rows without
// ground truth left out of every denominator.  The result is integer counts, so it does not depend on execution order.
//
// Two launches, no workspace, no host synchronisation; capturable:
//   1. eval_first_hit_kernel: one wave per query row, four rows per workgroup.  The lanes stride over the row's records with
//      16-byte loads; the row's spans sit in LDS; "correct" and "video matches" are balloted per 64-record chunk, the first set
//      bit of a threshold is its first hit (VCMR / VR: the position; SVMR: the running count of matching records up to it);
//      the row ends once every threshold has one.
//   2. eval_count_kernel: ONE workgroup turns first_hit into hits / rows -- 64 rows per wave and step, one ballot per counter,
//      added in LDS, then plain stores: every counter is overwritten, nothing is zero-filled and nothing is atomic in memory.
#include "common.h"

#pragma clang fp contract(off)   // the IoU is min / max / subtract / divide on f32, one rounding per operation

namespace {

constexpr int EVAL_MAX_THD = 4, EVAL_MAX_K = 8, EVAL_MAX_TS = 16, EVAL_ROWS_PER_WG = 4;

struct EvalThds { float v[EVAL_MAX_THD]; };
struct EvalTopks { int v[EVAL_MAX_K]; };

// np.maximum / np.minimum on f32: a NaN in either operand propagates
__device__ __forceinline__ float npmax(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float npmin(float a, float b) { return (a <= b || a != a) ? a : b; }

// compute_temporal_iou_batch on one (prediction, span) pair
__device__ __forceinline__ float tiou_f32(float st, float ed, float g_st, float g_ed) {
  const float inter = npmax(0.f, npmin(ed, g_ed) - npmax(st, g_st));
  const float uni = npmax(ed, g_ed) - npmin(st, g_st);         // hull, as in the reference
  return uni != 0.f ? inter / uni : 0.f;
}

__global__ __launch_bounds__(64 * EVAL_ROWS_PER_WG) void eval_first_hit_kernel(
    const xml_moment* __restrict__ rec, int64_t ld_rec, const int32_t* __restrict__ count, int nq, int n, int task,
    double scale, int max_pred, const int32_t* __restrict__ gt_vid, const float* __restrict__ gt_ts, int n_ts,
    const int32_t* __restrict__ n_gt, EvalThds thd, int n_thd, int32_t* __restrict__ first_hit) {
  __shared__ float s_ts[EVAL_ROWS_PER_WG][EVAL_MAX_TS][2];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * EVAL_ROWS_PER_WG + w;
  const bool row = q < nq;
  int ng = row ? n_gt[q] : 0;
  ng = min(max(ng, 0), n_ts);
  const bool multi = ng >= 4;                                  // DiDeMo: that many spans, >= 2 of them must hit
  const int n_span = multi ? ng : (ng > 0 ? 1 : 0);
  if (lane < 2 * n_span) (&s_ts[w][0][0])[lane] = gt_ts[(int64_t)q * n_ts * 2 + lane];
  __syncthreads();
  if (!row) return;
  int fh[EVAL_MAX_THD] = {0, 0, 0, 0};
  if (n_span > 0) {
    int m = count ? count[q] : n;
    m = min(min(max(m, 0), n), max_pred);
    const int g_vid = gt_vid[q];
    const xml_moment* r = rec + (int64_t)q * ld_rec;
    int matched = 0, found = 0;                                // SVMR: matching records before this chunk; thresholds done
    for (int base = 0; base < m && found < n_thd; base += 64) {
      const int i = base + lane;
      bool match = false;
      int hit_spans[EVAL_MAX_THD] = {0, 0, 0, 0};
      if (i < m) {
        const uint4 raw = *reinterpret_cast<const uint4*>(&r[i]);
        match = (int)raw.x == g_vid;
        if (task != 2) {
          const float st = (float)((double)__uint_as_float(raw.y) * scale);
          const float ed = (float)((double)__uint_as_float(raw.z) * scale);
          const float vm = match ? 1.f : 0.f;
          for (int j = 0; j < n_span; ++j) {
            const float iou = tiou_f32(st, ed, s_ts[w][j][0], s_ts[w][j][1]) * vm;
#pragma unroll
            for (int t = 0; t < EVAL_MAX_THD; ++t) hit_spans[t] += (t < n_thd && iou >= thd.v[t]) ? 1 : 0;
          }
        }
      }
      const unsigned long long mb = __ballot(match);
      found = 0;
#pragma unroll
      for (int t = 0; t < EVAL_MAX_THD; ++t) {
        if (t >= n_thd) continue;
        bool correct;
        if (task == 2) correct = match;                        // VR: the video alone
        else correct = (i < m) && (multi ? hit_spans[t] >= 2 : hit_spans[t] >= 1);
        if (task == 1) correct = correct && match;             // SVMR counts among the predictions of the query's video
        const unsigned long long cb = __ballot(correct);
        if (fh[t] == 0 && cb != 0) {
          const int first = __ffsll((long long)cb) - 1;
          fh[t] = task == 1 ? matched + (int)__popcll(mb & ((2ull << first) - 1ull)) : base + first + 1;
        }
        found += fh[t] != 0;
      }
      matched += (int)__popcll(mb);
    }
  }
  if (lane < n_thd) {
    int v = fh[0];
#pragma unroll
    for (int t = 1; t < EVAL_MAX_THD; ++t) v = lane == t ? fh[t] : v;
    first_hit[(int64_t)q * n_thd + lane] = v;
  }
}

constexpr int EVAL_COUNT_THREADS = 1024;
constexpr int EVAL_N_COUNTERS = 4 * EVAL_MAX_THD * EVAL_MAX_K;

__global__ __launch_bounds__(EVAL_COUNT_THREADS) void eval_count_kernel(
    const int32_t* __restrict__ first_hit, const int32_t* __restrict__ n_gt, const int32_t* __restrict__ desc_type, int nq,
    int n_thd, EvalTopks topk, int n_k, int32_t* __restrict__ hits, int32_t* __restrict__ rows) {
  __shared__ int s_hits[EVAL_N_COUNTERS];
  __shared__ int s_rows[4];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < EVAL_N_COUNTERS; i += EVAL_COUNT_THREADS) s_hits[i] = 0;
  if (tid < 4) s_rows[tid] = 0;
  __syncthreads();
  for (int q0 = (tid >> 6) * 64; q0 < nq; q0 += EVAL_COUNT_THREADS) {      // (wave-uniform trip count)
    const int q = q0 + lane;
    const bool counted = q < nq && n_gt[q] != 0;
    const int dt = (counted && desc_type) ? desc_type[q] : -1;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const unsigned long long b = __ballot(counted && (g == 0 || dt == g - 1));
      if (lane == 0 && b) atomicAdd(&s_rows[g], (int)__popcll(b));
    }
    for (int t = 0; t < n_thd; ++t) {
      const int fh = counted ? first_hit[(int64_t)q * n_thd + t] : 0;
      for (int k = 0; k < n_k; ++k) {
        const bool hit = fh >= 1 && fh <= topk.v[k];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const unsigned long long b = __ballot(hit && (g == 0 || dt == g - 1));
          if (lane == 0 && b) atomicAdd(&s_hits[(g * n_thd + t) * n_k + k], (int)__popcll(b));
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 4 * n_thd * n_k; i += EVAL_COUNT_THREADS) hits[i] = s_hits[i];
  if (tid < 4) rows[tid] = s_rows[tid];
}

}  // namespace

extern "C" int xml_eval_moments(const xml_moment* rec, int64_t ld_rec, const int32_t* count, int nq, int n, int task,
                                double scale, int max_pred, const int32_t* gt_vid, const float* gt_ts, int n_ts,
                                const int32_t* n_gt, const int32_t* desc_type, const float* iou_thd, int n_thd,
                                const int32_t* topk, int n_k, int32_t* first_hit, int32_t* hits, int32_t* rows,
                                xml_stream_t stream) {
  XML_ENTER();
  static_assert(sizeof(xml_moment) == 16, "xml_moment is a 16-byte record");
  if (!rec || !gt_vid || !gt_ts || !n_gt || !topk || !first_hit || !hits || !rows) return XML_ERR_BAD_ARG;
  if (task < 0 || task > 2 || (task != 2 && !iou_thd)) return XML_ERR_BAD_ARG;
  if (nq < 0 || n < 1 || n > 1024 || ld_rec < n || ((uintptr_t)rec & 15) != 0) return XML_ERR_BAD_ARG;
  if (n_thd < 1 || n_thd > EVAL_MAX_THD || n_k < 1 || n_k > EVAL_MAX_K || n_ts < 1 || n_ts > EVAL_MAX_TS) return XML_ERR_BAD_ARG;
  if (max_pred < 0 || scale != scale) return XML_ERR_BAD_ARG;
  EvalTopks ks = {};
  for (int k = 0; k < n_k; ++k) {
    if (topk[k] < 1 || (k > 0 && topk[k] <= topk[k - 1])) return XML_ERR_BAD_ARG;
    ks.v[k] = topk[k];
  }
  if (task == 2) n_thd = 1;                                    // VR has no IoU: one column of first_hit, one plane of hits
  EvalThds thds = {};
  for (int t = 0; t < n_thd && task != 2; ++t) thds.v[t] = iou_thd[t];
  if (nq == 0) return XML_OK;
  const int blocks = (nq + EVAL_ROWS_PER_WG - 1) / EVAL_ROWS_PER_WG;
  hipLaunchKernelGGL(eval_first_hit_kernel, dim3(blocks), dim3(64 * EVAL_ROWS_PER_WG), 0, (hipStream_t)stream, rec, ld_rec,
                     count, nq, n, task, scale, max_pred, gt_vid, gt_ts, n_ts, n_gt, thds, n_thd, first_hit);
  XML_CHECK_LAUNCH();
  hipLaunchKernelGGL(eval_count_kernel, dim3(1), dim3(EVAL_COUNT_THREADS), 0, (hipStream_t)stream, first_hit, n_gt, desc_type,
                     nq, n_thd, ks, n_k, hits, rows);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
