// Parts of long videos folded back into videos between K6 and K8 (include/xmlhip.h "Videos longer than max_ctx_l").
//   A video of more than max_ctx_l clips is stored as several overlapping PARTS, each an ordinary index row; K6 scores the
//   parts, and only the best part of each video competes in K8.  xml_group_best_allow turns K6's (rows, n_parts) scores into
//   the allow-bit matrix of xml_topk_rows_allowed: bit p is set iff p is the best part of its video for that row and the
//   caller allows the video.  xml_best_part_rows answers the same question for one named video per row (SVMR, ground truth).
// Best part of a group [b, e): the running best starts as (row b, -inf) and a part replaces it when its score is strictly
// greater -- ties go to the lowest row, a NaN never wins, a group of nothing but -inf / NaN keeps row b.
// Traffic: at most one pass over the scores (rows * n_parts * 4 bytes; the re-reads inside a group hit the same lines, and
// the score of a video's ONLY part is never read), rows * ceil(n_parts / 32) words written.  Measured, the fold is NOT
// bandwidth-bound: 0.229 ms for 10 000 x 21 914 scores of which 37 MB have to move, 1.65 x the time of streaming the whole
// matrix once (profiles/parts_timing.md); a form with more instructions per row is slower by 41 %, so it is the work per row.
#include "common.h"

namespace {

// best part of group [b, e) of one score row (b < e)
__device__ __forceinline__ int best_of_group(const float* __restrict__ s, int b, int e) {
  int best = b;
  float bv = -INFINITY;
  for (int j = b; j < e; ++j) {
    const float v = s[j];
    if (v > bv) { bv = v; best = j; }
  }
  return best;
}

// grid (ceil(n_parts / 256), ceil(rows / FOLD_ROWS)); one thread per part and FOLD_ROWS score rows, one wave per two output
// words of each row.  The part's group is looked up once (three dependent loads: with one row per thread that chain, not the
// scores, set the time -- 0.91 ms for 10 000 x 21 914, 6.6 x the byte floor) and serves every row.  A thread walks its WHOLE
// group, wherever it starts or ends: a group that begins in an earlier word, ends in a later one or spans several is seen in
// full by every thread of it, and each of them finds the same best part -- G^2 score loads per row for a group of G parts
// (1-2 on TVR).  A per-thread test that leaves at the first part that beats it was measured and not kept: 0.323 against
// 0.229 ms at the TVR shape, where the work per row of the loop below, not the loads, sets the time.  One pass per group
// with a wave reduction is the form for videos of hundreds of parts; not built.  The only part of a video is its best part whatever
// it scores: those rows are not read at all.
constexpr int FOLD_ROWS = 32;      // (0.23 ms at that shape, 8: 0.26 ms -- profiles/parts_timing.md)

__global__ __launch_bounds__(256) void group_best_allow_kernel(
    const float* __restrict__ scores, int64_t ld, int rows, int n_parts, const int32_t* __restrict__ part_video,
    const int32_t* __restrict__ group_start, int n_videos, const uint32_t* __restrict__ video_allow, int64_t allow_ld,
    int allow_rows, uint32_t* __restrict__ out_bits, int64_t out_ld) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int g = 0, b = 0, e = 0;
  bool in_group = false;
  if (p < n_parts) {
    g = part_video[p];
    if (g >= 0 && g < n_videos) {
      b = max(group_start[g], 0), e = min(group_start[g + 1], n_parts);
      in_group = b <= p && p < e;
    }
  }
  const bool single = e - b == 1;
  const int row0 = blockIdx.y * FOLD_ROWS;
#pragma unroll 4
  for (int r = 0; r < FOLD_ROWS; ++r) {
    const int row = row0 + r;
    if (row >= rows) break;                                // (uniform over the workgroup)
    bool set = false;
    if (in_group) {
      bool allowed = true;
      if (video_allow) {
        const uint32_t* a = video_allow + (allow_rows == 1 ? 0 : (int64_t)row * allow_ld);
        allowed = (a[g >> 5] >> (g & 31)) & 1u;
      }
      if (allowed) set = single || best_of_group(scores + (int64_t)row * ld, b, e) == p;
    }
    const unsigned long long bal = __ballot(set);          // (every lane of the wave arrives here)
    if ((lane & 31) == 0 && p < n_parts)                   // p is a multiple of 32: word p >> 5 exists; its padding bits are 0
      out_bits[(int64_t)row * out_ld + (p >> 5)] = (uint32_t)(bal >> lane);
  }
}

__global__ __launch_bounds__(256) void best_part_rows_kernel(
    const float* __restrict__ scores, int64_t ld, int rows, const int32_t* __restrict__ group_start, int n_videos,
    const int32_t* __restrict__ video, int32_t* __restrict__ out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int g = video[row];
  int r = -1;
  if (g >= 0 && g < n_videos) {
    const int n_parts = (int)min((int64_t)group_start[n_videos], ld);       // (a row holds no more than ld scores)
    const int b = max(group_start[g], 0), e = min(group_start[g + 1], n_parts);
    if (b < e) r = best_of_group(scores + (int64_t)row * ld, b, e);
  }
  out[row] = r;
}

}  // namespace

extern "C" int xml_group_best_allow(const float* scores, int64_t ld, int rows, int n_parts, const int32_t* part_video,
                                    const int32_t* group_start, int n_videos, const uint32_t* video_allow,
                                    int64_t allow_ld, int allow_rows, uint32_t* out_bits, int64_t out_ld,
                                    xml_stream_t stream) {
  XML_ENTER();
  if (!scores || !part_video || !group_start || !out_bits) return XML_ERR_BAD_ARG;
  if (rows < 0 || n_parts <= 0 || n_videos <= 0 || n_videos > n_parts || ld < n_parts) return XML_ERR_BAD_ARG;
  if (out_ld < (n_parts + 31) / 32) return XML_ERR_BAD_ARG;
  if (video_allow && (allow_ld < (n_videos + 31) / 32 || (allow_rows != 1 && allow_rows != rows))) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  const int slice = 65535 * FOLD_ROWS;           // grid.y limit: slices of rows, same stream (one launch up to 2 097 120 rows)
  for (int r0 = 0; r0 < rows; r0 += slice) {
    const int nr = rows - r0 < slice ? rows - r0 : slice;
    hipLaunchKernelGGL(group_best_allow_kernel, dim3((n_parts + 255) / 256, (nr + FOLD_ROWS - 1) / FOLD_ROWS), dim3(256), 0,
                       (hipStream_t)stream, scores + (int64_t)r0 * ld, ld, nr, n_parts, part_video, group_start, n_videos,
                       (video_allow && allow_rows != 1) ? video_allow + (int64_t)r0 * allow_ld : video_allow, allow_ld,
                       allow_rows == 1 ? 1 : nr, out_bits + (int64_t)r0 * out_ld, out_ld);
  }
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_best_part_rows(const float* scores, int64_t ld, int rows, const int32_t* group_start, int n_videos,
                                  const int32_t* video, int32_t* out, xml_stream_t stream) {
  XML_ENTER();
  if (!scores || !group_start || !video || !out) return XML_ERR_BAD_ARG;
  if (rows < 0 || n_videos <= 0 || ld < n_videos) return XML_ERR_BAD_ARG;
  if (rows == 0) return XML_OK;
  hipLaunchKernelGGL(best_part_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, ld, rows,
                     group_start, n_videos, video, out);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
