// What the one-launch backward passes of the in-batch video-level scores share (loss_tail.hip: xml_q2c_scores_l2norm_bwd;
// train_index.hip: xml_q2c_scores_arg_bwd_q): the in-order list of the pairs of a row of dscores that carry a gradient, and
// the limits both entries answer for through xml_q2c_scores_l2norm_bwd_supported.
#pragma once
#include "common.h"

namespace {

// In-order compaction of the non-zero entries of g[0 .. count) (stride `stride`) into s_idx / s_val (capacity cap, checked by
// the caller: count <= cap).  Returns the number of entries; all threads see it after the trailing barrier.
__device__ __forceinline__ int collect_active(const float* __restrict__ g, int64_t stride, int count, float scale, int* s_idx,
                                              float* s_val, int* s_cnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int i0 = 0; i0 < count; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const float v = i < count ? g[(int64_t)i * stride] * scale : 0.f;
    const unsigned long long b = __ballot(v != 0.f);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += s_cnt[w];
    if (v != 0.f) {
      const int pos = off + __popcll(b & ((1ull << lane) - 1ull));
      s_idx[pos] = i;
      s_val[pos] = v;
    }
    base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
  }
  return base;
}

constexpr int Q2C_BWD_CAP = 1024;      // pairs with a gradient per row / column of dscores (all of them when nq, nv <= 1024)
constexpr int Q2C_BWD_MAXH = 2048;

}  // namespace
