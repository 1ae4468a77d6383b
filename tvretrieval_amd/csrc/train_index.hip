// Training the query side on a resident index (include/xmlhip_train_index.h; tvretrieval_amd/train_index.py; DESIGN.md
// section 26): the context side of the model is frozen, so what its encoders would produce for the batch's videos is already
// in the index.  Three entries:
//   xml_index_gather_video_rows   the batch's cn / feat2 / mask from the index rows of its videos, both modalities, one launch
//   xml_q2c_scores_arg_bwd_q      the query half of q2c_l2_bwd_kernel (loss_tail.hip): no dfeat pass over the clip rows
//   xml_pair_sim_bwd_q            the dq half of pair_sim_bwd_vec_kernel (train.hip): no df2 store per clip row
#include "../../include/xmlhip_train_index.h"
#include "index_rows.h"
#include "loss_rows.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// The gather.  A pure copy, bandwidth-bound: reads and writes 2 * n * l * hidden elements per modality.  One thread per
// 16-byte chunk of an OUTPUT row (chunk index t = (i * l + c) * chunks + k): consecutive lanes store consecutive 16-byte
// pieces of cn and of f2, so every store instruction of a wave is one contiguous KiB.  The feat2 loads are contiguous per
// row the same way.  The image loads of a wave are contiguous per (row, 64-byte slice) and, for the rows of one block,
// across rows too (a block's slice is 1 KiB): with `chunks` = 16 (bf16 H = 128, f32 H = 64) a wave covers 4 rows = 4 pieces
// of 256 B.  A thread has its two 16-byte loads in flight together; thread k == 0 of a row also writes the row's mask.
// Items, slots and blocks out of range read nothing and give zero rows: every address is formed from checked values.
// ---------------------------------------------------------------------------------------------------------------------
struct GatherSide {          // one modality
  const char* cn_src;
  const char* f2_src;
  const float* mask_src;
  char* cn;
  char* f2;
  float* mask;
};

template <bool IMAGE>
__global__ __launch_bounds__(256) void index_gather_video_rows_kernel(
    Sides<GatherSide> sides, const int32_t* __restrict__ slot, const int32_t* __restrict__ first_block, int n,
    const int32_t* __restrict__ vlen, int64_t n_videos, int64_t n_blocks, int lpad, int L, int chunks) {
  const GatherSide& s = sides.m[blockIdx.y];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)n * L * chunks) return;
  const int64_t r = t / chunks;                        // output row (i, c)
  const int k = (int)(t - r * chunks);
  const int i = (int)(r / L), c = (int)(r - (int64_t)i * L);
  const int64_t v = slot[i];
  bool ok = v >= 0 && v < n_videos && c < lpad;
  if (ok) ok = c < vlen[v];
  int64_t row = 0;                                     // image row of the clip
  if (IMAGE && ok) {
    const int64_t fb = first_block[i];
    row = fb * k6img::BLOCK_ROWS + c;
    ok = fb >= 0 && (row >> 4) < n_blocks;
  }
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  float m = 0.f;
  if (ok) {
    const int64_t at = (v * lpad + c) * (int64_t)chunks + k;       // 16-byte piece of the row-major (n_videos, lpad, H)
    a = IMAGE ? ld_global16(k6img::row_chunk(s.cn_src, row, chunks >> 2, k)) : ld_global16(s.cn_src + at * 16);
    b = ld_global16(s.f2_src + at * 16);
    if (k == 0) m = s.mask_src[v * lpad + c];
  }
  st_global16(s.cn + t * 16, a);
  st_global16(s.f2 + t * 16, b);
  if (k == 0) s.mask[r] = m;
}

// ---------------------------------------------------------------------------------------------------------------------
// Query gradient of the in-batch scores: the query branch of q2c_l2_bwd_kernel with the arg-max clips kept by the forward
// pass, on the unpadded (nv, L, hidden) rows xml_q2c_scores_arg scored.  One workgroup per query row and modality; thread t
// owns the 8-element chunk t of the hidden dimension (hidden <= 2048); the pairs with a gradient are visited in ascending v.
// ---------------------------------------------------------------------------------------------------------------------
struct ArgBwdSet {
  const void *query, *cn;
  const float* mask;
  void* dq;
  const int32_t* arg;
  int L;
};
struct ArgBwdArgs {
  ArgBwdSet s[2];                       // blockIdx.y picks the modality
  const float* dscores;
  int64_t ld_ds, ld_arg;
  float scale, eps;
  int nv, hidden;
};

template <typename T>
__global__ __launch_bounds__(256) void q2c_arg_bwd_q_kernel(ArgBwdArgs a) {
  const ArgBwdSet& set = a.s[blockIdx.y];
  const T* __restrict__ query = (const T*)set.query;
  const T* __restrict__ cn = (const T*)set.cn;
  const float* __restrict__ mask = set.mask;
  const int32_t* __restrict__ arg = set.arg;
  T* __restrict__ dq = (T*)set.dq;
  const int L = set.L, hidden = a.hidden;
  const float eps = a.eps;
  __shared__ int s_idx[Q2C_BWD_CAP];
  __shared__ float s_val[Q2C_BWD_CAP];
  __shared__ float s_red[8];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunks = hidden >> 3;
  const int m = blockIdx.x;
  const int cnt = collect_active(a.dscores + (int64_t)m * a.ld_ds, 1, a.nv, a.scale, s_idx, s_val, s_cnt);
  const bool own = tid < chunks;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < cnt; ++j) {
    const int n = s_idx[j];
    const int bl = arg[(int64_t)m * a.ld_arg + n];
    if (bl < 0 || bl >= L) continue;                    // (never written by xml_q2c_scores_arg: nothing is read for it)
    const float gm = s_val[j] * mask[(int64_t)n * L + bl];
    if (gm != 0.f && own) {
      float cv[8];
      ld8<T>(cn + ((int64_t)n * L + bl) * hidden + tid * 8, cv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += gm * cv[e];
    }
  }
  // F.normalize backward of the query row: dx = (dy - x (x . dy) / den^2) / den, den = max(|x|, eps); a clamped norm is a
  // constant and only dy / den survives (l2norm_bwd_kernel, train.hip)
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (own) ld8<T>(query + (int64_t)m * hidden + tid * 8, x);
  float ss = 0.f, xd = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) { ss += x[e] * x[e]; xd += x[e] * acc[e]; }
  ss = wave_sum(ss);
  xd = wave_sum(xd);
  if (lane == 0) { s_red[wave] = ss; s_red[4 + wave] = xd; }
  __syncthreads();
  ss = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  xd = s_red[4] + s_red[5] + s_red[6] + s_red[7];
  const float nrm = sqrtf(ss), den = fmaxf(nrm, eps);
  if (own) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = nrm > eps ? (acc[e] - x[e] * xd / (den * den)) / den : acc[e] / den;
    st8<T>(dq + (int64_t)m * hidden + tid * 8, o);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// dq of the paired similarity: pair_sim_bwd_vec_kernel (train.hip) without the df2 stores.  One workgroup per batch row, its
// four waves take the clips l = w, w + 4, ..., four in flight; lanes hold 8-element chunks; the waves' sums meet in LDS and
// are added in one fixed order.  hidden % 8 == 0, hidden <= 2048.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pair_sim_bwd_q_kernel(const T* __restrict__ f2, const float* __restrict__ dsim,
                                                             T* __restrict__ dq, int L, int hidden) {
  __shared__ float s_acc[4][2048];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = hidden >> 3;
  for (int c0 = 0; c0 < chunks; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = c < chunks;
    const int cc = ok ? c : 0;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int l0 = wave; l0 < L; l0 += 16) {
      float fv[4][8], g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int l = min(l0 + 4 * u, L - 1);
        g[u] = (l0 + 4 * u < L) ? dsim[b * L + l] : 0.f;
        ld8<T>(f2 + (b * L + l) * hidden + cc * 8, fv[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += g[u] * fv[u][e];
    }
    if (ok)
#pragma unroll
      for (int e = 0; e < 8; ++e) s_acc[wave][c * 8 + e] = acc[e];
  }
  __syncthreads();
  for (int h = threadIdx.x; h < hidden; h += 256)
    DT<T>::st(dq + b * hidden + h, (s_acc[0][h] + s_acc[1][h]) + (s_acc[2][h] + s_acc[3][h]));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int xml_index_gather_video_rows(int n_mod, int form, const int32_t* slot, const int32_t* first_block, int n,
                                           const int32_t* vlen, int64_t n_videos, int64_t n_blocks, int lpad,
                                           const void* cn_src_a, const void* f2_src_a, const float* mask_src_a,
                                           const void* cn_src_b, const void* f2_src_b, const float* mask_src_b, void* cn_a,
                                           void* f2_a, float* mask_a, void* cn_b, void* f2_b, float* mask_b, int l,
                                           int hidden, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (form != XML_INDEX_ROW_MAJOR && form != XML_INDEX_BLOCK_IMAGE) return XML_ERR_BAD_ARG;
  const bool image = form == XML_INDEX_BLOCK_IMAGE;
  if (!slot || !vlen || (image && !first_block)) return XML_ERR_BAD_ARG;
  if (!cn_src_a || !f2_src_a || !mask_src_a || !cn_a || !f2_a || !mask_a) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!cn_src_b || !f2_src_b || !mask_src_b || !cn_b || !f2_b || !mask_b)) return XML_ERR_BAD_ARG;
  if (n <= 0 || l <= 0 || lpad <= 0 || hidden <= 0 || n_videos <= 0 || l > lpad) return XML_ERR_BAD_ARG;
  if (image && n_blocks <= 0) return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (!aligned16(cn_src_a) || !aligned16(f2_src_a) || !aligned16(cn_a) || !aligned16(f2_a)) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!aligned16(cn_src_b) || !aligned16(f2_src_b) || !aligned16(cn_b) || !aligned16(f2_b)))
    return XML_ERR_BAD_ARG;
  if (hidden > 4096) return XML_ERR_UNSUPPORTED;
  const int row_bytes = hidden * (dt == XML_F32 ? 4 : 2);
  if (image ? row_bytes % k6img::SLICE_BYTES != 0 : hidden % 8 != 0) return XML_ERR_UNSUPPORTED;
  const int chunks = row_bytes / 16;                              // 16-byte pieces per row (image: 4 per 64-byte slice)
  const int64_t total = (int64_t)n * l * chunks;
  if ((total + 255) / 256 > 0x7fffffff) return XML_ERR_UNSUPPORTED;
  Sides<GatherSide> sides;
  sides.m[0] = GatherSide{(const char*)cn_src_a, (const char*)f2_src_a, mask_src_a, (char*)cn_a, (char*)f2_a, mask_a};
  sides.m[1] = n_mod == 2 ? GatherSide{(const char*)cn_src_b, (const char*)f2_src_b, mask_src_b, (char*)cn_b, (char*)f2_b, mask_b}
                          : sides.m[0];
  const dim3 grid((unsigned)((total + 255) / 256), (unsigned)n_mod), blk(256);
  if (image)
    hipLaunchKernelGGL(index_gather_video_rows_kernel<true>, grid, blk, 0, (hipStream_t)stream, sides, slot, first_block, n,
                       vlen, n_videos, n_blocks, lpad, l, chunks);
  else
    hipLaunchKernelGGL(index_gather_video_rows_kernel<false>, grid, blk, 0, (hipStream_t)stream, sides, slot, first_block, n,
                       vlen, n_videos, n_blocks, lpad, l, chunks);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_q2c_scores_arg_bwd_q(int n_mod, const void* const* query, const void* const* qn, const void* const* cn,
                                        const float* const* mask, const float* dscores, int64_t ld_ds, float scale,
                                        void* const* dq, int nq, int nv, const int* l, int hidden, const int32_t* const* arg,
                                        int64_t ld_arg, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod < 1 || n_mod > 2 || !query || !qn || !cn || !mask || !dq || !l || !arg || !dscores) return XML_ERR_BAD_ARG;
  if (ld_ds < nv || ld_arg < nv) return XML_ERR_BAD_ARG;
  ArgBwdArgs a;
  for (int m = 0; m < n_mod; ++m)
    if (!query[m] || !qn[m] || !cn[m] || !mask[m] || !dq[m] || !arg[m]) return XML_ERR_BAD_ARG;
  for (int m = 0; m < n_mod; ++m) {
    if (!xml_q2c_scores_l2norm_bwd_supported(nq, nv, l[m], hidden, dt)) return XML_ERR_UNSUPPORTED;
    a.s[m] = ArgBwdSet{query[m], cn[m], mask[m], dq[m], arg[m], l[m]};
  }
  if (n_mod == 1) a.s[1] = a.s[0];
  a.dscores = dscores; a.ld_ds = ld_ds; a.ld_arg = ld_arg; a.scale = scale; a.eps = 1e-12f;
  a.nv = nv; a.hidden = hidden;
  const dim3 grid(nq, n_mod), blk(256);
  if (dt == XML_F32) hipLaunchKernelGGL(q2c_arg_bwd_q_kernel<float>, grid, blk, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(q2c_arg_bwd_q_kernel<bf16_t>, grid, blk, 0, (hipStream_t)stream, a);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_pair_sim_bwd_q(const void* f2, const float* dsim, void* dq, int64_t n, int l, int hidden, int dt,
                                  xml_stream_t stream) {
  XML_ENTER();
  if (!f2 || !dsim || !dq || n <= 0 || l <= 0 || hidden <= 0) return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (hidden % 8 != 0 || hidden > 2048 || n > 0x7fffffff) return XML_ERR_UNSUPPORTED;
  if (dt == XML_F32)
    hipLaunchKernelGGL(pair_sim_bwd_q_kernel<float>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const float*)f2,
                       dsim, (float*)dq, l, hidden);
  else
    hipLaunchKernelGGL(pair_sim_bwd_q_kernel<bf16_t>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)f2, dsim, (bf16_t*)dq, l, hidden);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
