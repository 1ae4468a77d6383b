// Which kernel a shape lands on: every shape-class decision and named threshold of libxmlhip, once.
// Host arithmetic over integers (plain C++17, no HIP): the launchers call these functions, the kernels take their ring
// geometry from the constants, and the xml_dispatch_* entries (api.hip) answer from the same functions.  Moving a rule
// is one edit here (and one in tests/test_reduction_width_plan.py::test_pinned_thresholds).  The debug library's
// xml_debug_* switches are applied by the launchers on top of these answers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/xmlhip.h"

namespace dispatch {

constexpr int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
constexpr size_t dt_size(int dt) { return (dt == XML_F32 || dt == XML_F16S) ? 4 : 2; }
constexpr size_t max_of(size_t a, size_t b) { return a > b ? a : b; }

// ---- constants ----------------------------------------------------------------------------------------------------
constexpr int LDS_BYTES = 160 * 1024;       // per workgroup
constexpr int SLICE_BYTES = 64;             // LDS-DMA ring kernels: bytes of K per row in one slot (ROWB)
constexpr int RING_SLOTS = 4;               // gemm256, gemm256p, q2c_ring, q2c_persist
constexpr int RING_SLOTS_NOMASK = 5;        // q2c_persist without mask patches: their 2 KiB make room for a fifth slot
constexpr int RING_LEAD = 5;                // q2c_ring: DMA units in front of the phase being computed
constexpr int RING_ROWS = 256;              // rows of one operand in a slot

// ---- GEMM (xmli_gemm, xmli_gemm_ln) -------------------------------------------------------------------------------
constexpr int GEMM_FEW_TILES = 64;            // fewer 256 x 256 tiles: a quarter of the chip at best behind a serial K loop
constexpr int GEMM256P_MIN_TILES = 3072;      // (2304 tiles: 2 % behind the one-tile kernel, 3516: 7 % ahead)
constexpr int64_t GEMM_LN_MIN_ROWS = 2048;    // below: small tiles fill the chip, six row blocks would not
constexpr int GEMM_MIN_K_BYTES = 256;         // the ring prologue issues four slices
constexpr int GEMM256_MIN_M = 256, GEMM256_MIN_N = 128;
constexpr int GEMM_TILE128_MIN_WG = 512, GEMM_TILE64_MIN_WG = 192;      // workgroups a small-tile size must reach
constexpr int GEMM_SMALL_STEP_BYTES = 128;    // bytes of K per row per step of the small-tile kernel

constexpr int64_t gemm_tiles(int64_t M, int N) { return (int64_t)cdiv(M, 256) * cdiv(N, 256); }
constexpr bool gemm_few(int64_t M, int N) { return gemm_tiles(M, N) < GEMM_FEW_TILES; }
// the ring kernels' K: an even number of slices, at least four
constexpr bool gemm_ring_k(size_t k_bytes) { return k_bytes % (2 * SLICE_BYTES) == 0 && k_bytes >= GEMM_MIN_K_BYTES; }
constexpr bool gemm256_ok(int64_t M, int N, int K, int dt) {
  return M >= GEMM256_MIN_M && N >= GEMM256_MIN_N && gemm_ring_k((size_t)K * dt_size(dt));
}
// split-f16 projection on K-concatenated halves: K3 = 3 x the logical K, f16 operands
constexpr bool gemm256_f16s_ok(int64_t M, int N, int K3) {
  return M >= GEMM256_MIN_M && N >= GEMM256_MIN_N && N % 8 == 0 && gemm_ring_k((size_t)K3 * 2);
}
// worth it when every workgroup gets several tiles; below that the one-tile-per-workgroup kernel is as good
constexpr bool gemm256p_ok(int64_t M, int N, int K, int dt) {
  return gemm_ring_k((size_t)K * dt_size(dt)) && N >= GEMM256_MIN_N && N % 8 == 0 && gemm_tiles(M, N) >= GEMM256P_MIN_TILES;
}
// LayerNorm in the GEMM epilogue: rows of 1-3 whole 256-column tiles (split-f16 projections take the three-launch path)
constexpr bool gemm_ln_fused(int64_t M, int N, int K, int dt) {
  return (dt == XML_F32 || dt == XML_BF16) && gemm_ring_k((size_t)K * dt_size(dt)) && N % 256 == 0 && N / 256 <= 3 &&
         M >= GEMM_LN_MIN_ROWS;
}
constexpr xml_gemm_kernel gemm_kernel(int64_t M, int N, int K, int dt) {
  if (dt == XML_F16S) return gemm256_f16s_ok(M, N, 3 * K) ? XML_GEMM_256 : XML_GEMM_SMALL;
  if (!gemm_few(M, N) && gemm256p_ok(M, N, K, dt)) return XML_GEMM_256P;
  if (!gemm_few(M, N) && gemm256_ok(M, N, K, dt)) return XML_GEMM_256;
  return XML_GEMM_SMALL;
}
// small-tile kernel: smaller tiles of the same mainloop until a few hundred workgroups exist
constexpr int gemm_small_tile(int64_t M, int N) {
  const int64_t wg128 = (int64_t)cdiv(N, 128) * cdiv(M, 128);
  return wg128 >= GEMM_TILE128_MIN_WG ? 128 : wg128 * 4 >= GEMM_TILE64_MIN_WG ? 64 : 32;
}
// its K loop: tiles below 128 load 3 (or 2) 128-byte steps ahead when the step count divides (f32 / bf16 operands only)
constexpr bool gemm_small_deep(int tile, bool f16_operands) { return tile < 128 && !f16_operands; }
// (the kernel passes its three K loops: it branches as written here, not on a returned code)
template <typename D3, typename D2, typename P>
constexpr void gemm_small_kloop_run(int k_bytes, D3&& deep3, D2&& deep2, P&& plain) {
  const int nsteps = (k_bytes + GEMM_SMALL_STEP_BYTES - 1) / GEMM_SMALL_STEP_BYTES;
  if (nsteps % 3 == 0) deep3();
  else if (nsteps % 2 == 0) deep2();
  else plain();
}
constexpr xml_gemm_kloop gemm_small_kloop(int k_bytes) {
  xml_gemm_kloop r = XML_KLOOP_PLAIN;
  gemm_small_kloop_run(k_bytes, [&] { r = XML_KLOOP_DEEP3; }, [&] { r = XML_KLOOP_DEEP2; }, [] {});
  return r;
}

// ---- K6 (xml_q2c_scores, xml_q2c_scores_fused, the tiled entries) -------------------------------------------------
constexpr int Q2C_PERSIST_MIN_K_BYTES = 384;      // the mask patch of segment s + 2 is fetched 4 slices ahead and must
                                                  // not land before the epilogue of segment s: at least six slices
constexpr bool q2c_dt_ok(int dt) { return dt == XML_F32 || dt == XML_BF16 || dt == XML_F16; }
constexpr bool q2c_shape_ok(int lpad, int hidden) { return lpad % 16 == 0 && lpad <= 128 && hidden % 8 == 0; }
constexpr bool q2c_tiled_ok(int lpad, int hidden, int dt) {
  const size_t kb = (size_t)hidden * dt_size(dt);
  return q2c_dt_ok(dt) && lpad == 128 && kb % (2 * SLICE_BYTES) == 0 && kb >= Q2C_PERSIST_MIN_K_BYTES;
}
// row-major operands (XML_F16 rows -- corpora too small / hidden sizes too short for the tiled kernel -- stay staged)
constexpr bool q2c_persist_ok(int lpad, int hidden, int dt) { return dt != XML_F16 && q2c_tiled_ok(lpad, hidden, dt); }
constexpr bool q2c_ring_ok(int hidden, int dt) { return dt != XML_F16 && ((size_t)hidden * dt_size(dt)) % (2 * SLICE_BYTES) == 0; }
constexpr xml_q2c_kernel q2c_kernel(int lpad, int hidden, int dt, bool combine) {
  if (!q2c_shape_ok(lpad, hidden)) return XML_Q2C_UNSUPPORTED;
  if (q2c_persist_ok(lpad, hidden, dt) && !combine) return XML_Q2C_PERSIST;
  return q2c_ring_ok(hidden, dt) ? XML_Q2C_RING : XML_Q2C_STAGED;
}
// xml_q2c_scores_fused: one persistent launch, or one xml_q2c_scores call per modality (the second with combine)
constexpr xml_q2c_kernel q2c_fused_kernel(int n_mod, int lpad, int hidden, int dt, int launch) {
  if (!q2c_shape_ok(lpad, hidden)) return launch == 0 ? XML_Q2C_UNSUPPORTED : XML_Q2C_NONE;
  if (q2c_persist_ok(lpad, hidden, dt)) return launch == 0 ? XML_Q2C_PERSIST : XML_Q2C_NONE;
  return launch < n_mod ? q2c_kernel(lpad, hidden, dt, launch > 0) : XML_Q2C_NONE;
}
// the persistent kernel's walk over tq x tc tiles of 256 queries x 2 videos: an XCD's super-tile is 2^qsh query tiles x
// 2^(5 - qsh) clip tiles.  Few queries: more workgroups share a query tile.
constexpr int q2c_tq(int nq) { return cdiv(nq, 256); }
constexpr int q2c_tc(int nv) { return cdiv(nv, 2); }
// slots the walk hands out, valid or not: every workgroup gets ceil(tq / 2^qsh) x ceil(tc / (8 x 2^(5 - qsh))) tiles
constexpr int64_t q2c_walk_slots(int tq, int tc, int qsh) {
  const int64_t qg = (tq + (1 << qsh) - 1) >> qsh, per = 8ll << (5 - qsh);
  return (qg << qsh) * ((tc + per - 1) / per * per);
}
constexpr int q2c_qsh(int tq, int tc) {
  const int qsh = tq >= 5 ? 3 : tq >= 3 ? 2 : tq == 2 ? 1 : 0;
  // With 43 query tiles (TVR val, 10 895 queries) the 8 x 4 super-tile walks 48 x 576 slots for 43 x 573 tiles, the 4 x 8
  // one 44 x 576 (-8 % of the kernel's time).  Take the 4 x 8 shape when it saves more than 3 % of the slots -- it fetches
  // every clip tile for 4 instead of 8 query tiles per XCD, which is what the 8 x 4 shape is there to avoid when the two tie.
  return qsh == 3 && q2c_walk_slots(tq, tc, 2) * 100 < q2c_walk_slots(tq, tc, 3) * 97 ? 2 : qsh;
}
constexpr int q2c_tiles_per_workgroup(int tq, int tc) {
  const int qsh = q2c_qsh(tq, tc);
  return cdiv(tq, 1 << qsh) * cdiv(tc, 8 << (5 - qsh));
}
// mask_mode 0 float masks, 1 no mask, 2 bit masks, 3 packed (four slots: the patch area carries the straddle hand-off)
constexpr int q2c_ring_slots(bool tiled, int mask_mode) {
  return tiled && (mask_mode == 1 || mask_mode == 2) ? RING_SLOTS_NOMASK : RING_SLOTS;
}

// ---- K7 / span evidence / exact-rank re-score (convse.hip: xml_convse_rerank*, xml_span_evidence, xml_q2c_rescore) -----
constexpr int CONVSE_TM = 64;                 // pairs per workgroup chunk (a video has ~46 pairs at C3: one chunk each)
constexpr int RESCORE_TM_BIG = 128;           // the split-f16 re-score when the average video is listed by more than CONVSE_TM pairs
// Popular videos: with few videos and many pairs (TVR val: 2 179 videos, 1.09 M pairs = 500 per counter) the counting
// atomics serialise on their addresses -- 138 us of a 1.1 ms K7.  Every video then gets CONVSE_SUB_MAX sub-counters, a pair
// uses sub-counter (pair id % sub): 16 x fewer collisions per address; the scan runs over the sub-buckets in (video, sub)
// order, so a video's bucket is still one contiguous range.
constexpr int CONVSE_SUB_MAX = 16;
constexpr int CONVSE_SUB_MIN_PAIRS_PER_VIDEO = 128;
// Small pair lists (the reference's 50-query batches: 5 000 pairs): ONE workgroup inverts the list, counters in LDS
constexpr int CONVSE_SMALL_NV = 4096, CONVSE_SMALL_P = 32768;
constexpr int CONVSE_MAX_KSIZE = 15, CONVSE_FAST_KSIZE = 5, CONVSE_MAX_LPAD = 128;
constexpr int CONVSE_STEP_BYTES = GEMM_SMALL_STEP_BYTES;      // the mainloops' K step (GemmCfg::ROWB)

constexpr bool convse_dt_ok(int dt) { return dt == XML_F32 || dt == XML_BF16 || dt == XML_F16S; }
// shapes the entries take (everything else: XML_ERR_UNSUPPORTED); the re-score has no filter and no l_ref
constexpr bool rescore_shape_ok(int lpad, int hidden, int dt) {
  return lpad > 0 && lpad % 16 == 0 && lpad <= CONVSE_MAX_LPAD && hidden % 8 == 0 && (dt != XML_F16S || hidden % 32 == 0);
}
constexpr bool convse_shape_ok(int lpad, int l_ref, int hidden, int ksize, int dt) {
  return rescore_shape_ok(lpad, hidden, dt) && l_ref > 0 && l_ref <= lpad && (ksize & 1) && ksize >= 1 && ksize <= CONVSE_MAX_KSIZE;
}
// the LDS-DMA mainloop (gemm.h): rows are whole 128-byte K steps and every row offset -- of the nq query rows, of a video's
// lpad clip rows -- fits the 32 bits it is addressed with; otherwise the register-staged loop with its zero-filled K tail
constexpr bool convse_dma(int64_t nq, int lpad, int hidden, int dt) {
  const int64_t kb = (int64_t)hidden * (int64_t)dt_size(dt);
  return kb % CONVSE_STEP_BYTES == 0 && nq * kb < (1ll << 32) && (int64_t)lpad * kb < (1ll << 32);
}
// split rows are whole 128-byte steps by construction (hidden % 32 == 0): without the DMA loop (offsets past 32 bits) refused
constexpr xml_convse_mainloop convse_mainloop(int64_t nq, int lpad, int hidden, int dt) {
  return convse_dma(nq, lpad, hidden, dt) ? XML_CONVSE_DMA : dt == XML_F16S ? XML_CONVSE_REFUSED : XML_CONVSE_STAGED;
}
constexpr int convse_sub(int64_t P, int nv) { return P >= CONVSE_SUB_MIN_PAIRS_PER_VIDEO * (int64_t)nv ? CONVSE_SUB_MAX : 1; }
constexpr bool convse_small_inversion(int64_t P, int nv) { return P <= CONVSE_SMALL_P && nv <= CONVSE_SMALL_NV; }
// K7 / span evidence; the re-score always counts in global memory (it has no rows to zero-fill in the same pass)
constexpr xml_convse_inversion convse_inversion(int64_t P, int nv, bool rescore) {
  if (!rescore && convse_small_inversion(P, nv)) return XML_CONVSE_INV_SMALL;
  return convse_sub(P, nv) > 1 ? XML_CONVSE_INV_SUB : XML_CONVSE_INV_GLOBAL;
}
// rows per chunk of the re-score: 128 when the average video is listed by more than 64 pairs (then most videos would need
// two 64-row chunks, each fetching the tile again)
constexpr int rescore_chunk_pairs(int64_t P, int nv, int dt) {
  return dt == XML_F16S && P > CONVSE_TM * (int64_t)nv ? RESCORE_TM_BIG : CONVSE_TM;
}
// chunks a launch must provide for: every video ends in at most one partly filled chunk
constexpr int64_t convse_max_chunks(int64_t P, int nv, int tm) { return P / tm + (P < nv ? P : nv); }
// K7's epilogue: half a wave per pair row and four clips per lane for the as-trained 5 taps, else the general row loop
// (which also forms the candidate summaries)
// (a macro: convse_kernel branches on it with the summaries' pointer as `summ`, evaluated only behind the ksize test -- as a
// function call, whose arguments are evaluated first, the kernel came out with another register allocation)
#define XML_CONVSE_FAST_EPILOGUE(ksize, summ) ((ksize) == dispatch::CONVSE_FAST_KSIZE && !(summ))
constexpr bool convse_fast_epilogue(int ksize, bool summ) { return XML_CONVSE_FAST_EPILOGUE(ksize, summ); }

// ---- L2 normalisation: the 16-byte kernel, half a wave (32 lanes) per row, up to L2N_MAXJ chunks per lane ------------
constexpr int L2N_MAXJ = 8, L2N_LANES = 32;       // rows of up to 32 * 8 chunks = 4096 bytes
constexpr bool l2n_vec_ok(int d, int dt) {
  const int vec = 16 / (int)dt_size(dt);
  return (dt == XML_F32 || dt == XML_BF16) && d % vec == 0 && d / vec <= L2N_LANES * L2N_MAXJ;
}
// fused normalise-and-tile index build: whole 64-byte slices on top
constexpr bool tile_rows_l2norm_ok(int hidden, int dt) {
  return hidden > 0 && l2n_vec_ok(hidden, dt) && (hidden * (int)dt_size(dt)) % SLICE_BYTES == 0;
}

// ---- attention core -------------------------------------------------------------------------------------------------
#define XML_ATTN_HEAD_SIZES(X) X(32) X(64) X(96) X(128) X(192)      // kernels are instantiated per head size
#define XML_ATTN_LIST(D) D,
constexpr int ATTN_HEAD_SIZES[] = {XML_ATTN_HEAD_SIZES(XML_ATTN_LIST)};
#undef XML_ATTN_LIST
constexpr int ATTN_N_HEAD_SIZES = sizeof(ATTN_HEAD_SIZES) / sizeof(ATTN_HEAD_SIZES[0]);
constexpr int ATTN_MAX_L = 128;             // longest sequence of either side
constexpr int ATTN_SMALL_MAX_L = 32;        // both sides at most this long: one wave per (sequence, head) ...
constexpr int ATTN_SMALL_UNITS = 4;         // ... four such units per workgroup
constexpr bool attn_head_size_ok(int dh) {
  for (int i = 0; i < ATTN_N_HEAD_SIZES; ++i)
    if (ATTN_HEAD_SIZES[i] == dh) return true;
  return false;
}
constexpr size_t attn_small_lds_bytes(int lk, int dh, int dt) {
  const int es = (int)dt_size(dt), ce = 64 / es;
  const int lkp = (lk + ce - 1) / ce * ce;
  const size_t k_stride = (size_t)dh * es + 16, vt_stride = (size_t)lkp * es + 16;
  const size_t kvb = es == 2 ? (size_t)32 * k_stride : max_of((size_t)32 * k_stride, (size_t)dh * vt_stride);
  return ATTN_SMALL_UNITS * (kvb + 16 * vt_stride);
}
constexpr size_t attn_lds_bytes(int lk, int dh, int dt) {
  const int es = (int)dt_size(dt), ce = 64 / es;
  const int lkp = (lk + ce - 1) / ce * ce;
  const size_t k_stride = (size_t)dh * es + 16, vt_stride = (size_t)lkp * es + 16;
  const size_t kvb = es == 2 ? (size_t)lkp * k_stride          // bf16: V row-major over K (transpose reads)
                             : max_of((size_t)((lk + 15) / 16 * 16) * k_stride, (size_t)dh * vt_stride);
  return kvb + 4 * 16 * vt_stride;
}
// in the order xmli_attention_core refuses
constexpr xml_attn_kernel attn_kernel(int lq, int lk, int hidden, int n_heads, int dt) {
  if (n_heads <= 0 || hidden % n_heads) return XML_ATTN_REFUSED_HEADS;
  const int dh = hidden / n_heads;
  if (lq > ATTN_MAX_L || lk > ATTN_MAX_L) return XML_ATTN_REFUSED_LENGTH;
  if (attn_lds_bytes(lk, dh, dt) > (size_t)LDS_BYTES) return XML_ATTN_REFUSED_LDS;
  if (!attn_head_size_ok(dh)) return XML_ATTN_REFUSED_DH;
  const bool small = lq <= ATTN_SMALL_MAX_L && lk <= ATTN_SMALL_MAX_L && attn_small_lds_bytes(lk, dh, dt) <= (size_t)LDS_BYTES;
  return small ? XML_ATTN_SMALL : XML_ATTN_LARGE;
}
constexpr bool attn_train_ok(int lq, int lk, int hidden, int n_heads, int dt) {
  return dt == XML_BF16 && n_heads > 0 && hidden % n_heads == 0 && lq > 0 && lk > 0 && lq <= ATTN_MAX_L && lk <= ATTN_MAX_L &&
         attn_head_size_ok(hidden / n_heads);
}

}  // namespace dispatch
