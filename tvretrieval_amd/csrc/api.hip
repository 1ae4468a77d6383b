// ABI bookkeeping for libxmlhip.so.
#include "common.h"

extern "C" int xml_abi_version(void) {
  return 6; }
extern "C" const char* xml_build_arch(void) { return "gfx950"; }
extern "C" const char* xml_status_string(int status) {
  switch (status) {
    case XML_OK: return "ok";
    case XML_ERR_BAD_ARG: return "bad argument";
    case XML_ERR_UNSUPPORTED: return "unsupported shape";
    case XML_ERR_WORKSPACE: return "workspace too small";
    case XML_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown status";
  }
}

// ---- dispatch introspection: dispatch.h's answers (the product dispatch, in the debug library too) ------------------
extern "C" int64_t xml_dispatch_const(int which) {
  namespace d = dispatch;
  static const int64_t v[] = {      // in the order of xml_dispatch_constant
      d::SLICE_BYTES, d::RING_SLOTS, d::RING_SLOTS_NOMASK, d::RING_LEAD, d::LDS_BYTES, d::GEMM_FEW_TILES, d::GEMM256P_MIN_TILES,
      d::GEMM_LN_MIN_ROWS, d::GEMM_MIN_K_BYTES, d::GEMM256_MIN_M, d::GEMM256_MIN_N, d::GEMM_TILE128_MIN_WG, d::GEMM_TILE64_MIN_WG,
      d::Q2C_PERSIST_MIN_K_BYTES, d::L2N_MAXJ, d::L2N_LANES, d::ATTN_MAX_L, d::ATTN_SMALL_MAX_L, d::ATTN_SMALL_UNITS,
      d::ATTN_N_HEAD_SIZES};
  static_assert(sizeof(v) / sizeof(v[0]) == XML_DC_ATTN_HEAD_SIZE0, "one value per xml_dispatch_constant");
  if (which >= 0 && which < XML_DC_ATTN_HEAD_SIZE0) return v[which];
  static const int64_t k7[] = {     // XML_DC_CONVSE_TM ...
      d::CONVSE_TM, d::RESCORE_TM_BIG, d::CONVSE_SMALL_P, d::CONVSE_SMALL_NV, d::CONVSE_SUB_MAX,
      d::CONVSE_SUB_MIN_PAIRS_PER_VIDEO, d::CONVSE_STEP_BYTES, d::CONVSE_MAX_KSIZE, d::CONVSE_FAST_KSIZE};
  static_assert(sizeof(k7) / sizeof(k7[0]) == XML_DC_CONVSE_END - XML_DC_CONVSE_TM, "one value per XML_DC_CONVSE_* constant");
  if (which >= XML_DC_CONVSE_TM && which < XML_DC_CONVSE_END) return k7[which - XML_DC_CONVSE_TM];
  const int i = which - XML_DC_ATTN_HEAD_SIZE0;
  return i >= 0 && i < d::ATTN_N_HEAD_SIZES ? d::ATTN_HEAD_SIZES[i] : -1;
}
static bool gemm_args_ok(int64_t M, int N, int K, int dt) {
  return M > 0 && N > 0 && K > 0 && (dt == XML_F32 || dt == XML_BF16 || dt == XML_F16S);
}
extern "C" int xml_dispatch_gemm(int64_t M, int N, int K, int dt) {
  return gemm_args_ok(M, N, K, dt) ? (int)dispatch::gemm_kernel(M, N, K, dt) : -1;
}
extern "C" int xml_dispatch_gemm_rules(int64_t M, int N, int K, int dt) {
  if (!gemm_args_ok(M, N, K, dt)) return -1;
  const int tile = dispatch::gemm_small_tile(M, N);       // 32 / 64 / 128 = XML_GEMM_TILE32 / 64 / 128
  if (dt == XML_F16S) return tile | (dispatch::gemm256_f16s_ok(M, N, 3 * K) ? XML_GEMM_256_OK : 0);
  return tile | (dispatch::gemm_few(M, N) ? XML_GEMM_FEW : 0) | (dispatch::gemm256_ok(M, N, K, dt) ? XML_GEMM_256_OK : 0) |
         (dispatch::gemm256p_ok(M, N, K, dt) ? XML_GEMM_256P_OK : 0) | (dispatch::gemm_ln_fused(M, N, K, dt) ? XML_GEMM_LN_FUSED : 0);
}
extern "C" int xml_dispatch_gemm_kloop(int K, int dt, int tile) {
  if (K <= 0 || (tile != 32 && tile != 64 && tile != 128) || !gemm_args_ok(1, 1, K, dt)) return -1;
  if (dt == XML_F16S) return XML_KLOOP_PLAIN;             // f16 operands over K' = 3 K
  return dispatch::gemm_small_deep(tile, false) ? dispatch::gemm_small_kloop(K * (int)dt_size(dt)) : XML_KLOOP_PLAIN;
}
extern "C" int xml_dispatch_q2c(int lpad, int hidden, int dt, int combine) {
  return lpad <= 0 || hidden <= 0 || !dispatch::q2c_dt_ok(dt) ? -1 : dispatch::q2c_kernel(lpad, hidden, dt, combine != 0);
}
extern "C" int xml_dispatch_q2c_fused(int n_mod, int lpad, int hidden, int dt, int launch) {
  if (n_mod < 1 || n_mod > 2 || launch < 0 || lpad <= 0 || hidden <= 0 || !dispatch::q2c_dt_ok(dt)) return -1;
  return dispatch::q2c_fused_kernel(n_mod, lpad, hidden, dt, launch);
}
extern "C" int xml_dispatch_q2c_walk(int what, int a, int b) {
  if (what == XML_Q2C_WALK_RING_SLOTS) return a < 0 || a > 1 || b < 0 || b > 3 ? -1 : dispatch::q2c_ring_slots(a != 0, b);
  if (a <= 0 || b <= 0) return -1;
  const int tq = dispatch::q2c_tq(a), tc = dispatch::q2c_tc(b);
  if (what == XML_Q2C_WALK_QSH) return dispatch::q2c_qsh(tq, tc);
  if (what == XML_Q2C_WALK_TILES_PER_WORKGROUP) return dispatch::q2c_tiles_per_workgroup(tq, tc);
  return -1;
}
extern "C" int xml_dispatch_attention(int lq, int lk, int hidden, int n_heads, int dt) {
  const bool ok = lq > 0 && lk > 0 && hidden > 0 && (dt == XML_F32 || dt == XML_BF16);
  return ok ? dispatch::attn_kernel(lq, lk, hidden, n_heads, dt) : -1;
}
static bool convse_entry_ok(int entry, int dt) {
  return entry >= XML_CONVSE_K7 && entry <= XML_CONVSE_RESCORE && dispatch::convse_dt_ok(dt);
}
extern "C" int xml_dispatch_convse_shape(int entry, int what, int64_t nq, int lpad, int l_ref, int hidden, int ksize, int summ,
                                         int dt) {
  if (!convse_entry_ok(entry, dt) || nq <= 0 || lpad <= 0 || hidden <= 0) return -1;
  const bool rescore = entry == XML_CONVSE_RESCORE;
  const bool shape_ok = rescore ? dispatch::rescore_shape_ok(lpad, hidden, dt) : dispatch::convse_shape_ok(lpad, l_ref, hidden, ksize, dt);
  const int loop = shape_ok ? dispatch::convse_mainloop(nq, lpad, hidden, dt) : XML_CONVSE_REFUSED;
  if (what == XML_CONVSE_ASK_MAINLOOP) return loop;
  if (what != XML_CONVSE_ASK_EPILOGUE || loop == XML_CONVSE_REFUSED) return -1;
  if (rescore) return XML_CONVSE_EPI_ROWMAX;
  // (span evidence forms no summaries)
  return dispatch::convse_fast_epilogue(ksize, entry == XML_CONVSE_K7 && summ != 0) ? XML_CONVSE_EPI_FAST : XML_CONVSE_EPI_GENERAL;
}
extern "C" int64_t xml_dispatch_convse_pairs(int entry, int what, int64_t n_pairs, int nv, int dt) {
  if (!convse_entry_ok(entry, dt) || n_pairs <= 0 || nv <= 0) return -1;
  const bool rescore = entry == XML_CONVSE_RESCORE;
  const int tm = rescore ? dispatch::rescore_chunk_pairs(n_pairs, nv, dt) : dispatch::CONVSE_TM;
  if (what == XML_CONVSE_ASK_INVERSION) return dispatch::convse_inversion(n_pairs, nv, rescore);
  if (what == XML_CONVSE_ASK_CHUNK_PAIRS) return tm;
  if (what == XML_CONVSE_ASK_MAX_CHUNKS) return dispatch::convse_max_chunks(n_pairs, nv, tm);
  return -1;
}
extern "C" int xml_dispatch_l2norm(int d, int dt) {
  return d <= 0 || (dt != XML_F32 && dt != XML_BF16) ? -1 : dispatch::l2n_vec_ok(d, dt) ? XML_L2N_VEC16 : XML_L2N_SCALAR;
}
