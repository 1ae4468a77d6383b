"""Python mirrors of the library's dispatch predicates, one per C++ decision, shared by the GPU tests that have to know
which kernel a shape lands on (tests/test_gpu_row_invariance.py, tests/test_gpu_reduction_width.py) and by the plan test
that needs no GPU (tests/test_reduction_width_plan.py, which also holds the threshold literals below against the .hip
sources).  Nothing here imports the library."""

# threshold literals (tests/test_reduction_width_plan.py greps the sources for each of them)
FEW_TILES = 64                  # linear.hip xmli_gemm: fewer 256 x 256 tiles -> the small-tile kernel
GEMM256P_MIN_TILES = 3072       # gemm256p.hip xmli_gemm256p_eligible
LN_FUSED_MIN_ROWS = 2048        # gemm256p.hip xmli_gemm_ln_eligible
GEMM_MIN_KB = 256               # gemm256 / gemm256p / LN epilogue: at least four 64-byte slices
K6_PERSIST_MIN_KB = 384         # q2c.hip persist_ok, q2c_persist.hip xml_q2c_tiled_ok: at least six 64-byte slices
L2N_MAXJ = 8                    # l2norm.h: 16-byte chunks per lane, 32 lanes per row
ATTN_DH = (32, 64, 96, 128, 192)    # attention.hip dispatch_attn_dh, attention_train.hip at_dispatch
ATTN_SMALL_MAX_L = 32           # attention.hip launch_attn: lq <= 32 and lk <= 32 -> the small kernel
ATTN_MAX_L = 128
LDS_BYTES = 160 * 1024
SLICE_BYTES = 64                # one ring slot row: 64 bytes of K


def cdiv(a, b):
    return -(-a // b)


# ---- GEMM (linear.hip xmli_gemm) ----------------------------------------------------------------------------------------
def few(m, n):
    """linear.hip xmli_gemm: `few` -- fewer than 64 tiles of 256 x 256 -> the small-tile gemm_bias_act_kernel."""
    return cdiv(m, 256) * cdiv(n, 256) < FEW_TILES


def small_bmn(m, n):
    """linear.hip launch_gemm: tile size of gemm_bias_act_kernel (bmn from wg128)."""
    wg128 = cdiv(n, 128) * cdiv(m, 128)
    return 128 if wg128 >= 512 else 64 if wg128 * 4 >= 192 else 32


def small_kloop(k, es, bmn):
    """linear.hip gemm_bias_act_kernel: K loop of the small tiles -- deep-3 / deep-2 / plain by the number of 128-byte steps."""
    if bmn == 128:
        return "plain"
    ns = cdiv(k * es, 128)
    return "deep3" if ns % 3 == 0 else "deep2" if ns % 2 == 0 else "plain"


def gemm256_ok(m, n, k, es):
    """gemm256.hip xmli_gemm256_eligible."""
    kb = k * es
    return m >= 256 and n >= 128 and kb % 128 == 0 and kb >= GEMM_MIN_KB


def gemm256p_ok(m, n, k, es):
    """gemm256p.hip xmli_gemm256p_eligible."""
    kb = k * es
    return kb % 128 == 0 and kb >= GEMM_MIN_KB and n >= 128 and n % 8 == 0 and cdiv(m, 256) * cdiv(n, 256) >= GEMM256P_MIN_TILES


def gemm_ln_fused(m, n, k, es):
    """gemm256p.hip xmli_gemm_ln_eligible (f32 / bf16): LN_FUSED_MIN_ROWS = 2 048."""
    kb = k * es
    return kb % 128 == 0 and kb >= GEMM_MIN_KB and n % 256 == 0 and n // 256 <= 3 and m >= LN_FUSED_MIN_ROWS


def gemm_form(m, n, k, es):
    """the kernel the product library's xmli_gemm runs for f32 / bf16."""
    if not few(m, n) and gemm256p_ok(m, n, k, es):
        return "gemm256p"
    if not few(m, n) and gemm256_ok(m, n, k, es):
        return "gemm256"
    b = small_bmn(m, n)
    return "small%d-%s" % (b, small_kloop(k, es, b))


def gemm256_f16s_ok(m, n, k):
    """gemm256.hip xmli_gemm256_f16s_eligible on the split operands (K3 = 3 K halves of 2 bytes)."""
    kb = 3 * k * 2
    return m >= 256 and n >= 128 and n % 8 == 0 and kb % 128 == 0 and kb >= GEMM_MIN_KB


def f16s_form(m, n, k):
    """linear.hip xmli_gemm, dt == XML_F16S: the 256 x 256 LDS-DMA kernel or the small-tile f16 kernel."""
    return "gemm256-f16s" if gemm256_f16s_ok(m, n, k) else "small%d-f16s" % small_bmn(m, n)


# ---- K6 (q2c.hip xml_q2c_scores / xml_q2c_scores_fused, q2c_persist.hip xml_q2c_tiled_ok) -------------------------------------
K6_MASK_FORMS = ("float", "nomask", "bitmask", "packed")      # mask_mode 0 / 1 / 2 / 3 of xmli_q2c_scores_persist


def q2c_tiled_ok(lpad, hidden, es):
    """q2c_persist.hip xml_q2c_tiled_ok (f32, bf16 and f16 operands)."""
    kb = hidden * es
    return lpad == 128 and kb % 128 == 0 and kb >= K6_PERSIST_MIN_KB


def q2c_persist_ok(lpad, hidden, es, f16=False):
    """q2c.hip persist_ok: row-major operands on the persistent kernel."""
    return not f16 and q2c_tiled_ok(lpad, hidden, es)


def q2c_dma_ok(hidden, es, f16=False):
    """q2c.hip dma_ok: the LDS-DMA ring kernel (q2c_ring.hip) takes the width."""
    return not f16 and (hidden * es) % 128 == 0


def q2c_persist_slots(tiled, mask_form):
    """q2c_persist.hip: ring depth of the persistent kernel -- five slots for the tiled NOMASK / BITMASK forms, else four."""
    return 5 if tiled and mask_form in ("nomask", "bitmask") else 4


def q2c_form(lpad, hidden, es, combine=False, f16=False):
    """the kernel one xml_q2c_scores call on row-major operands runs."""
    if lpad % 16 or lpad > 128 or hidden % 8:
        return "unsupported"
    if q2c_persist_ok(lpad, hidden, es, f16) and not combine:
        return "persist"
    if q2c_dma_ok(hidden, es, f16):
        return "ring"
    return "staged"


def q2c_fused_forms(n_mod, lpad, hidden, es, f16=False):
    """xml_q2c_scores_fused on row-major operands: one persistent launch, or one xml_q2c_scores call per modality (the
    second with combine)."""
    if q2c_persist_ok(lpad, hidden, es, f16):
        return ["persist"]
    return [q2c_form(lpad, hidden, es, combine=m > 0, f16=f16) for m in range(n_mod)]


def q2c_persist_qsh(nq, nv):
    """q2c_persist.hip xmli_q2c_scores_persist: log2 of the query tiles per XCD super-tile."""
    tq, tc = cdiv(nq, 256), cdiv(nv, 2)
    qsh = 3 if tq >= 5 else 2 if tq >= 3 else 1 if tq == 2 else 0
    if qsh == 3:
        def slots(q):
            qg, per = (tq + (1 << q) - 1) >> q, 8 << (5 - q)
            return (qg << q) * (cdiv(tc, per) * per)
        if slots(2) * 100 < slots(3) * 97:
            qsh = 2
    return qsh


def q2c_persist_tiles_per_workgroup(nq, nv):
    """most (query tile, clip tile) pairs one workgroup of the persistent kernel walks: query groups x rounds."""
    tq, tc = cdiv(nq, 256), cdiv(nv, 2)
    qsh = q2c_persist_qsh(nq, nv)
    return cdiv(tq, 1 << qsh) * cdiv(tc, 8 << (5 - qsh))


def l2n_vec_ok(d, es):
    """linear.hip xml_l2norm_rows: the 16-byte kernel (half a wave per row) takes the width."""
    vec = 16 // es
    return d % vec == 0 and d // vec <= 32 * L2N_MAXJ


def tile_rows_l2norm_ok(hidden, es):
    """index_build.hip xml_q2c_tile_rows_l2norm_ok."""
    vec = 16 // es
    return hidden > 0 and hidden % (4 * vec) == 0 and hidden // vec <= 32 * L2N_MAXJ


# ---- attention (attention.hip launch_attn / attn_lds_bytes, attention_train.hip) ---------------------------------------------
def attn_small_lds_bytes(lk, dh, es):
    ce = 64 // es
    lkp = cdiv(lk, ce) * ce
    k_stride, vt_stride = dh * es + 16, lkp * es + 16
    kvb = 32 * k_stride if es == 2 else max(32 * k_stride, dh * vt_stride)
    return 4 * (kvb + 16 * vt_stride)


def attn_lds_bytes(lk, dh, es):
    ce = 64 // es
    lkp = cdiv(lk, ce) * ce
    k_stride, vt_stride = dh * es + 16, lkp * es + 16
    kvb = lkp * k_stride if es == 2 else max(cdiv(lk, 16) * 16 * k_stride, dh * vt_stride)
    return kvb + 4 * 16 * vt_stride


def attn_form(lq, lk, hidden, n_heads, es):
    """attention.hip xmli_attention_core: "small" (four (sequence, head) units per workgroup), "large", or the reason it is
    refused."""
    if n_heads <= 0 or hidden % n_heads:
        return "refused: hidden % n_heads"
    dh = hidden // n_heads
    if lq > ATTN_MAX_L or lk > ATTN_MAX_L:
        return "refused: longer than %d" % ATTN_MAX_L
    if attn_lds_bytes(lk, dh, es) > LDS_BYTES:
        return "refused: LDS"
    if dh not in ATTN_DH:
        return "refused: DH"
    if lq <= ATTN_SMALL_MAX_L and lk <= ATTN_SMALL_MAX_L and attn_small_lds_bytes(lk, dh, es) <= LDS_BYTES:
        return "small"
    return "large"


def attn_train_ok(lq, lk, hidden, n_heads):
    """attention_train.hip xml_attention_train_supported (bf16)."""
    return n_heads > 0 and hidden % n_heads == 0 and 0 < lq <= ATTN_MAX_L and 0 < lk <= ATTN_MAX_L and hidden // n_heads in ATTN_DH
