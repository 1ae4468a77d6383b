"""Which kernel a shape lands on, asked of the library: thin wrappers over the xml_dispatch_* entries and the exported
predicates of include/xmlhip.h (tvretrieval_amd/csrc/dispatch.h answers them, the same functions the launchers call).
Shared by the GPU tests that have to place a case on a kernel (tests/test_gpu_row_invariance.py, test_gpu_reduction_width.py)
and by the plan test (tests/test_reduction_width_plan.py).  Needs the built library, not a GPU; no rule or threshold is
written down here.  Operand types are given as element sizes: 4 = f32, 2 = bf16 (f16=True: IEEE half)."""
import os
import re

from tvretrieval_amd import _lib

if not os.path.isfile(_lib.LIB_PATH):      # (as tests/test_capi.py: a tree that was never built)
    import __graft_entry__
    __graft_entry__.build()
LIB = _lib.load()


def _header_enums():
    """name -> value of every enumerator of include/xmlhip.h."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xmlhip.h")).read()
    out = {}
    for body in re.findall(r"typedef enum \{(.*?)\}", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, val = (p.strip() for p in item.partition("="))
            out[name] = nxt = int(val, 0) if val else nxt
            nxt += 1
    return out


E = _header_enums()


def ask(fn, *args):
    v = getattr(LIB, fn)(*args)
    assert v >= 0, "%s%r: outside the entry's domain" % (fn, args)
    return v


def const(name):
    return ask("xml_dispatch_const", E["XML_DC_" + name])


def dt_of(es, f16=False):
    return _lib.XML_F16 if f16 else {4: _lib.XML_F32, 2: _lib.XML_BF16}[es]


def cdiv(a, b):
    return -(-a // b)


FEW_TILES, GEMM256P_MIN_TILES, GEMM_MIN_KB = const("GEMM_FEW_TILES"), const("GEMM256P_MIN_TILES"), const("GEMM_MIN_K_BYTES")
LN_FUSED_MIN_ROWS, L2N_MAXJ, L2N_LANES = const("GEMM_LN_MIN_ROWS"), const("L2N_MAXJ"), const("L2N_LANES")
K6_PERSIST_MIN_KB, SLICE_BYTES, LDS_BYTES = const("Q2C_PERSIST_MIN_K_BYTES"), const("SLICE_BYTES"), const("LDS_BYTES")
ATTN_DH = tuple(ask("xml_dispatch_const", E["XML_DC_ATTN_HEAD_SIZE0"] + i) for i in range(const("ATTN_N_HEAD_SIZES")))
ATTN_SMALL_MAX_L, ATTN_SMALL_UNITS, ATTN_MAX_L = const("ATTN_SMALL_MAX_L"), const("ATTN_SMALL_UNITS"), const("ATTN_MAX_L")

# ---- GEMM (xmli_gemm): "small<tile>-<K loop>", "gemm256", "gemm256p"; split-f16: "gemm256-f16s", "small<tile>-f16s" -------------
KLOOPS = {E["XML_KLOOP_DEEP3"]: "deep3", E["XML_KLOOP_DEEP2"]: "deep2", E["XML_KLOOP_PLAIN"]: "plain"}
GEMM_KERNELS = {E["XML_GEMM_256"]: "gemm256", E["XML_GEMM_256P"]: "gemm256p"}


def gemm_rule(flag, m, n, k=8, dt=_lib.XML_F32):
    return ask("xml_dispatch_gemm_rules", m, n, k, dt) & E["XML_GEMM_" + flag]


def few(m, n):
    """fewer 256 x 256 tiles than the ring kernels are worth -> the small-tile gemm_bias_act_kernel."""
    return bool(gemm_rule("FEW", m, n))


def small_bmn(m, n):
    """tile size of gemm_bias_act_kernel."""
    return ask("xml_dispatch_gemm_rules", m, n, 8, _lib.XML_F32) & (E["XML_GEMM_TILE32"] | E["XML_GEMM_TILE64"] | E["XML_GEMM_TILE128"])


def small_kloop(k, es, bmn):
    """K loop of the small tiles: deep-3 / deep-2 / plain."""
    return KLOOPS[ask("xml_dispatch_gemm_kloop", k, dt_of(es), bmn)]


def gemm256_ok(m, n, k, es):
    return bool(gemm_rule("256_OK", m, n, k, dt_of(es)))


def gemm256p_ok(m, n, k, es):
    return bool(gemm_rule("256P_OK", m, n, k, dt_of(es)))


def gemm_ln_fused(m, n, k, es):
    """xmli_gemm_ln takes the shape (f32 / bf16)."""
    return bool(gemm_rule("LN_FUSED", m, n, k, dt_of(es)))


def gemm_form(m, n, k, es):
    """the kernel the product library's xmli_gemm runs for f32 / bf16."""
    kern = ask("xml_dispatch_gemm", m, n, k, dt_of(es))
    return GEMM_KERNELS.get(kern) or "small%d-%s" % (small_bmn(m, n), small_kloop(k, es, small_bmn(m, n)))


def f16s_form(m, n, k):
    """xmli_gemm, dt == XML_F16S: the 256 x 256 LDS-DMA kernel or the small-tile f16 kernel."""
    kern = ask("xml_dispatch_gemm", m, n, k, _lib.XML_F16S)
    return "gemm256-f16s" if kern == E["XML_GEMM_256"] else "small%d-f16s" % small_bmn(m, n)


# ---- K6 (xml_q2c_scores / xml_q2c_scores_fused, xml_q2c_tiled_ok) ----------------------------------------------------------
K6_MASK_FORMS = ("float", "nomask", "bitmask", "packed")      # mask_mode 0 / 1 / 2 / 3 of the persistent kernel
Q2C_KERNELS = {E["XML_Q2C_UNSUPPORTED"]: "unsupported", E["XML_Q2C_STAGED"]: "staged", E["XML_Q2C_RING"]: "ring",
               E["XML_Q2C_PERSIST"]: "persist"}


def q2c_tiled_ok(lpad, hidden, es, f16=False):
    return bool(LIB.xml_q2c_tiled_ok(lpad, hidden, dt_of(es, f16)))


def q2c_persist_slots(tiled, mask_form):
    """ring depth of the persistent kernel."""
    return ask("xml_dispatch_q2c_walk", E["XML_Q2C_WALK_RING_SLOTS"], int(tiled), K6_MASK_FORMS.index(mask_form))


def q2c_form(lpad, hidden, es, combine=False, f16=False):
    """the kernel one xml_q2c_scores call on row-major operands runs."""
    return Q2C_KERNELS[ask("xml_dispatch_q2c", lpad, hidden, dt_of(es, f16), int(combine))]


def q2c_fused_forms(n_mod, lpad, hidden, es, f16=False):
    """the launches of one xml_q2c_scores_fused call on row-major operands."""
    forms = []
    while True:
        kern = ask("xml_dispatch_q2c_fused", n_mod, lpad, hidden, dt_of(es, f16), len(forms))
        if kern == E["XML_Q2C_NONE"]:
            return forms
        forms.append(Q2C_KERNELS[kern])


def q2c_persist_qsh(nq, nv):
    """log2 of the query tiles per XCD super-tile."""
    return ask("xml_dispatch_q2c_walk", E["XML_Q2C_WALK_QSH"], nq, nv)


def q2c_persist_tiles_per_workgroup(nq, nv):
    """most (query tile, clip tile) pairs one workgroup of the persistent kernel walks."""
    return ask("xml_dispatch_q2c_walk", E["XML_Q2C_WALK_TILES_PER_WORKGROUP"], nq, nv)


def l2n_vec_ok(d, es):
    """xml_l2norm_rows: the 16-byte kernel (half a wave per row) takes the width."""
    return ask("xml_dispatch_l2norm", d, dt_of(es)) == E["XML_L2N_VEC16"]


def tile_rows_l2norm_ok(hidden, es):
    return bool(LIB.xml_q2c_tile_rows_l2norm_ok(hidden, dt_of(es)))


# ---- K7 / span evidence / exact-rank re-score (convse.hip) ----------------------------------------------------------------
# operand types here: torch-free names "f32", "bf16", "f16s" (the split-f16 form has 4-byte elements like f32)
CONVSE_DT = {"f32": _lib.XML_F32, "bf16": _lib.XML_BF16, "f16s": _lib.XML_F16S}
CONVSE_ENTRIES = {"k7": E["XML_CONVSE_K7"], "evidence": E["XML_CONVSE_EVIDENCE"], "rescore": E["XML_CONVSE_RESCORE"]}
CONVSE_LOOPS = {E["XML_CONVSE_REFUSED"]: "refused", E["XML_CONVSE_STAGED"]: "staged", E["XML_CONVSE_DMA"]: "dma"}
CONVSE_INVERSIONS = {E["XML_CONVSE_INV_SMALL"]: "one-workgroup", E["XML_CONVSE_INV_GLOBAL"]: "global", E["XML_CONVSE_INV_SUB"]: "sub"}
CONVSE_EPILOGUES = {E["XML_CONVSE_EPI_FAST"]: "fast", E["XML_CONVSE_EPI_GENERAL"]: "general", E["XML_CONVSE_EPI_ROWMAX"]: "rowmax"}
CONVSE_TM, RESCORE_TM_BIG = const("CONVSE_TM"), const("RESCORE_TM_BIG")
CONVSE_SMALL_P, CONVSE_SMALL_NV = const("CONVSE_SMALL_P"), const("CONVSE_SMALL_NV")
CONVSE_SUB_MIN_PAIRS_PER_VIDEO, CONVSE_STEP_BYTES = const("CONVSE_SUB_MIN_PAIRS_PER_VIDEO"), const("CONVSE_STEP_BYTES")


def convse_mainloop(entry, nq, lpad, l_ref, hidden, ksize, dt):
    """"dma" (LDS-DMA ring), "staged" (register-staged loop, zero-filled K tail) or "refused" (XML_ERR_UNSUPPORTED)."""
    return CONVSE_LOOPS[ask("xml_dispatch_convse_shape", CONVSE_ENTRIES[entry], E["XML_CONVSE_ASK_MAINLOOP"], nq, lpad, l_ref,
                            hidden, ksize, 0, CONVSE_DT[dt])]


def convse_steps(hidden, dt):
    """K steps of either mainloop, and the bytes of K in the last one (a whole step: CONVSE_STEP_BYTES)."""
    kb = hidden * (2 if dt == "bf16" else 4)
    return cdiv(kb, CONVSE_STEP_BYTES), kb - (cdiv(kb, CONVSE_STEP_BYTES) - 1) * CONVSE_STEP_BYTES


def convse_epilogue(entry, ksize, summ=False, dt="f32"):
    """K7 / span evidence: "fast" (5 taps, no summaries) or "general"; the re-score: "rowmax"."""
    return CONVSE_EPILOGUES[ask("xml_dispatch_convse_shape", CONVSE_ENTRIES[entry], E["XML_CONVSE_ASK_EPILOGUE"], 1, 16, 16, 32,
                                ksize, int(summ), CONVSE_DT[dt])]


def convse_inversion(entry, n_pairs, nv, dt="f32"):
    """how the pair list is inverted: "one-workgroup", "global" counters or 16 "sub"-counters per video."""
    return CONVSE_INVERSIONS[ask("xml_dispatch_convse_pairs", CONVSE_ENTRIES[entry], E["XML_CONVSE_ASK_INVERSION"], n_pairs, nv,
                                 CONVSE_DT[dt])]


def convse_chunk_pairs(entry, n_pairs, nv, dt="f32"):
    return ask("xml_dispatch_convse_pairs", CONVSE_ENTRIES[entry], E["XML_CONVSE_ASK_CHUNK_PAIRS"], n_pairs, nv, CONVSE_DT[dt])


def convse_max_chunks(entry, n_pairs, nv, dt="f32"):
    """workgroups of the launch: n_pairs / chunk_pairs + min(n_pairs, nv)."""
    return ask("xml_dispatch_convse_pairs", CONVSE_ENTRIES[entry], E["XML_CONVSE_ASK_MAX_CHUNKS"], n_pairs, nv, CONVSE_DT[dt])


def convse_form(nq, n_pairs, nv, lpad, l_ref, hidden, ksize, dt, summ=False, entry="k7"):
    """"<mainloop><steps>[+tail<bytes>]-<epilogue>-<inversion>" of one K7 / span-evidence launch, or "refused"."""
    loop = convse_mainloop(entry, nq, lpad, l_ref, hidden, ksize, dt)
    if loop == "refused":
        return loop
    steps, last = convse_steps(hidden, dt)
    tail = "" if last == CONVSE_STEP_BYTES else "+tail%d" % last
    return "%s%d%s-%s-%s" % (loop, steps, tail, convse_epilogue(entry, ksize, summ, dt), convse_inversion(entry, n_pairs, nv, dt))


def rescore_form(nq, n_pairs, nv, lpad, hidden, dt):
    """"<mainloop><steps>[+tail<bytes>]-chunk<pairs>-<inversion>" of one xml_q2c_rescore launch, or "refused"."""
    loop = convse_mainloop("rescore", nq, lpad, lpad, hidden, 5, dt)
    if loop == "refused":
        return loop
    steps, last = convse_steps(hidden, dt)
    tail = "" if last == CONVSE_STEP_BYTES else "+tail%d" % last
    return "%s%d%s-chunk%d-%s" % (loop, steps, tail, convse_chunk_pairs("rescore", n_pairs, nv, dt),
                                  convse_inversion("rescore", n_pairs, nv, dt))


# ---- attention -----------------------------------------------------------------------------------------------------------
ATTN_KERNELS = {E["XML_ATTN_SMALL"]: "small", E["XML_ATTN_LARGE"]: "large",
                E["XML_ATTN_REFUSED_HEADS"]: "refused: hidden % n_heads",
                E["XML_ATTN_REFUSED_LENGTH"]: "refused: longer than %d" % ATTN_MAX_L,
                E["XML_ATTN_REFUSED_LDS"]: "refused: LDS", E["XML_ATTN_REFUSED_DH"]: "refused: DH"}


def attn_form(lq, lk, hidden, n_heads, es):
    """xmli_attention_core: "small" (several (sequence, head) units per workgroup), "large", or the reason it is refused."""
    return ATTN_KERNELS[ask("xml_dispatch_attention", lq, lk, hidden, n_heads, dt_of(es))]


def attn_train_ok(lq, lk, hidden, n_heads):
    """xml_attention_train_supported (bf16)."""
    return bool(LIB.xml_attention_train_supported(lq, lk, hidden, n_heads, _lib.XML_BF16))
