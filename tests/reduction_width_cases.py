"""Parameter tables of the reduction-width sweep: tests/test_gpu_reduction_width.py runs every case on the GPU,
tests/test_reduction_width_plan.py (no GPU) proves from the same tables that every case lands on the kernel it is meant for
and that no residue class, minimum or above-model count is missing.

A software-pipelined kernel's prologue, steady state and drain depend on the number of 64-byte K slices per row,
n_slices = K * sizeof(T) / 64: on its value modulo the ring depth and on whether it exceeds the prefetch depth.  The persistent
kernels (gemm256p.hip, q2c_persist.hip) do not restart their ring per tile or per modality segment, so n_slices modulo the
ring depth decides in which slot every later tile starts.  The model's own widths (128 ... 768, 3 072) reach only some classes.

Every case is a plain tuple whose first entries name the form; `case_id` makes the pytest id."""
import kernel_forms as DM

ES = {"f32": 4, "bf16": 2, "f16": 2}
MODEL_MAX_SLICES = 48           # hidden 768 in f32: the largest count the model's hidden sizes give K6


def k_of(n_slices, dtype):
    """elements of K (or hidden) that make n_slices 64-byte slices."""
    return n_slices * DM.SLICE_BYTES // ES[dtype]


def case_id(case):
    return "-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in case)


# ---- GEMM through ops.linear -------------------------------------------------------------------------------------------
GEMM_DTYPES = ("f32", "bf16")
ATTN_HEADS = (1, 2, 3, 4, 8)
# >= 64 tiles of 256 x 256 and far fewer than 3 072; ragged M, N not a multiple of 256
GEMM256_SHAPES = ((16384, 256), (16421, 328))
GEMM256_SLICES = (4, 6, 8, 10, 12, 14, 18)
# 1 025 x 3 = 3 075 tiles, ragged last row tile: every workgroup walks ~12 tiles through one ring
GEMM256P_SHAPES = ((262145, 768),)
GEMM256P_SLICES = (4, 6, 8, 10, 14)


def gemm256_cases():
    """(form, dtype, (M, N), n_slices)"""
    return [("gemm256", dt, mn, s) for dt in GEMM_DTYPES for mn in GEMM256_SHAPES for s in GEMM256_SLICES]


def gemm256p_cases():
    return [("gemm256p", dt, mn, s) for dt in GEMM_DTYPES for mn in GEMM256P_SHAPES for s in GEMM256P_SLICES]


# small-tile kernel: one (M, N) per tile size, ns = ceil(K * es / 128) = 1 .. 9, each with a whole and a partial last step
SMALL_SHAPES = {32: (100, 136), 64: (1000, 700), 128: (65537, 120)}
SMALL_STEPS = tuple(range(1, 10))


def small_ks(ns, dtype):
    """K with ns whole 128-byte steps, and K whose last step holds 16 bytes (8 bf16 / 4 f32 elements)."""
    return 128 * ns // ES[dtype], (128 * (ns - 1) + 16) // ES[dtype]


def small_cases():
    """(form, dtype, (M, N), ns, K)"""
    return [("small%d" % bmn, dt, SMALL_SHAPES[bmn], ns, k) for bmn in sorted(SMALL_SHAPES) for dt in GEMM_DTYPES
            for ns in SMALL_STEPS for k in small_ks(ns, dt)]


# LayerNorm-epilogue GEMM through ops.linear_ln_relu_pos: 17 sequences x 128 = 2 176 rows, K = the projection's d_in
LN_SEQS, LN_LEN = 17, 128
LN_WIDTHS = (256, 512, 768)
LN_SLICES = (4, 6, 10, 14)


def ln_cases():
    """(form, dtype, N, n_slices)"""
    return [("gemm_ln", dt, h, s) for dt in GEMM_DTYPES for h in LN_WIDTHS for s in LN_SLICES]


# BertSelfOutput (ops.attention_block): the dense layer's K is the hidden size itself, so N picks the slice count; the head
# counts put the attention core at DH = 128 / 32 / 64 / 96
ATTENTION_BLOCK_CASES = tuple(("attention_block", dt, h, nh) for dt in GEMM_DTYPES
                              for h, nh in ((256, 2), (256, 8), (512, 8), (768, 8)))

# ... and the whole block at every head size and head count, on both attention kernels (behind the fused QKV buffer, row
# stride 3 H): 180 / 384 rows, so BertSelfOutput is the unfused GEMM + LayerNorm tail, at hidden sizes 32 ... 1 536
ATTENTION_BLOCK_SHAPES = ((6, 30), (3, 128))        # (n, l): small kernel, large kernel


def attention_block_cases(dtypes=GEMM_DTYPES):
    """(form, dtype, DH, n_heads, (n, l))"""
    return [("attention_block", dt, dh, nh, shp) for dt in dtypes for dh in DM.ATTN_DH for nh in ATTN_HEADS
            for shp in ATTENTION_BLOCK_SHAPES]


# split-f16 projection: n_slices = 6 K / 64; one row count on each side of M >= 256
F16S_KS = (64, 128, 192, 256, 320)
F16S_ROWS = (200, 300)
F16S_N = 328


def f16s_cases():
    """(form, M, K)"""
    return [("f16s", m, k) for m in F16S_ROWS for k in F16S_KS]


# ---- K6 -----------------------------------------------------------------------------------------------------------------
K6_FORMS = ("rowmajor", "tiled_float", "nomask", "bitmask", "packed")      # operand layout / mask form of the persistent kernel
K6_TILED = {"rowmajor": False, "tiled_float": True, "nomask": True, "bitmask": True, "packed": True}
K6_MASK = {"rowmajor": "float", "tiled_float": "float", "nomask": "nomask", "bitmask": "bitmask", "packed": "packed"}
K6_DTYPES = {"rowmajor": ("f32", "bf16"), "tiled_float": ("f32", "bf16", "f16"), "nomask": ("f32", "bf16", "f16"),
             "bitmask": ("f32", "bf16", "f16"), "packed": ("f32", "bf16", "f16")}
# (520, 300): three query tiles -> qsh = 2, three rounds per workgroup: the ring phase carries across tiles;
# (300, 5): an odd number of videos leaves half a clip tile
K6_PERSIST_SHAPES = ((520, 300), (300, 5))
K6_PERSIST_SLICES = (6, 8, 10, 12, 14, 16, 18, 20, 22, 30, 40, 64)
K6_N_MOD = (1, 2)


def k6_persist_keys():
    """(dtype, n_slices, (nq, nv)): one set of operands and float64 references, shared by the forms and modality counts."""
    return [(dt, s, shp) for dt in ("f32", "bf16", "f16") for s in K6_PERSIST_SLICES for shp in K6_PERSIST_SHAPES]


def k6_persist_cases():
    """(form, dtype, n_slices, (nq, nv), n_mod), the cases of one operand key next to each other"""
    return [(form, dt, s, shp, n_mod) for dt, s, shp in k6_persist_keys() for form in K6_FORMS if dt in K6_DTYPES[form]
            for n_mod in K6_N_MOD]


# q2c_ring: clip paddings below 128 (several videos per 128-column group), and lpad = 128 where the persistent kernel does
# not apply -- combine passes, and widths below its six-slice minimum
K6_RING_LPADS = (16, 48, 112, 128)
K6_RING_SLICES = (2, 4, 6, 8, 10, 12, 14)
K6_RING_SHAPE = (300, 37)


def k6_ring_cases():
    """(form, dtype, lpad, n_slices)"""
    return [("ring", dt, lpad, s) for dt in GEMM_DTYPES for lpad in K6_RING_LPADS for s in K6_RING_SLICES]


# register-staged q2c_scores_kernel<float> / <bf16_t>: hidden * es % 128 != 0
K6_STAGED_HIDDEN = (8, 24, 40, 72, 104, 200, 264)
K6_STAGED_LPADS = (16, 48, 128)
K6_STAGED_SHAPE = (130, 21)


def k6_staged_cases():
    """(form, dtype, lpad, hidden)"""
    return [("staged", dt, lpad, h) for dt in GEMM_DTYPES for lpad in K6_STAGED_LPADS for h in K6_STAGED_HIDDEN]


# normalise / tile passes at d / vec = 32 * L2N_MAXJ chunks of 16 bytes and 8 elements beyond
L2N_WIDTHS = {"f32": (1024, 1032), "bf16": (2048, 2056)}


def l2n_cases():
    """(form, dtype, d)"""
    return [("l2norm", dt, d) for dt in GEMM_DTYPES for d in L2N_WIDTHS[dt]]


# ---- attention ------------------------------------------------------------------------------------------------------------
ATTN_SHAPES = ((5, 13, 21), (3, 128, 128), (6, 30, 30))       # (n, lq, lk): small kernel (rectangular), large, small


def attention_cases(dtypes=GEMM_DTYPES):
    """(form, dtype, DH, n_heads, (n, lq, lk))"""
    return [("attention", dt, dh, nh, shp) for dt in dtypes for dh in DM.ATTN_DH for nh in ATTN_HEADS for shp in ATTN_SHAPES]
