"""Row invariance at every dispatch edge: an encoder output row has the same bits however many rows its launch holds.

The library picks kernels by row count (linear.hip xmli_gemm / launch_gemm, gemm256.hip, gemm256p.hip and the LayerNorm
epilogue's row threshold).  The corpus index being independent of the context batch, vcmr_search_host's chunked records
equalling the single launch and the packed query encoder equalling the padded one all rest on those forms giving the
same bits.  Each test below recomputes row PREFIXES of one large input on both sides of every edge (the helpers ask the
library for its dispatch rules, tests/kernel_forms.py, and assert that the chosen pairs really straddle them) and compares bit for bit; the GEMMs are also
held against float64 with a bound that scales with K, the LayerNorm rows against a float64 LayerNorm of the same
pre-LayerNorm values.  Run on the MI355X box:  pytest -m gpu"""
import ctypes

import pytest
import torch

from kernel_forms import (cdiv, few, gemm256_ok, gemm256p_ok, gemm_form, gemm_ln_fused,  # noqa: F401
                          small_bmn, small_kloop)      # the library's dispatch rules (xml_dispatch_*)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
U32 = 2.0 ** -24                       # unit roundoff of f32
BIG_BYTES = 3 << 30                    # largest A operand built for an edge (the gemm256p edge of N = 256 at K = 3 072 is 9.7 GB)


def first_true(pred, hi=1 << 24):
    """smallest m >= 1 with pred(m), for a predicate monotone in m (None if none up to hi)."""
    if not pred(hi):
        return None
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


def straddle(pred, name):
    """(e - 1, e) with pred(e - 1) != pred(e), asserted."""
    e = first_true(pred)
    if e is None or e < 2:
        return []
    assert pred(e - 1) != pred(e), name
    return [(name, e)]


def gemm_edges(n, k, es):
    """every row-count edge of xmli_gemm at (N, K) as (name, first row of the new side)."""
    edges = straddle(lambda m: not few(m, n), "few")
    edges += straddle(lambda m: small_bmn(m, n) >= 64, "bmn64")
    edges += straddle(lambda m: small_bmn(m, n) >= 128, "bmn128")
    edges += straddle(lambda m: gemm256_ok(m, n, k, es), "gemm256")
    edges += straddle(lambda m: gemm256p_ok(m, n, k, es), "gemm256p")
    return [(nm, e) for nm, e in edges if e * k * es <= BIG_BYTES]


FIXED_M = [1, 15, 16, 17, 255, 256, 257]


def edge_rows(edges):
    ms = set(FIXED_M)
    for _, e in edges:
        ms.update((e - 1, e, e + 1))
    return sorted(ms)


def test_edge_helpers_straddle_the_cpp_thresholds():
    """(no GPU needed, but kept with its users) the pairs really fall on both sides, and the forms they select differ."""
    for n, k, es in ((768, 768, 2), (256, 256, 4), (2304, 768, 4), (384, 256, 2)):
        for nm, e in gemm_edges(n, k, es):
            if nm in ("few", "gemm256p"):
                assert gemm_form(e - 1, n, k, es) != gemm_form(e, n, k, es), (n, k, es, nm, e)
    assert few(5376, 768) and not few(5377, 768)
    assert not gemm256p_ok(261888, 768, 768, 2) and gemm256p_ok(261889, 768, 768, 2)
    assert not gemm_ln_fused(2047, 768, 768, 2) and gemm_ln_fused(2048, 768, 768, 2)
    assert not gemm_ln_fused(1 << 20, 768, 3080, 4)             # TEF K: never fused
    assert small_kloop(3080, 4, 64) == "plain" and small_kloop(768, 2, 32) == "deep3" and small_kloop(256, 4, 64) == "deep2"


# ---- helpers -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from tvretrieval_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture
def dbg_lib(ops, monkeypatch):
    """the -DXML_DEBUG_VARIANTS build standing in for the product library during one test (see test_gpu_kernels.py)."""
    import os
    path = os.path.join(os.path.dirname(ops._lib.LIB_PATH), "libxmlhip_dbg.so")
    if not os.path.isfile(path):
        pytest.skip("libxmlhip_dbg.so not built (XML_DEBUG=1 bash tvretrieval_amd/csrc/build.sh)")
    lib = ops._lib.bind(ctypes.CDLL(path))
    monkeypatch.setattr(ops._lib, "_lib", lib)
    return lib


def grid_randn(shape, gen, scale=1.0):
    """N(0, scale^2) on the bf16 grid, built on the device (products of two such values are exact in f32)."""
    return (torch.randn(shape, device=DEV, generator=gen) * scale).to(torch.bfloat16).float()


def diff_msg(a, b):
    bad = (a != b) & ~(torch.isnan(a.float()) & torch.isnan(b.float()))
    r = bad.reshape(bad.shape[0], -1).any(1).nonzero()
    return "%d elements differ in %d rows (first row %s), max |d| %g" % (
        int(bad.sum()), r.numel(), int(r[0]) if r.numel() else -1, float((a.float() - b.float()).abs().max()))


def assert_bits(a, b, what):
    assert a.shape == b.shape, what
    assert torch.equal(a, b), "%s: %s" % (what, diff_msg(a, b))


def check_gemm_f64(y, x, w, b, addend, relu, rows, what, bf16_out):
    """|y - ref| <= K 2^-24 sum_k |x_k w_k| + 3 2^-24 (|b| + |addend| + |ref|) [+ one bf16 rounding of the output], per
    element: the products are exact (bf16-grid inputs), only the K-term sum and the epilogue's additions round."""
    xr, yr = x[rows].double(), y[rows].double()
    pre = xr @ w.double().t()
    mag = x.shape[1] * U32 * (xr.abs() @ w.double().abs().t())
    if b is not None:
        pre, mag = pre + b.double(), mag + 3 * U32 * b.double().abs()
    if relu:
        pre = pre.clamp_min(0)
    if addend is not None:
        ar = addend[rows].double()
        pre, mag = pre + ar, mag + 3 * U32 * ar.abs()
    lim = mag + 3 * U32 * pre.abs()
    if bf16_out:
        lim = 2 * lim + 2.0 ** -8 * pre.abs()
    err = (yr - pre).abs()
    bad = err > lim
    assert not bad.any(), "%s vs float64: %d off, worst err %.3e vs bound %.3e (row %d)" % (
        what, int(bad.sum()), float(err[bad].max()), float(lim[bad][err[bad].argmax()]),
        int(rows[int(bad.nonzero()[0, 0])]))


# every projection shape of the model at hidden 256 and 768: input projections (K = 3 072 / 768 / the TEF d_pad 3 080, whose
# last 128-byte K step is partial), QKV (3 H), stacked K / V (2 H), the output dense layer (H), and an N that is not a
# multiple of 256
GEMM_SHAPES = [(256, 3072), (256, 768), (256, 3080), (768, 256), (512, 256), (256, 256), (384, 256),
               (768, 3072), (768, 3080), (2304, 768), (1536, 768), (768, 768)]


# ---- (a, b) GEMM family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "n%d_k%d" % s)
def test_gemm_rows_do_not_depend_on_the_row_count(ops, dtype, shape):
    """ops.linear on row prefixes across every xmli_gemm edge (few / tile size / K loop / gemm256 / gemm256p, each +-1 row,
    and M = 1, 15 .. 257) gives the bits of the largest launch; bias, ReLU, residual addend, bf16 and f32 out.  The rows at
    the edges are held against float64."""
    n, k = shape
    es = 2 if dtype == torch.bfloat16 else 4
    ms = edge_rows(gemm_edges(n, k, es))
    m_big = ms[-1] + 1
    g = torch.Generator(device=DEV).manual_seed(n * 7 + k)
    x = grid_randn((m_big, k), g)
    x[1::7] *= 2.0 ** -12                      # small-magnitude rows: a dropped or doubled K tail would stand out there
    x = x.to(dtype)
    w = grid_randn((n, k), g, k ** -0.5).to(dtype)
    b = grid_randn((n,), g)
    add = grid_randn((m_big, n), g).to(dtype)
    check_rows = torch.tensor(sorted({min(r, m_big - 1) for m in ms for r in (m - 2, m - 1, m)} | set(range(16))), device=DEV)
    for relu, bias, addend in ((False, None, None), (False, b, None), (True, b, add)):
        big = ops.linear(x, w, bias, relu=relu, addend=addend)
        what = "N=%d K=%d %s relu=%d bias=%d addend=%d" % (n, k, dtype, relu, bias is not None, addend is not None)
        check_gemm_f64(big, x, w, bias, addend, relu, check_rows, what, dtype == torch.bfloat16)
        for m in ms:
            part = ops.linear(x[:m], w, bias, relu=relu, addend=None if addend is None else addend[:m])
            assert_bits(part, big[:m], "%s: M=%d (%s) vs M=%d (%s)" % (what, m, gemm_form(m, n, k, es), m_big,
                                                                         gemm_form(m_big, n, k, es)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(768, 768), (256, 3080), (2304, 768), (384, 256), (512, 256)], ids=lambda s: "n%d_k%d" % s)
def test_gemm_variants_give_the_same_bits_at_the_same_rows(ops, dbg_lib, dtype, shape):
    """xml_debug_set_gemm_variant 0 (product dispatch) / 1 (no persistent kernel) / 3 (no small-tile form for `few`) at the
    rows on both sides of each edge: every form the switches reach gives the same bits."""
    n, k = shape
    es = 2 if dtype == torch.bfloat16 else 4
    edges = gemm_edges(n, k, es)
    ms = sorted({m for _, e in edges for m in (e - 1, e)} | {255, 256})
    g = torch.Generator(device=DEV).manual_seed(n + k)
    x = grid_randn((ms[-1], k), g).to(dtype)
    w = grid_randn((n, k), g, k ** -0.5).to(dtype)
    b = grid_randn((n,), g)
    add = grid_randn((ms[-1], n), g).to(dtype)
    try:
        for m in ms:
            res = []
            for variant in (0, 1, 3):
                dbg_lib.xml_debug_set_gemm_variant(ctypes.c_int(variant))
                res.append(ops.linear(x[:m], w, b, relu=True, addend=add[:m]))
            assert_bits(res[1], res[0], "N=%d K=%d %s M=%d: variant 1 vs 0" % (n, k, dtype, m))
            assert_bits(res[2], res[0], "N=%d K=%d %s M=%d: variant 3 vs 0" % (n, k, dtype, m))
    finally:
        dbg_lib.xml_debug_set_gemm_variant(ctypes.c_int(0))


# ---- (c) split-f16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(768, 768), (256, 256), (2304, 768)], ids=lambda s: "n%d_k%d" % s)
def test_split_f16_rows_do_not_depend_on_the_row_count(ops, shape):
    """ops.pack_weights_f16s + ops.linear (gemm256_f16s from 256 rows, the small-tile f16 form below): row prefixes across
    M = 255 / 256 and the `few` edge give the bits of the largest launch."""
    n, k = shape
    e_few = first_true(lambda m: not few(m, n))
    ms = sorted(set(FIXED_M) | {e_few - 1, e_few, e_few + 1})
    g = torch.Generator(device=DEV).manual_seed(n + 3 * k)
    x = torch.randn(ms[-1] + 1, k, device=DEV, generator=g)
    w = torch.randn(n, k, device=DEV, generator=g) * k ** -0.5
    b = torch.randn(n, device=DEV, generator=g)
    sw = ops.pack_weights_f16s(w)
    big = ops.linear(x, sw, b, relu=True)
    for m in ms:
        assert_bits(ops.linear(x[:m].contiguous(), sw, b, relu=True), big[:m], "split-f16 N=%d K=%d M=%d" % (n, k, m))
    want = torch.relu(torch.nn.functional.linear(x[:300].double(), w.double(), b.double()))
    err = (big[:300].double() - want).abs().max()
    assert err < 1e-5 * float(want.abs().max()), "split-f16 vs float64: %g" % float(err)


# ---- (d) the LayerNorm-epilogue edge -------------------------------------------------------------------------------------
H_LN = [256, 512, 768]


def _ln_f64_check(y, pre64, d, g, beta, what):
    """y against LN(pre64) * g + beta in float64; pre64 is exact, the kernel's f32 pre-LayerNorm values are within d of it
    elementwise.  Bound per element: |g| rstd (2 max_row d + 40 2^-24 max|pre_row|) (1 + |xhat|) [+ one bf16 rounding]: the
    second term is the f32 statistics' own error (32 sequential additions per lane, then the butterfly and the combine)."""
    mean = pre64.mean(-1, keepdim=True)
    var = pre64.var(-1, unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    xhat = (pre64 - mean) * rstd
    ref = xhat * g.double() + beta.double()
    d_row = d.amax(-1, keepdim=True)
    lim = g.double().abs() * rstd * (2 * d_row + 40 * U32 * pre64.abs().amax(-1, keepdim=True)) * (1 + xhat.abs()) + 1e-6
    if y.dtype == torch.bfloat16:
        lim = lim + 2.0 ** -8 * ref.abs()
    err = (y.double() - ref).abs()
    bad = err > lim
    assert not bad.any(), "%s vs float64 LayerNorm: %d off, worst err %.3e (bound %.3e)" % (
        what, int(bad.sum()), float(err[bad].max()), float(lim[bad][err[bad].argmax()]))


def _k1_weights(h, d_in, l, dtype, gen, hi_mean):
    ln_in = (1 + 0.1 * grid_randn((d_in,), gen), 0.1 * grid_randn((d_in,), gen))
    w = grid_randn((h, d_in), gen, d_in ** -0.5)
    b = 0.1 * grid_randn((h,), gen)
    if hi_mean:         # every pre-LayerNorm row ~ 1e3 + N(0, 1e-2): large mean, small variance
        w = w * 2.0 ** -7
        b = 1e3 + 1e-2 * torch.randn(h, device=DEV, generator=gen)
    pos = grid_randn((l, h), gen, 0.5)
    if hi_mean:
        pos = pos * 2.0 ** -8
    ln_pos = (1 + 0.1 * grid_randn((h,), gen), 0.1 * grid_randn((h,), gen))
    return ln_in, w.to(dtype), b, pos.to(dtype), ln_pos


def _k1_reference(ops, x2d, pos_rows, ln_in, w, b, ln_pos, dtype, what, y):
    """float64 LayerNorm of the exact pre-LayerNorm values of the kernel's own LN_in output."""
    xn = ops.add_layernorm(x2d, None, ln_in[0], ln_in[1], out_dtype=dtype).double()
    wd = w.double()
    pre = torch.relu(xn @ wd.t() + b.double()) + pos_rows.double()
    d = w.shape[1] * U32 * (xn.abs() @ wd.abs().t()) + 2 * U32 * (b.double().abs() + pos_rows.double().abs() + pre.abs())
    _ln_f64_check(y.reshape(pre.shape), pre, d, ln_pos[0], ln_pos[1], what)


@pytest.mark.parametrize("hi_mean", [False, True], ids=["plain", "mean1e3"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", H_LN)
def test_k1k2_rows_do_not_depend_on_the_layernorm_edge(ops, h, dtype, hi_mean):
    """linear_ln_relu_pos: the LayerNorm runs in the GEMM epilogue from 2 048 rows on and behind a GEMM with f32 out below;
    rows of 2 047 / 2 048 raw rows, 15 / 16 sequences of 128, a 50-query batch (1 500 rows) and 7 680 rows equal the rows of
    the largest launch bit for bit, and a float64 LayerNorm of the same pre-LayerNorm values."""
    d_in = 768
    es = 2 if dtype == torch.bfloat16 else 4
    gen = torch.Generator(device=DEV).manual_seed(h + 11 * hi_mean)
    for l, ns in ((1, (2047, 2048, 2100)), (128, (15, 16, 60)), (30, (50, 70))):
        rows = [n_ * l for n_ in ns]
        assert any(not gemm_ln_fused(r, h, d_in, es) for r in rows) and gemm_ln_fused(max(rows), h, d_in, es), (l, ns)
        ln_in, w, b, pos, ln_pos = _k1_weights(h, d_in, l, dtype, gen, hi_mean)
        x = torch.randn(ns[-1], l, d_in, device=DEV, generator=gen)
        args = (ln_in[0], ln_in[1], w, b, pos, ln_pos[0], ln_pos[1])
        big = ops.linear_ln_relu_pos(x, *args)
        for n_ in ns[:-1]:
            part = ops.linear_ln_relu_pos(x[:n_].contiguous(), *args)
            assert_bits(part, big[:n_], "K1+K2 H=%d %s L=%d: %d rows (fused %d) vs %d rows (fused %d)" % (
                h, dtype, l, n_ * l, gemm_ln_fused(n_ * l, h, d_in, es), ns[-1] * l, gemm_ln_fused(ns[-1] * l, h, d_in, es)))
        nr = min(ns[-1], max(1, 256 // l))     # a few hundred rows against float64, fused side and unfused side
        pos_rows = pos.float().repeat(nr, 1)
        what = "K1+K2 H=%d %s L=%d" % (h, dtype, l)
        _k1_reference(ops, x[:nr].reshape(-1, d_in), pos_rows, ln_in, w, b, ln_pos, dtype, what, big[:nr])


def _lengths_hitting(targets, lq, gen):
    """query lengths in 1..lq whose running token count passes through every target exactly."""
    lens, tot = [], 0
    for t in sorted(targets):
        while t - tot > lq:
            v = int(torch.randint(1, lq + 1, (1,), generator=gen))
            v = min(v, t - tot - 1)
            lens.append(v)
            tot += v
        lens.append(t - tot)
        tot = t
    cum = torch.tensor(lens).cumsum(0).tolist()
    return lens, {t: cum.index(t) + 1 for t in targets}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", H_LN)
def test_packed_k1k2_and_varlen_attention_rows_do_not_depend_on_the_layernorm_edge(ops, h, dtype):
    """linear_ln_relu_pos_packed and attention_block_varlen on packed tokens: the first queries of a batch whose token count
    is 1 500 / 2 047 / 2 048 give the rows of a 7 680-token batch bit for bit (K1+K2 also against float64)."""
    lq, d_in, nh = 30, 768, 4
    es = 2 if dtype == torch.bfloat16 else 4
    gen = torch.Generator().manual_seed(h)
    gdev = torch.Generator(device=DEV).manual_seed(h + 1)
    targets = (1500, 2047, 2048, 7680)
    lens, n_at = _lengths_hitting(targets, lq, gen)
    assert not gemm_ln_fused(2047, h, d_in, es) and gemm_ln_fused(2048, h, d_in, es)
    n = len(lens)
    mask = (torch.arange(lq)[None] < torch.tensor(lens)[:, None]).float().to(DEV)
    x = torch.randn(n * lq, d_in, device=DEV, generator=gdev)
    ln_in, w, b, pos, ln_pos = _k1_weights(h, d_in, lq, dtype, gdev, False)
    args = (ln_in[0], ln_in[1], w, b, pos, ln_pos[0], ln_pos[1])
    wqkv = grid_randn((3 * h, h), gdev, h ** -0.5).to(dtype)
    wo = grid_randn((h, h), gdev, h ** -0.5).to(dtype)
    aw = (wqkv, 0.1 * grid_randn((3 * h,), gdev), wo, 0.1 * grid_randn((h,), gdev), 1 + 0.1 * grid_randn((h,), gdev),
          0.1 * grid_randn((h,), gdev), nh)
    res = {}
    for t in targets:
        nq = n_at[t]
        cu, src, rows = ops.pack_plan(mask[:nq].contiguous(), rows=t)
        enc = ops.linear_ln_relu_pos_packed(x[:nq * lq], src, rows, lq, *args)
        att = ops.attention_block_varlen(enc, cu, nq, lq, *aw)
        res[t] = (enc, att, src)
    big_enc, big_att, big_src = res[7680]
    for t in targets[:-1]:
        what = "H=%d %s: %d packed tokens (fused %d) vs 7680" % (h, dtype, t, gemm_ln_fused(t, h, d_in, es))
        assert_bits(res[t][0], big_enc[:t], "linear_ln_relu_pos_packed " + what)
        assert_bits(res[t][1], big_att[:t], "attention_block_varlen " + what)
    for lo, hi in ((0, 300), (2000, 2100)):
        src = big_src[lo:hi].long()
        _k1_reference(ops, x[src], pos.float()[src % lq], ln_in, w, b, ln_pos, dtype,
                      "packed K1+K2 H=%d %s rows %d..%d" % (h, dtype, lo, hi), big_enc[lo:hi])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", H_LN)
def test_attention_block_rows_do_not_depend_on_the_layernorm_edge(ops, h, dtype):
    """attention_block (BertSelfOutput: dense + residual + LayerNorm, fused from 2 048 rows): 15 / 16 sequences of 128 and a
    50-query batch of 30 tokens give the rows of a larger batch bit for bit; one sequence's residual rows sit at 1e3 with a
    spread of 1e-2 (f32: representable; bf16: the grid around 1e3 is 4 wide, so a spread of a few units)."""
    nh = 4
    gen = torch.Generator(device=DEV).manual_seed(h + 5)
    wqkv = grid_randn((3 * h, h), gen, h ** -0.5).to(dtype)
    wo = grid_randn((h, h), gen, h ** -0.5 * 2.0 ** -6).to(dtype)
    aw = (wqkv, 0.1 * grid_randn((3 * h,), gen), wo, 0.1 * grid_randn((h,), gen), 1 + 0.1 * grid_randn((h,), gen),
          0.1 * grid_randn((h,), gen), nh)
    for l, ns in ((128, (15, 16, 20)), (30, (50, 70))):
        x = torch.randn(ns[-1], l, h, device=DEV, generator=gen)
        x[1] = 1e3 + (1e-2 if dtype == torch.float32 else 4.0) * torch.randn(l, h, device=DEV, generator=gen)
        x = x.to(dtype)
        mask = (torch.arange(l, device=DEV)[None] < torch.randint(1, l + 1, (ns[-1], 1), device=DEV, generator=gen)).float()
        mask[0] = 1
        big = ops.attention_block(x, mask, *aw)
        assert torch.isfinite(big.float()).all()
        for n_ in ns[:-1]:
            part = ops.attention_block(x[:n_].contiguous(), mask[:n_].contiguous(), *aw)
            assert_bits(part, big[:n_], "attention_block H=%d %s L=%d: %d rows vs %d rows" % (h, dtype, l, n_ * l, ns[-1] * l))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention_rows_do_not_depend_on_the_gemm_edges(ops, dtype):
    """cross_attention always normalises behind its GEMMs (add_layernorm); its projections cross the xmli_gemm edges with
    the number of sequences: prefixes of 2 / 16 / 45 sequences of 128 give the rows of 60 bit for bit."""
    h, l, nh = 768, 128, 4
    gen = torch.Generator(device=DEV).manual_seed(9)
    main = torch.randn(60, l, h, device=DEV, generator=gen).to(dtype)
    side = torch.randn(60, l, h, device=DEV, generator=gen).to(dtype)
    mm = (torch.arange(l, device=DEV)[None] < torch.randint(1, l + 1, (60, 1), device=DEV, generator=gen)).float()
    sm = (torch.arange(l, device=DEV)[None] < torch.randint(1, l + 1, (60, 1), device=DEV, generator=gen)).float()
    cw = (grid_randn((h, h), gen, h ** -0.5).to(dtype), 0.1 * grid_randn((h,), gen),
          grid_randn((2 * h, h), gen, h ** -0.5).to(dtype), 0.1 * grid_randn((2 * h,), gen),
          1 + 0.1 * grid_randn((h,), gen), 0.1 * grid_randn((h,), gen), nh)
    es = 2 if dtype == torch.bfloat16 else 4
    assert few(2 * l, 2 * h) and not few(45 * l, 2 * h)
    big = ops.cross_attention(main, mm, side, sm, *cw)
    for n_ in (2, 16, 45):
        part = ops.cross_attention(main[:n_].contiguous(), mm[:n_].contiguous(), side[:n_].contiguous(), sm[:n_].contiguous(), *cw)
        assert_bits(part, big[:n_], "cross_attention %s: %d sequences (%s) vs 60 (%s)" % (
            dtype, n_, gemm_form(n_ * l, 2 * h, h, es), gemm_form(60 * l, 2 * h, h, es)))
