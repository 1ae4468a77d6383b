"""Every reduction-width class of the software-pipelined kernels against float64.

The kernels that stage their operands through an LDS ring with hand-counted waits (gemm256.hip, gemm256p.hip with its
LayerNorm epilogue, q2c_persist.hip, q2c_ring.hip) are right or wrong per NUMBER OF 64-BYTE K SLICES: its value modulo the ring
depth (the persistent kernels carry the ring phase across tiles and modality segments), whether it exceeds the prefetch
depth, and the minimum the predicates accept.  The model's widths reach only some of those classes; this file sweeps the rest,
through the public wrappers of the product library, at the smallest shapes that still select each form (tables:
tests/reduction_width_cases.py; the proof that every case lands on its form and no class is missing needs no GPU:
tests/test_reduction_width_plan.py).  The register-staged K6 kernel, the small-tile GEMM's three K loops, the split-f16 GEMM,
the normalise / tile passes at their width limit and attention at every head size and several head counts ride along.

Operands lie on the bf16 grid, so f32 and bf16 kernels see the same numbers and every product is exact in f32; references are
plain torch in float64 on the device.  Bounds, none of them fitted to what the kernels return:
* GEMM: |y - ref| <= K 2^-24 sum_k |x_k w_k| + 3 2^-24 (|b| + |addend| + |ref|) per element (K f32 additions, three roundings of
  the epilogue).  A bf16 output is ONE round-to-nearest of a value inside that interval: rne(ref - lim) <= y <= rne(ref + lim).
  (bf16 keeps 8 significand bits, so one rounding moves a value by up to 2^-8 of its magnitude at the bottom of a binade;
  profiles/numerics_margins.md, "Reduction-width sweep", has the figure of a plain torch product at these shapes.)
* K6: unit rows, so sum_k |q_k c_k| <= |q| |c| (Cauchy-Schwarz, with the rows' actual norms after the grid rounding):
  |s - ref| <= K 2^-24 |q| max_l |c_l| + 3 2^-24 |ref|; the masked maximum and the mean over modalities keep that bound.
* split-f16, LayerNorm epilogue, normalise passes, attention: the checkers and margins of the existing tests of those ops
  (tests/test_gpu_split16.py, tests/test_gpu_row_invariance.py, tests/test_gpu_numerics.py, tests/test_gpu_train_bf16.py).
Run on the MI355X box:  pytest -m gpu"""
import math

import pytest
import torch

import kernel_forms as DM
import numerics_regimes as NR
import reduction_width_cases as RC
import train_bf16_cases as TC
from test_gpu_row_invariance import DEV, U32, _k1_reference, _k1_weights, grid_randn, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
F16_SCALE = 2.0 ** 14           # ops.F16_UNIT_LOG2: unit rows in f16 form carry this fixed scale on both sides
C_ATTENTION, M_CHAIN_BF16, C_ROWWISE = 4, 4, 2       # the margins of tests/test_gpu_numerics.py for these ops


def params(cases):
    return pytest.mark.parametrize("case", cases, ids=[RC.case_id(c) for c in cases])


# ---- GEMM ---------------------------------------------------------------------------------------------------------------
def bf16_interval(want, lim):
    """[rne_bf16(want - lim), rne_bf16(want + lim)] as float64; the float32 step on the way is rounded outwards."""
    lo, hi = want - lim, want + lim
    lo32, hi32 = lo.float(), hi.float()
    lo32 = torch.where(lo32.double() > lo, torch.nextafter(lo32, torch.full_like(lo32, -math.inf)), lo32)
    hi32 = torch.where(hi32.double() < hi, torch.nextafter(hi32, torch.full_like(hi32, math.inf)), hi32)
    return lo32.to(torch.bfloat16).double(), hi32.to(torch.bfloat16).double()


def check_linear(runs, x, w, what, chunk=32768):
    """runs: [(y, bias, relu, addend)] of one (x, w); every output row against float64, a chunk of rows at a time."""
    k = x.shape[1]
    wd = w.double()
    wa = wd.abs()
    worst = [0.0] * len(runs)
    for r0 in range(0, x.shape[0], chunk):
        xr = x[r0:r0 + chunk].double()
        dot = xr @ wd.t()
        mag = k * U32 * (xr.abs() @ wa.t())
        for i, (y, b, relu, addend) in enumerate(runs):
            pre, lim = dot, mag
            if b is not None:
                pre, lim = pre + b.double(), lim + 3 * U32 * b.double().abs()
            if relu:
                pre = pre.clamp_min(0)
            if addend is not None:
                ar = addend[r0:r0 + chunk].double()
                pre, lim = pre + ar, lim + 3 * U32 * ar.abs()
            lim = lim + 3 * U32 * pre.abs()
            yr = y[r0:r0 + chunk].double()
            err = (yr - pre).abs()
            if y.dtype == torch.bfloat16:
                lo, hi = bf16_interval(pre, lim)
                ok = (yr >= lo) & (yr <= hi)
                unit = lim + 2.0 ** -8 * pre.abs()
            else:
                ok = err <= lim
                unit = lim
            worst[i] = max(worst[i], float((err / unit.clamp_min(1e-300)).max()))
            bad = ~ok
            assert not bad.any(), "%s run %d (bias %d relu %d addend %d) vs float64: %d off, first at row %d col %d: got %r want %r bound %.3e" % (
                what, i, b is not None, relu, addend is not None, int(bad.sum()), r0 + int(bad.nonzero()[0, 0]),
                int(bad.nonzero()[0, 1]), float(yr[bad][0]), float(pre[bad][0]), float(lim[bad][0]))
    print("WIDTH %s: worst err / bound %s" % (what, " ".join("%.3f" % v for v in worst)))


def run_linear(ops, m, n, k, dtype, what):
    """ops.linear without bias, with bias, and with bias + ReLU + addend (the epilogues of the projections)."""
    td = TDT[dtype]
    g = torch.Generator(device=DEV).manual_seed(m * 3 + n * 5 + k)
    x = grid_randn((m, k), g)
    x[1::7] *= 2.0 ** -12                      # small-magnitude rows: a dropped or doubled K slice would stand out there
    x = x.to(td)
    w = grid_randn((n, k), g, k ** -0.5).to(td)
    b = grid_randn((n,), g)
    add = grid_randn((m, n), g).to(td)
    runs = [(ops.linear(x, w, bias, relu=relu, addend=addend), bias, relu, addend)
            for relu, bias, addend in ((False, None, None), (False, b, None), (True, b, add))]
    assert all(y.dtype == td and tuple(y.shape) == (m, n) for y, _, _, _ in runs)
    check_linear(runs, x, w, what)


@params(RC.gemm256_cases())
def test_gemm256_slice_counts(ops, case):
    """gemm256.hip: a prologue of four slices, n_slices - 4 steady-state steps (0, one pair, several pairs), four peeled
    tail steps."""
    _, dtype, (m, n), s = case
    k = RC.k_of(s, dtype)
    assert DM.gemm_form(m, n, k, RC.ES[dtype]) == "gemm256"
    run_linear(ops, m, n, k, dtype, RC.case_id(case))


@params(RC.gemm256p_cases())
def test_gemm256p_slice_counts(ops, case):
    """gemm256p.hip: a four-slot ring that runs on across the ~12 tiles of a workgroup -- with n_slices = 2 (mod 4) every other
    tile starts in slot 2.  Every output row is checked."""
    _, dtype, (m, n), s = case
    k = RC.k_of(s, dtype)
    assert DM.gemm_form(m, n, k, RC.ES[dtype]) == "gemm256p"
    run_linear(ops, m, n, k, dtype, RC.case_id(case))


@params(RC.small_cases())
def test_small_tile_gemm_k_loops(ops, case):
    """gemm_bias_act_kernel at each tile size: 1 .. 9 steps of 128 bytes (deep-3, deep-2 and plain K loops), whole and with
    16 bytes in the last step."""
    form, dtype, (m, n), ns, k = case
    es = RC.ES[dtype]
    assert DM.cdiv(k * es, 128) == ns and DM.gemm_form(m, n, k, es).split("-")[0] == form
    run_linear(ops, m, n, k, dtype, "%s (%s)" % (RC.case_id(case), DM.gemm_form(m, n, k, es)))


@params(RC.f16s_cases())
def test_split_f16_gemm_slice_counts(ops, case):
    """ops.linear with a split-f16 weight: K' = 3 K halves = 6 K / 64 slices, on the 256 x 256 LDS-DMA kernel (M >= 256) and the
    small-tile f16 kernel; the relative bound of test_linear_f16s_vs_float64."""
    _, m, k = case
    n = RC.F16S_N
    assert DM.f16s_form(m, n, k) == ("gemm256-f16s" if m >= 256 else "small%d-f16s" % DM.small_bmn(m, n))
    g = torch.Generator(device=DEV).manual_seed(m + k)
    x = torch.randn(m, k, device=DEV, generator=g) * torch.logspace(-2, 2, m, device=DEV)[:, None]
    w = torch.randn(n, k, device=DEV, generator=g) * k ** -0.5
    b = torch.randn(n, device=DEV, generator=g)
    for relu in (False, True):
        want = x.double() @ w.double().t() + b.double()
        f32 = (x @ w.t() + b).double()
        if relu:
            want, f32 = want.clamp_min(0), f32.clamp_min(0)
        got = ops.linear(x, ops.pack_weights_f16s(w), b, relu=relu)
        scale = (x.norm(dim=1, keepdim=True) * w.norm(dim=1)[None]).double()              # |x||w| per output
        err = float(((got.double() - want).abs() / scale).max())
        f32_err = float(((f32 - want).abs() / scale).max())
        print("WIDTH %s relu %d: max err / (|x||w|) = %.2e (torch f32 GEMM: %.2e)" % (RC.case_id(case), relu, err, f32_err))
        assert err < max(8e-7, 2.0 * f32_err), (case, relu, err, f32_err)


@pytest.mark.parametrize("hi_mean", [False, True], ids=["plain", "mean1e3"])
@params(RC.ln_cases())
def test_layernorm_epilogue_gemm_slice_counts(ops, case, hi_mean):
    """ops.linear_ln_relu_pos at 2 176 rows: the LayerNorm-epilogue GEMM (gemm256p.hip, LNE) with K = d_in; a workgroup runs the
    N / 256 tiles of its row block back to back through one ring.  Every row against the float64 LayerNorm of the exact
    pre-LayerNorm values."""
    _, dtype, h, s = case
    td, es = TDT[dtype], RC.ES[dtype]
    d_in = RC.k_of(s, dtype)
    n, l = RC.LN_SEQS, RC.LN_LEN
    assert DM.gemm_ln_fused(n * l, h, d_in, es)
    gen = torch.Generator(device=DEV).manual_seed(h + s + 11 * hi_mean)
    ln_in, w, b, pos, ln_pos = _k1_weights(h, d_in, l, td, gen, hi_mean)
    x = torch.randn(n, l, d_in, device=DEV, generator=gen)
    y = ops.linear_ln_relu_pos(x, ln_in[0], ln_in[1], w, b, pos, ln_pos[0], ln_pos[1])
    _k1_reference(ops, x.reshape(-1, d_in), pos.float().repeat(n, 1), ln_in, w, b, ln_pos, td, RC.case_id(case), y)


def run_attention_block(ops, dtype, n, l, h, nh, holes, pre_ln, what):
    """ops.attention_block on NR.attention_case (logits of sd ~2) with the checks of test_attention_block_peaked."""
    td = TDT[dtype]
    c = NR.attention_case(2.0, n, l, h, nh, td, holes, pre_ln=pre_ln)
    print("WIDTH %s: logit sd %.2f, mean max probability %.3f" % (what, c["logit_std"], c["mean_max_prob"]))
    sd = c["sd"]
    wqkv = torch.cat([sd["self.%s.weight" % k] for k in ("query", "key", "value")])
    bqkv = torch.cat([sd["self.%s.bias" % k] for k in ("query", "key", "value")])
    dev = lambda t, d=None: (t.to(DEV) if d is None else t.to(DEV).to(d)).contiguous()      # noqa: E731
    got = ops.attention_block(dev(c["x"], td), dev(c["mask"]), dev(wqkv, td), dev(bqkv), dev(sd["output.dense.weight"], td),
                              dev(sd["output.dense.bias"]), dev(sd["output.LayerNorm.weight"]), dev(sd["output.LayerNorm.bias"]), nh)
    if td == torch.float32:
        NR.check_f32("attention_block", what, got, c["W"], c["R"], C_ATTENTION)
    else:
        NR.check_bf16_chain("attention_block", what, got, c["W"], c["S"], M_CHAIN_BF16, ref=c["R"])


@params(list(RC.ATTENTION_BLOCK_CASES))
def test_attention_block_layernorm_epilogue_head_counts(ops, case):
    """ops.attention_block at 2 176 rows: BertSelfOutput on the LayerNorm-epilogue GEMM at N = K = 256 / 512 / 768, behind the
    large attention kernel at DH = 128 / 32 / 64 / 96 with 2 and 8 heads; the checker of test_attention_block_peaked."""
    _, dtype, h, nh = case
    n, l = RC.LN_SEQS, RC.LN_LEN
    assert DM.gemm_ln_fused(n * l, h, h, RC.ES[dtype]) and DM.attn_form(l, l, h, nh, RC.ES[dtype]) == "large"
    run_attention_block(ops, dtype, n, l, h, nh, False, True, RC.case_id(case))


def attention_block_params():
    out = []
    for c in RC.attention_block_cases():
        _, dtype, dh, nh, (n, l) = c
        form = DM.attn_form(l, l, dh * nh, nh, RC.ES[dtype])
        marks = [pytest.mark.skip(reason="xml_attention_block " + form)] if form.startswith("refused") else []
        out.append(pytest.param(c, id="%s-%s" % (RC.case_id(c), form.replace(" ", "_")), marks=marks))
    return out


@pytest.mark.parametrize("case", attention_block_params())
def test_attention_block_head_sizes_and_counts(ops, case):
    """ops.attention_block at every DH x 1, 2, 3, 4, 8 heads: the QKV GEMM at N = 3 H, the small (l = 30, masks with holes) and
    the large (l = 128) attention kernel reading the fused QKV buffer (row stride 3 H), and below 2 048 rows the unfused
    BertSelfOutput -- GEMM with f32 out + LayerNorm tail -- at hidden sizes 32 ... 1 536, most of them no model width."""
    _, dtype, dh, nh, (n, l) = case
    h = dh * nh
    assert not DM.gemm_ln_fused(n * l, h, h, RC.ES[dtype])
    run_attention_block(ops, dtype, n, l, h, nh, l <= DM.ATTN_SMALL_MAX_L, False, RC.case_id(case))


# ---- K6 -------------------------------------------------------------------------------------------------------------------
_K6 = {}


def k6_data(dtype, hidden, nq, nv, lpad):
    """Operands and float64 references of one K6 shape, kept while consecutive cases ask for the same key:
    q / c: two modalities' unit rows on the bf16 grid in the kernel's dtype (f16: scaled by 2^14, the library's f16 form);
    masks / want per mask kind: ragged (binary prefixes; video 2 of modality 0 has no valid clip), ones, soft (1 / 0.5 / 0);
    kterm: K 2^-24 |q| max_l |c_l| per (query, video)."""
    key = (dtype, hidden, nq, nv, lpad)
    if key in _K6:
        return _K6[key]
    _K6.clear()
    td = TDT[dtype]
    g = torch.Generator(device=DEV).manual_seed(hidden * 7 + nq + nv * 3 + lpad + RC.ES[dtype])

    def unit(*shape):
        x = torch.nn.functional.normalize(torch.randn(*shape, hidden, device=DEV, generator=g), dim=-1).to(torch.bfloat16).float()
        if dtype == "f16":          # exact in f16 but for values below its normal range, which become zeros on both sides
            t = (x * F16_SCALE).to(td)
            t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
            return t.contiguous(), t.double() / F16_SCALE
        t = x.to(td).contiguous()
        return t, t.double()

    qs, cs = [unit(nq) for _ in range(2)], [unit(nv, lpad) for _ in range(2)]
    pos = torch.arange(lpad, device=DEV)[None]
    ragged = []
    for m in range(2):
        lens = torch.randint(1, lpad + 1, (nv,), device=DEV, generator=g)
        lens[0] = lpad
        if m == 0 and nv >= 3:
            lens[2] = 0
        ragged.append((pos < lens[:, None]).float().contiguous())
    masks = dict(ragged=ragged, ones=[torch.ones_like(m) for m in ragged],
                 soft=[(m * 0.5 + 0.5 * (m > 0) * (pos % 2 == 0)).contiguous() for m in ragged])
    want = {kind: [] for kind in masks}
    kterm = []
    for m in range(2):
        q64, c64 = qs[m][1], cs[m][1]
        s = (q64 @ c64.view(-1, hidden).t()).view(nq, nv, lpad)
        for kind in masks:
            mk = masks[kind][m].double()[None]
            want[kind].append((s * mk + (1 - mk) * -1e10).amax(-1))
        kterm.append(hidden * U32 * q64.norm(dim=-1)[:, None] * c64.norm(dim=-1).amax(-1)[None])
        del s
    _K6[key] = dict(q=[t for t, _ in qs], c=[t for t, _ in cs], masks=masks, want=want, kterm=kterm)
    return _K6[key]


def k6_want(d, kind, n_mod):
    w = d["want"][kind][0] if n_mod == 1 else (d["want"][kind][0] + d["want"][kind][1]) / 2
    kt = d["kterm"][0] if n_mod == 1 else (d["kterm"][0] + d["kterm"][1]) / 2
    return w, kt + 3 * U32 * w.abs()


def check_k6(got, want, lim, what):
    assert got.shape == want.shape and got.dtype == torch.float32, what
    err = (got.double() - want).abs()
    bad = ~(err <= lim)                              # (a NaN -- an element nobody wrote -- is bad)
    print("WIDTH %s: worst err / bound %.3f" % (what, float((err / lim).nan_to_num(1e30).max())))
    assert not bad.any(), "%s vs float64: %d of %d off, first at %s: got %r want %r bound %.3e" % (
        what, int(bad.sum()), bad.numel(), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(want[bad][0]),
        float(lim[bad][0]))


def nan_out(nq, nv):
    return torch.full((nq, nv), float("nan"), device=DEV)


@params(RC.k6_persist_cases())
def test_k6_persistent_slice_counts(ops, case):
    """q2c_persist.hip in its five product forms: row-major operands (float mask patches, four slots), tiled with a non-binary
    float mask (four slots), tiled NOMASK and BITMASK (five slots), PACKED (four slots).  With two modalities the ring phase
    carries across the segments of a tile, with (520, 300) across the three tiles of a workgroup as well.  Tile images round
    trip (to_rows) at every width."""
    form, dtype, s, (nq, nv), n_mod = case
    hidden, es = RC.k_of(s, dtype), RC.ES[dtype]
    assert DM.q2c_tiled_ok(128, hidden, es) and ops.q2c_tiled_ok(128, hidden, TDT[dtype])
    d = k6_data(dtype, hidden, nq, nv, 128)
    qs, cs = d["q"][:n_mod], d["c"][:n_mod]
    kind = {"rowmajor": "ragged", "tiled_float": "soft", "nomask": "ones", "bitmask": "ragged", "packed": "ragged"}[form]
    masks = d["masks"][kind][:n_mod]
    want, lim = k6_want(d, kind, n_mod)
    what = RC.case_id(case)
    if form == "rowmajor":
        assert DM.q2c_fused_forms(n_mod, 128, hidden, es) == ["persist"]
        check_k6(ops.q2c_scores_fused(qs, cs, masks, out=nan_out(nq, nv)), want, lim, what)
        if n_mod == 1:
            assert DM.q2c_form(128, hidden, es) == "persist"
            check_k6(ops.q2c_scores(qs[0], cs[0], masks[0], out=nan_out(nq, nv)), want, lim, what + " (q2c_scores)")
        return
    if form == "packed":
        plan = ops.PackPlan(masks)
        tiles = [ops.pack_q2c_corpus(c, m, plan) for c, m in zip(cs, masks)]
        in_map = torch.zeros(nv * 128, dtype=torch.bool, device=DEV)
        in_map[plan.row_map[plan.row_map >= 0].long()] = True
        for t, c in zip(tiles, cs):
            assert t.plan is plan and t.mask_bits is not None
            assert torch.equal(t.to_rows().view(-1, hidden), c.view(-1, hidden) * in_map[:, None].to(c.dtype)), what + ": to_rows"
    else:
        tiles = [ops.pack_q2c_corpus(c, m) for c, m in zip(cs, masks)]
        for t, c in zip(tiles, cs):
            assert isinstance(t, ops.TiledRows) and t.plan is None
            assert t.all_valid == (form == "nomask") and (t.mask_bits is not None) == (form == "bitmask")
            assert torch.equal(t.to_rows(), c), what + ": to_rows"
    check_k6(ops.q2c_scores_fused(qs, tiles, masks, out=nan_out(nq, nv)), want, lim, what)


def run_k6_two_passes(ops, dtype, hidden, nq, nv, lpad, forms, what):
    """xml_q2c_scores without and then with `combine` (the second modality averaged into the first one's scores), and the
    fused entry on the same operands."""
    es = RC.ES[dtype]
    d = k6_data(dtype, hidden, nq, nv, lpad)
    masks = d["masks"]["ragged"]
    assert [DM.q2c_form(lpad, hidden, es, combine=c) for c in (False, True)] == forms
    w0, lim0 = k6_want(d, "ragged", 1)
    out = ops.q2c_scores(d["q"][0], d["c"][0], masks[0], out=nan_out(nq, nv))
    check_k6(out, w0, lim0, what + " pass 0 (%s)" % forms[0])
    w2, lim2 = k6_want(d, "ragged", 2)
    out2 = ops.q2c_scores(d["q"][1], d["c"][1], masks[1], out=out.clone(), combine=True)
    check_k6(out2, w2, lim2, what + " combine (%s)" % forms[1])
    fused = ops.q2c_scores_fused(d["q"], d["c"], masks, out=nan_out(nq, nv))
    check_k6(fused, w2, lim2, what + " fused (%s)" % "+".join(DM.q2c_fused_forms(2, lpad, hidden, es)))


@params(RC.k6_ring_cases())
def test_k6_ring_slice_counts(ops, case):
    """q2c_ring.hip (DMA units five ahead of the MFMA phase): clip paddings 16 / 48 / 112 at 2 .. 14 slices, and lpad = 128
    where the persistent kernel does not apply -- the `combine` pass at every width, both passes below six slices."""
    _, dtype, lpad, s = case
    hidden = RC.k_of(s, dtype)
    nq, nv = RC.K6_RING_SHAPE
    first = "persist" if lpad == 128 and s * DM.SLICE_BYTES >= DM.K6_PERSIST_MIN_KB else "ring"
    run_k6_two_passes(ops, dtype, hidden, nq, nv, lpad, [first, "ring"], RC.case_id(case))


@params(RC.k6_staged_cases())
def test_k6_register_staged_widths(ops, case):
    """q2c_scores_kernel<float> / <bf16_t> (register-staged, hidden * sizeof(T) % 128 != 0): widths with a partial last
    128-byte step, below one step and above two, with and without `combine`."""
    _, dtype, lpad, hidden = case
    nq, nv = RC.K6_STAGED_SHAPE
    assert (hidden * RC.ES[dtype]) % 128 != 0
    run_k6_two_passes(ops, dtype, hidden, nq, nv, lpad, ["staged", "staged"], RC.case_id(case))


@params(RC.l2n_cases())
def test_normalise_and_tile_passes_at_the_width_limit(ops, case):
    """ops.l2norm_rows and ops.q2c_tile_rows_l2norm at d / vec = 32 * L2N_MAXJ chunks per row (every lane holds its eight
    16-byte chunks) and 8 elements beyond, where l2norm_rows takes its scalar kernel and the fused tile pass refuses."""
    _, dtype, d = case
    td, es = TDT[dtype], RC.ES[dtype]
    at_limit = DM.l2n_vec_ok(d, es)
    assert at_limit == (d == RC.L2N_WIDTHS[dtype][0]) and DM.tile_rows_l2norm_ok(d, es) == at_limit
    c = NR.l2norm_case("gaussian", 64, d, td)
    x = c["x"].to(DEV).to(td).contiguous()
    got = ops.l2norm_rows(x)
    if td == torch.float32:
        NR.check_f32("l2norm_rows", RC.case_id(case), got, c["W"], c["R"], C_ROWWISE)
    else:
        NR.check_bf16_rounding("l2norm_rows", RC.case_id(case), got, c["W"], c["R"], C_ROWWISE, strict=True)
    tiled = ops.q2c_tile_rows_l2norm(x)
    g = torch.Generator(device=DEV).manual_seed(d)
    feat = (torch.randn(3, 128, d, device=DEV, generator=g) * 3).to(td)
    packed = ops.pack_q2c_corpus(feat, None, None, normalize=True)
    if at_limit:
        assert torch.equal(tiled.to_rows(), got)                    # the fused pass: bitwise l2norm_rows, then the tiling
        assert isinstance(packed, ops.TiledRows) and torch.equal(packed.to_rows(), ops.l2norm_rows(feat))
    else:
        assert tiled is None                                        # refused: the callers normalise first
        assert not DM.q2c_tiled_ok(128, d, es) and isinstance(packed, torch.Tensor) and torch.equal(packed, ops.l2norm_rows(feat))


# ---- attention ---------------------------------------------------------------------------------------------------------------
def attention_params(dtypes):
    out = []
    for c in RC.attention_cases(dtypes):
        _, dtype, dh, nh, (n, lq, lk) = c
        form = DM.attn_form(lq, lk, dh * nh, nh, RC.ES[dtype])
        marks = [pytest.mark.skip(reason="xml_attention_core " + form)] if form.startswith("refused") else []
        out.append(pytest.param(c, id="%s-%s" % (RC.case_id(c), form.replace(" ", "_")), marks=marks))
    return out


def core_case(n, lq, lk, h, nh, td, seed):
    """NR.core_case for lq != lk: logits of sd ~2, key masks with holes (sequence 0 full, sequence 1 one key); W exact, S with
    P rounded to bf16 and the context rounded once, R the float32 computation."""
    from oracle import f64
    from oracle import xml_oracle as O
    g = torch.Generator().manual_seed(seed)
    dh, s = h // nh, math.sqrt(2.0)
    q = NR.grid(s * torch.randn(n, lq, h, generator=g), td)
    k = NR.grid(s * torch.randn(n, lk, h, generator=g), td)
    v = NR.grid(torch.randn(n, lk, h, generator=g), td)
    mask = NR.hole_masks(n, lk, seed)
    W, _ = f64.attention_core(q, k, v, None, mask, nh)
    S, _ = f64.attention_core(q, k, v, None, mask, nh, f64.bf16_round)
    sp = lambda t, l: t.view(n, l, nh, dh).permute(0, 2, 1, 3)      # noqa: E731
    sc = torch.matmul(sp(q, lq), sp(k, lk).transpose(-1, -2)) / math.sqrt(dh) + (1 - mask[:, None, None, :]) * O.ATT_NEG
    R = torch.matmul(torch.softmax(sc, dim=-1), sp(v, lk)).permute(0, 2, 1, 3).contiguous().view(n, lq, h)
    return dict(q=q, k=k, v=v, mask=mask, W=W, S=f64.bf16_round(S), R=R)


@pytest.mark.parametrize("case", attention_params(RC.GEMM_DTYPES))
def test_attention_core_head_sizes_and_counts(ops, case):
    """ops.attention_core, small kernel (four (sequence, head) units per workgroup: 5 / 6 sequences x 1, 2, 3, 4, 8 heads leave
    every remainder) and large kernel, at every DH; the checkers of test_attention_core_values."""
    _, dtype, dh, nh, (n, lq, lk) = case
    td, h = TDT[dtype], dh * nh
    c = core_case(n, lq, lk, h, nh, td, seed=dh + nh + lq)
    dev = lambda t, d=None: (t.to(DEV) if d is None else t.to(DEV).to(d)).contiguous()      # noqa: E731
    got = ops.attention_core(dev(c["q"], td), dev(c["k"], td), dev(c["v"], td), None, dev(c["mask"]), nh)
    if td == torch.float32:
        NR.check_f32("attention_core", RC.case_id(case), got, c["W"], c["R"], C_ATTENTION)
    else:
        NR.check_bf16_chain("attention_core", RC.case_id(case), got, c["W"], c["S"], M_CHAIN_BF16, ref=c["R"])


def attention_train_params():
    out = []
    for c in RC.attention_cases(("bf16",)):
        _, _, dh, nh, (n, lq, lk) = c
        ok = DM.attn_train_ok(lq, lk, dh * nh, nh)
        marks = [] if ok else [pytest.mark.skip(reason="xml_attention_train_supported refuses")]
        out.append(pytest.param(c, id=RC.case_id(c) + ("" if ok else "-refused"), marks=marks))
    return out


@pytest.mark.parametrize("case", attention_train_params())
def test_attention_train_head_sizes_and_counts(case):
    """AttentionCoreFn (fused training kernels, bf16), forward and backward, at every DH and head count; the cases, references
    and checks of test_attention_fns_bf16."""
    from test_gpu_train_bf16 import compare, run_node
    from tvretrieval_amd import train_ops as TO
    from tvretrieval_amd.autograd import AttentionCoreFn
    _, _, dh, nh, (n, lq, lk) = case
    tc = TC.attention_case(n, lq, lk, dh * nh, nh, "core", True)
    assert TO.attention_train_supported(lq, lk, dh * nh, nh, torch.bfloat16)
    cfg = tc.cfg
    qm = None if cfg["q_mask"] is None else cfg["q_mask"].to(DEV)
    km = cfg["k_mask"].to(DEV)
    outs, grads = run_node(tc, lambda q, k, v: ((AttentionCoreFn.apply(q, k, v, qm, km, nh),), (0, 1, 2)))
    keep = None if cfg["q_mask"] is None else (cfg["q_mask"] > 0)[:, :, None]
    compare(tc, outs, grads, keep_out=keep)
