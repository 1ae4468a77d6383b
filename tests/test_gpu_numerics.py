"""GPU kernels on TRAINED-MODEL operand regimes against float64 (oracle/f64.py): peaked softmaxes, outlier channels,
post-ReLU unit rows, LayerNorm rows with a large mean / tiny / zero variance, near-duplicate clips, masks with holes.
Operand generators, cases and assertion helpers: tests/numerics_regimes.py (its docstring derives the bf16 limits:
half an ulp, the bias bound).  The margins `c` (kernel error over the float32 reference's error, both against float64) and
the bf16 chain margins cite the table of measured ratios in profiles/numerics_margins.md.
Every test prints one `NUMERICS kernel regime storage: kernel_err ref_err ratio` line per case (pytest -s)."""
import pytest
import torch

import numerics_regimes as NR
from test_gpu_kernels import DEV, dev, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
# margins over the float32 reference's own error (profiles/numerics_margins.md, one row per kernel)
C_ROWWISE = 2         # add_layernorm, l2norm_rows, l2norm_rows_eps: one pass over a row
C_GEMM = 2            # linear (all epilogues) and its split-f16 form: the factor test_linear_f16s_vs_float64 uses
C_CHAIN = 8           # K1+K2 (worst ratio 6.41), K6 (5.95), cross attention, ConvSE, re-score: summation order differs from ATen's
C_ATTENTION = 4       # BertAttention block: worst ratio 1.72 -> 2, doubled once (the denominator is ATen on the host CPU)
C_POOL = 2            # modular pooling: worst ratio 0.91
M_CHAIN_BF16 = 4      # bf16 chains: max error over the staged float64 reference's distance from the exact value


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", sorted(NR.ROW_REGIMES))
def test_add_layernorm_regimes(ops, dtype, regime):
    """LN(a + b) per row regime; d = 768.  `constant` rows: exactly beta in float64, finite in the kernel."""
    case = NR.layernorm_case(regime, 64, 768, dtype)
    got = ops.add_layernorm(dev(case["a"]), dev(case["b"], dtype), dev(case["g"]), dev(case["beta"]), out_dtype=dtype)
    if regime == "constant":
        # float64 gives exactly beta, and so does ATen here -- by construction: the constants lie on the bf16 grid, so its
        # f32 row sum is exact.  A kernel whose mean is off by one f32 rounding (sum * (1/d)) leaves x - mean = |x| 2^-24,
        # which rstd = eps^-1/2 = 316 amplifies: the issue asks for a finite output; the derived bound is FLOOR_ULPS such
        # roundings (measured 9.96e-4 of max|beta|, profiles/numerics_margins.md), plus half a bf16 ulp for bf16 storage.
        NR.check_finite("add_layernorm constant", got, case["R"])
        x = (case["a"].double() + case["b"].double()).abs()
        lim = NR.FLOOR_ULPS * 2 * NR.F32_ULP * x * 1e-5 ** -0.5 * case["g"].double().abs()
        if dtype == BF16:
            lim = lim + 0.5 * NR.bf16_ulp(case["W"])
        assert bool(((got.cpu().double() - case["W"]).abs() <= lim).all())
    elif dtype == F32:
        NR.check_f32("add_layernorm", regime, got, case["W"], case["R"], C_ROWWISE)
    else:
        NR.check_bf16_rounding("add_layernorm", regime, got, case["W"], case["R"], C_ROWWISE,
                               strict=regime in NR.BF16_STRICT["layernorm"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", sorted(NR.ROW_REGIMES))
def test_l2norm_rows_regimes(ops, dtype, regime):
    case = NR.l2norm_case(regime, 64, 768, dtype)
    got = ops.l2norm_rows(dev(case["x"], dtype))
    if dtype == F32:
        NR.check_f32("l2norm_rows", regime, got, case["W"], case["R"], C_ROWWISE)
        NR.check_f32("l2norm_rows_eps", regime, ops.l2norm_rows_eps(dev(case["x"])), case["W_eps"], case["R_eps"], C_ROWWISE)
    else:
        NR.check_bf16_rounding("l2norm_rows", regime, got, case["W"], case["R"], C_ROWWISE,
                               strict=regime in NR.BF16_STRICT["l2norm"])


@pytest.mark.parametrize("dtype", [F32, BF16, "f16s"])
@pytest.mark.parametrize("regime", sorted(NR.ROW_REGIMES))
@pytest.mark.parametrize("shape", [(300, 256, 768), (520, 768, 3072)])
def test_linear_regimes(ops, dtype, regime, shape):
    """y = x W^T + b, plain / ReLU / addend, errors in units of |x||w| + |b| + |addend| per output."""
    m, n, k = shape
    store = F32 if dtype == "f16s" else dtype
    for relu, addend in ((False, False), (True, False), (False, True)):
        if addend and dtype == "f16s":
            continue                                                     # the split-f16 projection has no addend epilogue
        case = NR.linear_case(regime, m, n, k, store, relu, addend)
        w = ops.pack_weights_f16s(dev(case["w"])) if dtype == "f16s" else dev(case["w"], store)
        got = ops.linear(dev(case["x"], store), w, dev(case["b"]), relu=relu,
                         addend=dev(case["addend"], store) if addend else None)
        name = "linear%s%s" % ("+relu" if relu else "", "+addend" if addend else "")
        if dtype == BF16:
            NR.check_bf16_rounding(name, regime, got, case["W"], case["R"], C_GEMM, case["scale"],
                                   strict=regime in NR.BF16_STRICT["linear"])
        else:
            NR.check_f32(name, regime, got, case["W"], case["R"], C_GEMM, case["scale"], storage=str(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", ["post_relu_unit", "outlier_channels", "offset1e3", "mixed"])
@pytest.mark.parametrize("shape", [(8, 128, 3072, 768), (17, 128, 768, 256), (40, 30, 768, 768)])
def test_k1k2_regimes(ops, dtype, regime, shape):
    """K1+K2 on the rows the input projections really see; 1 024 / 1 200 rows run GEMM + LayerNorm launches, 2 176 rows the
    LayerNorm-epilogue GEMM (its gate: 2 048 rows).  Staged reference: bf16 at the LayerNorm'd GEMM operand, and at the
    pre-LayerNorm value for the epilogue form."""
    n, l, d_in, h = shape
    case = NR.k1k2_case(regime, n, l, d_in, h, dtype, pre_ln=n * l >= 2048)
    sd, pe = case["sd"], case["pe"]
    got = ops.linear_ln_relu_pos(dev(case["x"]), dev(sd["LayerNorm.weight"]), dev(sd["LayerNorm.bias"]),
                                 dev(sd["net.1.weight"], dtype), dev(sd["net.1.bias"]),
                                 dev(pe["position_embeddings.weight"], dtype), dev(pe["LayerNorm.weight"]),
                                 dev(pe["LayerNorm.bias"]))
    if dtype == F32:
        NR.check_f32("linear_ln_relu_pos", regime, got, case["W"], case["R"], C_CHAIN)
    else:
        NR.check_bf16_chain("linear_ln_relu_pos", regime, got, case["W"], case["S"], M_CHAIN_BF16, ref=case["R"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("logit_std", [2.0, 6.0, 12.0])
@pytest.mark.parametrize("shape", [(4, 128, 256, 4), (17, 128, 768, 4), (6, 30, 256, 4)])
def test_attention_block_peaked(ops, dtype, holes, logit_std, shape):
    """BertAttention with peaked attention (logit sd 2 / 6 / 12), prefix masks with a length-1 and a full sequence, and masks
    with holes (the padded entry point takes a mask tensor).  Every row has a valid key, so every row goes to float64.
    Staged reference: bf16 at Q/K/V, P, the context, and the pre-LayerNorm value for the LayerNorm-epilogue GEMM."""
    n, l, h, nh = shape
    case = NR.attention_case(logit_std, n, l, h, nh, dtype, holes, pre_ln=n * l >= 2048)
    print("peaked(%g): logit sd %.2f, mean max probability %.3f" % (logit_std, case["logit_std"], case["mean_max_prob"]))
    assert 0.7 * logit_std < case["logit_std"] < 1.4 * logit_std
    sd = case["sd"]
    wqkv = torch.cat([sd["self.%s.weight" % k] for k in ("query", "key", "value")])
    bqkv = torch.cat([sd["self.%s.bias" % k] for k in ("query", "key", "value")])
    got = ops.attention_block(dev(case["x"], dtype), dev(case["mask"]), dev(wqkv, dtype), dev(bqkv),
                              dev(sd["output.dense.weight"], dtype), dev(sd["output.dense.bias"]),
                              dev(sd["output.LayerNorm.weight"]), dev(sd["output.LayerNorm.bias"]), nh)
    regime = "peaked%g%s" % (logit_std, "+holes" if holes else "")
    if dtype == F32:
        NR.check_f32("attention_block", regime, got, case["W"], case["R"], C_ATTENTION)
    else:
        NR.check_bf16_chain("attention_block", regime, got, case["W"], case["S"], M_CHAIN_BF16, ref=case["R"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("logit_std", [2.0, 6.0, 12.0])
def test_modular_pool_peaked(ops, dtype, holes, logit_std):
    """K5 with a peaked pooling softmax; bf16 storage rounds once (the pooled row), statistics in f32."""
    case = NR.pool_case(logit_std, 33, 30, 256, 2, dtype, holes)
    got = ops.modular_pool(dev(case["enc"], dtype), dev(case["mask"]), dev(case["wm"]))
    regime = "peaked%g%s" % (logit_std, "+holes" if holes else "")
    if dtype == F32:
        NR.check_f32("modular_pool", regime, got, case["W"], case["R"], C_POOL)
    else:
        # bias bound at spread 2 only: a peaked pool returns (nearly) ONE token row, which already lies on the bf16 grid, so
        # the value under the rounding sits a hair inside a grid point and the correctly rounded reference is biased too
        NR.check_bf16_rounding("modular_pool", regime, got, case["W"], case["R"], C_POOL, strict=logit_std == 2.0, cap=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("kernel,shape", [("q2c_scores", (40, 9, 48, 256)), ("q2c_scores_fused", (40, 9, 48, 256)),
                                          ("q2c_scores_fused", (300, 11, 128, 768)), ("tiled", (300, 11, 128, 768))])
def test_q2c_near_duplicates(ops, dtype, holes, kernel, shape):
    """K6 (generic, fused row-major, fused on the tiled corpus image) on near-duplicate clips: cosines 0.9 ... 1 - 5e-9.
    Scores f32-grade against float64 (the output is f32 for both storage types; accumulation is f32); the duplicate video
    scores exactly like its original.  At lpad = 128 the row-major fused entry and the tiled corpus image run the same
    persistent kernel with a different source addressing (test_q2c_tiled_equals_row_major: bitwise equal scores), so their
    figures coincide; the (40, 9, 48, 256) shape takes the generic fused kernel."""
    nq, nv, l, h = shape
    case = NR.q2c_case(nq, nv, l, h, dtype, holes)
    q, c, m = dev(case["q"], dtype), dev(case["c"], dtype), dev(case["mask"])
    if kernel == "q2c_scores":
        got = ops.q2c_scores(q, c, m)
    elif kernel == "q2c_scores_fused":
        got = ops.q2c_scores_fused([q], [c], [m], out=torch.full((nq, nv), float("nan"), device=DEV))
    else:
        assert ops.q2c_tiled_ok(l, h, dtype)
        got = ops.q2c_scores_fused([q], [ops.pack_q2c_corpus(c, m)], [m], out=torch.full((nq, nv), float("nan"), device=DEV))
    regime = "near_duplicate%s" % ("+holes" if holes else "")
    # (the expected value IS float64's best clip score, so the value check is the "kernel's maximum = best clip" check)
    NR.check_f32(kernel, regime, got, case["W"], case["R"], C_CHAIN, scale=1.0, storage=str(dtype))
    assert torch.equal(got[:, -1], got[:, 0]), "exact duplicate videos must score exactly alike (K8's tie rules)"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("logit_std", [2.0, 6.0, 12.0])
def test_attention_core_probabilities(ops, dtype, holes, logit_std):
    """attention_core with V = identity per head: the context is the kernel's probability matrix.  Rows sum to 1, masked keys
    are exactly 0 where the reference's are, the arg-max key agrees with float64 wherever float64 is decided, values
    f32-grade (bf16 storage: P is rounded once on its way to the P.V MFMA -> half a bf16 ulp of <= 1 on top)."""
    n, l, h, nh = 5, 48, 256, 4
    case = NR.core_case(logit_std, n, l, h, nh, dtype, holes, identity_v=True)
    got = ops.attention_core(dev(case["q"], dtype), dev(case["k"], dtype), dev(case["v"], dtype), None, dev(case["mask"]), nh)
    P = got.float().cpu().view(n, l, nh, h // nh)[..., :l].permute(0, 2, 1, 3)
    regime = "peaked%g%s" % (logit_std, "+holes" if holes else "")
    if dtype == F32:
        kerr, ref_err = NR.check_f32("attention_core P", regime, P, case["Pw"], case["Pr"], C_ATTENTION, scale=1.0)
        allow = C_ATTENTION * ref_err + NR.FLOOR_ULPS * 2 * NR.F32_ULP
    else:
        _, ref_err, _ = NR.f32_allowance(case["Pw"], case["Pr"], C_ATTENTION, 1.0)
        allow = C_ATTENTION * ref_err + NR.FLOOR_ULPS * 2 * NR.F32_ULP + 2.0 ** -9
        NR.check_finite("attention_core P", P, case["Pr"])
        NR.report("attention_core P", regime, "bf16", float((P.double() - case["Pw"]).abs().max()), 2.0 ** -9)
        assert float((P.double() - case["Pw"]).abs().max()) <= allow
    NR.check_prob_rows("attention_core P", regime, P, case["Pw"], allow)
    assert bool((P[case["Pr"] == 0] == 0).all()), "masked keys must get exactly 0 where the reference gives 0"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logit_std", [2.0, 12.0])
def test_attention_core_values(ops, dtype, logit_std):
    n, l, h, nh = 6, 128, 256, 4
    case = NR.core_case(logit_std, n, l, h, nh, dtype, holes=True, identity_v=False)
    got = ops.attention_core(dev(case["q"], dtype), dev(case["k"], dtype), dev(case["v"], dtype), None, dev(case["mask"]), nh)
    if dtype == F32:
        NR.check_f32("attention_core", "peaked%g+holes" % logit_std, got, case["W"], case["R"], C_ATTENTION)
    else:      # staged: P rounded to bf16, the context rounded once
        NR.check_bf16_chain("attention_core", "peaked%g+holes" % logit_std, got, case["W"], case["S"], M_CHAIN_BF16, ref=case["R"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logit_std", [2.0, 12.0])
@pytest.mark.parametrize("shape", [(4, 33, 20, 128, 4), (5, 128, 128, 768, 4)])
def test_cross_attention_peaked(ops, dtype, logit_std, shape):
    """Rows with a valid query and a valid key go to float64; padded query rows and the sequence whose keys are all masked
    keep the float32 oracle as their expected value (the -10000 mask absorbs ~1e-3 of the score in f32: the reference's
    behaviour), with a limit derived from that absorption."""
    n, lq, lk, h, nh = shape
    case = NR.cross_case(logit_std, n, lq, lk, h, nh, dtype)
    att = case["att"]
    wkv = torch.cat([att["key.weight"], att["value.weight"]], 0)
    bkv = torch.cat([att["key.bias"], att["value.bias"]], 0)
    got = ops.cross_attention(dev(case["main"], dtype), dev(case["mm"]), dev(case["side"], dtype), dev(case["sm"]),
                              dev(att["query.weight"], dtype), dev(att["query.bias"]), dev(wkv, dtype), dev(bkv),
                              dev(case["ln_g"]), dev(case["ln_b"]), nh).float().cpu()
    rows = case["f64_rows"]
    assert 0.2 < float(rows.float().mean()) < 0.8
    regime = "peaked%g+holes" % logit_std
    if dtype == F32:
        NR.check_f32("cross_attention", regime, got[rows], case["W"][rows], case["R"][rows], C_CHAIN)
    else:
        NR.check_bf16_chain("cross_attention", regime, got[rows], case["W"][rows], case["S"][rows], M_CHAIN_BF16,
                            ref=case["R"][rows])
    # the other rows against the float32 oracle.  Their limit is derived from the number format: s - 10000 is rounded to
    # f32's spacing at 1e4, 2^-10, so a last-bit difference in s (summation order) moves a logit by 2^-10, every
    # probability by a relative 2^-10, and the output by at most 2 * 2^-10 of its scale.  bf16 storage adds the spread of the
    # bf16 staging (Q/K/V, P, context), measured on the same rows between the staged and the unstaged float64 forms,
    # with the chain margin.  (test_cross_attention's 2e-4 / 8e-2 were sized for flat softmaxes.)
    other = ~rows
    lim = 2 * 2.0 ** -10 * float(case["R"][other].abs().max())
    if dtype == BF16:
        lim += M_CHAIN_BF16 * float((case["S"][other] - case["W"][other]).abs().max())
    err = float((got[other].double() - case["R"][other].double()).abs().max())
    print("NUMERICS cross_attention padded %s %s: err vs f32 oracle %.3e limit %.3e" % (regime, dtype, err, lim))
    assert bool(torch.isfinite(got).all()) and err <= lim


def test_pack_plan_refuses_masks_with_holes(ops):
    """the packed (varlen) entry points are prefix-only: xml_pack_plan reports rows = -1 for a mask with holes, and the
    packed kernels are never fed one."""
    m = NR.hole_masks(9, 30)
    assert not NR.is_prefix(m) and ops.pack_plan(dev(m))[2] == -1
    assert ops.pack_plan(dev(NR.prefix_masks(9, 30)))[2] == int(NR.prefix_masks(9, 30).sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(40, 30, 768, 256), (80, 30, 768, 768)])
def test_varlen_query_path_regimes(ops, dtype, shape):
    """the packed query encoder: K1+K2 on packed tokens (outlier-channel rows: BERT features), BertAttention with peaked
    weights on the packed rows, modular pooling with a peaked vector -- each against float64 on the valid tokens
    (prefix masks with a length-1 and a full-length sequence; 40 x 30 under, 80 x 30 over the 2 048-row gate when full)."""
    n, l, d_in, h = shape
    mask = NR.prefix_masks(n, l, 3)
    mask[2:] = 1 if n == 80 else mask[2:]                       # 2 341 packed rows: over the LayerNorm-epilogue gate
    cu, src, rows = ops.pack_plan(dev(mask))
    assert rows == int(mask.sum())
    valid = mask.bool()
    case = NR.k1k2_case("outlier_channels", n, l, d_in, h, dtype, pre_ln=rows >= 2048)
    sd, pe = case["sd"], case["pe"]
    got = ops.linear_ln_relu_pos_packed(dev(case["x"]).reshape(n * l, d_in), src, rows, l, dev(sd["LayerNorm.weight"]),
                                        dev(sd["LayerNorm.bias"]), dev(sd["net.1.weight"], dtype), dev(sd["net.1.bias"]),
                                        dev(pe["position_embeddings.weight"], dtype), dev(pe["LayerNorm.weight"]),
                                        dev(pe["LayerNorm.bias"]))
    if dtype == F32:
        NR.check_f32("linear_ln_relu_pos_packed", "outlier_channels", got, case["W"][valid], case["R"][valid], C_CHAIN)
    else:
        NR.check_bf16_chain("linear_ln_relu_pos_packed", "outlier_channels", got, case["W"][valid], case["S"][valid],
                            M_CHAIN_BF16, ref=case["R"][valid])
    for std in (2.0, 12.0):
        ac = NR.attention_case(std, n, l, h, 4, dtype, holes=False, pre_ln=rows >= 2048, seed=3)
        assert torch.equal(ac["mask"][:2], mask[:2])
        amask = ac["mask"] if n != 80 else mask
        if n == 80:                                              # the case's own masks are random prefixes: rebuild on `mask`
            from oracle import f64
            from oracle import xml_oracle as O
            w64 = f64.Weights64(ac["sd"])
            ac["R"] = O.bert_attention(ac["x"], mask.unsqueeze(1), O.Weights(ac["sd"]), 4)
            ac["W"] = f64.bert_attention(ac["x"], mask.unsqueeze(1), w64, 4)
            ac["S"] = f64.bert_attention(ac["x"], mask.unsqueeze(1), w64, 4, f64.bf16_round, rows >= 2048)
        v = amask.bool()
        cu2, src2, rows2 = ops.pack_plan(dev(amask))
        a = ac["sd"]
        wqkv = torch.cat([a["self.%s.weight" % k] for k in ("query", "key", "value")])
        bqkv = torch.cat([a["self.%s.bias" % k] for k in ("query", "key", "value")])
        xp = dev(ac["x"], dtype).reshape(n * l, h)[src2[:rows2].long()].contiguous()
        got = ops.attention_block_varlen(xp, cu2, n, l, dev(wqkv, dtype), dev(bqkv), dev(a["output.dense.weight"], dtype),
                                         dev(a["output.dense.bias"]), dev(a["output.LayerNorm.weight"]),
                                         dev(a["output.LayerNorm.bias"]), 4)
        if dtype == F32:
            NR.check_f32("attention_block_varlen", "peaked%g" % std, got, ac["W"][v], ac["R"][v], C_ATTENTION)
        else:
            NR.check_bf16_chain("attention_block_varlen", "peaked%g" % std, got, ac["W"][v], ac["S"][v], M_CHAIN_BF16,
                                ref=ac["R"][v])
        pc = NR.pool_case(std, n, l, h, 2, dtype, holes=False, seed=3)
        pm = pc["mask"]
        cu3, src3, rows3 = ops.pack_plan(dev(pm))
        ep = dev(pc["enc"], dtype).reshape(n * l, h)[src3[:rows3].long()].contiguous()
        got = ops.modular_pool_varlen(ep, cu3, n, l, dev(pc["wm"]))
        if dtype == F32:
            NR.check_f32("modular_pool_varlen", "peaked%g" % std, got, pc["W"], pc["R"], C_POOL)
        else:
            NR.check_bf16_rounding("modular_pool_varlen", "peaked%g" % std, got, pc["W"], pc["R"], C_POOL, strict=std == 2.0,
                                       cap=False)


@pytest.mark.parametrize("dtype", [F32, BF16, "f16s"])
@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("n_mod,merged", [(2, True), (2, False), (1, False)])
def test_convse_peaked(ops, dtype, softmax, n_mod, merged):
    """K7 with a peaked span softmax (> 0.9 on one clip for most pairs), merged and per-stream, softmax on and off, f32 / bf16
    storage and the split-f16 form.  The outputs are f32 for every storage type (f32 accumulation), so all are held to the
    f32 check.  With softmax: rows sum to 1, masked clips are exactly 0, the arg-max clip agrees with float64."""
    nq, nv, l, h = 12, 9, 48, 128
    store = F32 if dtype == "f16s" else dtype
    case = NR.convse_case(nq, nv, l, h, n_mod, merged, store, softmax)
    peaked = float((case["W"][0].max(-1)[0] > 0.9).double().mean()) if softmax else 1.0
    assert peaked > 0.5
    if dtype == "f16s":
        q = [ops.split_f16_rows(dev(x)) for x in case["q"]]
        f = [ops.split_f16_rows(dev(x)) for x in case["f"]]
    else:
        q, f = [dev(x, dtype) for x in case["q"]], [dev(x, dtype) for x in case["f"]]
    st, ed = ops.convse_rerank(q, f, [dev(case["mask"])] * n_mod, dev(case["pair"]), dev(case["cw"]), l, merged, 5,
                               softmax=softmax)
    valid = case["valid"]
    regime = "peaked%s%s" % ("+merged" if merged else "+streams%d" % n_mod, "" if softmax else "+logits")
    for nm, got, W, R in (("st", st, case["W"][0], case["R"][0]), ("ed", ed, case["W"][1], case["R"][1])):
        got = got.cpu()
        if softmax:
            _, ref_err = NR.check_f32("convse_rerank " + nm, regime, got, W, R, C_CHAIN, scale=1.0, storage=str(dtype))
            assert bool((got[~valid] == 0).all()), "masked clips must be exactly 0"
            NR.check_prob_rows("convse_rerank " + nm, regime, got, W, C_CHAIN * ref_err + NR.FLOOR_ULPS * 2 * NR.F32_ULP)
        else:
            NR.check_f32("convse_rerank " + nm, regime, got[valid], W[valid], R[valid], C_CHAIN, storage=str(dtype))
            assert bool((got[~valid] == R[~valid]).all()), "masked clips carry the reference's fill value"


@pytest.mark.parametrize("dtype", [F32, BF16, "f16s"])
def test_q2c_rescore_near_duplicates(ops, dtype):
    nq, nv, l, h = 40, 9, 48, 256
    store = F32 if dtype == "f16s" else dtype
    case = NR.q2c_case(nq, nv, l, h, store, holes=True)
    g = torch.Generator().manual_seed(4)
    pair = torch.randint(0, nv, (nq, 6), generator=g).int()
    pair[:, 0] = 0
    pair[:, 1] = nv - 1                                      # the duplicate of video 0
    if dtype == "f16s":
        q, c = [ops.split_f16_rows(dev(case["q"]), ops.F16_UNIT_LOG2)], [ops.split_f16_rows(dev(case["c"]), ops.F16_UNIT_LOG2)]
    else:
        q, c = [dev(case["q"], dtype)], [dev(case["c"], dtype)]
    got = ops.q2c_rescore(q, c, [dev(case["mask"])], dev(pair))
    W, R = torch.gather(case["W"], 1, pair.long()), torch.gather(case["R"], 1, pair.long())
    NR.check_f32("q2c_rescore", "near_duplicate+holes", got, W, R, C_CHAIN, scale=1.0, storage=str(dtype))
    assert torch.equal(got[:, 0], got[:, 1]), "exact duplicate videos must score exactly alike"


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_ingest_rows_vs_float64(ops, out_dtype):
    """xml_ingest_rows: f16 store rows -> x / (|x| + eps) per clip in f32 / bf16, zero padding, masks."""
    n, lmax, d = 7, 32, 768
    case = NR.ingest_case(n, lmax, d)
    got, mask = ops.ingest_rows(dev(case["src"]), dev(case["row_start"]), n, lmax, lmax, normalize=True, out_dtype=out_dtype)
    assert torch.equal(mask.cpu(), case["mask"])
    pad = case["mask"] == 0
    assert bool((got.float().cpu()[pad] == 0).all())
    if out_dtype == F32:
        NR.check_f32("ingest_rows", "store_f16", got, case["W"], case["R"], C_ROWWISE)
    else:
        NR.check_bf16_rounding("ingest_rows", "store_f16", got, case["W"], case["R"], C_ROWWISE)
    raw, _ = ops.ingest_rows(dev(case["src"]), dev(case["row_start"]), n, lmax, lmax, normalize=False, out_dtype=F32)
    assert torch.equal(raw.cpu().double(), case["W_raw"]), "without normalisation the f16 values are widened exactly"


# ---- selection kernels: repeated (score, payload) pairs ---------------------------------------------------------------------
def _raw_topk(ops, s, pay, k):
    """xml_topk_rows through the C entry, outputs pre-filled with a sentinel (ops.topk_rows allocates with torch.empty)."""
    lib = ops._lib.load()
    rows, n = s.shape
    vals = torch.full((rows, k), -12345.0, device=DEV)
    idx = torch.full((rows, k), -777, dtype=torch.int32, device=DEV)
    ws = ops._workspace(lib.xml_topk_rows_workspace_bytes(rows, n, k), s.device)
    ops.check(lib.xml_topk_rows(ops._p(s), s.stride(0), ops._p(pay), ops._p(vals), ops._p(idx), rows, n, k, 0.0, ops._p(ws),
                                ws.numel(), ops._stream()), "xml_topk_rows")
    torch.cuda.synchronize()
    return vals.cpu(), idx.cpu()


def _check_selection(s, pay, vals, idx, k):
    assert not bool((idx == -777).any()) and not bool((vals == -12345.0).any()), \
        "%d output slots were never written" % int((idx == -777).sum())
    for r in range(s.shape[0]):
        pairs = sorted(zip((-s[r]).tolist(), pay[r].tolist()))[:k]           # score desc, payload asc: the documented order
        got = sorted(zip((-vals[r]).tolist(), idx[r].tolist()))
        assert got == pairs, "row %d: output multiset differs from the sorted input's first %d" % (r, k)
        assert torch.equal(vals[r].sort(descending=True)[0], torch.topk(s[r], k)[0])


def _duplicate_rows(n, k, seed):
    """rows with repeated (score, payload) pairs: real candidates, groups of identical pairs, and the filler of
    dist.topk_by_owner (-inf, 2^31 - 1) -- more fillers than k minus the real candidates."""
    g = torch.Generator().manual_seed(seed)
    rows = 6
    s = torch.round(torch.randn(rows, n, generator=g) * 4) / 4
    pay = torch.randint(0, 50, (rows, n), generator=g).int()                 # few payloads x few scores: many equal pairs
    n_real = max(k // 3, 1)
    s[2:4, n_real:] = float("-inf")                                            # filler rows: only n_real real candidates
    pay[2:4, n_real:] = 2 ** 31 - 1
    s[4] = 1.5                                                                 # one pair repeated n times
    pay[4] = 7
    s[5] = float("-inf")                                                       # a row of nothing but filler
    pay[5] = 2 ** 31 - 1
    return s, pay


@pytest.mark.parametrize("n,k", [(300, 100), (64, 17), (5000, 256), (2000, 200)])
def test_topk_rows_repeated_composites_fill_every_slot(ops, n, k):
    """xml_topk_rows ranks its <= 256 survivors by counting the entries that sort before each; with repeated (score, payload)
    pairs equal composites must still get distinct ranks (ties broken on the LDS slot), or two entries land on one output
    slot and another is never written."""
    s, pay = _duplicate_rows(n, k, n + k)
    vals, idx = _raw_topk(ops, dev(s), dev(pay), k)
    _check_selection(s, pay, vals, idx, k)


@pytest.mark.parametrize("world,c,k", [(4, 50, 100), (8, 32, 200)])
def test_merge_shard_topk_repeated_composites_fill_every_slot(ops, world, c, k):
    lib = ops._lib.load()
    s, pay = _duplicate_rows(world * c, k, world + c)
    rows = s.shape[0]
    rs = dev(s.view(rows, world, c).permute(1, 0, 2))                          # receive layout [rank][row][c]
    ri = dev(pay.view(rows, world, c).permute(1, 0, 2))
    vals = torch.full((rows, k), -12345.0, device=DEV)
    idx = torch.full((rows, k), -777, dtype=torch.int32, device=DEV)
    ws = ops._workspace(lib.xml_merge_shard_topk_workspace_bytes(world, rows, c), rs.device)
    ops.check(lib.xml_merge_shard_topk(ops._p(rs), ops._p(ri), world, rows, c, k, 0.0, ops._p(vals), ops._p(idx), ops._p(ws),
                                       ws.numel(), ops._stream()), "xml_merge_shard_topk")
    torch.cuda.synchronize()
    _check_selection(s, pay, vals.cpu(), idx.cpu(), k)


def test_moment_topk_massive_score_ties_fill_every_slot(ops):
    """K9 ranks its survivors the same way; its keys hold a unique flat index, so massive SCORE ties must still write every
    slot exactly once (no kernel change: this pins the assumption)."""
    nq, kk, l, n_out = 5, 6, 32, 100
    st = torch.full((nq, kk, l), 0.25, device=DEV)
    ed = torch.full((nq, kk, l), 0.5, device=DEV)
    w = torch.ones(nq, kk, device=DEV)
    scores, flat = ops.moment_topk(st, ed, w, l, 2, 16, n_out)[:2]
    scores, flat = scores.cpu(), flat.cpu()
    assert bool(torch.isfinite(scores).all()) and bool((scores == 0.125).all())
    assert bool((flat >= 0).all()) and bool((flat < kk * l * l).all())
    for r in range(nq):
        assert flat[r].unique().numel() == n_out, "row %d: a slot was written twice or never" % r
