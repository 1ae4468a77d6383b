"""CPU side of tests/test_gpu_numerics.py: the float64 oracle, the operand regimes and the assertion helpers, checked
without a GPU.
* the float64 forms equal the float32 oracle to float32 accuracy on the benign operands of test_gpu_kernels.py;
* each generator achieves the figure it promises;
* the float32 reference is finite in every regime and passes the new checks itself (as f32, and rounded to bf16 by torch),
  the 1 % cap on rounding-boundary elements included;
* the host model of the dropout mask (oracle/f64.py drop_keep) against a scalar restatement; the attention case table
  against the library's list of fused head sizes; the block-wise chain check on an f32-arithmetic model of a correct kernel;
* the staged float64 AUTOGRAD references of the training nodes (oracle/f64.py, tests/train_bf16_cases.py): identity stage ==
  plain float64 autograd bit for bit, staged != exact, one bf16 store stays within half a bf16 ulp of W (<= 2^-8 |W|) plus one f32 rounding;
* sensitivity: deliberately wrong stand-ins are rejected by the check meant for them while the existing `close(...)`
  limits of test_gpu_kernels.py accept them on that suite's operands;
* the case tables of the training loss tail and the optimizer (tests/train_tail_cases.py) meet their own conditions, and CPU
  restatements of six wrong kernels fail the new cases while the cases the suite had before accept them."""
import math

import pytest
import torch
import torch.nn.functional as F

import numerics_regimes as NR
import train_bf16_cases as TC
import train_tail_cases as TT
from oracle import f64
from oracle import xml_oracle as O
from test_gpu_kernels import _att_weights, _ragged_mask, close, rnd

BF16, F32 = torch.bfloat16, torch.float32
LN_REGIMES = sorted(NR.ROW_REGIMES)


def test_float64_forms_equal_the_float32_oracle_on_benign_operands():
    n, l, d_in, h, nh = 3, 24, 96, 128, 4
    x = rnd(n, l, d_in, seed=10)
    sd = {"LayerNorm.weight": 1 + 0.1 * rnd(d_in, seed=11), "LayerNorm.bias": 0.1 * rnd(d_in, seed=12),
          "net.1.weight": rnd(h, d_in, seed=13, scale=d_in ** -0.5), "net.1.bias": 0.1 * rnd(h, seed=14)}
    pe = {"position_embeddings.weight": rnd(l + 3, h, seed=15, scale=0.5), "LayerNorm.weight": 1 + 0.1 * rnd(h, seed=16),
          "LayerNorm.bias": 0.1 * rnd(h, seed=17)}
    want = O.trainable_pos_enc(O.linear_layer(x, O.Weights(sd)), O.Weights(pe))
    got = f64.linear_ln_relu_pos(x, f64.Weights64(sd), f64.Weights64(pe))
    assert got.dtype == torch.float64
    close("K1+K2", got, want, 5e-6)
    close("linear_layer", f64.linear_layer(x, f64.Weights64(sd)), O.linear_layer(x, O.Weights(sd)), 5e-6)
    y = want
    mask = _ragged_mask(n, l, 31)
    sa = _att_weights(h, 40)
    close("bert_attention", f64.bert_attention(y, mask.unsqueeze(1), f64.Weights64(sa), nh),
          O.bert_attention(y, mask.unsqueeze(1), O.Weights(sa), nh), 1e-5)
    att = O.Weights(sa).sub("self")
    close("bert_self_attention", f64.bert_self_attention(y, y, y, mask.unsqueeze(1), f64.Weights64(sa).sub("self"), nh),
          O.bert_self_attention(y, y, y, mask.unsqueeze(1), att, nh), 5e-6)
    close("bert_self_output", f64.bert_self_output(y, x.new_ones(y.shape), f64.Weights64(sa).sub("output")),
          O.bert_self_output(y, x.new_ones(y.shape), O.Weights(sa).sub("output")), 1e-5)
    wm = rnd(2, h, seed=72, scale=h ** -0.5)
    sc = torch.softmax(O.mask_logits(y @ wm.t(), mask.unsqueeze(2)), dim=1)
    close("modular_pool", f64.modular_pool(y, mask, wm)[0], torch.einsum("blm,bld->mbd", sc, y), 5e-6)
    q, c = F.normalize(rnd(7, h, seed=1), dim=-1), F.normalize(rnd(n, l, h, seed=2), dim=-1)
    s = torch.max(O.mask_logits(torch.einsum("md,nld->mln", q, c), mask.t().unsqueeze(0)), dim=1)[0]
    close("q2c", f64.q2c_scores(q, c, mask)[0], s, 1e-6)
    # the staged form differs from the exact one by bf16 roundings, not by more
    st = f64.bert_attention(y, mask.unsqueeze(1), f64.Weights64(sa), nh, f64.bf16_round, True)
    err = float((st - f64.bert_attention(y, mask.unsqueeze(1), f64.Weights64(sa), nh)).abs().max())
    assert 1e-4 < err < 8e-2, err


def test_generators_achieve_their_figures():
    x = NR.outlier_channels(64, 768)
    big = (x.abs().mean(0) > 4).sum()
    assert int(big) == 4 and 20 < float(x.abs().mean(0).max()) < 30
    for d in (3072, 768):
        x = NR.post_relu_unit(64, d)
        assert bool((x >= 0).all()) and float((x.norm(dim=-1) - 1).abs().max()) < 1e-6
        assert 0.5 < float((x.mean(-1) / x.std(-1)).mean()) < 1.5          # mean comparable to the standard deviation
        assert abs(float(x.mean()) - 0.3989 / math.sqrt(d / 2)) < 0.1 * float(x.mean())
    for mean, nm in ((10.0, "offset10"), (1e3, "offset1e3")):
        x = NR.ROW_REGIMES[nm](64, 768)
        assert abs(float(x.mean()) / mean - 1) < 0.01 and abs(float(x.var(-1).mean()) - 1) < 0.1
    assert float(NR.tiny(64, 768).var(-1).max()) < 2e-8
    c = NR.constant(64, 768)
    assert bool((c == c[:, :1]).all()) and float(c.double().var(-1).max()) == 0.0 and c.unique().numel() > 16
    oh = NR.one_hot(64, 768)
    assert bool((oh.sum(-1) == 1).all()) and bool(((oh == 0) | (oh == 1)).all())
    w = NR.layernorm_case("one_hot", 16, 768, F32)["W"]
    assert float(w.abs().max()) > 0.7 * math.sqrt(768)
    m = NR.mixed(64, 768)
    norms = m.norm(dim=-1)
    assert float(norms.max() / norms.min()) > 1e6                           # neighbouring rows 7 decades apart
    for target, lo, hi in ((2.0, 0.05, 0.45), (6.0, 0.4, 0.95), (12.0, 0.8, 1.0)):
        case = NR.attention_case(target, 4, 64, 128, 4, F32, holes=False, pre_ln=False)
        print("peaked(%g): logit sd %.2f mean max prob %.3f" % (target, case["logit_std"], case["mean_max_prob"]))
        assert 0.7 * target < case["logit_std"] < 1.4 * target
        assert lo < case["mean_max_prob"] < hi
        pc = NR.pool_case(target, 6, 30, 128, 2, F32, holes=True)
        assert lo < pc["mean_max_prob"] <= 1.0
    q, c = NR.near_duplicate_clips(8, 9, 32, 256)
    cos = torch.einsum("vld,vd->vl", c.double(), q[torch.arange(9) % 8].double())
    assert float(cos.min()) > 0.88 and float(cos.max()) > 1 - 1e-7
    assert torch.equal(c[-1], c[0]) and bool(torch.signbit(c[:, ::4, 0]).all()) and bool((c[:, ::4, 0] == 0).all())
    assert NR.is_prefix(NR.prefix_masks(9, 30)) and not NR.is_prefix(NR.hole_masks(9, 30))
    pm, hm = NR.prefix_masks(9, 30), NR.hole_masks(9, 30)
    assert pm[0].sum() == 30 and pm[1].sum() == 1 and hm[0].sum() == 30 and hm[1].sum() == 1 and bool((hm[:, 0] == 1).all())


@pytest.mark.parametrize("regime", LN_REGIMES)
def test_reference_passes_the_layernorm_and_l2norm_checks(regime):
    """G := the float32 reference (c = 1 holds trivially) and G := torch's bf16 rounding of it: finite, half an ulp,
    unbiased, under the boundary cap -- the generators are usable for the kernel checks."""
    for dtype in (F32, BF16):
        case = NR.layernorm_case(regime, 64, 768, dtype)
        assert bool(torch.isfinite(case["R"]).all()) and bool(torch.isfinite(case["W"]).all())
        if regime == "constant":
            assert torch.equal(case["W"], case["beta"].double().expand_as(case["W"]))
        NR.check_f32("ref layernorm", regime, case["R"], case["W"], case["R"], 1)
        NR.check_bf16_rounding("ref layernorm", regime, case["R"].to(BF16), case["W"], case["R"], 2,
                               strict=regime in NR.BF16_STRICT["layernorm"])
        case = NR.l2norm_case(regime, 64, 768, dtype)
        NR.check_f32("ref l2norm", regime, case["R"], case["W"], case["R"], 1)
        NR.check_bf16_rounding("ref l2norm", regime, case["R"].to(BF16), case["W"], case["R"], 2,
                               strict=regime in NR.BF16_STRICT["l2norm"])


@pytest.mark.parametrize("regime", NR.BF16_STRICT["linear"])
def test_reference_passes_the_linear_checks(regime):
    for relu, addend in ((False, False), (True, False), (False, True)):
        case = NR.linear_case(regime, 96, 256, 768, BF16, relu, addend)
        assert bool(torch.isfinite(case["R"]).all())
        NR.check_f32("ref linear", regime, case["R"], case["W"], case["R"], 1, case["scale"])
        NR.check_bf16_rounding("ref linear", regime, case["R"].to(BF16), case["W"], case["R"], 2, case["scale"])


def test_reference_is_finite_in_the_chain_regimes():
    for regime in ("post_relu_unit", "outlier_channels", "offset1e3", "mixed"):
        case = NR.k1k2_case(regime, 2, 16, 768, 256, BF16, pre_ln=True)
        assert all(bool(torch.isfinite(case[k]).all()) for k in "WRS")
        NR.check_bf16_chain("ref K1+K2", regime, case["S"], case["W"], case["S"], 1)
    for std in (2.0, 6.0, 12.0):
        for holes in (False, True):
            case = NR.attention_case(std, 3, 32, 128, 4, BF16, holes, pre_ln=True)
            assert all(bool(torch.isfinite(case[k]).all()) for k in "WRS")
            NR.check_f32("ref attention", "peaked%g" % std, case["R"], case["W"], case["R"], 1)
    case = NR.q2c_case(8, 9, 32, 256, F32, holes=True)
    NR.check_f32("ref q2c", "near_duplicate", case["R"], case["W"], case["R"], 1)
    assert bool((case["W"][:, -1] == case["W"][:, 0]).all())


def test_reference_passes_the_pooling_ingest_and_convse_checks():
    for std in (2.0, 6.0, 12.0):
        for holes in (False, True):
            for n, l, h, seed in ((33, 30, 256, 0), (40, 30, 256, 3), (80, 30, 768, 3)):
                c = NR.pool_case(std, n, l, h, 2, BF16, holes, seed=seed)
                NR.check_bf16_rounding("ref modular_pool", "peaked%g" % std, c["R"].to(BF16), c["W"], c["R"], 2,
                                       strict=std == 2.0, cap=False)
    c = NR.ingest_case(7, 32, 768)
    NR.check_bf16_rounding("ref ingest_rows", "store_f16", c["R"].to(BF16), c["W"], c["R"], 2)
    for n_mod, merged in ((2, True), (2, False), (1, False)):
        c = NR.convse_case(12, 9, 48, 128, n_mod, merged, BF16, True)
        assert float((c["W"][0].max(-1)[0] > 0.9).double().mean()) > 0.9            # the span softmax is peaked
        assert bool((c["R"][0][~c["valid"]] == 0).all()) and bool(torch.isfinite(c["R"][0]).all())
        NR.check_prob_rows("ref convse", "peaked", c["R"][0], c["W"][0], 1e-6)
    c = NR.core_case(12.0, 3, 48, 256, 4, F32, True, True)
    NR.check_prob_rows("ref attention_core P", "peaked12", c["Pr"], c["Pw"], 1e-5)
    assert torch.equal(c["W"].view(3, 48, 4, 64)[..., :48].permute(0, 2, 1, 3), c["Pw"])    # V = identity: context == P
    c = NR.cross_case(12.0, 4, 33, 20, 128, 4, BF16)
    assert all(bool(torch.isfinite(c[k]).all()) for k in "WRS") and 0.2 < float(c["f64_rows"].float().mean()) < 0.8


# ---- sensitivity: wrong stand-ins -------------------------------------------------------------------------------------
def _truncate_bf16(x):
    """f32 -> bf16 by dropping the low 16 bits (round toward zero) instead of rounding to nearest."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def test_truncated_bf16_store_is_rejected_by_the_bias_check_and_accepted_by_the_old_limits():
    m, n, k = 300, 136, 96
    x, w, b = rnd(m, k, seed=1), rnd(n, k, seed=2, scale=k ** -0.5), rnd(n, seed=3)
    want = F.linear(x, w, b)
    bad = _truncate_bf16(want)
    close("linear (test_linear's bf16 limits)", bad, want, 2e-2, 1e-2)                 # the existing suite accepts it
    scale = x.double().norm(dim=1, keepdim=True) * w.double().norm(dim=1)[None] + b.double().abs()[None]
    W = f64.linear(x, w, b)
    NR.check_bf16_rounding("linear", "gaussian", want.to(BF16), W, want, 2, scale)       # a correct store passes
    with pytest.raises(AssertionError, match="not a correct rounding"):
        NR.check_bf16_rounding("linear truncated", "gaussian", bad, W, want, 2, scale)
    # the bias check alone catches it too (the maximum of a truncation error is one ulp: the boundary rule could hide it)
    err = (bad.double() - W) * torch.sign(W) / NR.bf16_ulp(W)
    assert float(err.mean()) < -0.4 and abs(float(err.mean())) > 50 * 4 * NR.BIAS_SIGMA / math.sqrt(err.numel())


def _softmax_exp2_no_max(s):
    """float32 softmax WITHOUT max subtraction, exp as exp2(x log2 e).  As accurate as the shifted form while nothing
    overflows (the normalisation cancels the dominant term's relative error); what it lacks is range."""
    e = torch.exp2(s * 1.4426950408889634)
    return e / e.sum(-1, keepdim=True)


def test_softmax_without_max_subtraction_overflows_at_spread_12_on_an_offset_and_is_rejected_as_non_finite():
    g = torch.Generator().manual_seed(5)
    v = rnd(64, 32, seed=9)

    def pooled(spread, softmax):
        s = shift + torch.randn(200, 64, generator=g) * spread
        W = torch.softmax(s.double(), -1) @ v.double()
        return softmax(s) @ v, torch.softmax(s, -1) @ v, W
    shift = 0.0
    bad, ref, W = pooled(1.0, _softmax_exp2_no_max)
    close("attention on flat logits (test_attention_block's f32 limit)", bad, ref, 1e-4)
    NR.check_f32("softmax", "flat", bad, W, ref, 8)
    # at spread 12 around zero f32's exp does not overflow (max logit ~50 < 88) and the unshifted form is as accurate in
    # absolute terms as the shifted one: what max subtraction buys is RANGE.  A common offset of 60 on the logits (softmax
    # is shift invariant; the float64 value and the float32 reference do not move) overflows the unshifted form.
    shift = 60.0
    bad, ref, W = pooled(12.0, _softmax_exp2_no_max)
    assert bool(torch.isfinite(ref).all()) and not bool(torch.isfinite(bad).all())
    with pytest.raises(AssertionError, match="non-finite"):
        NR.check_f32("softmax no max", "peaked12", bad, W, ref, 8)


def _layernorm_one_pass(x, g, b):
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean
    return (x - mean) * torch.rsqrt(var.clamp_min(0) + 1e-5) * g + b


def test_one_pass_variance_is_rejected_at_mean_1e3_and_accepted_at_zero_mean():
    a, b = rnd(37, 200, seed=4), rnd(37, 200, seed=5)
    g, beta = 1 + 0.1 * rnd(200, seed=6), 0.1 * rnd(200, seed=7)
    want = F.layer_norm(a + b, (200,), g, beta, 1e-5)
    close("add_layernorm (test_layernorm_l2norm_convert's f32 limit)", _layernorm_one_pass(a + b, g, beta), want, 1e-5)
    case = NR.layernorm_case("offset1e3", 64, 768, F32)
    bad = _layernorm_one_pass(case["a"] + case["b"], case["g"], case["beta"])
    with pytest.raises(AssertionError, match="float32 reference"):
        NR.check_f32("layernorm one pass", "offset1e3", bad, case["W"], case["R"], 8)


# ---- staged float64 autograd references of the training nodes -----------------------------------------------------------
def _plain(case, ls):
    """the node of `case` as plain torch ops on float64 leaves (weights rounded to bf16 beforehand): no oracle/f64 staging."""
    cfg = case.cfg
    sp = lambda t, h: t.view(t.shape[0], t.shape[1], cfg["heads"], h // cfg["heads"]).permute(0, 2, 1, 3)     # noqa: E731
    if case.op == "LinearFn":
        y = F.linear(*ls)
        return y.clamp_min(0) if cfg["relu"] else y
    if case.op == "LayerNormFn":
        a, b, g, beta = ls
        x = a if b is None else a + b
        return F.layer_norm(x, (x.shape[-1],), g, beta, O.LN_EPS)
    if case.op in ("QkvFn", "QkvResFn"):
        y = F.linear(ls[0], torch.cat(ls[1::2], 0), torch.cat(ls[2::2], 0))
        return (y, ls[0]) if cfg["residual"] else y
    if case.op.startswith("Attention"):
        h = ls[0].shape[-1] // {"core": 1, "kv": 1, "qkv": 3}[cfg["form"]]
        q, k, v = {"core": lambda: ls, "kv": lambda: (ls[0], ls[1][..., :h], ls[1][..., h:]),
                   "qkv": lambda: (ls[0][..., :h], ls[0][..., h:2 * h], ls[0][..., 2 * h:])}[cfg["form"]]()
        km, qm = cfg["k_mask"].double(), cfg["q_mask"]
        att = km.unsqueeze(1) if qm is None else torch.einsum("bm,bn->bmn", qm.double(), km)
        s = torch.matmul(sp(q, h), sp(k, h).transpose(-1, -2)) / math.sqrt(h // cfg["heads"]) + (1 - att.unsqueeze(1)) * O.ATT_NEG
        p = torch.softmax(s, dim=-1)
        o = torch.matmul(p if cfg["drop"] is None else p * cfg["drop"], sp(v, h))
        return o.permute(0, 2, 1, 3).contiguous().view(q.shape)
    if case.op == "ModularPoolFn":
        enc, wm = ls
        sc = torch.softmax(O.mask_logits(enc @ wm.t(), cfg["mask"].double().unsqueeze(2)), dim=1)
        return torch.einsum("blm,bld->mbd", sc, enc)
    if case.op == "VideoLevelScoresFn":
        n_mod, tot = cfg["n_mod"], 0
        for i in range(n_mod):
            s = torch.einsum("md,nld->mln", F.normalize(ls[i], dim=-1), F.normalize(ls[n_mod + i], dim=-1))
            tot = tot + torch.max(O.mask_logits(s, cfg["masks"][i].double().t().unsqueeze(0)), dim=1)[0]
        return tot / n_mod
    assert case.op == "PairSimFn"
    return torch.einsum("bd,bld->bl", *ls)


ALL_CASES = TC.all_cases()           # references are computed once per case object: the attention tests below share them


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_training_node_references(case):
    refs = case.refs()
    (Wo, Wg), (So, Sg), (Ro, Rg) = refs["W"], refs["S"], refs["R"]
    for t in Wo + [g for g in Wg if g is not None]:
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all())
    assert [g is None for g in Wg] == [not n for n in case.needs] == [g is None for g in Sg]
    if case.op in ("SpanLossFn", "RankLossFn"):      # f32 nodes: nothing is staged
        assert all(torch.equal(a, b) for a, b in zip(Wo, So)) and all(torch.equal(a, b) for a, b in zip(Wg, Sg))
        for w, r in zip(Wo + Wg, Ro + Rg):
            assert float((r.double() - w).abs().max()) <= 1e-5 * float(w.abs().max())
        return
    # identity stage == plain float64 autograd on the same operands, bit for bit
    is_w = lambda i: case.leaves[i] is not None and case.leaves[i].dtype == F32 and case.leaves[i].dim() == 2 and \
        case.op in ("LinearFn", "QkvFn", "QkvResFn")                                                          # noqa: E731
    ls = [None if t is None else (f64.bf16_round(t) if is_w(i) else t.double()).requires_grad_(ng)
          for i, (t, ng) in enumerate(zip(case.leaves, case.needs))]
    outs = _plain(case, ls)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, [g.double() for g in case.gouts])
    for a, b in zip(Wo, outs):
        assert torch.equal(a, b.detach())
    for a, l in zip(Wg, ls):
        assert a is None or torch.equal(a, l.grad)
    # the staged form differs from the exact one, by bf16 roundings and not by more
    diff = max(float((s - w).abs().max() / w.abs().max()) for s, w in zip(So + Sg, Wo + Wg) if w is not None)
    assert 0 < diff < 2e-2, diff
    # One bf16 store: S = rne(W), i.e. within HALF A bf16 ULP of W -- per element at most 2^-8 |W| (8 significand bits: the
    # spacing in [2^e, 2^(e+1)) is 2^(e-7)) and exactly on the grid.  (2^-9 |W| cannot hold for a correct rounding: W = 0.3993
    # lies 8.3e-4 = 2.07e-3 |W| from its nearest bf16 neighbour 0.3984.)  f32 outputs in front of every boundary are untouched.
    # (bf16_round goes through float32 like the kernels' stores: a double rounding may add one f32 rounding of W)
    half_ulp = lambda w: 0.5 * NR.bf16_ulp(w) + 2.0 ** -24 * w.abs()      # noqa: E731
    if not case.chain:
        for i, (s, w) in enumerate(zip(So, Wo)):
            if case.out_is_bf16(i):
                assert bool(((s - w).abs() <= half_ulp(w)).all()) and bool(((s - w).abs() <= (2.0 ** -8 + 2.0 ** -24) * w.abs()).all())
                assert torch.equal(s, f64.bf16_round(s))
            else:
                assert torch.equal(s, w)
        for i, (s, w) in enumerate(zip(Sg, Wg)):
            if w is None:
                continue
            if case.grad_is_bf16(i):                      # one store: half a bf16 ulp
                assert bool(((s - w).abs() <= half_ulp(w)).all()) and bool(((s - w).abs() <= (2.0 ** -8 + 2.0 ** -24) * w.abs()).all())
                assert torch.equal(s, f64.bf16_round(s))


def test_staged_is_straight_through():
    x = torch.randn(64, dtype=torch.float64, requires_grad=True)
    g = torch.randn(64, dtype=torch.float64)
    assert f64.staged(x, f64.ident) is x
    for fwd, bwd in ((True, True), (True, False), (False, True)):
        x.grad = None
        y = f64.staged(x, f64.bf16_round, fwd, bwd)
        y.backward(g)
        assert torch.equal(y.detach(), f64.bf16_round(x.detach()) if fwd else x.detach())
        assert torch.equal(x.grad, f64.bf16_round(g) if bwd else g)
    w = torch.randn(8, 8, requires_grad=True)
    f64.operand(w).sum().backward()
    assert torch.equal(f64.operand(w).detach(), w.detach().to(BF16).float()) and torch.equal(w.grad, torch.ones(8, 8))


# ---- attention cases: dropout mask model, coverage of the case table, block-wise check ------------------------------------------
def _drop_hash_scalar(i, seed):
    """common.h xml_seed_words + drop_hash on Python integers."""
    m = 0xFFFFFFFF
    s0, s1 = seed & m, ((seed >> 32) * 0x27D4EB2F + 0x165667B1) & m
    h = ((i & m) * 0x9E3779B1 + s0) & m
    h ^= ((i >> 32) * 0x85EBCA77) & m
    h ^= h >> 16
    h = h * 0x85EBCA6B & m
    h ^= h >> 13
    h = (h + s1) & m
    h = h * 0xC2B2AE35 & m
    return h ^ (h >> 16)


def test_dropout_mask_host_model_is_self_consistent():
    """drop_keep (vectorised, uint64 cut to 32 bits) == the scalar form on Python integers; a prefix of a longer mask is the
    shorter mask (counter based); both seed words matter; the kept share is 1 - p; the threshold and scale are float32 p's.
    (Equality with xml_dropout itself: tests/test_gpu_train_bf16.py::test_dropout_mask_equals_the_host_model.)"""
    import numpy as np
    for p in (0.1, 0.2):
        thresh = int(float(np.float32(p)) * 4294967296.0)
        assert thresh != int(p * 4294967296.0)                       # float32(p) is not p: the kernels get a float
        for seed in (4242, (0x9E3779B9 << 32) + 7, (1 << 32) + 4242):
            keep = f64.drop_keep(5000, p, seed)
            assert keep.dtype == np.bool_ and keep.shape == (5000,)
            assert [bool(k) for k in keep[:600]] == [_drop_hash_scalar(i, seed) >= thresh for i in range(600)]
            assert np.array_equal(f64.drop_keep(777, p, seed), keep[:777])
            assert abs(float(keep.mean()) - (1 - p)) < 4 * math.sqrt(p * (1 - p) / 5000)
        assert not np.array_equal(f64.drop_keep(5000, p, 4242), f64.drop_keep(5000, p, (1 << 32) + 4242))
        assert not np.array_equal(f64.drop_keep(5000, p, 4242), f64.drop_keep(5000, p, 4243))
        assert f64.drop_scale(p) == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    assert f64.drop_scale(0.2) == 1.25 and f64.drop_scale(0.1) != 1 / (1 - 0.1)      # float32 arithmetic, as the kernels'
    # the attention layout: rows and columns padded to multiples of 8, the valid corner cut out
    d = f64.attention_drop(2, 4, 13, 21, 0.2, 99)
    full = torch.from_numpy(f64.drop_keep(8 * 16 * 24, 0.2, 99)).view(2, 4, 16, 24)
    assert d.shape == (2, 4, 13, 21) and torch.equal(d != 0, full[:, :, :13, :21])
    assert set(d.unique().tolist()) == {0.0, f64.drop_scale(0.2)}


ATTENTION = [c for c in ALL_CASES if c.op.startswith("Attention")]


def test_attention_case_table_reaches_every_fused_instantiation():
    """The set of head sizes H / heads over the fused attention cases IS the library's list XML_ATTN_HEAD_SIZES (a head size
    added to the dispatch list without a training case fails here), each in every entry form its shape admits and with dropout
    somewhere; head counts 1, 2, 4, 8, 24; every listed length on some side; every case has a masked key, none a sequence
    without a valid key; `supported` is the library's answer."""
    import kernel_forms as DM
    assert len({c.name for c in ATTENTION}) == len(ATTENTION)
    dh_of = lambda c: c.gouts[0].shape[2] // c.cfg["heads"]      # noqa: E731
    fused = [c for c in ATTENTION if c.cfg["fused"]]
    assert {dh_of(c) for c in fused} == set(DM.ATTN_DH)
    for dh in DM.ATTN_DH:
        forms = {(c.cfg["form"], c.cfg["q_mask"] is not None) for c in fused if dh_of(c) == dh}
        assert ("core", False) in forms or ("core", True) in forms, dh
        assert any(f == "qkv" for f, _ in forms) or any(f == "kv" for f, _ in forms), dh
        # a wave's second row tile (rows >= 64) in use on the query and on the key side
        assert any(c.gouts[0].shape[1] > 64 and c.cfg["k_mask"].shape[1] > 64 for c in fused if dh_of(c) == dh), dh
    assert {c.cfg["form"] for c in fused} == {"core", "kv", "qkv"}
    assert {c.cfg["heads"] for c in fused} == {1, 2, 4, 8, 24}
    lengths = {l for c in fused for l in (c.gouts[0].shape[1], c.cfg["k_mask"].shape[1])}
    assert {1, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128} <= lengths
    for c in ATTENTION:
        lq, lk, h = c.gouts[0].shape[1], c.cfg["k_mask"].shape[1], c.gouts[0].shape[2]
        assert DM.attn_train_ok(lq, lk, h, c.cfg["heads"]) == c.cfg["supported"], c
        assert c.cfg["supported"] or not c.cfg["fused"]
        km = c.cfg["k_mask"]
        assert bool((km == 0).any()) and bool((km.sum(1) > 0).all()) and bool((km[0] == 1).all())
        if c.cfg["drop"] is not None:
            qm = 1 if c.cfg["q_mask"] is None else c.cfg["q_mask"][:, None, :, None]
            assert bool(((c.cfg["drop"] == 0) & (km[:, None, None, :] * qm > 0)).flatten(2).any(-1).all()), c
    chain = [c for c in ATTENTION if not c.cfg["fused"]]
    assert any(not c.cfg["supported"] for c in chain) and {dh_of(c) for c in chain} - set(DM.ATTN_DH) == {48}
    drops = [c for c in ATTENTION if c.cfg["drop"] is not None]
    assert len(drops) == 7 and all(c.cfg["p_drop"] == 0.2 for c in drops) and len({c.cfg["seed"] for c in drops}) == 7
    # L8 != L on both sides in some dropout case (an index formed from lq / lk instead of lq8 / lk8 shows up)
    assert any(c.gouts[0].shape[1] % 8 and c.cfg["k_mask"].shape[1] % 8 for c in drops)


@pytest.mark.parametrize("case", ATTENTION, ids=TC.ids(ATTENTION))
def test_f32_arithmetic_model_passes_the_block_wise_check(case):
    """The model of a CORRECT kernel -- the staged reference evaluated in float32 arithmetic: f32 accumulation, bf16 stores --
    under the block-wise check of tests/test_gpu_train_bf16.py.  Its worst block ratios against S over the attention cases are
    1.07 in max (O of `core 2x65x97x384 h4`) and 1.007 in rms; doubled once and rounded up to a power of two the max figure
    gives C_TRAIN_CHAIN = 4.  Asserted here: the max bound with margin 2 (ratio <= C_TRAIN_CHAIN / 2), and the rms bound as the
    GPU test has it (ratio <= C_TRAIN_CHAIN / 2 = 2).  Margin 2 on the rms would be a limit of 1.0, which no model that rounds
    where S rounds can meet: its rms error scatters around S's on both sides (1.007 at worst)."""
    from test_gpu_train_bf16 import C_TRAIN_CHAIN
    (Wo, Wg), (So, Sg) = case.refs()["W"], case.refs()["S"]
    outs, grads = case.run(F32, f64.bf16_round)
    dh = case.gouts[0].shape[2] // case.cfg["heads"]
    for (name, g, rows), w, s in zip(TC.attention_tensors(case, outs, grads), Wo + Wg, So + Sg):
        assert torch.equal(g.double(), f64.bf16_round(g))                 # the model's results are bf16 stores
        TC.check_blocks("f32 model %s" % name, case.name, g, w, s, dh, C_TRAIN_CHAIN / 2, rows, c_rms=C_TRAIN_CHAIN / 2)


def test_block_wise_check_sees_a_fault_that_the_tensor_wide_bound_hides():
    """One wrong tile of small values: the last key tile of the short sequence's dV in one head, off by 3 times its own staged
    error -- far below the tensor's largest staged error, so max|G - W| <= c max|S - W| over the tensor holds."""
    from test_gpu_train_bf16 import C_TRAIN_CHAIN
    case = [c for c in ATTENTION if c.name == "core 2x17x33x128 h4 fused"][0]
    (Wo, Wg), (So, Sg) = case.refs()["W"], case.refs()["S"]
    w, s = Wg[2], Sg[2]
    dh = 32
    rows, cols = slice(16, 22), slice(2 * dh, 3 * dh)          # sequence 1 has 22 valid keys: key tile 1, head 2
    bad = s.clone()
    bad[1, rows, cols] = w[1, rows, cols] + 6 * (s - w)[1, rows, cols]
    kerr, serr = float((bad - w).abs().max()), float((s - w).abs().max())
    krms, srms = float((bad - w).pow(2).mean().sqrt()), float((s - w).pow(2).mean().sqrt())
    assert kerr <= C_TRAIN_CHAIN * serr and krms <= C_TRAIN_CHAIN / 2 * srms          # check_chain's two bounds hold
    TC.check_blocks("dV", case.name, s, w, s, dh, C_TRAIN_CHAIN)
    with pytest.raises(AssertionError, match=r"block \(n, tile, column block\) \[1, 1, 2\]"):
        TC.check_blocks("dV wrong tile", case.name, bad, w, s, dh, C_TRAIN_CHAIN)
    # an exact zero of W that the kernel misses where S has it: rejected whatever the size
    off = s.clone()
    assert float(w[1, 22:].abs().max()) == 0
    off[1, 32, 5] = 2.0 ** -30
    with pytest.raises(AssertionError, match="staged reference is exact"):
        TC.check_blocks("dV masked key", case.name, off, w, s, dh, C_TRAIN_CHAIN)


# ---- the training loss tail and the optimizer at every loop edge (tests/train_tail_cases.py, tests/test_gpu_train_tail.py) ------
TAIL = dict(pair=TT.pair_sim_cases(), span=TT.span_cases(), rank=TT.rank_cases(), scores=TT.scores_cases())
TOY = dict(pair=[TC.pair_sim_case()], span=TC.span_loss_cases(), rank=TC.rank_loss_cases(), scores=TC.scores_cases())


def _masks_of(case):
    return case.cfg["masks"] if "masks" in case.cfg else [case.cfg["mask"]] * case.cfg["n_sim"]


def _keep_out(case):
    if case.op != "VideoLevelScoresFn":
        return None
    keep = torch.ones(case.gouts[0].shape[1], dtype=torch.bool)
    keep[2] = False                                 # the fully masked video's column
    return keep


def _as_kernel(case, res):
    """(outs, grads) of a float64 model -> in the dtypes the kernel returns (bf16 gradients for bf16 leaves)."""
    outs, grads = res
    return outs, [g if g is None or t.dtype != BF16 else f64.bf16_round(g) for g, t in zip(grads, case.leaves)]


def test_tail_case_tables_meet_their_own_conditions():
    # PairSimFn: the listed shapes, both dtypes, a partial last workgroup of the forward kernel
    assert {tuple(c.leaves[1].shape) for c in TAIL["pair"]} == set(TT.PAIR_SIM_SHAPES) and len(TAIL["pair"]) == 2 * len(TT.PAIR_SIM_SHAPES)
    assert any((n * l) % 4 for n, l, _ in TT.PAIR_SIM_SHAPES)
    # SpanLossFn
    assert {l for _, l, _ in TT.SPAN_SHAPES} == {1, 3, 63, 64, 65, 100, 127, 128} and {k for _, _, k in TT.SPAN_SHAPES} == {1, 3, 5, 31}
    assert {n for n, _, _ in TT.SPAN_SHAPES} == {1, 4, 5, 9} and (4, 3, 31) in TT.SPAN_SHAPES and (4, 128, 31) in TT.SPAN_SHAPES
    two_masks = second_half = clip0 = last_clip = len1 = 0
    for c in TAIL["span"]:
        st_ed, masks = c.cfg["st_ed"], c.cfg["masks"]
        rows = torch.arange(c.cfg["n"])
        for m in masks:                             # targets on unmasked clips of every stream
            assert bool((m[rows, st_ed[:, 0]] == 1).all()) and bool((m[rows, st_ed[:, 1]] == 1).all())
        assert bool((st_ed[:, 0] <= st_ed[:, 1]).all())
        lens = masks[0].sum(1).long()
        two_masks += len(masks) == 2 and not torch.equal(masks[0], masks[1])
        second_half += bool((st_ed[:, 0] >= 64).any()) and bool((st_ed[:, 1] >= 64).any())
        clip0 += bool((st_ed[:, 0] == 0).any())
        last_clip += bool((st_ed[:, 1] == lens - 1).any()) and bool((st_ed[:, 0] == lens - 1).any())
        len1 += bool((lens == 1).any())
    assert two_masks >= 2 and second_half >= 9 and clip0 == len(TAIL["span"]) and last_clip >= 30 and len1 >= 30
    # RankLossFn
    assert {c.cfg["n"] for c in TAIL["rank"] if c.cfg["kind"] is None} == set(TT.RANK_NS)
    for c in TAIL["rank"]:
        n, rc, rq = c.cfg["n"], c.cfg["rc"], c.cfg["rq"]
        for r in (rc, rq):
            assert int(r.min()) >= 1 and int(r.max()) <= n - 1 and int(r[0]) == 1 and int(r[1]) == n - 1
        if not c.cfg["lse"]:
            assert TT.hinge_distance(c) > TT.HINGE_CLEAR, c
        # the tie rule shows in the tie cases ("higher index first" selects other positions) and in no other
        flipped = n - 1 - f64.rank_order(TT.rank_masked(c.leaves[0]).flip(1))[torch.arange(n), rc.long()]
        assert torch.equal(flipped, TT.rank_selected(c.leaves[0], rc, rq)[0]) == (c.cfg["kind"] is None), c
        if c.cfg["kind"] == "straddle":             # rows 8 .. 11 select columns 253 .. 256 in turn, columns 12 .. 15 those rows
            cols, rows = TT.rank_selected(c.leaves[0], rc, rq)
            assert cols[8:12].tolist() == [253, 254, 255, 256] and rows[12:16].tolist() == [253, 254, 255, 256]
    # VideoLevelScoresFn
    assert {c.cfg["shape"] for c in TAIL["scores"]} == set(TT.SCORES_SHAPES)
    for c in TAIL["scores"]:
        assert TT.scores_gap(c) >= TT.SCORE_GAP, c
        assert c.cfg["dense"] or int((c.gouts[0] != 0).sum(1).max()) <= 3
        for v, (p1, p2) in c.cfg["ties"].items():
            f = c.leaves[c.cfg["n_mod"]]
            assert p1 < p2 and torch.equal(f[v, p1], f[v, p2]) and float(c.cfg["masks"][0][v, p2]) == 1
    tiles = {(p1 // 16 == p2 // 16) for _, t in TT.SCORES_TIES for p1, p2 in t.values()}
    assert tiles == {True, False}
    # every case: R passes the checks by itself and at most ROW_CAP of the rows of any tensor are excluded
    for c in sum(TAIL.values(), []):
        assert all(s <= TT.ROW_CAP for s in TT.excluded_shares(c)), c
        refs = c.refs()
        outs, grads = refs["R"]
        grads = [g if g is None or t.dtype != BF16 else refs["S"][1][i] for i, (g, t) in enumerate(zip(grads, c.leaves))]
        TT.check_case(c, outs, grads, keep_out=_keep_out(c))


# -- wrong kernels, restated on the CPU in float64 (so that nothing but the fault separates them from W) ------------------------
def _span_lanes_below_64(case):
    """span_loss_kernel without its h = 1 half: clips >= 64 have no logit, no softmax term, no target match, no DC row."""
    cfg = case.cfg
    n_sim, st_ed = cfg["n_sim"], cfg["st_ed"]

    def fn(*t, stage):
        tot = 0
        for lg, tg in zip(f64.span_logits(t[:n_sim], t[n_sim:], _masks_of(case), cfg["merged"], cfg["ks"]), (st_ed[:, 0], st_ed[:, 1])):
            low = lg[:, :64]
            hit = tg < 64
            tl = torch.where(hit, low[torch.arange(lg.shape[0]), tg.clamp(max=low.shape[1] - 1)], torch.zeros((), dtype=lg.dtype))
            tot = tot + (torch.logsumexp(low, 1) - tl).mean()
        return tot
    return _as_kernel(case, TT.run_fn(case, fn))


def _rank_model(select):
    """rank_loss_kernel with another selection: select(masked (n, n), ranks) -> (index per row, pair counted per row)."""
    def model(case):
        cfg = case.cfg
        lse, rc, rq = cfg["lse"], cfg["rc"], cfg["rq"]

        def fn(s, stage):
            n = s.shape[0]
            ar = torch.arange(n)
            pos = s[ar, ar]
            m = TT.rank_masked(s)
            out = []
            for sc, mm, r in ((s, m, rc), (s.t(), m.t().contiguous(), rq)):
                idx, live = select(mm, r.long())
                x = sc[ar, idx] - pos
                term = torch.log1p(torch.exp(x)) if lse else torch.clamp(TT.MARGIN + x, min=0)
                out.append((term * live.to(term.dtype)).sum() / n)
            return torch.stack(out)
        return _as_kernel(case, TT.run_fn(case, fn))
    return model


def _sel_stable(m, r):
    ar = torch.arange(m.shape[0])
    return f64.rank_order(m)[ar, r], torch.ones(m.shape[0], dtype=torch.bool)


def _sel_higher_index_first(m, r):
    """`k > j` in place of `k < j`: equal values, higher index first."""
    ar = torch.arange(m.shape[0])
    return m.shape[0] - 1 - f64.rank_order(m.flip(1))[ar, r], torch.ones(m.shape[0], dtype=torch.bool)


def _sel_counting_itself(m, r):
    """`k <= j` in place of `k < j`: every element counts itself, the kernel selects rank - 1."""
    ar = torch.arange(m.shape[0])
    return f64.rank_order(m)[ar, r - 1], torch.ones(m.shape[0], dtype=torch.bool)


def _sel_first_pass_only(m, r):
    """the row loop without its j += 256 stride: a wanted element at j >= 256 is never found."""
    idx, _ = _sel_stable(m, r)
    return idx, idx < 256


def _pair_sim_first_64_chunks(case):
    """pair_sim_bwd_vec_kernel without its c0 += 64 loop: hidden columns >= 512 of dq and df2 are never written (zeros here)."""
    outs, grads = case.run(torch.float64, f64.ident)
    h = case.leaves[0].shape[-1]
    if h % 8 == 0 and h <= 2048:
        grads = [g.clone() for g in grads]
        for g in grads:
            g[..., 512:] = 0
    return _as_kernel(case, (outs, grads))


def _argmax_last_on_ties(case):
    if not case.cfg.get("ties"):
        return _as_kernel(case, case.run(torch.float64, f64.ident))
    cfg = case.cfg
    wrong = TT.scores_case(*cfg["shape"], cfg["n_mod"], cfg["dense"], fused=cfg["fused"], ties=cfg["ties"], last=True)
    return wrong.run(torch.float64, f64.ident)


MUTANTS = [("span: lanes >= 64 dropped", "span", _span_lanes_below_64),
           ("rank: ties, higher index first", "rank", _rank_model(_sel_higher_index_first)),
           ("rank: only j < 256", "rank", _rank_model(_sel_first_pass_only)),
           ("pair_sim_bwd: chunks >= 64 skipped", "pair", _pair_sim_first_64_chunks),
           ("arg-max: last clip on ties", "scores", _argmax_last_on_ties)]


def _rejected(case, res):
    try:
        TT.check_case(case, *res, keep_out=_keep_out(case))
    except AssertionError:
        return True
    if case.op == "RankLossFn":                     # the structural check of the GPU test
        return not torch.equal(res[1][0] != 0, case.refs()["W"][1][0] != 0)
    return False


@pytest.mark.parametrize("name,op,model", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_wrong_tail_kernels_fail_the_new_cases_and_pass_the_old_ones(name, op, model):
    """Each restated fault is rejected on at least one new case and accepted on every case the suite had before: the gap was real."""
    bad = [c.name for c in TAIL[op] if _rejected(c, model(c))]
    assert bad, "%s: accepted on every new case" % name
    print("MUTANT %s: rejected on %d of %d new cases, e.g. %s" % (name, len(bad), len(TAIL[op]), bad[:3]))
    for c in TOY[op]:
        assert not _rejected(c, model(c)), "%s: the old case %s already rejects it" % (name, c)
    # what rejects it is what was built for it
    expect = {"span": lambda c: c.cfg["l"] > 64, "pair": lambda c: 512 < c.leaves[0].shape[-1] <= 2048 and c.leaves[0].shape[-1] % 8 == 0,
              "scores": lambda c: bool(c.cfg["ties"]),
              "rank": lambda c: c.cfg["kind"] is not None if "ties" in name else c.cfg["n"] > 256}[op]
    want = [c.name for c in TAIL[op] if expect(c)]
    assert set(bad) <= set(want) and (op == "rank" or bad == want), (bad, want)


def test_correct_restatements_pass_every_new_case():
    """the mutants' scaffolding with the right rule is accepted everywhere: the rejections above come from the faults alone."""
    for c in TAIL["rank"] + TOY["rank"]:
        assert not _rejected(c, _rank_model(_sel_stable)(c)), c
    for c in TAIL["span"]:
        if c.cfg["l"] <= 64:
            assert not _rejected(c, _span_lanes_below_64(c)), c


def test_rank_loss_that_counts_an_element_itself_is_off_by_one_everywhere():
    """The literal `k <= j` in the tie count makes every element count itself: the kernel then selects rank - 1 for every row,
    ties or not.  The old n = 17 cases reject that already; it is listed for completeness -- the tie rule proper is the
    "higher index first" model above, which only the new tie cases reject."""
    model = _rank_model(_sel_counting_itself)
    assert all(_rejected(c, model(c)) for c in TAIL["rank"]) and all(_rejected(c, model(c)) for c in TOY["rank"])


def test_adam_norm_that_misses_blocks_past_64_fails_the_new_layout_only():
    for layout, caught in ((TT.adam_layout(9), True), (TT.adam_layout(10), False), (TT.adam_toy_layout(), False)):
        names, sizes = layout
        state = TT.adam_state(sizes)
        want = TT.adam_reference(state)
        # the scaffolding: the true norms through the injected-norm path give the oracle's own step
        same = TT.adam_reference(state, sumsq=lambda g, off: TT.adam_sumsq_all(g, off))
        assert TT.check_adam("true norms", same[:4], want[:4], state["seg_off"], names, tol=1e-12) <= 1e-12
        wrong = TT.adam_reference(state, sumsq=TT.adam_sumsq_first_64_blocks)
        if caught:
            with pytest.raises(AssertionError, match="tensor big"):
                TT.check_adam("first 64 blocks", wrong[:4], want[:4], state["seg_off"], names)
        else:                                       # total % 4 != 0: no block partials at all; toy: no tensor has 64 blocks
            TT.check_adam("first 64 blocks", wrong[:4], want[:4], state["seg_off"], names)
    big = TT.adam_layout(9)[1][4]
    assert max(TT.adam_toy_layout()[1]) // 1024 < 64 < big // 1024
