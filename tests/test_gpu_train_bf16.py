"""Every training node of tvretrieval_amd/autograd.py in bf16 against float64: forward output and every returned gradient
versus the exact value W and the staged float64 reference S (oracle/f64.py `train_*`; cases and references:
tests/train_bf16_cases.py), the gradient sinks (USE_GRAD_SINKS) at node and model level, weight shadows and the fused loss tail.

A case runs the node's forward on fresh leaves and then calls the node's backward DIRECTLY (grad_fn.apply) with one upstream
gradient: what comes back is what the node returns, before autograd drops or casts anything.  Checks per tensor:
* structure, exact: a gradient is None exactly where needs_input_grad is false; G == 0 wherever W == 0 (masked keys and clips,
  padded rows, a fully masked video, ReLU);
* f32 tensors that are f32 sums of products of exact bf16 operands (dW, db, dgamma, dbeta, dwm, filters, sims, losses):
  max|G - W| <= 2e-5 max|W| (gemm_tn's and the wide LayerNorm's figure: only the summation order remains);
* bf16 tensors one store away from exact operands: a correct round-to-nearest of a value within the f32 allowance of W
  (numerics_regimes.check_bf16_rounding, >= 25 % of the elements decided);
* bf16 (and VideoLevelScoresFn's f32 scores) behind more than one bf16 boundary: max|G - W| <= C_TRAIN_CHAIN max|S - W| and
  rms(G - W) <= C_TRAIN_CHAIN / 2 rms(S - W);
* the attention nodes in addition block by block -- one (sequence, head, 16-row tile) of O, dQ, dK, dV, what one wave of
  attention_train.hip computes as one tile: the same two bounds against the block's OWN staged error, and exactly W where the
  staged reference is exactly W (train_bf16_cases.check_blocks; tests/test_numerics_reference.py runs the same check on an
  f32-arithmetic model of a correct kernel).
Every case prints `NUMERICS node.tensor case storage: kernel_err ref_err ratio` lines (pytest -s); the table, the derivation of
C_TRAIN_CHAIN and the run time are in profiles/numerics_margins.md ("Training ops, bf16")."""
import numpy as np
import pytest
import torch

import numerics_regimes as NR
import train_bf16_cases as TC
from conftest import load_golden
from test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
F32_SUM = 2e-5          # f32 sums of exact products: the figure of gemm_tn / the wide LayerNorm (tests/test_gpu_train.py)
C_ALLOW = 2             # f32 allowance under a bf16 store: C_GEMM / C_ROWWISE of tests/test_gpu_numerics.py
# worst measured ratio over the chain cases of this module: 1.001 in max (VideoLevelScoresFn scores 7x19x128 m2: 7.09e-4 against
# the staged reference's 7.08e-4), 1.00 in rms -> doubled once = 2.003 -> rounded up to a power of two = 4, the inference
# chains' figure (table: profiles/numerics_margins.md, "Training ops, bf16").  The block-wise check of the attention cases uses
# the same constant, derived from the reference side alone: the f32-arithmetic model of a correct kernel has a worst BLOCK
# ratio of 1.07 in max and 1.007 in rms (tests/test_numerics_reference.py) -> doubled once, rounded up to a power of two = 4
C_TRAIN_CHAIN = 4


def _d(t):
    return t.detach().cpu().double()


def check_f32_sum(name, case, G, W, R):
    G, W = _d(G), _d(W)
    assert G.shape == W.shape, (name, G.shape, W.shape)
    scale = float(W.abs().max()) or 1.0
    kerr, rerr = float((G - W).abs().max()) / scale, float((_d(R) - W).abs().max()) / scale
    NR.report(name, case, "f32", kerr, rerr)
    assert kerr <= F32_SUM, "%s %s: max|G-W| = %.3e of max|W| > %.1e" % (name, case, kerr, F32_SUM)
    return kerr, rerr


def check_chain(name, case, G, W, S, storage="bf16"):
    G, W, S = _d(G), _d(W), _d(S)
    assert G.shape == W.shape == S.shape, (name, G.shape, W.shape)
    kerr, serr = float((G - W).abs().max()), float((S - W).abs().max())
    krms, srms = float((G - W).pow(2).mean().sqrt()), float((S - W).pow(2).mean().sqrt())
    NR.report(name, case, storage, kerr, serr)
    print("NUMERICS %s %s %s rms: kernel %.3e staged %.3e ratio %.2f" % (name, case, storage, krms, srms, krms / srms if srms else 0))
    assert kerr <= C_TRAIN_CHAIN * serr, "%s %s: max|G-W| %.3e > %g x the staged reference's %.3e" % (name, case, kerr, C_TRAIN_CHAIN, serr)
    assert krms <= C_TRAIN_CHAIN / 2 * srms, "%s %s: rms %.3e > %g x the staged reference's %.3e" % (name, case, krms, C_TRAIN_CHAIN / 2, srms)


def check_tensor(case, name, G, W, S, R, is_bf16, keep=None):
    """one output or gradient of a case; keep: boolean mask (broadcastable) of the elements that are compared."""
    assert G is not None, "%s %s: missing" % (case, name)
    assert bool(torch.isfinite(G).all()), "%s %s: non-finite" % (case, name)
    G = _d(G)
    if keep is not None:
        keep = keep.expand_as(W)
        G, W, S, R = G[keep], W[keep], S[keep], R[keep]
    zero = W == 0
    assert bool((G[zero] == 0).all()), "%s %s: %d elements are non-zero where the exact gradient is exactly zero" % (
        case, name, int((G[zero] != 0).sum()))
    tag = "%s.%s" % (case.op, name)
    if not is_bf16 and not (case.op == "VideoLevelScoresFn" and name == "out0"):
        check_f32_sum(tag, case.name, G, W, R)
    elif case.chain:
        check_chain(tag, case.name, G, W, S, "bf16" if is_bf16 else "f32")
    else:
        # strict: the mean signed error stays within 4 sigma of a round-to-nearest store (a truncating store shows as -0.5 ulp);
        # cap=False: instead of the 1 % cap on boundary elements (small gradients sit within the allowance of a boundary, which is
        # in units of the tensor's largest value) at least 25 % of the elements must be decided
        NR.check_bf16_rounding(tag, case.name, G, W, R, C_ALLOW, strict=True, cap=False)


def to_dev(case):
    return [None if t is None else t.to(DEV).clone().requires_grad_(ng) for t, ng in zip(case.leaves, case.needs)]


def run_node(case, apply):
    """apply(*device leaves) -> (outputs tuple, position of every leaf in the node's inputs).  Forward, then the node's backward
    called directly.  -> outputs, gradients per leaf; asserts the None pattern of the returned tuple."""
    ls = to_dev(case)
    outs, pos = apply(*ls)
    node = outs[0].grad_fn
    ret = node.apply(*[g.to(DEV) for g in case.gouts])
    ret = ret if isinstance(ret, tuple) else (ret,)
    n_in = len(node.needs_input_grad)               # (arguments left at their defaults are not inputs of the node)
    assert len(ret) >= n_in and all(r is None for r in ret[n_in:])
    for j, (r, need) in enumerate(zip(ret, node.needs_input_grad)):
        assert (r is None) == (not need), "%s: input %d: gradient %s, needs_input_grad %s" % (
            case, j, "None" if r is None else "returned", need)
    for t, p, ng in zip(ls, pos, case.needs):
        assert t is None or node.needs_input_grad[p] == ng
    return outs, [None if t is None else ret[p] for t, p in zip(ls, pos)]


def compare(case, outs, grads, keep_out=None):
    refs = case.refs()
    (Wo, Wg), (So, Sg), (Ro, Rg) = refs["W"], refs["S"], refs["R"]
    assert len(outs) == len(Wo)
    for i, o in enumerate(outs):
        assert o.dtype == case.gouts[i].dtype
        check_tensor(case, "out%d" % i, o, Wo[i], So[i], Ro[i], case.out_is_bf16(i), keep_out)
    for i, (g, w) in enumerate(zip(grads, Wg)):
        if w is None:
            assert g is None
            continue
        check_tensor(case, "grad%d" % i, g, w, Sg[i], Rg[i], case.grad_is_bf16(i))


# ---- LinearFn ---------------------------------------------------------------------------------------------------------------
LINEAR = TC.linear_cases()


@pytest.mark.parametrize("case", LINEAR, ids=TC.ids(LINEAR))
def test_linear_fn_bf16(case):
    from tvretrieval_amd import train_ops as TO
    from tvretrieval_amd.autograd import LinearFn
    rows, k = case.leaves[0].shape
    n = case.leaves[1].shape[0]
    assert TO.gemm_tn_supported(rows, n, k, BF16) == (n % 8 == 0)         # both weight-gradient paths are reached
    outs, grads = run_node(case, lambda x, w, b: ((LinearFn.apply(x, w, b, case.cfg["relu"]),), (0, 1, 2)))
    assert outs[0].dtype == BF16 and all(g is None or g.dtype == t.dtype for g, t in zip(grads, case.leaves))
    compare(case, outs, grads)


# ---- LayerNormFn ------------------------------------------------------------------------------------------------------------
LAYERNORM = TC.layernorm_cases()


@pytest.mark.parametrize("case", LAYERNORM, ids=TC.ids(LAYERNORM))
def test_layernorm_fn_bf16(case):
    from tvretrieval_amd.autograd import LayerNormFn
    outs, grads = run_node(case, lambda a, b, g, beta: ((LayerNormFn.apply(a, b, g, beta, BF16),), (0, 1, 2, 3)))
    # dx is ONE bf16 tensor: converted to a's dtype for a (exactly: f32 holds every bf16 value), handed to b as it is
    assert all(g is None or g.dtype == t.dtype for g, t in zip(grads, case.leaves))
    if grads[0] is not None and grads[1] is not None:
        assert torch.equal(grads[0].float(), grads[1].float())
    compare(case, outs, grads)


# ---- QkvFn / QkvResFn -------------------------------------------------------------------------------------------------------
QKV = TC.qkv_cases()


@pytest.mark.parametrize("case", QKV, ids=TC.ids(QKV))
def test_qkv_fn_bf16(case):
    from tvretrieval_amd.autograd import QkvFn, QkvResFn
    res = case.cfg["residual"]

    def apply(x, *wb):
        out = QkvResFn.apply(x, *wb) if res else (QkvFn.apply(x, *wb),)
        return out, tuple(range(1 + len(wb)))
    outs, grads = run_node(case, apply)
    h = case.leaves[1].shape[0]
    assert outs[0].shape[-1] == h * (len(case.leaves) // 2)
    if res:
        assert torch.equal(outs[1], case.leaves[0].to(DEV))               # the residual operand IS x
        # "fallback": dres arrives in f32 -> rne(dY W) + dres by torch, in f32 (autograd casts it to x's dtype afterwards)
        assert grads[0].dtype == (F32 if res == "fallback" else BF16)
        outs = outs[:1]
    refs = case.refs()
    (Wo, Wg), (So, Sg), (Ro, Rg) = refs["W"], refs["S"], refs["R"]
    if res:
        for key in "WSR":                                                 # (out1 = x itself: nothing to compare)
            assert torch.equal(refs[key][0][1].double(), case.leaves[0].double())
    check_tensor(case, "out0", outs[0], Wo[0], So[0], Ro[0], True)
    for i, (g, w) in enumerate(zip(grads, Wg)):
        check_tensor(case, "grad%d" % i, g, w, Sg[i], Rg[i], i == 0)


def test_qkv_res_fn_only_the_residual_used():
    """QkvResFn whose projection is not used: through autograd (which materialises a zero dY) x gets exactly dres and the
    parameters exactly zero; called with dY = None the node returns (dres, None, ...) without a launch."""
    from tvretrieval_amd.autograd import QkvResFn
    case = TC.qkv_case(2, 24, 128, 2, "epilogue")
    ls = to_dev(case)
    dres = case.gouts[1].to(DEV)
    y, x_res = QkvResFn.apply(*ls)
    ret = y.grad_fn.apply(None, dres)
    assert ret[0] is dres and all(r is None for r in ret[1:]) and len(ret) == len(ls)
    x_res.backward(dres)
    assert torch.equal(ls[0].grad, dres)
    for p in ls[1:]:
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0


# ---- attention --------------------------------------------------------------------------------------------------------------
ATTENTION = TC.attention_cases()


@pytest.mark.parametrize("case", ATTENTION, ids=TC.ids(ATTENTION))
def test_attention_fns_bf16(case):
    """Fused and unfused chain share ONE staged reference at p_drop = 0: both keep S and dP in f32 and round P, O, dS, dQ, dK,
    dV to bf16.  Dropout on the probabilities (fused only: the chain rounds P before its dropout launch -- another staging,
    compared in tests/test_gpu_train.py) has its references from the host model of the mask (oracle/f64.py drop_keep, pinned to
    the kernel by test_dropout_mask_equals_the_host_model).  A shape without a fused instantiation (`supported` false in the case
    table) runs the chain because the library says so, not because the test switched the fused kernels off."""
    from tvretrieval_amd import train_ops as TO
    from tvretrieval_amd.autograd import AttentionCoreFn, AttentionKvFn, AttentionQkvFn
    cfg = case.cfg
    qm = None if cfg["q_mask"] is None else cfg["q_mask"].to(DEV)
    km, heads = cfg["k_mask"].to(DEV), cfg["heads"]
    lq, lk, hidden = case.gouts[0].shape[1], km.shape[1], case.gouts[0].shape[2]
    assert TO.attention_train_supported(lq, lk, hidden, heads, BF16) == cfg["supported"]
    assert cfg["supported"] or not cfg["fused"]
    drop = (cfg["p_drop"], cfg["seed"])
    if cfg["drop"] is not None:          # the mask drops something in every (sequence, head), among the valid pairs too
        assert cfg["fused"] and TO.SEED_BASE is None
        valid = cfg["k_mask"][:, None, None, :] * (1 if cfg["q_mask"] is None else cfg["q_mask"][:, None, :, None])
        assert bool(((cfg["drop"] == 0) & (valid > 0)).flatten(2).any(-1).all())
    try:
        TO.DISABLE_FUSED_ATTENTION = cfg["supported"] and not cfg["fused"]
        if cfg["form"] == "core":
            outs, grads = run_node(case, lambda q, k, v: ((AttentionCoreFn.apply(q, k, v, qm, km, heads, *drop),), (0, 1, 2)))
        elif cfg["form"] == "kv":
            outs, grads = run_node(case, lambda q, kv: ((AttentionKvFn.apply(q, kv, qm, km, heads, *drop),), (0, 1)))
        else:
            outs, grads = run_node(case, lambda t: ((AttentionQkvFn.apply(t, km, heads, *drop),), (0,)))
    finally:
        TO.DISABLE_FUSED_ATTENTION = False
    keep = None if cfg["q_mask"] is None else (cfg["q_mask"] > 0)[:, :, None]
    compare(case, outs, grads, keep_out=keep)
    # keys that are masked out get exactly no gradient (covered by "G == 0 wherever W == 0"; make sure W has such rows)
    wk = case.refs()["W"][1][-1]
    assert bool((wk.view(wk.shape[0], wk.shape[1], -1)[cfg["k_mask"] == 0][..., -8:] == 0).all()) and bool((cfg["k_mask"] == 0).any())
    # block by block: one (sequence, head, 16-row tile) against its own staged error
    (Wo, Wg), (So, Sg) = case.refs()["W"], case.refs()["S"]
    for (name, g, rows), w, s in zip(TC.attention_tensors(case, outs, grads), Wo + Wg, So + Sg):
        TC.check_blocks("%s.%s" % (case.op, name), case.name, g, w, s, hidden // heads, C_TRAIN_CHAIN, rows)


@pytest.mark.parametrize("p", [0.1, 0.2])
@pytest.mark.parametrize("seed", [4242, (0x9E3779B9 << 32) + 7])
def test_dropout_mask_equals_the_host_model(p, seed):
    """oracle/f64.py drop_keep / drop_scale == xml_dropout bit for bit: on the (N * heads, L8, L8) tensor of the unfused
    attention chain with L8 != L (the layout the fused kernels index, attention_train.hip) and on a flat tensor of 2^16 + 3
    elements.  The second seed has a high word: both seed words of xml_seed_words matter."""
    from oracle import f64
    from tvretrieval_amd import train_ops as TO
    assert TO.SEED_BASE is None
    for shape in ((2 * 4, 24, 40), (2 ** 16 + 3,)):           # L = 21 / 33 -> L8 = 24 / 40
        got = TO.dropout(torch.ones(shape, device=DEV), p, seed).cpu()
        keep = torch.from_numpy(f64.drop_keep(got.numel(), p, seed)).view(shape)
        assert torch.equal(got != 0, keep), "%d of %d elements differ" % (int(((got != 0) != keep).sum()), got.numel())
        assert torch.equal(got.double(), keep.double() * f64.drop_scale(p))
        assert 0 < int((~keep).sum()) < keep.numel()
    n, heads, lq, lk = 2, 4, 21, 33
    want = TO.dropout(torch.ones(n * heads, 24, 40, device=DEV), p, seed).cpu().view(n, heads, 24, 40)[:, :, :lq, :lk]
    assert torch.equal(f64.attention_drop(n, heads, lq, lk, p, seed), want.double())


# ---- ModularPoolFn ----------------------------------------------------------------------------------------------------------
POOL = TC.pool_cases()


@pytest.mark.parametrize("case", POOL, ids=TC.ids(POOL))
def test_modular_pool_fn_bf16(case):
    from tvretrieval_amd.autograd import ModularPoolFn
    mask = case.cfg["mask"].to(DEV)
    outs, grads = run_node(case, lambda enc, wm: ((ModularPoolFn.apply(enc, mask, wm),), (0, 2)))
    compare(case, outs, grads)
    assert bool((grads[0][mask == 0] == 0).all()) and bool((mask == 0).any())          # padded tokens: exactly no gradient


# ---- VideoLevelScoresFn -----------------------------------------------------------------------------------------------------
SCORES = TC.scores_cases()


@pytest.mark.parametrize("case", SCORES, ids=TC.ids(SCORES))
def test_video_level_scores_fn_bf16(case):
    import tvretrieval_amd.autograd as AG
    from tvretrieval_amd import train_ops as TO
    n_mod, ms = case.cfg["n_mod"], [m.to(DEV) for m in case.cfg["masks"]]
    nq, h = case.leaves[0].shape
    nv, l, _ = case.leaves[n_mod].shape
    try:
        AG.FUSED_LOSS_TAIL = case.cfg["fused"]
        if case.cfg["fused"]:
            assert l <= 128 and h % 8 == 0 and TO.q2c_scores_l2norm_bwd_supported(nq, nv, l, h, BF16)
        outs, grads = run_node(case, lambda *t: ((AG.VideoLevelScoresFn.apply(n_mod, *t, *ms),), tuple(range(1, 1 + 2 * n_mod))))
    finally:
        AG.FUSED_LOSS_TAIL = True
    # the fully masked video: score exactly mask_logits' -1e10 and (below, through W == 0) exactly no gradient; its column is
    # left out of the relative comparison of the scores (it would be the scale)
    assert bool((outs[0][:, 2] == -1e10).all())
    keep = torch.ones(nv, dtype=torch.bool)
    keep[2] = False
    compare(case, outs, grads, keep_out=keep[None, :])
    for i in range(n_mod):
        df = grads[n_mod + i]
        assert float(df[2].float().abs().max()) == 0.0 and bool((df[ms[i] == 0] == 0).all())
        assert float(df[1, 0].float().abs().max()) == 0.0                              # the all-zero clip row is never the arg-max


# ---- PairSimFn (bf16), SpanLossFn / RankLossFn (f32 in the bf16 model: see tests/train_bf16_cases.py) -----------------------
def test_pair_sim_fn_bf16():
    from tvretrieval_amd.autograd import PairSimFn
    case = TC.pair_sim_case()
    outs, grads = run_node(case, lambda q, f2: ((PairSimFn.apply(q, f2),), (0, 1)))
    assert outs[0].dtype == F32
    compare(case, outs, grads)


SPAN = TC.span_loss_cases()


@pytest.mark.parametrize("case", SPAN, ids=TC.ids(SPAN))
def test_span_loss_fn_f32(case):
    from tvretrieval_amd.autograd import SpanLossFn
    cfg = case.cfg
    n_sim, mask, st_ed = cfg["n_sim"], cfg["mask"].to(DEV), cfg["st_ed"].to(DEV)
    n_f = len(case.leaves) - n_sim

    def apply(*t):
        out = SpanLossFn.apply(cfg["merged"], cfg["ks"], st_ed, n_sim, *t[:n_sim], *([mask] * n_sim), *t[n_sim:])
        return (out,), tuple(range(4, 4 + n_sim)) + tuple(range(4 + 2 * n_sim, 4 + 2 * n_sim + n_f))
    outs, grads = run_node(case, apply)
    compare(case, outs, grads)


RANK = TC.rank_loss_cases()


@pytest.mark.parametrize("case", RANK, ids=TC.ids(RANK))
def test_rank_loss_fn_f32(case):
    from tvretrieval_amd.autograd import RankLossFn
    cfg = case.cfg
    rc, rq = cfg["rc"].to(DEV).int(), cfg["rq"].to(DEV).int()
    outs, grads = run_node(case, lambda s: ((RankLossFn.apply(s, rc, rq, 0.1, cfg["lse"]),), (0,)))
    compare(case, outs, grads)


# ---- gradient sinks, node level ---------------------------------------------------------------------------------------------
def _sink_setup(case, order):
    """The case's parameters (leaf indices `order`, in the optimizer's order) registered with a real BertAdam next to a bystander
    parameter; flat_g prefilled with a pattern.  -> device leaves (parameters: the nn.Parameters), optimizer, pattern."""
    from tvretrieval_amd.train import BertAdam
    ls = to_dev(case)
    params = {i: torch.nn.Parameter(case.leaves[i].to(DEV).clone()) for i in order}
    bystander = torch.nn.Parameter(torch.ones(5, 3, device=DEV))          # 15 elements: a padded slot follows it
    opt = BertAdam([bystander] + [params[i] for i in order], lr=0.0, warmup=-1, t_total=-1, schedule="none")
    for i, p in params.items():
        ls[i] = p
    g = torch.Generator().manual_seed(17)
    base = (torch.randn(opt.flat_g.numel(), generator=g) * 0.25).to(BF16).float().to(DEV)
    opt.flat_g.copy_(base)
    return ls, opt, base


def _slices(opt):
    return {id(p): slice(o, o + p.numel()) for p, o in zip(opt.params, opt._offs)}


SINK_NODES = {
    "LinearFn": (lambda: TC.linear_case(37, 64, 48, True, True), (1, 2)),
    "QkvFn": (lambda: TC.qkv_case(2, 24, 128, 2, None), (1, 3, 2, 4)),        # weights back to back, then the biases
    "LayerNormFn": (lambda: TC.layernorm_case(50, 128, BF16, True, True), (2, 3)),
    "ModularPoolFn": (lambda: TC.pool_cases()[1], (1,)),
}


def _apply_sink_node(name, case, ls):
    from tvretrieval_amd import autograd as AG
    if name == "LinearFn":
        return AG.LinearFn.apply(ls[0], ls[1], ls[2], case.cfg["relu"]), (0, 1, 2)
    if name == "QkvFn":
        return AG.QkvFn.apply(*ls), tuple(range(len(ls)))
    if name == "LayerNormFn":
        return AG.LayerNormFn.apply(ls[0], ls[1], ls[2], ls[3], BF16), (0, 1, 2, 3)
    return AG.ModularPoolFn.apply(ls[0], case.cfg["mask"].to(DEV), ls[1]), (0, 2)


@pytest.mark.parametrize("name", sorted(SINK_NODES))
def test_gradient_sinks_node_level(name):
    """USE_GRAD_SINKS on: the node's backward returns None for its parameters and ADDS their gradients to the optimizer's flat
    .grad buffer; off: it returns them and autograd adds them to p.grad (the same views).  Same f32 sums in another order:
    both within 2e-5 max|W| of float64, a second backward into the non-zeroed buffer gives twice the gradient, everything
    outside the parameters' slices (the pattern, the bystander, the padding) stays bitwise."""
    import tvretrieval_amd.autograd as AG
    make, order = SINK_NODES[name]
    case = make()
    Wg = case.refs()["W"][1]
    gout = case.gouts[0].to(DEV)
    got = {}
    try:
        for sinks in (True, False):
            AG.USE_GRAD_SINKS = sinks
            ls, opt, base = _sink_setup(case, order)
            sl = _slices(opt)
            y, pos = _apply_sink_node(name, case, ls)
            assert y.grad_fn.sunk == sinks, "%s: sinks %s but the node claimed %s" % (name, sinks, y.grad_fn.sunk)
            ret = y.grad_fn.apply(gout)
            for i in order:
                assert (ret[pos[i]] is None) == sinks, "%s: sinks %s, parameter %d: %s" % (name, sinks, i, ret[pos[i]])
            assert ret[0] is not None
            touched = torch.zeros_like(base, dtype=torch.bool)
            for times in (1, 2):
                if times == 2 or not sinks:
                    if sinks:
                        y.grad_fn.apply(gout)                            # accumulates again, nothing zeroed in between
                    else:
                        y.backward(gout, retain_graph=True)              # AccumulateGrad: p.grad += returned gradient
                for i in order:
                    s = sl[id(ls[i])]
                    touched[s] = True
                    assert ls[i].grad.data_ptr() == opt.flat_g.data_ptr() + 4 * s.start
                    want = base[s].cpu().double() + times * Wg[i].reshape(-1)
                    err = float((opt.flat_g[s].cpu().double() - want).abs().max()) / float(Wg[i].abs().max())
                    NR.report("%s.sink%d" % (name, i), "sinks %s x%d" % ("on" if sinks else "off", times), "f32", err, 0.0)
                    assert err <= F32_SUM * times, (name, sinks, i, times, err)
                if times == 1:
                    got[sinks] = {i: ls[i].grad.detach().clone() - base[sl[id(ls[i])]].view(ls[i].shape) for i in order}
            assert torch.equal(opt.flat_g[~touched], base[~touched]), "%s: flat_g written outside the parameters' slices" % name
            assert int((~touched).sum()) >= 16
    finally:
        AG.USE_GRAD_SINKS = True
    for i in order:
        err = float((got[True][i] - got[False][i]).abs().max()) / float(Wg[i].abs().max())
        assert err <= F32_SUM, (name, i, err)


# ---- gradient sinks, weight shadows, fused loss tail: model level -----------------------------------------------------------
def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def model_grads():
    """Golden batch train_step_video_sub_h128, eval mode, one forward / backward through the optimizer's path per setting of
    (USE_GRAD_SINKS, SHADOW_WEIGHTS, FUSED_LOSS_TAIL); bf16 compute, and the f32 path once (pinned to the reference by
    test_golden_train_steps_fp32) as the stand-in for the exact value.  -> {setting: {parameter: gradient}}."""
    import tvretrieval_amd.autograd as AG
    import tvretrieval_amd.train as TR
    from test_gpu_train import build_train_model
    d, cfg, _ = load_golden("train_step_video_sub_h128")
    batch = dict(query_feat=_T(d["query_feat"]), query_mask=_T(d["query_mask"]), video_feat=_T(d["video_feat"]),
                 video_mask=_T(d["video_mask"]), sub_feat=_T(d["sub_feat"]), sub_mask=_T(d["sub_mask"]),
                 st_ed_indices=_T(d["st_ed_indices"]), neg_ctx_rank=d["neg_ctx_rank"], neg_q_rank=d["neg_q_rank"])
    out = {}
    settings = [("base", True, True, True, BF16), ("base again", True, True, True, BF16), ("sinks off", False, True, True, BF16),
                ("shadows off", True, False, True, BF16), ("tail unfused", True, True, False, BF16), ("f32", True, True, True, F32)]
    try:
        for name, sinks, shadows, tail, dt in settings:
            AG.USE_GRAD_SINKS, TR.SHADOW_WEIGHTS, AG.FUSED_LOSS_TAIL = sinks, shadows, tail
            m = build_train_model(cfg, d, dt)
            opt = TR.BertAdam(m.parameters(), lr=0.0, warmup=-1, t_total=-1, schedule="none")
            for _ in range(2):           # the second pass reads the transposed weight shadows that the first one asked for
                opt.zero_grad()
                loss, _ = TR.xml_forward_train(m, **batch)
                loss.backward()
            if dt == BF16:
                sh = opt._shadow
                assert bool(sh is not None and len(sh["t"]) >= 8) == shadows
            torch.cuda.synchronize()
            out[name] = {n: p.grad.detach().cpu().double().clone() for n, p in m.named_parameters()}
            assert all(p.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * o for p, o in zip(opt.params, opt._offs))
    finally:
        AG.USE_GRAD_SINKS, TR.SHADOW_WEIGHTS, AG.FUSED_LOSS_TAIL = True, True, True
    return out


def _scale(grads, n):
    """max of the tensor; a key bias has an analytically ZERO gradient (softmax is shift invariant): its gradient is the
    cancellation noise of the stacked column sum that also yields the value bias -- that sum's scale."""
    return float(grads[n.replace(".key.bias", ".value.bias")].abs().max())


@pytest.mark.parametrize("flip", ["base again", "sinks off", "shadows off"])
def test_model_gradients_do_not_depend_on_sinks_or_shadows(model_grads, flip):
    """Sinks and weight shadows change WHERE an f32 sum lands and who converts a weight, not a single bf16 operand: every
    parameter gradient agrees with the default setting's within 2e-5 of the tensor's max (order of the f32 atomics)."""
    base, other = model_grads["base"], model_grads[flip]
    assert base.keys() == other.keys() and len(base) > 80
    worst = sorted(((float((other[n] - base[n]).abs().max()) / _scale(base, n), n) for n in base), reverse=True)
    NR.report("model gradients", flip, "bf16", worst[0][0], 0.0)
    print("worst:", worst[:3])
    assert worst[0][0] <= F32_SUM, worst[:5]
    assert min(float(g.abs().max()) for n, g in base.items() if not n.endswith(".key.bias")) > 0


def test_model_gradients_fused_loss_tail_on_off(model_grads):
    """FUSED_LOSS_TAIL = False runs xml_q2c_scores_bwd, whose d(qn) / d(cn) are ATOMIC-ordered f32 sums over the (query, video)
    pairs, then xml_l2norm_bwd, which stores dquery / dfeat in bf16: a tensor upstream of VideoLevelScoresFn may see other bf16
    gradients than with the one-launch backward (measured: the 17 tensors of the query side -- query_input_proj, query_pos_embed,
    query_encoder; the context side stays within 2e-5).  Those tensors get the chain bound, with the f32 path's gradient as the
    exact value and the default setting as the staged reference; the span head (query linears, predictors: fed by PairSimFn /
    SpanLossFn only, untouched by the flag) stays within 2e-5."""
    base, other, exact = model_grads["base"], model_grads["tail unfused"], model_grads["f32"]
    n_chain = 0
    for n in sorted(base):
        s = _scale(base, n)
        err = float((other[n] - base[n]).abs().max()) / s
        if "_query_linear" in n or "predictor" in n:
            assert err <= F32_SUM, (n, err)
            continue
        if err <= F32_SUM:
            continue
        n_chain += 1          # (key biases included: cancellation noise on both sides, at the value bias's scale)
        kerr, serr = float((other[n] - exact[n]).abs().max()), float((base[n] - exact[n]).abs().max())
        krms, srms = float((other[n] - exact[n]).pow(2).mean().sqrt()), float((base[n] - exact[n]).pow(2).mean().sqrt())
        print("NUMERICS model gradient %s tail unfused bf16: kernel_err %.3e ref_err %.3e ratio %.2f (rms ratio %.2f)" % (
            n, kerr, serr, kerr / serr, krms / srms))
        assert kerr <= C_TRAIN_CHAIN * serr and krms <= C_TRAIN_CHAIN / 2 * srms, (n, kerr, serr, krms, srms)
    print("tail unfused: %d of %d tensors beyond 2e-5, under the chain bound" % (n_chain, len(base)))
    assert n_chain > 0, "FUSED_LOSS_TAIL = False changed no bf16 gradient: the flag no longer reaches the separate launches"
