"""The f32 "serial middle" of the training step and the optimizer kernels against float64 at every loop edge: PairSimFn (f32 and
bf16), SpanLossFn, RankLossFn, VideoLevelScoresFn's arg-kept backward (and the padded path), xml_bert_adam_step and
xml_clip_grad_norm.  Cases, references and the checks themselves: tests/train_tail_cases.py (its header names the branch each case
reaches); tests/test_numerics_reference.py runs the same checks on CPU restatements of wrong kernels.

Per tensor (train_tail_cases.check_tensor): G == 0 exactly where the float64 value W is exactly zero; max|G - W| / max|W| of the
whole tensor AND of every row (batch row of sim / dsim / dq / df2 / dquery, video of dfeat, row of dscores) within the larger of
the project's tolerance for the op (2e-5 pair_sim and rank, 5e-5 span and scores: tests/test_gpu_train.py) and C_TRAIN_CHAIN = 4
times the same figure of R, the float32 CPU evaluation.  Structure, exact: the rank loss' dscores is non-zero exactly where the
float64 reference's is, inside the positions the stable order selects plus the diagonal (the tie rule "lower index first");
dfeat rows without a gradient -- the duplicate of a tied winning clip among them -- are bit-zero; the kept arg-max is the
float64 arg-max of every pair ("first clip on ties").  Every case prints `NUMERICS ...` lines (pytest -s); the table is in
profiles/numerics_margins.md ("Training loss tail and optimizer, f32")."""
import pytest
import torch

import train_tail_cases as TT
from test_gpu_kernels import DEV
from test_gpu_train_bf16 import run_node

pytestmark = pytest.mark.gpu

F32 = torch.float32


# ---- PairSimFn --------------------------------------------------------------------------------------------------------------
PAIR = TT.pair_sim_cases()


@pytest.mark.parametrize("case", PAIR, ids=TT.ids(PAIR))
def test_pair_sim_fn_every_chunk_and_wave_edge(case):
    from tvretrieval_amd.autograd import PairSimFn
    outs, grads = run_node(case, lambda q, f2: ((PairSimFn.apply(q, f2),), (0, 1)))
    assert outs[0].dtype == F32 and all(g.dtype == t.dtype for g, t in zip(grads, case.leaves))
    TT.check_case(case, outs, grads)


# ---- SpanLossFn -------------------------------------------------------------------------------------------------------------
SPAN = TT.span_cases()


def _span_node(case):
    from tvretrieval_amd.autograd import SpanLossFn
    cfg = case.cfg
    n_sim, st_ed = cfg["n_sim"], cfg["st_ed"].to(DEV)
    masks = [m.to(DEV) for m in cfg["masks"]]
    n_f = len(case.leaves) - n_sim

    def apply(*t):
        out = SpanLossFn.apply(cfg["merged"], cfg["ks"], st_ed, n_sim, *t[:n_sim], *masks, *t[n_sim:])
        return (out,), tuple(range(4, 4 + n_sim)) + tuple(range(4 + 2 * n_sim, 4 + 2 * n_sim + n_f))
    return run_node(case, apply)


@pytest.mark.parametrize("case", SPAN, ids=TT.ids(SPAN))
def test_span_loss_fn_both_wave_halves_every_filter_width(case):
    outs, grads = _span_node(case)
    TT.check_case(case, outs, grads)


SPAN2 = [c for c in SPAN if c.cfg["n_sim"] == 2]


@pytest.mark.parametrize("case", SPAN2, ids=TT.ids(SPAN2))
def test_span_loss_one_fill_layout_equals_three_fill_layout(case):
    """xml_span_loss zero-fills [dsim0 | dsim1 | dconv_w] with one launch when the caller laid them out back to back
    (train_ops.span_loss does for n_sim = 2) and with three otherwise: the same gradients from separately allocated buffers.
    The atomics reorder the sums, so the two runs are compared like kernel and reference: both against W, and with each other
    within the per-row limit."""
    from tvretrieval_amd import _lib, train_ops as TO
    cfg = case.cfg
    n, l, ks, merged = cfg["n"], cfg["l"], cfg["ks"], cfg["merged"]
    sims = [t.to(DEV) for t in case.leaves[:2]]
    masks = [m.to(DEV) for m in cfg["masks"]]
    conv_w = torch.cat([f.reshape(-1) for f in case.leaves[2:]]).to(DEV)
    st_ed = cfg["st_ed"].to(DEV)
    gout = torch.ones(1, device=DEV)
    one_s, one_w = TO.span_loss(sims, conv_w, masks, st_ed, merged, ks, gout=gout)
    assert one_s[1].data_ptr() == one_s[0].data_ptr() + 4 * n * l and one_w.data_ptr() == one_s[1].data_ptr() + 4 * n * l
    # three allocations with a gap in front of each, filled with a pattern the zero fill has to remove
    pad = 64
    bufs = [torch.full((pad + k,), 7.0, device=DEV) for k in (n * l, n * l, conv_w.numel())]
    d0, d1, dw = bufs[0][pad:].view(n, l), bufs[1][pad:].view(n, l), bufs[2][pad:]
    assert not (d1.data_ptr() == d0.data_ptr() + 4 * n * l and dw.data_ptr() == d1.data_ptr() + 4 * n * l)
    p = TO._p
    TO.check(_lib.load().xml_span_loss(p(sims[0]), p(sims[1]), p(conv_w), p(masks[0]), p(masks[1]), p(st_ed), int(merged), 2, ks,
                                       n, l, p(gout), None, p(d0), p(d1), p(dw), TO._stream()), "xml_span_loss")
    assert all(float(b[:pad].min()) == 7.0 and float(b[:pad].max()) == 7.0 for b in bufs)
    _, Wg = case.refs()["W"]
    _, Rg = case.refs()["R"]
    tol = TT.TOL["SpanLossFn"]
    for i, (a, b) in enumerate(((one_s[0], d0), (one_s[1], d1))):
        TT.check_tensor("SpanLossFn.three_fill.grad%d" % i, case.name, b, Wg[i], Rg[i], tol)
        # one against the other: each is within its row's limit of W, so they are within twice that of each other
        top = Wg[i].abs().amax(1).clamp_min(1e-300)
        lim = 2 * torch.clamp(TT.C_TRAIN_CHAIN * (Rg[i].double() - Wg[i]).abs().amax(1) / top, min=tol)
        diff = (a.cpu().double() - b.cpu().double()).abs().amax(1) / top
        live = Wg[i].abs().amax(1) > 0
        assert bool((diff[live] <= lim[live]).all()) and bool((a.cpu()[~live] == b.cpu()[~live]).all())
    wcat = torch.cat([g.reshape(-1) for g in Wg[2:]])
    rcat = torch.cat([g.reshape(-1) for g in Rg[2:]])
    for name, got in (("one_fill", one_w), ("three_fill", dw)):
        TT.check_tensor("SpanLossFn.%s.dconv_w" % name, case.name, got, wcat, rcat, tol)


# ---- RankLossFn -------------------------------------------------------------------------------------------------------------
RANK = TT.rank_cases()


@pytest.mark.parametrize("case", RANK, ids=TT.ids(RANK))
def test_rank_loss_fn_every_row_pass_and_tie(case):
    from tvretrieval_amd.autograd import RankLossFn
    cfg = case.cfg
    rc, rq = cfg["rc"].to(DEV).int(), cfg["rq"].to(DEV).int()
    outs, grads = run_node(case, lambda s: ((RankLossFn.apply(s, rc, rq, TT.MARGIN, cfg["lse"]),), (0,)))
    TT.check_case(case, outs, grads)
    # the tie rule, exact: gradients sit where the stable float64 order puts them and nowhere else
    W = case.refs()["W"][1][0]
    got = grads[0].cpu() != 0
    assert torch.equal(got, W != 0), "dscores is non-zero at %d positions, the reference at %d; first difference (row, column) %s" % (
        int(got.sum()), int((W != 0).sum()), (got != (W != 0)).nonzero()[:1].tolist())
    assert not bool((got & ~TT.rank_expected_nonzero(case)).any())


def test_rank_loss_refuses_more_than_1024_pairs():
    from tvretrieval_amd import train_ops as TO
    n = 1025
    scores = torch.zeros(n, n, device=DEV)
    ranks = torch.ones(n, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        TO.rank_loss(scores, ranks, ranks, TT.MARGIN, False)


# ---- VideoLevelScoresFn -----------------------------------------------------------------------------------------------------
SCORES = TT.scores_cases()


@pytest.mark.parametrize("case", SCORES, ids=TT.ids(SCORES))
def test_video_level_scores_fn_every_tile_shape_and_tie(case):
    import tvretrieval_amd.autograd as AG
    from tvretrieval_amd import ops, train_ops as TO
    cfg = case.cfg
    n_mod, ms = cfg["n_mod"], [m.to(DEV) for m in cfg["masks"]]
    nq, h = case.leaves[0].shape
    nv = case.leaves[n_mod].shape[0]
    try:
        AG.FUSED_LOSS_TAIL = cfg["fused"]
        if cfg["fused"]:
            for f in case.leaves[n_mod:]:
                assert f.shape[1] <= 128 and h % 8 == 0 and TO.q2c_scores_l2norm_bwd_supported(nq, nv, f.shape[1], h, F32)
        outs, grads = run_node(case, lambda *t: ((AG.VideoLevelScoresFn.apply(n_mod, *t, *ms),), tuple(range(1, 1 + 2 * n_mod))))
    finally:
        AG.FUSED_LOSS_TAIL = True
    # the fully masked video: score exactly -1e10, left out of the relative comparison of the scores (it would be the scale)
    assert bool((outs[0][:, 2] == -1e10).all())
    keep = torch.ones(nv, dtype=torch.bool)
    keep[2] = False
    TT.check_case(case, outs, grads, keep_out=keep)
    Wg = case.refs()["W"][1]
    for i in range(n_mod):
        df = grads[n_mod + i].cpu()
        none = Wg[n_mod + i].abs().amax(-1) == 0                 # (video, clip) rows that receive no gradient
        assert bool((df[none] == 0).all()) and bool((df[cfg["masks"][i] == 0] == 0).all()) and float(df[2].abs().max()) == 0.0
        # the kept arg-max clip of every pair is the float64 one (top two at least SCORE_GAP apart; exact ties: the first clip)
        if cfg["fused"]:
            qn, cn = ops.l2norm_rows(case.leaves[i].to(DEV)), ops.l2norm_rows(case.leaves[n_mod + i].to(DEV))
            _, arg = TO.q2c_scores_arg(qn, cn, ms[i].contiguous())
            assert torch.equal(arg.cpu().long(), TT.scores_argmax(case, i))
    for v, (p1, p2) in cfg["ties"].items():
        df = grads[n_mod].cpu()
        assert float(df[v, p2].abs().max()) == 0.0, "video %d: the duplicate at clip %d received a gradient" % (v, p2)
        if float(Wg[n_mod][v, p1].abs().max()) > 0:
            assert float(df[v, p1].abs().max()) > 0, "video %d: the first of the tied clips (%d) received no gradient" % (v, p1)


# ---- xml_bert_adam_step -----------------------------------------------------------------------------------------------------
def _adam_run(state, max_grad_norm=TT.ADAM["max_grad_norm"], active=None, lr_mult=None, ws=True):
    """one step of the kernel on a device copy of `state` -> (p, g, m, v, norms)."""
    from tvretrieval_amd import train_ops as TO
    p, g, m, v = (state[k].to(DEV).clone() for k in "pgmv")
    n_seg = state["seg_lr"].numel()
    norms = torch.full((n_seg,), -1.0, device=DEV)
    norm_ws = torch.empty((p.numel() + 1023) // 1024, device=DEV) if ws else None
    TO.bert_adam_step(p, g, m, v, state["seg_off"].to(DEV), state["seg_lr"].to(DEV), state["seg_wd"].to(DEV), norms,
                      TT.ADAM["lr_mult"], TT.ADAM["b1"], TT.ADAM["b2"], TT.ADAM["eps"], max_grad_norm,
                      seg_active=None if active is None else torch.tensor(active, dtype=torch.uint8, device=DEV),
                      seg_lr_mult=None if lr_mult is None else lr_mult.to(DEV), norm_ws=norm_ws)
    torch.cuda.synchronize()
    return p, g, m, v, norms


@pytest.mark.parametrize("tail", [9, 10], ids=["total%4==0", "total%4!=0"])
def test_bert_adam_step_every_norm_and_update_path(tail):
    """tail = 10: (total & 3) != 0, every non-vector path of the three kernels."""
    names, sizes = TT.adam_layout(tail)
    state = TT.adam_state(sizes)
    off = state["seg_off"]
    want = TT.adam_reference(state)
    clipped = [TT.ADAM["max_grad_norm"] / (s ** 0.5 + 1e-6) < 1 for s in want[4]]
    assert any(clipped) and not all(clipped) and clipped[names.index("big")]
    got_ws, got_atomic = _adam_run(state, ws=True), _adam_run(state, ws=False)
    for tag, got in (("norm_ws tail%d" % tail, got_ws), ("atomics tail%d" % tail, got_atomic)):
        TT.check_adam(tag, got[:4], want[:4], off, names)
        ss = torch.tensor(want[4], dtype=torch.float64)
        err = ((got[4].cpu().double() - ss).abs() / ss).max()
        print("NUMERICS bert_adam_step norms %s f32: worst err %.3e" % (tag, float(err)))
        assert float(err) <= 2e-6
    a, b = got_ws[4].cpu().double(), got_atomic[4].cpu().double()
    assert float(((a - b).abs() / b).max()) <= 1e-6
    # the gradient of a tensor that is not clipped is not written
    for c, lo, hi in zip(clipped, off[:-1].tolist(), off[1:].tolist()):
        if not c:
            assert torch.equal(got_ws[1][lo:hi].cpu(), state["g"][lo:hi]) and torch.equal(got_atomic[1][lo:hi].cpu(), state["g"][lo:hi])
    # max_grad_norm = 0: no clipping, g bitwise untouched, the norm kernels not launched
    got = _adam_run(state, max_grad_norm=0.0)
    TT.check_adam("no clip tail%d" % tail, got[:4], TT.adam_reference(state, max_grad_norm=0.0)[:4], off, names)
    assert torch.equal(got[1].cpu(), state["g"]) and bool((got[4] == -1.0).all())
    # seg_active: "filler" (ends mid-block: the per-element path) and "aligned" (one whole block: the uniform path) inactive
    active = [nm not in ("filler", "aligned") for nm in names]
    got = _adam_run(state, active=active)
    TT.check_adam("seg_active tail%d" % tail, got[:4], TT.adam_reference(state, active=active)[:4], off, names)
    for nm in ("filler", "aligned"):
        lo, hi = int(off[names.index(nm)]), int(off[names.index(nm) + 1])
        for k, t in zip("pgmv", got[:4]):
            assert torch.equal(t[lo:hi].cpu(), state[k][lo:hi]), "%s of the inactive tensor %s was written" % (k, nm)
    # seg_lr_mult (per-tensor schedule step) against the scalar lr_mult: the reference with the same per-tensor factors, and
    # equal factors give the scalar run's step (not bit for bit: the norms' atomics land in another order every run)
    lm = state["seg_lr_mult"]
    got = _adam_run(state, lr_mult=lm)
    TT.check_adam("seg_lr_mult tail%d" % tail, got[:4], TT.adam_reference(state, lr_mult=lm)[:4], off, names)
    same = _adam_run(state, lr_mult=torch.full_like(lm, TT.ADAM["lr_mult"]))
    TT.check_adam("seg_lr_mult == lr_mult tail%d" % tail, same[:4], want[:4], off, names)
    assert not torch.equal(got[0], got_ws[0])


# ---- xml_clip_grad_norm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("n", TT.CLIP_NS)
def test_clip_grad_norm_scalar_tails_and_second_grid_pass(n, clip):
    from tvretrieval_amd import train_ops as TO
    g = torch.randn(n, generator=TT._gen(n % 1000)) * 0.5
    norm = float(g.double().norm(2))
    max_norm = norm * (0.25 if clip else 4.0)
    want, clipped = TT.clip_reference(g, max_norm)
    assert clipped == clip
    got = TO.clip_grad_norm(g.to(DEV).clone(), max_norm).cpu()
    if not clip:
        assert torch.equal(got, g)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("NUMERICS clip_grad_norm n%d %s f32: kernel_err %.3e" % (n, "clipped" if clip else "unclipped", err))
    assert err <= 2e-6
