"""The re-rank kernels of convse.hip -- K7 (ops.convse_rerank), its span-evidence instantiation (ops.span_evidence) and the
exact-rank re-score (ops.q2c_rescore) -- at every mainloop form, step count, filter width, chunk occupancy, row length and
inversion path, against float64 (oracle/f64.py: convse, q2c_rescore).  Cases, operands, references and the checks themselves:
tests/convse_cases.py (tests/test_convse_cases_reference.py proves without a GPU that the checks fail wrong stand-ins and
that the cases reach every form the library reports).  Every case prints its `NUMERICS` lines (pytest -s);
profiles/numerics_margins.md holds the worst ratio per kernel and form.  The margin is C_CHAIN of tests/test_gpu_numerics.py:
operands lie on the storage grid and accumulation is f32, so bf16 storage and the split-f16 form are held to the f32 check."""
import ctypes

import pytest
import torch

import convse_cases as CC
import kernel_forms as DM
from test_gpu_kernels import DEV, dbg_lib, dev, ops  # noqa: F401  (ops, dbg_lib: fixtures)
from test_gpu_numerics import C_CHAIN

pytestmark = pytest.mark.gpu

WIDTH, OCCUPANCY, FILTER, RAGGED = CC.width_cases(), CC.occupancy_cases(), CC.filter_cases(), CC.ragged_cases()
INVERSION, RESCORE_INVERSION = CC.inversion_cases(), CC.rescore_inversion_cases()
BAND = (2, 16)


def ids(cases):
    return [c.id for c in cases]


class Dev(object):
    """a case's operands on the device in its storage form, and -- split-f16 -- the values the split rows really hold."""

    def __init__(self, ops, case, o, rescore=False):
        td = CC.TORCH_DT[case.dt]
        names = ("qn", "cn") if rescore else ("q", "f")
        if case.dt == "f16s":
            fixed = ops.F16_UNIT_LOG2 if rescore else None      # the re-score takes unit rows at the fixed scale
            self.a, self.b = ([ops.split_f16_rows(dev(x), fixed) for x in o[n]] for n in names)
            self.values = tuple([ops.unsplit_f16_rows(s).cpu() for s in t] for t in (self.a, self.b))
        else:
            self.a, self.b = ([dev(x, td) for x in o[n]] for n in names)
            self.values = None
        self.masks, self.cw, self.pair = [dev(m) for m in o["masks"]], dev(o["cw"]), dev(o["pair_vid"])


def k7_expected(case, o, d):
    if d.values is None:
        return CC.expected(case)
    return tuple(CC.reference(case, o, dt, q=d.values[0], f=d.values[1]) for dt in (torch.float64, torch.float32))


def rescore_expected(case, o, d):
    if d.values is None:
        return CC.expected_rescore(case)
    return tuple(CC.rescore_reference(case, o, dt, d.values[0], d.values[1]) for dt in (torch.float64, torch.float32))


def run_k7(ops, case, d, **kw):
    return ops.convse_rerank(d.a, d.b, d.masks, d.pair, d.cw, case.l_ref, case.merged, case.ksize, softmax=case.softmax, **kw)


def k7_and_check(ops, case, o, d=None):
    d = d or Dev(ops, case, o)
    st, ed = run_k7(ops, case, d)
    W, R = k7_expected(case, o, d)
    CC.check_k7("convse_rerank", case, o, st, ed, W, R, C_CHAIN)
    return d, st, ed, W, R


def evidence_and_check(ops, case, o, d, W, R):
    """span evidence on the same pairs, explicit and shuffled: logits BITWISE those of convse_rerank(softmax=False) --
    the contract of ops.span_evidence --, similarities against float64."""
    pq, pv, perm = CC.explicit_pairs(case, o)
    ev = ops.span_evidence(d.a, d.b, d.masks, dev(pq), dev(pv), d.cw, case.l_ref, case.merged, case.ksize)
    st, ed = ops.convse_rerank(d.a, d.b, d.masks, d.pair, d.cw, case.l_ref, case.merged, case.ksize, softmax=False)
    back = torch.empty_like(perm)
    back[perm] = torch.arange(perm.numel())
    k7_rows = lambda t: t.reshape(-1, case.lpad).cpu()                                  # noqa: E731
    ev_rows = lambda t: t.cpu()[back]                                                   # noqa: E731
    assert torch.equal(ev_rows(ev.st_logits), k7_rows(st)) and torch.equal(ev_rows(ev.ed_logits), k7_rows(ed)), \
        "span evidence logits differ from convse_rerank(softmax=False) on the same pairs"
    sh = lambda t: ev_rows(t).view(case.nq, case.kpairs, case.lpad)                     # noqa: E731
    sims = [sh(ev.video_similarity)] + ([sh(ev.sub_similarity)] if case.n_mod == 2 else [])
    CC.check_sims("span_evidence", case, o, dict(sims=sims, sim=sh(ev.similarity)), W, R, C_CHAIN)


def rescore_and_check(ops, case, o):
    """the width and occupancy lists carry a video without a valid clip in any modality (exactly float32(-1e10)) and, with two
    modalities, videos without one in the second or in the first only (exactly float32(-5e9)): asserted here to be listed, so
    that check_rescore's exact-fill assertions cannot go vacuous."""
    if case.list in ("width", "occupancy") and not case.extra.get("pairs"):
        cl = CC.rescore_classes(case, o)
        assert bool(cl["empty"].any()) and bool(cl["half"].any()) == (case.n_mod == 2)
    d = Dev(ops, case, o, rescore=True)
    got = ops.q2c_rescore(d.a, d.b, d.masks, d.pair)
    W, R = rescore_expected(case, o, d)
    CC.check_rescore("q2c_rescore " + case.rescore_form(), case, o, got, W, R, C_CHAIN)
    return d, got


def test_split_rows_hold_what_the_reference_is_given(ops):
    """the split-f16 cases are referred to the values the split rows hold (ops.unsplit_f16_rows), which are not the f32 rows
    they were made from: both planes are populated, the residual is below 2^-21 of the row maximum."""
    case = next(c for c in WIDTH if c.dt == "f16s")
    o = CC.operands(case)
    d = Dev(ops, case, o)
    for x, v in zip(o["f"], d.values[1]):
        rel = (v - x).abs().amax(-1) / x.abs().amax(-1)
        assert 0 < float(rel.max()) <= 2.0 ** -21


# ---- reduction width: every mainloop form and step count -----------------------------------------------------------------------
@pytest.mark.parametrize("case", WIDTH, ids=ids(WIDTH))
def test_reduction_width(ops, case):
    o = CC.operands(case)
    d, st, ed, W, R = k7_and_check(ops, case, o)
    evidence_and_check(ops, case, o, d, W, R)
    if not case.merged:
        rescore_and_check(ops, case, o)


# ---- chunk occupancy --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", OCCUPANCY, ids=ids(OCCUPANCY))
def test_chunk_occupancy(ops, case):
    """videos listed by 1, 15, 16, 17, 33, 48, 49, 63, 64, 65, 127, 128 and 129 pairs in ONE launch (row tiles of 16, the fast
    epilogue's groups of 8, chunks of 64 / 128), a launch without a listed pair, one video listed by every pair.  A pair's rows
    do not depend on its company: each query alone with its own pair list (every video listed once) gives the same bits."""
    o = CC.operands(case)
    d, st, ed, W, R = k7_and_check(ops, case, o)
    evidence_and_check(ops, case, o, d, W, R)
    dr, sc = rescore_and_check(ops, case, o)
    if case.extra.get("pairs") == "allskipped":
        return
    one = case.extra.get("pairs") == "onevideo"
    for q in range(case.nq):            # every query, so every row of every chunk
        pair1 = d.pair[q:q + 1, :1].contiguous() if one else d.pair[q:q + 1].contiguous()
        st1, ed1 = ops.convse_rerank(_rows(ops, d.a, q), d.b, d.masks, pair1, d.cw, case.l_ref, case.merged,
                                     case.ksize, softmax=case.softmax)
        sc1 = ops.q2c_rescore(_rows(ops, dr.a, q), dr.b, dr.masks, pair1)
        if one:                         # the one pair, listed alone, against each of the query's 13 listings of it
            st1, ed1, sc1 = st1.expand(1, case.kpairs, -1), ed1.expand(1, case.kpairs, -1), sc1.expand(1, case.kpairs)
        assert torch.equal(st[q], st1[0]) and torch.equal(ed[q], ed1[0]), "K7 rows of query %d depend on its company" % q
        assert torch.equal(sc[q], sc1[0]), "re-score of query %d depends on its company" % q


def _rows(ops, xs, q):
    """row q of every modality's query operand, as an operand of its own."""
    if isinstance(xs[0], ops.SplitRows):
        return [ops.SplitRows(x.data[q:q + 1].contiguous(), x.inv[q:q + 1].contiguous()) for x in xs]
    return [x[q:q + 1].contiguous() for x in xs]


# ---- filter width and row length ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FILTER, ids=ids(FILTER))
def test_filter_and_row_length(ops, case):
    """ksize 1 ... 15 (5: the fast epilogue; `band`: 5 through the general loop) x l_ref 1 ... 128 on rows of 16 ... 128, prefix
    masks, masks with holes, one valid clip, no valid clip; two unmerged streams with a mask each (f32) / merged (bf16)."""
    o = CC.operands(case)
    if not case.band:
        k7_and_check(ops, case, o)
        return
    d = Dev(ops, case, o)
    pair_w = torch.rand(case.nq, case.kpairs, generator=torch.Generator().manual_seed(case.seed)) + 0.1
    st, ed, summ = run_k7(ops, case, d, band=BAND, pair_w=dev(pair_w))
    W, R = k7_expected(case, o, d)
    CC.check_k7("convse_rerank band", case, o, st, ed, W, R, C_CHAIN)
    st5, ed5 = run_k7(ops, case, d)                   # the same rows through the fast epilogue: close, not bitwise (32- vs 64-lane sums)
    CC.check_k7("convse_rerank", case, o, st5, ed5, W, R, C_CHAIN)
    want = CC.host_summaries(st, ed, pair_w, case.l_ref, *BAND)
    assert torch.equal(summ.cpu(), want), "candidate summaries differ from their definition on the kernel's own rows"


# ---- ragged rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RAGGED, ids=ids(RAGGED))
def test_ragged_rows_vs_float64(ops, case):
    """vid_len 1, 3, 4, 5, 8, l_ref - 1, l_ref in one launch into NaN-filled rows: stored entries against float64, entries from
    the valid length on (rounded up to 4 by the fast epilogue's 16-byte stores) still NaN, in between 0 or NaN."""
    o = CC.operands(case)
    d = Dev(ops, case, o)
    vlen = o["vid_len"]
    nan = lambda: torch.full((case.nq, case.kpairs, case.lpad), float("nan"), device=DEV)      # noqa: E731
    st, ed = run_k7(ops, case, d, vid_len=dev(vlen), out=(nan(), nan()))
    W, R = k7_expected(case, o, d)
    lv = vlen[o["pair_vid"].long()][..., None]
    live = torch.arange(case.lpad)[None, None, :] < lv
    fast = DM.convse_epilogue("k7", case.ksize) == "fast"
    maybe = (torch.arange(case.lpad)[None, None, :] < (lv + 3) // 4 * 4) if fast else live
    assert bool((live.sum(-1) == lv[..., 0]).all()) and float(W["st"][~live].abs().max()) == 0.0
    stored = {}
    for nm, G in (("st", st), ("ed", ed)):
        G = G.cpu()
        assert bool(torch.isnan(G[~maybe]).all()), nm + ": an entry beyond the valid length was written"
        assert bool(((G[maybe & ~live] == 0) | torch.isnan(G[maybe & ~live])).all()), nm + ": non-zero behind the valid length"
        assert not bool(torch.isnan(G[live]).any()), nm + ": an entry inside the valid length was not written"
        stored[nm] = torch.where(live, G, torch.zeros_like(G))      # (float64 has exact zeros from the valid length on)
    CC.check_k7("convse_rerank vid_len", case, o, stored["st"], stored["ed"], W, R, C_CHAIN)


# ---- inversion paths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INVERSION, ids=ids(INVERSION))
def test_inversion_paths(ops, case):
    """one workgroup (pairs in registers / through the scratch), global counters, sub-counters: the smallest shapes on each
    side of every gate, all of one set of operands.  Each against float64; pairs (q, q % 257) sit in column 0 of every shape and
    have the same bits on every path (the first shape is the reference)."""
    o = CC.operands(case)
    d, st, ed, _, _ = k7_and_check(ops, case, o)
    ref = next(c for c in INVERSION if c.dt == case.dt)
    n = CC.INVERSION_COMMON
    if case is not ref:
        st0, ed0 = run_k7(ops, ref, Dev(ops, ref, CC.operands(ref)))
        assert torch.equal(st[:n, 0], st0[:n, 0]) and torch.equal(ed[:n, 0], ed0[:n, 0]), \
            "%s and %s disagree on the same pairs" % (case.k7_form(), ref.k7_form())


@pytest.mark.parametrize("dt", ["f32", "f16s"])
def test_rescore_inversion_paths(ops, dt):
    """the re-score always counts in global memory: 255 / 256 pairs on 2 videos straddle its sub-counter gate (split-f16:
    128-pair chunks).  Column 0 lists video q % 2 in both shapes: the same bits."""
    a, b = [c for c in RESCORE_INVERSION if c.dt == dt]
    (_, ga), (_, gb) = (rescore_and_check(ops, c, CC.operands(c)) for c in (a, b))
    n = min(a.nq, b.nq)
    assert torch.equal(ga[:n, 0], gb[:n, 0]), "%s and %s disagree on the same pairs" % (a.rescore_form(), b.rescore_form())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,change", CC.REFUSALS, ids=[w for w, _ in CC.REFUSALS])
def test_refused_shapes_write_nothing(ops, what, change):
    """XML_ERR_UNSUPPORTED from K7, span evidence and (where the shape concerns it) the re-score; NaN-filled destinations stay NaN."""
    s = dict(dict(nq=4, nv=3, kpairs=2, lpad=32, l_ref=29, hidden=32, ksize=5, dt="f32"), **change)
    nq, nv, k, lpad, h = s["nq"], s["nv"], s["kpairs"], s["lpad"], s["hidden"]
    g = torch.Generator().manual_seed(1)
    if s["dt"] == "f16s":       # (ops.split_f16_rows refuses the width itself: rows of the right size stand in)
        split = lambda *shape: ops.SplitRows(torch.zeros(*shape, dtype=torch.int32, device=DEV),      # noqa: E731
                                             torch.ones(*shape[:-1], device=DEV))
        q, f = [split(nq, h)], [split(nv, lpad, h)]
    else:
        q, f = [dev(torch.randn(nq, h, generator=g))], [dev(torch.randn(nv, lpad, h, generator=g))]
    masks, cw = [torch.ones(nv, lpad, device=DEV)], dev(torch.randn(2 * s["ksize"], generator=g))
    pair = dev(torch.randint(0, nv, (nq, k), generator=g).int())
    st, ed = (torch.full((nq, k, lpad), float("nan"), device=DEV) for _ in range(2))
    with pytest.raises(ops._lib.XmlHipError, match="unsupported shape"):
        ops.convse_rerank(q, f, masks, pair, cw, s["l_ref"], False, s["ksize"], softmax=False, out=(st, ed))
    torch.cuda.synchronize()
    assert bool(torch.isnan(st).all()) and bool(torch.isnan(ed).all()), "a refused launch wrote to its destination"
    with pytest.raises(ops._lib.XmlHipError, match="unsupported shape"):
        ops.span_evidence(q, f, masks, pair[:, 0].contiguous(), pair[:, 1].contiguous(), cw, s["l_ref"], False, s["ksize"])
    if DM.convse_mainloop("rescore", nq, lpad, lpad, h, 5, s["dt"]) == "refused":
        lib = ops._lib.load()
        out = torch.full((nq, k), float("nan"), device=DEV)
        ws = ops._workspace(lib.xml_q2c_rescore_workspace_bytes(nq, nv, k), out.device)
        status = lib.xml_q2c_rescore(1, ops._p(q[0]), None, ops._p(f[0]), None, ops._p(masks[0]), None, ops._p(pair), ops._p(out), nq,
                                     nv, k, lpad, h, DM.CONVSE_DT[s["dt"]], ops._p(ws), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert status == -2 and bool(torch.isnan(out).all())
    else:
        assert what in ("even ksize", "ksize 17", "l_ref > lpad")       # (no filter, no l_ref)


# ---- the two mainloops on the same shape (debug library) -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mainloop_twin(ops, dbg_lib, dt):
    """The widths the product gives to the LDS-DMA mainloop, run through the register-staged loop too (ablation 40 of the
    debug library) -- K7 logits, both epilogue inputs, and the re-score.
    gemm.h: both loops write the same LDS image (lds_slot_off; the DMA loop moves the swizzle into the global address), read
    the same fragments (slots c * 4 + fg, c = 0, 1) and issue Mma<T>::chunk(acc[m][n], fa[m], fb[n]) per step in the same
    order, steps ascending -- every accumulator sees the same MFMAs in the same K order (the staged loop's zero-filled tail
    does not occur at these widths, and the rows beyond a chunk's pairs, zero in one loop and a stand-in row in the other,
    are never read).  Hence: bit equality."""
    cases = [c for c in WIDTH if c.dt == dt and c.k7_form().startswith("dma")]
    assert len(cases) >= 3 * 4
    for case in cases:
        o = CC.operands(case)
        d, dr = Dev(ops, case, o), Dev(ops, case, o, rescore=True)
        res = []
        try:
            for abl in (0, 40):
                dbg_lib.xml_debug_set_q2c_ablation(ctypes.c_int(abl))
                res.append(run_k7(ops, case, d) + (ops.q2c_rescore(dr.a, dr.b, dr.masks, dr.pair),))
        finally:
            dbg_lib.xml_debug_set_q2c_ablation(ctypes.c_int(0))
        for a, b in zip(*res):
            assert torch.equal(a, b), "%s: the staged and the DMA mainloop disagree" % case.id
        W, R = CC.expected(case)
        CC.check_k7("convse_rerank staged-twin", case, o, res[1][0], res[1][1], W, R, C_CHAIN)
