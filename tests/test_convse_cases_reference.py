"""The re-rank edge sweep without a GPU (cases, references and checks: tests/convse_cases.py):
* the float64 references of oracle/f64.py (convse, q2c_rescore) agree with the oracle's span head restated on the dense
  (query, video, clip) tensor and with tests/cpu_backend.py, to float32 accuracy, on every case -- and every case has a float32
  reference error above zero, so that check_f32's allowance is never its bare floor;
* the checks of the GPU test fail deliberately wrong stand-ins (float32 evaluations with one defect each);
* asked through the dispatch entries, the cases reach every form the library can answer with."""
import pytest
import torch
import torch.nn.functional as F

import convse_cases as CC
import kernel_forms as DM
import numerics_regimes as NR
from cpu_backend import CpuOps
from oracle import xml_oracle as O
from test_gpu_numerics import C_CHAIN

ALL = CC.all_cases()
K7_CASES = [c for c in ALL if c.list != "inversion-rescore"]
SMALL = [c for c in K7_CASES if c.P <= 2000]
F32_TOL = 64 * NR.F32_ULP       # "to float32 accuracy": two float32 evaluations of <= 320-term sums, in units of the output scale


def _close(name, a, b, scale):
    err = float((a.double() - b.double()).abs().max()) / scale
    assert err <= F32_TOL, "%s: %.3e of the output scale" % (name, err)


def _oracle_dense(case, o):
    """get_merged_st_ed_prob / _get_st_ed_prob (cross=True) restated on given query vectors: every query against every clip of
    every video, the rows of the listed pairs taken afterwards.  ksize 5 and l_ref == what the reference calls L."""
    l = case.l_ref
    sims = [torch.einsum("md,nld->mnl", o["q"][m], o["f"][m][:, :l]) for m in range(case.n_mod)]
    cw = o["cw"].view(2, case.n_conv, 1, 1, case.ksize)
    conv = lambda x, w: F.conv1d(x.reshape(-1, 1, l), w, padding=case.ksize // 2).view(case.nq, case.nv, l)      # noqa: E731
    mk = [m[:, :l].unsqueeze(0) for m in o["masks"]]
    if case.merged:
        x = (sims[0] + sims[1]) / 2
        st, ed = O.mask_logits(conv(x, cw[0, 0]), mk[0]), O.mask_logits(conv(x, cw[1, 0]), mk[0])
    else:
        st = sum(O.mask_logits(conv(sims[m], cw[0, m]), mk[m]) for m in range(case.n_mod)) / case.n_mod
        ed = sum(O.mask_logits(conv(sims[m], cw[1, m]), mk[m]) for m in range(case.n_mod)) / case.n_mod
    if case.softmax:
        st, ed = torch.softmax(st, -1), torch.softmax(ed, -1)
    pv = o["pair_vid"].long()
    ok = (pv >= 0) & (pv < case.nv)
    rows = torch.arange(case.nq).unsqueeze(1)
    out = []
    for t in (st, ed):
        r = torch.zeros(case.nq, case.kpairs, case.lpad)
        r[..., :l] = t[rows, pv.clamp(0, case.nv - 1)]
        r[~ok] = 0
        out.append(r)
    return out


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_references_agree(case):
    o = CC.operands(case)
    W, R = CC.expected(case)
    cl = CC.classes(case, o)
    sel = cl["ok"][..., None].expand_as(cl["valid"]) if case.softmax else cl["valid"]
    if not bool(cl["ok"].any()):
        assert float(W["st"].abs().max()) == 0.0
        return
    scale = 1.0 if case.softmax else float(W["st"][sel].abs().max())
    pv = o["pair_vid"].clone()
    pv[pv >= case.nv] = -1                                           # (the CPU backend knows -1 only)
    cst, ced = CpuOps.convse_rerank(o["q"], o["f"], o["masks"], pv, o["cw"], case.l_ref, case.merged, case.ksize, softmax=case.softmax)
    for nm, got in (("st", cst), ("ed", ced)):
        _close("cpu_backend " + nm, got[sel], W[nm][sel], scale)
        _close("float32 twin " + nm, R[nm][sel], W[nm][sel], scale)
        # (a softmax over ONE clip is the value 1 in every arithmetic: there the floor is all the check may allow)
        assert float((R[nm][sel].double() - W[nm][sel]).abs().max()) > 0 or (case.softmax and case.l_ref == 1), \
            "float32 reference error is zero: check_f32 would be its bare floor"
    if case.ksize == 5:
        for nm, got in zip(("st", "ed"), _oracle_dense(case, o)):
            _close("oracle restated " + nm, got[sel], W[nm][sel], scale)
    if not case.softmax:        # masked entries carry the fill exactly, in every evaluation
        for t in (cst, R["st"], W["st"].float()):
            assert bool((t[cl["dead"]] == CC.NEG).all())
    _rescore_references_agree(case, o, pv)      # the re-score on the same case


def _rescore_references_agree(case, o, pv):
    Wr, Rr = CC.expected_rescore(case)
    cr = CpuOps.q2c_rescore(o["qn"], o["cn"], o["masks"], pv)
    cl = CC.rescore_classes(case, o)
    ok, rest = cl["ok"], cl["ok"] & ~cl["half"]
    _close("cpu_backend re-score", cr[rest], Wr[rest], 1.0)
    _close("float32 twin re-score", Rr[rest], Wr[rest], 1.0)
    assert bool((Wr[~ok] == float("-inf")).all()) and bool((cr[~ok] == float("-inf")).all())
    assert float((Rr[rest].double() - Wr[rest]).abs().max()) > 0, "float32 re-score reference error is zero"
    for t in (cr, Rr):          # the fills, exactly, in every float32 evaluation (float64 keeps the other modality's half)
        assert bool((t[cl["empty"]] == CC.NEG).all()) and bool((t[cl["half"]] == 0.5 * CC.NEG).all())
    assert bool((Wr[cl["empty"]] == CC.NEG).all()) and float((Wr[cl["half"]] - 0.5 * CC.NEG).abs().max() if cl["half"].any() else 0) <= 0.5
    return cl


RESCORE_INV = [c for c in ALL if c.list == "inversion-rescore"]


@pytest.mark.parametrize("case", RESCORE_INV, ids=[c.id for c in RESCORE_INV])
def test_rescore_references_agree_on_its_inversion_shapes(case):
    o = CC.operands(case)
    _rescore_references_agree(case, o, o["pair_vid"])


def test_the_lists_hold_videos_without_a_valid_clip():
    """width and occupancy: a video empty in both streams, one empty in the second only (and, occupancy, in the first only),
    each listed -- so that the exact-fill assertions of check_k7 and check_rescore are not vacuous."""
    for case in [c for c in ALL if c.list in ("width", "occupancy") and not c.extra.get("pairs")]:
        cl = CC.rescore_classes(case, CC.operands(case))
        assert bool(cl["empty"].any()), case.id
        assert bool(cl["half"].any()) == (case.n_mod == 2), case.id
        k7 = CC.classes(case, CC.operands(case))
        assert bool(k7["dead"].any()) and bool(k7["part"].any()) == (case.streams == "2s"), case.id


BIG = [c for c in ALL if c.P > 2000]
BIG_SAMPLE = 48       # queries the CPU backend (a loop over queries) is run on


@pytest.mark.parametrize("case", BIG, ids=[c.id for c in BIG])
def test_references_agree_on_the_inversion_shapes(case):
    """33 000 pairs: the float32 twin on all of them, the CPU backend on the first queries, the reference error above zero."""
    o = CC.operands(case)
    cl = CC.classes(case, o)
    W, R = CC.expected(case)
    n = BIG_SAMPLE
    cpu = CpuOps.convse_rerank([q[:n] for q in o["q"]], o["f"], o["masks"], o["pair_vid"][:n], o["cw"], case.l_ref, case.merged,
                               case.ksize, softmax=case.softmax)
    for nm, got in zip(("st", "ed"), cpu):
        v = cl["valid"]
        scale = float(W[nm][v].abs().max())
        _close("float32 twin " + nm, R[nm][v], W[nm][v], scale)
        _close("cpu_backend " + nm, got[v[:n]], W[nm][:n][v[:n]], scale)
        assert float((R[nm][v].double() - W[nm][v]).abs().max()) > 0


def test_shared_operands_of_the_inversion_shapes():
    """the same (query, video) pair means the same operands on both sides of every gate."""
    a, b = [c for c in ALL if c.list == "inversion"][:2]
    oa, ob = CC.operands(a), CC.operands(b)
    n = min(a.nq, b.nq)
    assert torch.equal(oa["q"][0][:n], ob["q"][0][:n]) and torch.equal(oa["f"][0][:257], ob["f"][0][:257])
    assert torch.equal(oa["masks"][0][:257], ob["masks"][0][:257]) and torch.equal(oa["cw"], ob["cw"])
    assert torch.equal(oa["pair_vid"][:257, 0], ob["pair_vid"][:257, 0])


# ---- the checks have teeth --------------------------------------------------------------------------------------------------
def _first(lst, pred):
    return next(c for c in ALL if c.list == lst and pred(c))


def _flip_taps(case, o):
    return o["cw"].view(-1, case.ksize).flip(1).reshape(-1)


def _whole_steps(case, ts):
    es = 2 if case.dt == "bf16" else 4
    keep = case.hidden * es // DM.CONVSE_STEP_BYTES * DM.CONVSE_STEP_BYTES // es
    return [t[..., :keep] for t in ts]


def _chunk_last_row_is_row0(case, o, t):
    """the last pair row of every chunk (a video's listed pairs in query order, 64 per chunk) replaced by the chunk's row 0"""
    t = t.clone()
    pv = o["pair_vid"]
    for j in range(case.kpairs):
        rows = torch.nonzero(pv[:, j] >= 0).reshape(-1)
        for c0 in range(0, rows.numel(), DM.CONVSE_TM):
            ch = rows[c0:c0 + DM.CONVSE_TM]
            t[ch[-1], j] = t[ch[0], j]
    return t


def _softmax_over_lpad(case, t):
    p = torch.softmax(t, -1)
    p[..., case.l_ref:] = 0
    return p


WRONG_K7 = {
    "taps reversed": ("filter", lambda c: c.ksize == 7 and not c.softmax and c.l_ref == 33,
                      lambda c, o: CC.reference(c, o, torch.float32, cw=_flip_taps(c, o))),
    "zero padding taken at lpad instead of l_ref": ("filter", lambda c: c.ksize == 5 and not c.softmax and (c.lpad, c.l_ref) == (16, 5),
                                                    lambda c, o: _cut(c, CC.reference(c, o, torch.float32, l_ref=c.lpad))),
    "mask applied before the filter": ("filter", lambda c: c.ksize == 3 and not c.softmax and c.l_ref == 64 and c.dt == "bf16",
                                       lambda c, o: CC.reference(c, o, torch.float32, f=[x * o["masks"][0][..., None] for x in o["f"]])),
    "K tail past the last whole step dropped": ("width", lambda c: c.dt == "bf16" and c.hidden == 72 and c.n_mod == 1,
                                                lambda c, o: CC.reference(c, o, torch.float32, q=_whole_steps(c, o["q"]),
                                                                          f=_whole_steps(c, o["f"]))),
    "last pair row of a chunk replaced by row 0's": ("occupancy", lambda c: c.dt == "f32" and c.ksize == 5 and not c.tag,
                                                     lambda c, o: {k: _chunk_last_row_is_row0(c, o, v) for k, v in CC.expected(c)[1].items()
                                                                   if k in ("st", "ed")}),
    "1 / n_mod omitted": ("width", lambda c: c.dt == "f32" and c.hidden == 96 and c.streams == "2s",
                          lambda c, o: {k: torch.where(CC.classes(c, o)["valid"], 2 * v, v) for k, v in CC.expected(c)[1].items()
                                        if k in ("st", "ed")}),
    "softmax over lpad": ("filter", lambda c: c.ksize == 5 and c.softmax and not c.band and (c.lpad, c.l_ref) == (80, 65),
                          lambda c, o: {k: _softmax_over_lpad(c, v) for k, v in CC.reference(c, o, torch.float32, softmax=False).items()
                                        if k in ("st", "ed")}),
    "second stream overwrites instead of accumulating": ("width", lambda c: c.dt == "bf16" and c.hidden == 64 and c.streams == "2m",
                                                         lambda c, o: CC.reference(c, o, torch.float32,
                                                                                   f=[torch.zeros_like(o["f"][0]), o["f"][1]])),
}


def _cut(case, r):
    for k in ("st", "ed"):
        r[k] = r[k].clone()
        r[k][..., case.l_ref:] = 0
    return r


@pytest.mark.parametrize("bug", sorted(WRONG_K7))
def test_k7_check_fails_wrong_stand_ins(bug):
    lst, pred, make = WRONG_K7[bug]
    case = _first(lst, pred)
    o = CC.operands(case)
    W, R = CC.expected(case)
    CC.check_k7("float32 reference", case, o, R["st"], R["ed"], W, R, C_CHAIN)          # the honest evaluation passes
    bad = make(case, o)
    with pytest.raises(AssertionError):
        CC.check_k7(bug, case, o, bad["st"], bad["ed"], W, R, C_CHAIN)


def test_rescore_check_fails_wrong_stand_ins():
    case = _first("width", lambda c: c.dt == "f32" and c.hidden == 72 and c.n_mod == 2)
    o = CC.operands(case)
    W, R = CC.expected_rescore(case)
    CC.check_rescore("float32 reference", case, o, R, W, R, C_CHAIN)
    ok = CC.classes(case, o)["ok"]
    bad = {"1 / n_mod omitted": torch.where(ok, 2 * R, R),
           "K tail dropped": CC.rescore_reference(case, o, torch.float32, _whole_steps(case, o["qn"]), _whole_steps(case, o["cn"])),
           "second stream overwrites": CC.rescore_reference(case, o, torch.float32, cn=[torch.zeros_like(o["cn"][0]), o["cn"][1]]),
           "skipped pairs left at 0": torch.where(ok, R, torch.zeros_like(R))}
    occ = _first("occupancy", lambda c: c.dt == "f32" and c.ksize == 5 and not c.tag)
    oo = CC.operands(occ)
    Wo, Ro = CC.expected_rescore(occ)
    for name, t in bad.items():
        with pytest.raises(AssertionError):
            CC.check_rescore(name, case, o, t, W, R, C_CHAIN)
    with pytest.raises(AssertionError):
        CC.check_rescore("last row of a chunk", occ, oo, _chunk_last_row_is_row0(occ, oo, Ro), Wo, Ro, C_CHAIN)


@pytest.mark.parametrize("lpad,l_ref", [(80, 70), (16, 5), (128, 128)])
def test_host_summaries_follow_the_definition(lpad, l_ref):
    """the host restatement used for the band= cases against a plain loop over (start, length)."""
    g = torch.Generator().manual_seed(0)
    st, ed, w = torch.rand(2, 3, lpad, generator=g), torch.rand(2, 3, lpad, generator=g), torch.rand(2, 3, generator=g)
    lo, hi = 2, 16
    got = CC.host_summaries(st, ed, w, l_ref, lo, hi)
    want = torch.zeros(2, 3, 8)
    for q in range(2):
        for k in range(3):
            for i in range(l_ref):
                best = max([float(ed[q, k, i + d]) for d in range(lo, hi) if i + d < l_ref] or [0.0])
                v = float((st[q, k, i] * w[q, k]) * torch.tensor(best))
                grp = (i % 64) // 8
                want[q, k, grp] = max(float(want[q, k, grp]), v)
    assert torch.equal(got, want)


# ---- the plan: every answer of the dispatch entries is reached ----------------------------------------------------------------
def test_every_form_is_reached_and_no_case_is_refused():
    k7 = [c.k7_form() for c in K7_CASES]
    ev = [c.k7_form("evidence") for c in K7_CASES if c.list in ("width", "occupancy")]
    rs = [(c.dt, c.rescore_form()) for c in ALL if c.list in ("width", "occupancy", "inversion-rescore")]
    assert "refused" not in k7 + ev + [f for _, f in rs]
    by_dt = lambda dt: [f for c, f in zip(K7_CASES, k7) if c.dt == dt]      # noqa: E731
    for dt in ("f32", "bf16"):
        forms = by_dt(dt)
        assert any(f.startswith("staged") for f in forms) and any(f.startswith("dma") for f in forms), dt
        assert {s for s in (1, 2, 3, 5) if any(f.startswith("dma%d-" % s) for f in forms)} >= ({1, 2, 3} if dt == "f32" else {1, 2, 3, 5})
        assert any(f.startswith("staged") for d, f in rs if d == dt) and any(f.startswith("dma1-") for d, f in rs if d == dt)
    tails = {int(f.split("+tail")[1].split("-")[0]) for f in k7 if "+tail" in f}
    assert tails >= {16, 32, 48, 64, 112}, tails
    assert all(f.startswith("dma") for f in by_dt("f16s")) and by_dt("f16s")
    for what in ("one-workgroup", "global", "sub"):
        assert any(f.endswith(what) for f in k7), what
    assert any(f.endswith("global") for _, f in rs) and any(f.endswith("sub") for _, f in rs)
    for epi in ("-fast-", "-general-"):
        assert any(epi in f for f in k7) and any(epi in f for f in ev), epi
        for dt in ("f32", "bf16"):
            assert any(epi in f for f in by_dt(dt)), (epi, dt)
    for chunk in ("chunk64", "chunk128"):
        assert any(chunk in f for d, f in rs if d == "f16s"), chunk
    assert not any("chunk128" in f for d, f in rs if d != "f16s")
    # the gates are straddled by neighbouring shapes
    assert {c.dt for c in ALL if c.list == "inversion" and c.k7_form().startswith("dma1-")} == {"f32", "bf16"}
    inv = {(c.P, c.nv): DM.convse_inversion("k7", c.P, c.nv) for c in ALL if c.list == "inversion"}
    P, NV, PER = DM.CONVSE_SMALL_P, DM.CONVSE_SMALL_NV, DM.CONVSE_SUB_MIN_PAIRS_PER_VIDEO
    assert inv[(P, NV)] == "one-workgroup" and inv[(P + 1, NV)] == "global" and inv[(P, NV + 1)] == "global"
    assert inv[(PER * 257 - 1, 257)] == "global" and inv[(PER * 257, 257)] == "sub"
    rinv = {c.P: DM.convse_inversion("rescore", c.P, c.nv) for c in ALL if c.list == "inversion-rescore"}
    assert rinv == {PER * 2 - 1: "global", PER * 2: "sub"}
    # chunk occupancy: every count of the list, in one launch; the launch bound covers its chunks
    occ = _first("occupancy", lambda c: not c.tag)
    cnt = (CC.operands(occ)["pair_vid"] >= 0).sum(0).tolist()
    assert tuple(cnt) == CC.OCC_COUNTS
    assert sum(DM.cdiv(n, DM.CONVSE_TM) for n in cnt) <= DM.convse_max_chunks("k7", occ.P, occ.nv)
    # the refusal list is refused, for K7 and span evidence alike
    base = dict(nq=4, lpad=32, l_ref=29, hidden=32, ksize=5, dt="f32")
    for what, change in CC.REFUSALS:
        s = dict(base, **change)
        for entry in ("k7", "evidence"):
            assert DM.convse_mainloop(entry, s["nq"], s["lpad"], s["l_ref"], s["hidden"], s["ksize"], s["dt"]) == "refused", what
