"""Cases of the re-rank edge sweep (convse.hip: K7, span evidence, the exact-rank re-score), their operands, their float64 /
float32 references (oracle/f64.py: convse, q2c_rescore) and the checks the GPU test applies.  tests/test_gpu_convse_edges.py
runs every case on the GPU; tests/test_convse_cases_reference.py (no GPU) proves that the references agree with the oracle
and the CPU backend, that the checks fail deliberately wrong stand-ins, and -- asking the library's dispatch entries through
tests/kernel_forms.py -- that the cases reach every mainloop, inversion path, chunk size and epilogue.

What decides the path of a launch (tvretrieval_amd/csrc/dispatch.h, "K7 / span evidence / exact-rank re-score"):
  mainloop   rows of whole 128-byte K steps -> the LDS-DMA ring (two stages), else the register-staged loop, whose last step
             is zero-filled past the row's end;  steps = ceil(hidden * sizeof / 128)
  inversion  one workgroup (P <= 32 768 pairs on <= 4 096 videos; K7 and span evidence), global counters, 16 sub-counters
             per video from P >= 128 * nv
  chunk      a video's pairs in chunks of 64 (128: split-f16 re-score with P > 64 * nv); row tiles of 16 pairs are skipped,
             the fast epilogue walks rows in groups of 8
  epilogue   5 taps without summaries: half a wave per row, 4 clips per lane;  else one wave per row, 2 clips per lane

A case id names the forms the library reports for it."""
import functools

import torch
import torch.nn.functional as F

import kernel_forms as DM
import numerics_regimes as NR
from oracle import f64

TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16s": torch.float32}    # storage grid of the operand values
NEG = float(torch.tensor(-1e10, dtype=torch.float32))                              # mask_logits' fill as f32 holds it


class Case(object):
    def __init__(self, lst, dt, nq, nv, kpairs, lpad, l_ref, hidden, n_mod=1, merged=False, ksize=5, softmax=False, band=False,
                 tag="", seed=0, **extra):
        self.list, self.dt, self.nq, self.nv, self.kpairs, self.lpad, self.l_ref, self.hidden = lst, dt, nq, nv, kpairs, lpad, l_ref, hidden
        self.n_mod, self.merged, self.ksize, self.softmax, self.band, self.tag, self.seed = n_mod, merged, ksize, softmax, band, tag, seed
        self.extra = extra
        self.P = nq * kpairs
        self.n_conv = 1 if merged else n_mod

    def k7_form(self, entry="k7"):
        return DM.convse_form(self.nq, self.P, self.nv, self.lpad, self.l_ref, self.hidden, self.ksize, self.dt,
                              summ=self.band and entry == "k7", entry=entry)

    def rescore_form(self):
        return DM.rescore_form(self.nq, self.P, self.nv, self.lpad, self.hidden, self.dt)

    @property
    def streams(self):
        return "1" if self.n_mod == 1 else "2m" if self.merged else "2s"

    @property
    def id(self):
        form = self.rescore_form() if self.list == "inversion-rescore" else self.k7_form()
        return "-".join(str(x) for x in (self.list, self.dt, "h%d" % self.hidden, "s" + self.streams, "k%d" % self.ksize,
                                         "L%dof%d" % (self.l_ref, self.lpad), "P%dx%d" % (self.P, self.nv),
                                         "softmax" if self.softmax else "logits") + ((self.tag,) if self.tag else ()) + (form,))

    def __repr__(self):
        return self.id


# ---- the case lists ---------------------------------------------------------------------------------------------------------
# hidden 56 is ours: the only width that leaves 112 bytes (bf16) behind a whole step count; the others leave 16, 32, 48, 64, 80, 96
WIDTHS = (8, 24, 32, 40, 56, 64, 72, 96, 128, 136, 192, 200, 288, 320)
WIDTHS_F16S = (32, 96, 160)
STREAMS = ((1, False), (2, True), (2, False))


def width_cases():
    """every reduction width x storage type x stream form; 20 queries x 3 of 5 videos, 48-clip rows of which 40 exist."""
    return [Case("width", dt, 20, 5, 3, 48, 40, h, n_mod, merged, seed=h)
            for dt, hs in (("f32", WIDTHS), ("bf16", WIDTHS), ("f16s", WIDTHS_F16S)) for h in hs for n_mod, merged in STREAMS]


OCC_COUNTS = (1, 15, 16, 17, 33, 48, 49, 63, 64, 65, 127, 128, 129)
OCC_NQ = 129


def occupancy_cases():
    """one launch: column j of pair_vid lists video j for the first OCC_COUNTS[j] queries.  ksize 5: fast epilogue, 7: general.
    `nv27`: 14 more videos that nobody lists, so that P <= 64 * nv and the split-f16 re-score keeps its 64-pair chunks."""
    out = []
    for dt in ("f32", "bf16", "f16s"):
        for ks in (5, 7):
            out.append(Case("occupancy", dt, OCC_NQ, 13, 13, 32, 29, 64, 2, True, ks, seed=ks))
        out.append(Case("occupancy", dt, OCC_NQ, 27, 13, 32, 29, 64, 2, True, 5, tag="nv27", seed=3))
    out.append(Case("occupancy", "f32", OCC_NQ, 13, 13, 32, 29, 64, 1, False, 5, tag="allskipped", seed=4, pairs="allskipped"))
    out.append(Case("occupancy", "bf16", OCC_NQ, 13, 13, 32, 29, 64, 1, False, 5, tag="onevideo", seed=5, pairs="onevideo"))
    return out


FILTER_KS = (1, 3, 5, 7, 15)
ROW_LENGTHS = ((16, 1), (16, 3), (16, 4), (16, 5), (16, 16), (48, 33), (80, 64), (80, 65), (112, 97), (128, 113), (128, 127),
               (128, 128))
FILTER_NV = 9          # videos 0-3 prefix masks (0 full, 1 one clip), 4-7 masks with holes (4 full, 5 one clip), 8 all masked


def filter_cases():
    """filter widths x row lengths x softmax; f32 runs two unmerged streams with a mask each, bf16 the merged form.  hidden 72:
    the staged loop in both types.  `band`: ksize 5 through the general epilogue, with candidate summaries."""
    out = []
    for dt, n_mod, merged in (("f32", 2, False), ("bf16", 2, True)):
        for lpad, l_ref in ROW_LENGTHS:
            for ks in FILTER_KS:
                for softmax in (True, False):
                    out.append(Case("filter", dt, 6, FILTER_NV, FILTER_NV, lpad, l_ref, 72, n_mod, merged, ks, softmax, seed=lpad + l_ref + ks))
            out.append(Case("filter", dt, 6, FILTER_NV, FILTER_NV, lpad, l_ref, 72, n_mod, merged, 5, True, band=True, tag="band",
                            seed=lpad + l_ref))
    return out


def ragged_lens(l_ref):
    return (1, 3, 4, 5, 8, l_ref - 1, l_ref)


def ragged_cases():
    """vid_len per video in one launch (xml_convse_rerank_ex), probabilities; rows of 32 of 32 and 41 of 48 clips."""
    return [Case("ragged", dt, 5, 7, 7, lpad, l_ref, 64 if dt == "f32" else 72, 2, merged, ks, True, seed=ks + lpad)
            for dt, merged in (("f32", True), ("bf16", False)) for lpad, l_ref in ((32, 32), (48, 41)) for ks in (5, 15)]


# (nq, kpairs, nv): the smallest shapes on each side of every gate; 8 192 / 8 193 pairs: the one-workgroup kernel keeps up to
# 8 pairs per thread in registers
INVERSION_SHAPES = ((1024, 8, 4096), (2731, 3, 4096), (4096, 8, 4096), (3641, 9, 4096), (4096, 8, 4097), (2193, 15, 257), (257, 128, 257))
INVERSION_COMMON = 257        # query q lists video q % 257 in column 0 of every shape: the pairs compared across the paths
RESCORE_INVERSION_SHAPES = ((85, 3, 2), (64, 4, 2))


def inversion_cases():
    """lpad 16 and one 128-byte step per row (hidden 32 in f32, 64 in bf16) keep 33 000 pairs small."""
    return [Case("inversion", dt, nq, nv, k, 16, 13, h, 1, False, 5, seed=11) for dt, h in (("f32", 32), ("bf16", 64))
            for nq, k, nv in INVERSION_SHAPES]


def rescore_inversion_cases():
    return [Case("inversion-rescore", dt, nq, nv, k, 16, 13, 32, 2, False, seed=12)
            for dt in ("f32", "f16s") for nq, k, nv in RESCORE_INVERSION_SHAPES]


# (what, desc fields changed from a legal f32 / f16s shape): each must come back XML_ERR_UNSUPPORTED with nothing written
REFUSALS = (("even ksize", dict(ksize=4)), ("ksize 17", dict(ksize=17)), ("lpad % 16", dict(lpad=24, l_ref=20)),
            ("l_ref > lpad", dict(l_ref=33)), ("hidden % 8", dict(hidden=12)), ("f16s hidden % 32", dict(hidden=40, dt="f16s")))


def all_cases():
    return width_cases() + occupancy_cases() + filter_cases() + ragged_cases() + inversion_cases() + rescore_inversion_cases()


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _pad(mask, lpad):
    out = torch.zeros(mask.shape[0], lpad)
    out[:, :mask.shape[1]] = mask
    return out


# width, occupancy and inversion lists: videos without a valid clip -- in both streams, in the second only, in the first only
# (the last where there are more than five videos).  With one stream, or merged streams (the first mask counts), the second
# is an ordinary video.
EMPTY_BOTH, EMPTY_SECOND, EMPTY_FIRST = 2, 3, 5


def _masks(case, g):
    nv, l, lpad = case.nv, case.l_ref, case.lpad
    if case.list == "filter":
        m0 = torch.cat([NR.prefix_masks(4, l, case.seed), NR.hole_masks(4, l, case.seed), torch.zeros(1, l)])
        m1 = torch.cat([NR.hole_masks(4, l, case.seed + 1), NR.prefix_masks(4, l, case.seed + 1), torch.zeros(1, l)])
    elif case.list == "ragged":
        lens = torch.tensor(ragged_lens(l))
        m0 = (torch.arange(l)[None] < lens[:, None]).float()
        m1 = m0.clone()
        m0[4, 2] = 0                                        # a hole inside the valid length (vid_len 8)
        m1[5, 1:4] = 0
    else:
        m0, m1 = NR.prefix_masks(nv, l, case.seed), NR.hole_masks(nv, l, case.seed + 1)
        if nv > EMPTY_SECOND:                               # (the two-video re-score shapes have no room for them)
            m0[EMPTY_BOTH] = 0
            m1[EMPTY_BOTH] = 0
            m1[EMPTY_SECOND] = 0
        if nv > EMPTY_FIRST:
            m0[EMPTY_FIRST] = 0
    return [_pad(m0, lpad), _pad(m1, lpad)][:case.n_mod]


def _pairs(case, g):
    nq, nv, k = case.nq, case.nv, case.kpairs
    if case.list == "occupancy":
        kind = case.extra.get("pairs")
        if kind == "allskipped":
            return torch.full((nq, k), -1, dtype=torch.int32)
        if kind == "onevideo":
            return torch.full((nq, k), 7, dtype=torch.int32)
        pv = torch.arange(k).int()[None].repeat(nq, 1)
        pv[torch.arange(nq)[:, None] >= torch.tensor(OCC_COUNTS)[None]] = -1
        return pv
    if case.list.startswith("inversion"):
        pv = torch.randint(0, nv, (nq, k), generator=g).int()
        pv[:, 0] = (torch.arange(nq) % min(INVERSION_COMMON, nv)).int()
        pv[5::97, 1] = -1                                   # skipped pairs on every path
        return pv
    pv = torch.stack([torch.randperm(nv, generator=g)[:k] for _ in range(nq)]).int()
    if case.list == "width":
        pv[0, -1] = -1
        pv[3, 0] = nv                                       # outside [0, nv): skipped like -1
    return pv


@functools.lru_cache(maxsize=4)
def operands(case):
    """q, f: K7's operands on the storage grid (f32 tensors); qn, cn: unit rows for the re-score; masks, taps, pairs.  The
    inversion shapes share ONE set of operands (the largest), cut to each shape's rows, so that a pair means the same."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    td = TORCH_DT[case.dt]
    inv = {"inversion": INVERSION_SHAPES, "inversion-rescore": RESCORE_INVERSION_SHAPES}.get(case.list)
    nq = max(s[0] for s in inv) if inv else case.nq
    nv = max(s[2] for s in inv) if inv else case.nv
    h = case.hidden
    qr = [torch.randn(nq, h, generator=g) for _ in range(case.n_mod)]
    fr = [torch.randn(nv, case.lpad, h, generator=g) for _ in range(case.n_mod)]
    o = dict(q=[NR.grid(x, td)[:case.nq] for x in qr], f=[NR.grid(x * h ** -0.5, td)[:case.nv] for x in fr],
             qn=[NR.grid(F.normalize(x, dim=-1), td)[:case.nq] for x in qr],
             cn=[NR.grid(F.normalize(x, dim=-1), td)[:case.nv] for x in fr])
    if inv:                                                 # masks of the shared videos
        big = Case(case.list, case.dt, nq, nv, 1, case.lpad, case.l_ref, h, case.n_mod, seed=case.seed)
        o["masks"] = [m[:case.nv] for m in _masks(big, g)]
    else:
        o["masks"] = _masks(case, g)
    o["cw"] = 0.5 * torch.randn(2 * case.n_conv * case.ksize, generator=g)       # (random f32: off the bf16 grid)
    o["pair_vid"] = _pairs(case, torch.Generator().manual_seed(2000 + case.seed + case.nq))
    if case.list == "ragged":
        mk = torch.stack(o["masks"]).amax(0)
        o["vid_len"] = ((mk != 0).int() * torch.arange(1, case.lpad + 1).int()).amax(1).int()
    return o


def flat_pairs(case, o):
    """K7's pair p = (query p / kpairs, pair_vid[p])."""
    return torch.arange(case.nq).repeat_interleave(case.kpairs).int(), o["pair_vid"].reshape(-1)


def explicit_pairs(case, o):
    """the listed pairs as span evidence takes them: explicit (query, video) rows, shuffled; `perm` maps them to K7's rows."""
    pq, pv = flat_pairs(case, o)
    perm = torch.randperm(pq.numel(), generator=torch.Generator().manual_seed(case.seed))
    return pq[perm].contiguous(), pv[perm].contiguous(), perm


def reference(case, o, dtype, q=None, f=None, **over):
    """f64.convse on K7's pairs -> dict of (nq, kpairs, lpad) tensors (sims: list).  q / f: other operand VALUES (the unsplit
    split-f16 rows); over: l_ref / softmax / cw / masks of a deliberately wrong stand-in."""
    pq, pv = flat_pairs(case, o)
    r = f64.convse(q or o["q"], f or o["f"], over.get("masks", o["masks"]), pq, pv, over.get("cw", o["cw"]),
                   over.get("l_ref", case.l_ref), case.merged, case.ksize, over.get("softmax", case.softmax), dtype)
    sh = lambda t: t.view(case.nq, case.kpairs, case.lpad)      # noqa: E731
    return dict(st=sh(r["st"]), ed=sh(r["ed"]), sims=[sh(s) for s in r["sims"]], sim=sh(r["sim"]))


def rescore_reference(case, o, dtype, qn=None, cn=None):
    return f64.q2c_rescore(qn or o["qn"], cn or o["cn"], o["masks"], o["pair_vid"], dtype)


@functools.lru_cache(maxsize=4)
def expected(case):
    """(W, R) of K7 on the case's own operand values: float64, and the same code in float32."""
    o = operands(case)
    return reference(case, o, torch.float64), reference(case, o, torch.float32)


@functools.lru_cache(maxsize=4)
def expected_rescore(case):
    o = operands(case)
    return rescore_reference(case, o, torch.float64), rescore_reference(case, o, torch.float32)


# ---- entry classes and the checks -------------------------------------------------------------------------------------------
def classes(case, o):
    """(nq, kpairs, lpad) bool masks: ok pairs; entries inside l_ref that every stream keeps (`valid`), that every stream masks
    (`dead`), that some but not all mask (`part`); `beyond` l_ref; pairs of videos without an unmasked clip in any stream
    (`empty`) or in some but not all streams (`half`)."""
    pv = o["pair_vid"].long()
    ok = (pv >= 0) & (pv < case.nv)
    mk = torch.stack([m[pv.clamp(0, case.nv - 1)] != 0 for m in o["masks"][:case.n_conv]])       # (n_conv, nq, k, lpad)
    inside = (torch.arange(case.lpad) < case.l_ref)[None, None, :] & ok[..., None]
    valid, dead = mk.all(0) & inside, ~mk.any(0) & inside
    has = (mk & inside).any(-1)                                                                 # (n_conv, nq, k)
    return dict(ok=ok, valid=valid, dead=dead, part=inside & ~valid & ~dead, beyond=~inside & ok[..., None],
                empty=ok & ~has.any(0), half=ok & has.any(0) & ~has.all(0))


def rescore_classes(case, o):
    """`classes` as the re-score sees the case: every modality with its own mask, all lpad clips."""
    return classes(Case(case.list, case.dt, case.nq, case.nv, case.kpairs, case.lpad, case.lpad, case.hidden, case.n_mod), o)


def check_k7(name, case, o, st, ed, W, R, c, storage=None):
    """What tests/test_gpu_convse_edges.py asserts on K7's rows (and the CPU test on wrong stand-ins).  Logits: check_f32 on
    the entries every stream keeps; -1e10 exactly where every stream masks, -5e9 exactly where one of two unmerged streams does
    (f32 absorbs the other stream's logit, |x| < 512, in the fill before the halving).  Probabilities: check_f32 at scale 1 and
    check_prob_rows on every row of a listed pair, exact zeros on masked clips, the uniform row of a video without a valid clip.
    Entries l >= l_ref and the rows of skipped pairs: exactly 0.  Returns the worst kernel_err / ref_err ratio."""
    cl = classes(case, o)
    storage = storage or case.dt
    worst = 0.0
    for nm, G in (("st", st), ("ed", ed)):
        G, Wn, Rn = G.detach().float().cpu(), W[nm], R[nm]
        what = "%s %s" % (name, nm)
        assert bool((G[~cl["ok"]] == 0).all()), what + ": the rows of skipped pairs must be zero"
        assert bool((G[cl["beyond"]] == 0).all()), what + ": entries l >= l_ref must be exactly 0"
        if not bool(cl["ok"].any()):
            continue
        if case.softmax:
            rows = lambda t: t[cl["ok"]][:, :case.l_ref]      # noqa: E731
            kerr, ref_err = NR.check_f32(what, case.id, rows(G), rows(Wn), rows(Rn), c, scale=1.0, storage=storage)
            gone = (cl["dead"] | cl["part"]) & ~cl["empty"][..., None]
            assert bool((G[gone] == 0).all()), what + ": masked clips must be exactly 0"
            NR.check_prob_rows(what, case.id, rows(G), rows(Wn), c * ref_err + NR.FLOOR_ULPS * 2 * NR.F32_ULP)
            if bool(cl["empty"].any()):
                u = G[cl["empty"]][:, :case.l_ref]
                assert bool((u == u[:, :1]).all()) and float((u.double() - 1.0 / case.l_ref).abs().max()) <= 2.0 ** -23, \
                    what + ": a video without a valid clip has the uniform distribution over l_ref"
        else:
            assert bool(cl["valid"].any())
            kerr, ref_err = NR.check_f32(what, case.id, G[cl["valid"]], Wn[cl["valid"]], Rn[cl["valid"]], c, storage=storage)
            assert bool((G[cl["dead"]] == NEG).all()), what + ": masked logits must be float32(-1e10) exactly"
            assert bool((G[cl["part"]] == 0.5 * NEG).all()), what + ": a clip one of two streams masks must be float32(-5e9)"
        worst = max(worst, kerr / ref_err if ref_err > 0 else float("inf") if kerr > 0 else 0.0)
    return worst


def check_rescore(name, case, o, got, W, R, c, storage=None):
    """re-score: -inf for skipped pairs; float32(-1e10) exactly for a video without a valid clip in any modality, float32(-5e9)
    exactly for one that has none in one of two (the other modality's maximum, at most 1, is absorbed by the fill before the
    halving -- the float32 reference's own behaviour; float64 keeps it); check_f32 at scale 1 on every other listed pair."""
    cl = rescore_classes(case, o)
    G = got.detach().float().cpu()
    assert bool((G[~cl["ok"]] == float("-inf")).all()), name + ": skipped pairs must score -inf"
    if not bool(cl["ok"].any()):
        return 0.0
    assert bool((G[cl["empty"]] == NEG).all()), name + ": a video without a valid clip scores float32(-1e10) exactly"
    assert bool((G[cl["half"]] == 0.5 * NEG).all()), name + ": a video one of two modalities has no clip of scores float32(-5e9)"
    rest = cl["ok"] & ~cl["half"]
    kerr, ref_err = NR.check_f32(name, case.id, G[rest], W[rest], R[rest], c, scale=1.0, storage=storage or case.dt)
    return kerr / ref_err if ref_err > 0 else float("inf") if kerr > 0 else 0.0


def check_sims(name, case, o, got, W, R, c, storage=None):
    """span evidence: per-stream and mean similarities (unmasked), zero beyond l_ref and on skipped pairs."""
    cl = classes(case, o)
    inside = (torch.arange(case.lpad) < case.l_ref)[None, None, :] & cl["ok"][..., None]
    worst = 0.0
    for nm, G, Wn, Rn in [("sim%d" % m, got["sims"][m], W["sims"][m], R["sims"][m]) for m in range(case.n_mod)] + \
            [("sim", got["sim"], W["sim"], R["sim"])]:
        G = G.detach().float().cpu()
        assert bool((G[~inside] == 0).all()), "%s %s: entries beyond l_ref / of skipped pairs must be 0" % (name, nm)
        if not bool(inside.any()):
            continue
        kerr, ref_err = NR.check_f32("%s %s" % (name, nm), case.id, G[inside], Wn[inside], Rn[inside], c, storage=storage or case.dt)
        worst = max(worst, kerr / ref_err if ref_err > 0 else float("inf") if kerr > 0 else 0.0)
    return worst


def host_summaries(st, ed, pair_w, l_ref, min_l, max_l):
    """ConvseArgs' definition of the candidate summaries, in float32 from the rows themselves: summ[p][g] = the largest
    (st[i] * w[p]) * max_{min_l <= d < max_l, i + d < l_ref} ed[i + d] over the rows i < l_ref with i % 64 in [8 g, 8 g + 8)
    (never below 0)."""
    st, ed = st.float().cpu(), ed.float().cpu()
    nq, k, lpad = st.shape
    w = torch.ones(nq, k) if pair_w is None else pair_w.float().cpu()
    e = torch.zeros(nq, k, lpad + max_l)
    e[..., :l_ref] = ed[..., :l_ref]
    win = torch.stack([e[..., d:d + lpad] for d in range(min_l, max_l)]).amax(0)
    m = (st * w[..., None]) * win
    m[..., l_ref:] = 0
    m = m.clamp_min(0)
    out = torch.zeros(nq, k, 8)
    for g in range(8):
        cols = [i for i in range(lpad) if 8 * g <= i % 64 < 8 * g + 8]
        if cols:                                            # (rows shorter than 64 clips leave the upper groups at 0)
            out[..., g] = m[..., cols].amax(-1)
    return out
