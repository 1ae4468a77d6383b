"""Cases of tests/test_gpu_train_tail.py: the f32 "serial middle" of the training step (PairSimFn, SpanLossFn, RankLossFn,
VideoLevelScoresFn's arg-kept backward) and the optimizer kernels (xml_bert_adam_step, xml_clip_grad_norm) at every loop edge,
with their references --
W  float64 autograd of the plain function (oracle/f64.py `train_*`),
R  float32 autograd of the same function on the CPU (what correct f32 arithmetic costs at these operands),
S  for the bf16 PairSimFn only: the float64 value with the bf16 stores of dq / df2 modelled (takes R's place for those two).
No GPU is needed: tests/test_numerics_reference.py checks the tables' own conditions and runs the checks of this module on CPU
restatements of wrong kernels.  References are computed once per case (`refs`).

Which case reaches which branch (csrc/train.hip, csrc/loss_tail.hip):

pair_sim_bwd_vec_kernel / pair_sim_bwd_kernel           (n, L, H)
  L < 4: waves 1.. / 3.. hold no clip                    (3, 1, 8), (2, 3, 64)
  c0 += 64 chunk loop, second pass with 63 idle lanes    (5, 21, 520)   chunks = 65
  s_acc at its limit hidden = 2048                       (2, 17, 2048)
  scalar kernel: hidden > 2048                           (2, 5, 2056)
  scalar kernel: hidden % 8 != 0                         (3, 7, 100)
  l0 += 16 loop taken 8 times, one row                   (1, 128, 128)
  n L % 4 != 0: pair_sim_kernel's last workgroup partial (3, 1, 8), (2, 3, 64), (5, 21, 520), (2, 17, 2048), (2, 5, 2056), (3, 7, 100)
span_loss_kernel                                         SPAN_SHAPES (n, L, ks) x forms merged / split n_sim 2 / n_sim 1
  h = 1 half (lanes + 64): logits, softmax, target, DC   L = 65, 100, 127, 128; targets >= 64: row 0's end (L - 1), row 3's start (64)
  the h = 1 half empty / one lane short of it            L = 1, 3, 63, 64
  ks = 1 (no halo), 3, 5, 31 (halo 15 of 16)             ks = 31 at L = 3 (every tap but the middle ones off the row) and L = 128
  last workgroup partial (n % 4 != 0), one row           n = 1, 5, 9;  n = 4: full
  mask0 != mask1 (split, n_sim 2)                        L in SPAN_TWO_MASKS
  rows of length 1, targets at clip 0 / the last clip    rows 1, 0 / 0 and 2 of every case (n permitting)
  one fill vs three fills of dsim0 | dsim1 | dconv_w     tests/test_gpu_train_tail.py calls both layouts for n_sim = 2
rank_loss_kernel                                         n in RANK_NS x hinge / lse, plus RANK_TIES
  row loop j += 256 taken 0, 1, 2, 3, 4 times            n = 2, 17, 255, 256 | 257, 600 (3 passes) | 1024 (4 passes, the LDS row full)
  ranks 1 and n - 1                                      rows 0 and 1 of every case
  equal values: lower index first                        grid 1/8, -1e10 column block, wanted ranks first / inside / last in a group
  ties across j = 255 | 256                              "straddle" cases: columns / rows 253 .. 256 equal
  n = 1025 refused                                       tests/test_gpu_train_tail.py
q2c_scores_arg_kernel + q2c_l2_bwd_kernel                SCORES_SHAPES (nq, nv, L, H)
  lpad 32 (vpt 4)                                        (7, 7, 19, 128)
  lpad 48, 80, 112: dead columns in the 128-column tile  (9, 5, 37, 64), (6, 3, 70, 64), (5, 3, 100, 768)
  nq > 128: second query tile; vpt 8, nv % vpt != 0      (130, 11, 16, 64)
  nq > 256: collect_active's second pass, context side   (260, 4, 5, 8)
  nv > 256: collect_active's second pass, query side     (3, 260, 9, 16)
  hidden > 512: second chunk per lane, context side      (5, 3, 100, 768), (4, 4, 128, 520)
  first clip on exact ties, in one tile / across tiles   SCORES_TIES
adam_norm_partial_kernel / adam_norm_reduce_kernel / adam_norm_kernel / adam_update_kernel      `adam_layout`
  reduce stride b += 64                                  tensor "big": 70 000 elements from offset 13 -> 67 whole blocks
  ballot loop with several tensors in one wave           tensors of 1, 3, 4, 5 elements at offsets 0 .. 12
  uniform block / boundary blocks / inactive tensors     "aligned" (1024 at 69 x 1024), "filler" (ends mid-block), "odd_end" (ends at 1023 mod 1024)
  (total & 3) != 0: every non-vector path                adam_layout(tail=10)
sumsq_kernel                                             CLIP_NS: 1, 3, 4, 1023 (scalar tail), 2048 x 1024 + 1027 (grid-stride second pass)
"""
import functools

import numpy as np
import torch

import train_bf16_cases as TC
from oracle import f64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
_gen = TC._gen

C_TRAIN_CHAIN = 4             # the margin on the reference's own error (tests/test_gpu_train_bf16.py)
TOL = dict(PairSimFn=2e-5, RankLossFn=2e-5, SpanLossFn=5e-5, VideoLevelScoresFn=5e-5)      # tests/test_gpu_train.py
ROW_FLOOR = 1e-6              # a row whose largest reference value is below this share of the tensor's is not compared
ROW_CAP = 0.10                # at most this share of a tensor's rows may be left out that way
HINGE_CLEAR = 1e-4            # every selected pair of a hinge case is at least this far from margin + neg - pos == 0
SCORE_GAP = 1e-3              # the top two clips of every (query, video) pair are at least this far apart (float64 cosines)
MARGIN = 0.1


class Case(TC.Case):
    @functools.lru_cache(maxsize=None)
    def refs(self):
        """-> dict W / R (and S for bf16 leaves), each (outputs, gradients per leaf)."""
        out = dict(W=self.run(F64, f64.ident), R=self.run(F32, f64.ident))
        if any(t is not None and t.dtype == BF16 for t in self.leaves):
            out["S"] = self.run(F64, f64.bf16_round)
        return out


def run_fn(case, fn, dtype=F64):
    """a case (of this module or of train_bf16_cases) with another function in place of its own -- a restated wrong kernel:
    same leaves, same upstream gradients."""
    keep, case.fn = case.fn, fn
    try:
        return case.run(dtype, f64.ident)
    finally:
        case.fn = keep


# ---- the checks -------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().cpu().double()


def _rows(t):
    """(rows, everything else) view: a row = index 0 (batch row of dsim / dq / df2 / dquery, video of dfeat, row of dscores)."""
    return t.reshape(t.shape[0], -1) if t.dim() >= 2 else None


def row_split(W):
    """-> (compared, excluded, zero) boolean per row of W: zero rows are checked exactly (G is bit-zero there), rows below
    ROW_FLOOR of the tensor's maximum are excluded, the rest are compared."""
    w = _rows(W).abs().amax(1)
    top = float(w.max())
    zero = w == 0
    excluded = ~zero & (w < ROW_FLOOR * top)
    return ~zero & ~excluded, excluded, zero


def check_tensor(tag, case, G, W, R, tol, storage="f32", keep=None, rows=True):
    """One output or gradient G (kernel, or a model of one) against W with R's error as the yardstick.
    * finite; G == 0 exactly wherever W == 0 exactly (masked clips, rows without a gradient, hinge-inactive pairs);
    * whole tensor: max|G - W| / max|W| <= max(tol, C_TRAIN_CHAIN x the same figure of R);
    * per row (rows=True, tensors of two or more dimensions): max|G_r - W_r| / max|W_r| <= max(tol, C_TRAIN_CHAIN x the same figure
      of R in that row), rows split by `row_split`, at most ROW_CAP of them excluded.
    keep: boolean mask over the last dimension (columns that are compared).  -> dict of the figures."""
    assert G is not None, "%s %s: missing" % (tag, case)
    assert tuple(G.shape) == tuple(W.shape), "%s %s: shape %s, reference %s" % (tag, case, tuple(G.shape), tuple(W.shape))
    assert bool(torch.isfinite(G).all()), "%s %s: non-finite" % (tag, case)
    G, W, R = _d(G), _d(W), _d(R)
    if keep is not None:
        G, W, R = G[..., keep], W[..., keep], R[..., keep]
    zero = W == 0
    assert bool((G[zero] == 0).all()), "%s %s: %d elements are non-zero where the exact value is exactly zero" % (
        tag, case, int((G[zero] != 0).sum()))
    scale = float(W.abs().max()) or 1.0
    kerr, rerr = float((G - W).abs().max()) / scale, float((R - W).abs().max()) / scale
    lim = max(tol, C_TRAIN_CHAIN * rerr)
    print("NUMERICS %s %s %s whole: kernel_err %.3e ref_err %.3e limit %.3e" % (tag, case, storage, kerr, rerr, lim))
    assert kerr <= lim, "%s %s: max|G-W| = %.3e of max|W| > %.3e (tolerance %.1e, reference %.3e)" % (tag, case, kerr, lim, tol, rerr)
    res = dict(kerr=kerr, rerr=rerr, lim=lim, row_kerr=0.0, row_rerr=0.0, row_lim=tol, row_ratio=0.0)
    if not rows or W.dim() < 2:
        return res
    cmp_, excl, _ = row_split(W)
    share = float(excl.double().mean())
    assert share <= ROW_CAP, "%s %s: %.0f %% of the rows are below %g of the tensor's maximum" % (tag, case, 100 * share, ROW_FLOOR)
    if not bool(cmp_.any()):
        return res
    g, w, r = _rows(G)[cmp_], _rows(W)[cmp_], _rows(R)[cmp_]
    top = w.abs().amax(1)
    k_r, r_r = (g - w).abs().amax(1) / top, (r - w).abs().amax(1) / top
    lim_r = torch.clamp(C_TRAIN_CHAIN * r_r, min=tol)
    over = k_r / lim_r
    i = int(over.argmax())
    row = int(cmp_.nonzero()[i])
    print("NUMERICS %s %s %s rows: %d compared %d excluded; worst row %d kernel_err %.3e ref_err %.3e limit %.3e; "
          "largest kernel_err %.3e ref_err %.3e" % (tag, case, storage, int(cmp_.sum()), int(excl.sum()), row, float(k_r[i]),
                                                    float(r_r[i]), float(lim_r[i]), float(k_r.max()), float(r_r.max())))
    assert float(over[i]) <= 1.0, "%s %s: row %d: max|G-W| = %.3e of the row's max|W| > %.3e (tolerance %.1e, reference %.3e)" % (
        tag, case, row, float(k_r[i]), float(lim_r[i]), tol, float(r_r[i]))
    res.update(row_kerr=float(k_r.max()), row_rerr=float(r_r.max()), row_lim=float(lim_r[i]), row_ratio=float(over[i]))
    return res


def check_case(case, outs, grads, keep_out=None):
    """every output and gradient of a case (lists as Case.run returns them).  bf16 gradients (PairSimFn on bf16 leaves) are
    measured against S, the float64 value behind one bf16 store, in R's place: the store's rounding is the reference's own
    error there and an f32-grade value rounded once lies within two of them.  -> {tensor name: figures}."""
    refs = case.refs()
    (Wo, Wg), (Ro, Rg) = refs["W"], refs["R"]
    tol = TOL[case.op]
    res = {}
    assert len(outs) == len(Wo)
    for i, o in enumerate(outs):
        res["out%d" % i] = check_tensor("%s.out%d" % (case.op, i), case.name, o, Wo[i], Ro[i], tol, keep=keep_out)
    for i, (g, w) in enumerate(zip(grads, Wg)):
        if w is None:
            assert g is None
            continue
        bf = case.leaves[i].dtype == BF16
        res["grad%d" % i] = check_tensor("%s.grad%d" % (case.op, i), case.name, g, w, refs["S"][1][i] if bf else Rg[i], tol,
                                         storage="bf16" if bf else "f32")
    return res


def excluded_shares(case):
    """-> the share of excluded rows of every >= 2-d output / gradient of a case (ROW_CAP is asserted on the CPU)."""
    Wo, Wg = case.refs()["W"]
    return [float(row_split(w)[1].double().mean()) for w in list(Wo) + [g for g in Wg if g is not None] if w.dim() >= 2]


# ---- PairSimFn --------------------------------------------------------------------------------------------------------------
PAIR_SIM_SHAPES = [(3, 1, 8), (2, 3, 64), (5, 21, 520), (2, 17, 2048), (2, 5, 2056), (3, 7, 100), (1, 128, 128)]


def pair_sim_case(n, l, h, dt):
    q, f2 = torch.randn(n, h, generator=_gen(1)).to(dt), torch.randn(n, l, h, generator=_gen(2)).to(dt)
    fn = lambda q, f2, stage: f64.train_pair_sim(q, f2, stage)      # noqa: E731
    return Case("PairSimFn", "%dx%dx%d %s" % (n, l, h, "bf16" if dt == BF16 else "f32"), fn, [q, f2], [True, True],
                [TC.act(n, l, seed=4).float()])


def pair_sim_cases():
    assert any((n * l) % 4 for n, l, _ in PAIR_SIM_SHAPES)
    return [pair_sim_case(*s, dt) for s in PAIR_SIM_SHAPES for dt in (F32, BF16)]


# ---- SpanLossFn -------------------------------------------------------------------------------------------------------------
# (n, L, ks): L in {1, 3, 63, 64, 65, 100, 127, 128} crossed sparsely with ks in {1, 3, 5, 31}, n in {1, 4, 5, 9}
SPAN_SHAPES = [(1, 1, 1), (4, 1, 31), (4, 3, 31), (5, 3, 3), (9, 63, 5), (5, 63, 31), (4, 64, 3), (9, 64, 1), (5, 65, 1), (4, 65, 5),
               (9, 100, 5), (5, 100, 31), (5, 127, 31), (9, 127, 3), (4, 128, 31), (9, 128, 1), (1, 128, 5), (5, 128, 3)]
SPAN_FORMS = [(True, 2), (False, 2), (False, 1)]        # (merged, n_sim)
SPAN_TWO_MASKS = (3, 65, 100, 128)                      # split, n_sim 2: per-row lengths differ between the streams at these L


def span_lens(n, l, seed):
    """per-row lengths: row 0 full, row 1 of length 1, row 2 one short of full, the rest drawn."""
    lens = torch.randint(1, l + 1, (n,), generator=_gen(seed))
    lens[0] = l
    if n > 1:
        lens[1] = 1
    if n > 2:
        lens[2] = max(1, l - 1)
    if n > 3:
        lens[3] = max(int(lens[3]), min(l, 66))         # room for a start target in the second half
    return lens


def span_targets(lens, seed):
    """(start, end) per row on clips valid under `lens`: row 0 (clip 0, the last clip), row 1 (0, 0), row 2 (last, last),
    row 3 starts at clip 64 where it is that long, the rest drawn with start <= end."""
    g = _gen(seed)
    st_ed = []
    for b, x in enumerate(int(v) for v in lens):
        s = int(torch.randint(0, x, (1,), generator=g))
        e = int(torch.randint(s, x, (1,), generator=g))
        if b == 0:
            s, e = 0, x - 1
        elif b == 2:
            s, e = x - 1, x - 1
        elif b == 3 and x > 64:
            s, e = 64, max(e, 64)
        st_ed.append((s, e))
    return torch.tensor(st_ed, dtype=torch.int64)


def span_case(n, l, ks, merged, n_sim):
    sims = [torch.randn(n, l, generator=_gen(1 + i)) * 3.0 for i in range(n_sim)]
    filters = [torch.randn(1, 1, ks, generator=_gen(10 + i)) * 0.5 for i in range(2 * (1 if merged else n_sim))]
    lens = [span_lens(n, l, 5)]
    if n_sim == 2:
        two = not merged and l in SPAN_TWO_MASKS and n > 1
        lens.append(span_lens(n, l, 6) if two else lens[0])
        if two:
            lens[1][1] = min(l, 2)                     # row 1: length 1 in stream 0 only
    masks = [(torch.arange(l)[None, :] < x[:, None]).float() for x in lens]
    st_ed = span_targets(torch.minimum(lens[0], lens[-1]), 7)

    def fn(*t, stage):
        return f64.train_span_loss(t[:n_sim], t[n_sim:], masks, st_ed, merged, ks)
    name = "%dx%d ks%d %s" % (n, l, ks, "merged" if merged else "split%d" % n_sim)
    return Case("SpanLossFn", name, fn, sims + filters, [True] * (n_sim + len(filters)), [torch.ones(())], masks=masks,
                st_ed=st_ed, merged=merged, n_sim=n_sim, ks=ks, n=n, l=l)


def span_cases():
    return [span_case(*s, *f) for s in SPAN_SHAPES for f in SPAN_FORMS]


# ---- RankLossFn -------------------------------------------------------------------------------------------------------------
RANK_NS = [2, 17, 255, 256, 257, 600, 1024]
RANK_GOUT = torch.tensor([0.8125, -1.375])      # two magnitudes: the two sides' entries on the diagonal cannot cancel
# (n, kind): "grid" scores rounded to 1/8; "block" a block of columns at -1e10 (fully masked videos); "straddle" grid plus equal
# values in columns / rows 253 .. 256
RANK_TIES = [(17, "grid"), (257, "grid"), (600, "grid"), (17, "block"), (257, "block"), (257, "straddle"), (600, "straddle"),
             (1024, "straddle")]
RANK_BLOCK = {17: (5, 9), 257: (253, 257)}      # the -1e10 columns [lo, hi): the second across j = 255 | 256


def rank_masked(scores):
    n = scores.shape[0]
    m = scores.detach().clone().double()
    m[torch.arange(n), torch.arange(n)] = 999
    return m


def rank_selected(scores, rc, rq):
    """-> (columns selected by the context side per row, rows selected by the query side per column) under the rule
    "descending, equal values: lower index first" (f64.rank_order)."""
    ar = torch.arange(scores.shape[0])
    m = rank_masked(scores)
    return f64.rank_order(m)[ar, rc.long()], f64.rank_order(m.t().contiguous())[ar, rq.long()]


def rank_tie_groups(row_sorted):
    """sorted values of one row -> list of (first position, size) of the groups of equal values, the diagonal's 999 left out."""
    out, i, n = [], 1, len(row_sorted)
    while i < n:
        j = i
        while j + 1 < n and row_sorted[j + 1] == row_sorted[i]:
            j += 1
        out.append((i, j - i + 1))
        i = j + 1
    return out


def _rank_at(masked_row_order, col):
    return int((masked_row_order == col).nonzero()[0])


def rank_case(n, lse, kind=None, seed=1):
    """Ranks are drawn from [1, n - 1] as the reference does; row 0 wants rank 1 and row 1 rank n - 1 on both sides.  Tie cases
    then point rows 2 .. 7 at the first / an inner / the last member of a tie group (context side: rows, query side: columns),
    the "straddle" cases point rows 8 .. 11 (columns 12 .. 15) at the four equal entries in columns (rows) 253 .. 256, and the
    "block" cases point the rows of the masked videos themselves into the block (their positive is -1e10 too: a negative
    outside the block would make the lse loss infinite in the reference itself)."""
    g = _gen(seed)
    scores = torch.randn(n, n, generator=g) * 0.3           # plain f32 draws: no two equal in a row unless a tie is planted
    if kind in ("grid", "straddle"):
        scores = torch.round(scores * 8) / 8
    if kind == "block":
        lo, hi = RANK_BLOCK[n]
        scores[:, lo:hi] = -1e10
    if kind == "straddle":
        scores[8:12, 253:257] = 0.0625              # off the grid: groups of exactly four
        scores[253:257, 12:16] = -0.0625
    g2 = _gen(seed + 2)
    rc, rq = torch.randint(1, n, (n,), generator=g2), torch.randint(1, n, (n,), generator=g2)
    rc[0] = rq[0] = 1
    rc[1] = rq[1] = n - 1
    if kind is not None:
        m = rank_masked(scores)
        for side, (mm, ranks) in enumerate(((m, rc), (m.t().contiguous(), rq))):
            order = f64.rank_order(mm)
            srt = torch.gather(mm, 1, order)
            if kind == "block":
                lo, hi = RANK_BLOCK[n]
                for k, i in enumerate(range(lo, hi)):
                    if side == 0:                  # row i of the block: first / inner ... / last member of the bottom group
                        ranks[i] = n - (hi - lo - 1) + k % (hi - lo - 1)
                    else:                          # column i: every other entry ties
                        ranks[i] = (1, (n - 1) // 2, n - 1, 2, n - 2)[k % 5]
            else:
                for i in range(2, min(8, n)):
                    groups = [(p, s) for p, s in rank_tie_groups(srt[i].tolist()) if s >= 3]
                    if groups:
                        p, s = groups[(i // 3) % len(groups)]
                        ranks[i] = (p, p + s // 2, p + s - 1)[i % 3]
            if kind == "straddle":
                for k in range(4):
                    line = (8 + k) if side == 0 else (12 + k)
                    ranks[line] = _rank_at(order[line], 253 + k)
    name = "n%d %s%s" % (n, "lse" if lse else "hinge", " " + kind if kind else "")
    fn = lambda s, stage, rc=rc, rq=rq: f64.train_rank_loss(s, rc, rq, MARGIN, lse)      # noqa: E731
    return Case("RankLossFn", name, fn, [scores], [True], [RANK_GOUT.clone()], rc=rc, rq=rq, lse=lse, kind=kind, n=n)


def hinge_distance(case):
    """the smallest |margin + neg - pos| over the selected pairs of both sides (float64)."""
    s = case.leaves[0].double()
    ar = torch.arange(s.shape[0])
    cols, rows = rank_selected(s, case.cfg["rc"], case.cfg["rq"])
    pos = s[ar, ar]
    return float(torch.minimum((MARGIN + s[ar, cols] - pos).abs().min(), (MARGIN + s[rows, ar] - pos).abs().min()))


def rank_hinge_case(n, kind=None):
    """The hinge gradient at margin + neg - pos == 0 is a convention (the kernel: 0, torch.clamp: 1): a hinge case takes the first
    seed (1, 2, ...) whose selected pairs all stay HINGE_CLEAR away from the kink.  (The grid cases cannot sit there: 0.1 is
    0.025 away from the nearest multiple of 1/8.)"""
    for seed in range(1, 200):
        case = rank_case(n, False, kind, seed=seed)
        if hinge_distance(case) > HINGE_CLEAR:
            return case
    raise AssertionError("no seed keeps n = %d away from the hinge kink" % n)


def rank_cases():
    out = []
    for n in RANK_NS:
        out += [rank_hinge_case(n), rank_case(n, True)]
    for n, kind in RANK_TIES:
        out += [rank_hinge_case(n, kind), rank_case(n, True, kind)]
    return out


def rank_expected_nonzero(case):
    """the positions where dscores may be non-zero: what the stable float64 order selects on either side, and the diagonal."""
    s = case.leaves[0]
    n = s.shape[0]
    ar = torch.arange(n)
    cols, rows = rank_selected(s, case.cfg["rc"], case.cfg["rq"])
    sel = torch.zeros(n, n, dtype=torch.bool)
    sel[ar, cols] = True
    sel[rows, ar] = True
    sel[ar, ar] = True
    return sel


# ---- VideoLevelScoresFn -----------------------------------------------------------------------------------------------------
# (nq, nv, L, H) -> L of the second modality (n_mod = 2: another length, other masks)
SCORES_SHAPES = [(7, 7, 19, 128), (9, 5, 37, 64), (6, 3, 70, 64), (5, 3, 100, 768), (130, 11, 16, 64), (260, 4, 5, 8), (3, 260, 9, 16),
                 (4, 4, 128, 520)]
SCORES_L2 = {19: 24, 37: 21, 70: 33, 100: 90, 16: 13, 5: 7, 9: 12, 128: 100}
SCORES_PADDED = SCORES_SHAPES[:4]                   # also through FUSED_LOSS_TAIL = False (padded clips, separate launches)
# exact ties: shape -> {video: (first, second position of the duplicated winning clip)}: within one 16-column tile, across two
# tiles (the first in the earlier one), across tiles with a full tile in between
SCORES_TIES = [((9, 5, 37, 64), {0: (3, 9), 3: (5, 20), 4: (17, 36)}),
               ((5, 3, 100, 768), {0: (65, 70), 1: (2, 99)}),
               ((130, 11, 16, 64), {0: (1, 15), 5: (6, 7)})]


def sparse_dscores(nq, nv, seed):
    """ranking-loss-like: at most 3 entries per row."""
    g = _gen(seed)
    ds = torch.zeros(nq, nv)
    for m in range(nq):
        for n in torch.randint(0, nv, (3,), generator=g).tolist():
            ds[m, n] += float(torch.randn((), generator=g))
    return ds


def scores_case(nq, nv, l, h, n_mod, dense, fused=True, ties=None, last=False):
    """The planted-winner construction of train_bf16_cases.scores_cases on f32 operands, for nq != nv: all queries share a
    direction u, every video has one clip along u at a random valid position (not clip 0), video 1's clip 0 is an all-zero row
    that never wins, video 2 is fully masked in every modality.  Narrow rows (H < 64) get a stronger plant and quieter queries:
    a random clip's cosine has a spread of H^-1/2.
    ties: {video: (p1, p2)} -- the winning clip is planted at p1 and copied to p2 (video at full length, modality 0).  The
    REFERENCE sees clip p2 masked out: the maximum is unchanged and its gradient goes to p1 alone, "first clip on ties", without
    leaning on how torch.max breaks a tie; the kernels get the true mask (cfg["masks"]).  last=True swaps the roles (the wrong
    rule, for tests/test_numerics_reference.py)."""
    ties = ties or {}
    ls = [l, SCORES_L2[l]][:n_mod]
    ms, ref_ms, qs, fs = [], [], [], []
    for i, li in enumerate(ls):
        m = TC.lens_mask(nv, li, seed=30 + i, lo=min(2, li))
        g = _gen(40 + i)
        u = torch.nn.functional.normalize(torch.randn(h, generator=g), dim=0) * h ** 0.5
        noise, plant = (1.0, 2.0) if h >= 64 else (0.2, 8.0)
        qs.append(u[None] + noise * torch.randn(nq, h, generator=g))
        f = torch.randn(nv, li, h, generator=g)
        if i == 0:
            for v in ties:
                m[v] = 1
        peak = 1 + torch.randint(0, 10 ** 6, (nv,), generator=g) % (m.sum(1).long() - 1)
        if i == 0:
            for v, (p1, _) in ties.items():
                peak[v] = p1
        f[torch.arange(nv), peak] += plant * u
        f[1, 0] = 0
        m[2] = 0
        rm = m.clone()
        if i == 0:
            for v, (p1, p2) in ties.items():
                f[v, p2] = f[v, p1]
                rm[v, p1 if last else p2] = 0
        fs.append(f)
        ms.append(m)
        ref_ms.append(rm)

    def fn(*t, stage):
        return f64.train_video_level_scores(t[:n_mod], t[n_mod:], ref_ms, stage)
    ds = torch.randn(nq, nv, generator=_gen(4)) if dense else sparse_dscores(nq, nv, 7)
    name = "%dx%dx%dx%d m%d %s %s%s" % (nq, nv, l, h, n_mod, "dense" if dense else "sparse", "fused" if fused else "padded",
                                        " ties" if ties else "")
    return Case("VideoLevelScoresFn", name, fn, qs + fs, [True] * (2 * n_mod), [ds], masks=ms, ref_masks=ref_ms, n_mod=n_mod,
                fused=fused, ties=ties, dense=dense, shape=(nq, nv, l, h))


def scores_cases():
    out = [scores_case(*s, n_mod, dense) for s in SCORES_SHAPES for n_mod in (1, 2) for dense in (True, False)]
    out += [scores_case(*s, n_mod, True, fused=False) for s in SCORES_PADDED for n_mod in (1, 2)]
    out += [scores_case(*s, n_mod, dense, ties=t) for s, t in SCORES_TIES for n_mod, dense in ((1, True), (2, False))]
    return out


def scores_cosines(case, i, masks=None):
    """float64 cosines (nq, nv, L) of modality i, masked clips at -1e10 (masks: cfg["ref_masks"] by default)."""
    n_mod = case.cfg["n_mod"]
    m = (case.cfg["ref_masks"] if masks is None else masks)[i].double()
    qn = torch.nn.functional.normalize(case.leaves[i].double(), dim=-1)
    cn = torch.nn.functional.normalize(case.leaves[n_mod + i].double(), dim=-1)
    s = torch.einsum("md,nld->mnl", qn, cn)
    return s * m[None] + (1 - m[None]) * -1e10


def scores_argmax(case, i):
    """the float64 arg-max clip of every pair of modality i: (nq, nv) int64; a fully masked video reports clip 0."""
    return scores_cosines(case, i).argmax(-1)


def scores_gap(case):
    """the smallest distance between the top two clips over all pairs with at least two clips left in the reference's mask (the
    planted duplicates are out of it: the reference masks them)."""
    worst = float("inf")
    for i in range(case.cfg["n_mod"]):
        s = scores_cosines(case, i)
        if s.shape[-1] < 2:
            continue
        top = torch.topk(s, 2, dim=-1).values
        live = top[..., 1] > -1e9
        if bool(live.any()):
            worst = min(worst, float((top[..., 0] - top[..., 1])[live].min()))
    return worst


# ---- xml_bert_adam_step -----------------------------------------------------------------------------------------------------
ADAM_BLOCK = 1024
ADAM = dict(b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=1e-6, max_grad_norm=1.0, lr_mult=0.75)
# (b1, b2: the f32 values the kernel receives -- 1 - b is then exact in f32 and the float64 reference forms the same constant)


def adam_layout(tail=9):
    """-> (names, sizes): the flat buffer of the optimizer test.  Offsets: four tensors of 1, 3, 4, 5 elements in lanes 0 .. 12
    of one wave; "big" = 70 000 elements from offset 13 (67 whole blocks of 1024: the reduce kernel's b += 64 stride);
    "filler" to 69 x 1024 (ends mid-block); "aligned" = exactly one block; "odd_end" ends at an offset = 1023 mod 1024; "tail"
    makes the total 73 736 (a multiple of 4, not of 1024) -- tail=10: 73 737, (total & 3) != 0."""
    names = ["t1", "t3", "t4", "t5", "big", "filler", "aligned", "odd_end", "tail"]
    sizes = [1, 3, 4, 5, 70000, 69 * 1024 - 70013, 1024, 2047, tail]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert off[4] % 1024 != 0 and off[6] % 1024 == 0 and off[7] % 1024 == 0 and off[8] % 1024 == 1023
    assert off[-1] % 1024 != 0 and (off[-1] % 4 == 0) == (tail == 9)
    assert off[5] // 1024 - (off[4] + 1023) // 1024 > 64
    return names, sizes


ADAM_TOY_SHAPES = [(128, 96), (128,), (1, 1, 5), (40, 128), (3,), (257, 33), (300, 128), (4096,), (2, 4096), (1,)]


def adam_toy_layout():
    """the tensors of test_bert_adam_kernel_vs_oracle as BertAdam lays them out (each padded to 4 elements)."""
    sizes = [(int(np.prod(s)) + 3) // 4 * 4 for s in ADAM_TOY_SHAPES]
    return ["w%d" % i for i in range(len(sizes))], sizes


def adam_state(sizes, seed=0):
    """-> dict of flat f32 tensors p, g, m, v and per-tensor seg_off (int64), seg_lr, seg_wd, seg_lr_mult: gradients of scale 3
    (clipped at max_grad_norm 1) and 0.01 (not clipped) alternate, weight decay on every third tensor."""
    g_ = _gen(seed)
    total = int(sum(sizes))
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    gs = torch.cat([torch.randn(s, generator=g_) * (3.0 if i % 2 == 0 else 0.01) for i, s in enumerate(sizes)])
    return dict(p=torch.randn(total, generator=g_) * 0.05, g=gs, m=torch.randn(total, generator=g_) * 0.01,
                v=torch.rand(total, generator=g_) * 1e-3 + 1e-6, seg_off=off,
                seg_lr=torch.tensor([3e-4 * (1 + i % 3) for i in range(len(sizes))]),
                seg_wd=torch.tensor([0.01 if i % 3 == 0 else 0.0 for i in range(len(sizes))]),
                seg_lr_mult=torch.tensor([0.25 + 0.125 * i for i in range(len(sizes))]))


def adam_sumsq_all(g, seg_off):
    """float64 sum of squares of every tensor."""
    return [float(g[int(a):int(b)].double().pow(2).sum()) for a, b in zip(seg_off[:-1], seg_off[1:])]


def adam_sumsq_first_64_blocks(g, seg_off):
    """A WRONG norm (tests/test_numerics_reference.py): adam_norm_reduce_kernel without its b += 64 stride -- the boundary
    blocks' atomics and the first 64 whole blocks of a tensor only.  ((total & 3) != 0: no block stores a partial sum, every
    element goes through the atomics, and the fault has nothing to miss.)"""
    if int(seg_off[-1]) % 4:
        return adam_sumsq_all(g, seg_off)
    out = []
    for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()):
        b0, b1 = (a + ADAM_BLOCK - 1) // ADAM_BLOCK, b // ADAM_BLOCK
        keep = torch.ones(b - a, dtype=torch.bool)
        if b1 - b0 > 64:
            keep[(b0 + 64) * ADAM_BLOCK - a:b1 * ADAM_BLOCK - a] = False
        out.append(float(g[a:b].double()[keep].pow(2).sum()))
    return out


def adam_reference(state, max_grad_norm=ADAM["max_grad_norm"], active=None, lr_mult=None, sumsq=adam_sumsq_all):
    """One step in float64 on a copy of `state` -> (p, g, m, v, sumsq per tensor).  lr_mult: per-tensor tensor, or None for the
    scalar ADAM["lr_mult"]; active: per-tensor flags or None.  Each tensor's update is oracle.xml_oracle.bert_adam_step in
    float64 (its clip uses the float64 norm of the tensor).  sumsq = adam_sumsq_all by default; another function (a wrong
    norm, tests/test_numerics_reference.py) clips with ITS squared norms in front of the oracle's clip-free update."""
    from oracle import xml_oracle as O
    p, g, m, v = (state[k].double().clone() for k in "pgmv")
    off = state["seg_off"].tolist()
    ss = sumsq(state["g"], state["seg_off"])
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if active is not None and not active[s]:
            continue
        lm = ADAM["lr_mult"] if lr_mult is None else float(lr_mult[s])
        ps, gr, st = {"t": p[a:b].clone()}, {"t": g[a:b].clone()}, {"t": (m[a:b].clone(), v[a:b].clone())}
        mgn = max_grad_norm
        if sumsq is not adam_sumsq_all and max_grad_norm > 0:
            coef = max_grad_norm / (ss[s] ** 0.5 + 1e-6)
            if coef < 1:
                gr["t"].mul_(coef)
            mgn = -1.0
        O.bert_adam_step(ps, gr, st, 0, {"t": float(state["seg_wd"][s])}, lr=float(state["seg_lr"][s]) * lm, warmup=-1,
                         t_total=-1, b1=ADAM["b1"], b2=ADAM["b2"], e=ADAM["eps"], max_grad_norm=mgn)
        p[a:b], g[a:b], m[a:b], v[a:b] = ps["t"], gr["t"], st["t"][0], st["t"][1]
    return p, g, m, v, ss


def check_adam(tag, got, want, seg_off, names, tol=2e-6):
    """p, g, m, v of one step, tensor by tensor: max|got - want| <= tol max|want| (rel_err of tests/test_gpu_train.py)."""
    worst = 0.0
    for k, a, b in zip("pgmv", got, want):
        a, b = _d(a), _d(b)
        for nm, lo, hi in zip(names, seg_off[:-1].tolist(), seg_off[1:].tolist()):
            e = float((a[lo:hi] - b[lo:hi]).abs().max() / b[lo:hi].abs().max().clamp_min(1e-12))
            worst = max(worst, e)
            assert e <= tol, "%s: %s of tensor %s: max err / max|ref| = %.3e > %.1e" % (tag, k, nm, e, tol)
    print("NUMERICS bert_adam_step %s f32: worst tensor err %.3e limit %.1e" % (tag, worst, tol))
    return worst


# ---- xml_clip_grad_norm -----------------------------------------------------------------------------------------------------
CLIP_NS = [1, 3, 4, 1023, 2048 * 1024 + 1027]


def clip_reference(g, max_norm):
    """float64 torch.nn.utils.clip_grad_norm_ on one flat buffer -> (clipped gradient, clipped?)."""
    g = g.double()
    coef = max_norm / (float(g.norm(2)) + 1e-6)
    return (g * coef, True) if coef < 1 else (g.clone(), False)


def ids(cases):
    return [c.name for c in cases]
