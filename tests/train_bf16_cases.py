"""Cases of tests/test_gpu_train_bf16.py: the leaves of one training node (bf16 activations, f32 master parameters, one
upstream gradient on the bf16 grid), and the three reference values of its outputs and gradients --
W  float64 autograd on the bf16-rounded operands (oracle/f64.py, identity stage),
S  the staged float64 reference (bf16 where the kernels store an activation or a gradient in bf16),
R  float32 autograd on the CPU (the "f32 allowance" of numerics_regimes.check_bf16_rounding).
No GPU is needed: tests/test_numerics_reference.py checks the references themselves.  The shapes are the smallest that reach
each dispatch branch of autograd.py (see the tables in the test module); the attention shapes go further and reach every
instantiation of attention_train.hip (head sizes 32, 64, 96, 128, 192; tests/test_numerics_reference.py ties the table to the
library's list), the waves' second row tiles (rows >= 64), head counts 1, 2, 4, 8 and 24, every tile / padding edge of the sequence
lengths, the entry forms with ld = 2H / 3H, and dropout on the probabilities through a host model of the mask.  References are
computed once per case (`refs`)."""
import functools

import torch

from oracle import f64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def act(*shape, seed=0, scale=1.0):
    """a bf16 activation / upstream gradient."""
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(BF16)


def par(*shape, seed=0, scale=1.0, shift=0.0):
    """an f32 master parameter (NOT on the bf16 grid: the kernels round weights themselves, f64.operand)."""
    return shift + torch.randn(*shape, generator=_gen(seed)) * scale


def lens_mask(n, l, seed=0, lo=1):
    lens = torch.randint(lo, l + 1, (n,), generator=_gen(seed))
    lens[0] = l
    return (torch.arange(l)[None, :] < lens[:, None]).float()


class Case(object):
    """leaves: tensors in the dtype the node gets them in (None: absent input); needs: which of them want a gradient;
    fn(*leaves_in_reference_dtype, stage=...) -> output or tuple of outputs; gouts: upstream gradients (bf16-grid values);
    chain: the bf16 outputs sit behind more than one bf16 boundary (compared with S instead of one rounding of W)."""

    def __init__(self, op, name, fn, leaves, needs, gouts, chain=False, **cfg):
        self.op, self.name, self.fn, self.leaves, self.needs, self.gouts, self.chain, self.cfg = \
            op, name, fn, list(leaves), list(needs), list(gouts), chain, cfg

    def __repr__(self):
        return "%s[%s]" % (self.op, self.name)

    def run(self, dtype, stage):
        ls = [None if t is None else t.detach().to(dtype).clone().requires_grad_(ng) for t, ng in zip(self.leaves, self.needs)]
        outs = self.fn(*ls, stage=stage)
        outs = outs if isinstance(outs, tuple) else (outs,)
        torch.autograd.backward(outs, [g.to(dtype) for g in self.gouts])
        return [o.detach() for o in outs], [l.grad if (l is not None and ng) else None for l, ng in zip(ls, self.needs)]

    def out_is_bf16(self, i):
        return self.gouts[i].dtype == BF16

    def grad_is_bf16(self, i):
        """the gradient of leaf i comes out of a bf16 store (LayerNormFn's f32 `a` gets the bf16 dx widened by ops.convert)."""
        return self.leaves[i].dtype == BF16 or (self.op == "LayerNormFn" and i == 0)

    @functools.lru_cache(maxsize=None)
    def refs(self):
        """-> dict W / S / R, each (outputs, gradients per leaf)."""
        return dict(W=self.run(F64, f64.ident), S=self.run(F64, f64.bf16_round), R=self.run(F32, f64.ident))


# ---- LinearFn ---------------------------------------------------------------------------------------------------------------
# rows, k, n:  (37, 64, 48) gemm_tn taken, rows % 8 != 0;  (300, 72, 20) / (6, 128, 2): n % 8 != 0 -> gemm_tn refused (transposes +
# split-K dW, colsum db) and the zero-padded reduction of the dX GEMM;  (2077, 192, 192): the XCD-partitioned gemm_tn kernel
# (gemm_tn.hip dispatches to it for N % 192 == 0, K % 192 == 0, at most 32 tiles of 96 x 192 and rows >= 2048; the library
# exposes no predicate for that choice, so the case restates the condition instead of asserting the dispatch)
LINEAR_SHAPES = [(37, 64, 48), (300, 72, 20), (6, 128, 2), (2077, 192, 192)]


def linear_case(rows, k, n, relu, bias, x_grad=True):
    x, w = act(rows, k, seed=1), par(n, k, seed=2, scale=k ** -0.5)
    b = par(n, seed=3, scale=0.1) if bias else None
    fn = lambda x, w, b, stage: f64.train_linear(x, w, b, relu, stage)      # noqa: E731
    return Case("LinearFn", "%dx%dx%d%s%s%s" % (rows, k, n, "+relu" if relu else "", "+bias" if bias else "", "" if x_grad else
                                               "-dx"), fn, [x, w, b], [x_grad, True, bias], [act(rows, n, seed=4)], chain=relu, relu=relu)


def linear_cases():
    out = [linear_case(r, k, n, relu, bias) for (r, k, n) in LINEAR_SHAPES for relu in (False, True) for bias in (True, False)]
    return out + [linear_case(6, 128, 2, True, True, x_grad=False), linear_case(37, 64, 48, False, True, x_grad=False)]


# ---- LayerNormFn (bf16 out) -------------------------------------------------------------------------------------------------
def layernorm_case(rows, d, a_dt, a_grad, resid):
    a = act(rows, d, seed=1).to(a_dt) if a_dt == BF16 else torch.randn(rows, d, generator=_gen(1))
    b = act(rows, d, seed=2) if resid else None
    g, beta = par(d, seed=3, scale=0.2, shift=1.0), par(d, seed=4, scale=0.2)
    fn = lambda a, b, g, beta, stage: f64.train_layernorm(a, b, g, beta, stage)      # noqa: E731
    name = "%dx%d a=%s%s%s" % (rows, d, "bf16" if a_dt == BF16 else "f32", "+grad" if a_grad else "", "+resid" if resid else "")
    return Case("LayerNormFn", name, fn, [a, b, g, beta], [a_grad, resid, True, True], [act(rows, d, seed=5)])


def layernorm_cases():
    return [layernorm_case(50, 128, BF16, True, True),        # dx for a and b, both bf16
            layernorm_case(33, 768, F32, False, False),       # raw f32 features: parameter gradients only (dx = NULL)
            layernorm_case(33, 768, BF16, True, False),
            layernorm_case(9, 200, F32, True, True),          # dx (bf16) converted to a's f32; the same dx to b in bf16
            layernorm_case(9, 200, F32, False, True)]         # dx needed for b alone


# ---- QkvFn / QkvResFn -------------------------------------------------------------------------------------------------------
QKV_SHAPES = [(2, 24, 128, 2), (3, 13, 256, 3)]         # (N, L, H, weights)


def qkv_case(n, l, h, nw, residual):
    x = act(n, l, h, seed=1)
    ws = [par(h, h, seed=10 + i, scale=h ** -0.5) for i in range(nw)]
    bs = [par(h, seed=20 + i, scale=0.1) for i in range(nw)]

    def fn(x, *wb, stage):
        return f64.train_qkv(x, wb[0::2], wb[1::2], stage, residual)
    leaves = [x] + [t for pair in zip(ws, bs) for t in pair]
    gouts = [act(n, l, nw * h, seed=4)]
    if residual:
        dres = act(n, l, h, seed=5)
        gouts.append(dres.float() + 2.0 ** -12 * torch.randn(n, l, h, generator=_gen(6)) if residual == "fallback" else dres)
    return Case("QkvResFn" if residual else "QkvFn", "%dx%dx%d w%d%s" % (n, l, h, nw, " " + residual if residual else ""), fn,
                leaves, [True] * len(leaves), gouts, chain=bool(residual), residual=residual)


def qkv_cases():
    return [qkv_case(*s, r) for s in QKV_SHAPES for r in (None, "epilogue", "fallback")]


# ---- attention --------------------------------------------------------------------------------------------------------------
# (N, Lq, Lk, H, heads).  One workgroup of attention_train.hip handles a (sequence, head): wave w owns the 16-row tiles w and
# w + 4, reductions are padded to multiples of 32 (lkp / lqp), the dropout index runs in the (N * heads, lq8, lk8) layout of the
# unfused chain (multiples of 8), every operand goes through LDS rows of DH * 2 + 16 bytes.
ATTENTION_SHAPES = [(2, 13, 21, 128, 4), (2, 24, 24, 128, 4)]     # the first with a query mask; masks from lens_mask seeds
# every instantiation (DH 32, 64, 96, 128, 192) with the waves' second row tiles (rows >= 64) in use: all four at L = 128
ATTENTION_FULL = [(2, 128, 128, 128, 4), (2, 100, 100, 256, 4), (2, 65, 97, 384, 4), (2, 128, 128, 512, 4), (2, 100, 100, 768, 4)]
# head counts other than 4 (gridDim.x in `unit = n * heads + head` and the head * DH column offset): DH 128, 96, 32, 96, 32
ATTENTION_HEADS = [(2, 24, 24, 128, 1), (2, 40, 40, 192, 2), (2, 33, 64, 256, 8), (2, 30, 30, 768, 8), (2, 20, 20, 768, 24)]
# (Lq, Lk) at H = 128, 4 heads: 64 | 65 is where a wave's second row tile starts, multiples of 32 the reduction padding,
# multiples of 8 the dropout layout, 16 the tile
ATTENTION_EDGES = [(1, 17), (16, 16), (17, 33), (32, 31), (9, 8), (8, 9), (15, 63), (63, 15), (64, 32), (65, 64), (96, 65),
                   (97, 96), (127, 128), (128, 127)]
# the unfused bf16 chain; the last has DH = 48, no fused instantiation: the chain is what training runs there
ATTENTION_CHAIN = [(2, 65, 97, 384, 4), (2, 100, 100, 768, 4), (2, 40, 40, 192, 2), (2, 21, 21, 192, 4)]
ATTENTION_CHAIN_ONLY = (2, 21, 21, 192, 4)
# dropout on the probabilities, p = 0.2, fused only; the last two have L8 != L on both sides
ATTENTION_DROP = [((2, 65, 97, 384, 4), "core"), ((2, 65, 97, 384, 4), "kv"), ((2, 128, 128, 512, 4), "qkv"),
                  ((2, 100, 100, 768, 4), "core"), ((2, 30, 30, 768, 8), "qkv"), ((2, 17, 33, 128, 4), "core"),
                  ((2, 13, 21, 128, 4), "core")]
P_DROP = 0.2


def prefix_mask(l, lens):
    return (torch.arange(l)[None, :] < torch.tensor(lens)[:, None]).float()


def two_thirds(l):
    return (2 * l + 2) // 3


def attention_case(n, lq, lk, h, heads, form, fused, lens=None, p_drop=0.0, seed=0, supported=True):
    """form: core (q, k, v separate), kv (k, v the column blocks of one (N, Lk, 2H) leaf), qkv (one (N, L, 3H) leaf).
    lens: (valid keys per sequence, valid queries per sequence or None); None: the seeded masks of ATTENTION_SHAPES.
    p_drop > 0: dropout on the probabilities with the host model of the kernels' mask (oracle/f64.py drop_keep).
    supported: what attention_train_supported answers for the shape (False: no fused instantiation for H / heads).
    Rows of masked-out queries depend on float32's absorption of the score into -1e4 (oracle/f64.py header): their upstream
    gradient is zero and their outputs are not compared."""
    q, k, v = act(n, lq, h, seed=1), act(n, lk, h, seed=2), act(n, lk, h, seed=3)
    if lens is None:
        km = lens_mask(n, lk, seed=4, lo=3)
        qm = lens_mask(n, lq, seed=5, lo=3) if lq != lk else None
    else:
        km = prefix_mask(lk, lens[0])
        qm = None if lens[1] is None else prefix_mask(lq, lens[1])
    drop = f64.attention_drop(n, heads, lq, lk, p_drop, seed) if p_drop > 0 else None
    gout = act(n, lq, h, seed=6)
    if qm is not None:
        gout = gout * qm[:, :, None].to(BF16)
    att = lambda q, k, v, stage: f64.train_attention(q, k, v, qm, km, heads, stage, drop)      # noqa: E731
    if form == "core":
        leaves = [q, k, v]
        fn = att
    elif form == "kv":
        leaves = [q, torch.cat([k, v], -1)]
        fn = lambda q, kv, stage: att(q, kv[..., :h], kv[..., h:], stage)      # noqa: E731
    else:
        leaves = [torch.cat([q, k, v], -1)]
        fn = lambda t, stage: att(t[..., :h], t[..., h:2 * h], t[..., 2 * h:], stage)      # noqa: E731
    name = "%s %dx%dx%dx%d h%d %s%s" % (form, n, lq, lk, h, heads, "fused" if fused else "chain", " p%g" % p_drop if p_drop else "")
    return Case("Attention" + form.capitalize() + "Fn", name, fn, leaves, [True] * len(leaves), [gout], chain=True, q_mask=qm,
                k_mask=km, heads=heads, fused=fused, form=form, p_drop=p_drop, seed=seed, drop=drop, supported=supported)


def attention_case_at(shape, form, fused, **kw):
    """a case of the explicit table: N = 2, sequence 0 full, sequence 1 with ceil(2 L / 3) valid keys and -- cross attention
    (Lq != Lk): a query mask -- the same share of valid queries.  Every case has a masked key, no sequence has none valid."""
    n, lq, lk, h, heads = shape
    assert n == 2
    lens = ((lk, two_thirds(lk)), (lq, two_thirds(lq)) if lq != lk else None)
    return attention_case(n, lq, lk, h, heads, form, fused, lens=lens, **kw)


def attention_cases():
    cross, self_ = ATTENTION_SHAPES
    out = [attention_case(*cross, "core", True), attention_case(*cross, "core", False), attention_case(*cross, "kv", True),
           attention_case(*self_, "core", True), attention_case(*self_, "core", False), attention_case(*self_, "qkv", True),
           attention_case(*self_, "qkv", False)]
    for s in ATTENTION_FULL:                  # qkv / kv: ld = 3H / 2H and non-zero column offsets
        out += [attention_case_at(s, "core", True), attention_case_at(s, "qkv" if s[1] == s[2] else "kv", True)]
    for s in ATTENTION_HEADS:
        out += [attention_case_at(s, "core", True)] + ([attention_case_at(s, "qkv", True)] if s[1] == s[2] else [])
    out += [attention_case_at((2, lq, lk, 128, 4), "core", True) for lq, lk in ATTENTION_EDGES]
    out += [attention_case_at(s, "core", False, supported=s != ATTENTION_CHAIN_ONLY) for s in ATTENTION_CHAIN]
    # seeds: both seed words in use (xml_seed_words), a different mask per case
    out += [attention_case_at(s, form, True, p_drop=P_DROP, seed=(i << 32) + 4242 + i) for i, (s, form) in enumerate(ATTENTION_DROP)]
    return out


def attention_tensors(case, outs, grads):
    """-> [(name, tensor, compared rows (N, L) bool or None)] of an attention case's output and gradients: masked-out query
    rows of O are not compared (see attention_case)."""
    qm = case.cfg["q_mask"]
    return [("out0", outs[0], None if qm is None else qm > 0)] + [("grad%d" % i, g, None) for i, g in enumerate(grads)]


def block_errors(G, W, S, dh, rows=None):
    """Errors per block = (sequence, 16-row tile, dh-column block) of an (N, L, C) tensor -- what one wave of attention_train.hip
    computes as one tile of one head -- over the compared rows.  -> dict of (N, tiles, C // dh) tensors: kmax / smax = max|G - W| /
    max|S - W|, krms / srms, and cnt (compared elements; blocks with cnt == 0 hold no compared row)."""
    G, W, S = G.detach().cpu().double(), W.double(), S.double()
    n, l, c = W.shape
    assert G.shape == W.shape == S.shape and c % dh == 0
    nt = (l + 15) // 16
    keep = torch.ones(n, l, dtype=torch.bool) if rows is None else rows
    keep = torch.nn.functional.pad(keep, (0, nt * 16 - l))

    def blocks(e):
        e = torch.nn.functional.pad(e, (0, 0, 0, nt * 16 - l)) * keep[:, :, None]
        return e.view(n, nt, 16, c // dh, dh)
    eg, es = blocks((G - W).abs()), blocks((S - W).abs())
    cnt = keep.view(n, nt, 16).sum(2).double()[:, :, None].expand(n, nt, c // dh) * dh
    div = cnt.clamp_min(1)
    return dict(kmax=eg.amax((2, 4)), smax=es.amax((2, 4)), krms=(eg.pow(2).sum((2, 4)) / div).sqrt(),
                srms=(es.pow(2).sum((2, 4)) / div).sqrt(), cnt=cnt)


def check_blocks(name, case, G, W, S, dh, c, rows=None, c_rms=None):
    """Block-wise chain check: in every block max|G - W| <= c max|S - W| and rms(G - W) <= c_rms (c / 2) rms(S - W) (the block's own
    staged error, not the tensor's), and G == W exactly where S == W exactly.  A fault confined to one tile of small values (the
    far key tile of a short sequence, one head's column block) hides under the tensor-wide maximum of check_chain.
    -> worst max ratio, worst rms ratio, number of blocks."""
    c_rms = c / 2 if c_rms is None else c_rms
    e = block_errors(G, W, S, dh, rows)
    used = e["cnt"] > 0
    exact = used & (e["smax"] == 0)
    wrong = exact & (e["kmax"] != 0)
    assert not bool(wrong.any()), "%s %s: %d blocks differ from W where the staged reference is exact; (n, tile, column block) %s" % (
        name, case, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    live = used & ~exact
    one = torch.ones(())
    rmax = torch.where(live, e["kmax"] / torch.where(live, e["smax"], one), 0 * one)
    rrms = torch.where(live, e["krms"] / torch.where(live, e["srms"], one), 0 * one)
    wm, wr = float(rmax.max()), float(rrms.max())
    im = [int(x) for x in (rmax == rmax.max()).nonzero()[0]]
    ir = [int(x) for x in (rrms == rrms.max()).nonzero()[0]]
    print("NUMERICS %s %s bf16 blocks: %d worst max ratio %.3f at (n, tile, column block) %s kernel_err %.3e ref_err %.3e; "
          "worst rms ratio %.3f at %s" % (name, case, int(used.sum()), wm, im, float(e["kmax"][tuple(im)]),
                                          float(e["smax"][tuple(im)]), wr, ir))
    assert wm <= c, "%s %s: block (n, tile, column block) %s: max|G-W| %.3e > %g x the staged reference's %.3e in that block" % (
        name, case, im, float(e["kmax"][tuple(im)]), c, float(e["smax"][tuple(im)]))
    assert wr <= c_rms, "%s %s: block (n, tile, column block) %s: rms %.3e > %g x the staged reference's %.3e in that block" % (
        name, case, ir, float(e["krms"][tuple(ir)]), c_rms, float(e["srms"][tuple(ir)]))
    return wm, wr, int(used.sum())


# ---- ModularPoolFn ----------------------------------------------------------------------------------------------------------
def pool_cases():
    out = []
    for n, l, h in ((5, 11, 128), (4, 13, 100)):          # the 16-byte kernel (h % 8 == 0) and the scalar one
        for n_mod in (1, 2):
            enc, wm, mask = act(n, l, h, seed=1), par(n_mod, h, seed=2, scale=0.3), lens_mask(n, l, seed=3, lo=2)
            fn = lambda enc, wm, stage, mask=mask: f64.train_modular_pool(enc, mask, wm, stage)      # noqa: E731
            out.append(Case("ModularPoolFn", "%dx%dx%d m%d" % (n, l, h, n_mod), fn, [enc, wm], [True, True],
                            [act(n_mod, n, h, seed=4)], mask=mask))
    return out


# ---- VideoLevelScoresFn -----------------------------------------------------------------------------------------------------
def scores_cases():
    """video 2 is fully masked in every modality (score -1e10, gradients exactly zero); clip 0 of video 1 is an all-zero row
    (F.normalize clamps its norm; it is never the arg-max: some other clip has a positive cosine).  fused: the arg-kept
    one-launch backward; not fused: FUSED_LOSS_TAIL = False, clips padded to a multiple of 16, separate launches."""
    out = []
    for n, l, h in ((7, 19, 128), (9, 32, 64)):
        for n_mod in (1, 2):
            for fused in (True, False):
                ms = [lens_mask(n, l, seed=30 + i, lo=2) for i in range(n_mod)]
                qs, fs = [], []
                for i, m in enumerate(ms):
                    # The max over clips makes the gradient discontinuous in the operands: every (query, video) pair needs a
                    # winner that bf16 rounding of the normalised rows (~2^-8 of a cosine) cannot change.  All queries share a
                    # direction u; every video has one clip along u at a random valid position (not clip 0: video 1's is the
                    # zero row) -> its cosine is ~0.7 against < 0.4 for the other clips.
                    g = _gen(40 + i)
                    u = torch.nn.functional.normalize(torch.randn(h, generator=g), dim=0) * h ** 0.5
                    qs.append((u[None] + torch.randn(n, h, generator=g)).to(BF16))
                    f = torch.randn(n, l, h, generator=g)
                    peak = 1 + torch.randint(0, 10 ** 6, (n,), generator=g) % (m.sum(1).long() - 1)
                    f[torch.arange(n), peak] += 2.0 * u
                    f[1, 0] = 0
                    fs.append(f.to(BF16))
                    m[2] = 0

                def fn(*t, stage, ms=ms, n_mod=n_mod):
                    return f64.train_video_level_scores(t[:n_mod], t[n_mod:], ms, stage)
                out.append(Case("VideoLevelScoresFn", "%dx%dx%d m%d %s" % (n, l, h, n_mod, "fused" if fused else "padded"), fn,
                                qs + fs, [True] * (2 * n_mod), [act(n, n, seed=4).float()], chain=True, masks=ms, n_mod=n_mod,
                                fused=fused))
    return out


# ---- the loss tail ----------------------------------------------------------------------------------------------------------
# In the bf16 model (train.xml_forward_train) PairSimFn gets the bf16 query projection and the bf16 context and returns f32;
# SpanLossFn then runs on those f32 similarities and f32 filters, RankLossFn on VideoLevelScoresFn's f32 scores: these two have
# no bf16 form and run in f32 only.
def pair_sim_case():
    q, f2 = act(6, 128, seed=1), act(6, 23, 128, seed=2)
    fn = lambda q, f2, stage: f64.train_pair_sim(q, f2, stage)      # noqa: E731
    return Case("PairSimFn", "6x23x128", fn, [q, f2], [True, True], [act(6, 23, seed=4).float()])


def span_loss_cases():
    out = []
    n, l, ks = 9, 37, 5
    for merged, n_sim in ((True, 2), (False, 2), (False, 1)):
        sims = [act(n, l, seed=1 + i, scale=3.0).float() for i in range(n_sim)]
        mask = lens_mask(n, l, seed=5, lo=4)
        filters = [act(1, 1, ks, seed=10 + i, scale=0.5).float() for i in range(2 * (1 if merged else n_sim))]
        lens = mask.sum(1).long()
        g = _gen(7)
        st = torch.stack([torch.randint(0, int(x), (1,), generator=g)[0] for x in lens])
        ed = torch.stack([torch.randint(int(s), int(x), (1,), generator=g)[0] for s, x in zip(st, lens)])
        st_ed = torch.stack([st, ed], 1)

        def fn(*t, stage, n_sim=n_sim, mask=mask, st_ed=st_ed, merged=merged):
            return f64.train_span_loss(t[:n_sim], t[n_sim:], mask, st_ed, merged, ks)
        out.append(Case("SpanLossFn", "merged%d n_sim%d" % (merged, n_sim), fn, sims + filters, [True] * (n_sim + len(filters)),
                        [torch.ones(())], mask=mask, st_ed=st_ed, merged=merged, n_sim=n_sim, ks=ks))
    return out


def rank_loss_cases():
    out = []
    n = 17
    for lse in (False, True):
        scores = act(n, n, seed=1, scale=0.3).float()
        g = _gen(3)
        rc, rq = torch.randint(1, n, (n,), generator=g), torch.randint(1, n, (n,), generator=g)
        fn = lambda s, stage, rc=rc, rq=rq, lse=lse: f64.train_rank_loss(s, rc, rq, 0.1, lse)      # noqa: E731
        out.append(Case("RankLossFn", "lse%d" % lse, fn, [scores], [True], [act(2, seed=4).float()], rc=rc, rq=rq, lse=lse))
    return out


def all_cases():
    return (linear_cases() + layernorm_cases() + qkv_cases() + attention_cases() + pool_cases() + scores_cases() +
            [pair_sim_case()] + span_loss_cases() + rank_loss_cases())


def ids(cases):
    return [c.name for c in cases]
