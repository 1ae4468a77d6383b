"""float64 forms of the kernel-level oracle functions  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`oracle.xml_oracle` is the float32 restatement of the reference (its values are pinned by tests/test_oracle_golden.py and
stay as they are).  This module evaluates the same formulas in float64 on the SAME operand values (for bf16 storage: the
bf16-rounded tensors, widened), so that a kernel's and the float32 oracle's distances from the exact value can be compared
(tests/test_gpu_numerics.py).  The additive -10000 attention mask is kept, not "fixed": rows whose keys are all masked (or
padded query rows of cross attention) depend on float32's absorption of the score and keep the float32 oracle as their
expected value.

Every chain takes `stage`: a function applied where the bf16 kernels store an intermediate in the storage type (identity
for the exact value W; `bf16_round` for the staged reference S).  Boundaries modelled (attention.hip header):
projected Q / K / V, the normalised probabilities P (they reach the P.V MFMA through an LDS patch in the storage type), the
attention context, K1's ReLU output + position rows (`pre_ln=True`: only the LayerNorm-epilogue GEMM stores the
pre-LayerNorm value in the storage type; the unfused path keeps it in f32).

The training nodes (autograd.py) have autograd references at the end of this module (`train_*`): there `staged` applies the
stage to the forward value AND / OR to the gradient crossing the same point, as the bf16 backward kernels store gradients too.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import xml_oracle as O


def d(x):
    return O._t(x).double()


def ident(x):
    return x


def bf16_round(x):
    """round to nearest even onto the bf16 grid (through float32: the kernels round an f32 value)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


class Weights64(O.Weights):
    def sub(self, name):
        return Weights64(self.sd, self.prefix + name + ".")

    def __getitem__(self, name):
        return O._t(self.sd[self.prefix + name]).double()


def mask_logits(target, mask):
    return O.mask_logits(d(target), d(mask))


def layer_norm_plain(x, g, b):
    x = d(x)
    return F.layer_norm(x, (x.shape[-1],), d(g), d(b), O.LN_EPS)


def layer_norm(x, w, prefix):
    return O.layer_norm(d(x), w, prefix)


def l2norm_rows(x, eps=None):
    """F.normalize(dim=-1) (eps None: x / max(|x|, 1e-12)) or the dataset form x / (|x| + eps)."""
    x = d(x)
    n = x.norm(dim=-1, keepdim=True)
    return x / n.clamp_min(1e-12) if eps is None else x / (n + eps)


def linear(x, w, b=None, relu=False, addend=None):
    y = F.linear(d(x), d(w), None if b is None else d(b))
    if addend is not None:
        y = y + d(addend)
    return y.clamp_min(0) if relu else y


def linear_layer(x, w):
    return O.linear_layer(d(x), w)


def trainable_pos_enc(x, w, stage=ident, pre_ln=False):
    x = d(x)
    pos = w["position_embeddings.weight"][:x.shape[1]]
    y = x + pos.unsqueeze(0)
    return layer_norm(stage(y) if pre_ln else y, w, "LayerNorm")


def linear_ln_relu_pos(x, w_proj, w_pos, stage=ident, pre_ln=False):
    """K1+K2: LN -> linear -> ReLU -> + position rows -> LN.  The LayerNorm'd input is the GEMM's A operand (storage type)."""
    a = stage(layer_norm(d(x), w_proj, "LayerNorm"))
    y = F.relu(F.linear(a, w_proj["net.1.weight"], w_proj["net.1.bias"]))
    return trainable_pos_enc(y, w_pos, stage, pre_ln)


def attention_probs(q_states, k_states, att_mask, w, n_heads, stage=ident):
    n, lq, hsz = q_states.shape
    lk = k_states.shape[1]
    dh = hsz // n_heads
    add_mask = (1 - d(att_mask).unsqueeze(1)) * O.ATT_NEG
    q = stage(F.linear(d(q_states), w["query.weight"], w["query.bias"])).view(n, lq, n_heads, dh).permute(0, 2, 1, 3)
    k = stage(F.linear(d(k_states), w["key.weight"], w["key.bias"])).view(n, lk, n_heads, dh).permute(0, 2, 1, 3)
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh) + add_mask
    return scores, torch.softmax(scores, dim=-1)


def bert_self_attention(q_states, k_states, v_states, att_mask, w, n_heads, stage=ident):
    n, lq, hsz = q_states.shape
    lk = k_states.shape[1]
    dh = hsz // n_heads
    _, probs = attention_probs(q_states, k_states, att_mask, w, n_heads, stage)
    v = stage(F.linear(d(v_states), w["value.weight"], w["value.bias"])).view(n, lk, n_heads, dh).permute(0, 2, 1, 3)
    ctx = torch.matmul(stage(probs), v)
    return stage(ctx.permute(0, 2, 1, 3).contiguous().view(n, lq, hsz))


def attention_core(q, k, v, q_mask, k_mask, n_heads, stage=ident):
    """BertSelfAttention behind its projections (q, k, v given)."""
    n, lq, hsz = q.shape
    lk = k.shape[1]
    dh = hsz // n_heads
    att = d(k_mask).unsqueeze(1) if q_mask is None else torch.einsum("bm,bn->bmn", d(q_mask), d(k_mask))
    sp = lambda t, l: d(t).view(n, l, n_heads, dh).permute(0, 2, 1, 3)      # noqa: E731
    scores = torch.matmul(sp(q, lq), sp(k, lk).transpose(-1, -2)) / math.sqrt(dh) + (1 - att.unsqueeze(1)) * O.ATT_NEG
    probs = torch.softmax(scores, dim=-1)
    ctx = torch.matmul(stage(probs), sp(v, lk))
    return ctx.permute(0, 2, 1, 3).contiguous().view(n, lq, hsz), probs


def bert_self_output(hidden, residual, w, stage=ident, pre_ln=False):
    y = F.linear(d(hidden), w["dense.weight"], w["dense.bias"]) + d(residual)
    return layer_norm(stage(y) if pre_ln else y, w, "LayerNorm")


def bert_attention(x, att_mask, w, n_heads, stage=ident, pre_ln=False):
    a = bert_self_attention(x, x, x, att_mask, w.sub("self"), n_heads, stage)
    return bert_self_output(a, x, w.sub("output"), stage, pre_ln)


def cross_attention(main, main_mask, side, side_mask, w_att, ln_g, ln_b, n_heads, stage=ident):
    cross_mask = torch.einsum("bm,bn->bmn", d(main_mask), d(side_mask))
    cross = bert_self_attention(main, side, side, cross_mask, w_att, n_heads, stage)
    return layer_norm_plain(cross + d(main), ln_g, ln_b)


def modular_pool(enc, mask, w_m):
    """get_modularized_queries: softmax over tokens of enc . w_m, masked -> (n_mod, N, H), and the token probabilities."""
    enc = d(enc)
    sc = torch.softmax(mask_logits(enc @ d(w_m).t(), d(mask).unsqueeze(2)), dim=1)
    return torch.einsum("blm,bld->mbd", sc, enc), sc


def q2c_scores(q, c, mask):
    """get_video_level_scores behind the normalisation: per-clip cosines (Nq, L, Nv) masked, and their max over clips."""
    s = mask_logits(torch.einsum("md,nld->mln", d(q), d(c)), d(mask).t().unsqueeze(0))
    return torch.max(s, dim=1)[0], s


# ---- training ops: staged float64 AUTOGRAD references (tests/test_gpu_train_bf16.py) ----------------------------------------
# The bf16 training nodes of tvretrieval_amd/autograd.py store activations AND gradients in bf16.  `staged` is the
# straight-through form of `stage` for autograd: the forward value and / or the gradient crossing the boundary is put through
# `stage`; with stage = ident the node is not even recorded, so the reference IS plain float64 autograd (the exact value W).
# Each reference below is plain torch autograd in the dtype of its leaves (float64 for W and S; float32 gives the float32
# reference R of numerics_regimes.check_bf16_rounding) and names the stores it models.
class _Staged(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.clone() if fwd is None else fwd(x).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return (g if ctx.bwd is None else ctx.bwd(g).to(g.dtype)), None, None


def staged(x, stage=ident, fwd=True, bwd=True):
    """x with `stage` applied to its value (fwd) and to the gradient that flows back through this point (bwd)."""
    if stage is ident or not (fwd or bwd):
        return x
    return _Staged.apply(x, stage if fwd else None, stage if bwd else None)


def operand(w):
    """an f32 master parameter as the bf16 GEMM operand the kernels read (ops.pack_weights / BertAdam.refresh_shadows round
    it to nearest); its gradient stays f32 and goes to the master unchanged.  Part of the OPERANDS: applied for W and S alike."""
    return _Staged.apply(w, bf16_round, None)


def train_linear(x, w, b, relu, stage=ident):
    """LinearFn.  bf16 stores: y (ops.linear's epilogue, behind the ReLU) and dX (ops.linear on W^T: LinearFn.backward; the
    zero-padded reduction columns of n % 8 add exact zeros).  relu_bwd passes dY or 0: no rounding.  dW / db: f32 sums
    (gemm_tn, or transposes + split-K; colsum) of products of the bf16 values -- no boundary."""
    y = F.linear(staged(x, stage, fwd=False), operand(w), b)
    return staged(y.clamp_min(0) if relu else y, stage, bwd=False)


def train_layernorm(a, b, g, beta, stage=ident):
    """LayerNormFn without dropout sites.  bf16 stores: y (xml_add_layernorm) and dx (layernorm_bwd_kernel's st8 in dy's type;
    ONE dx serves a and b, ops.convert widens it exactly where `a` is f32).  Statistics, dgamma, dbeta: f32."""
    x = a if b is None else a + b
    y = F.layer_norm(staged(x, stage, fwd=False), (x.shape[-1],), g, beta, O.LN_EPS)
    return staged(y, stage, bwd=False)


def train_qkv(x, ws, bs, stage=ident, residual=None):
    """QkvFn / QkvResFn: one GEMM on the row-stacked weights.  bf16 stores: y, and dX --
    residual None: dX = rne(dY W);  "epilogue": the residual gradient is the addend of the dX GEMM, dX = rne(dY W + dres), one
    store;  "fallback" (dres in another dtype): rne(dY W) + dres in torch.  -> y, or (y, x as the residual operand)."""
    w = torch.cat([operand(w_) for w_ in ws], 0)
    bias = torch.cat(list(bs), 0)
    if residual == "fallback":
        return staged(F.linear(staged(x, stage, fwd=False), w, bias), stage, bwd=False), x
    xs = staged(x, stage, fwd=False)
    y = staged(F.linear(xs, w, bias), stage, bwd=False)
    return y if residual is None else (y, xs)


def drop_keep(count, p, seed):
    """Host model of xml_dropout's mask: keep[i] for the elements i = 0 .. count - 1 of a tensor (numpy bool).  Restates
    common.h: xml_seed_words (s0 = low seed word, s1 = high word * 0x27D4EB2F + 0x165667B1) and drop_hash, in uint64 arithmetic
    cut to 32 bits after every step; element i is kept when hash(i) >= uint32(double(float32 p) * 2^32).  No base seed
    (train_ops.SEED_BASE is None outside a captured step)."""
    m32 = np.uint64(0xFFFFFFFF)
    seed = int(seed) % (1 << 64)
    s0 = np.uint64(seed & 0xFFFFFFFF)
    s1 = np.uint64(((seed >> 32) * 0x27D4EB2F + 0x165667B1) & 0xFFFFFFFF)
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0) & 0xFFFFFFFF)
    i = np.arange(count, dtype=np.uint64)
    h = ((i & m32) * np.uint64(0x9E3779B1) + s0) & m32
    h ^= ((i >> np.uint64(32)) * np.uint64(0x85EBCA77)) & m32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h ^= h >> np.uint64(13)
    h = (h + s1) & m32
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h ^= h >> np.uint64(16)
    return h >= thresh


def drop_scale(p):
    """the factor of a kept element, 1 / (1 - p) in float32 arithmetic as xml_dropout and attention_train.hip compute it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def attention_drop(n, heads, lq, lk, p, seed):
    """The factor keep / (1 - p) of every probability, (N, heads, Lq, Lk) float64: the mask of the (N * heads, lq8, lk8) tensor
    of the unfused chain (lengths padded to multiples of 8), which the fused kernels index the same way."""
    lq8, lk8 = (lq + 7) // 8 * 8, (lk + 7) // 8 * 8
    keep = torch.from_numpy(drop_keep(n * heads * lq8 * lk8, p, seed)).view(n, heads, lq8, lk8)[:, :, :lq, :lk]
    return keep.double() * drop_scale(p)


def train_attention(q, k, v, q_mask, k_mask, n_heads, stage=ident, drop=None):
    """AttentionCoreFn / AttentionKvFn / AttentionQkvFn, fused (attention_train.hip) and -- for p_drop = 0 -- unfused chain alike.
    bf16 stores: P where it feeds P V and P^T dO (LDS patch / attn_softmax's P, P^T; the softmax backward itself uses the f32
    P), the context O, dS = P (dP - delta) / sqrt(dh) (LDS / attn_softmax's dS, dS^T: the gradient of the RAW Q K^T), and
    dQ, dK, dV.  S and dP stay f32 (accumulators / out_f32 GEMMs).
    drop: None, or the (N, heads, Lq, Lk) factors keep / (1 - p) (`attention_drop`) of the FUSED kernels' dropout: the f32
    probabilities are multiplied in registers and Pd = rne(P o M / (1 - p)) is what is stored -- forward: at_tile_times_rows' patch
    store in front of Pd V; backward: the Pd^T store into R2 in step 4, in front of dV = Pd^T dO.  dPd = dO V^T comes out of the
    accumulators and dP = dPd o M / (1 - p), delta and the softmax backward (on the f32 P, not on Pd) stay f32 (step 2); dS is
    rounded where it is without dropout (patch in step 3, dS^T in step 4).  The unfused chain rounds P to bf16 BEFORE its
    dropout launch and the product again: another staging, not modelled here."""
    n, lq, hsz = q.shape
    lk = k.shape[1]
    dh = hsz // n_heads
    km = k_mask.to(q.dtype)
    att = km.unsqueeze(1) if q_mask is None else torch.einsum("bm,bn->bmn", q_mask.to(q.dtype), km)
    sp = lambda t, l: staged(t, stage, fwd=False).view(n, l, n_heads, dh).permute(0, 2, 1, 3)      # noqa: E731
    raw = staged(torch.matmul(sp(q, lq), sp(k, lk).transpose(-1, -2)), stage, fwd=False)
    probs = torch.softmax(raw / math.sqrt(dh) + (1 - att.unsqueeze(1)) * O.ATT_NEG, dim=-1)
    if drop is not None:
        probs = probs * drop.to(probs.dtype)
    ctx = torch.matmul(staged(probs, stage, bwd=False), sp(v, lk))
    return staged(ctx.permute(0, 2, 1, 3).contiguous().view(n, lq, hsz), stage, bwd=False)


def train_modular_pool(enc, mask, wm, stage=ident):
    """ModularPoolFn.  bf16 stores: the pooled rows and denc; the softmax over tokens and dwm (f32 master, read as f32) are f32."""
    e = staged(enc, stage, fwd=False)
    sc = torch.softmax(O.mask_logits(e @ wm.t(), mask.to(e.dtype).unsqueeze(2)), dim=1)
    return staged(torch.einsum("blm,bld->mbd", sc, e), stage, bwd=False)


def train_video_level_scores(qs, fs, masks, stage=ident):
    """VideoLevelScoresFn.  bf16 stores: the normalised rows qn / cn (ops.l2norm_rows) and dquery / dfeat.  l2norm_bwd
    differentiates the normalisation of the UNROUNDED row (straight through the store of qn / cn); the cosines, their max and
    d(qn), d(cn) are f32 (scores f32; loss_tail.hip keeps the gradient of the normalised row in registers, the separate
    launches in f32 tensors)."""
    tot = 0
    for q, c, m in zip(qs, fs, masks):
        qn = staged(F.normalize(staged(q, stage, fwd=False), dim=-1), stage, bwd=False)
        cn = staged(F.normalize(staged(c, stage, fwd=False), dim=-1), stage, bwd=False)
        s = O.mask_logits(torch.einsum("md,nld->mln", qn, cn), m.to(qn.dtype).t().unsqueeze(0))
        tot = tot + torch.max(s, dim=1)[0]
    return tot / len(qs)


def train_pair_sim(q, f2, stage=ident):
    """PairSimFn: sim f32; bf16 stores: dq and df2."""
    return torch.einsum("bd,bld->bl", staged(q, stage, fwd=False), staged(f2, stage, fwd=False))


def span_logits(sims, filters, mask, merged, ks):
    """The masked start / end logits (N, L) of the span head.  mask: one (N, L) mask for every stream, or a list / tuple with
    one mask per stream (the split form masks stream i with mask i; the merged form has one stream and uses the first)."""
    n_sim = len(sims)
    masks = list(mask) if isinstance(mask, (list, tuple)) else [mask] * n_sim
    masks = [m.to(sims[0].dtype) for m in masks]
    conv = lambda s, w: F.conv1d(s.unsqueeze(1), w, padding=ks // 2).squeeze(1)     # noqa: E731
    if merged:
        s = (sims[0] + sims[1]) / 2
        lst, led = O.mask_logits(conv(s, filters[0]), masks[0]), O.mask_logits(conv(s, filters[1]), masks[0])
    else:
        lst = sum(O.mask_logits(conv(sims[i], filters[i]), masks[i]) for i in range(n_sim)) / n_sim
        led = sum(O.mask_logits(conv(sims[i], filters[n_sim + i]), masks[i]) for i in range(n_sim)) / n_sim
    return lst, led


def convse(q, f, masks, pair_q, pair_vid, conv_w, l_ref, merged, ks, softmax=False, dtype=torch.float64):
    """K7 / span evidence on explicit pairs, in `dtype` (float64: the exact value W; float32: the reference's own arithmetic R).
    q[m] (Nq, H), f[m] (Nv, Lpad, H): the STORED operand values; masks[m] (Nv, Lpad) -- one mask per stream, the merged form
    uses the first; pair_q, pair_vid (P,): pair p = query row pair_q[p] x video pair_vid[p], a video outside [0, Nv) = a
    skipped pair (zero rows); conv_w flat [st filters..., ed filters...], one pair of filters per unmerged stream.
    Similarities by einsum on the listed pairs only; taps zero-padded at l_ref (clips >= l_ref do not exist), mask_logits
    behind the filter, the mean over unmerged streams, optionally the softmax over the first l_ref clips.
    -> dict of (P, Lpad) rows, entries l >= l_ref zero: st, ed, sims (list, unmasked), sim (their mean)."""
    n_mod, n_conv = len(q), 1 if merged else len(q)
    nv, lpad = f[0].shape[0], f[0].shape[1]
    pq, pv = O._t(pair_q).long(), O._t(pair_vid).long()
    ok = (pv >= 0) & (pv < nv)
    pqc, pvc = pq.clamp(min=0), pv.clamp(0, nv - 1)
    sims = [torch.einsum("pd,pld->pl", O._t(q[m]).to(dtype)[pqc], O._t(f[m]).to(dtype)[pvc, :l_ref]) for m in range(n_mod)]
    cw = O._t(conv_w).to(dtype)
    filters = [cw[i * ks:(i + 1) * ks].view(1, 1, ks) for i in range(2 * n_conv)]
    mk = [O._t(masks[0 if merged else m]).to(dtype)[pvc, :l_ref] for m in range(n_conv)]
    st, ed = span_logits(sims, filters, mk, merged, ks)
    if softmax:
        st, ed = torch.softmax(st, -1), torch.softmax(ed, -1)

    def rows(x):
        out = x.new_zeros(x.shape[0], lpad)
        out[:, :l_ref] = x
        out[~ok] = 0
        return out
    return dict(st=rows(st), ed=rows(ed), sims=[rows(s) for s in sims], sim=rows(sum(sims) / n_mod))


def q2c_rescore(qn, cn, masks, pair_vid, dtype=torch.float64):
    """xml_q2c_rescore: out[q, j] = sum_m max_l mask_logits(qn_m[q] . cn_m[v, l]) / n_mod for v = pair_vid[q, j]; -inf for a
    video outside [0, Nv).  Stored operand values, `dtype` arithmetic."""
    pv = O._t(pair_vid).long()
    nq, kp = pv.shape
    nv = cn[0].shape[0]
    ok = (pv >= 0) & (pv < nv)
    pvc = pv.clamp(0, nv - 1).reshape(-1)
    pq = torch.arange(nq).repeat_interleave(kp)
    tot = 0
    for m in range(len(qn)):
        s = torch.einsum("pd,pld->pl", O._t(qn[m]).to(dtype)[pq], O._t(cn[m]).to(dtype)[pvc])
        tot = tot + O.mask_logits(s, O._t(masks[m]).to(dtype)[pvc]).max(1)[0]
    out = (tot / len(qn)).view(nq, kp)
    out[~ok] = float("-inf")
    return out


def train_span_loss(sims, filters, mask, st_ed, merged, ks):
    """SpanLossFn (f32 in the bf16 model too: PairSimFn's output is f32): no bf16 boundary.  mask: see `span_logits`."""
    lst, led = span_logits(sims, filters, mask, merged, ks)
    return F.cross_entropy(lst, st_ed[:, 0]) + F.cross_entropy(led, st_ed[:, 1])


def rank_order(scores_masked):
    """(N, N) -> the column order of every row, descending, equal values: lower index first (rank_loss_kernel's documented
    rule; a stable sort -- without it torch leaves the order of ties undefined)."""
    return torch.sort(scores_masked, descending=True, dim=1, stable=True)[1]


def train_rank_loss(scores, ranks_ctx, ranks_q, margin, lse):
    """RankLossFn (f32 scores from VideoLevelScoresFn): no bf16 boundary.  Ties: lower index first (`rank_order`)."""
    n = scores.shape[0]
    ar = torch.arange(n)
    pos = scores[ar, ar]
    masked = scores.detach().clone()
    masked[ar, ar] = 999

    def neg(sc, scm, r):
        return sc[ar, rank_order(scm)[ar, r.long()]]

    def rl(p, ng):
        # margin + (neg - pos), the difference first: a fully masked video has pos = neg = -1e10, whose difference is exactly 0,
        # whereas (margin + neg) - pos loses the margin to absorption (all of it in float32, 1e-6 of it in float64)
        return torch.log1p(torch.exp(ng - p)).sum() / n if lse else torch.clamp(margin + (ng - p), min=0).sum() / n
    return torch.stack([rl(pos, neg(scores, masked, ranks_ctx)), rl(pos, neg(scores.t(), masked.t(), ranks_q))])
