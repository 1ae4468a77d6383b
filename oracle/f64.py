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
"""
import math

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
