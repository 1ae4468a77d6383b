"""Operand regimes of a TRAINED XML checkpoint, built synthetically (no checkpoint is in the tree), and the assertion
helpers of tests/test_gpu_numerics.py.  No GPU is needed to import or to use this module: tests/test_numerics_reference.py
feeds the helpers with the float32 oracle and with deliberately wrong stand-ins.

Three values on the same operands:  W float64 (oracle/f64.py),  R the float32 oracle (torch on the CPU),  G the kernel.
* f32 storage / split-f16:  max|G - W| <= c * max|R - W| + FLOOR_ULPS f32 ulps of the output scale   (`check_f32`)
* bf16 storage, one rounding:  G is a correct round-to-nearest of a value within that allowance of W (bit equal to rne(W)
  off the rounding boundaries, either neighbour on one); boundary elements under 1 % of the case and the mean signed error
  (along the magnitude) within 4 * 0.29 / sqrt(n) ulp (round-to-nearest: mean 0, sigma 0.29 ulp; truncation: mean -0.5 ulp)
  wherever the correctly rounded reference meets them itself   (`check_bf16_rounding`, BF16_STRICT)
* bf16 storage, fused chains:  against the staged float64 reference S (bf16 at the documented stage boundaries):
  max|G - W| <= margin * max|S - W|, rms(G - W) <= 2 rms(S - W), mean signed error equal to S's within
  4 rms(G - S) / sqrt(rows)   (`check_bf16_chain`)
Each check prints `kernel regime storage: kernel_err ref_err ratio` (profiles/numerics_margins.md holds the table).
"""
import math

import torch

F32_ULP = 2.0 ** -24          # half the spacing of f32 at 1.0: the unit roundoff
FLOOR_ULPS = 4                # "a few f32 ulps of the output scale": what an exactly rounded f32 chain of 2-3 ops may add
BOUNDARY_CAP = 0.01           # share of a case's elements that may sit on a bf16 rounding boundary
BIAS_SIGMA = 0.29             # sigma of a round-to-nearest error in ulps (uniform on [-0.5, 0.5])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def grid(t, dtype):
    """the operand values a kernel of storage type `dtype` gets, as float32."""
    return t.to(dtype).to(torch.float32)


# ---- LayerNorm / GEMM input rows ------------------------------------------------------------------------------------------
def gaussian(rows, d, seed=0):
    """unit Gaussians: the regime of the existing suite (the control)."""
    return torch.randn(rows, d, generator=_gen(seed))


def outlier_channels(rows, d, seed=0):
    """BERT-like rows: unit Gaussians with 4 of the d channels multiplied by 8 ... 30."""
    g = _gen(seed)
    x = torch.randn(rows, d, generator=g)
    ch = torch.randperm(d, generator=g)[:4]
    x[:, ch] *= torch.tensor([8.0, 15.0, 22.0, 30.0])
    return x


def post_relu_unit(rows, d, seed=0):
    """what the video input projection's LayerNorm sees: relu(randn) rows, L2-normalised (ResNet/I3D features)."""
    x = torch.relu(torch.randn(rows, d, generator=_gen(seed)))
    return x / x.norm(dim=-1, keepdim=True)


def offset(rows, d, mean, seed=0):
    """rows with a mean far from zero (mean + randn): LayerNorm's variance must not be E[x^2] - E[x]^2."""
    return mean + torch.randn(rows, d, generator=_gen(seed))


def tiny(rows, d, seed=0):
    """1e-4 * randn: the variance (1e-8) is far below LayerNorm's eps."""
    return 1e-4 * torch.randn(rows, d, generator=_gen(seed))


def constant(rows, d, seed=0):
    """rows of one repeated value (variance exactly 0; values on the bf16 grid so that every storage type keeps them)."""
    v = (torch.randn(rows, 1, generator=_gen(seed)) * 3).to(torch.bfloat16).float()
    return v.expand(rows, d).contiguous()


def one_hot(rows, d, seed=0):
    """one non-zero channel per row: the LayerNorm output reaches sqrt(d)."""
    x = torch.zeros(rows, d)
    idx = torch.randint(0, d, (rows,), generator=_gen(seed))
    x[torch.arange(rows), idx] = 1.0
    return x


ROW_REGIMES = {
    "gaussian": gaussian, "outlier_channels": outlier_channels, "post_relu_unit": post_relu_unit,
    "offset10": lambda r, d, seed=0: offset(r, d, 10.0, seed), "offset1e3": lambda r, d, seed=0: offset(r, d, 1e3, seed),
    "tiny": tiny, "constant": constant, "one_hot": one_hot,
}


def mixed(rows, d, seed=0):
    """all row regimes interleaved row by row: neighbours in one tile differ by 7 decades."""
    names = sorted(k for k in ROW_REGIMES if k != "mixed")
    parts = [ROW_REGIMES[nm](rows, d, seed + i) for i, nm in enumerate(names)]
    x = torch.empty(rows, d)
    for r in range(rows):
        x[r] = parts[r % len(names)][r]
    return x


ROW_REGIMES["mixed"] = mixed


def ln_params(d, seed=0):
    g = _gen(seed)
    return 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


# ---- peaked softmaxes -------------------------------------------------------------------------------------------------
def peaked_attention_weights(h, logit_std, seed=0):
    """BertAttention weights whose Q/K projections give attention logits of standard deviation ~logit_std on unit-Gaussian
    inputs (2: mean max probability ~0.1 ... 12: ~1).  q, k entries have sd s -> logit q.k/sqrt(dh) has sd s^2."""
    g = _gen(seed)
    s = math.sqrt(logit_std)
    sd = {}
    for nm in ("query", "key", "value"):
        sc = (s if nm != "value" else 1.0) * h ** -0.5
        sd["self.%s.weight" % nm] = torch.randn(h, h, generator=g) * sc
        sd["self.%s.bias" % nm] = 0.1 * torch.randn(h, generator=g)
    sd["output.dense.weight"] = torch.randn(h, h, generator=g) * h ** -0.5
    sd["output.dense.bias"] = 0.1 * torch.randn(h, generator=g)
    sd["output.LayerNorm.weight"] = 1 + 0.1 * torch.randn(h, generator=g)
    sd["output.LayerNorm.bias"] = 0.1 * torch.randn(h, generator=g)
    return sd


def peaked_pool_vector(n_mod, h, logit_std, seed=0):
    """modular_vector_mapping rows giving pooling logits of sd ~logit_std on unit-Gaussian token rows."""
    return torch.randn(n_mod, h, generator=_gen(seed)) * (logit_std * h ** -0.5)


# ---- K6: near-duplicate clips -----------------------------------------------------------------------------------------
def near_duplicate_clips(nq, nv, l, h, seed=0):
    """L2-normalised clips = a query vector + noise of relative norm 0.45 ... 1e-4 (cosines 0.9 ... 1 - 5e-9): the max over
    clips is decided in the last bits.  The last video is an exact duplicate of video 0 (ties); channel 0 of every
    fourth clip is -0.0.  Returns q (nq, h), c (nv, l, h)."""
    g = _gen(seed)
    q = torch.nn.functional.normalize(torch.randn(nq, h, generator=g), dim=-1)
    sig = torch.logspace(math.log10(0.45), -4, l)[torch.randperm(l, generator=g)]
    base = q[torch.arange(nv) % nq]
    noise = torch.nn.functional.normalize(torch.randn(nv, l, h, generator=g), dim=-1)
    c = torch.nn.functional.normalize(base[:, None, :] + sig[None, :, None] * noise, dim=-1)
    c[:, ::4, 0] = -0.0
    if nv > 1:
        c[-1] = c[0]
    return q, c


# ---- masks ------------------------------------------------------------------------------------------------------------
def prefix_masks(n, l, seed=0):
    """prefix masks with the edges: sequence 0 full length, sequence 1 of length 1."""
    lens = torch.randint(1, l + 1, (n,), generator=_gen(seed))
    lens[0] = l
    if n > 1:
        lens[1] = 1
    return (torch.arange(l)[None] < lens[:, None]).float()


def hole_masks(n, l, seed=0):
    """masks with holes (1 1 0 1 0 ...): random bits, position 0 always valid; sequence 0 full, sequence 1 only position 0."""
    m = (torch.rand(n, l, generator=_gen(seed)) < 0.6).float()
    m[:, 0] = 1
    m[0] = 1
    if n > 1:
        m[1] = 0
        m[1, 0] = 1
    return m


def is_prefix(mask):
    return bool((mask[:, 1:] <= mask[:, :-1]).all()) and bool((mask[:, 0] == 1).all())


# ---- assertion helpers ------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().cpu().double()


def bf16_ulp(w):
    """spacing of the bf16 grid at |w| (8 significand bits; the grid of the smallest normal binade below it)."""
    e = torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def report(kernel, regime, storage, kernel_err, ref_err):
    ratio = kernel_err / ref_err if ref_err > 0 else (0.0 if kernel_err == 0 else float("inf"))
    print("NUMERICS %s %s %s: kernel_err %.3e ref_err %.3e ratio %.2f" % (kernel, regime, storage, kernel_err, ref_err, ratio))
    return ratio


def check_finite(name, got, ref):
    got, ref = _d(got), _d(ref)
    bad = ~torch.isfinite(got) & torch.isfinite(ref)
    assert not bool(bad.any()), "%s: %d non-finite outputs where the reference is finite" % (name, int(bad.sum()))


def f32_allowance(W, R, c, scale=None):
    """c * max|R - W| + FLOOR_ULPS f32 ulps, in units of `scale` (per element or scalar; default max|W|)."""
    W, R = _d(W), _d(R)
    scale = W.abs().max().clamp_min(2.0 ** -126) if scale is None else _d(torch.as_tensor(scale))
    ref_err = float(((R - W).abs() / scale).max())
    return c * ref_err + FLOOR_ULPS * 2 * F32_ULP, ref_err, scale


def check_f32(kernel, regime, G, W, R, c, scale=None, storage="f32"):
    """f32-grade: the kernel is at most c times as far from float64 as the float32 reference, plus the floor."""
    check_finite("%s %s" % (kernel, regime), G, R)
    G, W = _d(G), _d(W)
    assert G.shape == W.shape, (G.shape, W.shape)
    lim, ref_err, scale = f32_allowance(W, R, c, scale)
    err = (G - W).abs() / scale
    kerr = float(err.max())
    report(kernel, regime, storage, kerr, ref_err)
    assert kerr <= lim, "%s %s %s: max|G-W| = %.3e of the output scale at %s; float32 reference %.3e, limit %.3e (c = %g)" % (
        kernel, regime, storage, kerr, tuple(int(i) for i in (err == err.max()).nonzero()[0]), ref_err, lim, c)
    return kerr, ref_err


# bf16 storage, one rounding.  ALWAYS asserted, every regime: G is a correct round-to-nearest of SOME value within the f32
# allowance of W, i.e. rne(W - allow) <= G <= rne(W + allow) -- where W is not within the allowance of a rounding boundary
# that is bit equality with rne(W) (no half-ulp slack at all; a truncating store differs on half of those elements), on a
# boundary either neighbour.  This implies the issue's "half an ulp + allowance, one ulp on a boundary".
# On top of it, the issue's two statistics -- boundary share < 1 % and |mean signed error| <= 4 * 0.29 / sqrt(n) -- are
# asserted on the regimes where the float32 reference rounded by torch meets them itself (BF16_STRICT; proved by
# tests/test_numerics_reference.py).  On the others they CANNOT hold for a correct kernel: the outputs repeat (constant
# rows, one_hot rows, l2norm of offset rows: 768 near-equal values -> the rounding errors are one draw, not n), or the
# reference's own f32 error is a sizeable share of a bf16 ulp (LayerNorm at mean 1e3).  There the derived bound is the
# bit equality above on the decided elements, whose share must be at least DECIDED_MIN so that the check keeps its teeth.
BF16_STRICT = {"layernorm": ("gaussian", "post_relu_unit", "tiny"),
               "l2norm": ("gaussian", "offset10", "one_hot", "post_relu_unit", "tiny"),
               "linear": ("gaussian", "offset10", "outlier_channels", "post_relu_unit")}
DECIDED_MIN = 0.25


def _rne_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def check_bf16_rounding(kernel, regime, G, W, R, c, scale=None, strict=True, cap=None):
    """bf16 output = ONE round-to-nearest of an f32-grade value (see the comment above BF16_STRICT)."""
    check_finite("%s %s" % (kernel, regime), G, R)
    G, W = _d(G), _d(W)
    assert G.shape == W.shape, (G.shape, W.shape)
    _, ref_err, scale = f32_allowance(W, R, c, scale)
    # the f32 value under the rounding: c times the float32 reference's worst error (in units of the scale) plus a few f32
    # ulps OF THE ELEMENT (the floor in units of the largest output would put every small element on a "boundary")
    allow = c * ref_err * scale + FLOOR_ULPS * 2 * F32_ULP * W.abs()
    lo, hi = _rne_bf16(W - allow), _rne_bf16(W + allow)
    boundary = (lo != hi) & (W != 0)           # an exact zero (ReLU) has no boundary: G within the rounded allowance
    share = float(boundary.double().mean())
    bad = (G < lo) | (G > hi)
    ulp = bf16_ulp(torch.maximum(W.abs(), G.abs()))
    err_ulp = (G - W) * torch.sign(W) / ulp      # signed along the magnitude: a store that truncates toward zero shows as -0.5
    n = err_ulp.numel()
    bias, bias_lim = float(err_ulp.mean()), 4 * BIAS_SIGMA / math.sqrt(n)
    wrong = int((G != _rne_bf16(W))[~boundary].sum())
    print("NUMERICS %s %s bf16: max_err %.3f ulp  mean_signed %.2e ulp (limit %.2e)  boundary share %.2e  f32 ref_err %.3e"
          % (kernel, regime, float(err_ulp.abs().max()), bias, bias_lim, share, ref_err))
    assert not bool(bad.any()), "%s %s bf16: %d/%d are not a correct rounding of any value within the allowance (%d decided " \
        "elements differ from rne(W)); worst %.3f ulp" % (kernel, regime, int(bad.sum()), n, wrong, float(err_ulp.abs()[bad].max()))
    cap = strict if cap is None else cap     # cap=False: outputs much smaller than the case's largest (pooled rows) sit within
    if cap:                                  # the global allowance of a boundary; the bias bound still holds and is asserted
        assert share < BOUNDARY_CAP, "%s %s: %.2f %% of the elements sit on a rounding boundary" % (kernel, regime, 100 * share)
    else:
        assert 1 - share >= DECIDED_MIN, "%s %s: only %.1f %% of the elements are decided" % (kernel, regime, 100 * (1 - share))
    if strict:
        assert abs(bias) <= bias_lim, "%s %s bf16: mean signed error %.3e ulp, limit %.3e (truncation gives -0.5)" % (
            kernel, regime, bias, bias_lim)
    return float(err_ulp.abs().max()), bias


def check_bf16_chain(kernel, regime, G, W, S, margin, ref=None, rows=None):
    """bf16 chain with bf16 intermediates: max|G - W| within `margin` of the staged reference's own distance from W, RMS
    within twice the staged reference's, and the mean signed error equal to the staged reference's within
    4 * rms(G - S) / sqrt(rows): the kernel and the staged reference round at the same places, so G - S is a zero-mean
    difference of roundings; elements of one row share their LayerNorm statistics and softmax rows, so a ROW counts as one
    independent draw (conservative).  Errors are in bf16 ulps of max(|W|, rms W / 4): near a zero crossing an output's own
    ulp is far below the chain's error and a handful of such elements would carry the whole mean.  A truncating final
    store shifts the mean by -0.5 ulp on every element above that clamp."""
    check_finite("%s %s" % (kernel, regime), G, S if ref is None else ref)
    G, W, S = _d(G), _d(W), _d(S)
    assert G.shape == W.shape == S.shape
    kerr, serr = float((G - W).abs().max()), float((S - W).abs().max())
    krms, srms = float((G - W).pow(2).mean().sqrt()), float((S - W).pow(2).mean().sqrt())
    ulp = bf16_ulp(W.abs().clamp_min(0.25 * float(W.pow(2).mean().sqrt())))
    sgn = torch.sign(W)
    gb, sb = float(((G - W) * sgn / ulp).mean()), float(((S - W) * sgn / ulp).mean())
    rows = rows if rows is not None else G.numel() // G.shape[-1]
    blim = 4 * float(((G - S) / ulp).pow(2).mean().sqrt()) / math.sqrt(rows)
    report(kernel, regime, "bf16", kerr, serr)
    print("NUMERICS %s %s bf16 rms: kernel %.3e staged %.3e ratio %.2f  mean_signed kernel %.3e staged %.3e ulp (limit on the "
          "difference %.3e)" % (kernel, regime, krms, srms, krms / srms if srms else 0.0, gb, sb, blim))
    assert kerr <= margin * serr, "%s %s bf16: max|G-W| %.3e > %g x staged reference's %.3e" % (kernel, regime, kerr, margin, serr)
    assert krms <= 2 * srms, "%s %s bf16: rms %.3e > 2 x staged reference's %.3e" % (kernel, regime, krms, srms)
    assert abs(gb - sb) <= blim, "%s %s bf16: mean signed error %.3e ulp vs the staged reference's %.3e, limit %.3e" % (
        kernel, regime, gb, sb, blim)
    return kerr, serr


def check_prob_rows(kernel, regime, P, Pw, allow):
    """probability rows: sum to 1 within the allowance (times the row length), arg-max agrees with float64 wherever
    float64's top two are further apart than twice the allowance."""
    P, Pw = _d(P), _d(Pw)
    s = P.sum(-1)
    assert float((s - 1).abs().max()) <= allow * P.shape[-1], "%s %s: probability rows sum to 1 +- %.3e" % (
        kernel, regime, float((s - 1).abs().max()))
    check_argmax(kernel, regime, P, Pw, allow)


def check_argmax(kernel, regime, G, W, allow):
    G, W = _d(G), _d(W)
    top2 = W.topk(2, dim=-1)[0] if W.shape[-1] > 1 else None
    if top2 is None:
        return 0
    decided = (top2[..., 0] - top2[..., 1]) > 2 * allow
    same = G.argmax(-1) == W.argmax(-1)
    assert bool(same[decided].all()), "%s %s: arg-max differs from float64 on %d decided rows" % (
        kernel, regime, int((~same & decided).sum()))
    return int(decided.sum())


# ---- cases: operands + float64 value W + float32 oracle value R (+ staged float64 S), shared by the CPU and GPU tests ---
def layernorm_case(regime, rows, d, dtype, seed=0):
    """LN(a + b): a f32 rows of the regime, b = 0.1 a in the storage type (constant rows stay constant)."""
    import torch.nn.functional as F
    from oracle import f64
    a = ROW_REGIMES[regime](rows, d, seed)
    b = grid(0.1 * a, dtype)
    g, beta = ln_params(d, seed + 1)
    W = f64.layer_norm_plain(a.double() + b.double(), g, beta)
    R = F.layer_norm(a + b, (d,), g, beta, 1e-5)
    return dict(a=a, b=b, g=g, beta=beta, W=W, R=R)


def l2norm_case(regime, rows, d, dtype, seed=0):
    import torch.nn.functional as F
    from oracle import f64
    x = grid(ROW_REGIMES[regime](rows, d, seed), dtype)
    return dict(x=x, W=f64.l2norm_rows(x), R=F.normalize(x, dim=-1), W_eps=f64.l2norm_rows(x, 1e-5),
                R_eps=x / (x.norm(dim=-1, keepdim=True) + 1e-5))


def linear_case(regime, m, n, k, dtype, relu=False, addend=False, seed=0):
    """y = x W^T + b [+ addend] [ReLU]; scale = |x||w| + |b| + |addend| per output (the natural scale of the sum)."""
    import torch.nn.functional as F
    from oracle import f64
    g = _gen(seed + 100)
    x = grid(ROW_REGIMES[regime](m, k, seed), dtype)
    w = grid(torch.randn(n, k, generator=g) * k ** -0.5, dtype)
    b = torch.randn(n, generator=g)
    add = grid(torch.randn(m, n, generator=g), dtype) if addend else None
    W = f64.linear(x, w, b, relu, add)
    R = F.linear(x, w, b)
    if addend:
        R = R + add
    if relu:
        R = torch.relu(R)
    scale = x.double().norm(dim=1, keepdim=True) * w.double().norm(dim=1)[None] + b.double().abs()[None]
    if addend:
        scale = scale + add.double().abs()
    return dict(x=x, w=w, b=b, addend=add, W=W, R=R, scale=scale)


def k1k2_case(regime, n, l, d_in, h, dtype, pre_ln, seed=0):
    """K1+K2 (LN -> linear -> ReLU -> + position rows -> LN) on input rows of the regime.  S: bf16 at the LayerNorm'd GEMM
    operand and (LayerNorm-epilogue GEMM only: pre_ln) at the pre-LayerNorm value."""
    from oracle import f64
    from oracle import xml_oracle as O
    g = _gen(seed + 200)
    x = ROW_REGIMES[regime](n * l, d_in, seed).view(n, l, d_in)
    g_in, b_in = ln_params(d_in, seed + 2)
    g_pos, b_pos = ln_params(h, seed + 3)
    sd = {"LayerNorm.weight": g_in, "LayerNorm.bias": b_in,
          "net.1.weight": grid(torch.randn(h, d_in, generator=g) * d_in ** -0.5, dtype), "net.1.bias": 0.1 * torch.randn(h, generator=g)}
    pe = {"position_embeddings.weight": grid(0.5 * torch.randn(l, h, generator=g), dtype), "LayerNorm.weight": g_pos,
          "LayerNorm.bias": b_pos}
    R = O.trainable_pos_enc(O.linear_layer(x, O.Weights(sd)), O.Weights(pe))
    W = f64.linear_ln_relu_pos(x, f64.Weights64(sd), f64.Weights64(pe))
    S = f64.linear_ln_relu_pos(x, f64.Weights64(sd), f64.Weights64(pe), f64.bf16_round, pre_ln)
    return dict(x=x, sd=sd, pe=pe, W=W, R=R, S=S)


def attention_case(logit_std, n, l, h, n_heads, dtype, holes, pre_ln, seed=0):
    """BertAttention on unit-Gaussian rows with peaked Q/K weights.  Every row has a valid key (position 0), so every row
    goes to float64.  S: bf16 at Q/K/V, P, the context and (LayerNorm-epilogue GEMM only) the pre-LayerNorm value."""
    from oracle import f64
    from oracle import xml_oracle as O
    x = grid(torch.randn(n, l, h, generator=_gen(seed + 300)), dtype)
    mask = hole_masks(n, l, seed) if holes else prefix_masks(n, l, seed)
    sd = {k: (grid(v, dtype) if k.endswith("dense.weight") or k.startswith("self.") and k.endswith("weight") else v)
          for k, v in peaked_attention_weights(h, logit_std, seed).items()}
    R = O.bert_attention(x, mask.unsqueeze(1), O.Weights(sd), n_heads)
    w64 = f64.Weights64(sd)
    W = f64.bert_attention(x, mask.unsqueeze(1), w64, n_heads)
    S = f64.bert_attention(x, mask.unsqueeze(1), w64, n_heads, f64.bf16_round, pre_ln)
    scores, probs = f64.attention_probs(x, x, mask.unsqueeze(1), w64.sub("self"), n_heads)
    valid = (mask[:, None, None, :] > 0).expand_as(scores)
    return dict(x=x, mask=mask, sd=sd, W=W, R=R, S=S, logit_std=float(scores[valid].std()),
                mean_max_prob=float(probs[0].max(-1)[0].mean()))        # sequence 0: all keys valid


def pool_case(logit_std, n, l, h, n_mod, dtype, holes, seed=0):
    from oracle import f64
    from oracle import xml_oracle as O
    enc = grid(torch.randn(n, l, h, generator=_gen(seed + 400)), dtype)
    mask = hole_masks(n, l, seed) if holes else prefix_masks(n, l, seed)
    wm = peaked_pool_vector(n_mod, h, logit_std, seed)
    W, Pw = f64.modular_pool(enc, mask, wm)
    sc = torch.softmax(O.mask_logits(enc @ wm.t(), mask.unsqueeze(2)), dim=1)
    R = torch.einsum("blm,bld->mbd", sc, enc)
    return dict(enc=enc, mask=mask, wm=wm, W=W, R=R, probs=Pw, mean_max_prob=float(Pw.max(1)[0].mean()))


def q2c_case(nq, nv, l, h, dtype, holes, seed=0):
    from oracle import f64
    from oracle import xml_oracle as O
    q, c = near_duplicate_clips(nq, nv, l, h, seed)
    q, c = grid(q, dtype), grid(c, dtype)
    mask = hole_masks(nv, l, seed) if holes else prefix_masks(nv, l, seed)
    mask[-1] = mask[0]                                    # the duplicate video keeps video 0's mask
    W, Sw = f64.q2c_scores(q, c, mask)
    R = torch.max(O.mask_logits(torch.einsum("md,nld->mln", q, c), mask.t().unsqueeze(0)), dim=1)[0]
    return dict(q=q, c=c, mask=mask, W=W, R=R, clip_scores=Sw)


def core_case(logit_std, n, l, h, n_heads, dtype, holes, identity_v, seed=0):
    """attention_core behind its projections: q, k with entries of sd sqrt(logit_std) (logits of sd ~logit_std), k_mask with
    the edges.  identity_v: V = the identity per head (l <= h / n_heads), so the context IS the probability matrix:
    out[b, i, head * dh + j] = P[b, head, i, j] -- the kernel's probabilities made visible."""
    import torch.nn.functional as F
    from oracle import f64
    from oracle import xml_oracle as O
    g = _gen(seed + 500)
    dh = h // n_heads
    s = math.sqrt(logit_std)
    q, k = grid(s * torch.randn(n, l, h, generator=g), dtype), grid(s * torch.randn(n, l, h, generator=g), dtype)
    if identity_v:
        assert l <= dh
        v = torch.zeros(n, l, n_heads, dh)
        v[:, torch.arange(l), :, torch.arange(l)] = 1.0
        v = v.view(n, l, h)
    else:
        v = grid(torch.randn(n, l, h, generator=g), dtype)
    mask = hole_masks(n, l, seed) if holes else prefix_masks(n, l, seed)
    W, Pw = f64.attention_core(q, k, v, None, mask, n_heads)
    S, _ = f64.attention_core(q, k, v, None, mask, n_heads, f64.bf16_round)
    sp = lambda t: t.view(n, l, n_heads, dh).permute(0, 2, 1, 3)      # noqa: E731
    sc = torch.matmul(sp(q), sp(k).transpose(-1, -2)) / math.sqrt(dh) + (1 - mask[:, None, None, :]) * O.ATT_NEG
    Pr = torch.softmax(sc, dim=-1)
    R = torch.matmul(Pr, sp(v)).permute(0, 2, 1, 3).contiguous().view(n, l, h)
    return dict(q=q, k=k, v=v, mask=mask, W=W, S=f64.bf16_round(S), R=R, Pw=Pw, Pr=Pr)


def cross_case(logit_std, n, lq, lk, h, n_heads, dtype, seed=0):
    """cross attention + LayerNorm with peaked weights; main and side masks have holes, so there are padded QUERY rows, and
    sequence 2's side mask is all zero (every key masked).  `f64_rows` marks the rows that go to float64 (valid query, at
    least one valid key); the others keep the float32 oracle as their expected value: there f32's s - 10000 quantises the
    score to ~1e-3 before the softmax and float64 does not -- the reference's own behaviour."""
    from oracle import f64
    from oracle import xml_oracle as O
    import torch.nn.functional as F
    g = _gen(seed + 600)
    main, side = grid(torch.randn(n, lq, h, generator=g), dtype), grid(torch.randn(n, lk, h, generator=g), dtype)
    mm, sm = hole_masks(n, lq, seed), hole_masks(n, lk, seed + 1)
    sm[2] = 0
    sd = peaked_attention_weights(h, logit_std, seed)
    att = {k[5:]: (grid(v, dtype) if k.endswith("weight") else v) for k, v in sd.items() if k.startswith("self.")}
    ln_g, ln_b = sd["output.LayerNorm.weight"], sd["output.LayerNorm.bias"]
    cm = torch.einsum("bm,bn->bmn", mm, sm)
    R = F.layer_norm(O.bert_self_attention(main, side, side, cm, O.Weights(att), n_heads) + main, (h,), ln_g, ln_b, 1e-5)
    W = f64.cross_attention(main, mm, side, sm, f64.Weights64(att), ln_g, ln_b, n_heads)
    S = f64.cross_attention(main, mm, side, sm, f64.Weights64(att), ln_g, ln_b, n_heads, f64.bf16_round)
    f64_rows = (mm > 0) & (sm.sum(1, keepdim=True) > 0)
    return dict(main=main, side=side, mm=mm, sm=sm, att=att, ln_g=ln_g, ln_b=ln_b, W=W, R=R, S=S, f64_rows=f64_rows)


def convse_case(nq, nv, l, h, n_mod, merged, dtype, softmax, seed=0):
    """ConvSE with a peaked span softmax: every query lies near one direction u, every video has ONE clip along u (inside its
    valid length) and noise elsewhere, the filters have a dominant centre tap -> the span softmax puts > 0.9 on one clip
    for most pairs.  Expected values on the selected pairs; masked clips: exactly 0 with softmax, -1e10 without."""
    import torch.nn.functional as F
    from oracle import f64
    from oracle import xml_oracle as O
    g = _gen(seed + 700)
    u = F.normalize(torch.randn(h, generator=g), dim=0)
    mask = prefix_masks(nv, l, seed)
    lens = mask.sum(1).long()
    peak = (torch.randint(0, 10 ** 6, (nv,), generator=g) % lens)
    q, f = [], []
    for m in range(n_mod):
        q.append(grid(4.0 * (u[None] + 0.3 * torch.randn(nq, h, generator=g) * h ** -0.5), dtype))
        fm = 0.3 * torch.randn(nv, l, h, generator=g) * h ** -0.5
        fm[torch.arange(nv), peak] += 3.0 * u
        f.append(grid(fm, dtype))
    n_conv = 1 if merged else n_mod
    taps = torch.tensor([0.05, 0.1, 1.0, 0.1, 0.05])
    cw = torch.cat([taps * (1 + 0.05 * torch.randn(5, generator=g)) for _ in range(2 * n_conv)])
    k = min(5, nv)
    pair = torch.stack([torch.randperm(nv, generator=g)[:k] for _ in range(nq)]).int()
    pair[:, 0] = 1                                            # the length-1 video, selected by every query
    rows = torch.arange(nq).unsqueeze(1)

    def run(cast, conv_dtype):
        sims = [torch.einsum("md,nld->mnl", cast(q[m]), cast(f[m])) for m in range(n_mod)]
        wst, wed = cw[:n_conv * 5].view(n_conv, 1, 1, 5).to(conv_dtype), cw[n_conv * 5:].view(n_conv, 1, 1, 5).to(conv_dtype)
        conv = lambda x, w: F.conv1d(x.reshape(nq * nv, 1, l), w, padding=2).view(nq, nv, l)      # noqa: E731
        mk = mask.to(conv_dtype)
        if merged:
            x = sum(sims) / n_mod
            st, ed = O.mask_logits(conv(x, wst[0]), mk), O.mask_logits(conv(x, wed[0]), mk)
        else:
            st = sum(O.mask_logits(conv(sims[m], wst[m]), mk) for m in range(n_mod)) / n_mod
            ed = sum(O.mask_logits(conv(sims[m], wed[m]), mk) for m in range(n_mod)) / n_mod
        if softmax:
            st, ed = torch.softmax(st, -1), torch.softmax(ed, -1)
        return st[rows, pair.long()], ed[rows, pair.long()]
    W = run(lambda t: t.double(), torch.float64)
    R = run(lambda t: t, torch.float32)
    return dict(q=q, f=f, mask=mask, cw=cw, pair=pair, W=W, R=R, valid=mask[pair.long()] > 0)


def ingest_case(n, lmax, d, seed=0):
    """raw clip rows as the feature store holds them (f16, post-ReLU magnitudes up to a few units), back to back; video 0
    is full length, video 1 has one clip, one clip row is all zero."""
    g = _gen(seed + 800)
    lens = torch.randint(1, lmax + 1, (n,), generator=g)
    lens[0] = lmax
    if n > 1:
        lens[1] = 1
    src = (torch.relu(torch.randn(int(lens.sum()), d, generator=g)) * torch.logspace(-2, 1, int(lens.sum()))[:, None]).half()
    src[3] = 0
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    x = src.float()
    Wn = x.double() / (x.double().norm(dim=-1, keepdim=True) + 1e-5)
    Rn = x / (x.norm(dim=-1, keepdim=True) + 1e-5)
    pad = lambda t: torch.stack([torch.cat([t[row_start[i]:row_start[i + 1]], t.new_zeros(lmax - int(lens[i]), d)])   # noqa: E731
                                 for i in range(n)])
    mask = (torch.arange(lmax)[None] < lens[:, None]).float()
    return dict(src=src, row_start=row_start, lens=lens, mask=mask, W=pad(Wn), R=pad(Rn), W_raw=pad(x.double()))
