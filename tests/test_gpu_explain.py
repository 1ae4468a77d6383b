"""GPU tests of the explanation feature: XML.get_visualization_data against the reference's own output (fixture), the
attention-emitting K5 and the evidence-emitting K7 against their plain forms (bitwise) and against float64, and
inference.explain_moments against vcmr_search / get_visualization_data on a resident index."""
import numpy as np
import pytest
import torch

import numerics_regimes as NR
from conftest import load_golden
from oracle import xml_oracle as O
from test_gpu_kernels import DEV, close, dev, ops  # noqa: F401  (ops: module fixture)
from test_gpu_model import T, _feats, _synthetic_model, build_model

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAME = "xml_visualization_h128"
PER_CLIP = ("st_prob", "ed_prob", "similarity_scores", "video_similarity", "sub_similarity")
C_POOL = 2            # margin over the f32 reference's own error, as for the pooled vectors (tests/test_gpu_numerics.py)


def _viz(m, d):
    return m.get_visualization_data(T(d["query_feat"]), T(d["query_mask"]), T(d["video_feat"]), T(d["video_mask"]),
                                    T(d["sub_feat"]), T(d["sub_mask"]), None, None, T(d["st_ed_indices"]))


def _check_layout(got, d):
    import json
    assert isinstance(got, list) and len(got) == len(d["ctx_lens"])
    keys = json.loads(str(d["keys"]))
    for i, g in enumerate(got):
        assert sorted(g.keys()) == keys
        lq, l = int(d["q_lens"][i]), int(d["ctx_lens"][i])
        assert g["modular_att_scores"].shape == (lq, 2) and isinstance(g["modular_att_scores"], np.ndarray)
        for k in PER_CLIP:
            assert g[k].shape == (l,) and g[k].dtype == np.float32, (k, g[k].shape)
        assert np.array_equal(g["st_ed_indices"], d["viz/st_ed_indices"][i])


def test_visualization_data_matches_the_reference_fp32():
    """st / ed: the tolerances test_golden_fp32 applies to `st pair` / `ed pair`; the similarities are the same quantity one
    5-tap convolution earlier: the same; the attention weights: the 1e-4 of the pooled query vectors."""
    d, cfg, sd = load_golden(NAME)
    m = build_model(cfg, sd)
    got = _viz(m, d)
    _check_layout(got, d)
    for i, g in enumerate(got):
        lq, l = int(d["q_lens"][i]), int(d["ctx_lens"][i])
        close("modular_att_scores[%d]" % i, g["modular_att_scores"], d["viz/modular_att_scores"][i, :lq], 1e-4)
        for k in PER_CLIP:
            close("%s[%d]" % (k, i), g[k], d["viz/" + k][i, :l], 1e-3, 1e-6)


def test_merged_st_ed_prob_with_similarity_matches_the_untruncated_reference_rows():
    """get_merged_st_ed_prob(return_similaity=True) before the method cuts its rows: -1e10 fills compare exactly, the
    similarities at padded positions (which the taps of a video's last clips read) to the same tolerances."""
    d, cfg, sd = load_golden(NAME)
    m = build_model(cfg, sd)
    with torch.no_grad():
        _, v2, _, s2 = m.encode_context(T(d["video_feat"]), T(d["video_mask"]), T(d["sub_feat"]), T(d["sub_mask"]))
        enc = m.encode_input(T(d["query_feat"]), T(d["query_mask"]), m.query_input_proj, m.query_encoder, m.query_pos_embed)
        vq, sq, att = m.get_modularized_queries(enc, T(d["query_mask"]), return_modular_att=True)
        vq0, sq0 = m.get_modularized_queries(enc, T(d["query_mask"]))
        out = m.get_merged_st_ed_prob(vq, v2, sq, s2, T(d["video_mask"]), cross=False, return_similaity=True)
        st0, ed0 = m.get_merged_st_ed_prob(vq, v2, sq, s2, T(d["video_mask"]), cross=False)
    assert torch.equal(vq, vq0) and torch.equal(sq, sq0)
    assert att.shape == (len(d["q_lens"]), d["query_mask"].shape[1], 2)
    assert torch.equal(out[0], st0) and torch.equal(out[1], ed0)         # the evidence variant's logits ARE K7's
    for k, t in zip(PER_CLIP, out):
        want = d["full/" + k]
        close("full " + k, t, want, 1e-3, 1e-6)
        fill = want == np.float32(-1e10)
        assert np.array_equal(t.cpu().numpy() == np.float32(-1e10), fill)
    with pytest.raises(ValueError):
        m.get_merged_st_ed_prob(vq, v2, sq, s2, T(d["video_mask"]), cross=True, return_similaity=True)


def test_visualization_data_bf16_model():
    """bf16 compute against the f32 reference, with the pair the bf16 golden test of tests/test_gpu_model.py applies
    (test_golden_bf16_overlap: close(..., 0.12, 0.02), i.e. |got - want| <= 0.12 + 0.02 |want|), on every array."""
    d, cfg, sd = load_golden(NAME)
    m = build_model(cfg, sd, BF16)
    got = _viz(m, d)
    _check_layout(got, d)
    for i, g in enumerate(got):
        lq, l = int(d["q_lens"][i]), int(d["ctx_lens"][i])
        close("bf16 modular_att_scores[%d]" % i, g["modular_att_scores"], d["viz/modular_att_scores"][i, :lq], 0.12, 0.02)
        for k in PER_CLIP:
            want = d["viz/" + k][i, :l]
            err = float(np.abs(g[k] - want).max())
            print("EXPLAIN bf16 %s[%d]: max err %.3e, scale %.3e" % (k, i, err, float(np.abs(want).max())))
            close("bf16 %s[%d]" % (k, i), g[k], want, 0.12, 0.02)


# ---- K5 with attention output -----------------------------------------------------------------------------------------
def _f32_att(enc, mask, wm):
    """the float32 reference of the pooling weights (xml/model_xml.py:410-412)"""
    return torch.softmax(O.mask_logits(enc @ wm.t(), mask.unsqueeze(2)), dim=1)


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("logit_std", [2.0, 6.0, 12.0])
def test_modular_att_peaked_vs_float64(ops, holes, logit_std):  # noqa: F811
    """the weights themselves against float64 on the peaked-softmax / masks-with-holes regimes: at most C_POOL times as far
    from float64 as the float32 reference (probabilities: scale 1), exactly 0 at masked tokens."""
    case = NR.pool_case(logit_std, 33, 30, 256, 2, F32, holes)
    pooled, att = ops.modular_pool(dev(case["enc"]), dev(case["mask"]), dev(case["wm"]), return_att=True)
    regime = "peaked%g%s" % (logit_std, "+holes" if holes else "")
    R = _f32_att(case["enc"], case["mask"], case["wm"])
    NR.check_f32("modular_pool_att", regime, att, case["probs"], R, C_POOL, scale=1.0)
    assert bool((att.cpu()[case["mask"] == 0] == 0).all())
    NR.check_f32("modular_pool_att pooled", regime, pooled, case["W"], case["R"], C_POOL)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hidden", [128, 384, 1032])       # one wave per query / one workgroup per query / the general kernel
@pytest.mark.parametrize("lq", [1, 7, 30])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_modular_pool_att_is_bitwise_the_plain_kernel(ops, dtype, hidden, lq, n):  # noqa: F811
    g = torch.Generator().manual_seed(hidden + lq + n)
    enc = torch.randn(n, lq, hidden, generator=g)
    mask = NR.prefix_masks(n, lq, 5)
    wm = torch.randn(2, hidden, generator=g) * hidden ** -0.5
    e, mk, w = dev(enc, dtype), dev(mask), dev(wm)
    plain = ops.modular_pool(e, mk, w)
    pooled, att = ops.modular_pool(e, mk, w, return_att=True)
    assert torch.equal(pooled, plain)
    assert att.shape == (n, lq, 2) and att.dtype == F32
    assert bool((att[mk == 0] == 0).all())
    close("att rows sum to 1", att.sum(1), torch.ones(n, 2), 1e-5)
    close("att vs f32 reference", att, _f32_att(e.float().cpu(), mask, wm), 2e-2 if dtype == BF16 else 1e-5)
    one = ops.modular_pool(e, mk, w[:1].contiguous())
    p1, a1 = ops.modular_pool(e, mk, w[:1].contiguous(), return_att=True)
    assert torch.equal(p1, one) and a1.shape == (n, lq, 1)
    assert torch.equal(a1[..., 0], att[..., 0])
    if hidden > 1024:
        return                                               # (the varlen entry takes hidden <= 1024)
    cu, src, rows = ops.pack_plan(mk)
    assert rows == int(mask.sum())
    ep = e.reshape(n * lq, hidden)[src[:rows].long()].contiguous()
    vplain = ops.modular_pool_varlen(ep, cu, n, lq, w)
    vpooled, vatt = ops.modular_pool_varlen(ep, cu, n, lq, w, return_att=True)
    assert torch.equal(vpooled, vplain)
    assert torch.equal(vatt, att)                            # padded layout, zeros beyond every query's own tokens


def test_encode_query_attention_is_the_same_on_the_packed_path(monkeypatch):
    from tvretrieval_amd import model_xml as MX
    m, cfg = _synthetic_model("video_sub", 256, 64, 64, 64, 32, F32, seed=2)
    nq = 700                                                  # 700 x 30 padded rows: over PACK_MIN_ROWS
    qf, qm = _feats(nq, np.random.default_rng(1).integers(3, 31, nq), 64, 4)
    qf, qm = qf.to(DEV), qm.to(DEV)
    assert nq * qf.shape[1] >= MX.PACK_MIN_ROWS
    with torch.no_grad():
        vq, sq, att = m.encode_query(qf, qm, return_modular_att=True)
        vq0, sq0 = m.encode_query(qf, qm)
        monkeypatch.setattr(MX, "PACK_QUERY_TOKENS", False)
        vqp, sqp, attp = m.encode_query(qf, qm, return_modular_att=True)
    assert torch.equal(vq, vq0) and torch.equal(sq, sq0)
    assert att.shape == attp.shape == (nq, qf.shape[1], 2)
    assert bool((att[qm == 0] == 0).all()) and bool((attp[qm == 0] == 0).all())
    close("packed vs padded attention", att, attp, 1e-4)
    close("packed vs padded video query", vq, vqp, 1e-4)


# ---- span evidence ----------------------------------------------------------------------------------------------------
def _k7_operands(ops, dtype, n_mod, nq, nv, lpad, l_ref, hidden, seed, ragged):  # noqa: F811
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(nq, hidden, generator=g) for _ in range(n_mod)]
    f = [torch.randn(nv, lpad, hidden, generator=g) * hidden ** -0.5 for _ in range(n_mod)]
    lens = torch.randint(3, l_ref + 1, (nv,), generator=g) if ragged else torch.full((nv,), l_ref)
    lens[0] = l_ref
    mask = (torch.arange(lpad)[None] < lens[:, None]).float()
    for x in f:
        x[:, l_ref:] = 0
    if dtype == "f16s":
        qd = [ops.split_f16_rows(dev(x)) for x in q]
        fd = [ops.split_f16_rows(dev(x)) for x in f]
    else:
        qd, fd = [dev(x, dtype) for x in q], [dev(x, dtype) for x in f]
    return q, f, mask, lens, qd, fd


@pytest.mark.parametrize("dtype", [F32, BF16, "f16s"])
@pytest.mark.parametrize("n_mod,merged", [(2, True), (2, False), (1, False)])
@pytest.mark.parametrize("shape", [(9, 7, 48, 40, 128, 5), (40, 6, 128, 100, 256, 5), (12, 5, 64, 64, 128, 3)])
@pytest.mark.parametrize("ragged", [False, True])
def test_span_evidence_logits_are_bitwise_k7(ops, dtype, n_mod, merged, shape, ragged):  # noqa: F811
    """st / ed of the evidence entry == convse_rerank(softmax=False) on the same pairs (query-major pair lists that repeat
    videos; more than 64 pairs of one video -> two chunks), and the similarity rows against float64."""
    nq, nv, lpad, l_ref, hidden, ksize = shape
    kp = 4
    q, f, mask, lens, qd, fd = _k7_operands(ops, dtype, n_mod, nq, nv, lpad, l_ref, hidden, 7 + nq, ragged)
    g = torch.Generator().manual_seed(3)
    pair_vid = torch.randint(0, nv, (nq, kp), generator=g, dtype=torch.int32)
    pair_vid[:, 0] = 0                                                   # video 0 in every query's list
    if nq >= 40:
        pair_vid[:, 1] = 1
        pair_vid[:30, 2] = 1                                             # 70 pairs of video 1: two chunks
    n_conv = 1 if merged else n_mod
    conv_w = torch.randn(2 * n_conv * ksize, generator=g) * 0.5
    mk = [dev(mask)] * n_mod
    st, ed = ops.convse_rerank(qd, fd, mk, dev(pair_vid), dev(conv_w), l_ref, merged, ksize, softmax=False)
    pq = torch.arange(nq, dtype=torch.int32).repeat_interleave(kp)
    pv = pair_vid.reshape(-1)
    ev = ops.span_evidence(qd, fd, mk, dev(pq), dev(pv), dev(conv_w), l_ref, merged, ksize)
    assert torch.equal(ev.st_logits, st.reshape(nq * kp, lpad))
    assert torch.equal(ev.ed_logits, ed.reshape(nq * kp, lpad))
    # a permuted pair list gives the permuted rows (explicit pairs, any order)
    perm = torch.randperm(nq * kp, generator=g)
    ev2 = ops.span_evidence(qd, fd, mk, dev(pq[perm]), dev(pv[perm]), dev(conv_w), l_ref, merged, ksize)
    for a, b in zip(ev, ev2):
        assert (a is None and b is None) or torch.equal(a[dev(perm)], b)
    # logits: -1e10 at masked clips, zeros beyond l_ref
    valid = mask[pv.long()][:, :l_ref] != 0
    assert bool((ev.st_logits.cpu()[:, :l_ref][~valid] == -1e10).all())
    assert bool((ev.st_logits[:, l_ref:] == 0).all()) and bool((ev.similarity[:, l_ref:] == 0).all())
    # similarities against float64 of the operands the kernel saw
    qs = [x.float().cpu().double() for x in qd]
    fs = [x.float().cpu().double() for x in fd]
    sims = [torch.einsum("ph,plh->pl", qs[m][pq.long()], fs[m][pv.long()])[:, :l_ref] for m in range(n_mod)]
    scale = [float((qs[m].norm(dim=1).max() * fs[m].norm(dim=2).max())) for m in range(n_mod)]
    tol = 2e-6                                              # f32 accumulation of exact products in every storage form
    got = [ev.video_similarity, ev.sub_similarity]
    for m in range(n_mod):
        close("similarity of stream %d" % m, got[m][:, :l_ref].double().cpu(), sims[m], tol * scale[m] * hidden ** 0.5)
    if n_mod == 1:
        assert ev.sub_similarity is None
        assert torch.equal(ev.similarity, ev.video_similarity)
    else:
        close("merged similarity", ev.similarity[:, :l_ref].double().cpu(), (sims[0] + sims[1]) / 2,
              tol * max(scale) * hidden ** 0.5)
        if not merged:
            assert torch.equal(ev.similarity, (ev.video_similarity + ev.sub_similarity) * 0.5)


def test_span_evidence_skips_pairs_out_of_range(ops):  # noqa: F811
    nq, nv, lpad, l_ref, hidden = 5, 4, 48, 40, 128
    q, f, mask, lens, qd, fd = _k7_operands(ops, F32, 2, nq, nv, lpad, l_ref, hidden, 1, True)
    conv_w = dev(torch.randn(10, generator=torch.Generator().manual_seed(1)))
    pq = torch.tensor([0, 1, 7, -1, 2, 3], dtype=torch.int32)
    pv = torch.tensor([0, 9, 1, 1, -1, 3], dtype=torch.int32)
    ev = ops.span_evidence(qd, fd, [dev(mask)] * 2, dev(pq), dev(pv), conv_w, l_ref, True, 5)
    for t in ev:
        assert bool((t[1:5] == 0).all())
        assert bool((t[0] != 0).any()) and bool((t[5] != 0).any())
    empty = ops.span_evidence(qd, fd, [dev(mask)] * 2, dev(pq[:0]), dev(pv[:0]), conv_w, l_ref, True, 5)
    assert all(t.shape == (0, lpad) for t in empty)


# ---- engine -----------------------------------------------------------------------------------------------------------
def _world(dtype, nv=21, nq=9, l=40, hidden=128, seed=5, exact=False, ctx_mode="video_sub"):
    from tvretrieval_amd import inference as inf
    m, cfg = _synthetic_model(ctx_mode, hidden, 96, 64, 64, l, dtype, seed=seed)
    rng = np.random.default_rng(seed)
    lens = rng.integers(6, l + 1, nv)
    lens[0] = l
    vf, vm = _feats(nv, lens, 96, 1)
    sf, sm = _feats(nv, lens, 64, 2)
    qf, qm = _feats(nq, rng.integers(3, 31, nq), 64, 3)
    bs = 8       # (every batch tensor is padded to the corpus maximum l, like the batches of test_search_vs_oracle_fp32)
    batches = [(vf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV), sf[b:b + bs].to(DEV), sm[b:b + bs].to(DEV))
               for b in range(0, nv, bs)]
    with torch.no_grad():
        index = inf.build_corpus_index(m, batches, exact_filter=exact)
    return m, index, (vf, vm, sf, sm), qf.to(DEV), qm.to(DEV), lens


def test_explain_moments_is_consistent_with_the_search_and_the_model():
    from tvretrieval_amd import inference as inf
    m, index, (vf, vm, sf, sm), qf, qm, lens = _world(F32)
    assert index.ragged
    nq = qf.shape[0]
    with torch.no_grad():
        out = inf.vcmr_search(m, index, qf, qm, max_vcmr_video=5, max_before_nms=20)
        q2c = inf.stage_q2c(index, inf.stage_query_vectors(m, qf, qm))
    l_ref = index.l_ref
    flat = out["flat_indices"][:, 0].cpu().long()
    assert bool((flat >= 0).all())
    rank, st_i, ed_i = flat // (l_ref * l_ref), (flat // l_ref) % l_ref, flat % l_ref
    top_vid = out["top_indices"].cpu().long()[torch.arange(nq), rank]
    pq = torch.arange(nq, dtype=torch.int32)
    ex = inf.explain_moments(m, index, qf, qm, pq, top_vid.to(torch.int32) - index.video_offset)
    assert ex["modular_att"].shape == (nq, qf.shape[1], 2)
    for k in ("video_similarity", "sub_similarity", "similarity", "st_logits", "ed_logits"):
        assert ex[k].shape == (nq, l_ref) and ex[k].dtype == F32
    ctx_len = ex["ctx_len"].cpu().long()
    assert torch.equal(ctx_len, torch.from_numpy(lens)[top_vid])
    assert bool((st_i < ctx_len).all()) and bool((ed_i < ctx_len).all())
    rows = torch.arange(nq)
    assert bool(torch.isfinite(ex["st_logits"].cpu()[rows, st_i]).all()) and bool((ex["st_logits"].cpu()[rows, st_i] > -1e9).all())
    assert bool((ex["ed_logits"].cpu()[rows, ed_i] > -1e9).all())
    assert torch.equal(ex["q2c"].cpu(), q2c.cpu()[rows, top_vid])
    # beyond a video's length: K7's -1e10 in the logits
    beyond = torch.arange(l_ref)[None] >= ctx_len[:, None]
    assert bool((ex["st_logits"].cpu()[beyond] == -1e10).all()) and bool((ex["ed_logits"].cpu()[beyond] == -1e10).all())
    # the logits are K7's, bit for bit
    with torch.no_grad():
        q_lin = inf.query_linears(m, index, inf.stage_query_vectors(m, qf, qm))
        st, ed = m_ops().convse_rerank(q_lin, [index.feat2[k] for k in index.modalities],
                                       [index.mask[k] for k in index.modalities],
                                       top_vid.to(torch.int32).reshape(-1, 1).contiguous().to(DEV), m._conv_weights(), l_ref,
                                       True, 5, softmax=False)
    assert torch.equal(ex["st_logits"], st[:, 0, :l_ref]) and torch.equal(ex["ed_logits"], ed[:, 0, :l_ref])
    # ... and what get_visualization_data gives for (query q, video v) as one batch row; the video batch is the full-length
    # batch v was indexed in (the contents of its padded rows are observable through the taps)
    vrows = top_vid.numpy()
    for q in range(nq):
        v = int(vrows[q])
        b0 = v // 8 * 8
        sl = slice(b0, min(b0 + 8, len(lens)))
        n_b = sl.stop - sl.start
        viz = m.get_visualization_data(qf[q:q + 1].expand(n_b, -1, -1).contiguous(), qm[q:q + 1].expand(n_b, -1).contiguous(),
                                       vf[sl].to(DEV), vm[sl].to(DEV), sf[sl].to(DEV), sm[sl].to(DEV),
                                       None, None, torch.zeros(n_b, 2, dtype=torch.long))
        g = viz[v - b0]
        l = int(lens[v])
        lq = int(qm[q].sum())
        close("att q%d" % q, ex["modular_att"][q, :lq], g["modular_att_scores"], 1e-4)
        for k, name in (("st_logits", "st_prob"), ("ed_logits", "ed_prob"), ("similarity", "similarity_scores"),
                        ("video_similarity", "video_similarity"), ("sub_similarity", "sub_similarity")):
            close("%s q%d v%d" % (k, q, v), ex[k][q, :l], g[name], 1e-3, 1e-6)
    host = inf.explain_moments(m, index, qf, qm, pq, top_vid.to(torch.int32), to_host=True, with_q2c=False)
    assert host["q2c"] is None and isinstance(host["st_logits"], np.ndarray)
    assert np.array_equal(host["st_logits"], ex["st_logits"].cpu().numpy())


def m_ops():
    from tvretrieval_amd import ops as o
    return o


@pytest.mark.parametrize("mode", ["f32", "f16s", "bf16"])
def test_explain_moments_on_every_index_form(mode):
    """plain bf16 index, exact-rank f32 index, exact-rank split-f16 index (feat2 = SplitRows): logits bitwise K7's on the
    index's own operands; pairs that repeat a video and a query."""
    from tvretrieval_amd import inference as inf
    o = m_ops()
    dtype = {"f32": F32, "f16s": o.F16S, "bf16": BF16}[mode]
    m, index, _, qf, qm, lens = _world(dtype, exact=mode != "bf16", seed=9)
    if mode != "bf16":
        assert index.exact is not None and index.exact.mode == mode
    if mode == "f16s":
        assert isinstance(index.feat2["video"], o.SplitRows)
    pq = torch.tensor([0, 0, 3, 8, 8, 8, 5, 1], dtype=torch.int32)
    pv = torch.tensor([2, 2, 20, 0, 7, 2, 13, 13], dtype=torch.int32)
    ex = inf.explain_moments(m, index, qf, qm, pq, pv)
    mods = index.modalities
    with torch.no_grad():
        qvec = inf.stage_query_vectors(m, qf, qm)
        q_lin = inf.query_linears(m, index, qvec)
        if mode == "f16s":
            q_lin = [o.split_f16_rows(x.float().contiguous()) for x in q_lin]
        pair_vid = torch.full((qf.shape[0], 3), -1, dtype=torch.int32)
        slot = {}
        for p, (a, b) in enumerate(zip(pq.tolist(), pv.tolist())):
            slot[p] = (a, sum(1 for x in pq[:p].tolist() if x == a))
            pair_vid[slot[p]] = b
        st, ed = o.convse_rerank(q_lin, [index.feat2[k] for k in mods], [index.mask[k] for k in mods], pair_vid.to(DEV),
                                 m._conv_weights(), index.l_ref, True, 5, softmax=False)
    for p in range(len(pq)):
        a, j = slot[p]
        assert torch.equal(ex["st_logits"][p], st[a, j, :index.l_ref]), p
        assert torch.equal(ex["ed_logits"][p], ed[a, j, :index.l_ref]), p
    assert torch.equal(ex["st_logits"][0], ex["st_logits"][1]) and torch.equal(ex["similarity"][0], ex["similarity"][1])
    assert torch.equal(ex["ctx_len"].cpu().long(), torch.from_numpy(lens)[pv.long()])
    assert ex["q2c"].shape == (len(pq),) and bool(torch.isfinite(ex["q2c"]).all())
    if mode != "bf16":
        # the re-scored value of the pair: what the exact-rank search ranks by
        out = inf.vcmr_search(m, index, qf, qm, max_vcmr_video=index.n_videos, max_before_nms=10)
        w = out["top_scores"].cpu()
        ti = out["top_indices"].cpu().long()
        for p in range(len(pq)):
            a, b = int(pq[p]), int(pv[p])
            r = int((ti[a] == b).nonzero()[0])
            close("q2c pair %d" % p, torch.exp(20.0 * ex["q2c"][p].cpu()), w[a, r], 0, 1e-4)


def test_explain_moments_single_stream_model():
    from tvretrieval_amd import inference as inf
    m, index, _, qf, qm, lens = _world(F32, ctx_mode="sub", seed=4)
    ex = inf.explain_moments(m, index, qf, qm, [1, 2], [3, 0])
    assert ex["video_similarity"] is None and ex["modular_att"].shape[2] == 1
    assert torch.equal(ex["similarity"], ex["sub_similarity"])
    assert torch.equal(ex["q2c"].cpu(), inf.stage_q2c(index, inf.stage_query_vectors(m, qf, qm)).cpu()[[1, 2], [3, 0]])


def test_explain_moments_empty_inputs():
    from tvretrieval_amd import inference as inf
    m, index, _, qf, qm, lens = _world(F32, nv=5, nq=3)
    none = torch.zeros(0, dtype=torch.int32)
    ex = inf.explain_moments(m, index, qf, qm, none, none)
    assert ex["modular_att"].shape == (3, qf.shape[1], 2)
    for k in ("video_similarity", "sub_similarity", "similarity", "st_logits", "ed_logits"):
        assert ex[k].shape == (0, index.l_ref)
    assert ex["ctx_len"].shape == (0,) and ex["q2c"].shape == (0,)
    ex = inf.explain_moments(m, index, qf[:0], qm[:0], none, none, to_host=True)
    assert ex["modular_att"].shape == (0, qf.shape[1], 2) and ex["st_logits"].shape == (0, index.l_ref)
    with pytest.raises(ValueError):
        inf.explain_moments(m, index, qf[:0], qm[:0], [0], [0])
