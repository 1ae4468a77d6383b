"""Whole VCMR passes restricted to an allowed set of videos per query (vcmr_search(video_allow=)): the result must be
exactly what the unrestricted search returns on the corpus that holds only the allowed videos, in the full index's numbering."""
import numpy as np
import pytest
import torch

from oracle import xml_oracle as O
from oracle.listcmp import moment_keys, tie_aware_equal
from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from tvretrieval_amd import inference as inf

pytestmark = pytest.mark.gpu

KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
_WORLDS = {}


def _world(name):
    """Small worlds like test_gpu_fuzz.py's, built once: (model, cfg, index, corpus features, queries, l, K, n moments)."""
    if name in _WORLDS:
        return _WORLDS[name]
    hidden, nv, nq, l, ragged, kv, seed = {"big": (128, 300, 70, 64, True, 100, 1),
                                           "small": (256, 40, 8, 48, False, 10, 2)}[name]
    m, cfg = _synthetic_model("video_sub", hidden, 256, 128, 128, l, torch.float32, seed=40 + seed)
    rng = np.random.default_rng(50 + seed)
    lens = rng.integers(6, l + 1, nv) if ragged else np.full(nv, l)
    lens[0] = l
    vf, vm = _feats(nv, lens, 256, 1 + seed)
    sf, sm = _feats(nv, lens, 128, 2 + seed)
    qf, qm = _feats(nq, np.concatenate([[30], rng.integers(1, 31, nq - 1)]), 128, 3 + seed)
    with torch.no_grad():
        index = inf.build_corpus_index(m, [(vf.to(DEV), vm.to(DEV), sf.to(DEV), sm.to(DEV))])
    w = dict(m=m, cfg=cfg, index=index, vf=vf, vm=vm, sf=sf, sm=sm, qf=qf.to(DEV), qm=qm.to(DEV), qf_cpu=qf, qm_cpu=qm,
             l=l, nv=nv, nq=nq, kv=kv, kw=dict(max_vcmr_video=kv, max_before_nms=60))
    with torch.no_grad():
        w["free"] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in inf.vcmr_search(m, index, w["qf"], w["qm"], **w["kw"]).items()}
    _WORLDS[name] = w
    return w


def _search(w, allowed=None, **kw):
    akw = {} if allowed is None else dict(video_allow=inf.pack_video_allow(torch.from_numpy(np.atleast_2d(allowed)).to(DEV)))
    with torch.no_grad():
        return inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], **dict(w["kw"], **kw), **akw)


def _mask(w, rng, shared, density=0.5):
    return rng.random((1 if shared else w["nq"], w["nv"])) < density


def _expected_top(w, allowed, alpha=20.0):
    """The restricted video lists from the UNRESTRICTED pass's own numbers: q2c with the disallowed entries removed, stable
    sort (score desc, index asc), and exp(alpha * s) as K8 itself computes it for those columns (the unmasked kernel on
    one-column rows)."""
    from tvretrieval_amd import ops
    q2c = w["free"]["q2c"]
    nq, nv = q2c.shape
    ew, _ = ops.topk_rows(q2c.reshape(-1, 1).contiguous(), 1, alpha=alpha)
    ew = ew.reshape(nq, nv).cpu()
    allowed = np.broadcast_to(allowed, (nq, nv))
    s = torch.where(torch.from_numpy(allowed.copy()), q2c.cpu(), torch.full((), -float("inf")))
    order = torch.sort(s, dim=1, descending=True, stable=True)[1][:, :w["kv"]]
    return order.to(torch.int32), torch.gather(ew, 1, order)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("name", ["big", "small"])
def test_restricted_pass_is_bitwise_the_pass_over_the_expected_lists(name, shared):
    w = _world(name)
    allowed = _mask(w, np.random.default_rng(7), shared, 0.5 if name == "big" else 0.6)
    assert (np.broadcast_to(allowed, (w["nq"], w["nv"])).sum(1) >= w["kv"]).all()      # every row has K allowed videos
    top_i, top_w = _expected_top(w, allowed)
    ext = _search(w, external_top=(top_i.to(DEV).contiguous(), top_w.to(DEV).contiguous()))
    got = _search(w, allowed)
    assert torch.equal(got["top_indices"].cpu(), top_i)
    assert torch.equal(got["top_scores"].cpu().view(torch.int32), top_w.view(torch.int32))
    assert torch.equal(got["flat_indices"], ext["flat_indices"])
    assert torch.equal(got["flat_scores"].view(torch.int32), ext["flat_scores"].view(torch.int32))
    assert not torch.equal(got["top_indices"], w["free"]["top_indices"])                # the mask really restricted


@pytest.mark.parametrize("name", ["big", "small"])
def test_restricted_pass_against_the_oracle_on_the_sub_corpus(name):
    """The oracle's search over the allowed videos alone, indices mapped back; tolerances of test_gpu_fuzz.py's f32 searches."""
    w = _world(name)
    allowed = _mask(w, np.random.default_rng(11), True, 0.5 if name == "big" else 0.6)
    allowed[0, 0] = True                                             # (video 0 is the full-length one: same padded width)
    sel = np.nonzero(allowed[0])[0]
    kv, l, n_mom = w["kv"], w["l"], 60
    assert len(sel) >= kv + 6
    om = O.OracleXML(w["cfg"], {k: v.detach().cpu() for k, v in w["m"].state_dict().items()})
    with torch.no_grad():
        v1, v2, s1, s2 = om.encode_context(w["vf"][sel], w["vm"][sel], w["sf"][sel], w["sm"][sel])
        q2c, st, ed = om.get_pred_from_raw_query(w["qf_cpu"], w["qm_cpu"], v1, v2, w["vm"][sel], s1, s2, w["sm"][sel], cross=True)
        want = O.vcmr_tail(q2c, st, ed, 20.0, kv, 2, 16, n_mom + 16)
    got = _search(w, allowed)
    gi = got["top_indices"].cpu().numpy()
    assert np.isin(gi, sel).all()
    ww, wi2 = torch.topk(torch.exp(20.0 * q2c), kv + 6, dim=1)
    tie_aware_equal(gi, got["top_scores"].cpu().numpy(), sel[wi2.numpy()], ww.numpy(), kv, 4e-3, "restricted videos")
    wi = sel[want["top_indices"].numpy()]
    same = np.nonzero((gi == wi).all(1))[0]
    fs, fi = got["flat_scores"].cpu().numpy(), got["flat_indices"].cpu().numpy()
    gk, wk = moment_keys(fi, gi, l), moment_keys(want["flat_indices"].numpy(), wi, l)
    ws = want["flat_scores"].numpy()
    for q in same:
        npos = int((ws[q][:n_mom] > 0).sum())
        assert int((fi[q] >= 0).sum()) == npos, (q, npos)
        if npos > 2:
            tie_aware_equal(gk[q:q + 1, :npos], fs[q:q + 1, :npos], wk[q:q + 1], ws[q:q + 1], max(1, npos - 2), 1e-3,
                            "restricted moments of query %d" % q)
    assert len(same) >= 0.8 * w["nq"]


@pytest.mark.parametrize("name", ["big", "small"])
def test_queries_with_fewer_than_k_allowed_videos(name):
    w = _world(name)
    kv, l, nq = w["kv"], w["l"], w["nq"]
    rng = np.random.default_rng(13)
    allowed = _mask(w, rng, False, 0.6)
    short = {0: 0, 1: 1, 2: kv - 1}
    for q, a in short.items():
        allowed[q] = False
        allowed[q, rng.permutation(w["nv"])[:a]] = True
    got = _search(w, allowed)
    ti, tw = got["top_indices"].cpu().numpy(), got["top_scores"].cpu().numpy()
    fi, fs = got["flat_indices"].cpu().numpy(), got["flat_scores"].cpu().numpy()
    q2c = w["free"]["q2c"].cpu().numpy()
    for q in range(nq):
        a = min(kv, int(allowed[q].sum()))
        assert (ti[q, a:] == -1).all() and (tw[q, a:] == 0).all(), q                 # empty slots: id -1, exp(20 * -inf)
        cols = np.nonzero(allowed[q])[0]
        order = cols[np.argsort(-q2c[q, cols], kind="stable")][:a]                    # the allowed videos in score order
        assert ti[q, :a].tolist() == order.tolist(), q
        r = fi[q][fi[q] >= 0] // (l * l)
        assert (r < a).all(), "query %d: a moment decodes to an empty video slot" % q
        assert allowed[q, ti[q, r]].all(), q                                          # every returned moment's video is allowed
    assert (fi[0] == -1).all() and (fi[1] >= 0).any() and (fi[2] >= 0).any()


def _exact_world(mode):
    """nv = 700 > candidates, as in test_gpu_exact.py; n_candidates = k, so the certificate b_M + eps < T_k (M = k: the k-th
    filter score against the k-th re-scored one) cannot hold and the queries take the second tier."""
    from tvretrieval_amd import ops
    from tvretrieval_amd.model_xml import XML
    key = "exact-" + mode
    if key in _WORLDS:
        return _WORLDS[key]
    nq, nv, l, hidden, kv = 24, 700, 64, 128, 10
    m, cfg = _synthetic_model("video_sub", hidden, 256, 128, 128, l, torch.float32, seed=3)
    rng = np.random.default_rng(1)
    lens = rng.integers(8, l + 1, nv); lens[0] = l
    vf, vm = _feats(nv, lens, 256, 1)
    sf, sm = _feats(nv, lens, 128, 2)
    qf, qm = _feats(nq, rng.integers(5, 31, nq), 128, 3)
    mx = m
    if mode == "f16s":
        mx = XML(cfg, compute_dtype=ops.F16S)
        mx.load_state_dict(m.state_dict())
        mx = mx.to(DEV).eval()
    batch = [(vf.to(DEV), vm.to(DEV), sf.to(DEV), sm.to(DEV))]
    with torch.no_grad():
        plain = inf.build_corpus_index(m, batch, l_ref=l)
        exact = inf.build_corpus_index(mx, batch, l_ref=l, exact_filter=True)
    assert exact.exact.mode == mode
    exact.exact.n_candidates = kv
    _WORLDS[key] = dict(m=m, mx=mx, plain=plain, exact=exact, qf=qf.to(DEV), qm=qm.to(DEV), nq=nq, nv=nv, l=l, kv=kv)
    return _WORLDS[key]


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["f32", "f16s"])
def test_exact_rank_modes_give_the_plain_f32_lists_under_the_same_mask(mode, shared):
    w = _exact_world(mode)
    nq, nv, l, kv, n_mom = w["nq"], w["nv"], w["l"], w["kv"], 100
    rng = np.random.default_rng(17)
    allowed = rng.random((1 if shared else nq, nv)) < 0.5
    if not shared:                                  # two short rows: every allowed video is a candidate, the rest empty
        allowed[3] = False
        allowed[3, rng.permutation(nv)[:kv - 3]] = True
        allowed[5] = False
    bits = inf.pack_video_allow(torch.from_numpy(allowed).to(DEV))
    with torch.no_grad():
        ref = inf.vcmr_search(w["m"], w["plain"], w["qf"], w["qm"], max_vcmr_video=kv, max_before_nms=n_mom, video_allow=bits)
        more = inf.vcmr_search(w["m"], w["plain"], w["qf"], w["qm"], max_vcmr_video=kv + 8, max_before_nms=n_mom,
                               video_allow=bits)          # a few past the boundary
        out = inf.vcmr_search(w["mx"], w["exact"], w["qf"], w["qm"], max_vcmr_video=kv, max_before_nms=n_mom, video_allow=bits)
    info = out["exact"]
    n_tier2 = int(info["n_fail"])
    print("exact-rank %s, %s mask: %d of %d queries took the second tier, %d the full-row fallback"
          % (mode, "shared" if shared else "per-query", n_tier2 - int(info["n_full_rows"]), nq, int(info["n_full_rows"])))
    assert n_tier2 >= 1 and int(info["n_full_rows"]) == 0, "no query went through the second tier: the test shows nothing"
    gi, ri = out["top_indices"].cpu().numpy(), ref["top_indices"].cpu().numpy()
    full = np.nonzero(np.broadcast_to(allowed, (nq, nv)).sum(1) >= kv + 8)[0]
    tie_aware_equal(gi[full], out["top_scores"].cpu().numpy()[full], more["top_indices"].cpu().numpy()[full],
                    more["top_scores"].cpu().numpy()[full], kv, 2e-5, "exact %s videos" % mode)
    for q in sorted(set(range(nq)) - set(full.tolist())):           # short rows: the same videos, the same empty slots
        assert gi[q].tolist() == ri[q].tolist(), q
        assert (out["top_scores"][q][out["top_indices"][q] < 0] == 0).all()
    same = np.nonzero((gi == ri).all(1))[0]
    assert len(same) >= nq - 2
    gk = moment_keys(out["flat_indices"].cpu().numpy(), gi, l)
    wk = moment_keys(ref["flat_indices"].cpu().numpy(), ri, l)
    tie_aware_equal(gk[same], out["flat_scores"].cpu().numpy()[same], wk[same], ref["flat_scores"].cpu().numpy()[same],
                    n_mom - 8, 5e-5, "exact %s moments" % mode)
    allowed_q = np.broadcast_to(allowed, (nq, nv))
    assert all(allowed_q[q, gi[q][gi[q] >= 0]].all() for q in range(nq))


def test_graphed_search_replays_with_different_masks():
    w = _world("small")
    nq, nv = w["nq"], w["nv"]
    rng = np.random.default_rng(19)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(w["m"], w["index"], nq, w["qf"].shape[1], w["qf"].shape[2], video_allow_rows=nq, **w["kw"])
        g1 = inf.GraphedVcmrSearch(w["m"], w["index"], nq, w["qf"].shape[1], w["qf"].shape[2], video_allow_rows=1, **w["kw"])
    for rep, graph in ((0, g), (1, g), (2, g1), (3, g1)):
        allowed = rng.random((nq if graph is g else 1, nv)) < (0.6, 0.3, 0.6, 0.1)[rep]        # (0.1: rows shorter than K)
        want = _search(w, allowed)
        got = graph(w["qf"], w["qm"], video_allow=inf.pack_video_allow(torch.from_numpy(allowed).to(DEV)))
        for k in KEYS + ("q2c",):
            assert torch.equal(got[k], want[k]), (rep, k)
    got = g(w["qf"], w["qm"])                                         # no mask for this call: the unrestricted pass
    for k in KEYS:
        assert torch.equal(got[k], w["free"][k]), k
    with pytest.raises(ValueError, match="mask"):
        g(w["qf"], w["qm"], video_allow=torch.zeros((1, (nv + 31) // 32), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="mask"):
        g(w["qf"], w["qm"], video_allow=torch.zeros((nq, (nv + 31) // 32 + 1), dtype=torch.int32, device=DEV))
    with torch.no_grad():
        plain = inf.GraphedVcmrSearch(w["m"], w["index"], nq, w["qf"].shape[1], w["qf"].shape[2], **w["kw"])
    with pytest.raises(ValueError, match="without a video mask"):
        plain(w["qf"], w["qm"], video_allow=torch.zeros((1, (nv + 31) // 32), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="video_allow_rows"):
        inf.GraphedVcmrSearch(w["m"], w["index"], nq, w["qf"].shape[1], w["qf"].shape[2], video_allow_rows=3, **w["kw"])


def test_host_to_host_search_with_a_per_query_mask():
    """vcmr_search_host with one allow row per query and a chunk size that splits the queries (256 + 184): every chunk must
    use its own rows -- the records are bitwise those of the single launch under the same mask."""
    from tvretrieval_amd import ops
    from tvretrieval_amd.results import MOMENT_DTYPE
    nv, nq, l = 60, 440, 48
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, l, torch.float32, seed=21)
    rng = np.random.default_rng(23)
    lens = rng.integers(6, l + 1, nv); lens[0] = l
    vf, vm = _feats(nv, lens, 256, 1)
    sf, sm = _feats(nv, lens, 128, 2)
    qf, qm = _feats(nq, np.concatenate([[30], rng.integers(3, 31, nq - 1)]), 128, 3)
    allowed = rng.random((nq, nv)) < 0.4
    allowed[7] = False                                               # an empty row and a short one
    allowed[300, 12:] = False
    kw = dict(max_vcmr_video=10, max_before_nms=40)
    with torch.no_grad():
        index = inf.build_corpus_index(m, [(vf.to(DEV), vm.to(DEV), sf.to(DEV), sm.to(DEV))])
        bits = inf.pack_video_allow(torch.from_numpy(allowed).to(DEV))
        one = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), video_allow=bits, **kw)
        rec1, cnt1 = ops.moments_decode(one["flat_scores"], flat=one["flat_indices"], top_idx=one["top_indices"],
                                        meta2vid=torch.arange(nv, dtype=torch.int32, device=DEV), l_ref=index.l_ref,
                                        clip_length=1.5, seconds=True)
        want, want_cnt = rec1.cpu().numpy().view(MOMENT_DTYPE)[..., 0], cnt1.cpu().numpy()
        tm = {}
        rec, cnt = inf.vcmr_search_host(m, index, query_feat=qf.pin_memory(), query_mask=qm.pin_memory(), chunk=256,
                                        clip_length=1.5, timings=tm, video_allow=bits, **kw)
    assert tm["chunk_queries"] == [256, 184]
    np.testing.assert_array_equal(cnt, want_cnt)
    live = np.arange(rec.shape[1])[None] < cnt[:, None]
    for col in ("vid", "st", "ed", "score"):
        np.testing.assert_array_equal(np.where(live, rec[col], 0), np.where(live, want[col], 0), err_msg=col)
    assert cnt[7] == 0 and (cnt[:7] > 0).all()
    assert all(allowed[q, rec["vid"][q, :cnt[q]]].all() for q in range(nq))
    with pytest.raises(ValueError, match="device"):
        inf.vcmr_search_host(m, index, query_feat=qf.pin_memory(), query_mask=qm.pin_memory(), chunk=256, video_allow=bits.cpu(), **kw)


@pytest.mark.parametrize("name", ["big", "small"])
def test_video_allow_none_is_the_call_without_the_argument(name):
    w = _world(name)
    with torch.no_grad():
        got = inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], video_allow=None, **w["kw"])
    for k in KEYS + ("q2c",):
        assert torch.equal(got[k], w["free"][k]), k
    ones = _search(w, np.ones((1, w["nv"]), dtype=bool))              # ... and so is a mask that allows everything
    for k in KEYS:
        assert torch.equal(ones[k], w["free"][k]), k


def test_the_three_refusals():
    w = _world("small")
    bits = inf.pack_video_allow(torch.ones((1, w["nv"]), dtype=torch.bool, device=DEV))
    ext = (w["free"]["top_indices"], w["free"]["top_scores"])
    with torch.no_grad():
        with pytest.raises(ValueError, match="external_top"):
            inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], video_allow=bits, external_top=ext, **w["kw"])
        with pytest.raises(ValueError, match="pad_tail"):
            inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], video_allow=bits, pad_tail=True, **w["kw"])
        with pytest.raises(ValueError, match="video_allow"):          # a mask of another shape
            inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], video_allow=bits.repeat(3, 1), **w["kw"])
        with pytest.raises(ValueError, match="video_allow"):
            inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], video_allow=bits.to(torch.int64), **w["kw"])
