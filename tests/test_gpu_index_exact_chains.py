"""Long videos on an exact-rank index that takes updates (MutableCorpusIndex.create(..., exact_rank=True, exact_part_overlap=O);
DESIGN.md section 20g), in the world of tests/test_gpu_index_parts_search.py: l_ref = 32, overlap 16, capacity 70, hidden 128,
16 videos in 35 parts scattered over the word boundaries, SEED = 5; both exact modes (the f32 model, the ops.F16S model with
the same weights); the packed filter image at l_ref = 80, hidden 256.  20 candidates per query for the 10 best videos of 65
live slots, so the filter filters.
  1. DEFINITION, bitwise: the search's lists are K8 over the f32-grade scores of EVERY slot under the bits of each allowed
     video's best part (ops.chain_best_allow on that full row), then K7 / K9 -- a score depends on its (query, slot) pair alone,
     whichever tier computed it; eager and host-to-host, with and without a per-query video_allow;
  2. the test bites: a candidate list holds two slots of one chain, a listed slot is not its chain's head;
  3. every tier, asserted taken through the info dict, gives the lists of (1);
  4. against the plain f32 chain index of the same videos (tests/test_gpu_exact.py::_lists_equal) and against the oracle;
  5. the life cycle of tests/test_gpu_index_parts_search.py, plain and with the packed filter image: (1) after every step, and
     the per-slot operands and the running bound bitwise those of stand-alone puts of the same rows;
  6. an exact-rank index created without the keyword holds no chain tables and launches none of the new entries."""
import numpy as np
import pytest
import torch

from oracle import xml_oracle as O
from oracle.listcmp import moment_keys, tie_aware_equal
from test_gpu_exact import _lists_equal
from test_gpu_index_exact import _parts
from test_gpu_index_parts_search import (CLIP, IDS, KW, OV, W, _allow_bits, _best_mask, _life_cycle, _planted, _scattered,
                                         _tables, _world)
from test_gpu_index_update import CAP, KEYS, _bits, _rows
from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from test_gpu_parts import MOMENT_TOL, VIDEO_TOL, _excluded, _host
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16s"]
K, N_MOM = KW["max_vcmr_video"], KW["max_before_nms"]
_F16S = {}
_PLAIN_CREATE = MutableCorpusIndex.create.__func__        # (the exact_chains fixture replaces the attribute)


def _twin_model(m, cfg):
    """The ops.F16S model with the weights of the f32 model m."""
    from tvretrieval_amd.model_xml import XML
    if id(m) not in _F16S:
        mx = XML(cfg, compute_dtype=ops.F16S)
        mx.load_state_dict(m.state_dict())
        _F16S[id(m)] = mx.to(DEV).eval()
    return _F16S[id(m)]


def _w(mode):
    """The world of tests/test_gpu_index_parts_search.py with the model of the exact mode."""
    base = _world(torch.float32)
    if ("planted", W) not in base:
        base["planted", W] = _planted(base["m"], base["cfg"], W, 200 + W)
    return base if mode == "f32" else dict(base, m=_twin_model(base["m"], base["cfg"]))


@pytest.fixture
def exact_chains(monkeypatch):
    """MutableCorpusIndex.create(..., part_overlap=O), as the helpers of tests/test_gpu_index_parts_search.py spell it, makes
    the exact-rank index with exact_part_overlap=O (plus what the test sets in `extra`), 20 candidates per query, and keeps
    the maximum of the rounding-error norms of every row put, computed as the one-shot builder computes them."""
    extra = {}

    def create(cls, model, capacity, **kw):
        index = _PLAIN_CREATE(cls, model, capacity, exact_rank=True, exact_part_overlap=kw.pop("part_overlap"), **extra, **kw)
        index.exact.n_candidates = 20
        index.norms_put = torch.zeros(len(index.modalities), device=DEV)
        launch = index._launch_put

        def launch_put(slots, ids, enc, *rest):
            for j, mod in enumerate(index.modalities):
                err = ops.round_bf16_rows_err(ops.l2norm_rows(enc[mod][0].contiguous()))[1]
                index.norms_put[j] = torch.maximum(index.norms_put[j], err.max())
            return launch(slots, ids, enc, *rest)
        index._launch_put = launch_put
        return index
    monkeypatch.setattr(MutableCorpusIndex, "create", classmethod(create))
    return extra


def _query_operands(m, index, qf, qm):
    """(query vectors, the operands ops.q2c_rescore takes for them in the index's exact mode)"""
    qvec = inf.stage_query_vectors(m, qf, qm)
    qn = [ops.l2norm_rows(qvec[mod].contiguous()) for mod in index.modalities]
    if index.exact.mode == "f16s":
        qn = [ops.split_f16_rows(q, ops.F16_UNIT_LOG2) for q in qn]
    return qvec, qn


def _all_scores(index, qn):
    nq = qn[0].shape[0]
    every = torch.arange(CAP, dtype=torch.int32, device=DEV).repeat(nq, 1).contiguous()
    mods = index.modalities
    return ops.q2c_rescore(qn, [index.exact.feat1n_f32[mod] for mod in mods], [index.mask[mod] for mod in mods], every)


def _definition(m, index, qf, qm, allowed=None, k=K, n_mom=N_MOM):
    """The lists by definition (module docstring, 1) -> dict of the four lists, the full score rows and the best-part words."""
    with torch.no_grad():
        qvec, qn = _query_operands(m, index, qf, qm)
        allv = _all_scores(index, qn)
        allow = index.live if allowed is None else _allow_bits(allowed) & index.live
        best = ops.chain_best_allow(allv, index, allow)
        tw, ti = ops.topk_rows(allv, k, alpha=20.0, allow=best)
        fs, fi = inf.stage_moments(m, index, qvec, tw, ti, 2, OV, n_mom)
    return dict(top_scores=tw, top_indices=ti, flat_scores=fs, flat_indices=fi, allv=allv, best=best, qn=qn)


def _assert_definition(m, index, qf, qm, allowed=None, host=None, what="", **search_kw):
    """(1) for one search; returns (the search's output, the definition)."""
    akw = {} if allowed is None else dict(video_allow=_allow_bits(allowed))
    with torch.no_grad():
        got = inf.vcmr_search(m, index, qf, qm, **dict(KW, **search_kw), **akw)
    want = _definition(m, index, qf, qm, allowed, search_kw.get("max_vcmr_video", K), search_kw.get("max_before_nms", N_MOM))
    for key in KEYS:
        assert torch.equal(_bits(got[key]), _bits(want[key])), (what, key)
    assert got["q2c"] is None
    head = index.chain_head.long()
    ti = got["top_indices"]
    assert torch.equal(got["top_videos"], torch.where(ti >= 0, head[ti.clamp_min(0).long()].to(torch.int32), ti))
    tv = got["top_videos"].cpu().numpy()
    assert all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() for r in tv)          # no video takes two places of a list
    rec, cnt = ops.moments_decode(want["flat_scores"], flat=want["flat_indices"], top_idx=want["top_indices"],
                                  meta2vid=index.slot_ids, l_ref=index.l_ref, clip_length=CLIP, seconds=True,
                                  part_offset=index.chain_offset)
    assert torch.equal(got["records"], rec) and torch.equal(got["record_count"], cnt)
    info = got["exact"]
    for a, b in zip(info["q_rescore"], want["qn"]):
        for x, y in zip(_parts(a), _parts(b)):
            assert torch.equal(_bits(x), _bits(y))
    if host is not None:
        hkw = {key: v for key, v in dict(KW, **search_kw).items() if key not in ("nms_thd", "max_after_nms")}
        with torch.no_grad():
            hrec, hcnt = inf.vcmr_search_host(m, index, query_feat=host[0].pin_memory(), query_mask=host[1].pin_memory(), **hkw, **akw)
        cnt_h, rec_h = cnt.cpu().numpy(), rec.cpu().numpy()
        np.testing.assert_array_equal(hcnt, cnt_h)
        for q in range(len(cnt_h)):
            assert hrec[q, :cnt_h[q]].tobytes() == rec_h[q, :cnt_h[q]].tobytes(), (what, q)
    return got, want


def _allowed(w):
    """The per-query mask of tests/test_gpu_index_parts_search.py: a video is numbered by its head slot."""
    rng = np.random.default_rng(17)
    allowed = rng.random((w["nq"], CAP)) < 0.7
    allowed[:, 40] = False
    allowed[:, [41, 42, 43, 44, 45]] = True                                         # (bits of its other slots mean nothing)
    allowed[2] = False
    allowed[2, [9, 37, 0]] = True                                                   # fewer allowed videos than K
    allowed[5] = False                                                              # none at all
    return allowed


# ---------------------------------------------------------------------------------------------------------
# 1. / 2. the definition, and that the world makes the fold work
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_search_is_the_definition_and_the_fold_has_work(mode, exact_chains):
    w = _w(mode)
    m = w["m"]
    index, content = _scattered(w)
    assert index.exact is not None and index.exact.mode == mode and index.part_overlap == OV and index.max_parts == 8
    assert index.chain_head is not None and index.n_live == 65 and index.n_videos_live == 46
    _tables(index)
    got, want = _assert_definition(m, index, w["qf"], w["qm"], host=(w["qf_cpu"], w["qm_cpu"]), what=mode)
    info = got["exact"]
    assert int(info["n_candidates"]) == 20 and info["q2c_filter"].shape == (w["nq"], CAP)
    n_pass = int((info["fail"] == 0).sum())
    print("%s: %d of %d queries pass their certificate in the first tier, %d full rows" % (mode, n_pass, w["nq"], info["n_full_rows"]))
    assert n_pass >= 1, "no query passes its certificate: the test shows nothing about the first tier"
    # (2) the filter proposes several parts of one video, and a part that is not a head is listed
    head = index.chain_head.cpu().numpy()
    ci = info["cand_indices"].cpu().numpy()
    assert (ci >= 0).all() and ci.shape == (w["nq"], 20)
    assert any(len(set(head[r].tolist())) < 20 for r in ci), "no candidate list holds two slots of one chain"
    cf = info["cand_folded_indices"].cpu().numpy()
    assert ((cf == ci) | (cf == -1)).all() and (cf != ci).any()
    assert all(len(set(head[r[r >= 0]].tolist())) == (r >= 0).sum() for r in cf)     # folded: one slot per video
    kept = cf >= 0
    assert torch.equal(_bits(info["cand_folded_scores"])[torch.from_numpy(kept)], _bits(info["cand_scores"])[torch.from_numpy(kept)])
    assert bool(torch.isneginf(info["cand_folded_scores"][torch.from_numpy(~kept).to(DEV)]).all())
    ti = got["top_indices"].cpu().numpy()
    assert (ti >= 0).all() and (index.chain_offset.cpu().numpy()[ti] > 0).any(), "no listed slot is a later part of its video"
    assert (_host(got["records"])["st"] > W * CLIP).any()                          # moments beyond the first l_ref clips
    # a caller's mask numbers a video by its head slot
    allowed = _allowed(w)
    got, want = _assert_definition(m, index, w["qf"], w["qm"], allowed=allowed, host=(w["qf_cpu"], w["qm_cpu"]), what=mode + " allow")
    tv = got["top_videos"].cpu().numpy()
    assert sorted(tv[2][tv[2] >= 0].tolist()) == [0, 9, 37] and (tv[5] == -1).all() and not np.isin(tv, [40]).any()
    assert IDS[6] not in set(_host(got["records"])["vid"].ravel().tolist())
    assert all(allowed[q, v] for q in range(w["nq"]) for v in tv[q][tv[q] >= 0])
    # SVMR: a video named by ANY of its slots is searched in its best part
    rng = np.random.default_rng(18)
    vids = rng.integers(0, 65, w["nq"]).astype(np.int32)
    vids[:6] = [45, 40, 30, 0, 38, 44]
    vids = np.where(np.isin(vids, index.table.live_slots()), vids, 42).astype(np.int32)
    vids[-1] = 69                                                                   # a free slot: a video of one (empty) part
    with torch.no_grad():
        sv = inf.vcmr_search(m, index, w["qf"], w["qm"], svmr_video=torch.from_numpy(vids).to(DEV), **KW)
        rows = ops.chain_best_rows(want["allv"], index, torch.from_numpy(vids).to(DEV))
    assert torch.equal(sv["svmr_rows"], rows) and (head[rows.cpu().numpy()] == head[vids]).all()
    assert (rows.cpu().numpy() != vids).any() and (index.chain_offset.cpu().numpy()[rows.cpu().numpy()] > 0).any()
    with torch.no_grad():
        qvec = inf.stage_query_vectors(m, w["qf"], w["qm"])
        st1, ed1 = inf.stage_span_probs(m, index, qvec, rows.reshape(-1, 1), ops)
        ss, sf = ops.moment_topk(st1, ed1, None, W, 2, OV, N_MOM)
    assert torch.equal(_bits(sv["svmr_scores"]), _bits(ss)) and torch.equal(sv["svmr_flat"], sf)


# ---------------------------------------------------------------------------------------------------------
# 3. every tier
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_tier_gives_the_definitions_lists(mode, exact_chains, monkeypatch):
    w = _w(mode)
    m = w["m"]
    index, content = _scattered(w)
    nq = w["nq"]
    # second tier: 12 candidates fold to fewer than 10 videos for some queries -- T_k = -inf, the certificate fails
    index.exact.n_candidates, index.exact.tier2_rows = 12, nq       # (room for every query in the on-device second tier)
    got, _ = _assert_definition(m, index, w["qf"], w["qm"], what=mode + " tier 2")
    info = got["exact"]
    short = (info["cand_folded_indices"] >= 0).sum(1) < K
    assert bool(short.any()), "every folded list holds 10 videos: lower n_candidates"
    assert bool((info["fail"][short] == 1).all()) and info["n_fail"] >= int(short.sum()) and info["n_full_rows"] == 0
    print("%s: 12 candidates: %d of %d folded lists hold fewer than %d videos, %d queries in the second tier"
          % (mode, int(short.sum()), nq, K, info["n_fail"]))
    _assert_definition(m, index, w["qf"], w["qm"], allowed=_allowed(w), what=mode + " tier 2 allow")
    # third tier (f16s) / the fallback's full f32 row (f32): the second tier's capacity is exceeded
    index.exact.tier2_cap = 10
    monkeypatch.setattr(inf, "EXACT_TIER2_CAP", 10)
    got, _ = _assert_definition(m, index, w["qf"], w["qm"], what=mode + " full rows")
    assert got["exact"]["n_full_rows"] >= int(short.sum()) > 0
    got, _ = _assert_definition(m, index, w["qf"], w["qm"], allowed=_allowed(w), what=mode + " full rows allow")
    assert got["exact"]["n_full_rows"] > 0
    # every certificate forced to fail with room in the second tier: all lists come from it
    monkeypatch.setattr(inf, "EXACT_TIER2_CAP", 4096)
    index.exact.tier2_cap, index.exact.n_candidates = 1024, 20
    index.exact.e_c_dev.fill_(10.0)
    with torch.no_grad():
        forced = inf.vcmr_search(m, index, w["qf"], w["qm"], **KW)
    want = _definition(m, index, w["qf"], w["qm"])
    assert int(forced["exact"]["fail"].sum()) == nq and forced["exact"]["n_full_rows"] == 0
    for key in KEYS:
        assert torch.equal(_bits(forced[key]), _bits(want[key])), key


# ---------------------------------------------------------------------------------------------------------
# 4. against the f32 path and against the oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_lists_are_the_plain_f32_chain_indexes(mode, exact_chains, monkeypatch):
    w = _w(mode)
    index, _ = _scattered(w)
    monkeypatch.undo()                                             # MutableCorpusIndex.create(..., part_overlap=) is itself again
    w32 = _w("f32")
    plain, _ = _scattered(w32)
    assert plain.exact is None and plain.table.live_slots() == index.table.live_slots()
    with torch.no_grad():
        out = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], **KW)
        ref = dict(inf.vcmr_search(w32["m"], plain, w["qf"], w["qm"], **KW))
    best = torch.from_numpy(_best_mask(ref["q2c"], plain)).to(DEV)
    ref["q2c"] = ref["q2c"].masked_fill(~best, float("-inf"))     # one column per video: its best part's
    n_v, n_m, n_same = _lists_equal(out, ref, W, K, N_MOM, "exact chains (%s) vs plain f32 chains" % mode)
    print("%s: %d video / %d moment positions swapped in f32 ties, %d of %d queries with identical video lists"
          % (mode, n_v, n_m, n_same, w["nq"]))
    assert n_same >= w["nq"] - 6                                  # (tests/test_gpu_index_exact.py asks 10 of 12)


def _oracle(w):
    """The oracle's numbers for the 35 parts of the world's videos, once."""
    if "exact chains oracle" not in w:
        om = O.OracleXML(w["cfg"], {k: v.detach().cpu() for k, v in w["m"].state_dict().items()})
        pvf, pvm, psf, psm = w["vs"]["cpu"]
        with torch.no_grad():
            v1, v2, s1, s2 = om.encode_context(pvf, pvm, psf, psm)
            w["exact chains oracle"] = om.get_pred_from_raw_query(w["qf_cpu"], w["qm_cpu"], v1, v2, pvm, s1, s2, psm, cross=True)
    return w["exact chains oracle"]


@pytest.mark.parametrize("mode", MODES)
def test_search_against_the_oracle(mode, exact_chains):
    """tests/test_gpu_index_parts_search.py::test_search_against_the_oracle on the exact-rank index: per query the oracle's
    search over the sub-corpus of that query's best parts, at the tolerances of tests/test_gpu_parts.py."""
    w = _w(mode)
    vs, t, nq = w["vs"], w["vs"]["table"], w["nq"]
    index = MutableCorpusIndex.create(w["m"], CAP, l_ref=W, part_overlap=OV, max_parts=8)
    index.add(*tuple(x[:3] for x in w["filler"]))
    index.remove([0, 1, 2])
    heads = index.add(*vs["dev"], ids=IDS, parts=t)
    slots = np.array([s for h in heads for s in index.table.chain_of(h)])            # part p of the table lies in slots[p]
    q2c, st, ed = _oracle(_world(torch.float32))
    with torch.no_grad():
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], max_vcmr_video=K, max_before_nms=N_MOM, max_pred_l=OV)
    excl = _excluded(q2c, t)
    assert excl.mean() <= 0.05
    s = q2c.numpy()
    gi, gw = got["top_indices"].cpu().numpy(), got["top_scores"].cpu().numpy()
    fs, fi = got["flat_scores"].cpu().numpy(), got["flat_indices"].cpu().numpy()
    gs = t.group_start
    n_same = 0
    for q in np.nonzero(~excl)[0]:
        sel = np.array([gs[v] + int(np.argmax(s[q, gs[v]:gs[v + 1]])) for v in range(t.n_videos)])    # the sub-corpus, in parts
        with torch.no_grad():
            want = O.vcmr_tail(q2c[q:q + 1, sel], st[q:q + 1, sel], ed[q:q + 1, sel], 20.0, K, 2, OV, N_MOM + 16)
        assert np.isin(gi[q], slots[sel]).all(), q
        ww, wi2 = torch.topk(torch.exp(20.0 * q2c[q:q + 1, sel]), K + 6, dim=1)
        tie_aware_equal(gi[q:q + 1], gw[q:q + 1], slots[sel[wi2.numpy()]], ww.numpy(), K, VIDEO_TOL, "videos of query %d" % q)
        wi = slots[sel[want["top_indices"].numpy()]]
        if not (gi[q:q + 1] == wi).all():
            continue
        n_same += 1
        gk, wk = moment_keys(fi[q:q + 1], gi[q:q + 1], W), moment_keys(want["flat_indices"].numpy(), wi, W)
        ws = want["flat_scores"].numpy()
        npos = int((ws[0][:N_MOM] > 0).sum())
        assert int((fi[q] >= 0).sum()) == npos, (q, npos)
        if npos > 2:
            tie_aware_equal(gk[:, :npos], fs[q:q + 1, :npos], wk, ws, max(1, npos - 2), MOMENT_TOL, "moments of query %d" % q)
    assert n_same >= 0.8 * nq


# ---------------------------------------------------------------------------------------------------------
# 5. the life cycle
# ---------------------------------------------------------------------------------------------------------
def _slot_operands(index, mod):
    """Everything an exact-rank index holds per slot for one modality (the filter rows apart)."""
    return [index.mask[mod], index.exact.err_rows[mod]] + _parts(index.feat2[mod]) + _parts(index.exact.feat1n_f32[mod])


def _assert_stand_alone(m, index, content, l_ref):
    """Every per-slot operand of the live slots is bitwise what a stand-alone put of the same rows -- each part a video of
    its own in a fresh exact-rank index without chains -- leaves in that slot, and the bound is the maximum over every row
    ever put."""
    only = _PLAIN_CREATE(MutableCorpusIndex, m, CAP, l_ref=l_ref, exact_rank=True)
    by_batch = {}
    for s, (b, r) in sorted(content.items()):
        by_batch.setdefault(id(b), (b, [], []))
        by_batch[id(b)][1].append(r), by_batch[id(b)][2].append(s)
    for b, rows, slots in by_batch.values():
        only.put(slots, only.encode(*_rows(b, rows)))
    live = index.table.live_slots()
    assert live == only.table.live_slots() == sorted(content) and torch.equal(index.live, only.live)
    sl = torch.as_tensor(live, device=DEV)
    for mod in index.modalities:
        for x, y in zip(_slot_operands(index, mod), _slot_operands(only, mod)):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x[sl]), _bits(y[sl])), mod
        a, b = index.feat1n_rows(mod), only.feat1n_rows(mod)
        valid = (index.mask[mod][sl] != 0)                       # (a packed image holds the rows of a video's run only)
        assert a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16 and torch.equal(_bits(a[sl][valid]), _bits(b[sl][valid])), mod
        if index.blocks is None:
            assert torch.equal(_bits(a[sl]), _bits(b[sl])) and torch.equal(index.mask_bits[mod][sl], only.mask_bits[mod][sl]), mod
    assert torch.equal(index.vlen[sl], only.vlen[sl])
    assert torch.equal(_bits(index.exact.e_c_dev), _bits(index.norms_put))
    assert bool((index.exact.e_c_dev >= only.exact.e_c_dev).all())


@pytest.mark.parametrize("mode", MODES)
def test_the_life_cycle(mode, exact_chains):
    w = _w(mode)
    m = w["m"]
    steps = []

    def check(step, index, content):
        steps.append(step)
        _tables(index)
        _assert_definition(m, index, w["qf"], w["qm"], what="after step %r" % step)
        _assert_stand_alone(m, index, content, W)

    for step, index, info in _life_cycle(w, W, check):
        if step == "added":
            p = info["planted"]
            got, _ = _assert_definition(m, index, p["qf"].to(DEV), p["qm"].to(DEV), what="planted", max_vcmr_video=1,
                                        max_before_nms=20)
            assert info["n_long"] == 6 and int(got["top_videos"][0, 0]) == info["head"]
            row = int(got["top_indices"][0, 0])
            off = int(index.chain_offset[row])
            top = _host(got["nms_records"])[0, 0]
            assert row in info["chain"][3:] and off in (48, 64, 68)                 # a part that holds planted clips (64 .. 95)
            assert top["vid"] == 777 and top["st"] >= off * CLIP > W * CLIP and top["ed"] <= 100 * CLIP   # behind any cut at l_ref
            # SVMR by a slot that is not the head: the best part by definition
            name = torch.tensor([info["chain"][1]], dtype=torch.int32, device=DEV)
            with torch.no_grad():
                sv = inf.vcmr_search(m, index, p["qf"].to(DEV), p["qm"].to(DEV), svmr_video=name, **KW)
            assert int(sv["svmr_rows"][0]) == row
        if step == "removed":
            with torch.no_grad():
                got = inf.vcmr_search(m, index, w["qf"], w["qm"], **KW)
            assert 777 not in set(_host(got["records"])["vid"].ravel().tolist())
            with pytest.raises(ValueError, match="unknown video id"):
                index.slot_of(777)
    assert len(steps) == 6 and index.n_videos_live == 6 + 3 + 8 - 6 + 1 and index.n_live == 4 + 3 + 4 * 2 + 6
    # tighten_error_bound: the maximum over the live slots' rows, never above the bound of every row put
    before = index.exact.e_c_dev.clone()
    index.tighten_error_bound()
    sl = torch.as_tensor(index.table.live_slots(), device=DEV)
    tight = torch.stack([index.exact.err_rows[mod][sl].max() for mod in index.modalities])
    assert torch.equal(_bits(index.exact.e_c_dev), _bits(tight)) and bool((tight <= before).all())
    _assert_definition(m, index, w["qf"], w["qm"], what="tightened")


TILES = 4


@pytest.mark.parametrize("mode", MODES)
def test_the_life_cycle_with_the_packed_filter_image(mode, exact_chains, monkeypatch):
    """l_ref = 80 (128-clip slots), hidden 256 (the smallest whose bf16 rows have a tile image), filter_tiles = 4: 64 blocks,
    an 80-clip part takes 5 -- one step finds no run until the free blocks are compacted."""
    L = 80
    m32, cfg = _synthetic_model("video_sub", 256, 256, 128, 128, L, torch.float32, seed=63)
    m = m32 if mode == "f32" else _twin_model(m32, cfg)
    qf, qm = _feats(12, np.concatenate([[30], np.random.default_rng(5).integers(3, 31, 11)]), 128, 64)
    qf, qm = qf.to(DEV), qm.to(DEV)
    w = dict(m=m, cfg=cfg)
    w["planted", L] = _planted(m32, cfg, L, 200 + L)
    exact_chains.update(filter_tiles=TILES, auto_compact=True)
    compactions = []
    compact = MutableCorpusIndex.compact
    monkeypatch.setattr(MutableCorpusIndex, "compact", lambda self: compactions.append(compact(self)) or compactions[-1])
    steps = []

    def check(step, index, content):
        steps.append(step)
        _tables(index)
        assert index.blocks is not None and sorted(index.blocks.runs()) == index.table.live_slots()
        _assert_definition(m, index, qf, qm, what="after step %r" % step)
        _assert_stand_alone(m, index, content, L)

    for step, index, info in _life_cycle(w, L, check):
        pass
    assert len(steps) == 6
    assert any(c["blocks_moved"] > 0 for c in compactions), "no step needed a compaction: the test shows nothing"
    # compact() itself changes no record
    index.remove(ids=[203, 101])
    with torch.no_grad():
        before = inf.vcmr_search(m, index, qf, qm, **KW)
        done = compact(index)
        after = inf.vcmr_search(m, index, qf, qm, **KW)
    assert done["rounds"] >= 0
    for key in KEYS + ("records", "record_count", "nms_records", "nms_count"):
        assert torch.equal(_bits(before[key]), _bits(after[key])), key
    _assert_definition(m, index, qf, qm, what="compacted")


# ---------------------------------------------------------------------------------------------------------
# 6. nothing else moved
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_an_index_without_the_keyword_launches_none_of_the_new_entries(mode, monkeypatch):
    w = _w(mode)
    m = w["m"]
    calls = {}
    for name in ("cand_best_part", "chain_spread_allow", "chain_members"):
        def counted(*a, _name=name, _fn=getattr(ops, name), **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    index = MutableCorpusIndex.create(m, CAP, l_ref=W, exact_rank=True)
    assert index.chain_head is None and index.chain_next is None and index.chain_offset is None and index.part_overlap is None
    index.exact.n_candidates = 12
    index.add(*w["filler"])
    index.remove([1, 4, 5])
    rng = np.random.default_rng(2)
    allowed = rng.random((w["nq"], CAP)) < 0.6
    gt = torch.from_numpy(rng.choice(index.table.live_slots(), w["nq"]).astype(np.int32)).to(DEV)
    kw = {key: v for key, v in KW.items() if key not in ("nms_thd", "max_after_nms")}
    with torch.no_grad():
        out = inf.vcmr_search(m, index, w["qf"], w["qm"], svmr_video=gt, video_allow=_allow_bits(allowed), **KW)
        index.exact.e_c_dev.fill_(10.0)                            # every tier behind the first one too
        inf.vcmr_search(m, index, w["qf"], w["qm"], svmr_video=gt, **KW)
        inf.vcmr_search_host(m, index, query_feat=w["qf_cpu"].pin_memory(), query_mask=w["qm_cpu"].pin_memory(), **kw)
    assert calls == {} and "cand_folded_indices" not in out["exact"] and "top_videos" not in out
    with pytest.raises(ValueError, match="without part_overlap"):
        index.add(*w["vs"]["dev"], parts=w["vs"]["table"])
    # ... and one created with it launches them where the issue says: the fold always, the spread for a caller's mask only
    chained = MutableCorpusIndex.create(m, CAP, l_ref=W, exact_rank=True, exact_part_overlap=OV, max_parts=8)
    chained.exact.n_candidates = 20
    chained.add(*tuple(t[:30] for t in w["filler"]))
    chained.add(*w["vs"]["dev"], ids=IDS, parts=w["vs"]["table"])
    with torch.no_grad():
        inf.vcmr_search(m, chained, w["qf"], w["qm"], **KW)
    assert calls.get("cand_best_part", 0) >= 1 and "chain_spread_allow" not in calls and "chain_members" not in calls
    with torch.no_grad():
        inf.vcmr_search(m, chained, w["qf"], w["qm"], svmr_video=gt, video_allow=_allow_bits(allowed), **KW)
    assert calls["chain_spread_allow"] == 1 and calls["chain_members"] == 1
    with pytest.raises(ValueError, match="parts index"):
        inf.GraphedVcmrSearch(m, chained, w["nq"], w["qf"].shape[1], w["qf"].shape[2], max_pred_l=OV)
    with pytest.raises(ValueError, match="chains of slots"):
        inf.video_subset(chained, [0, 2])
    with torch.no_grad(), pytest.raises(ValueError, match="max_pred_l"):
        inf.vcmr_search(m, chained, w["qf"], w["qm"], max_pred_l=OV + 1)
    with torch.no_grad(), pytest.raises(ValueError, match="pad_tail"):
        inf.vcmr_search(m, chained, w["qf"], w["qm"], max_pred_l=OV, pad_tail=True)
