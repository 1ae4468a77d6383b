"""Searches on an updatable index whose long videos are chains of slots (MutableCorpusIndex.create(..., part_overlap=O);
DESIGN.md section 20c).  l_ref = 32, part_overlap = 16, capacity 70 (three live words, the last one partial), hidden 128,
f32 and bf16; videos of 1, 20, 32, 33, 48, 49 and 100 clips among others.
  1. a search is bit for bit the restricted search on the plain one-shot twin with the same slot contents (every part a row
     at its slot's position) under the numpy best-part mask; eager and host-to-host;
  2. against build_corpus_index(parts=) of the same videos the records {id, st, ed, score} are equal as sorted lists;
  3. against the oracle's search over each query's own sub-corpus of best parts;
  4. the life cycle: a moment behind clip 64 of the 100-clip video is returned, the video is removed, three short videos
     land in its slots (a missing reset of the chain tables fails here), replaces that grow and shrink -- (1) after each step;
  5. the packed form (tiles=N; it needs 128-clip slots, so l_ref = 80 there): the same steps on the plain and the packed
     index give the same records, one step needs a compaction, and compact() changes no record;
  6. the refusals."""
import numpy as np
import pytest
import torch

from oracle import xml_oracle as O
from oracle.listcmp import moment_keys, tie_aware_equal
from test_gpu_index_update import CAP, _bits, _fixed
from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from test_gpu_parts import MOMENT_TOL, VIDEO_TOL, _excluded, _host, _np_records, _part_batch, _same_records
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex
from tvretrieval_amd.ingest import plan_parts

pytestmark = pytest.mark.gpu

W, OV, CLIP = 32, 16, 1.5
KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
LENS = [1, 20, 32, 33, 48, 49, 100, 5, 64, 17, 80, 32, 40, 27, 96, 12]        # 1 1 1 2 2 3 6 1 3 1 4 1 2 1 5 1 = 35 parts
IDS = [700 + 3 * i for i in range(len(LENS))]
SEED = 5          # chosen on the CPU with the oracle alone: no query of this world has two best parts of a video within the
#                   video tolerance (test 3; seeds 3, 4, 6, 7, 8: 7, 3, 1, 4, 5 of 37), and neighbouring moment scores of the
#                   oracle's lists differ by 3.5e-5 relative at the least (test 2 asserts that no two listed scores are equal)
KW = dict(max_vcmr_video=10, max_before_nms=60, max_pred_l=OV, nms_thd=0.5, max_after_nms=20, clip_length=CLIP)
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]
_CACHE = {}


def _dev(batch):
    return tuple(t.to(DEV) for t in batch)


def _video_set(lens, w, ov, seed):
    """Features of the videos `lens`, their part table at (w, ov) and the part batch (CPU and device)."""
    table = plan_parts(np.array(lens), w, ov)
    vf, _ = _feats(len(lens), lens, 256, 70 + seed)
    sf, _ = _feats(len(lens), lens, 128, 80 + seed)
    pvf, pvm = _part_batch(vf, lens, table, 256)
    psf, psm = _part_batch(sf, lens, table, 128)
    cpu = (pvf, pvm, psf, psm)
    return dict(lens=list(lens), table=table, cpu=cpu, dev=_dev(cpu))


def _world(dtype):
    if dtype in _CACHE:
        return _CACHE[dtype]
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, W, dtype, seed=60 + SEED)
    rng = np.random.default_rng(90 + SEED)
    qf, qm = _feats(37, np.concatenate([[30], rng.integers(3, 31, 36)]), 128, 100 + SEED)
    fill_lens = rng.integers(4, W + 1, 36).tolist()
    fv, fm = _feats(36, fill_lens, 256, 110 + SEED)
    fs, _ = _feats(36, fill_lens, 128, 120 + SEED)
    w = dict(m=m, cfg=cfg, dtype=dtype, vs=_video_set(LENS, W, OV, SEED), filler=_dev((fv, fm, fs, fm)), qf=qf.to(DEV), qm=qm.to(DEV),
             qf_cpu=qf, qm_cpu=qm, nq=37)
    _CACHE[dtype] = w
    return w


def _add_chains(index, content, vs, ids, **kw):
    """add the videos of a video set as chains; record the slot contents; returns the head slots"""
    heads = index.add(*vs["dev"], ids=ids, parts=vs["table"], **kw)
    slots = [s for h in heads for s in index.table.chain_of(h)]
    assert len(slots) == vs["table"].n_parts
    content.update({s: (vs["dev"], r) for r, s in enumerate(slots)})
    return heads


def _scattered(w, l_ref=W, **create_kw):
    """36 short videos, six of them removed again, then the 16 videos of the world as chains: their 35 parts take the six
    scattered slots and slots 36 .. 64 -- chains cross both word boundaries.  -> (index, content)"""
    index = MutableCorpusIndex.create(w["m"], CAP, l_ref=l_ref, part_overlap=OV, max_parts=8, **create_kw)
    content = {}
    slots = index.add(*w["filler"])
    assert slots == list(range(36)) and index.n_videos_live == 36
    content.update({s: (w["filler"], r) for r, s in enumerate(slots)})
    gone = [1, 4, 5, 9, 30, 31]
    assert index.remove(gone) == gone
    for s in gone:
        del content[s]
    heads = _add_chains(index, content, w["vs"], IDS)
    assert heads[:6] == [1, 4, 5, 9, 31, 37] and index.table.chain_of(9) == [9, 30] and index.table.chain_of(37) == [37, 38, 39]
    assert index.table.chain_of(40) == [40, 41, 42, 43, 44, 45] and max(content) == 64
    assert index.n_live == 30 + 35 and index.n_videos_live == 30 + 16
    return index, content


def _tables(index):
    """The device chain tables; they must be the host table's mirror, with every free slot in the single state."""
    head, nxt, off = (t.cpu().numpy() for t in (index.chain_head, index.chain_next, index.chain_offset))
    for s in range(CAP):
        assert (head[s], nxt[s], off[s]) == index.table.state(s), s
        if not index.table.is_live(s):
            assert (head[s], nxt[s], off[s]) == (s, -1, 0), s
    return head, nxt, off


def _best_mask(q2c, index, allowed=None):
    """numpy restatement of the fold on the index's host table: (nq, CAP) bool, one True per allowed live video, at its best
    part (first maximum in chain order, NaN as -inf).  allowed (1 | nq, CAP) bool numbers a video by its head slot."""
    s = q2c.detach().float().cpu().numpy()
    nq = s.shape[0]
    out = np.zeros((nq, CAP), dtype=bool)
    for h in index.table.heads():
        ch = index.table.chain_of(h)
        ok = np.ones(nq, dtype=bool) if allowed is None else np.broadcast_to(allowed, (nq, CAP))[:, h]
        if len(ch) == 1:
            out[ok, h] = True
            continue
        v = s[:, ch].copy()
        v[np.isnan(v)] = -np.inf
        best = np.asarray(ch)[np.argmax(v, axis=1)]
        out[np.nonzero(ok)[0], best[ok]] = True
    return out


def _allow_bits(mask):
    return inf.pack_video_allow(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV))


def _assert_equals_the_twin(w, index, content, allowed=None, host=False, l_ref=W):
    """(1): the search on `index` against the restricted search on its plain twin under the numpy best-part mask."""
    m = w["m"]
    head, nxt, off = _tables(index)
    akw = {} if allowed is None else dict(video_allow=_allow_bits(allowed))
    with torch.no_grad():
        got = inf.vcmr_search(m, index, w["qf"], w["qm"], **KW, **akw)
        mask = _best_mask(got["q2c"], index, allowed)
        twin = _fixed(m, l_ref, content)
        want = inf.vcmr_search(m, twin, w["qf"], w["qm"], video_allow=_allow_bits(mask), **KW)
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    ti = got["top_indices"].cpu().numpy()
    tv = got["top_videos"].cpu().numpy()
    assert (tv == np.where(ti >= 0, head[np.maximum(ti, 0)], -1)).all()
    assert all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() for r in tv)          # no video takes two places of a list
    ids = index.slot_ids.cpu().numpy()
    rec, cnt = _np_records(want["flat_scores"].cpu().numpy(), want["flat_indices"].cpu().numpy(), ti, ids, off, l_ref, CLIP, True)
    _same_records(_host(got["records"]), rec, "records")
    assert (got["record_count"].cpu().numpy() == cnt).all()
    nrec, nidx, ncnt = ops.nms_moments(got["records"], got["record_count"], True, KW["nms_thd"], max_before=60, max_after=20)
    assert torch.equal(got["nms_records"], nrec) and torch.equal(got["nms_count"], ncnt)
    if host:
        hkw = {k: v for k, v in KW.items() if k not in ("nms_thd", "max_after_nms")}
        with torch.no_grad():
            hrec, hcnt = inf.vcmr_search_host(m, index, query_feat=w["qf_cpu"].pin_memory(), query_mask=w["qm_cpu"].pin_memory(),
                                              **hkw, **akw)
        np.testing.assert_array_equal(hcnt, cnt)
        live = np.arange(hrec.shape[1])[None] < hcnt[:, None]
        for col in ("vid", "st", "ed", "score"):
            np.testing.assert_array_equal(np.where(live, hrec[col], 0).view(np.int32), np.where(live, rec[col], 0).view(np.int32),
                                          err_msg=col)
    return got, mask


def _record_lists(rec, cnt):
    """Per query the sorted list of (id, st, ed, score) bit patterns."""
    out = []
    for q in range(len(cnt)):
        r = rec[q][: int(cnt[q])]
        out.append(sorted(zip(r["vid"].tolist(), r["st"].view(np.int32).tolist(), r["ed"].view(np.int32).tolist(),
                              r["score"].view(np.int32).tolist())))
    return out


# ---------------------------------------------------------------------------------------------------------
# 1. the restricted search on the twin
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_is_the_restricted_search_on_the_plain_twin(dtype):
    w = _world(dtype)
    index, content = _scattered(w)
    got, mask = _assert_equals_the_twin(w, index, content, host=True)
    assert mask.sum(1).tolist() == [46] * w["nq"]
    assert (_host(got["records"])["st"] > W * CLIP).any()                          # moments beyond the first l_ref clips
    ti = got["top_indices"].cpu().numpy()
    assert (index.chain_offset.cpu().numpy()[ti[ti >= 0]] > 0).any()                # a part that is not a head is listed
    # a caller's mask numbers a video by its head slot; one that clears the head of the 100-clip video removes all of it
    rng = np.random.default_rng(17)
    allowed = rng.random((w["nq"], CAP)) < 0.7
    allowed[:, 40] = False
    allowed[:, [41, 42, 43, 44, 45]] = True                                         # (bits of its other slots mean nothing)
    allowed[2] = False
    allowed[2, [9, 37, 0]] = True                                                   # fewer allowed videos than K
    allowed[5] = False                                                              # none at all
    got, mask = _assert_equals_the_twin(w, index, content, allowed=allowed, host=True)
    assert not mask[:, 40:46].any() and mask[2].sum() == 3 and not mask[5].any()
    tv = got["top_videos"].cpu().numpy()
    assert sorted(tv[2][tv[2] >= 0].tolist()) == [0, 9, 37] and (tv[5] == -1).all()
    assert IDS[6] not in set(_host(got["records"])["vid"].ravel().tolist())
    # SVMR / ground-truth videos are named by ANY slot of theirs: the best part for that query stands for the video
    vids = rng.integers(0, 65, w["nq"]).astype(np.int32)
    vids[:4] = [45, 40, 30, 0]
    vids = np.where(np.isin(vids, index.table.live_slots()), vids, 40).astype(np.int32)
    with torch.no_grad():
        sv = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], svmr_video=torch.from_numpy(vids).to(DEV), **KW)
    full = _best_mask(sv["q2c"], index)
    rows = np.array([next(s for s in index.table.chain_of(int(v)) if full[q, s]) for q, v in enumerate(vids)], dtype=np.int32)
    assert (sv["svmr_rows"].cpu().numpy() == rows).all()
    with torch.no_grad():
        want = inf.vcmr_search(w["m"], _fixed(w["m"], W, content), w["qf"], w["qm"], svmr_video=torch.from_numpy(rows).to(DEV), **KW)
    for k in ("svmr_scores", "svmr_flat"):
        assert torch.equal(sv[k], want[k]), k
    rec, _ = _np_records(want["svmr_scores"].cpu().numpy(), want["svmr_flat"].cpu().numpy(), None, index.slot_ids.cpu().numpy(),
                         index.chain_offset.cpu().numpy(), W, CLIP, False, row_vid=rows)
    _same_records(_host(sv["svmr_records"]), rec, "svmr records")


# ---------------------------------------------------------------------------------------------------------
# 2. against the fixed parts index of the same videos
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_records_equal_those_of_the_fixed_parts_index(dtype):
    w = _world(dtype)
    index = MutableCorpusIndex.create(w["m"], CAP, l_ref=W, part_overlap=OV, max_parts=8)
    content = {}
    index.add(*tuple(t[:7] for t in w["filler"]))
    index.remove([0, 2, 3, 6])
    _add_chains(index, content, w["vs"], IDS)                     # chains over 0 2 3 6 7 8 ...; the fillers 1 4 5 stay
    index.remove([1, 4, 5])
    assert index.n_videos_live == len(LENS) and index.n_live == 35
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        fixed = inf.build_corpus_index(w["m"], [w["vs"]["dev"]], parts=w["vs"]["table"], l_ref=W, length_buckets=False)
        want = inf.vcmr_search(w["m"], fixed, w["qf"], w["qm"], meta2vid=ids, **KW)
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], **KW)
    wrec, wcnt = _host(want["records"]), want["record_count"].cpu().numpy()
    # the precondition: the fixed parts index lists no two moments of a query with one score, and no two videos with one weight
    for q in range(w["nq"]):
        sc = wrec["score"][q][: int(wcnt[q])]
        assert len(np.unique(sc)) == len(sc), "query %d: tied moment scores -- choose another SEED" % q
        tw = want["top_scores"][q].cpu().numpy()
        assert len(np.unique(tw)) == len(tw), "query %d: tied video weights -- choose another SEED" % q
    assert _record_lists(_host(got["records"]), got["record_count"].cpu().numpy()) == _record_lists(wrec, wcnt)
    assert _record_lists(_host(got["nms_records"]), got["nms_count"].cpu().numpy()) == \
        _record_lists(_host(want["nms_records"]), want["nms_count"].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------
# 3. against the oracle: per query, its search over the sub-corpus of that query's best parts
# ---------------------------------------------------------------------------------------------------------
def test_search_against_the_oracle():
    w = _world(torch.float32)
    vs, t, kv, n_mom, nq = w["vs"], w["vs"]["table"], 10, 60, w["nq"]
    index = MutableCorpusIndex.create(w["m"], CAP, l_ref=W, part_overlap=OV, max_parts=8)
    index.add(*tuple(x[:3] for x in w["filler"]))
    index.remove([0, 1, 2])
    heads = index.add(*vs["dev"], ids=IDS, parts=t)
    slots = np.array([s for h in heads for s in index.table.chain_of(h)])            # part p of the table lies in slots[p]
    om = O.OracleXML(w["cfg"], {k: v.detach().cpu() for k, v in w["m"].state_dict().items()})
    pvf, pvm, psf, psm = vs["cpu"]
    with torch.no_grad():
        v1, v2, s1, s2 = om.encode_context(pvf, pvm, psf, psm)
        q2c, st, ed = om.get_pred_from_raw_query(w["qf_cpu"], w["qm_cpu"], v1, v2, pvm, s1, s2, psm, cross=True)
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], max_vcmr_video=kv, max_before_nms=n_mom, max_pred_l=OV)
    excl = _excluded(q2c, t)
    print("oracle: %d of %d queries have two best parts of a video within the tolerance" % (excl.sum(), nq))
    assert excl.mean() <= 0.05
    s = q2c.numpy()
    gi, gw = got["top_indices"].cpu().numpy(), got["top_scores"].cpu().numpy()
    fs, fi = got["flat_scores"].cpu().numpy(), got["flat_indices"].cpu().numpy()
    gs = t.group_start
    n_same = 0
    for q in np.nonzero(~excl)[0]:
        sel = np.array([gs[v] + int(np.argmax(s[q, gs[v]:gs[v + 1]])) for v in range(t.n_videos)])    # the sub-corpus, in parts
        with torch.no_grad():
            want = O.vcmr_tail(q2c[q:q + 1, sel], st[q:q + 1, sel], ed[q:q + 1, sel], 20.0, kv, 2, OV, n_mom + 16)
        assert np.isin(gi[q], slots[sel]).all(), q
        ww, wi2 = torch.topk(torch.exp(20.0 * q2c[q:q + 1, sel]), kv + 6, dim=1)
        tie_aware_equal(gi[q:q + 1], gw[q:q + 1], slots[sel[wi2.numpy()]], ww.numpy(), kv, VIDEO_TOL, "videos of query %d" % q)
        wi = slots[sel[want["top_indices"].numpy()]]
        if not (gi[q:q + 1] == wi).all():
            continue
        n_same += 1
        gk, wk = moment_keys(fi[q:q + 1], gi[q:q + 1], W), moment_keys(want["flat_indices"].numpy(), wi, W)
        ws = want["flat_scores"].numpy()
        npos = int((ws[0][:n_mom] > 0).sum())
        assert int((fi[q] >= 0).sum()) == npos, (q, npos)
        if npos > 2:
            tie_aware_equal(gk[:, :npos], fs[q:q + 1, :npos], wk, ws, max(1, npos - 2), MOMENT_TOL, "moments of query %d" % q)
    assert n_same >= 0.8 * nq


# ---------------------------------------------------------------------------------------------------------
# 4. / 5. the life cycle, plain and packed
# ---------------------------------------------------------------------------------------------------------
def _planted(m, cfg, w_clips, seed):
    """A query and a video of 3 * w_clips + 4 clips whose clips [2 w, 3 w) are the segment the ORACLE scores best for the
    query; its other clips come from the worst segments, the other videos are middling segments (one part each)."""
    n_seg = 40
    pv, pm = _feats(n_seg, [w_clips] * n_seg, 256, seed + 1)
    ps, _ = _feats(n_seg, [w_clips] * n_seg, 128, seed + 2)
    qf, qm = _feats(1, [12], 128, seed + 3)
    om = O.OracleXML(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        v1, v2, s1, s2 = om.encode_context(pv, pm, ps, pm)
        seg = om.get_pred_from_raw_query(qf, qm, v1, v2, pm, s1, s2, pm, cross=True)[0][0].numpy()
    order = np.argsort(seg)
    worst, best, others = order[:3], order[-1], order[12:24]
    assert seg[best] - seg[others].max() > 1e-3
    long_v = torch.cat([pv[worst[0]], pv[worst[1]], pv[best], pv[worst[2]][:4]])
    long_s = torch.cat([ps[worst[0]], ps[worst[1]], ps[best], ps[worst[2]][:4]])
    return dict(qf=qf, qm=qm, long=(long_v, long_s), others=[(pv[i], ps[i]) for i in others])


def _videos(pairs, w_clips, ov):
    """A video set from (video clips, sub clips) pairs of any length."""
    lens = [int(v.shape[0]) for v, _ in pairs]
    table = plan_parts(np.array(lens), w_clips, ov)
    lmax = max(lens)
    pad = lambda x: torch.cat([x, x.new_zeros(lmax - x.shape[0], x.shape[1])])           # noqa: E731
    fv, fs = torch.stack([pad(v) for v, _ in pairs]), torch.stack([pad(s) for _, s in pairs])
    pvf, pvm = _part_batch(fv, lens, table, 256)
    psf, psm = _part_batch(fs, lens, table, 128)
    return dict(lens=lens, table=table, dev=_dev((pvf, pvm, psf, psm)))


def _life_cycle(w, l_ref, check, **create_kw):
    """The steps of test 4 on an index of l_ref-clip slots; check(step, index, content) runs after each.  The long video has
    3 l_ref + 4 clips (100 at l_ref = 32: parts at 0 16 32 48 64 68), the planted segment is its clips [2 l_ref, 3 l_ref)."""
    m = w["m"]
    if ("planted", l_ref) not in w:
        w["planted", l_ref] = _planted(m, w["cfg"], l_ref, 200 + l_ref)
    p = w["planted", l_ref]
    cut = lambda x, n: x[:n]                                                              # noqa: E731
    index = MutableCorpusIndex.create(m, CAP, l_ref=l_ref, part_overlap=OV, max_parts=16, **create_kw)
    content = {}
    first = _videos(p["others"][:8], l_ref, OV)
    assert _add_chains(index, content, first, list(range(100, 108))) == list(range(8))
    index.remove([2, 5])
    del content[2], content[5]
    long = _videos([p["long"]], l_ref, OV)
    n_long = long["table"].n_parts
    (head,) = _add_chains(index, content, long, [777])
    chain = index.table.chain_of(head)
    assert head == 2 and chain[:3] == [2, 5, 8] and len(chain) == n_long and index.slot_of(777) == 2
    check("add", index, content)
    yield "added", index, dict(head=head, chain=chain, planted=p, n_long=n_long)
    # remove it by one of its middle slots: the whole chain goes, every slot back in the single state
    assert sorted(index.remove([chain[3]])) == sorted(chain)
    for s in chain:
        del content[s]
    check("remove", index, content)
    yield "removed", index, None
    # three short videos land in the freed slots; the fold must treat each as a video of one part
    short = _videos([(cut(v, 11 + 3 * i), cut(s, 11 + 3 * i)) for i, (v, s) in enumerate(p["others"][8:11])], l_ref, OV)
    assert _add_chains(index, content, short, [201, 202, 203]) == chain[:3]
    check("add three short videos into the freed slots", index, content)
    yield "three short", index, None
    # replace a short video by one of 2 l_ref - OV + 1 clips (49 at l_ref = 32: three parts), named by its id: it keeps its
    # slot as the head and takes the two lowest free slots
    more = l_ref - OV + 1
    grown = _videos([(torch.cat([p["others"][11][0], p["others"][0][0][:more]]), torch.cat([p["others"][11][1], p["others"][0][1][:more]]))],
                    l_ref, OV)
    assert grown["table"].n_parts == 3
    free2 = sorted(set(range(CAP)) - set(index.table.live_slots()))[:2]
    assert index.replace(None, *grown["dev"], ids=[202], parts=grown["table"]) == [chain[1]]
    new_chain = index.table.chain_of(chain[1])
    assert new_chain == [chain[1]] + free2 and free2 == [9, 10] and index.slot_of(202) == chain[1]
    content.update({s: (grown["dev"], r) for r, s in enumerate(new_chain)})
    check("replace: a short video grows to three parts", index, content)
    yield "grown", index, None
    # ... and that one by a 20-clip video, named by its last slot: two slots are freed and reset
    small = _videos([(cut(p["others"][3][0], 20), cut(p["others"][3][1], 20))], l_ref, OV)
    assert index.replace([new_chain[2]], *small["dev"], parts=small["table"]) == [chain[1]]
    assert index.table.chain_of(chain[1]) == [chain[1]] and index.table.id_of(chain[1]) == 202
    content[chain[1]] = (small["dev"], 0)
    del content[new_chain[1]], content[new_chain[2]]
    check("replace: three parts shrink to one", index, content)
    yield "shrunk", index, None
    # eight videos of 40 clips, six removals that leave scattered holes, and the long video once more: in the packed form
    # (tiles = TILES at l_ref = 80) its parts find no runs of 5 blocks until the free blocks are compacted
    oth = p["others"]
    forty = _videos([(torch.cat([oth[i][0], oth[i + 1][0]])[:40], torch.cat([oth[i][1], oth[i + 1][1]])[:40]) for i in range(8)],
                    l_ref, OV)
    _add_chains(index, content, forty, list(range(300, 308)))
    for s in index.remove(ids=[300, 302, 304, 306, 100, 103]):
        del content[s]
    (head,) = _add_chains(index, content, long, [778])
    assert head == 0 and len(index.table.chain_of(0)) == n_long and index.table.chain_of(0)[:3] == [0, 3, 9]
    check("the long video again, into scattered slots", index, content)
    yield "again", index, None


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_life_cycle(dtype):
    w = _world(dtype)

    def check(step, index, content):
        try:
            _assert_equals_the_twin(w, index, content)
        except AssertionError as e:
            raise AssertionError("after step %r: %s" % (step, e))

    for step, index, info in _life_cycle(w, W, check):
        if step == "added":
            p = info["planted"]
            kw = dict(KW, max_vcmr_video=1, max_before_nms=20)
            with torch.no_grad():
                got = inf.vcmr_search(w["m"], index, p["qf"].to(DEV), p["qm"].to(DEV), **kw)
            assert info["n_long"] == 6 and int(got["top_videos"][0, 0]) == info["head"]
            row = int(got["top_indices"][0, 0])
            off = int(index.chain_offset[row])
            top = _host(got["nms_records"])[0, 0]
            print("planted: best part at slot %d, offset %d; top moment %s" % (row, off, top))
            assert row in info["chain"][3:] and off in (48, 64, 68)                 # a part that holds planted clips (64 .. 95)
            assert top["vid"] == 777 and top["st"] >= off * CLIP > W * CLIP and top["ed"] <= 100 * CLIP   # behind any cut at l_ref
        if step == "removed":
            with torch.no_grad():
                got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], **KW)
            assert 777 not in set(_host(got["records"])["vid"].ravel().tolist())
            with pytest.raises(ValueError, match="unknown video id"):
                index.slot_of(777)
    assert index.n_videos_live == 6 + 3 + 8 - 6 + 1 and index.n_live == 4 + 3 + 4 * 2 + 6


TILES = 4


def test_the_packed_form_gives_the_plain_forms_records(monkeypatch):
    """l_ref = 80 (128-clip slots: the packed K6 image needs them), f32.  Every part takes a run of its own; with tiles = 4
    (64 blocks; an 80-clip part takes 5) one step of the sequence finds no run until the free blocks are compacted."""
    L = 80
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, L, torch.float32, seed=63)
    qf, qm = _feats(12, np.concatenate([[30], np.random.default_rng(5).integers(3, 31, 11)]), 128, 64)
    w = dict(m=m, cfg=cfg)
    seen = {"plain": [], "packed": []}
    compactions = []
    compact = MutableCorpusIndex.compact
    monkeypatch.setattr(MutableCorpusIndex, "compact", lambda self: compactions.append(compact(self)) or compactions[-1])

    def lists(index):
        with torch.no_grad():
            got = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), **KW)
        _tables(index)
        return (_record_lists(_host(got["records"]), got["record_count"].cpu().numpy()),
                _record_lists(_host(got["nms_records"]), got["nms_count"].cpu().numpy()))

    for _ in _life_cycle(w, L, lambda step, index, content: seen["plain"].append((step, lists(index)))):
        pass
    assert not compactions
    for _, packed, _ in _life_cycle(w, L, lambda step, index, content: seen["packed"].append((step, lists(index))),
                                    tiles=TILES, auto_compact=True):
        pass
    assert [s for s, _ in seen["plain"]] == [s for s, _ in seen["packed"]] and len(seen["plain"]) == 6
    for (step, plain), (_, pack) in zip(seen["plain"], seen["packed"]):
        assert any(plain[0]) and plain == pack, step
    assert any(c["blocks_moved"] > 0 for c in compactions), "no step needed a compaction: the test shows nothing"
    # compact() itself changes no record
    packed.remove(ids=[203, 101])
    before = lists(packed)
    done = compact(packed)
    assert lists(packed) == before and done["rounds"] >= 0


# ---------------------------------------------------------------------------------------------------------
# 6. the refusals
# ---------------------------------------------------------------------------------------------------------
def test_the_refusals():
    w = _world(torch.float32)
    m = w["m"]
    index = MutableCorpusIndex.create(m, CAP, l_ref=W, part_overlap=OV, max_parts=4)
    few = _video_set([20, 48, 33], W, OV, 5)
    index.add(*few["dev"], parts=few["table"])
    with torch.no_grad():
        free = inf.vcmr_search(m, index, w["qf"], w["qm"], max_vcmr_video=3, max_before_nms=20, max_pred_l=OV)
        with pytest.raises(ValueError, match="parts index"):                    # the wording of the fixed parts index's refusal
            inf.GraphedVcmrSearch(m, index, w["nq"], w["qf"].shape[1], w["qf"].shape[2], max_pred_l=OV)
        with pytest.raises(ValueError, match="max_pred_l"):
            inf.vcmr_search(m, index, w["qf"], w["qm"], max_pred_l=OV + 1)
        with pytest.raises(ValueError, match="max_pred_l"):
            inf.vcmr_search_host(m, index, query_feat=w["qf_cpu"].pin_memory(), query_mask=w["qm_cpu"].pin_memory(), max_pred_l=17)
        with pytest.raises(ValueError, match="external_top"):
            inf.vcmr_search(m, index, w["qf"], w["qm"], max_pred_l=OV, external_top=(free["top_indices"], free["top_scores"]))
        with pytest.raises(ValueError, match="pad_tail"):
            inf.vcmr_search(m, index, w["qf"], w["qm"], max_pred_l=OV, pad_tail=True)
        with pytest.raises(ValueError, match="pad_tail"):
            inf.vcmr_search_host(m, index, query_feat=w["qf_cpu"].pin_memory(), query_mask=w["qm_cpu"].pin_memory(), max_pred_l=OV,
                                 pad_tail=True)
    before = (index.n_live, index.n_videos_live, index.chain_next.clone())
    for lens, wd, ov, match in (([20, 48], W, 8, "part_overlap = 16"), ([20, 100], 48, OV, "l_ref = 32"), ([100], W, OV, "max_parts")):
        bad = _video_set(lens, wd, ov, 6)
        with pytest.raises(ValueError, match=match):
            index.add(*bad["dev"], parts=bad["table"])
    with pytest.raises(ValueError, match="parts"):                               # rows of the batch != parts of the table
        index.add(*tuple(t[:2] for t in few["dev"]), parts=few["table"])
    with pytest.raises(ValueError, match="part of the video"):
        index.put([2], index.encode(*tuple(t[:1] for t in few["dev"])))
    assert (index.n_live, index.n_videos_live) == before[:2] and torch.equal(index.chain_next, before[2])
    plain = MutableCorpusIndex.create(m, CAP, l_ref=W)
    with pytest.raises(ValueError, match="without part_overlap"):
        plain.add(*few["dev"], parts=few["table"])
    assert plain.chain_head is None and plain.n_videos_live == 0
