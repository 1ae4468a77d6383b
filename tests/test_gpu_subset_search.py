"""Searches through a subset view (inference.video_subset; vcmr_search(subset=view)) against the restricted search of the same
index, vcmr_search(video_allow=view.allow): bitwise the same lists and, on the view's columns, the same score matrix -- for
every form of parent a view is made of.  70 videos of 1..100 clips (l_ref = 100, lpad 128), 9 queries, K = 10."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex

pytestmark = pytest.mark.gpu

NV, NQ, L = 70, 9, 100
KW = dict(max_vcmr_video=10, max_before_nms=60)
KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
PARENTS = ["oneshot-full", "oneshot-masks", "oneshot-bucketed", "oneshot-f32-h128", "oneshot-exact", "mutable-plain",
           "mutable-packed", "mutable-exact"]
SUBSETS = ["one", "half", "all", "six", "empty"]
_MODELS, _WORLDS, _DATA = {}, {}, {}


def _lens(seed=31):
    lens = np.random.default_rng(seed).integers(1, L + 1, NV)
    lens[[0, 1, 2, 3]] = [L, 16, 17, L]
    return lens


def _model(dtype, hidden):
    if (dtype, hidden) not in _MODELS:
        m, cfg = _synthetic_model("video_sub", hidden, 256, 128, 128, L, torch.float32 if dtype is ops.F16S else dtype, seed=70)
        if dtype is ops.F16S:
            from tvretrieval_amd.model_xml import XML
            mx = XML(cfg, compute_dtype=ops.F16S)
            mx.load_state_dict(m.state_dict())
            m = mx.to(DEV).eval()
        _MODELS[dtype, hidden] = m
    return _MODELS[dtype, hidden]


def _batch(lens, seed):
    key = (tuple(int(x) for x in lens), seed)
    if key not in _DATA:
        vf, vm = _feats(len(lens), lens, 256, 2 * seed + 1)
        sf, sm = _feats(len(lens), lens, 128, 2 * seed + 2)
        _DATA[key] = tuple(t.to(DEV) for t in (vf, vm, sf, sm))
    return _DATA[key]


def _queries():
    if "q" not in _DATA:
        qf, qm = _feats(NQ, np.concatenate([[30], np.random.default_rng(5).integers(3, 31, NQ - 1)]), 128, 5)
        _DATA["q"] = (qf.to(DEV), qm.to(DEV))
    return _DATA["q"]


def _world(name):
    if name in _WORLDS:
        return _WORLDS[name]
    lens = _lens()
    with torch.no_grad():
        if name == "oneshot-full":                      # every video at the full length: the plain two-videos-per-tile image
            m = _model(torch.bfloat16, 256)
            index = inf.build_corpus_index(m, [_batch(np.full(NV, L), 1)])
            assert index.feat1n["video"].plan is None
        elif name == "oneshot-masks":                   # ragged, binary masks as bit words on the plain image
            m = _model(torch.bfloat16, 256)
            index = inf.build_corpus_index(m, [_batch(lens, 2)], length_buckets=False)
            assert index.feat1n["video"].plan is None and index.feat1n["video"].mask_bits is not None
        elif name == "oneshot-bucketed":
            m = _model(torch.bfloat16, 256)
            index = inf.build_corpus_index(m, [_batch(lens, 2)])
            assert index.feat1n["video"].plan is not None
        elif name == "oneshot-f32-h128":
            m = _model(torch.float32, 128)
            index = inf.build_corpus_index(m, [_batch(lens, 2)])
        elif name == "oneshot-exact":
            m = _model(ops.F16S, 256)                   # (bf16 filter rows of 512 bytes: the tiled image)
            index = inf.build_corpus_index(m, [_batch(lens, 2)], exact_filter=True)
            index.exact.n_candidates = 16               # fewer candidates than videos: the filter really filters
        elif name == "mutable-plain":
            m = _model(torch.bfloat16, 256)
            index = MutableCorpusIndex.create(m, NV)
            index.add(*_batch(lens, 2))
        elif name == "mutable-packed":                  # runs scattered by a remove and a replace
            m = _model(torch.bfloat16, 256)
            index = MutableCorpusIndex.create(m, NV, tiles=20)
            index.add(*_batch(lens[:40], 3), n_clips=lens[:40].tolist())
            index.add(*_batch(lens[40:], 4), n_clips=lens[40:].tolist())
            index.remove([5, 9, 30, 31, 50])
            index.replace([12, 40, 41], *_batch([90, 3, 40], 6), n_clips=[90, 3, 40])
            index.add(*_batch([20, 100], 7), n_clips=[20, 100])
        elif name == "mutable-exact":
            m = _model(torch.float32, 256)
            index = MutableCorpusIndex.create(m, NV, exact_rank=True)
            index.add(*_batch(lens, 2))
            index.exact.n_candidates = 16
        else:
            raise KeyError(name)
    live = np.arange(NV) if index.live is None else np.asarray(index.table.live_slots())
    qf, qm = _queries()
    w = dict(m=m, index=index, live=live, qf=qf, qm=qm)
    with torch.no_grad():
        w["free"] = _clone(inf.vcmr_search(m, index, qf, qm, **KW))
    _WORLDS[name] = w
    return w


def _clone(out):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def _members(w, which):
    live = w["live"]
    rng = np.random.default_rng(41)
    if which == "one":
        return live[[17]]
    if which == "half":
        return np.sort(rng.choice(live, len(live) // 2, replace=False))
    if which == "all":
        return live
    if which == "six":
        return np.sort(rng.choice(live, 6, replace=False))
    return live[:0]


def _matrix(out):
    return out["q2c"] if out.get("exact") is None else out["exact"]["q2c_filter"]


def _assert_same(got, want, cols, what=""):
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (what, k)
    sl = torch.as_tensor(np.asarray(cols), device=DEV, dtype=torch.long)
    a, b = _matrix(got).index_select(1, sl), _matrix(want).index_select(1, sl)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, "score matrix on the view's columns")


def _search(w, **kw):
    with torch.no_grad():
        return inf.vcmr_search(w["m"], w["index"], w["qf"], w["qm"], **dict(KW, **kw))


@pytest.mark.parametrize("which", SUBSETS)
@pytest.mark.parametrize("parent", PARENTS)
def test_subset_search_is_bitwise_the_restricted_search(parent, which):
    w = _world(parent)
    members = _members(w, which)
    view = inf.video_subset(w["index"], members.tolist())
    allowed = np.zeros(NV, dtype=bool)
    allowed[members] = True
    assert view.n_videos == len(members) and view.video_ids.cpu().tolist() == members.tolist()
    assert torch.equal(view.allow, inf.pack_video_allow(torch.from_numpy(allowed).to(DEV)))
    assert view.n_tiles >= 1 and view.hbm_bytes() > 0 and view.codes.shape == (2 * view.n_tiles, 8)
    want = _search(w, video_allow=view.allow)
    got = _search(w, subset=view)
    _assert_same(got, want, members, (parent, which))
    ti = got["top_indices"].cpu().numpy()
    n = min(KW["max_vcmr_video"], len(members))
    assert np.isin(ti[:, :n], members).all() and (ti[:, n:] == -1).all()          # fewer than K members: empty slots
    if which == "all":
        for k in KEYS:
            assert torch.equal(got[k].view(torch.int32), w["free"][k].view(torch.int32)), k
    if which == "empty":
        assert view.n_tiles == 1 and (view.codes == -2).all() and not view.allow.any()
        assert (got["flat_indices"] == -1).all()
    again = _search(w)                                                            # subset=None: today's pass, untouched
    for k in KEYS:
        assert torch.equal(again[k].view(torch.int32), w["free"][k].view(torch.int32)), k


@pytest.mark.parametrize("parent", ["oneshot-bucketed", "mutable-packed"])
def test_bool_array_and_fixed_tiles_give_the_same_view(parent):
    w = _world(parent)
    members = _members(w, "half")
    allowed = np.zeros(NV, dtype=bool)
    allowed[members] = True
    a = inf.video_subset(w["index"], members.tolist())
    b = inf.video_subset(w["index"], torch.from_numpy(allowed), tiles=a.n_tiles + 3)
    assert b.n_tiles == a.n_tiles + 3 and (b.codes[2 * a.n_tiles:] == -2).all()
    assert torch.equal(a.codes, b.codes[:2 * a.n_tiles]) and torch.equal(a.allow, b.allow)
    _assert_same(_search(w, subset=b), _search(w, subset=a), members)


def test_a_per_query_mask_on_top_is_the_and_on_the_parent():
    w = _world("oneshot-bucketed")
    members = _members(w, "half")
    view = inf.video_subset(w["index"], members.tolist())
    rng = np.random.default_rng(43)
    for rows in (1, NQ):
        extra = rng.random((rows, NV)) < 0.6
        extra[0] = False if rows == NQ else extra[0]                              # (a query with nothing allowed)
        bits = inf.pack_video_allow(torch.from_numpy(extra).to(DEV))
        got = _search(w, subset=view, video_allow=bits)
        want = _search(w, video_allow=bits & view.allow)
        _assert_same(got, want, members, rows)
    assert (got["top_indices"][0] == -1).all()


def _scratch_index():
    m = _model(torch.bfloat16, 256)
    lens = _lens(33)[:40]
    with torch.no_grad():
        index = MutableCorpusIndex.create(m, 48)
        index.add(*_batch(lens, 8))
    qf, qm = _queries()
    return dict(m=m, index=index, qf=qf, qm=qm, live=np.arange(40)), lens


def test_a_stale_view_raises_and_refresh_follows_the_parent():
    w, lens = _scratch_index()
    index = w["index"]
    members = [2, 3, 5, 8, 13, 21, 34]
    view = inf.video_subset(index, members, n_clips=[int(lens[v]) for v in members])
    before = _clone(_search(w, subset=view))
    v0 = index.version
    with torch.no_grad():
        index.remove([8])
        index.replace([13], *_batch([77], 9))
    assert index.version == v0 + 2 and view.stale
    with pytest.raises(ValueError, match="stale"):
        _search(w, subset=view)
    with pytest.raises(ValueError, match="stale"):
        inf.stage_video_topk(w["m"], index, None, subset=view)
    view.refresh()
    assert not view.stale and view.video_ids.cpu().tolist() == [2, 3, 5, 13, 21, 34]              # the removed member is gone
    got = _search(w, subset=view)
    want = _search(w, video_allow=view.allow)
    _assert_same(got, want, [2, 3, 5, 13, 21, 34])
    assert not (got["top_indices"] == 8).any()
    assert not torch.equal(got["top_scores"], before["top_scores"])                                # the replaced video scores anew
    with pytest.raises(ValueError, match="hold no video"):
        inf.video_subset(index, [2, 8])


def test_compact_leaves_a_view_valid():
    w = _world("mutable-packed")
    index = w["index"]
    members = _members(w, "half")
    view = inf.video_subset(index, members.tolist())
    want = _clone(_search(w, subset=view))
    v0 = index.version
    index.compact()
    assert index.version == v0 and not view.stale
    _assert_same(_search(w, subset=view), want, members)
    _assert_same(_search(w, subset=inf.video_subset(index, members.tolist())), want, members)     # gathered from the moved runs


def test_reset_to_a_set_that_does_not_fit_leaves_the_view():
    w = _world("oneshot-masks")
    view = inf.video_subset(w["index"], [0, 3])                                   # 7 + 7 blocks: one tile
    assert view.n_tiles == 1
    want = _clone(_search(w, subset=view))
    with pytest.raises(ValueError, match="does not fit"):
        view.reset(np.arange(NV).tolist())
    assert view.video_ids.cpu().tolist() == [0, 3] and view.n_videos == 2
    _assert_same(_search(w, subset=view), want, [0, 3])
    view.reset([1, 2, 4])                                                         # ... and one that fits is taken, in place
    assert view.n_tiles == 1 and view.video_ids.cpu().tolist() == [1, 2, 4]
    _assert_same(_search(w, subset=view), _search(w, video_allow=view.allow), [1, 2, 4])


def test_a_captured_search_sees_a_reset_between_replays():
    w = _world("oneshot-bucketed")
    a, b = _members(w, "half"), _members(w, "six")
    view = inf.video_subset(w["index"], a.tolist(), tiles=12)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(w["m"], w["index"], NQ, w["qf"].shape[1], w["qf"].shape[2], subset=view, **KW)
    _assert_same(g(w["qf"], w["qm"]), _search(w, video_allow=view.allow), a, "first set")
    view.reset(b.tolist())
    got = g(w["qf"], w["qm"])
    _assert_same(got, _search(w, video_allow=view.allow), b, "after reset")
    assert np.isin(got["top_indices"].cpu().numpy()[:, :6], b).all() and (got["top_indices"][:, 6:] == -1).all()


def test_a_captured_search_refuses_a_stale_view():
    w, lens = _scratch_index()
    view = inf.video_subset(w["index"], [1, 2, 3, 4], tiles=3)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(w["m"], w["index"], NQ, w["qf"].shape[1], w["qf"].shape[2], subset=view, **KW)
        g(w["qf"], w["qm"])
        w["index"].remove([2])
    with pytest.raises(ValueError, match="stale"):
        g(w["qf"], w["qm"])
    view.refresh()
    _assert_same(g(w["qf"], w["qm"]), _search(w, video_allow=view.allow), [1, 3, 4])


def test_host_to_host_search_through_a_view():
    from tvretrieval_amd.results import MOMENT_DTYPE  # noqa: F401
    w = _world("oneshot-masks")
    members = _members(w, "half")
    view = inf.video_subset(w["index"], members.tolist())
    qf, qm = w["qf"].cpu().pin_memory(), w["qm"].cpu().pin_memory()
    with torch.no_grad():
        rec0, cnt0 = inf.vcmr_search_host(w["m"], w["index"], qf, qm, video_allow=view.allow, **KW)
        rec0, cnt0 = rec0.copy(), cnt0.copy()
        rec1, cnt1 = inf.vcmr_search_host(w["m"], w["index"], qf, qm, subset=view, **KW)
    np.testing.assert_array_equal(cnt1, cnt0)
    live = np.arange(rec0.shape[1])[None] < cnt0[:, None]
    for col in ("vid", "st", "ed", "score"):
        np.testing.assert_array_equal(np.where(live, rec1[col], 0), np.where(live, rec0[col], 0), err_msg=col)
    assert (cnt1 > 0).all() and all(np.isin(rec1["vid"][q, :cnt1[q]], members).all() for q in range(NQ))


@pytest.mark.parametrize("parent", ["oneshot-masks", "oneshot-bucketed", "mutable-packed"])
def test_k6_over_a_view_writes_the_members_columns_only(parent):
    """K6 into a NaN-filled matrix: the members' columns are bitwise the parent's, no other column is written -- and the
    image K6 reads is the view's few tiles, not the parent's."""
    w = _world(parent)
    index, members = w["index"], _members(w, "six")
    view = inf.video_subset(index, members.tolist())
    mods = index.modalities
    assert all(view.k6[m].data.numel() < index.feat1n[m].data.numel() // 4 for m in mods) and view.n_tiles <= 3
    with torch.no_grad():
        vq, sq = w["m"].encode_query(w["qf"], w["qm"])
        outs = []
        for cn in ([view.k6[m] for m in mods], [index.feat1n[m] for m in mods]):
            out = torch.full((NQ, NV), float("nan"), dtype=torch.float32, device=DEV)
            ops.q2c_scores_fused([vq.contiguous(), sq.contiguous()], cn, [index.mask[m] for m in mods], out=out, normalize_q=True)
            outs.append(out)
    sl = torch.as_tensor(members, device=DEV, dtype=torch.long)
    assert torch.equal(outs[0][:, sl].view(torch.int32), outs[1][:, sl].view(torch.int32))
    rest = torch.ones(NV, dtype=torch.bool, device=DEV)
    rest[sl] = False
    assert torch.isnan(outs[0][:, rest]).all() and not torch.isnan(outs[0][:, sl]).any()
