"""An index that takes updates (index_update.MutableCorpusIndex): after any sequence of add / replace / remove its rows are
bitwise the rows a one-shot build_corpus_index(length_buckets=False) leaves for the same slot contents, and a search on it
is bitwise the restricted search over that fixed index under the live bits.  video_sub model, H = 128, f32 and bf16,
max_ctx_l = 100 (f32: lpad 128 and the tiled K6 operand; bf16 rows of H = 128 are 256 bytes, below the 384 the tiled kernel
takes, so that index is row-major at lpad 112 -- a bf16 case at H = 256 covers the tiled bf16 operand) and max_ctx_l = 40
(lpad 48, row-major); capacity 70 = three live words."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex

pytestmark = pytest.mark.gpu

CAP = 70
KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
CASES = [pytest.param(dt, l, h, id="%s-l%d-h%d" % (str(dt).split(".")[1], l, h))
         for dt, l, h in [(dt, l, 128) for dt in (torch.float32, torch.bfloat16) for l in (100, 40)] + [(torch.bfloat16, 100, 256)]]
KW = dict(max_vcmr_video=10, max_before_nms=60)
_MODELS, _BATCHES = {}, {}


def _model(dtype, l, h):
    if (dtype, l, h) not in _MODELS:
        _MODELS[dtype, l, h] = _synthetic_model("video_sub", h, 256, 128, 128, l, dtype, seed=60)[0]
    return _MODELS[dtype, l, h]


def _batch(n, width, seed):
    """A context batch of n videos padded to `width` clips (video 0 has the full width), on the device; built once."""
    if (n, width, seed) not in _BATCHES:
        lens = np.random.default_rng(seed).integers(6, width + 1, n)
        lens[0] = width
        vf, vm = _feats(n, lens, 256, 2 * seed + 1)
        sf, sm = _feats(n, lens, 128, 2 * seed + 2)
        _BATCHES[n, width, seed] = tuple(t.to(DEV) for t in (vf, vm, sf, sm))
    return _BATCHES[n, width, seed]


def _rows(batch, rows):
    idx = torch.as_tensor(list(rows), device=DEV)
    return tuple(t.index_select(0, idx).contiguous() for t in batch)


def _queries(nq, seed=5):
    qf, qm = _feats(nq, np.concatenate([[30], np.random.default_rng(seed).integers(3, 31, nq - 1)]), 128, seed)
    return qf.to(DEV), qm.to(DEV)


def _fixed(m, l, content):
    """The immutable index with position == slot: content[slot] = (batch, row); a run of consecutive slots from one batch is
    one builder batch at that batch's padded width (the encoder's rows do not depend on the batch size); slots without
    content get a filler video."""
    filler = _batch(2, 16, 99)
    runs = []
    for s in range(CAP):
        b, r = content.get(s, (filler, 1))
        if runs and runs[-1][0] is b:
            runs[-1][1].append(r)
        else:
            runs.append((b, [r]))
    with torch.no_grad():
        return inf.build_corpus_index(m, [_rows(b, rows) for b, rows in runs], l_ref=l, n_videos=CAP, length_buckets=False)


def _put(index, content, batch, slots):
    """put the whole batch (encoded in one call) into `slots` and record the slot contents"""
    index.put(slots, index.encode(*batch))
    content.update({s: (batch, r) for r, s in enumerate(slots)})


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _mask_words(index, m):
    """(n_videos, 4) mask-bit words: the builder's own where it makes them (tiled operand), else packed from its mask."""
    t = index.feat1n[m]
    if hasattr(t, "mask_bits") and t.mask_bits is not None:
        return t.mask_bits
    wide = torch.zeros((index.n_videos, 128), dtype=torch.bool, device=DEV)
    wide[:, :index.lpad] = index.mask[m] != 0
    return ops._pack_bits32(wide)


def _live_bool(index):
    live = np.zeros(CAP, dtype=bool)
    live[index.table.live_slots()] = True
    words = index.live.cpu().numpy().view(np.uint32)[0]
    assert [(int(words[s >> 5]) >> (s & 31)) & 1 for s in range(CAP)] == live.astype(int).tolist()      # device == host table
    return live


def _assert_rows_equal(index, fixed, slots):
    sl = torch.as_tensor(sorted(slots), device=DEV)
    assert index.lpad == fixed.lpad and index.l_ref == fixed.l_ref and index.n_videos == fixed.n_videos == CAP
    for m in index.modalities:
        assert type(index.feat1n[m]) is type(fixed.feat1n[m]), m                    # the same K6 layout
        for name, a, b in (("feat1n", index.feat1n_rows(m), fixed.feat1n_rows(m)), ("feat2", index.feat2[m], fixed.feat2[m]),
                           ("mask", index.mask[m], fixed.mask[m])):
            assert a.dtype == b.dtype and a.shape == b.shape, (m, name)
            assert torch.equal(_bits(a[sl]), _bits(b[sl])), (m, name)
        assert torch.equal(index.mask_bits[m][sl], _mask_words(fixed, m)[sl]), m
        assert torch.equal(_mask_words(index, m), index.mask_bits[m])
    assert torch.equal(index.vlen[sl], fixed.vlen[sl])
    assert index.vlen.dtype == fixed.vlen.dtype == torch.int32


def _three_batches(index, l):
    content = {}
    _put(index, content, _batch(6, l, 1), [0, 31, 32, 63, 64, 69])
    _put(index, content, _batch(5, 37, 2), [5, 7, 33, 40, 68])
    _put(index, content, _batch(4, 24, 3), [1, 30, 62, 65])
    return content


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_rows_are_the_builders_rows(dtype, l, h):
    m = _model(dtype, l, h)
    index = MutableCorpusIndex.create(m, CAP)
    tiled = l == 100 and h * (4 if dtype == torch.float32 else 2) >= 384
    assert index.l_ref == l and index.lpad == (48 if l == 40 else 128 if tiled else 112) and index.n_videos == CAP
    assert isinstance(index.feat1n["video"], ops.TiledRows) == tiled and index.n_live == 0
    assert tuple(index.live.shape) == (1, 3) and index.live.dtype == torch.int32 and index.ragged
    content = _three_batches(index, l)
    assert index.n_live == 15 and sorted(content) == index.table.live_slots()
    _assert_rows_equal(index, _fixed(m, l, content), content)
    live = _live_bool(index)
    free = torch.as_tensor(np.nonzero(~live)[0], device=DEV)
    for mod in index.modalities:
        assert not index.mask[mod][free].any() and not index.mask_bits[mod][free].any()
    assert (index.vlen[free] == l).all()
    occ = torch.as_tensor(sorted(content), device=DEV)
    assert torch.equal(index.slot_ids[occ], occ.to(torch.int32)) and (index.slot_ids[free] == -1).all()
    assert index.hbm_bytes() > sum(t.numel() * t.element_size() for t in index.feat2.values())


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_a_replace_leaves_nothing_behind(dtype, l, h):
    m = _model(dtype, l, h)
    index = MutableCorpusIndex.create(m, CAP)
    content = _three_batches(index, l)
    full = _batch(6, l, 1)
    assert int(full[1][0].sum()) == l and int(index.vlen[0]) == l            # slot 0 holds a full-length video
    assert bool((index.feat1n_rows("video")[0, 24:l] != 0).any())
    short = _batch(2, 24, 4)
    ptrs = [index.feat2[mod].data_ptr() for mod in index.modalities] + [index.live.data_ptr(), index.vlen.data_ptr()]
    assert index.replace([0, 63], *short) == [0, 63]
    content.update({0: (short, 0), 63: (short, 1)})
    assert index.n_live == 15
    for mod in index.modalities:
        for t in (index.feat1n_rows(mod), index.feat2[mod], index.mask[mod]):
            assert not t[0, 24:].any() and not t[63, 24:].any(), mod
        assert bool(index.feat2[mod][0, :24].any())
    assert int(index.vlen[0]) == 24
    _assert_rows_equal(index, _fixed(m, l, content), content)
    assert ptrs == [index.feat2[mod].data_ptr() for mod in index.modalities] + [index.live.data_ptr(), index.vlen.data_ptr()]


def _sequence(m, l):
    """add 60, remove 7, replace 5, add 4 into freed slots, put 3 at the far end -> (index, fixed index F that still holds the
    removed videos 32, 45 and 59, live bools)."""
    index = MutableCorpusIndex.create(m, CAP)
    content = {}
    for seed, width in ((11, l), (12, 37), (13, 24)):
        b = _batch(20, width, seed)
        slots = index.add(*b)
        content.update({s: (b, r) for r, s in enumerate(slots)})
    assert sorted(content) == list(range(60))
    assert index.remove([3, 20, 21, 31, 32, 45, 59]) == [3, 20, 21, 31, 32, 45, 59]
    rb = _batch(5, 30, 14)
    index.replace([0, 10, 25, 40, 58], *rb)
    content.update({s: (rb, r) for r, s in enumerate([0, 10, 25, 40, 58])})
    nb = _batch(4, l, 15)
    slots = index.add(*nb)
    assert slots == [3, 20, 21, 31]                                     # lowest free first
    content.update({s: (nb, r) for r, s in enumerate(slots)})
    _put(index, content, _batch(3, 37, 16), [63, 64, 69])
    assert index.n_live == 60
    live = _live_bool(index)
    assert not live[[32, 45, 59]].any() and not live[60:63].any() and live[[0, 31, 63, 64, 69]].all()
    return index, _fixed(m, l, content), live, content


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_search_equals_the_restricted_search_on_the_fixed_index(dtype, l, h):
    m = _model(dtype, l, h)
    index, fixed, live, content = _sequence(m, l)
    _assert_rows_equal(index, fixed, np.nonzero(live)[0].tolist())
    qf, qm = _queries(12)
    kw = dict(KW, nms_thd=0.5, max_after_nms=20)
    caller = np.random.default_rng(7).random((12, CAP)) < 0.6
    for name, mine, theirs in (("live alone", None, live[None]), ("caller mask", caller, caller & live[None])):
        akw = {} if mine is None else dict(video_allow=inf.pack_video_allow(torch.from_numpy(mine).to(DEV)))
        with torch.no_grad():
            got = inf.vcmr_search(m, index, qf, qm, **kw, **akw)
            want = inf.vcmr_search(m, fixed, qf, qm, video_allow=inf.pack_video_allow(torch.from_numpy(theirs).to(DEV)), **kw)
        for k in KEYS + ("records", "record_count", "nms_records", "nms_count"):
            assert torch.equal(_bits(got[k]), _bits(want[k])), (name, k)
        ti = got["top_indices"].cpu().numpy()
        assert (ti >= 0).all() and live[ti].all(), name                 # K = 10 <= the allowed live videos of every query
    with torch.no_grad():
        free = inf.vcmr_search(m, fixed, qf, qm, **kw)
    assert np.isin(free["top_indices"].cpu().numpy(), [32, 45, 59]).any(), "no removed video ranks: the test shows nothing"
    # explain_moments takes slot numbers: its q2c entry is the search's score of that (query, slot)
    with torch.no_grad():
        ev = inf.explain_moments(m, index, qf, qm, [0, 1], [int(ti[0, 0]), int(ti[1, 0])])
    assert torch.equal(ev["ctx_len"].cpu(), index.vlen[torch.as_tensor([int(ti[0, 0]), int(ti[1, 0])], device=DEV)].cpu())


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_fewer_live_videos_than_k(dtype, l, h):
    m = _model(dtype, l, h)
    index = MutableCorpusIndex.create(m, CAP)
    b = _batch(20, 37, 12)
    index.put([0, 31, 32, 63, 64, 69], index.encode(*_rows(b, range(6))))
    qf, qm = _queries(12)
    for n_live, gone in ((6, []), (4, [31, 64])):
        if gone:
            index.remove(gone)
        live = _live_bool(index)
        assert int(live.sum()) == n_live == index.n_live
        with torch.no_grad():
            got = inf.vcmr_search(m, index, qf, qm, **KW)
        ti, tw = got["top_indices"].cpu().numpy(), got["top_scores"].cpu().numpy()
        fi = got["flat_indices"].cpu().numpy()
        assert (ti[:, n_live:] == -1).all() and (tw[:, n_live:] == 0).all()
        assert (np.sort(ti[:, :n_live], axis=1) == np.nonzero(live)[0][None]).all()
        assert (fi >= 0).any(1).all()
        for q in range(12):
            r = fi[q][fi[q] >= 0] // (l * l)
            assert (r < n_live).all(), "query %d: a moment decodes to an empty video slot" % q


def test_against_the_oracle_on_the_sub_corpus():
    """test_restricted_pass_against_the_oracle_on_the_sub_corpus on world "big" with the live set in place of the caller's
    mask: the whole corpus is added, everything outside `sel` removed.  The result is bitwise the restricted pass, so that
    test's tolerances and its 0.8 of the queries with identical video lists are inherited."""
    from oracle import xml_oracle as O
    from oracle.listcmp import moment_keys, tie_aware_equal
    from test_gpu_restricted_search import _search, _world
    w = _world("big")
    allowed = np.random.default_rng(11).random((1, w["nv"])) < 0.5
    allowed[0, 0] = True
    sel = np.nonzero(allowed[0])[0]
    kv, l, n_mom = w["kv"], w["l"], 60
    assert len(sel) >= kv + 6
    index = MutableCorpusIndex.create(w["m"], w["nv"])
    assert index.add(w["vf"].to(DEV), w["vm"].to(DEV), w["sf"].to(DEV), w["sm"].to(DEV)) == list(range(w["nv"]))
    index.remove(np.nonzero(~allowed[0])[0])
    assert index.n_live == len(sel) and index.l_ref == l
    with torch.no_grad():
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], **w["kw"])
    same_as = _search(w, allowed)
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(same_as[k])), k
    om = O.OracleXML(w["cfg"], {k: v.detach().cpu() for k, v in w["m"].state_dict().items()})
    with torch.no_grad():
        v1, v2, s1, s2 = om.encode_context(w["vf"][sel], w["vm"][sel], w["sf"][sel], w["sm"][sel])
        q2c, st, ed = om.get_pred_from_raw_query(w["qf_cpu"], w["qm_cpu"], v1, v2, w["vm"][sel], s1, s2, w["sm"][sel], cross=True)
        want = O.vcmr_tail(q2c, st, ed, 20.0, kv, 2, 16, n_mom + 16)
    gi = got["top_indices"].cpu().numpy()
    assert np.isin(gi, sel).all()
    ww, wi2 = torch.topk(torch.exp(20.0 * q2c), kv + 6, dim=1)
    tie_aware_equal(gi, got["top_scores"].cpu().numpy(), sel[wi2.numpy()], ww.numpy(), kv, 4e-3, "live videos")
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
                            "moments of query %d on the live videos" % q)
    assert len(same) >= 0.8 * w["nq"]


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_a_captured_search_survives_updates(dtype, l, h):
    m = _model(dtype, l, h)
    index = MutableCorpusIndex.create(m, CAP)
    src = _batch(40, l, 21)
    assert index.add(*src) == list(range(40))
    qf, qm = _queries(8)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(m, index, 8, qf.shape[1], qf.shape[2], **KW)
    out = g(qf, qm)
    first = {k: out[k].clone() for k in KEYS}
    with torch.no_grad():
        eager = inf.vcmr_search(m, index, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(first[k]), _bits(eager[k])), k
    # copies of the three best videos of query 0 score what their originals score: they rank right behind them
    t0 = [int(s) for s in first["top_indices"][0, :3].tolist()]
    new = index.add(*_rows(src, t0))
    assert new == [40, 41, 42]
    gone = [int(first["top_indices"][1, 0]), int(first["top_indices"][2, 1])]
    if gone[0] == gone[1]:
        gone[1] = int(first["top_indices"][2, 0])
    index.remove(gone)
    second = g(qf, qm)                                                   # no re-capture
    with torch.no_grad():
        eager = inf.vcmr_search(m, index, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(second[k]), _bits(eager[k])), k
    ti = second["top_indices"].cpu().numpy()
    assert not np.isin(ti, gone).any() and np.isin(new, ti[0]).all()
    assert not torch.equal(second["top_indices"], first["top_indices"])


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_host_to_host_records_carry_the_callers_ids(dtype, l, h):
    m = _model(dtype, l, h)
    b = _batch(20, 37, 12)
    ids = [1000 + 7 * i for i in range(20)]
    index = MutableCorpusIndex.from_batches(m, [b], CAP, ids=ids)
    assert index.slot_of(1000 + 7 * 4) == 4 and index.n_live == 20
    index.remove(ids=[1000 + 7 * 4, 1000 + 7 * 9])
    index.add(*_rows(b, [4]), ids=[5555])                                # into slot 4, under a new id
    assert index.slot_of(5555) == 4
    id_of = index.slot_ids.cpu().numpy()
    qf, qm = _queries(12)
    kw = dict(max_vcmr_video=10, max_before_nms=40)
    with torch.no_grad():
        one = inf.vcmr_search(m, index, qf, qm, **kw)
        rec, cnt = inf.vcmr_search_host(m, index, query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory(), **kw)
    ti, fi = one["top_indices"].cpu().numpy(), one["flat_indices"].cpu().numpy()
    assert (cnt > 0).all()
    for q in range(12):
        n = int(cnt[q])
        assert n == int((fi[q] >= 0).sum())
        assert rec["vid"][q, :n].tolist() == id_of[ti[q, fi[q, :n] // (l * l)]].tolist(), q
    seen = set(np.concatenate([rec["vid"][q, :cnt[q]] for q in range(12)]).tolist())
    assert seen <= (set(ids) | {5555}) - {1000 + 7 * 4, 1000 + 7 * 9} and 5555 in seen


@pytest.mark.parametrize("dtype,l,h", CASES)
def test_refusals_leave_the_index_unchanged(dtype, l, h):
    from tvretrieval_amd import dist
    from tvretrieval_amd.model_xml import XML
    m = _model(dtype, l, h)
    index = MutableCorpusIndex.create(m, CAP)
    for seed, width in ((11, l), (12, 37), (13, 24)):
        index.add(*_batch(20, width, seed), ids=[100 * seed + i for i in range(20)])
    index.remove([7, 33])
    two = _batch(2, 24, 4)
    enc = index.encode(*two)
    torch.cuda.synchronize()
    before = (index.live.clone(), index.vlen.clone(), index.slot_ids.clone(), index.n_live, index.table.live_slots())
    wide = tuple(torch.cat([t, t], 1)[:, :l + 1].contiguous() for t in _batch(2, l, 5))
    f16s = XML(dict(m.config), compute_dtype=ops.F16S)
    for call, match in ((lambda: MutableCorpusIndex.create(f16s, CAP), "exact-rank"),
                        (lambda: MutableCorpusIndex.create(m, CAP, exact_filter=True), "exact-rank"),
                        (lambda: MutableCorpusIndex.create(m, CAP, parts=object()), "parts"),
                        (lambda: MutableCorpusIndex.create(m, CAP, video_offset=CAP), "shard"),
                        (lambda: dist.check_shards(index), "shard"),
                        (lambda: index.put([3, CAP], enc), "outside"),
                        (lambda: index.put([3, 3], enc), "duplicate slots"),
                        (lambda: index.replace([5, 5], *two), "duplicate slots"),
                        (lambda: index.add(*_batch(20, 37, 12)), "full"),
                        (lambda: index.replace([7, 8], *two), "free"),
                        (lambda: index.replace(None, *two, ids=[1100, 4242]), "unknown video id"),
                        (lambda: index.remove([33]), "free"),
                        (lambda: index.remove([64]), "free"),
                        (lambda: index.remove(ids=[1213]), "unknown video id"),
                        (lambda: index.remove([CAP]), "outside"),
                        (lambda: index.add(*two, ids=[1100, 1]), "already held"),
                        (lambda: index.add(*wide), "l_ref"),
                        (lambda: index.replace([1], *two), "slots for a batch"),
                        (lambda: inf.vcmr_search(m, index, *_queries(8), pad_tail=True, **KW), "pad_tail")):
        with pytest.raises(ValueError, match=match):
            call()
        after = (index.live, index.vlen, index.slot_ids, index.n_live, index.table.live_slots())
        assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(before, after)), match
    assert index.n_live == 58 and index.slot_of(1100) == 0
