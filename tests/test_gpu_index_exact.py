"""Exact-rank mode on an index that takes updates (MutableCorpusIndex.create(..., exact_rank=True)): after any sequence of
add / replace / remove every operand of a slot is bitwise what the one-shot build_corpus_index(exact_filter=True,
length_buckets=False) leaves for the same slot contents, the running bound e_c_dev is bitwise the maximum of the rounding-error
norms put so far, and a search is bitwise the restricted search over that fixed exact index under the live bits.
Shapes of tests/test_gpu_index_update.py: capacity 70 = three live words, a video_sub model in both exact modes (f32 and
ops.F16S), H = 128 (bf16 filter rows of 256 bytes: the image is row-major; lpad 128 for the f32 model, 112 for the F16S one,
whose lpad follows its f16 rows) and H = 256 (the tiled image), max_ctx_l = 100 and 40 (lpad 48), batch widths 100 / 40, 37
and 24; 20 candidates per query for the 10 best of 70 slots, so the filter really filters."""
import numpy as np
import pytest
import torch

from test_gpu_exact import _lists_equal
from test_gpu_index_update import CAP, _batch, _bits, _live_bool, _mask_words, _queries, _rows
from test_gpu_kernels import DEV
from test_gpu_model import _synthetic_model
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex

pytestmark = pytest.mark.gpu

KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
KW = dict(max_vcmr_video=10, max_before_nms=60)
CASES = [pytest.param(mode, l, h, id="%s-l%d-h%d" % (mode, l, h))
         for mode in ("f32", "f16s") for l, h in ((100, 128), (40, 128), (100, 256))]
_MODELS = {}


def _models(l, h):
    """(the f32 model, the ops.F16S model with the same weights)"""
    from tvretrieval_amd.model_xml import XML
    if (l, h) not in _MODELS:
        m, cfg = _synthetic_model("video_sub", h, 256, 128, 128, l, torch.float32, seed=60)
        mx = XML(cfg, compute_dtype=ops.F16S)
        mx.load_state_dict(m.state_dict())
        _MODELS[l, h] = (m, mx.to(DEV).eval())
    return _MODELS[l, h]


def _model(mode, l, h):
    return _models(l, h)[mode == "f16s"]


def _create(mode, l, h):
    m = _model(mode, l, h)
    index = MutableCorpusIndex.create(m, CAP, exact_rank=True)
    assert index.exact is not None and index.exact.mode == mode == inf.exact_mode_of(m)
    index.exact.n_candidates = 20
    return m, index


def _fixed(m, l, content):
    """The one-shot exact index with position == slot (tests/test_gpu_index_update.py::_fixed with exact_filter=True)."""
    filler = _batch(2, 16, 99)
    runs = []
    for s in range(CAP):
        b, r = content.get(s, (filler, 1))
        if runs and runs[-1][0] is b:
            runs[-1][1].append(r)
        else:
            runs.append((b, [r]))
    with torch.no_grad():
        fixed = inf.build_corpus_index(m, [_rows(b, rows) for b, rows in runs], l_ref=l, n_videos=CAP, length_buckets=False,
                                       exact_filter=True)
    fixed.exact.n_candidates = 20
    return fixed


def _put(index, content, errs, batch, slots):
    """put the whole batch (encoded in one call) into `slots`; record the slot contents and the rounding-error norms the
    one-shot chain computes for the encoder's rows"""
    enc = index.encode(*batch)
    index.put(slots, enc)
    content.update({s: (batch, r) for r, s in enumerate(slots)})
    for m in index.modalities:
        e = ops.round_bf16_rows_err(ops.l2norm_rows(enc[m][0].contiguous()))[1]
        for r, s in enumerate(slots):
            errs[m, s] = e[r]


def _three_batches(index, l):
    content, errs = {}, {}
    _put(index, content, errs, _batch(6, l, 1), [0, 31, 32, 63, 64, 69])
    _put(index, content, errs, _batch(5, 37, 2), [5, 7, 33, 40, 68])
    _put(index, content, errs, _batch(4, 24, 3), [1, 30, 62, 65])
    return content, errs


def _parts(t):
    """the tensors of an f32-grade operand: the rows, or the split rows' halves and scales"""
    return [t.data, t.inv] if isinstance(t, ops.SplitRows) else [t]


def _assert_rows_equal(index, fixed, slots):
    sl = torch.as_tensor(sorted(slots), device=DEV)
    assert index.lpad == fixed.lpad and index.l_ref == fixed.l_ref and index.n_videos == fixed.n_videos == CAP
    assert index.exact.mode == fixed.exact.mode
    for m in index.modalities:
        assert type(index.feat1n[m]) is type(fixed.feat1n[m]), m                    # the same layout of the filter image
        assert index.feat1n[m].dtype == fixed.feat1n[m].dtype == torch.bfloat16
        assert type(index.feat2[m]) is type(fixed.feat2[m]) and type(index.exact.feat1n_f32[m]) is type(fixed.exact.feat1n_f32[m])
        pairs = [("filter", index.feat1n_rows(m), fixed.feat1n_rows(m)), ("mask", index.mask[m], fixed.mask[m])]
        for name, mine, theirs in (("re-score", index.exact.feat1n_f32[m], fixed.exact.feat1n_f32[m]),
                                   ("feat2", index.feat2[m], fixed.feat2[m])):
            pairs += [(name + str(i), a, b) for i, (a, b) in enumerate(zip(_parts(mine), _parts(theirs)))]
        for name, a, b in pairs:
            assert a.dtype == b.dtype and a.shape == b.shape, (m, name)
            assert torch.equal(_bits(a[sl]), _bits(b[sl])), (m, name)
        assert torch.equal(index.mask_bits[m][sl], _mask_words(fixed, m)[sl]), m
        assert torch.equal(_mask_words(index, m), index.mask_bits[m])
    assert torch.equal(index.vlen[sl], fixed.vlen[sl])


def _assert_bound(index, errs, slots_put):
    """err_rows of the slots and the running bound against the one-shot chain's norms, bitwise."""
    for j, m in enumerate(index.modalities):
        top = None
        for s in slots_put:
            e = errs[m, s]
            row = index.exact.err_rows[m][s]
            assert torch.equal(_bits(row[:e.numel()]), _bits(e)) and not bool(row[e.numel():].any()), (m, s)
        for (mm, s), e in errs.items():                       # every row ever put, replaced ones included
            if mm == m:
                top = e.max() if top is None else torch.maximum(top, e.max())
        assert torch.equal(_bits(index.exact.e_c_dev[j:j + 1]), _bits(top.reshape(1))), m


@pytest.mark.parametrize("mode,l,h", CASES)
def test_rows_are_the_builders_rows(mode, l, h):
    m, index = _create(mode, l, h)
    lpad = 48 if l == 40 else 128 if (mode == "f32" or h == 256) else 112
    assert index.l_ref == l and index.lpad == lpad and index.n_videos == CAP and index.n_live == 0
    assert isinstance(index.feat1n["video"], ops.TiledRows) == (h == 256 and l == 100)
    assert isinstance(index.feat2["video"], ops.SplitRows) == (mode == "f16s")
    ex = index.exact
    assert tuple(ex.e_c_dev.shape) == (2,) and ex.e_c_dev.dtype == torch.float32 and not bool(ex.e_c_dev.any())
    assert tuple(ex.err_rows["sub"].shape) == (CAP, lpad) and tuple(ex.feat1n_f32["video"].shape) == (CAP, lpad, h)
    plain = sum(t.numel() * t.element_size() for d in (index.feat1n, index.feat2, index.mask) for t in d.values())
    assert index.hbm_bytes() > plain + sum(t.numel() * 4 for t in ex.feat1n_f32.values()) + 2 * CAP * lpad * 4   # err_rows counted
    content, errs = _three_batches(index, l)
    assert index.n_live == 15 and sorted(content) == index.table.live_slots()
    _assert_rows_equal(index, _fixed(m, l, content), content)
    _assert_bound(index, errs, content)
    assert [ex.e_c[mod] for mod in index.modalities] == ex.e_c_dev.tolist()                   # the diagnostic read-back
    live = _live_bool(index)
    free = torch.as_tensor(np.nonzero(~live)[0], device=DEV)
    for mod in index.modalities:                              # nothing of a slot the puts did not name was written
        assert not index.mask[mod][free].any() and not index.mask_bits[mod][free].any() and not ex.err_rows[mod][free].any()
        for t in _parts(index.feat2[mod]) + _parts(ex.feat1n_f32[mod]) + [index.feat1n_rows(mod)]:
            assert not t[free].any(), mod
    assert (index.vlen[free] == l).all()
    occ = torch.as_tensor(sorted(content), device=DEV)
    assert torch.equal(index.slot_ids[occ], occ.to(torch.int32)) and (index.slot_ids[free] == -1).all()


@pytest.mark.parametrize("mode,l,h", CASES)
def test_a_replace_leaves_nothing_behind(mode, l, h):
    m, index = _create(mode, l, h)
    content, errs = _three_batches(index, l)
    assert int(index.vlen[0]) == l and bool((index.feat1n_rows("video")[0, 24:l] != 0).any())
    short = _batch(2, 24, 4)
    ptrs = [t.data_ptr() for mod in index.modalities for t in _parts(index.feat2[mod]) + _parts(index.exact.feat1n_f32[mod])]
    bound = index.exact.e_c_dev.clone()
    assert index.replace([0, 63], *short) == [0, 63]
    content.update({0: (short, 0), 63: (short, 1)})
    only = MutableCorpusIndex.create(m, CAP, exact_rank=True)                # an index that only ever held the short ones
    only.put([0, 63], only.encode(*short))
    sl = torch.as_tensor([0, 63], device=DEV)
    for mod in index.modalities:
        mine = [index.feat1n_rows(mod), index.mask[mod], index.mask_bits[mod], index.exact.err_rows[mod]] + \
            _parts(index.feat2[mod]) + _parts(index.exact.feat1n_f32[mod])
        theirs = [only.feat1n_rows(mod), only.mask[mod], only.mask_bits[mod], only.exact.err_rows[mod]] + \
            _parts(only.feat2[mod]) + _parts(only.exact.feat1n_f32[mod])
        for a, b in zip(mine, theirs):
            assert torch.equal(_bits(a[sl]), _bits(b[sl])), mod
        for t in (index.feat1n_rows(mod), index.mask[mod], index.exact.err_rows[mod], _parts(index.feat2[mod])[0],
                  _parts(index.exact.feat1n_f32[mod])[0]):
            assert not t[0, 24:].any() and not t[63, 24:].any(), mod
    assert torch.equal(index.vlen[sl], only.vlen[sl]) and int(index.vlen[0]) == 24
    _assert_rows_equal(index, _fixed(m, l, content), content)
    assert bool((index.exact.e_c_dev >= bound).all())                        # a put never lowers the bound
    assert ptrs == [t.data_ptr() for mod in index.modalities for t in _parts(index.feat2[mod]) + _parts(index.exact.feat1n_f32[mod])]


@pytest.mark.parametrize("mode,l,h", [c for c in CASES if c.values[1:] == (100, 128)])
def test_the_bound_is_conservative_after_a_removal_and_tightens(mode, l, h):
    m, index = _create(mode, l, h)
    ex = index.exact
    index.tighten_error_bound()
    assert not bool(ex.e_c_dev.any())                                        # an empty index: 0
    content, errs = _three_batches(index, l)
    _assert_bound(index, errs, content)
    before = ex.e_c_dev.clone()
    worst = int(torch.argmax(ex.err_rows["video"].amax(1)))                  # the slot that holds the video bound
    assert index.table.is_live(worst)
    index.remove([worst])
    assert torch.equal(_bits(ex.e_c_dev), _bits(before))                     # stale, still valid
    assert index.tighten_error_bound() is index
    live = torch.as_tensor(index.table.live_slots(), device=DEV)
    want = torch.stack([ex.err_rows[mod][live].max() for mod in index.modalities])
    assert torch.equal(_bits(ex.e_c_dev), _bits(want)) and float(ex.e_c_dev[0]) < float(before[0])
    # a row with a non-finite element has a NaN norm: err_rows keeps it, the cell goes to +inf (never a NaN, never lower), the
    # other modality's cell follows its own rows; searches then fail every certificate and still return the lists of the
    # finite videos' scores; removing the slot and tightening ends it
    sub_before = ex.e_c_dev[1].clone()
    enc = index.encode(*_batch(2, 24, 4))
    enc["video"][0][1, 3, 5] = float("nan")
    free = [s for s in range(CAP) if not index.table.is_live(s)][:2]
    index.put(free, enc)
    assert float(ex.e_c_dev[0]) == float("inf") and bool(torch.isnan(ex.err_rows["video"][free[1], 3]))
    assert float(ex.e_c_dev[1]) >= float(sub_before) and bool(torch.isfinite(ex.e_c_dev[1]))
    qf, qm = _queries(12)
    bad = torch.zeros(CAP, dtype=torch.bool)
    bad[free[1]] = True
    ok = inf.pack_video_allow((~bad).to(DEV))
    with torch.no_grad():
        hot = inf.vcmr_search(m, index, qf, qm, video_allow=ok, **KW)
    assert int(hot["exact"]["fail"].sum()) == 12 and bool((hot["exact"]["eps"] == float("inf")).all())
    index.remove([free[1]])
    index.tighten_error_bound()
    assert bool(torch.isfinite(ex.e_c_dev).all())
    with torch.no_grad():
        cool = inf.vcmr_search(m, index, qf, qm, **KW)
    assert int(cool["exact"]["fail"].sum()) < 12
    for k in KEYS:
        assert torch.equal(_bits(hot[k]), _bits(cool[k])), k
    index.remove(index.table.live_slots())
    index.tighten_error_bound()
    assert not bool(ex.e_c_dev.any())


def _sequence(mode, l, h):
    """add 60, remove 7, replace 5, add 4 into freed slots, put 3 at the far end -> (model, index, the fixed exact index that
    still holds the removed videos 32, 45 and 59, live bools)."""
    m, index = _create(mode, l, h)
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
    far = _batch(3, 37, 16)
    index.put([63, 64, 69], index.encode(*far))
    content.update({s: (far, r) for r, s in enumerate([63, 64, 69])})
    assert index.n_live == 60
    live = _live_bool(index)
    assert not live[[32, 45, 59]].any() and not live[60:63].any() and live[[0, 31, 63, 64, 69]].all()
    return m, index, _fixed(m, l, content), live, content


def _ulps(a, b):
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


@pytest.mark.parametrize("mode,l,h", CASES)
def test_search_equals_the_restricted_search_on_the_fixed_exact_index(mode, l, h):
    m, index, fixed, live, content = _sequence(mode, l, h)
    _assert_rows_equal(index, fixed, np.nonzero(live)[0].tolist())
    qf, qm = _queries(12)
    gt = torch.as_tensor(np.nonzero(live)[0][[0, 5, 9, 14, 20, 27, 33, 41, 48, 52, 57, 59]], dtype=torch.int32, device=DEV)
    kw = dict(KW, svmr_video=gt)
    allow = inf.pack_video_allow(torch.from_numpy(live[None]).to(DEV))
    keys = KEYS + ("svmr_scores", "svmr_flat")

    def both():
        with torch.no_grad():
            return inf.vcmr_search(m, index, qf, qm, **kw), inf.vcmr_search(m, fixed, qf, qm, video_allow=allow, **kw)
    # 1. each index under its own bound: the lists do not depend on what the certificates decided
    got, want = both()
    for k in keys:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    ti = got["top_indices"].cpu().numpy()
    assert (ti >= 0).all() and live[ti].all()
    assert int(got["exact"]["n_candidates"]) == 20 and got["exact"]["q2c_filter"].shape == (12, CAP)
    # 2. the fixed index under the running bound: the same certificate decisions
    cells = index.exact.e_c_dev.tolist()
    fixed.exact.e_c = dict(zip(index.modalities, cells))
    got, want = both()
    for k in keys:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    gi, wi = got["exact"], want["exact"]
    worst = int(_ulps(gi["eps"], wi["eps"]).max())
    n_pass = int((gi["fail"] == 0).sum())
    print("%s l%d h%d: eps %d ulp apart at most, %d of 12 queries pass their certificate; bound %s"
          % (mode, l, h, worst, n_pass, cells))
    assert torch.equal(gi["fail"], wi["fail"]) and worst <= 2
    assert n_pass >= 1, "no query passes its certificate: the test shows nothing about the first tier"
    # 3. every certificate forced to fail: the second tier re-scores with the same kernel, the lists are bitwise the same
    first = {k: got[k].clone() for k in keys}
    kept = index.exact.e_c_dev.clone()
    index.exact.e_c_dev.fill_(10.0)
    with torch.no_grad():
        forced = inf.vcmr_search(m, index, qf, qm, **kw)
    assert int(forced["exact"]["fail"].sum()) == 12 and forced["exact"]["n_full_rows"] == 0
    for k in keys:
        assert torch.equal(_bits(forced[k]), _bits(first[k])), k
    # 4. a cell at +inf (what a NaN norm leaves there): eps = +inf in BOTH modes, every video re-scored, the same lists --
    # first either cell alone, then both
    for hot in ([float("inf"), cells[1]], [cells[0], float("inf")], [float("inf")] * 2):
        index.exact.e_c_dev.copy_(torch.tensor(hot, device=DEV))
        with torch.no_grad():
            forced = inf.vcmr_search(m, index, qf, qm, **kw)
        assert int(forced["exact"]["fail"].sum()) == 12 and bool((forced["exact"]["eps"] == float("inf")).all()), hot
        for k in keys:
            assert torch.equal(_bits(forced[k]), _bits(first[k])), (k, hot)
    index.exact.e_c_dev.copy_(kept)
    # a removed video would rank on the fixed index without the mask: the live words really restrict
    with torch.no_grad():
        free = inf.vcmr_search(m, fixed, qf, qm, **KW)
    assert np.isin(free["top_indices"].cpu().numpy(), [32, 45, 59]).any(), "no removed video ranks: the test shows nothing"


@pytest.mark.parametrize("mode,l,h", [c for c in CASES if c.values[1:] == (100, 256)])
def test_the_other_entry_points_take_the_index(mode, l, h):
    """vcmr_search_host and explain_moments accept a mutable index and an exact one: on the mutable exact index they give
    what they give on the fixed exact index under the live words."""
    m, index, fixed, live, content = _sequence(mode, l, h)
    qf, qm = _queries(12)
    allow = inf.pack_video_allow(torch.from_numpy(live[None]).to(DEV))
    kw = dict(max_vcmr_video=10, max_before_nms=40)
    with torch.no_grad():
        rec, cnt = inf.vcmr_search_host(m, index, query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory(), **kw)
        rec, cnt = rec.copy(), cnt.copy()
        wrec, wcnt = inf.vcmr_search_host(m, fixed, query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory(),
                                          video_allow=allow, **kw)
    assert (cnt > 0).all() and (cnt == wcnt).all()
    for q in range(12):
        assert rec[q, :cnt[q]].tobytes() == wrec[q, :wcnt[q]].tobytes(), q          # slot == position, ids == slots
    with torch.no_grad():
        top = inf.vcmr_search(m, index, qf, qm, **kw)["top_indices"][:, 0].tolist()
        ev = inf.explain_moments(m, index, qf, qm, list(range(12)), top)
        wev = inf.explain_moments(m, fixed, qf, qm, list(range(12)), top)
    assert set(ev) == set(wev)
    for k in ev:
        if torch.is_tensor(ev[k]):
            assert torch.equal(_bits(ev[k]), _bits(wev[k])), k


@pytest.mark.parametrize("mode,l,h", CASES)
def test_lists_are_the_plain_f32_paths(mode, l, h):
    """The mutable exact index against a plain f32 MutableCorpusIndex of the same videos, tie-aware at the tolerances of
    tests/test_gpu_exact.py::test_exact_mode_equals_f32_path (2e-5 on weights, 5e-5 on moments)."""
    m, index, fixed, live, content = _sequence(mode, l, h)
    m32 = _models(l, h)[0]
    plain = MutableCorpusIndex.create(m32, CAP)
    by_batch = {}
    for s, (b, r) in sorted(content.items()):
        if live[s]:
            by_batch.setdefault(id(b), (b, [], []))
            by_batch[id(b)][1].append(r), by_batch[id(b)][2].append(s)
    for b, rows, slots in by_batch.values():
        plain.put(slots, plain.encode(*_rows(b, rows)))
    assert plain.table.live_slots() == index.table.live_slots()
    qf, qm = _queries(12)
    with torch.no_grad():
        out = inf.vcmr_search(m, index, qf, qm, **KW)
        ref = inf.vcmr_search(m32, plain, qf, qm, **KW)
    ref = dict(ref)
    ref["q2c"] = ref["q2c"].masked_fill(~torch.from_numpy(live).to(DEV)[None], float("-inf"))     # free slots hold no video
    n_v, n_m, n_same = _lists_equal(out, ref, l, 10, 60, "mutable exact (%s) vs plain f32" % mode)
    print("%s l%d h%d: %d video / %d moment positions swapped in f32 ties, %d of 12 queries with identical video lists"
          % (mode, l, h, n_v, n_m, n_same))
    assert n_same >= 10


@pytest.mark.parametrize("l,h", [(100, 128), (100, 256)])
def test_a_captured_search_survives_updates(l, h):
    """Mode f16s only (the f32 mode reads its certificate on the host): one capture, replays after an add, a remove and
    tighten_error_bound() equal the eager searches bitwise -- the graph reads the live words AND the bound when it runs."""
    m, index = _create("f16s", l, h)
    src = _batch(40, l, 21)
    assert index.add(*src) == list(range(40))
    qf, qm = _queries(8)
    with pytest.raises(ValueError, match="not capturable"):
        inf.GraphedVcmrSearch(_models(l, h)[0], _create("f32", l, h)[1], 8, qf.shape[1], qf.shape[2], **KW)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(m, index, 8, qf.shape[1], qf.shape[2], **KW)

    def same_as_eager(out):
        with torch.no_grad():
            eager = inf.vcmr_search(m, index, qf, qm, **KW)
        for k in KEYS:
            assert torch.equal(_bits(out[k]), _bits(eager[k])), k
        assert torch.equal(out["exact"]["fail"], eager["exact"]["fail"])
        assert torch.equal(_bits(out["exact"]["eps"]), _bits(eager["exact"]["eps"]))
        return {k: out[k].clone() for k in KEYS}, out["exact"]["eps"].clone()
    first, eps0 = same_as_eager(g(qf, qm))
    # copies of the three best videos of query 0 score what their originals score: they rank right behind them; a wider
    # batch of other videos raises the bound
    t0 = [int(s) for s in first["top_indices"][0, :3].tolist()]
    assert index.add(*_rows(src, t0)) == [40, 41, 42]
    index.add(*_batch(6, l, 1))
    second, eps1 = same_as_eager(g(qf, qm))                                  # no re-capture
    assert np.isin([40, 41, 42], second["top_indices"][0].cpu().numpy()).all()
    assert bool((eps1 >= eps0).all())
    # the best video of query 1, and every slot that holds the video bound (a copy added above holds its original's norms)
    row_max = index.exact.err_rows["video"].amax(1)
    gone = sorted(set([int(first["top_indices"][1, 0])] + torch.nonzero(row_max == row_max.max()).reshape(-1).tolist()))
    index.remove(gone)
    third, eps2 = same_as_eager(g(qf, qm))
    assert not np.isin(third["top_indices"].cpu().numpy(), gone).any() and torch.equal(_bits(eps2), _bits(eps1))
    stale = index.exact.e_c_dev.clone()
    index.tighten_error_bound()
    assert float(index.exact.e_c_dev[0]) < float(stale[0])                   # the slot that held the video bound is gone
    fourth, eps3 = same_as_eager(g(qf, qm))
    assert bool((eps3 <= eps2).all())                                        # (the next norm is close: eps may round alike)
    # the replay reads the cells when it runs: a bound nobody could miss fails every certificate of the same graph
    index.exact.e_c_dev.fill_(10.0)
    out = g(qf, qm)
    assert int(out["exact"]["fail"].sum()) == 8 and bool((out["exact"]["eps"] > 10.0).all())
    fifth, _ = same_as_eager(out)
    for k in KEYS:                                                           # a bound changes certificates, never lists
        assert torch.equal(_bits(fourth[k]), _bits(third[k])) and torch.equal(_bits(fifth[k]), _bits(third[k])), k
