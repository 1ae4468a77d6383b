"""The ingest launches with the temporal endpoint columns (include/xmlhip_ingest_tef.h; ContextFeeder(ctx_mode=*_tef)) on the GPU.
  1. xml_ingest_rows_tef: the feature columns and the mask are bitwise xml_ingest_rows', the endpoint columns bitwise the
     float32 restatement (tests/ingest_tef_ref.py), rows behind a video's length zero -- at every row width that changes the
     kernel's path or puts the two columns at a 512-column boundary;
  2. xml_ingest_pool_rows_tef: the same against xml_ingest_pool_rows;
  3. tef_pos / tef_len: the columns of every part of a 75-clip video are the unsplit video's at those clips; values that
     cannot hold the item fall back to the item's own axis; half a place is refused;
  4. ContextFeeder(ctx_mode=) against the fixture made by the reference's StartEndEvalDataset (eval_collate_tef.npz);
  5. end to end: an index built from the feeder's batches is bitwise the index built from today's batches with host-made
     columns, and the searches agree;
  6. long videos: parts carry whole-video time through build_corpus_index(parts=) and MutableCorpusIndex chains.
  7. compute_context_info over StoreEvalDataset(ctx_mode=) encodes what the feeder's index holds.
All kernel comparisons are bitwise."""
import numpy as np
import pytest
import torch

import ingest_tef_ref as REF
from test_gpu_kernels import DEV

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(_bits(got), _bits(want)), "%s: %d elements differ bitwise" % (what, int((_bits(got) != _bits(want)).sum()))


def _want_tef(lens, lmax, max_len, dst_dt, pos=None, tot=None):
    w = REF.restate_tef(lens, lmax, max_len, pos, tot)
    return REF.to_bf16(w) if dst_dt is BF16 else torch.from_numpy(w)


def _check_rows_zero(feat, lens, max_len):
    for i, n in enumerate(lens):
        assert bool((_bits(feat[i, min(n, max_len):]) == 0).all()), i


# ---------------------------------------------------------------------------------------------------------
# 1. xml_ingest_rows_tef
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dst_dt", [F32, BF16], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src_dt", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("d", [6, 64, 72, 510, 512])
def test_rows_tef_kernel_sweep(d, src_dt, dst_dt, normalize):
    from tvretrieval_amd import ops
    c = REF.rows_case(d, src_dt)
    assert c["n"] == 5 and c["lmax"] == 33 and (c["n"] * c["lmax"]) % 4 != 0 and max(c["lens"]) > c["max_len"]
    src, rs = c["src"].to(DEV), c["row_start"].to(DEV)
    args = (src, rs, c["n"], c["lmax"], c["max_len"])
    old, old_mask = ops.ingest_rows(*args, normalize=bool(normalize), out_dtype=dst_dt)
    new, mask = ops.ingest_rows(*args, normalize=bool(normalize), out_dtype=dst_dt, tef=True)
    torch.cuda.synchronize()
    assert new.shape == (5, 33, d + 2) and new.dtype == dst_dt
    _same(new[:, :, :d], old, "feature columns")
    _same(mask, old_mask, "mask")
    _same(new[:, :, d:], _want_tef(c["lens"], c["lmax"], c["max_len"], dst_dt), "endpoint columns")
    _check_rows_zero(new, c["lens"], c["max_len"])
    if dst_dt is F32:       # and the whole contract in float32 numpy (the sum of squares is ordered differently there)
        want, wmask = REF.restate_rows(c["src"].float().numpy(), c["row_start"].numpy(), c["lmax"], c["max_len"], normalize)
        np.testing.assert_array_equal(mask.cpu().numpy(), wmask)
        np.testing.assert_allclose(new.cpu().numpy(), want, rtol=2e-6, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------
# 2. xml_ingest_pool_rows_tef
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("dst_dt", [F32, BF16], ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("dims", [(16, 8), (504, 8), (12, 6)], ids=lambda v: "%dx%d" % v)
def test_pool_rows_tef_kernel_sweep(dims, dst_dt, n_src, pool):
    from tvretrieval_amd import ops
    d_a, d_b = dims if n_src == 2 else (dims[0] + dims[1], 0)
    c = REF.pool_case(d_a, d_b, F16)
    D = d_a + d_b
    sources = [(s.to(DEV), g.to(DEV), k == 0) for k, (s, g) in enumerate(zip(c["srcs"], c["segs"]))]
    assert all(int(g[5, 0]) == int(g[5, 1]) for g in c["segs"])                    # the clip with an empty range
    args = (sources, c["row_start"].to(DEV), c["n"], c["lmax"], c["max_len"])
    old, old_mask, old_filled = ops.ingest_pool_rows(*args, pool=pool, normalize=True, out_dtype=dst_dt, want_filled=True)
    new, mask, filled = ops.ingest_pool_rows(*args, pool=pool, normalize=True, out_dtype=dst_dt, want_filled=True, tef=True)
    torch.cuda.synchronize()
    assert new.shape == (5, 33, D + 2) and new.dtype == dst_dt
    _same(new[:, :, :D], old, "feature columns")
    _same(mask, old_mask, "mask")
    _same(filled, old_filled, "filled")
    assert float(filled[1, 4]) == 0.0 and float(mask[1, 4]) == 1.0                 # clip row 5 = video 1, clip 4
    _same(new[:, :, D:], _want_tef(c["lens"], c["lmax"], c["max_len"], dst_dt), "endpoint columns")
    _check_rows_zero(new, c["lens"], c["max_len"])


# ---------------------------------------------------------------------------------------------------------
# 3. tef_pos / tef_len
# ---------------------------------------------------------------------------------------------------------
def _i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


def test_parts_carry_the_columns_of_the_whole_video():
    from tvretrieval_amd import ingest, ops
    from tvretrieval_amd._lib import XmlHipError
    d, total = 24, 75
    g = torch.Generator().manual_seed(77)
    video = torch.randn(total, d, generator=g).to(F16)
    table = ingest.plan_parts(np.array([total]), 32, overlap=8)
    offs, lens = table.part_offset.tolist(), table.part_len.tolist()
    assert table.n_parts == 3 and offs == [0, 24, 43] and lens == [32, 32, 32]
    whole, _ = ops.ingest_rows(video.to(DEV), torch.tensor([0, total], device=DEV), 1, total, total, tef=True)
    _same(whole[0, :, d:], torch.from_numpy(REF.endpoint_columns(total)), "unsplit columns")
    # + an item at position -1 and one whose video is too short for it: both get their own axis
    offs2, lens2, tots = offs + [-1, 50], lens + [9, 25], [total] * 3 + [total, 74]
    rows = torch.cat([video[o:o + n] if o >= 0 else video[:n] for o, n in zip(offs2, lens2)])
    rs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)).to(DEV)
    pool_src = (rows.to(DEV), torch.stack([torch.arange(len(rows)), torch.arange(len(rows)) + 1], 1).to(DEV), False)
    for dst_dt in (F32, BF16):
        got, _ = ops.ingest_rows(rows.to(DEV), rs, 5, 32, 32, out_dtype=dst_dt, tef=True, tef_pos=_i32(offs2), tef_len=_i32(tots))
        pooled, _ = ops.ingest_pool_rows([pool_src], rs, 5, 32, 32, out_dtype=dst_dt, tef=True, tef_pos=_i32(offs2),
                                         tef_len=_i32(tots))
        plain, _ = ops.ingest_rows(rows.to(DEV), rs, 5, 32, 32, out_dtype=dst_dt, tef=True)
        plain_pooled, _ = ops.ingest_pool_rows([pool_src], rs, 5, 32, 32, out_dtype=dst_dt, tef=True)
        for name, t, own in (("rows", got, plain), ("pooled", pooled, plain_pooled)):
            for p in range(3):
                _same(t[p, :, d:], whole[0, offs[p]:offs[p] + 32, d:].to(dst_dt), "%s part %d" % (name, p))
            _same(t[3:, :, d:], own[3:, :, d:], name + ": items whose place cannot hold them")
            _same(t[:, :, :d], own[:, :, :d], name + " feature columns")
        _same(got[3:, :, d:], _want_tef(lens2[3:], 32, 32, dst_dt), "own-axis columns")
    for kw in (dict(tef_pos=_i32(offs2)), dict(tef_len=_i32(tots))):
        with pytest.raises(XmlHipError, match="both or neither"):
            ops.ingest_rows(rows.to(DEV), rs, 5, 32, 32, tef=True, **kw)
        with pytest.raises(XmlHipError, match="both or neither"):
            ops.ingest_pool_rows([pool_src], rs, 5, 32, 32, tef=True, **kw)


# ---------------------------------------------------------------------------------------------------------
# 4. the feeder against the reference-made fixture
# ---------------------------------------------------------------------------------------------------------
def test_context_feeder_matches_reference_fixture(tmp_path):
    from test_ingest_tef import golden_stores
    from tvretrieval_amd import ingest
    z, names, stores, _ = golden_stores(tmp_path)
    max_l, bsz = int(z["max_l"]), int(z["bsz"])
    feeder = ingest.ContextFeeder(names, stores["video"], stores["sub"], max_ctx_len=max_l, batch_size=bsz, device=DEV,
                                  ctx_mode="video_sub_tef")
    for bi, (v, vm, s, sm) in enumerate(feeder):
        for tag, got, gm in (("video", v, vm), ("sub", s, sm)):
            d = stores[tag].dim
            want = z["video_sub_tef/batch%d/%s_feat" % (bi, tag)]
            np.testing.assert_array_equal(gm.cpu().numpy(), z["video_sub_tef/batch%d/%s_mask" % (bi, tag)])
            got = got.cpu().numpy()
            assert got.shape == want.shape and got.shape[2] == d + 2
            np.testing.assert_array_equal(got[:, :, d:], want[:, :, d:])
            np.testing.assert_allclose(got[:, :, :d], want[:, :, :d], rtol=2e-6, atol=1e-7)
    assert bi == (len(names) - 1) // bsz


def test_context_feeder_pooled_matches_reference_fixture(tmp_path):
    """video_tef over a PooledStore whose fine rows are the clip rows themselves, ranges of one row each."""
    from test_ingest_tef import golden_stores
    from tvretrieval_amd import ingest
    z, names, stores, _ = golden_stores(tmp_path)
    max_l, bsz = int(z["max_l"]), int(z["bsz"])
    ranges = {n: np.stack([np.arange(int(k)), np.arange(int(k)) + 1], 1) for n, k in zip(names, z["lens"])}
    pooled = ingest.PooledStore([(stores["video"], ranges, False)], pool="max")
    feeder = ingest.ContextFeeder(names, pooled, None, max_ctx_len=max_l, batch_size=bsz, device=DEV, ctx_mode="video_tef")
    d = stores["video"].dim
    for bi, (v, vm, s, sm) in enumerate(feeder):
        assert s is None and sm is None
        want = z["video_tef/batch%d/video_feat" % bi]
        np.testing.assert_array_equal(vm.cpu().numpy(), z["video_tef/batch%d/video_mask" % bi])
        got = v.cpu().numpy()
        assert got.shape == want.shape and got.shape[2] == d + 2
        np.testing.assert_array_equal(got[:, :, d:], want[:, :, d:])
        np.testing.assert_allclose(got[:, :, :d], want[:, :, :d], rtol=2e-6, atol=1e-7)
    assert bi == (len(names) - 1) // bsz


# ---------------------------------------------------------------------------------------------------------
# 5. end to end: index and search
# ---------------------------------------------------------------------------------------------------------
DV, DS, DQ, HID = 48, 32, 32, 128


def _stores(tmp_path, lens, seed):
    from tvretrieval_amd import ingest
    rng = np.random.default_rng(seed)
    names = ["v%02d" % i for i in range(len(lens))]
    for tag, dim in (("video", DV), ("sub", DS)):
        feats = {n: (rng.standard_normal((int(k), dim)) * rng.uniform(0.3, 2.0)).astype(np.float32) for n, k in zip(names, lens)}
        ingest.write_feature_store(str(tmp_path / tag), feats, dtype="float16")
    return names, ingest.FeatureStore(str(tmp_path / "video")), ingest.FeatureStore(str(tmp_path / "sub"))


def _model(max_ctx_l, seed):
    from test_gpu_model import _synthetic_model
    return _synthetic_model("video_sub", HID, DV + 2, DS + 2, DQ, max_ctx_l, torch.float32, seed=seed)[0]


def _queries(nq, seed):
    from test_gpu_model import _feats
    qf, qm = _feats(nq, np.random.default_rng(seed).integers(5, 31, nq), DQ, seed + 1)
    return qf.to(DEV), qm.to(DEV)


def test_index_from_the_feeder_equals_index_from_host_made_columns(tmp_path):
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ingest
    rng = np.random.default_rng(8)
    lens = rng.integers(10, 65, 10)
    lens[0] = 64
    names, vs, ss = _stores(tmp_path, lens, 9)
    m = _model(64, 9)
    kw = dict(max_ctx_len=64, batch_size=4, device=DEV)
    with torch.no_grad():
        a = inf.build_corpus_index(m, ingest.ContextFeeder(names, vs, ss, ctx_mode="video_sub_tef", **kw))
        batches = []
        for v, vm, s, sm in ingest.ContextFeeder(names, vs, ss, **kw):
            b = len(batches) * 4
            tef = torch.from_numpy(REF.restate_tef(lens[b:b + 4], v.shape[1], 64)).to(DEV)
            batches.append((torch.cat([v, tef], 2), vm, torch.cat([s, tef], 2), sm))
        b = inf.build_corpus_index(m, batches)
        qf, qm = _queries(7, 21)
        ra = inf.vcmr_search(m, a, qf, qm, max_vcmr_video=5, max_before_nms=50)
        rb = inf.vcmr_search(m, b, qf, qm, max_vcmr_video=5, max_before_nms=50)
    assert a.modalities == b.modalities == ["video", "sub"]
    for mod in a.modalities:
        _same(a.feat1n_rows(mod), b.feat1n_rows(mod), "feat1[%s]" % mod)
        _same(a.feat2[mod], b.feat2[mod], "feat2[%s]" % mod)
        _same(a.mask[mod], b.mask[mod], "mask[%s]" % mod)
    for k in ("top_indices", "flat_indices"):
        assert torch.equal(ra[k], rb[k]), k
    # explain_moments reads the resident rows of either index alike
    pq = torch.arange(7, dtype=torch.int32, device=DEV)
    pv = ra["top_indices"][:, 0].to(torch.int32)
    with torch.no_grad():
        ea, eb = inf.explain_moments(m, a, qf, qm, pq, pv), inf.explain_moments(m, b, qf, qm, pq, pv)
    for k in ("video_similarity", "sub_similarity", "similarity", "st_logits", "ed_logits", "ctx_len", "q2c"):
        _same(ea[k], eb[k], "explain_moments " + k)
    assert int(ea["ctx_len"].min()) >= 10


def test_mutable_indexes_take_the_wider_batches(tmp_path):
    """MutableCorpusIndex.from_batches, plain and packed (tiles=N), fed by ContextFeeder(ctx_mode="video_sub_tef"): the records of
    both equal those of the one-shot index over the same batches.  (The packed form needs 128-clip slots: max_ctx_l = 80.)"""
    from test_gpu_index_parts_search import _record_lists
    from test_gpu_parts import _host
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ingest
    from tvretrieval_amd.index_update import MutableCorpusIndex
    lens = np.random.default_rng(12).integers(10, 81, 10)
    lens[0] = 80
    names, vs, ss = _stores(tmp_path, lens, 13)
    m = _model(80, 13)
    ids = [300 + 7 * i for i in range(10)]
    skw = dict(max_vcmr_video=5, max_before_nms=50, nms_thd=0.5, max_after_nms=10, clip_length=1.5)

    def feeder():
        return ingest.ContextFeeder(names, vs, ss, max_ctx_len=80, batch_size=4, device=DEV, ctx_mode="video_sub_tef")

    qf, qm = _queries(7, 23)
    with torch.no_grad():
        fixed = inf.build_corpus_index(m, feeder(), length_buckets=False)
        want = inf.vcmr_search(m, fixed, qf, qm, meta2vid=torch.tensor(ids, dtype=torch.int32, device=DEV), **skw)
        plain = MutableCorpusIndex.from_batches(m, feeder(), 12, ids=ids)
        packed = MutableCorpusIndex.from_batches(m, feeder(), 12, ids=ids, n_clips=[int(x) for x in lens], tiles=8)
        got = [inf.vcmr_search(m, x, qf, qm, **skw) for x in (plain, packed)]
    wrec, wcnt = _host(want["records"]), want["record_count"].cpu().numpy()
    assert (wcnt > 0).all()
    for q in range(len(wcnt)):         # the precondition of comparing sorted lists: no two listed moments share a score
        sc = wrec["score"][q][: int(wcnt[q])]
        assert len(np.unique(sc)) == len(sc), "query %d: tied moment scores -- choose another seed" % q
    for out in got:
        assert _record_lists(_host(out["records"]), out["record_count"].cpu().numpy()) == _record_lists(wrec, wcnt)


# ---------------------------------------------------------------------------------------------------------
# 6. long videos
# ---------------------------------------------------------------------------------------------------------
def test_long_videos_carry_whole_video_time_into_both_indexes(tmp_path):
    from test_gpu_index_parts_search import _record_lists
    from test_gpu_parts import _host
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ingest
    from tvretrieval_amd.index_update import MutableCorpusIndex
    W, OV, CLIP = 32, 16, 1.5
    lens, ids = [75, 90], [501, 777]
    names, vs, ss = _stores(tmp_path, lens, 31)
    table = ingest.plan_parts(np.array(lens), W, overlap=OV)
    assert table.n_parts == 9
    m = _model(W, 31)
    skw = dict(max_vcmr_video=2, max_before_nms=40, max_pred_l=OV, nms_thd=0.5, max_after_nms=10, clip_length=CLIP)

    def feeder(bsz):
        return ingest.ContextFeeder(names, vs, ss, max_ctx_len=W, batch_size=bsz, device=DEV, parts=table, ctx_mode="video_sub_tef")

    qf, qm = _queries(7, 41)
    with torch.no_grad():
        # the parts' columns are the unsplit videos' (batches of 4 parts: a video's parts straddle batches)
        whole = [torch.from_numpy(REF.endpoint_columns(n)) for n in lens]
        p = 0
        for v, vm, s, sm in feeder(4):
            assert v.shape[2] == DV + 2 and s.shape[2] == DS + 2
            for k in range(v.shape[0]):
                vid, off, ln = int(table.part_video[p]), int(table.part_offset[p]), int(table.part_len[p])
                _same(v[k, :ln, DV:], whole[vid][off:off + ln], "video part %d" % p)
                _same(s[k, :ln, DS:], whole[vid][off:off + ln], "sub part %d" % p)
                p += 1
        assert p == 9
        fixed = inf.build_corpus_index(m, feeder(4), parts=table, l_ref=W, length_buckets=False)
        want = inf.vcmr_search(m, fixed, qf, qm, meta2vid=torch.tensor(ids, dtype=torch.int32, device=DEV), **skw)
        chained = MutableCorpusIndex.from_batches(m, feeder(16), 12, l_ref=W, ids=ids, parts=table, part_overlap=OV, max_parts=8)
        got = inf.vcmr_search(m, chained, qf, qm, **skw)
        added = MutableCorpusIndex.create(m, 12, l_ref=W, part_overlap=OV, max_parts=8)
        for batch in feeder(16):
            added.add(*batch, ids=ids, parts=table)
        got2 = inf.vcmr_search(m, added, qf, qm, **skw)
    wrec, wcnt = _host(want["records"]), want["record_count"].cpu().numpy()
    assert (wcnt > 0).all()
    for q in range(len(wcnt)):         # the precondition of comparing sorted lists: no two listed moments share a score
        sc = wrec["score"][q][: int(wcnt[q])]
        assert len(np.unique(sc)) == len(sc), "query %d: tied moment scores -- choose another seed" % q
    for out in (got, got2):
        assert _record_lists(_host(out["records"]), out["record_count"].cpu().numpy()) == _record_lists(wrec, wcnt)
        assert _record_lists(_host(out["nms_records"]), out["nms_count"].cpu().numpy()) == \
            _record_lists(_host(want["nms_records"]), want["nms_count"].cpu().numpy())
    n_clips = dict(zip(ids, lens))
    for out in (want, got, got2):
        rec, cnt = _host(out["records"]), out["record_count"].cpu().numpy()
        for q in range(len(cnt)):
            for r in rec[q][: int(cnt[q])]:
                assert int(r["vid"]) in n_clips
                assert 0.0 <= float(r["st"]) < float(r["ed"]) <= n_clips[int(r["vid"])] * CLIP, (q, r)


# ---------------------------------------------------------------------------------------------------------
# 7. the dataset path: compute_context_info over StoreEvalDataset(ctx_mode=) serves the same model
# ---------------------------------------------------------------------------------------------------------
def test_compute_context_info_over_the_store_dataset(tmp_path):
    """The host-made columns of StoreEvalDataset are bitwise the launch's, the features agree to the feeder's fixture tolerance
    (2e-6 relative); the encodings of the two paths are compared at the f32 encoder tolerance of tests/test_gpu_model.py (2e-4)."""
    import argparse
    from test_gpu_kernels import close
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ingest
    lens = [64, 10, 33, 1, 47]
    names = ["v%02d" % i for i in range(len(lens))]
    rng = np.random.default_rng(52)
    for tag, dim in (("video", DV), ("sub", DS)):        # f32 stores: both paths read the same numbers
        ingest.write_feature_store(str(tmp_path / tag), {n: rng.standard_normal((k, dim)).astype(np.float32)
                                                         for n, k in zip(names, lens)}, dtype="float32")
    ingest.write_feature_store(str(tmp_path / "desc"), {"0": np.ones((3, DQ), np.float32)}, dtype="float32")
    vs, ss = ingest.FeatureStore(str(tmp_path / "video")), ingest.FeatureStore(str(tmp_path / "sub"))
    ds = ingest.StoreEvalDataset([dict(desc_id=0, desc="d", vid_name=names[0])], [dict(vid_name=n, duration=1.0) for n in names],
                                 {n: i for i, n in enumerate(names)}, ingest.FeatureStore(str(tmp_path / "desc")), vs, ss,
                                 max_desc_len=6, max_ctx_len=64, ctx_mode="video_sub_tef")
    m = _model(64, 53)
    opt = argparse.Namespace(eval_context_bsz=2, device=torch.device(DEV))
    with torch.no_grad():
        ctx = inf.compute_context_info(m, ds, opt)
        index = inf.build_corpus_index(m, ingest.ContextFeeder(names, vs, ss, max_ctx_len=64, batch_size=2, device=DEV,
                                                               ctx_mode="video_sub_tef"), keep_raw=True)
    assert [e["vid_name"] for e in ctx["video_metas"]] == names
    for mod in ("video", "sub"):
        _same(ctx[mod + "_mask"], index.mask[mod][:, :index.l_ref], mod + " mask")
        for k, other in (("feat1", index.raw_feat1), ("feat2", index.feat2)):
            a, b = ctx["%s_%s" % (mod, k)], other[mod][:, :index.l_ref]
            print("%s %s: max |dataset - feeder| = %.3e" % (mod, k, float((a.float() - b.float()).abs().max())))
            close("%s %s" % (mod, k), a, b, 2e-4)
