"""ingest.PooledStore on the host (PooledStore.__getitem__): the clip rows a frame- / word-level store pools into, stated in
numpy against tests/ingest_pool_ref.restate, and the training / validation datasets and the training plan over pooled stores
against the same code over clip stores written from those rows.  No GPU."""
import numpy as np
import pytest
import torch

import ingest_pool_ref as ref

MAX_CTX, MAX_DESC, CLIP = 9, 5, 1.5
# four videos: frames per video -> 7, 12 (longer than MAX_CTX), 3 and 1 clips over the shared boundaries
BOUNDS = np.array([0, 5, 9, 14, 18, 23, 27, 32, 36, 41, 45, 50, 54, 59], dtype=np.int64)
FRAMES = {"v0": 30, "v1": 52, "v2": 12, "v3": 4}
CLIPS = {"v0": 7, "v1": 12, "v2": 3, "v3": 1}
# subtitles: (start, end) seconds and words per sentence; v0 has clips no sentence touches (clips 2, 3 and 6)
SUBS = {"v0": ([(0.2, 2.9), (6.1, 8.9)], [4, 6]),
        "v1": ([(0.0, 4.0), (3.5, 9.2), (9.0, 17.9)], [3, 5, 7]),
        "v2": ([(0.5, 4.4)], [5]),
        "v3": ([(0.1, 1.2)], [2])}
EXAMPLES = [dict(desc_id=i, desc="", vid_name=v, duration=CLIPS[v] * CLIP, ts=ts)
            for i, (v, ts) in enumerate([("v1", [3.0, 17.5]), ("v0", [0.0, 2.0]), ("v3", [0.2, 1.0]), ("v1", [14.0, 30.0]),
                                         ("v2", [1.6, 4.4]), ("v0", [7.0, 10.4])])]


def rows(g, n, d):
    """post-ReLU-like rows with a spread of magnitudes and no negative zeros, as ingest_pool_ref.small_case makes them"""
    x = torch.randn(n, d, generator=g) * torch.logspace(-1, 0.7, n)[:, None]
    return torch.where(torch.rand(n, d, generator=g) < 0.3, torch.zeros(()), x.abs() + 0.01 * x).numpy()


def build(tmp_path, dtype="float16", pool="max", norms=(True, True), tag=""):
    """-> (desc store, pooled video store [2 sources, shared boundaries], pooled subtitle store [sentence_word_ranges])"""
    from tvretrieval_amd import ingest
    g = torch.Generator().manual_seed(31)
    p = lambda name: str(tmp_path / (name + tag + dtype + pool))                  # noqa: E731
    feats = {"res": {}, "i3d": {}, "word": {}}
    for v in FRAMES:
        feats["res"][v], feats["i3d"][v] = rows(g, FRAMES[v], 24), rows(g, FRAMES[v], 16)
        feats["word"][v] = rows(g, sum(SUBS[v][1]), 12)
    order = {"res": ["v0", "v1", "v2", "v3"], "i3d": ["v2", "v0", "v3", "v1"], "word": ["v3", "v1", "v0", "v2"]}
    for k in feats:                                     # the sources order their items differently
        ingest.write_feature_store(p(k), {v: feats[k][v] for v in order[k]}, dtype)
    ingest.write_feature_store(p("desc"), {str(e["desc_id"]): rows(g, 3 + e["desc_id"], 12) for e in EXAMPLES}, "float32")
    st = {k: ingest.FeatureStore(p(k)) for k in ("res", "i3d", "word", "desc")}
    word_ranges = {v: ingest.sentence_word_ranges(SUBS[v][0], SUBS[v][1], CLIPS[v], CLIP) for v in FRAMES}
    video = ingest.PooledStore([(st["res"], BOUNDS, norms[0]), (st["i3d"], BOUNDS, norms[1])], pool=pool)
    sub = ingest.PooledStore([(st["word"], word_ranges, False)], pool=pool)
    return st, video, sub, word_ranges


def test_the_small_world_is_what_it_says(tmp_path):
    st, video, sub, word_ranges = build(tmp_path)
    assert {v: video.n_rows(v) for v in FRAMES} == CLIPS and {v: sub.n_rows(v) for v in FRAMES} == CLIPS
    assert CLIPS["v1"] > MAX_CTX
    untouched = np.flatnonzero(word_ranges["v0"][:, 0] == word_ranges["v0"][:, 1])
    assert len(untouched) and (word_ranges["v0"][untouched] == 0).all()          # a clip no sentence touches


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_getitem_equals_the_restatement(tmp_path, dtype, pool):
    for norms in ((False, False), (True, False), (False, True), (True, True)):
        st, video, sub, word_ranges = build(tmp_path, dtype, pool, norms, tag="%d%d" % norms)
        for v, n in CLIPS.items():
            row_start = np.array([0, n], dtype=np.int64)
            segs = video.clip_ranges(v)
            want, _, _ = ref.restate([np.asarray(st["res"][v]), np.asarray(st["i3d"][v])], segs, norms, row_start, 1, n, n, pool,
                                     normalize=False, dtype=np.float32)
            got = video[v]
            assert got.dtype == np.float32 and got.shape == (n, 40) and np.array_equal(got, want[0]), (v, norms)
            want, _, filled = ref.restate([np.asarray(st["word"][v])], [word_ranges[v]], [False], row_start, 1, n, n, pool,
                                          normalize=False, dtype=np.float32)
            got = sub[v]
            assert got.shape == (n, 12) and np.array_equal(got, want[0]), v
            assert not got[filled[0] == 0].any()                                  # a zero block where no sentence touches


def clip_stores(tmp_path, video, sub, tag):
    """f32 clip stores written from the pooled stores' rows"""
    from tvretrieval_amd import ingest
    ingest.write_feature_store(str(tmp_path / ("cv" + tag)), {v: video[v] for v in FRAMES}, "float32")
    ingest.write_feature_store(str(tmp_path / ("cs" + tag)), {v: sub[v] for v in FRAMES}, "float32")
    return ingest.FeatureStore(str(tmp_path / ("cv" + tag))), ingest.FeatureStore(str(tmp_path / ("cs" + tag)))


def same_items(a, b):
    assert a["meta"] == b["meta"] and set(a["model_inputs"]) == set(b["model_inputs"])
    for k, x in a["model_inputs"].items():
        x, y = np.asarray(x), np.asarray(b["model_inputs"][k])
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), k


@pytest.mark.parametrize("mode", ["video_sub", "video_sub_tef", "video_tef", "sub_tef"])
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_datasets_and_plan_over_pooled_stores_equal_those_over_clip_stores(tmp_path, mode, pool):
    from tvretrieval_amd import ingest, train_data as td
    st, video, sub, _ = build(tmp_path, "float16", pool)
    cv, cs = clip_stores(tmp_path, video, sub, pool)
    use_v, use_s = "video" in mode, "sub" in mode
    for norm in (True, False):
        kw = dict(max_desc_len=MAX_DESC, max_ctx_len=MAX_CTX, clip_length=CLIP, ctx_mode=mode, normalize_vfeat=norm,
                  normalize_tfeat=norm)
        a = td.StoreTrainDataset(EXAMPLES, st["desc"], video if use_v else None, sub if use_s else None, **kw)
        b = td.StoreTrainDataset(EXAMPLES, st["desc"], cv if use_v else None, cs if use_s else None, **kw)
        assert len(a) == len(b) == len(EXAMPLES)
        for i in range(len(a)):
            same_items(a[i], b[i])
        assert a[0]["model_inputs"]["video_feat" if use_v else "sub_feat"].shape[0] == MAX_CTX        # truncated
        vd = [dict(vid_name=v, duration=CLIPS[v] * CLIP) for v in FRAMES]
        ekw = dict(max_desc_len=MAX_DESC, max_ctx_len=MAX_CTX, normalize_vfeat=norm, normalize_tfeat=norm, ctx_mode=mode)
        a = ingest.StoreEvalDataset(EXAMPLES, vd, {v: i for i, v in enumerate(FRAMES)}, st["desc"], video if use_v else None,
                                    sub if use_s else None, **ekw)
        b = ingest.StoreEvalDataset(EXAMPLES, vd, {v: i for i, v in enumerate(FRAMES)}, st["desc"], cv if use_v else None,
                                    cs if use_s else None, **ekw)
        for ds in (a, b):
            ds.set_data_mode("context")
        for i in range(len(vd)):
            same_items(a[i], b[i])
    args = ("tvr", MAX_DESC, MAX_CTX, CLIP, mode)
    got = td.plan_examples(EXAMPLES, st["desc"], video if use_v else None, sub if use_s else None, *args)
    want = td.plan_examples(EXAMPLES, st["desc"], cv if use_v else None, cs if use_s else None, *args)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[1].max() == MAX_CTX and (got[2][:, 1] <= got[1] - 1).all()


def test_device_store_construction_errors_by_name(tmp_path):
    """What the reference's scripts or dataset would fail on is a ValueError from the host tables, naming the video."""
    from tvretrieval_amd import ingest, train_data as td
    st, video, sub, word_ranges = build(tmp_path)
    kw = dict(max_desc_len=MAX_DESC, max_ctx_len=MAX_CTX, clip_length=CLIP, device="cpu")
    # the sources disagree on a video's clip count: the second source has too few frames of v2
    g = torch.Generator().manual_seed(5)
    ingest.write_feature_store(str(tmp_path / "i3d_short"), {v: rows(g, 6 if v == "v2" else FRAMES[v], 16) for v in FRAMES})
    bad = ingest.PooledStore([(st["res"], BOUNDS, True), (ingest.FeatureStore(str(tmp_path / "i3d_short")), BOUNDS, True)])
    with pytest.raises(ValueError, match=r"disagree on the clip count of 'v2'"):
        td.DeviceTrainStore(EXAMPLES[:2], st["desc"], bad, None, ctx_mode="video", **kw)
    # a range outside its source
    wr = dict(word_ranges, v3=np.array([[0, 3]]))
    with pytest.raises(ValueError, match=r"range of 'v3' lies outside"):
        td.DeviceTrainStore(EXAMPLES[:2], st["desc"], None, ingest.PooledStore([(st["word"], wr, False)]), ctx_mode="sub", **kw)
    # an example's video with no clips
    wr = dict(word_ranges, v2=np.zeros((0, 2), np.int64))
    with pytest.raises(ValueError, match=r"video v2 has zero rows in the sub store"):
        td.DeviceTrainStore(EXAMPLES, st["desc"], None, ingest.PooledStore([(st["word"], wr, False)]), ctx_mode="sub", **kw)
    # ... which is no error for a video no example names
    store = td.DeviceTrainStore([e for e in EXAMPLES if e["vid_name"] != "v2"], st["desc"], None,
                                ingest.PooledStore([(st["word"], wr, False)]), ctx_mode="sub", **kw)
    r = store.res["sub"]
    assert r.pooled and r.names == ["v3", "v1", "v0", "v2"] and r.clip_start.tolist() == [0, 1, 13, 20, 20]


def test_the_pooled_resident_holds_absolute_ranges(tmp_path):
    from tvretrieval_amd import train_data as td
    st, video, sub, word_ranges = build(tmp_path)
    store = td.DeviceTrainStore(EXAMPLES, st["desc"], video, sub, max_desc_len=MAX_DESC, max_ctx_len=MAX_CTX, clip_length=CLIP,
                                device="cpu")
    rv, rs = store.res["video"], store.res["sub"]
    assert rv.pooled and rs.pooled and not store.res["query"].pooled
    assert rv.names == ["v0", "v1", "v2", "v3"] and rv.dim == 40 and rs.dim == 12 and rv.pool == "max"
    assert rv.clip_start.tolist() == [0, 7, 19, 22, 23] and len(rv.sources) == 2 and len(rs.sources) == 1
    for (rows_dev, seg, norm), key in zip(rv.sources + rs.sources, ("res", "i3d", "word")):
        assert norm == (key != "word") and np.array_equal(rows_dev.numpy(), np.asarray(st[key].data))
        r = rv if key != "word" else rs
        for name in r.names:
            a = int(r.clip_start[r.item[name]])
            rel = (video if key != "word" else sub).clip_ranges(name)[0 if key != "i3d" else 1]
            assert np.array_equal(seg[a:a + len(rel)].numpy(), rel + st[key].index[name][0]), (key, name)
    assert store.item_of["video"].tolist() == [rv.item[e["vid_name"]] for e in EXAMPLES]
