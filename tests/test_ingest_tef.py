"""The *_tef context modes on the corpus side, without a GPU: StoreEvalDataset(ctx_mode=) items against the fixture made by the
reference's StartEndEvalDataset._get_item_context + start_end_collate (tests/golden/eval_collate_tef.npz,
tools/make_golden.py::gen_eval_collate_tef_case), every refusal of ContextFeeder(ctx_mode=) / StoreEvalDataset(ctx_mode=) --
each a ValueError before any device work --, and ctx_mode=None as it ever was."""
import json
import os

import numpy as np
import pytest
import torch

import ingest_tef_ref as REF


def golden_stores(tmp_path, dtype="float32"):
    """The raw arrays of tests/golden/eval_collate_tef.npz written into FeatureStores."""
    from conftest import GOLDEN
    from tvretrieval_amd import ingest
    z = np.load(os.path.join(GOLDEN, "eval_collate_tef.npz"))
    lens = z["lens"]
    names = ["vid_%d" % i for i in range(len(lens))]
    off = np.concatenate([[0], np.cumsum(lens)])
    stores, raw = {}, {}
    for tag in ("video", "sub"):
        raw[tag] = {n: z["raw/" + tag][off[i]:off[i + 1]] for i, n in enumerate(names)}
        ingest.write_feature_store(str(tmp_path / tag), raw[tag], dtype=dtype)
        stores[tag] = ingest.FeatureStore(str(tmp_path / tag))
    return z, names, stores, raw


def _dataset(tmp_path, names, video_store, sub_store, max_l, **kw):
    from tvretrieval_amd import ingest
    if not os.path.isfile(str(tmp_path / "desc.json")):
        ingest.write_feature_store(str(tmp_path / "desc"), {"0": np.ones((3, 8), np.float32)}, dtype="float32")
    ds = ingest.StoreEvalDataset([dict(desc_id=0, desc="d", vid_name=names[0])], [dict(vid_name=n, duration=1.0) for n in names],
                                 {n: i for i, n in enumerate(names)}, ingest.FeatureStore(str(tmp_path / "desc")),
                                 video_store, sub_store, max_desc_len=6, max_ctx_len=max_l, **kw)
    ds.set_data_mode("context")
    return ds


def test_restatement_is_the_reference_formula():
    for L in (1, 2, 3, 7, 33, 75, 100, 129):
        st = torch.arange(0, L, 1.0) / L
        want = torch.stack([st, st + 1.0 / L], dim=1).numpy()
        np.testing.assert_array_equal(REF.endpoint_columns(L), want)
    whole = REF.endpoint_columns(75)
    np.testing.assert_array_equal(REF.endpoint_columns(32, 43, 75), whole[43:75])


@pytest.mark.parametrize("mode", ["video_sub_tef", "video_tef", "sub_tef"])
def test_dataset_items_match_reference_fixture(tmp_path, mode):
    z, names, stores, _ = golden_stores(tmp_path)
    assert mode in json.loads(str(z["modes"]))
    max_l, bsz = int(z["max_l"]), int(z["bsz"])
    tags = [t for t in ("video", "sub") if t in mode]
    ds = _dataset(tmp_path, names, stores["video"] if "video" in tags else None, stores["sub"] if "sub" in tags else None, max_l,
                  ctx_mode=mode)
    for i in range(len(names)):
        item = ds[i]["model_inputs"]
        assert sorted(item) == sorted(t + "_feat" for t in tags)
        n = min(int(z["lens"][i]), max_l)
        for tag in tags:
            want = z["%s/batch%d/%s_feat" % (mode, i // bsz, tag)][i % bsz]
            got = item[tag + "_feat"]
            d = stores[tag].dim
            assert got.shape == (n, d + 2) and got.dtype == np.float32
            np.testing.assert_array_equal(got[:, d:], want[:n, d:])
            np.testing.assert_array_equal(got[:, d:], REF.endpoint_columns(n))
            np.testing.assert_allclose(got[:, :d], want[:n, :d], rtol=1e-6, atol=1e-8)
            assert (want[n:] == 0).all()
            np.testing.assert_array_equal(z["%s/batch%d/%s_mask" % (mode, i // bsz, tag)][i % bsz, :n], 1)


def test_ctx_mode_none_gives_the_items_of_before(tmp_path):
    z, names, stores, raw = golden_stores(tmp_path)
    max_l = int(z["max_l"])
    ds = _dataset(tmp_path, names, stores["video"], stores["sub"], max_l)
    same = _dataset(tmp_path, names, stores["video"], stores["sub"], max_l, ctx_mode="video_sub")
    for i, n in enumerate(names):
        item, item2 = ds[i]["model_inputs"], same[i]["model_inputs"]
        assert sorted(item) == ["sub_feat", "video_feat"]
        for tag in ("video", "sub"):
            a = raw[tag][n][:max_l]
            want = a / (np.linalg.norm(a, axis=-1, keepdims=True) + 1e-5)
            np.testing.assert_array_equal(item[tag + "_feat"], want)
            np.testing.assert_array_equal(item2[tag + "_feat"], want)
    only_video = _dataset(tmp_path, names, stores["video"], None, max_l)
    assert sorted(only_video[0]["model_inputs"]) == ["video_feat"] and only_video[0]["model_inputs"]["video_feat"].shape[1] == 48


class _NoDeviceOps(object):
    """A backend that must never be reached: a refusal comes before any device work."""

    def __getattr__(self, name):
        raise AssertionError("ops.%s reached: the refusal must come before any device work" % name)


def test_refusals_come_before_any_device_work(tmp_path):
    from tvretrieval_amd import ingest
    z, names, stores, raw = golden_stores(tmp_path)
    vs, ss, max_l = stores["video"], stores["sub"], int(z["max_l"])
    ops = _NoDeviceOps()
    makers = (lambda v, s, **kw: ingest.ContextFeeder(names, v, s, max_ctx_len=max_l, batch_size=4, device="cpu", ops=ops, **kw),
              lambda v, s, **kw: _dataset(tmp_path, names, v, s, max_l, **kw))
    for make in makers:
        for bad in ("tef", "video_sub_tef_x", "", "VIDEO", "sub_video", 3):
            with pytest.raises(ValueError, match="ctx_mode"):
                make(vs, ss, ctx_mode=bad)
        # a mode that names a stream without its store
        for mode, v, s in (("video_sub_tef", vs, None), ("video_sub", None, ss), ("video_tef", None, None), ("sub_tef", None, None),
                           ("sub", None, None), ("video", None, None)):
            with pytest.raises(ValueError, match="needs a (video|sub) store"):
                make(v, s, ctx_mode=mode)
        # a store without its stream
        for mode, v, s in (("video_tef", vs, ss), ("sub_tef", vs, ss), ("video", vs, ss), ("sub", vs, ss)):
            with pytest.raises(ValueError, match="store is given"):
                make(v, s, ctx_mode=mode)
        for mode in ("video", "sub", "video_sub", "video_tef", "sub_tef", "video_sub_tef"):      # and the six modes are taken
            make(vs if "video" in mode else None, ss if "sub" in mode else None, ctx_mode=mode)
    # one endpoint feature for both streams: a video whose stores disagree on the clip count is named
    short = dict(raw["sub"])
    short[names[3]] = short[names[3]][:min(len(short[names[3]]), max_l) - 1]
    ingest.write_feature_store(str(tmp_path / "sub_short"), short, dtype="float32")
    ss2 = ingest.FeatureStore(str(tmp_path / "sub_short"))
    with pytest.raises(ValueError, match=names[3]):
        ingest.ContextFeeder(names, vs, ss2, max_ctx_len=max_l, batch_size=4, device="cpu", ops=ops, ctx_mode="video_sub_tef")
    ingest.ContextFeeder(names, vs, ss2, max_ctx_len=max_l, batch_size=4, device="cpu", ops=ops, ctx_mode="video_sub")
    ds = _dataset(tmp_path, names, vs, ss2, max_l, ctx_mode="video_sub_tef")
    with pytest.raises(ValueError, match=names[3]):
        ds[3]
    # with parts the existing check of the part table covers it
    table = ingest.plan_parts(np.array([len(raw["video"][n]) for n in names]), max_l, overlap=8)
    with pytest.raises(ValueError, match=names[3]):
        ingest.ContextFeeder(names, vs, ss2, max_ctx_len=max_l, batch_size=4, device="cpu", ops=ops, parts=table,
                             ctx_mode="video_sub_tef")


class _RecordingOps(object):
    """Stands in for the HIP backend on the CPU: records what the feeder asks of ingest_rows and answers with the restatement."""

    def __init__(self):
        self.calls = []

    def ingest_rows(self, src, row_start, n, lmax, max_len, normalize=True, eps=1e-5, out_dtype=torch.float32, **kw):
        self.calls.append(dict(kw, n=n, lmax=lmax))
        assert kw.get("tef") is True
        pos, tot = kw.get("tef_pos"), kw.get("tef_len")
        out, mask = REF.restate_rows(src.numpy(), row_start.numpy(), lmax, max_len, normalize,
                                     None if pos is None else pos.numpy(), None if tot is None else tot.numpy())
        return torch.from_numpy(out), torch.from_numpy(mask)


def test_feeder_hands_parts_their_place_in_the_whole_video(tmp_path):
    """ContextFeeder(parts=, ctx_mode=*_tef): tef_pos = the part's offset, tef_len = the whole video's clip count, (n,) int32
    with row_start; the columns of every part are then the unsplit video's at those clips.  Without parts: neither array."""
    from tvretrieval_amd import ingest
    z, names, stores, raw = golden_stores(tmp_path)
    counts = np.array([len(raw["video"][n]) for n in names])
    table = ingest.plan_parts(counts, 32, overlap=8)
    ops = _RecordingOps()
    feeder = ingest.ContextFeeder(names, stores["video"], None, max_ctx_len=32, batch_size=4, device="cpu", ops=ops, parts=table,
                                  ctx_mode="video_tef")
    p = 0
    for v, vm, s, sm in feeder:
        assert s is None and sm is None and v.shape[2] == 48 + 2
        call = ops.calls.pop(0)
        assert call["tef_pos"].dtype == torch.int32 and call["tef_len"].dtype == torch.int32
        assert call["tef_pos"].shape == call["tef_len"].shape == (v.shape[0],)
        for k in range(v.shape[0]):
            vid, off, ln = int(table.part_video[p]), int(table.part_offset[p]), int(table.part_len[p])
            assert (int(call["tef_pos"][k]), int(call["tef_len"][k])) == (off, int(counts[vid]))
            np.testing.assert_array_equal(v[k, :ln, 48:].numpy(), REF.endpoint_columns(int(counts[vid]))[off:off + ln])
            p += 1
    assert p == table.n_parts and not ops.calls
    feeder = ingest.ContextFeeder(names, stores["video"], None, max_ctx_len=40, batch_size=4, device="cpu", ops=ops,
                                  ctx_mode="video_tef")
    for bi, (v, vm, s, sm) in enumerate(feeder):
        call = ops.calls.pop(0)
        assert "tef_pos" not in call and "tef_len" not in call
        np.testing.assert_array_equal(v.numpy()[:, :, 48:], z["video_tef/batch%d/video_feat" % bi][:, :, 48:])
