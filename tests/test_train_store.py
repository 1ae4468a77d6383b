"""Training data path on the host (train_data.py): StoreTrainDataset + collate against batches made by the reference's own
StartEndDataset / start_end_collate / prepare_batch_inputs (tests/golden/train_collate.npz, tools/make_golden.py::
gen_train_collate_case), epoch planning, the store's ValueErrors, and the C ABI of the two gather entries (no GPU)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_collate_fixture(tmp_path, dtype="float32"):
    """-> (npz, examples, {"desc" | "video" | "sub": FeatureStore}) with the fixture's raw arrays written into stores."""
    from tvretrieval_amd import ingest
    z = np.load(os.path.join(GOLDEN, "train_collate.npz"))
    examples = json.loads(str(z["examples"]))
    voff = np.concatenate([[0], np.cumsum(z["vlens"])])
    qoff = np.concatenate([[0], np.cumsum(z["qlens"])])
    feats = dict(video={"vid_%d" % i: z["raw/video"][voff[i]:voff[i + 1]] for i in range(len(z["vlens"]))},
                 sub={"vid_%d" % i: z["raw/sub"][voff[i]:voff[i + 1]] for i in range(len(z["vlens"]))},
                 desc={str(e["desc_id"]): z["raw/desc"][qoff[i]:qoff[i + 1]] for i, e in enumerate(examples)})
    stores = {}
    for tag, f in feats.items():
        ingest.write_feature_store(str(tmp_path / tag), f, dtype=dtype)
        stores[tag] = ingest.FeatureStore(str(tmp_path / tag))
    return z, examples, stores


def fixture_cases(z):
    return [(m, bool(n)) for m, n in json.loads(str(z["cases"]))]


def fixture_kw(z, mode, norm):
    return dict(dset_name="tvr", max_desc_len=int(z["max_desc_len"]), max_ctx_len=int(z["max_ctx_len"]),
                clip_length=float(z["clip_length"]), ctx_mode=mode, normalize_vfeat=norm, normalize_tfeat=norm)


def test_dataset_and_collate_match_the_reference_batches(tmp_path):
    from tvretrieval_amd import train_data as td
    z, examples, st = load_collate_fixture(tmp_path)
    bsz, seen = int(z["bsz"]), 0
    for mode, norm in fixture_cases(z):
        ds = td.StoreTrainDataset(examples, st["desc"], st["video"], st["sub"], **fixture_kw(z, mode, norm))
        assert len(ds) == 9
        for b in range(0, len(ds), bsz):
            items = [ds[i] for i in range(b, min(b + bsz, len(ds)))]
            meta, batch = td.collate(items, ds.use_video, ds.use_sub)
            assert [m["desc_id"] for m in meta] == [e["desc_id"] for e in examples[b:b + bsz]]
            pre = "%s/%s/batch%d/" % (mode, "norm" if norm else "raw", b // bsz)
            np.testing.assert_array_equal(batch["st_ed_indices"], z[pre + "st_ed_indices"])
            for tag, use in (("query", True), ("video", ds.use_video), ("sub", ds.use_sub)):
                if not use:
                    assert batch[tag + "_feat"] is None and batch[tag + "_mask"] is None and (pre + tag + "_feat") not in z
                    continue
                want, wmask = z[pre + tag + "_feat"], z[pre + tag + "_mask"]
                got, gmask = batch[tag + "_feat"], batch[tag + "_mask"]
                assert got.shape == want.shape and got.dtype == np.float32
                np.testing.assert_array_equal(gmask, wmask)
                assert (got[wmask == 0] == 0).all()                                    # padding, TEF columns included
                d = got.shape[-1] - (2 if ds.use_tef and tag != "query" else 0)
                np.testing.assert_array_equal(got[..., d:], want[..., d:])           # TEF columns: exact
                if norm:
                    np.testing.assert_allclose(got[..., :d], want[..., :d], rtol=1e-6)
                else:
                    np.testing.assert_array_equal(got[..., :d], want[..., :d])
                seen += 1
            if ds.use_tef:
                tef = np.zeros_like(z[pre + "tef_feat"])
                for i, it in enumerate(items):
                    t = it["model_inputs"]["tef_feat"].numpy()
                    tef[i, :len(t)] = t
                np.testing.assert_array_equal(tef, z[pre + "tef_feat"])
    assert seen == 2 * (3 + 3 + 3 + 2 + 2)


def test_labels_and_lengths_of_the_plan_match_the_fixture(tmp_path):
    """plan_examples (what DeviceTrainStore uploads as its label table) restates get_st_ed_label: both clamps are hit."""
    from tvretrieval_amd import train_data as td
    z, examples, st = load_collate_fixture(tmp_path)
    q_len, ctx_len, labels = td.plan_examples(examples, st["desc"], st["video"], st["sub"], "tvr", 6, 40, 1.5, "video_sub")
    want = np.concatenate([z["video_sub/norm/batch0/st_ed_indices"], z["video_sub/norm/batch1/st_ed_indices"]])
    np.testing.assert_array_equal(labels, want)
    assert ctx_len.tolist() == [7, 1, 40, 7, 23, 1, 40, 7, 1] and q_len.tolist() == [4, 1, 6, 6, 3, 6, 2, 5, 6]
    assert labels[2].tolist() == [20, 39] and labels[3].tolist() == [6, 6] and labels[1].tolist() == [0, 0]


def test_didemo_agreed_timestamp_rule():
    from tvretrieval_amd import train_data as td
    assert td.didemo_agreed_ts([[1, 1], [1, 1], [1, 1], [0, 0]]) == (1, 1)
    assert td.didemo_agreed_ts([[2, 3], [0, 1], [0, 1], [2, 3]]) == (2, 3)          # tie: the first seen
    assert td.didemo_agreed_ts([[4, 4]]) == (4, 4)
    assert td.st_ed_label((3.2, 7.6), 1.5, 100) == (2, 6)


def test_epoch_planning_without_a_device():
    from tvretrieval_amd import train_data as td
    g = torch.Generator().manual_seed(7)
    want = torch.randperm(23, generator=torch.Generator().manual_seed(7)).numpy()
    state = torch.get_rng_state()
    order, batches = td.plan_epoch(23, 6, generator=g)
    assert torch.equal(torch.get_rng_state(), state)                               # the global generator is untouched
    np.testing.assert_array_equal(order, want)
    assert [len(b) for b in batches] == [6, 6, 6, 5]
    np.testing.assert_array_equal(np.concatenate(batches), want)
    order, batches = td.plan_epoch(23, 6, order=np.arange(23)[::-1])
    np.testing.assert_array_equal(batches[0], [22, 21, 20, 19, 18, 17])
    np.testing.assert_array_equal(batches[-1], [4, 3, 2, 1, 0])
    for world in (2, 4):
        parts = [td.plan_epoch(23, 6, order=want, rank=r, world=world)[1] for r in range(world)]
        for b in range(4):
            for r in range(world):
                np.testing.assert_array_equal(parts[r][b], want[6 * b:6 * b + 6][r::world])
        assert sorted(np.concatenate([np.concatenate(p) for p in parts]).tolist()) == list(range(23))
    assert len(td.plan_epoch(100, 6, order=np.arange(100), debug=True)[1]) == 4
    assert [len(b) for b in td.plan_epoch(3, 4, order=np.arange(3), rank=3, world=4)[1]] == []
    with pytest.raises(ValueError):
        td.plan_epoch(10, 4, rank=2, world=2)


def test_store_construction_errors(tmp_path):
    """Every ValueError is raised from the host tables, before anything is uploaded."""
    from tvretrieval_amd import ingest, train_data as td
    z, examples, st = load_collate_fixture(tmp_path)
    kw = dict(max_desc_len=6, max_ctx_len=40, clip_length=1.5, device="cpu")
    mk = lambda ex, mode="video_sub", **s: td.DeviceTrainStore(                                   # noqa: E731
        ex, s.get("desc", st["desc"]), s.get("video", st["video"]), s.get("sub", st["sub"]), ctx_mode=mode, **kw)
    with pytest.raises(ValueError, match="missing from the video store"):
        mk(examples + [dict(desc_id=100, desc="", vid_name="nope", duration=1.0, ts=[0, 1])])
    with pytest.raises(ValueError, match="missing from the description store"):
        mk(examples + [dict(desc_id=999, desc="", vid_name="vid_0", duration=1.0, ts=[0, 1])])
    with pytest.raises(ValueError, match="ctx_mode"):
        mk(examples, mode="tef")
    with pytest.raises(ValueError, match="ctx_mode"):
        td.StoreTrainDataset(examples, st["desc"], st["video"], st["sub"], ctx_mode="audio")
    with pytest.raises(ValueError, match="needs a sub store"):
        td.DeviceTrainStore(examples, st["desc"], st["video"], None, ctx_mode="video_sub", **kw)
    # a store with an empty item; subtitle lengths that differ from the video's after truncation
    w = ingest.FeatureStoreWriter(str(tmp_path / "empty"), 32, "float32")
    for i, n in enumerate((7, 0, 44, 40, 23)):
        w.add("vid_%d" % i, np.zeros((n, 32), np.float32))
    w.close()
    with pytest.raises(ValueError, match="zero rows"):
        mk(examples, sub=ingest.FeatureStore(str(tmp_path / "empty")))
    w = ingest.FeatureStoreWriter(str(tmp_path / "short"), 32, "float32")
    for i, n in enumerate((7, 1, 44, 40, 22)):
        w.add("vid_%d" % i, np.ones((n, 32), np.float32))
    w.close()
    short = ingest.FeatureStore(str(tmp_path / "short"))
    with pytest.raises(ValueError, match="22 subtitle clips"):
        mk(examples, mode="video_sub_tef", sub=short)
    q_len, ctx_len, labels = td.plan_examples(examples, st["desc"], st["video"], short, "tvr", 6, 40, 1.5, "video_sub")
    assert ctx_len[4] == 22                      # without TEF the reference runs, with the subtitle stream's length


def test_host_ids_are_validated(tmp_path):
    from tvretrieval_amd import train_data as td
    z, examples, st = load_collate_fixture(tmp_path)
    store = td.DeviceTrainStore.__new__(td.DeviceTrainStore)
    store.examples = examples
    for bad in ([0, 9], [-1], [], [[0, 1]], [0.5]):
        with pytest.raises(IndexError):
            store._host_ids(bad)
    assert store._host_ids([8, 0, 8]).tolist() == [8, 0, 8]


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_gather_entries_are_declared_exported_and_bound(lib):
    from tvretrieval_amd import _lib, inference, ops
    src = open(os.path.join(ROOT, "include", "xmlhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("xml_gather_feature_rows", 19), ("xml_gather_index_rows", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
        assert name[4:] not in inference.OPS_CONTRACT
    assert callable(ops.gather_feature_rows) and callable(ops.gather_index_rows)
    assert lib.xml_abi_version() == 6


def test_gather_entries_validate_arguments_without_gpu(lib):
    """Both entries reject bad arguments before any launch: -1 (bad argument), -2 (unsupported shape)."""
    p, z = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)

    def feat(src=p, src_dt=2, row_start=p, n_items=5, ids=p, n=4, item_of=p, n_examples=9, dst=p, dst_dt=0, mask=p,
             len_out=p, lmax=8, d=64, max_len=8, eps=1e-5, normalize=1, tef=0):
        return lib.xml_gather_feature_rows(src, src_dt, row_start, n_items, ids, n, item_of, n_examples, dst, dst_dt, mask,
                                           len_out, lmax, d, max_len, eps, normalize, tef, z)
    for kw in (dict(src=z), dict(row_start=z), dict(ids=z), dict(dst=z), dict(n=0), dict(lmax=0), dict(d=0), dict(max_len=-1),
               dict(n_items=0), dict(n_examples=0), dict(src_dt=1), dict(src_dt=3), dict(dst_dt=2), dict(dst_dt=7),
               dict(tef=2), dict(normalize=-1), dict(eps=float("nan"))):
        assert feat(**kw) == -1, kw
    assert feat(d=4100) == -2 and feat(d=4100, src_dt=0, dst_dt=1) == -2
    assert feat(d=4100, src=z) == -1                                    # bad arguments first

    def index(src=p, w=2, n_rows=9, ids=p, n=4, dst=p):
        return lib.xml_gather_index_rows(src, w, n_rows, ids, n, dst, z)
    for kw in (dict(src=z), dict(ids=z), dict(dst=z), dict(w=0), dict(n=0), dict(n_rows=0)):
        assert index(**kw) == -1, kw
    assert index(w=4100) == -2


def test_ops_layer_has_no_cpu_fallback_for_the_gathers():
    from tvretrieval_amd import _lib, ops
    with pytest.raises(_lib.XmlHipError):
        ops.gather_feature_rows(torch.zeros(4, 8), torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 4, 4)
    with pytest.raises(_lib.XmlHipError):
        ops.gather_index_rows(torch.zeros(4, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
