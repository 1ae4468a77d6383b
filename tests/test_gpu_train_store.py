"""GPU tests of the device-resident training data path (train_data.DeviceTrainStore, xml_gather_feature_rows,
xml_gather_index_rows, train_data.train_epoch): batches against the reference-made collate fixture
(tests/golden/train_collate.npz), f16 stores and bf16 output, the shapes at which the gather kernel takes another path, the
golden training steps fed through a store, and the epoch driver against a hand-written loop."""
import json
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_kernels import DEV
from test_gpu_train import NO_DECAY, T, build_train_model, rel_err
from test_train_store import fixture_cases, fixture_kw, load_collate_fixture

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
RTOL, ATOL = 2e-6, 1e-7            # the project's tolerance for xml_ingest_rows against the same reference arithmetic


def tef_columns(length):
    """the reference's temporal endpoint feature, as torch computes it on the CPU (xml/start_end_dataset.py:130-132)"""
    st = torch.arange(0, length, 1.0) / length
    return torch.stack([st, st + 1.0 / length], dim=1).numpy()


def restate(rows, row_start, ids, item_of, lmax, max_len, normalize, tef, eps=1e-5):
    """float64 restatement of xml_gather_feature_rows on the host -> (features f64 with exact f32 TEF columns, mask, len)"""
    rows = np.asarray(rows, dtype=np.float64)
    d = rows.shape[1]
    n_items = len(row_start) - 1
    out = np.zeros((len(ids), lmax, d + 2 * tef), np.float64)
    mask = np.zeros((len(ids), lmax), np.float32)
    lens = np.zeros(len(ids), np.int32)
    for i, e in enumerate(ids):
        if item_of is not None:
            if not 0 <= e < len(item_of):
                continue
            e = int(item_of[e])
        if not 0 <= e < n_items:
            continue
        n = int(min(row_start[e + 1] - row_start[e], max_len, lmax))
        x = rows[row_start[e]:row_start[e] + n]
        if normalize:
            x = x / (np.sqrt((x * x).sum(-1, keepdims=True)) + eps)
        out[i, :n, :d] = x
        if tef:
            out[i, :n, d:] = tef_columns(n)
        mask[i, :n] = 1
        lens[i] = n
    return out, mask, lens


def compare(got, gmask, glen, want, wmask, wlen, d, normalize):
    """masks, lengths, padding and TEF columns exactly; features at the ingest tolerance (bitwise without normalisation)"""
    got, gmask = got.float().cpu().numpy(), gmask.cpu().numpy()
    np.testing.assert_array_equal(gmask, wmask)
    if glen is not None:
        np.testing.assert_array_equal(glen.cpu().numpy(), wlen)
    assert (got[wmask == 0] == 0).all()
    np.testing.assert_array_equal(got[..., d:], want[..., d:].astype(np.float32))
    if normalize:
        np.testing.assert_allclose(got[..., :d], want[..., :d], rtol=RTOL, atol=ATOL)
    else:
        np.testing.assert_array_equal(got[..., :d], want[..., :d].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------
# 1. + 2. the reference-made fixture; f16 stores and bf16 output
# ---------------------------------------------------------------------------------------------------------
def test_store_batches_match_the_reference_fixture(tmp_path):
    from tvretrieval_amd import train_data as td
    z, examples, st = load_collate_fixture(tmp_path)
    bsz = int(z["bsz"])
    for mode, norm in fixture_cases(z):
        store = td.DeviceTrainStore(examples, st["desc"], st["video"], st["sub"], device=DEV, **fixture_kw(z, mode, norm))
        for b in range(0, len(examples), bsz):
            ids = list(range(b, min(b + bsz, len(examples))))
            batch = store.batch(ids)
            pre = "%s/%s/batch%d/" % (mode, "norm" if norm else "raw", b // bsz)
            assert batch["st_ed_indices"].dtype == torch.int64
            np.testing.assert_array_equal(batch["st_ed_indices"].cpu().numpy(), z[pre + "st_ed_indices"])
            for tag in ("query", "video", "sub"):
                if (pre + tag + "_feat") not in z:
                    assert batch[tag + "_feat"] is None and batch[tag + "_mask"] is None
                    continue
                want, wmask = z[pre + tag + "_feat"], z[pre + tag + "_mask"]
                got = batch[tag + "_feat"]
                assert tuple(got.shape) == want.shape and got.dtype == F32
                d = want.shape[-1] - (2 if "tef" in mode and tag != "query" else 0)
                compare(got, batch[tag + "_mask"], None, want, wmask, None, d, norm)
        # the same batch at a fixed shape and from ids that are already on the device
        fixed = store.batch(torch.tensor([3, 1], dtype=torch.int32, device=DEV), lmax=40, lq=6)
        free = store.batch([3, 1])
        for k, v in free.items():
            if v is not None and v.dim() >= 2 and k != "st_ed_indices":
                assert torch.equal(fixed[k][:, :v.shape[1]], v) and not fixed[k][:, v.shape[1]:].any()
        assert torch.equal(fixed["st_ed_indices"], free["st_ed_indices"])
    with pytest.raises(IndexError):
        store.batch([0, 9])
    with pytest.raises(ValueError):
        store.batch(torch.tensor([0], dtype=torch.int32, device=DEV))


def test_f16_store_and_bf16_output(tmp_path):
    from tvretrieval_amd import train_data as td
    z, examples, st = load_collate_fixture(tmp_path, dtype="float16")
    voff = np.concatenate([[0], np.cumsum(z["vlens"])]).astype(np.int64)
    ex_item = np.array([int(e["vid_name"][4:]) for e in examples], dtype=np.int32)
    for mode, norm in (("video_sub_tef", True), ("video_sub", False)):
        tef = int("tef" in mode)
        store = td.DeviceTrainStore(examples, st["desc"], st["video"], st["sub"], device=DEV, **fixture_kw(z, mode, norm))
        assert store.res["video"].rows.dtype == torch.float16
        store16 = td.DeviceTrainStore(examples, st["desc"], st["video"], st["sub"], device=DEV, feature_dtype=BF16,
                                      **fixture_kw(z, mode, norm))
        ids = [2, 0, 5, 7, 2, 8, 4]
        batch, batch16 = store.batch(ids), store16.batch(ids)
        for tag, raw in (("video", z["raw/video"]), ("sub", z["raw/sub"])):
            rows16 = raw.astype(np.float16)
            want, wmask, _ = restate(rows16, voff, ids, ex_item, 40, 40, norm, tef)
            compare(batch[tag + "_feat"], batch[tag + "_mask"], None, want, wmask, None, raw.shape[1], norm)
            assert batch16[tag + "_feat"].dtype == BF16
            assert torch.equal(batch16[tag + "_feat"], batch[tag + "_feat"].to(BF16))
            assert torch.equal(batch16[tag + "_mask"], batch[tag + "_mask"])
        assert torch.equal(batch16["query_feat"], batch["query_feat"].to(BF16))
    with pytest.raises(ValueError, match="query_feat"):
        store16.fill(batch, ids)                        # f32 tensors offered to a bf16 request
    with pytest.raises(ValueError):
        store.fill(batch, ids[:3])                      # another batch size


# ---------------------------------------------------------------------------------------------------------
# 3. shapes where the kernel can go wrong
# ---------------------------------------------------------------------------------------------------------
ITEM_LENS = [5, 1, 9, 3]                                # an item of one row; one longer than lmax
EX_ITEM = [2, 0, 1, 3, 0]                               # example -> item


@pytest.mark.parametrize("d,sdt", [(36, torch.float16), (3072, torch.float16), (4096, F32), (40, F32), (6, F32)])
@pytest.mark.parametrize("tef", [0, 1])
def test_gather_feature_rows_paths(d, sdt, tef):
    """d = 36 f16: 72-byte rows, the scalar path; 3072 f16 / 4096 f32: several 16-byte pieces per lane; tef = 1: destination
    rows of d + 2 values (8-byte aligned f32, 4-byte aligned bf16); n = 1 and n * lmax = 7; ids -1 and n_examples."""
    from tvretrieval_amd import ops
    g = torch.Generator().manual_seed(d + tef)
    start = np.concatenate([[0], np.cumsum(ITEM_LENS)]).astype(np.int64)
    rows = (torch.randn(int(start[-1]), d, generator=g) * 0.7).to(sdt)
    rows[3] = 0                                          # an all-zero row: x / (0 + eps) stays 0
    rows_h = rows.float().numpy()
    rows_d, start_d = rows.to(DEV), torch.from_numpy(start).to(DEV)
    item_of = torch.tensor(EX_ITEM, dtype=torch.int32, device=DEV)

    def run(ids, lmax, max_len, normalize, odt=F32, use_map=True):
        ids_d = torch.tensor(ids, dtype=torch.int32, device=DEV)
        out = ops.gather_feature_rows(rows_d, start_d, ids_d, lmax, max_len, item_of=item_of if use_map else None,
                                      normalize=normalize, tef=bool(tef), out_dtype=odt)
        want = restate(rows_h, start, ids, EX_ITEM if use_map else None, lmax, max_len, normalize, tef)
        return out, want

    ids_a = [0, 4, -1, 1, 0, 5, 2, 0, 3]
    for normalize in (True, False):
        (fa, ma, la), (wf, wm, wl) = run(ids_a, 7, 8, normalize)
        assert tuple(fa.shape) == (9, 7, d + 2 * tef)
        compare(fa, ma, la, wf, wm, wl, d, normalize)
        assert la.tolist() == [7, 5, 0, 5, 7, 0, 1, 7, 3]
        assert not fa[2].any() and not fa[5].any() and not ma[2].any() and not ma[5].any()
        assert torch.equal(fa[0], fa[4]) and torch.equal(fa[0], fa[7]) and torch.equal(fa[1], fa[3])     # position independence
        if tef:
            assert float(fa[6, 0, d + 1]) == 1.0 and float(fa[6, 0, d]) == 0.0                          # an item of one row
        # bf16: the f32 result rounded to nearest even
        (fb, mb, lb), _ = run(ids_a, 7, 8, normalize, odt=BF16)
        assert fb.dtype == BF16 and torch.equal(fb, fa.to(BF16)) and torch.equal(mb, ma) and torch.equal(lb, la)
        # n = 1, n * lmax = 7 (not a multiple of the four waves of a workgroup): the same bits as position 0 of the batch of 9
        (f1, m1, l1), (w1, wm1, wl1) = run([0], 7, 8, normalize)
        compare(f1, m1, l1, w1, wm1, wl1, d, normalize)
        assert torch.equal(f1[0], fa[0])
        # another n and lmax: the rows of example 1 (5 rows) carry the same bits; example 0 is now cut by max_len
        (fc, mc, lc), (wc, wmc, wlc) = run([3, 1, 0], 12, 6, normalize)
        compare(fc, mc, lc, wc, wmc, wlc, d, normalize)
        assert lc.tolist() == [3, 5, 6] and torch.equal(fc[1, :7], fa[1]) and not fc[1, 7:].any()
        assert torch.equal(fc[2, :6, :d], fa[0, :6, :d])
        # ids as item ids
        (fi, mi_, li), (wi, wmi, wli) = run([1, 4, 3, -1, 2], 9, 9, normalize, use_map=False)
        compare(fi, mi_, li, wi, wmi, wli, d, normalize)
        assert li.tolist() == [1, 0, 3, 0, 9]
    # out= arguments: written in place, everything else of the buffers untouched
    ids_d = torch.tensor(ids_a, dtype=torch.int32, device=DEV)
    buf = torch.full((2, 9, 7, d + 2 * tef), 3.0, device=DEV)
    mbuf, lbuf = torch.full((9, 7), 3.0, device=DEV), torch.full((9,), 3, dtype=torch.int32, device=DEV)
    f, m, l = ops.gather_feature_rows(rows_d, start_d, ids_d, 7, 8, item_of=item_of, normalize=False, tef=bool(tef),
                                      out=buf[0], mask_out=mbuf, len_out=lbuf)
    assert f.data_ptr() == buf.data_ptr() and torch.equal(buf[0], fa) and bool((buf[1] == 3.0).all())
    assert torch.equal(mbuf, ma) and torch.equal(lbuf, la)


def test_gather_feature_rows_misaligned_views():
    """A source that does not start on a 16-byte boundary takes the scalar path; a destination view at an odd element offset
    takes the narrow stores: the same bits as the aligned launch."""
    from tvretrieval_amd import ops
    g = torch.Generator().manual_seed(3)
    start = torch.tensor([0, 4, 9], dtype=torch.int64, device=DEV)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    for sdt, odt in ((torch.float16, F32), (torch.float16, BF16), (F32, BF16), (F32, F32)):
        rows = torch.randn(9, 64, generator=g).to(sdt).to(DEV)
        want, wm, _ = ops.gather_feature_rows(rows, start, ids, 6, 6, out_dtype=odt)
        flat = torch.zeros(9 * 64 + 8, dtype=sdt, device=DEV)
        flat[1:1 + 9 * 64] = rows.flatten()
        got, gm, _ = ops.gather_feature_rows(flat[1:1 + 9 * 64].view(9, 64), start, ids, 6, 6, out_dtype=odt)
        assert torch.equal(gm, wm)
        if odt == F32:                                   # (another summation order: not the same bits)
            torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL)
        for off in (1, 2, 4):
            dflat = torch.full((3 * 6 * 64 + 16,), 5.0, dtype=odt, device=DEV)
            view = dflat[off:off + 3 * 6 * 64].view(3, 6, 64)
            ops.gather_feature_rows(rows, start, ids, 6, 6, out=view)
            assert torch.equal(view, want) and bool((dflat[:off] == 5.0).all()) and bool((dflat[off + 3 * 6 * 64:] == 5.0).all())


def test_gather_index_rows():
    from tvretrieval_amd import ops
    table = torch.tensor([[1, 2], [3, 1 << 40], [-5, 6], [7, 8], [9, 10]], dtype=torch.int64, device=DEV)
    ids = torch.tensor([4, 0, -1, 5, 1, 1, 2], dtype=torch.int32, device=DEV)
    got = ops.gather_index_rows(table, ids)
    assert got.tolist() == [[9, 10], [1, 2], [0, 0], [0, 0], [3, 1 << 40], [3, 1 << 40], [-5, 6]]
    out = torch.full((7, 2), 11, dtype=torch.int64, device=DEV)
    assert ops.gather_index_rows(table, ids, out=out) is out and torch.equal(out, got)
    wide = torch.arange(3 * 130, dtype=torch.int64, device=DEV).view(3, 130)
    assert torch.equal(ops.gather_index_rows(wide, torch.tensor([2, 0], dtype=torch.int32, device=DEV)), wide[[2, 0]])


# ---------------------------------------------------------------------------------------------------------
# 4. golden training steps through the store
# ---------------------------------------------------------------------------------------------------------
def stores_from_batch(tmp_path, d):
    """f32 stores of the fixture batch's own rows cut at the mask lengths, clip_length 1.0 and ts = [st, ed]: the store's
    batch(range(n)) is then the fixture batch."""
    from tvretrieval_amd import ingest
    n = d["query_feat"].shape[0]
    st = {}
    for tag, key in (("desc", "query"), ("video", "video"), ("sub", "sub")):
        lens = d[key + "_mask"].sum(1).astype(int)
        feats = {("%d" % i if tag == "desc" else "v%d" % i): d[key + "_feat"][i, :lens[i]] for i in range(n)}
        ingest.write_feature_store(str(tmp_path / tag), feats, dtype="float32")
        st[tag] = ingest.FeatureStore(str(tmp_path / tag))
    examples = [dict(desc_id=i, desc="", vid_name="v%d" % i, duration=0.0,
                     ts=[float(d["st_ed_indices"][i, 0]), float(d["st_ed_indices"][i, 1])]) for i in range(n)]
    return examples, st


def golden_optimizer(m, d):
    from tvretrieval_amd.train import BertAdam
    named = list(m.named_parameters())
    groups = [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]
    return BertAdam(groups, **json.loads(str(d["optim"])))


@pytest.mark.parametrize("name", ["train_step_video_sub_h128", "train_step_nocross_lse_h128"])
def test_golden_train_steps_through_the_store(tmp_path, name):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import GraphedTrainStep, train_step
    d, cfg, _ = load_golden(name)
    examples, st = stores_from_batch(tmp_path, d)
    n = len(examples)
    store = td.DeviceTrainStore(examples, st["desc"], st["video"], st["sub"], max_desc_len=cfg["max_desc_l"],
                                max_ctx_len=cfg["max_ctx_l"], clip_length=1.0, ctx_mode=cfg["ctx_mode"], normalize_vfeat=False,
                                normalize_tfeat=False, device=DEV)
    batch = store.batch(range(n))
    for k in ("query_feat", "query_mask", "video_feat", "video_mask", "sub_feat", "sub_mask", "st_ed_indices"):
        assert batch[k].dtype == T(d[k]).dtype and torch.equal(batch[k], T(d[k])), k
    # three eager steps
    m = build_train_model(cfg, d)
    opt = golden_optimizer(m, d)
    for it in range(3):
        loss, _ = train_step(m, opt, dict(store.batch(range(n)), neg_ctx_rank=d["neg_ctx_rank_steps"][it],
                                          neg_q_rank=d["neg_q_rank_steps"][it]))
        print(name, "eager step", it, float(loss.detach()), float(d["step_losses"][it]))
        assert abs(float(loss.detach()) - float(d["step_losses"][it])) < 5e-5, (it, float(loss.detach()), float(d["step_losses"][it]))
    sd = m.state_dict()
    errs = sorted(((rel_err(sd[k[len("sd_after3/"):]], torch.from_numpy(v)), k) for k, v in d.items()
                   if k.startswith("sd_after3/")), reverse=True)
    print(name, "worst eager parameter errors:", errs[:3])
    assert errs[0][0] < 2e-4, errs[:5]
    # three fill + replay steps
    m = build_train_model(cfg, d)
    opt = golden_optimizer(m, d)
    step = GraphedTrainStep(m, opt, store.batch(range(n)))
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    for it in range(3):
        for v in step.static.values():
            if torch.is_tensor(v):
                v.fill_(7)                                   # whatever the buffers held: the fill rewrites all of it
        store.fill(step.static, ids)
        loss, parts = step(None, neg_ctx_rank=d["neg_ctx_rank_steps"][it], neg_q_rank=d["neg_q_rank_steps"][it])
        print(name, "graphed step", it, float(loss), float(d["step_losses"][it]))
        assert abs(float(loss.detach()) - float(d["step_losses"][it])) < 5e-5, (it, float(loss.detach()), float(d["step_losses"][it]))
    worst = max(float((p.detach().cpu() - torch.from_numpy(d["sd_after3/" + k])).abs().max()) for k, p in m.named_parameters())
    print(name, "worst graphed parameter error:", worst)
    assert worst < 2e-5, worst


# ---------------------------------------------------------------------------------------------------------
# 5. the epoch driver
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epoch_world(tmp_path_factory):
    """23 examples over 8 videos, dims 48 / 32 / 32, hidden 128, dropout probabilities 0, f32 (the golden training model's
    configuration and initial weights)."""
    from tvretrieval_amd import ingest
    tmp = tmp_path_factory.mktemp("epoch")
    d, cfg, _ = load_golden("train_step_video_sub_h128")
    cfg = dict(cfg, input_drop=0.0, drop=0.0, cross_att_drop=0.0)
    rng = np.random.default_rng(17)
    vlens = [24, 6, 17, 1, 30, 12, 24, 9]
    qlens = rng.integers(1, 15, 23)
    vid = {"v%d" % i: rng.standard_normal((l, 48)).astype(np.float32) for i, l in enumerate(vlens)}
    sub = {"v%d" % i: rng.standard_normal((l, 32)).astype(np.float32) for i, l in enumerate(vlens)}
    desc = {str(i): rng.standard_normal((int(l), 32)).astype(np.float32) for i, l in enumerate(qlens)}
    st = {}
    for tag, f, dt in (("desc", desc, "float32"), ("video", vid, "float16"), ("sub", sub, "float16")):
        ingest.write_feature_store(str(tmp / tag), f, dtype=dt)
        st[tag] = ingest.FeatureStore(str(tmp / tag))
    examples = []
    for i in range(23):
        v = int(rng.integers(0, 8))
        a = float(rng.uniform(0, vlens[v] * 1.5))
        examples.append(dict(desc_id=i, desc="", vid_name="v%d" % v, duration=vlens[v] * 1.5,
                             ts=[a, a + float(rng.uniform(0.5, 9.0))]))
    return d, cfg, examples, st


def epoch_setup(world, **cfg_kw):
    from tvretrieval_amd import train_data as td
    d, cfg, examples, st = world
    cfg = dict(cfg, **cfg_kw)
    store = td.DeviceTrainStore(examples, st["desc"], st["video"], st["sub"], max_desc_len=cfg["max_desc_l"],
                                max_ctx_len=cfg["max_ctx_l"], clip_length=1.5, ctx_mode="video_sub", device=DEV)
    m = build_train_model(cfg, d)
    return store, m, golden_optimizer(m, d), cfg


def epoch_opt(**kw):
    return types.SimpleNamespace(**dict(dict(bsz=6, grad_clip=-1, debug=False, hard_negtiave_start_epoch=-1, hard_pool_size=3,
                                             train_span_start_epoch=-1, lw_st_ed=0.01), **kw))


def test_train_epoch_eager_equals_a_hand_written_loop(epoch_world):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import train_step
    store, m1, o1, _ = epoch_setup(epoch_world)
    _, m2, o2, _ = epoch_setup(epoch_world)
    order = torch.randperm(23, generator=torch.Generator().manual_seed(3)).numpy()
    torch.manual_seed(5)
    hist = []
    avg = td.train_epoch(m1, o1, store, epoch_opt(), 0, generator=torch.Generator().manual_seed(3), history=hist)
    assert len(hist) == 4 and o1.step_count == 4
    torch.manual_seed(5)
    m2.train()
    want = []
    for b in range(0, 23, 6):
        ids = order[b:b + 6].tolist()
        batch = store.batch(ids)
        assert batch["video_feat"].shape[1] == int(store.ctx_len[ids].max())
        want.append(train_step(m2, o2, batch)[1])
    for it, (g, w) in enumerate(zip(hist, want)):
        for k in td.LOSS_KEYS:
            assert abs(g[k] - w[k]) < 5e-5, (it, k, g[k], w[k])
    for k in td.LOSS_KEYS:
        assert abs(avg[k] - float(np.mean([w[k] for w in want]))) < 5e-5
    errs = sorted(((rel_err(p1, p2), n) for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters())), reverse=True)
    print("worst parameter differences, driver vs loop:", errs[:3])
    assert errs[0][0] < 2e-4, errs[:5]
    # order= overrides the generator; opt.debug stops after four batches
    hist2 = []
    td.train_epoch(m1, o1, store, epoch_opt(bsz=4, debug=True), 0, training=False, order=np.arange(23), history=hist2)
    assert len(hist2) == 4


def test_train_epoch_without_training_changes_nothing(epoch_world):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import xml_forward_train
    store, m, o, _ = epoch_setup(epoch_world)
    before = o.flat_p.clone()
    torch.manual_seed(9)
    hist = []
    avg = td.train_epoch(m, o, store, epoch_opt(), 0, training=False, order=np.arange(23), history=hist)
    assert torch.equal(o.flat_p, before) and o.step_count == 0 and not m.training
    torch.manual_seed(9)
    with torch.no_grad():
        want = [xml_forward_train(m, **store.batch(list(range(b, min(b + 6, 23)))))[1] for b in range(0, 23, 6)]
    for g, w in zip(hist, want):
        for k in td.LOSS_KEYS:
            assert abs(g[k] - w[k]) < 5e-5, (k, g[k], w[k])
    assert abs(avg["loss_overall"] - float(np.mean([w["loss_overall"] for w in want]))) < 5e-5


def test_train_epoch_graphed_equals_eager_steps_at_the_fixed_shape(epoch_world):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import GraphedTrainStep, train_step
    store, m1, o1, cfg = epoch_setup(epoch_world)
    _, m2, o2, _ = epoch_setup(epoch_world)
    lmax, lq = cfg["max_ctx_l"], cfg["max_desc_l"]
    order = torch.randperm(23, generator=torch.Generator().manual_seed(4)).numpy()
    m1.train()
    step = GraphedTrainStep(m1, o1, store.batch(order[:6].tolist(), lmax=lmax, lq=lq))
    torch.manual_seed(6)
    hist = []
    td.train_epoch(m1, o1, store, epoch_opt(), 0, step=step, order=order, history=hist)
    assert len(hist) == 4 and o1.step_count == 4
    torch.manual_seed(6)
    m2.train()
    for it, b in enumerate(range(0, 23, 6)):
        w = train_step(m2, o2, store.batch(order[b:b + 6].tolist(), lmax=lmax, lq=lq))[1]
        for k in td.LOSS_KEYS:
            assert abs(hist[it][k] - w[k]) < 5e-5, (it, k, hist[it][k], w[k])


def test_train_epoch_switches_hard_negatives_and_span_loss_on(epoch_world):
    from tvretrieval_amd import train_data as td
    store, m, o, _ = epoch_setup(epoch_world, lw_st_ed=0.0)
    opt = epoch_opt(hard_negtiave_start_epoch=1, train_span_start_epoch=1, debug=True, bsz=5)
    torch.manual_seed(2)
    a0 = td.train_epoch(m, o, store, opt, 0, order=np.arange(23))
    assert not m.config.use_hard_negative and m.config.lw_st_ed == 0 and a0["loss_st_ed"] == 0.0 and a0["loss_neg_ctx"] > 0
    a1 = td.train_epoch(m, o, store, opt, 1, order=np.arange(23))
    assert m.config.use_hard_negative and m.config.hard_pool_size == 3 and m.config.lw_st_ed == 0.01
    assert a1["loss_st_ed"] > 0.0
    assert abs(a1["loss_overall"] - (a1["loss_st_ed"] + a1["loss_neg_ctx"] + a1["loss_neg_q"])) < 1e-5
