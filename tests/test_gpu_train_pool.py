"""xml_gather_pool_feature_rows / ops.gather_pool_feature_rows on the GPU (include/xmlhip_train_pool.h) and DeviceTrainStore over
ingest.PooledStore: the training gather with clip pooling in the launch.  Bitwise against the parent entry
(ops.ingest_pool_rows on the host-gathered ranges of the batch), against the numpy restatement with the margins of
tests/test_gpu_ingest_pool.py, and the store end to end: against the host datasets, the golden training steps and an epoch."""
import itertools

import numpy as np
import pytest
import torch

import ingest_pool_ref as REF
import large_offsets as LO
from conftest import load_golden
from test_gpu_ingest_pool import bits, check, restate
from test_gpu_kernels import DEV, dev, ops  # noqa: F401  (ops: fixture)
from test_gpu_train import T, build_train_model, rel_err
from test_gpu_train_store import epoch_opt, epoch_world, golden_optimizer, stores_from_batch  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ITEM_OF = [2, 0, 3, 1, 2, 0, 3]
IDS = [4, 1, 6, -1, 3, 0, 7, 2]
SHAPES = [pytest.param(da, db, s, o, tef, id="%dx%d-%s-%s-tef%d" % (da, db, str(s).split(".")[1], str(o).split(".")[1], tef))
          for (da, db), s, o, tef in itertools.product(REF.DIMS, (F16, F32), (F32, BF16), (0, 1))]


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def sources_of(case, norms, segs=None):
    segs = case["segs"] if segs is None else segs
    return [(dev(torch.from_numpy(s)), dev(torch.from_numpy(g)), nm) for s, g, nm in zip(case["srcs"], segs, norms)]


def items_of(ids, item_of, n_items):
    """the item of each batch position, -1 for an id or an item out of range"""
    out = []
    for e in ids:
        if item_of is not None:
            e = item_of[e] if 0 <= e < len(item_of) else -1
        out.append(e if 0 <= e < n_items else -1)
    return out


def host_gathered(case, items):
    """row_start / seg of the batch laid back to back, as the corpus side's feeder stages them; an empty example for -1"""
    rs = case["row_start"]
    counts = [int(rs[v + 1] - rs[v]) if v >= 0 else 0 for v in items]
    segs = [np.concatenate([g[rs[v]:rs[v + 1]] if v >= 0 else g[:0] for v in items] + [np.zeros((1, 2), np.int64)])
            for g in case["segs"]]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), segs, counts


@pytest.mark.parametrize("d_a,d_b,src_dtype,out_dtype,tef", SHAPES)
def test_bitwise_the_parent_entry_on_the_gathered_ranges(ops, d_a, d_b, src_dtype, out_dtype, tef):
    case = REF.small_case(d_a, d_b, src_dtype)
    n_src, max_len = len(case["srcs"]), case["max_len"]
    d = d_a + d_b
    norm_sets = [(False,) * n_src, (True,) * n_src] + ([(True, False)] if n_src == 2 else [])
    clip_start = dev(torch.from_numpy(case["row_start"]))
    for item_of, ids in ((ITEM_OF, IDS), (None, [2, 0, 3, -1, 1, 2, 4, 0])):
        items = items_of(ids, item_of, case["n"])
        assert items.count(-1) == 2 and 1 in items and len(set(items)) < len(items)
        start, segs, counts = host_gathered(case, items)
        for lmax in (11, 5):
            lens = np.minimum(np.minimum(counts, max_len), lmax)
            assert lmax > max_len or (np.array(counts) > lmax).sum() >= 2
            want_mask = (np.arange(lmax)[None] < lens[:, None]).astype(np.float32)
            for pool, norms, normalize in itertools.product(("max", "mean"), norm_sets, (False, True)):
                got, mask, ln = ops.gather_pool_feature_rows(
                    sources_of(case, norms), clip_start, i32(ids), lmax, max_len, item_of=None if item_of is None else i32(item_of),
                    pool=pool, normalize=normalize, tef=bool(tef), out_dtype=out_dtype)
                again, amask, aln = ops.gather_pool_feature_rows(
                    sources_of(case, norms), clip_start, i32(ids), lmax, max_len, item_of=None if item_of is None else i32(item_of),
                    pool=pool, normalize=normalize, tef=bool(tef), out_dtype=out_dtype)
                want, wmask = ops.ingest_pool_rows(sources_of(case, norms, segs), dev(torch.from_numpy(start)), len(ids), lmax,
                                                   min(max_len, lmax), pool=pool, normalize=normalize, out_dtype=out_dtype,
                                                   tef=bool(tef))
                key = (item_of is None, lmax, pool, norms, normalize)
                assert got.shape == (len(ids), lmax, d + 2 * tef) and got.dtype == out_dtype
                assert torch.equal(bits(got), bits(want)), key
                assert torch.equal(bits(mask), bits(wmask)) and np.array_equal(mask.cpu().numpy(), want_mask), key
                assert ln.dtype == torch.int32 and ln.cpu().tolist() == lens.tolist(), key
                assert torch.equal(bits(got), bits(again)) and torch.equal(mask, amask) and torch.equal(ln, aln), key
                for i, v in enumerate(items):
                    if v < 0 or counts[i] == 0:
                        assert not bits(got[i]).any() and not mask[i].any(), (key, i)


def test_against_the_restatement(ops):
    """The (2048, 1024) f16 case in item order, under the arguments tests/test_gpu_ingest_pool.py uses for it."""
    case = REF.small_case(2048, 1024, F16)
    dims = [x.shape[1] for x in case["srcs"]]
    clip_start = dev(torch.from_numpy(case["row_start"]))
    for out_dtype, pool, norms, normalize in itertools.product((F32, BF16), ("max", "mean"),
                                                               ((False, False), (True, True), (True, False)), (False, True)):
        got, mask, _ = ops.gather_pool_feature_rows(sources_of(case, norms), clip_start, i32(range(case["n"])), case["lmax"],
                                                    case["max_len"], pool=pool, normalize=normalize, out_dtype=out_dtype)
        R, rmask, _ = restate(case, norms, pool, normalize, np.float32)
        W, _, _ = restate(case, norms, pool, normalize, np.float64)
        assert np.array_equal(mask.cpu().numpy(), rmask)
        n_norms = int(any(norms)) + int(normalize)
        if pool == "max" and n_norms == 0:
            assert torch.equal(bits(got), bits(torch.from_numpy(R).to(out_dtype)))
        else:
            regime = "2048x1024 float16 %s norms=%s row=%d" % (pool, "".join(str(int(x)) for x in norms), normalize)
            check("gather_pool_feature_rows", regime, got, W, R, n_norms, pool, out_dtype, dims,
                  all_normed=bool(normalize or all(norms)))


@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_a_row_does_not_depend_on_where_it_stands(ops, out_dtype):
    case = REF.small_case(2048, 1024, F16)
    clip_start = dev(torch.from_numpy(case["row_start"]))
    for tef in (False, True):
        kw = dict(item_of=i32(ITEM_OF), pool="mean", normalize=True, tef=tef, out_dtype=out_dtype)
        alone, _, l1 = ops.gather_pool_feature_rows(sources_of(case, (True, True)), clip_start, i32([0]), 9, 9, **kw)
        among, _, l8 = ops.gather_pool_feature_rows(sources_of(case, (True, True)), clip_start, i32([3, 1, 6, 2, 5, 0, 4, 1]), 11, 9,
                                                    **kw)
        assert l1.tolist() == [9] and l8.tolist()[5] == 9            # example 0 is item 2: 12 clips cut at max_len
        assert torch.equal(bits(alone[0]), bits(among[5, :9])) and not bits(among[5, 9:]).any()
        assert bits(alone[0]).any()


def test_misaligned_views(ops):
    """Sources and destination 4 bytes past an aligned address, and (7, 5) columns: the element-wise path gives the bits of
    the aligned call."""
    for (d_a, d_b), sdt, odt, tef in itertools.product(((24, 40), (7, 5)), (F16, F32), (F32, BF16), (False, True)):
        case = REF.small_case(d_a, d_b, sdt)
        clip_start = dev(torch.from_numpy(case["row_start"]))
        kw = dict(item_of=i32(ITEM_OF), pool="mean", normalize=True, tef=tef)
        want, wm, wl = ops.gather_pool_feature_rows(sources_of(case, (True, True)), clip_start, i32(IDS), 11, 9, out_dtype=odt, **kw)
        skewed = []
        for src, seg, nm in sources_of(case, (True, True)):
            off = 4 // src.element_size()
            flat = torch.zeros(src.numel() + 16, dtype=src.dtype, device=DEV)
            flat[off:off + src.numel()] = src.flatten()
            skewed.append((flat[off:off + src.numel()].view(src.shape), seg, nm))
            assert skewed[-1][0].data_ptr() % 16 == 4
        numel, off = want.numel(), 4 // want.element_size()
        dflat = torch.full((numel + 16,), 5.0, dtype=odt, device=DEV)
        view = dflat[off:off + numel].view(want.shape)
        assert view.data_ptr() % 16 == 4
        _, gm, gl = ops.gather_pool_feature_rows(skewed, clip_start, i32(IDS), 11, 9, out=view, **kw)
        key = (d_a, d_b, sdt, odt, tef)
        assert torch.equal(bits(view), bits(want)) and torch.equal(gm, wm) and torch.equal(gl, wl), key
        assert bool((dflat[:off] == 5.0).all()) and bool((dflat[off + numel:] == 5.0).all()), key


def test_source_past_2_31_elements(ops):
    """A resident f16 frame store of more than 2^31 elements -- the store's normal case: ranges on both sides of every offset
    threshold of tests/large_offsets.py and one that straddles it, the first and the last source row.  Bitwise the parent
    entry on the same ranges, and max pooling bitwise the restatement.  Only the sampled rows of the source are written."""
    d = 768
    th = LO.thresholds(2)
    rows = th["T3"] // d + 64
    LO.assert_crosses(rows * d, 2, ("T1", "T2", "T3"))
    src = torch.empty((rows, d), dtype=F16, device=DEV)
    g = torch.Generator().manual_seed(37)
    seg = [(0, 3), (rows - 4, rows), (rows - 1, rows)]
    for t in sorted(set(th.values())):
        s = LO.straddler(t, d)
        assert s * d <= t < (s + 1) * d and s + 6 < rows
        seg += [(s - 5, s - 1), (s - 2, s), (s - 1, s + 2), (s, s + 1), (s + 1, s + 5)]
    seg = np.array(seg, dtype=np.int64)
    host = {}
    for lo, hi in seg:
        for r in range(lo, hi):
            if r not in host:
                host[r] = (torch.randn(d, generator=g).abs() * (0.2 + (r % 7))).half()
    idx = torch.tensor(sorted(host))
    src[idx.to(DEV)] = torch.stack([host[int(r)] for r in idx]).to(DEV)
    clip_start = np.array([0, 10, len(seg)], dtype=np.int64)            # two items; the batch names them in the other order
    lmax = int(max(np.diff(clip_start)))
    ids = [1, 0]
    bstart = np.array([0, len(seg) - 10, len(seg)], dtype=np.int64)
    bseg = np.concatenate([seg[10:], seg[:10]])
    remap = {int(r): k for k, r in enumerate(idx)}
    csrc = torch.stack([host[int(r)] for r in idx]).numpy()
    cseg = np.array([[remap[int(lo)], remap[int(hi - 1)] + 1] for lo, hi in bseg], dtype=np.int64)
    for pool, norm, out_dtype in (("max", False, F32), ("mean", True, F32), ("max", True, BF16)):
        got, mask, ln = ops.gather_pool_feature_rows([(src, dev(torch.from_numpy(seg)), norm)], dev(torch.from_numpy(clip_start)),
                                                     i32(ids), lmax, lmax, pool=pool, normalize=False, out_dtype=out_dtype)
        want, wmask = ops.ingest_pool_rows([(src, dev(torch.from_numpy(bseg)), norm)], dev(torch.from_numpy(bstart)), 2, lmax, lmax,
                                           pool=pool, normalize=False, out_dtype=out_dtype)
        assert torch.equal(bits(got), bits(want)) and torch.equal(mask, wmask) and ln.tolist() == np.diff(bstart).tolist()
        if not norm:
            R, _, _ = REF.restate([csrc], [cseg], [norm], bstart, 2, lmax, lmax, pool, False, np.float32)
            assert torch.equal(bits(got), bits(torch.from_numpy(R)))
            assert bits(got[0, 0]).any() and bits(got[1, 1]).any()
    del src
    torch.cuda.empty_cache()


# ---- DeviceTrainStore over pooled stores -------------------------------------------------------------------------------------
@pytest.mark.parametrize("feature_dtype", [F32, BF16])
@pytest.mark.parametrize("mode", ["video_sub", "video_sub_tef"])
def test_store_batches_equal_the_collated_host_dataset(ops, tmp_path, feature_dtype, mode):
    """batch(ids) against collate of StoreTrainDataset items over the same pooled stores (two video sources, word-level
    subtitles): masks, labels, padding and the endpoint columns equal, features within the margins of the restatement test."""
    import test_pooled_store_host as H
    from tvretrieval_amd import train_data as td
    st, video, sub, _ = H.build(tmp_path)
    kw = dict(max_desc_len=H.MAX_DESC, max_ctx_len=H.MAX_CTX, clip_length=H.CLIP, ctx_mode=mode)
    store = td.DeviceTrainStore(H.EXAMPLES, st["desc"], video, sub, device=DEV, feature_dtype=feature_dtype, **kw)
    ds = td.StoreTrainDataset(H.EXAMPLES, st["desc"], video, sub, **kw)
    # float64 statement of the same rows: the pooled stores' rows in float64, then the dataset's row norm
    tef = mode.endswith("tef")
    for ids in ([0, 1, 2, 3, 4, 5], [2, 4], [5, 3, 0]):
        _, want = td.collate([ds[i] for i in ids])
        got = store.batch(ids)
        assert torch.equal(got["st_ed_indices"].cpu(), torch.from_numpy(want["st_ed_indices"]))
        for key, pstore, srcs in (("video", video, ("res", "i3d")), ("sub", sub, ("word",))):
            f, m, w = got[key + "_feat"], got[key + "_mask"], want[key + "_feat"]
            assert f.dtype == feature_dtype and tuple(f.shape) == w.shape
            assert (m.cpu().numpy() == want[key + "_mask"]).all()
            assert bool((f[m == 0] == 0).all())
            dd = pstore.dim
            if tef:
                assert (f[..., dd:].cpu() == torch.from_numpy(w[..., dd:]).to(feature_dtype)).all()
            W = np.zeros(w[..., :dd].shape, np.float64)
            for i, e in enumerate(ids):
                name = H.EXAMPLES[e]["vid_name"]
                n = min(H.CLIPS[name], H.MAX_CTX)
                segs = pstore.clip_ranges(name)
                x, _, _ = REF.restate([np.asarray(st[k][name]) for k in srcs], segs, pstore.norms, np.array([0, n]), 1, n, n, "max",
                                      True, np.float64)
                W[i, :n] = x[0]
            dims = [int(st[k].dim) for k in srcs]
            check("DeviceTrainStore pooled", "%s %s" % (key, mode), f[..., :dd].contiguous(), W, np.ascontiguousarray(w[..., :dd]),
                  1 + int(any(pstore.norms)), "max", feature_dtype, dims, all_normed=False)
    # fill rewrites every element
    ids = [3, 1, 4, 0]
    want = store.batch(ids, lmax=H.MAX_CTX + 2, lq=H.MAX_DESC + 1)
    static = {k: torch.full_like(v, 7) for k, v in want.items()}
    out = store.fill(static, ids)
    for k in want:
        assert out[k] is static[k] and torch.equal(bits(static[k]) if static[k].is_floating_point() else static[k],
                                                   bits(want[k]) if want[k].is_floating_point() else want[k]), k


def fine_store(tmp_path, tag, store, dtype):
    """`store`'s clip rows as a fine store in which clip c of every item is repeated 1 + c % 5 times, and the PooledStore
    (max pooling, no norm) that pools them back"""
    from tvretrieval_amd import ingest
    feats, ranges = {}, {}
    for name in store.index:
        a = np.asarray(store[name])
        rep = 1 + np.arange(len(a)) % 5
        feats[name] = np.repeat(a, rep, axis=0)
        hi = np.cumsum(rep)
        ranges[name] = np.stack([hi - rep, hi], axis=1).astype(np.int64)
    ingest.write_feature_store(str(tmp_path / tag), feats, dtype=dtype)
    return ingest.PooledStore([(ingest.FeatureStore(str(tmp_path / tag)), ranges, False)], pool="max")


@pytest.mark.parametrize("name", ["train_step_video_sub_h128"])
def test_golden_train_steps_through_the_pooled_store(ops, tmp_path, name):
    """The exact route: max pooling over repeated rows without a norm hands over the fixture batch bit for bit; the golden
    steps meet the limits of tests/test_gpu_train_store.py."""
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import GraphedTrainStep, train_step
    d, cfg, _ = load_golden(name)
    examples, st = stores_from_batch(tmp_path, d)
    n = len(examples)
    video, sub = fine_store(tmp_path, "fine_v", st["video"], "float32"), fine_store(tmp_path, "fine_s", st["sub"], "float32")
    store = td.DeviceTrainStore(examples, st["desc"], video, sub, max_desc_len=cfg["max_desc_l"], max_ctx_len=cfg["max_ctx_l"],
                                clip_length=1.0, ctx_mode=cfg["ctx_mode"], normalize_vfeat=False, normalize_tfeat=False, device=DEV)
    assert store.res["video"].pooled and store.res["sub"].pooled
    assert store.res["video"].sources[0][0].shape[0] > st["video"].data.shape[0]
    batch = store.batch(range(n))
    for k in ("query_feat", "query_mask", "video_feat", "video_mask", "sub_feat", "sub_mask", "st_ed_indices"):
        assert batch[k].dtype == T(d[k]).dtype and torch.equal(batch[k], T(d[k])), k
    m = build_train_model(cfg, d)
    opt = golden_optimizer(m, d)
    for it in range(3):
        loss, _ = train_step(m, opt, dict(store.batch(range(n)), neg_ctx_rank=d["neg_ctx_rank_steps"][it],
                                          neg_q_rank=d["neg_q_rank_steps"][it]))
        assert abs(float(loss.detach()) - float(d["step_losses"][it])) < 5e-5, (it, float(loss.detach()), float(d["step_losses"][it]))
    sd = m.state_dict()
    errs = sorted(((rel_err(sd[k[len("sd_after3/"):]], torch.from_numpy(v)), k) for k, v in d.items()
                   if k.startswith("sd_after3/")), reverse=True)
    assert errs[0][0] < 2e-4, errs[:5]
    m = build_train_model(cfg, d)
    opt = golden_optimizer(m, d)
    step = GraphedTrainStep(m, opt, store.batch(range(n)))
    ids = torch.arange(n, dtype=torch.int32, device=DEV)
    for it in range(3):
        for v in step.static.values():
            if torch.is_tensor(v):
                v.fill_(7)
        store.fill(step.static, ids)
        loss, parts = step(None, neg_ctx_rank=d["neg_ctx_rank_steps"][it], neg_q_rank=d["neg_q_rank_steps"][it])
        assert abs(float(loss.detach()) - float(d["step_losses"][it])) < 5e-5, (it, float(loss.detach()), float(d["step_losses"][it]))
    worst = max(float((p.detach().cpu() - torch.from_numpy(d["sd_after3/" + k])).abs().max()) for k, p in m.named_parameters())
    assert worst < 2e-5, worst


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_train_epoch_over_pooled_stores_equals_the_clip_store_epoch(ops, epoch_world, tmp_path, graphed):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.train import GraphedTrainStep
    d, cfg, examples, st = epoch_world
    video, sub = fine_store(tmp_path, "fine_v", st["video"], "float16"), fine_store(tmp_path, "fine_s", st["sub"], "float16")
    lmax, lq = cfg["max_ctx_l"], cfg["max_desc_l"]
    order = torch.randperm(23, generator=torch.Generator().manual_seed(4)).numpy()
    hists = []
    for vs, ss in ((st["video"], st["sub"]), (video, sub)):
        store = td.DeviceTrainStore(examples, st["desc"], vs, ss, max_desc_len=lq, max_ctx_len=lmax, clip_length=1.5,
                                    ctx_mode="video_sub", device=DEV)
        m = build_train_model(cfg, d)
        o = golden_optimizer(m, d)
        m.train()
        step = GraphedTrainStep(m, o, store.batch(order[:6].tolist(), lmax=lmax, lq=lq)) if graphed else None
        torch.manual_seed(6)
        hist = []
        td.train_epoch(m, o, store, epoch_opt(), 0, step=step, order=order, history=hist)
        assert o.step_count == 4
        hists.append(hist)
    assert store.res["video"].pooled and store.res["sub"].pooled
    assert len(hists[0]) == len(hists[1]) == 4
    for it, (a, b) in enumerate(zip(*hists)):
        for k in td.LOSS_KEYS:
            assert abs(a[k] - b[k]) < 5e-5, (it, k, a[k], b[k])
