"""xml_ingest_pool_rows / ops.ingest_pool_rows on the GPU (include/xmlhip_ingest_pool.h): clip pooling from frame- and
word-level rows in the ingest launch, against the numpy restatement of tests/ingest_pool_ref.py -- bitwise where the arithmetic
is exact (max pooling without a norm), against float64 with the margins of tests/test_gpu_numerics.py elsewhere -- and the
feeder end to end: ContextFeeder over PooledStores against ContextFeeder over clip stores written from the restatement.
Every test prints `NUMERICS kernel regime storage: ...` lines (pytest -s)."""
import itertools

import numpy as np
import pytest
import torch

import ingest_pool_ref as REF
import large_offsets as LO
import numerics_regimes as NR
from test_gpu_kernels import DEV, dev, ops  # noqa: F401  (ops: fixture)
from test_gpu_numerics import C_CHAIN, C_ROWWISE

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SHAPES = [pytest.param(da, db, s, o, id="%dx%d-%s-%s" % (da, db, str(s).split(".")[1], str(o).split(".")[1]))
          for (da, db), s, o in itertools.product(REF.DIMS, (F16, F32), (F32, BF16))]


def run(ops, case, norms, pool, normalize, out_dtype, segs=None, want_filled=True):
    segs = case["segs"] if segs is None else segs
    sources = [(dev(torch.from_numpy(s)), dev(torch.from_numpy(g)), nm) for s, g, nm in zip(case["srcs"], segs, norms)]
    return ops.ingest_pool_rows(sources, dev(torch.from_numpy(case["row_start"])), case["n"], case["lmax"], case["max_len"],
                                pool=pool, normalize=normalize, out_dtype=out_dtype, want_filled=want_filled)


def restate(case, norms, pool, normalize, dtype, segs=None):
    return REF.restate(case["srcs"], case["segs"] if segs is None else segs, norms, case["row_start"], case["n"], case["lmax"],
                       case["max_len"], pool, normalize, dtype)


def bits(t):
    return t.contiguous().cpu().view(torch.int16 if t.element_size() == 2 else torch.int32)


def block_scale(W, dims):
    """max|W| of each (row, source block), spread over the block's columns: a normalised block next to a raw one, or a clip of
    small frames next to one of large frames, is measured against its own magnitude, not against the largest output."""
    out, col = torch.empty_like(W), 0
    for d in dims:
        out[..., col:col + d] = W[..., col:col + d].abs().amax(-1, keepdim=True)
        col += d
    return out.clamp_min(2.0 ** -126)


def check(name, regime, got, W, R, n_norms, pool, out_dtype, dims, all_normed=True):
    """(b): max pooling with one norm is the arithmetic of xml_ingest_rows (C_ROWWISE); the mean and the two-norm forms sum in
    another order than numpy (C_CHAIN).  The margin is over the float32 restatement's own distance from float64, in units of
    block_scale.  all_normed=False: some block reaches the store without a norm -- pooled f16 values (11 significand bits)
    are exact ties of the bf16 grid (8 bits) one time in eight, so the share of elements ON a rounding boundary is not small
    by construction; the helper then asserts the rounding itself and the bias, not the share."""
    c = C_ROWWISE if (pool == "max" and n_norms == 1) else C_CHAIN
    W, R = torch.from_numpy(W), torch.from_numpy(R)
    if out_dtype == F32:
        NR.check_f32(name, regime, got, W, R, c, scale=block_scale(W, dims))
    else:
        NR.check_bf16_rounding(name, regime, got, W, R, c, scale=block_scale(W, dims), cap=all_normed)


@pytest.mark.parametrize("d_a,d_b,src_dtype,out_dtype", SHAPES)
def test_pool_rows_small_shapes(ops, d_a, d_b, src_dtype, out_dtype):
    """Every edge of the small case (ingest_pool_ref.small_case) for both pools and each norm flag on and off."""
    case = REF.small_case(d_a, d_b, src_dtype)
    n_src = len(case["srcs"])
    norm_sets = [(False,) * n_src, (True,) * n_src] + ([(True, False)] if n_src == 2 else [])
    tag = "%dx%d %s" % (d_a, d_b, str(src_dtype).split(".")[1])
    lens = np.minimum(case["counts"], case["max_len"])
    want_mask = (np.arange(case["lmax"])[None] < lens[:, None]).astype(np.float32)
    for pool, norms, normalize in itertools.product(("max", "mean"), norm_sets, (False, True)):
        got, mask, filled = run(ops, case, norms, pool, normalize, out_dtype)
        again, _, _ = run(ops, case, norms, pool, normalize, out_dtype)
        assert torch.equal(bits(got), bits(again)), "two launches of the same input differ"
        R, rmask, rfilled = restate(case, norms, pool, normalize, np.float32)
        W, _, _ = restate(case, norms, pool, normalize, np.float64)
        # (c) masks and filled exact; padded rows and empty blocks exact zeros
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(rmask, want_mask)
        assert np.array_equal(filled.cpu().numpy(), rfilled)
        assert rfilled.sum() < want_mask.sum(), "the case has clips that no source fills"
        g = got.float().cpu().numpy()
        assert (g[want_mask == 0] == 0).all()
        col = 0
        for s, seg in zip(case["srcs"], case["segs"]):
            for i in range(case["n"]):
                for l in range(int(lens[i])):
                    lo, hi = seg[int(case["row_start"][i]) + l]
                    if lo == hi:
                        assert (g[i, l, col:col + s.shape[1]] == 0).all(), (i, l)
            col += s.shape[1]
        n_norms = int(any(norms)) + int(normalize)
        if pool == "max" and n_norms == 0:
            # (a) the maximum is exact in either dtype: bitwise the restatement (rounded once for bf16)
            assert torch.equal(bits(got), bits(torch.from_numpy(R).to(out_dtype))), (tag, "max without a norm is exact")
        else:
            regime = "%s %s norms=%s row=%d" % (tag, pool, "".join(str(int(x)) for x in norms), normalize)
            check("ingest_pool_rows", regime, got, W, R, n_norms, pool, out_dtype, [x.shape[1] for x in case["srcs"]],
                  all_normed=bool(normalize or all(norms)) and d_a + d_b >= 64)      # (8 and 12 columns: 1 % is 4 elements)


@pytest.mark.parametrize("d_a,d_b", REF.DIMS)
def test_single_row_segments_are_the_source_rows(ops, d_a, d_b):
    """(a): with one source row per clip, both pools and no norm hand over the source rows, widened exactly.  n = 1."""
    g = torch.Generator().manual_seed(d_a)
    dims = [d_a] + ([d_b] if d_b else [])
    srcs = [torch.randn(13, d, generator=g).half() for d in dims]
    pick = torch.tensor([12, 0, 5, 5, 7])
    seg = torch.stack([pick, pick + 1], 1)
    start = torch.tensor([0, 5])
    want = torch.cat([s[pick].float() for s in srcs], dim=1)[None]
    for pool in ("max", "mean"):
        got, mask = ops.ingest_pool_rows([(dev(s), dev(seg), False) for s in srcs], dev(start), 1, 5, 5, pool=pool,
                                         normalize=False)
        assert torch.equal(bits(got), bits(want)) and bool((mask == 1).all()), pool


@pytest.mark.parametrize("d_a,d_b", [(2048, 1024), (7, 5)])
@pytest.mark.parametrize("pool", ["max", "mean"])
def test_bad_ranges_read_nothing(ops, d_a, d_b, pool):
    """(d): out-of-range and inverted ranges give zero blocks -- the other source's block and the row norm go on as if the
    range were empty -- and filled is 0 where every source's range is bad."""
    case = REF.small_case(d_a, d_b, F16)
    bad = [REF.bad_ranges(case["segs"][0], len(case["srcs"][0])), case["segs"][1].copy()]
    for r in REF.BAD_ROWS[:2]:
        bad[1][r] = (len(case["srcs"][1]), len(case["srcs"][1]) + 1)
    empty = [g.copy() for g in bad]
    for k in range(2):
        for r in REF.BAD_ROWS:
            lo, hi = bad[k][r]
            if not 0 <= lo <= hi <= len(case["srcs"][k]):
                empty[k][r] = (0, 0)
    for norms, normalize in (((False, False), False), ((True, True), True)):
        got, mask, filled = run(ops, case, norms, pool, normalize, F32, segs=bad)
        want, wmask, wfilled = run(ops, case, norms, pool, normalize, F32, segs=empty)
        assert torch.equal(bits(got), bits(want)) and torch.equal(filled, wfilled) and torch.equal(mask, wmask)
        _, _, rfilled = restate(case, norms, pool, normalize, np.float32, segs=bad)
        assert np.array_equal(filled.cpu().numpy(), rfilled)
        g = got.cpu().numpy()
        assert (g[0, 0] == 0).all() and filled[0, 0] == 0 and (g[0, 3] == 0).all()        # both sources bad
        assert (g[0, 4, :d_a] == 0).all() and (g[0, 4, d_a:] != 0).any() and filled[0, 4] == 1


@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_rows_do_not_depend_on_batch_or_position(ops, out_dtype):
    """(e): a video's rows are bitwise the same alone, in another order, among other videos and at another lmax."""
    case = REF.small_case(2048, 1024, F16)
    kw = dict(pool="mean", normalize=True, out_dtype=out_dtype)
    norms = (True, True)
    full, _, _ = run(ops, case, norms, "mean", True, out_dtype)
    rs = case["row_start"]
    for order, lmax in (([2], 9), ([3, 2, 0], 12), ([0, 0, 3, 1, 2], 10)):
        segs = [np.concatenate([g[rs[v]:rs[v + 1]] for v in order]) for g in case["segs"]]
        start = np.concatenate([[0], np.cumsum([case["counts"][v] for v in order])]).astype(np.int64)
        sources = [(dev(torch.from_numpy(s)), dev(torch.from_numpy(g)), nm) for s, g, nm in zip(case["srcs"], segs, norms)]
        got, _ = ops.ingest_pool_rows(sources, dev(torch.from_numpy(start)), len(order), lmax, case["max_len"], **kw)
        for k, v in enumerate(order):
            ln = min(case["counts"][v], case["max_len"])
            assert torch.equal(bits(got[k, :ln]), bits(full[v, :ln])), (order, v)
            assert bool((got[k, ln:] == 0).all())


def test_wrapper_refuses_what_the_entry_refuses(ops):
    src, seg, start = torch.zeros(4, 8, device=DEV).half(), torch.zeros(2, 2, dtype=torch.int64, device=DEV), \
        torch.tensor([0, 2], device=DEV)
    with pytest.raises(ops._lib.XmlHipError, match="pool"):
        ops.ingest_pool_rows([(src, seg, True)], start, 1, 2, 2, pool="sum")
    with pytest.raises(ops._lib.XmlHipError, match="1 or 2 sources"):
        ops.ingest_pool_rows([(src, seg, True)] * 3, start, 1, 2, 2)
    with pytest.raises(ops._lib.XmlHipError, match="UNSUPPORTED|unsupported|not supported"):
        wide = torch.zeros(2, 4104, device=DEV).half()
        ops.ingest_pool_rows([(wide, seg, True)], start, 1, 2, 2)
    with pytest.raises(ops._lib.XmlHipError, match="GPU"):
        ops.ingest_pool_rows([(src.cpu(), seg, True)], start, 1, 2, 2)


# ---- past 2^31 elements ------------------------------------------------------------------------------------------------------
def test_source_past_2_31_elements(ops):
    """One f16 source of more than 2^31 elements (a frame store is corpus-sized): segments on both sides of every offset
    threshold of tests/large_offsets.py and one that straddles it, the first and the last source row, against float64 as in
    (b).  Only the sampled rows of the source are written; nothing else is read."""
    d = 768
    th = LO.thresholds(2)
    rows = th["T3"] // d + 64
    LO.assert_crosses(rows * d, 2, ("T1", "T2", "T3"))
    src = torch.empty((rows, d), dtype=F16, device=DEV)
    g = torch.Generator().manual_seed(31)
    seg = [(0, 3), (rows - 4, rows), (rows - 1, rows)]
    for t in sorted(set(th.values())):
        s = LO.straddler(t, d)                              # the source row that holds element offset t
        assert s * d <= t < (s + 1) * d and s + 6 < rows
        seg += [(s - 5, s - 1), (s - 2, s), (s - 1, s + 2), (s, s + 1), (s + 1, s + 5)]      # below, up to, across, on, above
    seg = np.array(seg, dtype=np.int64)
    host = {}
    for lo, hi in seg:
        for r in range(lo, hi):
            if r not in host:
                host[r] = (torch.randn(d, generator=g).abs() * (0.2 + (r % 7))).half()
    idx = torch.tensor(sorted(host))
    src[idx.to(DEV)] = torch.stack([host[int(r)] for r in idx]).to(DEV)
    n = 2
    start = np.array([0, 10, len(seg)], dtype=np.int64)
    lmax = int(max(np.diff(start)))
    # the restatement runs on a compacted copy of the sampled rows
    remap = {int(r): k for k, r in enumerate(idx)}
    csrc = torch.stack([host[int(r)] for r in idx]).numpy()
    cseg = np.array([[remap[int(lo)], remap[int(hi - 1)] + 1] for lo, hi in seg], dtype=np.int64)
    assert all(cseg[k, 1] - cseg[k, 0] == seg[k, 1] - seg[k, 0] for k in range(len(seg))), "sampled rows of a range are adjacent"
    for pool, norm, out_dtype in (("max", False, F32), ("mean", True, F32), ("max", True, BF16)):
        got, mask, filled = ops.ingest_pool_rows([(src, dev(torch.from_numpy(seg)), norm)], dev(torch.from_numpy(start)), n, lmax,
                                                 lmax, pool=pool, normalize=False, out_dtype=out_dtype, want_filled=True)
        R, rmask, rfilled = REF.restate([csrc], [cseg], [norm], start, n, lmax, lmax, pool, False, np.float32)
        W, _, _ = REF.restate([csrc], [cseg], [norm], start, n, lmax, lmax, pool, False, np.float64)
        assert np.array_equal(mask.cpu().numpy(), rmask) and np.array_equal(filled.cpu().numpy(), rfilled)
        if not norm:
            assert torch.equal(bits(got), bits(torch.from_numpy(R)))
        else:
            check("ingest_pool_rows", "past 2^31 %s" % pool, got, W, R, 1, pool, out_dtype, [d])
    del src
    torch.cuda.empty_cache()


# ---- the feeder end to end ---------------------------------------------------------------------------------------------------
D_RES, D_I3D, D_SUB, W_CTX = 64, 32, 48, 40


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """40 videos with TVR-like frame counts (3 feature rows per second, 20 .. 110 s) and subtitle timings; frame- and word-level
    f16 stores, and f32 CLIP stores written from the numpy restatement of the three conversion scripts."""
    from tvretrieval_amd.ingest import (FeatureStore, FeatureStoreWriter, frame_clip_boundaries, sentence_word_ranges,
                                        write_feature_store)
    tmp = tmp_path_factory.mktemp("pooled")
    rng = np.random.default_rng(17)
    b = frame_clip_boundaries()
    names = ["v%02d" % i for i in range(40)]
    frames = {k: int(rng.integers(60, 330)) for k in names}
    frames[names[0]], frames[names[1]] = 400, 4           # 89 clips: longer than W_CTX; one clip
    res = {k: np.abs(rng.standard_normal((n, D_RES))).astype(np.float16) for k, n in frames.items()}
    i3d = {k: np.abs(rng.standard_normal((n, D_I3D))).astype(np.float16) for k, n in frames.items()}
    n_clips = {k: int((b[:-1] < n).sum()) for k, n in frames.items()}
    words, wranges = {}, {}
    for k in names:
        dur = frames[k] / 3.0
        n_sub = max(1, int(dur / 3.5))
        st = np.sort(rng.uniform(0, dur, n_sub))
        sub = np.stack([st, st + rng.uniform(0.5, 4.0, n_sub)], 1)
        lens = rng.integers(0, 14, n_sub)
        words[k] = rng.standard_normal((max(int(lens.sum()), 1), D_SUB)).astype(np.float16)
        wranges[k] = sentence_word_ranges(sub, lens, n_clips[k])
    for tag, feats in (("res", res), ("i3d", i3d), ("words", words)):
        write_feature_store(str(tmp / tag), feats)
    clip_v = FeatureStoreWriter(str(tmp / "clip_v"), D_RES + D_I3D, "float32")
    clip_s = FeatureStoreWriter(str(tmp / "clip_s"), D_SUB, "float32")
    full = {}                                             # name -> the collated rows: float64 and the float32 restatement
    for k in names:
        fr = np.stack([b[:n_clips[k]], np.minimum(b[1:n_clips[k] + 1], frames[k])], 1).astype(np.int64)
        start, nc = np.array([0, n_clips[k]]), n_clips[k]
        v, _, _ = REF.restate([res[k], i3d[k]], [fr, fr], [True, True], start, 1, nc, nc, "max", False)
        s, _, _ = REF.restate([words[k]], [wranges[k]], [False], start, 1, nc, nc, "max", False)
        clip_v.add(k, v[0])
        clip_s.add(k, s[0])
        full[k] = {(tag, dt): REF.restate(srcs, segs, norms, start, 1, nc, nc, "max", True, dt)[0][0]
                   for tag, srcs, segs, norms in (("video", [res[k], i3d[k]], [fr, fr], [True, True]),
                                                  ("sub", [words[k]], [wranges[k]], [False]))
                   for dt in (np.float32, np.float64)}
    clip_v.close()
    clip_s.close()
    S = lambda t: FeatureStore(str(tmp / t))              # noqa: E731
    return dict(names=names, n_clips=n_clips, b=b, wranges=wranges, res=S("res"), i3d=S("i3d"), words=S("words"),
                clip_v=S("clip_v"), clip_s=S("clip_s"), full=full)


def _feeders(corpus, **kw):
    from tvretrieval_amd.ingest import ContextFeeder, PooledStore
    pv = PooledStore([(corpus["res"], corpus["b"], True), (corpus["i3d"], corpus["b"], True)])
    ps = PooledStore([(corpus["words"], corpus["wranges"], False)])
    a = ContextFeeder(corpus["names"], pv, ps, max_ctx_len=W_CTX, batch_size=16, device=DEV, **kw)
    b = ContextFeeder(corpus["names"], corpus["clip_v"], corpus["clip_s"], max_ctx_len=W_CTX, batch_size=16, device=DEV, **kw)
    return a, b


@pytest.mark.parametrize("with_parts", [False, True], ids=["cut", "parts"])
def test_feeder_over_pooled_stores_equals_feeder_over_clip_stores(ops, corpus, with_parts):
    """Masks equal, and both feeders' features within (b) of the float64 value of the collated rows: pooling, per-source norm
    and row norm are the two-norm form (C_CHAIN over the float32 restatement's own distance from float64).  The clip stores
    hold the restatement's pooled, per-source-normalised rows in f32, so the clip feeder adds the row norm only."""
    from tvretrieval_amd.ingest import plan_parts
    names = corpus["names"]
    counts = np.array([corpus["n_clips"][k] for k in names])
    table = plan_parts(counts, W_CTX, 8) if with_parts else None
    pooled, clips = _feeders(corpus, **(dict(parts=table) if with_parts else {}))
    assert len(pooled) == len(clips)
    if with_parts:
        assert table.n_parts > len(names)
        items = [(names[table.part_video[p]], int(table.part_offset[p]), int(table.part_len[p])) for p in range(table.n_parts)]
    else:
        items = [(k, 0, min(corpus["n_clips"][k], W_CTX)) for k in names]
    at = 0
    for (vf, vm, sf, sm), (cvf, cvm, csf, csm) in zip(pooled, clips):
        assert torch.equal(vm, cvm) and torch.equal(sm, csm) and torch.equal(vm, sm)
        assert vf.shape == cvf.shape and sf.shape == csf.shape
        batch = items[at:at + vf.shape[0]]
        at += vf.shape[0]
        assert vm.sum(1).cpu().tolist() == [ln for _, _, ln in batch]
        for tag, got, ref in (("video", vf, cvf), ("sub", sf, csf)):
            W, R = np.zeros(got.shape, np.float64), np.zeros(got.shape, np.float32)
            for i, (k, o, ln) in enumerate(batch):
                W[i, :ln], R[i, :ln] = corpus["full"][k][tag, np.float64][o:o + ln], corpus["full"][k][tag, np.float32][o:o + ln]
            W, R = torch.from_numpy(W), torch.from_numpy(R)
            NR.check_f32("pooled feeder", "%s parts=%d" % (tag, with_parts), got, W, R, C_CHAIN)
            NR.check_f32("clip feeder", "%s parts=%d" % (tag, with_parts), ref, W, R, C_CHAIN)
            assert bool((got[vm == 0] == 0).all())
    assert at == len(items)
    assert pooled.stats["rows"] > clips.stats["rows"] and pooled.stats["h2d_bytes"] > 0


def test_mutable_index_takes_the_pooled_feeder(ops, corpus):
    from test_gpu_model import _synthetic_model
    from tvretrieval_amd.index_update import MutableCorpusIndex
    m = _synthetic_model("video_sub", 128, D_RES + D_I3D, D_SUB, 128, W_CTX, F32, seed=61)[0]
    pooled, _ = _feeders(corpus)
    with torch.no_grad():
        index = MutableCorpusIndex.from_batches(m, pooled, 64)
    counts = np.array([corpus["n_clips"][k] for k in corpus["names"]])
    assert index.n_live == 40
    assert index.vlen[:40].cpu().tolist() == np.minimum(counts, W_CTX).tolist()
