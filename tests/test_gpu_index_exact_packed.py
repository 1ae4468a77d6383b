"""Exact-rank mode with the packed filter image (MutableCorpusIndex.create(..., exact_rank=True, filter_tiles=N); DESIGN.md
section 20f) against the exact-rank index with the plain per-slot filter image (exact_rank=True alone), which the suite holds
to the one-shot builder (tests/test_gpu_index_exact.py).  Both are driven through the sequence of operations of
tests/test_gpu_index_packed.py (two videos in one mask word, a straddling 100-clip video, a video with no valid clip, put at
the far end, remove, add into the hole, same-size replace, moving replace, lengths read from the masks); after every step the
device's code table and packed mask words are the numpy model's, the filter rows inside the runs, every per-slot operand and
the running bound are bitwise the plain index's, K6 writes bitwise its values into the live columns and nothing else, and
every search is bitwise its search.  Shapes of the two files: capacity 70 = three live words, 24 tiles, max_ctx_l = 100, a
video_sub model at H = 256 (the smallest hidden size whose bf16 rows have a tile image) in both exact modes, 20 candidates
per query for the 10 best of 70 slots, so the filter really filters."""
import numpy as np
import pytest
import torch

from test_block_table import ImageModel, decode_codes
from test_gpu_index_exact import _models, _parts
from test_gpu_index_packed import CAP, L, TILES, Pair, _batch, _steps
from test_gpu_index_update import KEYS, KW, _bits, _queries
from test_gpu_kernels import DEV
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex, blocks_of

pytestmark = pytest.mark.gpu

H = 256
MODES = ["f32", "f16s"]


def _model(mode):
    return _models(L, H)[mode == "f16s"]


def _create(m, **kw):
    index = MutableCorpusIndex.create(m, CAP, exact_rank=True, **kw)
    index.exact.n_candidates = 20
    return index


def _slot_tensors(index, mod):
    """Everything an exact-rank index holds per slot for one modality."""
    return [index.mask[mod], index.exact.err_rows[mod]] + _parts(index.feat2[mod]) + _parts(index.exact.feat1n_f32[mod])


class ExactPair(Pair):
    """The packed-filter index P and the plain exact-rank index R under the same calls, and the numpy model of P's tables."""

    def __init__(self, mode, tiles=TILES, **kw):
        self.m = _model(mode)
        self.P = _create(self.m, filter_tiles=tiles, **kw)
        self.R = _create(self.m)
        assert self.P.exact.mode == self.R.exact.mode == mode
        self.model = ImageModel(tiles)
        self.masks = {}

    def check_tables(self):
        P, R = self.P, self.R
        live = P.table.live_slots()
        assert live == R.table.live_slots() == sorted(self.masks) and sorted(P.blocks.runs()) == live
        codes = P.codes.cpu().numpy()
        assert codes.shape == (2 * P.blocks.n_tiles, 8) and (codes == self.model.code_table()).all()
        assert decode_codes(codes) == P.blocks.runs()
        for i, mod in enumerate(P.modalities):
            assert P.feat1n[mod].mask_bits is P.mask_bits[mod] and P.feat1n[mod].plan.slot_ids is P.codes
            assert (P.mask_bits[mod].cpu().numpy() == self.model.words(i)).all(), mod
        assert torch.equal(P.live, R.live)
        assert torch.equal(_bits(P.exact.e_c_dev), _bits(R.exact.e_c_dev))       # every row's norm, whatever the run
        if not live:
            return
        sl = torch.as_tensor(live, device=DEV, dtype=torch.long)
        for mod in P.modalities:
            assert isinstance(P.feat1n[mod], ops.TiledRows) and isinstance(R.feat1n[mod], ops.TiledRows)
            a, b = P.feat1n_rows(mod), R.feat1n_rows(mod)
            assert a.shape == b.shape == (CAP, 128, H) and a.dtype == b.dtype == torch.bfloat16
            in_run = torch.zeros((CAP, 128), dtype=torch.bool, device=DEV)
            for s in live:
                in_run[s, :16 * P.blocks.run_of(s)[1]] = True
            assert torch.equal(_bits(a[in_run]), _bits(b[in_run])), mod          # the rows the filter reads, bitwise
            assert not a[~in_run].any(), mod                                     # nothing of a video outside its run
            for x, y in zip(_slot_tensors(P, mod), _slot_tensors(R, mod)):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x[sl]), _bits(y[sl])), mod
        assert torch.equal(P.vlen[sl], R.vlen[sl]) and torch.equal(P.slot_ids[sl], R.slot_ids[sl])

    def check_k6(self, nq):
        """The filter pass into a NaN-filled matrix: the live columns are bitwise the plain index's, no other is written."""
        qf, qm = _queries(nq)
        outs = []
        with torch.no_grad():
            q_hi = [ops.round_bf16_rows_err(ops.l2norm_rows(q.contiguous()))[0] for q in self.m.encode_query(qf, qm)]
            for index in (self.P, self.R):
                out = torch.full((nq, CAP), float("nan"), dtype=torch.float32, device=DEV)
                mods = index.modalities
                got = ops.q2c_scores_fused(q_hi, [index.feat1n[mod] for mod in mods], [index.mask[mod] for mod in mods], out=out)
                assert got.data_ptr() == out.data_ptr()
                outs.append(out)
        lv = torch.zeros(CAP, dtype=torch.bool)
        lv[self.P.table.live_slots()] = True
        lv = lv.to(DEV)
        assert not torch.isnan(outs[1]).any()
        assert torch.equal(_bits(outs[0][:, lv]), _bits(outs[1][:, lv]))
        assert torch.isnan(outs[0][:, ~lv]).all(), "the filter wrote the column of a slot that holds no video"


@pytest.mark.parametrize("mode", MODES)
def test_tables_rows_bound_filter_and_searches_after_every_step(mode):
    pair = ExactPair(mode)
    P, R = pair.P, pair.R
    assert P.n_videos == CAP and P.lpad == 128 and tuple(P.codes.shape) == (2 * TILES, 8) and (P.codes == -2).all()
    assert P.feat1n["video"].plan.n_tiles == TILES and P.feat1n["video"].data.numel() == TILES * 256 * H
    assert isinstance(P.feat2["video"], ops.SplitRows) == (mode == "f16s") and not P.auto_compact
    # only the filter image and its tables differ: the packed image, (2 N, 4) mask words and the code table are counted
    k6, words = lambda ix: sum(ix.feat1n[m].data.numel() * 2 for m in ix.modalities), lambda ix: sum(t.numel() * 4 for t in ix.mask_bits.values())   # noqa: E731,E501
    assert k6(P) == 2 * TILES * 256 * H * 2 < k6(R) and words(P) == 2 * 2 * TILES * 4 * 4
    assert P.hbm_bytes() - R.hbm_bytes() == k6(P) - k6(R) + words(P) - words(R) + P.codes.numel() * 4 < 0
    qf, qm = _queries(8)
    g = None
    if mode == "f16s":
        with torch.no_grad():
            g = inf.GraphedVcmrSearch(pair.m, P, 8, qf.shape[1], qf.shape[2], **KW)       # captured on the EMPTY index
    ptrs = lambda: [P.codes.data_ptr(), P.live.data_ptr(), P.exact.e_c_dev.data_ptr()] + \
        [t.data_ptr() for mod in P.modalities for t in [P.feat1n[mod].data, P.mask_bits[mod]] + _slot_tensors(P, mod)]   # noqa: E731
    before = ptrs()
    pair.check_tables()
    pair.check_k6(37)                                            # the empty index: every block is unused
    n = 0
    for name in _steps(pair):
        pair.check_tables()
        pair.check_k6(37)
        pair.check_searches()
        n += 1
    assert n == 8 and P.n_live == 35 and ptrs() == before
    pair.check_k6(300)                                           # two query tiles
    with torch.no_grad():
        out = inf.vcmr_search(pair.m, P, qf, qm, **KW)
    assert int(out["exact"]["n_candidates"]) == 20 and out["exact"]["q2c_filter"].shape == (8, CAP)
    if g is None:
        return
    # the captured search: updates, then holes and a compaction -- no re-capture, n_tiles and every pointer are what they were
    for step in range(2):
        with torch.no_grad():
            want = inf.vcmr_search(pair.m, R, qf, qm, **KW)
        got = g(qf, qm)
        for k in KEYS:
            assert torch.equal(_bits(got[k]), _bits(want[k])), (k, step)
        ti = got["top_indices"].cpu().numpy()
        assert (ti >= 0).all() and np.isin(ti, P.table.live_slots()).all()
        if step == 0:
            gone = [s for s in P.table.live_slots() if s % 3 == 1]
            pair.remove(gone)
            done = P.compact()
            assert done["blocks_moved"] > 0 and ptrs() == before


@pytest.mark.parametrize("mode", MODES)
def test_a_short_n_clips_truncates_the_video_consistently(mode):
    """n_clips = 20 for a mask of 45 clips (a caller's error): the video is indexed with the EFFECTIVE mask, the first
    2 blocks = 32 clips of it -- packed bits, mask row, vlen and filter rows agree; the re-score rows, feat2 and the error
    norms are written whole, so the search is that of the plain exact index handed the same rows under the truncated mask."""
    m = _model(mode)
    P, R = _create(m, filter_tiles=TILES), _create(m)
    batch = _batch([45, 30, 64], 14)
    enc = P.encode(*batch)
    P.put([0, 1, 2], enc, n_clips=[20, 30, 64])
    cut = {mod: (f1, f2, mk.clone()) for mod, (f1, f2, mk) in enc.items()}
    for mod in cut:
        cut[mod][2][0, 32:] = 0
    R.put([0, 1, 2], cut)
    assert P.blocks.run_of(0)[1] == 2 == blocks_of(20)
    first = P.blocks.run_of(0)[0]
    for mod in P.modalities:
        assert int(P.mask[mod][0].sum()) == 32
        words = P.mask_bits[mod].view(-1).cpu().numpy().view(np.uint32)
        assert first % 2 == 0 and words[first // 2] == 0xFFFFFFFF
        a, b = P.feat1n_rows(mod), R.feat1n_rows(mod)
        assert torch.equal(_bits(a[0, :32]), _bits(b[0, :32])) and not a[0, 32:].any() and bool(b[0, 32:45].any())
        for x, y in zip(_slot_tensors(P, mod), _slot_tensors(R, mod)):           # rows 32..44 too: err_rows and the bound follow
            assert torch.equal(_bits(x[:3]), _bits(y[:3])), mod
        assert bool((P.exact.err_rows[mod][0, 32:45] > 0).all())
    assert int(P.vlen[0]) == 32 and torch.equal(P.vlen[:3], R.vlen[:3])
    assert torch.equal(_bits(P.exact.e_c_dev), _bits(R.exact.e_c_dev))
    qf, qm = _queries(12)
    with torch.no_grad():
        got, want = inf.vcmr_search(m, P, qf, qm, **KW), inf.vcmr_search(m, R, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k


def _churned(mode, **kw):
    """Twelve 3-block and six 7-block videos, five of them removed again: holes in tiles 0, 1 and 3."""
    pair = ExactPair(mode, **kw)
    pair.add([40] * 12, 21)
    pair.add([100] * 6, 22)
    pair.remove([1, 3, 5, 7, 13])
    return pair


@pytest.mark.parametrize("mode", MODES)
def test_compaction_changes_no_search_no_bound_and_no_pointer(mode):
    pair = _churned(mode)
    P, m = pair.P, pair.m
    qf, qm = _queries(12)
    allow = inf.pack_video_allow(torch.from_numpy(np.random.default_rng(9).random((12, CAP)) < 0.6).to(DEV))

    def searches():
        with torch.no_grad():
            return [inf.vcmr_search(m, P, qf, qm, **KW, **akw) for akw in ({}, dict(video_allow=allow))]
    want = [{k: o[k].clone() for k in KEYS} for o in searches()]
    bound = P.exact.e_c_dev.clone()
    state = [t.clone() for mod in P.modalities for t in _slot_tensors(P, mod)] + [P.vlen.clone(), P.live.clone()]
    ptrs = [P.codes.data_ptr(), P.exact.e_c_dev.data_ptr()] + [P.feat1n[mod].data.data_ptr() for mod in P.modalities]
    version = P.version
    done = P.compact()
    assert done["blocks_moved"] > 0 and done["rounds"] >= 1
    assert done["bytes_moved"] == done["blocks_moved"] * 16 * 2 * H * 2         # bf16 filter rows of two modalities
    assert decode_codes(P.codes.cpu().numpy()) == P.blocks.runs() and P.version == version
    for got, ref in zip(searches(), want):
        for k in KEYS:
            assert torch.equal(_bits(got[k]), _bits(ref[k])), k
    assert torch.equal(_bits(P.exact.e_c_dev), _bits(bound))
    now = [t for mod in P.modalities for t in _slot_tensors(P, mod)] + [P.vlen, P.live]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(now, state))      # the per-slot state is no operand of a move
    assert ptrs == [P.codes.data_ptr(), P.exact.e_c_dev.data_ptr()] + [P.feat1n[mod].data.data_ptr() for mod in P.modalities]
    with torch.no_grad():                                                        # and the plain exact index agrees
        ref = inf.vcmr_search(m, pair.R, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(want[0][k]), _bits(ref[k])), k


def test_auto_compact_and_from_batches():
    m = _model("f16s")
    index = _create(m, filter_tiles=1, auto_compact=True)
    assert index.auto_compact
    index.add(*_batch([40] * 5, 23), n_clips=[40] * 5)                           # 15 of 16 blocks
    index.remove([1, 3])                                                         # 7 free blocks, the largest run holds 3
    assert index.blocks.largest_free_run() == 3
    assert index.add(*_batch([100], 24), n_clips=[100]) == [1]                   # compacts, then finds its 7 blocks
    assert index.blocks.run_of(1) == (9, 7) and index.blocks.free_blocks == 0
    with pytest.raises(ValueError, match="no room"):
        index.add(*_batch([6], 25), n_clips=[6])
    with pytest.raises(ValueError, match="compact"):
        _create(m).compact()
    lens = [[16, 17, 100, 1, 0], [50, 64]]
    batches = [_batch(lens[0], 15), _batch(lens[1], 16)]
    ids = [500 + i for i in range(7)]
    kw = dict(ids=ids, exact_rank=True, filter_tiles=TILES)
    A = MutableCorpusIndex.from_batches(m, batches, CAP, n_clips=lens[0] + lens[1], **kw)
    B = MutableCorpusIndex.from_batches(m, batches, CAP, **kw)                   # lengths from the masks
    assert A.blocks.runs() == B.blocks.runs() and torch.equal(A.codes, B.codes) and A.slot_of(503) == 3
    for mod in A.modalities:
        assert torch.equal(A.mask_bits[mod], B.mask_bits[mod]) and torch.equal(_bits(A.feat1n[mod].data), _bits(B.feat1n[mod].data))
    assert torch.equal(A.slot_ids[:7].cpu(), torch.tensor(ids, dtype=torch.int32))


@pytest.mark.parametrize("mode", MODES)
def test_the_other_entry_points_take_the_index(mode):
    """stage_video_topk, vcmr_search_host and video_subset on the packed-filter index: what they give on the plain exact index,
    and the search through a subset view is the search under the view's allow row."""
    pair = _churned(mode)
    P, R, m = pair.P, pair.R, pair.m
    qf, qm = _queries(12)
    live = P.table.live_slots()
    members = live[::2]
    allowed = torch.zeros(CAP, dtype=torch.bool)
    allowed[members] = True
    allow = inf.pack_video_allow(allowed.to(DEV))
    with torch.no_grad():
        qvec = dict(zip(("video", "sub"), m.encode_query(qf, qm)))
        for akw in ({}, dict(video_allow=allow)):
            a = inf.stage_video_topk(m, P, qvec, max_vcmr_video=10, **akw)
            b = inf.stage_video_topk(m, R, qvec, max_vcmr_video=10, **akw)
            assert a[0] is None and a[3] is not None              # no f32 score matrix: the exact-rank chain ran
            for x, y in zip(a[1:3], b[1:3]):
                assert torch.equal(_bits(x), _bits(y)), sorted(akw)
    host = dict(query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory(), max_vcmr_video=10, max_before_nms=40)
    for akw in ({}, dict(video_allow=allow)):
        with torch.no_grad():
            rec, cnt = inf.vcmr_search_host(m, P, **host, **akw)
            rec, cnt = rec.copy(), cnt.copy()
            wrec, wcnt = inf.vcmr_search_host(m, R, **host, **akw)
        assert (cnt > 0).all() and (cnt == wcnt).all()
        for q in range(12):
            assert rec[q, :cnt[q]].tobytes() == wrec[q, :wcnt[q]].tobytes(), (q, sorted(akw))
    view = inf.video_subset(P, members)
    assert view.form == "packed" and view.dtype == torch.bfloat16 and torch.equal(view.allow, allow)
    with torch.no_grad():
        got = inf.vcmr_search(m, P, qf, qm, subset=view, **KW)
        want = inf.vcmr_search(m, P, qf, qm, video_allow=view.allow, **KW)
        ref = inf.vcmr_search(m, R, qf, qm, video_allow=allow, **KW)
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(want[k])) and torch.equal(_bits(got[k]), _bits(ref[k])), k
    ti, n = got["top_indices"].cpu().numpy(), min(10, len(members))
    assert np.isin(ti[:, :n], members).all() and (ti[:, n:] == -1).all()         # fewer than K members: empty slots
    P.compact()                                                                  # moves blocks, changes no video: the view stays valid
    with torch.no_grad():
        again = inf.vcmr_search(m, P, qf, qm, subset=view, **KW)
    for k in KEYS:
        assert torch.equal(_bits(again[k]), _bits(want[k])), k


@pytest.mark.parametrize("mode", MODES)
def test_a_nan_row_raises_the_cell_to_inf_and_the_lists_stay(mode):
    pair = ExactPair(mode)
    pair.add([40, 64, 17, 100, 33, 80], 31)
    P, R, m = pair.P, pair.R, pair.m
    cool = P.exact.e_c_dev.clone()
    batch = _batch([30, 24], 32)
    enc = P.encode(*batch)
    enc["video"][0][1, 3, 5] = float("nan")                      # inside the run of the second video
    P.put([10, 11], enc, n_clips=[30, 24])
    R.put([10, 11], enc)
    for index in (P, R):
        ex = index.exact
        assert float(ex.e_c_dev[0]) == float("inf") and bool(torch.isnan(ex.err_rows["video"][11, 3]))
        assert bool(torch.isfinite(ex.e_c_dev[1])) and float(ex.e_c_dev[1]) >= float(cool[1])
    assert torch.equal(_bits(P.exact.e_c_dev), _bits(R.exact.e_c_dev))
    bad = torch.zeros(CAP, dtype=torch.bool)
    bad[11] = True
    ok = inf.pack_video_allow((~bad).to(DEV))
    qf, qm = _queries(12)
    with torch.no_grad():
        hot = inf.vcmr_search(m, P, qf, qm, video_allow=ok, **KW)
        want = inf.vcmr_search(m, R, qf, qm, video_allow=ok, **KW)
    assert int(hot["exact"]["fail"].sum()) == 12 and bool((hot["exact"]["eps"] == float("inf")).all())
    for k in KEYS:
        assert torch.equal(_bits(hot[k]), _bits(want[k])), k
    for index in (P, R):                                         # removing the slot and tightening ends it, on both alike
        index.remove([11])
        index.tighten_error_bound()
    assert bool(torch.isfinite(P.exact.e_c_dev).all()) and torch.equal(_bits(P.exact.e_c_dev), _bits(R.exact.e_c_dev))
    with torch.no_grad():
        after, ref = inf.vcmr_search(m, P, qf, qm, **KW), inf.vcmr_search(m, R, qf, qm, **KW)
    assert bool(torch.isfinite(after["exact"]["eps"]).all()) and torch.equal(after["exact"]["fail"], ref["exact"]["fail"])
    for k in KEYS:
        assert torch.equal(_bits(after[k]), _bits(hot[k])), k
