"""The packed form of the updatable index (MutableCorpusIndex.create(..., tiles=N), DESIGN.md section 20 addendum) against the
plain form (tiles=None) driven through the identical sequence of operations: the device's code table and packed mask words
are the numpy model's (tests/test_block_table.py), the rows and per-slot tensors of the live slots are the plain index's,
K6 writes bitwise its scores into the live columns and nothing into the others, every search is bitwise its search.
video_sub model, max_ctx_l = 100, f32 at H = 128 and bf16 at H = 256 (the two dtypes of the tiled K6 operand), capacity 70 =
three live words, 24 tiles.

What `to_rows()` can show: the packed image holds rows [0, 16 nb) of a video, nb = ceil(valid length / 16) -- the rows K6
reads.  The plain index also holds the encoder's rows at the padded positions beyond them; these are masked columns of K6
that the packed image does not store, so the comparison is bitwise on the run's rows and `to_rows()` is zero beyond them."""
import numpy as np
import pytest
import torch

from test_block_table import ImageModel, decode_codes
from test_gpu_index_update import KEYS, KW, _bits, _model, _queries
from test_gpu_kernels import DEV
from test_gpu_model import _feats
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex, blocks_of

pytestmark = pytest.mark.gpu

CAP, TILES, L = 70, 24, 100
CASES = [pytest.param(torch.float32, 128, id="float32-h128"), pytest.param(torch.bfloat16, 256, id="bfloat16-h256")]
_BATCHES = {}


def _batch(lens, seed):
    """A context batch with these valid lengths (0: a video without a valid clip), padded to the longest; built once."""
    key = (tuple(lens), seed)
    if key not in _BATCHES:
        vf, vm = _feats(len(lens), lens, 256, 2 * seed + 1)
        sf, sm = _feats(len(lens), lens, 128, 2 * seed + 2)
        _BATCHES[key] = tuple(t.to(DEV) for t in (vf, vm, sf, sm))
    return _BATCHES[key]


class Pair(object):
    """A packed index P and the plain index R under the same calls, and the numpy model of P's tables."""

    def __init__(self, m, tiles=TILES):
        self.m = m
        self.P = MutableCorpusIndex.create(m, CAP, tiles=tiles)
        self.R = MutableCorpusIndex.create(m, CAP)
        self.model = ImageModel(tiles)
        self.masks = {}                                          # slot -> the two (lb,) host masks of its video

    def _after_put(self, slots, batch, before):
        vm, sm = batch[1].cpu().numpy(), batch[3].cpu().numpy()
        runs = [self.P.blocks.run_of(s) for s in slots]
        for s, r in zip(slots, runs):                            # the launch order of put: the moved videos' old runs first
            if s in before and before[s] != r:
                self.model.clear(*before[s])
        for i, (s, (first, nb)) in enumerate(zip(slots, runs)):
            self.model.put(s, first, nb, [vm[i], sm[i]])
            self.masks[s] = (vm[i], sm[i])
        return runs

    def add(self, lens, seed, n_clips=True):
        batch = _batch(lens, seed)
        before = self.P.blocks.runs()
        kw = dict(n_clips=list(lens)) if n_clips else {}         # the feeder's lengths, or the one read-back from the masks
        slots = self.P.add(*batch, **kw)
        assert self.R.add(*batch) == slots
        return slots, self._after_put(slots, batch, before)

    def replace(self, slots, lens, seed, n_clips=True):
        batch = _batch(lens, seed)
        before = self.P.blocks.runs()
        kw = dict(n_clips=list(lens)) if n_clips else {}
        assert self.P.replace(slots, *batch, **kw) == slots and self.R.replace(slots, *batch) == slots
        return self._after_put(slots, batch, before)

    def remove(self, slots):
        for s in slots:
            self.model.clear(*self.P.blocks.run_of(s))
            del self.masks[s]
        assert self.P.remove(slots) == slots and self.R.remove(slots) == slots

    # ---- what holds after every step ----
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
        sl = torch.as_tensor(live, device=DEV, dtype=torch.long)
        assert torch.equal(P.live, R.live)
        if not live:
            return
        for mod in P.modalities:
            assert isinstance(P.feat1n[mod], ops.TiledRows) and isinstance(R.feat1n[mod], ops.TiledRows)
            a, b = P.feat1n_rows(mod), R.feat1n_rows(mod)
            assert a.shape == b.shape == (CAP, 128, P.feat2[mod].shape[2]) and a.dtype == b.dtype
            in_run = torch.zeros((CAP, 128), dtype=torch.bool, device=DEV)
            for s in live:
                in_run[s, :16 * P.blocks.run_of(s)[1]] = True
            assert torch.equal(_bits(a[in_run]), _bits(b[in_run])), mod          # the rows K6 reads, bitwise
            assert not a[~in_run].any(), mod                                     # nothing of a video outside its run
            for name, x, y in (("feat2", P.feat2[mod], R.feat2[mod]), ("mask", P.mask[mod], R.mask[mod])):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x[sl]), _bits(y[sl])), (mod, name)
        assert torch.equal(P.vlen[sl], R.vlen[sl]) and torch.equal(P.slot_ids[sl], R.slot_ids[sl])

    def check_k6(self, nq):
        """K6 into a NaN-filled matrix: the live columns are bitwise the plain index's, no other column is written."""
        qf, qm = _queries(nq)
        outs = []
        with torch.no_grad():
            vq, sq = self.m.encode_query(qf, qm)
            for index in (self.P, self.R):
                out = torch.full((nq, CAP), float("nan"), dtype=torch.float32, device=DEV)
                mods = index.modalities
                got = ops.q2c_scores_fused([vq.contiguous(), sq.contiguous()], [index.feat1n[mod] for mod in mods],
                                           [index.mask[mod] for mod in mods], out=out, normalize_q=True)
                assert got.data_ptr() == out.data_ptr()
                outs.append(out)
            via_stage = inf.stage_q2c(self.P, dict(video=vq, sub=sq))
        live = np.zeros(CAP, dtype=bool)
        live[self.P.table.live_slots()] = True
        lv = torch.from_numpy(live).to(DEV)
        assert not torch.isnan(outs[1]).any()
        assert torch.equal(_bits(outs[0][:, lv]), _bits(outs[1][:, lv]))
        assert torch.isnan(outs[0][:, ~lv]).all(), "K6 wrote the column of a slot that holds no video"
        assert torch.equal(_bits(via_stage[:, lv]), _bits(outs[1][:, lv]))

    def check_searches(self, nq=12):
        qf, qm = _queries(nq)
        allow = np.random.default_rng(7).random((nq, CAP)) < 0.6
        for akw in ({}, dict(video_allow=inf.pack_video_allow(torch.from_numpy(allow).to(DEV)))):
            with torch.no_grad():
                got = inf.vcmr_search(self.m, self.P, qf, qm, **KW, **akw)
                want = inf.vcmr_search(self.m, self.R, qf, qm, **KW, **akw)
            for k in KEYS:
                assert torch.equal(_bits(got[k]), _bits(want[k])), (k, sorted(akw))


# lengths 16 | 17 (blocks 0 | 1, 2: one mask word shared by two videos of one call), 100 (7 blocks from block 3: a straddle),
# 1, a video without a valid clip, and more; slots 0..8 share a live word
FIRST = [16, 17, 100, 1, 0, 6, 40, 64, 33]


def _steps(pair):
    """The sequence; yields a name after every step."""
    slots, runs = pair.add(FIRST, 1)
    assert slots == list(range(9)) and runs[:3] == [(0, 1), (1, 2), (3, 7)]
    assert pair.P.blocks.stats()["straddles"] >= 1
    yield "first batch: two videos in one mask word, all in one live word"
    rng = np.random.default_rng(5)
    for seed, n in ((2, 7), (3, 9), (4, 9)):                     # 34 live slots: the second live word; lengths read from the masks
        pair.add([int(x) for x in rng.integers(6, 101, n)], seed, n_clips=(seed != 3))
    yield "three more batches (one without n_clips)"
    batch = _batch([37, 90, 12], 6)                              # the far end: the third live word, by put
    before = pair.P.blocks.runs()
    pair.P.put([63, 64, 69], pair.P.encode(*batch), n_clips=[37, 90, 12])
    pair.R.put([63, 64, 69], pair.R.encode(*batch))
    pair._after_put([63, 64, 69], batch, before)
    yield "put at the far end"
    hole = pair.P.blocks.run_of(2)
    pair.remove([2, 12])                                         # from the middle; slot 2 is the straddling 100-clip video
    yield "remove from the middle"
    slots, runs = pair.add([97], 7)
    assert slots == [2] and runs == [hole], "a 7-block video takes the lowest free slot and the 7-block hole"
    yield "add into the hole"
    keep = pair.P.blocks.run_of(6)
    assert pair.replace([6], [35], 8) == [keep] and keep[1] == 3                       # 40 -> 35 clips: 3 blocks still
    yield "same-size replace"
    old, kept5 = pair.P.blocks.run_of(7), pair.P.blocks.run_of(5)
    new = pair.replace([7, 5], [90, 9], 9, n_clips=False)                               # 64 -> 90 clips: 4 -> 6 blocks; 6 -> 9: kept
    assert new[0] != old and new[0][1] == 6 and new[1] == kept5
    yield "replace that moves"
    first, nb = pair.P.blocks.run_of(2)
    assert first % 16 < 8 < first % 16 + nb
    pair.remove([2])
    yield "remove of a straddling video"


@pytest.mark.parametrize("dtype,h", CASES)
def test_device_tables_rows_and_slot_state(dtype, h):
    m = _model(dtype, L, h)
    pair = Pair(m)
    assert pair.P.n_videos == CAP and pair.P.lpad == 128 and tuple(pair.P.codes.shape) == (2 * TILES, 8)
    assert (pair.P.codes == -2).all() and pair.P.feat1n["video"].plan.n_tiles == TILES
    es = 4 if dtype == torch.float32 else 2
    assert pair.P.feat1n["video"].data.numel() * es == TILES * 256 * h * es < pair.R.feat1n["video"].data.numel() * es
    assert pair.P.hbm_bytes() < pair.R.hbm_bytes()
    ptrs = [pair.P.codes.data_ptr(), pair.P.live.data_ptr()] + [pair.P.feat1n[mod].data.data_ptr() for mod in pair.P.modalities]
    pair.check_tables()
    n = 0
    for name in _steps(pair):
        pair.check_tables()
        n += 1
    assert n == 8 and pair.P.n_live == 35
    assert ptrs == [pair.P.codes.data_ptr(), pair.P.live.data_ptr()] + [pair.P.feat1n[mod].data.data_ptr() for mod in pair.P.modalities]


@pytest.mark.parametrize("dtype,h", CASES)
def test_k6_writes_the_live_columns_only(dtype, h):
    m = _model(dtype, L, h)
    pair = Pair(m)
    pair.check_k6(37)                                            # the empty index: every block is unused
    for name in _steps(pair):
        pair.check_k6(37)
    pair.check_k6(300)                                           # two query tiles
    # a whole empty tile between occupied ones: five 7-block videos fill tiles 0, 0, 1, 1, 2; the two of tile 1 leave
    gap = Pair(m)
    slots, runs = gap.add([100, 97, 99, 98, 100], 11)
    assert [r[0] // 16 for r in runs] == [0, 0, 1, 1, 2]
    gap.remove([2, 3])
    assert (gap.P.codes.view(-1, 16)[1] == -2).all() and (gap.P.codes.view(-1, 16)[[0, 2]] >= 0).any(1).all()
    gap.check_tables()
    gap.check_k6(37)
    gap.check_k6(300)


@pytest.mark.parametrize("dtype,h", CASES)
def test_searches_equal_the_plain_index(dtype, h):
    m = _model(dtype, L, h)
    pair = Pair(m)
    qf, qm = _queries(8)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(m, pair.P, 8, qf.shape[1], qf.shape[2], **KW)      # captured on the EMPTY index
    for name in _steps(pair):
        pair.check_searches()
    out = g(qf, qm)                                              # no re-capture: n_tiles and every pointer are what they were
    with torch.no_grad():
        want = inf.vcmr_search(m, pair.R, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(out[k]), _bits(want[k])), k
    ti = out["top_indices"].cpu().numpy()
    assert (ti >= 0).all() and np.isin(ti, pair.P.table.live_slots()).all()


def _state(index):
    t = [index.codes, index.live, index.vlen, index.slot_ids] + [index.mask_bits[m] for m in index.modalities] + \
        [index.mask[m] for m in index.modalities] + [index.feat1n[m].data for m in index.modalities]
    return [x.clone() for x in t], index.table.live_slots(), index.blocks.runs(), index.blocks.free_runs(), index.n_live


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]


def test_refusals_leave_device_and_table_unchanged():
    m = _model(torch.float32, L, 128)
    index = MutableCorpusIndex.create(m, CAP, tiles=2)
    assert index.add(*_batch([100, 97, 99, 98], 11), n_clips=[100, 97, 99, 98]) == [0, 1, 2, 3]      # 28 of 32 blocks
    two = _batch([30, 20], 12)
    enc = index.encode(*two)
    torch.cuda.synchronize()
    before = _state(index)
    bf16_h128 = _model(torch.bfloat16, L, 128)                   # bf16 rows of 128: the K6 operand is row-major
    for call, match in ((lambda: index.add(*_batch([100], 13), n_clips=[100]), "no room for a video of 7 blocks"),
                        (lambda: index.add(*_batch([100], 13)), "4 free blocks of 32, the largest free run holds 2"),
                        # a replace that would move: freeing the two 7-block runs (tiles 0 and 1) leaves no 8 blocks in a row
                        (lambda: index.replace([0, 2], *_batch([100, 100], 17), n_clips=[128, 128]), "no room for a video of 8 blocks"),
                        (lambda: index.add(*two, n_clips=[30, 129]), "0..128"),
                        (lambda: index.add(*two, n_clips=[30, -1]), "0..128"),
                        (lambda: index.add(*two, n_clips=[30]), "valid lengths"),
                        (lambda: index.put([5, 5], enc, n_clips=[30, 20]), "duplicate slots"),
                        (lambda: index.put([5, CAP], enc, n_clips=[30, 20]), "outside"),
                        (lambda: MutableCorpusIndex.create(bf16_h128, CAP, tiles=TILES), "tiles=None"),
                        (lambda: MutableCorpusIndex.create(m, CAP, tiles=0), "positive"),
                        (lambda: MutableCorpusIndex.create(m, CAP, tiles=TILES, exact_filter=True), "exact-rank"),
                        (lambda: MutableCorpusIndex.create(m, CAP, tiles=TILES, parts=object()), "parts"),
                        (lambda: MutableCorpusIndex.create(m, CAP, tiles=TILES, video_offset=CAP), "shard")):
        with pytest.raises(ValueError, match=match):
            call()
        torch.cuda.synchronize()
        assert _same(_state(index), before), match
    # a n_clips SHORTER than the batch's padded width allows is legal: two 2-block videos still find room
    assert index.put([5, 6], enc, n_clips=[30, 20]) == [5, 6] and index.n_live == 6
    assert index.blocks.run_of(5) == (14, 2) and index.blocks.run_of(6) == (30, 2)


@pytest.mark.parametrize("dtype,h", CASES)
def test_a_short_n_clips_truncates_the_video_consistently(dtype, h):
    """n_clips = 20 for a mask of 45 clips (a caller's error): the video is indexed with the EFFECTIVE mask, the first
    2 blocks = 32 clips of it -- packed bits, mask row and vlen agree, and its scores and the search are those of the plain
    index that was handed the same encoded rows under that truncated mask."""
    m = _model(dtype, L, h)
    P, R = MutableCorpusIndex.create(m, CAP, tiles=TILES), MutableCorpusIndex.create(m, CAP)
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
        assert int(P.mask[mod][0].sum()) == 32 and torch.equal(P.mask[mod][:3], R.mask[mod][:3])
        words = P.mask_bits[mod].view(-1).cpu().numpy().view(np.uint32)
        assert first % 2 == 0 and words[first // 2] == 0xFFFFFFFF
    assert int(P.vlen[0]) == 32 and torch.equal(P.vlen[:3], R.vlen[:3])
    qf, qm = _queries(12)
    with torch.no_grad():
        vq, sq = m.encode_query(qf, qm)
        a = inf.stage_q2c(P, dict(video=vq, sub=sq))
        b = inf.stage_q2c(R, dict(video=vq, sub=sq))
        got, want = inf.vcmr_search(m, P, qf, qm, **KW), inf.vcmr_search(m, R, qf, qm, **KW)
    assert torch.equal(_bits(a[:, :3]), _bits(b[:, :3]))
    for k in KEYS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k


def test_from_batches_and_hbm_bytes_follow_the_packed_form():
    m = _model(torch.float32, L, 128)
    lens = [[16, 17, 100, 1, 0], [50, 64]]
    batches = [_batch(lens[0], 15), _batch(lens[1], 16)]
    ids = [500 + i for i in range(7)]
    P = MutableCorpusIndex.from_batches(m, batches, CAP, ids=ids, n_clips=lens[0] + lens[1], tiles=TILES)
    Q = MutableCorpusIndex.from_batches(m, batches, CAP, ids=ids, tiles=TILES)          # lengths from the masks
    R = MutableCorpusIndex.from_batches(m, batches, CAP, ids=ids)
    assert P.blocks.runs() == Q.blocks.runs() and torch.equal(P.codes, Q.codes) and P.slot_of(503) == 3
    for mod in P.modalities:
        assert torch.equal(P.mask_bits[mod], Q.mask_bits[mod]) and torch.equal(_bits(P.feat1n[mod].data), _bits(Q.feat1n[mod].data))
    assert torch.equal(P.slot_ids[:7].cpu(), torch.tensor(ids, dtype=torch.int32))
    per = lambda ix: sum(t.numel() * t.element_size() for t in list(ix.feat2.values()) + list(ix.mask.values()))      # noqa: E731
    k6 = 2 * TILES * 256 * 128 * 4
    assert P.hbm_bytes() == per(P) + k6 + 2 * (2 * TILES * 4 * 4) + P.codes.numel() * 4 + (CAP + CAP + 3) * 4
    assert P.hbm_bytes() < R.hbm_bytes()
