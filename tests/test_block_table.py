"""Host side of the packed form of the updatable index (index_update.BlockTable): which run of 16-row blocks of the packed K6
image every live slot owns.  Pure bookkeeping, no GPU.  Also the numpy MODEL of what the two packed update kernels leave in
the code table and the packed mask words (include/xmlhip_index.h) -- tests/test_gpu_index_packed.py compares it with the
device after every step; here it is checked against the structure xml_q2c_scores_packed relies on."""
import json
import os

import numpy as np
import pytest
import torch

from tvretrieval_amd import ops
from tvretrieval_amd.index_update import BlockTable, blocks_of


# ---- the numpy model of the put / clear kernels' tables -----------------------------------------------------------------------
class ImageModel(object):
    """codes (n_tiles * 16,) one per block, bits[m] (n_tiles * 16,) the 16 mask bits of every block, per modality."""

    def __init__(self, n_tiles, n_mod=2):
        self.n_tiles = n_tiles
        self.codes = np.full(n_tiles * 16, -2, dtype=np.int64)
        self.bits = [np.zeros(n_tiles * 16, dtype=np.int64) for _ in range(n_mod)]

    @staticmethod
    def effective(mask, nb):
        """(lb,) 0/1 batch mask -> the (128,) bools the kernel indexes: the batch mask AND clip < 16 nb"""
        m = np.zeros(128, dtype=bool)
        m[:len(mask)] = np.asarray(mask) != 0
        m[16 * nb:] = False
        return m

    def put(self, slot, first, nb, masks):
        assert 1 <= nb <= 8 and first // 16 == (first + nb - 1) // 16 and 0 <= first and first + nb <= self.n_tiles * 16
        for k in range(nb):
            g = first + k
            self.codes[g] = slot if k == nb - 1 else (-3 if g % 16 == 7 else -1)
            for m, mask in enumerate(masks):
                self.bits[m][g] = int((self.effective(mask, nb)[16 * k:16 * k + 16].astype(np.int64) << np.arange(16)).sum())

    def clear(self, first, nb):
        self.codes[first:first + nb] = -2
        for b in self.bits:
            b[first:first + nb] = 0

    def code_table(self):
        return self.codes.reshape(2 * self.n_tiles, 8).astype(np.int32)

    def words(self, m):
        """(2 n_tiles, 4) int32: a block is half a word, the odd block the upper half"""
        w = (self.bits[m][0::2] | (self.bits[m][1::2] << 16)).astype(np.uint32)
        return w.view(np.int32).reshape(2 * self.n_tiles, 4)


def decode_codes(codes):
    """{slot: (first, nb)} from a code table, asserting what xml_q2c_scores_packed relies on: a run is -1 ... -1 slot inside
    one tile, -3 stands at block 7 of a tile exactly where the run goes on into block 8."""
    codes = np.asarray(codes).reshape(-1, 16)
    runs = {}
    for t in range(codes.shape[0]):
        b = 0
        while b < 16:
            if codes[t, b] == -2:
                b += 1
                continue
            start = b
            while codes[t, b] in (-1, -3):
                assert (codes[t, b] == -3) == (b == 7), (t, b)
                b += 1
                assert b < 16, "a run leaves its tile"
            slot = int(codes[t, b])
            assert slot >= 0 and slot not in runs
            runs[slot] = (t * 16 + start, b - start + 1)
            assert b - start + 1 <= 8
            b += 1
    return runs


# ---- a driver that does what MutableCorpusIndex does with a BlockTable ----------------------------------------------------------
class Driver(object):
    def __init__(self, n_tiles, capacity):
        self.table, self.model, self.capacity = BlockTable(n_tiles), ImageModel(n_tiles, 1), capacity
        self.length = {}                                        # slot -> valid length
        self.log = []

    def snapshot(self):
        return (self.table.runs(), self.table.free_runs(), self.table.free_blocks, self.table.stats(), dict(self.length))

    def put(self, slots, lens):
        before = self.snapshot()
        try:
            runs, clears = self.table.check_put(slots, [blocks_of(n) for n in lens])
        except ValueError as e:
            assert self.snapshot() == before, "a refused call changed the table"
            self.log.append(("refused", tuple(slots)))
            return str(e)
        assert self.snapshot() == before, "check_put changed the table"
        for first, nb in clears:                                 # the launch order of MutableCorpusIndex.put
            self.model.clear(first, nb)
        for s, n, (first, nb) in zip(slots, lens, runs):
            self.model.put(s, first, nb, [np.arange(128) < n])
            self.length[s] = n
        self.table.commit_put(slots, runs)
        self.log.append(("put", tuple(slots), tuple(runs), tuple(clears)))
        return None

    def remove(self, slots):
        for (first, nb) in self.table.check_remove(slots):
            self.model.clear(first, nb)
        self.table.commit_remove(slots)
        for s in slots:
            del self.length[s]
        self.log.append(("remove", tuple(slots)))

    def check(self):
        t = self.table
        runs, free = t.runs(), t.free_runs()
        owner = np.full(t.n_tiles * 16, -1)
        for s, (first, nb) in runs.items():
            assert first // 16 == (first + nb - 1) // 16, "a run crosses a tile"
            assert nb == blocks_of(self.length[s]) == max(-(-self.length[s] // 16), 1) and 1 <= nb <= 8
            assert (owner[first:first + nb] == -1).all(), "two live runs overlap"
            owner[first:first + nb] = s
        assert sorted(runs) == sorted(self.length)
        is_free = np.zeros(t.n_tiles * 16, dtype=bool)
        for first, n in free:
            assert n >= 1 and first // 16 == (first + n - 1) // 16 and not is_free[first:first + n].any()
            is_free[first:first + n] = True
            # maximal: freed neighbours have coalesced -- the blocks on both sides (inside the tile) are taken
            assert first % 16 == 0 or owner[first - 1] >= 0
            assert (first + n) % 16 == 0 or owner[first + n] >= 0
        assert (is_free == (owner < 0)).all() and t.free_blocks == int(is_free.sum())
        st = t.stats()
        assert st["free_blocks"] == t.free_blocks and st["live_runs"] == len(runs)
        assert st["largest_free_run"] == max([n for _, n in free] or [0]) == t.largest_free_run()
        assert st["tiles_empty"] + st["tiles_partial"] + st["tiles_full"] == t.n_tiles
        assert st["straddles"] == sum(1 for f, nb in runs.values() if f % 16 < 8 < f % 16 + nb)
        # the model's code table says the same, and the map for to_rows() follows the table
        assert decode_codes(self.model.codes) == runs
        rm = t.row_map().numpy()
        want = np.full(t.n_tiles * 256, -1)
        for s, (first, nb) in runs.items():
            want[first * 16:(first + nb) * 16] = s * 128 + np.arange(nb * 16)
        assert rm.dtype == np.int32 and (rm == want).all()
        for g in range(t.n_tiles * 16):
            if owner[g] >= 0:
                k = g - runs[owner[g]][0]
                n_valid = min(max(self.length[owner[g]] - 16 * k, 0), 16)
                assert self.model.bits[0][g] == (1 << n_valid) - 1
            else:
                assert self.model.bits[0][g] == 0 and self.model.codes[g] == -2


def _random_sequence(n_tiles, seed, steps=120):
    rng = np.random.default_rng(seed)
    capacity = n_tiles * 5
    d = Driver(n_tiles, capacity)
    refused = 0
    for _ in range(steps):
        live = sorted(d.length)
        free = [s for s in range(capacity) if s not in d.length]
        op = rng.choice(["add", "add", "remove", "replace", "mixed"])
        if op == "add" and free:
            k = int(rng.integers(1, min(4, len(free)) + 1))
            refused += d.put(free[:k], [int(x) for x in rng.integers(0, 129, k)]) is not None
        elif op == "remove" and live:
            k = int(rng.integers(1, min(3, len(live)) + 1))
            d.remove([int(s) for s in rng.choice(live, k, replace=False)])
        elif op == "replace" and live:
            k = int(rng.integers(1, min(3, len(live)) + 1))
            slots = [int(s) for s in rng.choice(live, k, replace=False)]
            lens = [d.length[s] if rng.random() < 0.3 else int(rng.integers(0, 129)) for s in slots]      # some keep their size
            refused += d.put(slots, lens) is not None
        elif op == "mixed" and live and free:
            refused += d.put([live[0], free[0]], [int(x) for x in rng.integers(1, 129, 2)]) is not None
        d.check()
    return d, refused


@pytest.mark.parametrize("n_tiles", [1, 3, 12])
def test_random_sequences_keep_every_invariant(n_tiles):
    total = 0
    for seed in range(4):
        d, refused = _random_sequence(n_tiles, 100 * n_tiles + seed)
        total += refused
        again, _ = _random_sequence(n_tiles, 100 * n_tiles + seed)
        assert d.log == again.log and d.table.runs() == again.table.runs(), "the same sequence placed differently"
    assert total > 0, "no call was refused: the refusal path was not exercised"


def test_placement_rule():
    t = BlockTable(2)
    runs, clears = t.check_put([0, 1, 2], [3, 8, 6])
    # the shortest free run that holds the video comes first: slot 1 goes behind slot 0 (13 free blocks) and straddles blocks
    # 7 | 8, the empty tile 1 (16) is opened by slot 2, which finds only 5 blocks left in tile 0
    assert runs == [(0, 3), (3, 8), (16, 6)] and clears == [] and t.runs() == {}
    t.commit_put([0, 1, 2], runs)
    assert t.free_runs() == [(11, 5), (22, 10)] and t.stats()["straddles"] == 1
    r, _ = t.check_put([3], [5])
    assert r == [(11, 5)]
    t.commit_put([3], r)
    # a replace that changes the block count frees its run first: slot 4 reuses blocks of slot 1's old run
    r, clears = t.check_put([1, 4], [2, 6])
    assert clears == [(3, 8)] and r == [(3, 2), (5, 6)]
    t.commit_put([1, 4], r)
    # the same block count keeps the run
    assert t.check_put([1], [2]) == ([(3, 2)], [])
    r, _ = t.check_put([5], [7])
    assert r == [(22, 7)]
    t.commit_put([5], r)
    assert t.free_runs() == [(29, 3)] and t.stats()["straddles"] == 2 and t.stats()["tiles_full"] == 1
    # freed neighbours are one run
    t.commit_remove([1])
    assert t.free_runs() == [(3, 2), (29, 3)]
    t.commit_remove([4])
    assert t.free_runs() == [(3, 8), (29, 3)]
    t.commit_remove([0])
    t.commit_remove([3])
    assert t.free_runs() == [(0, 16), (29, 3)] and t.stats()["tiles_empty"] == 1 and t.stats()["largest_free_run_partial"] == 3
    # refused as a whole: the first two videos of the call would have found room (what is free when the third asks is named)
    with pytest.raises(ValueError, match=r"4 blocks .*3 free blocks of 32, the largest free run holds 3"):
        t.check_put([6, 7, 8], [8, 8, 4])
    assert t.free_runs() == [(0, 16), (29, 3)] and 6 not in t.runs()
    # of two free runs of one length the one in which the video does not straddle, else the lowest
    u = BlockTable(2)
    r, _ = u.check_put([0, 1, 2, 3, 4], [6, 4, 6, 8, 4])
    assert r == [(0, 6), (6, 4), (10, 6), (16, 8), (24, 4)]
    u.commit_put([0, 1, 2, 3, 4], r)
    u.commit_remove([1])
    assert u.free_runs() == [(6, 4), (28, 4)]
    assert u.check_put([5], [3])[0] == [(28, 3)] and u.check_put([5], [2])[0] == [(6, 2)] and u.check_put([5], [4])[0] == [(28, 4)]
    for bad in ([0], [9]):
        with pytest.raises(ValueError, match="1..8 blocks"):
            t.check_put([9], bad)
    with pytest.raises(ValueError, match="distinct"):
        t.check_put([9, 9], [1, 1])
    with pytest.raises(ValueError, match="no run"):
        t.check_remove([0])
    with pytest.raises(ValueError):
        blocks_of(129)
    assert [blocks_of(n) for n in (0, 1, 16, 17, 100, 128)] == [1, 1, 1, 2, 7, 8]


def test_model_of_the_kernels_tables():
    m = ImageModel(2)
    ragged = np.zeros(40)
    ragged[[0, 5, 33]] = 1                                       # holes do not shorten a video: 34 clips, 3 blocks
    m.put(7, 6, 3, [np.ones(40), ragged])                        # blocks 6, 7, 8 of tile 0: a straddle
    m.put(9, 9, 1, [np.ones(100), np.zeros(100)])                # a mask longer than its run: cut at 16 clips
    assert m.codes[:11].tolist() == [-2] * 6 + [-1, -3, 7, 9, -2]
    assert decode_codes(m.codes) == {7: (6, 3), 9: (9, 1)}
    w0, w1 = m.words(0).view(np.uint32), m.words(1).view(np.uint32)
    assert w0.shape == (4, 4) and w0[0, 3] == 0xFFFFFFFF and w0[1, 0] == 0xFFFF00FF      # word 3: blocks 6 | 7; word 4: 8 | 9
    assert w1[0, 3] == 0x00000021 and w1[1, 0] == 0x00000002
    m.clear(6, 3)
    assert decode_codes(m.codes) == {9: (9, 1)} and m.words(0).view(np.uint32)[1, 0] == 0xFFFF0000


def test_bulk_loading_the_tvr_lengths_stays_within_the_plain_layout():
    """Any two runs of <= 8 blocks fit a tile, and a tile is opened only when no free run holds the video, i.e. when every
    opened tile holds two videos already: never more than ceil(videos / 2) tiles, the plain two-slots-per-tile layout."""
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tvr_clip_count_hist.json")))
    h = np.asarray(rec["hist"])
    lens = np.maximum(np.minimum(np.repeat(np.arange(len(h)), h), 128), 1)
    lens = np.random.default_rng(2018).permutation(lens)         # corpus order (tests/test_pack_plan.py)
    nv = len(lens)
    bound = (nv + 1) // 2
    t = BlockTable(bound)
    for r in range(0, nv, 200):
        slots = list(range(r, min(r + 200, nv)))
        runs, clears = t.check_put(slots, [blocks_of(n) for n in lens[r:r + 200]])
        assert not clears
        t.commit_put(slots, runs)
        assert t.tiles_used() <= (len(t.runs()) + 1) // 2
    used = t.tiles_used()
    assert used <= bound and t.stats()["live_runs"] == nv
    plan = ops.PackPlan([(torch.arange(128)[None] < torch.as_tensor(lens)[:, None]).float()])
    print("TVR clip counts, %d videos: BlockTable bulk load uses %d tiles, PackPlan %d (ratio %.4f), plain layout %d; "
          "%d straddles" % (nv, used, plan.n_tiles, used / plan.n_tiles, bound, t.stats()["straddles"]))
