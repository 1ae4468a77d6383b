"""Compaction of the packed form of the updatable index on the host (index_update.BlockTable.check_compact /
commit_compact): the planner against a numpy MODEL of xml_index_move_blocks_packed
(include/xmlhip_index_compact.h) and a checker of that entry's launch contract.  No GPU;
tests/test_gpu_index_compact.py replays the same plans on the device and compares with this model."""
import json
import os

import numpy as np
import pytest

from test_block_table import Driver, ImageModel, decode_codes
from tvretrieval_amd.index_update import BlockTable, NoRunError, blocks_of


# ---- the numpy model of the move kernel ---------------------------------------------------------------------------------------
def apply_move(model, records, content=None, order=1):
    """One xml_index_move_blocks_packed launch on an ImageModel (codes, bits per modality) and, when given, on `content` (one
    tag per block standing for its image rows): per tile everything is read before anything is written; the tiles are taken
    in record order (order=1) or in reverse (order=-1) -- under the launch contract both give the same."""
    for rec in list(records)[::order]:
        tile, src = rec[0], rec[1:]
        assert len(src) == 16
        old_codes = model.codes.copy()
        old_bits = [b.copy() for b in model.bits]
        old_content = None if content is None else content.copy()
        for b, s in enumerate(src):
            g = tile * 16 + b
            if s >= 0:
                c = old_codes[s]
                model.codes[g] = c if c >= 0 else (-3 if b == 7 else -1)
                for m in range(len(model.bits)):
                    model.bits[m][g] = old_bits[m][s]
                if content is not None:
                    content[g] = old_content[s]
            elif s == -2:
                model.codes[g] = -2
                for m in range(len(model.bits)):
                    model.bits[m][g] = 0
            else:
                assert s == -1


def check_contract(records, runs, n_tiles):
    """The launch contract of xml_index_move_blocks_packed for one launch; runs = {slot: (first, nb)} before it."""
    owner = {}
    for slot, (first, nb) in runs.items():
        for k in range(nb):
            owner[first + k] = (slot, k)
    tiles = [r[0] for r in records]
    assert len(set(tiles)) == len(tiles), "two records for one tile"
    written = set()                                              # blocks some record writes: destinations and freed ones
    for rec in records:
        assert len(rec) == 17 and 0 <= rec[0] < n_tiles
        for b, s in enumerate(rec[1:]):
            assert s in (-1, -2) or 0 <= s < 16 * n_tiles
            if s != -1:
                written.add(rec[0] * 16 + b)
    seen = set()
    for rec in records:
        tile, src = rec[0], rec[1:]
        own_sources = {s for s in src if s >= 0 and s // 16 == tile}
        placed = {}                                              # slot -> [(k, destination block)]
        for b, s in enumerate(src):
            g = tile * 16 + b
            if s != -1:
                assert g not in owner or g in own_sources, "block %d of a video is overwritten but not moved" % g
            if s >= 0:
                assert s in owner, "source block %d holds no video" % s
                assert s not in seen, "source block %d is used twice" % s
                seen.add(s)
                if s // 16 != tile:
                    assert s not in written, "cross-tile source block %d is written in the same launch" % s
                placed.setdefault(owner[s][0], []).append((owner[s][1], g))
        for slot, ks in placed.items():
            nb = runs[slot][1]
            assert [k for k, _ in ks] == list(range(nb)), "a run is mapped in part or out of order"
            assert [g for _, g in ks] == list(range(ks[0][1], ks[0][1] + nb)), "a run is not mapped to consecutive blocks"


class CompactDriver(Driver):
    """Driver + a content tag per block (what the image rows of the block hold) + compaction as MutableCorpusIndex.compact
    does it: per round the move launch, then the clear launch of the vacated runs, then the table's commit."""

    def __init__(self, n_tiles, capacity):
        Driver.__init__(self, n_tiles, capacity)
        self.content = np.full(n_tiles * 16, -1, dtype=np.int64)
        self.serial = 0

    def put(self, slots, lens):
        err = Driver.put(self, slots, lens)
        if err is None:
            for s in slots:
                first, nb = self.table.run_of(s)
                self.serial += 1
                self.content[first:first + nb] = self.serial * 16 + np.arange(nb)      # the video's rows, block by block
        return err

    def per_slot(self):
        out = {}
        for s, (first, nb) in self.table.runs().items():
            out[s] = (nb, self.model.bits[0][first:first + nb].tolist(), self.content[first:first + nb].tolist())
        return out

    def compact(self):
        t = self.table
        before, slots_before = self.snapshot(), self.per_slot()
        st0 = t.stats()
        plan = t.check_compact()
        assert self.snapshot() == before, "check_compact changed the table"
        assert t.check_compact() == plan, "the plan is not deterministic"
        old = (self.model.codes.copy(), self.model.bits[0].copy(), self.content.copy())
        touched, cleared = set(), set()
        for rnd in plan:
            runs = decode_codes(self.model.codes)                # the table as of this round
            check_contract(rnd["records"], runs, t.n_tiles)
            for slot, (was, now) in rnd["moves"].items():
                assert runs[slot] == was and was[1] == now[1]
            # the same launch with the tiles taken in the opposite order
            other, other_content = ImageModel(t.n_tiles, 1), self.content.copy()
            other.codes, other.bits = self.model.codes.copy(), [self.model.bits[0].copy()]
            apply_move(other, rnd["records"], other_content, order=-1)
            apply_move(self.model, rnd["records"], self.content, order=1)
            assert (other.codes == self.model.codes).all() and (other.bits[0] == self.model.bits[0]).all()
            assert (other_content == self.content).all(), "the launch depends on the order of its tiles"
            donors = {first // 16 for first, nb in rnd["clears"]}
            assert not donors & {r[0] for r in rnd["records"]}, "a donor tile has a record"
            assert sorted(rnd["clears"]) == sorted(r for s, r in runs.items() if r[0] // 16 in donors)
            for first, nb in rnd["clears"]:
                self.model.clear(first, nb)
            touched |= {r[0] for r in rnd["records"]}
            cleared |= donors
            want = dict(runs)
            want.update({s: now for s, (was, now) in rnd["moves"].items()})
            assert decode_codes(self.model.codes) == want
        t.commit_compact(plan)
        # ---- what holds afterwards
        assert decode_codes(self.model.codes) == t.runs()
        assert self.per_slot() == slots_before, "a video's blocks, bits or rows changed"
        st = t.stats()
        assert st["free_blocks"] == st0["free_blocks"] and st["tiles_empty"] >= st0["tiles_empty"]
        assert st["tiles_empty"] - st0["tiles_empty"] == len(cleared) and st["live_runs"] == st0["live_runs"]
        assert st["largest_free_run"] >= st0["largest_free_run"]
        owner = np.asarray([o is not None for o in t._owner]).reshape(-1, 16)
        for tile in range(t.n_tiles):
            used = int(owner[tile].sum())
            assert owner[tile, :used].all(), "tile %d: the free blocks are not one run at its end" % tile
        assert t.check_compact() == [], "a second compaction finds work"
        for tile in range(t.n_tiles):
            sl = slice(tile * 16, tile * 16 + 16)
            if tile not in touched:
                assert (self.content[sl] == old[2][sl]).all(), "rows of a tile without a record changed"
                if tile not in cleared:
                    assert (self.model.codes[sl] == old[0][sl]).all() and (self.model.bits[0][sl] == old[1][sl]).all()
        self.check()
        return plan


def _filled(n_tiles, nbs):
    """A CompactDriver with videos of these block counts in slots 0.. (one put)."""
    d = CompactDriver(n_tiles, len(nbs) + 8)
    assert d.put(list(range(len(nbs))), [16 * nb for nb in nbs]) is None
    return d


# ---- named cases --------------------------------------------------------------------------------------------------------------
def test_case_a_slide_inside_one_tile():
    d = _filled(1, [3, 5, 3, 5])                                 # lengths 48, 80, 48, 80
    t = d.table
    assert t.runs() == {0: (0, 3), 1: (3, 5), 2: (8, 3), 3: (11, 5)}
    d.remove([0, 2])
    msg = d.put([4], [96])
    assert "6 free blocks of 16, the largest free run holds 3" in msg and "compact()" in msg
    with pytest.raises(NoRunError) as e:
        t.check_put([4], [6])
    assert e.value.blocks_asked == 6 and e.value.blocks_free == 6
    assert d.model.codes.tolist() == [-2] * 3 + [-1] * 4 + [1] + [-2] * 3 + [-1] * 4 + [3]
    plan = d.compact()
    assert len(plan) == 1 and plan[0]["clears"] == []
    # slot 1 slides over its own blocks 3 and 4; slot 3 gains the straddle; blocks 11..15 held a video and are unused now
    assert plan[0]["records"] == [[0, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, -1, -2, -2, -2, -2, -2]]
    assert plan[0]["moves"] == {1: ((3, 5), (0, 5)), 3: ((11, 5), (5, 5))}
    assert t.runs() == {1: (0, 5), 3: (5, 5)} and t.free_runs() == [(10, 6)]
    assert d.model.codes.tolist() == [-1] * 4 + [1, -1, -1, -3, -1, 3] + [-2] * 6
    assert d.put([4], [96]) is None and t.run_of(4) == (10, 6)
    d.check()


def test_case_b_cross_tile_drain_loses_the_straddle():
    d = _filled(2, [5, 6, 5, 6, 4])
    t = d.table
    assert t.runs() == {0: (0, 5), 1: (5, 6), 2: (11, 5), 3: (16, 6), 4: (22, 4)}
    d.remove([0, 3])       # tile 0: 5 free blocks at its start; tile 1: one run across blocks 7 | 8 and nothing else
    assert d.model.codes[16:32].tolist() == [-2] * 6 + [-1, -3, -1, 4] + [-2] * 6
    plan = d.compact()
    assert len(plan) == 1 and plan[0]["clears"] == [(22, 4)]
    # tile 0 slid and received in ONE record (block 15 held the end of slot 2 and is unused now); tile 1, the donor, has none
    assert plan[0]["records"] == [[0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 22, 23, 24, 25, -2]]
    assert t.runs() == {1: (0, 6), 2: (6, 5), 4: (11, 4)} and t.free_runs() == [(15, 1), (16, 16)]
    # slot 1 lost its straddle, slot 2 gained one, slot 4 sits in tile 0 without a -3
    assert d.model.codes.tolist() == [-1] * 5 + [1, -1, -3, -1, -1, 2, -1, -1, -1, 4, -2] + [-2] * 16
    assert t.stats()["tiles_empty"] == 1 and t.stats()["straddles"] == 1


def test_a_packed_tile_that_receives_is_not_slid_and_a_packed_table_is_left_alone():
    d = _filled(3, [8, 3, 5, 8, 5])        # tile 0: 8 + 3 + 5, full; tile 1: 8 + 5, packed, 3 free blocks at its end
    assert d.table.runs() == {0: (0, 8), 1: (8, 3), 2: (11, 5), 3: (16, 8), 4: (24, 5)}
    assert d.compact() == []               # the one partial tile is packed and there is nowhere to drain it
    d.remove([0, 2])                       # tile 0: slot 1 alone at blocks 8..10
    plan = d.compact()
    assert len(plan) == 1 and plan[0]["records"] == [[1] + [-1] * 13 + [8, 9, 10]] and plan[0]["clears"] == [(8, 3)]
    assert d.table.runs() == {1: (29, 3), 3: (16, 8), 4: (24, 5)} and d.table.stats()["tiles_empty"] == 2


def test_no_donor_places_into_an_empty_tile_or_makes_a_receiver_overflow():
    # tiles 0, 1, 2 hold 6, 6, 12 blocks, tile 3 none: of the two tiles of 6 the higher one, tile 1, is asked first and drains
    # into tile 0 (tile 2's tail of 4 does not hold 6 blocks, the empty tile 3 is no target); tile 0, a receiver now, is no
    # donor; tile 2's 8-block run fits nowhere; the second round finds nothing
    d = _filled(4, [6, 8, 6, 8, 8, 4])
    assert d.table.runs() == {0: (0, 6), 1: (6, 8), 2: (16, 6), 3: (22, 8), 4: (32, 8), 5: (40, 4)}
    d.remove([1, 3])
    plan = d.compact()
    assert len(plan) == 1 and plan[0]["clears"] == [(16, 6)]
    assert d.table.runs() == {0: (0, 6), 2: (6, 6), 4: (32, 8), 5: (40, 4)}
    assert d.table.stats()["tiles_empty"] == 2


def test_compaction_that_cannot_help_leaves_the_refusal_and_the_table():
    d = _filled(3, [8, 7, 8, 7, 8, 7])     # every tile: one free block
    t = d.table
    assert t.free_runs() == [(15, 1), (31, 1), (47, 1)]
    assert d.compact() == []
    before = d.snapshot()
    with pytest.raises(NoRunError, match="3 free blocks of 48, the largest free run holds 1") as e:
        t.check_put([6], [2])
    assert e.value.blocks_free == 3 >= e.value.blocks_asked == 2
    assert d.snapshot() == before
    # a refusal for lack of BLOCKS says so: nothing compaction could do
    with pytest.raises(NoRunError) as e:
        t.check_put([6, 7], [2, 2])
    assert e.value.blocks_free == 3 < e.value.blocks_asked == 4
    # a stale plan is refused
    d.remove([1])
    plan = [dict(records=[], clears=[], moves={1: ((8, 7), (0, 7))})]
    with pytest.raises(ValueError, match="changed since"):
        t.commit_compact(plan)


# ---- random histories ---------------------------------------------------------------------------------------------------------
def _tvr_lengths():
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tvr_clip_count_hist.json")))
    h = np.asarray(rec["hist"])
    return np.maximum(np.minimum(np.repeat(np.arange(len(h)), h), 128), 1)


@pytest.mark.parametrize("n_tiles,steps", [(6, 400), (40, 600)])
def test_random_histories(n_tiles, steps):
    lens = _tvr_lengths()
    moved = rounds = helped = cross = 0
    for seed in range(3):
        rng = np.random.default_rng(1000 * n_tiles + seed)
        capacity = n_tiles * 6
        d = CompactDriver(n_tiles, capacity)
        for step in range(steps):
            live = sorted(d.length)
            free = [s for s in range(capacity) if s not in d.length]
            if free and (not live or rng.random() < 0.58):
                k = int(rng.integers(1, min(3, len(free)) + 1))
                new = [int(x) for x in rng.choice(lens, k)]
                msg = d.put(free[:k], new)
                if msg is not None and d.table.free_blocks >= sum(blocks_of(n) for n in new):
                    plan = d.compact()                           # what auto_compact does
                    helped += d.put(free[:k], new) is None
            elif live:
                k = int(rng.integers(1, min(3, len(live)) + 1))
                d.remove([int(s) for s in rng.choice(live, k, replace=False)])
            if step % 37 == 36:
                plan = d.compact()
                rounds += len(plan)
                moved += sum(len(r["moves"]) for r in plan)
                cross += sum(len(r["clears"]) for r in plan)
    assert moved > 0 and cross > 0 and helped > 0, (moved, cross, helped)
    print("tiles %d: %d rounds, %d runs moved (%d across tiles), %d refused puts succeeded after compaction"
          % (n_tiles, rounds, moved, cross, helped))
