"""The host table of an updatable index whose long videos are chains of slots (index_update.ChainTable; DESIGN.md section
20c) and the refusals that need no device.  DeviceTables replays the records the table produces for xml_index_set_chains:
after every call the device tables must equal the table's mirror, hold the single state in every free slot and every
one-part video, and contain no cycle."""
import numpy as np
import pytest
import torch

from tvretrieval_amd.index_update import BlockTable, ChainTable, MutableCorpusIndex, NoRunError, SlotTable
from tvretrieval_amd.ingest import plan_parts


class DeviceTables(object):
    """chain_head / chain_next / chain_offset as xml_index_set_chains leaves them."""

    def __init__(self, capacity):
        self.cap = capacity
        self.head, self.next, self.off = np.arange(capacity), np.full(capacity, -1), np.zeros(capacity, dtype=np.int64)

    def set(self, records):
        slots = [r[0] for r in records]
        assert len(set(slots)) == len(slots), "a slot twice in one launch"
        for s, h, n, o in records:
            if 0 <= s < self.cap:
                self.head[s], self.next[s], self.off[s] = h, n, o

    def check(self, t):
        for s in range(self.cap):
            assert (self.head[s], self.next[s], self.off[s]) == t.state(s), s
            if not t.is_live(s):
                assert t.state(s) == (s, -1, 0), "free slot %d is not in the single state" % s
        seen = set()
        for h in t.heads():
            chain, s = [], h
            while s != -1:
                assert s not in seen and len(chain) < t.max_parts, "a slot in two chains, a cycle or a chain over max_parts"
                seen.add(s)
                chain.append(s)
                assert t.is_live(s) and self.head[s] == h and t.id_of(s) == t.id_of(h)
                s = int(self.next[s])
            assert chain == t.chain_of(h) and self.off[h] == 0
            assert all(self.off[a] < self.off[b] for a, b in zip(chain, chain[1:]))
        assert seen == set(t.live_slots())


def _offsets(n_clips, l_ref=32, overlap=16):
    tab = plan_parts(np.asarray(n_clips), l_ref, overlap=overlap)
    gs = tab.group_start.tolist()
    return [gs[i + 1] - gs[i] for i in range(len(n_clips))], [tab.part_offset[gs[i]:gs[i + 1]].tolist() for i in range(len(n_clips))]


def _put(t, dev, n_clips, ids=None, old=None, what="add"):
    counts, offs = _offsets(n_clips)
    plan = t.check_chains(counts, offs, ids, old, what)
    dev.set(plan["records"])
    t.commit_chains(plan)
    dev.check(t)
    return plan


def _remove(t, dev, slots=None, ids=None):
    plan = t.check_remove_chains(t.resolve_videos(slots, ids, "remove"))
    dev.set(plan["records"])
    t.commit_remove_chains(plan)
    dev.check(t)
    return plan


def _snapshot(t):
    return (list(t._id), dict(t._slot), sorted(t._free), list(t._head), list(t._next), list(t._off))


def test_chains_are_handed_out_over_scattered_free_slots():
    t, dev = ChainTable(12, max_parts=8), DeviceTables(12)
    p = _put(t, dev, [20, 32, 20, 20, 20, 20], ids=[100, 101, 102, 103, 104, 105])          # six videos of one part
    assert p["heads"] == [0, 1, 2, 3, 4, 5] and p["records"] == []                         # singles never touch the tables
    assert _remove(t, dev, [1, 4])["records"] == []
    assert (t.n_live, t.n_videos_live) == (4, 4)
    p = _put(t, dev, [64], ids=[7])                                   # 64 clips at l_ref 32, overlap 16: offsets 0, 16, 32
    assert p["chains"] == [[1, 4, 6]] and p["heads"] == [1] and p["put_ids"] == [7, 7, 7]
    assert p["records"] == [[1, 1, 4, 0], [4, 1, 6, 16], [6, 1, -1, 32]]
    assert (t.n_live, t.n_videos_live) == (7, 5)
    assert t.slot_of(7) == 1 and [t.id_of(s) for s in (1, 4, 6)] == [7, 7, 7]                # id -> head; one id on every slot
    assert t.chain_of(6) == [1, 4, 6] and t.head_of(4) == 1 and t.chain_of(0) == [0]
    # two videos in one call, in call order; a single among them
    with pytest.raises(ValueError, match="already held"):            # no ids: a video gets its head slot's number, 7 is taken
        t.check_chains(*_offsets([33, 10, 48]))
    _remove(t, dev, [0])
    p = _put(t, dev, [33, 10, 48], ids=[200, 201, 202])
    assert p["chains"] == [[0, 7], [8], [9, 10]] and p["put_slots"] == [0, 7, 8, 9, 10]
    p = _put(t, dev, [5])
    assert p["heads"] == [11] and p["ids"] == [11] and t.slot_of(11) == 11
    assert t.n_live == 12
    with pytest.raises(ValueError, match="full"):
        t.check_chains([1], [[0]])


def test_remove_by_a_non_head_slot_frees_the_whole_chain_and_resets_it():
    t, dev = ChainTable(10, max_parts=8), DeviceTables(10)
    _put(t, dev, [20, 100, 20], ids=[5, 6, 8])                        # 100 clips: offsets 0 16 32 48 64 68 -> slots 1..6
    assert t.chain_of(1) == [1, 2, 3, 4, 5, 6] and t.state(6) == (1, -1, 68) and t.state(5) == (1, 6, 64)
    assert t.resolve_videos([4]) == [1] and t.resolve_videos(ids=[6]) == [1]
    with pytest.raises(ValueError, match="named twice"):
        t.resolve_videos([2, 5])
    p = _remove(t, dev, [4])
    assert sorted(p["slots"]) == [1, 2, 3, 4, 5, 6]
    assert p["records"] == [[s, s, -1, 0] for s in (1, 2, 3, 4, 5, 6)]    # every freed slot back in the single state
    assert t.live_slots() == [0, 7] and (t.n_live, t.n_videos_live) == (2, 2)
    with pytest.raises(ValueError, match="unknown video id"):
        t.slot_of(6)
    # the freed slots serve three short videos: each a single, no record needed -- the reset did it
    p = _put(t, dev, [20, 20, 20])
    assert p["heads"] == [1, 2, 3] and p["records"] == []
    for s in (1, 2, 3):
        assert t.state(s) == (s, -1, 0)


def test_replace_grows_and_shrinks_and_keeps_the_head():
    t, dev = ChainTable(10, max_parts=8), DeviceTables(10)
    _put(t, dev, [20, 20, 20, 20], ids=[40, 41, 42, 43])
    _remove(t, dev, [0])
    # grows: the single at slot 2 becomes 49 clips = offsets 0, 16, 17: its own slot, then the lowest free ones
    p = _put(t, dev, [49], old=t.resolve_videos([2], None, "replace"), what="replace")
    assert p["chains"] == [[2, 0, 4]] and p["heads"] == [2] and p["ids"] == [42] and p["surplus"] == []
    assert p["records"] == [[0, 2, 4, 16], [2, 2, 0, 0], [4, 2, -1, 17]]
    # shrinks: named by a non-head slot; the surplus slots are freed and reset
    p = _put(t, dev, [20], old=t.resolve_videos([4], None, "replace"), what="replace")
    assert p["chains"] == [[2]] and p["surplus"] == [0, 4] and p["ids"] == [42]
    assert p["records"] == [[0, 0, -1, 0], [2, 2, -1, 0], [4, 4, -1, 0]]
    assert t.live_slots() == [1, 2, 3] and t.slot_of(42) == 2
    # two videos in one call: one shrinks, the other grows into the slots the first gives up
    _put(t, dev, [48], ids=[50])                                      # slots 0, 4
    p = _put(t, dev, [10, 64], old=t.resolve_videos(ids=[50, 41]), ids=[50, 77], what="replace")
    assert p["chains"] == [[0], [1, 4, 5]] and p["surplus"] == [] and t.slot_of(77) == 1
    with pytest.raises(ValueError, match="unknown video id"):
        t.slot_of(41)
    # an id of a video that stays is refused, one of a video that leaves in the same call is free
    with pytest.raises(ValueError, match="already held"):
        t.check_chains([1], [[0]], [43], t.resolve_videos([0]), "replace")


def test_a_call_that_does_not_fit_changes_nothing():
    t, dev = ChainTable(8, max_parts=4), DeviceTables(8)
    _put(t, dev, [20, 48, 20], ids=[1, 2, 3])                         # slots 0, (1, 2), 3
    _remove(t, dev, [0])
    before = _snapshot(t)
    c64, o64 = _offsets([64, 64])
    for call, match in ((lambda: t.check_chains(c64, o64), "full"),                                       # 6 parts, 5 free slots
                        (lambda: t.check_chains(*_offsets([100])), "max_parts"),                            # 6 parts > 4
                        (lambda: t.check_chains(*_offsets([100]), old_heads=[1], what="replace"), "max_parts"),
                        (lambda: t.check_chains([2], [[0]]), "one offset per part"),
                        (lambda: t.check_chains([1, 1], [[0], [0]], [9, 9]), "duplicate video ids"),
                        (lambda: t.check_chains([1], [[0]], [3]), "already held"),
                        (lambda: t.check_chains([1], [[0]], [2 ** 31]), "int32"),
                        (lambda: t.check_chains([1, 1], [[0], [0]], [5]), "ids for"),
                        (lambda: t.check_chains([1], [[0]], None, [1, 3], "replace"), "slots for a batch"),
                        (lambda: t.resolve_videos([0], None, "remove"), "free"),
                        (lambda: t.resolve_videos([8], None, "remove"), "outside"),
                        (lambda: t.resolve_videos([1, 2], None, "remove"), "named twice"),
                        (lambda: t.resolve_videos(None, [99], "remove"), "unknown video id"),
                        (lambda: t.resolve_videos(None, None, "remove"), "slots or by ids"),
                        (lambda: t.check_put([2], None), "part of the video at head slot 1"),
                        (lambda: t.check_put([1], None), "part of the video at head slot 1")):
        with pytest.raises(ValueError, match=match):
            call()
        assert _snapshot(t) == before
    dev.check(t)
    with pytest.raises(ValueError, match="max_parts"):
        ChainTable(4, max_parts=0)


def test_slot_table_calls_still_serve_one_part_videos():
    t, dev = ChainTable(6), DeviceTables(6)
    slots, ids = t.check_add(2, [10, 11])
    t.commit_put(slots, ids)
    _put(t, dev, [40], ids=[12])
    slots, ids = t.check_put([0], [13], "replace")
    t.commit_put(slots, ids)
    t.commit_remove(t.resolve([1], None, "remove"))
    dev.check(t)
    assert t.live_slots() == [0, 2, 3] and t.slot_of(13) == 0 and (t.n_live, t.n_videos_live) == (3, 2)
    assert isinstance(t, SlotTable) and t.max_parts == 32


def test_a_call_short_of_a_block_run_leaves_both_tables_unchanged():
    """The packed form: every part takes a run of its own.  MutableCorpusIndex._find_runs with the slots a replace frees
    counted as room, on an index object that holds the two host tables only (nothing here touches a device)."""
    idx = object.__new__(MutableCorpusIndex)
    idx.blocks, idx.auto_compact, idx.table = BlockTable(2), False, ChainTable(16, max_parts=8)
    t, dev = idx.table, DeviceTables(16)

    def place(plan, n_clips):
        nbs = [max((n + 15) // 16, 1) for n in n_clips]
        if plan["surplus"]:
            idx.blocks.commit_remove(plan["surplus"])
        runs, _ = idx._find_runs(plan["put_slots"], nbs, "add")
        idx.blocks.commit_put(plan["put_slots"], runs)

    counts, offs = _offsets([40, 100, 100], l_ref=128, overlap=16)       # one part each: 3, 7 and 7 blocks
    plan = t.check_chains(counts, offs, [1, 2, 3])
    place(plan, [40, 100, 100])
    t.commit_chains(plan)
    assert idx.blocks.runs() == {0: (0, 3), 1: (3, 7), 2: (16, 7)}       # free: blocks 10..15 and 23..31
    counts, offs = _offsets([240], l_ref=128, overlap=16)                # two parts of 128 clips: 8 blocks each
    plan = t.check_chains(counts, offs, [4])
    before = (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs())
    with pytest.raises(NoRunError, match="no room"):                     # 15 free blocks; the second part finds no run
        idx._find_runs(plan["put_slots"], [8, 8], "add")
    assert (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs()) == before
    # replacing the 100-clip video at slot 1 by it: its 7 blocks count as room; nothing has changed when the check returns
    plan = t.check_chains(counts, offs, None, [1], "replace")
    assert plan["chains"] == [[1, 3]] and plan["surplus"] == []
    runs, clears = idx._find_runs(plan["put_slots"], [8, 8], "replace")
    assert runs == [(23, 8), (3, 8)] and clears == [(3, 7)]
    assert (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs()) == before
    idx.blocks.commit_put(plan["put_slots"], runs)
    dev.set(plan["records"])
    t.commit_chains(plan)
    dev.check(t)
    # a shrinking replace: the surplus slot's run is room for the call, and only for the call
    plan = t.check_chains([1, 1], [[0], [0]], None, [1, 0], "replace")
    assert plan["chains"] == [[1], [0]] and plan["surplus"] == [3]
    before = (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs())
    with pytest.raises(NoRunError):                                      # without the surplus run: blocks 0..2 and 11..15
        idx._find_runs(plan["put_slots"], [8, 8], "replace")
    assert (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs()) == before
    runs, clears = idx._find_runs(plan["put_slots"], [8, 8], "replace", freed=plan["surplus"])
    assert runs == [(23, 8), (0, 8)] and clears == [(0, 3)]
    assert (_snapshot(t), idx.blocks.runs(), idx.blocks.free_runs()) == before


def test_random_updates_never_emit_a_cycle():
    rng = np.random.RandomState(7)
    t, dev = ChainTable(40, max_parts=6), DeviceTables(40)
    next_id = 1000
    for step in range(300):
        heads = t.heads()
        op = rng.randint(3)
        try:
            if op == 0 or not heads:
                n = [int(x) for x in rng.choice([5, 32, 33, 48, 49, 80, 96], size=rng.randint(1, 4))]
                _put(t, dev, n, ids=list(range(next_id, next_id + len(n))))
                next_id += len(n)
            elif op == 1:
                pick = [int(h) for h in rng.choice(heads, size=min(len(heads), rng.randint(1, 4)), replace=False)]
                _remove(t, dev, [t.chain_of(h)[-1] for h in pick])           # named by their LAST slots
            else:
                pick = [int(h) for h in rng.choice(heads, size=min(len(heads), rng.randint(1, 3)), replace=False)]
                n = [int(x) for x in rng.choice([5, 33, 49, 96], size=len(pick))]
                p = _put(t, dev, n, old=t.resolve_videos(pick, None, "replace"), what="replace")
                assert p["heads"] == pick                                      # a replaced video keeps its head slot
        except ValueError as e:
            assert "full" in str(e)
            dev.check(t)


class _Cfg(object):
    max_ctx_l, hidden_size = 100, 128


class _Model(object):
    config, use_video, use_sub = _Cfg(), True, True
    compute_dtype = torch.float32


def test_create_refuses_before_any_allocation():
    with pytest.raises(ValueError, match="parts"):
        MutableCorpusIndex.create(_Model(), 70, parts=object())
    with pytest.raises(ValueError, match="parts"):
        MutableCorpusIndex.create(_Model(), 70, parts=object(), part_overlap=16)
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(), 70, exact_filter=True, part_overlap=16)
    with pytest.raises(ValueError, match="shard"):
        MutableCorpusIndex.create(_Model(), 70, video_offset=70, part_overlap=16)
    for bad in (100, -1, 2.5, True):
        with pytest.raises(ValueError, match="part_overlap"):
            MutableCorpusIndex.create(_Model(), 70, part_overlap=bad)
    with pytest.raises(ValueError, match="max_parts"):
        MutableCorpusIndex.create(_Model(), 70, part_overlap=16, max_parts=0)


def test_a_part_table_is_checked_against_the_index():
    idx = object.__new__(MutableCorpusIndex)
    idx.l_ref, idx.part_overlap, idx.chain_head = 32, 16, object()
    tab = plan_parts(np.asarray([20, 100, 33]), 32, overlap=16)
    counts, offs, lens = idx._part_lists(tab, 9, "add")
    assert counts == [1, 6, 2] and offs == [[0], [0, 16, 32, 48, 64, 68], [0, 1]] and lens == [20] + [32] * 8
    assert idx._part_lists(None, 3, "add") == ([1, 1, 1], [[0], [0], [0]], None)
    for table, b, match in ((plan_parts(np.asarray([20, 100]), 32, overlap=8), 8, "part_overlap = 16"),
                            (plan_parts(np.asarray([20, 100]), 48, overlap=16), 6, "l_ref = 32"),
                            (tab, 8, "9 parts"), (object(), 3, "PartTable")):
        with pytest.raises(ValueError, match=match):
            idx._part_lists(table, b, "add")
    idx.chain_head = None
    with pytest.raises(ValueError, match="without part_overlap"):
        idx._part_lists(tab, 9, "add")
