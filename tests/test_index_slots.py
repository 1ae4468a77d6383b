"""The host slot table of an index that takes updates (index_update.SlotTable) and the refusals of MutableCorpusIndex that
need no device."""
import numpy as np
import pytest
import torch

from tvretrieval_amd.index_update import MutableCorpusIndex, SlotTable


def _add(t, n, ids=None):
    slots, ids = t.check_add(n, ids)
    t.commit_put(slots, ids)
    return slots


def _remove(t, slots=None, ids=None):
    slots = t.resolve(slots, ids, "remove")
    t.commit_remove(slots)
    return slots


def test_slots_are_handed_out_lowest_free_first_and_reused():
    t = SlotTable(10)
    assert t.n_live == 0 and t.live_slots() == []
    assert _add(t, 4) == [0, 1, 2, 3]
    assert _add(t, 2) == [4, 5]
    assert _remove(t, [4, 1]) == [4, 1]
    assert t.n_live == 4 and t.live_slots() == [0, 2, 3, 5]
    assert _add(t, 3) == [1, 4, 6]                                    # the freed ones first, lowest first, then fresh ones
    _remove(t, [0])
    _remove(t, [6])
    assert _add(t, 1) == [0] and _add(t, 1) == [6]
    assert t.n_live == 7 and not t.is_live(7) and t.is_live(6)
    assert _add(t, 3) == [7, 8, 9]
    with pytest.raises(ValueError, match="full"):
        t.check_add(1)
    assert t.n_live == 10


def test_ids_map_to_slots_and_back():
    t = SlotTable(8)
    assert _add(t, 3, ids=[700, -5, 42]) == [0, 1, 2]
    assert [t.slot_of(v) for v in (700, -5, 42)] == [0, 1, 2] and t.id_of(1) == -5
    assert _add(t, 1) == [3] and t.id_of(3) == 3 and t.slot_of(3) == 3     # no id given: the slot number
    assert _remove(t, ids=[-5]) == [1]
    with pytest.raises(ValueError, match="unknown video id"):
        t.slot_of(-5)
    with pytest.raises(ValueError, match="free"):
        t.id_of(1)
    assert _add(t, 1, ids=[-5]) == [1]                                     # an id may come back, into the lowest free slot
    # a replace keeps the id unless told otherwise; a put over a live slot may hand the id on
    slots, ids = t.check_put(t.resolve(ids=[42]), None, "replace")
    assert (slots, ids) == ([2], [42])
    slots, ids = t.check_put([2, 0], [9, 42], "replace")                    # 42 moves from slot 2 to slot 0 within one call
    t.commit_put(slots, ids)
    assert t.slot_of(42) == 0 and t.slot_of(9) == 2 and t.n_live == 4
    with pytest.raises(ValueError, match="unknown video id"):
        t.slot_of(700)
    assert t.resolve(np.asarray([2, 0])) == [2, 0] and t.resolve(torch.tensor([3])) == [3] and t.resolve(1) == [1]


def test_the_table_refuses_and_stays_unchanged():
    t = SlotTable(6)
    _add(t, 4, ids=[10, 11, 12, 13])
    _remove(t, [2])
    before = (list(t._id), dict(t._slot), sorted(t._free))
    for call, match in ((lambda: t.check_put([6], None), "outside"),
                        (lambda: t.check_put([-1], None), "outside"),
                        (lambda: t.check_put([1, 3, 1], None), "duplicate slots"),
                        (lambda: t.resolve([0, 0], None, "remove"), "duplicate slots"),
                        (lambda: t.check_add(4), "full"),
                        (lambda: t.resolve([2], None, "remove"), "free"),
                        (lambda: t.resolve([5], None, "replace"), "free"),
                        (lambda: t.resolve([7], None, "replace"), "outside"),
                        (lambda: t.resolve(None, [12], "remove"), "unknown video id"),
                        (lambda: t.resolve(None, [99], "replace"), "unknown video id"),
                        (lambda: t.resolve(None, None, "remove"), "slots or by ids"),
                        (lambda: t.resolve([0], [10], "remove"), "slots or by ids"),
                        (lambda: t.check_add(2, [5, 5]), "duplicate video ids"),
                        (lambda: t.check_add(1, [10]), "already held"),
                        (lambda: t.check_add(1, [1, 2]), "ids for"),
                        (lambda: t.check_add(1, [2 ** 31]), "int32"),
                        (lambda: t.check_put([2.5], None), "integers")):
        with pytest.raises(ValueError, match=match):
            call()
        assert (list(t._id), dict(t._slot), sorted(t._free)) == before
    with pytest.raises(ValueError, match="capacity"):
        SlotTable(0)


class _Cfg(object):
    max_ctx_l, hidden_size = 100, 128


class _Model(object):
    """Just what MutableCorpusIndex.create looks at before it touches a device."""
    config, use_video, use_sub = _Cfg(), True, True

    def __init__(self, compute_dtype):
        self.compute_dtype = compute_dtype


def test_create_refuses_before_any_allocation():
    from tvretrieval_amd import ops
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(ops.F16S), 70)
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, exact_filter=True)
    with pytest.raises(ValueError, match="parts"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, parts=object())
    with pytest.raises(ValueError, match="shard"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, video_offset=70)
    with pytest.raises(ValueError, match="shard"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, n_total=140)
    with pytest.raises(ValueError, match="capacity"):
        MutableCorpusIndex.create(_Model(torch.float32), 0)
    with pytest.raises(TypeError, match="create"):
        MutableCorpusIndex()


def test_a_mutable_index_is_no_corpus_shard():
    from tvretrieval_amd import dist

    class _Idx(object):
        parts, live, n_videos = None, torch.zeros((1, 3), dtype=torch.int32), 70
    with pytest.raises(ValueError, match="corpus shard"):
        dist.check_shards(_Idx())
