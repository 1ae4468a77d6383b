"""Compaction of the packed form of the updatable index on the device (MutableCorpusIndex.compact, auto_compact;
xml_index_move_blocks_packed): the packed index P against the numpy model of its tables
(tests/test_block_table_compact.py replays the plan) and against the plain index R, which is driven through the same adds and
removes and is never compacted.  Shapes of tests/test_gpu_index_packed.py."""
import numpy as np
import pytest
import torch

from test_block_table_compact import apply_move, check_contract
from test_gpu_index_packed import CAP, CASES, L, TILES, Pair, _batch, _same, _state, _steps
from test_gpu_index_update import KEYS, KW, _bits, _model, _queries
from tvretrieval_amd import inference as inf
from tvretrieval_amd.index_update import MutableCorpusIndex

pytestmark = pytest.mark.gpu


class CPair(Pair):
    def compact(self):
        """P.compact() and the same plan on the numpy model; R is left alone.  Returns (what compact() returned, the plan)."""
        plan = self.P.blocks.check_compact()
        runs = self.P.blocks.runs()
        for rnd in plan:
            check_contract(rnd["records"], runs, self.P.blocks.n_tiles)
            runs.update({s: now for s, (was, now) in rnd["moves"].items()})
        res = self.P.compact()
        for rnd in plan:
            apply_move(self.model, rnd["records"])
            for first, nb in rnd["clears"]:
                self.model.clear(first, nb)
        assert self.P.blocks.runs() == runs
        assert res["rounds"] == len(plan) and res["blocks_moved"] == sum(nb for r in plan for (_, nb), _ in r["moves"].values())
        return res, plan

    def tile_bytes(self):
        """{modality: (n_tiles, bytes of a tile) uint8 copy of the image}"""
        n = self.P.blocks.n_tiles
        return {mod: self.P.feat1n[mod].data.view(torch.uint8).view(n, -1).clone() for mod in self.P.modalities}

    def pointers(self):
        P = self.P
        t = [P.codes, P.live, P.vlen, P.slot_ids] + [x[mod] for mod in P.modalities for x in (P.mask_bits, P.mask, P.feat2)]
        return [x.data_ptr() for x in t] + [P.feat1n[mod].data.data_ptr() for mod in P.modalities]


def _per_slot(P):
    return [x.clone() for x in [P.live, P.vlen, P.slot_ids] + [P.mask[mod] for mod in P.modalities] +
            [P.feat2[mod] for mod in P.modalities]]


@pytest.mark.parametrize("dtype,h", CASES)
def test_compact_after_the_eight_steps(dtype, h):
    m = _model(dtype, L, h)
    pair = CPair(m)
    for name in _steps(pair):
        pass
    pair.check_tables()
    slot_state, image, ptrs = _per_slot(pair.P), pair.tile_bytes(), pair.pointers()
    free = pair.P.blocks.free_blocks
    res, plan = pair.compact()
    assert res["blocks_moved"] > 0 and res["rounds"] >= 1 and res["tiles_emptied"] >= 1, res
    assert any(r["clears"] for r in plan) and any(-2 in rec for r in plan for rec in r["records"]), "no cross-tile move / no freed block"
    es = 4 if dtype == torch.float32 else 2
    assert res["bytes_moved"] == res["blocks_moved"] * 16 * h * es * 2
    assert res["largest_free_run_after"] == 16 >= res["largest_free_run_before"] and pair.P.blocks.free_blocks == free
    assert res["tiles_touched"] == len({rec[0] for r in plan for rec in r["records"]})
    pair.check_tables()
    pair.check_k6(37)
    pair.check_k6(300)
    pair.check_searches()
    for a, b in zip(slot_state, _per_slot(pair.P)):
        assert torch.equal(_bits(a), _bits(b)), "compaction changed per-slot state"
    assert ptrs == pair.pointers()
    touched = sorted({rec[0] for r in plan for rec in r["records"]})
    rest = torch.tensor([t for t in range(TILES) if t not in touched], device=image["video"].device)
    assert len(rest) and len(touched)
    for mod, was in pair.tile_bytes().items():
        assert torch.equal(was[rest], image[mod][rest]), "image bytes of a tile without a record changed (%s)" % mod
    again, plan2 = pair.compact()
    assert plan2 == [] and again["rounds"] == again["blocks_moved"] == again["bytes_moved"] == again["tiles_touched"] == 0
    pair.check_tables()


A_LENS = [48, 80, 48, 80]


def _case_a(pair):
    slots, runs = pair.add(A_LENS, 21)
    assert slots == [0, 1, 2, 3] and runs == [(0, 3), (3, 5), (8, 3), (11, 5)]
    pair.remove([0, 2])


@pytest.mark.parametrize("dtype,h", CASES)
def test_case_a_slide_over_own_blocks(dtype, h):
    m = _model(dtype, L, h)
    pair = CPair(m, tiles=1)
    _case_a(pair)
    with pytest.raises(ValueError, match="6 free blocks of 16, the largest free run holds 3"):
        pair.P.add(*_batch([96], 22), n_clips=[96])
    pair.check_tables()
    res, plan = pair.compact()
    assert plan[0]["records"] == [[0, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, -1, -2, -2, -2, -2, -2]] and plan[0]["clears"] == []
    assert res["rounds"] == 1 and res["blocks_moved"] == 10 and res["tiles_touched"] == 1 and res["tiles_emptied"] == 0
    assert res["largest_free_run_before"] == 3 and res["largest_free_run_after"] == 6
    assert pair.P.codes.view(-1).tolist() == [-1] * 4 + [1, -1, -1, -3, -1, 3] + [-2] * 6
    pair.check_tables()
    pair.check_k6(37)
    slots, runs = pair.add([96], 22)
    assert slots == [0] and runs == [(10, 6)]
    pair.check_tables()
    pair.check_k6(37)
    pair.check_searches()


B_LENS = [90, 60, 96, 9, 64, 40, 0, 45]      # 6, 4, 6 blocks fill tile 0 (slot 1 across blocks 7 | 8); 1, 4, 3, 1, 3 in tile 1


@pytest.mark.parametrize("dtype,h", CASES)
def test_case_b_drain_into_the_last_tile(dtype, h):
    m = _model(dtype, L, h)
    pair = CPair(m, tiles=2)
    slots, runs = pair.add(B_LENS, 23)
    assert runs == [(0, 6), (6, 4), (10, 6), (16, 1), (17, 4), (21, 3), (24, 1), (25, 3)]
    pair.remove([0, 2, 4])     # tile 0: the straddling run of slot 1 alone; tile 1: a hole of 4 blocks behind slot 3
    assert pair.P.codes.view(-1)[:16].tolist() == [-2] * 6 + [-1, -3, -1, 1] + [-2] * 6
    words = {mod: pair.P.mask_bits[mod].view(-1).cpu().numpy().view(np.uint32).copy() for mod in pair.P.modalities}
    res, plan = pair.compact()
    # one launch: slot 3 (9 clips) stays at block 16; slots 5, 6 (no valid clip), 7 slide left; slot 1 arrives from tile 0
    assert len(plan) == 1 and plan[0]["clears"] == [(6, 4)]
    assert plan[0]["records"] == [[1, -1, 21, 22, 23, 24, 25, 26, 27, 6, 7, 8, 9, -1, -1, -1, -1]]
    assert pair.P.blocks.runs() == {1: (24, 4), 3: (16, 1), 5: (17, 3), 6: (20, 1), 7: (21, 3)}
    assert res["tiles_emptied"] == 1 and res["tiles_touched"] == 1 and res["blocks_moved"] == 11
    codes = pair.P.codes.view(-1).tolist()
    assert codes[:16] == [-2] * 16 and codes[16:] == [3, -1, -1, 5, 6, -1, -1, 7, -1, -1, -1, 1] + [-2] * 4      # no -3 left
    for mod in pair.P.modalities:
        now = pair.P.mask_bits[mod].view(-1).cpu().numpy().view(np.uint32)
        # word 8 = blocks 16 | 17: the kept run's half is what it was, the other half is the first block of slot 5 (all 16 clips)
        assert now[8] & 0xFFFF == words[mod][8] & 0xFFFF == 0x1FF and now[8] >> 16 == 0xFFFF
        assert now[10] & 0xFFFF == 0 and (now[:8] == 0).all()      # slot 6 has no valid clip; tile 0 is unused
    pair.check_tables()
    pair.check_k6(37)
    pair.check_k6(300)
    pair.check_searches()


def test_auto_compact_retries_once_and_default_refuses_unchanged():
    m = _model(torch.float32, L, 128)
    pair = CPair(m, tiles=1)
    pair.P = MutableCorpusIndex.create(m, CAP, tiles=1, auto_compact=True)
    _case_a(pair)
    plan = pair.P.blocks.check_compact()
    slots, runs = pair.add([96], 22)                             # refused without compaction (the test above): one call here
    assert slots == [0] and runs == [(10, 6)] and pair.P.blocks.runs() == {0: (10, 6), 1: (0, 5), 3: (5, 5)}
    # the model: the compaction inside the call, then the put that _after_put has replayed at its final place
    model = type(pair.model)(1)
    for s, (first, nb) in pair.P.blocks.runs().items():
        model.put(s, first, nb, pair.masks[s])
    pair.model = model
    pair.check_tables()
    pair.check_k6(37)
    pair.check_searches()
    # still no room after a compaction: the same message, and it says that compaction was tried
    # still no room after the compaction: the same message, and it says that compaction was tried.  Runs (2, 3) (5, 2) (7, 4),
    # free (0, 2) (11, 5): slot 2 asks for 8 blocks, 9 are free once it has left; compacted (with slot 2 in place) the free
    # blocks are (9, 7), and slot 2's two blocks at 3 | 4 are not next to them
    index = MutableCorpusIndex.create(m, CAP, tiles=1, auto_compact=True)
    index.add(*_batch([32, 48, 32, 64], 25), n_clips=[32, 48, 32, 64])
    index.remove([0])
    assert index.blocks.runs() == {1: (2, 3), 2: (5, 2), 3: (7, 4)}
    with pytest.raises(ValueError, match=r"9 free blocks of 16, the largest free run holds 7 .* after compaction$"):
        index.replace([2], *_batch([100], 24), n_clips=[128])
    assert index.blocks.runs() == {1: (0, 3), 2: (3, 2), 3: (5, 4)} and index.n_live == 3
    assert index.codes.view(-1).tolist() == [-1, -1, 1, -1, 2, -1, -1, -3, 3] + [-2] * 7
    # the default: the same history is refused and nothing changes
    index = MutableCorpusIndex.create(m, CAP, tiles=1)
    assert index.auto_compact is False
    index.add(*_batch(A_LENS, 21), n_clips=A_LENS)
    index.remove([0, 2])
    torch.cuda.synchronize()
    before = _state(index)
    with pytest.raises(ValueError, match="6 free blocks of 16, the largest free run holds 3"):
        index.add(*_batch([96], 22), n_clips=[96])
    torch.cuda.synchronize()
    assert _same(_state(index), before)


@pytest.mark.parametrize("dtype,h", CASES)
def test_a_captured_graph_survives_compaction(dtype, h):
    m = _model(dtype, L, h)
    pair = CPair(m)
    qf, qm = _queries(8)
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(m, pair.P, 8, qf.shape[1], qf.shape[2], **KW)      # captured on the EMPTY index
    for name in _steps(pair):
        pass
    res, plan = pair.compact()
    assert res["blocks_moved"] > 0
    out = g(qf, qm)                                              # no re-capture: n_tiles and every pointer are what they were
    with torch.no_grad():
        want = inf.vcmr_search(m, pair.R, qf, qm, **KW)
    for k in KEYS:
        assert torch.equal(_bits(out[k]), _bits(want[k])), k


def test_compact_needs_the_packed_form():
    m = _model(torch.float32, L, 128)
    index = MutableCorpusIndex.create(m, CAP)
    with pytest.raises(ValueError, match="tiles=None"):
        index.compact()
    with pytest.raises(ValueError, match="tiles=None"):
        MutableCorpusIndex.create(m, CAP, auto_compact=True).compact()
