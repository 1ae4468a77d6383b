"""Host-side placement of a subset view (tvretrieval_amd.subset.place_members, invert_pack_plan): pure index arithmetic."""
import json
import os

import numpy as np
import pytest
import torch

from tvretrieval_amd import ops, subset
from tvretrieval_amd.index_update import BlockTable


def _nb(lens):
    return np.maximum(1, -(-np.asarray(lens, dtype=np.int64) // 16))


def _check(members, nb, first_src, src_block, codes, firsts):
    """The invariants xml_q2c_scores_packed and xml_index_gather_blocks rely on."""
    n_tiles = codes.shape[0] // 2
    assert src_block.shape == (16 * n_tiles,) and src_block.dtype == np.int32
    assert codes.shape == (2 * n_tiles, 8) and codes.dtype == np.int32
    flat = codes.reshape(-1)
    owner = np.full(16 * n_tiles, -1, dtype=np.int64)
    for i, (v, n, s, f) in enumerate(zip(members, nb, first_src, firsts)):
        assert f // 16 == (f + n - 1) // 16, "a run never crosses a tile boundary"
        assert (owner[f:f + n] == -1).all(), "runs do not overlap"
        owner[f:f + n] = i
        assert (src_block[f:f + n] == s + np.arange(n)).all()
        assert flat[f + n - 1] == v, "the video's number in the parent at its last block"
        for g in range(f, f + n - 1):
            assert flat[g] == (-3 if g % 16 == 7 else -1), "-3 exactly where a run goes on from block 7 into block 8"
    free = owner == -1
    assert (flat[free] == -2).all() and (src_block[free] == -2).all()
    assert len(set(firsts.tolist())) == len(members), "every member exactly once"
    return n_tiles


def _in_order_tiles(nb):
    table = BlockTable(max(1, len(nb)))
    for i, n in enumerate(nb):
        runs, _ = table.check_put([i], [int(n)])
        table.commit_put([i], runs)
    return max(1, table.tiles_used())


def test_placement_invariants_on_random_lengths():
    rng = np.random.default_rng(5)
    n_straddles = 0
    for trial in range(20):
        n = int(rng.integers(1, 120))
        members = np.sort(rng.choice(1000, n, replace=False))
        nb = _nb(rng.integers(0, 129, n))
        first_src = rng.integers(0, 5000, n) if trial % 2 else 8 * members
        src_block, codes, firsts = subset.place_members(members, nb, first_src)
        tiles = _check(members, nb, first_src, src_block, codes, firsts)
        assert tiles == _in_order_tiles(nb), "no more tiles than an in-order BlockTable"
        n_straddles += int((codes.reshape(-1) == -3).sum())
    assert n_straddles > 0, "the sample never exercised the 7|8 marker"


def test_straddle_marker_wherever_a_run_lands_on_7_8():
    # 5 + 5 blocks: the second run lies on blocks 5..9; 8 + 8: none; 7 + 2: blocks 7..8
    for nb, want in (([5, 5], 1), ([8, 8], 0), ([7, 2], 1), ([3, 3, 3, 3, 4], 1), ([4, 4, 4, 4], 0)):
        members = np.arange(len(nb)) * 3 + 1
        src_block, codes, firsts = subset.place_members(members, nb, 8 * members)
        _check(members, np.asarray(nb), 8 * members, src_block, codes, firsts)
        assert int((codes == -3).sum()) == want and codes.shape == (2, 8)
        assert ((codes == -3).nonzero()[1] == 7).all() and ((codes == -3).nonzero()[0] % 2 == 0).all()


def test_placement_on_the_tvr_clip_counts():
    rec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tvr_clip_count_hist.json")))
    h = np.asarray(rec["hist"])
    lens = np.maximum(np.minimum(np.repeat(np.arange(len(h)), h), 128), 1)
    lens = np.random.default_rng(2018).permutation(lens)
    rng = np.random.default_rng(7)
    for share in (0.01, 1 / 6.0):
        members = np.sort(rng.choice(len(lens), int(len(lens) * share), replace=False))
        nb = _nb(lens[members])
        src_block, codes, firsts = subset.place_members(members, nb, 8 * members)
        tiles = _check(members, nb, 8 * members, src_block, codes, firsts)
        assert tiles == _in_order_tiles(nb)
        assert tiles >= -(-int(nb.sum()) // 16)
        print("share %.3f: %d videos, %d blocks, %d tiles (lower bound %d)" % (share, len(members), nb.sum(), tiles,
                                                                               -(-int(nb.sum()) // 16)))


def test_fixed_tiles_and_refusals():
    members = np.arange(6)
    src_block, codes, firsts = subset.place_members(members, [8] * 6, 8 * members, tiles=5)
    assert codes.shape == (10, 8) and (codes[6:] == -2).all() and (src_block[48:] == -2).all()
    with pytest.raises(ValueError, match="does not fit"):
        subset.place_members(members, [8] * 6, 8 * members, tiles=2)
    src_block, codes, firsts = subset.place_members([], [], [])
    assert codes.shape == (2, 8) and (codes == -2).all() and (src_block == -2).all()       # the empty set: one unused tile
    src_block, codes, firsts = subset.place_members([], [], [], tiles=3)
    assert codes.shape == (6, 8) and (codes == -2).all()
    for bad in ((np.array([3, 2]), [1, 1]), (np.array([2, 2]), [1, 1]), (np.array([1, 2]), [0, 1]), (np.array([1, 2]), [9, 1])):
        with pytest.raises(ValueError):
            subset.place_members(bad[0], bad[1], 8 * bad[0])
    with pytest.raises(ValueError, match="tiles"):
        subset.place_members(members, [1] * 6, 8 * members, tiles=0)


def test_placement_is_deterministic():
    rng = np.random.default_rng(11)
    members = np.sort(rng.choice(500, 77, replace=False))
    nb = rng.integers(1, 9, 77)
    a = subset.place_members(members, nb, 8 * members)
    b = subset.place_members(members.copy(), nb.copy(), 8 * members)
    assert all((x == y).all() for x, y in zip(a, b))


def test_pack_plan_inversion_against_the_row_map():
    rng = np.random.default_rng(3)
    lens = np.concatenate([rng.integers(1, 33, 13), rng.integers(33, 65, 57), rng.integers(65, 129, 9),
                           [16, 17, 32, 64, 128, 1, 33, 65, 112, 113, 0]])
    rng.shuffle(lens)
    masks = (torch.arange(128)[None] < torch.as_tensor(lens)[:, None]).float()
    plan = ops.PackPlan([masks])
    first, nb = subset.invert_pack_plan(plan)
    assert subset.invert_pack_plan(plan)[0] is first, "kept beside the plan"
    rm = plan.row_map.numpy()
    assert (nb == _nb(lens)).all()
    for v in range(len(lens)):
        rows = rm[first[v] * 16:(first[v] + nb[v]) * 16]
        assert (rows == v * 128 + np.arange(nb[v] * 16)).all(), v
        assert first[v] // 16 == (first[v] + nb[v] - 1) // 16
    assert int(nb.sum()) * 16 == int((rm >= 0).sum()), "the runs are all the rows the plan maps"
