"""The search drivers see long videos held as several index rows through index.fold alone (DESIGN.md sections 19, 20c, 20g):
a recording fake `ops` on CPU tensors shows which entries a search calls, with what, on a plain index and on an index whose fold
is a third implementation written here -- which only works if no driver asks which of the two real forms it serves."""
import os
import re
import types

import pytest
import torch

from tvretrieval_amd import inference as inf

NQ, NV, LPAD, H = 2, 6, 16, 8
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tvretrieval_amd")


class _Ops(object):
    """Records (name, keyword arguments of interest) of every entry called; returns small CPU tensors."""

    def __init__(self):
        self.calls = []

    def q2c_scores_fused(self, qn, cn, masks, normalize_q=False):
        self.calls.append(("q2c_scores_fused", dict(normalize_q=normalize_q)))
        return torch.arange(NQ * NV, dtype=torch.float32).reshape(NQ, NV)

    def topk_rows(self, scores, k, alpha=0.0, idx_in=None, allow=None):
        self.calls.append(("topk_rows", dict(k=k, alpha=alpha, allow=allow)))
        return torch.zeros(NQ, k), torch.zeros(NQ, k, dtype=torch.int32)


def _index():
    t = {"video": torch.zeros(NV, LPAD, H)}
    return inf.CorpusIndex(["video"], t, dict(t), {"video": torch.ones(NV, LPAD)}, LPAD)


def _qvec():
    return {"video": torch.ones(NQ, H)}


class _ThirdFold(object):
    """Neither parts nor chains: videos numbered 0..39, a marker for the fold's allow words."""
    overlap, n_videos = 16, 40
    part_offset = torch.arange(NV, dtype=torch.int32)
    table = torch.arange(NV, dtype=torch.int32) + 100

    def __init__(self):
        self.marker = torch.tensor([[0x15]], dtype=torch.int32)

    def best_allow(self, ops, scores, allow):
        ops.calls.append(("best_allow", dict(allow=allow)))
        return self.marker

    def meta2vid(self, meta2vid):
        return self.table


def test_plain_index_has_no_fold_and_ranks_under_the_callers_mask():
    index, ops = _index(), _Ops()
    assert index.fold is None
    allow = torch.tensor([[0b101101]], dtype=torch.int32)
    q2c, top_w, top_i, exact = inf.stage_video_topk(None, index, _qvec(), max_vcmr_video=4, ops=ops, video_allow=allow)
    assert [c[0] for c in ops.calls] == ["q2c_scores_fused", "topk_rows"] and exact is None
    assert ops.calls[0][1] == dict(normalize_q=True)
    assert ops.calls[1][1]["allow"] is allow and ops.calls[1][1]["k"] == 4 and ops.calls[1][1]["alpha"] == 20.0
    assert inf._decode_operands(index, None) == (None, {})


def test_a_third_fold_is_served_without_the_drivers_knowing_its_form():
    index, ops, fold = _index(), _Ops(), _ThirdFold()
    index.fold = fold
    index.live = torch.tensor([[0b011111]], dtype=torch.int32)
    index.slot_ids = torch.arange(NV, dtype=torch.int32)
    # the mask is sized by the fold's videos (40 -> two words), not by the index rows (6 -> one word)
    with pytest.raises(ValueError, match=r">= 2\) words for 40 videos"):
        inf.stage_video_topk(None, index, _qvec(), ops=ops, video_allow=torch.zeros((1, 1), dtype=torch.int32))
    assert ops.calls == []
    allow = torch.tensor([[0b110110, -1]], dtype=torch.int32)
    assert inf._check_video_allow(allow, index, NQ) is allow
    q2c, top_w, top_i, exact = inf.stage_video_topk(None, index, _qvec(), max_vcmr_video=100, ops=ops, video_allow=allow)
    assert [c[0] for c in ops.calls] == ["q2c_scores_fused", "best_allow", "topk_rows"] and exact is None
    assert torch.equal(ops.calls[1][1]["allow"], torch.tensor([[0b010110]], dtype=torch.int32))       # ANDed with the live words
    assert ops.calls[2][1]["allow"] is fold.marker and ops.calls[2][1]["k"] == NV
    assert q2c.shape == (NQ, NV)
    # K10's operands come from the fold; what a search with a fold refuses is read off the fold as well
    m2v, pkw = inf._decode_operands(index, None)
    assert m2v is fold.table and list(pkw) == ["part_offset"] and pkw["part_offset"] is fold.part_offset
    with pytest.raises(ValueError, match="exceeds the part overlap of 16 clips"):
        inf._check_parts_search(index, 17)
    with pytest.raises(ValueError, match="external_top on a parts index"):
        inf.stage_video_topk(None, index, _qvec(), ops=ops, external_top=(top_i, top_w))
    with pytest.raises(ValueError, match="parts index"):
        inf.GraphedVcmrSearch(None, index, NQ, 4, 8)


def _members(fold):
    return {n for n in dir(fold) if not n.startswith("_")}


def test_the_two_folds_have_one_interface_and_two_places_set_them():
    tab = torch.arange(NV, dtype=torch.int32)
    parts = inf.PartsFold(types.SimpleNamespace(overlap=16, n_videos=4, part_offset=tab, part_video=tab))
    index = _index()
    index.part_overlap, index.chain_head, index.chain_offset = 16, tab, tab
    chain = inf.ChainFold(index)
    shared = {"overlap", "n_videos", "part_offset", "best_allow", "best_rows", "video_of", "meta2vid"}
    assert _members(parts) == shared
    assert _members(chain) == shared | {"slot_allow", "fold_candidates", "members"}
    assert (chain.overlap, chain.n_videos, parts.n_videos) == (16, NV, 4) and chain.part_offset is tab
    top_i = torch.tensor([[3, -1]], dtype=torch.int32)
    assert parts.video_of(top_i).tolist() == [[3, -1]] and chain.video_of(top_i).tolist() == [[3, -1]]
    assert chain.meta2vid(tab) is tab
    # index.parts is the table of the PartsFold and nothing else: clearing it leaves a plain index, a ChainFold has none
    assert index.parts is None
    index.fold = chain
    index.parts = None
    assert index.fold is chain and index.parts is None
    index.fold = parts
    assert index.parts.n_videos == 4
    with pytest.raises(AttributeError):
        index.parts = index.parts
    index.parts = None
    assert index.fold is None and index.parts is None
    # the package sets index.fold (to anything but the None of CorpusIndex.__init__) where the two forms are made, nowhere else
    sites = []
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            func = None
            for line in open(os.path.join(PKG, name)):
                func = (re.match(r"\s*def (\w+)", line) or [None, func])[1]
                if re.search(r"\.fold\s*=(?!=)(?!\s*None\b)", line):
                    sites.append((name, func))
    assert sites == [("index_update.py", "_init_chains"), ("inference.py", "build_corpus_index")]
