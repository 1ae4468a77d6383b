"""What a subset view refuses (inference.video_subset, searches with subset=): every refusal is a ValueError that names its
reason and comes before any launch -- stub indexes and models on the CPU are enough to see them."""
import types

import numpy as np
import pytest
import torch

from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops, subset


def _tiled(nv=6, hidden=128, dtype=torch.float32, all_valid=True, bits=False):
    t = ops.TiledRows(torch.zeros(1, dtype=dtype), nv * 128, hidden, (nv, 128, hidden), all_valid=all_valid)
    if bits:
        t.mask_bits = torch.zeros((nv, 4), dtype=torch.int32)
    return t


def _index(nv=6, **kw):
    d = dict(parts=None, chain_head=None, video_offset=0, n_total=nv, n_videos=nv, modalities=["video"], lpad=128, l_ref=100,
             feat1n={"video": _tiled(nv)}, blocks=None, live=None, exact=None, vlen=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _view(index, version=None):
    v = object.__new__(subset.VideoSubset)
    v.index, v._version = index, version
    return v


def test_a_good_stub_passes_the_parent_check():
    assert subset.check_parent(_index()) == "fixed"
    assert subset.check_parent(_index(feat1n={"video": _tiled(all_valid=False, bits=True)})) == "fixed"


@pytest.mark.parametrize("kw, reason", [
    (dict(parts=object()), "parts index"),
    (dict(chain_head=object()), "chains"),
    (dict(video_offset=4, n_total=10), "corpus shard"),
    (dict(n_total=10), "corpus shard"),
    (dict(lpad=112, feat1n={"video": torch.zeros(6, 112, 128)}), "not the tiled image"),
    (dict(feat1n={"video": torch.zeros(6, 128, 100)}), "not the tiled image"),
    (dict(feat1n={"video": _tiled(hidden=100)}), "not the tiled image"),
    (dict(feat1n={"video": _tiled(hidden=128, dtype=torch.bfloat16)}), "not the tiled image"),
    (dict(feat1n={"video": _tiled(hidden=256, dtype=torch.float16)}), "not the tiled image"),
    (dict(feat1n={"video": _tiled(all_valid=False)}), "non-binary"),
])
def test_video_subset_refuses_the_parent(kw, reason):
    index = _index(**kw)
    with pytest.raises(ValueError, match=reason):
        inf.video_subset(index, [0, 1])
    with pytest.raises(ValueError, match=reason):          # ... and so does a search handed a view of such an index
        inf.vcmr_search(None, index, None, None, subset=_view(index))


def test_searches_refuse_before_any_launch():
    index, other = _index(), _index()
    view = _view(index)
    model = None                    # never touched: every call below raises first
    for search in (lambda **kw: inf.vcmr_search(model, index, None, None, **kw),
                   lambda **kw: inf.stage_video_topk(model, index, None, **kw)):
        with pytest.raises(ValueError, match="another index"):
            search(subset=_view(other))
        with pytest.raises(ValueError, match="external_top"):
            search(subset=view, external_top=(None, None))
        with pytest.raises(ValueError, match="HIP-only"):
            search(subset=view, ops=types.SimpleNamespace())
    with pytest.raises(ValueError, match="pad_tail"):
        inf.vcmr_search(model, index, None, None, subset=view, pad_tail=True)
    with pytest.raises(ValueError, match="another index"):
        inf.vcmr_search_host(model, index, torch.zeros(2, 3, 4), torch.ones(2, 3), subset=_view(other))
    with pytest.raises(ValueError, match="pad_tail"):
        inf.vcmr_search_host(model, index, torch.zeros(2, 3, 4), torch.ones(2, 3), subset=view, pad_tail=True)
    with pytest.raises(ValueError, match="HIP-only"):
        inf.vcmr_search_host(model, index, torch.zeros(2, 3, 4), torch.ones(2, 3), subset=view, ops=types.SimpleNamespace())


def test_a_stale_view_is_refused():
    index = _index()
    index.version = 3
    with pytest.raises(ValueError, match="stale"):
        inf.vcmr_search(None, index, None, None, subset=_view(index, version=2))
    assert not _view(index, version=3).stale


def test_member_lists():
    index = _index(nv=10)
    assert subset.member_list(index, np.array([0, 1, 0, 0, 1, 0, 0, 0, 0, 1], dtype=bool)).tolist() == [1, 4, 9]
    assert subset.member_list(index, torch.tensor([2, 5])).tolist() == [2, 5]
    assert subset.member_list(index, []).tolist() == []
    for bad in ([3, 2], [2, 2], [-1, 2], [2, 10], [0.5, 1.0], np.zeros(9, dtype=bool)):
        with pytest.raises(ValueError):
            subset.member_list(index, bad)
