"""What MutableCorpusIndex.create(..., exact_rank=True, exact_part_overlap=O) refuses, before it touches a device (the stub
model of tests/test_index_exact_refusals.py, no GPU), and that the old spellings stay refused and point to the new keyword."""
import pytest
import torch

from test_index_exact_refusals import BOTH, _Model
from tvretrieval_amd.index_update import MutableCorpusIndex


@pytest.mark.parametrize("dt", BOTH)
def test_the_keyword_needs_exact_rank_mode(dt):
    for kw in (dict(), dict(part_overlap=16), dict(tiles=20)):
        with pytest.raises(ValueError, match="exact_part_overlap") as e:
            MutableCorpusIndex.create(_Model(dt), 70, exact_part_overlap=16, **kw)
        assert "exact_rank=True" in str(e.value)
    with pytest.raises(ValueError, match="exact_part_overlap"):
        MutableCorpusIndex.from_batches(_Model(dt), [], 70, exact_part_overlap=16)


@pytest.mark.parametrize("dt", BOTH)
def test_the_keyword_excludes_tiles_and_part_overlap(dt):
    with pytest.raises(ValueError, match="exact_part_overlap") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, exact_part_overlap=16, tiles=20)
    assert "tiles=" in str(e.value) and "filter_tiles=" in str(e.value)
    with pytest.raises(ValueError, match="exact_part_overlap") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, exact_part_overlap=16, part_overlap=16)
    assert "part_overlap=" in str(e.value)
    with pytest.raises(ValueError, match="exact_part_overlap"):
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, exact_part_overlap=16, filter_tiles=20, part_overlap=16)


@pytest.mark.parametrize("dt", BOTH)
def test_the_overlap_lies_inside_a_slot(dt):
    for bad in (-1, 100, 101, 16.5, True, 1000):
        with pytest.raises(ValueError, match=r"exact_part_overlap must be a number of clips in \[0, l_ref = 100\)"):
            MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, exact_part_overlap=bad)
    with pytest.raises(ValueError, match=r"l_ref = 32\)"):
        MutableCorpusIndex.create(_Model(dt), 70, l_ref=32, exact_rank=True, exact_part_overlap=32)
    with pytest.raises(ValueError, match=r"l_ref = 32\)"):
        MutableCorpusIndex.create(_Model(dt), 70, l_ref=32, exact_rank=True, exact_part_overlap=40, filter_tiles=20)


@pytest.mark.parametrize("dt", BOTH)
def test_the_old_spellings_stay_refused_and_point_here(dt):
    with pytest.raises(ValueError, match="score matrix") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, part_overlap=16)
    assert "exact_part_overlap=" in str(e.value)
    with pytest.raises(ValueError, match="filter_tiles") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=20, part_overlap=16)
    assert "part_overlap=" in str(e.value) and "exact_part_overlap=" in str(e.value)


def test_what_exact_rank_mode_refuses_is_refused_with_the_keyword_too():
    with pytest.raises(ValueError, match="f32 activations"):
        MutableCorpusIndex.create(_Model(torch.bfloat16), 70, exact_rank=True, exact_part_overlap=16)
    with pytest.raises(ValueError, match="xml_index_put_rows_exact"):
        MutableCorpusIndex.create(_Model(torch.float32, max_ctx_l=130), 70, exact_rank=True, exact_part_overlap=16)
    with pytest.raises(ValueError, match="capacity"):
        MutableCorpusIndex.create(_Model(torch.float32), 0, exact_rank=True, exact_part_overlap=16)
    with pytest.raises(ValueError, match="max_parts"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, exact_rank=True, exact_part_overlap=16, max_parts=0)


@pytest.mark.parametrize("dt", BOTH)
def test_what_is_accepted_reaches_the_allocation(dt):
    """The stub has no parameters(): a call that passes every refusal fails there, not with a ValueError."""
    for kw in (dict(), dict(filter_tiles=20), dict(max_parts=8), dict(filter_tiles=20, auto_compact=True)):
        for ov in (0, 16, 99):
            with pytest.raises(AttributeError, match="parameters"):
                MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, exact_part_overlap=ov, **kw)
