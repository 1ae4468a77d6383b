"""What MutableCorpusIndex.create(..., exact_rank=True) refuses, before it touches a device (a stub model, no GPU): every
message names exact-rank mode, and the calls that were refused before the keyword existed still are."""
import pytest
import torch

from tvretrieval_amd import inference, ops
from tvretrieval_amd.index_update import MutableCorpusIndex


class _Cfg(object):
    def __init__(self, hidden_size=256, max_ctx_l=100):
        self.hidden_size, self.max_ctx_l = hidden_size, max_ctx_l


class _Model(object):
    """Just what MutableCorpusIndex.create looks at before it touches a device (no parameters(): an allocation would fail
    with an AttributeError, not a ValueError)."""
    use_video, use_sub = True, True

    def __init__(self, compute_dtype, **cfg):
        self.compute_dtype, self.config = compute_dtype, _Cfg(**cfg)


BOTH = [pytest.param(torch.float32, id="f32"), pytest.param(ops.F16S, id="f16s")]


@pytest.mark.parametrize("dt", BOTH)
def test_the_packed_image_is_out_of_scope(dt):
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, tiles=20)
    assert "tiles=None" in str(e.value) and "exact_rank=True" in str(e.value)
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.from_batches(_Model(dt), [], 70, exact_rank=True, tiles=20)


@pytest.mark.parametrize("dt", BOTH)
def test_chains_are_refused_for_the_builders_reason(dt):
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, part_overlap=16)
    assert "part_overlap" in str(e.value) and "score matrix" in str(e.value)


def test_a_bf16_model_is_refused():
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(torch.bfloat16), 70, exact_rank=True)
    assert "f32 activations" in str(e.value)


def test_only_the_bf16_filter_is_built(monkeypatch):
    monkeypatch.setattr(inference, "EXACT_F16S_FILTER", "f16")
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(ops.F16S), 70, exact_rank=True)
    assert "EXACT_F16S_FILTER" in str(e.value)


@pytest.mark.parametrize("dt,cfg", [(torch.float32, dict(hidden_size=100)), (ops.F16S, dict(hidden_size=100)),
                                    (ops.F16S, dict(hidden_size=48, max_ctx_l=40)),
                                    (torch.float32, dict(hidden_size=1088, max_ctx_l=40)),
                                    (torch.float32, dict(max_ctx_l=130)), (ops.F16S, dict(max_ctx_l=130))])
def test_shapes_the_put_kernel_does_not_take(dt, cfg):
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(dt, **cfg), 70, exact_rank=True)
    assert "xml_index_put_rows_exact" in str(e.value)


def test_what_was_refused_before_still_is():
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(ops.F16S), 70)
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, exact_filter=True)
    with pytest.raises(ValueError, match="exact-rank"):
        MutableCorpusIndex.create(_Model(torch.float32), 70, exact_filter=True, exact_rank=True)
    for kw in (dict(tiles=20), dict(part_overlap=16)):
        with pytest.raises(ValueError, match="exact-rank"):
            MutableCorpusIndex.create(_Model(ops.F16S), 70, **kw)
        with pytest.raises(ValueError, match="exact-rank"):
            MutableCorpusIndex.create(_Model(torch.float32), 70, exact_filter=True, **kw)


def test_accepted_arguments_reach_the_allocation():
    """The stub has no parameters(): a call that passes every refusal fails there, not with a ValueError."""
    for dt in (torch.float32, ops.F16S):
        with pytest.raises(AttributeError, match="parameters"):
            MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True)
    with pytest.raises(ValueError, match="capacity"):
        MutableCorpusIndex.create(_Model(torch.float32), 0, exact_rank=True)


def test_tighten_error_bound_is_for_exact_rank_indexes():
    class _Plain(MutableCorpusIndex):
        def __init__(self):
            self.exact = None
    with pytest.raises(ValueError, match="exact-rank"):
        _Plain().tighten_error_bound()
