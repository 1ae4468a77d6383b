"""The C ABI of exact-rank mode with the packed filter image (include/xmlhip_index_exact_packed.h:
xml_index_put_rows_packed_exact) and what MutableCorpusIndex.create(..., exact_rank=True, filter_tiles=N) refuses, without a
GPU: the header declares exactly the one function, it is exported and bound, every bad-argument class returns before a launch,
and every refusal of create comes before an allocation and names its reason."""
import ctypes
import os
import re

import pytest
import torch

from test_index_exact_refusals import BOTH, _Model
from tvretrieval_amd import ops
from tvretrieval_amd.index_update import MutableCorpusIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_exact_packed.h")
NAME = "xml_index_put_rows_packed_exact"
BAD_ARG, UNSUPPORTED = -1, -2
F32, F16S = 0, 1                 # XML_EXACT_F32 / XML_EXACT_F16S


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_header_symbol_is_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src))) == [NAME]
    assert hasattr(lib, NAME), "libxmlhip.so does not export %s" % NAME
    assert set(_lib.SIGNATURES_EXACT_PACKED) == {NAME}
    res, args = _lib.SIGNATURES_EXACT_PACKED[NAME]
    fn = getattr(lib, NAME)
    assert fn.restype is res and list(fn.argtypes) == args                 # bind() applied it
    params = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, src).group(1)
    assert len(params.split(",")) == len(args) == 42
    # the operands of xml_index_put_rows_exact without `tiled`, plus runs, nb_max, codes and n_tiles
    assert len(args) == len(_lib.SIGNATURES_EXACT["xml_index_put_rows_exact"][1]) - 1 + 4
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INDEX) | set(_lib.SIGNATURES_COMPACT) | set(_lib.SIGNATURES_PARTS) | \
        set(_lib.SIGNATURES_EXACT) | set(_lib.SIGNATURES_VIEW)
    assert not set(_lib.SIGNATURES_EXACT_PACKED) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip_index_exact.h"' in src
    assert "dropped whole" in text and "atomicAnd" in text and "+inf" in text


def test_the_build_knows_the_header():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    assert "xmlhip_index_exact_packed.h -nt" in sh and "index_rows.h -nt" in sh
    assert "index_update_exact.hip" in re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
SIDE = ("k6", "rescore", "rescore_inv", "feat2", "feat2_inv", "err", "imask", "bits")


def _put(lib, n_mod=2, mode=F16S, b=3, lb=100, nb_max=7, capacity=70, n_tiles=24, lpad=128, l_ref=100, hidden=256, dt=0, null=(),
         second=P, inv=P):
    """xml_index_put_rows_packed_exact with P everywhere except the names in `null`."""
    batch = dict(f1_a=P, f2_a=P, mask_a=P, f1_b=second, f2_b=second, mask_b=second, slots=P, ids=P, runs=P)
    index = {}
    for sfx, p in (("_a", P), ("_b", second)):
        for name in SIDE:
            index[name + sfx] = (inv if p is P else p) if name.endswith("_inv") else p
    state = dict(codes=P, ec=P, vlen=P, slot_ids=P, live=P)
    for name in null:
        d = batch if name in batch else index if name in index else state
        assert name in d, name
        d[name] = Z
    return getattr(lib, NAME)(n_mod, mode, *batch.values(), b, lb, nb_max, *index.values(), *state.values(), capacity, n_tiles,
                              lpad, l_ref, hidden, dt, Z)


def test_put_rejects_bad_arguments(lib):
    for name in ("f1_a", "f2_a", "mask_a", "slots", "runs", "k6_a", "rescore_a", "feat2_a", "err_a", "imask_a", "bits_a", "codes",
                 "ec", "vlen", "slot_ids", "live"):
        for mode in (F32, F16S):
            assert _put(lib, mode=mode, null=[name]) == BAD_ARG, (name, mode)
    for name in ("f1_b", "f2_b", "mask_b", "k6_b", "rescore_b", "feat2_b", "err_b", "imask_b", "bits_b"):
        assert _put(lib, null=[name]) == BAD_ARG, name
    for name in ("rescore_inv_a", "feat2_inv_a", "rescore_inv_b", "feat2_inv_b"):      # needed by the split form only
        assert _put(lib, mode=F16S, null=[name]) == BAD_ARG, name
        assert _put(lib, mode=F32, null=[name], b=0) == BAD_ARG and _put(lib, mode=F32, null=[name], hidden=100) == UNSUPPORTED
    assert _put(lib, second=Z) == BAD_ARG                                   # two modalities, the second one missing
    assert _put(lib, mode=2) == BAD_ARG and _put(lib, mode=-1) == BAD_ARG
    assert _put(lib, n_mod=0) == BAD_ARG and _put(lib, n_mod=3) == BAD_ARG
    assert _put(lib, b=0) == BAD_ARG and _put(lib, b=-2) == BAD_ARG
    assert _put(lib, b=71) == BAD_ARG                                       # more videos than slots: they cannot be distinct
    assert _put(lib, b=65536, capacity=70000) == BAD_ARG
    assert _put(lib, lb=129) == BAD_ARG and _put(lib, lb=0) == BAD_ARG
    assert _put(lib, l_ref=0) == BAD_ARG and _put(lib, l_ref=129) == BAD_ARG
    assert _put(lib, capacity=0) == BAD_ARG
    for lpad in (48, 112, 144, 0):                                          # the packed image: 128-clip slots
        assert _put(lib, lpad=lpad, lb=40, l_ref=40) == BAD_ARG, lpad
    assert _put(lib, nb_max=0) == BAD_ARG and _put(lib, nb_max=9) == BAD_ARG and _put(lib, nb_max=-1) == BAD_ARG
    assert _put(lib, n_tiles=0) == BAD_ARG and _put(lib, n_tiles=-3) == BAD_ARG
    assert _put(lib, null=["ids"], hidden=100) == UNSUPPORTED               # ids may be NULL (the slot number): stopped by the shape
    assert _put(lib, nb_max=1, hidden=100) == UNSUPPORTED and _put(lib, nb_max=8, hidden=100) == UNSUPPORTED


def test_put_answers_unsupported_for_what_the_kernel_does_not_take(lib):
    for dt in (1, 2, 3):                                                    # the inputs are f32 rows
        assert _put(lib, dt=dt) == UNSUPPORTED, dt
    assert _put(lib, hidden=100) == UNSUPPORTED                             # not whole 64-byte slices
    assert _put(lib, hidden=8 * 32 * 4 + 64) == UNSUPPORTED                 # rows longer than l2norm.h takes
    assert _put(lib, hidden=128) == UNSUPPORTED                             # bf16 rows of 256 bytes: no tiled K6 operand
    assert _put(lib, hidden=128, mode=F32) == UNSUPPORTED
    assert _put(lib, hidden=208, mode=F16S) == UNSUPPORTED                  # split-f16 rows come in groups of 32 (and bf16 slices)
    assert lib.xml_q2c_tiled_ok(128, 256, 1) == 1 and lib.xml_q2c_tiled_ok(128, 128, 1) == 0


def test_put_with_one_modality_needs_no_second_side(lib):
    assert _put(lib, n_mod=1, second=Z, b=0) == BAD_ARG
    assert _put(lib, n_mod=1, second=Z, hidden=100) == UNSUPPORTED
    assert _put(lib, n_mod=1, second=Z, mode=F32, inv=Z, hidden=100) == UNSUPPORTED


def test_the_wrapper_is_a_hip_only_entry():
    from tvretrieval_amd import inference
    assert callable(ops.index_put_rows_packed_exact)
    assert "index_put_rows_packed_exact" not in inference.OPS_CONTRACT
    assert "index_put_rows_packed_exact" in inference.__doc__


# ---- MutableCorpusIndex.create(..., exact_rank=True, filter_tiles=N): refused before any allocation (the stub has no
# parameters(): a call that passes every refusal fails there with an AttributeError)
@pytest.mark.parametrize("dt", BOTH)
def test_filter_tiles_needs_exact_rank(dt):
    m = _Model(dt)
    for kw in (dict(), dict(tiles=20), dict(exact_rank=False, auto_compact=True)):
        with pytest.raises(ValueError, match="filter_tiles") as e:
            MutableCorpusIndex.create(m, 70, filter_tiles=20, **kw)
        assert "exact_rank=True" in str(e.value)
    with pytest.raises(ValueError, match="filter_tiles"):
        MutableCorpusIndex.from_batches(m, [], 70, filter_tiles=20)


@pytest.mark.parametrize("dt", BOTH)
def test_filter_tiles_excludes_tiles_and_chains(dt):
    with pytest.raises(ValueError, match="filter_tiles") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=20, tiles=20)
    assert "tiles=" in str(e.value) and "exact-rank" in str(e.value)
    with pytest.raises(ValueError, match="filter_tiles") as e:
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=20, part_overlap=16)
    assert "part_overlap=" in str(e.value) and "exact-rank" in str(e.value)
    with pytest.raises(ValueError, match="exact-rank") as e:                # still refused, and pointing here
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, tiles=20)
    assert "tiles=None" in str(e.value) and "filter_tiles=" in str(e.value)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("bad", [0, -4, 2.5, True])
def test_filter_tiles_is_a_positive_integer(dt, bad):
    with pytest.raises(ValueError, match="filter_tiles must be a positive integer"):
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=bad)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("cfg,what", [(dict(max_ctx_l=40), "lpad 48"), (dict(hidden_size=128), "hidden 128")])
def test_shapes_without_a_tiled_bf16_image(dt, cfg, what):
    with pytest.raises(ValueError, match="exact-rank") as e:
        MutableCorpusIndex.create(_Model(dt, **cfg), 70, exact_rank=True, filter_tiles=20)
    assert "filter_tiles=20" in str(e.value) and what in str(e.value) and "filter_tiles=None" in str(e.value)
    with pytest.raises(AttributeError, match="parameters"):                 # the same shape without the packed filter image
        MutableCorpusIndex.create(_Model(dt, **cfg), 70, exact_rank=True)


@pytest.mark.parametrize("dt", BOTH)
def test_what_exact_rank_refuses_it_refuses_with_filter_tiles_too(dt):
    with pytest.raises(ValueError, match="xml_index_put_rows_exact"):
        MutableCorpusIndex.create(_Model(dt, hidden_size=100), 70, exact_rank=True, filter_tiles=20)
    with pytest.raises(ValueError, match="f32 activations"):
        MutableCorpusIndex.create(_Model(torch.bfloat16), 70, exact_rank=True, filter_tiles=20)


@pytest.mark.parametrize("dt", BOTH)
def test_accepted_arguments_reach_the_allocation(dt):
    with pytest.raises(AttributeError, match="parameters"):
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=20)
    with pytest.raises(AttributeError, match="parameters"):
        MutableCorpusIndex.create(_Model(dt), 70, exact_rank=True, filter_tiles=20, auto_compact=True)
    with pytest.raises(ValueError, match="capacity"):
        MutableCorpusIndex.create(_Model(dt), 0, exact_rank=True, filter_tiles=20)
