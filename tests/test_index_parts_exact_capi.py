"""The C ABI of the chain entries of an exact-rank index (include/xmlhip_index_parts_exact.h: xml_cand_best_part and its limit
query, xml_chain_spread_allow, xml_chain_members) without a GPU: the header declares exactly those functions, they are exported
and bound, and every bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_parts_exact.h")
BAD_ARG = -1
NAMES = ["xml_cand_best_part", "xml_cand_best_part_max_m", "xml_chain_members", "xml_chain_spread_allow"]


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_header_symbols_are_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    src = _source()
    syms = sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))
    assert syms == NAMES
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_PARTS_EXACT, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        res, args = _lib.SIGNATURES_PARTS_EXACT[s]
        assert fn.restype is res and list(fn.argtypes) == args                  # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(args), s
    assert set(_lib.SIGNATURES_PARTS_EXACT) == set(syms)
    others = (_lib.SIGNATURES, _lib.SIGNATURES_INDEX, _lib.SIGNATURES_COMPACT, _lib.SIGNATURES_PARTS, _lib.SIGNATURES_EXACT,
              _lib.SIGNATURES_VIEW, _lib.SIGNATURES_EXACT_PACKED)
    for table in others:
        assert not set(_lib.SIGNATURES_PARTS_EXACT) & set(table)
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src


def test_the_limit_is_the_widest_list_the_search_folds(lib):
    from tvretrieval_amd import inference, ops
    assert lib.xml_cand_best_part_max_m() == ops.cand_best_part_max_m() == 4096
    assert inference.EXACT_TIER2_CAP <= lib.xml_cand_best_part_max_m()          # the second tier's widest re-scored list


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)


def _fold(lib, ld=256, rows=5, m=256, n=70, out_ld=256, ptrs=None):
    ptrs = ptrs or [P] * 6                                       # scores, ids, group, order, out_scores, out_ids
    return lib.xml_cand_best_part(ptrs[0], ptrs[1], ld, rows, m, ptrs[2], ptrs[3], n, ptrs[4], ptrs[5], out_ld, Z)


def _spread(lib, allow_ld=3, allow_rows=1, rows=5, capacity=70, out_ld=3, ptrs=None):
    ptrs = ptrs or [P] * 3                                       # video_allow, chain_head, out_bits
    return lib.xml_chain_spread_allow(ptrs[0], allow_ld, allow_rows, rows, capacity, ptrs[1], ptrs[2], out_ld, Z)


def _members(lib, rows=5, capacity=70, max_parts=8, out_ld=8, ptrs=None):
    ptrs = ptrs or [P] * 4                                       # video, chain_head, chain_next, out
    return lib.xml_chain_members(ptrs[0], rows, capacity, ptrs[1], ptrs[2], max_parts, ptrs[3], out_ld, Z)


def test_cand_best_part_rejects_bad_arguments(lib):
    limit = lib.xml_cand_best_part_max_m()
    for i in range(6):
        ptrs = [P] * 6
        ptrs[i] = Z
        assert _fold(lib, ptrs=ptrs) == BAD_ARG, i
    assert _fold(lib, rows=-1) == BAD_ARG
    assert _fold(lib, m=0, ld=1, out_ld=1) == BAD_ARG and _fold(lib, m=-4) == BAD_ARG
    assert _fold(lib, m=limit + 1, ld=limit + 1, out_ld=limit + 1) == BAD_ARG
    assert _fold(lib, ld=255) == BAD_ARG and _fold(lib, out_ld=255) == BAD_ARG
    assert _fold(lib, n=0) == BAD_ARG and _fold(lib, n=-1) == BAD_ARG
    assert _fold(lib, rows=0, ld=255) == BAD_ARG and _fold(lib, rows=0, m=limit + 1, ld=limit + 1, out_ld=limit + 1) == BAD_ARG
    assert _fold(lib, rows=0) == 0 and _fold(lib, rows=0, m=limit, ld=limit, out_ld=limit) == 0      # no rows: no launch


def test_chain_spread_allow_rejects_bad_arguments(lib):
    for i in range(3):
        ptrs = [P] * 3
        ptrs[i] = Z
        assert _spread(lib, ptrs=ptrs) == BAD_ARG, i
    assert _spread(lib, rows=-1) == BAD_ARG
    assert _spread(lib, capacity=0) == BAD_ARG and _spread(lib, capacity=-1) == BAD_ARG
    assert _spread(lib, out_ld=2) == BAD_ARG and _spread(lib, allow_ld=2) == BAD_ARG             # 70 slots need 3 words
    assert _spread(lib, allow_rows=0) == BAD_ARG and _spread(lib, allow_rows=4) == BAD_ARG and _spread(lib, allow_rows=6) == BAD_ARG
    assert _spread(lib, rows=0, out_ld=2) == BAD_ARG and _spread(lib, rows=0, allow_rows=2) == BAD_ARG
    assert _spread(lib, rows=0) == 0 and _spread(lib, rows=0, allow_rows=0) == 0                 # no rows: no launch


def test_chain_members_rejects_bad_arguments(lib):
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = Z
        assert _members(lib, ptrs=ptrs) == BAD_ARG, i
    assert _members(lib, rows=-1) == BAD_ARG and _members(lib, capacity=0) == BAD_ARG and _members(lib, capacity=-2) == BAD_ARG
    assert _members(lib, max_parts=0) == BAD_ARG and _members(lib, max_parts=-1) == BAD_ARG
    assert _members(lib, out_ld=7) == BAD_ARG and _members(lib, rows=0, out_ld=7) == BAD_ARG
    assert _members(lib, rows=0) == 0


def test_the_wrappers_are_hip_only_entries():
    from tvretrieval_amd import inference, ops
    for name in ("cand_best_part", "chain_spread_allow", "chain_members"):
        assert callable(getattr(ops, name))
        assert name not in inference.OPS_CONTRACT
        assert name in inference.__doc__
