"""The C ABI of the chain entries (include/xmlhip_index_parts.h: xml_index_set_chains, xml_chain_best_allow,
xml_chain_best_rows) without a GPU: the header declares exactly those functions, they are exported and bound, and every
bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_parts.h")
BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))


def test_the_header_symbols_are_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    syms = header_symbols()
    assert syms == ["xml_chain_best_allow", "xml_chain_best_rows", "xml_index_set_chains"]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_PARTS, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        assert fn.restype is _lib.SIGNATURES_PARTS[s][0] and list(fn.argtypes) == _lib.SIGNATURES_PARTS[s][1]   # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES_PARTS[s][1]), s
    assert set(_lib.SIGNATURES_PARTS) == set(syms)
    assert not set(_lib.SIGNATURES_PARTS) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INDEX) | set(_lib.SIGNATURES_COMPACT))
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)


def _set(lib, n=3, capacity=70, ptrs=None):
    ptrs = ptrs or [P] * 4                                       # records, chain_head, chain_next, chain_offset
    return lib.xml_index_set_chains(ptrs[0], n, ptrs[1], ptrs[2], ptrs[3], capacity, Z)


def _fold(lib, ld=70, rows=5, capacity=70, max_parts=8, allow_ld=3, allow_rows=1, out_ld=3, ptrs=None):
    ptrs = ptrs or [P] * 5                                       # scores, chain_head, chain_next, video_allow, out_bits
    return lib.xml_chain_best_allow(ptrs[0], ld, rows, capacity, ptrs[1], ptrs[2], max_parts, ptrs[3], allow_ld, allow_rows,
                                    ptrs[4], out_ld, Z)


def _rows(lib, ld=70, rows=5, capacity=70, max_parts=8, ptrs=None):
    ptrs = ptrs or [P] * 5                                       # scores, chain_head, chain_next, video, out
    return lib.xml_chain_best_rows(ptrs[0], ld, rows, capacity, ptrs[1], ptrs[2], max_parts, ptrs[3], ptrs[4], Z)


def test_set_chains_rejects_bad_arguments(lib):
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = Z
        assert _set(lib, ptrs=ptrs) == BAD_ARG, i
    assert _set(lib, n=-1) == BAD_ARG and _set(lib, capacity=0) == BAD_ARG and _set(lib, capacity=-3) == BAD_ARG
    assert _set(lib, n=0, capacity=0) == BAD_ARG                 # validation comes before the n == 0 return
    assert _set(lib, n=0) == 0                                   # nothing to do: no launch


def test_chain_best_allow_rejects_bad_arguments(lib):
    for i in range(5):                                           # video_allow is not optional here
        ptrs = [P] * 5
        ptrs[i] = Z
        assert _fold(lib, ptrs=ptrs) == BAD_ARG, i
    assert _fold(lib, rows=-1) == BAD_ARG
    assert _fold(lib, capacity=0) == BAD_ARG and _fold(lib, capacity=-1) == BAD_ARG
    assert _fold(lib, max_parts=0) == BAD_ARG and _fold(lib, max_parts=-2) == BAD_ARG
    assert _fold(lib, ld=69) == BAD_ARG
    assert _fold(lib, out_ld=2) == BAD_ARG and _fold(lib, allow_ld=2) == BAD_ARG           # 70 slots need 3 words
    assert _fold(lib, allow_rows=0) == BAD_ARG and _fold(lib, allow_rows=4) == BAD_ARG and _fold(lib, allow_rows=6) == BAD_ARG
    assert _fold(lib, rows=0, ld=69) == BAD_ARG and _fold(lib, rows=0, allow_rows=2) == BAD_ARG
    assert _fold(lib, rows=0) == 0 and _fold(lib, rows=0, allow_rows=0) == 0               # no rows: no launch


def test_chain_best_rows_rejects_bad_arguments(lib):
    for i in range(5):
        ptrs = [P] * 5
        ptrs[i] = Z
        assert _rows(lib, ptrs=ptrs) == BAD_ARG, i
    assert _rows(lib, rows=-1) == BAD_ARG and _rows(lib, capacity=0) == BAD_ARG and _rows(lib, max_parts=0) == BAD_ARG
    assert _rows(lib, ld=69) == BAD_ARG and _rows(lib, rows=0, ld=69) == BAD_ARG
    assert _rows(lib, rows=0) == 0


def test_the_wrappers_are_hip_only_entries():
    from tvretrieval_amd import inference, ops
    for name in ("index_set_chains", "chain_best_allow", "chain_best_rows"):
        assert callable(getattr(ops, name))
        assert name not in inference.OPS_CONTRACT
        assert name in inference.__doc__
