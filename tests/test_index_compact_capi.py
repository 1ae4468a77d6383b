"""The C ABI of the compaction entry (include/xmlhip_index_compact.h: xml_index_move_blocks_packed) without a GPU: the
header declares exactly that function, it is exported and bound, and every bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_compact.h")
BAD_ARG, UNSUPPORTED = -1, -2


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


def test_the_header_symbol_is_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    syms = header_symbols()
    assert syms == ["xml_index_move_blocks_packed"]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_COMPACT, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        assert fn.restype is _lib.SIGNATURES_COMPACT[s][0] and list(fn.argtypes) == _lib.SIGNATURES_COMPACT[s][1]   # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES_COMPACT[s][1]), s
    assert set(_lib.SIGNATURES_COMPACT) == set(syms)
    assert not set(_lib.SIGNATURES_COMPACT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INDEX))
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)


def _move(lib, n_mod=2, n=3, n_tiles=24, hidden=128, dt=0, ptrs=None):
    ptrs = ptrs or [P] * 6                                       # records, k6_a, bits_a, k6_b, bits_b, codes
    return lib.xml_index_move_blocks_packed(n_mod, ptrs[0], n, *ptrs[1:], n_tiles, hidden, dt, Z)


def test_move_blocks_packed_rejects_bad_arguments(lib):
    for i in range(6):
        ptrs = [P] * 6
        ptrs[i] = Z
        assert _move(lib, ptrs=ptrs) == BAD_ARG, i
    assert _move(lib, n_mod=0) == BAD_ARG and _move(lib, n_mod=3) == BAD_ARG and _move(lib, n_mod=-1) == BAD_ARG
    assert _move(lib, n=0) == BAD_ARG and _move(lib, n=-4) == BAD_ARG and _move(lib, n=65536) == BAD_ARG
    assert _move(lib, n_tiles=0) == BAD_ARG and _move(lib, n_tiles=-1) == BAD_ARG and _move(lib, n_tiles=(1 << 26) + 1) == BAD_ARG
    assert _move(lib, dt=2) == BAD_ARG and _move(lib, dt=3) == BAD_ARG and _move(lib, dt=-1) == BAD_ARG        # f16, split f16
    # a hidden size the tiled K6 operand does not take: bf16 rows of 128 are 256 bytes, below the kernel's 384
    assert _move(lib, hidden=128, dt=1) == UNSUPPORTED and _move(lib, hidden=100) == UNSUPPORTED
    # one modality needs no second side; stopped by the one remaining bad argument
    one = [P, P, P, Z, Z, P]
    assert _move(lib, n_mod=1, ptrs=one, n=0) == BAD_ARG and _move(lib, n_mod=1, ptrs=one, dt=2) == BAD_ARG
    assert _move(lib, n_mod=1, ptrs=one, hidden=100) == UNSUPPORTED
    for i in (0, 1, 2, 5):
        ptrs = list(one)
        ptrs[i] = Z
        assert _move(lib, n_mod=1, ptrs=ptrs) == BAD_ARG, i


def test_the_wrapper_is_a_hip_only_entry():
    from tvretrieval_amd import inference, ops
    assert callable(ops.index_move_blocks_packed)
    assert "index_move_blocks_packed" not in inference.OPS_CONTRACT
