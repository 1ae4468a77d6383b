"""The C ABI of the subset-view entry (include/xmlhip_index_view.h: xml_index_gather_blocks) without a GPU: the header
declares exactly that function, it is exported and bound, and every bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_view.h")
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
    assert syms == ["xml_index_gather_blocks"]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_VIEW, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        assert fn.restype is _lib.SIGNATURES_VIEW[s][0] and list(fn.argtypes) == _lib.SIGNATURES_VIEW[s][1]   # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES_VIEW[s][1]) == 15, s
    assert set(_lib.SIGNATURES_VIEW) == set(syms)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INDEX) | set(_lib.SIGNATURES_COMPACT) | set(_lib.SIGNATURES_PARTS) |
              set(_lib.SIGNATURES_EXACT))
    assert not set(_lib.SIGNATURES_VIEW) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
# src_block, k6_src_a, bits_src_a, k6_src_b, bits_src_b, k6_dst_a, bits_dst_a, k6_dst_b, bits_dst_b
SRC_BLOCK, K6_SRC_A, BITS_SRC_A, K6_SRC_B, BITS_SRC_B, K6_DST_A, BITS_DST_A, K6_DST_B, BITS_DST_B = range(9)


def _gather(lib, n_mod=2, n_tiles=3, n_blocks_src=160, hidden=100, dt=0, ptrs=None):
    """hidden = 100 is refused by xml_q2c_tiled_ok: a call that passes every argument check ends in UNSUPPORTED, still
    before a launch."""
    p = ptrs or [P] * 9
    return lib.xml_index_gather_blocks(n_mod, p[0], n_tiles, p[1], p[2], p[3], p[4], n_blocks_src, p[5], p[6], p[7], p[8],
                                       hidden, dt, Z)


def test_gather_blocks_rejects_bad_arguments(lib):
    assert _gather(lib) == UNSUPPORTED and _gather(lib, hidden=128, dt=1) == UNSUPPORTED      # bf16 rows of 256 bytes
    for i in (SRC_BLOCK, K6_SRC_A, K6_SRC_B, K6_DST_A, BITS_DST_A, K6_DST_B, BITS_DST_B):
        ptrs = [P] * 9
        ptrs[i] = Z
        assert _gather(lib, ptrs=ptrs) == BAD_ARG, i
    for i in (BITS_SRC_A, BITS_SRC_B):                 # NULL source bits: that modality is all-valid, not an error
        ptrs = [P] * 9
        ptrs[i] = Z
        assert _gather(lib, ptrs=ptrs) == UNSUPPORTED, i
    assert _gather(lib, n_mod=0) == BAD_ARG and _gather(lib, n_mod=3) == BAD_ARG and _gather(lib, n_mod=-1) == BAD_ARG
    assert _gather(lib, n_tiles=0) == BAD_ARG and _gather(lib, n_tiles=-2) == BAD_ARG
    assert _gather(lib, n_blocks_src=0) == BAD_ARG and _gather(lib, n_blocks_src=-16) == BAD_ARG
    assert _gather(lib, dt=2) == BAD_ARG and _gather(lib, dt=3) == BAD_ARG and _gather(lib, dt=-1) == BAD_ARG   # f16, split f16
    # one modality needs no second side
    one = [P, P, P, Z, Z, P, P, Z, Z]
    assert _gather(lib, n_mod=1, ptrs=one) == UNSUPPORTED
    assert _gather(lib, n_mod=1, ptrs=one, n_tiles=0) == BAD_ARG and _gather(lib, n_mod=1, ptrs=one, dt=2) == BAD_ARG
    for i in (SRC_BLOCK, K6_SRC_A, K6_DST_A, BITS_DST_A):
        ptrs = list(one)
        ptrs[i] = Z
        assert _gather(lib, n_mod=1, ptrs=ptrs) == BAD_ARG, i


def test_build_script_knows_the_source_and_the_header():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "index_view.hip" in srcs
    assert os.path.isfile(os.path.join(ROOT, "tvretrieval_amd", "csrc", "index_view.hip"))
    assert "../../include/xmlhip_index_view.h -nt" in sh, "the header is part of the staleness checks"


def test_the_wrapper_is_a_hip_only_entry():
    from tvretrieval_amd import inference, ops
    assert callable(ops.index_gather_blocks)
    assert "index_gather_blocks" not in inference.OPS_CONTRACT
    assert "index_gather_blocks" in inference.__doc__
