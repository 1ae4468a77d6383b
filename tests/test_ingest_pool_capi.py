"""The C ABI of the pooled-ingest entry (include/xmlhip_ingest_pool.h: xml_ingest_pool_rows) without a GPU, in the manner of
tests/test_index_view_capi.py: the header declares exactly that function, it is exported and bound, and every bad-argument
class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_ingest_pool.h")
BAD_ARG, UNSUPPORTED = -1, -2
F32, BF16, F16, F16S = 0, 1, 2, 3
N_ARGS = 25


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
    assert syms == ["xml_ingest_pool_rows"]
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_INGEST_POOL, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        res, args = _lib.SIGNATURES_INGEST_POOL[s]
        assert fn.restype is res and list(fn.argtypes) == args                     # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(args) == N_ARGS, s
    assert set(_lib.SIGNATURES_INGEST_POOL) == set(syms)
    others = set()
    for name in dir(_lib):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_INGEST_POOL":
            others |= set(getattr(_lib, name))
    assert "xml_ingest_rows" in others and not set(_lib.SIGNATURES_INGEST_POOL) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src
    assert re.search(r"#define\s+XML_POOL_MAX\s+0\b", src) and re.search(r"#define\s+XML_POOL_MEAN\s+1\b", src)


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
GOOD = dict(n_src=2, src_a=P, dt_a=F16, rows_a=100, d_a=4000, seg_a=P, norm_a=1, src_b=P, dt_b=F16, rows_b=100, d_b=200,
            seg_b=P, norm_b=1, row_start=P, dst=P, dst_dt=F32, mask=P, filled=P, n=3, lmax=8, max_len=8, eps=1e-5, normalize=1,
            pool=0)
ONE = dict(GOOD, n_src=1, d_a=5000, src_b=Z, seg_b=Z, rows_b=0, d_b=0, dt_b=-7)


def _pool(lib, base=GOOD, **kw):
    """d_a + d_b = 4200 > 4096: a call that passes every argument check ends in UNSUPPORTED, still before a launch."""
    a = dict(base, **kw)
    return lib.xml_ingest_pool_rows(a["n_src"], a["src_a"], a["dt_a"], a["rows_a"], a["d_a"], a["seg_a"], a["norm_a"],
                                    a["src_b"], a["dt_b"], a["rows_b"], a["d_b"], a["seg_b"], a["norm_b"], a["row_start"],
                                    a["dst"], a["dst_dt"], a["mask"], a["filled"], a["n"], a["lmax"], a["max_len"], a["eps"],
                                    a["normalize"], a["pool"], Z)


def test_pool_rows_rejects_bad_arguments(lib):
    assert _pool(lib) == UNSUPPORTED
    assert _pool(lib, dst_dt=BF16, dt_a=F32, pool=1, normalize=0, norm_a=0) == UNSUPPORTED
    for k in ("mask", "filled"):                           # optional outputs
        assert _pool(lib, **{k: Z}) == UNSUPPORTED, k
    for k in ("src_a", "seg_a", "src_b", "seg_b", "row_start", "dst"):
        assert _pool(lib, **{k: Z}) == BAD_ARG, k
    for k in ("n", "lmax", "max_len", "d_a", "d_b", "rows_a", "rows_b"):
        assert _pool(lib, **{k: 0}) == BAD_ARG and _pool(lib, **{k: -3}) == BAD_ARG, k
    for k in ("dt_a", "dt_b"):
        for dt in (BF16, F16S, -1, 4):
            assert _pool(lib, **{k: dt}) == BAD_ARG, (k, dt)
    for dt in (F16, F16S, -1, 4):
        assert _pool(lib, dst_dt=dt) == BAD_ARG, dt
    for n_src in (0, 3, -1):
        assert _pool(lib, n_src=n_src) == BAD_ARG
    for pool in (2, -1, 7):
        assert _pool(lib, pool=pool) == BAD_ARG
    assert _pool(lib, d_a=4096, d_b=1) == UNSUPPORTED
    # one source needs no second side: its arguments are ignored, whatever they hold
    assert _pool(lib, ONE) == UNSUPPORTED
    assert _pool(lib, ONE, n=0) == BAD_ARG and _pool(lib, ONE, dt_a=BF16) == BAD_ARG and _pool(lib, ONE, pool=2) == BAD_ARG
    for k in ("src_a", "seg_a", "row_start", "dst"):
        assert _pool(lib, ONE, **{k: Z}) == BAD_ARG, k
    assert _pool(lib, ONE, d_a=4097) == UNSUPPORTED


def test_build_script_knows_the_source_and_the_header():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "ingest_pool.hip" in srcs
    assert os.path.isfile(os.path.join(ROOT, "tvretrieval_amd", "csrc", "ingest_pool.hip"))
    assert "../../include/xmlhip_ingest_pool.h -nt" in sh, "the header is part of the staleness checks"


def test_the_wrapper_is_a_hip_only_entry():
    from tvretrieval_amd import inference, ops
    assert callable(ops.ingest_pool_rows)
    assert "ingest_pool_rows" not in inference.OPS_CONTRACT
    assert "ingest_pool_rows" in inference.__doc__
