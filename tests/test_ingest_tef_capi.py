"""The C ABI of the ingest entries with the temporal endpoint columns (include/xmlhip_ingest_tef.h: xml_ingest_rows_tef,
xml_ingest_pool_rows_tef) without a GPU, in the manner of tests/test_index_view_capi.py: the header declares exactly those
functions, they are exported and bound, and every bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_ingest_tef.h")
BAD_ARG, UNSUPPORTED = -1, -2
F32, BF16, F16, F16S = 0, 1, 2, 3
N_ARGS = {"xml_ingest_rows_tef": 15, "xml_ingest_pool_rows_tef": 27}


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
    assert syms == sorted(N_ARGS)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_INGEST_TEF, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        res, args = _lib.SIGNATURES_INGEST_TEF[s]
        assert fn.restype is res and list(fn.argtypes) == args                     # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(args) == N_ARGS[s], s
    assert set(_lib.SIGNATURES_INGEST_TEF) == set(syms)
    others = set()
    for name in dir(_lib):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_INGEST_TEF":
            others |= set(getattr(_lib, name))
    assert {"xml_ingest_rows", "xml_ingest_pool_rows"} <= others and not set(_lib.SIGNATURES_INGEST_TEF) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6               # an added function breaks no caller
    assert '#include "xmlhip_ingest_pool.h"' in src
    # the pooled entry takes every argument of xml_ingest_pool_rows in its order, then the two arrays, then the stream
    old = _lib.SIGNATURES_INGEST_POOL["xml_ingest_pool_rows"][1]
    new = _lib.SIGNATURES_INGEST_TEF["xml_ingest_pool_rows_tef"][1]
    assert new == old[:-1] + [ctypes.c_void_p, ctypes.c_void_p] + old[-1:]
    pool_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xmlhip_ingest_pool.h")).read(), flags=re.S)
    names = lambda text, s: [p.split()[-1].lstrip("*") for p in re.search(r"\b%s\s*\(([^)]*)\)" % s, text).group(1).split(",")]
    old_names = names(pool_h, "xml_ingest_pool_rows")
    assert names(src, "xml_ingest_pool_rows_tef") == old_names[:-1] + ["tef_pos", "tef_len", "stream"]


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
ROWS = dict(src=P, src_dt=F16, row_start=P, tef_pos=P, tef_len=P, dst=P, dst_dt=F32, mask=P, n=3, lmax=8, d=5000, max_len=8,
            eps=1e-5, normalize=1)


def _rows(lib, **kw):
    """d = 5000 > 4096: a call that passes every argument check ends in UNSUPPORTED, still before a launch."""
    a = dict(ROWS, **kw)
    return lib.xml_ingest_rows_tef(a["src"], a["src_dt"], a["row_start"], a["tef_pos"], a["tef_len"], a["dst"], a["dst_dt"],
                                   a["mask"], a["n"], a["lmax"], a["d"], a["max_len"], a["eps"], a["normalize"], Z)


def test_rows_tef_rejects_bad_arguments(lib):
    assert _rows(lib) == UNSUPPORTED
    assert _rows(lib, src_dt=F32, dst_dt=BF16, normalize=0) == UNSUPPORTED
    assert _rows(lib, mask=Z) == UNSUPPORTED                               # optional output
    assert _rows(lib, tef_pos=Z, tef_len=Z) == UNSUPPORTED                 # both or neither
    assert _rows(lib, tef_pos=Z) == BAD_ARG and _rows(lib, tef_len=Z) == BAD_ARG
    for k in ("src", "row_start", "dst"):
        assert _rows(lib, **{k: Z}) == BAD_ARG, k
    for k in ("n", "lmax", "d", "max_len"):
        assert _rows(lib, **{k: 0}) == BAD_ARG and _rows(lib, **{k: -3}) == BAD_ARG, k
    for dt in (BF16, F16S, -1, 4):
        assert _rows(lib, src_dt=dt) == BAD_ARG, dt
    for dt in (F16, F16S, -1, 4):
        assert _rows(lib, dst_dt=dt) == BAD_ARG, dt
    assert _rows(lib, d=4097) == UNSUPPORTED                               # d + 2 > 4098
    assert _rows(lib, d=4097, tef_pos=Z) == BAD_ARG


GOOD = dict(n_src=2, src_a=P, dt_a=F16, rows_a=100, d_a=4000, seg_a=P, norm_a=1, src_b=P, dt_b=F16, rows_b=100, d_b=200,
            seg_b=P, norm_b=1, row_start=P, dst=P, dst_dt=F32, mask=P, filled=P, n=3, lmax=8, max_len=8, eps=1e-5, normalize=1,
            pool=0, tef_pos=P, tef_len=P)
ONE = dict(GOOD, n_src=1, d_a=5000, src_b=Z, seg_b=Z, rows_b=0, d_b=0, dt_b=-7)


def _pool(lib, base=GOOD, **kw):
    """d_a + d_b = 4200 > 4096: a call that passes every argument check ends in UNSUPPORTED, still before a launch."""
    a = dict(base, **kw)
    return lib.xml_ingest_pool_rows_tef(a["n_src"], a["src_a"], a["dt_a"], a["rows_a"], a["d_a"], a["seg_a"], a["norm_a"],
                                        a["src_b"], a["dt_b"], a["rows_b"], a["d_b"], a["seg_b"], a["norm_b"], a["row_start"],
                                        a["dst"], a["dst_dt"], a["mask"], a["filled"], a["n"], a["lmax"], a["max_len"], a["eps"],
                                        a["normalize"], a["pool"], a["tef_pos"], a["tef_len"], Z)


def test_pool_rows_tef_rejects_bad_arguments(lib):
    assert _pool(lib) == UNSUPPORTED
    assert _pool(lib, dst_dt=BF16, dt_a=F32, pool=1, normalize=0, norm_a=0) == UNSUPPORTED
    for k in ("mask", "filled"):                           # optional outputs
        assert _pool(lib, **{k: Z}) == UNSUPPORTED, k
    assert _pool(lib, tef_pos=Z, tef_len=Z) == UNSUPPORTED
    assert _pool(lib, tef_pos=Z) == BAD_ARG and _pool(lib, tef_len=Z) == BAD_ARG
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
    assert _pool(lib, d_a=4096, d_b=1) == UNSUPPORTED      # D + 2 > 4098
    # one source needs no second side: its arguments are ignored, whatever they hold
    assert _pool(lib, ONE) == UNSUPPORTED
    assert _pool(lib, ONE, n=0) == BAD_ARG and _pool(lib, ONE, dt_a=BF16) == BAD_ARG and _pool(lib, ONE, pool=2) == BAD_ARG
    assert _pool(lib, ONE, tef_len=Z) == BAD_ARG
    for k in ("src_a", "seg_a", "row_start", "dst"):
        assert _pool(lib, ONE, **{k: Z}) == BAD_ARG, k
    assert _pool(lib, ONE, d_a=4097) == UNSUPPORTED


def test_build_script_knows_the_headers():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    assert "../../include/xmlhip_ingest_tef.h -nt" in sh and "ingest_tef.h -nt" in sh, "the headers are part of the staleness checks"
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "ingest.hip" in srcs and "ingest_pool.hip" in srcs


def test_the_wrappers_refuse_half_a_place_and_keep_their_defaults():
    import inspect
    from tvretrieval_amd import ops
    for fn in (ops.ingest_rows, ops.ingest_pool_rows):
        sig = inspect.signature(fn).parameters
        assert sig["tef"].default is False and sig["tef_pos"].default is None and sig["tef_len"].default is None
