"""The C ABI of the training gather over resident frame- and word-level stores (include/xmlhip_train_pool.h:
xml_gather_pool_feature_rows) without a GPU, in the manner of tests/test_ingest_tef_capi.py: the header declares exactly that
function, it is exported and bound, and every bad-argument class returns before a launch."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_train_pool.h")
BAD_ARG, UNSUPPORTED = -1, -2
F32, BF16, F16, F16S = 0, 1, 2, 3
N_ARGS = {"xml_gather_pool_feature_rows": 30}


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_the_header_symbol_is_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    src = _code(HEADER)
    syms = sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))
    assert syms == sorted(N_ARGS)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_TRAIN_POOL, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        res, args = _lib.SIGNATURES_TRAIN_POOL[s]
        assert fn.restype is res and list(fn.argtypes) == args                     # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(args) == N_ARGS[s], s
    assert set(_lib.SIGNATURES_TRAIN_POOL) == set(syms)
    others = set()
    for name in dir(_lib):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_TRAIN_POOL":
            others |= set(getattr(_lib, name))
    assert {"xml_gather_feature_rows", "xml_ingest_pool_rows", "xml_ingest_pool_rows_tef"} <= others
    assert not set(_lib.SIGNATURES_TRAIN_POOL) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6               # an added function breaks no caller
    assert '#include "xmlhip_ingest_tef.h"' in src
    # the twelve source arguments are those of xml_ingest_pool_rows, in its order and with its types
    names = lambda text, s: [p.split()[-1].lstrip("*") for p in re.search(r"\b%s\s*\(([^)]*)\)" % s, text).group(1).split(",")]
    old_names = names(_code(os.path.join(ROOT, "include", "xmlhip_ingest_pool.h")), "xml_ingest_pool_rows")
    new_names = names(src, "xml_gather_pool_feature_rows")
    assert new_names[:13] == old_names[:13]
    assert new_names[13:] == ["clip_start", "n_items", "ids", "n", "item_of", "n_examples", "dst", "dst_dt", "mask", "len_out",
                              "lmax", "max_len", "eps", "normalize", "pool", "tef", "stream"]
    assert _lib.SIGNATURES_TRAIN_POOL["xml_gather_pool_feature_rows"][1][:13] == \
        _lib.SIGNATURES_INGEST_POOL["xml_ingest_pool_rows"][1][:13]


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
GOOD = dict(n_src=2, src_a=P, dt_a=F16, rows_a=100, d_a=4000, seg_a=P, norm_a=1, src_b=P, dt_b=F16, rows_b=100, d_b=200,
            seg_b=P, norm_b=1, clip_start=P, n_items=9, ids=P, n=3, item_of=P, n_examples=12, dst=P, dst_dt=F32, mask=P, len_out=P,
            lmax=8, max_len=8, eps=1e-5, normalize=1, pool=0, tef=1)
ONE = dict(GOOD, n_src=1, d_a=5000, src_b=Z, seg_b=Z, rows_b=0, d_b=0, dt_b=-7)


def _call(lib, base=GOOD, **kw):
    """d_a + d_b = 4200 > 4096: a call that passes every argument check ends in UNSUPPORTED, still before a launch."""
    a = dict(base, **kw)
    return lib.xml_gather_pool_feature_rows(
        a["n_src"], a["src_a"], a["dt_a"], a["rows_a"], a["d_a"], a["seg_a"], a["norm_a"], a["src_b"], a["dt_b"], a["rows_b"],
        a["d_b"], a["seg_b"], a["norm_b"], a["clip_start"], a["n_items"], a["ids"], a["n"], a["item_of"], a["n_examples"], a["dst"],
        a["dst_dt"], a["mask"], a["len_out"], a["lmax"], a["max_len"], a["eps"], a["normalize"], a["pool"], a["tef"], Z)


def test_rejects_bad_arguments(lib):
    assert _call(lib) == UNSUPPORTED
    assert _call(lib, dst_dt=BF16, dt_a=F32, pool=1, normalize=0, norm_a=0, tef=0) == UNSUPPORTED
    for k in ("mask", "len_out"):                          # optional outputs
        assert _call(lib, **{k: Z}) == UNSUPPORTED, k
    assert _call(lib, item_of=Z, n_examples=0) == UNSUPPORTED          # ids are item ids
    for k in ("src_a", "seg_a", "src_b", "seg_b", "clip_start", "ids", "dst"):
        assert _call(lib, **{k: Z}) == BAD_ARG, k
    for k in ("n", "lmax", "max_len", "d_a", "d_b", "rows_a", "rows_b", "n_items", "n_examples"):
        assert _call(lib, **{k: 0}) == BAD_ARG and _call(lib, **{k: -3}) == BAD_ARG, k
    for k in ("dt_a", "dt_b"):
        for dt in (BF16, F16S, -1, 4):
            assert _call(lib, **{k: dt}) == BAD_ARG, (k, dt)
    for dt in (F16, F16S, -1, 4):
        assert _call(lib, dst_dt=dt) == BAD_ARG, dt
    for n_src in (0, 3, -1):
        assert _call(lib, n_src=n_src) == BAD_ARG
    for pool in (2, -1, 7):
        assert _call(lib, pool=pool) == BAD_ARG
    for k in ("tef", "normalize"):
        for v in (2, -1):
            assert _call(lib, **{k: v}) == BAD_ARG, (k, v)
    assert _call(lib, eps=float("nan")) == BAD_ARG
    assert _call(lib, d_a=4096, d_b=1) == UNSUPPORTED and _call(lib, d_a=4096, d_b=1, tef=0) == UNSUPPORTED


def test_one_source_ignores_the_second_side(lib):
    assert _call(lib, ONE) == UNSUPPORTED
    assert _call(lib, ONE, src_b=P, seg_b=P, rows_b=-5, d_b=-1, norm_b=3) == UNSUPPORTED
    assert _call(lib, ONE, n=0) == BAD_ARG and _call(lib, ONE, dt_a=BF16) == BAD_ARG and _call(lib, ONE, pool=2) == BAD_ARG
    assert _call(lib, ONE, tef=2) == BAD_ARG and _call(lib, ONE, n_items=0) == BAD_ARG
    for k in ("src_a", "seg_a", "clip_start", "ids", "dst"):
        assert _call(lib, ONE, **{k: Z}) == BAD_ARG, k
    assert _call(lib, ONE, d_a=4097) == UNSUPPORTED


def test_build_script_knows_the_header():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    assert "../../include/xmlhip_train_pool.h -nt" in sh, "the header is part of the staleness checks"
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "ingest_pool.hip" in srcs


def test_the_wrapper_follows_gather_feature_rows_and_stays_out_of_the_ops_contract():
    from tvretrieval_amd import inference, ops
    new = inspect.signature(ops.gather_pool_feature_rows).parameters
    old = inspect.signature(ops.gather_feature_rows).parameters
    assert list(new) == ["sources", "clip_start", "ids", "lmax", "max_len", "item_of", "pool", "normalize", "eps", "tef",
                         "out_dtype", "out", "mask_out", "len_out", "want_len"]
    for k in ("item_of", "normalize", "eps", "tef", "out_dtype", "out", "mask_out", "len_out", "want_len"):
        assert new[k].default == old[k].default, k
    assert new["pool"].default == "max"
    assert "gather_pool_feature_rows" not in inference.OPS_CONTRACT
