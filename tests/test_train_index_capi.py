"""The C ABI of training on a resident index (include/xmlhip_train_index.h: xml_index_gather_video_rows,
xml_q2c_scores_arg_bwd_q, xml_pair_sim_bwd_q) without a GPU, in the manner of tests/test_train_pool_capi.py: the header declares
exactly these functions, they are exported and bound, and every documented bad-argument class returns before a launch."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_train_index.h")
BAD_ARG, UNSUPPORTED = -1, -2
F32, BF16, F16, F16S = 0, 1, 2, 3
ROWS, IMAGE = 0, 1
N_ARGS = {"xml_index_gather_video_rows": 25, "xml_q2c_scores_arg_bwd_q": 17, "xml_pair_sim_bwd_q": 8}


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_the_header_symbols_are_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    src = _code(HEADER)
    syms = sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))
    assert syms == sorted(N_ARGS)
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_TRAIN_INDEX, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        res, args = _lib.SIGNATURES_TRAIN_INDEX[s]
        assert fn.restype is res and list(fn.argtypes) == args                     # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(args) == N_ARGS[s], s
    assert set(_lib.SIGNATURES_TRAIN_INDEX) == set(syms)
    others = set()
    for name in dir(_lib):
        if name.startswith("SIGNATURES") and name != "SIGNATURES_TRAIN_INDEX":
            others |= set(getattr(_lib, name))
    assert {"xml_q2c_scores_l2norm_bwd_multi", "xml_pair_sim_bwd", "xml_index_gather_blocks", "xml_gather_feature_rows"} <= others
    assert not set(_lib.SIGNATURES_TRAIN_INDEX) & others
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6               # an added function breaks no caller
    assert '#include "xmlhip.h"' in src
    assert (_lib.XML_INDEX_ROW_MAJOR, _lib.XML_INDEX_BLOCK_IMAGE) == (ROWS, IMAGE)
    assert re.search(r"XML_INDEX_ROW_MAJOR\s*=\s*0\s*,\s*XML_INDEX_BLOCK_IMAGE\s*=\s*1", src)
    # the existing entries keep their contracts: same argument lists as before this header existed
    old = _code(os.path.join(ROOT, "include", "xmlhip.h"))
    assert len(re.search(r"\bxml_pair_sim_bwd\s*\(([^)]*)\)", old).group(1).split(",")) == 10
    assert len(re.search(r"\bxml_q2c_scores_l2norm_bwd_multi\s*\(([^)]*)\)", old).group(1).split(",")) == 20


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)

# ---- xml_index_gather_video_rows: hidden = 4104 > 4096 -> a call that passes every argument check ends in UNSUPPORTED --------
GATHER = dict(n_mod=2, form=IMAGE, slot=P, first_block=P, n=3, vlen=P, n_videos=10, n_blocks=80, lpad=128, cn_src_a=P, f2_src_a=P,
              mask_src_a=P, cn_src_b=P, f2_src_b=P, mask_src_b=P, cn_a=P, f2_a=P, mask_a=P, cn_b=P, f2_b=P, mask_b=P, l=100,
              hidden=4104, dt=BF16)
GATHER_ORDER = ["n_mod", "form", "slot", "first_block", "n", "vlen", "n_videos", "n_blocks", "lpad", "cn_src_a", "f2_src_a",
                "mask_src_a", "cn_src_b", "f2_src_b", "mask_src_b", "cn_a", "f2_a", "mask_a", "cn_b", "f2_b", "mask_b", "l",
                "hidden", "dt"]


def _gather(lib, base=GATHER, **kw):
    a = dict(base, **kw)
    return lib.xml_index_gather_video_rows(*[a[k] for k in GATHER_ORDER], Z)


def test_gather_rejects_bad_arguments(lib):
    src = _code(HEADER)
    names = [p.split()[-1].lstrip("*") for p in re.search(r"\bxml_index_gather_video_rows\s*\(([^)]*)\)", src).group(1).split(",")]
    assert names == GATHER_ORDER + ["stream"]
    assert _gather(lib) == UNSUPPORTED
    assert _gather(lib, form=ROWS, dt=F32, first_block=Z, n_blocks=0) == UNSUPPORTED       # row-major: no block operands
    assert _gather(lib, form=ROWS, first_block=Z, n_blocks=-4) == UNSUPPORTED
    assert _gather(lib, l=128) == UNSUPPORTED and _gather(lib, l=1) == UNSUPPORTED
    for k in ("slot", "first_block", "vlen", "cn_src_a", "f2_src_a", "mask_src_a", "cn_src_b", "f2_src_b", "mask_src_b", "cn_a",
              "f2_a", "mask_a", "cn_b", "f2_b", "mask_b"):
        assert _gather(lib, **{k: Z}) == BAD_ARG, k
    for k in ("n", "l", "lpad", "hidden", "n_videos", "n_blocks"):
        assert _gather(lib, **{k: 0}) == BAD_ARG and _gather(lib, **{k: -3}) == BAD_ARG, k
    assert _gather(lib, l=129) == BAD_ARG and _gather(lib, lpad=64) == BAD_ARG         # l > lpad
    for n_mod in (0, 3, -1):
        assert _gather(lib, n_mod=n_mod) == BAD_ARG
    for form in (2, -1):
        assert _gather(lib, form=form) == BAD_ARG
    for dt in (F16, F16S, -1, 4):
        assert _gather(lib, dt=dt) == BAD_ARG, dt
    for k in ("cn_src_a", "f2_src_a", "cn_a", "f2_a", "cn_src_b", "f2_src_b", "cn_b", "f2_b"):       # 16-byte loads and stores
        assert _gather(lib, **{k: ctypes.c_void_p(0x1008)}) == BAD_ARG, k
    assert _gather(lib, mask_a=ctypes.c_void_p(0x1004), mask_src_b=ctypes.c_void_p(0x1004)) == UNSUPPORTED
    # widths: the block image takes rows of whole 64-byte slices, row-major rows hidden % 8 == 0; neither more than 4096
    for hidden, dt in ((100, BF16), (72, F32), (4100, F32), (4128, BF16)):
        assert _gather(lib, hidden=hidden, dt=dt) == UNSUPPORTED, (hidden, dt)
    assert _gather(lib, form=ROWS, hidden=100) == UNSUPPORTED and _gather(lib, form=ROWS, hidden=4100, dt=F32) == UNSUPPORTED


def test_gather_with_one_modality_ignores_the_second_side(lib):
    one = dict(GATHER, n_mod=1, cn_src_b=Z, f2_src_b=Z, mask_src_b=Z, cn_b=Z, f2_b=Z, mask_b=Z)
    assert _gather(lib, one) == UNSUPPORTED
    assert _gather(lib, one, cn_src_b=ctypes.c_void_p(0x1001), f2_b=ctypes.c_void_p(0x1002)) == UNSUPPORTED
    for k in ("slot", "first_block", "vlen", "cn_src_a", "f2_src_a", "mask_src_a", "cn_a", "f2_a", "mask_a"):
        assert _gather(lib, one, **{k: Z}) == BAD_ARG, k
    assert _gather(lib, one, n=0) == BAD_ARG and _gather(lib, one, dt=F16) == BAD_ARG and _gather(lib, one, l=129) == BAD_ARG


# ---- xml_q2c_scores_arg_bwd_q: nq = 1025 > 1024 -> UNSUPPORTED behind the argument checks -----------------------------------
def _vp(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _scores(lib, n_mod=2, nq=1025, nv=7, l=(19, 19), hidden=128, dt=BF16, ld_ds=7, ld_arg=7, null=None, null_entry=None,
            dscores=P):
    ptr = lambda name: None if null == name else _vp(*[0 if null_entry == (name, m) else 0x1000 for m in range(n_mod)])  # noqa: E731
    return lib.xml_q2c_scores_arg_bwd_q(n_mod, ptr("query"), ptr("qn"), ptr("cn"), ptr("mask"), dscores, ld_ds, 0.5, ptr("dq"), nq,
                                        nv, None if null == "l" else (ctypes.c_int * n_mod)(*l[:n_mod]), hidden, ptr("arg"), ld_arg,
                                        dt, Z)


def test_scores_bwd_q_rejects_bad_arguments(lib):
    assert _scores(lib) == UNSUPPORTED and _scores(lib, n_mod=1) == UNSUPPORTED
    assert _scores(lib, nq=7, nv=1025, ld_ds=1025, ld_arg=1025) == UNSUPPORTED
    for name in ("query", "qn", "cn", "mask", "dq", "arg", "l"):
        assert _scores(lib, null=name) == BAD_ARG, name
    for name in ("query", "qn", "cn", "mask", "dq", "arg"):
        for m in (0, 1):
            assert _scores(lib, null_entry=(name, m)) == BAD_ARG, (name, m)
        assert _scores(lib, n_mod=1, null_entry=(name, 1)) == UNSUPPORTED           # one modality: entry 1 does not exist
    assert _scores(lib, dscores=Z) == BAD_ARG
    assert lib.xml_q2c_scores_arg_bwd_q(0, _vp(0x1000), _vp(0x1000), _vp(0x1000), _vp(0x1000), P, 7, 0.5, _vp(0x1000), 7, 7,
                                        (ctypes.c_int * 1)(19), 128, _vp(0x1000), 7, BF16, Z) == BAD_ARG
    assert lib.xml_q2c_scores_arg_bwd_q(3, _vp(0x1000), _vp(0x1000), _vp(0x1000), _vp(0x1000), P, 7, 0.5, _vp(0x1000), 7, 7,
                                        (ctypes.c_int * 1)(19), 128, _vp(0x1000), 7, BF16, Z) == BAD_ARG
    assert _scores(lib, ld_ds=6) == BAD_ARG and _scores(lib, ld_arg=6) == BAD_ARG
    # the limits are those of xml_q2c_scores_l2norm_bwd_supported, asked of the library
    for kw in (dict(nq=7, hidden=100), dict(nq=7, hidden=2056), dict(nq=7, dt=F16), dict(nq=7, dt=F16S), dict(nq=7, l=(19, 0)),
               dict(nq=0), dict(nq=7, nv=0, ld_ds=0, ld_arg=0)):
        a = dict(nq=1025, nv=7, l=(19, 19), hidden=128, dt=BF16)
        a.update(kw)
        assert not all(lib.xml_q2c_scores_l2norm_bwd_supported(a["nq"], a["nv"], x, a["hidden"], a["dt"]) for x in a["l"])
        assert _scores(lib, **kw) == UNSUPPORTED, kw


# ---- xml_pair_sim_bwd_q: hidden = 2056 > 2048 -> UNSUPPORTED behind the argument checks ------------------------------------
def _pair(lib, f2=P, dsim=P, dq=P, n=6, l=23, hidden=2056, dt=BF16):
    return lib.xml_pair_sim_bwd_q(f2, dsim, dq, n, l, hidden, dt, Z)


def test_pair_sim_bwd_q_rejects_bad_arguments(lib):
    assert _pair(lib) == UNSUPPORTED and _pair(lib, dt=F32) == UNSUPPORTED
    assert _pair(lib, hidden=100) == UNSUPPORTED and _pair(lib, hidden=4) == UNSUPPORTED
    for k in ("f2", "dsim", "dq"):
        assert _pair(lib, **{k: Z}) == BAD_ARG, k
    for k in ("n", "l", "hidden"):
        assert _pair(lib, **{k: 0}) == BAD_ARG and _pair(lib, **{k: -2}) == BAD_ARG, k
    for dt in (F16, F16S, -1, 4):
        assert _pair(lib, dt=dt) == BAD_ARG, dt


def test_build_script_knows_the_header_and_the_source():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    assert "../../include/xmlhip_train_index.h -nt" in sh, "the header is part of the staleness checks"
    assert "loss_rows.h -nt" in sh, "the header loss_tail.hip and train_index.hip share is part of the staleness checks"
    srcs = re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "train_index.hip" in srcs and "loss_tail.hip" in srcs


def test_the_wrappers_and_the_ops_contract():
    from tvretrieval_amd import inference, ops, train_ops
    assert list(inspect.signature(ops.index_gather_video_rows).parameters) == [
        "slots", "first_block", "vlen", "cn_src", "f2_src", "mask_src", "length", "n_blocks", "out"]
    assert list(inspect.signature(train_ops.q2c_scores_arg_bwd_q).parameters) == ["sets", "dscores", "scale"]
    assert list(inspect.signature(train_ops.pair_sim_bwd_q).parameters) == ["f2", "dsim"]
    assert "index_gather_video_rows" not in inference.OPS_CONTRACT
