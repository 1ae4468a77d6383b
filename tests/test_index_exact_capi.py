"""The C ABI of exact-rank mode on an updatable index (include/xmlhip_index_exact.h: xml_index_put_rows_exact,
xml_exact_certificate_dev, xml_index_exact_bound) without a GPU: the header declares exactly those functions, they are
exported and bound, and every bad-argument class returns before a launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xmlhip_index_exact.h")
BAD_ARG, UNSUPPORTED = -1, -2
F32, F16S = 0, 1                 # XML_EXACT_F32 / XML_EXACT_F16S


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_header_symbols_are_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))
    assert syms == ["xml_exact_certificate_dev", "xml_index_exact_bound", "xml_index_put_rows_exact"]
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_EXACT, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        assert fn.restype is _lib.SIGNATURES_EXACT[s][0] and list(fn.argtypes) == _lib.SIGNATURES_EXACT[s][1]   # bind() applied it
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES_EXACT[s][1]), s
    assert set(_lib.SIGNATURES_EXACT) == set(syms)
    assert not set(_lib.SIGNATURES_EXACT) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_INDEX) | set(_lib.SIGNATURES_COMPACT)
                                             | set(_lib.SIGNATURES_PARTS))
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    assert '#include "xmlhip.h"' in src
    assert re.search(r"#define\s+XML_EXACT_F32\s+0\b", src) and re.search(r"#define\s+XML_EXACT_F16S\s+1\b", src)
    assert "NaN" in text and "+inf" in text                     # the header says what a NaN norm does to the bound


def test_the_build_knows_the_new_source_and_headers():
    sh = open(os.path.join(ROOT, "tvretrieval_amd", "csrc", "build.sh")).read()
    assert "index_update_exact.hip" in re.search(r'^SRCS="([^"]*)"', sh, flags=re.M).group(1).split()
    assert "xmlhip_index_exact.h -nt" in sh and "split16.h -nt" in sh


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)
SIDE = ("k6", "rescore", "rescore_inv", "feat2", "feat2_inv", "err", "imask", "bits")


def _put(lib, n_mod=2, mode=F16S, b=3, lb=100, capacity=70, lpad=128, l_ref=100, hidden=256, dt=0, tiled=1, null=(),
         second=P, inv=P):
    """xml_index_put_rows_exact with P everywhere except the names in `null`."""
    batch = dict(f1_a=P, f2_a=P, mask_a=P, f1_b=second, f2_b=second, mask_b=second, slots=P, ids=P)
    index = {}
    for sfx, p in (("_a", P), ("_b", second)):
        for name in SIDE:
            index[name + sfx] = (inv if p is P else p) if name.endswith("_inv") else p
    state = dict(ec=P, vlen=P, slot_ids=P, live=P)
    for name in null:
        d = batch if name in batch else index if name in index else state
        assert name in d, name
        d[name] = Z
    return lib.xml_index_put_rows_exact(n_mod, mode, *batch.values(), b, lb, *index.values(), *state.values(), capacity, lpad,
                                        l_ref, hidden, dt, tiled, Z)


def test_put_rows_exact_rejects_bad_arguments(lib):
    for name in ("f1_a", "f2_a", "mask_a", "slots", "k6_a", "rescore_a", "feat2_a", "err_a", "imask_a", "bits_a", "ec", "vlen",
                 "slot_ids", "live"):
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
    assert _put(lib, lpad=48, lb=49, l_ref=40, tiled=0) == BAD_ARG
    assert _put(lib, l_ref=0) == BAD_ARG and _put(lib, l_ref=129) == BAD_ARG
    assert _put(lib, capacity=0) == BAD_ARG
    assert _put(lib, null=["ids"], hidden=100) == UNSUPPORTED               # ids may be NULL (the slot number): stopped by the shape


def test_put_rows_exact_answers_unsupported_for_what_the_kernel_does_not_take(lib):
    for dt in (1, 2, 3):                                                    # the inputs are f32 rows
        assert _put(lib, dt=dt) == UNSUPPORTED, dt
    assert _put(lib, hidden=100) == UNSUPPORTED                             # not whole 64-byte slices
    assert _put(lib, hidden=8 * 32 * 4 + 64, tiled=0) == UNSUPPORTED        # rows longer than l2norm.h takes
    assert _put(lib, hidden=128, tiled=1) == UNSUPPORTED                    # bf16 rows of 256 bytes: no tiled K6 operand
    assert _put(lib, hidden=48, tiled=0, mode=F16S) == UNSUPPORTED          # split-f16 rows come in groups of 32
    assert _put(lib, lpad=48, lb=40, l_ref=40, tiled=1) == UNSUPPORTED      # the tile image holds 128-row slots only
    assert _put(lib, lpad=144, lb=100, l_ref=130, tiled=0) == UNSUPPORTED   # 4 mask words per slot: lpad <= 128
    assert _put(lib, lpad=40, lb=40, l_ref=40, tiled=0) == UNSUPPORTED      # lpad % 16
    assert lib.xml_q2c_tiled_ok(128, 256, 1) == 1 and lib.xml_q2c_tiled_ok(128, 128, 1) == 0
    assert lib.xml_q2c_tile_rows_l2norm_ok(48, 0) == 1


def test_put_rows_exact_with_one_modality_needs_no_second_side(lib):
    assert _put(lib, n_mod=1, second=Z, b=0) == BAD_ARG
    assert _put(lib, n_mod=1, second=Z, hidden=100) == UNSUPPORTED
    assert _put(lib, n_mod=1, second=Z, mode=F32, inv=Z, hidden=100) == UNSUPPORTED


def _cert(lib, m=20, k=10, n_mod=2, nq=12, ptrs=None):
    ptrs = ptrs or [P] * 9                      # filter_scores, top_val, eq0, eq1, ec, fail, eps_out, thr_out, n_fail
    return lib.xml_exact_certificate_dev(ptrs[0], m, ptrs[1], k, ptrs[2], ptrs[3], ptrs[4], n_mod, 1e-4, 4.0, 20.0, 1, ptrs[5],
                                         ptrs[6], ptrs[7], ptrs[8], nq, Z)


def test_certificate_dev_rejects_bad_arguments(lib):
    for i in (0, 1, 2, 3, 4, 5, 8):             # eps_out and thr_out are optional, as in xml_exact_certificate
        ptrs = [P] * 9
        ptrs[i] = Z
        assert _cert(lib, ptrs=ptrs) == BAD_ARG, i
    assert _cert(lib, nq=0) == BAD_ARG and _cert(lib, m=0) == BAD_ARG and _cert(lib, k=0) == BAD_ARG
    assert _cert(lib, k=21) == BAD_ARG
    assert _cert(lib, n_mod=0) == BAD_ARG and _cert(lib, n_mod=3) == BAD_ARG
    ptrs = [P] * 9
    ptrs[3] = Z                                 # one modality needs no eq1; stopped by the next bad argument
    assert _cert(lib, n_mod=1, nq=0, ptrs=ptrs) == BAD_ARG and _cert(lib, n_mod=2, ptrs=ptrs) == BAD_ARG


def _bound(lib, n_mod=2, capacity=70, lpad=128, ptrs=None):
    ptrs = ptrs or [P] * 4                      # err_a, err_b, live, ec
    return lib.xml_index_exact_bound(n_mod, ptrs[0], ptrs[1], ptrs[2], ptrs[3], capacity, lpad, Z)


def test_exact_bound_rejects_bad_arguments(lib):
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = Z
        assert _bound(lib, ptrs=ptrs) == BAD_ARG, i
    assert _bound(lib, n_mod=0) == BAD_ARG and _bound(lib, n_mod=3) == BAD_ARG
    assert _bound(lib, capacity=0) == BAD_ARG and _bound(lib, capacity=-1) == BAD_ARG and _bound(lib, lpad=0) == BAD_ARG
    assert _bound(lib, n_mod=1, ptrs=[P, Z, P, P], capacity=0) == BAD_ARG


def test_the_wrappers_are_hip_only_entries():
    from tvretrieval_amd import inference, ops
    for name in ("index_put_rows_exact", "exact_certificate_dev", "index_exact_bound"):
        assert callable(getattr(ops, name))
        assert name not in inference.OPS_CONTRACT
        assert name in inference.__doc__
    assert (ops.EXACT_F32, ops.EXACT_F16S) == (F32, F16S)
