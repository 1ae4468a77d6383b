"""The C ABI of the packed form of the updatable index (include/xmlhip_index.h: xml_index_put_rows_packed,
xml_index_clear_rows_packed) without a GPU: what tests/test_capi.py asks of include/xmlhip.h -- every declared function is
exported and bound, nothing else is bound -- and the argument validation that comes before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "xmlhip_index.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src)))


def test_every_companion_header_symbol_is_exported_and_bound(lib):
    from tvretrieval_amd import _lib
    syms = header_symbols()
    assert syms == ["xml_index_clear_rows_packed", "xml_index_put_rows_packed"]
    for s in syms:
        assert hasattr(lib, s), "libxmlhip.so does not export %s" % s
        assert s in _lib.SIGNATURES_INDEX, "ctypes binding missing for %s" % s
        fn = getattr(lib, s)
        assert fn.restype is _lib.SIGNATURES_INDEX[s][0] and list(fn.argtypes) == _lib.SIGNATURES_INDEX[s][1]      # load() applied it
    assert set(_lib.SIGNATURES_INDEX) == set(syms)
    assert not set(_lib.SIGNATURES_INDEX) & set(_lib.SIGNATURES)
    assert lib.xml_abi_version() == _lib.ABI_VERSION == 6
    # the header's parameter lists are as long as the bound ones
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xmlhip_index.h")).read(), flags=re.S)
    for s in syms:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES_INDEX[s][1]), s
    assert '#include "xmlhip.h"' in src


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)


def _put(lib, n_mod=2, b=3, lb=100, nb_max=7, capacity=70, n_tiles=24, lpad=128, l_ref=100, hidden=128, dt=0, null=(), second=P):
    batch = [P, P, P, second, second, second, P, P, P]           # f1_a f2_a mask_a f1_b f2_b mask_b slots ids runs
    index = [P, P, P, P, second, second, second, second, P, P, P, P]   # k6_a .. bits_a, k6_b .. bits_b, codes vlen slot_ids live
    for kind, i in null:
        (batch if kind == "batch" else index)[i] = Z
    return lib.xml_index_put_rows_packed(n_mod, *batch, b, lb, nb_max, *index, capacity, n_tiles, lpad, l_ref, hidden, dt, Z)


def test_put_rows_packed_rejects_bad_arguments(lib):
    for i in (0, 1, 2, 6, 8):                                    # f1_a, f2_a, mask_a, slots, runs (ids may be NULL)
        assert _put(lib, null=[("batch", i)]) == BAD_ARG, i
    for i in (0, 1, 2, 3, 8, 9, 10, 11):                         # k6_a, feat2_a, imask_a, bits_a, codes, vlen, slot_ids, live
        assert _put(lib, null=[("index", i)]) == BAD_ARG, i
    assert _put(lib, second=Z) == BAD_ARG                        # two modalities, the second one missing
    assert _put(lib, n_mod=0) == BAD_ARG and _put(lib, n_mod=3) == BAD_ARG
    assert _put(lib, b=0) == BAD_ARG and _put(lib, b=-2) == BAD_ARG
    assert _put(lib, b=71) == BAD_ARG                            # more videos than slots: they cannot be distinct
    assert _put(lib, nb_max=0) == BAD_ARG and _put(lib, nb_max=9) == BAD_ARG and _put(lib, nb_max=-1) == BAD_ARG
    assert _put(lib, lpad=112) == BAD_ARG and _put(lib, lpad=48, lb=40, l_ref=40) == BAD_ARG and _put(lib, lpad=256) == BAD_ARG
    assert _put(lib, dt=2) == BAD_ARG and _put(lib, dt=3) == BAD_ARG and _put(lib, dt=-1) == BAD_ARG      # f16, split f16
    assert _put(lib, lb=129) == BAD_ARG and _put(lib, lb=0) == BAD_ARG
    assert _put(lib, l_ref=0) == BAD_ARG and _put(lib, l_ref=129) == BAD_ARG
    assert _put(lib, capacity=0) == BAD_ARG and _put(lib, n_tiles=0) == BAD_ARG
    # a hidden size the tiled K6 operand / l2norm.h does not take: bf16 rows of 128 are 256 bytes, below the kernel's 384
    assert _put(lib, hidden=128, dt=1) == UNSUPPORTED and _put(lib, hidden=100) == UNSUPPORTED
    # one modality needs no second side; stopped by the one remaining bad argument
    assert _put(lib, n_mod=1, second=Z, b=0) == BAD_ARG and _put(lib, n_mod=1, second=Z, nb_max=9) == BAD_ARG


def _clear(lib, n_mod=2, n=2, nb_max=8, capacity=70, n_tiles=24, lpad=128, l_ref=100, ptrs=None):
    ptrs = ptrs or [P] * 9                                       # slots, runs, imask_a, bits_a, imask_b, bits_b, codes, vlen, live
    return lib.xml_index_clear_rows_packed(n_mod, ptrs[0], ptrs[1], n, nb_max, *ptrs[2:], capacity, n_tiles, lpad, l_ref, Z)


def test_clear_rows_packed_rejects_bad_arguments(lib):
    for i in range(9):
        ptrs = [P] * 9
        ptrs[i] = Z
        assert _clear(lib, ptrs=ptrs) == BAD_ARG, i
    assert _clear(lib, n_mod=0) == BAD_ARG and _clear(lib, n_mod=3) == BAD_ARG
    assert _clear(lib, n=0) == BAD_ARG and _clear(lib, n=-1) == BAD_ARG
    assert _clear(lib, nb_max=0) == BAD_ARG and _clear(lib, nb_max=9) == BAD_ARG
    assert _clear(lib, lpad=112) == BAD_ARG and _clear(lib, lpad=48, l_ref=40) == BAD_ARG
    assert _clear(lib, capacity=0) == BAD_ARG and _clear(lib, n_tiles=0) == BAD_ARG
    assert _clear(lib, l_ref=0) == BAD_ARG and _clear(lib, l_ref=129) == BAD_ARG
    assert _clear(lib, n_mod=1, ptrs=[P, P, P, P, Z, Z, P, P, P], n=0) == BAD_ARG


def test_the_wrappers_are_hip_only_entries():
    from tvretrieval_amd import inference, ops
    assert callable(ops.index_put_rows_packed) and callable(ops.index_clear_rows_packed)
    assert "index_put_rows_packed" not in inference.OPS_CONTRACT and "index_clear_rows_packed" not in inference.OPS_CONTRACT
