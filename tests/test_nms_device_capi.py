"""CPU-side checks of xml_nms_moments (temporal NMS on the device): the symbol is exported and bound, and the entry rejects
bad arguments before any launch (no GPU here, so a launch would fail differently)."""
import ctypes
import os

import pytest

BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbol_is_exported_bound_and_declared(lib):
    from tvretrieval_amd import _lib
    assert hasattr(lib, "xml_nms_moments")
    res, args = _lib.SIGNATURES["xml_nms_moments"]
    assert res is ctypes.c_int and len(args) == 16
    assert lib.xml_nms_moments.argtypes == args
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int xml_nms_moments(const xml_moment* in," in open(os.path.join(root, "include", "xmlhip.h")).read()
    assert lib.xml_abi_version() == 6          # additive: nothing existing changed signature


def _call(lib, inp=0x1000, ld_in=8, count=0, nq=2, n=8, by_video=1, thd=0.5, scale=1.0, max_before=8, max_after=4,
          out=0x2000, ld_out=4, out_index=0x3000, ld_index=4, out_count=0x4000):
    p = ctypes.c_void_p
    return lib.xml_nms_moments(p(inp), ld_in, p(count), nq, n, by_video, thd, scale, max_before, max_after, p(out), ld_out,
                               p(out_index), ld_index, p(out_count), p(0))


@pytest.mark.parametrize("bad", [
    dict(inp=0),                                        # in == NULL
    dict(out=0, out_index=0, out_count=0),              # all outputs NULL
    dict(n=0, ld_in=8),                                 # n = 0
    dict(n=1025, ld_in=1025),                           # n above xml_moment_topk's n_out limit
    dict(max_after=5, ld_out=4, ld_index=8),            # ld_out < max_after
    dict(max_after=5, ld_out=8, ld_index=4),            # ld_index < max_after
    dict(thd=float("nan")),                             # NaN thd
    dict(max_before=-1),
    dict(max_after=-1),
    dict(nq=-1),
    dict(ld_in=7),                                      # row stride below n
    dict(inp=0x1008),                                   # records not 16-byte aligned
], ids=["in_null", "no_output", "n_0", "n_1025", "ld_out", "ld_index", "nan_thd", "max_before_neg", "max_after_neg", "nq_neg",
        "ld_in", "misaligned"])
def test_bad_arguments_are_rejected_before_any_launch(lib, bad):
    assert _call(lib, **bad) == BAD_ARG


def test_empty_query_set_is_a_no_op(lib):
    assert _call(lib, nq=0) == 0
