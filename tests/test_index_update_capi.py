"""The two index-update entries (xml_index_put_rows, xml_index_clear_rows) validate their arguments before any launch:
-1 for null pointers / bad sizes, -2 for dtypes and shapes the kernel does not take.  No GPU needed."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


P = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before a launch
Z = ctypes.c_void_p(0)


def _put(lib, n_mod=2, b=3, lb=100, capacity=70, lpad=128, l_ref=100, hidden=128, dt=1, tiled=1, null=(), second=P):
    """xml_index_put_rows with P everywhere except the argument positions in `null` (0-based within the pointer lists)."""
    batch = [P, P, P, second, second, second, P, P]                        # f1_a f2_a mask_a f1_b f2_b mask_b slots ids
    index = [P, P, P, P, second, second, second, second, P, P, P]          # k6_a .. bits_a, k6_b .. bits_b, vlen slot_ids live
    for kind, i in null:
        (batch if kind == "batch" else index)[i] = Z
    return lib.xml_index_put_rows(n_mod, *batch, b, lb, *index, capacity, lpad, l_ref, hidden, dt, tiled, Z)


def test_put_rows_rejects_bad_arguments(lib):
    for i in (0, 1, 2, 6):                                                  # f1_a, f2_a, mask_a, slots
        assert _put(lib, null=[("batch", i)]) == -1, i
    for i in (0, 1, 2, 3, 8, 9, 10):                                        # k6_a, feat2_a, imask_a, bits_a, vlen, slot_ids, live
        assert _put(lib, null=[("index", i)]) == -1, i
    assert _put(lib, second=Z) == -1                                        # two modalities, the second one missing
    assert _put(lib, n_mod=0) == -1 and _put(lib, n_mod=3) == -1
    assert _put(lib, b=0) == -1 and _put(lib, b=-2) == -1
    assert _put(lib, b=71) == -1                                            # more videos than slots: they cannot be distinct
    assert _put(lib, lb=129) == -1 and _put(lib, lb=0) == -1                # lb > lpad
    assert _put(lib, lpad=48, lb=49, l_ref=40, tiled=0) == -1
    assert _put(lib, l_ref=0) == -1 and _put(lib, l_ref=129) == -1
    assert _put(lib, capacity=0) == -1


def test_put_rows_answers_unsupported_for_what_the_kernel_does_not_take(lib):
    assert _put(lib, dt=2) == -2 and _put(lib, dt=3) == -2                  # f16, split f16
    assert _put(lib, hidden=100) == -2                                      # not whole 64-byte slices
    assert _put(lib, hidden=8 * 32 * 8 + 32) == -2                          # rows longer than l2norm.h takes
    assert _put(lib, hidden=136, dt=0) == -2 and _put(lib, hidden=136, dt=1) == -2
    assert _put(lib, lpad=48, lb=40, l_ref=40, tiled=1) == -2               # the tile image holds 128-row slots only
    assert _put(lib, lpad=144, lb=100, l_ref=130, tiled=0) == -2            # 4 mask words per slot: lpad <= 128
    assert _put(lib, lpad=40, lb=40, l_ref=40, tiled=0) == -2               # lpad % 16
    for hidden in (128, 768):
        for dt in (0, 1):
            assert lib.xml_q2c_tile_rows_l2norm_ok(hidden, dt) == 1


def test_put_rows_with_one_modality_needs_no_second_side(lib):
    """n_mod == 1 with NULL second pointers passes validation; stopped here by the one remaining bad argument."""
    assert _put(lib, n_mod=1, second=Z, b=0) == -1
    assert _put(lib, n_mod=1, second=Z, hidden=100) == -2


def _clear(lib, n_mod=2, n=2, capacity=70, lpad=128, l_ref=100, ptrs=None):
    ptrs = ptrs or [P] * 7                                                  # slots, imask_a, bits_a, imask_b, bits_b, vlen, live
    return lib.xml_index_clear_rows(n_mod, ptrs[0], n, *ptrs[1:], capacity, lpad, l_ref, Z)


def test_clear_rows_rejects_bad_arguments(lib):
    for i in range(7):
        ptrs = [P] * 7
        ptrs[i] = Z
        assert _clear(lib, ptrs=ptrs) == -1, i
    assert _clear(lib, n_mod=0) == -1
    assert _clear(lib, n=0) == -1 and _clear(lib, n=71) == -1
    assert _clear(lib, capacity=0) == -1 and _clear(lib, l_ref=0) == -1 and _clear(lib, l_ref=129) == -1
    assert _clear(lib, lpad=144, l_ref=130) == -2 and _clear(lib, lpad=40, l_ref=40) == -2
    assert _clear(lib, n_mod=1, ptrs=[P, P, P, Z, Z, P, P], n=0) == -1


def test_the_wrappers_are_hip_only_entries():
    """ops.index_put_rows / index_clear_rows exist and are not part of the backend contract (the CPU stand-in has none)."""
    from tvretrieval_amd import inference, ops
    assert callable(ops.index_put_rows) and callable(ops.index_clear_rows)
    assert "index_put_rows" not in inference.OPS_CONTRACT and "index_clear_rows" not in inference.OPS_CONTRACT
