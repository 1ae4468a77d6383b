"""Guard-band cases of include/xmlhip_index_compact.h (xml_index_move_blocks_packed) through tests/abi_arena.py, in the
manner of tests/test_gpu_index_packed_arena.py: the status, untouched guard bytes around every operand, independence of the
arena's fill, bitwise the values of the ops.* wrapper -- and, beyond the wrapper (the same kernel), the header's words: what
the numpy model of tests/test_block_table_compact.py says about codes and bits, block-for-block copies of the image, and a
dropped record that changes nothing.  One case per dtype."""
import numpy as np
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_block_table import ImageModel
from test_block_table_compact import apply_move
from test_gpu_abi_arena import BF16, DEV, DTN, F32, G, I32, XDT, _ops, _st, _take_state, put_all
from test_gpu_index_packed_arena import CAP, N_TILES, _state

pytestmark = pytest.mark.gpu

STATE = ("k6_a", "bits_a", "k6_b", "bits_b", "codes")
# tile 0: blocks 3..10 slide to 0..7 over their own old place, 8..10 become unused; tile 2 receives 25..28 of tile 1 (which
# has no record); tile 3: a src outside the image (80 = 16 * 5) -- dropped whole, the valid entries with it; tile 4, the LAST
# tile: its block 0 goes to its last block, block 14 comes from tile 1, block 0 becomes unused; a tile outside the image
RECORDS = [[0, 3, 4, 5, 6, 7, 8, 9, 10, -2, -2, -2, -1, -1, -1, -1, -1],
           [2, -1, -1, -1, -1, 25, 26, 27, 28, -1, -1, -1, -1, -1, -1, -1, -1],
           [3, 50, 51, -2, -1, -1, -1, -1, 80, -1, -1, -1, -1, -1, -1, -1, -1],
           [4, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 20, 64],
           [5, 0, 1, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1]]
LIVE = [RECORDS[0], RECORDS[1], RECORDS[3]]
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _case(dt, hidden):
    def inputs():
        d = _state(G(181), hidden, dt)
        d = {nm: d[nm] for nm in STATE}
        d["records"] = torch.tensor(RECORDS, dtype=I32)
        return d

    def raw(lib, A, inp):
        (records,) = put_all(A, inp, ("records",))
        s = _take_state(A, inp, STATE)
        st = lib.xml_index_move_blocks_packed(2, P(records), len(RECORDS), P(s["k6_a"]), P(s["bits_a"]), P(s["k6_b"]),
                                              P(s["bits_b"]), P(s["codes"]), N_TILES, hidden, XDT[dt], _st())
        return st, s

    def wrap(inp):
        o = _ops()
        s = {nm: inp[nm].clone() for nm in STATE}
        k6 = [o.TiledRows(s["k6_" + m], CAP * 128, hidden, (CAP, 128, hidden)) for m in "ab"]
        o.index_move_blocks_packed(inp["records"], k6, [s["bits_a"], s["bits_b"]], s["codes"])
        return s

    CASES.append(Case("index_move_blocks_packed_%s_h%d" % (DTN[dt], hidden), ["xml_index_move_blocks_packed"], inputs, raw, wrap,
                      nbytes=1 << 23, note="5 tiles; a slide over the run's own blocks, a cross-tile record, a record for the "
                                           "last tile, two records the device drops (a src and a tile outside the image)"))


_case(F32, 128)
_case(BF16, 256)


def test_the_compaction_entry_has_a_case():
    from test_index_compact_capi import header_symbols
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_move_blocks(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    # codes and bits: the numpy model (arbitrary previous contents: a source code >= 0 is carried, any other becomes -1 / -3)
    model = ImageModel(N_TILES)
    model.codes = inp["codes"].reshape(-1).numpy().astype(np.int64)
    for i, m in enumerate("ab"):
        w = inp["bits_" + m].reshape(-1).numpy().view(np.uint32).astype(np.int64)
        model.bits[i] = np.stack([w & 0xFFFF, w >> 16], 1).reshape(-1)
    apply_move(model, LIVE)
    assert (host["codes"][0].numpy() == model.code_table()).all()
    for i, m in enumerate("ab"):
        assert (host["bits_" + m][0].numpy() == model.words(i)).all(), m
    # the image: block-for-block copies, every other byte as before -- the dropped record's tile 3 among them
    for m in "ab":
        old = inp["k6_" + m].view(torch.uint8).view(N_TILES, -1, 16, 1024)         # (tile, slice, block, 1 KiB)
        want = old.clone()
        for rec in LIVE:
            for b, s in enumerate(rec[1:]):
                if s >= 0:
                    want[rec[0], :, b] = old[s // 16, :, s % 16]
        got = host["k6_" + m][0].view(torch.uint8).view(N_TILES, -1, 16, 1024)
        assert torch.equal(got, want), m
        assert torch.equal(got[3], old[3]) and torch.equal(got[1], old[1])
    assert torch.equal(host["codes"][0].reshape(-1)[48:64], inp["codes"].reshape(-1)[48:64])
    for m in "ab":
        assert torch.equal(host["bits_" + m][0].reshape(-1)[24:32], inp["bits_" + m].reshape(-1)[24:32])
