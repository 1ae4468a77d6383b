"""Guard-band cases of the companion header include/xmlhip_index.h (xml_index_put_rows_packed, xml_index_clear_rows_packed)
through tests/abi_arena.py -- what tests/test_gpu_abi_arena.py holds for every entry of include/xmlhip.h, and what
tests/test_abi_arena.py would demand of these two if they stood there: the status, untouched guard bytes around every
operand, independence of the arena's fill, bitwise the values of the ops.* wrapper.  One case per entry and dtype."""
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F32, G, I32, I64, XDT, _allow_words, _ops, _st, _take_state, prefix_mask, put_all, randn

pytestmark = pytest.mark.gpu

CAP, N_TILES, LB = 37, 5, 21        # two live words; 80 blocks
SLOTS = [3, 36, 5, 31]              # slots 3, 5, 31 share live word 0, slot 36 is the last
# blocks 6 | 7 | 8 of tile 0 (a straddle), block 9 (shares a mask word with block 8), the image's last block, tile 1's first two
RUNS = [[6, 3], [9, 1], [79, 1], [16, 2]]
STATE = ("k6_a", "feat2_a", "imask_a", "bits_a", "k6_b", "feat2_b", "imask_b", "bits_b", "codes", "vlen", "slot_ids", "live")
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _state(g, hidden, dt):
    """A populated packed index (arbitrary previous contents) as CPU tensors."""
    from tvretrieval_amd import _lib
    n_k6 = int(_lib.load().xml_q2c_tiled_bytes(N_TILES * 256, hidden, XDT[dt])) // (2 if dt is BF16 else 4)
    d = {"vlen": torch.randint(1, 129, (CAP,), generator=g).to(I32), "slot_ids": torch.randint(0, 10 ** 6, (CAP,), generator=g).to(I32),
         "live": torch.tensor([0x0F0F00F1, 0x00000001], dtype=I64).to(I32),
         "codes": torch.randint(-3, CAP, (2 * N_TILES, 8), generator=g).to(I32)}
    for m in "ab":
        d["k6_" + m] = randn(g, n_k6, dtype=dt)
        d["feat2_" + m] = randn(g, CAP, 128, hidden, dtype=dt)
        d["imask_" + m] = (torch.rand(CAP, 128, generator=g) < 0.5).float()
        d["bits_" + m] = _allow_words(g, 2 * N_TILES, 4)
    return d


def _put_case(dt, hidden):
    l_ref = 125

    def inputs():
        g = G(178)
        d = _state(g, hidden, dt)
        for m, lens in (("a", [21, 1, 9, 21]), ("b", [20, 3, 9, 1])):
            d["f1_" + m], d["f2_" + m] = randn(g, 4, LB, hidden, dtype=dt), randn(g, 4, LB, hidden, dtype=dt)
            d["mask_" + m] = prefix_mask(lens, LB)
        d["mask_b"][3] = prefix_mask([21], LB)[0]                           # video 3: 21 clips of modality b in a 2-block run
        d["mask_a"][2] = prefix_mask([19], LB)[0]                           # video 2: 19 clips in a ONE-block run: cut at 16
        d["slots"], d["ids"] = torch.tensor(SLOTS, dtype=I32), torch.tensor([900, 901, 902, 903], dtype=I32)
        d["runs"] = torch.tensor(RUNS, dtype=I32)
        return d

    def raw(lib, A, inp):
        f1a, f2a, ma, f1b, f2b, mb, slots, ids, runs = put_all(
            A, inp, ("f1_a", "f2_a", "mask_a", "f1_b", "f2_b", "mask_b", "slots", "ids", "runs"))
        s = _take_state(A, inp, STATE)
        st = lib.xml_index_put_rows_packed(2, P(f1a), P(f2a), P(ma), P(f1b), P(f2b), P(mb), P(slots), P(ids), P(runs), 4, LB, 3,
                                           P(s["k6_a"]), P(s["feat2_a"]), P(s["imask_a"]), P(s["bits_a"]), P(s["k6_b"]),
                                           P(s["feat2_b"]), P(s["imask_b"]), P(s["bits_b"]), P(s["codes"]), P(s["vlen"]),
                                           P(s["slot_ids"]), P(s["live"]), CAP, N_TILES, 128, l_ref, hidden, XDT[dt], _st())
        return st, s

    def wrap(inp):
        o = _ops()
        s = {nm: inp[nm].clone() for nm in STATE}
        k6 = [o.TiledRows(s["k6_" + m], CAP * 128, hidden, (CAP, 128, hidden)) for m in "ab"]
        o.index_put_rows_packed([inp["f1_a"], inp["f1_b"]], [inp["f2_a"], inp["f2_b"]], [inp["mask_a"], inp["mask_b"]],
                                inp["slots"], inp["ids"], inp["runs"], 3, k6, [s["feat2_a"], s["feat2_b"]],
                                [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]], s["codes"], s["vlen"], s["slot_ids"],
                                s["live"], l_ref)
        return s

    CASES.append(Case("index_put_rows_packed_%s_h%d" % (DTN[dt], hidden), ["xml_index_put_rows_packed"], inputs, raw, wrap,
                      nbytes=1 << 25, note="5 tiles; a straddling run, two runs in one mask word, the image's last block; "
                                           "slots 3, 5, 31 share a live word; lb = 21; one mask longer than its run"))


def _clear_case():
    names = ("imask_a", "bits_a", "imask_b", "bits_b", "codes", "vlen", "live")

    def inputs():
        d = _state(G(179), 128, F32)
        d["live"] = torch.tensor([-1, 0x1F], dtype=I32)
        d["slots"] = torch.tensor([3, -1, 36, 31], dtype=I32)             # -1: the run alone
        d["runs"] = torch.tensor(RUNS, dtype=I32)
        return d

    def raw(lib, A, inp):
        slots, runs = put_all(A, inp, ("slots", "runs"))
        s = _take_state(A, inp, names)
        st = lib.xml_index_clear_rows_packed(2, P(slots), P(runs), 4, 8, P(s["imask_a"]), P(s["bits_a"]), P(s["imask_b"]),
                                             P(s["bits_b"]), P(s["codes"]), P(s["vlen"]), P(s["live"]), CAP, N_TILES, 128, 125, _st())
        return st, s

    def wrap(inp):
        s = {nm: inp[nm].clone() for nm in names}
        _ops().index_clear_rows_packed(inp["slots"], inp["runs"], 8, [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]],
                                       s["codes"], s["vlen"], s["live"], 125)
        return s

    CASES.append(Case("index_clear_rows_packed", ["xml_index_clear_rows_packed"], inputs, raw, wrap, nbytes=1 << 23,
                      note="three slots and one run alone; slots 3 and 31 share a live word, blocks 8 and 9 a mask word"))


_put_case(F32, 128)
_put_case(BF16, 256)
_clear_case()


def test_every_companion_entry_has_a_case():
    from test_index_packed_capi import header_symbols
    covered = {s for c in CASES for s in c.symbols}
    assert covered == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_packed_index(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    # beyond the wrapper's values (the same kernel): what the header says about codes, live and the dropped nothing
    codes = host["codes"][0].reshape(-1)
    inp = case.inputs()
    before = inp["codes"].reshape(-1)
    touched = torch.zeros(N_TILES * 16, dtype=torch.bool)
    for first, nb in RUNS:
        touched[first:first + nb] = True
    assert torch.equal(codes[~touched], before[~touched]), "codes outside the runs changed"
    if case.name.startswith("index_put"):
        assert codes[6:10].tolist() == [-1, -3, 3, 36] and codes[79] == 5 and codes[16:18].tolist() == [-1, 31]
        bits = host["bits_a"][0].reshape(-1).numpy().view("uint32")
        old = inp["bits_a"].reshape(-1).numpy().view("uint32")
        # block 6 | 7: word 3 (21 clips: 16 + 5), block 8 | 9: word 4 (0 of video 0, 1 clip of video 1), block 79: the upper half
        # of word 39 (19 clips cut to 16), the lower half keeps the caller's bits
        assert bits[3] == 0x001FFFFF and bits[4] == 0x00010000 and bits[39] == (0xFFFF0000 | (old[39] & 0xFFFF))
        assert bits[8] == 0x001FFFFF and host["vlen"][0][5] == 16 and host["imask_a"][0][5].sum() == 16
        live = host["live"][0].numpy().view("uint32")
        assert live[0] == (0x0F0F00F1 | 1 << 3 | 1 << 5 | 1 << 31) and live[1] == (1 | 1 << 4)
    else:
        assert (codes[touched] == -2).all()
        live = host["live"][0].numpy().view("uint32")
        assert live[0] == (0xFFFFFFFF & ~(1 << 3 | 1 << 31)) and live[1] == 0x0F
        assert torch.equal(host["vlen"][0][[3, 31, 36]], torch.full((3,), 125, dtype=I32))
