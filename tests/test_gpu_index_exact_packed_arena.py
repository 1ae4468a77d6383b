"""Guard-band cases of include/xmlhip_index_exact_packed.h (xml_index_put_rows_packed_exact) through tests/abi_arena.py, in
the manner of tests/test_gpu_index_exact_arena.py and tests/test_gpu_index_packed_arena.py: the status, untouched guard bytes
around every operand, independence of the arena's fill, bitwise the values of the ops.* wrapper -- and, beyond the wrapper,
what the header says about the runs, the codes, the slots the call does not name and the other modality's bound cell.
Both exact modes at H = 256 (the smallest hidden size whose bf16 rows have a tile image), capacity 37, 5 tiles."""
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, G, I32, I64, _allow_words, _ops, _st, _take_state, prefix_mask, put_all, randn

pytestmark = pytest.mark.gpu

CAP, N_TILES, LB, HIDDEN, L_REF = 37, 5, 21, 256, 125        # two live words; 80 blocks
SLOTS, IDS = [3, 36, 5, 31], [900, 901, 902, 903]            # slots 3, 5, 31 share live word 0, slot 36 is the last
# blocks 6 | 7 | 8 of tile 0 (a straddle), block 9 (shares a mask word with block 8), the image's last block, tile 1's first two
RUNS = [[6, 3], [9, 1], [79, 1], [16, 2]]
SIDE = ("k6", "rescore", "rescore_inv", "feat2", "feat2_inv", "err", "imask", "bits")
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _state_names(split):
    side = [n for n in SIDE if split or not n.endswith("_inv")]
    return tuple(n + "_" + m for m in "ab" for n in side) + ("codes", "ec", "vlen", "slot_ids", "live")


def _put_case(split):
    names = _state_names(split)

    def inputs():
        from tvretrieval_amd import _lib
        g = G(311)
        d = {"vlen": torch.randint(1, 129, (CAP,), generator=g).to(I32),
             "slot_ids": torch.randint(0, 10 ** 6, (CAP,), generator=g).to(I32),
             "live": torch.tensor([0x0F0F00F1, 0x00000001], dtype=I64).to(I32),
             "codes": torch.randint(-3, CAP, (2 * N_TILES, 8), generator=g).to(I32),
             "ec": torch.tensor([1e-4, 0.5])}         # the first cell is raised, the second (larger than any norm) stays
        n_k6 = int(_lib.load().xml_q2c_tiled_bytes(N_TILES * 256, HIDDEN, 1)) // 2
        for m in "ab":                                # arbitrary previous occupants everywhere
            d["k6_" + m] = randn(g, n_k6, dtype=BF16)
            for nm in ("rescore_", "feat2_"):
                d[nm + m] = torch.randint(-2 ** 31, 2 ** 31, (CAP, 128, HIDDEN), generator=g).to(I32) if split else \
                    randn(g, CAP, 128, HIDDEN)
                if split:
                    d[nm + "inv_" + m] = torch.rand(CAP, 128, generator=g)
            d["err_" + m] = torch.rand(CAP, 128, generator=g) * 1e-3
            d["imask_" + m] = (torch.rand(CAP, 128, generator=g) < 0.5).float()
            d["bits_" + m] = _allow_words(g, 2 * N_TILES, 4)
        for m, lens in (("a", [21, 1, 9, 21]), ("b", [20, 3, 9, 1])):
            d["f1_" + m], d["f2_" + m] = randn(g, 4, LB, HIDDEN), randn(g, 4, LB, HIDDEN, scale=3.0)
            d["mask_" + m] = prefix_mask(lens, LB)
        d["mask_b"][3] = prefix_mask([21], LB)[0]     # video 3: 21 clips of modality b in a 2-block run
        d["mask_a"][2] = prefix_mask([19], LB)[0]     # video 2: 19 clips in a ONE-block run: cut at 16 (keep < lb)
        d["f2_a"][2, 4] = 0.0                         # a zero row inside the batch: scale 1, halves 0
        d["slots"], d["ids"] = torch.tensor(SLOTS, dtype=I32), torch.tensor(IDS, dtype=I32)
        d["runs"] = torch.tensor(RUNS, dtype=I32)
        return d

    def raw(lib, A, inp):
        f1a, f2a, ma, f1b, f2b, mb, slots, ids, runs = put_all(
            A, inp, ("f1_a", "f2_a", "mask_a", "f1_b", "f2_b", "mask_b", "slots", "ids", "runs"))
        s = _take_state(A, inp, names)
        side = [P(s.get(n + "_" + m)) for m in "ab" for n in SIDE]
        st = lib.xml_index_put_rows_packed_exact(2, int(split), P(f1a), P(f2a), P(ma), P(f1b), P(f2b), P(mb), P(slots), P(ids),
                                                 P(runs), 4, LB, 3, *side, P(s["codes"]), P(s["ec"]), P(s["vlen"]),
                                                 P(s["slot_ids"]), P(s["live"]), CAP, N_TILES, 128, L_REF, HIDDEN, 0, _st())
        return st, s

    def wrap(inp):
        o = _ops()
        s = {nm: inp[nm].clone() for nm in names}
        k6 = [o.TiledRows(s["k6_" + m], CAP * 128, HIDDEN, (CAP, 128, HIDDEN)) for m in "ab"]
        rows = lambda nm: [o.SplitRows(s[nm + "_" + m], s[nm + "_inv_" + m]) if split else s[nm + "_" + m] for m in "ab"]   # noqa: E731
        o.index_put_rows_packed_exact([inp["f1_a"], inp["f1_b"]], [inp["f2_a"], inp["f2_b"]], [inp["mask_a"], inp["mask_b"]],
                                      inp["slots"], inp["ids"], inp["runs"], 3, k6, rows("rescore"), rows("feat2"),
                                      [s["err_a"], s["err_b"]], [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]],
                                      s["codes"], s["ec"], s["vlen"], s["slot_ids"], s["live"], L_REF)
        return s

    CASES.append(Case("put_rows_packed_exact_%s_h%d" % ("f16s" if split else "f32", HIDDEN), ["xml_index_put_rows_packed_exact"],
                      inputs, raw, wrap, nbytes=1 << 26,
                      note="5 tiles; a straddling run, two runs in one mask word, the image's last block; slots 3, 5, 31 share "
                           "a live word; lb = 21; one mask longer than its run"))


_put_case(False)
_put_case(True)


def test_the_entry_has_a_case():
    from tvretrieval_amd import _lib
    assert {s for c in CASES for s in c.symbols} == set(_lib.SIGNATURES_EXACT_PACKED)


def _image_rows(flat):
    """(N_TILES * 256, H) rows of a flat bf16 tile image."""
    return flat.view(N_TILES, HIDDEN // 32, 256, 32).permute(0, 2, 1, 3).reshape(N_TILES * 256, HIDDEN)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_packed_exact_entry(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    others = torch.tensor([s for s in range(CAP) if s not in SLOTS])
    in_run = torch.zeros(N_TILES * 256, dtype=torch.bool)
    touched = torch.zeros(N_TILES * 16, dtype=torch.bool)
    for first, nb in RUNS:
        in_run[first * 16:(first + nb) * 16] = True
        touched[first:first + nb] = True
    for nm, (v0, _, _, _) in host.items():
        was = inp[nm]
        if nm.startswith("k6_"):                                   # no row outside the runs is written
            assert torch.equal(_image_rows(v0)[~in_run].view(torch.int16), _image_rows(was)[~in_run].view(torch.int16)), nm
        elif nm.startswith("bits_") or nm in ("ec", "live", "codes"):
            continue
        else:                                                      # the per-slot operands of the slots the call does not name
            assert torch.equal(v0[others].view(torch.uint8), was[others].view(torch.uint8)), nm
    codes, before = host["codes"][0].reshape(-1), inp["codes"].reshape(-1)
    assert torch.equal(codes[~touched], before[~touched]), "codes outside the runs changed"
    assert codes[6:10].tolist() == [-1, -3, 3, 36] and codes[79] == 5 and codes[16:18].tolist() == [-1, 31]
    for m in "ab":
        err = host["err_" + m][0]
        assert bool((err[SLOTS, :LB] > 0).all()) and not bool(err[SLOTS, LB:].any()), m      # all lb rows, whatever the run
        rows = _image_rows(host["k6_" + m][0])
        for (first, nb), lens in zip(RUNS, (LB, LB, 16, LB)):       # zero from lb (from the run's end) on
            run = rows[first * 16:(first + nb) * 16].float()
            assert bool(run[:min(lens, 16 * nb)].any(1).all()) and not bool(run[lens:].any()), (m, first)
    bits = host["bits_a"][0].reshape(-1).numpy().view("uint32")
    old = inp["bits_a"].reshape(-1).numpy().view("uint32")
    # block 6 | 7: word 3 (21 clips: 16 + 5), block 8 | 9: word 4 (0 of video 0, 1 clip of video 1), block 79: the upper half
    # of word 39 (19 clips cut to 16), the lower half keeps the caller's bits
    assert bits[3] == 0x001FFFFF and bits[4] == 0x00010000 and bits[39] == (0xFFFF0000 | (old[39] & 0xFFFF))
    assert bits[8] == 0x001FFFFF and host["vlen"][0][5] == 16 and host["imask_a"][0][5].sum() == 16
    ec = host["ec"][0]
    assert float(ec[0]) == float(host["err_a"][0][SLOTS].max()) > 1e-4          # raised to the batch's largest norm
    assert float(ec[1]) == 0.5                                                   # a cell above every norm stays
    assert host["slot_ids"][0][SLOTS].tolist() == IDS
    live = host["live"][0].numpy().view("uint32")
    assert live[0] == (0x0F0F00F1 | 1 << 3 | 1 << 5 | 1 << 31) and live[1] == (1 | 1 << 4)
