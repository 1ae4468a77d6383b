"""Guard-band cases of include/xmlhip_index_parts.h (xml_index_set_chains, xml_chain_best_allow, xml_chain_best_rows)
through tests/abi_arena.py, in the manner of tests/test_gpu_index_compact_arena.py: the status, untouched guard bytes around
every operand, independence of the arena's fill, bitwise the values of the ops.* wrapper.  The three entries at their
extents write nothing outside out_bits, out and the three tables: the row gaps of out_bits (out_ld = words + 2) are guard
bytes, as are the gaps of the strided scores and allow words."""
import types

import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import DEV, G, I32, _allow_words, _ops, _st, _take_state, put_all, randn

pytestmark = pytest.mark.gpu

CAP, MAX_PARTS, ROWS = 77, 6, 6                                   # three bit words, 13 valid bits in the last one
WORDS = (CAP + 31) // 32
CHAINS = [[3, 76, 31, 32], [64, 63], [40, 7, 70, 0, 33, 65], [10, 11, 12, 13, 14]]      # 6 = max_parts; 5 > the register slots
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _chain_tables():
    head, nxt = torch.arange(CAP, dtype=I32), torch.full((CAP,), -1, dtype=I32)
    for ch in CHAINS:
        for j, s in enumerate(ch):
            head[s] = ch[0]
            nxt[s] = ch[j + 1] if j + 1 < len(ch) else -1
    return head, nxt


def _scores(g):
    s = randn(g, ROWS, CAP)
    s[0, [3, 76]] = float(s[0, 31])                                    # ties
    s[1, 7] = float("nan")
    s[2, [10, 11, 12, 13, 14]] = float("-inf")
    alone = torch.ones(CAP, dtype=torch.bool)
    alone[[x for ch in CHAINS for x in ch]] = False
    s[:, alone] = float("nan")                                     # chains of one slot: never read
    return s


def _tables_of(inp):
    return types.SimpleNamespace(chain_head=inp["chain_head"], chain_next=inp["chain_next"], max_parts=MAX_PARTS)


def _set_chains():
    records = [[3, 3, 76, 0], [76, 3, 31, 16], [31, 3, 32, 32], [CAP, 1, 2, 3], [32, 3, -1, 41], [-1, 4, 5, 6], [CAP - 1 + 100, 7, 8, 9],
               [0, 0, -1, 0], [75, 74, -1, 5]]
    state = ("chain_head", "chain_next", "chain_offset")

    def inputs():
        g = G(191)
        d = {nm: torch.randint(-5, CAP + 5, (CAP,), generator=g).to(I32) for nm in state}     # arbitrary previous contents
        d["records"] = torch.tensor(records, dtype=I32)
        return d

    def raw(lib, A, inp):
        (rec,) = put_all(A, inp, ("records",), skew=4)             # (the records need no 16-byte alignment)
        s = _take_state(A, inp, state)
        st = lib.xml_index_set_chains(P(rec), len(records), P(s["chain_head"]), P(s["chain_next"]), P(s["chain_offset"]), CAP, _st())
        return st, s

    def wrap(inp):
        s = {nm: inp[nm].clone() for nm in state}
        _ops().index_set_chains(inp["records"], s["chain_head"], s["chain_next"], s["chain_offset"])
        return s

    CASES.append(Case("index_set_chains", ["xml_index_set_chains"], inputs, raw, wrap,
                      note="9 records: the first and the last slot, three slots outside [0, capacity) that write nothing"))


def _chain_best_allow(skew, allow_rows):
    ld, out_ld, allow_ld = CAP + 3, WORDS + 2, WORDS + 1

    def inputs():
        g = G(192)
        head, nxt = _chain_tables()
        return {"scores": _scores(g), "chain_head": head, "chain_next": nxt, "allow": _allow_words(g, allow_rows, WORDS)}

    def raw(lib, A, inp):
        s = A.put("scores", inp["scores"], ld=ld, skew=skew)
        head, nxt = put_all(A, inp, ("chain_head", "chain_next"))
        al = A.put("allow", inp["allow"], ld=allow_ld, skew=skew)
        out = A.take("bits", (ROWS, WORDS), I32, ld=out_ld, skew=skew)      # words beyond ceil(capacity / 32): guard bytes
        st = lib.xml_chain_best_allow(P(s), ld, ROWS, CAP, P(head), P(nxt), MAX_PARTS, P(al), allow_ld, allow_rows, P(out), out_ld,
                                      _st())
        return st, {"bits": out}

    def wrap(inp):
        return {"bits": _ops().chain_best_allow(inp["scores"], _tables_of(inp), inp["allow"])}

    CASES.append(Case("chain_best_allow_rows%d_skew%d" % (allow_rows, skew), ["xml_chain_best_allow"], inputs, raw, wrap,
                      note="77 slots: 3 bit words with 19 padding bits; ld = capacity + 3, out_ld = words + 2, allow_ld = words + 1"))


def _chain_best_rows():
    ld = CAP + 3

    def inputs():
        head, nxt = _chain_tables()
        return {"scores": _scores(G(193)), "chain_head": head, "chain_next": nxt,
                "video": torch.tensor([32, CAP - 2, -1, CAP, 65, CAP - 1], dtype=I32)}

    def raw(lib, A, inp):
        s = A.put("scores", inp["scores"], ld=ld, skew=4)
        head, nxt, vid = put_all(A, inp, ("chain_head", "chain_next", "video"))
        out = A.take("out", (ROWS,), I32)
        return lib.xml_chain_best_rows(P(s), ld, ROWS, CAP, P(head), P(nxt), MAX_PARTS, P(vid), P(out), _st()), {"out": out}

    CASES.append(Case("chain_best_rows", ["xml_chain_best_rows"], inputs, raw,
                      lambda inp: {"out": _ops().chain_best_rows(inp["scores"], _tables_of(inp), inp["video"])},
                      note="ld = capacity + 3; the last slot (a part of a chain), a slot alone, slots one past the end and below zero"))


_set_chains()
for _skew in (0, 4):
    for _allow_rows in (1, ROWS):
        _chain_best_allow(_skew, _allow_rows)
_chain_best_rows()


def test_every_chain_entry_has_a_case():
    from test_index_parts_capi import header_symbols
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_chain_entries(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    if case.name == "index_set_chains":            # the header's words, beyond the wrapper (the same kernel)
        want = {nm: inp[nm].clone() for nm in ("chain_head", "chain_next", "chain_offset")}
        for s, h, n, o in inp["records"].tolist():
            if 0 <= s < CAP:
                want["chain_head"][s], want["chain_next"][s], want["chain_offset"][s] = h, n, o
        for nm, w in want.items():
            assert torch.equal(host[nm][0], w), nm
    if case.name == "chain_best_rows":
        out = host["out"][0].tolist()
        assert out[1:4] == [CAP - 2, -1, -1] and out[0] in (3, 76, 31, 32) and out[5] in (3, 76, 31, 32) and out[4] in CHAINS[2]
