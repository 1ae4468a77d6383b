"""Guard-band cases of include/xmlhip_index_exact.h (xml_index_put_rows_exact, xml_exact_certificate_dev,
xml_index_exact_bound) through tests/abi_arena.py, in the manner of tests/test_gpu_index_parts_arena.py: the status,
untouched guard bytes around every operand, independence of the arena's fill, bitwise the values of the ops.* wrapper -- and,
beyond the wrapper, that the rows of the slots a put does not name, their err rows and the other modality's bound cell keep
what they held."""
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, F32, G, I32, I64, _allow_words, _ops, _st, _take_state, prefix_mask, put_all, randn

pytestmark = pytest.mark.gpu

CAP = 37                         # two live words; slots 3, 5 and 31 share word 0, slot 36 is the last
SLOTS, IDS = [3, 36, 5, 31], [900, 901, 902, 903]
SIDE = ("k6", "rescore", "rescore_inv", "feat2", "feat2_inv", "err", "imask", "bits")
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _state_names(split):
    side = [n for n in SIDE if split or not n.endswith("_inv")]
    return tuple(n + "_" + m for m in "ab" for n in side) + ("ec", "vlen", "slot_ids", "live")


def _put_exact(split, hidden, tiled):
    b, lb = 4, 21
    lpad = 128 if tiled else 48
    l_ref = lpad - 3
    names = _state_names(split)

    def inputs():
        from tvretrieval_amd import _lib
        g = G(301)
        d = {"vlen": torch.randint(1, lpad + 1, (CAP,), generator=g).to(I32),
             "slot_ids": torch.randint(0, 10 ** 6, (CAP,), generator=g).to(I32),
             "live": torch.tensor([0x0F0F00F1, 0x00000001], dtype=I64).to(I32),
             "ec": torch.tensor([1e-4, 0.5])}         # the first cell is raised, the second (larger than any norm) stays
        for m in "ab":                                # arbitrary previous occupants everywhere
            if tiled:
                d["k6_" + m] = randn(g, int(_lib.load().xml_q2c_tiled_bytes(CAP * 128, hidden, 1)) // 2, dtype=BF16)
            else:
                d["k6_" + m] = randn(g, CAP, lpad, hidden, dtype=BF16)
            for nm in ("rescore_", "feat2_"):
                d[nm + m] = torch.randint(-2 ** 31, 2 ** 31, (CAP, lpad, hidden), generator=g).to(I32) if split else \
                    randn(g, CAP, lpad, hidden)
                if split:
                    d[nm + "inv_" + m] = torch.rand(CAP, lpad, generator=g)
            d["err_" + m] = torch.rand(CAP, lpad, generator=g) * 1e-3
            d["imask_" + m] = (torch.rand(CAP, lpad, generator=g) < 0.5).float()
            d["bits_" + m] = _allow_words(g, CAP, 4)
        for m, lens in (("a", [21, 1, 9, 21]), ("b", [20, 3, 9, 1])):
            d["f1_" + m], d["f2_" + m] = randn(g, b, lb, hidden), randn(g, b, lb, hidden, scale=3.0)
            d["mask_" + m] = prefix_mask(lens, lb)
        d["f2_a"][2, 4] = 0.0                         # a zero row inside the batch: scale 1, halves 0
        d["slots"], d["ids"] = torch.tensor(SLOTS, dtype=I32), torch.tensor(IDS, dtype=I32)
        return d

    def raw(lib, A, inp):
        f1a, f2a, ma, f1b, f2b, mb, slots, ids = put_all(A, inp, ("f1_a", "f2_a", "mask_a", "f1_b", "f2_b", "mask_b", "slots", "ids"))
        s = _take_state(A, inp, names)
        side = [P(s.get(n + "_" + m)) for m in "ab" for n in SIDE]
        st = lib.xml_index_put_rows_exact(2, int(split), P(f1a), P(f2a), P(ma), P(f1b), P(f2b), P(mb), P(slots), P(ids), b, lb,
                                          *side, P(s["ec"]), P(s["vlen"]), P(s["slot_ids"]), P(s["live"]), CAP, lpad, l_ref,
                                          hidden, 0, int(tiled), _st())
        return st, s

    def wrap(inp):
        o = _ops()
        s = {nm: inp[nm].clone() for nm in names}
        k6 = [o.TiledRows(s["k6_" + m], CAP * 128, hidden, (CAP, 128, hidden)) if tiled else s["k6_" + m] for m in "ab"]
        rows = lambda nm: [o.SplitRows(s[nm + "_" + m], s[nm + "_inv_" + m]) if split else s[nm + "_" + m] for m in "ab"]   # noqa: E731
        o.index_put_rows_exact([inp["f1_a"], inp["f1_b"]], [inp["f2_a"], inp["f2_b"]], [inp["mask_a"], inp["mask_b"]],
                               inp["slots"], inp["ids"], k6, rows("rescore"), rows("feat2"), [s["err_a"], s["err_b"]],
                               [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]], s["ec"], s["vlen"], s["slot_ids"],
                               s["live"], l_ref)
        return s

    CASES.append(Case("put_rows_exact_%s_h%d_%s" % ("f16s" if split else "f32", hidden, "tiled" if tiled else "rowmajor"),
                      ["xml_index_put_rows_exact"], inputs, raw, wrap, nbytes=1 << 26,
                      note="capacity 37 (18.5 tiles), slots 3, 5, 31 share a live word, slot 36 is the last; lb = 21 < lpad = %d" % lpad))


def _certificate_dev(n_mod):
    nq, m, k = 70, 37, 10

    def inputs():
        g = G(302)
        return {"filter": randn(g, nq, m).sort(dim=1, descending=True).values, "top": randn(g, nq, k).sort(dim=1, descending=True).values,
                "eq0": torch.rand(nq, generator=g) * 1e-3, "eq1": torch.rand(nq, generator=g) * 1e-3,
                "ec": torch.tensor([1e-3, 2e-3][:n_mod])}

    def raw(lib, A, inp):
        f, e0, e1, ec = put_all(A, inp, ("filter", "eq0", "eq1", "ec"))
        top = A.take("top", (nq, k), F32)
        top.copy_(inp["top"])                                   # raw on entry, exp(alpha s) on return: an in-out operand
        nf = A.take("n_fail", (1,), I32)
        nf.zero_()                                              # zeroed by the caller
        fail, eps, thr = A.take("fail", (nq,), I32), A.take("eps", (nq,), F32), A.take("thr", (nq,), F32)
        st = lib.xml_exact_certificate_dev(P(f), m, P(top), k, P(e0), P(e1) if n_mod == 2 else None, P(ec), n_mod, 1e-6, 4.0, 20.0, 1,
                                           P(fail), P(eps), P(thr), P(nf), nq, _st())
        return st, {"top": top, "fail": fail, "eps": eps, "thr": thr, "n_fail": nf}

    def wrap(inp):
        top = inp["top"].clone()
        fail, eps, thr, nf = _ops().exact_certificate_dev(inp["filter"], top, [inp["eq0"], inp["eq1"]][:n_mod], inp["ec"], 1e-6, 4.0,
                                                          20.0, True)
        return {"top": top, "fail": fail, "eps": eps, "thr": thr, "n_fail": nf}

    CASES.append(Case("exact_certificate_dev_mod%d" % n_mod, ["xml_exact_certificate_dev"], inputs, raw, wrap,
                      note="nq = 70: a ragged block of queries; ec holds exactly n_mod floats, its neighbours are guard bytes"))


def _exact_bound(n_mod, lpad):
    def inputs():
        g = G(303)
        d = {"err_" + m: torch.rand(CAP, lpad, generator=g) for m in "ab"[:n_mod]}
        d["err_a"][4, 7] = 5.0                                  # a free slot's row: not counted
        d["live"] = torch.tensor([0x0F0F00E9, 0x00000010], dtype=I64).to(I32)      # slot 4 free, slot 36 (the last) live
        return d

    def raw(lib, A, inp):
        errs = put_all(A, inp, ["err_" + m for m in "ab"[:n_mod]])
        live = A.put("live", inp["live"])
        ec = A.take("ec", (n_mod,), F32)
        st = lib.xml_index_exact_bound(n_mod, P(errs[0]), P(errs[1]) if n_mod == 2 else None, P(live), P(ec), CAP, lpad, _st())
        return st, {"ec": ec}

    def wrap(inp):
        ec = torch.full((n_mod,), -1.0, device=DEV)
        _ops().index_exact_bound([inp["err_" + m] for m in "ab"[:n_mod]], inp["live"], ec)
        return {"ec": ec}

    CASES.append(Case("index_exact_bound_mod%d_lpad%d" % (n_mod, lpad), ["xml_index_exact_bound"], inputs, raw, wrap,
                      note="capacity 37: 5 padding bits in the second live word; ec holds exactly n_mod floats"))


_put_exact(False, 192, True)
_put_exact(True, 192, True)
_put_exact(False, 48, False)
_put_exact(True, 96, False)
_certificate_dev(1)
_certificate_dev(2)
_exact_bound(2, 128)
_exact_bound(1, 48)


def test_every_exact_entry_has_a_case():
    from tvretrieval_amd import _lib
    assert {s for c in CASES for s in c.symbols} == set(_lib.SIGNATURES_EXACT)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_exact_entries(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    if case.name.startswith("put_rows_exact"):
        # the header's words, beyond the wrapper (the same kernel): nothing of a slot the call does not name changes
        others = torch.tensor([s for s in range(CAP) if s not in SLOTS])
        hidden = inp["f1_a"].shape[2]
        rows = lambda t: _ops().TiledRows(t, CAP * 128, hidden, (CAP, 128, hidden)).to_rows()      # noqa: E731
        for nm, (v0, _, _, _) in host.items():
            if nm in ("ec", "live"):
                continue
            was = inp[nm]
            if nm.startswith("k6_") and v0.dim() == 1:             # the tiled filter image, read back slot by slot
                v0, was = rows(v0), rows(was)
            assert torch.equal(v0[others].view(torch.uint8), was[others].view(torch.uint8)), nm
        lpad = inp["imask_a"].shape[1]
        for m in "ab":
            err = host["err_" + m][0]
            assert bool((err[SLOTS, :21] > 0).all()) and not bool(err[SLOTS, 21:].any()), m      # rows beyond lb: zero rows
            k6 = host["k6_" + m][0]
            assert not bool((rows(k6) if k6.dim() == 1 else k6)[SLOTS, 21:].float().any())
        ec = host["ec"][0]
        assert float(ec[0]) == float(host["err_a"][0][SLOTS].max()) > 1e-4          # raised to the batch's largest norm
        assert float(ec[1]) == 0.5                                                   # a cell above every norm stays
        assert host["slot_ids"][0][SLOTS].tolist() == IDS
        live = host["live"][0].view(torch.int32).tolist()
        want0 = 0x0F0F00F1 | sum(1 << s for s in SLOTS if s < 32)
        assert (live[0] & 0xFFFFFFFF) == want0 and live[1] == (0x1 | (1 << 4)) and lpad in (48, 128)
    if case.name.startswith("index_exact_bound"):
        live = [s for s in range(CAP) if (inp["live"].view(torch.int32)[s >> 5].item() >> (s & 31)) & 1]
        assert 4 not in live and 36 in live
        for j, m in enumerate("ab"[:len(host["ec"][0])]):
            assert float(host["ec"][0][j]) == float(inp["err_" + m][live].max()) < 5.0
