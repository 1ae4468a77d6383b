"""CPU checks of the guard-band harness (tests/abi_arena.py) with fake cases, of the registry of real cases
(tests/test_gpu_abi_arena.py: every header symbol has a case or a stated exemption), and of the argument refusals."""
import re

import pytest
import torch

import abi_arena
from abi_arena import Arena, ArenaError, Case, run_case
from test_capi import header_symbols, lib  # noqa: F401  (lib: module fixture that builds / loads libxmlhip.so)


def _fake(name, body, partly=None, ld=None, wrapper=True):
    """A fake entry on the CPU: out (5, 7) f32 = 2 x, computed by `body(arena, x, out)` in place of a kernel."""
    def inputs():
        return {"x": torch.arange(35, dtype=torch.float32).view(5, 7) - 3.0}

    def raw(lib, arena, inp):
        x = arena.put("x", inp["x"])
        out = arena.take("out", (5, 7), torch.float32, ld=ld, partly_written=partly)
        body(arena, x, out)
        return 0, {"out": out}

    return Case(name, ["fake"], inputs, raw, (lambda inp: {"out": inp["x"] * 2}) if wrapper else None, nbytes=1 << 16)


def _honest(arena, x, out):
    out.copy_(x * 2)


def test_honest_case_passes():
    run_case(_fake("honest", _honest), None, "cpu")
    run_case(_fake("honest_strided", _honest, ld=10), None, "cpu")


def test_store_into_a_gap_is_caught_and_names_the_region():
    def body(arena, x, out):
        _honest(arena, x, out)
        arena.buf[arena.region("out").end] = 0x5A                    # one byte behind the output
    with pytest.raises(ArenaError, match=r"1 bytes after the end of region 'out'"):
        run_case(_fake("overrun", body), None, "cpu")

    def before(arena, x, out):
        _honest(arena, x, out)
        arena.buf[arena.region("out").off - 3] = 0x5A
    with pytest.raises(ArenaError, match=r"3 bytes before the start of region 'out'"):
        run_case(_fake("underrun", before), None, "cpu")


def test_store_of_zeros_shows_under_the_other_fill():
    def body(arena, x, out):
        _honest(arena, x, out)
        arena.buf[arena.region("out").end + 8] = 0x00
    with pytest.raises(ArenaError, match=r"fill 0xFF.*9 bytes after the end of region 'out'"):
        run_case(_fake("zero_store", body), None, "cpu")


def test_store_between_strided_rows_is_caught():
    def body(arena, x, out):
        _honest(arena, x, out)
        r = arena.region("out")
        arena.buf[r.off + 2 * r.ld_bytes + r.row_bytes] = 0x11       # first byte behind row 2 (ld = 10 > 7)
    with pytest.raises(ArenaError, match=r"inside region 'out', in the gap behind row 2 \(1 bytes past"):
        run_case(_fake("row_gap", body, ld=10), None, "cpu")


def test_unwritten_output_element_is_caught():
    def body(arena, x, out):
        _honest(arena, x, out)
        out.view(-1).view(torch.uint8)[-4:] = arena.fill             # element [4, 6] keeps the bytes it started with
    with pytest.raises(ArenaError, match=r"output 'out' \(region 'out'\).*index \[4, 6\].*never written"):
        run_case(_fake("unwritten", body), None, "cpu")


def test_fill_dependent_element_is_caught():
    def body(arena, x, out):
        _honest(arena, x, out)
        out[1, 2] = float(arena.fill)                                # a value made from outside bytes
    with pytest.raises(ArenaError, match=r"region 'out'.*index \[1, 2\].*depends on the fill"):
        run_case(_fake("fill_dependent", body), None, "cpu")


def test_store_into_declared_unwritten_element_is_caught():
    partly = torch.ones(5, 7, dtype=torch.bool)
    partly[3, 5:] = False

    def ok(arena, x, out):
        out[partly] = (x * 2)[partly]
    run_case(_fake("partly", ok, partly=partly), None, "cpu")

    def body(arena, x, out):
        ok(arena, x, out)
        out[3, 6] = 7.0
    with pytest.raises(ArenaError, match=r"region 'out'.*declares unwritten were written.*index \[3, 6\]"):
        run_case(_fake("partly_store", body, partly=partly), None, "cpu")


def test_changed_input_and_wrong_value_and_status_are_caught():
    def body(arena, x, out):
        _honest(arena, x, out)
        x[0, 0] = 9.0
    with pytest.raises(ArenaError, match=r"changed its input operand, region 'x'"):
        run_case(_fake("input_changed", body), None, "cpu")

    def wrong(arena, x, out):
        out.copy_(x * 2)
        out[2, 2] += 1.0
    with pytest.raises(ArenaError, match=r"region 'out'.*differ bitwise from the wrapper's.*\[2, 2\]"):
        run_case(_fake("wrong_value", wrong), None, "cpu")

    c = _fake("status", _honest)
    raw = c.raw
    c.raw = lambda lib, arena, inp: (-3, raw(lib, arena, inp)[1])
    with pytest.raises(ArenaError, match="returned status -3"):
        run_case(c, None, "cpu")


def test_documented_refusal_must_write_nothing():
    def body(arena, x, out):
        pass
    c = _fake("refusal", body, wrapper=False)
    raw = c.raw
    c.raw = lambda lib, arena, inp: (-2, raw(lib, arena, inp)[1])
    c.expect_status = -2
    run_case(c, None, "cpu")
    c2 = _fake("refusal_wrote", lambda arena, x, out: out[0, 0].fill_(1.0), wrapper=False)
    raw2 = c2.raw
    c2.raw = lambda lib, arena, inp: (-2, raw2(lib, arena, inp)[1])
    c2.expect_status = -2
    with pytest.raises(ArenaError, match="refused the call but wrote to output 'out'"):
        run_case(c2, None, "cpu")
    with pytest.raises(ArenaError, match="returned status 0"):
        c3 = _fake("not_refused", _honest)
        c3.expect_status = -2
        run_case(c3, None, "cpu")


def test_layout_margins_alignment_and_exact_extent():
    a = Arena(1 << 16, 0xFF, "cpu")
    v = a.take("m", (6, 300), torch.float32, ld=303, skew=4)
    r = a.region("m")
    assert r.off >= abi_arena.MARGIN + 4096 and (v.data_ptr() - 4) % 256 == 0 and v.data_ptr() % 256 == 4
    assert r.end - r.off == (5 * 303 + 300) * 4 and v.stride() == (303, 1)
    w = a.take("w", (3, 2, 8), torch.bfloat16, ld=16)
    assert w.data_ptr() % 256 == 0 and w.stride() == (32, 16, 1) and w.data_ptr() - a.base >= r.end + 4096
    ws, n = a.workspace(100)
    assert n == 100 and a.region("ws").end - a.region("ws").off == 100
    assert a.size - a.region("ws").end >= abi_arena.MARGIN + 4096
    assert int(a.owned.sum()) == 6 * 300 * 4 + 3 * 2 * 8 * 2 + 100
    assert bool(torch.isnan(v).all()) and bool((a.take("i", (4,), torch.int32) == -1).all())
    a.check_guards()
    with pytest.raises(ArenaError, match="arena too small"):
        a.take("big", (1 << 20,), torch.uint8)


# ---- the registry of real cases ----
def test_every_header_symbol_has_a_case_or_a_stated_exemption():
    import test_gpu_abi_arena as G
    syms = set(header_symbols())
    covered = set(G.CASES)
    assert covered <= syms, "cases for symbols the header does not declare: %s" % sorted(covered - syms)
    assert set(G.EXEMPT) <= syms, "exemptions for symbols the header does not declare: %s" % sorted(set(G.EXEMPT) - syms)
    both = covered & set(G.EXEMPT)
    assert not both, "symbols that are both covered and exempt: %s" % sorted(both)
    missing = syms - covered - set(G.EXEMPT)
    assert not missing, "header symbols with neither a guard-band case nor a stated exemption: %s" % sorted(missing)
    for s, why in G.EXEMPT.items():
        assert isinstance(why, str) and len(why) > 8 and "\n" not in why, s
    for s, cases in G.CASES.items():
        assert cases and all(s in c.symbols for c in cases)


def test_completeness_bites_when_a_case_is_deleted(monkeypatch):
    import test_gpu_abi_arena as G
    cases = dict(G.CASES)
    del cases["xml_topk_rows"]
    monkeypatch.setattr(G, "CASES", cases)
    with pytest.raises(AssertionError, match="xml_topk_rows"):
        test_every_header_symbol_has_a_case_or_a_stated_exemption()


def test_case_names_are_unique_and_carry_a_note():
    import test_gpu_abi_arena as G
    names = [c.name for c in G.ALL_CASES]
    assert len(names) == len(set(names))
    for c in G.ALL_CASES:
        assert c.note and re.match(r"^[a-z0-9_\-]+$", c.name), c.name


def test_packed_pooling_refuses_rows_that_are_no_multiple_of_8(lib):  # noqa: F811
    """xml_modular_pool_varlen / _att_varlen have no scalar path (tests/test_gpu_abi_arena.py runs the refusal in an arena)."""
    import ctypes
    p = ctypes.c_void_p(0x1000)
    assert lib.xml_modular_pool_varlen(p, p, p, p, 7, 32, 100, 2, 0, None) == -2
    assert lib.xml_modular_pool_att_varlen(p, p, p, p, p, 7, 32, 100, 2, 1, None) == -2
    assert lib.xml_modular_pool_varlen(p, p, p, p, 7, 33, 128, 2, 0, None) == -2          # max_len > 32
