"""Guard-band cases of include/xmlhip_ingest_pool.h (xml_ingest_pool_rows) through tests/abi_arena.py, in the manner of
tests/test_gpu_index_view_arena.py: the status, untouched guard bytes around every operand of exactly its documented extent,
untouched inputs, independence of the arena's fill -- a range that names rows outside its source must read nothing, and the
sources end where the guard bytes begin -- and bitwise the values of the ops.* wrapper.  Sources and the destination sit 16
bytes (the 16-byte path) or 4 bytes (the element-wise path) past an aligned address, the int64 tables 8 bytes.  One and two
sources, NULL mask and NULL filled."""
import pytest
import torch

import ingest_pool_ref as REF
from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F16, F32, XDT, _ops, _st

pytestmark = pytest.mark.gpu

CASES = []
POOL = {"max": 0, "mean": 1}


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _case(d_a, d_b, src_dt, dst_dt, skew, pool, norms, normalize, null=()):
    n_src = 2 if d_b else 1
    mods = "ab"[:n_src]

    def inputs():
        c = REF.small_case(d_a, d_b, src_dt, seed=3)
        d = {"row_start": torch.from_numpy(c["row_start"])}
        for k, m in enumerate(mods):
            d["src_" + m] = torch.from_numpy(c["srcs"][k])
            # the bad ranges of test_bad_ranges_read_nothing: past the end, before 0, inverted, far outside
            d["seg_" + m] = torch.from_numpy(REF.bad_ranges(c["segs"][k], len(c["srcs"][k])) if k == 0 else c["segs"][k])
        d.update(n=c["n"], lmax=c["lmax"], max_len=c["max_len"])
        return d

    def raw(lib, A, inp):
        n, lmax = inp["n"], inp["lmax"]
        rs = A.put("row_start", inp["row_start"], skew=8)
        src = {m: A.put("src_" + m, inp["src_" + m], skew=skew) for m in mods}
        seg = {m: A.put("seg_" + m, inp["seg_" + m], skew=8) for m in mods}
        outs = {"dst": A.take("dst", (n, lmax, d_a + d_b), dst_dt, skew=skew)}
        for name in ("mask", "filled"):
            if name not in null:
                outs[name] = A.take(name, (n, lmax), F32, skew=4)
        b = "b" if n_src == 2 else None
        st = lib.xml_ingest_pool_rows(
            n_src, P(src["a"]), XDT[src_dt], src["a"].shape[0], d_a, P(seg["a"]), int(norms[0]),
            P(src[b]) if b else None, XDT[src_dt] if b else 0, src[b].shape[0] if b else 0, d_b, P(seg[b]) if b else None,
            int(norms[1]) if b else 0, P(rs), P(outs["dst"]), XDT[dst_dt], P(outs.get("mask")), P(outs.get("filled")), n, lmax,
            inp["max_len"], 1e-5, int(normalize), POOL[pool], _st())
        return st, outs

    def wrap(inp):
        sources = [(inp["src_" + m], inp["seg_" + m], norms[k]) for k, m in enumerate(mods)]
        dst, mask, filled = _ops().ingest_pool_rows(sources, inp["row_start"], inp["n"], inp["lmax"], inp["max_len"], pool=pool,
                                                    normalize=normalize, out_dtype=dst_dt, want_filled=True)
        out = {"dst": dst, "mask": mask, "filled": filled}
        return {k: v for k, v in out.items() if k not in null}

    CASES.append(Case("ingest_pool_rows_%dx%d_%s_%s_skew%d_%s%s" % (d_a, d_b, DTN[src_dt], DTN[dst_dt], skew, pool,
                                                                     "".join("_no" + x for x in null)),
                      ["xml_ingest_pool_rows"], inputs, raw, wrap, nbytes=1 << 23,
                      note="a video of no clips, one cut at max_len, lmax > max_len; ranges from source row 0 and to the last "
                           "source row, and bad ranges whose rows would lie in the guard bytes"))


_case(2048, 1024, F16, F32, 16, "max", (True, True), True)
_case(24, 40, F32, BF16, 4, "mean", (True, False), True, null=("mask",))
_case(768, 0, F16, BF16, 16, "mean", (False,), True, null=("filled",))
_case(7, 5, F16, F32, 4, "max", (False, False), False, null=("mask", "filled"))


def test_the_pool_entry_has_a_case():
    from test_ingest_pool_capi import header_symbols
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_ingest_pool_rows(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    v0, v1, _, _ = host["dst"]
    rs = inp["row_start"]
    for r in REF.BAD_ROWS:                                  # clip rows 0 .. 6 are video 0's: zero blocks of source a, both fills
        if r < int(rs[1]):
            d_a = inp["src_a"].shape[1]
            assert bool((v0[0, r, :d_a] == 0).all()) and bool((v1[0, r, :d_a] == 0).all()), r
    assert bool((v0[1] == 0).all()) and bool((v1[1] == 0).all())          # the video of no clips
