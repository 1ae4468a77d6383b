"""Guard-band cases of include/xmlhip_index_view.h (xml_index_gather_blocks) through tests/abi_arena.py, in the manner of
tests/test_gpu_index_compact_arena.py: the status, untouched guard bytes around every operand of exactly its documented
extent, untouched inputs, independence of the arena's fill -- the rows of unused destination blocks keep the fill, every mask
word is written -- and bitwise the values of the ops.* wrapper.  Pointers sit 16 bytes (images) and 4 bytes (tables) past an
aligned address.  One case per dtype, one with a single modality."""
import numpy as np
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F32, G, I32, XDT, _ops, _st
from test_gpu_index_view_kernel import N_SRC, SRC_TILES, src_blocks

pytestmark = pytest.mark.gpu

DST_TILES = 3
CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _case(dt, hidden, n_mod, null_bits_a):
    es = torch.empty(0, dtype=dt).element_size()
    slices = hidden * es // 64
    per = 1024 // es                                       # elements of one block's KiB
    mods = "ab"[:n_mod]

    def inputs():
        g = G(191 + hidden + n_mod)
        d = {"src_block": torch.from_numpy(src_blocks(DST_TILES, 23))}
        for m in mods:
            u = torch.randint(0, 256, (SRC_TILES, slices, 16, 1024), generator=g, dtype=torch.uint8)
            d["k6_src_" + m] = u.view(-1).view(dt).view(SRC_TILES, slices, 16, per)
            d["bits_src_" + m] = torch.randint(-2 ** 31, 2 ** 31, (N_SRC // 2,), generator=g, dtype=torch.int64).to(I32)
        return d

    def written(inp):
        sb = inp["src_block"].numpy()
        ok = ((sb >= 0) & (sb < N_SRC)).reshape(DST_TILES, 1, 16, 1)
        return torch.from_numpy(np.broadcast_to(ok, (DST_TILES, slices, 16, per)).copy())

    def raw(lib, A, inp):
        sb = A.put("src_block", inp["src_block"], skew=4)
        src = {m: A.put("k6_src_" + m, inp["k6_src_" + m], skew=16) for m in mods}
        bsrc = {m: A.put("bits_src_" + m, inp["bits_src_" + m], skew=4) for m in mods}
        if null_bits_a:
            bsrc["a"] = None
        outs = {}
        for m in mods:
            outs["k6_dst_" + m] = A.take("k6_dst_" + m, (DST_TILES, slices, 16, per), dt, skew=16, partly_written=written(inp))
            outs["bits_dst_" + m] = A.take("bits_dst_" + m, (2 * DST_TILES, 4), I32, skew=4)
        b = "b" if n_mod == 2 else None
        st = lib.xml_index_gather_blocks(n_mod, P(sb), DST_TILES, P(src["a"]), P(bsrc["a"]), P(src[b]) if b else None,
                                         P(bsrc[b]) if b else None, N_SRC, P(outs["k6_dst_a"]), P(outs["bits_dst_a"]),
                                         P(outs["k6_dst_b"]) if b else None, P(outs["bits_dst_b"]) if b else None, hidden,
                                         XDT[dt], _st())
        return st, outs

    def wrap(inp):
        o = _ops()
        dst = [torch.zeros(DST_TILES * slices * 16 * per, dtype=dt, device=DEV) for _ in mods]
        bits = [torch.zeros((2 * DST_TILES, 4), dtype=I32, device=DEV) for _ in mods]
        bsrc = [None if (null_bits_a and m == "a") else inp["bits_src_" + m] for m in mods]
        o.index_gather_blocks(inp["src_block"], [inp["k6_src_" + m].reshape(-1) for m in mods], bsrc, N_SRC, dst, bits, hidden)
        out = {}
        for i, m in enumerate(mods):
            out["k6_dst_" + m] = dst[i].view(DST_TILES, slices, 16, per)
            out["bits_dst_" + m] = bits[i]
        return out

    CASES.append(Case("index_gather_blocks_%s_h%d_%dmod%s" % (DTN[dt], hidden, n_mod, "_nullbits" if null_bits_a else ""),
                      ["xml_index_gather_blocks"], inputs, raw, wrap, nbytes=1 << 24,
                      note="20 source tiles into 3; runs that straddle in the source only and in the destination only, the "
                           "last source block into the last destination block, out-of-range entries handled as unused"))


_case(F32, 128, 2, False)
_case(BF16, 256, 2, True)
_case(F32, 192, 1, False)


def test_the_view_entry_has_a_case():
    from test_index_view_capi import header_symbols
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_gather_blocks(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    sb = inp["src_block"].numpy()
    ok = (sb >= 0) & (sb < N_SRC)
    for name, (v0, v1, mask, _) in host.items():
        if not name.startswith("k6_dst_"):
            continue
        src = inp["k6_src_" + name[-1]]
        for g in np.nonzero(ok)[0]:                        # block-for-block copies, under both fills
            s = int(sb[g])
            for v in (v0, v1):
                assert torch.equal(v[g // 16, :, g % 16].contiguous().view(torch.uint8),
                                   src[s // 16, :, s % 16].contiguous().view(torch.uint8)), (name, g)
