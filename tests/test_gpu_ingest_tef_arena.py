"""Guard-band cases of include/xmlhip_ingest_tef.h (xml_ingest_rows_tef, xml_ingest_pool_rows_tef) through tests/abi_arena.py, in
the manner of tests/test_gpu_ingest_pool_arena.py: the status, untouched guard bytes around every operand of exactly its
documented extent, untouched inputs, independence of the arena's fill, and bitwise the values of the ops.* wrapper.  The
destination's row pitch (D + 2) * size is never a multiple of 16, and its base sits only 8 bytes (f32) or 4 bytes (bf16) past
an aligned address: the widest store the header promises ends exactly at the row's end.  The sweep shapes, the smallest
launch n = 1, lmax = 1, and the d = 4096 extent."""
import pytest
import torch

import ingest_tef_ref as REF
from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F16, F32, XDT, _ops, _st

pytestmark = pytest.mark.gpu

CASES = []
POOL = {"max": 0, "mean": 1}
SKEW = {F32: 8, BF16: 4}          # the destination's base: natural alignment of the widest promised store, nothing more


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _place(c, place):
    """tef_pos / tef_len of a case: item i sits at clip 3 i of a video 5 clips longer than its end; item 1's video is too short."""
    if not place:
        return {}
    lens = [min(int(n), c["max_len"]) for n in c["lens"]]
    pos = [3 * i for i in range(len(lens))]
    tot = [p + n + 5 for p, n in zip(pos, lens)]
    if len(tot) > 1:
        tot[1] = pos[1] + lens[1] - 1
    return dict(tef_pos=torch.tensor(pos, dtype=torch.int32), tef_len=torch.tensor(tot, dtype=torch.int32))


def _rows_case(d, src_dt, dst_dt, src_skew, normalize, lens=REF.LENS, place=False, nbytes=1 << 22):
    def inputs():
        c = REF.rows_case(d, src_dt, seed=1, lens=lens)
        out = dict(src=c["src"], row_start=c["row_start"], n=c["n"], lmax=c["lmax"], max_len=c["max_len"])
        out.update(_place(c, place))
        return out

    def raw(lib, A, inp):
        n, lmax = inp["n"], inp["lmax"]
        rs = A.put("row_start", inp["row_start"], skew=8)
        src = A.put("src", inp["src"], skew=src_skew)
        pos = A.put("tef_pos", inp["tef_pos"], skew=4) if place else None
        tot = A.put("tef_len", inp["tef_len"], skew=4) if place else None
        outs = {"dst": A.take("dst", (n, lmax, d + 2), dst_dt, skew=SKEW[dst_dt]), "mask": A.take("mask", (n, lmax), F32, skew=4)}
        st = lib.xml_ingest_rows_tef(P(src), XDT[src_dt], P(rs), P(pos), P(tot), P(outs["dst"]), XDT[dst_dt], P(outs["mask"]), n,
                                     lmax, d, inp["max_len"], 1e-5, int(normalize), _st())
        return st, outs

    def wrap(inp):
        dst, mask = _ops().ingest_rows(inp["src"], inp["row_start"], inp["n"], inp["lmax"], inp["max_len"],
                                       normalize=bool(normalize), out_dtype=dst_dt, tef=True, tef_pos=inp.get("tef_pos"),
                                       tef_len=inp.get("tef_len"))
        return {"dst": dst, "mask": mask}

    CASES.append(Case("ingest_rows_tef_d%d_%s_%s_srcskew%d_norm%d_n%d%s" % (d, DTN[src_dt], DTN[dst_dt], src_skew, normalize,
                                                                           len(lens), "_place" if place else ""),
                      ["xml_ingest_rows_tef"], inputs, raw, wrap, nbytes=nbytes,
                      note="dst base %d bytes past an aligned address, pitch %d bytes" % (SKEW[dst_dt], (d + 2) * (4 if dst_dt is F32 else 2))))


def _pool_case(d_a, d_b, src_dt, dst_dt, src_skew, pool, norms, normalize, lens=REF.LENS, place=False, null=(), nbytes=1 << 22):
    n_src = 2 if d_b else 1
    mods = "ab"[:n_src]

    def inputs():
        c = REF.pool_case(d_a, d_b, src_dt, seed=2, lens=lens)
        out = dict(row_start=c["row_start"], n=c["n"], lmax=c["lmax"], max_len=c["max_len"])
        for k, m in enumerate(mods):
            out["src_" + m], out["seg_" + m] = c["srcs"][k], c["segs"][k]
        out.update(_place(c, place))
        return out

    def raw(lib, A, inp):
        n, lmax = inp["n"], inp["lmax"]
        rs = A.put("row_start", inp["row_start"], skew=8)
        src = {m: A.put("src_" + m, inp["src_" + m], skew=src_skew) for m in mods}
        seg = {m: A.put("seg_" + m, inp["seg_" + m], skew=8) for m in mods}
        pos = A.put("tef_pos", inp["tef_pos"], skew=4) if place else None
        tot = A.put("tef_len", inp["tef_len"], skew=4) if place else None
        outs = {"dst": A.take("dst", (n, lmax, d_a + d_b + 2), dst_dt, skew=SKEW[dst_dt])}
        for name in ("mask", "filled"):
            if name not in null:
                outs[name] = A.take(name, (n, lmax), F32, skew=4)
        b = "b" if n_src == 2 else None
        st = lib.xml_ingest_pool_rows_tef(
            n_src, P(src["a"]), XDT[src_dt], src["a"].shape[0], d_a, P(seg["a"]), int(norms[0]),
            P(src[b]) if b else None, XDT[src_dt] if b else 0, src[b].shape[0] if b else 0, d_b, P(seg[b]) if b else None,
            int(norms[1]) if b else 0, P(rs), P(outs["dst"]), XDT[dst_dt], P(outs.get("mask")), P(outs.get("filled")), n, lmax,
            inp["max_len"], 1e-5, int(normalize), POOL[pool], P(pos), P(tot), _st())
        return st, outs

    def wrap(inp):
        sources = [(inp["src_" + m], inp["seg_" + m], norms[k]) for k, m in enumerate(mods)]
        dst, mask, filled = _ops().ingest_pool_rows(sources, inp["row_start"], inp["n"], inp["lmax"], inp["max_len"], pool=pool,
                                                    normalize=normalize, out_dtype=dst_dt, want_filled=True, tef=True,
                                                    tef_pos=inp.get("tef_pos"), tef_len=inp.get("tef_len"))
        out = {"dst": dst, "mask": mask, "filled": filled}
        return {k: v for k, v in out.items() if k not in null}

    CASES.append(Case("ingest_pool_rows_tef_%dx%d_%s_%s_srcskew%d_%s_n%d%s%s" % (
        d_a, d_b, DTN[src_dt], DTN[dst_dt], src_skew, pool, len(lens), "_place" if place else "", "".join("_no" + x for x in null)),
        ["xml_ingest_pool_rows_tef"], inputs, raw, wrap, nbytes=nbytes,
        note="dst base %d bytes past an aligned address; a clip with an empty range" % SKEW[dst_dt]))


# the vector kernel (rows of whole 16-byte pieces on a 16-byte base) and the element-wise one (any other row, any other base)
_rows_case(72, F16, F32, 16, 1, place=True)
_rows_case(72, F16, BF16, 16, 1)
_rows_case(512, F32, F32, 16, 0)
_rows_case(512, F32, BF16, 16, 1, place=True)
_rows_case(510, F16, F32, 16, 1)
_rows_case(64, F16, BF16, 2, 1, place=True)
_rows_case(6, F32, F32, 4, 0)
# the smallest launch; the widest row
_rows_case(64, F16, F32, 16, 1, lens=(1,))
_rows_case(6, F16, BF16, 2, 1, lens=(1,))
_rows_case(4096, F16, F32, 16, 1, lens=(1,))
_rows_case(4096, F32, BF16, 16, 1, lens=(2, 1), nbytes=1 << 23)
_rows_case(4096, F16, BF16, 2, 1, lens=(1,))

_pool_case(504, 8, F16, F32, 16, "max", (True, True), True, place=True)
_pool_case(504, 8, F16, BF16, 16, "mean", (True, False), True, null=("mask",))
_pool_case(16, 8, F32, F32, 16, "mean", (False, True), False, null=("filled",))
_pool_case(16, 8, F16, BF16, 16, "max", (True, True), True, place=True)
_pool_case(12, 6, F16, F32, 4, "max", (False, False), True, place=True, null=("mask", "filled"))
_pool_case(16, 8, F16, BF16, 2, "mean", (True, True), True)
_pool_case(16, 8, F16, F32, 16, "max", (True, True), True, lens=(1,))
_pool_case(7, 0, F16, BF16, 2, "max", (True,), True, lens=(1,))
_pool_case(2048, 2048, F16, F32, 16, "max", (True, True), True, lens=(1,))
_pool_case(4096, 0, F16, BF16, 16, "mean", (False,), True, lens=(2, 1), nbytes=1 << 23)


def test_both_entries_have_cases():
    from test_ingest_tef_capi import header_symbols
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_ingest_tef(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    v0, _, _, _ = host["dst"]
    n, lmax, max_len = inp["n"], inp["lmax"], inp["max_len"]
    lens = [min(int(x), max_len) for x in (inp["row_start"][1:] - inp["row_start"][:-1]).tolist()]
    want = REF.restate_tef(lens, lmax, max_len, inp.get("tef_pos"), inp.get("tef_len"))
    want = REF.to_bf16(want) if v0.dtype is BF16 else torch.from_numpy(want)
    D = v0.shape[2] - 2
    assert torch.equal(v0[:, :, D:].contiguous().view(torch.int16 if v0.dtype is BF16 else torch.int32),
                       want.view(torch.int16 if v0.dtype is BF16 else torch.int32))
    for i, ln in enumerate(lens):
        assert bool((v0[i, ln:].float() == 0).all())
