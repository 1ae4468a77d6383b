"""Guard-band cases of include/xmlhip_train_pool.h (xml_gather_pool_feature_rows) through tests/abi_arena.py, in the manner of
tests/test_gpu_ingest_pool_arena.py: the status, untouched guard bytes around every operand of exactly its documented extent,
untouched inputs, independence of the arena's fill -- a range that names rows outside its source, and an example or item id out
of range, must read nothing -- and bitwise the values of the ops.* wrapper.  Sources and the destination sit 16 bytes (the
16-byte path) or 4 bytes (the element-wise path) past an aligned address, the int64 tables 8 bytes, the int32 tables 4.  One and
two sources, with and without the endpoint columns, NULL mask and NULL len_out."""
import pytest
import torch

import ingest_pool_ref as REF
from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F16, F32, XDT, _ops, _st

pytestmark = pytest.mark.gpu

CASES = []
POOL = {"max": 0, "mean": 1}
ITEM_OF = [2, 0, 3, 1, 2, 0, 3]
IDS = [4, 1, 6, -1, 3, 0, 7, 2]           # a repeat, the empty item, one id on each side out of range


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def header_symbols():
    from test_train_pool_capi import N_ARGS
    return sorted(N_ARGS)


def _case(d_a, d_b, src_dt, dst_dt, skew, pool, norms, normalize, tef, null=()):
    n_src = 2 if d_b else 1
    mods = "ab"[:n_src]

    def inputs():
        c = REF.small_case(d_a, d_b, src_dt, seed=3)
        d = {"clip_start": torch.from_numpy(c["row_start"]), "ids": torch.tensor(IDS, dtype=torch.int32),
             "item_of": torch.tensor(ITEM_OF, dtype=torch.int32)}
        for k, m in enumerate(mods):
            d["src_" + m] = torch.from_numpy(c["srcs"][k])
            d["seg_" + m] = torch.from_numpy(REF.bad_ranges(c["segs"][k], len(c["srcs"][k])) if k == 0 else c["segs"][k])
        d.update(n_items=c["n"], lmax=c["lmax"], max_len=c["max_len"])
        return d

    def raw(lib, A, inp):
        n, lmax = len(IDS), inp["lmax"]
        cs = A.put("clip_start", inp["clip_start"], skew=8)
        ids = A.put("ids", inp["ids"], skew=4)
        item_of = A.put("item_of", inp["item_of"], skew=4)
        src = {m: A.put("src_" + m, inp["src_" + m], skew=skew) for m in mods}
        seg = {m: A.put("seg_" + m, inp["seg_" + m], skew=8) for m in mods}
        outs = {"dst": A.take("dst", (n, lmax, d_a + d_b + 2 * tef), dst_dt, skew=skew)}
        if "mask" not in null:
            outs["mask"] = A.take("mask", (n, lmax), F32, skew=4)
        if "len_out" not in null:
            outs["len_out"] = A.take("len_out", (n,), torch.int32, skew=4)
        b = "b" if n_src == 2 else None
        st = lib.xml_gather_pool_feature_rows(
            n_src, P(src["a"]), XDT[src_dt], src["a"].shape[0], d_a, P(seg["a"]), int(norms[0]),
            P(src[b]) if b else None, XDT[src_dt] if b else 0, src[b].shape[0] if b else 0, d_b, P(seg[b]) if b else None,
            int(norms[1]) if b else 0, P(cs), inp["n_items"], P(ids), n, P(item_of), len(ITEM_OF), P(outs["dst"]), XDT[dst_dt],
            P(outs.get("mask")), P(outs.get("len_out")), lmax, inp["max_len"], 1e-5, int(normalize), POOL[pool], int(tef), _st())
        return st, outs

    def wrap(inp):
        sources = [(inp["src_" + m], inp["seg_" + m], norms[k]) for k, m in enumerate(mods)]
        dst, mask, ln = _ops().gather_pool_feature_rows(sources, inp["clip_start"], inp["ids"], inp["lmax"], inp["max_len"],
                                                        item_of=inp["item_of"], pool=pool, normalize=normalize, tef=bool(tef),
                                                        out_dtype=dst_dt)
        out = {"dst": dst, "mask": mask, "len_out": ln}
        return {k: v for k, v in out.items() if k not in null}

    CASES.append(Case("gather_pool_feature_rows_%dx%d_%s_%s_skew%d_%s_tef%d%s" % (d_a, d_b, DTN[src_dt], DTN[dst_dt], skew, pool, tef,
                                                                                 "".join("_no" + x for x in null)),
                      ["xml_gather_pool_feature_rows"], inputs, raw, wrap, nbytes=1 << 23,
                      note="an item of no clips, one cut at max_len, lmax > max_len, a repeated item, ids below 0 and past the "
                           "examples; ranges from source row 0 and to the last source row, and bad ranges whose rows would lie in "
                           "the guard bytes"))


_case(2048, 1024, F16, F32, 16, "max", (True, True), True, 0)
_case(24, 40, F32, BF16, 4, "mean", (True, False), True, 1, null=("mask",))
_case(768, 0, F16, BF16, 16, "mean", (False,), True, 1, null=("len_out",))
_case(7, 5, F16, F32, 4, "max", (False, False), False, 0, null=("mask", "len_out"))


def test_the_gather_entry_has_a_case():
    assert {s for c in CASES for s in c.symbols} == set(header_symbols())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_gather_pool_feature_rows(lib, case):
    try:
        host = run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
    inp = case.inputs()
    v0, v1, _, _ = host["dst"]
    d_a = inp["src_a"].shape[1]
    # batch position 1 is item 0 (clip rows 0 .. 6), positions 0 and 5 are item 2 (clip rows 7 ..): zero blocks of source a where
    # its range is bad, under both fills
    for pos, first in ((1, 0), (0, 7), (5, 7)):
        for r in REF.BAD_ROWS:
            if first <= r < first + 7:
                assert bool((v0[pos, r - first, :d_a] == 0).all()) and bool((v1[pos, r - first, :d_a] == 0).all()), (pos, r)
    for pos in (3, 4, 6):                                   # an id below 0, the item of no clips, an id past the examples
        assert bool((v0[pos] == 0).all()) and bool((v1[pos] == 0).all()), pos
