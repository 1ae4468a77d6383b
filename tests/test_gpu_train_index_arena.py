"""Guard-band cases of include/xmlhip_train_index.h (xml_index_gather_video_rows, xml_q2c_scores_arg_bwd_q,
xml_pair_sim_bwd_q) through tests/abi_arena.py, in the manner of tests/test_gpu_index_view_arena.py: the status, untouched
guard bytes around every operand of exactly its documented extent, untouched inputs, independence of the arena's fill -- every
output element is written, whatever slot / first_block / arg say -- and bitwise the values of the ops.* / train_ops.* wrappers.
Feature pointers sit 16 bytes, tables and masks 4 bytes past an aligned address."""
import ctypes

import numpy as np
import pytest
import torch

from abi_arena import Case, ptr as P, run_case
from test_gpu_abi_arena import BF16, DEV, DTN, F32, G, I32, XDT, _ops, _st
from test_gpu_train_index_gather import batch_of, make_source

pytestmark = pytest.mark.gpu

CASES = []


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


def _gather_case(form, dt, hidden, n_mod, n, length):
    mods = "ab"[:n_mod]
    es = torch.empty(0, dtype=dt).element_size()

    def inputs():
        src = make_source(form, dt, hidden, n_mod, 77 + hidden)
        slots, first = batch_of(form, src, n, 5)
        d = dict(slot=torch.from_numpy(slots.astype(np.int32)), first_block=torch.from_numpy(first.astype(np.int32)),
                 vlen=torch.from_numpy(src["vlen"]), n_blocks=src["n_blocks"], lpad=src["lpad"])
        for m, mod in zip(mods, src["mods"]):
            u = mod["cn_u8"]
            d["cn_src_" + m] = u.view(-1).view(dt).view(u.shape[:-1] + (u.shape[-1] // es,))
            d["f2_src_" + m] = mod["f2_u8"].view(-1).view(dt).view(len(src["vlen"]), src["lpad"], hidden)
            d["mask_src_" + m] = mod["mask"]
        return d

    def raw(lib, A, inp):
        t = {k: A.put(k, v, skew=16 if k[:2] in ("cn", "f2") else 4) for k, v in inp.items() if torch.is_tensor(v)}
        outs = {}
        for m in mods:
            outs["cn_" + m] = A.take("cn_" + m, (n, length, hidden), dt, skew=16)
            outs["f2_" + m] = A.take("f2_" + m, (n, length, hidden), dt, skew=16)
            outs["mask_" + m] = A.take("mask_" + m, (n, length), F32, skew=4)
        b = "b" if n_mod == 2 else None
        g = lambda k: P(t[k + "_" + b]) if b else None         # noqa: E731
        o = lambda k: P(outs[k + "_" + b]) if b else None      # noqa: E731
        st = lib.xml_index_gather_video_rows(
            n_mod, 0 if form == "rows" else 1, P(t["slot"]), None if form == "rows" else P(t["first_block"]), n, P(t["vlen"]),
            len(inp["vlen"]), inp["n_blocks"], inp["lpad"], P(t["cn_src_a"]), P(t["f2_src_a"]), P(t["mask_src_a"]), g("cn_src"),
            g("f2_src"), g("mask_src"), P(outs["cn_a"]), P(outs["f2_a"]), P(outs["mask_a"]), o("cn"), o("f2"), o("mask"), length,
            hidden, XDT[dt], _st())
        return st, outs

    def wrap(inp):
        o = _ops()
        nv = len(inp["vlen"])
        cn = [inp["cn_src_" + m] if form == "rows" else o.TiledRows(inp["cn_src_" + m].reshape(-1), nv * 128, hidden, (nv, 128, hidden))
              for m in mods]
        got = o.index_gather_video_rows(inp["slot"], None if form == "rows" else inp["first_block"], inp["vlen"], cn,
                                        [inp["f2_src_" + m] for m in mods], [inp["mask_src_" + m] for m in mods], length,
                                        n_blocks=inp["n_blocks"])
        out = {}
        for m, (c, f, k) in zip(mods, got):
            out["cn_" + m], out["f2_" + m], out["mask_" + m] = c, f, k
        return out

    CASES.append(Case("index_gather_video_rows_%s_%s_h%d_%dmod_n%d_l%d" % (form, DTN[dt], hidden, n_mod, n, length),
                      ["xml_index_gather_video_rows"], inputs, raw, wrap, nbytes=1 << 25,
                      note="slots -1 / n_videos / 2^31 - 1, first blocks -1, n_blocks and -2^31; the last thread block is partial"))


def _scores_case(dt, hidden, n_mod, nq, nv, ls, skew_ld):
    mods = list(range(n_mod))

    def inputs():
        g = G(500 + hidden + n_mod)
        d = dict(dscores=torch.randn(nq, nv, generator=g) * (torch.rand(nq, nv, generator=g) < 0.5))
        for m in mods:
            l = ls[m]
            d["query_%d" % m] = torch.randn(nq, hidden, generator=g).to(dt)
            d["qn_%d" % m] = torch.nn.functional.normalize(d["query_%d" % m].float(), dim=-1).to(dt)
            d["cn_%d" % m] = torch.nn.functional.normalize(torch.randn(nv, l, hidden, generator=g), dim=-1).to(dt)
            d["mask_%d" % m] = (torch.rand(nv, l, generator=g) < 0.8).float()
            arg = torch.randint(0, l, (nq, nv), generator=g).to(I32)
            arg[0, 0], arg[nq - 1, nv - 1], arg[1, 0] = l - 1, l - 1, 0
            d["arg_%d" % m] = arg
        d["query_0"][1] = 0                                    # a zero query row: the clamped-norm branch
        return d

    def raw(lib, A, inp):
        ld_ds, ld_arg = nv + skew_ld, nv + 2 * skew_ld
        ds = A.put("dscores", inp["dscores"], ld=ld_ds, skew=4)
        t = {}
        for m in mods:
            for k in ("query", "qn", "cn"):
                t[k, m] = A.put("%s_%d" % (k, m), inp["%s_%d" % (k, m)], skew=16)
            t["mask", m] = A.put("mask_%d" % m, inp["mask_%d" % m], skew=4)
            t["arg", m] = A.put("arg_%d" % m, inp["arg_%d" % m], ld=ld_arg, skew=4)
        outs = {"dq_%d" % m: A.take("dq_%d" % m, (nq, hidden), dt, skew=16) for m in mods}
        vp = lambda k: (ctypes.c_void_p * n_mod)(*[t[k, m].data_ptr() for m in mods])      # noqa: E731
        st = lib.xml_q2c_scores_arg_bwd_q(n_mod, vp("query"), vp("qn"), vp("cn"), vp("mask"), P(ds), ld_ds, 0.5,
                                          (ctypes.c_void_p * n_mod)(*[outs["dq_%d" % m].data_ptr() for m in mods]), nq, nv,
                                          (ctypes.c_int * n_mod)(*ls[:n_mod]), hidden, vp("arg"), ld_arg, XDT[dt], _st())
        return st, outs

    def wrap(inp):
        from tvretrieval_amd import train_ops
        sets = [tuple(inp["%s_%d" % (k, m)] for k in ("query", "qn", "cn", "mask", "arg")) for m in mods]
        return {"dq_%d" % m: v for m, v in enumerate(train_ops.q2c_scores_arg_bwd_q(sets, inp["dscores"], scale=0.5))}

    CASES.append(Case("q2c_scores_arg_bwd_q_%s_h%d_%dmod_%dx%d" % (DTN[dt], hidden, n_mod, nq, nv), ["xml_q2c_scores_arg_bwd_q"],
                      inputs, raw, wrap, nbytes=1 << 23,
                      note="row strides of dscores and arg beyond nv, arg = l - 1 at the last video, a zero query row"))


def _pair_case(dt, hidden, n, l):
    def inputs():
        g = G(600 + hidden)
        return dict(f2=torch.randn(n, l, hidden, generator=g).to(dt), dsim=torch.randn(n, l, generator=g))

    def raw(lib, A, inp):
        f2, dsim = A.put("f2", inp["f2"], skew=16), A.put("dsim", inp["dsim"], skew=4)
        outs = dict(dq=A.take("dq", (n, hidden), dt, skew=16))
        return lib.xml_pair_sim_bwd_q(P(f2), P(dsim), P(outs["dq"]), n, l, hidden, XDT[dt], _st()), outs

    def wrap(inp):
        from tvretrieval_amd import train_ops
        return dict(dq=train_ops.pair_sim_bwd_q(inp["f2"], inp["dsim"]))

    CASES.append(Case("pair_sim_bwd_q_%s_h%d_%dx%d" % (DTN[dt], hidden, n, l), ["xml_pair_sim_bwd_q"], inputs, raw, wrap,
                      nbytes=1 << 23, note="l no multiple of the 16 clips a workgroup has in flight; hidden beyond one 64-lane pass"))


_gather_case("packed", BF16, 128, 2, 130, 128)
_gather_case("fixed", F32, 64, 1, 130, 100)
_gather_case("plan", BF16, 128, 1, 3, 17)
_gather_case("rows", F32, 64, 2, 130, 17)
_scores_case(BF16, 128, 2, 7, 9, (19, 19), 3)
_scores_case(F32, 64, 1, 5, 4, (32,), 0)
_pair_case(BF16, 128, 6, 23)
_pair_case(F32, 520, 3, 17)


def test_every_entry_of_the_header_has_a_case():
    from test_train_index_capi import N_ARGS
    assert {s for c in CASES for s in c.symbols} == set(N_ARGS)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_abi_arena_train_index(lib, case):
    try:
        run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise
