"""Guard-band cases of the C ABI (include/xmlhip.h) on the GPU, through tests/abi_arena.py.

Every case places ALL operands, outputs and the workspace of one entry in an arena of known bytes, calls the C entry through
ctypes with raw pointers and a workspace of exactly *_workspace_bytes() bytes, and the runner asserts status, untouched
guard bytes, independence of the fill, and bitwise the values of the ops.* / train_ops.* wrapper the rest of the suite
checks against float64.  CASES (symbol -> cases) and EXEMPT (symbol -> reason) are read by tests/test_abi_arena.py: a new
entry point cannot join the header without a case or a stated reason.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from abi_arena import Case, ptr as P, run_case

DEV = "cuda:0"
F32, BF16, F16, I32, I64 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64
XML_F32, XML_BF16, XML_F16, XML_F16S = 0, 1, 2, 3
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
XDT = {F32: XML_F32, BF16: XML_BF16, F16: XML_F16}

CASES = {}          # header symbol -> [Case, ...]
ALL_CASES = []


def add(name, symbols, note, inputs, raw, wrapper, **kw):
    c = Case(name, symbols, inputs, raw, wrapper, note=note, **kw)
    ALL_CASES.append(c)
    for s in c.symbols:
        CASES.setdefault(s, []).append(c)
    return c


def _ops():
    from tvretrieval_amd import ops
    return ops


def _tops():
    from tvretrieval_amd import train_ops
    return train_ops


def _st():
    return _ops()._stream()


def G(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def unit(g, *shape, dtype=F32):
    return F.normalize(torch.randn(shape, generator=g), dim=-1).to(dtype)


def prefix_mask(lens, l):
    return (torch.arange(l)[None] < torch.as_tensor(lens)[:, None]).float()


def _cu(lens, dtype=I32):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=dtype)


def put_all(A, inp, names, **kw):
    return [A.put(n, inp[n], **kw) for n in names]


# =====================================================================================================================
# 6. rows in, rows out
# =====================================================================================================================
def _rowwise(name, symbol, note, make_x, call, wrap, out_dtype, out_shape=None):
    def inputs():
        return {"x": make_x()}

    def raw(lib, A, inp):
        x = A.put("x", inp["x"])
        y = A.take("y", out_shape or tuple(x.shape), out_dtype)
        return call(lib, x, y), {"y": y}

    add(name, [symbol], note, inputs, raw, lambda inp: {"y": wrap(inp["x"])})


for dt in (F32, BF16):
    for rows in (37, 300):      # 37: one partial block of rows; 300: more than one 256-row block, ragged end
        _rowwise("convert_f32_to_%s_r%d" % (DTN[dt], rows), "xml_convert", "n = rows * 100 elements: no multiple of 8 per thread",
                 lambda rows=rows: randn(G(1), rows, 100),
                 lambda lib, x, y, dt=dt: lib.xml_convert(P(x), XML_F32, P(y), XDT[dt], x.numel(), _st()),
                 lambda x, dt=dt: _ops().convert(x, dt), dt)
        _rowwise("l2norm_rows_%s_r%d" % (DTN[dt], rows), "xml_l2norm_rows", "rows not a multiple of the rows per block",
                 lambda rows=rows, dt=dt: randn(G(2), rows, 128, dtype=dt),
                 lambda lib, x, y, dt=dt: lib.xml_l2norm_rows(P(x), P(y), x.shape[0], 128, XDT[dt], _st()),
                 lambda x: _ops().l2norm_rows(x), dt)
    _rowwise("convert_%s_to_f32" % DTN[dt], "xml_convert", "n = 37 * 100 + 3 elements: scalar tail behind the vector body",
             lambda dt=dt: randn(G(3), 3703, dtype=dt),
             lambda lib, x, y, dt=dt: lib.xml_convert(P(x), XDT[dt], P(y), XML_F32, x.numel(), _st()),
             lambda x: _ops().convert(x, F32), F32)
    _rowwise("pack_weights_%s" % DTN[dt], "xml_pack_weights", "n = 128 * 66 + 5 elements: scalar tail behind the vector body",
             lambda: randn(G(4), 128 * 66 + 5),
             lambda lib, x, y, dt=dt: lib.xml_pack_weights(P(x), P(y), XDT[dt], x.numel(), _st()),
             lambda x, dt=dt: _ops().pack_weights(x, dt), dt)
for rows, d in ((37, 128), (300, 100)):      # d = 100: no multiple of the 4-wide vector rows
    _rowwise("l2norm_rows_eps_r%d_d%d" % (rows, d), "xml_l2norm_rows_eps", "ragged row block; d %% 8 = %d; one all-zero row" % (d % 8),
             lambda rows=rows, d=d: randn(G(5), rows, d) * (torch.arange(rows) != 3).float()[:, None],
             lambda lib, x, y: lib.xml_l2norm_rows_eps(P(x), P(y), x.shape[0], x.shape[1], 1e-5, _st()),
             lambda x: _ops().l2norm_rows_eps(x, 1e-5), F32)


def _add_layernorm(dt, rows, a_f32):
    def inputs():
        g = G(6)
        return {"a": randn(g, rows, 128, dtype=F32 if a_f32 else dt), "b": randn(g, rows, 128, dtype=dt),
                "g": randn(g, 128) + 1.0, "beta": randn(g, 128)}

    def raw(lib, A, inp):
        a, b, gg, beta = put_all(A, inp, ("a", "b", "g", "beta"))
        y = A.take("y", (rows, 128), dt)
        return lib.xml_add_layernorm(P(a), XDT[a.dtype], P(b), P(gg), P(beta), P(y), rows, 128, XDT[dt], _st()), {"y": y}

    add("add_layernorm_%s_r%d%s" % (DTN[dt], rows, "_af32" if a_f32 else ""), ["xml_add_layernorm"],
        "rows %% 4 waves per block = %d: ragged last block" % (rows % 4), inputs, raw,
        lambda inp: {"y": _ops().add_layernorm(inp["a"], inp["b"], inp["g"], inp["beta"], out_dtype=dt)})


for dt in (F32, BF16):
    _add_layernorm(dt, 37, False)
    _add_layernorm(dt, 300, dt is BF16)


def _round_bf16(rows):
    def inputs():
        return {"y": unit(G(7), rows, 128)}

    def raw(lib, A, inp):
        y = A.put("y", inp["y"])
        yb, err = A.take("yb", (rows, 128), BF16), A.take("err", (rows,), F32)
        return lib.xml_round_bf16_rows_err(P(y), P(yb), P(err), rows, 128, _st()), {"yb": yb, "err": err}

    def wrap(inp):
        yb, err = _ops().round_bf16_rows_err(inp["y"])
        return {"yb": yb, "err": err}

    add("round_bf16_rows_err_r%d" % rows, ["xml_round_bf16_rows_err"], "rows not a multiple of the rows per block; err is rows * 4 bytes",
        inputs, raw, wrap)


_round_bf16(37)
_round_bf16(300)


def _split_f16(rows, k, fixed):
    def inputs():
        g = G(8)
        return {"x": unit(g, rows, k) if fixed is not None else randn(g, rows, k, scale=3.0)}

    def raw(lib, A, inp):
        x = A.put("x", inp["x"])
        y, inv = A.take("y", (rows, k), I32), A.take("inv", (rows,), F32)
        hi, err = A.take("hi", (rows, k), F16), A.take("err", (rows,), F32)
        st = lib.xml_split_f16_rows(P(x), P(y), P(inv), P(hi), P(err), rows, k, -1 if fixed is None else fixed, _st())
        back = A.take("back", (rows, k), F32)
        st2 = lib.xml_unsplit_f16_rows(P(y), P(inv), P(back), rows, k, _st())
        return [st, st2], {"y": y, "inv": inv, "hi": hi, "err": err, "back": back}

    def wrap(inp):
        sr, hi, err = _ops().split_f16_rows(inp["x"], fixed_log2=fixed, want_hi=True, want_err=True)
        return {"y": sr.data, "inv": sr.inv, "hi": hi, "err": err, "back": _ops().unsplit_f16_rows(sr)}

    add("split_unsplit_f16_rows_r%d_k%d_%s" % (rows, k, "row_scale" if fixed is None else "fixed"),
        ["xml_split_f16_rows", "xml_unsplit_f16_rows"], "k = %d: %d groups of 32 per row; rows not a multiple of the block" % (k, k // 32),
        inputs, raw, wrap)


_split_f16(37, 32, None)
_split_f16(300, 96, 14)


def _pack_f16s_weight(w):
    """(n, k) f32 CPU -> the packed bytes (CPU uint8) of xml_pack_weights_f16s, made by the tested wrapper."""
    return _ops().pack_weights_f16s(w.to(DEV)).data.cpu()


def _pack_weights_f16s(n, k):
    def inputs():
        return {"w": randn(G(9), n, k, scale=0.1)}

    def raw(lib, A, inp):
        w = A.put("w", inp["w"])
        nb = lib.xml_pack_weights_f16s_bytes(n, k)
        assert nb == (n * k * 6 + 15) // 16 * 16 + 16
        dst = A.take("dst", (nb,), torch.uint8,          # the header defines the trailer's first float only
                     partly_written=torch.arange(nb) < nb - 12, may_be_written=torch.arange(nb) >= nb - 12)
        return lib.xml_pack_weights_f16s(P(w), P(dst), n, k, _st()), {"dst": dst}

    add("pack_weights_f16s_n%d_k%d" % (n, k), ["xml_pack_weights_f16s", "xml_pack_weights_f16s_bytes"],
        "n * k * 6 = %d bytes: the trailer sits %d bytes past a 256-byte line" % (n * k * 6, n * k * 6 % 256), inputs, raw,
        lambda inp: {"dst": _ops().pack_weights_f16s(inp["w"]).data})


_pack_weights_f16s(40, 72)


# ---- feature ingest -------------------------------------------------------------------------------------------------
def _ingest(src_dt, dst_dt, normalize):
    n, lmax, d, max_len = 5, 21, 100, 19
    lens = [0, 7, 30, 19, 1]                                  # an empty video, one longer than max_len, one of length 1

    def inputs():
        rs = _cu(lens, I64)
        return {"src": randn(G(10), int(rs[-1]), d, dtype=src_dt), "row_start": rs}

    def raw(lib, A, inp):
        src, rs = put_all(A, inp, ("src", "row_start"))
        dst, mask = A.take("dst", (n, lmax, d), dst_dt), A.take("mask", (n, lmax), F32)
        st = lib.xml_ingest_rows(P(src), XDT[src_dt], P(rs), P(dst), XDT[dst_dt], P(mask), n, lmax, d, max_len, 1e-5, normalize, _st())
        return st, {"dst": dst, "mask": mask}

    def wrap(inp):
        out, mask = _ops().ingest_rows(inp["src"], inp["row_start"], n, lmax, max_len, normalize=bool(normalize), out_dtype=dst_dt)
        return {"dst": out, "mask": mask}

    add("ingest_rows_%s_to_%s_norm%d" % (DTN[src_dt], DTN[dst_dt], normalize), ["xml_ingest_rows"],
        "d = 100, lmax = 21: rows of 400 / 200 bytes, no multiple of 16; padding rows behind every video", inputs, raw, wrap)


_ingest(F32, F32, 1)
_ingest(F16, BF16, 1)
_ingest(F16, F32, 0)


def _gather_feature_rows(src_dt, dst_dt, tef):
    n, lmax, d, max_len = 6, 13, 100, 11
    lens = [4, 0, 20, 11, 1]                                  # items: an empty one, one longer than max_len and lmax

    def inputs():
        rs = _cu(lens, I64)
        return {"src": randn(G(11), int(rs[-1]), d, dtype=src_dt), "row_start": rs,
                "ids": torch.tensor([3, 0, 7, 6, -1, 2], dtype=I32),                  # 7 and -1: ids out of range; 6 -> item 9: out of range
                "item_of": torch.tensor([0, 1, 2, 3, 4, 2, 9], dtype=I32)}

    def raw(lib, A, inp):
        src, rs, ids, item_of = put_all(A, inp, ("src", "row_start", "ids", "item_of"))
        dst, mask, ln = A.take("dst", (n, lmax, d + 2 * tef), dst_dt), A.take("mask", (n, lmax), F32), A.take("len", (n,), I32)
        st = lib.xml_gather_feature_rows(P(src), XDT[src_dt], P(rs), len(lens), P(ids), n, P(item_of), item_of.numel(), P(dst),
                                         XDT[dst_dt], P(mask), P(ln), lmax, d, max_len, 1e-5, 1, tef, _st())
        return st, {"dst": dst, "mask": mask, "len": ln}

    def wrap(inp):
        out, mask, ln = _ops().gather_feature_rows(inp["src"], inp["row_start"], inp["ids"], lmax, max_len, item_of=inp["item_of"],
                                                   tef=bool(tef), out_dtype=dst_dt)
        return {"dst": out, "mask": mask, "len": ln}

    add("gather_feature_rows_%s_to_%s_tef%d" % (DTN[src_dt], DTN[dst_dt], tef), ["xml_gather_feature_rows"],
        "d + 2 tef = %d columns: rows that are no multiple of 16 bytes; ids and an item out of range" % (d + 2 * tef), inputs, raw, wrap)


_gather_feature_rows(F32, F32, 1)
_gather_feature_rows(F16, BF16, 1)
_gather_feature_rows(F16, F32, 0)


def _gather_index_rows():
    def inputs():
        return {"src": torch.arange(37 * 2, dtype=I64).view(37, 2) * 1000003, "ids": torch.tensor([36, 0, 37, -1, 5], dtype=I32)}

    def raw(lib, A, inp):
        src, ids = put_all(A, inp, ("src", "ids"))
        dst = A.take("dst", (5, 2), I64)
        return lib.xml_gather_index_rows(P(src), 2, 37, P(ids), 5, P(dst), _st()), {"dst": dst}

    add("gather_index_rows", ["xml_gather_index_rows"], "the last table row, and ids one past the end and below zero", inputs, raw,
        lambda inp: {"dst": _ops().gather_index_rows(inp["src"], inp["ids"])})


_gather_index_rows()


# =====================================================================================================================
# 1. projections and encoders
# =====================================================================================================================
def _gemm_path(rows, n, kbytes):
    """which GEMM xmli_gemm (csrc/linear.hip) runs for an f32 / bf16 product of this shape"""
    if -(-rows // 256) * -(-n // 256) < 64:
        return "fewer than 64 tiles of 256 x 256: the small-tile register-staged kernel"
    if rows >= 256 and n >= 128 and kbytes % 128 == 0 and kbytes >= 256:
        return "%d tiles of 256 x 256, K rows of %d bytes: the 256-row LDS-DMA kernel (gemm256)" % (-(-rows // 256) * -(-n // 256), kbytes)
    return "%d tiles of 256 x 256, K rows of %d bytes (no multiple of 128): the full-size register-staged kernel" % (
        -(-rows // 256) * -(-n // 256), kbytes)


def _linear(dt, rows, n, k, relu, addend, nbytes=1 << 20):
    def inputs():
        g = G(20)
        d = {"x": randn(g, rows, k, dtype=dt), "w": randn(g, n, k, dtype=dt, scale=k ** -0.5), "b": randn(g, n)}
        if addend:
            d["addend"] = randn(g, rows, n, dtype=dt)
        return d

    def raw(lib, A, inp):
        x, w, b = put_all(A, inp, ("x", "w", "b"))
        y = A.take("y", (rows, n), dt)
        if addend:
            ad = A.put("addend", inp["addend"])
            return lib.xml_linear_add(P(x), P(w), P(b), P(ad), P(y), rows, n, k, relu, XDT[dt], _st()), {"y": y}
        return lib.xml_linear(P(x), P(w), P(b), P(y), rows, n, k, relu, XDT[dt], _st()), {"y": y}

    add("linear%s_%s_r%d_n%d_k%d" % ("_add" if addend else "", DTN[dt], rows, n, k), ["xml_linear_add" if addend else "xml_linear"],
        "%s; rows %% 32 = %d, n %% 32 = %d, K bytes %% 128 = %d" % (_gemm_path(rows, n, k * (2 if dt is BF16 else 4)), rows % 32, n % 32,
                                                                 k * (2 if dt is BF16 else 4) % 128), inputs, raw,
        lambda inp: {"y": _ops().linear(inp["x"], inp["w"], inp["b"], relu=bool(relu), addend=inp.get("addend"))}, nbytes=nbytes)


for dt in (F32, BF16):
    for addend in (False, True):
        _linear(dt, 37, 128, 128, 1, addend)
        _linear(dt, 300, 128, 72, 0, addend)        # k = 72 = d_pad of d_in 66: a K tail behind the last full K step
        _linear(dt, 300, 136, 128, 0, addend)       # n = 136: a column tail of 8
        # 33 x 2 = 66 tiles of 256 x 256 (not "few"), a ragged last row tile of 37 rows: K rows of 384 bytes take gemm256,
        # K = 72 (no multiple of 128 bytes) the register-staged kernel at its full tile size
        _linear(dt, 8192 + 37, 512, 96 if dt is F32 else 192, 1, addend, nbytes=1 << 26)
        _linear(dt, 8192 + 37, 512, 72, 0, addend, nbytes=1 << 26)


def _linear_f16s(rows, n, k, nbytes=1 << 22):
    def inputs():
        g = G(21)
        w = randn(g, n, k, scale=k ** -0.5)
        return {"x": randn(g, rows, k), "w": w, "wp": _pack_f16s_weight(w), "b": randn(g, n)}

    def raw(lib, A, inp):
        x, wp, b = put_all(A, inp, ("x", "wp", "b"))
        y = A.take("y", (rows, n), F32)
        ws, nb = A.workspace(lib.xml_linear_f16s_workspace_bytes(rows, k))
        return lib.xml_linear_f16s(P(x), P(wp), P(b), P(y), rows, n, k, 1, ws, nb, _st()), {"y": y}

    def wrap(inp):
        return {"y": _ops().linear(inp["x"], _ops().SplitWeight(inp["wp"], n, k), inp["b"], relu=True)}

    add("linear_f16s_r%d_n%d_k%d" % (rows, n, k), ["xml_linear_f16s", "xml_linear_f16s_workspace_bytes"],
        "%s; K' = 3 k = %d; the split rows live in the workspace" % (
            "the 256-row LDS-DMA kernel (gemm256_f16s)" if rows >= 256 and n >= 128 and k * 6 % 128 == 0 and k * 6 >= 256
            else "the register-staged kernel (rows < 256 or K' rows no multiple of 128 bytes)", 3 * k), inputs, raw, wrap, nbytes=nbytes)


_linear_f16s(37, 128, 128)
_linear_f16s(300, 128, 72)
_linear_f16s(300, 128, 128)                          # 300 rows >= 256, K' rows of 768 bytes: gemm256_f16s, ragged second row tile
_linear_f16s(8192 + 37, 512, 64, nbytes=1 << 26)     # 66 tiles, K' rows of 384 bytes, ragged last row tile


def _model_w(g, n, k, dt, d_in=None):
    """(n, k) projection weight in the dtype the entry takes: plain dt rows, or the packed split-f16 bytes for XML_F16S."""
    w = randn(g, n, k, scale=k ** -0.5)
    if d_in is not None:
        w[:, d_in:] = 0                     # header: columns >= d_in are ZERO (pack time)
    return _pack_f16s_weight(w) if dt == "f16s" else w.to(dt)


def _wrap_w(w, n, k, dt):
    return _ops().SplitWeight(w, n, k) if dt == "f16s" else w


def _dtn(dt):
    return "f16s" if dt == "f16s" else DTN[dt]


def _xdt(dt):
    return XML_F16S if dt == "f16s" else XDT[dt]


def _act(dt):
    return F32 if dt == "f16s" else dt


def _ln_relu_pos(dt, n, seq_len, d_in, hidden, x_f32, note, nbytes=1 << 22):
    d_pad = (d_in + 7) // 8 * 8
    rows = n * seq_len

    def inputs():
        g = G(22)
        return {"x": randn(g, n, seq_len, d_in, dtype=F32 if x_f32 else _act(dt)), "ln_in_g": randn(g, d_in) + 1.0, "ln_in_b": randn(g, d_in),
                "w": _model_w(g, hidden, d_pad, dt, d_in), "b": randn(g, hidden), "pos": randn(g, seq_len, hidden, dtype=_act(dt)),
                "ln_pos_g": randn(g, hidden) + 1.0, "ln_pos_b": randn(g, hidden)}

    def raw(lib, A, inp):
        x, lg, lb, w, b, pos, pg, pb = put_all(A, inp, ("x", "ln_in_g", "ln_in_b", "w", "b", "pos", "ln_pos_g", "ln_pos_b"))
        y = A.take("y", (n, seq_len, hidden), _act(dt))
        ws, nb = A.workspace(lib.xml_linear_ln_relu_pos_workspace_bytes(rows, d_in, hidden, _xdt(dt)))
        st = lib.xml_linear_ln_relu_pos(P(x), XDT[x.dtype], P(lg), P(lb), P(w), P(b), P(pos), P(pg), P(pb), P(y), rows, seq_len, d_in,
                                        hidden, _xdt(dt), ws, nb, _st())
        return st, {"y": y}

    def wrap(inp):
        return {"y": _ops().linear_ln_relu_pos(inp["x"], inp["ln_in_g"], inp["ln_in_b"], _wrap_w(inp["w"], hidden, d_pad, dt), inp["b"],
                                               inp["pos"], inp["ln_pos_g"], inp["ln_pos_b"])}

    add("linear_ln_relu_pos_%s_n%d_l%d_d%d_h%d%s" % (_dtn(dt), n, seq_len, d_in, hidden, "_xf32" if x_f32 and dt is BF16 else ""),
        ["xml_linear_ln_relu_pos", "xml_linear_ln_relu_pos_workspace_bytes"], note, inputs, raw, wrap, nbytes=nbytes)


for dt in (F32, BF16, "f16s"):
    _ln_relu_pos(dt, 1, 37, 128, 128, True, "rows = 37: one ragged row tile")
    _ln_relu_pos(dt, 3, 100, 128, 128, dt is F32, "rows = 300: more rows than one 256-row tile (these products are small: the small-tile kernel)")
    _ln_relu_pos(dt, 1, 37, 66, 128, True, "d_in = 66: d_pad = 72, LayerNorm statistics over 66, GEMM over 72")
for dt, d_in in ((F32, 64), (BF16, 128)):        # K bytes = 256: the smallest the LayerNorm-epilogue GEMM takes
    _ln_relu_pos(dt, 15, 139, d_in, 256, True, "rows = 2048 + 37, hidden 256: the LayerNorm-epilogue GEMM and its scratch formula",
                 nbytes=1 << 24)
    _ln_relu_pos(dt, 15, 139, d_in, 512, True, "rows = 2048 + 37, hidden 512: the epilogue GEMM parks a column tile in 64 MiB of scratch",
                 nbytes=(64 << 20) + (1 << 25))


def _attn_weights(g, hidden, dt):
    return {"wqkv": _model_w(g, 3 * hidden, hidden, dt), "bqkv": randn(g, 3 * hidden, scale=0.1), "wo": _model_w(g, hidden, hidden, dt),
            "bo": randn(g, hidden, scale=0.1), "ln_g": randn(g, hidden) + 1.0, "ln_b": randn(g, hidden)}


def _attention_block(dt, n, seq_len, hidden, heads, note, nbytes=1 << 22):
    def inputs():
        g = G(23)
        d = _attn_weights(g, hidden, dt)
        lens = [seq_len] + [1 + (7 * i) % seq_len for i in range(1, n)]
        d.update(x=randn(g, n, seq_len, hidden, dtype=_act(dt)), key_mask=prefix_mask(lens, seq_len))
        return d

    def raw(lib, A, inp):
        x, m, wqkv, bqkv, wo, bo, lg, lb = put_all(A, inp, ("x", "key_mask", "wqkv", "bqkv", "wo", "bo", "ln_g", "ln_b"))
        y = A.take("y", (n, seq_len, hidden), _act(dt))
        ws, nb = A.workspace(lib.xml_attention_block_workspace_bytes(n, seq_len, hidden, _xdt(dt)))
        st = lib.xml_attention_block(P(x), P(m), P(wqkv), P(bqkv), P(wo), P(bo), P(lg), P(lb), P(y), n, seq_len, hidden, heads, _xdt(dt),
                                     ws, nb, _st())
        return st, {"y": y}

    def wrap(inp):
        return {"y": _ops().attention_block(inp["x"], inp["key_mask"], _wrap_w(inp["wqkv"], 3 * hidden, hidden, dt), inp["bqkv"],
                                            _wrap_w(inp["wo"], hidden, hidden, dt), inp["bo"], inp["ln_g"], inp["ln_b"], heads)}

    add("attention_block_%s_n%d_l%d_h%d" % (_dtn(dt), n, seq_len, hidden), ["xml_attention_block", "xml_attention_block_workspace_bytes"],
        note, inputs, raw, wrap, nbytes=nbytes)


for dt in (F32, BF16, "f16s"):
    _attention_block(dt, 1, 37, 128, 4, "rows = 37, seq_len 37: ragged key blocks of the core, one ragged GEMM row tile")
    _attention_block(dt, 3, 100, 128, 4, "rows = 300, seq_len 100 is no multiple of 16; fewer than 64 big tiles: the small-tile GEMM")
for dt in (F32, BF16):
    _attention_block(dt, 139, 15, 256, 4, "rows = 2048 + 37, hidden 256: output dense + LayerNorm in the epilogue GEMM", nbytes=1 << 25)
    _attention_block(dt, 139, 15, 512, 4, "rows = 2048 + 37, hidden 512: the epilogue GEMM's 64 MiB scratch inside the block's workspace",
                     nbytes=(64 << 20) + (1 << 26))


def _cross_attention(dt, n, lq, lk, hidden, heads, note, nbytes=1 << 22):
    def inputs():
        g = G(24)
        return {"main": randn(g, n, lq, hidden, dtype=_act(dt)), "side": randn(g, n, lk, hidden, dtype=_act(dt)),
                "main_mask": prefix_mask([lq] + [1 + (5 * i) % lq for i in range(1, n)], lq),
                "side_mask": prefix_mask([lk] + [1 + (3 * i) % lk for i in range(1, n)], lk),
                "wq": _model_w(g, hidden, hidden, dt), "bq": randn(g, hidden, scale=0.1), "wkv": _model_w(g, 2 * hidden, hidden, dt),
                "bkv": randn(g, 2 * hidden, scale=0.1), "ln_g": randn(g, hidden) + 1.0, "ln_b": randn(g, hidden)}

    def raw(lib, A, inp):
        mx, mm, sx, sm, wq, bq, wkv, bkv, lg, lb = put_all(A, inp, ("main", "main_mask", "side", "side_mask", "wq", "bq", "wkv", "bkv",
                                                                     "ln_g", "ln_b"))
        y = A.take("y", (n, lq, hidden), _act(dt))
        ws, nb = A.workspace(lib.xml_cross_attention_workspace_bytes(n, lq, lk, hidden, _xdt(dt)))
        st = lib.xml_cross_attention(P(mx), P(mm), P(sx), P(sm), P(wq), P(bq), P(wkv), P(bkv), P(lg), P(lb), P(y), n, lq, lk, hidden,
                                     heads, _xdt(dt), ws, nb, _st())
        return st, {"y": y}

    def wrap(inp):
        return {"y": _ops().cross_attention(inp["main"], inp["main_mask"], inp["side"], inp["side_mask"], _wrap_w(inp["wq"], hidden, hidden, dt),
                                            inp["bq"], _wrap_w(inp["wkv"], 2 * hidden, hidden, dt), inp["bkv"], inp["ln_g"], inp["ln_b"],
                                            heads)}

    add("cross_attention_%s_n%d_lq%d_lk%d_h%d" % (_dtn(dt), n, lq, lk, hidden),
        ["xml_cross_attention", "xml_cross_attention_workspace_bytes"], note, inputs, raw, wrap, nbytes=nbytes)


for dt in (F32, BF16, "f16s"):
    _cross_attention(dt, 3, 13, 21, 128, 4, "lq = 13 != lk = 21: 39 query rows, 63 key rows, both ragged")
    _cross_attention(dt, 12, 25, 31, 128, 4, "300 query rows / 372 key rows: ragged tiles on both sides (small-tile GEMM)")
for dt in (F32, BF16):
    _cross_attention(dt, 139, 15, 7, 256, 4, "rows = 2048 + 37 query rows, hidden 256: the LayerNorm-epilogue GEMM", nbytes=1 << 25)
    _cross_attention(dt, 139, 15, 7, 512, 4, "rows = 2048 + 37 query rows, hidden 512: the epilogue GEMM's 64 MiB scratch in the workspace",
                     nbytes=(64 << 20) + (1 << 26))


# ---- packed variable-length sequences ------------------------------------------------------------------------------------
VARLEN_LENS = [1, 32, 17, 32, 5, 1, 30]            # max_len 32 with lengths 1 and 32 present


def _varlen_lens(rows):
    """Sequence lengths (1 .. 32, with 1 and 32 present) of a packed batch of exactly `rows` tokens."""
    lens = []
    while sum(lens) + VARLEN_LENS[len(lens) % 7] <= rows:
        lens.append(VARLEN_LENS[len(lens) % 7])
    while sum(lens) < rows:
        lens.append(min(32, rows - sum(lens)))
    assert sum(lens) == rows and 1 in lens and 32 in lens and max(lens) <= 32
    return lens


def _pack_plan():
    n, lq = len(VARLEN_LENS), 32

    def inputs():
        return {"mask": prefix_mask(VARLEN_LENS, lq)}

    def raw(lib, A, inp):
        m = A.put("mask", inp["mask"])
        rows = sum(VARLEN_LENS)
        cu = A.take("cu", (n + 1,), I32)
        tail = torch.arange(n * lq) >= rows                  # the header defines packed token i for i < rows, and status[0]
        src = A.take("src", (n * lq,), I32, partly_written=~tail, may_be_written=tail)
        status = A.take("status", (2,), I32, partly_written=torch.tensor([True, False]), may_be_written=torch.tensor([False, True]))
        return lib.xml_pack_plan(P(m), n, lq, P(cu), P(src), P(status), _st()), {"cu": cu, "src": src, "status": status}

    def wrap(inp):
        cu, src, rows = _ops().pack_plan(inp["mask"])
        return {"cu": cu, "src": src, "status": torch.tensor([rows, 0], dtype=I32)}

    add("pack_plan_n7_lq32", ["xml_pack_plan"], "7 sequences of 32 slots, 118 valid tokens: src_row defined for the packed tokens only",
        inputs, raw, wrap)


_pack_plan()


def _ln_relu_pos_packed(dt, d_in, hidden, rows, note, nbytes=1 << 22):
    lens = _varlen_lens(rows)
    n, lq = len(lens), 32

    def inputs():
        g = G(25)
        m = prefix_mask(lens, lq)
        return {"x": randn(g, n * lq, d_in), "src_row": torch.nonzero(m.view(-1))[:, 0].to(I32), "ln_in_g": randn(g, d_in) + 1.0,
                "ln_in_b": randn(g, d_in), "w": _model_w(g, hidden, d_in, dt), "b": randn(g, hidden), "pos": randn(g, lq, hidden, dtype=_act(dt)),
                "ln_pos_g": randn(g, hidden) + 1.0, "ln_pos_b": randn(g, hidden)}

    def raw(lib, A, inp):
        x, sr, lg, lb, w, b, pos, pg, pb = put_all(A, inp, ("x", "src_row", "ln_in_g", "ln_in_b", "w", "b", "pos", "ln_pos_g", "ln_pos_b"))
        y = A.take("y", (rows, hidden), _act(dt))
        ws, nb = A.workspace(lib.xml_linear_ln_relu_pos_packed_workspace_bytes(rows, d_in, hidden, _xdt(dt)))
        st = lib.xml_linear_ln_relu_pos_packed(P(x), XML_F32, P(sr), lq, P(lg), P(lb), P(w), P(b), P(pos), P(pg), P(pb), P(y), rows, d_in,
                                               hidden, _xdt(dt), ws, nb, _st())
        return st, {"y": y}

    def wrap(inp):
        return {"y": _ops().linear_ln_relu_pos_packed(inp["x"], inp["src_row"], rows, lq, inp["ln_in_g"], inp["ln_in_b"],
                                                      _wrap_w(inp["w"], hidden, d_in, dt), inp["b"], inp["pos"], inp["ln_pos_g"],
                                                      inp["ln_pos_b"])}

    add("linear_ln_relu_pos_packed_%s_r%d_d%d_h%d" % (_dtn(dt), rows, d_in, hidden),
        ["xml_linear_ln_relu_pos_packed", "xml_linear_ln_relu_pos_packed_workspace_bytes"],
        "%d packed rows of %d x 32 padded ones; the gathered positional rows live in the workspace; %s" % (rows, n, note), inputs, raw, wrap,
        nbytes=nbytes)


def _attention_block_varlen(dt, hidden, heads, rows, note, nbytes=1 << 22):
    lens = _varlen_lens(rows)
    n = len(lens)

    def inputs():
        g = G(26)
        d = _attn_weights(g, hidden, dt)
        d.update(x=randn(g, rows, hidden, dtype=_act(dt)), cu=_cu(lens))
        return d

    def raw(lib, A, inp):
        x, cu, wqkv, bqkv, wo, bo, lg, lb = put_all(A, inp, ("x", "cu", "wqkv", "bqkv", "wo", "bo", "ln_g", "ln_b"))
        y = A.take("y", (rows, hidden), _act(dt))
        ws, nb = A.workspace(lib.xml_attention_block_varlen_workspace_bytes(rows, hidden, _xdt(dt)))
        st = lib.xml_attention_block_varlen(P(x), P(cu), P(wqkv), P(bqkv), P(wo), P(bo), P(lg), P(lb), P(y), rows, n, 32, hidden, heads,
                                            _xdt(dt), ws, nb, _st())
        return st, {"y": y}

    def wrap(inp):
        return {"y": _ops().attention_block_varlen(inp["x"], inp["cu"], n, 32, _wrap_w(inp["wqkv"], 3 * hidden, hidden, dt), inp["bqkv"],
                                                   _wrap_w(inp["wo"], hidden, hidden, dt), inp["bo"], inp["ln_g"], inp["ln_b"], heads)}

    add("attention_block_varlen_%s_r%d_h%d" % (_dtn(dt), rows, hidden),
        ["xml_attention_block_varlen", "xml_attention_block_varlen_workspace_bytes"],
        "max_len 32, %d sequences of 1 .. 32 tokens (1 and 32 present), %d rows in all; %s" % (n, rows, note), inputs, raw, wrap,
        nbytes=nbytes)


for dt in (F32, BF16, "f16s"):
    for rows, note in ((118, "one ragged row tile"), (300, "more rows than one 256-row block, ragged end")):
        _ln_relu_pos_packed(dt, 72, 128, rows, note)
        _attention_block_varlen(dt, 128, 4, rows, note)
for dt, d_in in ((F32, 64), (BF16, 128)):          # K bytes = 256; rows = 2048 + 37: dispatch::gemm_ln_fused accepts both entries
    _ln_relu_pos_packed(dt, d_in, 256, 2085, "hidden 256: the LayerNorm-epilogue GEMM beside the 3-launch scratch formula", nbytes=1 << 25)
    _ln_relu_pos_packed(dt, d_in, 512, 2085, "hidden 512: the epilogue GEMM's 64 MiB scratch inside the packed workspace",
                        nbytes=(64 << 20) + (1 << 26))
    _attention_block_varlen(dt, 256, 4, 2085, "hidden 256: output dense + LayerNorm in the epilogue GEMM", nbytes=1 << 25)
    _attention_block_varlen(dt, 512, 4, 2085, "hidden 512: the epilogue GEMM's 64 MiB scratch inside the block's workspace",
                            nbytes=(64 << 20) + (1 << 26))


# =====================================================================================================================
# 2. attention core and pooling
# =====================================================================================================================
def _attention_core(dt, skew):
    n, lq, lk, hidden, heads = 3, 13, 21, 128, 4
    es = 2 if dt is BF16 else 4

    def inputs():
        g = G(30)
        return {"qs": randn(g, n, lq, 3 * hidden, dtype=dt), "kvs": randn(g, n, lk, 3 * hidden, dtype=dt),
                "q_mask": prefix_mask([lq, 1, 7], lq), "k_mask": prefix_mask([lk, 20, 1], lk)}

    def raw(lib, A, inp):
        # q = column block 0 of one stacked (n, lq, 3H) tensor, k / v = column blocks 1 and 2 of a stacked (n, lk, 3H) one
        qs, kvs = A.put("qs", inp["qs"], skew=skew), A.put("kvs", inp["kvs"], skew=skew)
        qm, km = put_all(A, inp, ("q_mask", "k_mask"))
        out = A.take("out", (n, lq, hidden), dt, skew=skew)
        st = lib.xml_attention_core(P(qs), 3 * hidden, P(kvs, hidden * es), 3 * hidden, P(kvs, 2 * hidden * es), 3 * hidden, P(qm), P(km),
                                    P(out), n, lq, lk, hidden, heads, XDT[dt], _st())
        return st, {"out": out}

    def wrap(inp):
        q = inp["qs"][..., :hidden].contiguous()
        k, v = inp["kvs"][..., hidden:2 * hidden].contiguous(), inp["kvs"][..., 2 * hidden:].contiguous()
        return {"out": _ops().attention_core(q, k, v, inp["q_mask"], inp["k_mask"], heads)}

    add("attention_core_%s_skew%d" % (DTN[dt], skew), ["xml_attention_core"],
        "lq = 13, lk = 21, ld = 3 H: q / k / v are offset pointers into stacked tensors; base %d bytes past a 256-byte line" % skew,
        inputs, raw, wrap)


for dt in (F32, BF16):
    _attention_core(dt, 0)
    _attention_core(dt, 16)


def _modular_pool(dt, hidden, n_mod, att, varlen):
    n, lq = (len(VARLEN_LENS), 32) if varlen else (5, 13)
    lens = VARLEN_LENS if varlen else [13, 1, 7, 12, 2]
    sym = "xml_modular_pool" + ("_att" if att else "") + ("_varlen" if varlen else "")

    def inputs():
        g = G(31)
        d = {"w_m": randn(g, n_mod, hidden, scale=hidden ** -0.5)}
        if varlen:
            d.update(enc=randn(g, sum(lens), hidden, dtype=dt), cu=_cu(lens))
        else:
            d.update(enc=randn(g, n, lq, hidden, dtype=dt), mask=prefix_mask(lens, lq))
        return d

    def raw(lib, A, inp):
        enc, wm = put_all(A, inp, ("enc", "w_m"))
        second = A.put("cu", inp["cu"]) if varlen else A.put("mask", inp["mask"])
        out = A.take("out", (n_mod, n, hidden), dt)
        outs = {"out": out}
        args = [P(enc), P(second), P(wm), P(out)]
        if att:
            outs["att"] = A.take("att", (n, lq, n_mod), F32)
            args.append(P(outs["att"]))
        return getattr(lib, sym)(*(args + [n, lq, hidden, n_mod, XDT[dt], _st()])), outs

    def wrap(inp):
        if varlen:
            r = _ops().modular_pool_varlen(inp["enc"], inp["cu"], n, lq, inp["w_m"], return_att=att)
        else:
            r = _ops().modular_pool(inp["enc"], inp["mask"], inp["w_m"], return_att=att)
        return {"out": r[0], "att": r[1]} if att else {"out": r}

    # the packed-sequence forms have no scalar path: hidden % 8 != 0 is refused before any launch (XML_ERR_UNSUPPORTED)
    refused = varlen and hidden % 8 != 0
    add("%s_%s_h%d_m%d" % (sym[4:], DTN[dt], hidden, n_mod), [sym],
        "hidden %d (%s), n_mod %d, sequences of 1 token and of the full length"
        % (hidden, "vector path" if hidden % 8 == 0 else ("refused: nothing is written" if refused else "scalar path"), n_mod),
        inputs, raw, None if refused else wrap, expect_status=-2 if refused else 0)


for dt in (F32, BF16):
    for hidden in (128, 100):
        for n_mod in (1, 2):
            for att in (False, True):
                for varlen in (False, True):
                    _modular_pool(dt, hidden, n_mod, att, varlen)


# =====================================================================================================================
# 3. K6
# =====================================================================================================================
def _k6_operands(g, nq, nv, lpad, hidden, dt, n_mod):
    d = {}
    for m in range(n_mod):
        lens = [lpad] + [1 + (11 * i + 3 * m) % lpad for i in range(1, nv)]
        mask = prefix_mask(lens, lpad)
        d["qn%d" % m] = unit(g, nq, hidden, dtype=dt)
        d["cn%d" % m] = (unit(g, nv, lpad, hidden) * mask[..., None]).to(dt)        # zero rows beyond a video's stored length
        d["mask%d" % m] = mask
    return d


def _q2c_scores(dt, lpad, hidden, skew, ld_extra=3):
    nq, nv = 70, 5                                    # both operands end inside their first 256-row tile
    ld = nv + ld_extra

    def inputs():
        return _k6_operands(G(40), nq, nv, lpad, hidden, dt, 2)

    def raw(lib, A, inp):
        q0, c0, m0, q1, c1, m1 = put_all(A, inp, ("qn0", "cn0", "mask0", "qn1", "cn1", "mask1"))
        out = A.take("out", (nq, nv), F32, ld=ld, skew=skew)
        st = [lib.xml_q2c_scores(P(q0), P(c0), P(m0), P(out), ld, nq, nv, lpad, hidden, 0, XDT[dt], _st()),
              lib.xml_q2c_scores(P(q1), P(c1), P(m1), P(out), ld, nq, nv, lpad, hidden, 1, XDT[dt], _st())]      # combine
        fused = A.take("fused", (nq, nv), F32, ld=ld, skew=skew)
        st.append(lib.xml_q2c_scores_fused(2, P(q0), P(c0), P(m0), P(q1), P(c1), P(m1), P(fused), ld, nq, nv, lpad, hidden, XDT[dt], _st()))
        one = A.take("one", (nq, nv), F32, ld=ld, skew=skew)
        st.append(lib.xml_q2c_scores_fused(1, P(q0), P(c0), P(m0), None, None, None, P(one), ld, nq, nv, lpad, hidden, XDT[dt], _st()))
        return st, {"out": out, "fused": fused, "one": one}

    def wrap(inp):
        o = _ops()
        out = o.q2c_scores(inp["qn0"], inp["cn0"], inp["mask0"])
        out = o.q2c_scores(inp["qn1"], inp["cn1"], inp["mask1"], out=out, combine=True)
        qn, cn, mk = [inp["qn0"], inp["qn1"]], [inp["cn0"], inp["cn1"]], [inp["mask0"], inp["mask1"]]
        return {"out": out, "fused": o.q2c_scores_fused(qn, cn, mk), "one": o.q2c_scores_fused(qn[:1], cn[:1], mk[:1])}

    add("q2c_scores_%s_l%d_h%d_skew%d%s" % (DTN[dt], lpad, hidden, skew, "" if ld_extra == 3 else "_ld%d" % ld_extra),
        ["xml_q2c_scores", "xml_q2c_scores_fused"],
        "nq = 70, nv = 5, lpad = %d, ld_out = nv + %d, out %d bytes past a 256-byte line: ragged query and video tiles, row gaps in the "
        "score matrix" % (lpad, ld_extra, skew), inputs, raw, wrap,
        nbytes=1 << 23)


for dt, hidden in ((F32, 128), (BF16, 256)):
    for lpad in (16, 112, 128):
        _q2c_scores(dt, lpad, hidden, 0)
    _q2c_scores(dt, 128, hidden, 4)
    _q2c_scores(dt, 16, hidden, 4)
    _q2c_scores(dt, 128, hidden, 4, ld_extra=7)      # ld_out = 12: ld % 4 == 0 behind a base 4 bytes past a line
    _q2c_scores(dt, 112, hidden, 4, ld_extra=7)
_q2c_scores(BF16, 112, 40, 0)                        # 80-byte rows: the register-staged kernel (no LDS-DMA path)


def _tiled_bytes(lib, rows, hidden, dt):
    return int(lib.xml_q2c_tiled_bytes(rows, hidden, XDT[dt]))


def _q2c_tile_rows(dt, hidden, rows):
    rows_dst = (rows + 255) // 256 * 256

    def inputs():
        g = G(41)
        rm = torch.randint(-1, rows, (rows_dst,), generator=g).to(I32)
        rm[::7] = -1
        return {"src": randn(g, rows, hidden, dtype=dt), "row_map": rm}

    def raw(lib, A, inp):
        src, rm = put_all(A, inp, ("src", "row_map"))
        nb = _tiled_bytes(lib, rows, hidden, dt)
        assert nb == rows_dst * hidden * src.element_size()
        n = nb // src.element_size()
        t, gt = A.take("tiled", (n,), dt), A.take("gathered", (n,), dt)
        st = [lib.xml_q2c_tile_rows(P(src), P(t), rows, hidden, XDT[dt], _st()),
              lib.xml_q2c_tile_rows_gather(P(src), P(rm), P(gt), rows_dst, hidden, XDT[dt], _st())]
        outs = {"tiled": t, "gathered": gt}
        assert lib.xml_q2c_tile_rows_l2norm_ok(hidden, XDT[dt]) == (dt is not F16)      # hi planes are tiled, never normalised
        if dt is not F16:
            tn, gn = A.take("tiled_l2norm", (n,), dt), A.take("gathered_l2norm", (n,), dt)
            st += [lib.xml_q2c_tile_rows_l2norm(P(src), None, P(tn), rows, rows_dst, hidden, XDT[dt], _st()),
                   lib.xml_q2c_tile_rows_l2norm(P(src), P(rm), P(gn), rows, rows_dst, hidden, XDT[dt], _st())]
            outs.update(tiled_l2norm=tn, gathered_l2norm=gn)
        return st, outs

    def wrap(inp):
        o = _ops()
        x, rm = inp["src"], inp["row_map"]
        out = {"tiled": o._tile(x, rows).data, "gathered": o._tile(x, rows_dst, rm).data}
        if dt is not F16:
            out.update(tiled_l2norm=o._tile(x, rows, None, True).data, gathered_l2norm=o._tile(x, rows_dst, rm, True).data)
        return out

    add("q2c_tile_rows_%s_h%d_r%d" % (DTN[dt], hidden, rows),
        ["xml_q2c_tile_rows", "xml_q2c_tile_rows_gather", "xml_q2c_tiled_bytes"] + ([] if dt is F16 else ["xml_q2c_tile_rows_l2norm"]),
        "%d rows: the last tile holds %d source rows and zero rows behind them; images of exactly xml_q2c_tiled_bytes" % (rows, rows % 256),
        inputs, raw, wrap, nbytes=1 << 23)


for dt, hidden in ((F32, 128), (BF16, 256), (F16, 256)):
    _q2c_tile_rows(dt, hidden, 70)
    _q2c_tile_rows(dt, hidden, 5 * 128)


def _q2c_scores_tiled(dt, hidden, mode, skew):
    nq, nv, lpad = 70, 5, 128
    ld = nv + 3

    def inputs():
        o = _ops()
        d = _k6_operands(G(42), nq, nv, lpad, hidden, F32, 2)
        if dt is F16:      # hi planes of the split rows at the fixed unit scale (xml_split_f16_rows)
            for k in ("qn0", "qn1", "cn0", "cn1"):
                d[k] = o.split_f16_rows(d[k].to(DEV), fixed_log2=o.F16_UNIT_LOG2, want_hi=True)[1].cpu()
        else:
            for k in ("qn0", "qn1", "cn0", "cn1"):
                d[k] = d[k].to(dt)
        if mode == 1:
            d["mask0"], d["mask1"] = torch.ones(nv, lpad), torch.ones(nv, lpad)
        for k in ("qn0", "qn1", "cn0", "cn1"):
            d[k + "_t"] = o.q2c_tile_rows(d[k].to(DEV)).data.cpu()
        for m in (0, 1):
            d["bits%d" % m] = o._pack_bits32(d["mask%d" % m] != 0)
        return d

    def raw(lib, A, inp):
        q0, c0, q1, c1, m0, m1 = put_all(A, inp, ("qn0_t", "cn0_t", "qn1_t", "cn1_t", "mask0", "mask1"))
        b0, b1 = put_all(A, inp, ("bits0", "bits1")) if mode == 2 else (None, None)
        assert lib.xml_q2c_tiled_ok(lpad, hidden, XDT[dt]) == 1
        out = A.take("out", (nq, nv), F32, ld=ld, skew=skew)
        st = lib.xml_q2c_scores_tiled(2, P(q0), P(c0), P(m0), P(q1), P(c1), P(m1), P(out), ld, nq, nv, lpad, hidden, XDT[dt], mode, P(b0),
                                      P(b1), _st())
        return st, {"out": out}

    def wrap(inp):
        o = _ops()
        cn = []
        for m in (0, 1):
            t = o.TiledRows(inp["cn%d_t" % m], nv * lpad, hidden, (nv, lpad, hidden), all_valid=mode == 1)
            t.mask_bits = inp["bits%d" % m] if mode == 2 else None
            cn.append(t)
        return {"out": o.q2c_scores_fused([inp["qn0"], inp["qn1"]], cn, [inp["mask0"], inp["mask1"]])}

    add("q2c_scores_tiled_%s_h%d_mode%d_skew%d" % (DTN[dt], hidden, mode, skew), ["xml_q2c_scores_tiled", "xml_q2c_tiled_ok"],
        "nq = 70, nv = 5 (640 clip rows: 2.5 tiles), ld_out = nv + 3, mask mode %d" % mode, inputs, raw, wrap, nbytes=1 << 23)


for dt, hidden in ((F32, 128), (BF16, 256), (F16, 256)):
    for mode in (0, 1, 2):
        _q2c_scores_tiled(dt, hidden, mode, 0)
    _q2c_scores_tiled(dt, hidden, 0, 4)


def _q2c_scores_packed(dt, hidden, skew):
    nq, nv, lpad = 70, 9, 128
    ld = nv + 3
    lens = [128, 1, 16, 17, 100, 40, 64, 5, 90]

    def inputs():
        o = _ops()
        g = G(43)
        mask = prefix_mask(lens, lpad)
        d = {"mask": mask}
        plan = o.q2c_pack_plan([mask.to(DEV), mask.to(DEV)])
        assert plan is not None
        d["slot_ids"], d["n_tiles"] = plan.slot_ids.cpu(), plan.n_tiles
        for m in (0, 1):
            q, c = unit(g, nq, hidden), unit(g, nv, lpad, hidden) * mask[..., None]
            if dt is F16:
                q = o.split_f16_rows(q.to(DEV), fixed_log2=o.F16_UNIT_LOG2, want_hi=True)[1].cpu()
                c = o.split_f16_rows(c.to(DEV), fixed_log2=o.F16_UNIT_LOG2, want_hi=True)[1].cpu()
            q, c = q.to(dt), c.to(dt)
            d["qn%d" % m], d["cn%d" % m] = q, c
            d["qt%d" % m] = o.q2c_tile_rows(q.to(DEV)).data.cpu()
            t = o.pack_q2c_corpus(c.to(DEV), mask.to(DEV), plan=plan)
            d["ct%d" % m], d["bits%d" % m] = t.data.cpu(), t.mask_bits.cpu()
        return d

    def raw(lib, A, inp):
        q0, c0, q1, c1, ids, b0, b1 = put_all(A, inp, ("qt0", "ct0", "qt1", "ct1", "slot_ids", "bits0", "bits1"))
        out = A.take("out", (nq, nv), F32, ld=ld, skew=skew)
        st = lib.xml_q2c_scores_packed(2, P(q0), P(c0), P(q1), P(c1), P(out), ld, nq, inp["n_tiles"], P(ids), P(b0), P(b1), hidden, XDT[dt],
                                       _st())
        return st, {"out": out}

    def wrap(inp):
        o = _ops()
        mask = inp["mask"]
        plan = o.q2c_pack_plan([mask, mask])
        cn = [o.pack_q2c_corpus(inp["cn%d" % m], mask, plan=plan) for m in (0, 1)]
        return {"out": o.q2c_scores_fused([inp["qn0"], inp["qn1"]], cn, [mask, mask])}

    add("q2c_scores_packed_%s_h%d_skew%d" % (DTN[dt], hidden, skew), ["xml_q2c_scores_packed"],
        "9 ragged videos packed into tiles, nq = 70: the last query tile and the last wave tile are ragged; ld_out = nv + 3 = 12, out %d "
        "bytes past a 256-byte line" % skew, inputs, raw, wrap,
        nbytes=1 << 23)


for dt, hidden in ((F32, 128), (BF16, 256), (F16, 256)):
    _q2c_scores_packed(dt, hidden, 0)
    _q2c_scores_packed(dt, hidden, 4)


def _q2c_rescore(dt, lpad, hidden):
    nq, nv, kp = 70, 5, 7

    def inputs():
        o = _ops()
        g = G(44)
        d = _k6_operands(g, nq, nv, lpad, hidden, F32, 2)
        pv = torch.randint(0, nv, (nq, kp), generator=g).to(I32)
        pv[0, 0], pv[1, 1], pv[69, 6] = -1, nv, nv - 1
        d["pair_vid"] = pv
        for k in ("qn0", "qn1", "cn0", "cn1"):
            d[k] = o.split_f16_rows(d[k].to(DEV), fixed_log2=o.F16_UNIT_LOG2).data.cpu() if dt == "f16s" else d[k].to(dt)
        return d

    def raw(lib, A, inp):
        q0, q1, c0, c1, m0, m1, pv = put_all(A, inp, ("qn0", "qn1", "cn0", "cn1", "mask0", "mask1", "pair_vid"))
        out = A.take("out", (nq, kp), F32)
        ws, nb = A.workspace(lib.xml_q2c_rescore_workspace_bytes(nq, nv, kp))
        st = lib.xml_q2c_rescore(2, P(q0), P(q1), P(c0), P(c1), P(m0), P(m1), P(pv), P(out), nq, nv, kp, lpad, hidden, _xdt(dt), ws, nb,
                                 _st())
        return st, {"out": out}

    def wrap(inp):
        o = _ops()

        def rows(t):
            if dt != "f16s":
                return t
            return o.SplitRows(t, torch.full(t.shape[:-1], 2.0 ** -o.F16_UNIT_LOG2, device=t.device))
        return {"out": o.q2c_rescore([rows(inp["qn0"]), rows(inp["qn1"])], [rows(inp["cn0"]), rows(inp["cn1"])],
                                     [inp["mask0"], inp["mask1"]], inp["pair_vid"])}

    add("q2c_rescore_%s_l%d_h%d" % (_dtn(dt), lpad, hidden), ["xml_q2c_rescore", "xml_q2c_rescore_workspace_bytes"],
        "nq = 70, nv = 5, 7 pairs per query, pair ids -1 and nv present; the inverted pair list lives in the workspace", inputs, raw, wrap,
        nbytes=1 << 23)


for lpad in (16, 112, 128):
    _q2c_rescore(F32, lpad, 128)
_q2c_rescore(BF16, 112, 256)
_q2c_rescore("f16s", 112, 128)


# =====================================================================================================================
# 4. selection and lists
# =====================================================================================================================
def _allow_words(g, rows, n_words):
    w = torch.randint(-2 ** 31, 2 ** 31, (rows, n_words), generator=g, dtype=I64).to(I32)
    return w


def _topk(skew, allowed, payload, alpha, rows=6, n=300, k=100, ld_extra=3):
    ld, col0 = n + ld_extra, 5
    need = (col0 + n + 31) // 32
    ld_allow = need + 2

    def inputs():
        g = G(50)
        s = randn(g, rows, n)
        s[1, :50] = s[1, 50]                                  # ties
        d = {"scores": s, "pay": torch.stack([torch.randperm(100000, generator=g)[:n] for _ in range(rows)]).to(I32)}
        if allowed:
            a = _allow_words(g, rows, need)
            a[2] = 0                                           # a row without any allowed column
            a[3, 3:] = 0                                       # a row with fewer than k allowed columns
            d["allow"] = a
        return d

    def raw(lib, A, inp):
        s = A.put("scores", inp["scores"], ld=ld, skew=skew)
        pay = A.put("pay", inp["pay"], ld=ld, skew=skew) if payload else None            # the payload shares the row stride ld
        val, idx = A.take("val", (rows, k), F32), A.take("idx", (rows, k), I32)
        ws, nb = A.workspace(lib.xml_topk_rows_workspace_bytes(rows, n, k))
        if not allowed:
            return lib.xml_topk_rows(P(s), ld, P(pay), P(val), P(idx), rows, n, k, alpha, ws, nb, _st()), {"val": val, "idx": idx}
        al = A.put("allow", inp["allow"], ld=ld_allow, skew=skew)
        cnt = A.take("cnt", (rows,), I32)
        st = lib.xml_topk_rows_allowed(P(s), ld, P(pay), P(al), ld_allow, rows, col0, P(val), P(idx), P(cnt), rows, n, k, alpha, ws, nb, _st())
        return st, {"val": val, "idx": idx, "cnt": cnt}

    def wrap(inp):
        pay = inp["pay"] if payload else None
        if not allowed:
            v, i = _ops().topk_rows(inp["scores"], k, alpha, pay)
            return {"val": v, "idx": i}
        v, i, c = _ops().topk_rows(inp["scores"], k, alpha, pay, allow=inp["allow"], col0=col0, return_count=True)
        return {"val": v, "idx": i, "cnt": c}

    add("topk_rows%s_%s_alpha%g_skew%d%s" % ("_allowed" if allowed else "", "payload" if payload else "columns", alpha, skew,
                                             "" if ld_extra == 3 else "_ld%d" % ld_extra),
        ["xml_topk_rows_allowed" if allowed else "xml_topk_rows", "xml_topk_rows_workspace_bytes"],
        "rows 6, n 300, k 100, ld = n + %d%s; scores %d bytes past a 256-byte line" % (
            ld_extra, ", col0 = 5, ld_allow = words + 2" if allowed else "", skew),
        inputs, raw, wrap)


for skew in (0, 4):
    for allowed in (False, True):
        _topk(skew, allowed, True, 20.0)
        _topk(skew, allowed, False, 0.0)
for allowed in (False, True):        # a base 4 bytes past a line with ld % 4 == 0: every row is misaligned the same way
    _topk(4, allowed, True, 20.0, ld_extra=4)


def _canon_rows(t, mask):
    big = torch.iinfo(t.dtype).max
    return torch.where(mask, t, torch.full_like(t, big)).sort(dim=1).values


def _select_ge(skew, allowed, cap, ld_extra=3):
    rows, n = 6, 300
    ld, col0 = n + ld_extra, 5
    need = (col0 + n + 31) // 32
    ld_allow = need + 2

    def inputs():
        g = G(51)
        d = {"scores": randn(g, rows, n), "thr": torch.tensor([0.0, 1.5, 9.0, -9.0, 0.5, 2.5])}
        if allowed:
            d["allow"] = _allow_words(g, rows, need)
        return d

    def selected(inp):
        ge = inp["scores"] >= inp["thr"][:, None]
        if allowed:
            c = torch.arange(n) + col0
            ge &= ((inp["allow"].long()[:, c >> 5] >> (c & 31)[None]) & 1).bool()
        return ge

    def count(inp):
        return selected(inp).sum(1)

    def raw(lib, A, inp):
        s, thr = A.put("scores", inp["scores"], ld=ld, skew=skew), A.put("thr", inp["thr"])
        cnt = A.take("cnt", (rows,), I32)
        outs = {"cnt": cnt}
        idx = None
        if cap:     # entries beyond cnt[row] are left untouched
            idx = outs["idx"] = A.take("idx", (rows, cap), I32, partly_written=torch.arange(cap)[None] < count(inp)[:, None])
        if allowed:
            al = A.put("allow", inp["allow"], ld=ld_allow, skew=skew)
            return lib.xml_select_ge_rows_allowed(P(s), ld, P(thr), P(al), ld_allow, rows, col0, P(idx), cap, P(cnt), rows, n, _st()), outs
        return lib.xml_select_ge_rows(P(s), ld, P(thr), P(idx), cap, P(cnt), rows, n, _st()), outs

    def wrap(inp):
        kw = dict(allow=inp["allow"], col0=col0) if allowed else {}
        r = _ops().select_ge_rows(inp["scores"], inp["thr"], cap or None, **kw)
        return {"idx": r[0], "cnt": r[1]} if cap else {"cnt": r}

    def canon(t, mask):
        """rows in ascending order; a row with more selected columns than cap holds an unspecified subset of them: its cap
        entries must be distinct selected columns, and are then taken out of the comparison"""
        t = _canon_rows(t, mask)
        sel = selected(inputs())
        for r in torch.nonzero(sel.sum(1) > cap)[:, 0].tolist():
            row = t[r].long()
            assert bool(((row >= 0) & (row < n)).all()), "row %d: an index outside [0, n): %s" % (r, row.tolist())
            assert row.unique().numel() == cap, "row %d: %d distinct entries of %d" % (r, row.unique().numel(), cap)
            assert bool(sel[r][row].all()), "row %d: a column below the threshold or disallowed was selected" % r
            t[r] = 0
        return t

    add("select_ge_rows%s_cap%d_skew%d%s" % ("_allowed" if allowed else "", cap, skew, "" if ld_extra == 3 else "_ld%d" % ld_extra),
        ["xml_select_ge_rows_allowed" if allowed else "xml_select_ge_rows"],
        "rows 6, n 300, ld = n + %d, scores %d bytes past a 256-byte line; rows with 0 and with all 300 columns selected; %s" % (
            ld_extra, skew, "counts only (idx = NULL)" if cap == 0 else ("cap %d is smaller than some counts" % cap if cap < n
                                                                          else "cap %d holds every row's list" % cap)),
        inputs, raw, wrap, canon={"idx": canon})


for skew in (0, 4):
    for allowed in (False, True):
        _select_ge(skew, allowed, 0)
        _select_ge(skew, allowed, 300)
_select_ge(0, False, 40)        # cap < some counts: those rows must hold 40 distinct selected columns, WHICH is unspecified
_select_ge(0, True, 40)
_select_ge(4, True, 300, ld_extra=4)     # a base 4 bytes past a line with ld % 4 == 0: every row is misaligned the same way


def _merge_shard_topk():
    world, rows, c, k = 3, 5, 37, 100

    def inputs():
        g = G(52)
        s = randn(g, world, rows, c).sort(dim=2, descending=True).values
        return {"score": s, "id": torch.randperm(world * rows * c, generator=g).view(world, rows, c).to(I32)}

    def raw(lib, A, inp):
        s, i = put_all(A, inp, ("score", "id"))
        val, idx = A.take("val", (rows, k), F32), A.take("idx", (rows, k), I32)
        ws, nb = A.workspace(lib.xml_merge_shard_topk_workspace_bytes(world, rows, c))
        return lib.xml_merge_shard_topk(P(s), P(i), world, rows, c, k, 20.0, P(val), P(idx), ws, nb, _st()), {"val": val, "idx": idx}

    def wrap(inp):
        v, i = _ops().merge_shard_topk(inp["score"], inp["id"], k, 20.0)
        return {"val": v, "idx": i}

    add("merge_shard_topk_w3_c37_k100", ["xml_merge_shard_topk", "xml_merge_shard_topk_workspace_bytes"],
        "3 shards x 37 candidates = 111 >= k = 100: the staged row in the workspace is no multiple of 64 entries", inputs, raw, wrap)


_merge_shard_topk()


def _exact_certificate():
    nq, m, k = 70, 37, 10

    def inputs():
        g = G(53)
        return {"filter": randn(g, nq, m).sort(dim=1, descending=True).values, "top": randn(g, nq, k).sort(dim=1, descending=True).values,
                "eq0": torch.rand(nq, generator=g) * 1e-3, "eq1": torch.rand(nq, generator=g) * 1e-3}

    def raw(lib, A, inp):
        f, e0, e1 = put_all(A, inp, ("filter", "eq0", "eq1"))
        top = A.take("top", (nq, k), F32)
        top.copy_(inp["top"])                                   # raw on entry, exp(alpha s) on return: an in-out operand
        nf = A.take("n_fail", (1,), I32)
        nf.zero_()                                              # zeroed by the caller
        fail, eps, thr = A.take("fail", (nq,), I32), A.take("eps", (nq,), F32), A.take("thr", (nq,), F32)
        st = lib.xml_exact_certificate(P(f), m, P(top), k, P(e0), P(e1), 1e-3, 2e-3, 2, 1e-6, 20.0, 1, P(fail), P(eps), P(thr), P(nf), nq,
                                       _st())
        return st, {"top": top, "fail": fail, "eps": eps, "thr": thr, "n_fail": nf}

    def wrap(inp):
        top = inp["top"].clone()
        fail, eps, thr, nf = _ops().exact_certificate(inp["filter"], top, [inp["eq0"], inp["eq1"]], [1e-3, 2e-3], 1e-6, 20.0, True)
        return {"top": top, "fail": fail, "eps": eps, "thr": thr, "n_fail": nf}

    add("exact_certificate_nq70", ["xml_exact_certificate"], "nq = 70: a ragged block of queries; m = 37, k = 10 rows of odd length",
        inputs, raw, wrap)


_exact_certificate()


class _Parts(object):
    def __init__(self, part_video, group_start):
        self.part_video, self.group_start = part_video, group_start


PART_COUNTS = [1, 3, 1, 2, 5, 1, 1, 4, 1, 2, 1, 3, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1]        # 23 videos in 37 index rows


def _part_tables():
    pv = torch.repeat_interleave(torch.arange(len(PART_COUNTS)), torch.tensor(PART_COUNTS)).to(I32)
    return pv, _cu(PART_COUNTS)


def _group_best_allow(skew, allow_rows):
    rows, n_videos = 6, len(PART_COUNTS)
    n_parts = sum(PART_COUNTS)
    ld, words = n_parts + 3, (n_parts + 31) // 32
    out_ld, allow_ld = words + 2, (n_videos + 31) // 32 + 1

    def inputs():
        g = G(54)
        s = randn(g, rows, n_parts)
        s[0, 1:4] = s[0, 1]                                    # ties: the lowest row wins
        s[1, 4] = float("nan")
        s[2, 6:11] = float("-inf")
        pv, gs = _part_tables()
        d = {"scores": s, "part_video": pv, "group_start": gs}
        if allow_rows:
            d["allow"] = _allow_words(g, allow_rows, (n_videos + 31) // 32)
        return d

    def raw(lib, A, inp):
        s = A.put("scores", inp["scores"], ld=ld, skew=skew)
        pv, gs = put_all(A, inp, ("part_video", "group_start"))
        al = A.put("allow", inp["allow"], ld=allow_ld, skew=skew) if allow_rows else None
        # words beyond ceil(n_parts / 32) are not written: here the row gaps of out_ld = words + 2
        out = A.take("bits", (rows, words), I32, ld=out_ld, skew=skew)
        st = lib.xml_group_best_allow(P(s), ld, rows, n_parts, P(pv), P(gs), n_videos, P(al), allow_ld if allow_rows else 0, allow_rows,
                                      P(out), out_ld, _st())
        return st, {"bits": out}

    def wrap(inp):
        return {"bits": _ops().group_best_allow(inp["scores"], _Parts(inp["part_video"], inp["group_start"]), inp.get("allow"))}

    add("group_best_allow_rows%d_skew%d" % (allow_rows, skew), ["xml_group_best_allow"],
        "37 index rows of 23 videos: 2 bit words with 27 padding bits; ld = n_parts + 3, out_ld = words + 2, allow_ld = words + 1",
        inputs, raw, wrap)


for skew in (0, 4):
    for allow_rows in (0, 1, 6):
        _group_best_allow(skew, allow_rows)


def _best_part_rows():
    rows, n_videos = 6, len(PART_COUNTS)
    n_parts = sum(PART_COUNTS)
    ld = n_parts + 3

    def inputs():
        pv, gs = _part_tables()
        return {"scores": randn(G(55), rows, n_parts), "part_video": pv, "group_start": gs,
                "video": torch.tensor([4, 0, 22, 23, -1, 7], dtype=I32)}

    def raw(lib, A, inp):
        s = A.put("scores", inp["scores"], ld=ld, skew=4)
        gs, vid = put_all(A, inp, ("group_start", "video"))
        out = A.take("out", (rows,), I32)
        return lib.xml_best_part_rows(P(s), ld, rows, P(gs), n_videos, P(vid), P(out), _st()), {"out": out}

    add("best_part_rows", ["xml_best_part_rows"], "ld = n_parts + 3; the last video, and ids one past the end and below zero", inputs, raw,
        lambda inp: {"out": _ops().best_part_rows(inp["scores"], _Parts(inp["part_video"], inp["group_start"]), inp["video"])})


_best_part_rows()


# =====================================================================================================================
# 5. K7, K9, K10 - K12
# =====================================================================================================================
def _conv1d(ksize, l):
    rows = 3

    def inputs():
        g = G(60)
        return {"x": randn(g, rows, l), "w": randn(g, ksize)}

    def raw(lib, A, inp):
        x, w = put_all(A, inp, ("x", "w"))
        y = A.take("y", (rows, l), F32)
        return lib.xml_conv1d_rows(P(x), P(w), P(y), rows, l, ksize, _st()), {"y": y}

    add("conv1d_rows_k%d_l%d" % (ksize, l), ["xml_conv1d_rows"], "taps reach %d positions past both row ends; the next row starts right there"
        % (ksize // 2), inputs, raw, lambda inp: {"y": _ops().conv1d_rows(inp["x"], inp["w"])})


for ksize in (1, 5, 15):
    for l in (1, 37, 128):
        _conv1d(ksize, l)


def _convse_inputs(g, nq, nv, kp, lpad, l_ref, hidden, n_mod, n_conv, ksize, dt):
    o = _ops()
    lens = [l_ref] + [1 + (13 * i) % l_ref for i in range(1, nv)]
    d = {"vid_len": torch.tensor(lens, dtype=I32), "conv_w": randn(g, 2 * n_conv * ksize, scale=0.3)}
    pv = torch.randint(0, nv, (nq, kp), generator=g).to(I32)
    if kp > 1:
        pv[0, 1], pv[nq - 1, kp - 1] = -1, -1                 # skipped pairs
    d["pair_vid"] = pv
    d["pair_w"] = torch.rand(nq, kp, generator=g)
    for m in range(n_mod):
        mask = prefix_mask(lens, lpad)
        q, f2 = randn(g, nq, hidden, scale=hidden ** -0.5), randn(g, nv, lpad, hidden) * (torch.arange(lpad) < l_ref).float()[None, :, None]
        d["mask%d" % m] = mask
        if dt == "f16s":
            sq, sf = o.split_f16_rows(q.to(DEV)), o.split_f16_rows(f2.to(DEV))
            d["q%d" % m], d["qinv%d" % m], d["f%d" % m], d["finv%d" % m] = sq.data.cpu(), sq.inv.cpu(), sf.data.cpu(), sf.inv.cpu()
        else:
            d["q%d" % m], d["f%d" % m] = q.to(dt), f2.to(dt)
    return d


def _convse_lists(inp, n_mod, dt):
    o = _ops()
    if dt == "f16s":
        q = [o.SplitRows(inp["q%d" % m], inp["qinv%d" % m]) for m in range(n_mod)]
        f = [o.SplitRows(inp["f%d" % m], inp["finv%d" % m]) for m in range(n_mod)]
    else:
        q, f = [inp["q%d" % m] for m in range(n_mod)], [inp["f%d" % m] for m in range(n_mod)]
    return q, f, [inp["mask%d" % m] for m in range(n_mod)]


def _convse(dt, n_mod, merged, softmax, ex=None, lpad=48, l_ref=37, hidden=128, ksize=5):
    """ex: None (xml_convse_rerank / _f16s) or (vid_len given, summ_out given) for xml_convse_rerank_ex."""
    nq, nv, kp = 7, 5, 3
    n_conv = 1 if merged else n_mod
    sym = "xml_convse_rerank_ex" if ex else ("xml_convse_rerank_f16s" if dt == "f16s" else "xml_convse_rerank")
    skip_unwritten = bool(softmax & 2)

    def inputs():
        return _convse_inputs(G(61), nq, nv, kp, lpad, l_ref, hidden, n_mod, n_conv, ksize, dt)

    def written(inp):
        """the elements of st / ed the header defines"""
        pv = inp["pair_vid"]
        w = torch.ones(nq, kp, lpad, dtype=torch.bool)
        if skip_unwritten:
            w &= (pv >= 0)[..., None]
        if ex and ex[0]:       # entries l >= vid_len[v] are not written; whole 16-byte pieces are: up to 3 zeros behind may be
            vl = inp["vid_len"].long()[pv.clamp_min(0).long()]
            w &= (torch.arange(lpad)[None, None] < vl[..., None]) | (pv < 0)[..., None]
        return w

    def may_be_written(inp):
        pv = inp["pair_vid"]
        vl = (inp["vid_len"].long()[pv.clamp_min(0).long()] + 3) // 4 * 4
        return (torch.arange(lpad)[None, None] < vl[..., None]) & (pv >= 0)[..., None]

    def raw(lib, A, inp):
        from tvretrieval_amd._lib import ConvseDesc
        two = n_mod == 2
        names = ["q0", "f0", "mask0"] + (["q1", "f1", "mask1"] if two else [])
        t = dict(zip(names, put_all(A, inp, names)))
        if dt == "f16s":
            inv = ["qinv0", "finv0"] + (["qinv1", "finv1"] if two else [])
            t.update(zip(inv, put_all(A, inp, inv)))
        pv, cw = put_all(A, inp, ("pair_vid", "conv_w"))
        d = ConvseDesc(nq=nq, nv=nv, kpairs=kp, lpad=lpad, l_ref=l_ref, hidden=hidden, n_mod=n_mod, merged=merged, ksize=ksize,
                       softmax=softmax, dt=_xdt(dt))
        w = written(inp)
        part = None if bool(w.all()) else w
        may = may_be_written(inp) if (ex and ex[0]) else None
        st_o = A.take("st", (nq, kp, lpad), F32, partly_written=part, may_be_written=may)
        ed_o = A.take("ed", (nq, kp, lpad), F32, partly_written=part, may_be_written=may)
        ws, nb = A.workspace(lib.xml_convse_rerank_workspace_bytes(ctypes.byref(d)))
        g = t.get
        if ex:
            vl = A.put("vid_len", inp["vid_len"]) if ex[0] else None
            pw = A.put("pair_w", inp["pair_w"])
            outs = {"st": st_o, "ed": ed_o}
            if ex[1]:      # rows of skipped pairs are not written
                outs["summ"] = A.take("summ", (nq, kp, 8), F32, partly_written=(inp["pair_vid"] >= 0)[..., None].expand(nq, kp, 8))
            st = lib.xml_convse_rerank_ex(ctypes.byref(d), P(t["q0"]), P(g("q1")), P(g("qinv0")), P(g("qinv1")), P(t["f0"]), P(g("f1")),
                                          P(g("finv0")), P(g("finv1")), P(t["mask0"]), P(g("mask1")), P(pv), P(cw), P(pw), 2, 16, P(vl),
                                          P(st_o), P(ed_o), P(outs.get("summ")), ws, nb, _st())
            return st, outs
        if dt == "f16s":
            st = lib.xml_convse_rerank_f16s(ctypes.byref(d), P(t["q0"]), P(g("q1")), P(t["qinv0"]), P(g("qinv1")), P(t["f0"]), P(g("f1")),
                                            P(t["finv0"]), P(g("finv1")), P(t["mask0"]), P(g("mask1")), P(pv), P(cw), P(st_o), P(ed_o),
                                            ws, nb, _st())
        else:
            st = lib.xml_convse_rerank(ctypes.byref(d), P(t["q0"]), P(g("q1")), P(t["f0"]), P(g("f1")), P(t["mask0"]), P(g("mask1")), P(pv),
                                       P(cw), P(st_o), P(ed_o), ws, nb, _st())
        return st, {"st": st_o, "ed": ed_o}

    def wrap(inp):
        q, f, masks = _convse_lists(inp, n_mod, dt)
        kw = {}
        if ex:
            kw = dict(pair_w=inp["pair_w"], band=(2, 16) if ex[1] else None, vid_len=inp["vid_len"] if ex[0] else None)
        r = _ops().convse_rerank(q, f, masks, inp["pair_vid"], inp["conv_w"], l_ref, merged, ksize, softmax=bool(softmax & 1),
                                 zero_skipped=not skip_unwritten, **kw)
        out = {"st": r[0], "ed": r[1]}
        if ex and ex[1]:
            out["summ"] = r[2]
        return out

    add("%s_%s_m%d_merged%d_sm%d%s_l%d" % (sym[4:], _dtn(dt), n_mod, merged, softmax, "_vl%d_summ%d" % ex if ex else "", lpad), [sym, "xml_convse_rerank_workspace_bytes"],
        "nq 7, nv 5, 3 pairs, lpad %d > l_ref %d, skipped pairs present%s" % (lpad, l_ref, ", ragged vid_len" if ex and ex[0] else ""),
        inputs, raw, wrap, nbytes=1 << 22)


for dt in (F32, BF16, "f16s"):
    _convse(dt, 2, 1, 1)
    _convse(dt, 2, 0, 0)
    _convse(dt, 1, 0, 3)                 # softmax bit 1: the rows of skipped pairs stay unwritten
    _convse(dt, 2, 1, 1, ex=(0, 1))
    _convse(dt, 2, 1, 3, ex=(1, 0))
    _convse(dt, 1, 0, 1, ex=(1, 1))
_convse(F32, 2, 1, 1, lpad=128, l_ref=100, ksize=15)
_convse(F32, 2, 1, 1, ex=(1, 1), lpad=128, l_ref=100, ksize=15)


def _span_evidence(dt, n_mod, merged):
    nq, nv, lpad, l_ref, hidden, ksize, n_pairs = 7, 5, 48, 37, 128, 5, 9
    n_conv = 1 if merged else n_mod

    def inputs():
        g = G(62)
        d = _convse_inputs(g, nq, nv, 1, lpad, l_ref, hidden, n_mod, n_conv, ksize, dt)
        d["pair_q"] = torch.tensor([0, 6, 3, 7, 2, -1, 1, 5, 4], dtype=I32)       # 7 and -1: out of range
        d["pair_v"] = torch.tensor([4, 0, 5, 1, -1, 2, 3, 3, 0], dtype=I32)       # 5 and -1: out of range
        return d

    def raw(lib, A, inp):
        from tvretrieval_amd._lib import ConvseDesc
        two = n_mod == 2
        names = ["q0", "f0", "mask0"] + (["q1", "f1", "mask1"] if two else [])
        t = dict(zip(names, put_all(A, inp, names)))
        if dt == "f16s":
            inv = ["qinv0", "finv0"] + (["qinv1", "finv1"] if two else [])
            t.update(zip(inv, put_all(A, inp, inv)))
        pq, pv, cw = put_all(A, inp, ("pair_q", "pair_v", "conv_w"))
        d = ConvseDesc(nq=nq, nv=nv, kpairs=1, lpad=lpad, l_ref=l_ref, hidden=hidden, n_mod=n_mod, merged=merged, ksize=ksize, softmax=0,
                       dt=_xdt(dt))
        outs = {nm: A.take(nm, (n_pairs, lpad), F32) for nm in (["sim0"] + (["sim1"] if two else []) + ["sim", "st", "ed"])}
        ws, nb = A.workspace(lib.xml_span_evidence_workspace_bytes(ctypes.byref(d), n_pairs))
        g = t.get
        st = lib.xml_span_evidence(ctypes.byref(d), P(t["q0"]), P(g("q1")), P(g("qinv0")), P(g("qinv1")), P(t["f0"]), P(g("f1")),
                                   P(g("finv0")), P(g("finv1")), P(t["mask0"]), P(g("mask1")), P(pq), P(pv), n_pairs, P(cw), P(outs["sim0"]),
                                   P(outs.get("sim1")), P(outs["sim"]), P(outs["st"]), P(outs["ed"]), ws, nb, _st())
        return st, outs

    def wrap(inp):
        q, f, masks = _convse_lists(inp, n_mod, dt)
        e = _ops().span_evidence(q, f, masks, inp["pair_q"], inp["pair_v"], inp["conv_w"], l_ref, merged, ksize)
        out = {"sim0": e.video_similarity, "sim": e.similarity, "st": e.st_logits, "ed": e.ed_logits}
        if n_mod == 2:
            out["sim1"] = e.sub_similarity
        return out

    add("span_evidence_%s_m%d_merged%d" % (_dtn(dt), n_mod, merged), ["xml_span_evidence", "xml_span_evidence_workspace_bytes"],
        "9 pairs, query and video indices out of range on both sides, lpad 48 > l_ref 37", inputs, raw, wrap, nbytes=1 << 22)


for dt in (F32, BF16, "f16s"):
    _span_evidence(dt, 2, 1)
    _span_evidence(dt, 1, 0)


def _moment_topk(nq, ex, kp, lpad=32, l_ref=29):
    """ex: None = xml_moment_topk; "vid_len" = xml_moment_topk_ex on ragged rows.
    moment.hip launches the 1024-thread kernel when nq <= 128 AND kpairs >= 32 (kpairs <= 128), the 256-thread one otherwise."""
    n_out, min_l, max_l = 100, 0, 8
    nv = 6
    threads = 1024 if (nq <= 128 and kp >= 32) else 256

    def inputs():
        g = G(63)
        lens = torch.tensor([29, 1, 3, 20, 29, 7], dtype=I32).clamp(max=l_ref)
        pv = torch.randint(0, nv, (nq, kp), generator=g).to(I32)
        pv[0] = 1                                              # kp pairs of a 1-clip video: kp candidates < n_out
        pv[1, 0], pv[1, 1:] = 2, -1                            # one pair of a 3-clip video, the others skipped: 6 candidates
        pv[2, kp - 1] = -1                                     # one skipped pair among valid ones
        vl = lens.long()[pv.clamp_min(0).long()] * (pv >= 0)
        valid = torch.arange(lpad)[None, None] < vl[..., None]
        st = torch.softmax(randn(g, nq, kp, lpad).masked_fill(~valid, -1e10), -1) * valid
        ed = torch.softmax(randn(g, nq, kp, lpad).masked_fill(~valid, -1e10), -1) * valid
        return {"st": st, "ed": ed, "w": torch.rand(nq, kp, generator=g) + 0.1, "pair_vid": pv, "vid_len": lens, "valid": valid}

    def raw(lib, A, inp):
        rag = ex == "vid_len"
        if rag:      # entries l >= vid_len[v] are taken as 0 WITHOUT being read: leave them as fill
            st, ed = A.take("st", (nq, kp, lpad), F32), A.take("ed", (nq, kp, lpad), F32)
            v = inp["valid"].to(st.device)
            st[v], ed[v] = inp["st"].to(st.device)[v], inp["ed"].to(st.device)[v]
        else:
            st, ed = put_all(A, inp, ("st", "ed"))
        w = A.put("w", inp["w"])
        sc, fl = A.take("score", (nq, n_out), F32), A.take("flat", (nq, n_out), I32)
        if ex is None:
            return lib.xml_moment_topk(P(st), P(ed), P(w), P(sc), P(fl), nq, kp, lpad, l_ref, min_l, max_l, n_out, _st()), \
                {"score": sc, "flat": fl}
        pv, vl = put_all(A, inp, ("pair_vid", "vid_len")) if rag else (None, None)
        return lib.xml_moment_topk_ex(P(st), P(ed), P(w), None, P(pv), P(vl), P(sc), P(fl), nq, kp, lpad, l_ref, min_l, max_l, n_out,
                                      _st()), {"score": sc, "flat": fl}

    def wrap(inp):
        kw = dict(pair_vid=inp["pair_vid"], vid_len=inp["vid_len"]) if ex == "vid_len" else {}
        sc, fl = _ops().moment_topk(inp["st"], inp["ed"], inp["w"], l_ref, min_l, max_l, n_out, **kw)
        return {"score": sc, "flat": fl}

    few = ("rows with %d and 6 candidates and a skipped pair" % kp if ex else
           ("every row has %d candidates < n_out" % (kp * sum(min(max_l, l_ref - i) for i in range(l_ref))) if l_ref < 4
            else "full rows"))
    add("moment_topk%s_nq%d_kp%d_lref%d" % ("" if ex is None else "_ex_" + ex, nq, kp, l_ref),
        ["xml_moment_topk" if ex is None else "xml_moment_topk_ex"],
        "nq = %d, kpairs = %d: the %d-thread kernel; n_out = 100, %s; lpad %d > l_ref %d" % (nq, kp, threads, few, lpad, l_ref),
        inputs, raw, wrap, nbytes=1 << 23)


for nq, kp in ((128, 32), (129, 32), (128, 2)):      # 1024 threads; 256 threads by nq; 256 threads by kpairs
    _moment_topk(nq, None, kp)
    _moment_topk(nq, "vid_len", kp)
_moment_topk(128, None, 32, lpad=16, l_ref=2)        # 1024 threads, 32 x 3 = 96 candidates per row: fewer than n_out
_moment_topk(128, None, 128, lpad=16, l_ref=2)       # the largest kpairs the entry takes (4 * MT_PPW)


def _moments_decode(skew, parts, vr):
    nq, n, k, l_ref = 5, 37, 4, 29
    ld_in, ld_out = n + 3, n + 2

    def inputs():
        g = G(64)
        flat = torch.randint(0, k * l_ref * l_ref, (nq, n), generator=g).to(I32)
        flat[0] = -1                                          # a row of 0 candidates; every other row has all n
        flat[1, 30:] = -1
        return {"flat": flat, "score": torch.rand(nq, n, generator=g), "top_idx": torch.randint(0, 50, (nq, n if vr else k), generator=g).to(I32),
                "meta2vid": torch.randperm(1000, generator=g)[:50].to(I32), "part_offset": torch.randint(0, 200, (50,), generator=g).to(I32)}

    def raw(lib, A, inp):
        score = A.put("score", inp["score"], ld=ld_in, skew=skew)
        flat = None if vr else A.put("flat", inp["flat"], ld=ld_in, skew=skew)
        top = A.put("top_idx", inp["top_idx"], ld=ld_in, skew=skew) if vr else A.put("top_idx", inp["top_idx"])
        m2v = A.put("meta2vid", inp["meta2vid"])
        out2 = A.take("rec", (nq, n * 4), I32, ld=ld_out * 4)   # n records of 16 bytes per row, row stride ld_out records
        cnt = A.take("count", (nq,), I32)
        if parts:
            po = A.put("part_offset", inp["part_offset"])
            st = lib.xml_moments_decode_parts(P(flat), P(score), P(top), None, P(m2v), P(po), nq, n, ld_in, 0 if vr else k, l_ref, 1.5, 1,
                                              P(out2), ld_out, P(cnt), _st())
        else:
            st = lib.xml_moments_decode(P(flat), P(score), P(top), None, P(m2v), nq, n, ld_in, 0 if vr else k, l_ref, 1.5, 1, P(out2),
                                        ld_out, P(cnt), _st())
        return st, {"rec": out2, "count": cnt}

    def wrap(inp):
        rec, cnt = _ops().moments_decode(inp["score"], None if vr else inp["flat"], inp["top_idx"], None, inp["meta2vid"], l_ref, 1.5, True,
                                         part_offset=inp["part_offset"] if parts else None)
        return {"rec": rec.view(nq, n * 4), "count": cnt}

    add("moments_decode%s%s_skew%d" % ("_parts" if parts else "", "_vr" if vr else "", skew),
        ["xml_moments_decode_parts" if parts else "xml_moments_decode"],
        "n = 37 records per row, ld_in = n + 3, ld_out = n + 2 records; rows with 0, 30 and n candidates; flat / score %d bytes past a line" % skew,
        inputs, raw, wrap)


for parts in (0, 1):
    _moments_decode(0, parts, 0)
    _moments_decode(4, parts, 0)
_moments_decode(0, 0, 1)


def _records(g, nq, n, n_vid):
    rec = torch.zeros(nq, n, 4, dtype=I32)
    rec[..., 0] = torch.randint(0, n_vid, (nq, n), generator=g).to(I32)
    st = torch.randint(0, 40, (nq, n), generator=g).float() * 1.5
    rec[..., 1] = st.view(I32)
    rec[..., 2] = (st + torch.randint(1, 9, (nq, n), generator=g).float() * 1.5).view(I32)
    rec[..., 3] = torch.rand(nq, n, generator=g).sort(dim=1, descending=True).values.view(I32)
    return rec


def _nms_moments(by_video):
    nq, n, max_after = 4, 37, 20
    ld_in, ld_out, ld_index = n + 3, max_after + 2, max_after + 3

    def inputs():
        g = G(65)
        return {"rec": _records(g, nq, n, 3).view(nq, n * 4), "count": torch.tensor([0, n, 11, 50], dtype=I32)}

    def raw(lib, A, inp):
        rec = A.put("rec", inp["rec"], ld=ld_in * 4)
        cnt = A.put("count", inp["count"])
        out = A.take("out", (nq, max_after * 4), I32, ld=ld_out * 4)
        oi, oc = A.take("out_index", (nq, max_after), I32, ld=ld_index), A.take("out_count", (nq,), I32)
        st = lib.xml_nms_moments(P(rec), ld_in, P(cnt), nq, n, by_video, 0.5, 1.0, n, max_after, P(out), ld_out, P(oi), ld_index, P(oc), _st())
        return st, {"out": out, "out_index": oi, "out_count": oc}

    def wrap(inp):
        o, i, c = _ops().nms_moments(inp["rec"].view(nq, n, 4), inp["count"], bool(by_video), 0.5, 1.0, None, max_after)
        return {"out": o.view(nq, max_after * 4), "out_index": i, "out_count": c}

    add("nms_moments_by_video%d" % by_video, ["xml_nms_moments"],
        "n = 37, max_after = 20; ld_in, ld_out and ld_index larger than the rows; counts 0, n, 11 and one above n", inputs, raw, wrap)


_nms_moments(0)
_nms_moments(1)


class _GT(object):
    pass


def _eval_moments(task):
    nq, n, n_ts = 5, 37, 4
    ld = n + 3
    tasks = {"VCMR": 0, "SVMR": 1, "VR": 2}
    n_thd = 1 if task == "VR" else 2
    topks = (1, 5, 10, 100)

    def inputs():
        g = G(66)
        ts = torch.rand(nq, n_ts, 2, generator=g).sort(dim=2).values * 60
        return {"rec": _records(g, nq, n, 3).view(nq, n * 4), "count": torch.tensor([0, n, 11, 50, 3], dtype=I32),
                "gt_vid": torch.tensor([0, 1, 2, 0, 1], dtype=I32), "gt_ts": ts, "n_gt": torch.tensor([1, 1, 0, 4, 1], dtype=I32),
                "desc_type": torch.tensor([0, 1, 2, 0, 1], dtype=I32)}

    def raw(lib, A, inp):
        rec = A.put("rec", inp["rec"], ld=ld * 4)
        cnt, gv, gts, ng, dty = put_all(A, inp, ("count", "gt_vid", "gt_ts", "n_gt", "desc_type"))
        fh, hits, rows = A.take("first_hit", (nq, n_thd), I32), A.take("hits", (4, n_thd, len(topks)), I32), A.take("rows", (4,), I32)
        thd = (ctypes.c_float * 2)(0.5, 0.7)
        ks = (ctypes.c_int32 * 4)(*topks)
        st = lib.xml_eval_moments(P(rec), ld, P(cnt), nq, n, tasks[task], 1.0, 100, P(gv), P(gts), n_ts, P(ng), P(dty),
                                  ctypes.cast(thd, ctypes.c_void_p), n_thd, ctypes.cast(ks, ctypes.c_void_p), 4, P(fh), P(hits), P(rows),
                                  _st())
        return st, {"first_hit": fh, "hits": hits, "rows": rows}

    def wrap(inp):
        gt = _GT()
        gt.gt_vid, gt.gt_ts, gt.n_gt, gt.desc_type = inp["gt_vid"], inp["gt_ts"], inp["n_gt"], inp["desc_type"]
        fh, hits, rows = _ops().eval_moments(inp["rec"].view(nq, n, 4), inp["count"], task, gt, 1.0, 100, (0.5, 0.7), topks)
        return {"first_hit": fh, "hits": hits, "rows": rows}

    add("eval_moments_%s" % task.lower(), ["xml_eval_moments"],
        "n = 37, ld_rec = n + 3 records; counts 0, n, 11, one above n; a row without ground truth and a 4-span row", inputs, raw, wrap)


for task in ("VCMR", "SVMR", "VR"):
    _eval_moments(task)


# =====================================================================================================================
# 7. training entries that take scratch or a leading dimension
# =====================================================================================================================
def _transpose_batched(dt):
    batch, rows, cols = 3, 37, 21
    ld_out = 40

    def inputs():
        return {"x": randn(G(70), batch, rows, cols, dtype=dt)}

    def raw(lib, A, inp):
        x = A.put("x", inp["x"])
        y = A.take("y", (batch, cols, rows), dt, ld=ld_out)          # columns beyond `rows` are not written: row gaps here
        return lib.xml_transpose_batched(P(x), P(y), batch, rows, cols, ld_out, XDT[dt], _st()), {"y": y}

    add("transpose_batched_%s" % DTN[dt], ["xml_transpose_batched"], "37 x 21 matrices: ragged 32 x 32 tiles both ways; ld_out = 40 > rows",
        inputs, raw, lambda inp: {"y": _tops().transpose(inp["x"], ld_out)[..., :rows]})


def _heads(dt):
    n, l, hidden, heads = 3, 13, 128, 4               # L = 13 is no multiple of 8: l8 = 16
    l8, dh = 16, 32
    ld, col0 = 3 * hidden, hidden

    def inputs():
        g = G(71)
        return {"x": randn(g, n, l, ld, dtype=dt), "xh": randn(g, n * heads, l8, dh, dtype=dt)}

    def raw_split(lib, A, inp):
        x = A.put("x", inp["x"])
        dst, dst_t = A.take("dst", (n * heads, l8, dh), dt), A.take("dst_t", (n * heads, dh, l8), dt)
        st = lib.xml_split_heads(P(x), ld, col0, n, l, l8, heads, dh, P(dst), P(dst_t), XDT[dt], _st())
        return st, {"dst": dst, "dst_t": dst_t}

    def wrap_split(inp):
        d, t = _tops().split_heads(inp["x"], heads, True, True, col0, hidden)
        return {"dst": d, "dst_t": t}

    add("split_heads_%s" % DTN[dt], ["xml_split_heads"], "col0 = H of ld = 3 H; L = 13 -> l8 = 16: three padding rows per head", inputs,
        raw_split, wrap_split)

    def raw_merge(lib, A, inp):
        xh = A.put("xh", inp["xh"])
        # the columns [col0, col0 + H) of an (n, l, 3 H) tensor: a region of H columns with the row stride 3 H
        out = A.take("out", (n, l, hidden), dt, ld=ld)
        st = lib.xml_merge_heads(P(xh), ctypes.c_void_p(out.data_ptr() - col0 * out.element_size()), ld, col0, n, l, l8, heads, dh, XDT[dt],
                                 _st())
        return st, {"out": out}

    def wrap_merge(inp):
        out = torch.zeros(n, l, ld, dtype=dt, device=inp["xh"].device)
        _tops().merge_heads(inp["xh"], n, l, heads, out=out, col0=col0)
        return {"out": out[..., col0:col0 + hidden]}

    add("merge_heads_%s" % DTN[dt], ["xml_merge_heads"], "into the columns [H, 2 H) of rows of 3 H: the other columns are guard bytes",
        inputs, raw_merge, wrap_merge)


for dt in (F32, BF16):
    _transpose_batched(dt)
    _heads(dt)


def _q2c_scores_arg(dt, l, skew):
    nq, nv, hidden = 70, 5, 128
    ld_out, ld_arg = nv + 3, nv + 5

    def inputs():
        return _k6_operands(G(73), nq, nv, l, hidden, dt, 2)

    def raw(lib, A, inp):
        q0, c0, m0, q1, c1, m1 = put_all(A, inp, ("qn0", "cn0", "mask0", "qn1", "cn1", "mask1"))
        out = A.take("out", (nq, nv), F32, ld=ld_out, skew=skew)
        arg0, arg1 = A.take("arg0", (nq, nv), I32, ld=ld_arg, skew=skew), A.take("arg1", (nq, nv), I32, ld=ld_arg, skew=skew)
        st = [lib.xml_q2c_scores_arg(P(q0), P(c0), P(m0), P(out), ld_out, P(arg0), ld_arg, nq, nv, l, hidden, 0, XDT[dt], _st()),
              lib.xml_q2c_scores_arg(P(q1), P(c1), P(m1), P(out), ld_out, P(arg1), ld_arg, nq, nv, l, hidden, 1, XDT[dt], _st())]
        return st, {"out": out, "arg0": arg0, "arg1": arg1}

    def wrap(inp):
        out, a0 = _tops().q2c_scores_arg(inp["qn0"], inp["cn0"], inp["mask0"])
        out, a1 = _tops().q2c_scores_arg(inp["qn1"], inp["cn1"], inp["mask1"], out=out, combine=True)
        return {"out": out, "arg0": a0, "arg1": a1}

    add("q2c_scores_arg_%s_l%d_skew%d" % (DTN[dt], l, skew), ["xml_q2c_scores_arg"],
        "nq = 70, nv = 5, unpadded l = %d, ld_out = nv + 3, ld_arg = nv + 5" % l, inputs, raw, wrap, nbytes=1 << 23)


for dt in (F32, BF16):
    _q2c_scores_arg(dt, 37, 0)
    _q2c_scores_arg(dt, 128, 4)


def _gemm_batched(dt, batch, m, n, k, out_f32, atomic):
    odt = F32 if (out_f32 or dt is F32) else dt

    def inputs():
        g = G(74)
        return {"a": randn(g, batch, m, k, dtype=dt), "b": randn(g, batch, n, k, dtype=dt)}

    def raw(lib, A, inp):
        a, b = put_all(A, inp, ("a", "b"))
        out = A.take("out", (batch, m, n), odt)
        return lib.xml_gemm_batched(P(a), P(b), P(out), batch, m, n, k, 0.5, out_f32, XDT[dt], _st()), {"out": out}

    # split-K adds with f32 atomics: tests/test_gpu_train.py:727 compares this path within 2e-5 of max|ref|
    add("gemm_batched_%s_b%d_m%d_n%d_k%d%s" % (DTN[dt], batch, m, n, k, "_f32out" if out_f32 else ""), ["xml_gemm_batched"],
        "M = %d, N = %d: one ragged 128 x 128 tile per matrix; %s" % (m, n, "K >= 1024 with one matrix: the split-K path" if atomic
                                                                      else "K = %d: a K tail" % k),
        inputs, raw, lambda inp: {"out": _tops().gemm_batched(inp["a"], inp["b"], 0.5, bool(out_f32))}, atomic=atomic)


_gemm_batched(F32, 3, 37, 21, 36, 0, None)
_gemm_batched(BF16, 3, 37, 21, 40, 0, None)
_gemm_batched(BF16, 3, 37, 21, 40, 1, None)
_gemm_batched(BF16, 1, 37, 21, 1032, 1, 2e-5)
_gemm_batched(F32, 1, 37, 21, 1028, 0, 2e-5)


def _gemm_tn(rows):
    n, k = 40, 72

    def inputs():
        g = G(75)
        return {"a": randn(g, rows, n, dtype=BF16), "b": randn(g, rows, k, dtype=BF16)}

    def raw(lib, A, inp):
        a, b = put_all(A, inp, ("a", "b"))
        assert lib.xml_gemm_tn_supported(rows, n, k, XML_BF16) == 1
        out, cs = A.take("out", (n, k), F32), A.take("colsum", (n,), F32)
        return lib.xml_gemm_tn(P(a), P(b), P(out), P(cs), rows, n, k, XML_BF16, 0, _st()), {"out": out, "colsum": cs}

    def wrap(inp):
        out, cs = _tops().gemm_tn(inp["a"], inp["b"], colsum=True)
        return {"out": out, "colsum": cs}

    # row ranges are combined with f32 atomics: tests/test_gpu_train.py:722-727 compares within 2e-5 of max|ref|
    add("gemm_tn_r%d" % rows, ["xml_gemm_tn"], "rows = %d, N = 40, K = 72: ragged row range, ragged 128 x 128 output tile; out and the "
        "column sums are separate regions" % rows, inputs, raw, wrap, atomic=2e-5)


_gemm_tn(37)
_gemm_tn(300)


def _clip_grad_norm():
    n = 1024 + 37                      # two blocks of partial sums: a + b is the same in either order, so the bits are stable

    def inputs():
        return {"g": randn(G(76), n, scale=0.1)}

    def raw(lib, A, inp):
        g = A.take("g", (n,), F32)
        g.copy_(inp["g"])              # clipped in place
        ws, nb = A.workspace(4)
        return lib.xml_clip_grad_norm(P(g), n, 1.0, ws, _st()), {"g": g}

    def wrap(inp):
        return {"g": _tops().clip_grad_norm(inp["g"].clone(), 1.0)}

    add("clip_grad_norm_n1061", ["xml_clip_grad_norm"], "n = 1024 + 37: a ragged second block; 4 bytes of scratch", inputs, raw, wrap)


_clip_grad_norm()


def _attention_train(skew, p_drop):
    n, l, hidden, heads = 2, 13, 128, 4              # L = 13: no multiple of 8; dh = 32
    ld = 3 * hidden

    def inputs():
        g = G(77)
        return {"qkv": randn(g, n, l, ld, dtype=BF16), "dout": randn(g, n, l, hidden, dtype=BF16), "k_mask": prefix_mask([l, 5], l)}

    def raw(lib, A, inp):
        assert lib.xml_attention_train_supported(l, l, hidden, heads, XML_BF16) == 1
        qkv = A.put("qkv", inp["qkv"], skew=skew)
        dout, km = A.put("dout", inp["dout"], skew=skew), A.put("k_mask", inp["k_mask"])
        out = A.take("out", (n, l, hidden), BF16, skew=skew)
        dqkv = A.take("dqkv", (n, l, ld), BF16, skew=skew)          # dq / dk / dv: the three column blocks of ONE gradient tensor
        h2 = hidden * 2
        st = [lib.xml_attention_train_fwd(P(qkv), ld, P(qkv, h2), ld, P(qkv, 2 * h2), ld, None, P(km), P(out), hidden, n, l, l, hidden,
                                          heads, p_drop, 1234, None, XML_BF16, _st()),
              lib.xml_attention_train_bwd(P(qkv), ld, P(qkv, h2), ld, P(qkv, 2 * h2), ld, None, P(km), P(dout), hidden, P(dqkv), ld,
                                          P(dqkv, h2), ld, P(dqkv, 2 * h2), ld, n, l, l, hidden, heads, p_drop, 1234, None, XML_BF16,
                                          _st())]
        return st, {"out": out, "dqkv": dqkv}

    def wrap(inp):
        T = _tops()
        qkv = inp["qkv"]
        out = T.attention_train_fwd(qkv, qkv, qkv, None, inp["k_mask"], heads, hidden, p_drop, 1234, 0, hidden, 2 * hidden)
        dqkv = torch.empty_like(qkv)
        T.attention_train_bwd(qkv, qkv, qkv, None, inp["k_mask"], inp["dout"], dqkv, dqkv, dqkv, heads, hidden, p_drop, 1234, 0, hidden,
                              2 * hidden, 0, hidden, 2 * hidden)
        return {"out": out, "dqkv": dqkv}

    add("attention_train_p%d_skew%d" % (round(p_drop * 100), skew), ["xml_attention_train_fwd", "xml_attention_train_bwd"],
        "L = 13, q / k / v and dq / dk / dv as offset pointers into one (n, L, 3 H) tensor each; base %d bytes past a line" % skew,
        inputs, raw, wrap)


_attention_train(0, 0.0)
_attention_train(16, 0.0)
_attention_train(0, 0.2)


# ---- in-place index updates ---------------------------------------------------------------------------------------------------
INDEX_CAP = 37                                        # two live words; slots 3, 5 and 31 share word 0, slot 36 sits in word 1


def _index_state(g, cap, lpad, hidden, dt, tiled, lib_bytes):
    """A populated index of `cap` slots (arbitrary previous occupants) as CPU tensors."""
    d = {"vlen": torch.randint(1, lpad + 1, (cap,), generator=g).to(I32), "slot_ids": torch.randint(0, 10 ** 6, (cap,), generator=g).to(I32),
         "live": torch.tensor([0x0F0F00F1, 0x00000001], dtype=I64).to(I32)}
    for m in "ab":
        n_k6 = lib_bytes // (2 if dt is BF16 else 4) if tiled else cap * lpad * hidden
        d["k6_" + m] = randn(g, n_k6, dtype=dt) if tiled else randn(g, cap, lpad, hidden, dtype=dt)
        d["feat2_" + m] = randn(g, cap, lpad, hidden, dtype=dt)
        d["imask_" + m] = (torch.rand(cap, lpad, generator=g) < 0.5).float()
        d["bits_" + m] = _allow_words(g, cap, 4)
    return d


STATE = ("k6_a", "feat2_a", "imask_a", "bits_a", "k6_b", "feat2_b", "imask_b", "bits_b", "vlen", "slot_ids", "live")


def _take_state(A, inp, names):
    out = {}
    for nm in names:                                   # in-out operands: the caller's contents, rewritten in place
        v = A.take(nm, inp[nm].shape, inp[nm].dtype)
        v.copy_(inp[nm])
        out[nm] = v
    return out


def _index_put(dt, hidden, tiled):
    cap, b, lb = INDEX_CAP, 4, 21
    lpad = 128 if tiled else 48
    l_ref = lpad - 3

    def inputs():
        from tvretrieval_amd import _lib
        g = G(78)
        nb = int(_lib.load().xml_q2c_tiled_bytes(cap * 128, hidden, XDT[dt])) if tiled else 0
        d = _index_state(g, cap, lpad, hidden, dt, tiled, nb)
        for m, lens in (("a", [21, 1, 9, 21]), ("b", [20, 3, 9, 1])):
            d["f1_" + m], d["f2_" + m] = randn(g, b, lb, hidden, dtype=dt), randn(g, b, lb, hidden, dtype=dt)
            d["mask_" + m] = prefix_mask(lens, lb)
        d["slots"], d["ids"] = torch.tensor([3, 36, 5, 31], dtype=I32), torch.tensor([900, 901, 902, 903], dtype=I32)
        return d

    def raw(lib, A, inp):
        f1a, f2a, ma, f1b, f2b, mb, slots, ids = put_all(A, inp, ("f1_a", "f2_a", "mask_a", "f1_b", "f2_b", "mask_b", "slots", "ids"))
        s = _take_state(A, inp, STATE)
        st = lib.xml_index_put_rows(2, P(f1a), P(f2a), P(ma), P(f1b), P(f2b), P(mb), P(slots), P(ids), b, lb, P(s["k6_a"]),
                                    P(s["feat2_a"]), P(s["imask_a"]), P(s["bits_a"]), P(s["k6_b"]), P(s["feat2_b"]), P(s["imask_b"]),
                                    P(s["bits_b"]), P(s["vlen"]), P(s["slot_ids"]), P(s["live"]), cap, lpad, l_ref, hidden, XDT[dt],
                                    int(tiled), _st())
        return st, s

    def wrap(inp):
        o = _ops()
        s = {nm: inp[nm].clone() for nm in STATE}
        k6 = [o.TiledRows(s["k6_" + m], cap * 128, hidden, (cap, 128, hidden)) if tiled else s["k6_" + m] for m in "ab"]
        o.index_put_rows([inp["f1_a"], inp["f1_b"]], [inp["f2_a"], inp["f2_b"]], [inp["mask_a"], inp["mask_b"]], inp["slots"], inp["ids"],
                         k6, [s["feat2_a"], s["feat2_b"]], [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]], s["vlen"],
                         s["slot_ids"], s["live"], l_ref)
        return s

    add("index_put_rows_%s_h%d_%s" % (DTN[dt], hidden, "tiled" if tiled else "rowmajor"), ["xml_index_put_rows"],
        "capacity 37 (18.5 tiles), slots 3, 5, 31 share a live word, slot 36 is the last; lb = 21 < lpad = %d" % lpad, inputs, raw, wrap,
        nbytes=1 << 25)


def _index_clear():
    cap, lpad = INDEX_CAP, 48
    names = ("imask_a", "bits_a", "imask_b", "bits_b", "vlen", "live")

    def inputs():
        d = _index_state(G(79), cap, lpad, 8, F32, False, 0)
        d["live"] = torch.tensor([-1, 0x1F], dtype=I32)
        d["slots"] = torch.tensor([3, 36, 31], dtype=I32)
        return d

    def raw(lib, A, inp):
        slots = A.put("slots", inp["slots"])
        s = _take_state(A, inp, names)
        st = lib.xml_index_clear_rows(2, P(slots), 3, P(s["imask_a"]), P(s["bits_a"]), P(s["imask_b"]), P(s["bits_b"]), P(s["vlen"]),
                                      P(s["live"]), cap, lpad, lpad - 3, _st())
        return st, s

    def wrap(inp):
        s = {nm: inp[nm].clone() for nm in names}
        _ops().index_clear_rows(inp["slots"], [s["imask_a"], s["imask_b"]], [s["bits_a"], s["bits_b"]], s["vlen"], s["live"], lpad - 3)
        return s

    add("index_clear_rows", ["xml_index_clear_rows"], "capacity 37: slots 3 and 31 share a live word, slot 36 is the last slot", inputs,
        raw, wrap)


_index_put(F32, 128, True)
_index_put(BF16, 256, True)
_index_put(F32, 128, False)
_index_put(BF16, 128, False)
_index_clear()


def _zeroed(A, name, shape, dtype=F32):
    v = A.take(name, shape, dtype)
    v.zero_()                                              # a gradient sink: the entry ADDS to what the caller put there
    return v


def _layernorm_bwd():
    rows, d = 37, 3072

    def inputs():
        g = G(80)
        return {"a": randn(g, rows, d) * 2 + 0.3, "g": randn(g, d, scale=0.2) + 1.0, "dy": randn(g, rows, d)}

    def raw(lib, A, inp):
        a, gg, dy = put_all(A, inp, ("a", "g", "dy"))
        dx, dg, db = A.take("dx", (rows, d), F32), _zeroed(A, "dg", (d,)), _zeroed(A, "dbeta", (d,))
        ws, nb = A.workspace(rows * 16)
        st = lib.xml_layernorm_bwd(P(a), XML_F32, None, P(gg), P(dy), P(dx), P(dg), P(db), rows, d, XML_F32, ws, nb, _st())
        return st, {"dx": dx, "dg": dg, "dbeta": db}

    def wrap(inp):
        dx, dg, db = _tops().layernorm_bwd(inp["a"], None, inp["g"], inp["dy"], need_dx=True)
        return {"dx": dx, "dg": dg, "dbeta": db}

    # dgamma / dbeta are summed with atomics below 1024 rows: tests/test_gpu_train.py:121-122 compares them within 2e-5 of max|ref|
    add("layernorm_bwd_d3072_r37", ["xml_layernorm_bwd"], "d = 3072 > 1024: the two-kernel path with ws = rows * 16 bytes, 37 rows", inputs,
        raw, wrap, nbytes=1 << 22, atomic=2e-5)


def _layernorm_bwd_drop_ws(rows):
    d = 3072

    def inputs():
        g = G(81)
        return {"a": randn(g, rows, d) * 2 + 0.3, "g": randn(g, d, scale=0.2) + 1.0, "dy": randn(g, rows, d, dtype=BF16)}

    def raw(lib, A, inp):
        a, gg, dy = put_all(A, inp, ("a", "g", "dy"))
        dg, db = _zeroed(A, "dg", (d,)), _zeroed(A, "dbeta", (d,))
        ws, nb = A.workspace(lib.xml_layernorm_bwd_partials_bytes(rows, d))
        st = lib.xml_layernorm_bwd_drop_ws(P(a), XML_F32, None, P(gg), P(dy), None, None, P(dg), P(db), rows, d, XML_BF16, 0.0, 0, 0.1, 99,
                                           None, ws, nb, _st())
        return st, {"dg": dg, "dbeta": db}

    def wrap(inp):
        r = _tops().layernorm_bwd_drop(inp["a"], None, inp["g"], inp["dy"], 0.0, 0, 0.1, 99, need_dx=False)
        return {"dg": r[2], "dbeta": r[3]}

    # per-workgroup partials or atomics, by the row count: tests/test_gpu_train.py:117-118 compares within 2e-5 of max|ref|
    add("layernorm_bwd_drop_ws_d3072_r%d" % rows, ["xml_layernorm_bwd_drop_ws"],
        "d = 3072, %d rows, ws = xml_layernorm_bwd_partials_bytes exactly" % rows, inputs, raw, wrap, nbytes=1 << 25, atomic=2e-5)


def _bert_adam_step(total):
    n_seg = 3                                              # total is no multiple of XML_ADAM_NORM_BLOCK: 3 floats of norm scratch
    state = ("p", "g", "m", "v")

    def inputs():
        g = G(82)
        return {"p": randn(g, total), "g": randn(g, total, scale=0.5), "m": randn(g, total, scale=0.1), "v": torch.rand(total, generator=g) * 0.01,
                "seg_off": torch.tensor([0, 1000, 1030, total], dtype=I64), "seg_lr": torch.tensor([1e-3, 2e-3, 1e-3]),
                "seg_wd": torch.tensor([0.01, 0.0, 0.01])}

    def raw(lib, A, inp):
        so, lr, wd = put_all(A, inp, ("seg_off", "seg_lr", "seg_wd"))
        s = _take_state(A, inp, state)
        norms = A.take("norms", (n_seg,), F32)
        nws = A.take("norm_ws", ((total + 1023) // 1024,), F32)          # scratch: ceil(total / XML_ADAM_NORM_BLOCK) floats
        st = lib.xml_bert_adam_step(P(s["p"]), P(s["g"]), P(s["m"]), P(s["v"]), P(so), P(lr), P(wd), n_seg, total, 0.5, 0.9, 0.999, 1e-6, 1.0,
                                    P(norms), None, None, P(nws), _st())
        s["norms"] = norms
        return st, s

    def wrap(inp):
        s = {nm: inp[nm].clone() for nm in state}
        s["norms"] = torch.empty(n_seg, device=inp["p"].device)
        nws = torch.empty((total + 1023) // 1024, device=inp["p"].device)
        _tops().bert_adam_step(s["p"], s["g"], s["m"], s["v"], inp["seg_off"], inp["seg_lr"], inp["seg_wd"], s["norms"], 0.5, 0.9, 0.999, 1e-6,
                               1.0, norm_ws=nws)
        return s

    # blocks that hold a tensor boundary add their sums of squares with atomics (and all of them when total % 4 != 0): order
    # dependent in the last bit; tests/test_gpu_train.py:408-409 compares parameters and clipped gradients within 2e-6 of max|ref|
    add("bert_adam_step_total%d" % total, ["xml_bert_adam_step"],
        "total = %d, tensors [0, 1000), [1000, 1030), [1030, total), ceil(total / 1024) = 3 floats of norm scratch: %s" % (
            total, "block 0 holds both boundaries (atomics), blocks 1 and 2 lie inside the last tensor: their partials, the ragged last "
            "block's included, are written to norm_ws and read back in a fixed order" if total % 4 == 0 else
            "total % 4 != 0, so no block takes the vector loads: every sum goes through the atomics and norm_ws is only zeroed"),
        inputs, raw, wrap, atomic=2e-6)


_layernorm_bwd()
_layernorm_bwd_drop_ws(37)
_layernorm_bwd_drop_ws(1100)
_bert_adam_step(2084)
_bert_adam_step(2085)


# =====================================================================================================================
# exemptions
# =====================================================================================================================
_PRED = "pure predicate / size function: no device memory; called by the cases of the entry it belongs to or on the CPU"
_TRAIN = "training entry without scratch or leading dimension: out of scope of the guard-band cases (issue section 7)"
EXEMPT = {
    "xml_abi_version": "introspection", "xml_build_arch": "introspection", "xml_status_string": "introspection",
    "xml_nms_vcmr_host": "host-memory entry", "xml_nms_svmr_host": "host-memory entry",
    "xml_nms_vcmr_batched_host": "host-memory entry", "xml_nms_svmr_batched_host": "host-memory entry",
    "xml_q2c_tile_rows_l2norm_ok": _PRED, "xml_gemm_tn_supported": _PRED,
    "xml_attention_train_supported": _PRED, "xml_q2c_scores_l2norm_bwd_supported": _PRED,
    "xml_layernorm_bwd_partials_bytes": _PRED,
    "xml_colsum": _TRAIN, "xml_relu_bwd": _TRAIN, "xml_add_inplace": _TRAIN, "xml_attn_softmax": _TRAIN,
    "xml_modular_pool_bwd": _TRAIN, "xml_l2norm_bwd": _TRAIN, "xml_pair_sim": _TRAIN, "xml_pair_sim_bwd": _TRAIN,
    "xml_span_loss": _TRAIN, "xml_rank_loss": _TRAIN, "xml_dropout": _TRAIN, "xml_q2c_scores_l2norm_bwd": _TRAIN,
    "xml_q2c_scores_l2norm_bwd_multi": _TRAIN, "xml_loss_combine": _TRAIN, "xml_loss_combine_bwd": _TRAIN,
    "xml_transpose_segments": _TRAIN, "xml_add_layernorm_drop": _TRAIN, "xml_layernorm_bwd_drop": _TRAIN,
    "xml_q2c_scores_bwd": _TRAIN,
}
for _s in ("xml_rccl_available", "xml_rccl_unique_id", "xml_rccl_comm_init", "xml_rccl_comm_destroy", "xml_rccl_allgather",
           "xml_rccl_allreduce_avg_f32", "xml_rccl_allgather_topk_workspace_bytes", "xml_rccl_allgather_topk",
           "xml_rccl_topk_by_owner_workspace_bytes", "xml_rccl_topk_by_owner"):
    EXEMPT[_s] = "xml_rccl_*: needs a communicator; tests/test_gpu_dist.py"
for _s in ("xml_dispatch_const", "xml_dispatch_gemm", "xml_dispatch_gemm_rules", "xml_dispatch_gemm_kloop", "xml_dispatch_q2c",
           "xml_dispatch_q2c_fused", "xml_dispatch_q2c_walk", "xml_dispatch_attention", "xml_dispatch_l2norm"):
    EXEMPT[_s] = "dispatch introspection: integers in, an enum out, no memory; tests/test_reduction_width_plan.py"
for _s in ("xml_dispatch_convse_shape", "xml_dispatch_convse_pairs"):
    EXEMPT[_s] = "dispatch introspection: integers in, an enum out, no memory; tests/test_convse_cases_reference.py"


# =====================================================================================================================
# the tests
# =====================================================================================================================
@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    return _lib.load()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_abi_arena(lib, case):
    try:
        run_case(case, lib, DEV)
    except RuntimeError as e:      # a HIP error is sticky: nothing that runs after it on this card means anything
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit("GPU fault in guard-band case %s: %s" % (case.name, str(e).splitlines()[0]), returncode=3)
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("ksize", [1, 5, 15])
@pytest.mark.parametrize("l", [1, 37, 128])
def test_conv1d_rows_vs_float64(ksize, l):
    """xml_conv1d_rows against F.conv1d in float64; the allowance is that of the one-pass row kernels (C_ROWWISE of
    tests/test_gpu_numerics.py) over the float32 F.conv1d's own error, as numerics_regimes.check_f32 computes it."""
    import numerics_regimes as NR
    from test_gpu_numerics import C_ROWWISE
    g = G(100 + ksize + l)
    x, w = randn(g, 40, l), randn(g, ksize)
    got = _ops().conv1d_rows(x.to(DEV), w.to(DEV))
    W = F.conv1d(x.double()[:, None], w.double()[None, None], padding=ksize // 2)[:, 0]
    R = F.conv1d(x[:, None], w[None, None], padding=ksize // 2)[:, 0]
    NR.check_f32("conv1d_rows", "k%d_l%d" % (ksize, l), got, W, R, C_ROWWISE)
