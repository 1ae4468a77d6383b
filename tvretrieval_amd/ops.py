"""Thin tensor-level wrappers over the C ABI (include/xmlhip.h).

PyTorch is plumbing here: it owns device memory (torch.empty), the current HIP stream and nothing else.
Every function launches hand-written gfx950 kernels from libxmlhip.so and fails loudly when the library or a
GPU tensor is missing -- there is no eager/CPU fallback.
"""
import collections
import ctypes
import types

import numpy as np

import torch

from . import _lib
from ._lib import XML_BF16, XML_F32, ConvseDesc, check

class _SplitF16(object):
    """dtype tag of the split-f16 forms (XML_F16S, include/xmlhip.h): f32-grade values carried as hi + lo halves and
    multiplied on the 16-bit MFMA pipe.  As a MODEL compute dtype (XML(cfg, compute_dtype=ops.F16S)) the activations stay
    torch.float32 and every projection weight is a SplitWeight."""

    def __repr__(self):
        return "tvretrieval_amd.ops.F16S"


F16S = _SplitF16()
_DT = {torch.float32: XML_F32, torch.bfloat16: XML_BF16, torch.float16: _lib.XML_F16, F16S: _lib.XML_F16S}
F16_UNIT_LOG2 = 14         # XML_F16_UNIT_LOG2: fixed scale of unit-norm rows in f16 / split-f16 form


def act_dtype(dtype):
    """Storage dtype of the activations of a model computing in `dtype`."""
    return torch.float32 if dtype is F16S else dtype


class SplitWeight(object):
    """A projection weight (n, k) packed by xml_pack_weights_f16s: (n, 3k) f16 [hi | hi | lo] at one power-of-two scale +
    a 16-byte trailer holding 1 / scale.  Quacks like a tensor for the wrappers below (shape / dtype / device / data_ptr)."""

    def __init__(self, data, n, k):
        self.data, self.shape, self.dtype, self.device, self.is_cuda = data, (int(n), int(k)), F16S, data.device, data.is_cuda

    def data_ptr(self):
        return self.data.data_ptr()

    def is_contiguous(self):
        return True


class SplitRows(object):
    """Rows of f32-grade values in split-f16 form (xml_split_f16_rows): `data` int32 (..., k) -- 4 bytes per element, per 32
    elements [32 x hi | 32 x lo] halves -- and `inv` f32 (...) = 1 / scale of every row."""

    def __init__(self, data, inv):
        self.data, self.inv, self.shape, self.dtype, self.device, self.is_cuda = data, inv, tuple(data.shape), F16S, \
            data.device, data.is_cuda

    def data_ptr(self):
        return self.data.data_ptr()

    def is_contiguous(self):
        return self.data.is_contiguous()

    def numel(self):
        return self.data.numel()

    def element_size(self):
        return 4

    def __getitem__(self, idx):
        return SplitRows(self.data[idx], self.inv[idx])

    def float(self):
        return unsplit_f16_rows(self)


def dt_of(t):
    try:
        return _DT[t.dtype if hasattr(t, "dtype") else t]
    except KeyError:
        raise _lib.XmlHipError("unsupported dtype %s" % (t.dtype if hasattr(t, "dtype") else t))


def _req(t, name, dtype=None):
    if not isinstance(t, (torch.Tensor, SplitWeight, SplitRows)):
        raise _lib.XmlHipError("%s: expected a tensor" % name)
    if not t.is_cuda:
        raise _lib.XmlHipError("%s: tensor must live on the GPU (got %s); the HIP path has no CPU fallback"
                               % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise _lib.XmlHipError("%s: expected dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.XmlHipError("%s: tensor must be contiguous" % name)
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = torch._C._cuda_getCurrentRawStream      # (device index) -> hipStream_t as int; ~0.3 us
_cur_device = torch._C._cuda_getDevice


def _stream():
    """The current HIP stream of the current device as a void*.  (torch.cuda.current_stream() builds a Stream object through
    three Python layers -- ~10 us per call, 90 calls per training step: 0.9 ms of a 6 ms step was spent asking for it.)"""
    return ctypes.c_void_p(_raw_stream(_cur_device()))


_ws_cache = {}


def _workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream).  The C ABI never allocates."""
    key = (device.index, _raw_stream(device.index if device.index is not None else _cur_device()))
    buf = _ws_cache.get(key)
    nbytes = max(int(nbytes), 256)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def convert(x, dtype):
    """xml_convert: dtype conversion on the device (round-to-nearest-even to bf16)."""
    _req(x, "x")
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(_lib.load().xml_convert(_p(x), dt_of(x), _p(out), dt_of(dtype), x.numel(), _stream()), "xml_convert")
    return out


def pack_weights(w_f32, dtype, out=None):
    _req(w_f32, "w", torch.float32)
    if dtype is F16S:
        assert out is None, "pack_weights: out= is for the plain low-precision copies"
        return pack_weights_f16s(w_f32)
    if out is None:
        out = torch.empty(w_f32.shape, dtype=dtype, device=w_f32.device)
    else:
        _req(out, "out", dtype)
        assert out.numel() == w_f32.numel(), "pack_weights: out has the wrong size"
    check(_lib.load().xml_pack_weights(_p(w_f32), _p(out), dt_of(dtype), w_f32.numel(), _stream()), "xml_pack_weights")
    return out


def linear_ln_relu_pos(x, ln_in_g, ln_in_b, w, b, pos, ln_pos_g, ln_pos_b):
    """K1+K2.  x (N, L, D_in) f32 or compute dtype; w (H, ceil8(D_in)) compute dtype, zero columns beyond D_in
    -> (N, L, H)."""
    _req(x, "x"); _req(w, "w"); _req(pos, "pos", act_dtype(w.dtype))
    n, seq_len, d_in = x.shape
    hidden = w.shape[0]
    assert w.shape[1] == (d_in + 7) // 8 * 8 and pos.shape[1] == hidden and pos.shape[0] >= seq_len, "shape mismatch"
    for t, nm in ((ln_in_g, "ln_in_g"), (ln_in_b, "ln_in_b"), (b, "b"), (ln_pos_g, "ln_pos_g"), (ln_pos_b, "ln_pos_b")):
        _req(t, nm, torch.float32)
    lib = _lib.load()
    dt = dt_of(w)
    rows = n * seq_len
    y = torch.empty((n, seq_len, hidden), dtype=act_dtype(w.dtype), device=x.device)
    nb = lib.xml_linear_ln_relu_pos_workspace_bytes(rows, d_in, hidden, dt)
    ws = _workspace(nb, x.device)
    check(lib.xml_linear_ln_relu_pos(_p(x), dt_of(x), _p(ln_in_g), _p(ln_in_b), _p(w), _p(b), _p(pos), _p(ln_pos_g),
                                     _p(ln_pos_b), _p(y), rows, seq_len, d_in, hidden, dt, _p(ws), ws.numel(),
                                     _stream()), "xml_linear_ln_relu_pos")
    return y


def check_count(v, what):
    if v < 0:
        check(v, what)
    return v


def _req_w(w, name, x):
    """weight of a projection applied to activations x: x's dtype, or a SplitWeight for f32 activations (XML_F16S)."""
    _req(w, name)
    if not (w.dtype == x.dtype or (w.dtype is F16S and x.dtype == torch.float32)):
        raise _lib.XmlHipError("%s: weight dtype %s does not go with activations of dtype %s" % (name, w.dtype, x.dtype))
    return w


def attention_block(x, key_mask, wqkv, bqkv, wo, bo, ln_g, ln_b, n_heads, out=None):
    """K3+K4 (BertAttention).  x (N, L, H); key_mask (N, L) f32.  out: optional (N, L, H) contiguous destination (e.g. a
    slice of a preallocated index tensor), must not alias x."""
    _req(x, "x"); _req(key_mask, "key_mask", torch.float32); _req_w(wqkv, "wqkv", x); _req_w(wo, "wo", x)
    for t, nm in ((bqkv, "bqkv"), (bo, "bo"), (ln_g, "ln_g"), (ln_b, "ln_b")):
        _req(t, nm, torch.float32)
    n, seq_len, hidden = x.shape
    lib = _lib.load()
    dt = dt_of(wqkv)
    if out is None:
        y = torch.empty_like(x)
    else:
        _req(out, "out", x.dtype)
        assert out.shape == x.shape and out.data_ptr() != x.data_ptr()
        y = out
    ws = _workspace(lib.xml_attention_block_workspace_bytes(n, seq_len, hidden, dt), x.device)
    check(lib.xml_attention_block(_p(x), _p(key_mask), _p(wqkv), _p(bqkv), _p(wo), _p(bo), _p(ln_g), _p(ln_b), _p(y),
                                  n, seq_len, hidden, n_heads, dt, _p(ws), ws.numel(), _stream()),
          "xml_attention_block")
    return y


def attention_core(q, k, v, q_mask, k_mask, n_heads):
    """BertSelfAttention.forward behind its projections: q (N, Lq, H), k / v (N, Lk, H) projected states (compute dtype),
    k_mask (N, Lk) f32, q_mask (N, Lq) f32 or None -> context layer (N, Lq, H)."""
    _req(q, "q"); _req(k, "k", q.dtype); _req(v, "v", q.dtype); _req(k_mask, "k_mask", torch.float32)
    if q_mask is not None:
        _req(q_mask, "q_mask", torch.float32)
    n, lq, hidden = q.shape
    lk = k.shape[1]
    assert k.shape == v.shape and k.shape[0] == n and k.shape[2] == hidden
    out = torch.empty((n, lq, hidden), dtype=q.dtype, device=q.device)
    check(_lib.load().xml_attention_core(_p(q), hidden, _p(k), hidden, _p(v), hidden, _p(q_mask), _p(k_mask), _p(out), n, lq,
                                         lk, hidden, int(n_heads), dt_of(q), _stream()), "xml_attention_core")
    return out


def conv1d_rows(x, w):
    """nn.Conv1d(1, 1, k, padding=k // 2, bias=False) on the last dimension of x (..., L) f32; w (k,) f32."""
    _req(x, "x", torch.float32); _req(w, "w", torch.float32)
    y = torch.empty_like(x)
    l = x.shape[-1]
    check(_lib.load().xml_conv1d_rows(_p(x), _p(w), _p(y), x.numel() // l, l, w.numel(), _stream()), "xml_conv1d_rows")
    return y


def cross_attention(main_x, main_mask, side_x, side_mask, wq, bq, wkv, bkv, ln_g, ln_b, n_heads):
    """LN(MHA(main, side, side, main_mask (x) side_mask) + main), xml/model_xml.py:369-371."""
    _req(main_x, "main_x"); _req(side_x, "side_x", main_x.dtype)
    _req(main_mask, "main_mask", torch.float32); _req(side_mask, "side_mask", torch.float32)
    _req_w(wq, "wq", main_x); _req_w(wkv, "wkv", main_x)
    for t, nm in ((bq, "bq"), (bkv, "bkv"), (ln_g, "ln_g"), (ln_b, "ln_b")):
        _req(t, nm, torch.float32)
    n, lq, hidden = main_x.shape
    lk = side_x.shape[1]
    lib = _lib.load()
    dt = dt_of(wq)
    y = torch.empty_like(main_x)
    ws = _workspace(lib.xml_cross_attention_workspace_bytes(n, lq, lk, hidden, dt), main_x.device)
    check(lib.xml_cross_attention(_p(main_x), _p(main_mask), _p(side_x), _p(side_mask), _p(wq), _p(bq), _p(wkv),
                                  _p(bkv), _p(ln_g), _p(ln_b), _p(y), n, lq, lk, hidden, n_heads, dt, _p(ws),
                                  ws.numel(), _stream()), "xml_cross_attention")
    return y


def modular_pool(enc, mask, w_m, return_att=False):
    """K5.  enc (N, Lq, H); mask (N, Lq) f32; w_m (n_mod, H) f32 -> (n_mod, N, H).
    return_att: -> (pooled, att (N, Lq, n_mod) f32), the softmax weights (0 at masked tokens); pooled is bitwise the same."""
    _req(enc, "enc"); _req(mask, "mask", torch.float32); _req(w_m, "w_m", torch.float32)
    n, lq, hidden = enc.shape
    n_mod = w_m.shape[0]
    out = torch.empty((n_mod, n, hidden), dtype=enc.dtype, device=enc.device)
    if return_att:
        att = torch.empty((n, lq, n_mod), dtype=torch.float32, device=enc.device)
        check(_lib.load().xml_modular_pool_att(_p(enc), _p(mask), _p(w_m), _p(out), _p(att), n, lq, hidden, n_mod,
                                               dt_of(enc), _stream()), "xml_modular_pool_att")
        return out, att
    check(_lib.load().xml_modular_pool(_p(enc), _p(mask), _p(w_m), _p(out), n, lq, hidden, n_mod, dt_of(enc),
                                       _stream()), "xml_modular_pool")
    return out


def linear(x, w, b=None, relu=False, addend=None):
    """y = x W^T + b [+ addend].  x (..., K), w (N, K) same dtype; addend (..., N) of x's dtype, added in the GEMM epilogue."""
    _req(x, "x"); _req_w(w, "w", x)
    if b is not None:
        _req(b, "b", torch.float32)
    k = x.shape[-1]
    rows = x.numel() // k
    y = torch.empty(x.shape[:-1] + (w.shape[0],), dtype=x.dtype, device=x.device)
    if addend is not None:
        _req(addend, "addend", x.dtype)
        assert w.dtype is not F16S and addend.numel() == y.numel()
        check(_lib.load().xml_linear_add(_p(x), _p(w), _p(b), _p(addend), _p(y), rows, w.shape[0], k, int(relu), dt_of(x),
                                         _stream()), "xml_linear_add")
        return y
    if w.dtype is F16S:
        lib = _lib.load()
        ws = _workspace(lib.xml_linear_f16s_workspace_bytes(rows, k), x.device)
        check(lib.xml_linear_f16s(_p(x), _p(w), _p(b), _p(y), rows, w.shape[0], k, int(relu), _p(ws), ws.numel(), _stream()),
              "xml_linear_f16s")
        return y
    check(_lib.load().xml_linear(_p(x), _p(w), _p(b), _p(y), rows, w.shape[0], k, int(relu), dt_of(x), _stream()),
          "xml_linear")
    return y


def l2norm_rows(x):
    _req(x, "x")
    d = x.shape[-1]
    y = torch.empty_like(x)
    check(_lib.load().xml_l2norm_rows(_p(x), _p(y), x.numel() // d, d, dt_of(x), _stream()), "xml_l2norm_rows")
    return y


def l2norm_rows_eps(x, eps=1e-5):
    """dataset normalisation x / (||x|| + eps) on the device (f32)."""
    _req(x, "x", torch.float32)
    d = x.shape[-1]
    y = torch.empty_like(x)
    check(_lib.load().xml_l2norm_rows_eps(_p(x), _p(y), x.numel() // d, d, float(eps), _stream()), "xml_l2norm_rows_eps")
    return y


def _tef_place(what, tef, tef_pos, tef_len, n):
    """The optional (n,) int32 tef_pos / tef_len of the *_tef ingest entries: both or neither, and only with tef=True."""
    if (tef_pos is None) != (tef_len is None):
        raise _lib.XmlHipError("%s: tef_pos and tef_len are given both or neither" % what)
    if tef_pos is None:
        return
    if not tef:
        raise _lib.XmlHipError("%s: tef_pos / tef_len need tef=True" % what)
    for t, name in ((tef_pos, "tef_pos"), (tef_len, "tef_len")):
        _req(t, name, torch.int32)
        if t.dim() != 1 or t.numel() != n:
            raise _lib.XmlHipError("%s: %s must hold n = %d entries" % (what, name, n))


def ingest_rows(src, row_start, n, lmax, max_len, normalize=True, eps=1e-5, out_dtype=torch.float32, tef=False, tef_pos=None,
                tef_len=None):
    """Context collate on the device (xml_ingest_rows): src (rows, d) f32 / f16 = the batch's raw clip rows back to back,
    row_start (n + 1,) int64 -> (features (n, lmax, d) out_dtype [x / (||x|| + eps) per clip, zero padding], mask (n, lmax)).
    tef=True (xml_ingest_rows_tef): features are (n, lmax, d + 2), the d columns as before plus the temporal endpoint columns
    (P + l) / L and that + 1 / L of the *_tef context modes; P = tef_pos[i], L = tef_len[i] ((n,) int32, for the parts of a
    long video) or P = 0, L = the item's truncated length."""
    _req(src, "src"); _req(row_start, "row_start", torch.int64)
    assert src.dtype in (torch.float32, torch.float16) and row_start.numel() == n + 1
    d = src.shape[-1]
    _tef_place("ingest_rows", tef, tef_pos, tef_len, int(n))
    if tef:
        out = torch.empty((n, lmax, d + 2), dtype=out_dtype, device=src.device)
        mask = torch.empty((n, lmax), dtype=torch.float32, device=src.device)
        check(_lib.load().xml_ingest_rows_tef(_p(src), dt_of(src), _p(row_start), _p(tef_pos), _p(tef_len), _p(out),
                                              dt_of(out_dtype), _p(mask), int(n), int(lmax), d, int(max_len), float(eps),
                                              int(bool(normalize)), _stream()), "xml_ingest_rows_tef")
        return out, mask
    out = torch.empty((n, lmax, d), dtype=out_dtype, device=src.device)
    mask = torch.empty((n, lmax), dtype=torch.float32, device=src.device)
    check(_lib.load().xml_ingest_rows(_p(src), dt_of(src), _p(row_start), _p(out), dt_of(out_dtype), _p(mask), int(n), int(lmax),
                                      d, int(max_len), float(eps), int(bool(normalize)), _stream()), "xml_ingest_rows")
    return out, mask


# ---- ingest from frame- / word-level stores (include/xmlhip_ingest_pool.h; ingest.PooledStore) ----------------------------------
POOLS = {"max": 0, "mean": 1}         # XML_POOL_MAX / XML_POOL_MEAN


def ingest_pool_rows(sources, row_start, n, lmax, max_len, pool="max", normalize=True, eps=1e-5, out_dtype=torch.float32,
                     want_filled=False, tef=False, tef_pos=None, tef_len=None):
    """Context collate with clip pooling on the device (xml_ingest_pool_rows): sources = 1 or 2 tuples (src, seg, norm) -- src
    (rows_x, d_x) f16 / f32 rows FINER than clips (frames, words), seg (R, 2) int64 on the device: the half-open source-row range
    of each of the batch's R = row_start[n] clip rows (an empty or out-of-range range gives a zero block), norm: x / (||x|| + eps)
    on that source's pooled block.  row_start (n + 1,) int64 clip rows per video, back to back -> (features (n, lmax, sum d_x)
    out_dtype [max or mean over each range, per-source norm, with normalize the norm of the whole row, zero padding], mask
    (n, lmax)) and with want_filled also filled (n, lmax): 1 where a source had rows for the clip.
    tef=True (xml_ingest_pool_rows_tef): features are (n, lmax, sum d_x + 2), ending in the temporal endpoint columns; tef_pos /
    tef_len as in ingest_rows."""
    if len(sources) not in (1, 2):
        raise _lib.XmlHipError("ingest_pool_rows: 1 or 2 sources expected, got %d" % len(sources))
    if pool not in POOLS:
        raise _lib.XmlHipError("ingest_pool_rows: pool must be 'max' or 'mean', got %r" % (pool,))
    _req(row_start, "row_start", torch.int64)
    n, lmax = int(n), int(lmax)
    if row_start.numel() != n + 1:
        raise _lib.XmlHipError("ingest_pool_rows: row_start must hold n + 1 = %d entries" % (n + 1))
    args, d = [], 0
    for src, seg, norm in sources:
        _req(src, "src"); _req(seg, "seg", torch.int64)
        if src.dtype not in (torch.float32, torch.float16) or src.dim() != 2:
            raise _lib.XmlHipError("ingest_pool_rows: src: expected (rows, d) float32 or float16")
        if seg.dim() != 2 or seg.shape[1] != 2:
            raise _lib.XmlHipError("ingest_pool_rows: seg: expected (R, 2) int64, one source-row range per clip row")
        args += [_p(src), dt_of(src), int(src.shape[0]), int(src.shape[1]), _p(seg), int(bool(norm))]
        d += int(src.shape[1])
    if len(sources) == 1:
        args += [None, 0, 0, 0, None, 0]
    dev = sources[0][0].device
    _tef_place("ingest_pool_rows", tef, tef_pos, tef_len, n)
    out = torch.empty((n, lmax, d + (2 if tef else 0)), dtype=out_dtype, device=dev)
    mask = torch.empty((n, lmax), dtype=torch.float32, device=dev)
    filled = torch.empty((n, lmax), dtype=torch.float32, device=dev) if want_filled else None
    if tef:
        check(_lib.load().xml_ingest_pool_rows_tef(len(sources), *args, _p(row_start), _p(out), dt_of(out_dtype), _p(mask),
                                                   _p(filled), n, lmax, int(max_len), float(eps), int(bool(normalize)), POOLS[pool],
                                                   _p(tef_pos), _p(tef_len), _stream()), "xml_ingest_pool_rows_tef")
        return (out, mask, filled) if want_filled else (out, mask)
    check(_lib.load().xml_ingest_pool_rows(len(sources), *args, _p(row_start), _p(out), dt_of(out_dtype), _p(mask), _p(filled), n,
                                           lmax, int(max_len), float(eps), int(bool(normalize)), POOLS[pool], _stream()),
          "xml_ingest_pool_rows")
    return (out, mask, filled) if want_filled else (out, mask)


def gather_feature_rows(src, row_start, ids, lmax, max_len, item_of=None, normalize=True, eps=1e-5, tef=False,
                        out_dtype=torch.float32, out=None, mask_out=None, len_out=None, want_len=True):
    """One stream of a training batch from a device-resident ragged store (xml_gather_feature_rows): src (rows, d) f32 / f16,
    row_start (n_items + 1,) int64, ids (n,) int32 example ids, item_of (n_examples,) int32 example -> item or None (ids are
    item ids) -> (features (n, lmax, d + 2 * tef) [x / (||x|| + eps) per row, the temporal endpoint columns, zero padding],
    mask (n, lmax) f32, lengths (n,) int32 or None with want_len=False).  out / mask_out / len_out: existing tensors to write
    into."""
    _req(src, "src"); _req(row_start, "row_start", torch.int64); _req(ids, "ids", torch.int32)
    if src.dtype not in (torch.float32, torch.float16) or src.dim() != 2:
        raise _lib.XmlHipError("src: expected (rows, d) float32 or float16")
    n, d = int(ids.numel()), int(src.shape[1])
    dd = d + (2 if tef else 0)
    if item_of is not None:
        _req(item_of, "item_of", torch.int32)
    for t, name, shape, dtype in ((out, "out", (n, int(lmax), dd), None), (mask_out, "mask_out", (n, int(lmax)), torch.float32),
                                  (len_out, "len_out", (n,), torch.int32)):
        if t is not None:
            _req(t, name, dtype)
            if tuple(t.shape) != shape:
                raise _lib.XmlHipError("%s: expected shape %s, got %s" % (name, shape, tuple(t.shape)))
    if out is None:
        out = torch.empty((n, int(lmax), dd), dtype=out_dtype, device=src.device)
    if mask_out is None:
        mask_out = torch.empty((n, int(lmax)), dtype=torch.float32, device=src.device)
    if len_out is None and want_len:
        len_out = torch.empty((n,), dtype=torch.int32, device=src.device)
    check(_lib.load().xml_gather_feature_rows(
        _p(src), dt_of(src), _p(row_start), row_start.numel() - 1, _p(ids), n, _p(item_of),
        0 if item_of is None else item_of.numel(), _p(out), dt_of(out), _p(mask_out), _p(len_out), int(lmax), d, int(max_len),
        float(eps), int(bool(normalize)), int(bool(tef)), _stream()), "xml_gather_feature_rows")
    return out, mask_out, len_out


def gather_pool_feature_rows(sources, clip_start, ids, lmax, max_len, item_of=None, pool="max", normalize=True, eps=1e-5,
                             tef=False, out_dtype=torch.float32, out=None, mask_out=None, len_out=None, want_len=True):
    """One stream of a training batch from a device-resident FRAME- or WORD-level store (xml_gather_pool_feature_rows; include/
    xmlhip_train_pool.h): gather_feature_rows with the pooling of ingest_pool_rows in the launch.  sources = 1 or 2 tuples
    (src, seg, norm) -- src (rows_x, d_x) f16 / f32: the fine rows of the WHOLE store, seg (clip_start[-1], 2) int64: the
    absolute half-open source-row range of every clip of every item, norm as in ingest_pool_rows.  clip_start (n_items + 1,)
    int64, ids (n,) int32 example ids, item_of (n_examples,) int32 example -> item or None (ids are item ids) -> (features
    (n, lmax, sum d_x + 2 * tef) [the rows of ingest_pool_rows on the same ranges, the temporal endpoint columns, zero padding],
    mask (n, lmax) f32, lengths (n,) int32 or None with want_len=False).  out / mask_out / len_out: existing tensors to write
    into."""
    if len(sources) not in (1, 2):
        raise _lib.XmlHipError("gather_pool_feature_rows: 1 or 2 sources expected, got %d" % len(sources))
    if pool not in POOLS:
        raise _lib.XmlHipError("gather_pool_feature_rows: pool must be 'max' or 'mean', got %r" % (pool,))
    _req(clip_start, "clip_start", torch.int64); _req(ids, "ids", torch.int32)
    args, d = [], 0
    for src, seg, norm in sources:
        _req(src, "src"); _req(seg, "seg", torch.int64)
        if src.dtype not in (torch.float32, torch.float16) or src.dim() != 2:
            raise _lib.XmlHipError("gather_pool_feature_rows: src: expected (rows, d) float32 or float16")
        if seg.dim() != 2 or seg.shape[1] != 2:
            raise _lib.XmlHipError("gather_pool_feature_rows: seg: expected (R, 2) int64, one source-row range per clip row")
        args += [_p(src), dt_of(src), int(src.shape[0]), int(src.shape[1]), _p(seg), int(bool(norm))]
        d += int(src.shape[1])
    if len(sources) == 1:
        args += [None, 0, 0, 0, None, 0]
    dev = sources[0][0].device
    n, lmax = int(ids.numel()), int(lmax)
    dd = d + (2 if tef else 0)
    if item_of is not None:
        _req(item_of, "item_of", torch.int32)
    for t, name, shape, dtype in ((out, "out", (n, lmax, dd), None), (mask_out, "mask_out", (n, lmax), torch.float32),
                                  (len_out, "len_out", (n,), torch.int32)):
        if t is not None:
            _req(t, name, dtype)
            if tuple(t.shape) != shape:
                raise _lib.XmlHipError("%s: expected shape %s, got %s" % (name, shape, tuple(t.shape)))
    if out is None:
        out = torch.empty((n, lmax, dd), dtype=out_dtype, device=dev)
    if mask_out is None:
        mask_out = torch.empty((n, lmax), dtype=torch.float32, device=dev)
    if len_out is None and want_len:
        len_out = torch.empty((n,), dtype=torch.int32, device=dev)
    check(_lib.load().xml_gather_pool_feature_rows(
        len(sources), *args, _p(clip_start), clip_start.numel() - 1, _p(ids), n, _p(item_of),
        0 if item_of is None else item_of.numel(), _p(out), dt_of(out), _p(mask_out), _p(len_out), lmax, int(max_len), float(eps),
        int(bool(normalize)), POOLS[pool], int(bool(tef)), _stream()), "xml_gather_pool_feature_rows")
    return out, mask_out, len_out


def gather_index_rows(table, ids, out=None):
    """out[i, :] = table[ids[i], :] for an (n_rows, w) int64 table and int32 ids, zeros for an id out of range
    (xml_gather_index_rows): the (N, 2) start / end labels -> the batch's st_ed_indices."""
    _req(table, "table", torch.int64); _req(ids, "ids", torch.int32)
    if table.dim() != 2:
        raise _lib.XmlHipError("table: expected (n_rows, w)")
    n, w = int(ids.numel()), int(table.shape[1])
    if out is None:
        out = torch.empty((n, w), dtype=torch.int64, device=table.device)
    else:
        _req(out, "out", torch.int64)
        if tuple(out.shape) != (n, w):
            raise _lib.XmlHipError("out: expected shape %s, got %s" % ((n, w), tuple(out.shape)))
    check(_lib.load().xml_gather_index_rows(_p(table), w, int(table.shape[0]), _p(ids), n, _p(out), _stream()),
          "xml_gather_index_rows")
    return out


def add_layernorm(a, b, g, beta, out_dtype=None):
    _req(a, "a"); _req(g, "g", torch.float32); _req(beta, "beta", torch.float32)
    out_dtype = out_dtype or (b.dtype if b is not None else a.dtype)
    d = a.shape[-1]
    y = torch.empty(a.shape, dtype=out_dtype, device=a.device)
    check(_lib.load().xml_add_layernorm(_p(a), dt_of(a), _p(b), _p(g), _p(beta), _p(y), a.numel() // d, d,
                                        dt_of(out_dtype), _stream()), "xml_add_layernorm")
    return y


def q2c_scores(qn, cn, mask, out=None, combine=False):
    """K6.  qn (Nq, H) and cn (Nv, Lpad, H) L2-normalised; mask (Nv, Lpad) f32 -> out (Nq, Nv) f32."""
    _req(qn, "qn"); _req(cn, "cn", qn.dtype); _req(mask, "mask", torch.float32)
    nq, hidden = qn.shape
    nv, lpad, h2 = cn.shape
    assert h2 == hidden and tuple(mask.shape) == (nv, lpad)
    if out is None:
        assert not combine
        out = torch.empty((nq, nv), dtype=torch.float32, device=qn.device)
    _req(out, "out", torch.float32)
    check(_lib.load().xml_q2c_scores(_p(qn), _p(cn), _p(mask), _p(out), out.stride(0), nq, nv, lpad, hidden,
                                     int(combine), dt_of(qn), _stream()), "xml_q2c_scores")
    return out


class TiledRows(object):
    """Rows of a (rows, H) operand in K6's slice-major tile layout (xml_q2c_tile_rows): `data` is the flat tiled
    image, `rows` / `hidden` / `dtype` describe the row-major tensor it was made from."""

    def __init__(self, data, rows, hidden, shape, all_valid=False):
        self.data, self.rows, self.hidden, self.shape = data, int(rows), int(hidden), tuple(shape)
        self.dtype, self.device = data.dtype, data.device
        self.all_valid = bool(all_valid)     # every clip mask of the corpus is 1: K6 may skip the masks (5-slot ring)
        self.mask_bits = None                # (Nv, 4) int32: binary clip masks packed 128 bits per video (ragged corpora)
        self.plan = None                     # PackPlan: length-bucketed image (mask_bits are then per wave tile)

    def numel(self):
        return self.data.numel()

    def element_size(self):
        return self.data.element_size()

    def to_rows(self):
        """Back to the row-major tensor of the original shape (tests, the CPU baseline sample)."""
        per = 64 // self.data.element_size()
        t = self.data.view(-1, self.hidden // per, 256, per).permute(0, 2, 1, 3).reshape(-1, self.hidden)
        if self.plan is not None:            # un-bucket: packed row i came from original row row_map[i]
            rm = self.plan.row_map.long()
            out = torch.zeros((self.rows, self.hidden), dtype=t.dtype, device=t.device)
            ok = rm >= 0
            out[rm[ok]] = t[:rm.numel()][ok]
            return out.reshape(self.shape)
        return t[:self.rows].reshape(self.shape).contiguous()


_TILE_PATTERNS = None


def _tile_patterns():
    """Every multiset of video sizes (1..8 blocks of 16 clips) that fits the 16 blocks of a K6 tile: (P, 9) counts per
    size, (P,) blocks used, and per pattern the order in which its videos are laid out -- a sub-multiset that fills the
    left wave tile exactly (8 blocks) goes first when there is one, so that no video straddles the two wave tiles."""
    global _TILE_PATTERNS
    if _TILE_PATTERNS is None:
        pats = []

        def rec(rem, mx, cur):
            if cur:
                pats.append(list(cur))
            for part in range(min(mx, rem), 0, -1):
                cur.append(part)
                rec(rem - part, part, cur)
                cur.pop()
        rec(16, 8, [])
        cnt = np.zeros((len(pats), 9), dtype=np.int64)
        orders = []
        for i, pat in enumerate(pats):
            for x in pat:
                cnt[i, x] += 1
            best = None
            for bits in range(1 << len(pat)):                  # <= 2^16 subsets, once per process
                if sum(x for j, x in enumerate(pat) if bits >> j & 1) == 8:
                    best = bits
                    break
            if best is None:
                orders.append(list(pat))
            else:
                orders.append([x for j, x in enumerate(pat) if best >> j & 1] + [x for j, x in enumerate(pat) if not best >> j & 1])
        _TILE_PATTERNS = (cnt, (cnt * np.arange(9)).sum(1), orders)
    return _TILE_PATTERNS


class PackPlan(object):
    """Packed layout of a ragged corpus for K6 (xml_q2c_scores_packed): every video is padded to a multiple of 16 clips
    ("blocks") and the videos are laid back to back into the 16 blocks of a 256-row tile; a video may straddle the two
    wave tiles (8 blocks each) of a tile, never two tiles.
      row_map  (n_tiles * 256,) int32  original row (video * 128 + clip) of every packed row, -1 = zero row
      slot_ids (2 * n_tiles, 8) int32  per block: id >= 0 last block of video id, -1 the video continues in the next block,
                                       -2 unused, -3 (block 7 of an even wave tile) continues in the next wave tile
      padded_clips                     sum of the padded lengths; n_tiles * 256 = the clip rows K6 executes
    The tiles are filled by a greedy bin packing over the 794 size multisets that fit a tile: fullest pattern first, ties
    to the pattern that draws on the sizes holding most of the remaining blocks (the real TVR lengths, mean 51.4 clips:
    4 871 tiles = the lower bound ceil(blocks / 16); 1.114 x the valid clip rows against 1.31 x for 128 / 64 / 32 buckets)."""

    def __init__(self, masks):
        m = masks[0]
        for o in masks[1:]:
            m = torch.maximum(m, o)
        nv, l = m.shape
        assert l == 128
        dev = m.device
        pos = torch.arange(1, l + 1, device=dev, dtype=torch.float32)
        lens = ((m != 0).float() * pos).amax(1).cpu().numpy().astype(np.int64)      # last valid clip + 1 (one read-back)
        blocks = np.maximum((lens + 15) // 16, 1)
        pat_cnt, pat_fill, pat_order = _tile_patterns()
        counts = np.bincount(blocks, minlength=9).astype(np.int64)
        queues = {s: np.nonzero(blocks == s)[0] for s in range(1, 9)}             # ascending ids per size
        taken = np.zeros(9, dtype=np.int64)
        sizes = np.arange(9)
        seg_tile, seg_start, seg_nb, seg_vid = [], [], [], []
        n_tiles = 0
        while counts.sum() > 0:
            weight = counts * sizes
            score = pat_fill * 1000.0 + (pat_cnt * sizes * (weight / weight.sum())).sum(1) * 50.0
            score = np.where((pat_cnt <= counts).all(1), score, -1.0)
            i = int(score.argmax())
            used = pat_cnt[i]
            rep = max(1, int(min(counts[s] // used[s] for s in range(1, 9) if used[s])) // 4)
            order = np.asarray(pat_order[i], dtype=np.int64)
            start = np.concatenate([[0], np.cumsum(order)[:-1]])
            vid = np.empty((rep, len(order)), dtype=np.int64)
            for s in range(1, 9):
                if used[s]:
                    ids = queues[s][taken[s]:taken[s] + rep * used[s]].reshape(rep, used[s])
                    vid[:, order == s] = ids
                    taken[s] += rep * used[s]
            seg_tile.append(np.repeat(np.arange(n_tiles, n_tiles + rep), len(order)))
            seg_start.append(np.tile(start, rep))
            seg_nb.append(np.tile(order, rep))
            seg_vid.append(vid.reshape(-1))
            counts = counts - used * rep
            n_tiles += rep
        seg_tile, seg_start = np.concatenate(seg_tile), np.concatenate(seg_start)
        seg_nb, seg_vid = np.concatenate(seg_nb), np.concatenate(seg_vid)
        first = seg_tile * 16 + seg_start                                          # first block of every video
        codes = np.full(n_tiles * 16, -2, dtype=np.int64)
        seg_of_block = np.repeat(np.arange(len(seg_nb)), seg_nb)
        blk = first[seg_of_block] + (np.arange(seg_nb.sum()) - np.repeat(np.cumsum(seg_nb) - seg_nb, seg_nb))
        codes[blk] = -1
        codes[first + seg_nb - 1] = seg_vid
        straddles = (seg_start < 8) & (seg_start + seg_nb > 8)
        codes[seg_tile[straddles] * 16 + 7] = -3
        rows = np.full(n_tiles * 256, -1, dtype=np.int64)
        seg_of_row = np.repeat(np.arange(len(seg_nb)), seg_nb * 16)
        within = np.arange(seg_nb.sum() * 16) - np.repeat(np.cumsum(seg_nb * 16) - seg_nb * 16, seg_nb * 16)
        rows[first[seg_of_row] * 16 + within] = seg_vid[seg_of_row] * 128 + within
        self.row_map = torch.from_numpy(rows.astype(np.int32)).to(dev).contiguous()
        self.slot_ids = torch.from_numpy(codes.astype(np.int32).reshape(2 * n_tiles, 8)).to(dev).contiguous()
        self.n_tiles = n_tiles
        self.n_videos = nv
        self.n_straddles = int(straddles.sum())
        self.padded_clips = int(seg_nb.sum() * 16)

    def mask_bits(self, mask):
        """(nv, 128) binary f32 mask -> (2 * n_tiles, 4) int32: the masks of every wave tile's 128 packed columns."""
        flat = torch.cat([(mask != 0).reshape(-1), torch.zeros(1, dtype=torch.bool, device=mask.device)])
        rm = self.row_map.long()
        return _pack_bits32(flat[torch.where(rm >= 0, rm, torch.full_like(rm, flat.numel() - 1))].view(-1, 128))


def _pack_bits32(bits):
    """(..., 32 k) bool or 0/1 tensor -> (..., k) int32 words: bit j of word w is element 32 w + j."""
    w = bits.reshape(bits.shape[:-1] + (-1, 32)).to(torch.int64) << torch.arange(32, device=bits.device, dtype=torch.int64)
    w = w.sum(-1)                                                  # 0 .. 2^32 - 1
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def q2c_pack_plan(masks):
    """PackPlan for the corpus with these per-modality (Nv, 128) clip masks, or None when packing does not apply
    (non-binary masks, full-length corpus, fewer than 5 % of the clip rows to save)."""
    for m in masks:
        if m.shape[1] != 128 or not bool(((m == 0) | (m == 1)).all()):
            return None
    if all(bool((m == 1).all()) for m in masks):
        return None                           # full-length corpus: the mask-free kernel on the plain tiles
    plan = PackPlan(masks)
    # the packed kernel runs a four-slot ring and a per-video epilogue: it has to save rows to pay (plain: 2 videos per tile)
    return plan if plan.n_tiles * 2 <= 0.95 * ((plan.n_videos + 1) // 2 * 2) else None


def q2c_tiled_ok(lpad, hidden, dtype):
    return dtype in _DT and bool(_lib.load().xml_q2c_tiled_ok(int(lpad), int(hidden), dt_of(dtype)))


def q2c_tiled_numel(rows, hidden, dtype):
    """Elements of the K6 tile image of (rows, hidden) rows of `dtype`, 0 when the tiled kernel does not take the shape."""
    if not q2c_tiled_ok(128, hidden, dtype):
        return 0
    return int(_lib.load().xml_q2c_tiled_bytes(rows, hidden, _DT[dtype])) // torch.empty(0, dtype=dtype).element_size()


def _tile(x, rows_dst, row_map=None, normalize=False, out=None, rows_src=None):
    """The K6 tile image of rows_dst rows (rounded up to whole 256-row tiles) made from the (..., H) rows of x: destination
    row i holds source row row_map[i] (-1: a zero row), or row i without a map; normalize: F.normalize inside the pass.
    out: caller-owned flat buffer of exactly the image's size.  rows_src: x is the head of a longer contiguous buffer."""
    lib = _lib.load()
    hidden, dt = x.shape[-1], dt_of(x)
    rows = x.numel() // hidden if rows_src is None else rows_src
    n = lib.xml_q2c_tiled_bytes(rows_dst, hidden, dt) // x.element_size()
    if out is None:
        out = torch.empty(n, dtype=x.dtype, device=x.device)
    else:
        _req(out, "out", x.dtype)
        assert out.numel() == n
    if normalize:
        check(lib.xml_q2c_tile_rows_l2norm(_p(x), _p(row_map), _p(out), rows, n // hidden, hidden, dt, _stream()),
              "xml_q2c_tile_rows_l2norm")
    elif row_map is not None:
        check(lib.xml_q2c_tile_rows_gather(_p(x), _p(row_map), _p(out), n // hidden, hidden, dt, _stream()),
              "xml_q2c_tile_rows_gather")
    else:
        assert rows_dst == rows
        check(lib.xml_q2c_tile_rows(_p(x), _p(out), rows, hidden, dt, _stream()), "xml_q2c_tile_rows")
    return TiledRows(out, rows, hidden, x.shape)


def q2c_tile_rows(x):
    """(..., H) contiguous rows -> TiledRows (K6 operand layout)."""
    _req(x, "x")
    return _tile(x, x.numel() // x.shape[-1])


def q2c_tile_rows_l2norm(x):
    """F.normalize(x, dim=-1) + the K6 tile layout in ONE pass (xml_q2c_tile_rows_l2norm; bitwise l2norm_rows then
    q2c_tile_rows), or None when the fused pass does not take the shape."""
    _req(x, "x")
    if not _lib.load().xml_q2c_tile_rows_l2norm_ok(x.shape[-1], dt_of(x)):
        return None
    return _tile(x, x.numel() // x.shape[-1], normalize=True)


def pack_q2c_corpus(feat1n, mask=None, plan=None, normalize=False, out=None):
    """Resident form of the similarity operand: slice-major tiles when the persistent kernel takes it, else as is.
    mask (Nv, Lpad): if every entry is 1 (full-length videos) the tiles are marked all_valid and K6 skips the masks;
    binary masks are packed into bit words, any other mask (or None) stays the float mask K6 is handed per call.
    plan (q2c_pack_plan over ALL modalities' masks): the length-bucketed image instead.
    normalize: feat1n holds the UN-normalised clip features; F.normalize runs inside the tiling pass
    (xml_q2c_tile_rows_l2norm: bitwise the values of l2norm_rows followed by the tiling, one pass over the index less).
    out: caller-owned buffer for the plain (plan-less) tile image (inference.IndexStorage.tiles)."""
    nv, lpad, hidden = feat1n.shape
    tiled = q2c_tiled_ok(lpad, hidden, feat1n.dtype)
    fused = normalize and tiled and bool(_lib.load().xml_q2c_tile_rows_l2norm_ok(hidden, dt_of(feat1n)))
    if normalize and not fused:
        feat1n = l2norm_rows(feat1n)
    if not tiled:
        return feat1n
    _req(feat1n, "feat1n")
    if plan is not None:
        t = _tile(feat1n, plan.n_tiles * 256, plan.row_map, fused)
        t.plan = plan
        t.mask_bits = plan.mask_bits(mask)
        return t
    t = _tile(feat1n, nv * lpad, None, fused, out)
    t.all_valid = mask is not None and bool((mask == 1).all())
    if mask is not None and not t.all_valid and bool(((mask == 0) | (mask == 1)).all()):
        t.mask_bits = _pack_bits32(mask != 0)
    return t


_pair_maps = {}


def q2c_tile_rows_l2norm_pair(q0, q1):
    """q2c_tile_rows_l2norm of BOTH modalities' query vectors in ONE launch when they are the two halves of one contiguous
    (2, nq, H) tensor -- what xml_modular_pool returns: the tiled image of 2 R rows (R = nq rounded up to the 256-row tile) IS
    the two modalities' images back to back, and a row map (cached per nq) sends source row m nq + i to destination row m R + i.
    Same values as two launches; one kernel fewer in a 50-query batch's chain.  None when the layout does not match."""
    if q0.shape != q1.shape or q0.dtype != q1.dtype or not (q0.is_contiguous() and q1.is_contiguous()):
        return None
    nq, hidden = q0.shape
    if q1.data_ptr() != q0.data_ptr() + nq * hidden * q0.element_size():
        return None
    lib = _lib.load()
    if not lib.xml_q2c_tile_rows_l2norm_ok(hidden, dt_of(q0)):
        return None
    r = (nq + 255) // 256 * 256
    key = (nq, str(q0.device))
    rmap = _pair_maps.get(key)
    if rmap is None:
        i = torch.arange(2 * r, dtype=torch.int32, device=q0.device)
        m, j = i // r, i % r
        rmap = torch.where(j < nq, m * nq + j, torch.full_like(i, -1)).contiguous()
        _pair_maps[key] = rmap
    half = lib.xml_q2c_tiled_bytes(nq, hidden, dt_of(q0)) // q0.element_size()
    data = _tile(q0, 2 * r, rmap, True, rows_src=2 * nq).data
    return [TiledRows(data[:half], nq, hidden, q0.shape), TiledRows(data[half:], nq, hidden, q0.shape)]


def q2c_scores_fused(qn, cn, masks, out=None, normalize_q=False):
    """K6 for all modalities in one launch.  qn / cn / masks: lists (len 1 or 2) of (Nq,H), (Nv,Lpad,H), (Nv,Lpad) f32.
    out (Nq, Nv) f32 = mean over modalities of the masked max-over-clips cosine.
    cn[m] may be TiledRows (pack_q2c_corpus): the queries are tiled here and the tiled entry runs.
    normalize_q: qn holds the UN-normalised modular query vectors; on the tiled path F.normalize runs inside the tiling pass
    (one launch per modality instead of two -- 10 us of a 350 us 50-query batch), elsewhere as l2norm_rows first."""
    n_mod = len(qn)
    qt_pre = None
    if normalize_q:
        if isinstance(cn[0], TiledRows):
            qt_pre = q2c_tile_rows_l2norm_pair(qn[0], qn[1]) if n_mod == 2 else None      # (one launch for both modalities)
            if qt_pre is None:
                qt_pre = [q2c_tile_rows_l2norm(q.contiguous()) for q in qn]
            if any(t is None for t in qt_pre):
                qt_pre = None
        if qt_pre is None:
            qn = [l2norm_rows(q.contiguous()) for q in qn]
    if isinstance(cn[0], TiledRows):
        nq, hidden = qn[0].shape
        nv, lpad = masks[0].shape
        for m in range(n_mod):
            _req(qn[m], "qn"); _req(masks[m], "mask", torch.float32)
            assert isinstance(cn[m], TiledRows) and cn[m].shape == (nv, lpad, hidden) and cn[m].dtype == qn[m].dtype
        qt = qt_pre if qt_pre is not None else [q2c_tile_rows(q) for q in qn]
        if out is None:
            out = torch.empty((nq, nv), dtype=torch.float32, device=qn[0].device)
        _req(out, "out", torch.float32)
        j = 1 if n_mod > 1 else 0
        plan = cn[0].plan
        if plan is not None:                  # packed image: one masked maximum per video, original columns
            assert all(c.plan is plan for c in cn[:n_mod]) and plan.n_videos == nv
            check(_lib.load().xml_q2c_scores_packed(n_mod, _p(qt[0].data), _p(cn[0].data), _p(qt[j].data),
                                                    _p(cn[j].data), _p(out), out.stride(0), nq, plan.n_tiles,
                                                    _p(plan.slot_ids), _p(cn[0].mask_bits),
                                                    _p(cn[j].mask_bits), hidden, dt_of(qn[0]), _stream()),
                  "xml_q2c_scores_packed")
            return out
        bits = [c.mask_bits for c in cn[:n_mod]]
        if all(c.all_valid for c in cn[:n_mod]):
            mode, bits = 1, [None, None]
        elif all(b is not None or c.all_valid for b, c in zip(bits, cn[:n_mod])):
            mode = 2       # a fully valid modality next to a ragged one: all-ones bit rows
            bits = [b if b is not None else torch.full((nv, 4), -1, dtype=torch.int32, device=out.device) for b in bits]
        else:
            mode, bits = 0, [None, None]
        bits = (bits + [None])[:2] if n_mod == 1 else bits
        check(_lib.load().xml_q2c_scores_tiled(n_mod, _p(qt[0].data), _p(cn[0].data), _p(masks[0]), _p(qt[j].data),
                                               _p(cn[j].data), _p(masks[j]), _p(out), out.stride(0), nq, nv, lpad,
                                               hidden, dt_of(qn[0]), mode, _p(bits[0]), _p(bits[j]), _stream()),
              "xml_q2c_scores_tiled")
        return out
    for m in range(n_mod):
        _req(qn[m], "qn"); _req(cn[m], "cn", qn[m].dtype); _req(masks[m], "mask", torch.float32)
        assert qn[m].shape == qn[0].shape and cn[m].shape == cn[0].shape and tuple(masks[m].shape) == tuple(cn[0].shape[:2])
    nq, hidden = qn[0].shape
    nv, lpad, _ = cn[0].shape
    if out is None:
        out = torch.empty((nq, nv), dtype=torch.float32, device=qn[0].device)
    _req(out, "out", torch.float32)
    j = 1 if n_mod > 1 else 0
    check(_lib.load().xml_q2c_scores_fused(n_mod, _p(qn[0]), _p(cn[0]), _p(masks[0]), _p(qn[j]), _p(cn[j]),
                                           _p(masks[j]), _p(out), out.stride(0), nq, nv, lpad, hidden, dt_of(qn[0]),
                                           _stream()), "xml_q2c_scores_fused")
    return out


def _allow_args(allow, col0, rows, n, device, what):
    """Validate an allow-bit matrix (inference.pack_video_allow's layout) against a (rows, n) score matrix."""
    if not torch.is_tensor(allow) or allow.dtype != torch.int32:
        raise ValueError("%s: allow must be an int32 tensor of bit words (inference.pack_video_allow), got %s"
                         % (what, getattr(allow, "dtype", type(allow).__name__)))
    if allow.device != device:
        raise ValueError("%s: allow is on %s, the scores are on %s" % (what, allow.device, device))
    col0 = int(col0)
    if col0 < 0:
        raise ValueError("%s: col0 must be >= 0, got %d" % (what, col0))
    need = (col0 + n + 31) // 32
    if allow.dim() != 2 or allow.shape[1] < need:
        raise ValueError("%s: allow must be (R, >= %d) words for columns %d .. %d, got %s"
                         % (what, need, col0, col0 + n - 1, tuple(allow.shape)))
    if allow.shape[0] not in (1, rows):
        raise ValueError("%s: allow has %d rows; 1 (shared) or %d (one per score row) expected" % (what, allow.shape[0], rows))
    if allow.stride(1) != 1 or allow.stride(0) < allow.shape[1]:
        allow = allow.contiguous()
    return allow, col0


def topk_rows(scores, k, alpha=0.0, idx_in=None, allow=None, col0=0, return_count=False):
    """K8.  scores (rows, n) f32 -> (values (rows, k) f32 [exp(alpha*s) if alpha], indices (rows, k) int32).
    allow (1 | rows, >= ceil((col0 + n) / 32)) int32 bit words: the top-k of each row's ALLOWED columns only (column c needs
    bit col0 + c); rows with fewer than k allowed columns end in empty slots (index -1, value 0, or -inf when alpha == 0).
    return_count=True: additionally counts (rows,) int32 = min(k, allowed columns)."""
    _req(scores, "scores", torch.float32)
    rows, n = scores.shape
    if idx_in is not None:
        _req(idx_in, "idx_in", torch.int32)
        assert idx_in.shape == scores.shape
    if allow is None and (col0 or return_count):
        raise ValueError("topk_rows: col0 / return_count belong to allow=")
    if allow is not None:
        allow, col0 = _allow_args(allow, col0, rows, n, scores.device, "topk_rows")
    vals = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((rows, k), dtype=torch.int32, device=scores.device)
    lib = _lib.load()
    ws = _workspace(lib.xml_topk_rows_workspace_bytes(rows, n, k), scores.device)      # header contract: caller's scratch
    if allow is not None:
        cnt = torch.empty((rows,), dtype=torch.int32, device=scores.device) if return_count else None
        check(lib.xml_topk_rows_allowed(_p(scores), scores.stride(0), _p(idx_in), _p(allow), allow.stride(0), allow.shape[0],
                                        col0, _p(vals), _p(idx), _p(cnt), rows, n, k, float(alpha), _p(ws), ws.numel(),
                                        _stream()), "xml_topk_rows_allowed")
        return (vals, idx, cnt) if return_count else (vals, idx)
    check(lib.xml_topk_rows(_p(scores), scores.stride(0), _p(idx_in), _p(vals), _p(idx), rows, n, k,
                            float(alpha), _p(ws), ws.numel(), _stream()), "xml_topk_rows")
    return vals, idx


def merge_shard_topk(recv_score, recv_id, k, alpha=0.0):
    """The owner's merge of a sharded pass behind the wire (xml_merge_shard_topk): recv_score / recv_id (world, rows, c)
    -- every shard's local top-c of the same query rows, source rank major -> (values (rows, k), ids (rows, k)) ordered
    like topk_rows (score desc, id asc)."""
    _req(recv_score, "recv_score", torch.float32); _req(recv_id, "recv_id", torch.int32)
    world, rows, c = recv_score.shape
    assert recv_id.shape == recv_score.shape
    vals = torch.empty((rows, k), dtype=torch.float32, device=recv_score.device)
    idx = torch.empty((rows, k), dtype=torch.int32, device=recv_score.device)
    lib = _lib.load()
    ws = _workspace(lib.xml_merge_shard_topk_workspace_bytes(world, rows, c), recv_score.device)
    check(lib.xml_merge_shard_topk(_p(recv_score), _p(recv_id), world, rows, c, int(k), float(alpha), _p(vals), _p(idx), _p(ws),
                                   ws.numel(), _stream()), "xml_merge_shard_topk")
    return vals, idx


MOMENT_SUMM = 8        # XML_MOMENT_SUMM


def convse_rerank(q_lin, feat2, masks, pair_vid, conv_w, l_ref, merged, ksize, softmax=True, zero_skipped=True,
                  pair_w=None, band=None, vid_len=None, out=None):
    """K7.  q_lin / feat2 / masks: lists over modalities (len 1 or 2).
    q_lin[m] (Nq, H); feat2[m] (Nv, Lpad, H); masks[m] (Nv, Lpad) f32; pair_vid (Nq, K) int32;
    conv_w flat f32 [st filters..., ed filters...].  Returns st, ed (Nq, K, Lpad) f32.
    zero_skipped=False leaves the rows of skipped pairs (pair_vid < 0) unwritten -- for callers that never read them
    (the sharded pass: K9 skips pairs of weight 0).
    band = (min_l, max_l) [+ pair_w (Nq, K) f32, the video weights]: also returns summ (Nq, K, 8) f32, the 8 largest banded
    row maxima of every pair (xml_convse_rerank_ex) -- hand it to moment_topk(..., summ=summ), which then reads the rows once.
    vid_len (Nv,) int32: ragged corpora -- valid clips per video; entries l >= vid_len[v] of st / ed are left UNWRITTEN (exact
    zeros of the masked softmax) for moment_topk(..., pair_vid=pair_vid, vid_len=vid_len), which does not read them."""
    n_mod = len(q_lin)
    for m in range(n_mod):
        _req(q_lin[m], "q_lin"); _req(feat2[m], "feat2", q_lin[m].dtype); _req(masks[m], "mask", torch.float32)
    _req(pair_vid, "pair_vid", torch.int32); _req(conv_w, "conv_w", torch.float32)
    nq, hidden = q_lin[0].shape
    nv, lpad, _ = feat2[0].shape
    kpairs = pair_vid.shape[1]
    d = ConvseDesc(nq=nq, nv=nv, kpairs=kpairs, lpad=lpad, l_ref=int(l_ref), hidden=hidden, n_mod=n_mod,
                   merged=int(merged), ksize=int(ksize), softmax=int(bool(softmax)) | (0 if zero_skipped else 2),
                   dt=dt_of(q_lin[0]))
    n_conv = 1 if merged else n_mod
    assert conv_w.numel() == 2 * n_conv * ksize
    lib = _lib.load()
    if out is not None:            # (st, ed) destination tensors of the caller
        st, ed = out
        _req(st, "st", torch.float32); _req(ed, "ed", torch.float32)
        assert tuple(st.shape) == tuple(ed.shape) == (nq, kpairs, lpad)
    else:
        st = torch.empty((nq, kpairs, lpad), dtype=torch.float32, device=pair_vid.device)
        ed = torch.empty_like(st)
    ws = _workspace(lib.xml_convse_rerank_workspace_bytes(ctypes.byref(d)), pair_vid.device)
    if band is not None or vid_len is not None:
        assert softmax, "candidate summaries / unwritten zero tails are those of probabilities"
        if pair_w is not None:
            _req(pair_w, "pair_w", torch.float32)
            assert tuple(pair_w.shape) == (nq, kpairs)
        if vid_len is not None:
            _req(vid_len, "vid_len", torch.int32)
            assert vid_len.numel() == nv
        summ = torch.empty((nq, kpairs, MOMENT_SUMM), dtype=torch.float32, device=pair_vid.device) if band is not None else None
        band = band if band is not None else (0, 1)
        one, sp = n_mod == 1, q_lin[0].dtype is F16S
        inv = lambda t: _p(t.inv) if sp else None          # noqa: E731
        check(lib.xml_convse_rerank_ex(ctypes.byref(d), _p(q_lin[0]), None if one else _p(q_lin[1]), inv(q_lin[0]),
                                       None if one else inv(q_lin[1]), _p(feat2[0]), None if one else _p(feat2[1]),
                                       inv(feat2[0]), None if one else inv(feat2[1]), _p(masks[0]),
                                       None if one else _p(masks[1]), _p(pair_vid), _p(conv_w), _p(pair_w), int(band[0]),
                                       int(band[1]), _p(vid_len), _p(st), _p(ed), _p(summ), _p(ws), ws.numel(), _stream()),
              "xml_convse_rerank_ex")
        return (st, ed, summ) if summ is not None else (st, ed)
    if q_lin[0].dtype is F16S:       # split-f16 rows on both sides: f32-grade similarities on the 16-bit pipe
        one = n_mod == 1
        check(lib.xml_convse_rerank_f16s(ctypes.byref(d), _p(q_lin[0]), None if one else _p(q_lin[1]), _p(q_lin[0].inv),
                                         None if one else _p(q_lin[1].inv), _p(feat2[0]), None if one else _p(feat2[1]),
                                         _p(feat2[0].inv), None if one else _p(feat2[1].inv), _p(masks[0]),
                                         None if one else _p(masks[1]), _p(pair_vid), _p(conv_w), _p(st), _p(ed), _p(ws),
                                         ws.numel(), _stream()), "xml_convse_rerank_f16s")
        return st, ed
    check(lib.xml_convse_rerank(ctypes.byref(d), _p(q_lin[0]), _p(q_lin[1]) if n_mod > 1 else None, _p(feat2[0]),
                                _p(feat2[1]) if n_mod > 1 else None, _p(masks[0]),
                                _p(masks[1]) if n_mod > 1 else None, _p(pair_vid), _p(conv_w), _p(st), _p(ed),
                                _p(ws), ws.numel(), _stream()), "xml_convse_rerank")
    return st, ed


SpanEvidence = collections.namedtuple("SpanEvidence", "video_similarity sub_similarity similarity st_logits ed_logits")


def span_evidence(q_lin, feat2, masks, pair_q, pair_vid, conv_w, l_ref, merged, ksize):
    """What K7 computes on the way to its logits, for P explicit pairs (xml_span_evidence).  q_lin / feat2 / masks as for
    convse_rerank (f32, bf16 or SplitRows); pair_q, pair_vid (P,) int32: pair p = query row pair_q[p] x video row pair_vid[p].
    Returns SpanEvidence of (P, Lpad) f32 rows: the per-stream similarities (unmasked; sub_similarity is None for one-stream
    models), their mean, and the masked start / end LOGITS -- bitwise those of convse_rerank(..., softmax=False) on the same
    pairs.  Pairs with an index out of range come back as zero rows."""
    n_mod = len(q_lin)
    for m in range(n_mod):
        _req(q_lin[m], "q_lin"); _req(feat2[m], "feat2", q_lin[m].dtype); _req(masks[m], "mask", torch.float32)
    _req(pair_q, "pair_q", torch.int32); _req(pair_vid, "pair_vid", torch.int32); _req(conv_w, "conv_w", torch.float32)
    if pair_q.dim() != 1 or pair_q.shape != pair_vid.shape:
        raise ValueError("span_evidence: pair_q and pair_vid must be 1-D and of equal length")
    nq, hidden = q_lin[0].shape
    nv, lpad, _ = feat2[0].shape
    P = pair_q.numel()
    dev = pair_q.device
    n_conv = 1 if merged else n_mod
    assert conv_w.numel() == 2 * n_conv * ksize
    rows = [torch.empty((P, lpad), dtype=torch.float32, device=dev) for _ in range(5)]
    if n_mod == 1:
        rows[1] = None
    if P == 0 or nq == 0:
        for r in rows:
            if r is not None:
                r.zero_()
        return SpanEvidence(*rows)
    d = ConvseDesc(nq=nq, nv=nv, kpairs=1, lpad=lpad, l_ref=int(l_ref), hidden=hidden, n_mod=n_mod, merged=int(merged),
                   ksize=int(ksize), softmax=0, dt=dt_of(q_lin[0]))
    lib = _lib.load()
    ws = _workspace(lib.xml_span_evidence_workspace_bytes(ctypes.byref(d), P), dev)
    one, sp = n_mod == 1, q_lin[0].dtype is F16S
    inv = lambda t: _p(t.inv) if sp else None          # noqa: E731
    check(lib.xml_span_evidence(ctypes.byref(d), _p(q_lin[0]), None if one else _p(q_lin[1]), inv(q_lin[0]),
                                None if one else inv(q_lin[1]), _p(feat2[0]), None if one else _p(feat2[1]), inv(feat2[0]),
                                None if one else inv(feat2[1]), _p(masks[0]), None if one else _p(masks[1]), _p(pair_q),
                                _p(pair_vid), P, _p(conv_w), _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(rows[3]), _p(rows[4]),
                                _p(ws), ws.numel(), _stream()), "xml_span_evidence")
    return SpanEvidence(*rows)


def moment_topk(st, ed, w, l_ref, min_l, max_l, n_out, summ=None, pair_vid=None, vid_len=None):
    """K9/K10.  st, ed (Nq, K, Lpad) f32 probabilities; w (Nq, K) f32 or None.
    summ (Nq, K, 8) f32: the candidate summaries convse_rerank(..., band=(min_l, max_l), pair_w=w) returned for THESE rows.
    pair_vid (Nq, K) int32 + vid_len (Nv,) int32: the rows came from convse_rerank(..., vid_len=vid_len) -- entries beyond a
    video's valid length were not written and are not read.  vid_len=None (full rows): pair_vid is not looked at.
    Returns (scores (Nq, n_out) f32 desc, flat (Nq, n_out) int32 = (r*l_ref + i)*l_ref + j, -1 = empty)."""
    _req(st, "st", torch.float32); _req(ed, "ed", torch.float32)
    if w is not None:
        _req(w, "w", torch.float32)
    nq, kpairs, lpad = st.shape
    if summ is not None:
        _req(summ, "summ", torch.float32)
        assert tuple(summ.shape) == (nq, kpairs, MOMENT_SUMM)
    if vid_len is None:
        pair_vid = None
    else:
        _req(pair_vid, "pair_vid", torch.int32); _req(vid_len, "vid_len", torch.int32)
        assert tuple(pair_vid.shape) == (nq, kpairs)
    sc = torch.empty((nq, n_out), dtype=torch.float32, device=st.device)
    fl = torch.empty((nq, n_out), dtype=torch.int32, device=st.device)
    check(_lib.load().xml_moment_topk_ex(_p(st), _p(ed), _p(w), _p(summ), _p(pair_vid), _p(vid_len), _p(sc), _p(fl), nq, kpairs,
                                         lpad, int(l_ref), int(min_l), int(max_l), int(n_out), _stream()), "xml_moment_topk_ex")
    return sc, fl


def _parts_args(scores, parts, what):
    """Validate a device part table (ingest.PartTable.to(device)) against a (rows, n_parts) score matrix."""
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.XmlHipError("%s: scores must be a tensor on the GPU; the HIP path has no CPU fallback" % what)
    if scores.dtype != torch.float32:
        raise _lib.XmlHipError("%s: scores: expected dtype torch.float32, got %s" % (what, scores.dtype))
    if scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError("%s: scores must be a (rows, n_parts) f32 matrix with unit column stride, got %s strides %s"
                         % (what, tuple(scores.shape), tuple(scores.stride())))
    for name in ("part_video", "group_start"):
        t = getattr(parts, name, None)
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s: parts.%s must be a contiguous 1-D int32 tensor (ingest.PartTable.to(device))" % (what, name))
        if t.device != scores.device:
            raise ValueError("%s: parts.%s is on %s, the scores are on %s" % (what, name, t.device, scores.device))
    n_parts, n_videos = int(parts.part_video.numel()), int(parts.group_start.numel()) - 1
    if n_videos < 1 or n_parts < n_videos:
        raise ValueError("%s: a part table of %d videos in %d parts" % (what, n_videos, n_parts))
    if scores.shape[1] != n_parts:
        raise ValueError("%s: scores have %d columns, the part table has %d index rows" % (what, scores.shape[1], n_parts))
    if scores.shape[0] and scores.stride(0) < n_parts:
        raise ValueError("%s: score row stride %d < %d columns" % (what, scores.stride(0), n_parts))
    return n_parts, n_videos


def group_best_allow(scores, parts, video_allow=None):
    """The fold of a parts index between K6 and K8 (xml_group_best_allow).  scores (rows, n_parts) f32 (row stride >= n_parts);
    parts: device part table (part_video (n_parts,) / group_start (n_videos + 1,) int32); video_allow None or
    (1 | rows, >= ceil(n_videos / 32)) int32 words over SOURCE videos (inference.pack_video_allow).
    -> (rows, ceil(n_parts / 32)) int32 words over index rows: bit p set iff p is its video's best part for that row (maximum,
    ties to the lowest row, NaN never wins) and the video is allowed -- topk_rows(scores, k, allow=) of it ranks videos."""
    n_parts, n_videos = _parts_args(scores, parts, "group_best_allow")
    rows = scores.shape[0]
    allow_ld = allow_rows = 0
    if video_allow is not None:
        video_allow, _ = _allow_args(video_allow, 0, rows, n_videos, scores.device, "group_best_allow")
        allow_ld, allow_rows = video_allow.stride(0), video_allow.shape[0]
    out = torch.empty((rows, (n_parts + 31) // 32), dtype=torch.int32, device=scores.device)
    check(_lib.load().xml_group_best_allow(_p(scores), scores.stride(0) if rows else n_parts, rows, n_parts,
                                           _p(parts.part_video), _p(parts.group_start), n_videos, _p(video_allow), allow_ld,
                                           allow_rows, _p(out), out.stride(0), _stream()), "xml_group_best_allow")
    return out


def best_part_rows(scores, parts, video):
    """scores (rows, n_parts) f32, video (rows,) int32 SOURCE video per row -> (rows,) int32 index row of that video's best
    part (group_best_allow's rule), -1 for an id outside [0, n_videos)  (xml_best_part_rows)."""
    n_parts, n_videos = _parts_args(scores, parts, "best_part_rows")
    rows = scores.shape[0]
    if not torch.is_tensor(video) or video.dtype != torch.int32 or video.dim() != 1 or video.numel() != rows:
        raise ValueError("best_part_rows: video must be a (%d,) int32 tensor of source-video ids, got %s %s"
                         % (rows, getattr(video, "dtype", type(video).__name__), tuple(getattr(video, "shape", ()))))
    if video.device != scores.device:
        raise ValueError("best_part_rows: video is on %s, the scores are on %s" % (video.device, scores.device))
    video = video.contiguous()
    out = torch.empty((rows,), dtype=torch.int32, device=scores.device)
    check(_lib.load().xml_best_part_rows(_p(scores), scores.stride(0) if rows else n_parts, rows, _p(parts.group_start),
                                         n_videos, _p(video), _p(out), _stream()), "xml_best_part_rows")
    return out


def moments_decode(scores, flat=None, top_idx=None, row_vid=None, meta2vid=None, l_ref=0, clip_length=1.5, seconds=True,
                   n=None, out=None, out_count=None, part_offset=None):
    """K10.  (flat (Nq, n) int32, scores (Nq, n) f32) -> records (Nq, n, 4) int32 = xml_moment {vid i32, st f32, ed f32,
    score f32} (view the host copy as results.MOMENT_DTYPE) and count (Nq,) int32.
    top_idx (Nq, K) int32: video of local rank r; row_vid (Nq,) int32: the one video of each query (SVMR); meta2vid (Nv,)
    int32: meta index -> video2idx value.  flat=None: the VR list of top_idx[:, :n] / scores[:, :n].
    out / out_count: write into these rows of a larger result buffer ((Nq, >= n, 4) int32 / (Nq,) int32 views).
    part_offset (index rows,) int32 (a parts index: PartTable.part_offset on the device): the row's first clip in its source
    video is added to st_idx / ed_idx before the float conversion (xml_moments_decode_parts); meta2vid should then be
    PartTable.meta2vid(...), index row -> source video id."""
    _req(scores, "scores", torch.float32)
    nq = scores.shape[0]
    n = scores.shape[1] if n is None else int(n)
    src = flat if flat is not None else top_idx
    _req(src, "flat / top_idx", torch.int32)
    assert src.shape[0] == nq and src.stride(0) == scores.stride(0) and n <= scores.shape[1]
    k = 0
    if flat is not None and top_idx is not None:
        _req(top_idx, "top_idx", torch.int32)
        k = top_idx.shape[1]
    for t, name in ((row_vid, "row_vid"), (meta2vid, "meta2vid")):
        if t is not None:
            _req(t, name, torch.int32)
    if out is None:
        out = torch.empty((nq, n, 4), dtype=torch.int32, device=scores.device)
    if out_count is None:
        out_count = torch.empty((nq,), dtype=torch.int32, device=scores.device)
    assert out.dtype == torch.int32 and out.shape[0] == nq and out.shape[2] == 4 and out.stride(2) == 1 and out.stride(1) == 4
    assert out_count.dtype == torch.int32 and out_count.is_contiguous() and out_count.numel() == nq
    if part_offset is not None:
        _req(part_offset, "part_offset", torch.int32)
        if part_offset.dim() != 1 or (meta2vid is not None and meta2vid.numel() != part_offset.numel()):
            raise ValueError("moments_decode: part_offset must be (index rows,) int32, one entry per entry of meta2vid; got %s"
                             % (tuple(part_offset.shape),))
        check(_lib.load().xml_moments_decode_parts(_p(flat), _p(scores), _p(top_idx), _p(row_vid), _p(meta2vid),
                                                   _p(part_offset), nq, n, scores.stride(0), k, int(l_ref),
                                                   float(clip_length), 1 if seconds else 0, _p(out), out.stride(0) // 4,
                                                   _p(out_count), _stream()), "xml_moments_decode_parts")
        return out, out_count
    check(_lib.load().xml_moments_decode(_p(flat), _p(scores), _p(top_idx), _p(row_vid), _p(meta2vid), nq, n,
                                         scores.stride(0), k, int(l_ref), float(clip_length), 1 if seconds else 0,
                                         _p(out), out.stride(0) // 4, _p(out_count), _stream()), "xml_moments_decode")
    return out, out_count


def nms_moments(records, count, by_video, thd, scale=1.0, max_before=None, max_after=100, want_records=True,
                want_index=True, out=None, out_index=None, out_count=None):
    """K11: greedy temporal NMS of K10's records on the device (xml_nms_moments; the semantics of postproc.nms_batched).
    records (Nq, n, 4) int32 = xml_moment rows (row stride >= n records: a view of a wider buffer is fine), count (Nq,) int32
    valid prefix per row or None (whole rows); by_video: True = filter_vcmr_by_nms (NMS per video, merged by score), False =
    post_processing_svmr_nms (the row is one video).  scale: float64 factor on st / ed (clip_length for records in clip units).
    max_before (default n): only the first min(count, max_before) entries of a row take part.
    -> (records (Nq, max_after, 4) int32 or None, index (Nq, max_after) int32 into each input row or None, count (Nq,) int32);
    beyond a row's count the records are {-1, 0, 0, 0} and the indices -1.  out / out_index / out_count: destinations to use
    instead of new tensors (rows of a larger buffer; at least max_after wide)."""
    if not isinstance(records, torch.Tensor) or not records.is_cuda:
        raise _lib.XmlHipError("records: tensor must live on the GPU; the HIP path has no CPU fallback")
    if records.dtype != torch.int32 or records.dim() != 3 or records.shape[2] != 4 or records.stride(2) != 1 \
            or records.stride(1) != 4 or records.stride(0) % 4 != 0:
        raise _lib.XmlHipError("records: expected (Nq, n, 4) int32 xml_moment rows, got %s %s strides %s"
                               % (records.dtype, tuple(records.shape), tuple(records.stride())))
    nq, n = records.shape[0], records.shape[1]
    if count is not None:
        _req(count, "count", torch.int32)
        assert count.numel() == nq
    max_before = n if max_before is None else int(max_before)
    max_after = int(max_after)
    width = max(max_after, 1)
    dev = records.device
    if out is None and want_records:
        out = torch.empty((nq, width, 4), dtype=torch.int32, device=dev)
    if out_index is None and want_index:
        out_index = torch.empty((nq, width), dtype=torch.int32, device=dev)
    if out_count is None:
        out_count = torch.empty((nq,), dtype=torch.int32, device=dev)
    if out is not None:
        assert out.is_cuda and out.dtype == torch.int32 and out.dim() == 3 and out.shape[0] == nq and out.shape[2] == 4 \
            and out.stride(2) == 1 and out.stride(1) == 4 and out.stride(0) % 4 == 0 and out.shape[1] >= max_after
    if out_index is not None:
        assert out_index.is_cuda and out_index.dtype == torch.int32 and out_index.dim() == 2 and out_index.shape[0] == nq \
            and out_index.stride(1) == 1 and out_index.shape[1] >= max_after
    assert out_count.is_cuda and out_count.dtype == torch.int32 and out_count.is_contiguous() and out_count.numel() == nq
    if nq:
        check(_lib.load().xml_nms_moments(_p(records), records.stride(0) // 4, _p(count), nq, n, 1 if by_video else 0,
                                          float(thd), float(scale), max_before, max_after, _p(out),
                                          out.stride(0) // 4 if out is not None else 0, _p(out_index),
                                          out_index.stride(0) if out_index is not None else 0, _p(out_count), _stream()),
              "xml_nms_moments")
    return out, out_index, out_count


EVAL_TASKS = {"VCMR": 0, "SVMR": 1, "VR": 2}


def eval_moments(rec, count, task, gt, scale=1.0, max_pred=100, iou_thds=(0.5, 0.7), topks=(1, 5, 10, 100),
                 first_hit=None, hits=None, rows=None):
    """K12: the recall counters of K10 / K11 records on the device (xml_eval_moments; the semantics of
    evaluate.eval_by_task_type on the array path).
    rec (Nq, n, 4) int32 = xml_moment rows (row stride >= n records: a view of a wider buffer is fine), count (Nq,) int32 valid
    prefix per row or None (whole rows); task "VCMR" | "SVMR" | "VR"; gt: the ground truth of the same rows in the same order --
    an evaluate.DeviceGroundTruth, or anything with gt_vid (Nq,) int32, gt_ts (Nq, n_ts, 2) f32, n_gt (Nq,) int32 and
    desc_type (Nq,) int32 or None.  scale: float64 factor on st / ed (clip_length for SVMR records in clip units).
    -> (first_hit (Nq, n_thd) int32, hits (4, n_thd, n_k) int32, rows (4,) int32) on the device; n_thd is 1 for "VR".
    first_hit / hits / rows: destinations to use instead of new tensors."""
    if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
        raise _lib.XmlHipError("rec: tensor must live on the GPU; the HIP path has no CPU fallback")
    if rec.dtype != torch.int32 or rec.dim() != 3 or rec.shape[2] != 4 or rec.stride(2) != 1 or rec.stride(1) != 4 \
            or rec.stride(0) % 4 != 0:
        raise _lib.XmlHipError("rec: expected (Nq, n, 4) int32 xml_moment rows, got %s %s strides %s"
                               % (rec.dtype, tuple(rec.shape), tuple(rec.stride())))
    if task not in EVAL_TASKS:
        raise ValueError("task: expected one of %s, got %r" % (sorted(EVAL_TASKS), task))
    nq, n = rec.shape[0], rec.shape[1]
    if count is not None:
        _req(count, "count", torch.int32)
        assert count.numel() == nq
    _req(gt.gt_vid, "gt.gt_vid", torch.int32)
    _req(gt.gt_ts, "gt.gt_ts", torch.float32)
    _req(gt.n_gt, "gt.n_gt", torch.int32)
    if gt.desc_type is not None:
        _req(gt.desc_type, "gt.desc_type", torch.int32)
        assert gt.desc_type.numel() == nq
    assert gt.gt_vid.numel() == nq and gt.n_gt.numel() == nq and gt.gt_ts.dim() == 3 and gt.gt_ts.shape[0] == nq \
        and gt.gt_ts.shape[2] == 2, "the ground truth holds one row per record row"
    n_ts = gt.gt_ts.shape[1]
    n_thd = 1 if task == "VR" else len(iou_thds)
    thd = (ctypes.c_float * max(len(iou_thds), 1))(*[float(x) for x in iou_thds])
    ks = (ctypes.c_int32 * len(topks))(*[int(k) for k in topks])
    dev = rec.device
    if first_hit is None:
        first_hit = torch.empty((nq, n_thd), dtype=torch.int32, device=dev)
    if hits is None:
        hits = torch.empty((4, n_thd, len(topks)), dtype=torch.int32, device=dev)
    if rows is None:
        rows = torch.empty((4,), dtype=torch.int32, device=dev)
    for t, name, numel in ((first_hit, "first_hit", nq * n_thd), (hits, "hits", 4 * n_thd * len(topks)), (rows, "rows", 4)):
        _req(t, name, torch.int32)
        assert t.numel() == numel, "%s: expected %d elements, got %d" % (name, numel, t.numel())
    if nq == 0:                     # (the entry leaves its outputs untouched: no row, no hit)
        hits.zero_()
        rows.zero_()
        return first_hit, hits, rows
    check(_lib.load().xml_eval_moments(_p(rec), rec.stride(0) // 4, _p(count), nq, n, EVAL_TASKS[task], float(scale),
                                       int(max_pred), _p(gt.gt_vid), _p(gt.gt_ts), n_ts, _p(gt.n_gt), _p(gt.desc_type),
                                       ctypes.cast(thd, ctypes.c_void_p), len(iou_thds) if task != "VR" else 1,
                                       ctypes.cast(ks, ctypes.c_void_p), len(topks), _p(first_hit), _p(hits), _p(rows),
                                       _stream()), "xml_eval_moments")
    return first_hit, hits, rows


# ---- exact-rank mode (bf16 K6 as a filter in front of f32 scores; include/xmlhip.h "Exact-rank mode") --------------------
def round_bf16_rows_err(y):
    """y (..., d) f32 L2-normalised rows -> (yb bf16 = rne(y), err (...) f32 = ||y - yb||_2 per row)."""
    _req(y, "y", torch.float32)
    d = y.shape[-1]
    yb = torch.empty(y.shape, dtype=torch.bfloat16, device=y.device)
    err = torch.empty(y.shape[:-1], dtype=torch.float32, device=y.device)
    check(_lib.load().xml_round_bf16_rows_err(_p(y), _p(yb), _p(err), y.numel() // d, d, _stream()),
          "xml_round_bf16_rows_err")
    return yb, err


def q2c_rescore(qn, cn, masks, pair_vid):
    """Video-level scores of the listed pairs only.  qn / cn / masks: lists over modalities of (Nq, H), (Nv, Lpad, H)
    row-major L2-normalised, (Nv, Lpad) f32; pair_vid (Nq, K) int32 -> (Nq, K) f32 (-inf for ids outside [0, Nv))."""
    n_mod = len(qn)
    for m in range(n_mod):
        _req(qn[m], "qn"); _req(cn[m], "cn", qn[m].dtype); _req(masks[m], "mask", torch.float32)
        assert cn[m].shape == cn[0].shape and qn[m].shape == qn[0].shape and tuple(masks[m].shape) == tuple(cn[0].shape[:2])
    _req(pair_vid, "pair_vid", torch.int32)
    nq, hidden = qn[0].shape
    nv, lpad, _ = cn[0].shape
    kp = pair_vid.shape[1]
    assert pair_vid.shape[0] == nq
    out = torch.empty((nq, kp), dtype=torch.float32, device=pair_vid.device)
    lib = _lib.load()
    ws = _workspace(lib.xml_q2c_rescore_workspace_bytes(nq, nv, kp), pair_vid.device)
    j = 1 if n_mod > 1 else 0
    check(lib.xml_q2c_rescore(n_mod, _p(qn[0]), _p(qn[j]), _p(cn[0]), _p(cn[j]), _p(masks[0]), _p(masks[j]), _p(pair_vid),
                              _p(out), nq, nv, kp, lpad, hidden, dt_of(qn[0]), _p(ws), ws.numel(), _stream()),
          "xml_q2c_rescore")
    return out


def exact_certificate(filter_scores, top_val, eq, ec, slack, alpha, outside):
    """Per-query certificate of the exact-rank filter.  filter_scores (Nq, M) f32 desc (bf16 pass); top_val (Nq, K) f32 desc,
    raw re-scored values -- turned into exp(alpha * s) IN PLACE; eq: list of (Nq,) f32 per modality; ec: list of floats.
    Returns (fail (Nq,) int32, eps (Nq,) f32, thr (Nq,) f32 = raw T_k - eps, n_fail (1,) int32 device tensor)."""
    _req(filter_scores, "filter_scores", torch.float32); _req(top_val, "top_val", torch.float32)
    n_mod = len(eq)
    for e in eq:
        _req(e, "eq", torch.float32)
    nq, m = filter_scores.shape
    k = top_val.shape[1]
    dev = top_val.device
    fail = torch.empty((nq,), dtype=torch.int32, device=dev)
    eps = torch.empty((nq,), dtype=torch.float32, device=dev)
    thr = torch.empty((nq,), dtype=torch.float32, device=dev)
    n_fail = torch.zeros((1,), dtype=torch.int32, device=dev)
    j = 1 if n_mod > 1 else 0
    check(_lib.load().xml_exact_certificate(_p(filter_scores), m, _p(top_val), k, _p(eq[0]), _p(eq[j]), float(ec[0]),
                                            float(ec[j]), n_mod, float(slack), float(alpha), int(bool(outside)), _p(fail),
                                            _p(eps), _p(thr), _p(n_fail), nq, _stream()), "xml_exact_certificate")
    return fail, eps, thr, n_fail


# ---- packed variable-length sequences (the query encoder without its padding rows) -------------------------------------
def pack_plan(mask, rows=None):
    """Packing plan of a padded batch.  mask (n, lq) f32 -> (cu_seqlens (n + 1,) int32, src_row (n * lq,) int32, rows);
    rows = -1 when some mask row is not a non-empty prefix of ones.  (One 4-byte read-back: the launch shapes of the
    packed kernels depend on rows.)
    rows (host int): the caller KNOWS the number of valid tokens -- it built the masks on the host, like the reference's
    collate (start_end_dataset.py:346-370) -- and vouches that every mask row is a non-empty prefix of ones: no read-back, the
    pass stays asynchronous (the read-back is a host synchronisation: ~0.6 ms of idle device per 10 000-query pass)."""
    _req(mask, "mask", torch.float32)
    n, lq = mask.shape
    cu = torch.empty(n + 1, dtype=torch.int32, device=mask.device)
    src = torch.empty(n * lq, dtype=torch.int32, device=mask.device)
    status = torch.empty(2, dtype=torch.int32, device=mask.device)
    check(_lib.load().xml_pack_plan(_p(mask), n, lq, _p(cu), _p(src), _p(status), _stream()), "xml_pack_plan")
    if rows is not None:
        rows = int(rows)
        if not n <= rows <= n * lq:
            raise ValueError("pack_plan: %d valid tokens cannot be right for %d sequences of <= %d" % (rows, n, lq))
        return cu, src, rows
    return cu, src, int(status[0].item())


def linear_ln_relu_pos_packed(x, src_row, rows, lq, ln_in_g, ln_in_b, w, b, pos, ln_pos_g, ln_pos_b):
    """K1+K2 on packed tokens: x (n * lq, d_in) f32 or w.dtype is the PADDED batch, packed token i = x[src_row[i]] with
    positional row pos[src_row[i] % lq] -> (rows, hidden) w.dtype."""
    _req(x, "x"); _req(src_row, "src_row", torch.int32); _req(w, "w"); _req(pos, "pos", act_dtype(w.dtype))
    for t, nm in ((ln_in_g, "ln_in_g"), (ln_in_b, "ln_in_b"), (b, "b"), (ln_pos_g, "ln_pos_g"), (ln_pos_b, "ln_pos_b")):
        _req(t, nm, torch.float32)
    d_in, hidden = x.shape[1], w.shape[0]
    assert w.shape[1] == d_in and pos.shape[0] >= lq and pos.shape[1] == hidden and src_row.numel() >= rows
    lib = _lib.load()
    dt = dt_of(w)
    y = torch.empty((rows, hidden), dtype=act_dtype(w.dtype), device=x.device)
    ws = _workspace(lib.xml_linear_ln_relu_pos_packed_workspace_bytes(rows, d_in, hidden, dt), x.device)
    check(lib.xml_linear_ln_relu_pos_packed(_p(x), dt_of(x), _p(src_row), int(lq), _p(ln_in_g), _p(ln_in_b), _p(w), _p(b),
                                            _p(pos), _p(ln_pos_g), _p(ln_pos_b), _p(y), rows, d_in, hidden, dt, _p(ws),
                                            ws.numel(), _stream()), "xml_linear_ln_relu_pos_packed")
    return y


def attention_block_varlen(x, cu_seqlens, n, max_len, wqkv, bqkv, wo, bo, ln_g, ln_b, n_heads):
    """K3+K4 on packed tokens.  x (rows, H); cu_seqlens (n + 1,) int32 -> (rows, H)."""
    _req(x, "x"); _req(cu_seqlens, "cu_seqlens", torch.int32); _req_w(wqkv, "wqkv", x); _req_w(wo, "wo", x)
    for t, nm in ((bqkv, "bqkv"), (bo, "bo"), (ln_g, "ln_g"), (ln_b, "ln_b")):
        _req(t, nm, torch.float32)
    rows, hidden = x.shape
    assert cu_seqlens.numel() == n + 1
    lib = _lib.load()
    dt = dt_of(wqkv)
    y = torch.empty_like(x)
    ws = _workspace(lib.xml_attention_block_varlen_workspace_bytes(rows, hidden, dt), x.device)
    check(lib.xml_attention_block_varlen(_p(x), _p(cu_seqlens), _p(wqkv), _p(bqkv), _p(wo), _p(bo), _p(ln_g), _p(ln_b), _p(y),
                                         rows, n, int(max_len), hidden, n_heads, dt, _p(ws), ws.numel(), _stream()),
          "xml_attention_block_varlen")
    return y


def modular_pool_varlen(enc, cu_seqlens, n, max_len, w_m, return_att=False):
    """K5 on packed tokens.  enc (rows, H); w_m (n_mod, H) f32 -> (n_mod, n, H).
    return_att: -> (pooled, att (n, max_len, n_mod) f32) in the PADDED layout, 0 beyond every query's own tokens."""
    _req(enc, "enc"); _req(cu_seqlens, "cu_seqlens", torch.int32); _req(w_m, "w_m", torch.float32)
    hidden = enc.shape[1]
    n_mod = w_m.shape[0]
    out = torch.empty((n_mod, n, hidden), dtype=enc.dtype, device=enc.device)
    if return_att:
        att = torch.empty((n, int(max_len), n_mod), dtype=torch.float32, device=enc.device)
        check(_lib.load().xml_modular_pool_att_varlen(_p(enc), _p(cu_seqlens), _p(w_m), _p(out), _p(att), n, int(max_len),
                                                      hidden, n_mod, dt_of(enc), _stream()), "xml_modular_pool_att_varlen")
        return out, att
    check(_lib.load().xml_modular_pool_varlen(_p(enc), _p(cu_seqlens), _p(w_m), _p(out), n, int(max_len), hidden, n_mod,
                                              dt_of(enc), _stream()), "xml_modular_pool_varlen")
    return out


def select_ge_rows(scores, thr, cap=None, allow=None, col0=0):
    """Columns of every row of scores (rows, n) f32 that reach thr (rows,) f32.  cap None -> counts (rows,) int32;
    else -> (idx (rows, cap) int32 filled with -1 beyond each row's count, counts).
    allow / col0 (as in topk_rows): only allowed columns are selected or counted."""
    _req(scores, "scores", torch.float32); _req(thr, "thr", torch.float32)
    rows, n = scores.shape
    if allow is None and col0:
        raise ValueError("select_ge_rows: col0 belongs to allow=")
    if allow is not None:
        allow, col0 = _allow_args(allow, col0, rows, n, scores.device, "select_ge_rows")
    cnt = torch.empty((rows,), dtype=torch.int32, device=scores.device)
    idx = None
    if cap is not None:
        idx = torch.full((rows, int(cap)), -1, dtype=torch.int32, device=scores.device)
    if allow is not None:
        check(_lib.load().xml_select_ge_rows_allowed(_p(scores), scores.stride(0), _p(thr), _p(allow), allow.stride(0),
                                                     allow.shape[0], col0, _p(idx), int(cap or 0), _p(cnt), rows, n,
                                                     _stream()), "xml_select_ge_rows_allowed")
    else:
        check(_lib.load().xml_select_ge_rows(_p(scores), scores.stride(0), _p(thr), _p(idx), int(cap or 0), _p(cnt), rows, n,
                                             _stream()), "xml_select_ge_rows")
    return cnt if idx is None else (idx, cnt)


# ---- split-f16 forms (XML_F16S; include/xmlhip.h "Exact-rank mode on the 16-bit pipe") ------------------------------------
def pack_weights_f16s(w_f32):
    """(n, k) f32 weight -> SplitWeight ((n, 3k) f16 [hi | hi | lo] + scale trailer)."""
    _req(w_f32, "w", torch.float32)
    n, k = w_f32.shape
    lib = _lib.load()
    data = torch.empty(int(lib.xml_pack_weights_f16s_bytes(n, k)), dtype=torch.uint8, device=w_f32.device)
    check(lib.xml_pack_weights_f16s(_p(w_f32), _p(data), n, k, _stream()), "xml_pack_weights_f16s")
    return SplitWeight(data, n, k)


def split_f16_rows(x, fixed_log2=None, want_hi=False, want_err=False):
    """x (..., k) f32 -> SplitRows [, hi plane (..., k) torch.float16] [, err (...) f32 = || x - hi / S ||_2 per row].
    fixed_log2 None: one power-of-two scale per row (row maximum -> [2^13, 2^14)); an int: that scale for every row
    (F16_UNIT_LOG2 for unit-norm rows -- what K6 / the re-score expect)."""
    _req(x, "x", torch.float32)
    k = x.shape[-1]
    rows = x.numel() // k
    data = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    inv = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    hi = torch.empty(x.shape, dtype=torch.float16, device=x.device) if want_hi else None
    err = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if want_err else None
    check(_lib.load().xml_split_f16_rows(_p(x), _p(data), _p(inv), _p(hi), _p(err), rows, k,
                                         -1 if fixed_log2 is None else int(fixed_log2), _stream()), "xml_split_f16_rows")
    out = (SplitRows(data, inv),)
    if want_hi:
        out += (hi,)
    if want_err:
        out += (err,)
    return out[0] if len(out) == 1 else out


def unsplit_f16_rows(sr):
    """SplitRows -> f32 rows (hi + lo) / scale (tests, the CPU baseline's view of a split index)."""
    k = sr.shape[-1]
    x = torch.empty(sr.shape, dtype=torch.float32, device=sr.device)
    check(_lib.load().xml_unsplit_f16_rows(_p(sr.data), _p(sr.inv), _p(x), sr.data.numel() // k, k, _stream()),
          "xml_unsplit_f16_rows")
    return x


# ---- in-place index updates (include/xmlhip.h "In-place updates of a resident index"; inference.MutableCorpusIndex) ---------
def _second(n_mod):
    """The _b operand of an entry out of a per-modality list: the address of its second tensor, NULL with one modality."""
    return (lambda t: _p(t[1])) if n_mod == 2 else (lambda t: None)


def _batch_sides(what, f1, f2, masks, n_mod, hidden, dtype):
    """Checks the per-modality (b, lb, H) / (b, lb, H) / (b, lb) batch operands of a put entry; returns (b, lb)."""
    if not (len(f1) == len(f2) == len(masks) == n_mod):
        raise _lib.XmlHipError("%s: the batch holds %d modalities, the index %d" % (what, len(f1), n_mod))
    b, lb = int(f1[0].shape[0]), int(f1[0].shape[1])
    for m in range(n_mod):
        _req(f1[m], "f1", dtype); _req(f2[m], "f2", dtype); _req(masks[m], "mask", torch.float32)
        if tuple(f1[m].shape) != (b, lb, hidden) or tuple(f2[m].shape) != (b, lb, hidden) or tuple(masks[m].shape) != (b, lb):
            raise _lib.XmlHipError("%s: f1 / f2 (b, lb, H) and mask (b, lb) of one batch expected" % what)
    return b, lb


def _slot_records(what, slots, ids, b):
    _req(slots, "slots", torch.int32)
    if slots.numel() != b or (ids is not None and (_req(ids, "ids", torch.int32).numel() != b)):
        raise _lib.XmlHipError("%s: one slot (and id) per video of the batch" % what)


def _codes_tiles(what, codes):
    """Checks the (2 * n_tiles, 8) int32 code table of a packed image; returns n_tiles."""
    _req(codes, "codes", torch.int32)
    if codes.dim() != 2 or codes.shape[1] != 8 or codes.shape[0] % 2 or not codes.shape[0]:
        raise _lib.XmlHipError("%s: codes (2 * n_tiles, 8) int32 expected" % what)
    return int(codes.shape[0]) // 2


def _k6_side(what, k6, tiled, cap, lpad, hidden, dtype, image):
    """Checks one modality's K6 operand of a per-slot index (`image`: what the messages call it); returns its buffer."""
    if isinstance(k6, TiledRows) != tiled:
        raise _lib.XmlHipError("%s: the %ss of the modalities differ in layout" % (what, image))
    d = k6.data if tiled else k6
    _req(d, "k6", dtype)
    if tiled:
        if k6.shape != (cap, lpad, hidden) or lpad != 128 or d.numel() != q2c_tiled_numel(cap * lpad, hidden, d.dtype):
            raise _lib.XmlHipError("%s: the tile image does not hold (capacity, 128, H) rows" % what)
    elif tuple(d.shape) != (cap, lpad, hidden):
        raise _lib.XmlHipError("%s: row-major %s of shape %s expected" % (what, image, (cap, lpad, hidden)))
    return d


def _index_sides(k6, feat2, imask, bits):
    """Checks the per-modality index tensors of the two update entries; returns (capacity, lpad, hidden, tiled, k6 buffers)."""
    n_mod = len(feat2)
    if n_mod not in (1, 2) or not (len(k6) == len(imask) == len(bits) == n_mod):
        raise _lib.XmlHipError("index update: 1 or 2 modalities, the same number of k6 / feat2 / mask / bits tensors")
    cap, lpad, hidden = feat2[0].shape
    tiled = isinstance(k6[0], TiledRows)
    data = []
    for m in range(n_mod):
        _req(feat2[m], "feat2", feat2[0].dtype); _req(imask[m], "mask", torch.float32); _req(bits[m], "bits", torch.int32)
        if tuple(feat2[m].shape) != (cap, lpad, hidden) or tuple(imask[m].shape) != (cap, lpad) or tuple(bits[m].shape) != (cap, 4):
            raise _lib.XmlHipError("index update: feat2 (capacity, lpad, H), mask (capacity, lpad), bits (capacity, 4) expected")
        data.append(_k6_side("index update", k6[m], tiled, cap, lpad, hidden, feat2[0].dtype, "K6 operand"))
    return int(cap), int(lpad), int(hidden), tiled, data


def _index_state(vlen, live, cap, slot_ids=None):
    _req(vlen, "vlen", torch.int32); _req(live, "live", torch.int32)
    if vlen.numel() != cap or live.numel() != (cap + 31) // 32:
        raise _lib.XmlHipError("index update: vlen (capacity,) and live (ceil(capacity / 32),) int32 expected")
    if slot_ids is not None:
        _req(slot_ids, "slot_ids", torch.int32)
        if slot_ids.numel() != cap:
            raise _lib.XmlHipError("index update: slot_ids (capacity,) int32 expected")


def index_put_rows(f1, f2, masks, slots, ids, k6, feat2, imask, bits, vlen, slot_ids, live, l_ref):
    """xml_index_put_rows: one encoded context batch into its slots of a fixed-capacity index, one launch, nothing read back.
    f1 / f2 / masks: per-modality lists of the batch's (b, lb, H), (b, lb, H), (b, lb) f32 tensors; slots (b,) int32 device,
    DISTINCT and in [0, capacity) (the caller's slot table guarantees both); ids (b,) int32 device or None (the slot number).
    k6 / feat2 / imask / bits: per-modality lists of the index's K6 operand (TiledRows or (capacity, lpad, H)), feat2, f32 mask
    and (capacity, 4) mask-bit words; vlen / slot_ids (capacity,) int32, live (ceil(capacity / 32),) int32."""
    cap, lpad, hidden, tiled, data = _index_sides(k6, feat2, imask, bits)
    _index_state(vlen, live, cap, slot_ids)
    n_mod = len(feat2)
    b, lb = _batch_sides("index_put_rows", f1, f2, masks, n_mod, hidden, feat2[0].dtype)
    _slot_records("index_put_rows", slots, ids, b)
    sec = _second(n_mod)
    check(_lib.load().xml_index_put_rows(
        n_mod, _p(f1[0]), _p(f2[0]), _p(masks[0]), sec(f1), sec(f2), sec(masks), _p(slots), _p(ids), b, lb,
        _p(data[0]), _p(feat2[0]), _p(imask[0]), _p(bits[0]), sec(data), sec(feat2), sec(imask), sec(bits),
        _p(vlen), _p(slot_ids), _p(live), cap, lpad, int(l_ref), hidden, dt_of(feat2[0]), int(tiled), _stream()),
        "xml_index_put_rows")


def index_clear_rows(slots, imask, bits, vlen, live, l_ref):
    """xml_index_clear_rows: free the DISTINCT slots (n,) int32 device -- live bits cleared, mask rows and mask bits zeroed,
    vlen = l_ref; one launch, nothing read back."""
    n_mod = len(imask)
    if n_mod not in (1, 2) or len(bits) != n_mod:
        raise _lib.XmlHipError("index_clear_rows: 1 or 2 modalities")
    cap, lpad = imask[0].shape
    for m in range(n_mod):
        _req(imask[m], "mask", torch.float32); _req(bits[m], "bits", torch.int32)
        if tuple(imask[m].shape) != (cap, lpad) or tuple(bits[m].shape) != (cap, 4):
            raise _lib.XmlHipError("index_clear_rows: mask (capacity, lpad) and bits (capacity, 4) expected")
    _index_state(vlen, live, cap)
    _req(slots, "slots", torch.int32)
    sec = _second(n_mod)
    check(_lib.load().xml_index_clear_rows(n_mod, _p(slots), int(slots.numel()), _p(imask[0]), _p(bits[0]), sec(imask), sec(bits),
                                           _p(vlen), _p(live), int(cap), int(lpad), int(l_ref), _stream()),
          "xml_index_clear_rows")


# ---- the same on the packed K6 image (include/xmlhip_index.h; MutableCorpusIndex(tiles=N)) ------------------------------------
def _packed_sides(k6, feat2, imask, bits, codes):
    """Checks the index tensors of the two packed update entries; returns (capacity, hidden, n_tiles, k6 buffers or None)."""
    n_mod = len(imask)
    if n_mod not in (1, 2) or len(bits) != n_mod or (k6 is not None and not (len(k6) == len(feat2) == n_mod)):
        raise _lib.XmlHipError("packed index update: 1 or 2 modalities, the same number of k6 / feat2 / mask / bits tensors")
    n_tiles, cap = _codes_tiles("packed index update", codes), int(imask[0].shape[0])
    hidden, data = None, None
    for m in range(n_mod):
        _req(imask[m], "mask", torch.float32); _req(bits[m], "bits", torch.int32)
        if tuple(imask[m].shape) != (cap, 128) or tuple(bits[m].shape) != (2 * n_tiles, 4):
            raise _lib.XmlHipError("packed index update: mask (capacity, 128) and bits (2 * n_tiles, 4) expected")
    if k6 is not None:
        hidden, data = int(feat2[0].shape[2]), []
        for m in range(n_mod):
            _req(feat2[m], "feat2", feat2[0].dtype)
            if tuple(feat2[m].shape) != (cap, 128, hidden) or not isinstance(k6[m], TiledRows):
                raise _lib.XmlHipError("packed index update: feat2 (capacity, 128, H) and a TiledRows K6 operand expected")
            d = k6[m].data
            _req(d, "k6", feat2[0].dtype)
            if not q2c_tiled_ok(128, hidden, d.dtype) or d.numel() != q2c_tiled_numel(n_tiles * 256, hidden, d.dtype):
                raise _lib.XmlHipError("packed index update: the tile image does not hold n_tiles * 256 rows of H = %d" % hidden)
            data.append(d)
    return cap, hidden, n_tiles, data


def _packed_records(slots, runs, what):
    _req(slots, "slots", torch.int32); _req(runs, "runs", torch.int32)
    n = int(slots.numel())
    if tuple(runs.shape) != (n, 2) or not n:
        raise _lib.XmlHipError("%s: one slot and one (first block, blocks) run per video" % what)
    return n


def index_put_rows_packed(f1, f2, masks, slots, ids, runs, nb_max, k6, feat2, imask, bits, codes, vlen, slot_ids, live, l_ref):
    """xml_index_put_rows_packed: one encoded context batch into its slots AND its runs of the packed K6 image, one launch,
    nothing read back.  f1 / f2 / masks, slots, ids as ops.index_put_rows; runs (b, 2) int32 device = (first block, blocks)
    per video, handed out by index_update.BlockTable; nb_max: the longest run of the call (1..8).  k6: per-modality TiledRows
    over n_tiles * 256 rows; bits: per-modality (2 * n_tiles, 4) packed mask words; codes (2 * n_tiles, 8) int32."""
    cap, hidden, n_tiles, data = _packed_sides(k6, feat2, imask, bits, codes)
    _index_state(vlen, live, cap, slot_ids)
    n_mod = len(feat2)
    b, lb = _batch_sides("index_put_rows_packed", f1, f2, masks, n_mod, hidden, feat2[0].dtype)
    if _packed_records(slots, runs, "index_put_rows_packed") != b or (ids is not None and _req(ids, "ids", torch.int32).numel() != b):
        raise _lib.XmlHipError("index_put_rows_packed: one slot, run (and id) per video of the batch")
    sec = _second(n_mod)
    check(_lib.load().xml_index_put_rows_packed(
        n_mod, _p(f1[0]), _p(f2[0]), _p(masks[0]), sec(f1), sec(f2), sec(masks), _p(slots), _p(ids), _p(runs), b, lb, int(nb_max),
        _p(data[0]), _p(feat2[0]), _p(imask[0]), _p(bits[0]), sec(data), sec(feat2), sec(imask), sec(bits), _p(codes),
        _p(vlen), _p(slot_ids), _p(live), cap, n_tiles, 128, int(l_ref), hidden, dt_of(feat2[0]), _stream()),
        "xml_index_put_rows_packed")


def index_clear_rows_packed(slots, runs, nb_max, imask, bits, codes, vlen, live, l_ref):
    """xml_index_clear_rows_packed: n records (slot, run): the run's codes become -2 and its mask bits 0; the slot is freed as
    ops.index_clear_rows frees it, unless it is -1 (the run alone: a replace that moves its video).  One launch."""
    cap, _, n_tiles, _ = _packed_sides(None, None, imask, bits, codes)
    _index_state(vlen, live, cap)
    n = _packed_records(slots, runs, "index_clear_rows_packed")
    sec = _second(len(imask))
    check(_lib.load().xml_index_clear_rows_packed(len(imask), _p(slots), _p(runs), n, int(nb_max), _p(imask[0]), _p(bits[0]),
                                                  sec(imask), sec(bits), _p(codes), _p(vlen), _p(live), cap, n_tiles, 128,
                                                  int(l_ref), _stream()),
          "xml_index_clear_rows_packed")


def index_move_blocks_packed(records, k6, bits, codes):
    """xml_index_move_blocks_packed (include/xmlhip_index_compact.h): n records (n, 17) int32 device = {tile, src[16]} -- block
    b of the tile receives block src[b] (>= 0, any tile), stays (-1) or becomes unused (-2); image rows, codes and mask bits
    move together, the per-slot state is no operand.  k6: per-modality TiledRows over n_tiles * 256 rows; bits: per-modality
    (2 * n_tiles, 4) packed mask words; codes (2 * n_tiles, 8) int32.  One launch, nothing read back; the launch contract is
    the caller's (index_update.BlockTable.check_compact)."""
    n_mod = len(k6)
    if n_mod not in (1, 2) or len(bits) != n_mod:
        raise _lib.XmlHipError("index_move_blocks_packed: 1 or 2 modalities, one k6 image and one bits tensor each")
    n_tiles = _codes_tiles("index_move_blocks_packed", codes)
    _req(records, "records", torch.int32)
    if records.dim() != 2 or records.shape[1] != 17 or not records.shape[0]:
        raise _lib.XmlHipError("index_move_blocks_packed: records (n, 17) int32 = {tile, src[16]} expected")
    data = []
    for m in range(n_mod):
        if not isinstance(k6[m], TiledRows) or not isinstance(k6[0], TiledRows):
            raise _lib.XmlHipError("index_move_blocks_packed: a TiledRows K6 operand per modality expected")
        d, hidden = k6[m].data, k6[0].hidden
        _req(d, "k6", k6[0].data.dtype); _req(bits[m], "bits", torch.int32)
        if k6[m].hidden != hidden or not q2c_tiled_ok(128, hidden, d.dtype) or \
                d.numel() != q2c_tiled_numel(n_tiles * 256, hidden, d.dtype) or tuple(bits[m].shape) != (2 * n_tiles, 4):
            raise _lib.XmlHipError("index_move_blocks_packed: tile images of n_tiles * 256 = %d rows of one hidden size and bits "
                                   "(2 * n_tiles, 4) expected -- the same n_tiles as codes" % (n_tiles * 256))
        data.append(d)
    sec = _second(n_mod)
    check(_lib.load().xml_index_move_blocks_packed(n_mod, _p(records), int(records.shape[0]), _p(data[0]), _p(bits[0]), sec(data),
                                                   sec(bits), _p(codes), n_tiles, int(k6[0].hidden), dt_of(data[0]), _stream()),
          "xml_index_move_blocks_packed")


# ---- subset views of a resident index (include/xmlhip_index_view.h; tvretrieval_amd/subset.py) --------------------------------
def index_gather_blocks(src_block, k6_src, bits_src, n_blocks_src, k6_dst, bits_dst, hidden):
    """xml_index_gather_blocks: the 16-row blocks named by src_block (16 * n_tiles_dst int32 device, one per DESTINATION block:
    a source block >= 0, or -2 = unused; anything out of range counts as -2) are copied out of the resident K6 image(s) k6_src
    into the packed image(s) k6_dst, with their 16 mask bits per modality.  k6_src / k6_dst: per-modality flat tile images
    (TiledRows.data) of one dtype, the source holding at least ceil(n_blocks_src / 16) tiles, the destination exactly
    n_tiles_dst; bits_src: per modality the source's packed mask words (int32, at least ceil(n_blocks_src / 2) of them) or None =
    that modality is all-valid; bits_dst: per-modality (2 * n_tiles_dst, 4) int32, every word of which is written.  Source
    and destination must not overlap.  One launch, nothing read back."""
    n_mod = len(k6_src)
    if n_mod not in (1, 2) or not (len(bits_src) == len(k6_dst) == len(bits_dst) == n_mod):
        raise _lib.XmlHipError("index_gather_blocks: 1 or 2 modalities, one source image, source bits (or None), destination "
                               "image and destination bits each")
    _req(src_block, "src_block", torch.int32)
    n_blocks_src, hidden = int(n_blocks_src), int(hidden)
    if src_block.dim() != 1 or not src_block.numel() or src_block.numel() % 16 or n_blocks_src <= 0:
        raise _lib.XmlHipError("index_gather_blocks: src_block (16 * n_tiles_dst,) int32 and n_blocks_src >= 1 expected")
    n_tiles = int(src_block.numel()) // 16
    dt = k6_src[0].dtype
    if not q2c_tiled_ok(128, hidden, dt):
        raise _lib.XmlHipError("index_gather_blocks: the tiled K6 kernel takes no %s rows of hidden size %d" % (dt, hidden))
    per_tile = q2c_tiled_numel(256, hidden, dt)
    for m in range(n_mod):
        _req(k6_src[m], "k6_src", dt); _req(k6_dst[m], "k6_dst", dt); _req(bits_dst[m], "bits_dst", torch.int32)
        if k6_src[m].numel() < (n_blocks_src + 15) // 16 * per_tile:
            raise _lib.XmlHipError("index_gather_blocks: the source image holds fewer than n_blocks_src = %d blocks" % n_blocks_src)
        if k6_dst[m].numel() != n_tiles * per_tile or tuple(bits_dst[m].shape) != (2 * n_tiles, 4):
            raise _lib.XmlHipError("index_gather_blocks: a destination image of n_tiles_dst * 256 = %d rows and bits "
                                   "(2 * n_tiles_dst, 4) expected" % (n_tiles * 256))
        if bits_src[m] is not None:
            _req(bits_src[m], "bits_src", torch.int32)
            if bits_src[m].numel() < (n_blocks_src + 1) // 2:
                raise _lib.XmlHipError("index_gather_blocks: the source mask words cover fewer than n_blocks_src = %d blocks"
                                       % n_blocks_src)
    sec = _second(n_mod)
    check(_lib.load().xml_index_gather_blocks(n_mod, _p(src_block), n_tiles, _p(k6_src[0]), _p(bits_src[0]), sec(k6_src),
                                              sec(bits_src), n_blocks_src, _p(k6_dst[0]), _p(bits_dst[0]), sec(k6_dst),
                                              sec(bits_dst), hidden, dt_of(k6_src[0]), _stream()),
          "xml_index_gather_blocks")


# ---- training on a resident index (include/xmlhip_train_index.h; tvretrieval_amd/train_index.py) ------------------------------
def index_gather_video_rows(slots, first_block, vlen, cn_src, f2_src, mask_src, length, n_blocks=0, out=None):
    """xml_index_gather_video_rows: the context operands of a training batch from the index rows of its videos, the model's 1
    or 2 modalities in one launch.  slots (n,) int32 device: index row / slot per batch item; first_block (n,) int32 device:
    the first block of every item's run when cn_src holds TiledRows (n_blocks: the blocks of their image), else None;
    vlen (Nv,) int32.  cn_src / f2_src / mask_src: per modality the index's K6 operand (a TiledRows, or a row-major
    (Nv, lpad, H) tensor), feat2 (Nv, lpad, H) and mask (Nv, lpad) f32.  -> per modality (cn (n, length, H), f2 (n, length, H),
    mask (n, length) f32); rows beyond a video's valid length and items out of range are zero with mask 0.
    out: the same structure of existing tensors to write into."""
    n_mod = len(cn_src)
    if n_mod not in (1, 2) or not (len(f2_src) == len(mask_src) == n_mod):
        raise _lib.XmlHipError("index_gather_video_rows: 1 or 2 modalities, one K6 operand, feat2 and mask each")
    image = isinstance(cn_src[0], TiledRows)
    if any(isinstance(t, TiledRows) != image for t in cn_src):
        raise _lib.XmlHipError("index_gather_video_rows: the modalities' K6 operands must have one form")
    _req(slots, "slots", torch.int32); _req(vlen, "vlen", torch.int32)
    n, length = int(slots.numel()), int(length)
    nv, lpad, hidden = (int(x) for x in f2_src[0].shape)
    dt = f2_src[0].dtype
    if image:
        _req(first_block, "first_block", torch.int32)
        if first_block.numel() != n or int(n_blocks) <= 0:
            raise _lib.XmlHipError("index_gather_video_rows: first_block (n,) int32 and n_blocks >= 1 expected with a block image")
        es = f2_src[0].element_size()
        per_tile = 256 * hidden if (hidden * es) % 64 == 0 else 0          # elements of a tile of whole 64-byte slices
    if vlen.numel() != nv or not 0 < length <= lpad or n <= 0:
        raise _lib.XmlHipError("index_gather_video_rows: vlen (Nv,), a batch of n >= 1 and 0 < length <= lpad = %d expected" % lpad)
    outs = []
    for m in range(n_mod):
        _req(f2_src[m], "feat2", dt); _req(mask_src[m], "mask", torch.float32)
        data = cn_src[m].data if image else cn_src[m]
        _req(data, "cn_src", dt)
        if tuple(f2_src[m].shape) != (nv, lpad, hidden) or tuple(mask_src[m].shape) != (nv, lpad):
            raise _lib.XmlHipError("index_gather_video_rows: feat2 (Nv, lpad, H) and mask (Nv, lpad) expected per modality")
        if image and (not per_tile or data.numel() < (int(n_blocks) + 15) // 16 * per_tile):
            raise _lib.XmlHipError("index_gather_video_rows: a K6 image of whole 64-byte slices that holds n_blocks = %d blocks "
                                   "expected" % int(n_blocks))
        if not image and tuple(data.shape) != (nv, lpad, hidden):
            raise _lib.XmlHipError("index_gather_video_rows: a row-major K6 operand of shape (Nv, lpad, H) expected")
        if out is not None:
            cn, f2, mk = out[m]
            _req(cn, "cn", dt); _req(f2, "f2", dt); _req(mk, "mask_out", torch.float32)
            if tuple(cn.shape) != (n, length, hidden) or tuple(f2.shape) != (n, length, hidden) or tuple(mk.shape) != (n, length):
                raise _lib.XmlHipError("index_gather_video_rows: out: (n, length, H) x 2 and (n, length) expected per modality")
        else:
            cn = torch.empty((n, length, hidden), dtype=dt, device=slots.device)
            f2 = torch.empty((n, length, hidden), dtype=dt, device=slots.device)
            mk = torch.empty((n, length), dtype=torch.float32, device=slots.device)
        outs.append((cn, f2, mk, data))
    b = outs[1] if n_mod == 2 else (None, None, None, None)
    a = outs[0]
    check(_lib.load().xml_index_gather_video_rows(
        n_mod, _lib.XML_INDEX_BLOCK_IMAGE if image else _lib.XML_INDEX_ROW_MAJOR, _p(slots), _p(first_block) if image else None, n,
        _p(vlen), nv, int(n_blocks) if image else 0, lpad, _p(a[3]), _p(f2_src[0]), _p(mask_src[0]), _p(b[3]),
        _p(f2_src[1]) if n_mod == 2 else None, _p(mask_src[1]) if n_mod == 2 else None, _p(a[0]), _p(a[1]), _p(a[2]), _p(b[0]),
        _p(b[1]), _p(b[2]), length, hidden, dt_of(dt), _stream()), "xml_index_gather_video_rows")
    return [o[:3] for o in outs]


# ---- long videos as chains of slots (include/xmlhip_index_parts.h; MutableCorpusIndex(part_overlap=O)) ------------------------
def _chain_tables(tables, names, what):
    """The (capacity,) int32 chain tables `names` of an index (or of any object that carries them) and its max_parts."""
    out, cap = [], None
    for name in names:
        t = getattr(tables, name, None)
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise _lib.XmlHipError("%s: %s must be a contiguous (capacity,) int32 tensor on the GPU "
                                   "(MutableCorpusIndex.create(..., part_overlap=))" % (what, name))
        if cap is not None and t.numel() != cap:
            raise _lib.XmlHipError("%s: the chain tables hold %d and %d slots" % (what, cap, t.numel()))
        cap = int(t.numel())
        out.append(t)
    if not cap:
        raise _lib.XmlHipError("%s: empty chain tables" % what)
    return out, cap


def _chain_scores(scores, cap, device, what):
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise _lib.XmlHipError("%s: scores must be a tensor on the GPU; the HIP path has no CPU fallback" % what)
    if scores.dtype != torch.float32:
        raise _lib.XmlHipError("%s: scores: expected dtype torch.float32, got %s" % (what, scores.dtype))
    if scores.dim() != 2 or scores.shape[1] != cap or (cap > 1 and scores.stride(1) != 1) or \
            (scores.shape[0] and scores.stride(0) < cap):
        raise ValueError("%s: scores must be a (rows, %d slots) f32 matrix with unit column stride, got %s strides %s"
                         % (what, cap, tuple(scores.shape), tuple(scores.stride())))
    if scores.device != device:
        raise ValueError("%s: the scores are on %s, the chain tables on %s" % (what, scores.device, device))


def index_set_chains(records, chain_head, chain_next, chain_offset):
    """xml_index_set_chains: records (n, 4) int32 device = {slot, head, next, offset} scattered into the three (capacity,)
    int32 chain tables -- links a new chain, or puts freed slots back into the single state {s, s, -1, 0}.  The slots of a call
    are distinct (the caller's, index_update.ChainTable); a slot outside [0, capacity) writes nothing.  One launch."""
    t = types.SimpleNamespace(chain_head=chain_head, chain_next=chain_next, chain_offset=chain_offset)
    (head, nxt, off), cap = _chain_tables(t,("chain_head", "chain_next", "chain_offset"), "index_set_chains")
    _req(records, "records", torch.int32)
    if records.dim() != 2 or records.shape[1] != 4:
        raise _lib.XmlHipError("index_set_chains: records (n, 4) int32 = {slot, head, next, offset} expected")
    if not records.shape[0]:          # (an empty tensor has no address to pass; the entry launches nothing for n == 0 either)
        return
    check(_lib.load().xml_index_set_chains(_p(records), int(records.shape[0]), _p(head), _p(nxt), _p(off), cap, _stream()),
          "xml_index_set_chains")


def chain_best_allow(scores, chains, video_allow):
    """The fold of an updatable index with chains between K6 and K8 (xml_chain_best_allow).  scores (rows, capacity) f32 (row
    stride >= capacity); chains: the index (chain_head / chain_next (capacity,) int32 device, max_parts); video_allow
    (1 | rows, >= ceil(capacity / 32)) int32 words, required -- the caller's mask ANDed with the live words, or the live words.
    -> (rows, ceil(capacity / 32)) int32 words: bit s set iff the allow bit of s's HEAD is set and s is the best part of its
    chain for that row (maximum, ties to the lowest offset, NaN never wins; the score of a one-slot chain is not read)."""
    (head, nxt), cap = _chain_tables(chains, ("chain_head", "chain_next"), "chain_best_allow")
    _chain_scores(scores, cap, head.device, "chain_best_allow")
    rows = scores.shape[0]
    if video_allow is None:
        raise ValueError("chain_best_allow: video_allow is required (the live words of the index at least)")
    video_allow, _ = _allow_args(video_allow, 0, rows, cap, scores.device, "chain_best_allow")
    out = torch.empty((rows, (cap + 31) // 32), dtype=torch.int32, device=scores.device)
    check(_lib.load().xml_chain_best_allow(_p(scores), scores.stride(0) if rows else cap, rows, cap, _p(head), _p(nxt),
                                           int(chains.max_parts), _p(video_allow), video_allow.stride(0),
                                           video_allow.shape[0], _p(out), out.stride(0), _stream()), "xml_chain_best_allow")
    return out


def chain_best_rows(scores, chains, video):
    """scores (rows, capacity) f32, video (rows,) int32: ANY slot of one video per row -> (rows,) int32 slot of that video's
    best part (chain_best_allow's rule), -1 for a slot outside [0, capacity)  (xml_chain_best_rows)."""
    (head, nxt), cap = _chain_tables(chains, ("chain_head", "chain_next"), "chain_best_rows")
    _chain_scores(scores, cap, head.device, "chain_best_rows")
    rows = scores.shape[0]
    if not torch.is_tensor(video) or video.dtype != torch.int32 or video.dim() != 1 or video.numel() != rows:
        raise ValueError("chain_best_rows: video must be a (%d,) int32 tensor of slots, got %s %s"
                         % (rows, getattr(video, "dtype", type(video).__name__), tuple(getattr(video, "shape", ()))))
    if video.device != scores.device:
        raise ValueError("chain_best_rows: video is on %s, the scores are on %s" % (video.device, scores.device))
    video = video.contiguous()
    out = torch.empty((rows,), dtype=torch.int32, device=scores.device)
    check(_lib.load().xml_chain_best_rows(_p(scores), scores.stride(0) if rows else cap, rows, cap, _p(head), _p(nxt),
                                          int(chains.max_parts), _p(video), _p(out), _stream()), "xml_chain_best_rows")
    return out


# ---- chains on an exact-rank index (include/xmlhip_index_parts_exact.h; create(..., exact_rank=True, exact_part_overlap=O)) ----
def cand_best_part_max_m():
    """The widest candidate list cand_best_part folds (xml_cand_best_part_max_m)."""
    return int(_lib.load().xml_cand_best_part_max_m())


def cand_best_part(scores, ids, group, order, out=None):
    """The fold of a chain index on a candidate list (xml_cand_best_part).  scores (rows, m) f32 and ids (rows, m) int32
    (slots; an id outside [0, n) is an empty candidate), contiguous; group / order (n,) int32
    per-slot tables (chain_head / chain_offset).  Candidates of one group (in-range ids with equal group values; a group
    value outside [0, n) is a group of its own) are reduced to the best one -- the greatest isnan(s) ? -inf : s, ties to the
    smallest order, then to the lower position --, which keeps its score bits and id; the others become (-inf, -1).
    out=None -> new (scores, ids); out=(scores, ids) writes there, the inputs themselves fold in place."""
    _req(scores, "scores", torch.float32); _req(ids, "ids", torch.int32)
    (g, o), n = _chain_tables(types.SimpleNamespace(group=group, order=order), ("group", "order"), "cand_best_part")
    if scores.dim() != 2 or ids.shape != scores.shape or scores.shape[1] < 1:
        raise ValueError("cand_best_part: scores and ids must be (rows, m >= 1) matrices of one shape, got %s and %s"
                         % (tuple(scores.shape), tuple(ids.shape)))
    rows, m = scores.shape
    if m > cand_best_part_max_m():
        raise ValueError("cand_best_part: a list of %d candidates; xml_cand_best_part folds at most %d" % (m, cand_best_part_max_m()))
    if scores.device != g.device or ids.device != g.device:
        raise ValueError("cand_best_part: the lists are on %s / %s, the tables on %s" % (scores.device, ids.device, g.device))
    if out is None:
        out = (torch.empty((rows, m), dtype=torch.float32, device=scores.device),
               torch.empty((rows, m), dtype=torch.int32, device=scores.device))
    out_s, out_i = out
    _req(out_s, "out scores", torch.float32); _req(out_i, "out ids", torch.int32)
    if out_s.shape != scores.shape or out_i.shape != scores.shape:
        raise ValueError("cand_best_part: out must be a (scores, ids) pair of shape %s" % (tuple(scores.shape),))
    if rows:          # (contiguous lists: both row strides are m)
        check(_lib.load().xml_cand_best_part(_p(scores), _p(ids), m, rows, m, _p(g), _p(o), n, _p(out_s), _p(out_i), m,
                                             _stream()), "xml_cand_best_part")
    return out_s, out_i


def chain_spread_allow(video_allow, chains):
    """A caller's head-bit mask made per-slot (xml_chain_spread_allow).  video_allow (R, >= ceil(capacity / 32)) int32 words
    in which a video is numbered by its HEAD slot; chains: the index (chain_head) -> (R, ceil(capacity / 32)) int32 words, bit
    s = the allow bit of chain_head[s] (0 for a head outside the index; padding bits 0)."""
    (head,), cap = _chain_tables(chains, ("chain_head",), "chain_spread_allow")
    if not torch.is_tensor(video_allow) or video_allow.dim() != 2:
        raise ValueError("chain_spread_allow: video_allow must be a 2-D int32 tensor of bit words (inference.pack_video_allow)")
    rows = video_allow.shape[0]
    video_allow, _ = _allow_args(video_allow, 0, rows, cap, head.device, "chain_spread_allow")
    out = torch.empty((rows, (cap + 31) // 32), dtype=torch.int32, device=head.device)
    if rows:
        check(_lib.load().xml_chain_spread_allow(_p(video_allow), video_allow.stride(0), rows, rows, cap, _p(head), _p(out),
                                                 out.stride(0), _stream()), "xml_chain_spread_allow")
    return out


def chain_members(chains, video):
    """video (rows,) int32: ANY slot of one video per row -> (rows, max_parts) int32, the slots of that video's chain in rising
    offset order, -1 behind its end (all -1 for a slot outside the index)  (xml_chain_members)."""
    (head, nxt), cap = _chain_tables(chains, ("chain_head", "chain_next"), "chain_members")
    if not torch.is_tensor(video) or video.dtype != torch.int32 or video.dim() != 1:
        raise ValueError("chain_members: video must be a (rows,) int32 tensor of slots, got %s %s"
                         % (getattr(video, "dtype", type(video).__name__), tuple(getattr(video, "shape", ()))))
    if video.device != head.device:
        raise ValueError("chain_members: video is on %s, the chain tables on %s" % (video.device, head.device))
    video = video.contiguous()
    rows, mp = video.numel(), int(chains.max_parts)
    out = torch.empty((rows, mp), dtype=torch.int32, device=head.device)
    if rows:
        check(_lib.load().xml_chain_members(_p(video), rows, cap, _p(head), _p(nxt), mp, _p(out), out.stride(0), _stream()),
              "xml_chain_members")
    return out


# ---- exact-rank mode on an updatable index (include/xmlhip_index_exact.h; MutableCorpusIndex.create(..., exact_rank=True)) ------
EXACT_F32, EXACT_F16S = 0, 1          # XML_EXACT_F32 / XML_EXACT_F16S


def _exact_sides(k6, rescore, feat2, err, imask, bits, n_tiles=None):
    """Checks the per-modality tensors of an exact-rank slot; returns (capacity, lpad, hidden, tiled, mode, k6 buffers).
    n_tiles (index_put_rows_packed_exact): the filter image is the packed one over n_tiles * 256 rows, bits its mask words."""
    n_mod = len(feat2)
    if n_mod not in (1, 2) or not (len(k6) == len(rescore) == len(err) == len(imask) == len(bits) == n_mod):
        raise _lib.XmlHipError("exact index update: 1 or 2 modalities, the same number of k6 / rescore / feat2 / err / mask / "
                               "bits tensors")
    split = isinstance(feat2[0], SplitRows)
    cap, lpad, hidden = (int(x) for x in feat2[0].shape)
    tiled = isinstance(k6[0], TiledRows)
    data = []
    for m in range(n_mod):
        for t, name in ((rescore[m], "rescore"), (feat2[m], "feat2")):
            if isinstance(t, SplitRows) != split:
                raise _lib.XmlHipError("exact index update: re-score rows and feat2 are all f32 tensors or all SplitRows")
            if split:
                _req(t.data, name, torch.int32); _req(t.inv, name + ".inv", torch.float32)
                if tuple(t.inv.shape) != (cap, lpad):
                    raise _lib.XmlHipError("exact index update: %s.inv (capacity, lpad) expected" % name)
            else:
                _req(t, name, torch.float32)
            if tuple(t.shape) != (cap, lpad, hidden):
                raise _lib.XmlHipError("exact index update: %s of shape %s expected" % (name, (cap, lpad, hidden)))
        _req(err[m], "err", torch.float32); _req(imask[m], "mask", torch.float32); _req(bits[m], "bits", torch.int32)
        if tuple(err[m].shape) != (cap, lpad) or tuple(imask[m].shape) != (cap, lpad):
            raise _lib.XmlHipError("exact index update: err / mask (capacity, lpad) expected")
        if n_tiles is None:
            if tuple(bits[m].shape) != (cap, 4):
                raise _lib.XmlHipError("exact index update: bits (capacity, 4) expected")
            data.append(_k6_side("exact index update", k6[m], tiled, cap, lpad, hidden, torch.bfloat16, "filter image"))
            continue
        if lpad != 128 or tuple(bits[m].shape) != (2 * n_tiles, 4) or not tiled or not isinstance(k6[m], TiledRows):
            raise _lib.XmlHipError("packed exact index update: slots of 128 clips, bits (2 * n_tiles, 4) and a TiledRows filter "
                                   "image expected")
        d = k6[m].data
        _req(d, "k6", torch.bfloat16)
        if not q2c_tiled_ok(128, hidden, d.dtype) or d.numel() != q2c_tiled_numel(n_tiles * 256, hidden, d.dtype):
            raise _lib.XmlHipError("packed exact index update: the filter image does not hold n_tiles * 256 rows of H = %d"
                                   % hidden)
        data.append(d)
    return cap, lpad, hidden, tiled, EXACT_F16S if split else EXACT_F32, data


def index_put_rows_exact(f1, f2, masks, slots, ids, k6, rescore, feat2, err, imask, bits, ec, vlen, slot_ids, live, l_ref):
    """xml_index_put_rows_exact: one encoded f32 context batch into its slots of an exact-rank index -- bf16 filter image,
    re-score rows, feat2, rounding-error norms, mask, mask words, vlen, ids, live bits -- and the running bound ec raised; one
    launch, nothing read back.  f1 / f2 / masks, slots, ids: as index_put_rows (f32).  k6: per-modality TiledRows or
    (capacity, lpad, H) tensors, bf16; rescore / feat2: per-modality (capacity, lpad, H) f32 tensors (mode "f32") or SplitRows
    (mode "f16s"); err (capacity, lpad) f32 per modality; ec (n_mod,) f32; the rest as index_put_rows."""
    cap, lpad, hidden, tiled, mode, data = _exact_sides(k6, rescore, feat2, err, imask, bits)
    _index_state(vlen, live, cap, slot_ids)
    n_mod = len(feat2)
    _req(ec, "ec", torch.float32)
    if ec.numel() != n_mod:
        raise _lib.XmlHipError("index_put_rows_exact: ec (n_mod,) f32 expected")
    b, lb = _batch_sides("index_put_rows_exact", f1, f2, masks, n_mod, hidden, torch.float32)
    _slot_records("index_put_rows_exact", slots, ids, b)
    split = mode == EXACT_F16S
    side = []
    for m in range(n_mod):
        side += [_p(data[m]), _p(rescore[m]), _p(rescore[m].inv) if split else None, _p(feat2[m]),
                 _p(feat2[m].inv) if split else None, _p(err[m]), _p(imask[m]), _p(bits[m])]
    side += [None] * (16 - len(side))
    sec = _second(n_mod)
    check(_lib.load().xml_index_put_rows_exact(
        n_mod, mode, _p(f1[0]), _p(f2[0]), _p(masks[0]), sec(f1), sec(f2), sec(masks), _p(slots), _p(ids), b, lb, *side,
        _p(ec), _p(vlen), _p(slot_ids), _p(live), cap, lpad, int(l_ref), hidden, XML_F32, int(tiled), _stream()),
        "xml_index_put_rows_exact")


def index_put_rows_packed_exact(f1, f2, masks, slots, ids, runs, nb_max, k6, rescore, feat2, err, imask, bits, codes, ec, vlen,
                                slot_ids, live, l_ref):
    """xml_index_put_rows_packed_exact (include/xmlhip_index_exact_packed.h): index_put_rows_exact on an exact-rank index whose
    bf16 FILTER image is the packed one -- the filter rows, codes and mask words go to the videos' runs as
    index_put_rows_packed puts them, every per-slot operand (rescore, feat2, err, mask) and the running bound are written as
    index_put_rows_exact writes them; one launch, nothing read back.  runs (b, 2) int32 device, nb_max: index_put_rows_packed;
    k6: per-modality bf16 TiledRows over n_tiles * 256 rows; bits: per-modality (2 * n_tiles, 4); codes (2 * n_tiles, 8)
    int32; the rest as index_put_rows_exact."""
    n_tiles = _codes_tiles("index_put_rows_packed_exact", codes)
    cap, _, hidden, _, mode, data = _exact_sides(k6, rescore, feat2, err, imask, bits, n_tiles)
    _index_state(vlen, live, cap, slot_ids)
    n_mod = len(feat2)
    _req(ec, "ec", torch.float32)
    if ec.numel() != n_mod:
        raise _lib.XmlHipError("index_put_rows_packed_exact: ec (n_mod,) f32 expected")
    b, lb = _batch_sides("index_put_rows_packed_exact", f1, f2, masks, n_mod, hidden, torch.float32)
    if _packed_records(slots, runs, "index_put_rows_packed_exact") != b or \
            (ids is not None and _req(ids, "ids", torch.int32).numel() != b):
        raise _lib.XmlHipError("index_put_rows_packed_exact: one slot, run (and id) per video of the batch")
    split = mode == EXACT_F16S
    side = []
    for m in range(n_mod):
        side += [_p(data[m]), _p(rescore[m]), _p(rescore[m].inv) if split else None, _p(feat2[m]),
                 _p(feat2[m].inv) if split else None, _p(err[m]), _p(imask[m]), _p(bits[m])]
    side += [None] * (16 - len(side))
    sec = _second(n_mod)
    check(_lib.load().xml_index_put_rows_packed_exact(
        n_mod, mode, _p(f1[0]), _p(f2[0]), _p(masks[0]), sec(f1), sec(f2), sec(masks), _p(slots), _p(ids), _p(runs), b, lb,
        int(nb_max), *side, _p(codes), _p(ec), _p(vlen), _p(slot_ids), _p(live), cap, n_tiles, 128, int(l_ref), hidden, XML_F32,
        _stream()), "xml_index_put_rows_packed_exact")


def exact_certificate_dev(filter_scores, top_val, eq, ec, slack_base, slack_ec2, alpha, outside):
    """exact_certificate with the corpus bound on the device: ec (n_mod,) f32 device tensor, read when the kernel runs (a
    captured search sees the bound of its replay); slack = slack_base + slack_ec2 * max(ec)^2 in f32 in the kernel.
    Returns (fail, eps, thr, n_fail) as exact_certificate."""
    _req(filter_scores, "filter_scores", torch.float32); _req(top_val, "top_val", torch.float32)
    n_mod = len(eq)
    for e in eq:
        _req(e, "eq", torch.float32)
    _req(ec, "ec", torch.float32)
    if ec.numel() != n_mod:
        raise _lib.XmlHipError("exact_certificate_dev: ec (n_mod,) f32 expected")
    nq, m = filter_scores.shape
    k = top_val.shape[1]
    dev = top_val.device
    fail = torch.empty((nq,), dtype=torch.int32, device=dev)
    eps = torch.empty((nq,), dtype=torch.float32, device=dev)
    thr = torch.empty((nq,), dtype=torch.float32, device=dev)
    n_fail = torch.zeros((1,), dtype=torch.int32, device=dev)
    j = 1 if n_mod > 1 else 0
    check(_lib.load().xml_exact_certificate_dev(_p(filter_scores), m, _p(top_val), k, _p(eq[0]), _p(eq[j]), _p(ec), n_mod,
                                                float(slack_base), float(slack_ec2), float(alpha), int(bool(outside)),
                                                _p(fail), _p(eps), _p(thr), _p(n_fail), nq, _stream()),
          "xml_exact_certificate_dev")
    return fail, eps, thr, n_fail


def index_exact_bound(err, live, ec):
    """xml_index_exact_bound: ec[m] = max of err[m] (capacity, lpad) over the slots whose live bit is set (0 when none is);
    one launch, nothing read back."""
    n_mod = len(err)
    if n_mod not in (1, 2):
        raise _lib.XmlHipError("index_exact_bound: 1 or 2 modalities")
    cap, lpad = (int(x) for x in err[0].shape)
    for e in err:
        _req(e, "err", torch.float32)
        if tuple(e.shape) != (cap, lpad):
            raise _lib.XmlHipError("index_exact_bound: err (capacity, lpad) per modality expected")
    _req(live, "live", torch.int32); _req(ec, "ec", torch.float32)
    if live.numel() != (cap + 31) // 32 or ec.numel() != n_mod:
        raise _lib.XmlHipError("index_exact_bound: live (ceil(capacity / 32),) int32 and ec (n_mod,) f32 expected")
    check(_lib.load().xml_index_exact_bound(n_mod, _p(err[0]), _p(err[1]) if n_mod == 2 else None, _p(live), _p(ec), cap, lpad,
                                            _stream()), "xml_index_exact_bound")
