"""float32 numpy restatement of the temporal endpoint columns of include/xmlhip_ingest_tef.h and of the truncate / normalise /
pad contract of xml_ingest_rows_tef, and the small cases of its GPU tests (tests/test_gpu_ingest_tef.py,
tests/test_gpu_ingest_tef_arena.py).  A plain helper module: imports without a GPU.

The two columns follow xml/start_end_dataset.py:328-342 of the reference: tef_st = torch.arange(0, L, 1.0) / L is one f32
division per clip, and tef_ed = tef_st + 1.0 / L adds the Python double 1.0 / L, which torch rounds to f32 before the f32 sum.
Placed on a longer axis (the parts of a long video) the numerator is P + l and the denominator the whole video's clip count."""
import numpy as np
import torch

EPS = 1e-5
LENS = (1, 7, 32, 33, 36)        # at max_len 33: lmax 33, 165 destination rows (no multiple of the 4 per workgroup), one cut
MAX_LEN = 33


def endpoint_columns(length, pos=0, total=None):
    """(length, 2) float32: clips pos .. pos + length - 1 of a video of `total` clips (default: the item is the video)."""
    total = int(length if total is None else total)
    st = (np.arange(pos, pos + length, dtype=np.int64).astype(np.float32) / np.float32(total)).astype(np.float32)
    ed = (st + np.float32(1.0 / float(total))).astype(np.float32)
    return np.stack([st, ed], axis=1)


def place(length, pos, total):
    """The (P, L) the entries use for an item of `length` clips: the caller's unless they cannot hold the item."""
    if pos is None or pos < 0 or pos + length > total:
        return 0, length
    return pos, total


def restate_tef(lens, lmax, max_len, tef_pos=None, tef_len=None):
    """(n, lmax, 2) float32 endpoint columns of a batch; rows l >= len are zero."""
    out = np.zeros((len(lens), lmax, 2), dtype=np.float32)
    for i, n in enumerate(lens):
        ln = min(int(n), max_len)
        p, t = place(ln, None if tef_pos is None else int(tef_pos[i]), None if tef_len is None else int(tef_len[i]))
        out[i, :ln] = endpoint_columns(ln, p, t)
    return out


def restate_rows(src, row_start, lmax, max_len, normalize, tef_pos=None, tef_len=None):
    """xml_ingest_rows_tef in float32: src (rows, d) -> (features (n, lmax, d + 2), mask (n, lmax))."""
    n, d = len(row_start) - 1, src.shape[1]
    lens = np.diff(row_start)
    out = np.zeros((n, lmax, d + 2), dtype=np.float32)
    mask = np.zeros((n, lmax), dtype=np.float32)
    for i in range(n):
        ln = min(int(lens[i]), max_len)
        x = src[int(row_start[i]):int(row_start[i]) + ln].astype(np.float32)
        if normalize:
            x = x / (np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32)) + np.float32(EPS))
        out[i, :ln, :d] = x
        mask[i, :ln] = 1
    out[:, :, d:] = restate_tef(lens, lmax, max_len, tef_pos, tef_len)
    return out, mask


def to_bf16(a):
    """float32 array rounded to bf16 (nearest even), as a torch tensor"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def rows_case(d, src_dtype, seed=0, lens=LENS):
    """The batch of the kernel sweep: rows with a spread of magnitudes, row 3 (if there is one) all zero."""
    g = torch.Generator().manual_seed(4100 + seed + d)
    row_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(row_start[-1])
    x = torch.randn(rows, d, generator=g) * torch.logspace(-1.3, 0.5, rows)[:, None]
    if rows > 3:
        x[3] = 0.0
    return dict(src=x.to(src_dtype), row_start=torch.from_numpy(row_start), n=len(lens), lmax=min(max(lens), MAX_LEN),
                max_len=MAX_LEN, lens=lens)


def pool_case(d_a, d_b, src_dtype, seed=0, lens=LENS):
    """The batch of the pooled sweep: every clip row is pooled over 1-4 source rows; clip row 5 (if there is one) has an empty
    range in every source.  Post-ReLU-like values without negative zeros (the maximum of -0 and +0 has no defined sign)."""
    g = torch.Generator().manual_seed(4300 + seed + d_a + 7 * d_b)
    row_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = int(row_start[-1])
    srcs, segs = [], []
    for k, d in enumerate([d_a] + ([d_b] if d_b else [])):
        cnt = np.array([1 + (j + k) % 4 for j in range(R)])
        if R > 5:
            cnt[5] = 0
        lo = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        n_rows = int(cnt.sum())
        x = torch.randn(n_rows, d, generator=g) * torch.logspace(-1, 0.7, n_rows)[:, None]
        x = torch.where(torch.rand(n_rows, d, generator=g) < 0.3, torch.zeros(()), x.abs() + 0.01 * x)
        srcs.append(x.to(src_dtype))
        segs.append(torch.from_numpy(np.stack([lo, lo + cnt], axis=1).astype(np.int64)))
    return dict(srcs=srcs, segs=segs, row_start=torch.from_numpy(row_start), n=len(lens), lmax=min(max(lens), MAX_LEN),
                max_len=MAX_LEN, lens=lens)
