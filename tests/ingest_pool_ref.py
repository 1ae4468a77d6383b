"""numpy restatement of xml_ingest_pool_rows (include/xmlhip_ingest_pool.h) and the small cases of its GPU tests
(tests/test_gpu_ingest_pool.py, tests/test_gpu_ingest_pool_arena.py).  A plain helper module: imports without a GPU.

The restatement follows the reference's three scripts stage by stage, in the dtype it is given: pool each source's rows
(np.max / np.mean, axis 0: convert_feature_frm_to_clip.py:29-34, convert_sub_feature_word_to_clip.py:75-86, zero rows where a
range is empty), x / (||x|| + eps) per source and concatenate (normalize_and_concat.py:24-29), then the dataset's
x / (||x|| + eps) over the row, truncation, zero padding and the mask (xml/start_end_dataset.py:297-321)."""
import numpy as np
import torch

EPS = 1e-5
# (d_a, d_b): the real shape; the word stream; two 16-byte-able blocks inside one chunk; one lane's worth; the narrow path with a
# misaligned second block
DIMS = [(2048, 1024), (768, 0), (24, 40), (8, 0), (7, 5)]


def _norm(x, dtype):
    x = x.astype(dtype)
    return x / (np.sqrt((x * x).sum(dtype=dtype), dtype=dtype) + dtype(EPS))


def restate(srcs, segs, norms, row_start, n, lmax, max_len, pool, normalize, dtype=np.float32):
    """srcs: [(rows_x, d_x) array]; segs: [(R, 2) int64]; -> features (n, lmax, sum d_x) `dtype`, mask, filled (n, lmax) f32."""
    d = sum(s.shape[1] for s in srcs)
    out = np.zeros((n, lmax, d), dtype=dtype)
    mask = np.zeros((n, lmax), dtype=np.float32)
    filled = np.zeros((n, lmax), dtype=np.float32)
    f = np.max if pool == "max" else np.mean
    for i in range(n):
        ln = min(max_len, int(row_start[i + 1] - row_start[i]))
        for l in range(ln):
            r = int(row_start[i]) + l
            blocks = []
            for src, seg, norm in zip(srcs, segs, norms):
                lo, hi = int(seg[r, 0]), int(seg[r, 1])
                if 0 <= lo < hi <= len(src):
                    b = f(src[lo:hi].astype(dtype), axis=0)
                    filled[i, l] = 1
                else:
                    b = np.zeros(src.shape[1], dtype=dtype)
                blocks.append(_norm(b, dtype) if norm else b)
            row = np.concatenate(blocks)
            out[i, l] = _norm(row, dtype) if normalize else row
            mask[i, l] = 1
    return out, mask, filled


def small_case(d_a, d_b, src_dtype, seed=0, rows=(150, 131)):
    """Four videos of 7, 0, 12 and 3 clip rows at max_len 9 and lmax 11: a video of no clips, one longer than max_len, padding
    beyond max_len.  Segment lengths 0, 1, 2, 5 and ~60 with overlapping neighbours, a range from source row 0 and one to the
    last source row.  Source values are post-ReLU-like with a spread of row magnitudes, as the stores hold them; no negative
    zeros (the maximum of -0 and +0 has no defined sign)."""
    g = torch.Generator().manual_seed(900 + seed + d_a + 7 * d_b)
    counts = [7, 0, 12, 3]
    row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(row_start[-1])
    dims = [d_a] + ([d_b] if d_b else [])
    srcs, segs = [], []
    for k, d in enumerate(dims):
        n_rows = rows[k]
        x = torch.randn(n_rows, d, generator=g) * torch.logspace(-1, 0.7, n_rows)[:, None]
        x = torch.where(torch.rand(n_rows, d, generator=g) < 0.3, torch.zeros(()), x.abs() + 0.01 * x)
        srcs.append(x.to(src_dtype).numpy())
        lens = np.array([0, 1, 2, 5, 60, 1, 5, 2, 61, 0, 5, 1, 2, 59, 5, 1, 0, 2, 5, 1, 2, 5][:R])
        lo = np.array([(11 * j + 3 * k) % (n_rows - 62) for j in range(R)])
        lo[1::2] = np.maximum(lo[0::2] + lens[0::2] - 1, 0)[:len(lo[1::2])]          # a neighbour that overlaps its predecessor
        lo = np.minimum(lo, n_rows - lens)
        lo[2], lo[10] = 0, n_rows - lens[10]                   # touches source row 0; ends at the last source row
        segs.append(np.stack([lo, lo + lens], axis=1).astype(np.int64))
    return dict(srcs=srcs, segs=segs, row_start=row_start, n=4, lmax=11, max_len=9, counts=counts)


def bad_ranges(seg, n_rows):
    """seg with five of its ranges replaced by ranges that must read nothing: past the end, starting before 0, inverted,
    starting past the end, and huge."""
    seg = seg.copy()
    seg[0] = (n_rows - 2, n_rows + 1)
    seg[3] = (-1, 4)
    seg[4] = (9, 3)
    seg[7] = (n_rows + 5, n_rows + 9)
    seg[8] = (-2 ** 62, 2 ** 62)
    return seg


BAD_ROWS = (0, 3, 4, 7, 8)
