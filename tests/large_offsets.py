"""Shape, thresholds and sample set of the large-offset tests (tests/test_gpu_large_offsets.py on the GPU,
tests/test_large_offsets_plan.py without one).  Imports without a GPU and without the built library.

A kernel that addresses a corpus-sized operand can go wrong at three offsets:
  T1  2^31 bytes     a signed 32-bit byte offset
  T2  2^32 bytes     an unsigned 32-bit byte offset, or the 32-bit vector offset of a DMA against a scalar base
  T3  2^31 elements  an `int row * d` element index
The headline corpus (21 793 videos x 128 clips x 768) ends 0.24 % below T3 and, in bf16, 0.24 % below T2.  NV_BIG is the
smallest round corpus past T3 at the project's own row width: 21 888 x 128 x 768 = 2 151 677 952 elements."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LPAD, HIDDEN, NV_BIG = 128, 768, 21888
ES = {"f32": 4, "bf16": 2, "f16": 2, "f16s": 4, "i32": 4, "i64": 8}
HEADERS = ("xmlhip.h", "xmlhip_index.h", "xmlhip_index_parts.h", "xmlhip_index_compact.h")

# the fixed list of reasons a header symbol may give for having no large-offset case
NO_DEVICE = "no device operand"
BATCH_ONLY = "operands sized by the batch only, not the corpus or store"
TRAINING = "training step only"
COLLECTIVE = "collective wrapper around a covered kernel"
REASONS = (NO_DEVICE, BATCH_ONLY, TRAINING, COLLECTIVE)


def thresholds(es):
    """The three offsets in ELEMENTS of an operand whose elements are `es` bytes."""
    return {"T1": 2 ** 31 // es, "T2": 2 ** 32 // es, "T3": 2 ** 31}


def straddler(t, per):
    """The unit (video, tile, row ...) of `per` elements that holds element offset t: the first one a 32-bit index that
    breaks at t addresses wrongly."""
    return t // per


def sample_videos(nv, lpad, hidden, es):
    """Video 0, video nv - 1 and, for each threshold inside the (nv, lpad, hidden) operand, the video whose rows hold it and
    both of its neighbours.  Sorted, distinct."""
    per = lpad * hidden
    out = {0, nv - 1}
    for t in thresholds(es).values():
        if t < nv * per:
            v = straddler(t, per)
            out.update(u for u in (v - 1, v, v + 1) if 0 <= u < nv)
    return sorted(out)


def missed_thresholds(samples, nv, lpad, hidden, es):
    """Names of the thresholds inside the operand that `samples` does not cover: the straddling video or one of its
    neighbours is missing."""
    per = lpad * hidden
    have = set(samples)
    missed = []
    for name, t in sorted(thresholds(es).items()):
        if t >= nv * per:
            continue
        v = straddler(t, per)
        assert v * per <= t < (v + 1) * per
        if not {u for u in (v - 1, v, v + 1) if 0 <= u < nv} <= have:
            missed.append(name)
    return missed


def assert_crosses(extent_elems, es, which):
    """Every GPU case calls this on the operand it claims to exercise: a case that silently shrinks below its threshold
    fails instead of passing.  which: one threshold name or several."""
    names = (which,) if isinstance(which, str) else tuple(which)
    th = thresholds(es)
    for name in names:
        assert extent_elems > th[name], "an operand of %d elements of %d bytes ends below %s (%d elements): the case no " \
            "longer crosses what it claims to" % (extent_elems, es, name, th[name])


def header_symbols(headers=HEADERS):
    """{symbol: header} of every xml_* function the public headers declare."""
    out = {}
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        for s in re.findall(r"\b(xml_[a-z0-9_]+)\s*\(", src):
            out.setdefault(s, h)
    return out


def tile_image_bytes(rows_u8, row_bytes):
    """Independent restatement of K6's tile layout from the header's description, in numpy: rows_u8 (n_tiles * 256, row_bytes)
    uint8 row-major -> the image [tile][slice][row][64 B] as (n_tiles, row_bytes / 64 * 256 * 64) uint8."""
    import numpy as np
    assert rows_u8.dtype == np.uint8 and rows_u8.shape[0] % 256 == 0 and rows_u8.shape[1] == row_bytes and row_bytes % 64 == 0
    n_tiles, n_slices = rows_u8.shape[0] // 256, row_bytes // 64
    out = np.empty((n_tiles, n_slices, 256, 64), dtype=np.uint8)
    for t in range(n_tiles):
        for s in range(n_slices):               # slice s of the tile: 64 bytes of each of its 256 rows, row after row
            out[t, s] = rows_u8[t * 256:(t + 1) * 256, s * 64:(s + 1) * 64]
    return out.reshape(n_tiles, -1)
