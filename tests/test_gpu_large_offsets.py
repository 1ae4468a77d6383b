"""Corpus-side kernels past 2^31 elements and 4 GiB offsets (tests/large_offsets.py has the shape, the
three thresholds T1 / T2 / T3 and the sample set, tests/test_large_offsets_plan.py checks both and the registry below
without a GPU).

The headline corpus ends a quarter of a percent below the sizes at which 32-bit index arithmetic breaks.  Every entry that
reads or writes an operand of nv x lpad x hidden, nv x lpad, rows x d with corpus-sized rows, or a feature store runs here
once on an operand of NV_BIG = 21 888 videos x 128 clips x 768 (2 151 677 952 elements: past T3, and in every dtype past T1
and T2), or on score rows whose leading dimension puts the last row past T3.  Operands are filled on the device; the
references see only the sampled videos (video 0, the last, the videos that hold a threshold and their neighbours) copied to
the host.  No bound is new: values go against float64 with the helpers and margins of tests/test_gpu_numerics.py, or are
bitwise those of the same entry on operands below every threshold -- the two halves of the corpus, or a TWIN that holds
copies of just the sampled videos, renumbered.  The small-size tests tie those to float64 and to the builder.

Every case calls large_offsets.assert_crosses on the operand it claims to exercise.  LARGE_CASES / LARGE_EXEMPT name, for
every symbol of the four public headers, the cases that cover it or the reason it needs none.
One corpus-sized operand set is alive at a time: the kernel-level cases peak below 23 GB, the whole-search cases at 25 - 31 GB
while the builder holds feat1, feat2 and the tile image of NV_BIG videos (profiles/large_offsets.md has every figure).
Every test prints `LARGE <id>: wall, peak, live` (pytest -s).  Run on the MI355X box:  pytest -m gpu -s tests/test_gpu_large_offsets.py"""
import gc
import time
import types

import numpy as np
import pytest
import torch

import large_offsets as LO
import numerics_regimes as NR
import reduction_width_cases as RC
from large_offsets import BATCH_ONLY, COLLECTIVE, NO_DEVICE, TRAINING
from test_gpu_kernels import DEV, close, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

C_ROWWISE, C_CHAIN = 2, 8       # the margins of tests/test_gpu_numerics.py for the row-wise passes and for K6 / the re-score
NV, L, H = LO.NV_BIG, LO.LPAD, LO.HIDDEN
ROWS = NV * L                   # 2 801 664 clip rows
HALF = NV // 2                  # the corpus splits into two operands below T3 (and into whole tiles: HALF is even)
N_TILES = NV // 2               # 10 944 tiles of 256 rows: the tile image is as large as the row-major operand
ALL = ("T1", "T2", "T3")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
# one sample set for every dtype: the f32 set (11 videos) contains the bf16 one
SAMPLE = sorted(set(LO.sample_videos(NV, L, H, 2)) | set(LO.sample_videos(NV, L, H, 4)))
SAMPLE_TILES = sorted(set(LO.sample_videos(N_TILES, 256, H, 2)) | set(LO.sample_videos(N_TILES, 256, H, 4)))
NQ = RC.K6_PERSIST_SHAPES[0][1]          # 300 queries: three query tiles
LD_BIG = 2 ** 30 + 64                    # leading dimension of the score-side cases: row 2 starts past 2^31 elements


# ---- shared state: one corpus-sized operand set at a time ------------------------------------------------------------------
_BIG = {}


def _free(*keys):
    """Drop the cached corpus-sized operands (all of them without arguments) and hand their memory back."""
    for k in (keys or list(_BIG)):
        _BIG.pop(k, None)
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _module_teardown():
    yield
    _WORLD.clear()
    _free()


@pytest.fixture(scope="module", params=["bf16", "f32"])
def dtype(request):
    """Module-scoped so that pytest runs the cases of one storage type next to each other: the corpus is built twice."""
    return request.param


@pytest.fixture(autouse=True)
def _measure(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("LARGE %s: wall %.2f s, peak %.1f GB, live behind it %.1f GB" % (
        request.node.name, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 1e9, torch.cuda.memory_allocated() / 1e9))


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def filled(shape, dtype):
    """An output whose every byte is 0xFF (a NaN in every float type, -1 in every integer type)."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def assert_every_row_written(t, what, step=1152 * L):
    """Whole-extent device check, in chunks: no row of t (rows, d) is left at its 0xFF pre-fill."""
    u = t.view(-1, t.shape[-1]).view(torch.uint8)
    for r0 in range(0, u.shape[0], step):
        left = ~(u[r0:r0 + step] != 0xFF).any(1)
        assert not bool(left.any()), "%s: row %d was never written" % (what, r0 + int(left.nonzero()[0]))


def assert_every_element_written(t, what):
    """... and for one 4-byte value per row (norms, scales): no element is left at 0xFFFFFFFF."""
    left = t.view(-1).view(torch.int32) == -1
    assert not bool(left.any()), "%s: element %d was never written" % (what, int(left.nonzero()[0]))


def video_rows(videos):
    """Row indices (device) of the clip rows of `videos` in the (ROWS, H) view."""
    v = torch.as_tensor(videos, device=DEV, dtype=torch.int64)
    return (v[:, None] * L + torch.arange(L, device=DEV)[None]).view(-1)


def corpus(dt):
    """The (NV, L, H) operand of storage type dt -- torch.randn on the device under a seeded generator, then the dataset
    normalisation x / (|x| + 1e-5) -- with its masks, queries and the host copies of the sampled videos.  Built when a test
    asks for it and kept until a test asks for the other dtype or frees it."""
    d = _BIG.get("corpus")
    if d is not None and d["dt"] == dt:
        return d
    _free()
    td = TDT[dt]
    g = torch.Generator(device=DEV).manual_seed(2031 + LO.ES[dt])
    c = torch.empty((NV, L, H), dtype=td, device=DEV)
    step = 1152
    assert NV % step == 0
    for i in range(0, NV, step):
        x = torch.randn(step, L, H, device=DEV, generator=g)
        c[i:i + step] = (x / (x.norm(dim=-1, keepdim=True) + 1e-5)).to(td)
    del x
    pos = torch.arange(L, device=DEV)[None]
    st = torch.as_tensor(SAMPLE, device=DEV)
    ragged = []
    for m, edge in enumerate(((128, 1, 17, 64, 100, 33, 96, 5, 128, 80, 49), (90, 128, 3, 40, 16, 112, 7, 128, 60, 31, 128))):
        lens = torch.randint(113, L + 1, (NV,), device=DEV, generator=g)       # eight blocks of 16: the packed image stays whole
        lens[st] = torch.as_tensor([edge[i % len(edge)] for i in range(len(SAMPLE))], device=DEV)
        ragged.append((pos < lens[:, None]).float().contiguous())
    masks = dict(ragged=ragged, ones=[torch.ones_like(m) for m in ragged],
                 soft=[(m * 0.5 + 0.5 * (m > 0) * (pos % 2 == 0)).contiguous() for m in ragged])
    q = [torch.nn.functional.normalize(torch.randn(NQ, H, device=DEV, generator=g), dim=-1).to(torch.bfloat16).to(td).contiguous()
         for _ in range(2)]
    hg = torch.Generator().manual_seed(7)
    cols = sorted(set(SAMPLE) | set(torch.randperm(NV, generator=hg)[:64].tolist()))      # + 64 random columns
    cols_t = torch.as_tensor(cols, device=DEV)
    d = dict(dt=dt, td=td, es=LO.ES[dt], c=c, masks=masks, q=q, sample_t=st, cols=cols, cols_t=cols_t,
             c_cols=c[cols_t].float().cpu(), q_host=[t.float().cpu() for t in q], refs={})
    _BIG["corpus"] = d
    return d


# ---- a. K6, every operand form ----------------------------------------------------------------------------------------------
K6_KIND = {"rowmajor": "ragged", "tiled_float": "soft", "nomask": "ones", "bitmask": "ragged", "packed": "ragged"}


def k6_reference(d, kind, n_mod):
    """float64 value W and float32 oracle value R of the scores of d["cols"] (sampled + 64 random videos), per mask kind."""
    from oracle import f64
    from oracle import xml_oracle as O
    if kind not in d["refs"]:
        per = []
        for m in range(2):
            mk = d["masks"][kind][m][d["cols_t"]].cpu()
            W, _ = f64.q2c_scores(d["q_host"][m], d["c_cols"], mk)
            R = torch.max(O.mask_logits(torch.einsum("md,nld->mln", d["q_host"][m], d["c_cols"]), mk.t().unsqueeze(0)), dim=1)[0]
            per.append((W, R))
        d["refs"][kind] = per
    per = d["refs"][kind]
    if n_mod == 1:
        return per[0]
    return (per[0][0] + per[1][0]) / 2, (per[0][1] + per[1][1]) / 2


def k6_operands(ops, form, c, masks):
    """The K6 corpus operand of `form` for every modality; the modalities share the clip rows (one image) and differ in their
    queries and masks.  -> (list for ops.q2c_scores_fused, elements of the operand the kernel addresses)"""
    if form == "rowmajor":
        return [c] * len(masks), c.numel()
    if form == "packed":
        plan = ops.PackPlan(masks)
        first = ops.pack_q2c_corpus(c, masks[0], plan)
        out = [first]
        for m in masks[1:]:
            t = ops.TiledRows(first.data, first.rows, first.hidden, first.shape)
            t.plan, t.mask_bits = plan, plan.mask_bits(m)
            out.append(t)
        return out, first.data.numel()
    first = ops.pack_q2c_corpus(c, masks[0])
    out = [first]
    for m in masks[1:]:
        t = ops.TiledRows(first.data, first.rows, first.hidden, first.shape)
        t.all_valid = bool((m == 1).all())
        if not t.all_valid and bool(((m == 0) | (m == 1)).all()):
            t.mask_bits = ops._pack_bits32(m != 0)
        out.append(t)
    assert all(t.all_valid == (form == "nomask") and (t.mask_bits is not None) == (form == "bitmask") for t in out)
    return out, first.data.numel()


def k6_run(ops, form, qs, c, masks):
    cn, extent = k6_operands(ops, form, c, masks)
    out = torch.full((qs[0].shape[0], c.shape[0]), float("nan"), device=DEV)
    ops.q2c_scores_fused(qs, cn, masks, out=out)
    return out, extent


@pytest.mark.parametrize("n_mod", RC.K6_N_MOD)
@pytest.mark.parametrize("form", RC.K6_FORMS)
def test_k6_forms(ops, dtype, form, n_mod):
    """K6 on the NV_BIG corpus in each of its five operand forms, one and two modalities: the scores of the sampled videos and
    of 64 random ones against float64 (check_f32, the margin of test_q2c_near_duplicates), and the whole (300, NV_BIG) output
    bitwise the same entry on the two halves of the corpus as operands of their own, each below T3.  (Every form is bitwise
    against its halves at small sizes too: a score does not depend on where its video sits, test_q2c_length_buckets_bitwise
    and test_q2c_packed_shapes_bitwise.)  The packed image holds head-room of its own: the unsampled videos are 113 .. 128
    clips long, so it keeps > 10 922 tiles and crosses T3 like the plain image."""
    d = corpus(dtype)
    c, es, kind = d["c"], d["es"], K6_KIND[form]
    qs, masks = d["q"][:n_mod], d["masks"][kind][:n_mod]
    LO.assert_crosses(c.numel(), es, ALL)
    got, extent = k6_run(ops, form, qs, c, masks)
    LO.assert_crosses(extent, es, ALL)
    assert not bool(torch.isnan(got).any()), "a score column was never written"
    W, R = k6_reference(d, kind, n_mod)
    what = "k6 %s x%d" % (form, n_mod)
    NR.check_f32(what, "large", got[:, d["cols_t"]], W, R, C_CHAIN, scale=1.0, storage=dtype)
    if form == "rowmajor" and n_mod == 1:
        single = ops.q2c_scores(qs[0], c, masks[0], out=torch.full((NQ, NV), float("nan"), device=DEV))
        NR.check_f32("q2c_scores", "large", single[:, d["cols_t"]], W, R, C_CHAIN, scale=1.0, storage=dtype)
        assert same_bits(single, got)
        del single
    halves = []
    for lo, hi in ((0, HALF), (HALF, NV)):
        ch = c[lo:hi].clone() if form == "rowmajor" else c[lo:hi]        # (the tiled forms build an image of their own)
        out, ext = k6_run(ops, form, qs, ch, [m[lo:hi].contiguous() for m in masks])
        assert ext <= LO.thresholds(es)["T3"] and ch.numel() < LO.thresholds(es)["T3"]
        halves.append(out)
        del ch
    assert same_bits(got, torch.cat(halves, 1)), what + ": the scores differ from those of the two halves of the corpus"


# ---- b. tile passes --------------------------------------------------------------------------------------------------------
def untile(data, t0, t1, es):
    """Rows of tiles t0 .. t1-1 of a tile image back in row-major order (ops.TiledRows.to_rows on a range of tiles)."""
    per = 64 // es
    return data[t0 * 256 * H:t1 * 256 * H].view(t1 - t0, H // per, 256, per).permute(0, 2, 1, 3).reshape(-1, H)


def check_tile_image(data, src_rows, es, what):
    """The sampled tiles bitwise against the numpy restatement of the layout [tile][slice][row][64 B], and every tile, in
    chunks on the device, against its source rows (which makes the per-row sums of squares of image and source equal)."""
    for t in SAMPLE_TILES:
        got = data[t * 256 * H:(t + 1) * 256 * H].view(torch.uint8).cpu().numpy()
        rows = src_rows(t * 256, (t + 1) * 256).contiguous().view(torch.uint8).cpu().numpy()
        assert np.array_equal(got, LO.tile_image_bytes(rows, H * es)[0]), "%s: tile %d" % (what, t)
    step = 576
    for t0 in range(0, N_TILES, step):
        t1 = min(t0 + step, N_TILES)
        assert same_bits(untile(data, t0, t1, es), src_rows(t0 * 256, t1 * 256)), "%s: tiles %d .. %d" % (what, t0, t1 - 1)


def test_tile_passes(ops, dtype):
    """xml_q2c_tile_rows, xml_q2c_tile_rows_gather and xml_q2c_tile_rows_l2norm on the NV_BIG corpus.  The row map sends the
    videos in reverse order -- high source rows into low tiles and low rows into high tiles -- and leaves one video out."""
    d = corpus(dtype)
    c, es = d["c"], d["es"]
    rows = c.view(-1, H)
    LO.assert_crosses(c.numel(), es, ALL)
    img = ops.q2c_tile_rows(c)
    LO.assert_crosses(img.data.numel(), es, ALL)
    check_tile_image(img.data, lambda r0, r1: rows[r0:r1], es, "tile_rows")
    del img
    src_vid = torch.arange(NV - 1, -1, -1, device=DEV)
    row_map = (src_vid[:, None] * L + torch.arange(L, device=DEV)[None]).view(-1)
    row_map[3 * L:4 * L] = -1
    row_map[(NV - 2) * L + 5] = -1
    row_map = row_map.to(torch.int32).contiguous()

    def gathered(r0, r1):
        rm = row_map[r0:r1].long()
        x = rows[rm.clamp(min=0)]
        x[rm < 0] = 0
        return x

    img = ops._tile(c, ROWS, row_map)
    LO.assert_crosses(img.data.numel(), es, ALL)
    check_tile_image(img.data, gathered, es, "tile_rows_gather")
    del img
    for rm, src, what in ((row_map, lambda r0, r1: ops.l2norm_rows(gathered(r0, r1)), "tile_rows_l2norm + map"),
                          (None, lambda r0, r1: ops.l2norm_rows(rows[r0:r1]), "tile_rows_l2norm")):
        img = ops._tile(c, ROWS, rm, normalize=True)
        LO.assert_crosses(img.data.numel(), es, ALL)
        check_tile_image(img.data, src, es, what)       # bitwise xml_l2norm_rows, then the tiling: the header's contract
        del img


# ---- c. row-wise passes at rows x d past T3 ----------------------------------------------------------------------------------
def _raw(ops, name, *args):
    ops.check(getattr(ops._lib.load(), name)(*args), name)


def test_l2norm_rows(ops, dtype):
    """xml_l2norm_rows (and, f32, xml_l2norm_rows_eps) over the (ROWS, H) view of the corpus, outputs pre-filled with 0xFF."""
    from oracle import f64
    d = corpus(dtype)
    x, td, es = d["c"].view(-1, H), d["td"], d["es"]
    LO.assert_crosses(x.numel(), es, ALL)
    idx = video_rows(SAMPLE)
    xs = x[idx].float().cpu()
    y = filled(x.shape, td)
    _raw(ops, "xml_l2norm_rows", ops._p(x), ops._p(y), ROWS, H, ops.dt_of(x), ops._stream())
    W, R = f64.l2norm_rows(xs), torch.nn.functional.normalize(xs, dim=-1)
    if dtype == "f32":
        NR.check_f32("l2norm_rows", "large", y[idx], W, R, C_ROWWISE)
    else:   # near-unit rows: the correctly rounded float32 reference meets the strict statistics (as for post_relu_unit)
        NR.check_bf16_rounding("l2norm_rows", "large", y[idx], W, R, C_ROWWISE, strict=True)
    assert_every_row_written(y, "l2norm_rows")
    if dtype == "f32":
        y.view(-1).view(torch.uint8).fill_(0xFF)
        _raw(ops, "xml_l2norm_rows_eps", ops._p(x), ops._p(y), ROWS, H, 1e-5, ops._stream())
        NR.check_f32("l2norm_rows_eps", "large", y[idx], f64.l2norm_rows(xs, 1e-5), xs / (xs.norm(dim=-1, keepdim=True) + 1e-5),
                     C_ROWWISE)
        assert_every_row_written(y, "l2norm_rows_eps")


def test_convert(ops, dtype):
    """xml_convert of the whole corpus, f32 -> bf16 (round to nearest even) and bf16 -> f32 (exact): every element, in chunks,
    bitwise torch's conversion."""
    d = corpus(dtype)
    x, es = d["c"].view(-1, H), d["es"]
    other = torch.bfloat16 if dtype == "f32" else torch.float32
    for e in (2, 4):                                   # source and destination: one of each size
        LO.assert_crosses(x.numel(), e, ALL)
    y = filled(x.shape, other)
    _raw(ops, "xml_convert", ops._p(x), ops.dt_of(x), ops._p(y), ops.dt_of(other), x.numel(), ops._stream())
    idx = video_rows(SAMPLE)
    assert same_bits(y[idx].cpu(), x[idx].cpu().to(other))
    assert_every_row_written(y, "convert")
    step = 1152 * L
    for r0 in range(0, ROWS, step):
        assert same_bits(y[r0:r0 + step], x[r0:r0 + step].to(other)), "convert: rows %d .." % r0


def _split_ref(x, log2s):
    """hi / lo halves of x * 2^log2s as split16.hip defines them (tests/test_gpu_split16.py)."""
    xs = x.double() * 2.0 ** log2s
    hi = xs.float().half()
    hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
    r = (xs - hi.double()).float()
    lo = r.half()
    lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    return hi, lo, r


def test_split_and_unsplit_f16_rows(ops):
    """xml_split_f16_rows (split rows, hi plane, scales, error norms) and xml_unsplit_f16_rows on the f32 corpus at the fixed
    unit scale: the sampled rows against the float64 definition, as tests/test_gpu_split16.py checks 700 rows."""
    d = corpus("f32")
    x = d["c"].view(-1, H)
    LO.assert_crosses(x.numel(), 4, ALL)
    idx = video_rows(SAMPLE)
    xs = x[idx].cpu()
    y, hi = filled(x.shape, torch.int32), filled(x.shape, torch.float16)
    inv, err = filled((ROWS,), torch.float32), filled((ROWS,), torch.float32)
    LO.assert_crosses(hi.numel(), 2, ALL)
    _raw(ops, "xml_split_f16_rows", ops._p(x), ops._p(y), ops._p(inv), ops._p(hi), ops._p(err), ROWS, H, ops.F16_UNIT_LOG2,
         ops._stream())
    want_hi, want_lo, r = _split_ref(xs, 14)
    n = xs.shape[0]
    assert torch.equal(hi[idx].cpu(), want_hi)
    assert bool((inv == 2.0 ** -14).all())
    close("rounding-error norms", err[idx], (r.double().norm(dim=-1) * 2.0 ** -14).float(), 1e-10, 1e-5)
    raw = y[idx].cpu().view(torch.float16).view(n, H // 32, 2, 32)
    assert torch.equal(raw[:, :, 0].reshape(n, H), want_hi) and torch.equal(raw[:, :, 1].reshape(n, H), want_lo)
    assert_every_row_written(y, "split rows")
    assert_every_row_written(hi, "hi plane")
    assert_every_element_written(err, "error norms")
    del hi, err, x, d
    _free()                                            # the corpus: the halves alone give it back
    back = filled((ROWS, H), torch.float32)
    _raw(ops, "xml_unsplit_f16_rows", ops._p(y), ops._p(inv), ops._p(back), ROWS, H, ops._stream())
    bs = back[idx].cpu()
    assert float((bs.double() - (want_hi.double() + want_lo.double()) * 2.0 ** -14).abs().max()) == 0.0
    assert bool(((bs - xs).abs() <= 2.0 ** -21 * xs.abs() + 2.0 ** -28).all())
    assert_every_row_written(back, "unsplit rows")


def test_round_bf16_rows_err(ops):
    """xml_round_bf16_rows_err on the f32 corpus: every element bitwise torch's round to nearest even (in chunks), the error
    norms of the sampled rows as tests/test_gpu_exact.py checks them."""
    d = corpus("f32")
    x = d["c"].view(-1, H)
    LO.assert_crosses(x.numel(), 4, ALL)
    yb, err = filled(x.shape, torch.bfloat16), filled((ROWS,), torch.float32)
    LO.assert_crosses(yb.numel(), 2, ALL)
    _raw(ops, "xml_round_bf16_rows_err", ops._p(x), ops._p(yb), ops._p(err), ROWS, H, ops._stream())
    idx = video_rows(SAMPLE)
    xs = x[idx].cpu()
    want_b = xs.to(torch.bfloat16)
    assert torch.equal(yb[idx].cpu(), want_b)
    close("rounding-error norms", err[idx], (xs.double() - want_b.double()).norm(dim=-1).float(), 1e-9, 1e-5)
    assert_every_row_written(yb, "rounded rows")
    assert_every_element_written(err, "error norms")
    step = 1152 * L
    for r0 in range(0, ROWS, step):
        assert same_bits(yb[r0:r0 + step], x[r0:r0 + step].to(torch.bfloat16)), "rounded rows %d .." % r0


# ---- d. kernels that gather corpus rows by video id ----------------------------------------------------------------------------
def pair_forms(ops, d, fixed_scale):
    """The corpus as the feat2 / cn operand of the pair kernels in every storage form this dtype gives -- plain rows and, for
    f32, split-f16 rows -- each with its twin: copies of just the sampled videos, renumbered 0 .. len(SAMPLE) - 1.
    Yields (name, es, convert(query rows), big operand, twin operand); one split image is alive at a time."""
    c, st = d["c"], d["sample_t"]
    yield d["dt"], d["es"], (lambda q: q.to(d["td"]).contiguous()), c, c[st].contiguous()
    if d["dt"] == "f32":
        log2 = ops.F16_UNIT_LOG2 if fixed_scale else None
        sp = ops.split_f16_rows(c, log2)
        twin = ops.SplitRows(sp.data[st].contiguous(), sp.inv[st].contiguous())
        again = ops.split_f16_rows(c[st].contiguous(), log2)                  # the twin IS the split of the copied rows
        assert same_bits(twin.data, again.data) and same_bits(twin.inv, again.inv)
        yield "f16s", 4, (lambda q: ops.split_f16_rows(q.float().contiguous(), log2)), sp, twin


def pair_lists(nq, with_skip):
    """pair_vid (nq, K) naming the sampled videos in a different order per query, for the big corpus and for the twin."""
    g = torch.Generator().manual_seed(11)
    k = len(SAMPLE)
    tw = torch.stack([torch.randperm(k, generator=g) for _ in range(nq)]).int()
    big = torch.as_tensor(SAMPLE, dtype=torch.int32)[tw.long()]
    if with_skip:
        tw[1, 2] = big[1, 2] = -1
    return big.to(DEV).contiguous(), tw.to(DEV).contiguous()


def test_convse_rerank_twin(ops, dtype):
    """xml_convse_rerank, xml_convse_rerank_f16s and xml_convse_rerank_ex: the pairs name the sampled videos of the NV_BIG
    corpus; every output is bitwise that of the same call on the twin corpus."""
    d = corpus(dtype)
    masks, st = d["masks"]["ragged"], d["sample_t"]
    tw_masks = [m[st].contiguous() for m in masks]
    vlen = torch.stack([(m != 0).int().sum(1) for m in masks]).amax(0).int().contiguous()       # prefix masks: last valid + 1
    nq = 24
    g = torch.Generator().manual_seed(3)
    q32 = [(0.5 * torch.randn(nq, H, generator=g)).to(DEV) for _ in range(2)]
    pair_w = (torch.rand(nq, len(SAMPLE), generator=g) + 0.1).to(DEV)
    for name, es, conv, big, twin in pair_forms(ops, d, fixed_scale=False):
        LO.assert_crosses(big.numel(), es, ALL)
        qs = [conv(q) for q in q32]
        for n_mod, merged in ((2, True), (2, False), (1, False)):
            cw = torch.randn(2 * (1 if merged else n_mod) * 5, generator=g).to(DEV)
            args = lambda f, mk, p: (qs[:n_mod], [f] * n_mod, mk[:n_mod], p, cw, L, merged, 5)          # noqa: E731
            for softmax in (True, False):
                pb, pt = pair_lists(nq, with_skip=True)
                a, b = ops.convse_rerank(*args(big, masks, pb), softmax=softmax), ops.convse_rerank(*args(twin, tw_masks, pt),
                                                                                                  softmax=softmax)
                assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), (name, n_mod, merged, softmax)
            pb, pt = pair_lists(nq, with_skip=False)
            zeros = lambda: (torch.zeros(nq, len(SAMPLE), L, device=DEV), torch.zeros(nq, len(SAMPLE), L, device=DEV))  # noqa: E731
            a = ops.convse_rerank(*args(big, masks, pb), pair_w=pair_w, band=(2, 16), vid_len=vlen, out=zeros())
            b = ops.convse_rerank(*args(twin, tw_masks, pt), pair_w=pair_w, band=(2, 16), vid_len=vlen[st].contiguous(), out=zeros())
            assert all(same_bits(x, y) for x, y in zip(a, b)) and len(a) == 3, (name, n_mod, merged, "ex")
        del big, twin


def test_span_evidence_twin(ops, dtype):
    """xml_span_evidence on pairs that name the sampled videos (and one video out of range): the five rows of every pair
    bitwise those of the call on the twin corpus."""
    d = corpus(dtype)
    masks, st = d["masks"]["ragged"], d["sample_t"]
    tw_masks = [m[st].contiguous() for m in masks]
    nq, k = 7, len(SAMPLE)
    g = torch.Generator().manual_seed(4)
    q32 = [(0.5 * torch.randn(nq, H, generator=g)).to(DEV) for _ in range(2)]
    pv_tw = torch.cat([torch.randperm(k, generator=g) for _ in range(3)] + [torch.tensor([k])]).int()
    pv_big = torch.cat([torch.as_tensor(SAMPLE, dtype=torch.int32)[pv_tw[:-1].long()], torch.tensor([NV], dtype=torch.int32)])
    pq = torch.randint(0, nq, (pv_tw.numel(),), generator=g).int().to(DEV)
    for name, es, conv, big, twin in pair_forms(ops, d, fixed_scale=False):
        LO.assert_crosses(big.numel(), es, ALL)
        qs = [conv(q) for q in q32]
        for n_mod, merged in ((2, True), (1, False)):
            cw = torch.randn(2 * (1 if merged else n_mod) * 5, generator=g).to(DEV)
            a = ops.span_evidence(qs[:n_mod], [big] * n_mod, masks[:n_mod], pq, pv_big.to(DEV), cw, L, merged, 5)
            b = ops.span_evidence(qs[:n_mod], [twin] * n_mod, tw_masks[:n_mod], pq, pv_tw.to(DEV), cw, L, merged, 5)
            for x, y in zip(a, b):
                assert (x is None and y is None) or same_bits(x, y), (name, n_mod, merged)
            assert not bool(a.st_logits[-1].any()) and bool(a.st_logits[0].any())          # the pair out of range: zero rows
        del big, twin


def test_q2c_rescore_twin(ops, dtype):
    """xml_q2c_rescore (f32, bf16 and split-f16 rows at the unit scale) on listed pairs of the NV_BIG corpus: bitwise the call
    on the twin, and against float64 like test_q2c_rescore_near_duplicates."""
    d = corpus(dtype)
    masks, st = d["masks"]["ragged"], d["sample_t"]
    tw_masks = [m[st].contiguous() for m in masks]
    nq = 24
    pb, pt = pair_lists(nq, with_skip=True)
    W, R = k6_reference(d, "ragged", 2)
    col_of = {v: i for i, v in enumerate(d["cols"])}
    pick = torch.as_tensor([[col_of[int(v)] if v >= 0 else 0 for v in row] for row in pb.cpu()])
    for name, es, conv, big, twin in pair_forms(ops, d, fixed_scale=True):
        LO.assert_crosses(big.numel(), es, ALL)
        qs = [conv(q[:nq]) for q in d["q"]]
        a = ops.q2c_rescore(qs, [big, big], masks, pb)
        b = ops.q2c_rescore(qs, [twin, twin], tw_masks, pt)
        assert same_bits(a, b), name
        assert float(a[1, 2]) == float("-inf")
        ok = (pb >= 0).cpu()
        NR.check_f32("q2c_rescore", "large", a.cpu()[ok], torch.gather(W[:nq], 1, pick)[ok], torch.gather(R[:nq], 1, pick)[ok],
                     C_CHAIN, scale=1.0, storage=name)
        del big, twin


# ---- e. resident index that takes updates ---------------------------------------------------------------------------------------
class Index(object):
    """The device state of an updatable index as xml_index_put_rows[_packed] sees it (index_update.MutableCorpusIndex.create)."""

    def __init__(self, ops, cap, n_mod, td, n_tiles=None):
        self.cap, self.n_mod, self.n_tiles = cap, n_mod, n_tiles
        rows = cap * L if n_tiles is None else n_tiles * 256
        z = lambda *s, dt=td: torch.zeros(s, dtype=dt, device=DEV)          # noqa: E731
        self.k6 = [ops.TiledRows(z(ops.q2c_tiled_numel(rows, H, td)), cap * L, H, (cap, L, H)) for _ in range(n_mod)]
        self.feat2 = [z(cap, L, H) for _ in range(n_mod)]
        self.imask = [z(cap, L, dt=torch.float32) for _ in range(n_mod)]
        self.bits = [z(cap if n_tiles is None else 2 * n_tiles, 4, dt=torch.int32) for _ in range(n_mod)]
        self.codes = None if n_tiles is None else torch.full((2 * n_tiles, 8), -2, dtype=torch.int32, device=DEV)
        self.vlen = torch.full((cap,), L, dtype=torch.int32, device=DEV)
        self.slot_ids = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
        self.live = z((cap + 31) // 32, dt=torch.int32)

    def put(self, ops, batch, slots, ids, runs=None):
        f1, f2, mk = batch
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=DEV).contiguous()         # noqa: E731
        if runs is None:
            ops.index_put_rows(f1, f2, mk, i32(slots), i32(ids), self.k6, self.feat2, self.imask, self.bits, self.vlen,
                               self.slot_ids, self.live, L)
        else:
            ops.index_put_rows_packed(f1, f2, mk, i32(slots), i32(ids), i32(runs), max(nb for _, nb in runs), self.k6, self.feat2,
                                      self.imask, self.bits, self.codes, self.vlen, self.slot_ids, self.live, L)

    def clear(self, ops, slots, runs=None):
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=DEV).contiguous()         # noqa: E731
        if runs is None:
            ops.index_clear_rows(i32(slots), self.imask, self.bits, self.vlen, self.live, L)
        else:
            ops.index_clear_rows_packed(i32(slots), i32(runs), 8, self.imask, self.bits, self.codes, self.vlen, self.live, L)

    def live_bits(self, slots):
        s = torch.as_tensor(list(slots), device=DEV)
        return (self.live[s >> 5] >> (s & 31)) & 1

    def census(self):
        """Whole-extent counts: what is non-zero / set anywhere in the state."""
        def nnz(t, step=1 << 28):           # (in chunks: a reduction over 2^31 elements at once takes a temporary of 19 GB)
            t = t.view(-1)
            return sum(int((t[i:i + step] != 0).sum()) for i in range(0, t.numel(), step))
        out = [nnz(t.data) for t in self.k6] + [nnz(t) for t in self.feat2 + self.imask]
        out += [nnz(t) for t in self.bits] + [int((self.vlen != L).sum()), int((self.slot_ids != -1).sum())]
        out += [sum(bin(w & 0xFFFFFFFF).count("1") for w in self.live.cpu().tolist())]
        return out + ([] if self.codes is None else [int((self.codes != -2).sum())])


def make_batch(b, lb, td, n_mod, seed, lens=None):
    """An encoded context batch: f1 / f2 (b, lb, H) rows and prefix masks per modality (video 0 full width)."""
    g = torch.Generator().manual_seed(seed)
    f1 = [torch.randn(b, lb, H, generator=g).to(DEV).to(td).contiguous() for _ in range(n_mod)]
    f2 = [torch.randn(b, lb, H, generator=g).to(DEV).to(td).contiguous() for _ in range(n_mod)]
    mk = []
    for m in range(n_mod):
        ln = torch.randint(1, lb + 1, (b,), generator=g) if lens is None else torch.as_tensor(lens) - 3 * m
        if lens is None:
            ln[0] = lb
        mk.append((torch.arange(lb)[None] < ln[:, None]).float().to(DEV).contiguous())
    return f1, f2, mk


def slot_rows(t, slots, es):
    """(len(slots), L, H) K6 rows of the slots of a plain (two slots per tile) image."""
    return torch.stack([untile(t.data, s // 2, s // 2 + 1, es)[(s % 2) * L:(s % 2 + 1) * L] for s in slots])


def test_index_update_plain(ops, dtype):
    """xml_index_put_rows / xml_index_clear_rows on an index of capacity NV_BIG: put into the sampled slots, replace, remove.
    After every step the sampled slots hold bitwise what a twin index of len(SAMPLE) slots holds after the same calls with the
    slots renumbered, the rows are the builder's rows (F.normalize'd f1, f2, zero behind the batch width), and a census of
    the whole state finds nothing written anywhere else."""
    _free()
    td, es = TDT[dtype], LO.ES[dtype]
    n_mod = 2 if dtype == "bf16" else 1                 # (four f32 planes of this size would be 34 GB)
    b = len(SAMPLE)
    big, twin = Index(ops, NV, n_mod, td), Index(ops, b, n_mod, td)
    for t in (big.k6[0].data, big.feat2[0]):
        LO.assert_crosses(t.numel(), es, ALL)
    LO.assert_crosses(big.imask[0].numel() * H, es, "T3")
    st = torch.as_tensor(SAMPLE, device=DEV)
    ids = list(range(1000, 1000 + b))

    def agree(step):
        for m in range(n_mod):
            assert same_bits(slot_rows(big.k6[m], SAMPLE, es), slot_rows(twin.k6[m], range(b), es)), (step, m, "k6")
            assert same_bits(big.feat2[m][st], twin.feat2[m]) and same_bits(big.imask[m][st], twin.imask[m]), (step, m)
            assert torch.equal(big.bits[m][st], twin.bits[m]), (step, m, "bits")
        assert torch.equal(big.vlen[st], twin.vlen) and torch.equal(big.slot_ids[st], twin.slot_ids), step
        assert torch.equal(big.live_bits(SAMPLE), twin.live_bits(range(b))), step
        assert big.census() == twin.census(), (step, big.census(), twin.census())

    def builders_rows(batch, lb):
        f1, f2, mk = batch
        for m in range(n_mod):
            k6 = slot_rows(big.k6[m], SAMPLE, es)
            assert same_bits(k6[:, :lb], ops.l2norm_rows(f1[m])) and not bool(k6[:, lb:].any())
            assert same_bits(big.feat2[m][st][:, :lb], f2[m]) and not bool(big.feat2[m][st][:, lb:].any())
            assert torch.equal(big.imask[m][st][:, :lb], mk[m]) and not bool(big.imask[m][st][:, lb:].any())

    first = make_batch(b, 100, td, n_mod, 21)
    big.put(ops, first, SAMPLE, ids)
    twin.put(ops, first, list(range(b)), ids)
    agree("put")
    builders_rows(first, 100)
    assert int(big.live_bits(SAMPLE).sum()) == b and torch.equal(big.slot_ids[st].cpu(), torch.as_tensor(ids, dtype=torch.int32))
    short = make_batch(b, 24, td, n_mod, 22)            # a replace leaves nothing behind
    big.put(ops, short, SAMPLE, ids)
    twin.put(ops, short, list(range(b)), ids)
    agree("replace")
    builders_rows(short, 24)
    gone = [0, b // 2, b - 3, b - 1]                    # remove: the first, a middle one, the T3 straddler, the last
    big.clear(ops, [SAMPLE[i] for i in gone])
    twin.clear(ops, gone)
    agree("remove")
    assert int(big.live_bits(SAMPLE).sum()) == b - len(gone)
    gt = torch.as_tensor([SAMPLE[i] for i in gone], device=DEV)
    assert bool((big.vlen[gt] == L).all()) and not bool(big.imask[0][gt].any()) and not bool(big.bits[0][gt].any())


def test_index_update_packed_and_compact(ops, dtype):
    """xml_index_put_rows_packed / _clear_rows_packed / xml_index_move_blocks_packed and the packed K6 on an image of 10 944
    tiles (past T3) that is almost empty: runs in the first tile, the last tile and the tiles that hold a threshold (with
    their neighbours).  put, a compaction plan that moves one run from the last tile into the first and slides one inside the
    T3 tile, replace and remove: after every step tiles, codes, mask words and the per-slot state are bitwise those of a twin
    image that holds just the sampled tiles, renumbered, and K6 scores the live slots alike on both."""
    _free()
    td, es, n_mod, cap = TDT[dtype], LO.ES[dtype], 2, 64
    tiles = SAMPLE_TILES
    tmap = {t: i for i, t in enumerate(tiles)}
    big, twin = Index(ops, cap, n_mod, td, N_TILES), Index(ops, cap, n_mod, td, len(tiles))
    LO.assert_crosses(big.k6[0].data.numel(), es, ALL)
    per = 256 * H
    low, t3, high = tiles[0], LO.straddler(LO.thresholds(es)["T3"], per), tiles[-1]
    assert t3 in tmap and low == 0 and high == N_TILES - 1

    def twin_block(g):
        return tmap[g >> 4] * 16 + (g & 15)

    def agree(step):
        for m in range(n_mod):
            for t in tiles:
                u = tmap[t]
                assert same_bits(big.k6[m].data[t * per:(t + 1) * per], twin.k6[m].data[u * per:(u + 1) * per]), (step, m, t)
                assert torch.equal(big.bits[m][2 * t:2 * t + 2], twin.bits[m][2 * u:2 * u + 2]), (step, m, t, "bits")
            assert same_bits(big.feat2[m], twin.feat2[m]) and same_bits(big.imask[m], twin.imask[m]), (step, m)
        for t in tiles:
            assert torch.equal(big.codes[2 * t:2 * t + 2], twin.codes[2 * tmap[t]:2 * tmap[t] + 2]), (step, t, "codes")
        assert torch.equal(big.vlen, twin.vlen) and torch.equal(big.slot_ids, twin.slot_ids) and torch.equal(big.live, twin.live)
        assert big.census() == twin.census(), (step, big.census(), twin.census())
        outs = []
        for ix in (big, twin):
            plan = types.SimpleNamespace(slot_ids=ix.codes, n_tiles=ix.n_tiles, n_videos=cap)
            for m in range(n_mod):
                ix.k6[m].plan, ix.k6[m].mask_bits = plan, ix.bits[m]
            out = torch.full((NQ, cap), float("nan"), device=DEV)
            ops.q2c_scores_fused(qs, ix.k6, ix.imask, out=out)
            outs.append(out)
        assert same_bits(*outs), (step, "packed K6")
        return outs[0]

    g = torch.Generator().manual_seed(9)
    qs = [torch.nn.functional.normalize(torch.randn(NQ, H, generator=g), dim=-1).to(DEV).to(td).contiguous() for _ in range(n_mod)]
    # two runs per sampled tile: blocks 0 .. 2 and 6 .. 9 (across the two wave tiles)
    slots = list(range(2 * len(tiles)))
    runs = [r for t in tiles for r in ((t * 16, 3), (t * 16 + 6, 4))]
    lens = [nb * 16 - 5 for _, nb in runs]
    batch = make_batch(len(slots), 64, td, n_mod, 31, lens)
    ids = [500 + s for s in slots]
    big.put(ops, batch, slots, ids, runs)
    twin.put(ops, batch, slots, ids, [(twin_block(f), nb) for f, nb in runs])
    out = agree("put")
    assert not bool(torch.isnan(out[:, :len(slots)]).any()) and bool(torch.isnan(out[:, len(slots):]).all())
    # compaction: the 4-block run of the last tile into blocks 10 .. 13 of the first; the 4-block run of the T3 tile slides
    # from blocks 6 .. 9 to 3 .. 6, over its own old blocks
    rec_low = [low] + [-1] * 16
    rec_low[1 + 10:1 + 14] = range(high * 16 + 6, high * 16 + 10)
    rec_t3 = [t3] + [-1] * 16
    rec_t3[1 + 3:1 + 7] = range(t3 * 16 + 6, t3 * 16 + 10)
    rec_t3[1 + 7:1 + 10] = [-2] * 3
    for ix, conv in ((big, lambda x: x), (twin, twin_block)):
        recs = [[tmap[r[0]] if ix is twin else r[0]] + [conv(x) if x >= 0 else x for x in r[1:]] for r in (rec_low, rec_t3)]
        ops.index_move_blocks_packed(torch.as_tensor(recs, dtype=torch.int32, device=DEV).contiguous(), ix.k6, ix.bits, ix.codes)
        ix.clear(ops, [-1], [(conv(high * 16 + 6), 4)])                              # the vacated run alone
    moved = agree("compact")
    assert same_bits(moved[:, :len(slots)], out[:, :len(slots)]), "a score changed when its video moved"
    code = big.codes.view(-1)
    hi_slot, t3_slot = 2 * tmap[high] + 1, 2 * tmap[t3] + 1
    assert int(code[low * 16 + 13]) == hi_slot and int(code[t3 * 16 + 6]) == t3_slot and int(code[high * 16 + 9]) == -2
    # replace: the 3-block videos of three tiles by 2-block ones (old run freed, slot -1, then the put); remove two videos
    t1 = LO.straddler(LO.thresholds(es)["T1"], per)
    who = [2 * tmap[t] for t in (t1, t3, high)]
    new_runs = [((t * 16, 2)) for t in (t1, t3, high)]
    short = make_batch(3, 32, td, n_mod, 32, [27, 20, 32])
    for ix, conv in ((big, lambda x: x), (twin, twin_block)):
        ix.clear(ops, [-1] * 3, [(conv(f), 3) for f, _ in new_runs])
        ix.put(ops, short, who, [900, 901, 902], [(conv(f), nb) for f, nb in new_runs])
    agree("replace")
    for ix, conv in ((big, lambda x: x), (twin, twin_block)):
        ix.clear(ops, [0, hi_slot], [(conv(low * 16), 3), (conv(low * 16 + 10), 4)])
    agree("remove")
    assert int(big.live_bits([0, hi_slot]).sum()) == 0 and int(code[low * 16 + 13]) == -2


def test_index_chains(ops):
    """xml_index_set_chains on the tables of an index of capacity NV_BIG: a chain whose slots lie on both sides of every
    threshold of the slot space (slot x 128 x 768 elements).  test_score_strides folds scores over these chains."""
    _free()
    LO.assert_crosses(NV * L * H, 2, ALL)
    head = torch.arange(NV, dtype=torch.int32, device=DEV)
    nxt = torch.full((NV,), -1, dtype=torch.int32, device=DEV)
    off = torch.zeros(NV, dtype=torch.int32, device=DEV)
    want = [t.clone() for t in (head, nxt, off)]
    chain = [SAMPLE[1], SAMPLE[-2], SAMPLE[-1], SAMPLE[len(SAMPLE) // 2], 0]
    recs = [[s, chain[0], chain[i + 1] if i + 1 < len(chain) else -1, 90 * i] for i, s in enumerate(chain)] + [[NV, 0, 0, 0]]
    for s, h, n, o in recs[:-1]:
        want[0][s], want[1][s], want[2][s] = h, n, o
    ops.index_set_chains(torch.as_tensor(recs, dtype=torch.int32, device=DEV), head, nxt, off)
    assert all(torch.equal(a, b) for a, b in zip((head, nxt, off), want))            # (the record out of range wrote nothing)


# ---- f. whole searches --------------------------------------------------------------------------------------------------------
BATCH = 2048                    # the corpus is encoded in context batches of 2048 videos (the last one holds 1408)
ALLOWED = sorted(set(SAMPLE) | set(torch.randperm(NV, generator=torch.Generator().manual_seed(5))[:13].tolist()))
SEARCH_KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
SEARCH_KW = dict(max_vcmr_video=10, max_before_nms=60)
_WORLD = {}


def search_world(dt):
    """Model (H = 768; bf16: video + subtitles, f32: video only -- six f32 planes of this size would be 51 GB), queries, the
    clip counts of the NV_BIG videos, and the TWIN: the fixed index of the ALLOWED videos alone (24 of them: a context batch
    of >= 16 videos, so that its rows are bitwise those of any other batch that holds them) with its unrestricted search."""
    if _WORLD.get("dt") == dt:
        return _WORLD
    from test_gpu_model import _feats, _synthetic_model
    from tvretrieval_amd import inference as inf
    _WORLD.clear()
    m, _ = _synthetic_model("video_sub" if dt == "bf16" else "video", H, 256, 128, 128, L, TDT[dt], seed=70)
    lens = torch.randint(16, L + 1, (NV,), generator=torch.Generator().manual_seed(6))
    lens[::BATCH] = L
    qf, qm = _feats(40, np.concatenate([[30], np.random.default_rng(8).integers(3, 31, 39)]), 128, 9)
    _WORLD.update(dt=dt, m=m, lens=lens, qf=qf.to(DEV), qm=qm.to(DEV), sub=dt == "bf16")
    rows = []
    for b0 in sorted({v // BATCH * BATCH for v in ALLOWED}):
        sel = torch.as_tensor([v - b0 for v in ALLOWED if v // BATCH * BATCH == b0], device=DEV)
        rows.append([None if t is None else t.index_select(0, sel) for t in raw_batch(_WORLD, b0)])
    twin_batch = tuple(None if ts[0] is None else torch.cat(ts).contiguous() for ts in zip(*rows))
    with torch.no_grad():
        twin = inf.build_corpus_index(m, [twin_batch], l_ref=L, n_videos=len(ALLOWED), length_buckets=False)
        want = inf.vcmr_search(m, twin, _WORLD["qf"], _WORLD["qm"], **SEARCH_KW)
    allow = np.zeros((1, NV), dtype=bool)
    allow[0, ALLOWED] = True
    _WORLD.update(want={k: want[k].clone() for k in SEARCH_KEYS}, allow=inf.pack_video_allow(torch.from_numpy(allow).to(DEV)))
    return _WORLD


def raw_batch(w, b0):
    """Context batch b0 .. b0 + 2047 of the corpus: randn on the device under the batch's own seed, dataset normalisation, on
    the bf16 grid, zero beyond each video's clip count.  The same call gives the same rows (the twin is made from them)."""
    n = min(BATCH, NV - b0)
    g = torch.Generator(device=DEV).manual_seed(9000 + b0)
    mask = (torch.arange(L)[None] < w["lens"][b0:b0 + n, None]).float().to(DEV)

    def feat(dim):
        x = torch.randn(n, L, dim, device=DEV, generator=g)
        return ((x / (x.norm(dim=-1, keepdim=True) + 1e-5)).to(torch.bfloat16).float() * mask[..., None]).contiguous()

    vf = feat(256)
    return (vf, mask, feat(128), mask) if w["sub"] else (vf, mask, None, None)


def corpus_batches(w):
    return (raw_batch(w, b0) for b0 in range(0, NV, BATCH))


def check_search(w, index, what):
    """vcmr_search(video_allow = the ALLOWED videos) on the NV_BIG index == the unrestricted search on the twin index,
    record for record, in the big index's numbering."""
    from tvretrieval_amd import inference as inf
    with torch.no_grad():
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], video_allow=w["allow"], **SEARCH_KW)
    want = w["want"]
    ids = torch.as_tensor(ALLOWED, dtype=torch.int32, device=DEV)
    assert torch.equal(got["top_indices"], ids[want["top_indices"].long()]), what + ": video lists"
    assert same_bits(got["top_scores"], want["top_scores"]), what + ": video scores"
    assert torch.equal(got["flat_indices"], want["flat_indices"]) and same_bits(got["flat_scores"], want["flat_scores"]), \
        what + ": moments"
    assert bool((want["flat_indices"] >= 0).all()) and bool((want["top_indices"] >= 0).all())


@pytest.mark.parametrize("form", ["tiled-bf16", "tiled-f32", "bucketed-bf16"])
def test_search_on_a_fixed_index(form):
    """The fixed index of NV_BIG videos -- plain tiled (bf16 and f32 model) and length-bucketed -- searched under the allow bits
    of the sampled videos: the unrestricted search on the corpus of the allowed videos, which is the stated contract."""
    from tvretrieval_amd import inference as inf
    _free()
    kind, dt = form.split("-")
    w = search_world(dt)
    with torch.no_grad():
        index = inf.build_corpus_index(w["m"], corpus_batches(w), l_ref=L, n_videos=NV, length_buckets=kind == "bucketed")
    for mod in index.modalities:
        LO.assert_crosses(index.feat2[mod].numel(), LO.ES[dt], ALL)
        assert isinstance(index.feat1n[mod], ops_module().TiledRows) and (index.feat1n[mod].plan is not None) == (kind == "bucketed")
    if kind == "tiled":
        LO.assert_crosses(index.feat1n["video"].data.numel(), LO.ES[dt], ALL)
    check_search(w, index, form)
    del index


@pytest.mark.parametrize("form", ["plain", "packed"])
def test_search_on_an_index_that_takes_updates(form):
    """index_update.MutableCorpusIndex of capacity NV_BIG, filled batch by batch, plain and over 10 944 tiles: the same
    search equals the twin's."""
    from tvretrieval_amd.index_update import MutableCorpusIndex
    _free()
    w = search_world("bf16")
    kw = dict(tiles=N_TILES) if form == "packed" else {}
    index = MutableCorpusIndex.from_batches(w["m"], corpus_batches(w), NV, l_ref=L, n_clips=w["lens"].tolist(), **kw)
    assert index.n_live == NV
    for mod in index.modalities:
        LO.assert_crosses(index.feat2[mod].numel(), 2, ALL)
        LO.assert_crosses(index.feat1n[mod].data.numel(), 2, ALL)
    check_search(w, index, form)
    del index


def test_search_on_a_parts_index():
    """A parts index whose NV_BIG index rows are the parts of 13 680 source videos (1, 2, 1, 3, 1 parts, repeating): the
    search under the allow bits of the source videos that own the ALLOWED rows equals the unrestricted search on the twin
    parts index built from those videos alone -- rows, source videos, scores and moments."""
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd.ingest import PartTable
    _free()
    w = search_world("bf16")
    sizes = np.tile([1, 2, 1, 3, 1], NV // 8)
    gs = np.concatenate([[0], np.cumsum(sizes)])
    pv = np.repeat(np.arange(len(sizes)), sizes)
    po = (np.arange(NV) - gs[:-1][pv]) * (L - 16)
    lens = w["lens"].numpy()
    table = PartTable(pv, po, lens, gs, L, 16)
    assert table.n_parts == NV and table.n_videos == 13680
    vids = sorted({int(pv[r]) for r in ALLOWED})
    rows = [r for v in vids for r in range(gs[v], gs[v + 1])]
    tsz = sizes[vids]
    tgs = np.concatenate([[0], np.cumsum(tsz)])
    twin_table = PartTable(np.repeat(np.arange(len(vids)), tsz), po[rows], lens[rows], tgs, L, 16)
    parts = []
    for b0 in sorted({r // BATCH * BATCH for r in rows}):
        sel = torch.as_tensor([r - b0 for r in rows if r // BATCH * BATCH == b0], device=DEV)
        parts.append([t.index_select(0, sel) for t in raw_batch(w, b0)])
    twin_batch = tuple(torch.cat(ts).contiguous() for ts in zip(*parts))
    allow = np.zeros((1, table.n_videos), dtype=bool)
    allow[0, vids] = True
    with torch.no_grad():
        twin = inf.build_corpus_index(w["m"], [twin_batch], l_ref=L, n_videos=len(rows), parts=twin_table)
        want = inf.vcmr_search(w["m"], twin, w["qf"], w["qm"], **SEARCH_KW)
        index = inf.build_corpus_index(w["m"], corpus_batches(w), l_ref=L, n_videos=NV, parts=table)
        for mod in index.modalities:
            LO.assert_crosses(index.feat2[mod].numel(), 2, ALL)
        got = inf.vcmr_search(w["m"], index, w["qf"], w["qm"], video_allow=inf.pack_video_allow(torch.from_numpy(allow).to(DEV)),
                              **SEARCH_KW)
    row_of = torch.as_tensor(rows, dtype=torch.int32, device=DEV)
    vid_of = torch.as_tensor(vids, dtype=torch.int32, device=DEV)
    assert bool((want["top_indices"] >= 0).all()) and len(rows) >= 16
    assert torch.equal(got["top_indices"], row_of[want["top_indices"].long()]), "index rows"
    assert torch.equal(got["top_videos"], vid_of[want["top_videos"].long()]), "source videos"
    assert same_bits(got["top_scores"], want["top_scores"]) and same_bits(got["flat_scores"], want["flat_scores"])
    assert torch.equal(got["flat_indices"], want["flat_indices"])
    del index


def ops_module():
    from tvretrieval_amd import ops as o
    return o


# ---- g. stores ------------------------------------------------------------------------------------------------------------------
# which video of numerics_regimes.ingest_case(11, 128, 768) each sampled video holds: their lengths become
# 32 | 16 13 32 | 128 90 1 | 84 83 35 | 27, so that the store rows at 2^30 and 2^31 elements belong to sampled videos
STORE_PERM = (4, 5, 6, 7, 0, 3, 1, 2, 9, 10, 8)


def store():
    """An f16 feature store of ROWS x H (past T3): post-ReLU rows on the device; the clip rows of the sampled videos are those of
    numerics_regimes.ingest_case (ragged lengths, a video of one clip, an all-zero row), copied in from the host."""
    s = _BIG.get("store")
    if s is not None:
        return s
    _free()
    g = torch.Generator(device=DEV).manual_seed(77)
    src = torch.empty((ROWS, H), dtype=torch.float16, device=DEV)
    step = 1152 * L
    for r0 in range(0, ROWS, step):
        src[r0:r0 + step] = (torch.relu(torch.randn(step, H, device=DEV, generator=g)) * 0.7).half()
    case = NR.ingest_case(len(SAMPLE), L, H)
    assert case["lens"].tolist() == [128, 1, 84, 90, 32, 16, 13, 32, 27, 83, 35] and len(SAMPLE) == len(STORE_PERM)
    perm = torch.as_tensor(STORE_PERM)
    lens = torch.full((NV,), L, dtype=torch.int64)
    lens[torch.as_tensor(SAMPLE)] = case["lens"][perm]
    short = 0
    for i, v in enumerate(SAMPLE):          # the video behind each group of sampled ones holds the rows they are short of
        short += L - int(lens[v])           # (more than max_len rows: the first 128 are kept), so every other video starts
        if v + 1 < NV and (i + 1 == len(SAMPLE) or SAMPLE[i + 1] != v + 1):         # at row 128 v, as in the destination
            lens[v + 1] += short
            short = 0
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    assert int(row_start[-1]) <= ROWS and int(row_start[SAMPLE[-1]]) == SAMPLE[-1] * L
    for i, v in enumerate(SAMPLE):
        j = STORE_PERM[i]
        src[int(row_start[v]):int(row_start[v + 1])] = case["src"][int(case["row_start"][j]):int(case["row_start"][j + 1])].to(DEV)
    s = dict(src=src, row_start=row_start.to(DEV), lens=lens, case=case, perm=perm)
    _BIG["store"] = s
    return s


@pytest.mark.parametrize("out_dtype", ["bf16", "f32"])
def test_ingest_rows(ops, out_dtype):
    """xml_ingest_rows: the source is addressed through row_start past T3 and the (NV, 128, 768) destination lies past T3; the
    sampled videos against float64 as in test_ingest_rows_vs_float64, every destination row written, the masks whole."""
    s = store()
    td, case, perm = TDT[out_dtype], s["case"], s["perm"]
    LO.assert_crosses(int(s["row_start"][SAMPLE[-1]]) * H, 2, ALL)          # where the last video starts in the store
    for t in LO.thresholds(2).values():                                     # the store rows at the thresholds are sampled ones
        holder = int(torch.searchsorted(s["row_start"], torch.as_tensor([t // H], device=DEV), right=True)) - 1
        assert holder in SAMPLE and int(s["lens"][holder]) <= L, (t, holder)
    dst, mask = filled((NV, L, H), td), filled((NV, L), torch.float32)
    LO.assert_crosses(dst.numel(), LO.ES[out_dtype], ALL)
    _raw(ops, "xml_ingest_rows", ops._p(s["src"]), ops.dt_of(s["src"]), ops._p(s["row_start"]), ops._p(dst), ops.dt_of(td),
         ops._p(mask), NV, L, H, L, 1e-5, 1, ops._stream())
    st = torch.as_tensor(SAMPLE, device=DEV)
    got, want_mask = dst[st], case["mask"][perm]
    assert torch.equal(mask[st].cpu(), want_mask)
    assert bool((got.float().cpu()[want_mask == 0] == 0).all())
    if out_dtype == "f32":
        NR.check_f32("ingest_rows", "large", got, case["W"][perm], case["R"][perm], C_ROWWISE)
    else:
        NR.check_bf16_rounding("ingest_rows", "large", got, case["W"][perm], case["R"][perm], C_ROWWISE)
    assert_every_row_written(dst.view(-1, H), "ingest_rows")
    assert torch.equal(mask.sum(1).long().cpu(), s["lens"].clamp(max=L)) and bool(((mask == 0) | (mask == 1)).all())


def test_gather_feature_rows(ops):
    """xml_gather_feature_rows from the f16 store past T3: ids name its first, straddling and last items; without
    normalisation the rows are bitwise the store's, indexed with torch."""
    s = store()
    LO.assert_crosses(s["src"].numel(), 2, ALL)
    items = SAMPLE[::-1] + [1]                                  # (item 1 holds more rows than max_len: the first 128 are kept)
    ids = torch.as_tensor(items + [NV], dtype=torch.int32, device=DEV)                # one id out of range: an empty item
    out, mask, ln = ops.gather_feature_rows(s["src"], s["row_start"], ids, L, L, normalize=False)
    rs = s["row_start"].cpu()
    for i, v in enumerate(items):
        n = min(int(s["lens"][v]), L)
        assert int(ln[i]) == n and int(mask[i].sum()) == n and bool(mask[i, :n].all())
        assert torch.equal(out[i, :n], s["src"][int(rs[v]):int(rs[v]) + n].float()) and not bool(out[i, n:].any()), v
    assert int(ln[-1]) == 0 and not bool(out[-1].any()) and not bool(mask[-1].any())


def test_gather_index_rows(ops):
    """xml_gather_index_rows from an int64 table of 524 800 x 4096 entries (past 2^31 elements): bitwise torch's indexing."""
    _free()
    w, n_rows = 4096, 2 ** 31 // 4096 + 512
    LO.assert_crosses(n_rows * w, 8, "T3")
    table = torch.arange(n_rows * w, dtype=torch.int64, device=DEV).view(n_rows, w)
    at = 2 ** 31 // w
    ids = [0, at - 1, at, at + 1, n_rows - 1, n_rows, -1]
    got = ops.gather_index_rows(table, torch.as_tensor(ids, dtype=torch.int32, device=DEV))
    assert torch.equal(got[:5], table[torch.as_tensor(ids[:5], device=DEV)]) and not bool(got[5:].any())


# ---- h. score-side strides ------------------------------------------------------------------------------------------------------
def test_score_strides(ops):
    """Every entry that takes a leading dimension of score rows, allow words or output words: 3 rows with ld = 2^30 + 64, so
    that the last row starts past 2^31 elements (8 GiB into the buffer); only 3 x n elements are ever written.  The results are
    bitwise those of the contiguous call on the same rows (select_ge returns its columns in unspecified order: as sets)."""
    _free()
    lib = ops._lib.load()
    rows, n, k = 3, 5000, 100
    LO.assert_crosses(2 * LD_BIG + n, 4, ALL)
    g = torch.Generator().manual_seed(13)
    A = torch.empty(2 * LD_BIG + 8192, dtype=torch.float32, device=DEV)
    B = torch.empty(2 * LD_BIG + 8192, dtype=torch.int32, device=DEV)

    def view(buf, cols, offset=0):
        return torch.as_strided(buf, (rows, cols), (LD_BIG, 1), offset)

    # K6's ld_out first (it writes into A): xml_q2c_scores on a small corpus, out rows LD_BIG apart
    nv = 37
    cn = torch.nn.functional.normalize(torch.randn(nv, L, H, generator=g), dim=-1).to(DEV).to(torch.bfloat16)
    qn = torch.nn.functional.normalize(torch.randn(rows, H, generator=g), dim=-1).to(DEV).to(torch.bfloat16)
    mk = NR.prefix_masks(nv, L).to(DEV)
    out = view(A, nv)
    out.fill_(float("nan"))
    _raw(ops, "xml_q2c_scores", ops._p(qn), ops._p(cn), ops._p(mk), ops._p(out), LD_BIG, rows, nv, L, H, 0, ops.dt_of(qn),
         ops._stream())
    assert same_bits(out.contiguous(), ops.q2c_scores(qn, cn, mk))

    sc = view(A, n)
    sc.copy_(torch.randn(rows, n, generator=g).to(DEV))
    flat = sc.contiguous()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)                      # noqa: E731
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)                    # noqa: E731
    ws = ops._workspace(lib.xml_topk_rows_workspace_bytes(rows, n, k), sc.device)

    # xml_topk_rows, with a payload matrix at the same stride
    pay = view(B, n)
    pay.copy_(torch.stack([torch.randperm(n, generator=g) for _ in range(rows)]).int().to(DEV))
    pflat = pay.contiguous()
    for alpha in (0.0, 20.0):
        res = []
        for s_, p_, ld in ((sc, pay, LD_BIG), (flat, pflat, n)):
            v, i = f32(rows, k), i32(rows, k)
            _raw(ops, "xml_topk_rows", ops._p(s_), ld, ops._p(p_), ops._p(v), ops._p(i), rows, n, k, alpha, ops._p(ws), ws.numel(),
                 ops._stream())
            res.append((v, i))
        assert same_bits(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), alpha

    # xml_topk_rows_allowed / xml_select_ge_rows[_allowed]: the allow words LD_BIG apart as well
    col0 = 7
    words = (col0 + n + 31) // 32
    allow = view(B, words)
    allow.copy_(torch.randint(-2 ** 31, 2 ** 31, (rows, words), generator=g).int().to(DEV))
    aflat = allow.contiguous()
    res = []
    for s_, a_, ld, lda in ((sc, allow, LD_BIG, LD_BIG), (flat, aflat, n, words)):
        v, i, cnt = f32(rows, k), i32(rows, k), i32(rows)
        _raw(ops, "xml_topk_rows_allowed", ops._p(s_), ld, None, ops._p(a_), lda, rows, col0, ops._p(v), ops._p(i), ops._p(cnt),
             rows, n, k, 20.0, ops._p(ws), ws.numel(), ops._stream())
        res.append((v, i, cnt))
    assert all(same_bits(x, y) for x, y in zip(*res)) and bool((res[0][2] == k).all())
    thr = flat.topk(60, dim=1)[0][:, -1].contiguous()
    cap = 64
    res = []
    for s_, a_, ld, lda in ((sc, allow, LD_BIG, LD_BIG), (flat, aflat, n, words)):
        idx, cnt = torch.full((rows, cap), -1, dtype=torch.int32, device=DEV), i32(rows)
        _raw(ops, "xml_select_ge_rows", ops._p(s_), ld, ops._p(thr), ops._p(idx), cap, ops._p(cnt), rows, n, ops._stream())
        idx2, cnt2 = torch.full((rows, cap), -1, dtype=torch.int32, device=DEV), i32(rows)
        _raw(ops, "xml_select_ge_rows_allowed", ops._p(s_), ld, ops._p(thr), ops._p(a_), lda, rows, col0, ops._p(idx2), cap,
             ops._p(cnt2), rows, n, ops._stream())
        res.append((idx.sort(1)[0], cnt, idx2.sort(1)[0], cnt2))
    assert all(torch.equal(x, y) for x, y in zip(*res)) and bool((res[0][1] == 60).all()) and bool((res[0][3] > 0).all())

    # the folds of a parts index: xml_group_best_allow / xml_best_part_rows
    sizes = torch.randint(1, 5, (n,), generator=g)
    sizes = sizes[:int((sizes.cumsum(0) <= n).sum())]
    sizes[-1] += n - int(sizes.sum())
    n_videos = sizes.numel()
    parts = types.SimpleNamespace(part_video=torch.repeat_interleave(torch.arange(n_videos), sizes).int().to(DEV).contiguous(),
                                  group_start=torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).int().to(DEV).contiguous())
    vwords = (n_videos + 31) // 32
    vallow = view(B, vwords)
    vallow.copy_(torch.randint(-2 ** 31, 2 ** 31, (rows, vwords), generator=g).int().to(DEV))
    a, b = ops.group_best_allow(sc, parts, vallow), ops.group_best_allow(flat, parts, vallow.contiguous())
    assert torch.equal(a, b) and bool(a.any())
    video = torch.as_tensor([0, n_videos - 1, 17], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.best_part_rows(sc, parts, video), ops.best_part_rows(flat, parts, video))
    # ... with the output words LD_BIG apart too (behind the allow words of each row of B)
    ob = view(B, (n + 31) // 32, 4096)
    _raw(ops, "xml_group_best_allow", ops._p(sc), LD_BIG, rows, n, ops._p(parts.part_video), ops._p(parts.group_start), n_videos,
         ops._p(vallow), LD_BIG, rows, ops._p(ob), LD_BIG, ops._stream())
    assert torch.equal(ob.contiguous(), a)

    # the folds of an updatable index with chains: xml_chain_best_allow / xml_chain_best_rows over n slots
    chains = types.SimpleNamespace(chain_head=torch.arange(n, dtype=torch.int32, device=DEV),
                                   chain_next=torch.full((n,), -1, dtype=torch.int32, device=DEV), max_parts=32)
    off = torch.zeros(n, dtype=torch.int32, device=DEV)
    recs = []
    for ch in ([3, 4999, 2500, 17], [100, 101], [4000, 7, 4998]):
        recs += [[s, ch[0], ch[i + 1] if i + 1 < len(ch) else -1, 90 * i] for i, s in enumerate(ch)]
    ops.index_set_chains(torch.as_tensor(recs, dtype=torch.int32, device=DEV), chains.chain_head, chains.chain_next, off)
    sallow = view(B, (n + 31) // 32)
    sallow.fill_(-1)
    a, b = ops.chain_best_allow(sc, chains, sallow), ops.chain_best_allow(flat, chains, sallow.contiguous())
    assert torch.equal(a, b)
    for r in range(rows):                                  # exactly one bit per chain: its best part
        for ch in ([3, 4999, 2500, 17], [100, 101], [4000, 7, 4998]):
            best = max(ch, key=lambda s: (float(flat[r, s]), -ch.index(s)))
            assert [int(a[r, s >> 5]) >> (s & 31) & 1 for s in ch] == [int(s == best) for s in ch], (r, ch)
    video = torch.as_tensor([4999, 101, 7], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.chain_best_rows(sc, chains, video), ops.chain_best_rows(flat, chains, video))
    ob = view(B, (n + 31) // 32, 4096)
    ob.fill_(0)
    _raw(ops, "xml_chain_best_allow", ops._p(sc), LD_BIG, rows, n, ops._p(chains.chain_head), ops._p(chains.chain_next), 32,
         ops._p(sallow), LD_BIG, rows, ops._p(ob), LD_BIG, ops._stream())
    assert torch.equal(ob.contiguous(), a)


# ---- registry: every symbol of the four public headers has a large-offset case or one of the four reasons ---------------------
_K6, _TILE = ["test_k6_forms"], ["test_tile_passes"]
_PLAIN, _PACKED = ["test_index_update_plain"], ["test_index_update_packed_and_compact"]
LARGE_CASES = {
    "xml_q2c_scores": _K6 + ["test_score_strides"], "xml_q2c_scores_fused": _K6, "xml_q2c_scores_tiled": _K6,
    "xml_q2c_scores_packed": _K6 + _PACKED,
    "xml_q2c_tile_rows": _TILE + _K6, "xml_q2c_tile_rows_gather": _TILE + _K6, "xml_q2c_tile_rows_l2norm": _TILE,
    "xml_l2norm_rows": ["test_l2norm_rows"], "xml_l2norm_rows_eps": ["test_l2norm_rows"], "xml_convert": ["test_convert"],
    "xml_split_f16_rows": ["test_split_and_unsplit_f16_rows"], "xml_unsplit_f16_rows": ["test_split_and_unsplit_f16_rows"],
    "xml_round_bf16_rows_err": ["test_round_bf16_rows_err"],
    "xml_convse_rerank": ["test_convse_rerank_twin"], "xml_convse_rerank_f16s": ["test_convse_rerank_twin"],
    "xml_convse_rerank_ex": ["test_convse_rerank_twin"], "xml_span_evidence": ["test_span_evidence_twin"],
    "xml_q2c_rescore": ["test_q2c_rescore_twin"],
    "xml_index_put_rows": _PLAIN, "xml_index_clear_rows": _PLAIN,
    "xml_index_put_rows_packed": _PACKED, "xml_index_clear_rows_packed": _PACKED, "xml_index_move_blocks_packed": _PACKED,
    "xml_index_set_chains": ["test_index_chains", "test_score_strides"],
    "xml_chain_best_allow": ["test_score_strides"], "xml_chain_best_rows": ["test_score_strides"],
    "xml_group_best_allow": ["test_score_strides"], "xml_best_part_rows": ["test_score_strides"],
    "xml_topk_rows": ["test_score_strides"], "xml_topk_rows_allowed": ["test_score_strides"],
    "xml_select_ge_rows": ["test_score_strides"], "xml_select_ge_rows_allowed": ["test_score_strides"],
    "xml_ingest_rows": ["test_ingest_rows"], "xml_gather_feature_rows": ["test_gather_feature_rows"],
    "xml_gather_index_rows": ["test_gather_index_rows"],
}

LARGE_EXEMPT = {}
LARGE_EXEMPT.update({s: NO_DEVICE for s in (
    "xml_abi_version", "xml_build_arch", "xml_status_string", "xml_linear_ln_relu_pos_workspace_bytes",
    "xml_attention_block_workspace_bytes", "xml_linear_ln_relu_pos_packed_workspace_bytes",
    "xml_attention_block_varlen_workspace_bytes", "xml_cross_attention_workspace_bytes", "xml_q2c_tiled_ok",
    "xml_q2c_tile_rows_l2norm_ok", "xml_q2c_tiled_bytes", "xml_topk_rows_workspace_bytes", "xml_q2c_rescore_workspace_bytes",
    "xml_pack_weights_f16s_bytes", "xml_linear_f16s_workspace_bytes", "xml_convse_rerank_workspace_bytes",
    "xml_span_evidence_workspace_bytes", "xml_gemm_tn_supported", "xml_attention_train_supported",
    "xml_q2c_scores_l2norm_bwd_supported", "xml_layernorm_bwd_partials_bytes", "xml_rccl_available", "xml_rccl_unique_id",
    "xml_rccl_comm_init", "xml_rccl_comm_destroy", "xml_rccl_allgather_topk_workspace_bytes",
    "xml_rccl_topk_by_owner_workspace_bytes", "xml_merge_shard_topk_workspace_bytes", "xml_nms_vcmr_host", "xml_nms_svmr_host",
    "xml_nms_vcmr_batched_host", "xml_nms_svmr_batched_host", "xml_dispatch_const", "xml_dispatch_gemm",
    "xml_dispatch_gemm_rules", "xml_dispatch_gemm_kloop", "xml_dispatch_q2c", "xml_dispatch_q2c_fused", "xml_dispatch_q2c_walk",
    "xml_dispatch_attention", "xml_dispatch_l2norm", "xml_dispatch_convse_shape", "xml_dispatch_convse_pairs")})
# the encoders, the query side and everything behind K8 see a batch of videos or queries (and the model's weights), never the
# resident corpus: their row counts are those of tests/test_gpu_fullsize.py at most
LARGE_EXEMPT.update({s: BATCH_ONLY for s in (
    "xml_pack_weights", "xml_linear_ln_relu_pos", "xml_attention_block", "xml_attention_core", "xml_pack_plan",
    "xml_linear_ln_relu_pos_packed", "xml_attention_block_varlen", "xml_modular_pool_varlen", "xml_cross_attention",
    "xml_modular_pool", "xml_modular_pool_att", "xml_modular_pool_att_varlen", "xml_linear", "xml_linear_add",
    "xml_exact_certificate", "xml_pack_weights_f16s", "xml_linear_f16s", "xml_moment_topk", "xml_moment_topk_ex",
    "xml_conv1d_rows", "xml_moments_decode", "xml_moments_decode_parts", "xml_nms_moments", "xml_eval_moments",
    "xml_add_layernorm", "xml_merge_shard_topk")})
LARGE_EXEMPT.update({s: TRAINING for s in (
    "xml_transpose_batched", "xml_colsum", "xml_relu_bwd", "xml_add_inplace", "xml_layernorm_bwd", "xml_gemm_batched",
    "xml_split_heads", "xml_merge_heads", "xml_attn_softmax", "xml_gemm_tn", "xml_attention_train_fwd",
    "xml_attention_train_bwd", "xml_modular_pool_bwd", "xml_l2norm_bwd", "xml_q2c_scores_bwd", "xml_q2c_scores_l2norm_bwd",
    "xml_q2c_scores_l2norm_bwd_multi", "xml_q2c_scores_arg", "xml_loss_combine", "xml_loss_combine_bwd", "xml_pair_sim",
    "xml_pair_sim_bwd", "xml_span_loss", "xml_rank_loss", "xml_dropout", "xml_transpose_segments", "xml_add_layernorm_drop",
    "xml_layernorm_bwd_drop", "xml_layernorm_bwd_drop_ws", "xml_clip_grad_norm", "xml_bert_adam_step")})
LARGE_EXEMPT.update({s: COLLECTIVE for s in (
    "xml_rccl_allgather", "xml_rccl_allreduce_avg_f32", "xml_rccl_allgather_topk", "xml_rccl_topk_by_owner")})
