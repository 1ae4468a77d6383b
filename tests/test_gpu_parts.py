"""Videos longer than max_ctx_l, indexed in parts and ranked by the best part: the fold between K6 and
K8 (ops.group_best_allow / best_part_rows), the clip offset in K10 (ops.moments_decode(part_offset=)), and whole searches on a
parts index -- by definition the restricted search over the index rows that allows exactly each query's best parts."""
import copy

import numpy as np
import pytest
import torch

from oracle import xml_oracle as O
from oracle.listcmp import moment_keys, tie_aware_equal
from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops
from tvretrieval_amd.ingest import plan_parts
from tvretrieval_amd.results import MOMENT_DTYPE

pytestmark = pytest.mark.gpu

KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")
W, OV, CLIP = 32, 8, 1.5
# 1 / 1 / 2 / 2 / 3 / 3 / 8 parts per length at W = 32, O = 8; 992 clips are 41 parts.  The order puts the 41 parts on index rows
# 30 .. 70 (they begin in word 0, fill word 1 and end in word 2) and a 200-clip video on rows 94 .. 101 (across row 96).
LENS = [5, 32, 33, 56, 57, 80, 200, 200, 33, 992, 57, 80, 56, 200, 5, 32, 33, 57, 200, 80, 56, 5, 200]
SEED = 74         # chosen on the CPU with the oracle alone: no query of this world has two best parts of a video within the
#                   video tolerance (seeds 0 .. 11 have 3 .. 11 such queries of 37: the 992-clip video has 41 parts to tie among)
_CACHE = {}


def _best_mask(scores, table):
    """Torch / numpy restatement of the fold: (R, P) bool, True where column p holds the maximum of its video's columns, the
    first such column on ties; a NaN counts as -inf (it never wins)."""
    s = scores.detach().float().cpu().numpy().copy()
    s[np.isnan(s)] = -np.inf
    gs = np.asarray(table.group_start.cpu() if torch.is_tensor(table.group_start) else table.group_start)
    out = np.zeros(s.shape, dtype=bool)
    rows = np.arange(s.shape[0])
    for v in range(len(gs) - 1):
        b, e = int(gs[v]), int(gs[v + 1])
        out[rows, b + np.argmax(s[:, b:e], axis=1)] = True         # (np.argmax: the first of equal maxima)
    return out


def _part_batch(feat, lens, table, dim):
    """The parts of (n_videos, Lmax, dim) padded features as a padded batch (n_parts, W, dim) + mask."""
    x = torch.zeros(table.n_parts, table.max_ctx_len, dim)
    m = torch.zeros(table.n_parts, table.max_ctx_len)
    for p in range(table.n_parts):
        v, o, l = int(table.part_video[p]), int(table.part_offset[p]), int(table.part_len[p])
        x[p, :l] = feat[v, o:o + l]
        m[p, :l] = 1
    return x, m


def _world():
    """f32, hidden 128, max_ctx_l 32, overlap 8, 37 queries; built once, with the plain twin of the index (the same rows
    without the part table)."""
    if "w" in _CACHE:
        return _CACHE["w"]
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, W, torch.float32, seed=60 + SEED)
    table = plan_parts(np.array(LENS), W, OV)
    vf, _ = _feats(len(LENS), LENS, 256, 70 + SEED)
    sf, _ = _feats(len(LENS), LENS, 128, 80 + SEED)
    rng = np.random.default_rng(90 + SEED)
    qf, qm = _feats(37, np.concatenate([[30], rng.integers(3, 31, 36)]), 128, 100 + SEED)
    pvf, pvm = _part_batch(vf, LENS, table, 256)
    psf, psm = _part_batch(sf, LENS, table, 128)
    bs = 48                                                          # three batches, the last one short
    batches = [(pvf[b:b + bs].to(DEV), pvm[b:b + bs].to(DEV), psf[b:b + bs].to(DEV), psm[b:b + bs].to(DEV))
               for b in range(0, table.n_parts, bs)]
    with torch.no_grad():
        index = inf.build_corpus_index(m, batches, parts=table)
    plain = copy.copy(index)
    plain.parts, plain.n_source_videos = None, plain.n_videos
    w = dict(m=m, cfg=cfg, table=table, index=index, plain=plain, pvf=pvf, pvm=pvm, psf=psf, psm=psm, qf=qf.to(DEV),
             qm=qm.to(DEV), qf_cpu=qf, qm_cpu=qm, nq=37, kw=dict(max_vcmr_video=10, max_before_nms=60, max_pred_l=OV))
    _CACHE["w"] = w
    return w


def _bits(mask):
    return inf.pack_video_allow(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV))


def _np_records(fs, fi, top_i, row2vid, off, l_ref, clip, seconds, row_vid=None):
    """K10 in numpy float32 arithmetic, written as the reference writes it (xml/inference.py:415-439, :229-233) with the part's
    clip offset added to the integer indices first."""
    fs, fi = np.asarray(fs), np.asarray(fi).astype(np.int64)
    ok = fi >= 0
    f = np.where(ok, fi, 0)
    r, rem = f // (l_ref * l_ref), f % (l_ref * l_ref)
    st_idx, ed_idx = rem // l_ref, rem % l_ref
    row = np.take_along_axis(np.asarray(top_i).astype(np.int64), r, 1) if row_vid is None else \
        np.broadcast_to(np.asarray(row_vid).astype(np.int64)[:, None], f.shape)
    st_idx, ed_idx = st_idx + np.asarray(off)[row], ed_idx + np.asarray(off)[row]
    if seconds:
        st = st_idx.astype(np.float32) * clip
        ed = ed_idx.astype(np.float32) * clip + clip
    else:
        st, ed = st_idx.astype(np.float32), (ed_idx + 1).astype(np.float32)
    assert st.dtype == np.float32 and ed.dtype == np.float32
    rec = np.zeros(fi.shape, dtype=MOMENT_DTYPE)
    rec["vid"] = np.where(ok, np.asarray(row2vid)[row], -1)
    rec["st"], rec["ed"], rec["score"] = np.where(ok, st, 0), np.where(ok, ed, 0), np.where(ok, fs, 0)
    return rec, ok.sum(1).astype(np.int32)


def _host(rec):
    return rec.cpu().numpy().view(MOMENT_DTYPE)[..., 0]


def _same_records(got, want, what=""):
    for col in ("vid", "st", "ed", "score"):
        np.testing.assert_array_equal(got[col].view(np.int32), want[col].view(np.int32), err_msg="%s %s" % (what, col))


# ---------------------------------------------------------------------------------------------------------
# 1. the fold kernels against the restatement
# ---------------------------------------------------------------------------------------------------------
def test_the_layout_exercises_the_word_boundaries():
    t = plan_parts(np.array(LENS), W, OV)
    gs = t.group_start
    assert t.n_parts % 32 != 0 and t.n_parts == 116
    b, e = int(gs[9]), int(gs[10])
    assert e - b == 41 and b // 32 == 0 and (e - 1) // 32 == 2                 # starts in word 0, spans word 1, ends in word 2
    assert any(gs[v] // 32 != (gs[v + 1] - 1) // 32 and gs[v + 1] - gs[v] <= 8 for v in range(t.n_videos))   # a short straddler


@pytest.mark.parametrize("rows", [1, 3, 37])
@pytest.mark.parametrize("allow", [None, "shared", "per_row"])
def test_group_best_allow_and_best_part_rows_match_the_restatement(rows, allow):
    t = plan_parts(np.array(LENS), W, OV)
    d = t.to(DEV)
    n_parts, nv = t.n_parts, t.n_videos
    rng = np.random.default_rng(rows * 7 + (0 if allow is None else len(allow)))
    ld = n_parts + 5                                                            # ld > n_parts
    buf = torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32))
    s = buf[:, :n_parts]
    gs = t.group_start
    s[:, gs[9] + 3] = 5.0                                                       # exact ties at the maximum: a duplicated column
    s[:, gs[9] + 20] = s[:, gs[9] + 3]                                          # in another word (rows 33 and 50)
    s[:, gs[3] + 1] = s[:, gs[3]]                                               # ... and a whole group tied
    s[:, gs[6]:gs[7]] = -float("inf")                                           # a video of nothing but -inf
    s[:, gs[7] + 2] = -float("inf")                                             # a -inf column among finite ones
    s[:, gs[13]] = float("nan")                                                 # NaN in the first part of a group
    s[:, gs[18] + 5] = float("nan")                                             # ... and in the middle of one
    if rows > 1:
        s[1, gs[9]:gs[10]] = 0.25                                               # all 41 parts tied in one row
    dev = buf.to(DEV)[:, :n_parts]
    assert dev.stride(0) == ld
    best = _best_mask(s, t)
    assert best.sum(1).tolist() == [nv] * rows
    allowed = None
    if allow is not None:
        allowed = rng.random((1 if allow == "shared" else rows, nv)) < 0.6
        allowed[:, 9] = True
        allowed[-1, 4] = False                                                  # a video with no allowed part
        if allow == "per_row" and rows > 1:
            allowed[0] = False                                                  # a row that allows nothing
    got = ops.group_best_allow(dev, d, None if allowed is None else _bits(allowed))
    want = best if allowed is None else best & np.broadcast_to(allowed, (rows, nv))[:, t.part_video]
    assert got.dtype == torch.int32 and tuple(got.shape) == (rows, (n_parts + 31) // 32)
    g = got.cpu().numpy()
    assert (g == inf.pack_video_allow(want)).all()
    assert ((g[:, -1].view(np.uint32) >> np.uint32(n_parts % 32)) == 0).all()   # padding bits of the last word
    if allowed is not None:
        assert not want[-1, gs[4]:gs[5]].any()
    video = torch.from_numpy(rng.integers(0, nv, rows).astype(np.int32))
    video[0] = 9
    if rows > 2:
        video[1], video[2] = -1, nv                                             # out of range on both sides
    rows_got = ops.best_part_rows(dev, d, video.to(DEV)).cpu().numpy()
    for r in range(rows):
        v = int(video[r])
        want_row = -1 if not 0 <= v < nv else int(gs[v] + np.argmax(best[r, gs[v]:gs[v + 1]]))
        assert rows_got[r] == want_row, (r, v)


def test_fold_ops_validate_their_arguments():
    t = plan_parts(np.array(LENS), W, OV)
    d = t.to(DEV)
    s = torch.zeros((3, t.n_parts), device=DEV)
    with pytest.raises(ValueError, match="columns"):
        ops.group_best_allow(s[:, :-1].contiguous(), d)
    with pytest.raises(ValueError, match="allow"):
        ops.group_best_allow(s, d, torch.zeros((2, 1), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="allow"):
        ops.group_best_allow(s, d, torch.zeros((1, 1), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="part_video"):
        ops.group_best_allow(s, t)                                              # the host table
    with pytest.raises(ValueError, match="video"):
        ops.best_part_rows(s, d, torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(Exception, match="float32"):
        ops.group_best_allow(s.double(), d)


# ---------------------------------------------------------------------------------------------------------
# 2. K10 with a clip offset against numpy float32 arithmetic
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seconds", [True, False])
@pytest.mark.parametrize("clip", [1.5, 0.1])
def test_moments_decode_with_part_offsets_is_numpy_float32_arithmetic(seconds, clip):
    nq, n, k, l_ref, n_rows = 5, 300, 4, 32, 40
    rng = np.random.default_rng(5)
    fi = rng.integers(0, k * l_ref * l_ref, (nq, n)).astype(np.int32)
    fi[:, 250:] = -1
    fi[3, 10:] = -1
    fs = rng.random((nq, n)).astype(np.float32)
    top_i = rng.integers(0, n_rows, (nq, k)).astype(np.int32)
    off = rng.integers(0, 961, n_rows).astype(np.int32)
    off[top_i[0, 0]] = 0
    off[top_i[1, 1]] = (1 << 24) + 1        # the sum is formed in integers: f32(st_idx + offset), not f32(st_idx) + f32(offset)
    row2vid = rng.permutation(1000)[:n_rows].astype(np.int32)
    dev = lambda a: torch.from_numpy(a).to(DEV)          # noqa: E731
    rec, cnt = ops.moments_decode(dev(fs), flat=dev(fi), top_idx=dev(top_i), meta2vid=dev(row2vid), l_ref=l_ref,
                                  clip_length=clip, seconds=seconds, part_offset=dev(off))
    want, want_cnt = _np_records(fs, fi, top_i, row2vid, off, l_ref, clip, seconds)
    _same_records(_host(rec), want, "VCMR")
    assert (cnt.cpu().numpy() == want_cnt).all()
    # SVMR form: one index row per query
    row_vid = rng.integers(0, n_rows, nq).astype(np.int32)
    fi1 = np.where(fi >= 0, fi % (l_ref * l_ref), -1).astype(np.int32)
    rec, cnt = ops.moments_decode(dev(fs), flat=dev(fi1), row_vid=dev(row_vid), meta2vid=dev(row2vid), l_ref=l_ref,
                                  clip_length=clip, seconds=seconds, part_offset=dev(off))
    want, want_cnt = _np_records(fs, fi1, None, row2vid, off, l_ref, clip, seconds, row_vid=row_vid)
    _same_records(_host(rec), want, "SVMR")
    # part_offset=None is bitwise the call without the keyword, and a table of zeros changes nothing
    a, ac = ops.moments_decode(dev(fs), flat=dev(fi), top_idx=dev(top_i), meta2vid=dev(row2vid), l_ref=l_ref,
                               clip_length=clip, seconds=seconds)
    b, bc = ops.moments_decode(dev(fs), flat=dev(fi), top_idx=dev(top_i), meta2vid=dev(row2vid), l_ref=l_ref,
                               clip_length=clip, seconds=seconds, part_offset=None)
    z, zc = ops.moments_decode(dev(fs), flat=dev(fi), top_idx=dev(top_i), meta2vid=dev(row2vid), l_ref=l_ref,
                               clip_length=clip, seconds=seconds, part_offset=dev(np.zeros(n_rows, dtype=np.int32)))
    assert torch.equal(a, b) and torch.equal(ac, bc) and torch.equal(a, z) and torch.equal(ac, zc)
    want0, _ = _np_records(fs, fi, top_i, row2vid, np.zeros(n_rows, dtype=np.int32), l_ref, clip, seconds)
    _same_records(_host(a), want0, "no offsets")
    with pytest.raises(ValueError, match="part_offset"):
        ops.moments_decode(dev(fs), flat=dev(fi), top_idx=dev(top_i), meta2vid=dev(row2vid), l_ref=l_ref,
                           part_offset=dev(off[:-1].copy()))


# ---------------------------------------------------------------------------------------------------------
# 3. a search on a parts index IS the restricted search over the rows that allows each query's best parts
# ---------------------------------------------------------------------------------------------------------
def _search(w, index, nq=None, **kw):
    nq = w["nq"] if nq is None else nq
    with torch.no_grad():
        return inf.vcmr_search(w["m"], index, w["qf"][:nq].contiguous(), w["qm"][:nq].contiguous(), **dict(w["kw"], **kw))


def _check_against_plain(w, got, nq, allowed=None, nms=None):
    """got = a search on the parts index -> (the best-part mask derived in numpy from got["q2c"], ANDed with the caller's
    source-video mask; the plain twin's search restricted to it)."""
    table = w["table"]
    mask = _best_mask(got["q2c"], table)
    if allowed is not None:
        mask &= np.broadcast_to(allowed, (nq, table.n_videos))[:, table.part_video]
    return mask, _search(w, w["plain"], nq, video_allow=_bits(mask), nms_thd=nms)


@pytest.mark.parametrize("nms", [None, 0.5])
@pytest.mark.parametrize("nq", [1, 3, 37])
def test_search_on_parts_is_the_restricted_search_over_the_best_parts(nq, nms):
    w = _world()
    t = w["table"]
    got = _search(w, w["index"], nq, nms_thd=nms)
    mask, want = _check_against_plain(w, got, nq, nms=nms)
    for k in KEYS + ("q2c",):
        assert torch.equal(got[k], want[k]), k
    ti = got["top_indices"].cpu().numpy()
    assert (ti >= 0).all() and mask[np.arange(nq)[:, None], ti].all()
    tv = got["top_videos"].cpu().numpy()
    assert (tv == t.part_video[ti]).all()
    assert all(len(set(r.tolist())) == len(r) for r in tv)                      # no video takes two slots
    assert (got["flat_indices"] >= 0).any()
    if nms is None:
        assert "records" not in got
        return
    # records: the numpy K10 of the PLAIN search's lists, moved into whole-video terms; NMS sees ordinary records
    l_ref = w["index"].l_ref
    rec, cnt = _np_records(want["flat_scores"].cpu().numpy(), want["flat_indices"].cpu().numpy(), ti, t.part_video,
                           t.part_offset, l_ref, CLIP, True)
    _same_records(_host(got["records"]), rec, "records")
    assert (got["record_count"].cpu().numpy() == cnt).all()
    nrec, nidx, ncnt = ops.nms_moments(got["records"], got["record_count"], True, nms, max_before=60, max_after=100)
    assert torch.equal(got["nms_records"], nrec) and torch.equal(got["nms_index"], nidx) and torch.equal(got["nms_count"], ncnt)
    assert (_host(got["records"])["st"] > W * CLIP).any()                         # moments beyond the first max_ctx_l clips


def test_search_on_parts_bf16_packed_rows():
    """max_ctx_l = 100, bf16, hidden 256: the rows take the packed (length-bucketed, lpad 128) K6 image."""
    lens = [100, 101, 250, 60, 184, 30, 333, 17, 116]
    m, cfg = _synthetic_model("video_sub", 256, 256, 128, 128, 100, torch.bfloat16, seed=77)
    t = plan_parts(np.array(lens), 100)
    assert t.overlap == 16 and t.n_parts == 1 + 2 + 3 + 1 + 2 + 1 + 4 + 1 + 2
    vf, _ = _feats(len(lens), lens, 256, 78)
    sf, _ = _feats(len(lens), lens, 128, 79)
    qf, qm = _feats(9, [30, 4, 9, 17, 22, 5, 12, 28, 8], 128, 80)
    pvf, pvm = _part_batch(vf, lens, t, 256)
    psf, psm = _part_batch(sf, lens, t, 128)
    with torch.no_grad():
        index = inf.build_corpus_index(m, [(pvf.to(DEV), pvm.to(DEV), psf.to(DEV), psm.to(DEV))], parts=t)
    assert index.lpad == 128 and index.n_videos == t.n_parts and index.n_source_videos == len(lens)
    assert isinstance(index.feat1n["video"], ops.TiledRows)                     # K6's tiled image
    plain = copy.copy(index)
    plain.parts, plain.n_source_videos = None, plain.n_videos
    kw = dict(max_vcmr_video=6, max_before_nms=50, nms_thd=0.5)
    with torch.no_grad():
        got = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), **kw)
        mask = _best_mask(got["q2c"], t)
        want = inf.vcmr_search(m, plain, qf.to(DEV), qm.to(DEV), video_allow=_bits(mask), **kw)
    for k in KEYS + ("q2c",):
        assert torch.equal(got[k], want[k]), k
    ti = got["top_indices"].cpu().numpy()
    rec, cnt = _np_records(want["flat_scores"].cpu().numpy(), want["flat_indices"].cpu().numpy(), ti, t.part_video,
                           t.part_offset, index.l_ref, CLIP, True)
    _same_records(_host(got["records"]), rec, "records")
    assert (got["top_videos"].cpu().numpy() == t.part_video[ti]).all()


# ---------------------------------------------------------------------------------------------------------
# 4. against the oracle: per query, its search over the sub-corpus of that query's best parts
# ---------------------------------------------------------------------------------------------------------
VIDEO_TOL, MOMENT_TOL = 4e-3, 1e-3          # test_restricted_pass_against_the_oracle_on_the_sub_corpus's (on exp(20 s) / products)


def _oracle(w):
    """The oracle's per-part numbers (a part is a video: the corpus of parts defines them), once."""
    if "oracle" not in _CACHE:
        om = O.OracleXML(w["cfg"], {k: v.detach().cpu() for k, v in w["m"].state_dict().items()})
        with torch.no_grad():
            v1, v2, s1, s2 = om.encode_context(w["pvf"], w["pvm"], w["psf"], w["psm"])
            _CACHE["oracle"] = om.get_pred_from_raw_query(w["qf_cpu"], w["qm_cpu"], v1, v2, w["pvm"], s1, s2, w["psm"],
                                                          cross=True)
    return _CACHE["oracle"]


def _excluded(q2c, table):
    """Queries in which the two best parts of some video lie closer than the video tolerance: exp(20 a) and exp(20 b) within
    VIDEO_TOL relative, |a - b| <= VIDEO_TOL / 20 -- the oracle's own f32 scores cannot name the best part there."""
    s = q2c.numpy()
    bad = np.zeros(len(s), dtype=bool)
    for v in range(table.n_videos):
        b, e = int(table.group_start[v]), int(table.group_start[v + 1])
        if e - b > 1:
            top2 = np.sort(s[:, b:e], axis=1)[:, -2:]
            bad |= (top2[:, 1] - top2[:, 0]) <= VIDEO_TOL / 20.0
    return bad


def test_search_on_parts_against_the_oracle():
    w = _world()
    t, kv, l, n_mom, nq = w["table"], 10, W, 60, w["nq"]
    q2c, st, ed = _oracle(w)
    excl = _excluded(q2c, t)
    print("oracle: %d of %d queries have two best parts of a video within the tolerance: %s"
          % (excl.sum(), nq, np.nonzero(excl)[0].tolist()))
    assert excl.mean() <= 0.05
    best = _best_mask(q2c, t)
    got = _search(w, w["index"])
    gi, gs_ = got["top_indices"].cpu().numpy(), got["top_scores"].cpu().numpy()
    fs, fi = got["flat_scores"].cpu().numpy(), got["flat_indices"].cpu().numpy()
    n_same = 0
    for q in np.nonzero(~excl)[0]:
        sel = np.nonzero(best[q])[0]                                            # this query's sub-corpus: one row per video
        assert len(sel) == t.n_videos >= kv + 6
        with torch.no_grad():
            want = O.vcmr_tail(q2c[q:q + 1, sel], st[q:q + 1, sel], ed[q:q + 1, sel], 20.0, kv, 2, OV, n_mom + 16)
        assert np.isin(gi[q], sel).all(), q
        ww, wi2 = torch.topk(torch.exp(20.0 * q2c[q:q + 1, sel]), kv + 6, dim=1)
        tie_aware_equal(gi[q:q + 1], gs_[q:q + 1], sel[wi2.numpy()], ww.numpy(), kv, VIDEO_TOL, "videos of query %d" % q)
        wi = sel[want["top_indices"].numpy()]
        if not (gi[q:q + 1] == wi).all():
            continue
        n_same += 1
        gk, wk = moment_keys(fi[q:q + 1], gi[q:q + 1], l), moment_keys(want["flat_indices"].numpy(), wi, l)
        ws = want["flat_scores"].numpy()
        npos = int((ws[0][:n_mom] > 0).sum())
        assert int((fi[q] >= 0).sum()) == npos, (q, npos)
        if npos > 2:
            tie_aware_equal(gk[:, :npos], fs[q:q + 1, :npos], wk, ws, max(1, npos - 2), MOMENT_TOL, "moments of query %d" % q)
    assert n_same >= 0.8 * nq


# ---------------------------------------------------------------------------------------------------------
# 5. reachability: a moment beyond the first max_ctx_l clips is found; the truncated corpus cannot return it
# ---------------------------------------------------------------------------------------------------------
def test_a_moment_late_in_a_long_video_is_reachable():
    """A planted query: 48 random 32-clip segments are scored against it by the ORACLE (a segment alone is a video, and a part
    is a video, so the part at offset 168 of the long video scores exactly what its segment scores).  The best segment becomes
    clips 168 .. 199 of a 200-clip video whose other clips come from the worst segments; the other videos are middling
    segments.  Only through that late part can the long video win."""
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, W, torch.float32, seed=91)
    n_seg = 48
    pv, pm = _feats(n_seg, [W] * n_seg, 256, 92)
    ps, _ = _feats(n_seg, [W] * n_seg, 128, 93)
    qf, qm = _feats(1, [12], 128, 94)
    om = O.OracleXML(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        v1, v2, s1, s2 = om.encode_context(pv, pm, ps, pm)
        seg_score = om.get_pred_from_raw_query(qf, qm, v1, v2, pm, s1, s2, pm, cross=True)[0][0].numpy()
    order = np.argsort(seg_score)                                               # ascending
    worst, best, others = order[:6], order[-1], order[20:30]
    assert seg_score[best] - seg_score[others].max() > 1e-3                     # (f32 scores agree to ~1e-6)
    long_v = torch.cat([pv[i] for i in worst[:5]] + [pv[worst[5]][:8], pv[best]])          # 5 * 32 + 8 + 32 = 200 clips
    long_s = torch.cat([ps[i] for i in worst[:5]] + [ps[worst[5]][:8], ps[best]])
    assert long_v.shape[0] == 200
    x_id = 3                                                                    # the long video's place in the corpus
    vids_v = [pv[i] for i in others[:x_id]] + [long_v] + [pv[i] for i in others[x_id:]]
    vids_s = [ps[i] for i in others[:x_id]] + [long_s] + [ps[i] for i in others[x_id:]]
    lens = [int(v.shape[0]) for v in vids_v]
    t = plan_parts(np.array(lens), W, OV)
    assert t.part_offset[t.group_start[x_id + 1] - 1] == 168
    pad = lambda vs, d: torch.stack([torch.cat([v, v.new_zeros(200 - v.shape[0], d)]) for v in vs])   # noqa: E731
    fv, fs_ = pad(vids_v, 256), pad(vids_s, 128)
    pvf, pvm = _part_batch(fv, lens, t, 256)
    psf, psm = _part_batch(fs_, lens, t, 128)
    video_ids = torch.arange(1000, 1000 + len(lens), dtype=torch.int32, device=DEV)       # the caller's ids
    kw = dict(max_vcmr_video=1, max_before_nms=20, max_pred_l=OV, nms_thd=0.5, meta2vid=video_ids, clip_length=CLIP)
    first = torch.from_numpy(t.group_start[:-1].astype(np.int64))               # part 0 of a video = its first 32 clips
    with torch.no_grad():
        index = inf.build_corpus_index(m, [(pvf.to(DEV), pvm.to(DEV), psf.to(DEV), psm.to(DEV))], parts=t)
        cut = inf.build_corpus_index(m, [(pvf[first].to(DEV), pvm[first].to(DEV), psf[first].to(DEV), psm[first].to(DEV))])
        got = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), **kw)
        trunc = inf.vcmr_search(m, cut, qf.to(DEV), qm.to(DEV), **kw)
    assert int(got["top_videos"][0, 0]) == x_id
    row = int(got["top_indices"][0, 0])
    assert t.part_video[row] == x_id and t.part_offset[row] >= 120              # a part that holds planted clips
    top = _host(got["nms_records"])[0, 0]
    assert top["vid"] == 1000 + x_id and top["st"] > W * CLIP and top["st"] >= t.part_offset[row] * CLIP
    assert top["ed"] <= 200 * CLIP
    # the corpus cut to max_ctx_l clips per video: the long video is the WORST match, and nothing beyond 48 s exists
    assert int(trunc["top_indices"][0, 0]) != x_id
    tr = _host(trunc["records"])[0][: int(trunc["record_count"][0])]
    assert (tr["vid"] != 1000 + x_id).all() and (tr["ed"] <= W * CLIP).all()


# ---------------------------------------------------------------------------------------------------------
# 6. masks and SVMR in source numbering, the host path, the refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
def test_video_allow_numbers_source_videos(shared):
    w = _world()
    t, nq = w["table"], w["nq"]
    rng = np.random.default_rng(31)
    allowed = rng.random((1 if shared else nq, t.n_videos)) < 0.7
    allowed[:, 9] = True
    if not shared:
        allowed[2] = False
        allowed[2, [9, 4, 0]] = True                                            # fewer allowed videos than K
        allowed[5] = False                                                      # none at all
    got = _search(w, w["index"], video_allow=_bits(allowed))
    mask, want = _check_against_plain(w, got, nq, allowed=allowed)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    tv = got["top_videos"].cpu().numpy()
    al = np.broadcast_to(allowed, (nq, t.n_videos))
    for q in range(nq):
        live = tv[q][tv[q] >= 0]
        assert al[q, live].all() and len(live) == min(10, int(al[q].sum())), q
    with pytest.raises(ValueError, match="video_allow"):                        # 1 or Nq rows
        _search(w, w["index"], video_allow=torch.zeros((3, 4), dtype=torch.int32, device=DEV))
    assert (t.n_videos + 31) // 32 == 1                                         # one word of SOURCE videos is enough
    got1 = _search(w, w["index"], video_allow=torch.full((1, 1), -1, dtype=torch.int32, device=DEV))
    free = _search(w, w["index"])
    for k in KEYS:
        assert torch.equal(got1[k], free[k]), k


def test_svmr_video_names_source_videos():
    w = _world()
    t, nq = w["table"], w["nq"]
    rng = np.random.default_rng(37)
    vids = rng.integers(0, t.n_videos, nq).astype(np.int32)
    vids[:3] = [9, 0, 6]
    sv = torch.from_numpy(vids).to(DEV)
    got = _search(w, w["index"], svmr_video=sv, nms_thd=0.5)
    best = _best_mask(got["q2c"], t)
    rows = np.array([t.group_start[v] + np.argmax(best[q, t.group_start[v]:t.group_start[v + 1]]) for q, v in enumerate(vids)])
    assert (got["svmr_rows"].cpu().numpy() == rows).all()
    want = _search(w, w["plain"], svmr_video=torch.from_numpy(rows.astype(np.int32)).to(DEV), nms_thd=0.5)
    for k in ("svmr_scores", "svmr_flat", "svmr_st", "svmr_ed"):
        assert torch.equal(got[k], want[k]), k
    rec, cnt = _np_records(want["svmr_scores"].cpu().numpy(), want["svmr_flat"].cpu().numpy(), None, t.part_video,
                           t.part_offset, w["index"].l_ref, CLIP, False, row_vid=rows)
    _same_records(_host(got["svmr_records"]), rec, "svmr records")
    assert (_host(got["svmr_records"])["vid"][:, 0] == vids).all()


def test_host_to_host_search_on_parts():
    w = _world()
    t, nq = w["table"], w["nq"]
    video_ids = torch.arange(500, 500 + t.n_videos, dtype=torch.int32, device=DEV)
    allowed = np.random.default_rng(43).random((nq, t.n_videos)) < 0.6
    kw = dict(max_vcmr_video=10, max_before_nms=60, max_pred_l=OV)
    for bits in (None, _bits(allowed)):
        one = _search(w, w["index"], video_allow=bits, nms_thd=0.5, meta2vid=video_ids)
        with torch.no_grad():
            rec, cnt = inf.vcmr_search_host(w["m"], w["index"], query_feat=w["qf_cpu"].pin_memory(),
                                            query_mask=w["qm_cpu"].pin_memory(), meta2vid=video_ids, clip_length=CLIP,
                                            video_allow=bits, **kw)
        want, want_cnt = _host(one["records"]), one["record_count"].cpu().numpy()
        np.testing.assert_array_equal(cnt, want_cnt)
        live = np.arange(rec.shape[1])[None] < cnt[:, None]
        for col in ("vid", "st", "ed", "score"):
            np.testing.assert_array_equal(np.where(live, rec[col], 0), np.where(live, want[col], 0), err_msg=col)
        assert ((rec["vid"][live] >= 500) & (rec["vid"][live] < 500 + t.n_videos)).all()
        assert (rec["st"][live] > W * CLIP).any()


def test_the_refusals():
    w = _world()
    free = _search(w, w["index"])
    with torch.no_grad():
        with pytest.raises(ValueError, match="exact"):
            inf.build_corpus_index(w["m"], [(w["pvf"].to(DEV), w["pvm"].to(DEV), w["psf"].to(DEV), w["psm"].to(DEV))],
                                   parts=w["table"], exact_filter=True)
        with pytest.raises(ValueError, match="external_top"):
            _search(w, w["index"], external_top=(free["top_indices"], free["top_scores"]))
        with pytest.raises(ValueError, match="max_pred_l"):
            _search(w, w["index"], max_pred_l=OV + 1)
        with pytest.raises(ValueError, match="max_pred_l"):
            inf.vcmr_search_host(w["m"], w["index"], query_feat=w["qf_cpu"].pin_memory(), query_mask=w["qm_cpu"].pin_memory(),
                                 max_pred_l=16)
        with pytest.raises(ValueError, match="parts"):
            from tvretrieval_amd import dist
            dist.check_shards(w["index"])
        with pytest.raises(ValueError, match="parts index"):                    # no captured pass on a parts index (not built)
            inf.GraphedVcmrSearch(w["m"], w["index"], w["nq"], w["qf"].shape[1], w["qf"].shape[2], **w["kw"])
        with pytest.raises(ValueError, match="parts"):                          # the batches must hold exactly the table's rows
            inf.build_corpus_index(w["m"], [(w["pvf"][:50].to(DEV), w["pvm"][:50].to(DEV), w["psf"][:50].to(DEV),
                                             w["psm"][:50].to(DEV))], parts=w["table"])
