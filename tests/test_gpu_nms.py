"""xml_nms_moments (temporal NMS on the device) against the host implementation (xml_nms_{vcmr,svmr}_batched_host), the oracle's
restatement of the reference (oracle.xml_oracle.vcmr_nms / temporal_nms) and the golden NMS arrays.  NMS only selects and
orders existing records, and both sides decide with the same float64 operations on the same values: every comparison here
is exact equality."""
import itertools
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, L, CLIP = 37, 24, 1.5
THDS = (0.0, 0.3, 0.5, 0.7, 1.0)
ROW_IOU, ROW_ORDER = 3, 5          # rows with planted entries (see make_rows)


def _dtype():
    from tvretrieval_amd.results import MOMENT_DTYPE
    return MOMENT_DTYPE


def make_rows(n, n_vid, sort_rows, clip_units, seed):
    """(NQ, n) records as K10 emits them + ragged counts.  Spans on the clip grid (start clip i, end clip j, 2..16 clips of L
    = 24): seconds f32(i) * f32(1.5), f32(j) * f32(1.5) + f32(1.5) -- or clip units (i, j + 1) for scale = clip_length --
    video ids of n_vid videos, scores in sixteenths (ties are common), a zero-score tail like pad_tail's in every third row,
    {-1, 0, 0, 0} behind the count.  Planted (n >= 7): row ROW_IOU starts with [0, 3] s / [0, 6] s of one video (IoU exactly
    0.5) on top scores; row ROW_ORDER with (video A, 5.0), (video B, 4.5), (video A, 4.5), A's spans disjoint."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(2, 17, (NQ, n))
    i = (rng.random((NQ, n)) * (L - ln + 1)).astype(np.int64)
    j = i + ln - 1
    vid = 1000 + 7 * rng.integers(0, n_vid, (NQ, n))
    score = rng.integers(1, 64, (NQ, n)).astype(np.float32) / np.float32(16)
    count = rng.integers(0, n + 1, NQ)
    count[:3] = (0, 1, n)
    count[[ROW_IOU, ROW_ORDER]] = n
    for q in range(0, NQ, 3):
        score[q, int(count[q]) // 2:] = 0.0
    if sort_rows:
        order = np.argsort(-score, axis=1, kind="stable")
        i, j, vid, score = (np.take_along_axis(a, order, 1) for a in (i, j, vid, score))
    if n >= 7:
        q = ROW_IOU
        i[q, :2], j[q, :2], vid[q, :2], score[q, :2] = (0, 0), (1, 3), 1000, (5.0, 4.75)
        q = ROW_ORDER
        i[q, :3], j[q, :3], vid[q, :3], score[q, :3] = (0, 4, 10), (1, 6, 11), (1000, 1007, 1000), (5.0, 4.5, 4.5)
    rec = np.zeros((NQ, n), _dtype())
    rec["vid"], rec["score"] = vid, score
    if clip_units:
        rec["st"], rec["ed"] = i.astype(np.float32), (j + 1).astype(np.float32)
    else:
        c = np.float32(CLIP)
        rec["st"], rec["ed"] = i.astype(np.float32) * c, j.astype(np.float32) * c + c
    dead = np.arange(n)[None, :] >= count[:, None]
    rec["vid"][dead] = -1
    for f in ("st", "ed", "score"):
        rec[f][dead] = 0
    return rec, count.astype(np.int32)


def widen(rec, scale):
    """The columns the host entries take: what MomentResults.from_records(scale=) makes of the records."""
    st, ed = rec["st"].astype(np.float64), rec["ed"].astype(np.float64)
    if scale != 1.0:
        st, ed = st * float(scale), ed * float(scale)
    c = np.ascontiguousarray
    return c(rec["vid"].astype(np.int64)), c(st), c(ed), c(rec["score"].astype(np.float64))


def host_nms(cols, count, by_video, thd, max_before, max_after):
    from tvretrieval_amd import _lib
    vid, st, ed, sc = cols
    nq, n = vid.shape
    idx = np.full((nq, max(max_after, 1)), -1, np.int32)
    cnt = np.zeros(nq, np.int32)
    count = np.ascontiguousarray(count, dtype=np.int32)
    lib = _lib.load()
    if by_video:
        _lib.check(lib.xml_nms_vcmr_batched_host(vid.ctypes.data, st.ctypes.data, ed.ctypes.data, sc.ctypes.data,
                                                 count.ctypes.data, nq, n, float(thd), max_before, max_after, idx.ctypes.data,
                                                 idx.shape[1], cnt.ctypes.data, 1), "host vcmr nms")
    else:
        _lib.check(lib.xml_nms_svmr_batched_host(st.ctypes.data, ed.ctypes.data, sc.ctypes.data, count.ctypes.data, nq, n,
                                                 float(thd), max_before, max_after, idx.ctypes.data, idx.shape[1],
                                                 cnt.ctypes.data, 1), "host svmr nms")
    idx[np.arange(idx.shape[1])[None, :] >= cnt[:, None]] = -1
    return idx, cnt


def device_nms(rec_dev, cnt_dev, by_video, thd, scale, max_before, max_after):
    from tvretrieval_amd import ops
    out, idx, cnt = ops.nms_moments(rec_dev, cnt_dev, by_video, thd, scale=scale, max_before=max_before, max_after=max_after)
    return out.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def gathered(rec, idx, cnt):
    """The input records at idx, bitwise, {-1, 0, 0, 0} behind the count -- as (Nq, m, 4) int32 words."""
    words = np.ascontiguousarray(rec).view(np.int32).reshape(rec.shape[0], rec.shape[1], 4)
    got = np.take_along_axis(words, np.maximum(idx, 0).astype(np.int64)[:, :, None], axis=1)
    behind = np.arange(idx.shape[1])[None, :] >= cnt[:, None]
    got[behind] = (-1, 0, 0, 0)
    return got


def oracle_rows(cols, count, q, by_video, thd, max_before, max_after):
    from oracle import xml_oracle as O
    vid, st, ed, sc = cols
    c = int(count[q])
    rows = [[int(vid[q, k]), float(st[q, k]), float(ed[q, k]), float(sc[q, k])] for k in range(c)]
    if by_video:
        return O.vcmr_nms(rows, thd, max_before_nms=max_before, max_after_nms=max_after)
    kept = O.temporal_nms([r[1:] for r in rows[:max_before]], thd) if min(c, max_before) > 0 else []
    return [[None] + list(p) for p in kept[:max_after]]         # (one video: the ids play no part)


def iou64(s0, e0, s1, e1):
    inter = max(0.0, min(e0, e1) - max(s0, s1))
    uni = max(e0, e1) - min(s0, s1)
    return 0.0 if uni == 0 else inter / uni


def walk_ious(st, ed, sc, members, thd):
    """The IoUs the greedy walk of one group takes (float64), in order: [(head, other, iou)]."""
    order = sorted(members, key=lambda k: -sc[k])          # stable: ties by position
    dead, seen = set(), []
    for a, h in enumerate(order):
        if h in dead:
            continue
        for k in order[a + 1:]:
            if k not in dead:
                v = iou64(st[h], ed[h], st[k], ed[k])
                seen.append((h, k, v))
                if v > thd:
                    dead.add(k)
    return seen


@pytest.mark.parametrize("n", [1, 7, 64, 65, 200, 257, 1024])
def test_generated_rows_equal_host_and_oracle(n):
    thd_iou_seen = order_seen = False
    n_oracle = 0
    # the oracle is Python lists: a subsample of the rows of every input (fewer of the long ones), 64 or more per n
    oracle_q = [1, 2, ROW_IOU, ROW_ORDER] + ([] if n >= 1024 else [0, NQ - 3, NQ - 2, NQ - 1])
    for n_vid, sort_rows, scale in itertools.product((3, 50), (True, False), (1.0, CLIP)):
        rec, count = make_rows(n, n_vid, sort_rows, scale != 1.0, seed=1000 * n + 10 * n_vid + 2 * sort_rows + (scale != 1.0))
        cols = widen(rec, scale)
        rec_dev = torch.from_numpy(rec.view(np.int32).reshape(NQ, n, 4)).to(DEV)
        cnt_dev = torch.from_numpy(count).to(DEV)
        if n >= 7:          # generator conditions, in float64 numpy: a weak input must not hide a fault
            vid, st, ed, sc = (c[ROW_IOU] for c in cols)
            seen = walk_ious(st, ed, sc, [k for k in range(n) if vid[k] == vid[0]], 0.5)
            assert (0, 1, 0.5) in seen, "no compared same-group pair with IoU exactly 0.5"
            thd_iou_seen = True
        for by_video, thd, mb, ma in itertools.product((1, 0), THDS, (n, n // 2, 1), (100, 5, n)):
            want_idx, want_cnt = host_nms(cols, count, by_video, thd, mb, ma)
            out, idx, cnt = device_nms(rec_dev, cnt_dev, by_video, thd, scale, mb, ma)
            what = "n=%d vids=%d sorted=%d scale=%g by_video=%d thd=%g max_before=%d max_after=%d" % (
                n, n_vid, sort_rows, scale, by_video, thd, mb, ma)
            np.testing.assert_array_equal(cnt, want_cnt, err_msg=what)
            np.testing.assert_array_equal(idx[:, :ma], want_idx[:, :ma], err_msg=what)
            np.testing.assert_array_equal(out[:, :ma], gathered(rec, want_idx, want_cnt)[:, :ma], err_msg=what)
            if n >= 7 and by_video and mb == n and ma >= 3:
                row, k = idx[ROW_ORDER], int(cnt[ROW_ORDER])
                sc = cols[3][ROW_ORDER]
                if thd == 0.5:
                    assert 1 in idx[ROW_IOU, :int(cnt[ROW_IOU])], "the pair with IoU == thd must survive (strictly greater)"
                if any(sc[row[r]] == sc[row[r + 1]] and row[r] > row[r + 1] and cols[0][ROW_ORDER][row[r]] !=
                       cols[0][ROW_ORDER][row[r + 1]] for r in range(k - 1)):
                    order_seen = True
                assert list(row[:3]) == [0, 2, 1], what
            if mb == n and ma == 100 and thd == 0.5:
                for q in oracle_q:
                    want = oracle_rows(cols, count, q, by_video, thd, mb, ma)
                    k = int(cnt[q])
                    got = [[int(cols[0][q, p]) if by_video else None, float(cols[1][q, p]), float(cols[2][q, p]),
                            float(cols[3][q, p])] for p in idx[q, :k]]
                    assert got == [list(w) for w in want], what + " row %d vs oracle" % q
                    n_oracle += 1
    if n >= 7:
        assert thd_iou_seen and order_seen
    assert n_oracle >= 64


def test_per_group_cap_is_hit():
    """n = 1024, one video, thd = 1.0 (nothing is suppressed), arbitrary f32 spans: more than 100 survivors, 100 are kept."""
    n = 1024
    rng = np.random.default_rng(7)
    rec = np.zeros((NQ, n), _dtype())
    st = (rng.random((NQ, n)) * 100).astype(np.float32)
    rec["vid"], rec["st"], rec["ed"] = 1234, st, st + (rng.random((NQ, n)) * 20 + 0.01).astype(np.float32)
    rec["score"] = rng.random((NQ, n)).astype(np.float32)
    count = np.full(NQ, n, np.int32)
    count[1] = 101
    count[2] = 100
    cols = widen(rec, 1.0)
    rec_dev = torch.from_numpy(rec.view(np.int32).reshape(NQ, n, 4)).to(DEV)
    cnt_dev = torch.from_numpy(count).to(DEV)
    for by_video, thd in itertools.product((1, 0), (1.0, 0.5)):
        want_idx, want_cnt = host_nms(cols, count, by_video, thd, n, n)
        out, idx, cnt = device_nms(rec_dev, cnt_dev, by_video, thd, 1.0, n, n)
        if thd == 1.0:
            assert (want_cnt == 100).all() and int(count.min()) >= 100        # > 100 survivors, the cap keeps 100
        np.testing.assert_array_equal(cnt, want_cnt)
        np.testing.assert_array_equal(idx, want_idx)
        np.testing.assert_array_equal(out, gathered(rec, want_idx, want_cnt))
    # count == NULL: whole rows
    from tvretrieval_amd import ops
    _, idx2, cnt2 = ops.nms_moments(rec_dev, None, True, 0.5, max_before=n, max_after=100)
    want_idx, want_cnt = host_nms(cols, np.full(NQ, n, np.int32), 1, 0.5, n, 100)
    np.testing.assert_array_equal(cnt2.cpu().numpy(), want_cnt)
    np.testing.assert_array_equal(idx2.cpu().numpy(), want_idx)


def test_strided_rows_and_optional_outputs():
    """Rows of a wider buffer (ld_in > n), destinations inside wider buffers, and each output on its own."""
    from tvretrieval_amd import ops
    n, wide = 65, 80
    rec, count = make_rows(n, 3, False, False, seed=99)
    cols = widen(rec, 1.0)
    buf = torch.full((NQ, wide, 4), 7, dtype=torch.int32, device=DEV)
    buf[:, :n] = torch.from_numpy(rec.view(np.int32).reshape(NQ, n, 4)).to(DEV)
    cnt_dev = torch.from_numpy(count).to(DEV)
    want_idx, want_cnt = host_nms(cols, count, 1, 0.5, n, 20)
    dst = torch.full((NQ, 32, 4), 9, dtype=torch.int32, device=DEV)
    dst_i = torch.full((NQ, 32), 9, dtype=torch.int32, device=DEV)
    out, idx, cnt = ops.nms_moments(buf[:, :n], cnt_dev, True, 0.5, max_before=n, max_after=20, out=dst[:, :20],
                                    out_index=dst_i[:, :20])
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_cnt)
    np.testing.assert_array_equal(dst_i.cpu().numpy()[:, :20], want_idx)
    np.testing.assert_array_equal(dst.cpu().numpy()[:, :20], gathered(rec, want_idx, want_cnt))
    assert (dst.cpu().numpy()[:, 20:] == 9).all() and (dst_i.cpu().numpy()[:, 20:] == 9).all()      # nothing behind max_after
    o1, i1, c1 = ops.nms_moments(buf[:, :n], cnt_dev, True, 0.5, max_before=n, max_after=20, want_index=False)
    assert i1 is None
    np.testing.assert_array_equal(o1.cpu().numpy(), gathered(rec, want_idx, want_cnt))
    o2, i2, c2 = ops.nms_moments(buf[:, :n], cnt_dev, True, 0.5, max_before=n, max_after=20, want_records=False)
    assert o2 is None
    np.testing.assert_array_equal(i2.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(c1.cpu().numpy(), want_cnt)
    np.testing.assert_array_equal(c2.cpu().numpy(), want_cnt)
    o3, i3, c3 = ops.nms_moments(buf[:, :n], cnt_dev, True, 0.5, max_before=n, max_after=0)          # nothing asked for
    assert (c3.cpu().numpy() == 0).all()


@pytest.mark.parametrize("name", ["pipeline_video_sub_h128", "pipeline_video_only_h128"])
def test_golden_lists(name):
    """The reference's pre-NMS lists as records -> the device -> the reference's after-NMS lists, exactly."""
    from tvretrieval_amd import postproc
    from tvretrieval_amd.results import MomentResults
    d, cfg, sd = load_golden(name)
    opt = json.loads(str(d["opt"]))
    clip = opt["clip_length"]
    for task in ("VCMR", "SVMR"):
        raw = d["res/" + task]
        nq, n = raw.shape[:2]
        rec = np.zeros((nq, n), _dtype())
        rec["vid"] = raw[..., 0].astype(np.int32)
        rec["score"] = raw[..., 3].astype(np.float32)
        unit = 1.0 if task == "VCMR" else clip          # VCMR times are f32 seconds already; SVMR in clip units
        rec["st"], rec["ed"] = (raw[..., 1] / unit).astype(np.float32), (raw[..., 2] / unit).astype(np.float32)
        res = MomentResults.from_records(list(range(nq)), [""] * nq, rec, np.full(nq, n, np.int32),
                                         scale=None if task == "VCMR" else clip)
        for a, b in ((res.vid, raw[..., 0]), (res.st, raw[..., 1]), (res.ed, raw[..., 2]), (res.score, raw[..., 3])):
            np.testing.assert_array_equal(a, b)         # the records ARE the fixture's lists
        rec_dev = torch.from_numpy(rec.view(np.int32).reshape(nq, n, 4)).to(DEV)
        idx, cnt = postproc.nms_batched_device(rec_dev, None, task, opt["nms_thd"], opt["max_before_nms"], 100,
                                               scale=None if task == "VCMR" else clip)
        kept = res.take(idx, cnt)
        for i in range(nq):
            np.testing.assert_array_equal(np.array(kept.predictions(i)).reshape(-1, 4), d["nms/%s/%d" % (task, i)])
