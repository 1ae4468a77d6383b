"""xml_eval_moments (retrieval metrics on the device) against the reference's stored metrics (tests/golden/eval_*.json), against
the host evaluator (evaluate.eval_retrieval) and a numpy restatement of first_hit on planted record sets, under graph capture,
and end to end through eval_epoch (opt.eval_on_device / opt.metrics_only)."""
import argparse
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_kernels import DEV
from tvretrieval_amd import evaluate, ops
from tvretrieval_amd.results import MOMENT_DTYPE, MomentResults

pytestmark = pytest.mark.gpu

THDS, TOPKS = (0.5, 0.7), (1, 5, 10, 100)
TASKS = ("VCMR", "SVMR", "VR")
CLIP = 1.5


def _same(a, b):
    """== on nested metric dicts with NaN equal to NaN (a description type without a row)."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def _plain(d):
    return json.loads(json.dumps(d))


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eval_tvr_style", "eval_didemo_style", "eval_more_tiny", "eval_more_large",
                                  "eval_more_vcmr_only", "eval_more_svmr_vr_didemo"])
def test_device_metrics_equal_the_reference(name):
    case = json.load(open(os.path.join(GOLDEN, name + ".json")))
    sub = case["submission"]
    tasks = [t for t in TASKS if t in sub]
    desc_ids = [e["desc_id"] for e in sub[tasks[0]]]
    assert all([e["desc_id"] for e in sub[t]] == desc_ids for t in tasks)
    gt = evaluate.DeviceGroundTruth(case["ground_truth"], sub["video2idx"], desc_ids, DEV,
                                    use_desc_type=case["use_desc_type"], match_number=True)
    on_dev = {}
    for t in tasks:
        rec, cnt = evaluate.records_from_results(MomentResults.from_list(sub[t]))
        on_dev[t] = (torch.from_numpy(rec).to(DEV), torch.from_numpy(cnt).to(DEV))
    got = evaluate.eval_retrieval_device(on_dev, gt, iou_thds=THDS, use_desc_type=case["use_desc_type"])
    assert _same(_plain(got), case["metrics"]), (_plain(got), case["metrics"])


def test_ground_truth_ids_must_match_like_on_the_host():
    case = json.load(open(os.path.join(GOLDEN, "eval_more_tiny.json")))
    ids = [e["desc_id"] for e in case["submission"]["VCMR"]]
    with pytest.raises(AssertionError, match="desc_ids in predictions and ground_truth must match"):
        evaluate.DeviceGroundTruth(case["ground_truth"], case["submission"]["video2idx"], ids[:-1], DEV)
    g = evaluate.DeviceGroundTruth(case["ground_truth"], case["submission"]["video2idx"], ids[:-1] + [10 ** 9], DEV,
                                   match_number=False)
    assert g.n_gt.cpu().tolist() == [1] * (len(ids) - 1) + [0]


# ---- generated -------------------------------------------------------------------------------------------------------------
POSITIONS = (1, 2, 5, 6, 10, 11, 100, 101)
F32 = np.float32
_UNIT = {"below_05": np.nextafter(F32(0.5), F32(0)), "above_05": np.nextafter(F32(0.5), F32(1)),
         "below_07": np.nextafter(F32(0.7), F32(0)), "above_07": np.nextafter(F32(0.7), F32(1))}
# per row kind: (ground-truth spans, the planted correct prediction); all values exact in f32, also times 1.5
SPECS = [
    ("iou_05", [0.0, 10.0], (0.0, 5.0)),                 # IoU exactly 0.5
    ("iou_07", [0.0, 10.0], (0.0, 7.0)),                 # IoU = f32(7 / 10) against the f32 threshold 0.7
    ("below_05", [0.0, 1.0], (0.0, _UNIT["below_05"])),  # gt [0, 1]: IoU = ed exactly
    ("count_0", [0.0, 10.0], (0.0, 10.0)),
    ("no_gt", None, (0.0, 10.0)),
    ("below_07", [0.0, 1.0], (0.0, _UNIT["below_07"])),
    ("above_07", [0.0, 1.0], (0.0, _UNIT["above_07"])),
    ("didemo", [[0.0, 10.0], [0.0, 10.0], [20.0, 30.0], [40.0, 50.0]], (0.0, 10.0)),     # two spans hit; (20, 30): one
    ("zero_hull", [3.0, 3.0], (3.0, 3.0)),               # st == ed == g_st == g_ed: union 0 -> IoU 0
    ("above_05", [0.0, 1.0], (0.0, _UNIT["above_05"])),
    ("perfect", [2.0, 9.5], (2.0, 9.5)),
]


def _generate(nq, n, svmr, first=0, seed=0):
    """Planted rows: (records (nq, n + 3, 4) int32 with row stride n + 3 > n, count, ground truth, desc_ids, video2idx).
    Row q is of kind SPECS[(first + q) % 11] with its first correct entry at position POSITIONS[(first + q) % 8] (capped at n);
    the entries in front of it alternate between the WRONG video with the right span and the right video with a disjoint span,
    so the matched rank of SVMR differs from the position; behind it random entries; behind the row's count -- and behind n --
    perfect predictions that must never be read.  svmr: the records are in clip units (scale 1.5), the ground truth in seconds."""
    rng = np.random.default_rng(1000 + 31 * nq + n + seed)
    ld = n + 3
    rec = np.zeros((nq, ld), dtype=MOMENT_DTYPE)
    count = np.full(nq, n, dtype=np.int32)
    gt, desc_ids = [], []
    k = CLIP if svmr else 1.0
    for q in range(nq):
        kind, spans, good = SPECS[(first + q) % len(SPECS)]
        pos = min(POSITIONS[(first + q) % len(POSITIONS)], n)
        vid = (q * 7 + 3) % 50 + 1
        desc_ids.append(500 + q)
        r = rec[q]
        r["vid"] = np.where(rng.random(ld) < 0.5, vid, vid + 1)
        r["st"] = np.round(rng.uniform(0, 20, ld))
        r["ed"] = r["st"] + np.round(rng.uniform(0, 12, ld))
        r["score"] = -np.sort(-rng.random(ld).astype(F32))
        front = np.arange(pos - 1)
        r["vid"][front] = np.where(front % 2 == 0, vid + 1, vid)
        r["st"][front] = np.where(front % 2 == 0, good[0], 50.0)
        r["ed"][front] = np.where(front % 2 == 0, good[1], 60.0)
        if kind == "didemo" and pos >= 2:
            r["vid"][pos - 2], r["st"][pos - 2], r["ed"][pos - 2] = vid, 20.0, 30.0      # exactly one span hits: not correct
        r["vid"][pos - 1], r["st"][pos - 1], r["ed"][pos - 1] = vid, good[0], good[1]
        if kind == "count_0":
            count[q] = 0
        elif kind == "perfect":
            count[q] = max(1, n // 2)
        elif kind == "iou_07" and n > 2:
            count[q] = n - 1
        behind = np.arange(ld) >= count[q]
        perfect = SPECS[-1][2] if spans is None else (spans[0] if isinstance(spans[0], list) else spans)
        r["vid"][behind], r["st"][behind], r["ed"][behind] = vid, perfect[0], perfect[1]
        if spans is not None:
            ts = (np.asarray(spans, dtype=np.float64) * k).tolist()
            gt.append(dict(desc_id=500 + q, desc="", vid_name="v%d" % vid, ts=ts, type="v" if q % 2 == 0 else "vt"))
    video2idx = {"v%d" % i: i for i in range(60)}
    return rec, count, gt, desc_ids, video2idx


def _first_hit_numpy(rec, count, task, scale, max_pred, gt, n):
    """first_hit restated with numpy, row by row, from the contract in include/xmlhip.h."""
    gt_vid, gt_ts, n_gt = (t.cpu().numpy() for t in (gt.gt_vid, gt.gt_ts, gt.n_gt))
    out = np.zeros((rec.shape[0], 1 if task == "VR" else len(THDS)), dtype=np.int32)
    for q in range(rec.shape[0]):
        if n_gt[q] == 0:
            continue
        m = min(max(int(count[q]), 0), n, max_pred)
        r = rec[q, :m]
        match = r["vid"] == gt_vid[q]
        st = (r["st"].astype(np.float64) * scale).astype(F32)
        ed = (r["ed"].astype(np.float64) * scale).astype(F32)
        spans = gt_ts[q, :n_gt[q]] if n_gt[q] >= 4 else gt_ts[q, :1]
        inter = np.maximum(0, np.minimum(ed[:, None], spans[None, :, 1]) - np.maximum(st[:, None], spans[None, :, 0]))
        union = np.maximum(ed[:, None], spans[None, :, 1]) - np.minimum(st[:, None], spans[None, :, 0])
        iou = np.divide(inter, union, out=np.zeros_like(inter), where=union != 0) * match[:, None]
        assert iou.dtype == F32
        for t in range(out.shape[1]):
            if task == "VR":
                c = match
            else:
                hit = iou >= F32(THDS[t])
                c = hit.sum(1) >= 2 if n_gt[q] >= 4 else hit[:, 0]
            if task == "SVMR":
                c = c & match
            idx = np.nonzero(c)[0]
            if len(idx):
                out[q, t] = idx[0] + 1 if task != "SVMR" else match[:idx[0] + 1].sum()
    return out


def _hits_numpy(first_hit, gt):
    n_gt = gt.n_gt.cpu().numpy()
    dt = gt.desc_type.cpu().numpy()
    hits = np.zeros((4, first_hit.shape[1], len(TOPKS)), dtype=np.int32)
    rows = np.zeros(4, dtype=np.int32)
    for g in range(4):
        sel = (n_gt != 0) & ((dt == g - 1) if g else True)
        rows[g] = sel.sum()
        for t in range(first_hit.shape[1]):
            for ki, k in enumerate(TOPKS):
                hits[g, t, ki] = (sel & (first_hit[:, t] >= 1) & (first_hit[:, t] <= k)).sum()
    return hits, rows


def _host_metrics(recs, count, gt_list, desc_ids, video2idx, n):
    """evaluate.eval_retrieval on the same records as MomentResults (SVMR scaled in float64 like the reference's tail)."""
    sub = dict(video2idx=video2idx)
    for t in TASKS:
        sub[t] = MomentResults.from_records(desc_ids, [""] * len(desc_ids), recs[t][:, :n].copy(), count.copy(),
                                            scale=CLIP if t == "SVMR" else None)
    with np.errstate(all="ignore"):
        return evaluate.eval_retrieval(sub, gt_list, iou_thds=THDS, verbose=False, match_number=False, use_desc_type=True)


def _strictly_between(host):
    """Every threshold of every task has a recall strictly between 0 and 100: neither an all-miss nor an all-hit table."""
    for t in ("VCMR", "SVMR"):
        for thd in THDS:
            assert any(0 < host[t]["%s-r%d" % (thd, k)] < 100 for k in TOPKS), (t, thd, host[t])
    assert any(0 < host["VR"]["r%d" % k] < 100 for k in TOPKS), host["VR"]


def _run_generated(nq, n, first=0):
    recs = {}
    rec, count, gt_list, desc_ids, video2idx = _generate(nq, n, svmr=False, first=first)
    recs["VCMR"] = recs["VR"] = rec
    recs["SVMR"], count_s, gt_list_s, _, _ = _generate(nq, n, svmr=True, first=first)
    assert (count_s == count).all()
    host = {}
    for t, gl in (("VCMR", gt_list), ("SVMR", gt_list_s), ("VR", gt_list)):     # (SVMR's ground truth is its own, in seconds)
        host.update({k: v for k, v in _host_metrics(recs, count, gl, desc_ids, video2idx, n).items() if k.startswith(t)})
    dev = {}
    for t, gl in (("VCMR", gt_list), ("SVMR", gt_list_s), ("VR", gt_list)):
        gt = evaluate.DeviceGroundTruth(gl, video2idx, desc_ids, DEV, match_number=False)
        scale = CLIP if t == "SVMR" else 1.0
        r_dev = torch.from_numpy(recs[t].view(np.int32).reshape(nq, n + 3, 4)).to(DEV)[:, :n]      # row stride n + 3 > n
        assert r_dev.stride(0) == 4 * (n + 3)
        c_dev = torch.from_numpy(count).to(DEV)
        first_hit, hits, rows = ops.eval_moments(r_dev, c_dev, t, gt, scale=scale, max_pred=100, iou_thds=THDS, topks=TOPKS)
        want_fh = _first_hit_numpy(recs[t], count, t, scale, 100, gt, n)
        np.testing.assert_array_equal(first_hit.cpu().numpy(), want_fh, err_msg="first_hit " + t)
        want_hits, want_rows = _hits_numpy(want_fh, gt)
        np.testing.assert_array_equal(hits.cpu().numpy(), want_hits, err_msg="hits " + t)
        np.testing.assert_array_equal(rows.cpu().numpy(), want_rows, err_msg="rows " + t)
        got = evaluate.eval_retrieval_device({t: (r_dev, c_dev, scale)}, gt, iou_thds=THDS)
        dev.update(got)
    assert set(dev) == set(host)
    for k in host:
        assert _same(_plain(dev[k]), _plain(host[k])), (k, dev[k], host[k])
    return host


@pytest.mark.parametrize("n", [1, 5, 100, 130])
@pytest.mark.parametrize("nq", [7, 300])
def test_generated_rows_against_the_host_evaluator(nq, n):
    host = _run_generated(nq, n)
    _strictly_between(host)
    assert math.isnan(host["VCMR_by_type"]["t-0.5-r1"])           # one description type has no row


@pytest.mark.parametrize("n", [1, 5, 100, 130])
def test_generated_single_rows_against_the_host_evaluator(n):
    """nq = 1: a one-row table is all-hit or all-miss, so three different rows are evaluated -- planted hits at 0.5 only, at
    both thresholds, at neither -- and the host evaluator must give both 0 and 100 for every threshold among them."""
    seen = [_run_generated(1, n, first=f) for f in (0, 1, 2)]
    for t in ("VCMR", "SVMR"):
        for thd in THDS:         # (the random entries behind the planted one may hit as well: only 0 and 100 are asserted)
            assert {h[t]["%s-r100" % thd] for h in seen} == {0.0, 100.0}, (t, thd, [h[t] for h in seen])


def test_max_pred_cuts_the_rows():
    """max_pred below n: entries behind it do not count (eval_by_task_type's max_pred_per_query)."""
    nq, n = 40, 12
    rec, count, gt_list, desc_ids, video2idx = _generate(nq, n, svmr=False)
    gt = evaluate.DeviceGroundTruth(gt_list, video2idx, desc_ids, DEV, match_number=False)
    r_dev = torch.from_numpy(rec.view(np.int32).reshape(nq, n + 3, 4)).to(DEV)[:, :n]
    c_dev = torch.from_numpy(count).to(DEV)
    for max_pred in (0, 1, 5, 10):
        for t in TASKS:
            first_hit, hits, rows = ops.eval_moments(r_dev, c_dev, t, gt, max_pred=max_pred, iou_thds=THDS, topks=TOPKS)
            want = _first_hit_numpy(rec, count, t, 1.0, max_pred, gt, n)
            np.testing.assert_array_equal(first_hit.cpu().numpy(), want)
            np.testing.assert_array_equal(hits.cpu().numpy(), _hits_numpy(want, gt)[0])
        res = MomentResults.from_records(desc_ids, [""] * nq, rec[:, :n].copy(), count.copy())
        if max_pred:
            with np.errstate(all="ignore"):
                m, mt = evaluate.eval_by_task_type(res, video2idx, gt_list, iou_thds=THDS, recall_topks=TOPKS, task_type="VCMR",
                                                   max_pred_per_query=max_pred, match_number=False, verbose=False)
            _, hits, rows = ops.eval_moments(r_dev, c_dev, "VCMR", gt, max_pred=max_pred, iou_thds=THDS, topks=TOPKS)
            dm, dmt = evaluate.metrics_from_hits(hits.cpu().numpy(), rows.cpu().numpy(), "VCMR", THDS, TOPKS, True)
            assert _same(_plain(dm), _plain(m)) and _same(_plain(dmt), _plain(mt))
    # count == None: whole rows
    first_hit, _, _ = ops.eval_moments(r_dev, None, "VCMR", gt, iou_thds=THDS, topks=TOPKS)
    np.testing.assert_array_equal(first_hit.cpu().numpy(), _first_hit_numpy(rec, np.full(nq, n), "VCMR", 1.0, 100, gt, n))


# ---- capture ---------------------------------------------------------------------------------------------------------------
def test_captured_entry_gives_each_record_set_its_own_counters():
    nq, n = 300, 20
    sets = [_generate(nq, n, svmr=False, first=f, seed=f) for f in (0, 5)]
    gt = evaluate.DeviceGroundTruth(sets[0][2], sets[0][4], sets[0][3], DEV, match_number=False)
    rec = torch.zeros((nq, n + 3, 4), dtype=torch.int32, device=DEV)
    cnt = torch.zeros((nq,), dtype=torch.int32, device=DEV)
    first_hit = torch.empty((nq, 2), dtype=torch.int32, device=DEV)
    hits = torch.full((4, 2, 4), 12345, dtype=torch.int32, device=DEV)
    rows = torch.full((4,), 12345, dtype=torch.int32, device=DEV)
    ops.eval_moments(rec[:, :n], cnt, "VCMR", gt, iou_thds=THDS, topks=TOPKS, first_hit=first_hit, hits=hits, rows=rows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):           # one stream: the capture stream every other captured pass of the suite uses
        ops.eval_moments(rec[:, :n], cnt, "VCMR", gt, iou_thds=THDS, topks=TOPKS, first_hit=first_hit, hits=hits, rows=rows)
    seen = []
    for r_np, c_np, _, _, _ in sets + sets[:1]:
        rec.copy_(torch.from_numpy(r_np.view(np.int32).reshape(nq, n + 3, 4)))
        cnt.copy_(torch.from_numpy(c_np))
        graph.replay()
        torch.cuda.synchronize()
        want = _first_hit_numpy(r_np, c_np, "VCMR", 1.0, 100, gt, n)
        np.testing.assert_array_equal(first_hit.cpu().numpy(), want)
        want_hits, want_rows = _hits_numpy(want, gt)
        np.testing.assert_array_equal(hits.cpu().numpy(), want_hits)          # (stale counters would add up)
        np.testing.assert_array_equal(rows.cpu().numpy(), want_rows)
        seen.append(want_hits)
    assert not (seen[0] == seen[1]).all() and (seen[0] == seen[2]).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------
_E2E = {}


def _e2e_world():
    """The small world of test_gpu_nms_search (H = 128, 12 videos, 9 queries) with a ground truth made of moments the model
    does retrieve: query i's span is its own SVMR prediction of rank i % 4 (so the ranks 1..4 occur), in its search video --
    except every third query, whose span lies outside every video, so that no recall can reach 100."""
    if _E2E:
        return _E2E
    from test_gpu_nms_search import CLIP as W_CLIP, KV, L, N_MOM, NQ, NV, _Queries, _world
    from tvretrieval_amd import inference as inf
    w = _world()
    ds = _Queries(w)
    ctx = dict(index=w["index"], video_metas=[dict(vid_name="v%03d" % i) for i in range(NV)])
    opt = argparse.Namespace(eval_query_bsz=4, device=torch.device(DEV), q2c_alpha=20.0, min_pred_l=2, max_pred_l=16,
                             clip_length=W_CLIP, debug=False, external_inference_vr_res_path=None, max_ctx_l=L,
                             max_before_nms=N_MOM, max_vcmr_video=KV, nms_thd=-1, dset_name="tvr", graph_search=False,
                             max_desc_l=30)
    with torch.no_grad():
        sub, _, _, _ = inf.eval_epoch(w["m"], ds, opt, tasks=TASKS, max_after_nms=20, ground_truth=None, as_arrays=True,
                                      ctx_info=ctx)
    gt = []
    for i in range(NQ):
        r = max(0, min(i % 4, int(sub["SVMR"].count[i]) - 1))
        ts = [float(sub["SVMR"].st[i, r]), float(sub["SVMR"].ed[i, r])] if i % 3 != 2 else [500.0, 510.0]
        gt.append(dict(desc_id=700 + i, desc="", type=["v", "t", "vt"][i % 3], vid_name="v%03d" % ds.gt_video[i], ts=ts))
    _E2E.update(w=w, ds=ds, ctx=ctx, opt=opt, gt=gt, inf=inf)
    return _E2E


def _assert_same_lists(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == "video2idx":
            assert got[k] == want[k]
            continue
        np.testing.assert_array_equal(got[k].count, want[k].count)
        for col in ("vid", "st", "ed", "score"):
            np.testing.assert_array_equal(getattr(got[k], col), getattr(want[k], col), err_msg="%s: %s" % (k, col))


@pytest.mark.parametrize("nms_thd", [-1, 0.5])
@pytest.mark.parametrize("graph", [False, True])
def test_eval_epoch_on_device_is_eval_epoch(graph, nms_thd):
    e = _e2e_world()
    inf = e["inf"]

    def run(timings=None, **extra):
        o = copy.copy(e["opt"])
        o.graph_search, o.nms_thd = graph, nms_thd
        for k, v in extra.items():
            setattr(o, k, v)
        with torch.no_grad():
            return inf.eval_epoch(e["w"]["m"], e["ds"], o, tasks=TASKS, max_after_nms=20, ground_truth=e["gt"], as_arrays=True,
                                  ctx_info=e["ctx"], timings=timings)
    tm_h, tm_d, tm_m = {}, {}, {}
    sub_h, met_h, nms_h, mnms_h = run(tm_h)
    # the ground truth is retrievable: the default path's table is neither empty nor full
    assert all(0 < met_h["SVMR"]["%s-r100" % t] < 100 for t in THDS), met_h["SVMR"]
    assert (mnms_h is None) == (nms_thd == -1)
    # with NMS: K11's kept records, and -- eagerly only, a captured pass is built per run -- host NMS with its lists sent back
    variants = [dict(eval_on_device=True)] if nms_thd == -1 else [dict(eval_on_device=True, nms_on_device=True)]
    if nms_thd != -1 and not graph:
        variants.append(dict(eval_on_device=True))
    for extra in variants:
        sub_d, met_d, nms_d, mnms_d = run(tm_d, **extra)
        assert _same(_plain(met_d), _plain(met_h)), (extra, met_d, met_h)
        assert list(met_d) == list(met_h) and [list(v) for v in met_d.values()] == [list(v) for v in met_h.values()]
        _assert_same_lists(sub_d, sub_h)
        if nms_thd == -1:
            assert nms_d is None and mnms_d is None
        else:
            assert _same(_plain(mnms_d), _plain(mnms_h)), (extra, mnms_d, mnms_h)
            _assert_same_lists(nms_d, nms_h)
    sub_m, met_m, nms_m, mnms_m = run(tm_m, eval_on_device=True, metrics_only=True, nms_on_device=True)
    assert sub_m is None and nms_m is None
    assert _same(_plain(met_m), _plain(met_h))
    assert mnms_m is None if nms_thd == -1 else _same(_plain(mnms_m), _plain(mnms_h))
    assert set(tm_m) == set(tm_h) == set(tm_d)


def test_no_ground_truth_gives_no_metrics():
    e = _e2e_world()
    o = copy.copy(e["opt"])
    o.nms_thd, o.eval_on_device, o.metrics_only, o.nms_on_device = 0.5, True, True, True
    with torch.no_grad():
        assert e["inf"].eval_epoch(e["w"]["m"], e["ds"], o, tasks=TASKS, max_after_nms=20, ground_truth=None, as_arrays=True,
                                   ctx_info=e["ctx"]) == (None, None, None, None)
        o.metrics_only = False
        sub, met, nms, mnms = e["inf"].eval_epoch(e["w"]["m"], e["ds"], o, tasks=TASKS, max_after_nms=20, ground_truth=None,
                                                  as_arrays=True, ctx_info=e["ctx"])
    assert met is None and mnms is None and set(sub) == {"video2idx"} | set(TASKS) and set(nms) == {"video2idx", "SVMR", "VCMR"}


def test_missing_options_are_named():
    e = _e2e_world()
    inf = e["inf"]

    def run(**extra):
        o = copy.copy(e["opt"])
        for k, v in extra.items():
            setattr(o, k, v)
        with torch.no_grad():
            return inf.eval_epoch(e["w"]["m"], e["ds"], o, tasks=TASKS, max_after_nms=20, ground_truth=e["gt"], as_arrays=True,
                                  ctx_info=e["ctx"])
    with pytest.raises(ValueError, match="eval_on_device"):
        run(metrics_only=True)
    with pytest.raises(ValueError, match="nms_on_device"):
        run(metrics_only=True, eval_on_device=True, nms_thd=0.5)
    run(metrics_only=True, eval_on_device=True)                 # no NMS: nothing else is needed


def test_sinks_keep_their_keys_and_lists_without_the_options():
    """compute_query2ctx_info(_svmr_only) without the private keyword: the same keys and lists as eval_epoch's raw results."""
    from test_gpu_nms_search import KV, N_MOM
    e = _e2e_world()
    inf = e["inf"]
    o = copy.copy(e["opt"])
    o.eval_on_device = True                                     # an eval_epoch option: the sinks' public results ignore it
    with torch.no_grad():
        plain = inf.compute_query2ctx_info(e["w"]["m"], e["ds"], e["opt"], e["ctx"], max_before_nms=N_MOM, max_n_videos=KV,
                                           tasks=TASKS, as_arrays=True)
        same = inf.compute_query2ctx_info(e["w"]["m"], e["ds"], o, e["ctx"], max_before_nms=N_MOM, max_n_videos=KV,
                                          tasks=TASKS, as_arrays=True)
        only = inf.compute_query2ctx_info_svmr_only(e["w"]["m"], e["ds"], o, e["ctx"], max_before_nms=N_MOM, as_arrays=True)
        sub, met, _, _ = inf.eval_epoch(e["w"]["m"], e["ds"], o, tasks=("SVMR",), max_after_nms=20, ground_truth=e["gt"],
                                        as_arrays=True, ctx_info=e["ctx"])
        sub_h, met_h, _, _ = inf.eval_epoch(e["w"]["m"], e["ds"], e["opt"], tasks=("SVMR",), max_after_nms=20,
                                            ground_truth=e["gt"], as_arrays=True, ctx_info=e["ctx"])
    assert set(plain) == set(same) == set(TASKS) and set(only) == {"SVMR"}
    _assert_same_lists(same, plain)
    assert _same(_plain(met), _plain(met_h)) and set(sub) == set(sub_h) == {"video2idx", "SVMR"}      # the svmr-only route
