#!/usr/bin/env python
"""Retrieval metrics on the device (xml_eval_moments) in eval_epoch at the TVR-val shape (bench.WORKLOADS["tvr_val"]: 10 895
queries x 2 179 videos, real clip counts; the set-up of tools/bench_e2e.py: opt.graph_search, tasks VCMR + SVMR + VR, NMS 0.5):
  wall time of eval_epoch (after the corpus encode, as_arrays=True) for four settings of one process, alternated round by round
  after one warm-up round, median (min) of --rounds:
    host            host NMS, host evaluator (every default)
    nms_on_device   K11 + host evaluator -- what the commit before this option did at its fastest
    eval_on_device  K11 + xml_eval_moments, lists still fetched
    metrics_only    K11 + xml_eval_moments, no record buffer leaves the device
  and the entry's own time per task: HIP events around single ops.eval_moments calls on the sinks' records, median (min) of
  --reps after 3 warm-up calls.
The four settings' metrics are checked to be equal.  Prints one JSON line.  GPU box only; reads nothing outside the repository."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tvr_val")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--bsz", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import bench
    from bench_e2e import SyntheticQueries
    from tvretrieval_amd import evaluate, ops
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd.model_xml import XML
    nq, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS[a.workload]
    nq = a.queries or nq
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = XML(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), compute_dtype=torch.bfloat16).to(dev).eval()
    lens = bench.real_clip_counts(nv, l) if a.workload in bench.RAGGED else None
    with torch.no_grad():
        index = inf.build_corpus_index(model, bench.context_batches(0, nv, l, dv, ds, True, ctx_mode == "video_sub", dev, lens),
                                       n_total=nv, l_ref=l)
    qf, qm = bench.synth_queries(nq, dq, dev)
    rng = np.random.default_rng(2018)
    gt_video = rng.integers(0, nv, nq)
    ds_q = SyntheticQueries(qf, qm, gt_video, nv)
    ctx = dict(index=index, video_metas=[dict(vid_name="v%05d" % i) for i in range(nv)])
    clip = 1.5
    st = rng.integers(0, 40, nq)
    gt = [dict(desc_id=90000 + i, desc="", type=["v", "t", "vt"][i % 3], vid_name="v%05d" % gt_video[i],
               ts=[float(st[i] * clip), float((st[i] + rng.integers(2, 11)) * clip)]) for i in range(nq)]
    tasks = ("VCMR", "SVMR", "VR")
    base = argparse.Namespace(eval_query_bsz=a.bsz, device=dev, q2c_alpha=20.0, min_pred_l=2, max_pred_l=16, clip_length=clip,
                              debug=False, external_inference_vr_res_path=None, max_ctx_l=l, max_before_nms=200,
                              max_vcmr_video=100, nms_thd=0.5, dset_name="tvr", graph_search=True, max_desc_l=int(qm.shape[1]))
    settings = [("host", {}), ("nms_on_device", dict(nms_on_device=True)),
                ("eval_on_device", dict(nms_on_device=True, eval_on_device=True)),
                ("metrics_only", dict(nms_on_device=True, eval_on_device=True, metrics_only=True))]
    walls = {k: [] for k, _ in settings}
    stages = {k: [] for k, _ in settings}
    metrics = {}
    for rnd in range(a.rounds + 1):                 # round 0 = warm-up (workspaces, weight packing, graph capture, allocator)
        for name, extra in settings:
            opt = copy.copy(base)
            for k, v in extra.items():
                setattr(opt, k, v)
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                _, met, _, met_nms = inf.eval_epoch(model, ds_q, opt, tasks=tasks, ground_truth=gt, as_arrays=True, timings=tm,
                                                    ctx_info=ctx)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                walls[name].append(dt)
                stages[name].append(tm)
            metrics[name] = json.dumps([met, met_nms])
    equal = len(set(metrics.values())) == 1
    # the entry alone, on the sinks of one more pass
    opt = copy.copy(base)
    opt.nms_on_device = True
    with torch.no_grad():
        sinks = inf.compute_query2ctx_info(model, ds_q, opt, ctx, max_before_nms=200, max_n_videos=100, tasks=tasks,
                                           as_arrays=True, _sinks="only")["_sinks"]
    dgt = evaluate.DeviceGroundTruth(gt, ds_q.video2idx, sinks["desc_ids"], dev)
    calls = [(t, "raw") + s.eval_raw(100) + (sc,) for t, (s, sc) in sinks["raw"].items()]
    calls += [(t, "kept") + s.eval_kept() for t, s in sinks["kept"].items()]
    entry = {}
    for t, what, rec, cnt, scale in calls:
        out = None
        for _ in range(3):
            out = ops.eval_moments(rec, cnt, t, dgt, scale=scale)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.eval_moments(rec, cnt, t, dgt, scale=scale, first_hit=out[0], hits=out[1], rows=out[2])
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        entry["%s_%s" % (t, what)] = dict(records_per_row=int(rec.shape[1]), ms_median=round(statistics.median(ms), 4),
                                          ms_min=round(min(ms), 4))

    def med(name, key):
        return round(statistics.median(s.get(key, 0.0) for s in stages[name]), 4)
    print(json.dumps({
        "workload": a.workload, "queries": nq, "videos": nv, "eval_query_bsz": a.bsz, "nms_thd": 0.5, "max_before_nms": 200,
        "graph_search": True, "rounds": a.rounds, "reps": a.reps, "metrics_equal": equal,
        "eval_epoch_wall_s": {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4),
                                      all=[round(x, 4) for x in v]) for k, v in walls.items()},
        "stage_s_median": {k: {s: med(k, s) for s in ("search", "top_n", "eval", "nms", "eval_nms")} for k in walls},
        "metrics_only_over_nms_on_device": round(statistics.median(walls["metrics_only"])
                                                 / statistics.median(walls["nms_on_device"]), 4),
        "entry_ms": entry, "host_threads": os.cpu_count()}))


if __name__ == "__main__":
    main()
