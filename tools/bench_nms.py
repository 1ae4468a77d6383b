#!/usr/bin/env python
"""Temporal NMS on the device (xml_nms_moments) against the host implementation (xml_nms_vcmr_batched_host) on TVR-val-shaped
record sets: the 10 895 x 200 pre-NMS VCMR records of a synthetic search at the as-trained shape (bench.WORKLOADS["tvr_val"],
the search tools/bench_e2e.py runs) -- real group structure: 100 videos per query, moments clustered around each video's
span peaks -- with max_before 100 and 200.
  device: kernel time, median over HIP events around single launches after warm-up;
  host:   wall time of postproc.nms_batched (one xml_nms_vcmr_batched_host call) at --threads host threads, same process;
  and the host-to-host pass both ways: vcmr_search_host(nms_thd=0.5) against the plain pass + host NMS of its records.
The device result is checked against the host's (index lists and counts equal).  Prints one JSON line.  GPU box only."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tvr_val")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the batched host NMS")
    ap.add_argument("--thd", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import bench
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ops, postproc
    from tvretrieval_amd.model_xml import XML
    from tvretrieval_amd.results import MomentResults
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
    host_q = dict(query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory())
    n_before, n_after = 200, 100

    def wall(fn, n=5):
        fn()                                   # warm-up: buffers, workspaces
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), r

    with torch.no_grad():
        t_plain, (rec, cnt) = wall(lambda: inf.vcmr_search_host(model, index, max_before_nms=n_before, **host_q))
        rec, cnt = rec.copy(), cnt.copy()
        res = MomentResults.from_records(list(range(nq)), [""] * nq, rec, cnt)
        t_h2h_nms, (nrec, ncnt) = wall(lambda: inf.vcmr_search_host(model, index, max_before_nms=n_before, nms_thd=a.thd,
                                                                    max_after_nms=n_after, **host_q))
        nrec, ncnt = nrec.copy(), ncnt.copy()

        def plain_then_host():
            r, c = inf.vcmr_search_host(model, index, max_before_nms=n_before, **host_q)
            rr = MomentResults.from_records(list(range(nq)), [""] * nq, r, c)
            return postproc.nms_batched(rr, "VCMR", a.thd, n_before, n_after, n_threads=a.threads)
        t_plain_host_nms, (hidx, hcnt) = wall(plain_then_host)
        kept = res.take(hidx, hcnt)
        h2h_equal = bool(np.array_equal(ncnt, hcnt) and all(
            np.array_equal(np.where(np.arange(n_after)[None] < hcnt[:, None], nrec[c], 0).astype(np.float64), getattr(kept, c))
            for c in ("vid", "st", "ed", "score")))
        rec_dev = torch.from_numpy(rec.view(np.int32).reshape(nq, n_before, 4)).to(dev)
        cnt_dev = torch.from_numpy(cnt).to(dev)
        cases = []
        for mb in (100, 200):
            for _ in range(3):
                _, idx, dcnt = ops.nms_moments(rec_dev, cnt_dev, True, a.thd, max_before=mb, max_after=n_after)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.nms_moments(rec_dev, cnt_dev, True, a.thd, max_before=mb, max_after=n_after)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            hs = []
            for _ in range(5):
                t0 = time.perf_counter()
                hidx, hcnt = postproc.nms_batched(res, "VCMR", a.thd, mb, n_after, n_threads=a.threads)
                hs.append(time.perf_counter() - t0)
            didx, dcnt = idx.cpu().numpy(), dcnt.cpu().numpy()
            keep = np.arange(n_after)[None] < hcnt[:, None]
            cases.append(dict(max_before=mb, max_after=n_after, device_kernel_ms_median=round(statistics.median(ms), 4),
                              device_kernel_ms_min=round(min(ms), 4), host_wall_ms_median=round(statistics.median(hs) * 1e3, 3),
                              host_wall_ms_min=round(min(hs) * 1e3, 3), kept_per_query=round(float(hcnt.mean()), 2),
                              equal=bool(np.array_equal(dcnt, hcnt) and np.array_equal(np.where(keep, didx, 0),
                                                                                       np.where(keep, hidx, 0)))))
    print(json.dumps({"workload": a.workload, "queries": nq, "videos": nv, "records_per_query": n_before, "nms_thd": a.thd,
                      "valid_records_per_query": round(float(cnt.mean()), 2),
                      "videos_per_query": round(float(np.mean([len(np.unique(r[:c])) for r, c in zip(rec["vid"][:512], cnt[:512])])), 2),
                      "host_threads": a.threads, "reps": a.reps, "cases": cases,
                      "h2h_plain_ms": round(t_plain * 1e3, 2), "h2h_nms_on_device_ms": round(t_h2h_nms * 1e3, 2),
                      "h2h_plain_plus_host_nms_ms": round(t_plain_host_nms * 1e3, 2), "h2h_equal": h2h_equal,
                      "d2h_records_per_query": {"plain": n_before, "nms_on_device": n_after}}))


if __name__ == "__main__":
    main()
