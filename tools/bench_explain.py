"""inference.explain_moments at the headline shape (bench.py workload c3: 10 000 queries x 21 793 videos x 128 clips, H = 768,
bf16) for two pair lists: the top-1 video of every query (P = 10 000) and the top-100 videos of 50 queries (P = 5 000).

Per list: the whole call without / with the video-level score (which costs a K6 pass over the corpus on a plain index), the
span-evidence kernel alone, and ops.convse_rerank(softmax=False) on the same pairs -- the same products, two output rows per
pair instead of five.  `--k7-only` stops after the K7 figure and touches nothing newer than ops.convse_rerank: run from a
checkout of the parent commit it gives the baseline the evidence kernel is put next to (profiles/explain_timing.md).
EXPLAIN_WORKLOAD=tiny for a quick run."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tvretrieval_amd import inference as inf, ops  # noqa: E402
from tvretrieval_amd.model_xml import XML  # noqa: E402


def median_ms(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in evs:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return sorted(s.elapsed_time(e) for s, e in evs)[reps // 2]


def main():
    k7_only = "--k7-only" in sys.argv
    wl = os.environ.get("EXPLAIN_WORKLOAD", "c3")
    nq, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS[wl]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = XML(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), compute_dtype=torch.bfloat16).to(dev).eval()
    res = dict(workload=wl, device=torch.cuda.get_device_name(0), k7_only=k7_only)
    with torch.no_grad():
        index = inf.build_corpus_index(m, bench.context_batches(0, nv, l, dv, ds, True, True, dev, None), n_total=nv, l_ref=l)
        qf, qm = bench.synth_queries(nq, dq, dev)
        qvec = inf.stage_query_vectors(m, qf, qm)
        tw, ti = ops.topk_rows(inf.stage_q2c(index, qvec), min(100, nv), alpha=20.0)
        q_lin = inf.query_linears(m, index, qvec)
        mods = index.modalities
        f2, mk = [index.feat2[k] for k in mods], [index.mask[k] for k in mods]
        conv_w = m._conv_weights()
        n50 = min(50, nq)
        cases = {"top1_of_%d_queries" % nq: (qf, qm, q_lin, ti[:, :1].contiguous()),
                 "top%d_of_%d_queries" % (ti.shape[1], n50): (qf[:n50], qm[:n50], [q[:n50].contiguous() for q in q_lin],
                                                             ti[:n50].contiguous())}
        for name, (cqf, cqm, cql, pair_vid) in cases.items():
            n, k = pair_vid.shape
            r = dict(pairs=n * k)
            r["convse_rerank_logits_ms"] = median_ms(lambda: ops.convse_rerank(cql, f2, mk, pair_vid, conv_w, l, True, 5,
                                                                               softmax=False))
            if not k7_only:
                pq = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(k).contiguous()
                pv = pair_vid.reshape(-1).contiguous()
                r["span_evidence_ms"] = median_ms(lambda: ops.span_evidence(cql, f2, mk, pq, pv, conv_w, l, True, 5))
                r["explain_moments_ms"] = median_ms(lambda: inf.explain_moments(m, index, cqf, cqm, pq, pv, with_q2c=False))
                r["explain_moments_with_q2c_ms"] = median_ms(lambda: inf.explain_moments(m, index, cqf, cqm, pq, pv))
                ev = ops.span_evidence(cql, f2, mk, pq, pv, conv_w, l, True, 5)
                st, ed = ops.convse_rerank(cql, f2, mk, pair_vid, conv_w, l, True, 5, softmax=False)
                r["logits_bitwise_equal"] = bool(torch.equal(ev.st_logits, st.reshape(n * k, -1)) and
                                                 torch.equal(ev.ed_logits, ed.reshape(n * k, -1)))
            res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
