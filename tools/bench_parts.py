"""Timing of the parts path (videos longer than max_ctx_l indexed in parts): the fold kernel
xml_group_best_allow next to its byte floor, and the whole search on the same index rows with and without the part table --
their difference is what the fold costs a search.  GPU box only.

usage: python tools/bench_parts.py [--videos 21793] [--w 100] [--overlap 16] [--reps 21] [--pass-reps 7] [--queries 10000]
                                   [--no-pass] [--out profiles/parts_timing.md]

The corpus is the TVR clip-count histogram (tests/golden/tvr_clip_count_hist.json; counts above 128 are recorded as 128) cut
into parts by ingest.plan_parts(W, overlap).  Every figure is the median of --reps launches between HIP events after two
warm-up launches; min .. max is the spread.  The byte floor of the fold is rows * n_parts * 4 bytes of scores read once, at
6.3 TB/s (the achievable HBM stream rate of an MI355X; 8.0 TB/s is the specification)."""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tvretrieval_amd import inference as inf, ops  # noqa: E402
from tvretrieval_amd.ingest import plan_parts  # noqa: E402

HBM_STREAM = 6.3e12       # bytes / s


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in evs:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(t):
    return "%.3f ms (min %.3f .. max %.3f)" % t


def fold_leg(table, args, lines):
    d = table.to("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    shared = inf.pack_video_allow(torch.rand((1, table.n_videos), device="cuda", generator=g) < 0.5)
    sizes = np.diff(table.group_start)
    multi = int(sizes[sizes > 1].sum())           # index rows whose score can decide something: parts of multi-part videos
    words = (table.n_parts + 31) // 32
    lines += ["## The fold kernel alone", "",
              "The byte floor is the whole score matrix read once (rows x index rows x 4 B) at 6.3 TB/s.  The kernel does not read",
              "the score of a video's only part (it is the best part whatever it scores): what it has to move is the %d columns of"
              % multi, "multi-part videos and %d output words per row, the last column." % words, "",
              "| rows x index rows | scores | no mask | shared mask over source videos | byte floor, whole matrix | bytes it must move |",
              "|---|---|---|---|---|---|"]
    res = {}
    for rows in (args.queries, 50):
        x = torch.empty(rows, table.n_parts, device="cuda")
        for b in range(0, rows, 1000):
            x[b:b + 1000] = torch.rand(min(1000, rows - b), table.n_parts, device="cuda", generator=g)
        t0 = timed(lambda: ops.group_best_allow(x, d), args.reps)
        t1 = timed(lambda: ops.group_best_allow(x, d, shared), args.reps)
        floor = rows * table.n_parts * 4 / HBM_STREAM * 1e3
        must = rows * (multi + words) * 4
        res[rows] = t0
        lines.append("| %d x %d | %.1f MB | %s | %s | %.4f ms | %.1f MB = %.4f ms |"
                     % (rows, table.n_parts, rows * table.n_parts * 4 / 1e6, fmt(t0), fmt(t1), floor, must / 1e6,
                        must / HBM_STREAM * 1e3))
        print(lines[-1], flush=True)
    return res


def pass_leg(table, args, lines, fold):
    import bench
    nq, _, _, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
    nq = args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, args.w), torch.bfloat16)
    lens = torch.from_numpy(table.part_len.astype(np.int64))
    with torch.no_grad():
        index = inf.build_corpus_index(model, bench.context_batches(0, table.n_parts, args.w, dv, ds, model.use_video,
                                                                    model.use_sub, be.device, lens=lens),
                                       l_ref=args.w, n_videos=table.n_parts, parts=table)
        plain = copy.copy(index)
        plain.parts, plain.n_source_videos = None, plain.n_videos
        qf, qm = bench.synth_queries(nq, dq, be.device)
        n_tok = int(qm.sum().item())
        kw = dict(n_valid_tokens=n_tok, max_pred_l=args.overlap)
        a = timed(lambda: inf.vcmr_search(model, plain, qf, qm, **kw), args.pass_reps)
        b = timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps)
        a2 = timed(lambda: inf.vcmr_search(model, plain, qf, qm, **kw), args.pass_reps)
        b2 = timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps)
    spread = max(a[2], a2[2]) - min(a[1], a2[1])
    diff = (b[0] + b2[0] - a[0] - a2[0]) / 2
    lines += ["", "## The whole search (vcmr_search, bf16, hidden %d, %d queries x %d index rows of <= %d clips), %d passes each, "
              "alternating" % (hidden, nq, table.n_parts, args.w, args.pass_reps), "",
              "| index | pass |", "|---|---|",
              "| the rows without the part table | %s |" % fmt(a), "| with the part table | %s |" % fmt(b),
              "| without, again | %s |" % fmt(a2), "| with, again | %s |" % fmt(b2), "",
              "Difference of the medians (with - without, mean of the two rounds): %.3f ms; the fold kernel alone at this shape: "
              "%.3f ms; run-to-run spread of the search without parts in this process (max - min over both rounds): %.3f ms."
              % (diff, fold[nq][0], spread)]
    note = ("The difference exceeds the kernel's own time by more than that spread: besides the fold, a search with parts runs K8 "
            "through xml_topk_rows_allowed (a per-row mask of %.1f MB) instead of xml_topk_rows, and K7 / K9 see other videos."
            % (nq * ((table.n_parts + 31) // 32) * 4 / 1e6)) if diff - fold[nq][0] > spread else \
        "The difference lies within that spread of the kernel's own time."
    lines += ["", note]
    for ln in lines[-12:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=21793)
    ap.add_argument("--w", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--pass-reps", type=int, default=7)
    ap.add_argument("--no-pass", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_timing.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_parts.py measures on the GPU; none is visible")
    import bench
    n_clips = bench.real_clip_counts(args.videos, 128).numpy()
    table = plan_parts(n_clips, args.w, args.overlap)
    sizes = np.diff(table.group_start)
    lines = ["# Videos in parts: what the fold costs", "",
             "`python tools/bench_parts.py` on one MI355X.  %d videos with the TVR clip counts (histogram clipped at 128), "
             "max_ctx_l = %d, overlap = %d: %d index rows; %d videos have 2 parts, %d have more."
             % (table.n_videos, args.w, args.overlap, table.n_parts, int((sizes == 2).sum()), int((sizes > 2).sum())),
             "Medians of %d launches between HIP events after two warm-up launches (min .. max)." % args.reps, ""]
    fold = fold_leg(table, args, lines)
    if not args.no_pass:
        pass_leg(table, args, lines, fold)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
