"""Subset views (inference.video_subset) against the restricted search (video_allow=) they replace, at the headline shape
(bf16, 21 793 videos x 128 clips x 768, 10 000 queries), full length (c3) and with the TVR clip counts (c3r), in ONE process on
one GPU -> profiles/subset_timing.md.  GPU box only.

usage: python tools/bench_subset.py [--corpora c3,c3r] [--pass-reps 7] [--replay-reps 41] [--reps 21] [--out profiles/subset_timing.md]

Per corpus and per share of the videos (1 %, 1/6, 50 %, 100 %; a seeded random set):
  * the 10 000-query pass: unrestricted, video_allow=, subset= -- HIP events around whole passes, the legs alternate;
  * the 50-query pass as one captured graph (GraphedVcmrSearch), the same three;
  * creating the view and view.reset(same set): host clock around a device synchronise, and the gather launch alone between
    HIP events with bytes moved per second (read + written, image rows of both modalities), next to
    xml_index_move_blocks_packed moving the same number of blocks (every used block of the view onto itself) and to the
    6.3 TB/s stream rate the README quotes;
  * tiles used against ceil(blocks / 16).
Every figure is the median of its repetitions after warm-up launches; min .. max is the spread the condition is read against:
at 1/6 and at 1 % the subset= pass must be faster than the video_allow= pass by more than either spread."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tvretrieval_amd import inference as inf, ops  # noqa: E402

SHARES = [("1 %", 0.01), ("1/6", 1 / 6.0), ("50 %", 0.5), ("100 %", 1.0)]
STREAM_TBS = 6.3


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in evs:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % t


def identity_records(view):
    """Records of xml_index_move_blocks_packed that move every used block of the view onto itself."""
    sb = view.src_block.cpu().numpy().reshape(view.n_tiles, 16)
    own = np.arange(view.n_tiles * 16).reshape(view.n_tiles, 16)
    rec = np.concatenate([np.arange(view.n_tiles)[:, None], np.where(sb >= 0, own, -1)], 1)
    rec = rec[(sb >= 0).any(1)]
    return torch.from_numpy(rec.astype(np.int32)).to(view.src_block.device)


def corpus_leg(name, args, lines):
    import bench
    nq, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS[name]
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    lens = bench.real_clip_counts(nv, l) if name in bench.RAGGED else None
    with torch.no_grad():
        index = inf.build_corpus_index(model, bench.context_batches(0, nv, l, dv, ds, True, True, be.device, lens=lens),
                                       l_ref=l, n_videos=nv)
        qf, qm = bench.synth_queries(nq, dq, be.device)
    kw = dict(n_valid_tokens=int(qm.sum().item()))
    t = index.feat1n[index.modalities[0]]
    layout = "length-bucketed image, %d tiles" % t.plan.n_tiles if t.plan is not None else \
        ("plain tiles, mask-free K6" if t.all_valid else "plain tiles, mask bits")
    row_bytes = sum(index.feat1n[m].hidden * index.feat1n[m].element_size() for m in index.modalities)
    rng = np.random.default_rng(2018)
    start = len(lines)
    lines += ["", "## %s: %d videos x %d clips%s, hidden %d, bf16 -- %s" % (name, nv, l, ", TVR clip counts" if lens is not None
                                                                              else ", full length", hidden, layout), ""]
    passes, replays, creates, ok = [], [], [], True
    with torch.no_grad():
        g_free = inf.GraphedVcmrSearch(model, index, 50, qf.shape[1], qf.shape[2])
        for label, share in SHARES:
            members = np.sort(rng.choice(nv, max(1, int(round(nv * share))), replace=False)) if share < 1 else np.arange(nv)
            allowed = np.zeros(nv, dtype=bool)
            allowed[members] = True
            t0 = time.perf_counter()
            view = inf.video_subset(index, allowed)
            torch.cuda.synchronize()
            first_ms = (time.perf_counter() - t0) * 1e3
            bits = view.allow
            free = timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps)
            rounds = []
            for _ in range(2):               # alternating: allow, subset, allow, subset
                rounds.append((timed(lambda: inf.vcmr_search(model, index, qf, qm, video_allow=bits, **kw), args.pass_reps),
                               timed(lambda: inf.vcmr_search(model, index, qf, qm, subset=view, **kw), args.pass_reps)))
            a = inf.vcmr_search(model, index, qf[:512], qm[:512], video_allow=bits)
            b = inf.vcmr_search(model, index, qf[:512], qm[:512], subset=view)
            same = all(torch.equal(a[k], b[k]) for k in ("top_indices", "top_scores", "flat_indices", "flat_scores"))
            for r, (al, su) in enumerate(rounds):
                passes.append((label, len(members), r, free, al, su, same))
                if label in ("1 %", "1/6") and not al[0] - su[0] > max(al[2] - al[1], su[2] - su[1]):
                    ok = False
            g_allow = inf.GraphedVcmrSearch(model, index, 50, qf.shape[1], qf.shape[2], video_allow_rows=1)
            g_view = inf.GraphedVcmrSearch(model, index, 50, qf.shape[1], qf.shape[2], subset=view)
            replays.append((label, timed(lambda: g_free(qf[:50], qm[:50]), args.replay_reps),
                            timed(lambda: g_allow(qf[:50], qm[:50], video_allow=bits), args.replay_reps),
                            timed(lambda: g_view(qf[:50], qm[:50]), args.replay_reps)))
            del g_allow, g_view
            # creation and reset
            create = wall(lambda: inf.video_subset(index, allowed), 5)
            reset = wall(lambda: view.reset(allowed), 5)
            t0 = time.perf_counter()
            view._plan(members, view.n_tiles, None)
            host_ms = (time.perf_counter() - t0) * 1e3
            src = [index.feat1n[m] for m in index.modalities]
            bsrc = [None if (view.form == "fixed" and s.all_valid) else s.mask_bits for s in src]
            gather = timed(lambda: ops.index_gather_blocks(view.src_block, [s.data for s in src], bsrc, view._n_blocks_src(),
                                                           [view.k6[m].data for m in index.modalities],
                                                           [view.bits[m] for m in index.modalities], view.hidden), args.reps)
            rec = identity_records(view)
            k6v, bv = [view.k6[m] for m in index.modalities], [view.bits[m] for m in index.modalities]
            move = timed(lambda: [ops.index_move_blocks_packed(rec[i:i + 65535], k6v, bv, view.codes)
                                  for i in range(0, rec.shape[0], 65535)], args.reps)
            moved = 2.0 * view.blocks_used * 16 * row_bytes
            creates.append((label, len(members), view.blocks_used, view.n_tiles, -(-view.blocks_used // 16), first_ms, create,
                            reset, host_ms, gather, moved / (gather[0] * 1e-3) / 1e12, move, moved / (move[0] * 1e-3) / 1e12,
                            view.hbm_bytes()))
            del view
            torch.cuda.empty_cache()
    lines += ["### The 10 000-query pass, ms: median (min .. max) of %d passes; the two rounds alternate" % args.pass_reps, "",
              "| share | videos | round | unrestricted | video_allow= | subset= | subset / video_allow | lists of the first 512 queries |",
              "|---|---|---|---|---|---|---|---|"]
    for label, n, r, free, al, su, same in passes:
        lines.append("| %s | %d | %d | %s | %s | %s | %.3f | %s |" % (label, n, r + 1, fmt(free) if r == 0 else "", fmt(al), fmt(su),
                                                                      su[0] / al[0], "bitwise equal" if same else "DIFFER"))
    lines += ["", "Timing condition (1 %% and 1/6, every round: median video_allow= minus median subset= exceeds max - min of either): %s."
              % ("met" if ok else "NOT met"), "",
              "### The 50-query pass as one captured graph, ms: median (min .. max) of %d replays" % args.replay_reps, "",
              "| share | unrestricted | video_allow= | subset= |", "|---|---|---|---|"]
    for label, f, al, su in replays:
        lines.append("| %s | %s | %s | %s |" % (label, fmt(f), fmt(al), fmt(su)))
    lines += ["", "### Creating a view and view.reset(same set)", "",
              "Host clock around a device synchronise for the calls (ms, median (min .. max) of 5; the first call of a share "
              "also reads vlen / inverts the plan once); HIP events for the launches (median of %d).  Bytes moved = image rows "
              "read + written, both modalities; the stream rate the README quotes is %.1f TB/s." % (args.reps, STREAM_TBS), "",
              "| share | videos | blocks | tiles used | ceil(blocks / 16) | first video_subset() | video_subset() | view.reset() | "
              "of which host placement | xml_index_gather_blocks | TB/s | xml_index_move_blocks_packed, same blocks | TB/s | "
              "view bytes |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for (label, n, blocks, tiles, lower, first_ms, create, reset, host_ms, gather, gtb, move, mtb, nbytes) in creates:
        lines.append("| %s | %d | %d | %d | %d | %.1f | %s | %s | %.1f | %s | %.2f | %s | %.2f | %.1f MB |"
                     % (label, n, blocks, tiles, lower, first_ms, fmt(create), fmt(reset), host_ms, fmt(gather), gtb,
                        fmt(move), mtb, nbytes / 1e6))
    for ln in lines[start:]:
        print(ln, flush=True)
    del index, model
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpora", default="c3,c3r")
    ap.add_argument("--pass-reps", type=int, default=7)
    ap.add_argument("--replay-reps", type=int, default=41)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_timing.md"))
    args = ap.parse_args()
    lines = ["# Subset views: restricted search at the cost of the allowed videos", "",
             "`python tools/bench_subset.py`, one process on one MI355X (%s).  `subset=` is `inference.video_subset(index, "
             "allowed)` handed to the search; `video_allow=` is the same set as allow bits, K6 over the whole corpus."
             % torch.cuda.get_device_name(0)]
    ok = True
    for name in args.corpora.split(","):
        ok = corpus_leg(name, args, lines) and ok
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s; timing condition %s" % (args.out, "met" if ok else "NOT met"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
