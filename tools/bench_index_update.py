"""Timing of an index that takes updates (index_update.MutableCorpusIndex).  GPU box only.

usage: python tools/bench_index_update.py [--legs put,putp,e2e,c3,c3r,c3rp,compact,chains,exact,exactp,exactc] [--batch 200] [--reps 21]
                                          [--pass-reps 5] [--queries 10000] [--videos 21793] [--suite-wall "..."]
                                          [--parent-lib path/to/another/libxmlhip.so]
                                          [--out profiles/index_update_timing.md; --legs exact: profiles/index_exact_timing.md]

  put   xml_index_put_rows alone on a --batch-video batch at the headline shape (H = 768, lpad = 128, bf16, two modalities),
        next to the existing passes it replaces run on the same rows in the same process: the fused normalise-and-tile pass
        (what pack_q2c_corpus(normalize=True) launches; its host read-back of the masks is left out) and the feat2 / mask copies
  e2e   add() of the batch, encoder included, against build_corpus_index on the same batch
  c3    the full-length headline corpus: search on a mutable index at capacity = n_videos against the one-shot index (the
        price of mask-bit mode against the mask-free K6), the 10 000-query pass and the 50-query graph replay
  c3r   the same on the ragged corpus with the real TVR clip counts (the price of giving up the length-bucketed image)
  putp  xml_index_put_rows_packed (the packed form, MutableCorpusIndex(tiles=N)) next to xml_index_put_rows on the same batch
  c3rp  the ragged corpus on three forms in one process: one-shot packed index, mutable index, packed mutable index
  compact  (not in the default set) the packed mutable index on the ragged corpus at tiles = plan + 10 %, churned -- a random
        10 % removed and re-added with freshly drawn TVR lengths until an add is refused or 20 rounds have passed -- then
        compact(): the launches alone between HIP events, the whole call on the host clock, bytes moved, stats() and the
        10 000-query pass before and after.  Run it together with putp to have the put kernel's rate from the same run
  chains  (not in the default set) the ragged corpus with the TVR clip counts, the fixture's last bin
        (clipped at 128) spread over 128 .. 182 clips, at l_ref = --chains-l (128: 6 long videos; 100, the shape of
        profiles/parts_timing.md: 121), overlap 16: the packed mutable index with part_overlap (long videos as chains of slots) next to the one without (the
        videos cut at 128 clips), the 10 000-query pass on both; xml_chain_best_allow alone for 10 000 and 50 queries next to
        xml_group_best_allow on the part table of the same videos and the same score matrix (capacity = parts, filled in
        corpus order: slot p holds part p), and on the same chains over a random permutation of the slots
  exact   (not in the default set) exact-rank mode on a mutable index at the headline shape (ops.F16S
        model, tiles=None): xml_index_put_rows_exact on batches of 256 and 2 048 videos next to xml_index_put_rows on a plain
        f32 index and to the one-shot chain over the same rows; the 10 000-query pass and the 50-query replay next to the
        one-shot exact index of the same videos; certificate failures per pass under the running bound, after removing 10 % of
        the slots, and after tighten_error_bound(); hbm_bytes()
  exactp  (not in the default set) exact-rank mode with the packed filter image (filter_tiles=N):
        xml_index_put_rows_packed_exact on batches of 256 and 2 048 videos with the TVR clip counts next to
        xml_index_put_rows_exact on the same rows; on the ragged corpus at the headline shape (ops.F16S model) the 10 000-query
        pass and the 50-query replay on filter_tiles = what the corpus order needs and that plus 10 %, on the exact-rank index
        with the plain per-slot filter image and on the one-shot exact index with length buckets: bitwise equality of the first
        512 queries' lists, certificate failures per pass, hbm_bytes(); with --parent-lib PATH (a libxmlhip.so built from the
        commit to compare with) an A/B of xml_index_put_rows_exact between the two libraries in this process.  Its report
        (--out, default profiles/index_exact_packed_run.md) is the source of the last sections of profiles/index_exact_timing.md
  exactc  (not in the default set) long videos on the exact-rank index (exact_part_overlap=16, ops.F16S
        model, filter_tiles=N) on the corpus of the chains leg at l_ref = 128 and l_ref = 100: the 10 000-query pass and the
        50-query eager pass on the index with chains, on the same corpus truncated at l_ref on an index created without the
        keyword, and on the truncated corpus on an index created WITH it (no long video: the price of the fold alone);
        failing certificates and third-tier queries per pass, xml_cand_best_part alone on the pass's candidate lists,
        hbm_bytes().  Its report: --out, default profiles/index_exact_parts_run.md

Every figure is the median of repeated runs between HIP events after warm-up runs (min .. max); two versions are timed in the
same process, alternating.  Bytes are counted from the shapes: per modality the batch's feat1 and feat2 rows read once, the
slot's K6 rows and feat2 rows written once, plus the masks.  --suite-wall: a sentence on the GPU suite's wall time, copied into
the report (the suite is not run from here)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tvretrieval_amd import inference as inf, ops  # noqa: E402
from tvretrieval_amd.index_update import BlockTable, MutableCorpusIndex, blocks_of  # noqa: E402

HBM_STREAM = 6.3e12       # bytes / s: the achievable HBM stream rate of an MI355X (8.0 TB/s is the specification)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in evs:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in evs)
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(t, unit="ms"):
    k = 1e3 if unit == "us" else 1.0
    return "%.3g %s (min %.3g .. max %.3g)" % (t[0] * k, unit, t[1] * k, t[2] * k)


def put_leg(args, lines):
    dev, dt, h, lpad, b = "cuda", torch.bfloat16, 768, 128, args.batch
    cap = 2 * b
    g = torch.Generator(device=dev).manual_seed(0)
    enc = [(torch.randn((b, lpad, h), device=dev, generator=g).to(dt), torch.randn((b, lpad, h), device=dev, generator=g).to(dt),
            torch.ones((b, lpad), device=dev)) for _ in range(2)]
    k6 = [ops.TiledRows(torch.zeros(ops.q2c_tiled_numel(cap * lpad, h, dt), dtype=dt, device=dev), cap * lpad, h, (cap, lpad, h))
          for _ in range(2)]
    f2 = [torch.zeros((cap, lpad, h), dtype=dt, device=dev) for _ in range(2)]
    mk = [torch.zeros((cap, lpad), device=dev) for _ in range(2)]
    bits = [torch.zeros((cap, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    vlen = torch.zeros(cap, dtype=torch.int32, device=dev)
    sid = torch.zeros(cap, dtype=torch.int32, device=dev)
    live = torch.zeros((cap + 31) // 32, dtype=torch.int32, device=dev)
    scattered = torch.from_numpy(np.random.default_rng(0).permutation(cap)[:b].astype(np.int32)).to(dev)
    dense = torch.arange(b, dtype=torch.int32, device=dev)

    def put(slots):
        ops.index_put_rows([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], slots, None, k6, f2, mk, bits, vlen,
                           sid, live, lpad)

    # the one-shot build's passes for the same rows (rows [0, b) of the same tensors)
    head = [t.data[:ops.q2c_tiled_numel(b * lpad, h, dt)] for t in k6]

    def passes():
        for m in range(2):
            ops._tile(enc[m][0], b * lpad, None, True, head[m])
            f2[m][:b, :lpad] = enc[m][1]
            mk[m][:b, :lpad] = enc[m][2]

    def tile_only():
        for m in range(2):
            ops._tile(enc[m][0], b * lpad, None, True, head[m])

    nbytes = 2 * (4 * b * lpad * h * 2 + 2 * b * lpad * 4 + b * 16)
    res = [("xml_index_put_rows, scattered slots", timed(lambda: put(scattered), args.reps)),
           ("existing passes (normalise + tile, feat2 copy, mask copy; 6 launches)", timed(passes, args.reps)),
           ("xml_index_put_rows, slots 0 .. b - 1", timed(lambda: put(dense), args.reps)),
           ("existing passes, again", timed(passes, args.reps)),
           ("of which the normalise + tile pass (2 launches)", timed(tile_only, args.reps))]
    lines += ["## The put kernel alone", "",
              "%d videos x %d clips x H = %d, bf16, two modalities into an index of %d slots: %.1f MB read + written per call "
              "(counted from the shapes), %.1f us at the %.1f TB/s HBM stream rate." % (b, lpad, h, cap, nbytes / 1e6,
                                                                                     nbytes / HBM_STREAM * 1e6, HBM_STREAM / 1e12),
              "", "| what | time per call | bytes / s |", "|---|---|---|"]
    for name, t in res:
        moved = nbytes if "tile pass" not in name else 2 * 2 * b * lpad * h * 2
        lines.append("| %s | %s | %.2f TB/s |" % (name, fmt(t, "us"), moved / (t[0] * 1e-3) / 1e12))
    old = (res[1][1][0] + res[3][1][0]) / 2
    new = (res[0][1][0] + res[2][1][0]) / 2
    lines += ["", "Rate of the new kernel over the rate of the passes it replaces (same bytes, medians, mean of both rounds): %.2f."
              % (old / new)]
    for ln in lines[-10:]:
        print(ln, flush=True)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def e2e_leg(args, lines):
    import bench
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    b = args.batch
    batch = tuple(t[:b].contiguous() for t in next(iter(bench.context_batches(0, bench.CHUNK, l, dv, ds, True, True, be.device))))
    index = MutableCorpusIndex.create(model, 2 * b)
    slots = index.add(*batch)

    def readd():
        index.replace(slots, *batch)

    def build():
        with torch.no_grad():
            inf.build_corpus_index(model, [batch], l_ref=l, n_videos=b)

    def encode():
        index.encode(*batch)

    rows = [("MutableCorpusIndex: encode + put of %d videos (replace of live slots: the path of add)" % b, wall(readd, args.pass_reps)),
            ("build_corpus_index on the same batch (encode, copies, packing pass, valid lengths)", wall(build, args.pass_reps)),
            ("MutableCorpusIndex, again", wall(readd, args.pass_reps)), ("build_corpus_index, again", wall(build, args.pass_reps)),
            ("model.encode_context alone", wall(encode, args.pass_reps))]
    lines += ["", "## Adding %d videos end to end (headline model, %d clips, bf16), host clock around a device synchronise" % (b, l),
              "", "| what | wall time per call |", "|---|---|"]
    lines += ["| %s | %s |" % (n, fmt(t)) for n, t in rows]
    for ln in lines[-7:]:
        print(ln, flush=True)


def graph_ms(model, index, qf, qm, batch=50, n=60):
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(model, index, batch, qf.shape[1], qf.shape[2])
    return timed(lambda: g(qf[:batch], qm[:batch]), n)


def search_leg(name, args, lines):
    import bench
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS[name]
    nv, nq = args.videos, args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    lens = bench.real_clip_counts(nv, l) if name in bench.RAGGED else None
    batches = lambda: bench.context_batches(0, nv, l, dv, ds, True, True, be.device, lens=lens)      # noqa: E731
    with torch.no_grad():
        fixed = inf.build_corpus_index(model, batches(), l_ref=l, n_videos=nv)
        t0 = time.perf_counter()
        mut = MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l)
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
        qf, qm = bench.synth_queries(nq, dq, be.device)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        rows = []
        for rnd in ("", ", again"):
            rows.append(("one-shot index" + rnd, timed(lambda: inf.vcmr_search(model, fixed, qf, qm, **kw), args.pass_reps, 2)))
            rows.append(("mutable index" + rnd, timed(lambda: inf.vcmr_search(model, mut, qf, qm, **kw), args.pass_reps, 2)))
        a = inf.vcmr_search(model, fixed, qf[:512], qm[:512])
        b = inf.vcmr_search(model, mut, qf[:512], qm[:512])
        same = bool(torch.equal(a["top_indices"], b["top_indices"]))
        g_fixed, g_mut = graph_ms(model, fixed, qf, qm), graph_ms(model, mut, qf, qm)
    t = fixed.feat1n[fixed.modalities[0]]
    layout = "length-bucketed image, %d tiles" % t.plan.n_tiles if getattr(t, "plan", None) is not None else \
        ("mask-free K6 (all_valid)" if getattr(t, "all_valid", False) else "plain tiles, mask bits")
    fa, fb = (rows[0][1][0] + rows[2][1][0]) / 2, (rows[1][1][0] + rows[3][1][0]) / 2
    lines += ["", "## Search on the %s corpus (%d videos x %d clips%s, hidden %d, bf16)" %
              (name, nv, l, ", real TVR clip counts" if lens is not None else ", full length", hidden), "",
              "One-shot index: %s, %.2f GB.  Mutable index at capacity = n_videos: plain tiles, mask bits, valid lengths always "
              "on, %.2f GB; filled by add() in %.1f s.  First 512 queries: the video lists are %s."
              % (layout, fixed.hbm_bytes() / 1e9, mut.hbm_bytes() / 1e9, fill_s, "identical" if same else "NOT identical"),
              "", "| index | vcmr_search, %d queries | 50-query graph replay |" % nq, "|---|---|---|"]
    for i, (n, tm) in enumerate(rows):
        lines.append("| %s | %s | %s |" % (n, fmt(tm), fmt((g_fixed, g_mut)[i & 1]) if i < 2 else ""))
    lines += ["", "Price of mutability on this corpus (medians, mean of both rounds): %.1f ms -> %.1f ms per %d-query pass (%+.1f %%); "
              "50-query replay %.3f ms -> %.3f ms (%+.1f %%)."
              % (fa, fb, nq, (fb / fa - 1) * 100, g_fixed[0], g_mut[0], (g_mut[0] / g_fixed[0] - 1) * 100)]
    for ln in lines[-12:]:
        print(ln, flush=True)
    del fixed, mut
    torch.cuda.empty_cache()


def putp_leg(args, lines):
    """xml_index_put_rows_packed next to xml_index_put_rows on the same batch (the put leg's shape), alternating."""
    import bench
    dev, dt, h, lpad, b = "cuda", torch.bfloat16, 768, 128, args.batch
    cap = 2 * b
    g = torch.Generator(device=dev).manual_seed(0)
    enc = [(torch.randn((b, lpad, h), device=dev, generator=g).to(dt), torch.randn((b, lpad, h), device=dev, generator=g).to(dt),
            torch.ones((b, lpad), device=dev)) for _ in range(2)]
    f2 = [torch.zeros((cap, lpad, h), dtype=dt, device=dev) for _ in range(2)]
    mk = [torch.zeros((cap, lpad), device=dev) for _ in range(2)]
    vlen = torch.zeros(cap, dtype=torch.int32, device=dev)
    sid = torch.zeros(cap, dtype=torch.int32, device=dev)
    live = torch.zeros((cap + 31) // 32, dtype=torch.int32, device=dev)
    slots = torch.from_numpy(np.random.default_rng(0).permutation(cap)[:b].astype(np.int32)).to(dev)
    k6 = [ops.TiledRows(torch.zeros(ops.q2c_tiled_numel(cap * lpad, h, dt), dtype=dt, device=dev), cap * lpad, h, (cap, lpad, h))
          for _ in range(2)]
    bits = [torch.zeros((cap, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    tiles = cap // 2                                          # as many tiles as the plain image: room for any lengths
    pk6 = [ops.TiledRows(torch.zeros(ops.q2c_tiled_numel(tiles * 256, h, dt), dtype=dt, device=dev), cap * lpad, h, (cap, lpad, h))
           for _ in range(2)]
    pbits = [torch.zeros((2 * tiles, 4), dtype=torch.int32, device=dev) for _ in range(2)]
    codes = torch.full((2 * tiles, 8), -2, dtype=torch.int32, device=dev)

    def runs_for(lens):
        table = BlockTable(tiles)
        nbs = [blocks_of(n) for n in lens]
        runs, _ = table.check_put(list(range(b)), nbs)
        return torch.tensor(runs, dtype=torch.int32, device=dev), max(nbs), sum(nbs)

    full, tvr = runs_for([lpad] * b), runs_for(bench.real_clip_counts(b, lpad).tolist())

    def plain():
        ops.index_put_rows([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], slots, None, k6, f2, mk, bits, vlen,
                           sid, live, lpad)

    def packed(r):
        ops.index_put_rows_packed([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], slots, None, r[0], r[1], pk6, f2,
                                  mk, pbits, codes, vlen, sid, live, lpad)

    row = 2 * b * lpad * h * 2                                  # bytes of one pass over the batch's rows, both modalities
    res = []
    for rnd in ("", ", again"):
        res += [("xml_index_put_rows" + rnd, timed(plain, args.reps), 4 * row),
                ("xml_index_put_rows_packed, 8-block runs (the same bytes)" + rnd, timed(lambda: packed(full), args.reps), 4 * row),
                ("xml_index_put_rows_packed, TVR clip counts (%d blocks of %d)" % (tvr[2], 8 * b) + rnd,
                 timed(lambda: packed(tvr), args.reps), 3 * row + row * tvr[2] // (8 * b))]
    lines += ["", "## The packed put kernel next to xml_index_put_rows", "",
              "The same %d-video batch (x %d clips x H = %d, bf16, two modalities, scattered slots, one process, alternating).  The "
              "packed entry reads f1 and writes K6 rows only inside a video's run; feat2 is read and written whole." % (b, lpad, h),
              "", "| what | time per call | bytes / s |", "|---|---|---|"]
    lines += ["| %s | %s | %.2f TB/s |" % (n, fmt(t, "us"), nb / (t[0] * 1e-3) / 1e12) for n, t, nb in res]
    for ln in lines[-10:]:
        print(ln, flush=True)


def tiles_in_corpus_order(lens, chunk):
    """Tiles a BlockTable uses when the corpus is added in order, `chunk` videos per call (host arithmetic only)."""
    table = BlockTable((len(lens) + 1) // 2)
    for r in range(0, len(lens), chunk):
        slots = list(range(r, min(r + chunk, len(lens))))
        table.commit_put(slots, table.check_put(slots, [blocks_of(n) for n in lens[r:r + chunk]])[0])
    return table.tiles_used(), table.stats()["straddles"]


def packed_search_leg(args, lines):
    """The ragged corpus on three forms in one process: one-shot packed index, mutable index (tiles=None), packed mutable
    index at tiles = what the corpus order needs (>= the one-shot plan's n_tiles) and at the plan's n_tiles + 10 %."""
    import bench
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3r"]
    nv, nq = args.videos, args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    lens = bench.real_clip_counts(nv, l)
    n_clips = [int(x) for x in lens.tolist()]
    batches = lambda: bench.context_batches(0, nv, l, dv, ds, True, True, be.device, lens=lens)      # noqa: E731
    need, straddles = tiles_in_corpus_order(n_clips, bench.CHUNK)
    with torch.no_grad():
        fixed = inf.build_corpus_index(model, batches(), l_ref=l, n_videos=nv)
        plan = fixed.feat1n[fixed.modalities[0]].plan
        t_plan = plan.n_tiles
        forms = [("one-shot packed index, %d tiles" % t_plan, fixed, t_plan),
                 ("mutable index, tiles=None (%d tiles)" % ((nv + 1) // 2), MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l),
                  (nv + 1) // 2)]
        for t in sorted({max(t_plan, need), max(-(-t_plan * 11 // 10), need)}):
            forms.append(("packed mutable index, tiles=%d" % t,
                          MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l, n_clips=n_clips, tiles=t), t))
        qf, qm = bench.synth_queries(nq, dq, be.device)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        passes = [[], []]
        for rnd in (0, 1):
            for _, index, _ in forms:
                passes[rnd].append(timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps, 2))
        want = inf.vcmr_search(model, fixed, qf[:512], qm[:512])
        same = [all(bool(torch.equal(want[k], inf.vcmr_search(model, index, qf[:512], qm[:512])[k])) for k in
                    ("top_indices", "top_scores", "flat_indices", "flat_scores")) for _, index, _ in forms]
        graphs = [graph_ms(model, index, qf, qm) for _, index, _ in forms]
    lines += ["", "## The ragged corpus (c3r) on three forms of index, one process", "",
              "%d videos x %d clips, real TVR clip counts, hidden %d, bf16, %d queries.  The one-shot plan packs the corpus into %d "
              "tiles (%d straddling videos); a BlockTable filled in corpus order, %d videos per call, needs %d tiles (%d straddling "
              "videos), so `tiles=%d` is the smallest packed mutable index this order fills%s.  First 512 queries against the one-shot "
              "index, video lists, scores, moments: %s."
              % (nv, l, hidden, nq, t_plan, plan.n_straddles, bench.CHUNK, need, straddles, max(t_plan, need),
                 "" if need <= t_plan else " (tiles=%d, the plan's own count, is refused)" % t_plan,
                 ", ".join("%s: %s" % (n.split(",")[0], "identical" if s else "NOT identical") for (n, _, _), s in zip(forms, same))),
              "", "| index | tiles / plan's | vcmr_search, %d queries | again | 50-query graph replay | index bytes |" % nq,
              "|---|---|---|---|---|---|"]
    for i, (name, index, t) in enumerate(forms):
        lines.append("| %s | %.3f | %s | %s | %s | %.2f GB |" % (name, t / t_plan, fmt(passes[0][i]), fmt(passes[1][i]), fmt(graphs[i]),
                                                               index.hbm_bytes() / 1e9))
    med = [(passes[0][i][0] + passes[1][i][0]) / 2 for i in range(len(forms))]
    for i in range(2, len(forms)):
        lines += ["", "%s: %.1f ms per pass against %.1f ms on tiles=None (%+.1f %%) and %.1f ms one-shot (x %.3f at a tile ratio of "
                  "%.3f); replay %.3f ms against %.3f ms and %.3f ms."
                  % (forms[i][0], med[i], med[1], (med[i] / med[1] - 1) * 100, med[0], med[i] / med[0], forms[i][2] / t_plan,
                     graphs[i][0], graphs[1][0], graphs[0][0])]
    for ln in lines[-14:]:
        print(ln, flush=True)
    del forms, fixed
    torch.cuda.empty_cache()


def compact_leg(args, lines):
    """Churn a packed mutable index on the ragged corpus until it is fragmented, then compact it (module docstring)."""
    import bench
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3r"]
    nv, nq = args.videos, args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    lens = bench.real_clip_counts(nv, l)
    n_clips = [int(x) for x in lens.tolist()]
    t_plan = ops.PackPlan([(torch.arange(l)[None] < lens[:, None]).float()]).n_tiles
    need, _ = tiles_in_corpus_order(n_clips, bench.CHUNK)
    tiles = max(-(-t_plan * 11 // 10), need)
    rng = np.random.default_rng(20)
    with torch.no_grad():
        index = MutableCorpusIndex.from_batches(model, bench.context_batches(0, nv, l, dv, ds, True, True, be.device, lens=lens),
                                                nv, l_ref=l, n_clips=n_clips, tiles=tiles)
        qf, qm = bench.synth_queries(nq, dq, be.device)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        search = lambda: inf.vcmr_search(model, index, qf, qm, **kw)      # noqa: E731
        keys = ("top_indices", "top_scores", "flat_indices", "flat_scores")
        k = nv // 10

        def churn(max_rounds):
            """-> (rounds done, the refusal or None)"""
            for rnd in range(max_rounds):
                index.remove([int(s) for s in rng.choice(index.table.live_slots(), k, replace=False)])
                new = torch.from_numpy(rng.choice(lens.numpy(), k))
                try:
                    at = 0
                    for batch in bench.context_batches(0, k, l, dv, ds, True, True, be.device, lens=new):
                        b = int(batch[0].shape[0])
                        index.add(*batch, n_clips=[int(x) for x in new[at:at + b].tolist()])
                        at += b
                except ValueError as e:
                    return rnd + 1, str(e)
            return max_rounds, None

        fresh = index.blocks.stats()
        t_fresh = timed(search, args.pass_reps, 2)
        # ---- first fragmentation: the launches of compact() alone, between HIP events (records uploaded beforehand)
        rounds1, refusal1 = churn(20)
        st_before = index.blocks.stats()
        t_before = timed(search, args.pass_reps, 2)
        want = {key: v.clone() for key, v in inf.vcmr_search(model, index, qf[:512], qm[:512]).items() if key in keys}
        mods = index.modalities
        t0 = time.perf_counter()
        plan = index.blocks.check_compact()
        plan_s = time.perf_counter() - t0
        staged = []
        for rnd in plan:
            recs, clears = rnd["records"], rnd["clears"]
            dev = index._to_device([x for r in recs for x in r] + [-1] * len(clears) + [x for r in clears for x in r])
            staged.append((dev, 17 * len(recs), len(clears)))
        # warm-up: a record that keeps every block of tile 0 (the first launch of a kernel is not its steady state)
        ops.index_move_blocks_packed(index._to_device([0] + [-1] * 16).view(1, 17), [index.feat1n[m] for m in mods],
                                     [index.mask_bits[m] for m in mods], index.codes)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(staged) + 1)]
        ev[0].record()
        for i, (dev, n, c) in enumerate(staged):
            ops.index_move_blocks_packed(dev[:n].view(-1, 17), [index.feat1n[m] for m in mods], [index.mask_bits[m] for m in mods],
                                         index.codes)
            ev[2 * i + 1].record()
            if c:
                ops.index_clear_rows_packed(dev[n:n + c], dev[n + c:].view(c, 2), 8, [index.mask[m] for m in mods],
                                            [index.mask_bits[m] for m in mods], index.codes, index.vlen, index.live.view(-1), l)
            ev[2 * i + 2].record()
        torch.cuda.synchronize()
        index.blocks.commit_compact(plan)
        per_round = [ev[2 * i].elapsed_time(ev[2 * i + 2]) for i in range(len(staged))]
        move_only = [ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(len(staged))]
        moved = [sum(nb for (_, nb), _ in rnd["moves"].values()) for rnd in plan]
        row_bytes = sum(index.feat2[m].shape[2] * index.feat2[m].element_size() for m in mods)
        nbytes = [mv * 16 * row_bytes for mv in moved]
        st_after = index.blocks.stats()
        t_after = timed(search, args.pass_reps, 2)
        got = inf.vcmr_search(model, index, qf[:512], qm[:512])
        same = all(bool(torch.equal(want[key], got[key])) for key in keys)
        # ---- second fragmentation: the whole compact() call as a caller sees it
        rounds2, refusal2 = churn(20)
        st2_before = index.blocks.stats()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        res = index.compact()
        e1.record()
        torch.cuda.synchronize()
        call_ms, call_ev = (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
        st2_after = index.blocks.stats()
    tot_ms, tot_b = sum(per_round), sum(nbytes)
    show = lambda st: ", ".join("%s %d" % (key, st[key]) for key in      # noqa: E731
                                ("free_blocks", "largest_free_run", "largest_free_run_partial", "tiles_empty", "tiles_partial",
                                 "tiles_full", "tiles_used", "straddles"))
    lines += ["", "## Compaction of the packed mutable index (compact leg)", "",
              "%d videos, real TVR clip counts, hidden %d, bf16, two modalities; the one-shot plan needs %d tiles, the index has "
              "`tiles=%d` (plan + 10 %%; filling in corpus order needs %d).  Churn: a random 10 %% (%d videos) removed and re-added "
              "with lengths drawn afresh from the TVR counts, until an add is refused or 20 rounds have passed."
              % (nv, hidden, t_plan, tiles, need, k), "",
              "First churn: %d rounds, %s.  Then the launches of `compact()` alone, records uploaded beforehand, between HIP events "
              "(host planning, `check_compact`: %.1f ms):" % (rounds1, "refused: `%s`" % refusal1 if refusal1 else "no add refused", plan_s * 1e3),
              "", "| round | records (tiles touched) | runs cleared | blocks moved | image bytes moved | move launch | move + clear launches | payload rate | read + written |",
              "|---|---|---|---|---|---|---|---|---|"]
    for i, rnd in enumerate(plan):
        rate = nbytes[i] / (move_only[i] * 1e-3) / 1e12 if move_only[i] > 0 else 0.0      # of the move launch alone
        lines.append("| %d | %d | %d | %d | %.1f MB | %.1f us | %.1f us | %.2f TB/s | %.2f TB/s |"
                     % (i + 1, len(rnd["records"]), len(rnd["clears"]), moved[i], nbytes[i] / 1e6, move_only[i] * 1e3,
                        per_round[i] * 1e3, rate, 2 * rate))
    if plan:
        mv_ms = sum(move_only)
        lines.append("| all | | | %d | %.1f MB | %.1f us | %.1f us | %.2f TB/s | %.2f TB/s |"
                     % (sum(moved), tot_b / 1e6, mv_ms * 1e3, tot_ms * 1e3, tot_b / (mv_ms * 1e-3) / 1e12,
                        2 * tot_b / (mv_ms * 1e-3) / 1e12))
    lines += ["", "The rates are image bytes over the move launch alone (one event pair around a single launch: a single sample, "
              "event resolution included); `read + written` counts every moved byte twice, as the put kernel's rows above do."]
    lines += ["", "`stats()` freshly filled: %s." % show(fresh), "", "`stats()` before: %s." % show(st_before), "",
              "`stats()` after: %s." % show(st_after), "",
              "| %d-query pass (vcmr_search) | time |" % nq, "|---|---|", "| freshly filled | %s |" % fmt(t_fresh),
              "| churned, before compaction | %s |" % fmt(t_before), "| after compaction | %s |" % fmt(t_after), "",
              "First 512 queries before against after compaction (video lists, scores, moments): %s."
              % ("identical" if same else "NOT identical"), "",
              "Second churn: %d rounds, %s.  The whole `index.compact()` call: %.1f ms on the host clock around a device synchronise, "
              "%.1f ms between HIP events around the call (planning and enqueueing included); it returned %s.  `stats()` before: "
              "%s; after: %s." % (rounds2, "refused: `%s`" % refusal2 if refusal2 else "no add refused", call_ms, call_ev,
                                  ", ".join("%s %s" % kv for kv in sorted(res.items())), show(st2_before), show(st2_after))]
    for ln in lines[-26:]:
        print(ln, flush=True)
    del index
    torch.cuda.empty_cache()


def full_clip_counts(nv):
    """bench.real_clip_counts with the histogram's last bin undone: the fixture is clipped at 128 clips and records the longest
    video (182 clips), so the videos of that bin get lengths spread evenly over 128 .. 182."""
    import bench
    import json
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "tvr_clip_count_hist.json")))
    lens = bench.real_clip_counts(nv, rec["clipped_at"]).clone()
    last = torch.nonzero(lens == rec["clipped_at"]).view(-1)
    lens[last] = torch.linspace(rec["clipped_at"], rec["max_unclipped"], last.numel()).round().to(lens.dtype)
    return lens


def chains_leg(args, lines):
    """Long videos as chains of slots on the packed mutable index (module docstring)."""
    import bench
    from tvretrieval_amd.ingest import plan_parts
    _, _, _, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3r"]
    nv, nq, ov, l = args.videos, args.queries, 16, args.chains_l
    be = bench.HipBackend(0)
    dev = be.device
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    full = full_clip_counts(nv)
    cut = torch.clamp(full, max=l)
    table = plan_parts(full.numpy(), l, ov)
    n_parts = table.n_parts
    counts = np.diff(table.group_start)
    part_len = torch.from_numpy(table.part_len.astype(np.int64))
    tiles = max(tiles_in_corpus_order([int(x) for x in table.part_len], bench.CHUNK)[0],
                tiles_in_corpus_order([int(x) for x in cut.tolist()], bench.CHUNK)[0])

    def part_batches():
        """(batch, its part table) for groups of ~bench.CHUNK - 64 videos; rows [r0, r1) of the synthetic corpus of parts"""
        v0 = 0
        while v0 < nv:
            v1 = min(v0 + bench.CHUNK - 64, nv)
            t = plan_parts(full[v0:v1].numpy(), l, ov)
            r0 = int(table.group_start[v0])
            pieces = list(bench.context_batches(r0, r0 + t.n_parts, l, dv, ds, True, True, dev, lens=part_len))
            yield tuple(torch.cat([p[i] for p in pieces]) for i in range(4)), t
            v0 = v1

    with torch.no_grad():
        t0 = time.perf_counter()
        chained = MutableCorpusIndex.create(model, n_parts, l_ref=l, tiles=tiles, part_overlap=ov)
        for batch, t in part_batches():
            chained.add(*batch, parts=t)
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
        plain = MutableCorpusIndex.from_batches(model, bench.context_batches(0, nv, l, dv, ds, True, True, dev, lens=cut), n_parts,
                                                l_ref=l, n_clips=[int(x) for x in cut.tolist()], tiles=tiles)
        assert chained.n_live == n_parts and chained.n_videos_live == nv == plain.n_live
        assert chained.table.heads() == [int(x) for x in table.group_start[:-1]]           # slot p holds part p
        qf, qm = bench.synth_queries(nq, dq, dev)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        passes = []
        for rnd in ("", ", again"):
            passes.append(("packed mutable index, videos cut at %d clips (no part_overlap)%s" % (l, rnd),
                           timed(lambda: inf.vcmr_search(model, plain, qf, qm, **kw), args.pass_reps, 2)))
            passes.append(("packed mutable index, part_overlap=%d%s" % (ov, rnd),
                           timed(lambda: inf.vcmr_search(model, chained, qf, qm, **kw), args.pass_reps, 2)))
        q2c = inf.vcmr_search(model, chained, qf, qm, **kw)["q2c"]
        parts_dev = table.to(dev)
        live = chained.live
        # the same chains over a random permutation of the slots (what an index looks like after many updates)
        perm = np.random.default_rng(0).permutation(n_parts)
        head, nxt = np.arange(n_parts, dtype=np.int32), np.full(n_parts, -1, dtype=np.int32)
        gs = table.group_start
        for v in np.nonzero(counts > 1)[0]:
            ch = perm[gs[v]:gs[v + 1]]
            head[ch] = ch[0]
            nxt[ch[:-1]] = ch[1:]
        import types
        scattered = types.SimpleNamespace(chain_head=torch.from_numpy(head).to(dev), chain_next=torch.from_numpy(nxt).to(dev),
                                          max_parts=chained.max_parts)
        all_videos = torch.full((1, (nv + 31) // 32), -1, dtype=torch.int32, device=dev)
        want = ops.group_best_allow(q2c[:512], parts_dev, None)
        same = bool(torch.equal(want, ops.chain_best_allow(q2c[:512], chained, live)))
        folds = []
        for rows in (nq, 50):
            s = q2c[:rows]
            for rnd in ("", ", again"):
                folds += [(rows, "xml_group_best_allow, fixed part table (the yardstick)" + rnd,
                           timed(lambda: ops.group_best_allow(s, parts_dev, None), args.reps)),
                          (rows, "xml_group_best_allow with allow words over the videos" + rnd,
                           timed(lambda: ops.group_best_allow(s, parts_dev, all_videos), args.reps)),
                          (rows, "xml_chain_best_allow, slots in corpus order" + rnd,
                           timed(lambda: ops.chain_best_allow(s, chained, live), args.reps)),
                          (rows, "xml_chain_best_allow, the same chains over permuted slots" + rnd,
                           timed(lambda: ops.chain_best_allow(s, scattered, live), args.reps))]
    lines += ["", "## Long videos as chains of slots (chains leg)", "",
              "%d videos with the TVR clip counts (the clipped last bin spread up to %d clips), l_ref = %d, part_overlap = %d: %d videos of more than %d "
              "clips, %d parts = slots (capacity = parts, filled in corpus order in %.1f s, so slot p holds part p of the fixed part "
              "table), hidden %d, bf16, %d queries, both packed indexes at tiles = %d.  Fold of the first 512 score rows, chain fold "
              "against xml_group_best_allow: %s."
              % (nv, int(full.max()), l, ov, int((counts > 1).sum()), l, n_parts, fill_s, hidden, nq, tiles,
                 "identical" if same else "NOT identical"),
              "", "| index | vcmr_search, %d queries |" % nq, "|---|---|"]
    lines += ["| %s | %s |" % (n, fmt(t)) for n, t in passes]
    a, b = (passes[0][1][0] + passes[2][1][0]) / 2, (passes[1][1][0] + passes[3][1][0]) / 2
    lines += ["", "Price of the chains on this corpus (medians, mean of both rounds): %.2f ms -> %.2f ms per %d-query pass (%+.2f %%)."
              % (a, b, nq, (b / a - 1) * 100), "", "| score rows | fold | time per call |", "|---|---|---|"]
    lines += ["| %d | %s | %s |" % (r, n, fmt(t, "us")) for r, n, t in folds]
    for rows in (nq, 50):
        med = {}
        for r, n, t in folds:
            if r == rows:
                med.setdefault(n.replace(", again", ""), []).append(t[0])
        m = {k: sum(v) / len(v) for k, v in med.items()}
        base = m["xml_group_best_allow, fixed part table (the yardstick)"]
        lines += ["", "%d rows: chain fold over contiguous fold %.2f (corpus order), %.2f (permuted slots); %.1f us against %.1f us; "
                  "the score matrix is %.1f MB, %.1f us at the %.1f TB/s stream rate."
                  % (rows, m["xml_chain_best_allow, slots in corpus order"] / base,
                     m["xml_chain_best_allow, the same chains over permuted slots"] / base,
                     m["xml_chain_best_allow, slots in corpus order"] * 1e3, base * 1e3, rows * n_parts * 4 / 1e6,
                     rows * n_parts * 4 / HBM_STREAM * 1e6, HBM_STREAM / 1e12)]
    for ln in lines[-34:]:
        print(ln, flush=True)
    del chained, plain
    torch.cuda.empty_cache()


def exact_put_leg(args, lines, b):
    """(a) xml_index_put_rows_exact on a b-video f32 batch, next to xml_index_put_rows on a plain f32 index fed the same rows and
    to the one-shot exact-rank chain over the same rows."""
    dev, h, lpad, bf16 = "cuda", 768, 128, torch.bfloat16
    cap = 2 * b
    g = torch.Generator(device=dev).manual_seed(0)
    enc = [(torch.randn((b, lpad, h), device=dev, generator=g), torch.randn((b, lpad, h), device=dev, generator=g),
            torch.ones((b, lpad), device=dev)) for _ in range(2)]
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)        # noqa: E731
    split = lambda: ops.SplitRows(z(cap, lpad, h, dt=torch.int32), z(cap, lpad))   # noqa: E731
    k6 = [ops.TiledRows(z(ops.q2c_tiled_numel(cap * lpad, h, bf16), dt=bf16), cap * lpad, h, (cap, lpad, h)) for _ in range(2)]
    resc, f2, err = [split() for _ in range(2)], [split() for _ in range(2)], [z(cap, lpad) for _ in range(2)]
    mk, bits = [z(cap, lpad) for _ in range(2)], [z(cap, 4, dt=torch.int32) for _ in range(2)]
    ec, vlen, sid, live = z(2), z(cap, dt=torch.int32), z(cap, dt=torch.int32), z((cap + 31) // 32, dt=torch.int32)
    pk6 = [ops.TiledRows(z(ops.q2c_tiled_numel(cap * lpad, h, torch.float32)), cap * lpad, h, (cap, lpad, h)) for _ in range(2)]
    pf2 = [z(cap, lpad, h) for _ in range(2)]
    scattered = torch.from_numpy(np.random.default_rng(0).permutation(cap)[:b].astype(np.int32)).to(dev)
    cols = lambda i: [e[i] for e in enc]                                           # noqa: E731

    def put_exact():
        ops.index_put_rows_exact(cols(0), cols(1), cols(2), scattered, None, k6, resc, f2, err, mk, bits, ec, vlen, sid, live, lpad)

    def put_plain():
        ops.index_put_rows(cols(0), cols(1), cols(2), scattered, None, pk6, pf2, mk, bits, vlen, sid, live, lpad)

    def chain():        # inference._exact_filter_operands + _finish_index; no mask handed over: no host read of it
        for m in range(2):
            fn = ops.l2norm_rows(enc[m][0])
            fb, _ = ops.round_bf16_rows_err(fn)
            ops.split_f16_rows(fn, ops.F16_UNIT_LOG2)
            ops.split_f16_rows(enc[m][1])
            ops.pack_q2c_corpus(fb)

    per = b * lpad * h
    by_exact = 2 * (per * (4 + 4 + 2 + 4 + 4) + b * lpad * 4 * 5 + b * 16)        # f1, f2 read; filter, re-score, feat2 written
    by_plain = 2 * (per * 16 + b * lpad * 4 * 2 + b * 16)
    res = []
    for rnd in ("", ", again"):
        res += [("xml_index_put_rows_exact (mode f16s), scattered slots" + rnd, timed(put_exact, args.reps), by_exact),
                ("xml_index_put_rows, plain f32 index, the same rows" + rnd, timed(put_plain, args.reps), by_plain),
                ("one-shot chain: l2norm_rows + round_bf16_rows_err + split_f16_rows x 2 + pack_q2c_corpus, per modality (10 launches)" + rnd,
                 timed(chain, args.reps), by_exact)]
    lines += ["", "### Batches of %d videos" % b, "",
              "%d videos x %d clips x H = %d, f32 rows, two modalities into an index of %d slots.  Bytes counted from the shapes: "
              "%.1f MB per exact-rank put (f1 and f2 read once; bf16 filter rows, split-f16 re-score rows and split-f16 feat2 written "
              "once; norms, scales, masks), %.1f us at the %.1f TB/s HBM stream rate; %.1f MB per plain f32 put.  The chain is "
              "charged the exact-rank put's bytes: its temporaries are its own cost."
              % (b, lpad, h, cap, by_exact / 1e6, by_exact / HBM_STREAM * 1e6, HBM_STREAM / 1e12, by_plain / 1e6),
              "", "| what | time per call | videos / s | bytes / s |", "|---|---|---|---|"]
    for name, t, moved in res:
        lines.append("| %s | %s | %.3g | %.2f TB/s |" % (name, fmt(t, "us"), b / (t[0] * 1e-3), moved / (t[0] * 1e-3) / 1e12))
    med = lambda i: (res[i][1][0] + res[i + 3][1][0]) / 2                         # noqa: E731
    lines += ["", "Medians, mean of both rounds: exact-rank put %.1f us, plain f32 put %.1f us (x %.2f), one-shot chain %.1f us "
              "(x %.2f of the exact-rank put)." % (med(0) * 1e3, med(1) * 1e3, med(0) / med(1), med(2) * 1e3, med(2) / med(0))]
    for ln in lines[-12:]:
        print(ln, flush=True)
    torch.cuda.empty_cache()


def exact_leg(args, lines):
    """Exact-rank mode on a mutable index at the headline shape (capacity 21 793, H = 768, ops.F16S model, tiles=None)."""
    import bench
    lines += ["## Exact-rank mode on an index that takes updates (create(..., exact_rank=True), mode f16s)", "",
              "## (a) The put kernel alone"]
    for b in (256, 2048):
        exact_put_leg(args, lines, b)
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
    nv, nq = args.videos, args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), ops.F16S)
    batches = lambda: bench.context_batches(0, nv, l, dv, ds, True, True, be.device)      # noqa: E731
    with torch.no_grad():
        fixed = inf.build_corpus_index(model, batches(), l_ref=l, n_videos=nv, exact_filter=True, length_buckets=False)
        t0 = time.perf_counter()
        mut = MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l, exact_rank=True)
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
        qf, qm = bench.synth_queries(nq, dq, be.device)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        same_bound = [mut.exact.e_c[m] == fixed.exact.e_c[m] for m in mut.modalities]
        rows = []
        for rnd in ("", ", again"):
            rows.append(("one-shot exact index" + rnd, timed(lambda: inf.vcmr_search(model, fixed, qf, qm, **kw), args.pass_reps, 2)))
            rows.append(("mutable exact index" + rnd, timed(lambda: inf.vcmr_search(model, mut, qf, qm, **kw), args.pass_reps, 2)))
        a = inf.vcmr_search(model, fixed, qf[:512], qm[:512])
        b = inf.vcmr_search(model, mut, qf[:512], qm[:512])
        same = all(bool(torch.equal(a[k], b[k])) for k in ("top_indices", "top_scores", "flat_indices", "flat_scores"))
        g_fixed, g_mut = graph_ms(model, fixed, qf, qm), graph_ms(model, mut, qf, qm)
        # (c) certificate failures per pass: the running bound, stale after removals, tightened
        fails = [("one-shot index, its host e_c", int(inf.vcmr_search(model, fixed, qf, qm, **kw)["exact"]["n_fail"]), fixed.exact.e_c),
                 ("mutable index right after the adds (running bound)", int(inf.vcmr_search(model, mut, qf, qm, **kw)["exact"]["n_fail"]),
                  dict(mut.exact.e_c.items()))]
        gone = np.random.default_rng(3).permutation(nv)[:nv // 10].tolist()
        mut.remove(gone)
        fails.append(("after removing %d slots (10 %%), bound left alone" % len(gone),
                      int(inf.vcmr_search(model, mut, qf, qm, **kw)["exact"]["n_fail"]), dict(mut.exact.e_c.items())))
        t_tight = timed(mut.tighten_error_bound, args.reps)
        fails.append(("after tighten_error_bound()", int(inf.vcmr_search(model, mut, qf, qm, **kw)["exact"]["n_fail"]),
                      dict(mut.exact.e_c.items())))
    fa, fb = (rows[0][1][0] + rows[2][1][0]) / 2, (rows[1][1][0] + rows[3][1][0]) / 2
    plain_bytes = sum(t.numel() * t.element_size() for d in (mut.feat1n, mut.feat2, mut.mask) for t in d.values())
    lines += ["", "## (b) Search at the headline shape (%d videos x %d clips, full length, hidden %d, ops.F16S model)" % (nv, l, hidden),
              "", "One-shot build_corpus_index(exact_filter=True, length_buckets=False): %.2f GB.  Mutable exact index at capacity = "
              "n_videos: %.2f GB, filled by add() in %.1f s (encoder included).  The running bound equals the one-shot e_c bit for "
              "bit: %s.  First 512 queries: video lists, weights, moment lists and scores are %s."
              % (fixed.hbm_bytes() / 1e9, mut.hbm_bytes() / 1e9, fill_s, same_bound, "bitwise identical" if same else "NOT identical"),
              "", "| index | vcmr_search, %d queries | 50-query graph replay |" % nq, "|---|---|---|"]
    for i, (n, tm) in enumerate(rows):
        lines.append("| %s | %s | %s |" % (n, fmt(tm), fmt((g_fixed, g_mut)[i & 1]) if i < 2 else ""))
    lines += ["", "Price of mutability in exact-rank mode (medians, mean of both rounds): %.1f ms -> %.1f ms per %d-query pass "
              "(%+.1f %%); 50-query replay %.3f ms -> %.3f ms (%+.1f %%).  The same kernels run on both; the mutable index adds the "
              "live words to the candidate K8 and to select_ge_rows, K6 reads mask bits, K7 / K9 take the valid lengths."
              % (fa, fb, nq, (fb / fa - 1) * 100, g_fixed[0], g_mut[0], (g_mut[0] / g_fixed[0] - 1) * 100),
              "", "## (c) Certificate failures per %d queries" % nq, "", "| state | failing queries | e_c (video, sub) |", "|---|---|---|"]
    lines += ["| %s | %d | %s |" % (n, f, ", ".join("%.6g" % ec[m] for m in mut.modalities)) for n, f, ec in fails]
    lines += ["", "tighten_error_bound() over %d slots x %d rows x 2 modalities (one workgroup per modality): %s."
              % (nv, mut.lpad, fmt(t_tight)),
              "", "## (d) hbm_bytes()", "",
              "Mutable exact index %.3f GB: filter image, feat2 and masks %.3f GB, re-score rows and the scales of the split rows "
              "%.3f GB, err_rows + e_c_dev %.3f GB (ExactFilter.hbm_bytes_extra: %d bytes), the rest mask words, vlen, live, slot_ids."
              % (mut.hbm_bytes() / 1e9, plain_bytes / 1e9,
                 sum(t.numel() * 4 + t.inv.numel() * 4 for t in mut.exact.feat1n_f32.values()) / 1e9
                 + sum(t.inv.numel() * 4 for t in mut.feat2.values()) / 1e9,
                 mut.exact.hbm_bytes_extra() / 1e9, mut.exact.hbm_bytes_extra())]
    for ln in lines[-24:]:
        print(ln, flush=True)
    del fixed, mut
    torch.cuda.empty_cache()


def exactp_put_leg(args, lines, b):
    """xml_index_put_rows_packed_exact on a b-video f32 batch with the TVR clip counts next to xml_index_put_rows_exact on the
    same rows and masks (the plain per-slot filter image), alternating."""
    import bench
    dev, h, lpad, bf16 = "cuda", 768, 128, torch.bfloat16
    cap = 2 * b
    lens = [int(x) for x in bench.real_clip_counts(b, lpad).tolist()]
    g = torch.Generator(device=dev).manual_seed(0)
    mask = (torch.arange(lpad, device=dev)[None] < torch.tensor(lens, device=dev)[:, None]).float()
    enc = [(torch.randn((b, lpad, h), device=dev, generator=g), torch.randn((b, lpad, h), device=dev, generator=g), mask)
           for _ in range(2)]
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)        # noqa: E731
    split = lambda: ops.SplitRows(z(cap, lpad, h, dt=torch.int32), z(cap, lpad))   # noqa: E731
    tiles = cap // 2                                          # as many tiles as the plain image: room for any lengths
    image = lambda rows: [ops.TiledRows(z(ops.q2c_tiled_numel(rows, h, bf16), dt=bf16), cap * lpad, h, (cap, lpad, h))   # noqa: E731
                          for _ in range(2)]
    k6, pk6 = image(cap * lpad), image(tiles * 256)
    resc, f2, err = [split() for _ in range(2)], [split() for _ in range(2)], [z(cap, lpad) for _ in range(2)]
    mk = [z(cap, lpad) for _ in range(2)]
    bits, pbits = [z(cap, 4, dt=torch.int32) for _ in range(2)], [z(2 * tiles, 4, dt=torch.int32) for _ in range(2)]
    codes = torch.full((2 * tiles, 8), -2, dtype=torch.int32, device=dev)
    ec, vlen, sid, live = z(2), z(cap, dt=torch.int32), z(cap, dt=torch.int32), z((cap + 31) // 32, dt=torch.int32)
    scattered = torch.from_numpy(np.random.default_rng(0).permutation(cap)[:b].astype(np.int32)).to(dev)
    table = BlockTable(tiles)
    nbs = [blocks_of(n) for n in lens]
    runs = torch.tensor(table.check_put(list(range(b)), nbs)[0], dtype=torch.int32, device=dev)
    cols = lambda i: [e[i] for e in enc]                                           # noqa: E731

    def put_exact():
        ops.index_put_rows_exact(cols(0), cols(1), cols(2), scattered, None, k6, resc, f2, err, mk, bits, ec, vlen, sid, live, lpad)

    def put_packed():
        ops.index_put_rows_packed_exact(cols(0), cols(1), cols(2), scattered, None, runs, max(nbs), pk6, resc, f2, err, mk, pbits,
                                        codes, ec, vlen, sid, live, lpad)

    per = b * lpad * h
    rest = 2 * (per * (4 + 4 + 4 + 4) + b * lpad * 4 * 5 + b * 16)                # f1, f2 read; re-score, feat2 written; norms, masks
    by_exact, by_packed = rest + 2 * per * 2, rest + 2 * sum(nbs) * 16 * h * 2
    res = []
    for rnd in ("", ", again"):
        res += [("xml_index_put_rows_packed_exact (mode f16s), TVR clip counts: %d blocks of %d" % (sum(nbs), 8 * b) + rnd,
                 timed(put_packed, args.reps), by_packed),
                ("xml_index_put_rows_exact (mode f16s), the same rows and masks" + rnd, timed(put_exact, args.reps), by_exact)]
    lines += ["", "### Batches of %d videos" % b, "",
              "%d videos x %d clips x H = %d, f32 rows, two modalities, prefix masks of the TVR clip counts, scattered slots of %d; "
              "runs handed out by a BlockTable of %d tiles.  Bytes counted from the shapes: %.1f MB per packed put (the filter rows "
              "of the runs only), %.1f MB per plain exact-rank put." % (b, lpad, h, cap, tiles, by_packed / 1e6, by_exact / 1e6),
              "", "| what | time per call | videos / s | bytes / s |", "|---|---|---|---|"]
    for name, t, moved in res:
        lines.append("| %s | %s | %.3g | %.2f TB/s |" % (name, fmt(t, "us"), b / (t[0] * 1e-3), moved / (t[0] * 1e-3) / 1e12))
    med = lambda i: (res[i][1][0] + res[i + 2][1][0]) / 2                         # noqa: E731
    lines += ["", "Medians, mean of both rounds: packed exact-rank put %.1f us, exact-rank put %.1f us (x %.3f)."
              % (med(0) * 1e3, med(1) * 1e3, med(0) / med(1))]
    for ln in lines[-10:]:
        print(ln, flush=True)
    torch.cuda.empty_cache()


def exact_put_ab_leg(args, lines):
    """xml_index_put_rows_exact of this library against the same entry of another build of it (--parent-lib: a libxmlhip.so
    built from the commit to compare with), both loaded into this process and called through the C ABI on the same tensors
    (exact_put_leg's shapes), alternating, four rounds: the regression guard of a change to that kernel's source."""
    import ctypes
    from tvretrieval_amd import _lib
    new, old = _lib.load(), ctypes.CDLL(os.path.abspath(args.parent_lib))
    old.xml_index_put_rows_exact.restype, old.xml_index_put_rows_exact.argtypes = _lib.SIGNATURES_EXACT["xml_index_put_rows_exact"]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                  # noqa: E731
    lines += ["", "## (g) A/B of xml_index_put_rows_exact against another build of the library", "",
              "`xml_index_put_rows_exact` of this library and of `--parent-lib` (built from the parent commit), loaded into one "
              "process and called through the C ABI on the same tensors (section (a)'s shapes: ones masks, scattered slots, mode "
              "f16s, tiled filter image), alternating, four rounds of %d repetitions each." % args.reps]
    for b in (256, 2048):
        dev, h, lpad, bf16 = "cuda", 768, 128, torch.bfloat16
        cap = 2 * b
        g = torch.Generator(device=dev).manual_seed(0)
        enc = [(torch.randn((b, lpad, h), device=dev, generator=g), torch.randn((b, lpad, h), device=dev, generator=g),
                torch.ones((b, lpad), device=dev)) for _ in range(2)]
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)    # noqa: E731
        side, outs = [], []
        for _ in range(2):      # k6, rescore, rescore_inv, feat2, feat2_inv, err, imask, bits
            t = [z(ops.q2c_tiled_numel(cap * lpad, h, bf16), dt=bf16), z(cap, lpad, h, dt=torch.int32), z(cap, lpad),
                 z(cap, lpad, h, dt=torch.int32), z(cap, lpad), z(cap, lpad), z(cap, lpad), z(cap, 4, dt=torch.int32)]
            side += [ptr(x) for x in t]
            outs += t
        ec, vlen, sid, live = z(2), z(cap, dt=torch.int32), z(cap, dt=torch.int32), z((cap + 31) // 32, dt=torch.int32)
        outs += [ec, vlen, sid, live]
        slots = torch.from_numpy(np.random.default_rng(0).permutation(cap)[:b].astype(np.int32)).to(dev)

        def call(lib):
            st = lib.xml_index_put_rows_exact(2, ops.EXACT_F16S, ptr(enc[0][0]), ptr(enc[0][1]), ptr(enc[0][2]), ptr(enc[1][0]),
                                              ptr(enc[1][1]), ptr(enc[1][2]), ptr(slots), None, b, lpad, *side, ptr(ec), ptr(vlen),
                                              ptr(sid), ptr(live), cap, lpad, lpad, h, 0, 1,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if st != 0:
                raise RuntimeError("xml_index_put_rows_exact returned %d" % st)
        call(new)
        mine = [t.clone() for t in outs]
        for t in outs:
            t.zero_()
        call(old)
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(mine, outs))
        rounds = [(timed(lambda: call(old), args.reps), timed(lambda: call(new), args.reps)) for _ in range(4)]
        mo, mn = (float(np.median([r[i][0] for r in rounds])) for i in (0, 1))
        lo, hi = min(r[0][0] for r in rounds), max(r[0][0] for r in rounds)
        lines += ["", "### Batches of %d videos; every output tensor bitwise equal: %s" % (b, same), "",
                  "| round | --parent-lib | this library |", "|---|---|---|"]
        lines += ["| %d | %s | %s |" % (i, fmt(r[0], "us"), fmt(r[1], "us")) for i, r in enumerate(rounds)]
        lines += ["", "Median of the four medians: --parent-lib %.1f us, this library %.1f us (%+.2f %%); the medians of --parent-lib "
                  "span %.1f .. %.1f us (%.2f %% of their median)."
                  % (mo * 1e3, mn * 1e3, (mn / mo - 1) * 100, lo * 1e3, hi * 1e3, (hi - lo) / mo * 100)]
        for ln in lines[-9:]:
            print(ln, flush=True)
        del enc, outs, mine, side
        torch.cuda.empty_cache()


def exactp_leg(args, lines):
    """Exact-rank mode with the packed filter image (create(..., exact_rank=True, filter_tiles=N)) on the ragged corpus at the
    headline shape: the put next to xml_index_put_rows_exact, the 10 000-query pass and the 50-query replay on four forms."""
    import bench
    lines += ["## Exact-rank mode with the packed filter image (create(..., exact_rank=True, filter_tiles=N), mode f16s)", "",
              "## (e) The packed exact-rank put next to xml_index_put_rows_exact"]
    for b in (256, 2048):
        exactp_put_leg(args, lines, b)
    _, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3r"]
    nv, nq = args.videos, args.queries
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), ops.F16S)
    lens = bench.real_clip_counts(nv, l)
    n_clips = [int(x) for x in lens.tolist()]
    batches = lambda: bench.context_batches(0, nv, l, dv, ds, True, True, be.device, lens=lens)      # noqa: E731
    need, straddles = tiles_in_corpus_order(n_clips, bench.CHUNK)
    keys = ("top_indices", "top_scores", "flat_indices", "flat_scores")
    with torch.no_grad():
        forms = [("filter_tiles=%d (corpus order)" % t,
                  MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l, n_clips=n_clips, exact_rank=True, filter_tiles=t), t)
                 for t in (need, -(-need * 11 // 10))]
        forms.append(("exact_rank=True, plain per-slot filter image",
                      MutableCorpusIndex.from_batches(model, batches(), nv, l_ref=l, exact_rank=True), (nv + 1) // 2))
        fixed = inf.build_corpus_index(model, batches(), l_ref=l, n_videos=nv, exact_filter=True)
        plan = fixed.feat1n[fixed.modalities[0]].plan
        forms.append(("one-shot build_corpus_index(exact_filter=True), length buckets", fixed, plan.n_tiles))
        qf, qm = bench.synth_queries(nq, dq, be.device)
        kw = dict(n_valid_tokens=int(qm.sum().item()))
        passes = [[], []]
        for rnd in (0, 1):
            for _, index, _ in forms:
                passes[rnd].append(timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps, 2))
        firsts = [inf.vcmr_search(model, index, qf[:512], qm[:512]) for _, index, _ in forms]
        same = [all(bool(torch.equal(firsts[2][k], o[k])) for k in keys) for o in firsts]
        fails = [int(inf.vcmr_search(model, index, qf, qm, **kw)["exact"]["n_fail"]) for _, index, _ in forms]
        bounds = [[float(index.exact.e_c[m]) for m in index.modalities] for _, index, _ in forms]
        graphs = [graph_ms(model, index, qf, qm) for _, index, _ in forms]
    lines += ["", "## (f) Search on the ragged corpus (%d videos x %d clips, real TVR clip counts, hidden %d, ops.F16S model, %d queries)"
              % (nv, l, hidden, nq), "",
              "A BlockTable filled in corpus order, %d videos per call, needs %d tiles (%d straddling videos); the one-shot plan "
              "packs the corpus into %d tiles; the plain per-slot filter image has %d.  First 512 queries, video lists, weights, "
              "moment lists and scores against the plain exact-rank index: %s."
              % (bench.CHUNK, need, straddles, plan.n_tiles, (nv + 1) // 2,
                 "; ".join("%s: %s" % (n, "bitwise identical" if s else "NOT identical") for (n, _, _), s in zip(forms, same))),
              "", "| index | filter tiles | vcmr_search, %d queries | again | 50-query graph replay | failing certificates per pass | "
              "e_c (video, sub) | hbm_bytes() |" % nq, "|---|---|---|---|---|---|---|---|"]
    for i, (name, index, t) in enumerate(forms):
        lines.append("| %s | %d | %s | %s | %s | %d | %s | %.3f GB |"
                     % (name, t, fmt(passes[0][i]), fmt(passes[1][i]), fmt(graphs[i]), fails[i],
                        ", ".join("%.6g" % x for x in bounds[i]), index.hbm_bytes() / 1e9))
    med = [(passes[0][i][0] + passes[1][i][0]) / 2 for i in range(len(forms))]
    for i in (0, 1):
        lines += ["", "%s: %.1f ms per pass against %.1f ms on the plain filter image (%+.1f %%) and %.1f ms one-shot (x %.3f); replay "
                  "%.3f ms against %.3f ms and %.3f ms."
                  % (forms[i][0], med[i], med[2], (med[i] / med[2] - 1) * 100, med[3], med[i] / med[3], graphs[i][0], graphs[2][0],
                     graphs[3][0])]
    for ln in lines[-14:]:
        print(ln, flush=True)
    del forms, fixed, firsts
    torch.cuda.empty_cache()
    if args.parent_lib:
        exact_put_ab_leg(args, lines)


def exactc_leg(args, lines):
    """Long videos on the exact-rank index (create(..., exact_rank=True, filter_tiles=N, exact_part_overlap=16)), module
    docstring."""
    import bench
    from tvretrieval_amd.ingest import plan_parts
    _, _, _, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3r"]
    nv, nq, ov = args.videos, args.queries, 16
    be = bench.HipBackend(0)
    dev = be.device
    lines += ["## Long videos on the exact-rank index (create(..., exact_rank=True, filter_tiles=N, exact_part_overlap=%d), mode f16s)" % ov]
    for l in (128, 100):
        torch.manual_seed(0)
        model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), ops.F16S)
        full = full_clip_counts(nv)
        cut = torch.clamp(full, max=l)
        n_cut = [int(x) for x in cut.tolist()]
        table = plan_parts(full.numpy(), l, ov)
        n_parts = table.n_parts
        counts = np.diff(table.group_start)
        part_len = torch.from_numpy(table.part_len.astype(np.int64))
        tiles = max(tiles_in_corpus_order([int(x) for x in table.part_len], bench.CHUNK)[0],
                    tiles_in_corpus_order(n_cut, bench.CHUNK)[0])

        def part_batches():
            v0 = 0
            while v0 < nv:
                v1 = min(v0 + bench.CHUNK - 64, nv)
                t = plan_parts(full[v0:v1].numpy(), l, ov)
                r0 = int(table.group_start[v0])
                pieces = list(bench.context_batches(r0, r0 + t.n_parts, l, dv, ds, True, True, dev, lens=part_len))
                yield tuple(torch.cat([p[i] for p in pieces]) for i in range(4)), t
                v0 = v1

        cut_batches = lambda: bench.context_batches(0, nv, l, dv, ds, True, True, dev, lens=cut)      # noqa: E731
        ekw = dict(l_ref=l, exact_rank=True, filter_tiles=tiles)
        with torch.no_grad():
            chained = MutableCorpusIndex.create(model, n_parts, exact_part_overlap=ov, **ekw)
            for batch, t in part_batches():
                chained.add(*batch, parts=t)
            assert chained.n_live == n_parts and chained.n_videos_live == nv
            forms = [("exact_part_overlap=%d, videos of up to %d clips in %d slots" % (ov, int(full.max()), n_parts), chained),
                     ("no keyword, videos cut at %d clips" % l,
                      MutableCorpusIndex.from_batches(model, cut_batches(), n_parts, n_clips=n_cut, **ekw)),
                     ("exact_part_overlap=%d, videos cut at %d clips (no long video)" % (ov, l),
                      MutableCorpusIndex.from_batches(model, cut_batches(), n_parts, n_clips=n_cut, exact_part_overlap=ov, **ekw))]
            qf, qm = bench.synth_queries(nq, dq, dev)
            kw = dict(n_valid_tokens=int(qm.sum().item()))
            kw50 = dict(n_valid_tokens=int(qm[:50].sum().item()))
            passes, small = [[], []], [[], []]
            for rnd in (0, 1):
                for _, index in forms:
                    passes[rnd].append(timed(lambda: inf.vcmr_search(model, index, qf, qm, **kw), args.pass_reps, 2))
                for _, index in forms:
                    small[rnd].append(timed(lambda: inf.vcmr_search(model, index, qf[:50], qm[:50], **kw50), args.reps))
            infos = [inf.vcmr_search(model, index, qf, qm, **kw)["exact"] for _, index in forms]
            folds, lost = [], []
            for (_, index), info in zip(forms, infos):
                if index.chain_head is None:
                    folds.append(None), lost.append(0)
                    continue
                cs, ci = info["cand_scores"], info["cand_indices"]
                folds.append(timed(lambda: ops.cand_best_part(cs, ci, index.chain_head, index.chain_offset), args.reps))
                lost.append(int(((info["cand_folded_indices"] < 0) & (ci >= 0)).sum()))
            cut_lists = [inf.vcmr_search(model, index, qf[:512], qm[:512]) for _, index in forms[1:]]
            same = all(bool(torch.equal(cut_lists[0][k], cut_lists[1][k]))
                       for k in ("top_indices", "top_scores", "flat_indices", "flat_scores"))
        m_c = int(infos[0]["n_candidates"])
        lines += ["", "## l_ref = %d: %d videos with the TVR clip counts (last bin spread up to %d clips), %d of more than %d clips, %d "
                  "parts, hidden %d, ops.F16S model, %d queries, filter_tiles = %d, capacity %d on all three"
                  % (l, nv, int(full.max()), int((counts > 1).sum()), l, n_parts, hidden, nq, tiles, n_parts), "",
                  "First 512 queries on the two indexes that hold the cut corpus (with and without the keyword): %s."
                  % ("bitwise identical lists" if same else "lists NOT identical"), "",
                  "| index | vcmr_search, %d queries | again | 50 queries, eager | again | failing certificates | third-tier queries | "
                  "xml_cand_best_part alone, %d x %d | candidates folded away | hbm_bytes() |" % (nq, nq, m_c),
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for i, (name, index) in enumerate(forms):
            lines.append("| %s | %s | %s | %s | %s | %d | %d | %s | %d | %.3f GB |"
                         % (name, fmt(passes[0][i]), fmt(passes[1][i]), fmt(small[0][i]), fmt(small[1][i]), int(infos[i]["n_fail"]),
                            int(infos[i]["n_full_rows"]), "-" if folds[i] is None else fmt(folds[i], "us"), lost[i],
                            index.hbm_bytes() / 1e9))
        med = [(passes[0][i][0] + passes[1][i][0]) / 2 for i in range(3)]
        lines += ["", "l_ref = %d, medians (mean of both rounds): %.2f ms with chains, %.2f ms cut without the keyword, %.2f ms cut "
                  "with it (%+.2f %% for the long videos, %+.2f %% for the keyword alone); the fold moves %.1f MB in and out, %.1f us "
                  "at the %.1f TB/s stream rate."
                  % (l, med[0], med[1], med[2], (med[0] / med[1] - 1) * 100, (med[2] / med[1] - 1) * 100, 2 * nq * m_c * 8 / 1e6,
                     2 * nq * m_c * 8 / HBM_STREAM * 1e6, HBM_STREAM / 1e12)]
        for ln in lines[-12:]:
            print(ln, flush=True)
        del forms, chained, infos, cut_lists
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="put,putp,e2e,c3,c3r,c3rp")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--videos", type=int, default=21793)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--chains-l", type=int, default=128)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--suite-wall", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:      # the exact leg has a report of its own
        args.out = os.path.join(ROOT, "profiles", {"exact": "index_exact_timing.md", "exactp": "index_exact_packed_run.md",
                                                   "exactc": "index_exact_parts_run.md"}.get(
            args.legs, "index_update_timing.md"))
    if not torch.cuda.is_available():
        sys.exit("bench_index_update.py measures on the GPU; none is visible")
    p = torch.cuda.get_device_properties(0)
    lines = ["# An index that takes updates: what it costs", "",
             "`python tools/bench_index_update.py` on one %s (%d CUs, clock %d MHz as reported by the runtime), torch %s.  Medians of "
             "repeated runs between HIP events after warm-up runs (min .. max); compared versions run in one process, alternating."
             % (p.name, p.multi_processor_count, getattr(p, "clock_rate", 0) // 1000, torch.__version__), ""]
    legs = args.legs.split(",")
    if "put" in legs:
        put_leg(args, lines)
    if "putp" in legs:
        putp_leg(args, lines)
    if "e2e" in legs:
        e2e_leg(args, lines)
    for name in ("c3", "c3r"):
        if name in legs:
            search_leg(name, args, lines)
    if "c3rp" in legs:
        packed_search_leg(args, lines)
    if "compact" in legs:
        compact_leg(args, lines)
    if "chains" in legs:
        chains_leg(args, lines)
    if "exact" in legs:
        exact_leg(args, lines)
    if "exactp" in legs:
        exactp_leg(args, lines)
    if "exactc" in legs:
        exactc_leg(args, lines)
    if args.suite_wall:
        lines += ["", "## GPU test wall time", "", args.suite_wall]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
