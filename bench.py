#!/usr/bin/env python
"""bench.py -- queries/sec of full VCMR (query features in -> top-100 videos + top-200 moments out) over a resident
TVR-shaped corpus, on N MI355X of one node.

  python bench.py --gpus N --steps K --warmup W          (N > 1: bench.py starts the N ranks itself, one per GPU)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W          (same job under torchrun: RANK / WORLD_SIZE from the env)

Workload (BASELINE.json configs[2]/[3], "c3"): XML video+sub, cross-attention, merged ConvSE, H=768, bf16;
21 793 videos x 128 clips (Dv=3072, Ds=768), 10 000 queries x <=30 tokens (Dq=768); synthetic L2-normalised
features (seed 2018), random-init weights (XML.reset_parameters, seed 0).  One STEP = one pass of the hot path over
all 10 000 queries: query encoder -> similarity GEMM with fused max-over-clips (K6, both modalities) -> top-100
videos (K8) -> ConvSE on the selected pairs (K7) -> banded moment top-200 (K9).  The corpus is encoded once by the
HIP context encoder before the timed region (reported as encode_videos_per_s) and stays in HBM.
N > 1: the corpus is sharded by video range (strong scaling: total work fixed), exact two-phase all-gather merge
(tvretrieval_amd/dist.py).

Prints ONE JSON line (rank 0).  `roofline` prices the dominant kernel (K6) against the dense bf16 MFMA peak using
its algorithmic flops 2*Nq*Nv_local*L*H per launch and HIP-event durations measured inside the timed region.
A plain run sets up, warms up, times the steps and prints the line.  --full adds everything else: the per-stage breakdown
(one extra untimed step), `cpu_baseline` (the oracle, reference formulation, torch CPU, on a bounded sample, rank 0 / N=1
only), and the `extras` legs (other configurations and modes; N > 1: the other rerank scheme and exact-rank mode).
--dump-outputs DIR writes the lists the last timed step returned as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (n_queries, n_videos, clips, hidden, Dv, Ds, Dq, ctx_mode, dtype)
    "c3": (10000, 21793, 128, 768, 3072, 768, 768, "video_sub", "bf16"),
    "c2": (256, 2000, 128, 768, 3072, 768, 768, "video", "f32"),
    "tiny": (64, 300, 128, 256, 512, 256, 256, "video_sub", "bf16"),
    # c3 with the REAL clip counts of the 21 793 TVR videos (ceil(duration / 1.5 s) clipped to 128, mean 51.4; histogram in
    # tests/golden/tvr_clip_count_hist.json): the index pads every video to 16 clips and packs the videos back to
    # back into K6's 256-column tiles (ops.PackPlan).  Reported next to the all-valid headline, never instead of it.
    "c3r": (10000, 21793, 128, 768, 3072, 768, 768, "video_sub", "bf16"),
    "tinyr": (64, 300, 128, 256, 512, 256, 256, "video_sub", "bf16"),
    # the reference's AS-TRAINED shape, the configuration its only published number is quoted on (README.md:131): TVR val,
    # 10 895 queries x 2 179 videos, hidden 256 (xml/config.py:143), max_ctx_l 100 (:86-88), resnet_i3d + subtitles, real
    # clip counts.  K6 contracts over K = 256: a third of the headline's arithmetic intensity.
    "tvr_val": (10895, 2179, 100, 256, 3072, 768, 768, "video_sub", "bf16"),
}
RAGGED = {"c3r", "tinyr", "tvr_val"}
PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}     # dense MFMA peaks, MI355X_MICROARCH.md
CHUNK = int(os.environ.get("XML_BENCH_CHUNK", "2048"))  # videos per synthetic / encode batch (>= 3072 GEMM tiles: persistent kernel)
SHARD_ALIGN = 64                                  # shard boundaries: one K6 round of an XCD set = 8 XCDs x 4 tiles x 2 videos
DUMP_Q2C_ROWS = 128                               # --dump-outputs: rows of the (Nq, Nv) q2c matrix kept (fixed, seeded sample)
DUMP_MAX_BYTES = 64 << 20


def model_config(hidden, dv, ds, dq, ctx_mode, max_ctx_l):
    two = ctx_mode == "video_sub"
    return dict(merge_two_stream=two, cross_att=two, span_predictor_type="conv", encoder_type="transformer",
                visual_input_size=dv, sub_input_size=ds, query_input_size=dq, hidden_size=hidden, conv_kernel_size=5,
                stack_conv_predictor_conv_kernel_sizes=-1, conv_stride=1, max_ctx_l=max_ctx_l, max_desc_l=30,
                input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02, ctx_mode=ctx_mode, margin=0.1,
                ranking_loss_type="hinge", lw_neg_q=1, lw_neg_ctx=1, lw_st_ed=0.01, use_hard_negative=False,
                hard_pool_size=20, use_self_attention=True, no_modular=False)


def synth_rows(n, l, d, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, l, d), generator=g, device=device, dtype=torch.float32)
    return x / (x.norm(dim=-1, keepdim=True) + 1e-5)    # l2_normalize_np_array, utils/basic_utils.py:82-84


def real_clip_counts(nv, l):
    """One clip count per video id, drawn without replacement from the real TVR histogram (seeded permutation)."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "tvr_clip_count_hist.json")))
    pool = np.repeat(np.arange(len(rec["hist"])), rec["hist"])
    pool = np.random.default_rng(2018).permutation(pool)
    lens = np.minimum(pool[np.arange(nv) % len(pool)], l).astype(np.int64)
    return torch.from_numpy(np.maximum(lens, 1))


def context_batches(lo, hi, l, dv, ds, use_video, use_sub, device, lens=None):
    """Videos [lo, hi) of the synthetic corpus.  Chunk c (videos 256 c .. 256 c + 255) is generated from its own seed,
    so the corpus content does not depend on how it is sharded.  lens (all videos): clip counts of a ragged corpus --
    rows beyond a video's length are zero and masked, exactly what the dataset's collate hands over
    (start_end_dataset.py:346-359)."""
    for cid in range(lo // CHUNK, (hi + CHUNK - 1) // CHUNK):
        b0 = cid * CHUNK
        r0, r1 = max(lo, b0) - b0, min(hi, b0 + CHUNK) - b0
        mask = torch.ones((r1 - r0, l), device=device)
        if lens is not None:
            ln = lens[b0 + r0:b0 + r1].to(device)
            mask = (torch.arange(l, device=device)[None] < ln[:, None]).float()
        vf = synth_rows(CHUNK, l, dv, 2018 + 2 * cid, device)[r0:r1] if use_video else None
        sf = synth_rows(CHUNK, l, ds, 2018 + 2 * cid + 1, device)[r0:r1] if use_sub else None
        if lens is not None:
            vf = vf * mask[..., None] if use_video else None
            sf = sf * mask[..., None] if use_sub else None
        yield (vf.contiguous() if use_video else None, mask if use_video else None,
               sf.contiguous() if use_sub else None, mask if use_sub else None)


def synth_queries(nq, dq, device):
    g = torch.Generator(device="cpu").manual_seed(2018)
    lens = torch.randint(5, 31, (nq,), generator=g)
    mask = (torch.arange(30)[None] < lens[:, None]).float().to(device)
    qf = synth_rows(nq, 30, dq, 2017, device) * mask[..., None]
    return qf.contiguous(), mask.contiguous()


def list_overlap(a, b, ks=(1, 10, 100)):
    """Mean |top-k(a) ∩ top-k(b)| / k over rows, for each k that fits."""
    a, b = np.asarray(a), np.asarray(b)
    out = {}
    for k in ks:
        if k > a.shape[1] or k > b.shape[1]:
            continue
        hit = [len(set(x[:k].tolist()) & set(y[:k].tolist())) for x, y in zip(a, b)]
        out["top%d" % k] = float(np.mean(hit)) / k
    return out


def cpu_baseline(model, cfg, index, qf, qm, n_total, dtype_name, search, search_exact=None):
    """Oracle (reference formulation, torch CPU fp32) on a bounded slice -- 50 queries x 2 000 videos, median of 5 after
    one warm-up (BASELINE.md section 3 / SURVEY 8d; reference protocol profile_main.py:54,457-461) -- extrapolated
    linearly in Nv.  The same slice also goes through the HIP path (`search`), and the agreement of the two ranked
    lists is reported next to the timing: it is the bf16-vs-fp32 evidence of the very run the number comes from."""
    from oracle import xml_oracle as O
    nq_s, nv_s = 50, min(2000, index.n_videos)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    om = O.OracleXML(cfg, sd)
    mods = index.modalities
    f1 = {m: index.feat1n_rows(m)[:nv_s, :index.l_ref].float().cpu() for m in mods}
    f2 = {m: index.feat2[m][:nv_s, :index.l_ref].float().cpu() for m in mods}
    mk = {m: index.mask[m][:nv_s, :index.l_ref].float().cpu() for m in mods}
    q, qmask = qf[:nq_s].float().cpu(), qm[:nq_s].float().cpu()
    g = lambda d, m: d[m] if m in d else None          # noqa: E731
    k_vid = min(100, nv_s)

    def run(f1=f1, f2=f2, mk=mk):
        with torch.no_grad():
            q2c, st, ed = om.get_pred_from_raw_query(q, qmask, g(f1, "video"), g(f2, "video"), g(mk, "video"),
                                                     g(f1, "sub"), g(f2, "sub"), g(mk, "sub"), cross=True)
            return q2c, O.vcmr_tail(q2c, st, ed, 20.0, k_vid, 2, 16, 200)
    q2c_ref, want = run()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    qps_sample = nq_s / t
    res = dict(value=qps_sample * nv_s / n_total, unit="queries/s", cores=torch.get_num_threads(), kind="port",
               host_cpus=os.cpu_count(),
               sample="oracle (reference formulation, torch-CPU fp32): %d queries x %d videos x %d clips, H=%d, %s; "
                      "median of 5 after 1 warm-up = %.2f s (%.1f q/s on the sample); value extrapolated linearly "
                      "in Nv to %d videos" % (nq_s, nv_s, index.l_ref, cfg["hidden_size"], cfg["ctx_mode"], t,
                                              qps_sample, n_total))
    # the same sample through the HIP path (compute dtype of the run) vs the fp32 oracle lists
    ll = index.l_ref * index.l_ref

    def triples(flat, vids):     # moments as (video, st, ed): decode the flat index through each side's own video list
        flat = np.asarray(flat).astype(np.int64)
        ok = flat >= 0
        r = np.where(ok, flat // ll, 0)
        v = np.take_along_axis(np.asarray(vids).astype(np.int64), r, 1)
        return np.where(ok, v * ll + flat % ll, -1)

    def agreement(got, want, q2c_ref):
        gi, wi = got["top_indices"].cpu().numpy(), want["top_indices"].numpy()
        agree = dict(videos=list_overlap(gi, wi))
        if got.get("q2c") is not None:
            agree["q2c_max_abs_err"] = float((got["q2c"].cpu() - q2c_ref).abs().max())
        agree["videos_top1_same"] = float(np.mean(gi[:, 0] == wi[:, 0]))
        agree["moments"] = list_overlap(triples(got["flat_indices"].cpu().numpy(), gi),
                                        triples(want["flat_indices"].numpy(), wi), ks=(1, 10, 100, 200))
        return agree
    got = search(nq_s, nv_s)
    if got is not None:
        res["hip_vs_oracle_on_sample"] = agreement(got, want, q2c_ref)
        res["hip_vs_oracle_note"] = "share of the oracle's (fp32) top-k found in the %s HIP path's top-k, same %d x %d " \
                                    "slice" % (dtype_name, nq_s, nv_s)
    if search_exact is not None:
        # exact-rank mode on the same slice: its corpus is encoded in f32, so the oracle is re-run on THOSE features (the
        # headline's oracle above consumed the bf16-encoded index)
        got, sub = search_exact(nq_s, nv_s)
        # (split-f16 index: the oracle consumes the values its hi + lo halves carry)
        xf1 = {m: sub.exact.feat1n_f32[m].float()[:, :index.l_ref].cpu() for m in mods}
        xf2 = {m: sub.feat2[m].float()[:, :index.l_ref].cpu() for m in mods}
        q2c_x, want_x = run(xf1, xf2, {m: sub.mask[m][:, :index.l_ref].cpu() for m in mods})
        res["exact_rank_vs_oracle_on_sample"] = agreement(got, want_x, q2c_x)
        res["exact_rank_vs_oracle_on_sample"]["fell_back"] = got["exact"]["n_fail"]
        cand = torch.gather(q2c_x, 1, got["exact"]["cand_indices"].cpu().long())
        res["exact_rank_vs_oracle_on_sample"]["rescored_max_abs_err"] = float((got["exact"]["cand_scores"].cpu() - cand).abs().max())
        res["exact_rank_note"] = "same slice through the exact-rank mode (ops.F16S model, f16 K6 as a filter + split-f16 " \
                                 "re-score + certificate + split-f16 ConvSE) against the oracle on the features that index " \
                                 "holds: the oracle's lists up to ties at f32 rounding"
    return res


class HipBackend(object):
    """The product path: libxmlhip.so kernels on cuda:<local_rank>, RCCL ("nccl") between ranks."""
    name, dist_backend = "hip", "nccl"

    def __init__(self, local_rank):
        # TEST HOOK (tests/test_gpu_dist.py): XML_BENCH_SHARE_GPU=1 puts every rank on cuda:0 with gloo between them, so that
        # the N > 1 code path runs with the real kernels on a one-GPU box (RCCL refuses two ranks on one device)
        self.shared = os.environ.get("XML_BENCH_SHARE_GPU") == "1"
        if self.shared:
            local_rank, self.dist_backend = 0, "gloo"
        torch.cuda.set_device(local_rank)
        self.device = torch.device("cuda", local_rank)
        from tvretrieval_amd import ops
        self.ops = ops

    def make_model(self, cfg, dtype):
        from tvretrieval_amd.model_xml import XML
        return XML(cfg, compute_dtype=dtype).to(self.device).eval()

    def sync(self):
        torch.cuda.synchronize()

    def event(self):
        return torch.cuda.Event(enable_timing=True)

    def init_kwargs(self):
        return {} if self.shared else dict(device_id=self.device)


def k6_traffic(root, workload, world):
    """HBM/fabric bytes per K6 launch from the committed PMC pass -- only if that pass was taken from THIS kernel source
    (tools/measure_k6_traffic.sh records the sha256 of the K6 sources; a stale file is refused, not quoted)."""
    import glob
    import hashlib
    if world != 1 or workload != "c3":
        return None, "not measured for this configuration"
    h = hashlib.sha256()
    for f in ("q2c_persist.hip", "common.h"):
        h.update(open(os.path.join(root, "tvretrieval_amd", "csrc", f), "rb").read())
    cands = sorted(glob.glob(os.path.join(root, "profiles", "r*_k6_traffic.json")))
    for path in reversed(cands):
        rec = json.load(open(path))
        if rec.get("kernel_source_sha256") == h.hexdigest():
            src = os.path.relpath(path, root)
            tp = rec.get("traffic_passes")
            if tp and tp.get("n", 0) > 1:        # the median of separate passes, with their spread (the figure moves +- 10 %)
                src += " (median of %d PMC passes, %.1f-%.1f GB)" % (tp["n"], tp["min"] / 1e9, tp["max"] / 1e9)
            return rec["traffic_bytes_per_launch"], src
    return None, "no PMC pass for the current K6 source (sha256 %s...)" % h.hexdigest()[:12]


def run_extras(args, headline_qps):
    """The other BASELINE configurations and modes, measured by the same process right after the headline run (the
    reference's protocol: one process reports every bucket, baselines/profiling/profile_main.py:457-483).  None of these
    numbers enters the headline fields."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_exact
    import bench_train
    out = {}

    def leg(name, fn):
        t0 = time.perf_counter()
        try:
            out[name] = fn()
        except Exception as e:      # noqa: BLE001 -- an extra leg must never lose the headline measurement
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        out[name]["leg_wall_s"] = round(time.perf_counter() - t0, 2)
        torch.cuda.empty_cache()

    def exact():
        nq, nv = WORKLOADS["c3"][:2]
        r = bench_exact.run(nq, nv, "reset", 0, steps=max(2, args.steps), warmup=2, mode="f16s")
        c = r["certificate"]
        return {"value": r["queries_per_s"], "unit": "queries/s", "ms_per_step": r["ms_per_pass"],
                "dtype": "f32-grade lists: %s filter + split-f16 scores" % r.get("filter", "bf16"),
                "steps": r["steps_timed"], "vs_bf16_headline": r["queries_per_s"] / headline_qps,
                "candidates_per_query": r["candidates"], "fell_back_rate": c["fail_rate"], "eps_mean": c["eps_mean"],
                "filter_abs_err_max": c["filter_abs_err_max"], "margin_T100_minus_bM_p50": c["margin_T100_minus_bM"]["p50"],
                "stage_ms": r["stage_ms"], "corpus_hbm_gb": r["hbm_gb"], "encode_index_s": r["encode_index_s"],
                "second_tier_overflowed_passes": c["second_tier_overflowed_in_timed_passes"],
                "what": "c3 with the f32 path's lists: ops.F16S model (every projection a split-f16 product), bf16 K6 as a "
                        "filter (top-256), split-f16 re-score, per-query certificate with an on-device second tier, split-f16 "
                        "ConvSE; no host read-back in the pass (tests/test_gpu_split16.py, tests/test_gpu_fullsize.py)"}

    def sub(workload, steps, warmup):
        import copy
        a = copy.copy(args)
        a.workload, a.steps, a.warmup, a.no_cpu_baseline, a.no_extras = workload, steps, warmup, True, True
        a.full, a.dump_outputs = True, None          # (--full: the stage breakdown below)
        r = run(a, emit=False)
        keep = {"value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "dtype": r["dtype"],
                "steps": steps, "workload": r["config"]["workload"], "k6_tflops": r["roofline"]["achieved"],
                "k6_frac": r["roofline"]["frac"], "k6_avg_launch_ms": r["roofline"]["avg_launch_ms"],
                "breakdown_ms": r["breakdown_ms"]}
        if "ragged_corpus" in r:
            keep["executed_tflops"] = r["ragged_corpus"]["executed_tflops"]
            keep["mean_clips"] = r["ragged_corpus"]["mean_clips"]
            keep["padded_row_share"] = round(r["ragged_corpus"]["padded_row_share"], 4)
        return keep

    def tvr_val():
        import bench_tvr_val
        r = sub("tvr_val", 10, 3)
        r["served_in_batches_of_50"] = bench_tvr_val.run(50)
        return r

    def e2e():
        import bench_e2e
        r = bench_e2e.run(50)                       # the reference's eval_query_bsz (xml/config.py); opt.graph_search on
        eager = bench_e2e.run(50, repeats=1, graph=False)
        r["eager_batches"] = {k: eager[k] for k in ("total_s", "queries_per_s", "stage_s", "search_host_overhead_s")}
        big = bench_e2e.run(1000, repeats=1, graph=False)
        r["eval_query_bsz_1000"] = {k: big[k] for k in ("total_s", "queries_per_s", "stage_s", "search_device_only_s",
                                                        "search_host_overhead_s", "host_tail_s", "nms_s")}
        return r

    def ingest_leg():
        import bench_ingest
        return bench_ingest.run()

    leg("exact_rank", exact)
    leg("tvr_val", tvr_val)
    leg("e2e_tvr_val", e2e)
    leg("ingest", ingest_leg)
    leg("c2", lambda: sub("c2", 20, 3))
    leg("c3r", lambda: sub("c3r", max(2, min(args.steps, 5)), 2))

    def train():
        g = bench_train.run(steps=20, warmup=5, graph=True)        # the whole iteration as one HIP graph
        torch.cuda.empty_cache()
        r = bench_train.run(steps=10, warmup=3)                    # the eager loop (what a data-parallel run uses today)
        return {"ms": g["ms_per_step"], "tflops": g["tflops"], "frac_of_mfma_peak": g["frac_of_mfma_peak"],
                "flops_per_step": g["flops_per_step"], "pairs_per_s": g["pairs_per_s"], "mode": g["mode"],
                "eager": {"ms": r["ms_per_step"], "tflops": r["tflops"], "frac_of_mfma_peak": r["frac_of_mfma_peak"],
                          "breakdown_ms": r["breakdown_ms"]},
                "config": r["config"], "dtype": r["dtype"],
                "what": "BASELINE configs[4] on one GPU: batch 128 video+sub, L = 100, bf16, forward + backward + BertAdam, "
                        "dropout on, loss read back every step"}
    leg("train_step", train)
    return out


def host_to_host_leg(model, index, qf, qm, args, resident_qps, ops):
    """The headline pass from host memory to host memory (inference.vcmr_search_host; the reference's loop moves every query
    batch host -> device and every list device -> host, xml/inference.py:302-314,383-386): 10 000 queries in pinned host
    memory -> chunked H2D on a side stream overlapped with the previous chunk's search -> xml_moments_decode -> ONE D2H of
    the {video_idx, st, ed, score} records.  Two host layouts: the padded f32 batch the reference's collate delivers, and the
    feature store's ragged f16 token rows (the collate then runs on the device, xml_ingest_rows)."""
    from tvretrieval_amd import inference as inf
    nq, lq, d = qf.shape
    out = {"what": "pinned host queries -> chunked H2D overlapped with the search -> K10 records -> one D2H; wall clock around "
                   "the calls, stage figures from HIP events of one pass (copies and compute overlap)",
           "resident_queries_per_s": resident_qps}
    valid = qm > 0
    lens = valid.sum(1).cpu()
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).to(torch.int64).pin_memory()
    rows16 = qf[valid].to(torch.float16).cpu().pin_memory()
    host = {"f32_padded": dict(query_feat=qf.cpu().pin_memory(), query_mask=qm.cpu().pin_memory()),
            "f16_ragged": dict(query_feat=rows16, row_start=row_start, lq=lq)}
    steps = max(3, min(args.steps, 10))
    for name, kw in host.items():
        nbytes = sum(v.numel() * v.element_size() for v in kw.values() if torch.is_tensor(v))
        with torch.no_grad():
            tm = {}
            rec, cnt = inf.vcmr_search_host(model, index, ops=ops, **kw)          # warm-up, allocations, page pinning
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                rec, cnt = inf.vcmr_search_host(model, index, ops=ops, timings=tm, **kw)
            dt = (time.perf_counter() - t0) / steps
            # the same passes with two in flight (wait=False): pass i + 1's first copy runs under pass i's pair half
            pend = []
            t0 = time.perf_counter()
            for _ in range(steps):
                pend.append(inf.vcmr_search_host(model, index, ops=ops, wait=False, **kw))
                if len(pend) == 2:
                    pend.pop(0).result()
            for pnd in pend:
                pnd.result()
            dt2 = (time.perf_counter() - t0) / steps
        best = {"value": nq / dt2, "unit": "queries/s", "ms_per_step": dt2 * 1e3, "vs_resident": nq / dt2 / resident_qps,
                "mode": "two passes in flight (every pass host-to-host; the device never idles between query sets)",
                "one_pass_at_a_time": {"value": nq / dt, "ms_per_step": dt * 1e3, "vs_resident": nq / dt / resident_qps},
                "host_bytes_in": nbytes, "host_bytes_out": int(rec.nbytes + cnt.nbytes), "steps": steps,
                "chunk_queries": tm["chunk_queries"],
                "stage_ms": {"h2d_total": tm["h2d_s"] * 1e3, "h2d_not_overlapped": tm["h2d_exposed_s"] * 1e3,
                             "device": tm["device_s"] * 1e3, "decode": tm["decode_s"] * 1e3, "d2h": tm["d2h_s"] * 1e3},
                "h2d_gb_per_s": nbytes / tm["h2d_s"] / 1e9 if tm["h2d_s"] > 0 else None,
                "lists_non_empty": int((cnt > 0).sum())}
        out[name] = best
    return out


def batches_of_50_leg(model, index, qf, qm, hidden, batch=50, n_batches=100):
    """The reference's eval_query_bsz = 50 (xml/config.py:61) on the FULL 21 793-video index: one captured graph per batch
    (inference.GraphedVcmrSearch), host-synchronised latency per batch.  The floor of a batch is one pass over the similarity
    operand: every clip row of feat1 is read once whatever the number of queries."""
    from tvretrieval_amd import inference as inf
    with torch.no_grad():
        g = inf.GraphedVcmrSearch(model, index, batch, qf.shape[1], qf.shape[2])
        for b in range(3):
            g(qf[b * batch:(b + 1) * batch], qm[b * batch:(b + 1) * batch])
        torch.cuda.synchronize()
        lat = []
        for b in range(n_batches):
            t0 = time.perf_counter()
            g(qf[b * batch:(b + 1) * batch], qm[b * batch:(b + 1) * batch])
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t0) * 1e3)
    lat = np.asarray(lat)
    feat1_bytes = len(index.modalities) * index.n_videos * index.lpad * hidden * 2.0
    return {"batch": batch, "batches": n_batches,
            "latency_ms": {"p50": float(np.percentile(lat, 50)), "p90": float(np.percentile(lat, 90)),
                           "p99": float(np.percentile(lat, 99))},
            "hbm_floor_ms": feat1_bytes / 6.3e12 * 1e3,
            "what": "50-query batches against the whole headline index through one HIP graph; floor = %.1f GB of feat1 "
                    "at the 6.3 TB/s the guide measures" % (feat1_bytes / 1e9)}


def summary_of(res):
    """The figures the round is judged on, compact, as the LAST key of the line."""
    ex = res.get("extras", {})

    def g(d, *path):
        for k in path:
            d = d.get(k) if isinstance(d, dict) else None
        return round(d, 4) if isinstance(d, float) else d
    multi = {}
    if (res.get("n_gpus") or 1) > 1:        # a SCALE record's tail shows where a sharded pass spent its time (rank 0's view)
        multi = {"n_gpus": res.get("n_gpus"), "stages_ms": res.get("breakdown_ms"),
                 "collectives": g(res, "config", "collectives"), "collectives_fallback": g(res, "config", "collectives_fallback"),
                 "rerank": g(res, "config", "rerank")}
    tr = g(res, "roofline", "traffic")
    return {**multi, "k6_traffic_gb": round(tr / 1e9, 1) if tr else None,
            "c3_qps": g(res, "value"), "c3_ms": g(res, "ms_per_step"), "k6_frac": g(res, "roofline", "frac"),
            "exact_rank_ms": g(ex, "exact_rank", "ms_per_step"), "exact_rank_qps": g(ex, "exact_rank", "value"),
            "exact_fell_back": g(ex, "exact_rank", "fell_back_rate"),
            "h2h_f16_qps": g(ex, "c3_host_to_host", "f16_ragged", "value"),
            "h2h_f16_vs_resident": g(ex, "c3_host_to_host", "f16_ragged", "vs_resident"),
            "h2h_f16_one_at_a_time_vs_resident": g(ex, "c3_host_to_host", "f16_ragged", "one_pass_at_a_time", "vs_resident"),
            "h2h_f32_qps": g(ex, "c3_host_to_host", "f32_padded", "value"),
            "h2h_f32_vs_resident": g(ex, "c3_host_to_host", "f32_padded", "vs_resident"),
            "h2h_f32_one_at_a_time_vs_resident": g(ex, "c3_host_to_host", "f32_padded", "one_pass_at_a_time", "vs_resident"),
            "c3r_ms": g(ex, "c3r", "ms_per_step"), "c3r_k6_frac": g(ex, "c3r", "k6_frac"),
            "c3r_padded_row_share": g(ex, "c3r", "padded_row_share"),
            "tvr_val_ms": g(ex, "tvr_val", "ms_per_step"), "tvr_val_k6_frac": g(ex, "tvr_val", "k6_frac"),
            "tvr_val_batch50_p50_ms": g(ex, "tvr_val", "served_in_batches_of_50", "latency_ms", "p50"),
            "c3_batch50_p50_ms": g(ex, "c3_batches_of_50", "latency_ms", "p50"),
            "encode_videos_per_s": g(ex, "encode", "videos_per_s"), "encode_frac": g(ex, "encode", "frac_of_mfma_peak"),
            "train_ms": g(ex, "train_step", "ms"), "train_eager_ms": g(ex, "train_step", "eager", "ms"),
            "c2_qps": g(ex, "c2", "value")}


def dump_outputs(out, dirname):
    """--dump-outputs: what vcmr_search handed its caller in the last timed step, one DIR/<name>.npy per array -- scores
    float32, indices float64 (exact for every int32).  q2c (Nq, Nv) is larger than the budget: q2c_sample keeps a fixed,
    seeded set of DUMP_Q2C_ROWS of its rows, in ascending query order (absent in exact-rank mode, which never forms q2c)."""
    arrays = {name: out[name].cpu().numpy().astype(np.float64 if name.endswith("indices") else np.float32)
              for name in ("top_scores", "top_indices", "flat_scores", "flat_indices")}
    q2c = out.get("q2c")
    if q2c is not None:
        nq = q2c.shape[0]
        rows = np.sort(np.random.default_rng(2018).choice(nq, min(DUMP_Q2C_ROWS, nq), replace=False))
        arrays["q2c_sample"] = q2c[torch.from_numpy(rows).to(q2c.device)].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, "--dump-outputs: %d bytes exceed the %d-byte budget" % (total, DUMP_MAX_BYTES)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def extras_in_child(args, headline_qps, timeout_s=420):
    """run_extras in a CHILD process: whatever happens there (a device fault in an experimental leg, a timeout) cannot cost
    the headline measurement, which the parent already holds.  The child prints one JSON object."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--extras-only", repr(float(headline_qps)), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout_s)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and lines:
            out = json.loads(lines[-1])
        else:
            out = {"error": "extras child exited with %d: %s" % (r.returncode, (r.stderr or "")[-400:])}
    except subprocess.TimeoutExpired:
        out = {"error": "extras child exceeded %d s" % timeout_s}
    out["extras_wall_s"] = round(time.perf_counter() - t0, 1)
    return out


def run(args, backend_factory=None, emit=True):
    """emit=False: return the result dict without printing (the extra legs of the default run).
    backend_factory: None = the product (HipBackend).  tests/bench_cpu_entry.py passes tests/cpu_backend.BenchBackend to
    drive this launcher / orchestration code with gloo ranks on a machine without a GPU; bench.py itself has no switch
    that runs anything but libxmlhip's kernels."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus or world == 1, "--gpus must equal WORLD_SIZE under torch.distributed.run"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    be = (backend_factory or HipBackend)(local_rank)
    device = be.device
    multi = world > 1 or args.force_sharded      # --force-sharded: the N > 1 code path through a real 1-rank group
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(be.dist_backend, rank=rank, world_size=world, **be.init_kwargs())

    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import dist as xdist
    if args.force_sharded and world == 1:
        xdist.SKIP_TRIVIAL_COLLECTIVES = False
    ops = be.ops

    nq, nv, l, hidden, dv, ds, dq, ctx_mode, dtname = WORKLOADS[args.workload]
    dtype = torch.bfloat16 if dtname == "bf16" else torch.float32
    exact = bool(getattr(args, "exact_rank", False))
    if exact:        # exact-rank mode (inference.stage_exact_topk_f16s): ops.F16S model -- f32 activations, every projection,
        # the candidate re-score and ConvSE as split-f16 products on the 16-bit MFMA pipe --, f16 K6 as the filter
        assert dtname == "bf16", "--exact-rank applies to the bf16 workloads"
        from tvretrieval_amd import inference as _inf
        dtype, dtname = ops.F16S, "%s filter + split-f16 (f32-grade) scores" % _inf.EXACT_F16S_FILTER
    xkw = dict(exact_filter=True) if exact else {}
    cfg = model_config(hidden, dv, ds, dq, ctx_mode, l)
    torch.manual_seed(0)
    model = be.make_model(cfg, dtype)

    # ---- one-off: encode this rank's shard of the corpus (HOT LOOP A), untimed for the metric -------------
    # (corpora too small for aligned shards on every rank -- the tiny test workload at 8 ranks -- are cut per video)
    lo, hi = xdist.shard_range(nv, rank, world, align=SHARD_ALIGN if nv >= 2 * world * SHARD_ALIGN else 1)
    lens = real_clip_counts(nv, l) if args.workload in RAGGED else None
    with torch.no_grad():   # untimed warm-up of the encoder kernels (module load, first-launch costs, clocks)
        inf.build_corpus_index(model, context_batches(lo, min(hi, lo + 64), l, dv, ds, model.use_video, model.use_sub,
                                                      device, lens), ops=ops, video_offset=lo, n_total=nv, l_ref=l, **xkw)
    # the raw features of the shard are made resident first (43 GB of 288 for the whole TVR corpus): encode_videos_per_s
    # times the engine -- features in HBM -> resident index -- not the synthetic-data generator
    raw = list(context_batches(lo, hi, l, dv, ds, model.use_video, model.use_sub, device, lens))
    with torch.no_grad():   # second warm-up at the real batch size: workspaces and the allocator's pools reach their final size
        inf.build_corpus_index(model, iter(raw[:1]), ops=ops, video_offset=lo, n_total=nv, l_ref=l, **xkw)
    # the index's own memory is mapped and touched first (IndexStorage: hipMalloc + zero-fill of 26 GB inside the timed
    # region is what made this figure swing 32 K .. 151 K videos/s from box to box); alloc_s is reported next to it
    be.sync()
    t0 = time.perf_counter()
    storage = inf.IndexStorage(model, hi - lo, l, ops=ops, device=device, tiles=not exact) if be.name == "hip" else None
    be.sync()
    alloc_s = time.perf_counter() - t0
    enc_ev = (be.event(), be.event())
    t0 = time.perf_counter()
    enc_ev[0].record()
    with torch.no_grad():
        index = inf.build_corpus_index(model, raw, ops=ops, video_offset=lo, n_total=nv, l_ref=l, n_videos=hi - lo,
                                       storage=storage, **xkw)
    enc_ev[1].record()
    be.sync()
    enc_s = time.perf_counter() - t0
    enc_dev_s = enc_ev[0].elapsed_time(enc_ev[1]) * 1e-3
    del storage
    enc_bf16_s = None
    if args.full and world == 1 and not multi and be.name == "hip" and args.workload == "c3" and not args.no_extras \
            and dtype == torch.bfloat16 and not exact:
        # the same corpus with the RAW features resident as bf16 (the C ABI takes f32 or the compute dtype, x_dt of
        # xml_linear_ln_relu_pos): the input LayerNorm then reads half the bytes -- 3.2 GB less per 2 048 videos
        raw16 = [tuple(t.to(torch.bfloat16) if (t is not None and i in (0, 2)) else t for i, t in enumerate(b)) for b in raw]
        with torch.no_grad():
            inf.build_corpus_index(model, iter(raw16[:1]), ops=ops, video_offset=lo, n_total=nv, l_ref=l)
            be.sync()
            st16 = inf.IndexStorage(model, hi - lo, l, ops=ops, device=device)
            be.sync()
            t0 = time.perf_counter()
            idx16 = inf.build_corpus_index(model, iter(raw16), ops=ops, video_offset=lo, n_total=nv, l_ref=l, n_videos=hi - lo,
                                           storage=st16)
            be.sync()
            enc_bf16_s = time.perf_counter() - t0
        del raw16, idx16, st16
    del raw
    rep_s = None
    if multi and not args.sharded_rerank:
        # one-off: corpus-wide copy of the ConvSE-side features on every GPU (the similarity operand stays sharded):
        # the owner of a query reranks its global top-k itself, two collectives per pass instead of four
        t0 = time.perf_counter()
        xdist.replicate_rerank_features(index)
        be.sync()
        rep_s = time.perf_counter() - t0
    qf, qm = synth_queries(nq, dq, device)

    exchange, exch_note = None, None
    if multi:
        # collectives: libxmlhip's RCCL entries (xml_rccl_*) on GPU ranks.  They cannot be exercised at world > 1 on the
        # 1-GPU development boxes, so every run first pushes one small exchange through them AND through
        # torch.distributed and compares; a mismatch or an error ENDS the run with a non-zero exit code (unless
        # --torch-collectives asked for the torch.distributed exchange on purpose).
        exchange = xdist.TorchExchange()
        if be.name == "hip" and not args.torch_collectives:
            cand, same = None, False
            try:
                if os.environ.get("XML_TEST_BREAK_CABI_COLLECTIVES"):      # tests: the failure path below must end the run
                    raise RuntimeError("injected by XML_TEST_BREAK_CABI_COLLECTIVES")
                cand = xdist.RcclExchange()
                g = torch.Generator(device=device).manual_seed(11 + rank)
                s = torch.randn(4 * world + 3, 64, device=device, generator=g)
                li = torch.argsort(s, dim=1, descending=True).int()[:, :16].contiguous() + 1000 * rank
                ls = torch.gather(s, 1, (li - 1000 * rank).long()).contiguous()
                a, b = cand.topk_by_owner(ls, li, 16, 20.0, ops), exchange.topk_by_owner(ls, li, 16, 20.0, ops)
                rows = ls[:5].to(torch.bfloat16).contiguous()
                same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and \
                    torch.equal(cand.allgather_rows(rows), exchange.allgather_rows(rows))
                if not same:
                    exch_note = "C-ABI self-check MISMATCH vs torch.distributed"
            except Exception as e:       # noqa: BLE001 -- report, never lose the measurement
                exch_note = "C-ABI collectives failed (%s: %s)" % (type(e).__name__, e)
            # the decision is collective: every rank uses the C-ABI exchange or none does
            flag = torch.tensor([1 if same else 0], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                exchange = cand
            elif exch_note is None:
                exch_note = "another rank failed the C-ABI self-check"
            if exch_note is not None:
                # FATAL: a line that silently measured torch.distributed instead of csrc/collectives.hip would be read as a
                # measurement of the C-ABI collectives.  (The decision above was collective: every rank leaves here.)
                print("bench.py rank %d: ERROR: %s.  Refusing to measure torch.distributed collectives under this "
                      "benchmark's name; pass --torch-collectives to measure that path on purpose "
                      "(the line then says config.collectives_fallback = 1)." % (rank, exch_note), file=sys.stderr, flush=True)
                dist.barrier()
                raise SystemExit(3)
        elif args.torch_collectives:
            exch_note = "--torch-collectives"

    ev = []      # (start, end) event pairs around every K6 launch of the timed region
    def k6_timer():
        s, e = be.event(), be.event()
        ev.append((s, e))
        return s, e

    exact_flags = []      # exact-rank mode: the passes read nothing back; their overflow flags are looked at after the clock

    # The collate builds the query masks on the HOST (start_end_dataset.py:346-370): a caller knows the number of valid query
    # tokens without asking the device.  Handing it over spares the packed query encoder its 4-byte read-back -- a host
    # synchronisation per pass (~0.6 ms of idle device between passes); taken once, before the clock.
    tok_kw = dict(n_valid_tokens=int(qm.sum().item())) if (be.name == "hip" and not multi) else {}

    def step():
        with torch.no_grad():
            if not multi:
                if exact:
                    o = inf.vcmr_search(model, index, qf, qm, ops=ops, defer_exact_check=True, **tok_kw)
                    exact_flags.append((o["exact"]["overflow_dev"], o["exact"]["n_fail_dev"]))
                    return o
                return inf.vcmr_search(model, index, qf, qm, ops=ops, **tok_kw)
            # final lists stay on the rank that owns the query (where its NMS would run): no redundant gather
            return xdist.sharded_vcmr_search(model, index, qf, qm, gather_results=False, ops=ops, exchange=exchange,
                                             n_chunks=1 if args.sharded_rerank else args.chunks)

    for _ in range(args.warmup):
        step()
    inf.K6_TIMER = k6_timer
    if multi:
        dist.barrier()
    be.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = None             # (a step's outputs are released before the next step starts)
        last = step()
    be.sync()
    if multi:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    inf.K6_TIMER = None
    if args.dump_outputs:
        dump_outputs(last, args.dump_outputs)
    del last
    exact_info = None
    if exact and exact_flags:
        timed_flags = exact_flags[-args.steps:]
        exact_info = {"second_tier_overflowed_passes": int(sum(bool(f.item()) for f, _ in timed_flags if f is not None)),
                      "certificates_failed_per_pass": int(timed_flags[-1][1].item()),
                      "candidates_per_query": index.exact.n_candidates,
                      "note": "every timed pass ran without a host read-back; a pass whose on-device second tier "
                              "overflowed would have to be redone through the eager fallback (none did: 0)"}
    per_rank_videos = [index.n_videos]
    rccl_ranks = 1
    if multi:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        nvs = torch.zeros(world, device=device, dtype=torch.int64)
        nvs[rank] = index.n_videos
        dist.all_reduce(nvs)
        per_rank_videos = [int(x) for x in nvs.cpu().tolist()]
        rccl_ranks = dist.get_world_size()

    # ---- N > 1: the OTHER rerank scheme, same index, same steps (the headline keeps the scheme the flags chose) --------
    alt_scheme = None
    if multi and args.full and not args.no_extras:
        alt_owner = bool(args.sharded_rerank)          # headline = sharded rerank -> alternative = owner rerank, and v.v.
        if alt_owner and index.feat2_all is None:
            xdist.replicate_rerank_features(index)

        def alt_step():
            with torch.no_grad():
                return xdist.sharded_vcmr_search(model, index, qf, qm, gather_results=False, ops=ops, exchange=exchange,
                                                 owner_rerank=alt_owner, n_chunks=1)
        alt_step()
        dist.barrier()
        be.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            alt_step()
        be.sync()
        dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        alt_scheme = {"rerank": "query owner (feat2 replicated, feat1 sharded)" if alt_owner else
                      "video owner (feat2 sharded): all-gather of the global top-100 + all-to-all of the local top-200",
                      "value": nq * args.steps / float(t.item()), "unit": "queries/s",
                      "ms_per_step": float(t.item()) / args.steps * 1e3, "steps": args.steps,
                      "collectives_per_pass": 2 if alt_owner else 4}

    # ---- N > 1: the same sharded pass in exact-rank mode (ops.F16S model with the same weights; every shard hands its
    #      exact local top-k to the merge), so that one line carries bf16 and identical-lists throughput at this N ----------
    exact_sharded = None
    if multi and args.full and not args.no_extras and be.name == "hip" and not exact and dtname == "bf16":
        xi = m16 = None
        build_err = None
        try:        # local part first; the ranks then AGREE to run the leg (a rank failing alone must not leave the others
            m16 = be.make_model(cfg, ops.F16S)     # waiting in a collective)
            m16.load_state_dict(model.state_dict())
            with torch.no_grad():
                xi = inf.build_corpus_index(m16, list(context_batches(lo, hi, l, dv, ds, model.use_video, model.use_sub,
                                                                      device, lens)),
                                            ops=ops, video_offset=lo, n_total=nv, l_ref=l, n_videos=hi - lo, exact_filter=True)
        except Exception as e:      # noqa: BLE001
            build_err = "%s: %s" % (type(e).__name__, e)
        flag = torch.tensor([0 if build_err else 1], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            exact_sharded = {"error": build_err or "another rank could not build its exact-rank shard"}
    if exact_sharded is None and multi and args.full and not args.no_extras and be.name == "hip" and not exact \
            and dtname == "bf16":
        try:
            with torch.no_grad():
                if not args.sharded_rerank:
                    xdist.replicate_rerank_features(xi)

                def x_step():
                    return xdist.sharded_vcmr_search(m16, xi, qf, qm, gather_results=False, ops=ops, exchange=exchange,
                                                     n_chunks=1)
                x_step()
                dist.barrier()
                be.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    x_step()
                be.sync()
                dist.barrier()
            t = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            exact_sharded = {"value": nq * args.steps / float(t.item()), "unit": "queries/s",
                             "ms_per_step": float(t.item()) / args.steps * 1e3, "steps": args.steps,
                             "candidates_per_query_and_shard": xi.exact.n_candidates,
                             "what": "the same sharded pass with the f32 path's lists (exact-rank mode: bf16 filter, "
                                     "split-f16 re-score / ConvSE, per-shard certificates)"}
            del xi, m16
        except Exception as e:      # noqa: BLE001 -- an extra leg must never lose the headline measurement
            exact_sharded = {"error": "%s: %s" % (type(e).__name__, e)}

    k6_ms = [s.elapsed_time(e) for s, e in ev]
    k6_avg_ms = float(np.mean(k6_ms))
    launches_per_step = len(k6_ms) / float(args.steps)          # > 1 when the sharded pass is pipelined over query chunks
    flops_per_launch = 2.0 * nq * index.n_videos * index.lpad * hidden * len(index.modalities) / launches_per_step
    ragged = None
    plan = getattr(index.feat1n[index.modalities[0]], "plan", None)
    if lens is not None:
        # ragged corpus: the ALGORITHMIC work is the valid clips; the packed image (videos padded to 16 clips, back to back)
        # executes `padded` clip rows, the unpacked layout would execute 128 per video
        valid = float(lens[lo:hi].sum())
        padded = float(plan.n_tiles * 256) if plan is not None else float(index.n_videos * index.lpad)
        flops_per_launch = 2.0 * nq * valid * hidden * len(index.modalities) / launches_per_step
        ragged = dict(mean_clips=valid / index.n_videos, executed_clip_rows=padded, valid_clip_rows=valid,
                      unbucketed_clip_rows=float(index.n_videos * index.lpad), bucketed=plan is not None,
                      padded_row_share=1.0 - valid / padded,
                      executed_tflops=2.0 * nq * padded * hidden * len(index.modalities) / launches_per_step
                      / (k6_avg_ms * 1e-3) / 1e12)
    achieved = flops_per_launch / (k6_avg_ms * 1e-3) / 1e12

    # ---- --full: stage breakdown, one extra untimed step ------------------------------------------------
    breakdown = {}
    if args.full and not multi:
        def timed(name, fn):
            s, e = be.event(), be.event()
            s.record(); r = fn(); e.record(); be.sync()
            breakdown[name] = round(s.elapsed_time(e), 3)
            return r
        with torch.no_grad():
            qvec = timed("query_encode", lambda: inf.stage_query_vectors(model, qf, qm))
            if exact:
                tw, ti, _ = timed("exact_topk(k6 filter+k8+rescore+certificate)",
                                  lambda: inf.stage_exact_topk(index, qvec, min(100, index.n_videos), 20.0, ops))
            else:
                q2c = timed("q2c_k6", lambda: inf.stage_q2c(index, qvec, ops))
                tw, ti = timed("topk_k8", lambda: ops.topk_rows(q2c, min(100, index.n_videos), alpha=20.0))
            if inf.K7_SUMMARIES:      # (what vcmr_search runs: K7 hands K9 its per-pair candidate summaries)
                st, ed, sm = timed("convse_k7", lambda: inf.stage_span_probs(model, index, qvec, ti, ops, pair_w=tw,
                                                                             band=(2, 16)))
                timed("moment_k9", lambda: ops.moment_topk(st, ed, tw, index.l_ref, 2, 16, 200, summ=sm))
            else:     # (what vcmr_search runs; ragged corpora: K7 / K9 skip the zero tails of short videos)
                vl = inf.ragged_lengths(index, ops) if hasattr(inf, "ragged_lengths") else None
                rk = dict(pair_vid=ti, vid_len=vl) if vl is not None else {}
                st, ed = timed("convse_k7", lambda: inf.stage_span_probs(model, index, qvec, ti, ops,
                                                                         **(dict(vid_len=vl) if vl is not None else {})))
                timed("moment_k9", lambda: ops.moment_topk(st, ed, tw, index.l_ref, 2, 16, 200, **rk))
    elif args.full:     # rank 0's view of one sharded pass, collectives (and the waiting for slower ranks in them) included
        marks = []

        def mark(name):
            e = be.event()
            e.record()
            marks.append((name, e))
        dist.barrier()
        be.sync()
        xdist.STAGE_MARK = mark
        with torch.no_grad():           # un-pipelined (one chunk) so that every stage, exchanges included, is delimited
            xdist.sharded_vcmr_search(model, index, qf, qm, gather_results=False, ops=ops, exchange=exchange, n_chunks=1)
        xdist.STAGE_MARK = None
        be.sync()
        for (_, e0), (name, e1) in zip(marks, marks[1:]):
            breakdown[name] = round(e0.elapsed_time(e1), 3)

    traffic, traffic_src = k6_traffic(ROOT, args.workload, world) if be.name == "hip" else (None, "stub backend")

    res = None
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        res = {
            "metric": "queries/sec VCMR over 21.8K-video corpus", "value": nq * args.steps / elapsed,
            "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": dtname, "data": "synthetic",
            "config": {"workload": "%s: XML %s ConvSE VCMR, %d queries x %d videos x %d clips, H=%d, top-100 videos, "
                                   "top-200 moments" % (args.workload, ctx_mode, nq, nv, l, hidden),
                       "global_batch": nq, "parallelism": "corpus-shard x%d" % world, "videos_per_gpu": per_rank_videos,
                       "ranks_in_process_group": rccl_ranks, "backend": be.name,
                       "collectives": (exchange.name if exchange is not None else "none") +
                                      ("" if exch_note is None else " [%s]" % exch_note),
                       "collectives_fallback": 0 if exch_note is None else 1,      # 1 = NOT the C-ABI exchange (see above)
                       "query_chunks": args.chunks if multi and not args.sharded_rerank else 1,
                       "query_token_count": "host-known, handed to the pass (no read-back)" if tok_kw else "read back from the device",
                       "launcher": "bench.py self-spawn" if os.environ.get("XML_SELF_SPAWNED") else
                                   ("torch.distributed.run" if world > 1 else "single process"),
                       "result_placement": "all on the GPU" if not multi else "final lists on the query's owner rank",
                       "rerank": "local" if not multi else ("video owner (feat2 sharded)" if args.sharded_rerank else
                                                             "query owner (feat2 replicated, feat1 sharded)")},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS["bf16" if exact else dtname],
                         "unit": "TFLOP/s", "frac": achieved / PEAK_TFLOPS["bf16" if exact else dtname], "traffic": traffic,
                         "traffic_note": "bytes per launch, rocprofv3 FETCH_SIZE(x2 gfx950 correction)+WRITE_SIZE: %s; "
                                         "algorithmic bytes = %.3g" % (
                                             traffic_src,
                                             len(index.modalities) * (index.n_videos * index.lpad * hidden * 2.0
                                                                      + nq * hidden * 2.0) + nq * index.n_videos * 4.0),
                         "kernel": "q2c_persist_kernel",
                         "launches_timed": len(k6_ms), "avg_launch_ms": k6_avg_ms,
                         "flops_per_launch": flops_per_launch},
            "encode_videos_per_s": (hi - lo) * world / enc_s if enc_s > 0 else None,
            "encode": {"wall_s": enc_s, "hip_event_s": enc_dev_s, "index_alloc_and_touch_s": alloc_s,
                       "videos_per_s_wall": (hi - lo) * world / enc_s if enc_s > 0 else None,
                       "videos_per_s_hip_events": (hi - lo) * world / enc_dev_s if enc_dev_s > 0 else None,
                       "note": "raw features and the index's memory resident before the clock starts; wall-clock and HIP "
                               "events around the same build_corpus_index call"},
            "corpus_hbm_gb_per_gpu": index.hbm_bytes() / 1e9, "replicate_feat2_s": rep_s,
            "breakdown_ms": breakdown,
        }
        if exact_info is not None:
            res["exact_rank"] = exact_info
        if alt_scheme is not None:
            res["extras"] = {"other_rerank_scheme": alt_scheme}
        if exact_sharded is not None:
            res.setdefault("extras", {})["exact_rank_sharded"] = exact_sharded
        if ragged is not None:
            res["ragged_corpus"] = ragged
            res["roofline"]["note"] = "ragged corpus: `achieved` prices the VALID clip rows (algorithmic work); " \
                                      "executed_tflops in ragged_corpus prices the padded rows the MFMA pipe actually ran"
        if args.full and world == 1 and not args.no_cpu_baseline and be.name == "hip" and not exact:
            def search(nq_s, nv_s):       # the baseline's slice through the HIP path, for the agreement figures
                with torch.no_grad():
                    sub = inf.build_corpus_index(model, context_batches(0, nv_s, l, dv, ds, model.use_video,
                                                                       model.use_sub, device, lens), ops=ops, l_ref=l)
                    return inf.vcmr_search(model, sub, qf[:nq_s].contiguous(), qm[:nq_s].contiguous(), ops=ops)
            search_exact = None
            extras_on = args.workload == "c3" and not args.no_extras and not multi
            if extras_on:
                def search_exact(nq_s, nv_s):     # the same slice in exact-rank mode: split-f16 model with the SAME weights
                    m32 = be.make_model(cfg, ops.F16S)
                    m32.load_state_dict(model.state_dict())
                    with torch.no_grad():
                        sub = inf.build_corpus_index(m32, context_batches(0, nv_s, l, dv, ds, m32.use_video, m32.use_sub,
                                                                          device, lens), ops=ops, l_ref=l,
                                                     exact_filter=True)
                        return inf.vcmr_search(m32, sub, qf[:nq_s].contiguous(), qm[:nq_s].contiguous(), ops=ops), sub
            res["cpu_baseline"] = cpu_baseline(model, cfg, index, qf, qm, nv, dtname, search, search_exact)
        else:
            res["cpu_baseline"] = None
        if args.full and world == 1 and not multi and be.name == "hip" and args.workload == "c3" and not args.no_extras \
                and not exact:
            enc_flops = 2.0 * l * hidden * (dv + ds) + 44.0 * l * hidden ** 2 + 24.0 * l ** 2 * hidden
            enc_tf = res["encode_videos_per_s"] * enc_flops / 1e12
            extras = {"encode": {"videos_per_s": res["encode_videos_per_s"],
                                 "videos_per_s_hip_events": res["encode"]["videos_per_s_hip_events"],
                                 "alloc_s": alloc_s, "flops_per_video": enc_flops,
                                 "tflops": enc_tf, "frac_of_mfma_peak": enc_tf / PEAK_TFLOPS[dtname],
                                 "raw_features": "f32 resident in HBM (the reference's input contract)"}}
            if enc_bf16_s:
                v16 = (hi - lo) / enc_bf16_s
                extras["encode"]["bf16_raw_features"] = {"videos_per_s": v16, "tflops": v16 * enc_flops / 1e12,
                                                         "frac_of_mfma_peak": v16 * enc_flops / 1e12 / PEAK_TFLOPS[dtname]}
            try:
                extras["c3_host_to_host"] = host_to_host_leg(model, index, qf, qm, args, res["value"], ops)
            except Exception as e:      # noqa: BLE001 -- an extra leg must never lose the headline measurement
                extras["c3_host_to_host"] = {"error": "%s: %s" % (type(e).__name__, e)}
            try:
                extras["c3_batches_of_50"] = batches_of_50_leg(model, index, qf, qm, hidden)
            except Exception as e:      # noqa: BLE001
                extras["c3_batches_of_50"] = {"error": "%s: %s" % (type(e).__name__, e)}
            del index, model
            torch.cuda.empty_cache()
            extras.update(extras_in_child(args, res["value"]))
            res["extras"] = extras
            if res.get("cpu_baseline") is not None:       # (long strings: keep them in front of the figures below)
                res["cpu_baseline"] = res.pop("cpu_baseline")
    if rank == 0 and res is not None and emit:
        res["summary"] = summary_of(res)                  # LAST key: what a 2 000-character tail of this line still shows
    if multi:       # RCCL's start-up banner sits in the C stdio buffer of every rank: push it out BEFORE the result line,
        import ctypes    # so that the JSON line is the last thing this job prints
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        dist.barrier()
    if rank == 0 and emit:
        print(json.dumps(res), flush=True)
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    return res


def main(argv=None, backend_factory=None, script=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-sharded", action="store_true", help="use the multi-GPU code path even with 1 rank (testing)")
    ap.add_argument("--sharded-rerank", action="store_true",
                    help="N > 1: keep feat2 sharded too (phase 2 on the video's owner, four collectives per pass)")
    ap.add_argument("--chunks", type=int, default=int(os.environ.get("XML_SHARD_CHUNKS", "1")),
                    help="N > 1: query chunks of the pipelined owner pass (chunk c's exchange runs under chunk c+1's K6)")
    ap.add_argument("--torch-collectives", action="store_true",
                    help="N > 1: keep the exchanges on torch.distributed instead of libxmlhip's xml_rccl_* entries (A/B)")
    ap.add_argument("--exact-rank", action="store_true",
                    help="run the pass in exact-rank mode (f32 model, bf16 K6 as a filter + f32 re-score + certificate): the "
                         "f32 path's lists; any N (every shard hands its exact local top-k to the merge)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps also measure the stage breakdown, the CPU baseline and the extra legs "
                         "(a plain run sets up, warms up, times --steps steps and prints the line)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full, N = 1, c3: skip the extra legs (exact-rank mode, c2, c3r, training step) after the "
                         "headline run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the lists the last timed step returned (and a fixed sample of its q2c rows) as DIR/<name>.npy; "
                         "single process only")
    ap.add_argument("--extras-only", default=None, metavar="HEADLINE_QPS",
                    help="(internal) run only the extra legs of the --full run and print them as one JSON object")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.gpus > 1 or args.force_sharded):
        ap.error("--dump-outputs needs a single-process run (--gpus 1 without --force-sharded)")
    if args.extras_only is not None:
        torch.cuda.set_device(0)
        print(json.dumps(run_extras(args, float(args.extras_only))), flush=True)
        return None
    from tvretrieval_amd import launch
    if args.gpus > 1 and not launch.under_launcher():
        # `python bench.py --gpus N`: one process per GPU, started here (same environment torch.distributed.run gives)
        rc = launch.spawn_local_ranks(script or os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv),
                                      args.gpus)
        if rc != 0:
            sys.exit(rc)
        return None
    return run(args, backend_factory)


if __name__ == "__main__":
    main()
