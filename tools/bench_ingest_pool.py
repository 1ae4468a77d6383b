"""Ingest from frame- and word-level stores (xml_ingest_pool_rows, ingest.PooledStore), measured two ways; one JSON line.

kernel   2 048 videos x 128 clips, operands resident in HBM, xml_ingest_pool_rows and xml_ingest_rows interleaved in one
         process after a warm-up, HIP events around each launch, median and min..max over the rounds:
           video  ResNet 2048 + I3D 1024 f16 frame rows, 4-5 per clip (ingest.frame_clip_boundaries), max pooling, both
                  per-source norms and the row norm -> (2048, 128, 3072)
           sub    768-wide f16 word rows with subtitle-like ranges (ingest.sentence_word_ranges: sentences of 0-13 words every
                  ~3.5 s, clips without words, words shared by neighbouring clips), max pooling, the row norm -> (2048, 128, 768)
         next to xml_ingest_rows writing the same output shape from PRE-POOLED f16 clip rows.  Bytes: every source row once
         per clip that names it + the output; GB/s = bytes / median time.
feeder   the same corpus shape on disk as frame / word stores and as clip stores (pooled on the host once, outside the
         timing): ContextFeeder -> inference.build_corpus_index, wall-clock videos/s after a two-batch warm-up, the way
         tools/bench_ingest.py measures the clip-store path.
usage: python tools/bench_ingest_pool.py [n_videos_kernel [n_videos_feeder [rounds]]]"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, D_RES, D_I3D, D_SUB = 128, 2048, 1024, 768


def word_ranges(rng, n_patterns=64):
    """(n_patterns, L, 2) word ranges of videos of L clips and their word counts: sentences every ~3.5 s, 0.5-4 s long."""
    from tvretrieval_amd.ingest import sentence_word_ranges
    out, n_words = [], []
    for _ in range(n_patterns):
        dur = L * 1.5
        st = np.sort(rng.uniform(0, dur, int(dur / 3.5)))
        lens = rng.integers(0, 14, len(st))
        out.append(sentence_word_ranges(np.stack([st, st + rng.uniform(0.5, 4.0, len(st))], 1), lens, L))
        n_words.append(int(lens.sum()))
    return np.stack(out), np.array(n_words)


def time_interleaved(fns, rounds, warmup=3):
    """fns: name -> callable; every round runs each once, in turn -> name -> sorted microseconds"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return {k: sorted(v) for k, v in us.items()}


def kernel_leg(nv, rounds):
    from tvretrieval_amd import ops
    from tvretrieval_amd.ingest import frame_clip_boundaries
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(3)
    b = frame_clip_boundaries()[:L + 1].astype(np.int64)
    per_video = int(b[-1])                                                   # 576 frames
    start = torch.arange(0, (nv + 1) * L, L, dtype=torch.int64, device=dev)
    seg_v = (np.stack([b[:-1], b[1:]], 1)[None] + (np.arange(nv) * per_video)[:, None, None]).reshape(-1, 2)
    rng = np.random.default_rng(4)
    pat, n_words = word_ranges(rng)
    pick = rng.integers(0, len(pat), nv)
    off = np.concatenate([[0], np.cumsum(n_words[pick])])
    seg_s = np.where((pat[pick][..., 1] > pat[pick][..., 0])[..., None], pat[pick] + off[:-1, None, None], 0).reshape(-1, 2)
    res = (torch.randn((nv * per_video, D_RES), generator=g, device=dev).abs() * 0.5).half()
    i3d = (torch.randn((nv * per_video, D_I3D), generator=g, device=dev).abs() * 0.5).half()
    words = (torch.randn((int(off[-1]), D_SUB), generator=g, device=dev) * 0.5).half()
    clip_v = (torch.randn((nv * L, D_RES + D_I3D), generator=g, device=dev).abs() * 0.5).half()
    clip_s = (torch.randn((nv * L, D_SUB), generator=g, device=dev) * 0.5).half()
    dseg_v, dseg_s = torch.from_numpy(seg_v).to(dev), torch.from_numpy(seg_s).to(dev)
    out = {}
    for tag, odt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
        fns = {
            "video_pool": lambda: ops.ingest_pool_rows([(res, dseg_v, True), (i3d, dseg_v, True)], start, nv, L, L, out_dtype=odt),
            "video_rows": lambda: ops.ingest_rows(clip_v, start, nv, L, L, out_dtype=odt),
            "sub_pool": lambda: ops.ingest_pool_rows([(words, dseg_s, False)], start, nv, L, L, out_dtype=odt),
            "sub_rows": lambda: ops.ingest_rows(clip_s, start, nv, L, L, out_dtype=odt),
        }
        us = time_interleaved(fns, rounds)
        n_out = nv * L
        rd = {"video_pool": int((seg_v[:, 1] - seg_v[:, 0]).sum()) * (D_RES + D_I3D) * 2, "video_rows": n_out * (D_RES + D_I3D) * 2,
              "sub_pool": int((seg_s[:, 1] - seg_s[:, 0]).sum()) * D_SUB * 2, "sub_rows": n_out * D_SUB * 2}
        wr = {"video": n_out * (D_RES + D_I3D) * es, "sub": n_out * D_SUB * es}
        leg = {}
        for k, v in us.items():
            bytes_ = rd[k] + wr[k.split("_")[0]]
            med = statistics.median(v)
            leg[k] = {"us_median": round(med, 1), "us_min": round(v[0], 1), "us_max": round(v[-1], 1), "gb": round(bytes_ / 1e9, 3),
                      "gb_per_s": round(bytes_ / 1e3 / med, 1)}
        for s in ("video", "sub"):
            leg[s + "_bytes_per_s_ratio_pool_over_rows"] = round(leg[s + "_pool"]["gb_per_s"] / leg[s + "_rows"]["gb_per_s"], 3)
        out[tag] = leg
    out["words_per_filled_clip"] = round(float((seg_s[:, 1] - seg_s[:, 0]).sum() / max((seg_s[:, 1] > seg_s[:, 0]).sum(), 1)), 2)
    out["clips_without_words"] = round(float((seg_s[:, 1] == seg_s[:, 0]).mean()), 3)
    return out


def feeder_leg(nv, batch=512):
    import bench
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ingest, ops
    from tvretrieval_amd.model_xml import XML
    dev = torch.device("cuda", torch.cuda.current_device())
    root = os.environ.get("XML_INGEST_DIR") or tempfile.gettempdir()
    b = ingest.frame_clip_boundaries()[:L + 1].astype(np.int64)
    per_video = int(b[-1])
    need = nv * (per_video + L) * (D_RES + D_I3D + D_SUB) * 2
    while need > 0.5 * shutil.disk_usage(root).free and nv > 256:
        nv, need = nv // 2, need // 2
    d = tempfile.mkdtemp(prefix="xml_ingest_pool_", dir=root)
    names = ["v%05d" % i for i in range(nv)]
    rng = np.random.default_rng(5)
    pat, n_words = word_ranges(rng)
    try:
        w = {t: ingest.FeatureStoreWriter(os.path.join(d, t), dim, "float16")
             for t, dim in (("res", D_RES), ("i3d", D_I3D), ("words", D_SUB), ("clip_v", D_RES + D_I3D), ("clip_s", D_SUB))}
        g = torch.Generator(device=dev).manual_seed(7)
        wranges = {}
        for i, name in enumerate(names):                                     # one video at a time: pooled on the device, once
            p = i % len(pat)
            r = (torch.randn((per_video, D_RES), generator=g, device=dev).abs() * 0.5).half()
            x = (torch.randn((per_video, D_I3D), generator=g, device=dev).abs() * 0.5).half()
            t = (torch.randn((max(int(n_words[p]), 1), D_SUB), generator=g, device=dev) * 0.5).half()
            wranges[name] = pat[p]
            seg = torch.from_numpy(np.stack([b[:-1], b[1:]], 1)).to(dev)
            one = torch.tensor([0, L], device=dev)
            cv, _ = ops.ingest_pool_rows([(r, seg, True), (x, seg, True)], one, 1, L, L, normalize=False)
            cs, _ = ops.ingest_pool_rows([(t, torch.from_numpy(pat[p]).to(dev), False)], one, 1, L, L, normalize=False)
            for tag, a in (("res", r), ("i3d", x), ("words", t), ("clip_v", cv[0]), ("clip_s", cs[0])):
                w[tag].add(name, a.cpu().numpy())
        for x in w.values():
            x.close()
        S = lambda t: ingest.FeatureStore(os.path.join(d, t))                # noqa: E731
        stores = {"pooled": (ingest.PooledStore([(S("res"), b, True), (S("i3d"), b, True)]),
                             ingest.PooledStore([(S("words"), wranges, False)])),
                  "clips": (S("clip_v"), S("clip_s"))}
        nq, _, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
        torch.manual_seed(0)
        model = XML(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), compute_dtype=torch.bfloat16).to(dev).eval()
        out = {"videos": nv, "batch_videos": batch}
        for rep in range(2):                                                 # interleaved: pooled, clips, pooled, clips
            for tag, (vs, ss) in stores.items():
                kw = dict(max_ctx_len=L, batch_size=batch, device=dev, feature_dtype=torch.bfloat16)
                feeder = ingest.ContextFeeder(names, vs, ss, **kw)
                warm = ingest.ContextFeeder(names[:2 * batch], vs, ss, **kw)  # pins both staging slots, packs weights: not timed
                warm._stage = feeder._stage
                with torch.no_grad():
                    inf.build_corpus_index(model, warm, n_total=min(nv, 2 * batch), l_ref=L)
                    torch.cuda.synchronize()
                    feeder._slot_done = {}
                    t0 = time.perf_counter()
                    index = inf.build_corpus_index(model, feeder, n_total=nv, l_ref=L)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                st = feeder.stats
                out.setdefault(tag, []).append({"wall_s": round(dt, 4), "videos_per_s": round(nv / dt, 1),
                                                "h2d_gb": round(st["h2d_bytes"] / 1e9, 3), "host_gather_s": round(st["gather_s"], 4)})
                del index, feeder, warm
                torch.cuda.empty_cache()
        out["videos_per_s_ratio_pooled_over_clips"] = round(
            max(r["videos_per_s"] for r in out["pooled"]) / max(r["videos_per_s"] for r in out["clips"]), 3)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    nv_k, nv_f, rounds = (a + [None] * 3)[:3]
    res = {"kernel": kernel_leg(nv_k or 2048, rounds or 20)}
    if nv_f != 0:
        res["feeder"] = feeder_leg(nv_f or 1024)
    print(json.dumps(res))
