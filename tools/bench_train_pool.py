"""Time the training gather over resident frame- and word-level stores (xml_gather_pool_feature_rows, DeviceTrainStore over
ingest.PooledStore) at batch 128 on synthetic stores that hold real TVR clip counts (tests/golden/tvr_clip_count_hist.json).

    python tools/bench_train_pool.py [--videos 600] [--examples 1024] [--out profiles/train_pool_timing.md]

Frames are ResNet 2048 || I3D 1024 f16 rows over ingest.frame_clip_boundaries() (4-5 per clip), words 768 f16 rows with the
subtitle-like ranges of tools/bench_ingest_pool.py.  Per stream and output dtype three launches are interleaved in one process
after a warm-up, HIP events around each, median and min..max of --rounds:
  gather_pool   xml_gather_pool_feature_rows on the resident fine rows, the batch named by example ids
  (a)           xml_ingest_pool_rows on the same ranges laid back to back: the same row body without the indirection
  (b)           xml_gather_feature_rows from pre-pooled f16 clip rows: the same output shape from 1 / 4.5 of the source bytes
Bytes: every source row once per clip row that names it + the output + the mask; GB/s = bytes / median time.
Then the graphed step fed through train_epoch(step=...) from the pooled store against the same steps from the clip store
(alternating rounds, every round listed), and the resident bytes of both stores.  One JSON line, and the table in --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D_RES, D_I3D, D_SUB = 2048, 1024, 768


def make_stores(tmp, a, dev):
    """-> examples, {desc, res, i3d, words, clip_v, clip_s} FeatureStores, word ranges, clip counts.  The clip stores hold the
    rows the fine stores pool into (max, per-source norm on the video side), pooled on the device once, in f16."""
    from bench_ingest_pool import word_ranges
    from tvretrieval_amd import ingest, ops
    rng = np.random.default_rng(0)
    hist = np.asarray(json.load(open(os.path.join(ROOT, "tests", "golden", "tvr_clip_count_hist.json")))["hist"], dtype=np.float64)
    hist[0] = 0
    vlens = rng.choice(len(hist), size=a.videos, p=hist / hist.sum())
    b = ingest.frame_clip_boundaries().astype(np.int64)
    pat, _ = word_ranges(rng, 16)                          # (16, 128, 2) ranges of videos of 128 clips
    names = ["v%d" % i for i in range(a.videos)]
    w = {t: ingest.FeatureStoreWriter(os.path.join(tmp, t), dim, "float16")
         for t, dim in (("res", D_RES), ("i3d", D_I3D), ("words", D_SUB), ("clip_v", D_RES + D_I3D), ("clip_s", D_SUB),
                        ("desc", D_SUB))}
    base = {t: np.abs(rng.standard_normal((4096, dim))).astype(np.float16) * 0.5 for t, dim in (("res", D_RES), ("i3d", D_I3D))}
    base["words"] = (rng.standard_normal((4096, D_SUB)) * 0.5).astype(np.float16)
    wranges = {}
    for i, (name, l) in enumerate(zip(names, vlens)):
        l = int(l)
        frames = int(b[l])
        r, x = base["res"][rng.integers(0, 4096, frames)], base["i3d"][rng.integers(0, 4096, frames)]
        wr = pat[i % len(pat)][:l]
        n_words = max(int(wr[:, 1].max()), 1)
        t = base["words"][rng.integers(0, 4096, n_words)]
        wranges[name] = wr
        seg = torch.from_numpy(np.stack([b[:l], b[1:l + 1]], 1)).to(dev)
        one = torch.tensor([0, l], device=dev)
        cv, _ = ops.ingest_pool_rows([(torch.from_numpy(r).to(dev), seg, True), (torch.from_numpy(x).to(dev), seg, True)], one, 1, l,
                                     l, normalize=False)
        cs, _ = ops.ingest_pool_rows([(torch.from_numpy(t).to(dev), torch.from_numpy(wr).to(dev), False)], one, 1, l, l,
                                     normalize=False)
        for tag, arr in (("res", r), ("i3d", x), ("words", t), ("clip_v", cv[0].cpu().numpy()), ("clip_s", cs[0].cpu().numpy())):
            w[tag].add(name, arr)
    qlens = rng.integers(5, a.desc_l + 1, a.examples)
    for i, l in enumerate(qlens):
        w["desc"].add(str(i), base["words"][rng.integers(0, 4096, int(l))])
    for x in w.values():
        x.close()
    examples = []
    for i in range(a.examples):
        v = int(rng.integers(0, a.videos))
        s = float(rng.uniform(0, vlens[v] * 1.5))
        examples.append(dict(desc_id=i, desc="", vid_name="v%d" % v, duration=float(vlens[v] * 1.5),
                             ts=[s, s + float(rng.uniform(1.0, 12.0))]))
    stores = {t: ingest.FeatureStore(os.path.join(tmp, t)) for t in w}
    return examples, stores, b, wranges, vlens


def bench_gather(pooled, clips, ids, lmax, rounds):
    from bench_ingest_pool import time_interleaved
    from tvretrieval_amd import ops
    dev = pooled.device
    n = len(ids)
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=dev)
    out = {}
    for tag in ("video", "sub"):
        rp, rc = pooled.res[tag], clips.res[tag]
        max_len = pooled.max_ctx_len
        items = pooled.item_of[tag][ids_dev.long()].cpu().numpy()
        cstart = rp.clip_start.cpu().numpy()
        lens = np.minimum(cstart[items + 1] - cstart[items], min(max_len, lmax))
        rows_idx = np.concatenate([np.arange(cstart[i], cstart[i] + l) for i, l in zip(items, lens)])
        bstart = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        bsrc = [(rows, seg[torch.from_numpy(rows_idx).to(dev)].contiguous(), nm) for rows, seg, nm in rp.sources]
        fine_rows = sum(int((seg[:, 1] - seg[:, 0]).sum()) * rows.shape[1] * rows.element_size() for rows, seg, _ in bsrc)
        clip_rows = int(lens.sum()) * rc.dim * rc.rows.element_size()
        for oname, odt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            f = torch.empty((n, lmax, rp.dim), dtype=odt, device=dev)
            m = torch.empty((n, lmax), dtype=torch.float32, device=dev)
            fns = {
                "gather_pool": lambda: ops.gather_pool_feature_rows(rp.sources, rp.clip_start, ids_dev, lmax, max_len,
                                                                    item_of=pooled.item_of[tag], pool=rp.pool, out=f, mask_out=m,
                                                                    want_len=False),
                "a_ingest_pool": lambda: ops.ingest_pool_rows(bsrc, bstart, n, lmax, max_len, pool=rp.pool, out_dtype=odt),
                "b_gather_clips": lambda: ops.gather_feature_rows(rc.rows, rc.row_start, ids_dev, lmax, max_len,
                                                                  item_of=clips.item_of[tag], out=f, mask_out=m, want_len=False),
            }
            us = time_interleaved(fns, rounds)
            wr = f.numel() * es + m.numel() * 4
            leg = {}
            for k, v in us.items():
                nbytes = (clip_rows if k == "b_gather_clips" else fine_rows) + wr
                med = statistics.median(v)
                leg[k] = dict(us_median=round(med, 2), us_min=round(v[0], 2), us_max=round(v[-1], 2), bytes=nbytes,
                              gb_per_s=round(nbytes / 1e3 / med, 1))
            for k in ("a_ingest_pool", "b_gather_clips"):
                leg["bytes_per_s_ratio_over_" + k] = round(leg["gather_pool"]["gb_per_s"] / leg[k]["gb_per_s"], 3)
                leg["time_ratio_over_" + k] = round(leg["gather_pool"]["us_median"] / leg[k]["us_median"], 3)
            out["%s_%s" % (tag, oname)] = leg
        out[tag + "_source_rows_per_clip"] = round(fine_rows / max(clip_rows, 1), 2)
    return out


def bench_steps(pooled, clips, examples, a):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.model_xml import XML, xml_base_config
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep
    dev = pooled.device
    cfg = dict(xml_base_config)
    cfg.update(visual_input_size=D_RES + D_I3D, sub_input_size=D_SUB, query_input_size=D_SUB, hidden_size=a.hidden,
               max_ctx_l=a.ctx_l, max_desc_l=a.desc_l, lw_st_ed=0.01)
    torch.manual_seed(1234)
    model = XML(cfg, compute_dtype=torch.bfloat16).to(dev)
    named = list(model.named_parameters())
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    opt = BertAdam([{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
                    {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}],
                   lr=1e-4, warmup=0.01, t_total=100000)
    model.train()
    n = len(examples) // a.bsz * a.bsz
    order = np.arange(n)
    step = GraphedTrainStep(model, opt, clips.batch(order[:a.bsz].tolist(), lmax=a.ctx_l, lq=a.desc_l))
    o = types.SimpleNamespace(bsz=a.bsz, grad_clip=-1, debug=False, hard_negtiave_start_epoch=-1, hard_pool_size=20,
                              train_span_start_epoch=-1, lw_st_ed=0.01)
    steps = n // a.bsz

    def fed(store):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        td.train_epoch(model, opt, store, o, 0, step=step, order=order)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    fed(clips), fed(pooled)
    tc, tp = [], []
    for _ in range(a.step_rounds):
        tc.append(fed(clips))
        tp.append(fed(pooled))
    return dict(steps_per_epoch=steps, clip_store_ms=round(float(np.median(tc)), 3), pooled_store_ms=round(float(np.median(tp)), 3),
                clip_store_all=[round(x, 3) for x in tc], pooled_store_all=[round(x, 3) for x in tp])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=600)
    ap.add_argument("--examples", type=int, default=1024)
    ap.add_argument("--bsz", type=int, default=128)
    ap.add_argument("--ctx-l", type=int, default=100)
    ap.add_argument("--desc-l", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_pool_timing.md"))
    a = ap.parse_args()
    from tvretrieval_amd import ingest, train_data as td
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        examples, st, b, wranges, vlens = make_stores(tmp, a, dev)
        pv = ingest.PooledStore([(st["res"], b, True), (st["i3d"], b, True)])
        ps = ingest.PooledStore([(st["words"], wranges, False)])
        kw = dict(max_desc_len=a.desc_l, max_ctx_len=a.ctx_l, ctx_mode="video_sub", device=dev)
        t0 = time.perf_counter()
        pooled = td.DeviceTrainStore(examples, st["desc"], pv, ps, **kw)
        upload_pooled = time.perf_counter() - t0
        t0 = time.perf_counter()
        clips = td.DeviceTrainStore(examples, st["desc"], st["clip_v"], st["clip_s"], **kw)
        upload_clips = time.perf_counter() - t0
        assert np.array_equal(pooled.ctx_len, clips.ctx_len) and np.array_equal(pooled.labels_host, clips.labels_host)
        resident = {k: {tag: int(r.nbytes) for tag, r in s.res.items()} for k, s in (("pooled", pooled), ("clips", clips))}
        gather = bench_gather(pooled, clips, list(range(a.bsz)), a.ctx_l, a.rounds)
        steps = None if a.no_steps else bench_steps(pooled, clips, examples, a)
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip() + " + working tree"
        except Exception:
            commit = "unknown"
    box = "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    res = dict(metric="train_pool", box=box, torch=torch.__version__, hip=torch.version.hip, commit=commit,
               config=dict(bsz=a.bsz, ctx_l=a.ctx_l, desc_l=a.desc_l, hidden=a.hidden, videos=a.videos, examples=a.examples,
                           rounds=a.rounds, mean_clips=round(float(np.minimum(vlens, a.ctx_l).mean()), 1)),
               resident_bytes=resident, upload_s=dict(pooled=round(upload_pooled, 2), clips=round(upload_clips, 2)), gather=gather,
               graphed=steps)
    print(json.dumps(res))
    lines = ["# Training from resident frame- and word-level stores: timing", "",
             "Written by `tools/bench_train_pool.py`.  Box: %s, torch %s, HIP %s.  Commit: %s." % (
                 res["box"], res["torch"], res["hip"], commit), "",
             "Shape: batch %d, max_ctx_len %d, video ResNet %d || I3D %d f16 frame rows over `frame_clip_boundaries()`, subtitle %d "
             "f16 word rows; %d videos with TVR clip counts (mean %.1f after truncation), %d examples.  Max pooling, both video "
             "sources normalised, the row norm on." % (a.bsz, a.ctx_l, D_RES, D_I3D, D_SUB, a.videos, res["config"]["mean_clips"],
                                                       a.examples), "",
             "## One batch's gather (HIP events around each launch, the three launches interleaved, median [min .. max] of %d)"
             % a.rounds, "",
             "(a) `xml_ingest_pool_rows` on the same ranges laid back to back; (b) `xml_gather_feature_rows` from pre-pooled f16 "
             "clip rows.  Bytes: source rows named by the batch + output + mask.", "",
             "| stream | output | launch | us | bytes | GB/s | gather_pool GB/s over it | gather_pool time over it |",
             "|---|---|---|---|---|---|---|---|"]
    for tag in ("video", "sub"):
        for oname in ("f32", "bf16"):
            leg = gather["%s_%s" % (tag, oname)]
            for k in ("gather_pool", "a_ingest_pool", "b_gather_clips"):
                t = leg[k]
                lines.append("| %s | %s | %s | %.2f [%.2f .. %.2f] | %d | %.1f | %s | %s |" % (
                    tag, oname, k, t["us_median"], t["us_min"], t["us_max"], t["bytes"], t["gb_per_s"],
                    "" if k == "gather_pool" else "%.3f" % leg["bytes_per_s_ratio_over_" + k],
                    "" if k == "gather_pool" else "%.3f" % leg["time_ratio_over_" + k]))
    lines += ["", "Fine source bytes per pre-pooled clip byte in this batch: video %.2f, subtitles %.2f." % (
        gather["video_source_rows_per_clip"], gather["sub_source_rows_per_clip"]), ""]
    if steps is not None:
        lines += ["## Graphed step fed through `train_epoch(step=...)` (ms per step, %d alternating rounds of %d steps, hidden %d, "
                  "bf16 model)" % (a.step_rounds, steps["steps_per_epoch"], a.hidden), "",
                  "| store | median ms per step | rounds |", "|---|---|---|",
                  "| clip stores (`xml_gather_feature_rows`) | %.3f | %s |" % (steps["clip_store_ms"], steps["clip_store_all"]),
                  "| pooled stores (`xml_gather_pool_feature_rows`) | %.3f | %s |" % (steps["pooled_store_ms"],
                                                                                      steps["pooled_store_all"]), ""]
    lines += ["## Resident bytes", "", "| store | query | video | sub | total | uploaded in |", "|---|---|---|---|---|---|"]
    for k in ("pooled", "clips"):
        r = resident[k]
        lines.append("| %s | %d | %d | %d | %d | %.2f s |" % (k, r["query"], r["video"], r["sub"], sum(r.values()),
                                                             res["upload_s"][k]))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
