"""Time the training data path at the C5 shape (batch 128, video 3072-d, subtitle / query 768-d, bf16 model) on synthetic
feature stores that hold real TVR clip counts (tests/golden/tvr_clip_count_hist.json).

    python tools/bench_train_epoch.py [--videos 1200] [--examples 4096] [--out profiles/train_store_timing.md]

Three measurements, printed as one JSON line and written to --out:
  fill        one batch's fill from the device-resident store (three xml_gather_feature_rows launches + the label gather),
              f16 -> f32 and f16 -> bf16, event-timed; per modality against xml_ingest_rows on the same batch's rows laid back
              to back (same bytes, same arithmetic), alternating in the same process
  graphed     the store-fed graphed epoch (train_data.train_epoch: fill + replay, losses read at the end) against the same
              captured step replayed on a resident batch without a per-step loss read, alternating in the same process
  host_fed    the same steps fed from the host: StoreTrainDataset + collate + one pinned copy per step (reported, not judged)
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, nominal


def make_stores(tmp, n_videos, n_examples, dv, ds, max_desc_len, seed=0):
    from tvretrieval_amd import ingest
    rng = np.random.default_rng(seed)
    hist = np.asarray(json.load(open(os.path.join(ROOT, "tests", "golden", "tvr_clip_count_hist.json")))["hist"], dtype=np.float64)
    hist[0] = 0
    vlens = rng.choice(len(hist), size=n_videos, p=hist / hist.sum())
    qlens = rng.integers(5, max_desc_len + 1, n_examples)
    stores = {}
    for tag, dim, lens, names in (("video", dv, vlens, ["v%d" % i for i in range(n_videos)]),
                                  ("sub", ds, vlens, ["v%d" % i for i in range(n_videos)]),
                                  ("desc", ds, qlens, [str(i) for i in range(n_examples)])):
        base = rng.standard_normal((4096, dim)).astype(np.float16)
        w = ingest.FeatureStoreWriter(os.path.join(tmp, tag), dim, "float16")
        for name, l in zip(names, lens):
            w.add(name, base[rng.integers(0, 4096, int(l))])
        w.close()
        stores[tag] = ingest.FeatureStore(os.path.join(tmp, tag))
    examples = []
    for i in range(n_examples):
        v = int(rng.integers(0, n_videos))
        a = float(rng.uniform(0, vlens[v] * 1.5))
        examples.append(dict(desc_id=i, desc="", vid_name="v%d" % v, duration=float(vlens[v] * 1.5),
                             ts=[a, a + float(rng.uniform(1.0, 12.0))]))
    return examples, stores, vlens


def timed(fn, reps):
    """ms per call of `reps` back-to-back calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_fill(store, ids, lmax, lq, rounds=9, reps=20):
    from tvretrieval_amd import ops
    dev = store.device
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=dev)
    out = {}
    for odt, oname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        store.feature_dtype = odt
        static = store.batch(ids_dev, lmax=lmax, lq=lq)
        whole = [timed(lambda: store.fill(static, ids_dev), reps) for _ in range(rounds)]
        res = dict(fill_ms=round(float(np.median(whole)), 4))
        total_bytes = 0
        for tag, length, max_len in (("query", lq, store.max_desc_len), ("video", lmax, store.max_ctx_len),
                                     ("sub", lmax, store.max_ctx_len)):
            r = store.res[tag]
            items = store.item_of[tag][ids_dev.long()].cpu().numpy()
            start = r.row_start.cpu().numpy()
            lens = np.minimum(start[items + 1] - start[items], min(max_len, length))
            packed = torch.cat([r.rows[int(start[i]):int(start[i]) + int(l)] for i, l in zip(items, lens)])
            pstart = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
            f, m = static[tag + "_feat"], static[tag + "_mask"]
            gather = lambda: ops.gather_feature_rows(r.rows, r.row_start, ids_dev, length, max_len,            # noqa: E731
                                                     item_of=store.item_of[tag], normalize=store.norm[tag], out=f, mask_out=m,
                                                     want_len=False)
            ingest = lambda: ops.ingest_rows(packed, pstart, len(ids), length, max_len, normalize=store.norm[tag],    # noqa: E731
                                             out_dtype=odt)
            ingest()
            tg, ti = [], []
            for _ in range(rounds):           # alternating
                tg.append(timed(gather, reps))
                ti.append(timed(ingest, reps))
            nbytes = int(lens.sum()) * r.dim * r.rows.element_size() + f.numel() * f.element_size() + m.numel() * 4
            total_bytes += nbytes
            g, i_ = float(np.median(tg)), float(np.median(ti))
            res[tag] = dict(gather_us=round(g * 1e3, 2), ingest_rows_us=round(i_ * 1e3, 2), ratio=round(g / i_, 3),
                            bytes=nbytes, gather_gbs=round(nbytes / g / 1e6, 1),
                            hbm_share=round(nbytes / g / 1e6 / HBM_PEAK_GBS, 3))
        res["bytes"] = total_bytes
        res["fill_gbs"] = round(total_bytes / res["fill_ms"] / 1e6, 1)
        res["hbm_share"] = round(res["fill_gbs"] / HBM_PEAK_GBS, 3)
        out["f16_to_" + oname] = res
    store.feature_dtype = torch.float32
    return out


def bench_steps(store, examples, stores, a):
    from tvretrieval_amd import train_data as td
    from tvretrieval_amd.model_xml import XML, xml_base_config
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep
    dev = store.device
    cfg = dict(xml_base_config)
    cfg.update(visual_input_size=a.dv, sub_input_size=a.ds, query_input_size=a.ds, hidden_size=a.hidden, max_ctx_l=a.ctx_l,
               max_desc_l=a.desc_l, lw_st_ed=0.01)
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
    step = GraphedTrainStep(model, opt, store.batch(order[:a.bsz].tolist(), lmax=a.ctx_l, lq=a.desc_l))
    o = types.SimpleNamespace(bsz=a.bsz, grad_clip=-1, debug=False, hard_negtiave_start_epoch=-1, hard_pool_size=20,
                              train_span_start_epoch=-1, lw_st_ed=0.01)
    steps = n // a.bsz

    def resident():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def fed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        td.train_epoch(model, opt, store, o, 0, step=step, order=order)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    resident(), fed()
    tr, tf = [], []
    for _ in range(a.rounds):
        tr.append(resident())
        tf.append(fed())
    # host-fed: what a user writes without the device store
    ds = td.StoreTrainDataset(examples, stores["desc"], stores["video"], stores["sub"], max_desc_len=a.desc_l,
                              max_ctx_len=a.ctx_l, ctx_mode="video_sub")
    pinned = None
    hsteps = min(a.host_steps, steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(hsteps):
        _, batch = td.collate([ds[int(i)] for i in order[b * a.bsz:(b + 1) * a.bsz]], lmax=a.ctx_l, lq=a.desc_l)
        if pinned is None:
            pinned = {k: torch.from_numpy(v).pin_memory() for k, v in batch.items()}
        for k, v in batch.items():
            pinned[k].numpy()[...] = v
        step(pinned)
        torch.cuda.synchronize()        # the pinned buffers are rewritten by the next step
    host_ms = (time.perf_counter() - t0) / hsteps * 1e3
    return dict(steps_per_epoch=steps, resident_ms=round(float(np.median(tr)), 3), store_fed_ms=round(float(np.median(tf)), 3),
                resident_all=[round(x, 3) for x in tr], store_fed_all=[round(x, 3) for x in tf],
                host_fed_ms=round(host_ms, 2), host_fed_steps=hsteps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=1200)
    ap.add_argument("--examples", type=int, default=4096)
    ap.add_argument("--bsz", type=int, default=128)
    ap.add_argument("--ctx-l", type=int, default=100)
    ap.add_argument("--desc-l", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--dv", type=int, default=3072)
    ap.add_argument("--ds", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=6)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_store_timing.md"))
    a = ap.parse_args()
    from tvretrieval_amd import train_data as td
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        examples, stores, vlens = make_stores(tmp, a.videos, a.examples, a.dv, a.ds, a.desc_l)
        t0 = time.perf_counter()
        store = td.DeviceTrainStore(examples, stores["desc"], stores["video"], stores["sub"], max_desc_len=a.desc_l,
                                    max_ctx_len=a.ctx_l, ctx_mode="video_sub", device=dev)
        upload_s = time.perf_counter() - t0
        resident_bytes = sum(r.rows.numel() * r.rows.element_size() for r in store.res.values())
        fill = bench_fill(store, list(range(a.bsz)), a.ctx_l, a.desc_l)
        steps = bench_steps(store, examples, stores, a)
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip() + " + working tree"
        except Exception:
            commit = "unknown"
    res = dict(metric="train_store", box=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, commit=commit,
               config=dict(bsz=a.bsz, ctx_l=a.ctx_l, desc_l=a.desc_l, hidden=a.hidden, dv=a.dv, ds=a.ds, videos=a.videos,
                           examples=a.examples, mean_clips=round(float(np.minimum(vlens, a.ctx_l).mean()), 1)),
               resident_mb=round(resident_bytes / 1e6, 1), upload_s=round(upload_s, 2), fill=fill, graphed=steps)
    print(json.dumps(res))
    lines = ["# Training from a device-resident feature store: timing", "",
             "Written by `tools/bench_train_epoch.py`.  Box: %s, torch %s, HIP %s.  Commit: %s." % (
                 res["box"], res["torch"], res["hip"], commit), "",
             "Shape: batch %d, max_ctx_len %d, max_desc_len %d, video %d-d, subtitle / query %d-d, hidden %d, bf16 model; %d "
             "videos with TVR clip counts (mean %.1f after truncation), %d examples; stores in f16, %.0f MB resident, uploaded in "
             "%.2f s." % (a.bsz, a.ctx_l, a.desc_l, a.dv, a.ds, a.hidden, a.videos, res["config"]["mean_clips"], a.examples,
                          res["resident_mb"], upload_s), "",
             "## Fill time (one batch; medians of %d rounds of %d back-to-back launches, event-timed)" % (9, 20), "",
             "| output | stream | gather us | xml_ingest_rows us | ratio | bytes | GB/s | share of %d GB/s |" % HBM_PEAK_GBS,
             "|---|---|---|---|---|---|---|---|"]
    for oname, f in fill.items():
        for tag in ("query", "video", "sub"):
            t = f[tag]
            lines.append("| %s | %s | %.2f | %.2f | %.3f | %d | %.1f | %.3f |" % (
                oname, tag, t["gather_us"], t["ingest_rows_us"], t["ratio"], t["bytes"], t["gather_gbs"], t["hbm_share"]))
        lines.append("| %s | whole fill (3 gathers + labels) | %.2f | | | %d | %.1f | %.3f |" % (
            oname, f["fill_ms"] * 1e3, f["bytes"], f["fill_gbs"], f["hbm_share"]))
    g = steps
    lines += ["", "## Graphed step (ms per step, medians of %d alternating rounds of %d steps)" % (a.rounds, g["steps_per_epoch"]), "",
              "| feed | ms per step | rounds |", "|---|---|---|",
              "| resident batch, `step(None)`, no per-step loss read | %.3f | %s |" % (g["resident_ms"], g["resident_all"]),
              "| store-fed `train_epoch(step=...)`: fill + replay, losses read at the end | %.3f | %s |" % (
                  g["store_fed_ms"], g["store_fed_all"]),
              "| host-fed: StoreTrainDataset + collate + one pinned copy per step (%d steps) | %.2f | |" % (
                  g["host_fed_steps"], g["host_fed_ms"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
