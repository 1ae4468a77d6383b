"""Time the training step on a resident index (tvretrieval_amd/train_index.py) against the full step at the training bench's
shape: batch 128, bf16, hidden 768, video 3072 / subtitle 768 / query 768 features, TVR clip counts
(tests/golden/tvr_clip_count_hist.json) truncated to 100 clips, dropout on.

    python tools/bench_train_index.py [--videos 512] [--rounds 30] [--out profiles/train_index_timing.md]

Three steps, eager and captured (train.GraphedTrainStep), alternated round by round in one process after a warm-up; a round is
--steps steps between two device synchronisations on the host clock; median [min .. max] of --rounds:
  full     train.xml_forward_train, every parameter trains
  frozen   the same forward with the context side frozen by requires_grad_(False) -- the honest baseline: what a user could
           do before this module existed
  index    train_index.xml_forward_train_index on an index of --videos videos built from the same model
Then the gather alone (xml_index_gather_video_rows, HIP events, interleaved with xml_gather_feature_rows writing the same
number of output bytes from a resident f16 clip store): microseconds and bytes moved (read + written) per second.
One JSON line, and the table in --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DV, DS, DQ = 3072, 768, 768


def make_model(a, dev, seed=1234):
    from tvretrieval_amd.model_xml import XML, xml_base_config
    cfg = dict(xml_base_config)
    cfg.update(visual_input_size=DV, sub_input_size=DS, query_input_size=DQ, hidden_size=a.hidden, max_ctx_l=a.ctx_l,
               max_desc_l=a.desc_l, lw_st_ed=0.01)
    torch.manual_seed(seed)
    return XML(cfg, compute_dtype=torch.bfloat16).to(dev)


def make_data(a, dev):
    rng = np.random.default_rng(0)
    hist = np.asarray(json.load(open(os.path.join(ROOT, "tests", "golden", "tvr_clip_count_hist.json")))["hist"], dtype=np.float64)
    hist[0] = 0
    vlens = np.minimum(rng.choice(len(hist), size=a.videos, p=hist / hist.sum()), a.ctx_l)
    vlens[0] = a.ctx_l
    g = torch.Generator().manual_seed(1)
    mask = (torch.arange(a.ctx_l)[None, :] < torch.as_tensor(vlens)[:, None]).float()

    def feats(n, l, d, m):
        return (torch.nn.functional.normalize(torch.randn(n, l, d, generator=g), dim=-1) * m[:, :, None]).to(dev)
    qlens = torch.as_tensor(np.concatenate([[a.desc_l], rng.integers(5, a.desc_l + 1, a.bsz - 1)]))
    qm = (torch.arange(a.desc_l)[None, :] < qlens[:, None]).float()
    vf, sf = [], []
    for b in range(0, a.videos, a.bsz):                          # (generated batch by batch: 3072-wide f32 rows)
        vf.append(feats(min(a.bsz, a.videos - b), a.ctx_l, DV, mask[b:b + a.bsz]))
        sf.append(feats(min(a.bsz, a.videos - b), a.ctx_l, DS, mask[b:b + a.bsz]))
    lens = torch.as_tensor(vlens[:a.bsz])
    st = (torch.rand(a.bsz, generator=g) * lens).long()
    ed = torch.minimum(st + 1 + (torch.rand(a.bsz, generator=g) * 4).long(), lens - 1).clamp_min(0)
    st = torch.minimum(st, ed)
    batch = dict(query_feat=feats(a.bsz, a.desc_l, DQ, qm), query_mask=qm.to(dev), video_feat=vf[0], video_mask=mask[:a.bsz].to(dev),
                 sub_feat=sf[0], sub_mask=mask[:a.bsz].to(dev), st_ed_indices=torch.stack([st, ed], 1).to(dev))
    return batch, [(v, mask[i * a.bsz:(i + 1) * a.bsz].to(dev), s, mask[i * a.bsz:(i + 1) * a.bsz].to(dev))
                   for i, (v, s) in enumerate(zip(vf, sf))], vlens


def make_runners(a, dev, batch, ctx_batches):
    """name -> (eager callable, graphed callable): one step each."""
    from tvretrieval_amd import inference, train_index as TI
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep, train_step
    okw = dict(lr=1e-4, warmup=0.01, t_total=100000)
    runners, info = {}, {}
    for name in ("full", "frozen", "index"):
        model = make_model(a, dev)
        fwd_batch, forward = batch, None
        if name == "index":
            with torch.no_grad():
                index = inference.build_corpus_index(model.eval(), ctx_batches)
            form = TI.index_form(model, index)
            slots = np.arange(a.bsz)
            fwd_batch = dict(index=index, query_feat=batch["query_feat"], query_mask=batch["query_mask"],
                             ctx_slots=torch.from_numpy(slots.astype(np.int32)).to(dev),
                             ctx_first_block=torch.from_numpy(TI.slot_first_blocks(index, form, slots).astype(np.int32)).to(dev),
                             st_ed_indices=batch["st_ed_indices"], ctx_len=a.ctx_l)
            forward = TI.xml_forward_train_index
            info.update(index_form=form, index_bytes=int(index.hbm_bytes()), index=index, slots=fwd_batch["ctx_slots"],
                        first_block=fwd_batch["ctx_first_block"])
        params = TI.query_side_parameters(model) if name != "full" else list(model.parameters())
        model.train()
        opt = BertAdam(params, **okw)
        kw = {} if forward is None else dict(forward=forward)
        step = GraphedTrainStep(model, opt, fwd_batch, **kw)
        runners[name] = (lambda m=model, o=opt, b=fwd_batch, kw=kw: train_step(m, o, b, **kw), lambda s=step: s(None))
        info[name + "_trained_tensors"] = len(opt.params)
    return runners, info


def time_steps(fns, rounds, steps, warmup=2):
    """fns: name -> callable; every round runs each `steps` times in turn between two synchronisations -> name -> sorted ms."""
    ms = {k: [] for k in fns}
    for r in range(warmup + rounds):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: sorted(v) for k, v in ms.items()}


def bench_gather(a, dev, info, vlens, rounds):
    from bench_ingest_pool import time_interleaved
    from tvretrieval_amd import ops, train_index as TI
    index = info["index"]
    form = info["index_form"]
    h = a.hidden
    out = TI.gather_context(index, form, info["slots"], info["first_block"], a.ctx_l)
    # the same number of OUTPUT bytes from a resident f16 clip store: n_mod * 2 streams of (bsz, ctx_l, hidden) bf16
    rows = int(vlens.sum())
    src = torch.randn((rows, h), device=dev).half()
    start = torch.from_numpy(np.concatenate([[0], np.cumsum(vlens)]).astype(np.int64)).to(dev)
    f = torch.empty((a.bsz, a.ctx_l, h), dtype=torch.bfloat16, device=dev)
    m = torch.empty((a.bsz, a.ctx_l), dtype=torch.float32, device=dev)
    n_streams = 2 * len(index.modalities)

    def feature_rows():
        for _ in range(n_streams):
            ops.gather_feature_rows(src, start, info["slots"], a.ctx_l, a.ctx_l, out_dtype=torch.bfloat16, out=f, mask_out=m,
                                    want_len=False)
    us = time_interleaved({"index_gather_video_rows": lambda: TI.gather_context(index, form, info["slots"], info["first_block"],
                                                                                 a.ctx_l, out=out),
                           "gather_feature_rows_x%d" % n_streams: feature_rows}, rounds)
    valid = int(vlens[:a.bsz].sum())
    wr = n_streams * a.bsz * a.ctx_l * h * 2
    res = {}
    for k, v in us.items():
        rd = n_streams * valid * h * 2
        med = statistics.median(v)
        res[k] = dict(us_median=round(med, 2), us_min=round(v[0], 2), us_max=round(v[-1], 2), bytes=rd + wr,
                      tb_per_s=round((rd + wr) / 1e6 / med, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=512)
    ap.add_argument("--bsz", type=int, default=128)
    ap.add_argument("--ctx-l", type=int, default=100)
    ap.add_argument("--desc-l", type=int, default=30)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_index_timing.md"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    batch, ctx_batches, vlens = make_data(a, dev)
    runners, info = make_runners(a, dev, batch, ctx_batches)
    eager = time_steps({k: v[0] for k, v in runners.items()}, max(3, a.rounds // 3), max(2, a.steps // 4))
    graphed = time_steps({k: v[1] for k, v in runners.items()}, a.rounds, a.steps)
    gather = bench_gather(a, dev, info, vlens, a.rounds)
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip() + " + working tree"
        except Exception:
            commit = "unknown"
    box = "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    summ = lambda v: dict(ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))      # noqa: E731
    res = dict(metric="train_index", box=box, torch=torch.__version__, hip=torch.version.hip, commit=commit,
               config=dict(bsz=a.bsz, ctx_l=a.ctx_l, desc_l=a.desc_l, hidden=a.hidden, videos=a.videos, rounds=a.rounds, steps=a.steps,
                           mean_clips=round(float(vlens.mean()), 1), index_form=info["index_form"], index_bytes=info["index_bytes"],
                           trained_tensors={k: info[k + "_trained_tensors"] for k in runners}),
               eager={k: summ(v) for k, v in eager.items()}, graphed={k: summ(v) for k, v in graphed.items()}, gather=gather)
    print(json.dumps(res))
    g = res["graphed"]
    verdict = ("The index step is %.2f x the frozen step's time (captured)." % (g["index"]["ms_median"] / g["frozen"]["ms_median"]))
    if g["index"]["ms_median"] >= g["frozen"]["ms_median"]:
        verdict += "  It does NOT beat the frozen baseline: what it gives is the raw training features out of HBM, not time."
    lines = ["# Training the query side on a resident index: timing", "",
             "Written by `tools/bench_train_index.py`.  Box: %s, torch %s, HIP %s.  Commit: %s." % (box, res["torch"], res["hip"], commit),
             "", "Shape: batch %d, bf16, hidden %d, video %d / subtitle %d / query %d features, %d videos with TVR clip counts "
             "truncated to %d (mean %.1f), %d query tokens, dropout on.  Index: %s K6 operand, %d bytes resident."
             % (a.bsz, a.hidden, DV, DS, DQ, a.videos, a.ctx_l, res["config"]["mean_clips"], a.desc_l, info["index_form"],
                info["index_bytes"]), "",
             "## One step (host clock around %d steps between two synchronisations, the three alternated; median [min .. max] ms)"
             % a.steps, "", "| step | trained tensors | eager | captured |", "|---|---|---|---|"]
    names = dict(full="full step (`xml_forward_train`)", frozen="context side frozen by `requires_grad_(False)`",
                 index="on the index (`xml_forward_train_index`)")
    for k in ("full", "frozen", "index"):
        e, c = res["eager"][k], g[k]
        lines.append("| %s | %d | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] |" % (
            names[k], res["config"]["trained_tensors"][k], e["ms_median"], e["ms_min"], e["ms_max"], c["ms_median"], c["ms_min"],
            c["ms_max"]))
    lines += ["", verdict, "", "## The gather alone (HIP events, interleaved, median [min .. max] of %d)" % a.rounds, "",
              "Bytes: the valid rows read + every output row written (both bf16, hidden %d).  `xml_gather_feature_rows` is launched "
              "once per output stream on a resident f16 clip store of the same clip counts." % a.hidden, "",
              "| launch | us | bytes | TB/s |", "|---|---|---|---|"]
    for k, t in gather.items():
        lines.append("| `%s` | %.2f [%.2f .. %.2f] | %d | %.3f |" % (k, t["us_median"], t["us_min"], t["us_max"], t["bytes"], t["tb_per_s"]))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
