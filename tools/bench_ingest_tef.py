"""The ingest launches with the temporal endpoint columns (xml_ingest_rows_tef, xml_ingest_pool_rows_tef) next to the launches
they extend and to the training gather that has the same unaligned row pitch; one JSON line, and the table of
profiles/ingest_tef_timing.md.

All operands resident in HBM, every launch of a group interleaved in one process after a warm-up, HIP events around each launch,
median and min..max over the rounds.  Bytes: every source row once per clip row that names it + the output; GB/s = bytes /
median time.
  clip rows    n videos x 128 clips x 3072 f16 -> f32 and bf16: xml_ingest_rows_tef, xml_ingest_rows (same rows, 8 bytes per row
               less written) and xml_gather_feature_rows(tef = 1) with ids = arange (the same rows and the same d + 2 pitch)
  pooled rows  n videos x 128 clips, ResNet 2048 + I3D 1024 f16 frame rows, 4-5 per clip (ingest.frame_clip_boundaries), max
               pooling, both per-source norms and the row norm: xml_ingest_pool_rows_tef and xml_ingest_pool_rows
Before timing, the feature columns of each *_tef launch are compared bitwise with the launch it extends.
usage: python tools/bench_ingest_tef.py [--videos 2048] [--rounds 20] [--commit ID] [--out profiles/ingest_tef_timing.md]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, D_RES, D_I3D = 128, 2048, 1024
D = D_RES + D_I3D


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


def _leg(us, bytes_):
    out = {}
    for k, v in us.items():
        med = statistics.median(v)
        out[k] = {"us_median": round(med, 1), "us_min": round(v[0], 1), "us_max": round(v[-1], 1), "gb": round(bytes_[k] / 1e9, 3),
                  "gb_per_s": round(bytes_[k] / 1e3 / med, 1)}
    return out


def measure(nv, rounds):
    from tvretrieval_amd import ops
    from tvretrieval_amd.ingest import frame_clip_boundaries
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(3)
    start = torch.arange(0, (nv + 1) * L, L, dtype=torch.int64, device=dev)
    ids = torch.arange(nv, dtype=torch.int32, device=dev)
    clip = (torch.randn((nv * L, D), generator=g, device=dev).abs() * 0.5).half()
    b = frame_clip_boundaries()[:L + 1].astype(np.int64)
    per_video = int(b[-1])
    seg = (np.stack([b[:-1], b[1:]], 1)[None] + (np.arange(nv) * per_video)[:, None, None]).reshape(-1, 2)
    res = (torch.randn((nv * per_video, D_RES), generator=g, device=dev).abs() * 0.5).half()
    i3d = (torch.randn((nv * per_video, D_I3D), generator=g, device=dev).abs() * 0.5).half()
    dseg = torch.from_numpy(seg).to(dev)
    sources = [(res, dseg, True), (i3d, dseg, True)]
    n_out, frames = nv * L, int((seg[:, 1] - seg[:, 0]).sum())
    out = {"videos": nv, "clips": L, "rounds": rounds, "device": torch.cuda.get_device_name(dev)}
    for tag, odt, es in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
        # the same feature bits as the launches without the columns, at the timed size
        new, _ = ops.ingest_rows(clip, start, nv, L, L, out_dtype=odt, tef=True)
        old, _ = ops.ingest_rows(clip, start, nv, L, L, out_dtype=odt)
        same_rows = bool(torch.equal(new[:, :, :D], old))
        gat = ops.gather_feature_rows(clip, start, ids, L, L, tef=True, out_dtype=odt, want_len=False)[0]
        same_tef = bool(torch.equal(new[:, :, D:], gat[:, :, D:]))
        del new, old, gat
        new, _ = ops.ingest_pool_rows(sources, start, nv, L, L, out_dtype=odt, tef=True)
        old, _ = ops.ingest_pool_rows(sources, start, nv, L, L, out_dtype=odt)
        same_pool = bool(torch.equal(new[:, :, :D], old))
        del new, old
        torch.cuda.empty_cache()
        rows = time_interleaved({
            "ingest_rows_tef": lambda: ops.ingest_rows(clip, start, nv, L, L, out_dtype=odt, tef=True),
            "ingest_rows": lambda: ops.ingest_rows(clip, start, nv, L, L, out_dtype=odt),
            "gather_feature_rows_tef": lambda: ops.gather_feature_rows(clip, start, ids, L, L, tef=True, out_dtype=odt, want_len=False),
        }, rounds)
        pooled = time_interleaved({
            "ingest_pool_rows_tef": lambda: ops.ingest_pool_rows(sources, start, nv, L, L, out_dtype=odt, tef=True),
            "ingest_pool_rows": lambda: ops.ingest_pool_rows(sources, start, nv, L, L, out_dtype=odt),
        }, rounds)
        rd, prd = n_out * D * 2, frames * D * 2
        out[tag] = {
            "feature_columns_bitwise_equal": {"rows": same_rows, "pooled": same_pool, "endpoint_columns_equal_gather": same_tef},
            "rows": _leg(rows, {"ingest_rows_tef": rd + n_out * (D + 2) * es, "ingest_rows": rd + n_out * D * es,
                                "gather_feature_rows_tef": rd + n_out * (D + 2) * es}),
            "pooled": _leg(pooled, {"ingest_pool_rows_tef": prd + n_out * (D + 2) * es, "ingest_pool_rows": prd + n_out * D * es}),
        }
        torch.cuda.empty_cache()
    return out


def markdown(res, commit):
    nv = res["videos"]
    lines = [
        "# Ingest for *_tef models: the endpoint columns in the ingest launch", "",
        "`python tools/bench_ingest_tef.py`, one process on one %s; commit: %s.  %d videos x %d clips, operands resident in HBM, the "
        "launches of a group interleaved after 3 warm-up rounds, HIP events around each launch; µs: median (min .. max) of %d rounds.  "
        "Bytes: every source row once per clip row that names it, x d x 2, plus n x lmax x (d or d + 2) x 4 (f32) or x 2 (bf16) "
        "written; GB/s = bytes / median." % (res["device"], commit, nv, res["clips"], res["rounds"]), "",
        "## Clip rows: %d f16 columns per clip" % D, "",
        "| output | launch | µs | GB read + written | GB/s | bytes/s over `xml_gather_feature_rows(tef = 1)` |", "|---|---|---|---|---|---|"]
    names = {"ingest_rows_tef": "`xml_ingest_rows_tef`", "ingest_rows": "`xml_ingest_rows`",
             "gather_feature_rows_tef": "`xml_gather_feature_rows(tef = 1)`, ids = arange",
             "ingest_pool_rows_tef": "`xml_ingest_pool_rows_tef`", "ingest_pool_rows": "`xml_ingest_pool_rows`"}
    for tag in ("f32", "bf16"):
        base = res[tag]["rows"]["gather_feature_rows_tef"]["gb_per_s"]
        for k, v in res[tag]["rows"].items():
            lines.append("| %s | %s | %.1f (%.1f .. %.1f) | %.3f | %.0f | %.2f |" % (
                tag, names[k], v["us_median"], v["us_min"], v["us_max"], v["gb"], v["gb_per_s"], v["gb_per_s"] / base))
    lines += ["", "## Pooled rows: ResNet %d + I3D %d f16 frame rows, 4 - 5 per clip, max pooling, both per-source norms and the row norm"
              % (D_RES, D_I3D), "",
              "| output | launch | µs | GB read + written | GB/s | time over `xml_ingest_pool_rows` |", "|---|---|---|---|---|---|"]
    for tag in ("f32", "bf16"):
        base = res[tag]["pooled"]["ingest_pool_rows"]["us_median"]
        for k, v in res[tag]["pooled"].items():
            lines.append("| %s | %s | %.1f (%.1f .. %.1f) | %.3f | %.0f | %.3f |" % (
                tag, names[k], v["us_median"], v["us_min"], v["us_max"], v["gb"], v["gb_per_s"], v["us_median"] / base))
    eq = {tag: res[tag]["feature_columns_bitwise_equal"] for tag in ("f32", "bf16")}
    lines += ["", "Checked in the same process at the timed size, before timing: the feature columns of each `*_tef` launch bitwise equal "
              "to the launch it extends (clip rows f32 / bf16: %s / %s; pooled: %s / %s), and the endpoint columns of "
              "`xml_ingest_rows_tef` bitwise equal to those of `xml_gather_feature_rows(tef = 1)` (%s / %s)." % (
                  eq["f32"]["rows"], eq["bf16"]["rows"], eq["f32"]["pooled"], eq["bf16"]["pooled"],
                  eq["f32"]["endpoint_columns_equal_gather"], eq["bf16"]["endpoint_columns_equal_gather"]), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_tef_timing.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ingest_tef: no GPU -- a timing needs the device")
    result = measure(a.videos, a.rounds)
    with open(a.out, "w") as f:
        f.write(markdown(result, a.commit))
    print(json.dumps(result))
