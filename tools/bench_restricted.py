"""Timing of the restricted search (video_allow): K8 with and without an allow mask at the headline shape, how many rows
leave the one-pass pre-filter for the multi-pass fallback under each mask, and the whole pass with a shared 1/6 mask.
GPU box only.

usage: python tools/bench_restricted.py [--rows 10000] [--n 21793] [--k 100] [--reps 21] [--parent-lib PATH] [--no-pass]

  --parent-lib PATH   a libxmlhip.so built from the parent commit: its xml_topk_rows is timed in the same process,
                      alternating with this tree's (the unmasked entry is held to it)
  --no-pass           skip the whole-pass leg (it encodes the headline corpus first)

Every figure is the median of --reps launches between HIP events after two warm-up launches; min .. max is the spread.
The fallback counts restate the kernel's own criterion (topk.hip: r-th largest allowed key of the first 2 048 columns,
candidates >= it counted over the row, accepted when k <= count <= 1024) in torch on the same data: "unscaled" is r as the
unmasked kernel chooses it with the disallowed sample columns counting as below everything, "scaled" is r scaled by the
allowed share of the sample, which is what xml_topk_rows_allowed does."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tvretrieval_amd import _lib, inference as inf, ops  # noqa: E402

SAMPLE, CAND_CAP = 2048, 1024


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


def k6_like_scores(rows, n):
    """Rows shaped like K6's output: the max over clips of cosines (positive, a handful of distinct exponents)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.empty(rows, n, device="cuda")
    for b in range(0, rows, 1000):
        e = min(rows, b + 1000)
        x[b:e] = (torch.randn(e - b, n, 16, device="cuda", generator=g) * 0.036).max(-1)[0]
    return x


def fallback_rows(x, allowed, k, scaled):
    """Rows of x (rows, n) that the pre-filter of topk.hip hands to the multi-pass path under `allowed` (1 | rows, n) bool."""
    rows, n = x.shape
    if n < 2 * SAMPLE:
        return rows
    n_fall = 0
    for b in range(0, rows, 500):
        xs = x[b:b + 500]
        al = allowed if allowed.shape[0] == 1 else allowed[b:b + 500]
        al = al.expand(xs.shape[0], n)
        a_n, a_s = al.sum(1), al[:, :SAMPLE].sum(1)
        k_sel = torch.clamp(a_n, max=k)
        if scaled:
            r = (3 * k_sel * a_s + a_n - 1) // a_n.clamp_min(1) + 2
            usable = (r <= SAMPLE // 8) & (r <= a_s) & (k_sel > 0)
        else:
            r = torch.full_like(a_n, (3 * k * SAMPLE + n - 1) // n + 2)
            usable = (r <= SAMPLE // 8) & (k_sel > 0)
        masked = torch.where(al, xs, torch.full((), -float("inf"), device=x.device))       # disallowed: below every real key
        samp = torch.sort(masked[:, :SAMPLE], dim=1, descending=True)[0]
        t0 = torch.gather(samp, 1, (r.clamp(1, SAMPLE) - 1)[:, None])                     # the r-th largest sample key
        cnt = (al & (masked >= t0)).sum(1)              # (r beyond the allowed sample columns: every allowed column)
        ok = usable & (cnt >= k_sel) & (cnt <= CAND_CAP)
        n_fall += int((~ok & (k_sel > 0)).sum())
    return n_fall


def parent_topk(path):
    lib = ctypes.CDLL(path)
    name = "xml_topk_rows"
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]

    def call(x, k, alpha, vals, idx):
        rows, n = x.shape
        _lib.check(fn(ops._p(x), x.stride(0), None, ops._p(vals), ops._p(idx), rows, n, k, float(alpha), None, 0,
                      ops._stream()), "parent xml_topk_rows")
    return call


def k8_leg(args):
    rows, n, k = args.rows, args.n, args.k
    x = k6_like_scores(rows, n)
    print("K8 at %d x %d, k = %d, alpha = 20 (scores: %.0f MB, allow words: %.1f MB per-row / %.1f KB shared)"
          % (rows, n, k, rows * n * 4 / 1e6, rows * ((n + 31) // 32) * 4 / 1e6, ((n + 31) // 32) * 4 / 1e3))
    base = timed(lambda: ops.topk_rows(x, k, alpha=20.0), args.reps)
    print("  xml_topk_rows, this tree                 : %s" % fmt(base))
    if args.parent_lib:
        par = parent_topk(args.parent_lib)
        vals, idx = torch.empty((rows, k), device="cuda"), torch.empty((rows, k), dtype=torch.int32, device="cuda")
        pairs = []
        for _ in range(3):             # alternating: parent, this tree, parent, ...
            pairs.append((timed(lambda: par(x, k, 20.0, vals, idx), args.reps), timed(lambda: ops.topk_rows(x, k, alpha=20.0), args.reps)))
        for p, t in pairs:
            print("  alternating  parent %s | this tree %s" % (fmt(p), fmt(t)))
        v2, i2 = ops.topk_rows(x, k, alpha=20.0)
        par(x, k, 20.0, vals, idx)
        print("  parent and this tree agree bit for bit   : %s" % bool(torch.equal(vals, v2) and torch.equal(idx, i2)))
    g = torch.Generator(device="cuda").manual_seed(1)
    masks = {
        "all ones (shared row)": torch.ones((1, n), dtype=torch.bool, device="cuda"),
        "shared random 1/6": torch.rand((1, n), device="cuda", generator=g) < 1 / 6,
        "per-query random 1/6": torch.rand((rows, n), device="cuda", generator=g) < 1 / 6,
        "only columns >= 2048 (shared)": (torch.arange(n, device="cuda") >= SAMPLE)[None, :],
    }
    for name, al in masks.items():
        bits = inf.pack_video_allow(al)
        t = timed(lambda: ops.topk_rows(x, k, alpha=20.0, allow=bits), args.reps)
        print("  xml_topk_rows_allowed, %-30s: %s = %.2f x unmasked; fallback rows of %d: %d with r unscaled, %d with r scaled"
              % (name, fmt(t), t[0] / base[0], rows, fallback_rows(x, al, k, False), fallback_rows(x, al, k, True)), flush=True)


def pass_leg(args):
    import bench
    nq, nv, l, hidden, dv, ds, dq, ctx_mode, dtname = bench.WORKLOADS["c3"]
    be = bench.HipBackend(0)
    torch.manual_seed(0)
    model = be.make_model(bench.model_config(hidden, dv, ds, dq, ctx_mode, l), torch.bfloat16)
    with torch.no_grad():
        index = inf.build_corpus_index(model, bench.context_batches(0, nv, l, dv, ds, model.use_video, model.use_sub, be.device),
                                       l_ref=l, n_total=nv)
        qf, qm = bench.synth_queries(nq, dq, be.device)
        g = torch.Generator(device="cuda").manual_seed(2)
        bits = inf.pack_video_allow(torch.rand((1, nv), device="cuda", generator=g) < 1 / 6)
        n_tok = int(qm.sum().item())
        free = timed(lambda: inf.vcmr_search(model, index, qf, qm, n_valid_tokens=n_tok), args.pass_reps)
        res = timed(lambda: inf.vcmr_search(model, index, qf, qm, n_valid_tokens=n_tok, video_allow=bits), args.pass_reps)
        free2 = timed(lambda: inf.vcmr_search(model, index, qf, qm, n_valid_tokens=n_tok), args.pass_reps)
    print("whole pass (vcmr_search, bf16, %d queries x %d videos), %d passes each:" % (nq, nv, args.pass_reps))
    print("  unrestricted            : %s" % fmt(free))
    print("  shared random 1/6 mask  : %s = %.3f x unrestricted" % (fmt(res), res[0] / free[0]))
    print("  unrestricted, again     : %s" % fmt(free2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--n", type=int, default=21793)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--pass-reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-pass", action="store_true")
    args = ap.parse_args()
    k8_leg(args)
    if not args.no_pass:
        pass_leg(args)


if __name__ == "__main__":
    main()
