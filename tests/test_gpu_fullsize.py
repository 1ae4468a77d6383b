"""Full-size parity for the two single-GPU BASELINE configurations.

  C2  (configs[1]) at its STATED shape -- 256 queries x 2 000 videos x 128 clips, video-only (Dv = 3072), fp32, H = 768 --
      HIP path vs the oracle run on the GPU box's host cores: q2c within 1e-4 (north_star's tolerance), top-100 video
      indices and top-200 (video, st, ed) moments identical up to groups of scores tied within rounding.
  C3  (configs[2]) bf16 vs the oracle-pinned fp32 HIP path on 1 000 queries x the full 21 793-video corpus:
      ranking agreement measured by tools/rank_agreement.py and bounded here.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import xml_oracle as O
from oracle.listcmp import tie_aware_equal as _tie_aware_equal
from test_gpu_kernels import DEV
from test_gpu_model import _synthetic_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c2_full_shape_vs_oracle_fp32():
    from tvretrieval_amd import inference as inf
    nq, nv, l, hidden, dv, dq = 256, 2000, 128, 768, 3072, 768
    m, cfg = _synthetic_model("video", hidden, dv, 768, dq, l, torch.float32, seed=11)
    g = torch.Generator().manual_seed(2018)
    lens = torch.randint(24, l + 1, (nv,), generator=g)
    lens[::7] = l                                         # C2 is "x 128 clips": plenty of full-length videos, the rest ragged
    vm = (torch.arange(l)[None] < lens[:, None]).float()
    vf = torch.randn(nv, l, dv, generator=g)
    vf = (vf / (vf.norm(dim=-1, keepdim=True) + 1e-5)) * vm[..., None]          # dataset normalisation, zero padding
    qlens = torch.randint(5, 31, (nq,), generator=g)
    qm = (torch.arange(30)[None] < qlens[:, None]).float()
    qf = torch.randn(nq, 30, dq, generator=g)
    qf = (qf / (qf.norm(dim=-1, keepdim=True) + 1e-5)) * qm[..., None]

    # ---- HIP path, context batches of eval_context_bsz = 200 (xml/config.py:63) like the reference driver
    bs = 200
    with torch.no_grad():
        batches = ((vf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV), None, None) for b in range(0, nv, bs))
        index = inf.build_corpus_index(m, batches, l_ref=l)
        out = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), max_vcmr_video=100, max_before_nms=200)
        # the same shape in exact-rank mode (bf16 K6 as a filter in front of the f32 scores): must be the same lists
        batches = ((vf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV), None, None) for b in range(0, nv, bs))
        xindex = inf.build_corpus_index(m, batches, l_ref=l, exact_filter=True)
        xout = inf.vcmr_search(m, xindex, qf.to(DEV), qm.to(DEV), max_vcmr_video=100, max_before_nms=200)
        del xindex
        # ... and in the split-f16 exact-rank mode (ops.F16S model with the same weights: f16 filter, split-f16 re-score and
        # ConvSE, second tier on the device)
        from tvretrieval_amd import ops as hops
        m16, _ = _synthetic_model("video", hidden, dv, 768, dq, l, hops.F16S, seed=11)
        m16.load_state_dict(m.state_dict())
        batches = ((vf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV), None, None) for b in range(0, nv, bs))
        xindex16 = inf.build_corpus_index(m16, batches, l_ref=l, exact_filter=True)
        assert xindex16.exact.mode == "f16s"
        xout16 = inf.vcmr_search(m16, xindex16, qf.to(DEV), qm.to(DEV), max_vcmr_video=100, max_before_nms=200)
        del xindex16
    torch.cuda.synchronize()

    # ---- oracle on the host cores, same batching (every batch holds a full-length video: same padded-row semantics)
    om = O.OracleXML(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    f1, f2 = [], []
    with torch.no_grad():
        for b in range(0, nv, bs):
            assert int(lens[b:b + bs].max()) == l
            v1, v2, _, _ = om.encode_context(vf[b:b + bs], vm[b:b + bs], None, None)
            f1.append(v1), f2.append(v2)
        f1, f2 = torch.cat(f1), torch.cat(f2)
        q2c, st, ed = om.get_pred_from_raw_query(qf, qm, f1, f2, vm, None, None, None, cross=True)
    err = float((out["q2c"].cpu() - q2c).abs().max())
    assert err <= 1e-4, "q2c max abs err %g" % err

    kv, kn, extra = 100, 200, 24
    gi, gw = out["top_indices"].cpu().numpy().astype(np.int64), out["top_scores"].cpu().numpy()
    gfi, gfs = out["flat_indices"].cpu().numpy().astype(np.int64), out["flat_scores"].cpu().numpy()
    n_vid_diff = n_mom_diff = n_mom_rows = 0
    ll = l * l
    for c in range(0, nq, 32):                            # the (32, 100, 128, 128) product + full sort per chunk
        sl = slice(c, c + 32)
        with torch.no_grad():
            tail = O.vcmr_tail(q2c[sl], st[sl], ed[sl], 20.0, kv, 2, 16, kn + extra)
            ww, wi = torch.topk(torch.exp(20.0 * q2c[sl]), kv + extra, dim=1)
        n_vid_diff += _tie_aware_equal(gi[sl], gw[sl], wi.numpy(), ww.numpy(), kv, 2e-4, "top-100 videos")
        # moments as (video, st, ed) keys: decode each side's flat index through its own video list
        wfi, wfs = tail["flat_indices"].numpy(), tail["flat_scores"].numpy()
        wkey = np.take_along_axis(tail["top_indices"].numpy(), wfi // ll, 1) * ll + wfi % ll
        gkey = np.take_along_axis(gi[sl], np.clip(gfi[sl] // ll, 0, kv - 1), 1) * ll + gfi[sl] % ll
        rows = np.nonzero((np.sort(gi[sl], 1) == np.sort(tail["top_indices"].numpy(), 1)).all(1))[0]
        # (a query whose top-100 SET differs through a rank-100/101 tie has a legitimately different candidate pool)
        n_mom_rows += len(rows)
        assert (gfi[sl][rows] >= 0).all()
        n_mom_diff += _tie_aware_equal(gkey[rows], gfs[sl][rows], wkey[rows], wfs[rows], kn, 5e-4, "top-200 moments")
    assert n_mom_rows >= nq - 1, "video sets differ for %d queries" % (nq - n_mom_rows)      # measured: 0 or 1 of 256
    # exact-rank modes against the SAME oracle lists, same tie-aware rule
    for what, xo in (("f32 re-score", xout), ("split-f16", xout16)):
        xi, xw = xo["top_indices"].cpu().numpy().astype(np.int64), xo["top_scores"].cpu().numpy()
        xfi, xfs = xo["flat_indices"].cpu().numpy().astype(np.int64), xo["flat_scores"].cpu().numpy()
        x_vid = x_mom = x_rows = 0
        for c in range(0, nq, 32):
            sl = slice(c, c + 32)
            with torch.no_grad():
                tail = O.vcmr_tail(q2c[sl], st[sl], ed[sl], 20.0, kv, 2, 16, kn + extra)
                ww, wi = torch.topk(torch.exp(20.0 * q2c[sl]), kv + extra, dim=1)
            x_vid += _tie_aware_equal(xi[sl], xw[sl], wi.numpy(), ww.numpy(), kv, 2e-4, "exact-rank (%s) top-100 videos" % what)
            wfi, wfs = tail["flat_indices"].numpy(), tail["flat_scores"].numpy()
            wkey = np.take_along_axis(tail["top_indices"].numpy(), wfi // ll, 1) * ll + wfi % ll
            xkey = np.take_along_axis(xi[sl], np.clip(xfi[sl] // ll, 0, kv - 1), 1) * ll + xfi[sl] % ll
            rows = np.nonzero((np.sort(xi[sl], 1) == np.sort(tail["top_indices"].numpy(), 1)).all(1))[0]
            x_rows += len(rows)
            x_mom += _tie_aware_equal(xkey[rows], xfs[sl][rows], wkey[rows], wfs[rows], kn, 5e-4,
                                      "exact-rank (%s) top-200 moments" % what)
        print("C2 full shape, exact-rank mode (%s): %d queries failed their certificate; %d / %d video and %d / %d moment "
              "positions swapped in ties" % (what, xo["exact"]["n_fail"], x_vid, nq * kv, x_mom, x_rows * kn))
        assert x_rows >= nq - 1 and x_vid <= 40 and x_mom <= 170, (what, x_rows, x_vid, x_mom)
    print("C2 full shape: q2c max err %.2e; %d / %d video positions and %d / %d moment positions swapped inside tie groups"
          % (err, n_vid_diff, nq * kv, n_mom_diff, n_mom_rows * kn))
    # measured 13 / 25 600 and 56 / 51 000; bounds at ~3x (a regression of an order of magnitude fails)
    assert n_vid_diff <= 40 and n_mom_diff <= 170, (n_vid_diff, n_mom_diff)


def test_c3_slice_exact_rank_split_f16_vs_oracle():
    """configs[2]'s model (video + subtitles, cross attention, merged ConvSE, H = 768, Dv = 3072) on a slice the oracle
    finishes in a minute -- 160 queries x 1 200 videos x 128 clips, ragged -- in the split-f16 exact-rank mode (ops.F16S model:
    every projection, the candidate re-score and ConvSE on the 16-bit MFMA pipe; bf16 filter with 160 candidates so that it
    really filters) against the ORACLE run on the host cores: re-scored cosines within 1e-6, top-100 videos and top-200
    (video, st, ed) moments identical up to groups of scores tied within rounding -- the same rule and bounds the f32 HIP path
    is held to at configs[1]'s shape."""
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ops as hops
    nq, nv, l, hidden, dv, ds_, dq = 160, 1200, 128, 768, 3072, 768, 768
    m16, cfg = _synthetic_model("video_sub", hidden, dv, ds_, dq, l, hops.F16S, seed=21)
    g = torch.Generator().manual_seed(2019)
    lens = torch.randint(24, l + 1, (nv,), generator=g)
    lens[::5] = l
    vm = (torch.arange(l)[None] < lens[:, None]).float()

    def rows(n, ll, d, mask):
        x = torch.randn(n, ll, d, generator=g)
        return (x / (x.norm(dim=-1, keepdim=True) + 1e-5)) * mask[..., None]
    vf, sf = rows(nv, l, dv, vm), rows(nv, l, ds_, vm)
    qlens = torch.randint(5, 31, (nq,), generator=g)
    qm = (torch.arange(30)[None] < qlens[:, None]).float()
    qf = rows(nq, 30, dq, qm)
    bs = 200
    with torch.no_grad():
        batches = [(vf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV), sf[b:b + bs].to(DEV), vm[b:b + bs].to(DEV))
                   for b in range(0, nv, bs)]
        index = inf.build_corpus_index(m16, batches, l_ref=l, exact_filter=True)
        assert index.exact.mode == "f16s"
        index.exact.n_candidates = 160
        out = inf.vcmr_search(m16, index, qf.to(DEV), qm.to(DEV), max_vcmr_video=100, max_before_nms=200)
    torch.cuda.synchronize()
    om = O.OracleXML(cfg, {k: v.detach().cpu() for k, v in m16.state_dict().items()})
    f1v, f2v, f1s, f2s = [], [], [], []
    with torch.no_grad():
        for b in range(0, nv, bs):
            assert int(lens[b:b + bs].max()) == l
            o = om.encode_context(vf[b:b + bs], vm[b:b + bs], sf[b:b + bs], vm[b:b + bs])
            f1v.append(o[0]), f2v.append(o[1]), f1s.append(o[2]), f2s.append(o[3])
        q2c, st, ed = om.get_pred_from_raw_query(qf, qm, torch.cat(f1v), torch.cat(f2v), vm, torch.cat(f1s), torch.cat(f2s), vm,
                                                 cross=True)
    cand = torch.gather(q2c, 1, out["exact"]["cand_indices"].cpu().long())
    err = float((out["exact"]["cand_scores"].cpu() - cand).abs().max())
    assert err <= 2e-6, "re-scored cosines vs oracle: %g" % err
    kv, kn, extra = 100, 200, 24
    gi, gw = out["top_indices"].cpu().numpy().astype(np.int64), out["top_scores"].cpu().numpy()
    gfi, gfs = out["flat_indices"].cpu().numpy().astype(np.int64), out["flat_scores"].cpu().numpy()
    ll = l * l
    n_vid = n_mom = n_rows = 0
    for c in range(0, nq, 32):
        sl = slice(c, c + 32)
        with torch.no_grad():
            tail = O.vcmr_tail(q2c[sl], st[sl], ed[sl], 20.0, kv, 2, 16, kn + extra)
            ww, wi = torch.topk(torch.exp(20.0 * q2c[sl]), kv + extra, dim=1)
        n_vid += _tie_aware_equal(gi[sl], gw[sl], wi.numpy(), ww.numpy(), kv, 2e-4, "split-f16 exact-rank top-100 videos")
        wfi, wfs = tail["flat_indices"].numpy(), tail["flat_scores"].numpy()
        wkey = np.take_along_axis(tail["top_indices"].numpy(), wfi // ll, 1) * ll + wfi % ll
        gkey = np.take_along_axis(gi[sl], np.clip(gfi[sl] // ll, 0, kv - 1), 1) * ll + gfi[sl] % ll
        rws = np.nonzero((np.sort(gi[sl], 1) == np.sort(tail["top_indices"].numpy(), 1)).all(1))[0]
        n_rows += len(rws)
        n_mom += _tie_aware_equal(gkey[rws], gfs[sl][rws], wkey[rws], wfs[rws], kn, 5e-4, "split-f16 exact-rank top-200 moments")
    print("C3-model slice, split-f16 exact-rank mode vs oracle: re-scored cosines within %.1e; %d / %d video and %d / %d moment "
          "positions swapped inside tie groups; %d certificates failed" % (err, n_vid, nq * kv, n_mom, n_rows * kn,
                                                                         out["exact"]["n_fail"]))
    assert n_rows >= nq - 1 and n_vid <= 40 and n_mom <= 170, (n_rows, n_vid, n_mom)


def test_c3_bf16_vs_fp32_rank_agreement():
    """Bounds on how far the bf16 lists move from the fp32 lists (full corpus, 1 000 queries).  The measured values are
    committed in profiles/r0*_bf16_vs_fp32_rank_agreement.json; the bounds here sit 0.4-0.8 points below them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rank_agreement
    res = rank_agreement.run(1000, 21793)
    print(res)
    for part in ("pipeline_bf16", "k6_only_bf16"):
        r = res[part]
        assert r["q2c_max_abs_diff"] < 2e-2, (part, r)
        assert r["videos_top100_overlap"] >= BOUNDS[part]["videos_top100_overlap"], (part, r)
        assert r["videos_top10_overlap"] >= BOUNDS[part]["videos_top10_overlap"], (part, r)
        assert r["videos_top1_same"] >= BOUNDS[part]["videos_top1_same"], (part, r)
        assert r["moment_top1_iou_ge_0.7"] >= BOUNDS[part]["moment_top1_iou_ge_0.7"], (part, r)


BOUNDS = {      # the run is deterministic; measured (profiles/r02_bf16_vs_fp32_rank_agreement.json, same on every box):
    "pipeline_bf16": {"videos_top100_overlap": 0.984, "videos_top10_overlap": 0.981, "videos_top1_same": 0.972,
                      "moment_top1_iou_ge_0.7": 0.952},                # pipeline 0.9869 / 0.9841 / 0.980 / 0.961
    "k6_only_bf16": {"videos_top100_overlap": 0.989, "videos_top10_overlap": 0.986, "videos_top1_same": 0.98,
                     "moment_top1_iou_ge_0.7": 0.972},                 # k6_only 0.9924 / 0.9916 / 0.986 / 0.979
}


@pytest.mark.parametrize("mode", ["f16s", "f32"])
def test_c3_exact_rank_mode_gives_the_fp32_lists(mode):
    """configs[2] in exact-rank mode -- "f16s": f16 K6 as a filter + split-f16 re-score / ConvSE on an ops.F16S model
    (tests/test_gpu_split16.py); "f32": round 3's bf16 filter + exact-f32 re-score (tests/test_gpu_exact.py) -- against the
    plain f32 HIP path on 1 000 queries x the full 21 793-video corpus: EQUALITY, not overlap floors -- every top-100
    video position and every top-192 (video, st, ed) position identical except inside groups of scores tied to f32
    rounding (1e-6 on the cosine) -- position 0 included: the top-1 video is identical for every query, the top-1 moment for
    all but at most two in a thousand, whose two best moments tie to f32 rounding (which of two such paths the plain f32 run
    takes moves with every last-bit change of the encoder, e.g. which batches run the LayerNorm-epilogue GEMM)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_exact
    res = bench_exact.run(1000, 21793, "perturbed", 1000, mode=mode)
    print(res)
    v = res["vs_plain_f32"]
    assert v["video_positions_really_different"] == 0 and v["moment_positions_really_different"] == 0, v
    # a differing top-1 moment is inside an f32 tie: moment_positions_really_different comes from
    # tools/bench_exact.py::tie_aware_diff, which walks EVERY differing position of the first 192, position 0 included, and
    # counts it as "really different" unless the entry sits in the other list with a score within the tie tolerance -- so
    # the line above already is the per-query tie check for the (at most 0.2 %) differing top-1s
    assert v["top1_video_same"] == 1.0 and v["top1_moment_same"] >= 0.998, v
    if mode == "f32":      # same kernels behind the filter as the plain path: almost nothing may move
        assert v["video_positions_swapped_in_f32_ties"] <= 50 and v["moment_positions_swapped_in_f32_ties"] <= 100, v
        assert v["queries_with_identical_top100_order"] >= 990, v
    else:                  # f32-GRADE arithmetic (2^-22 per operand): neighbours closer than that swap; measured 73 / 134+76
        assert v["video_positions_swapped_in_f32_ties"] <= 200 and v["moment_positions_swapped_in_f32_ties"] <= 600, v
        assert v["queries_with_identical_top100_order"] >= 940, v
        assert v["rescored_vs_f32_scores_max_abs"] <= 1e-6, v
        assert v["moment_score_rel_dev_same_position"]["max"] <= 5e-4, v     # (the bound both paths are held to against the oracle)
    c = res["certificate"]
    assert c["fail_rate"] <= 0.05, c                                   # measured 0.1 %: the fallback stays rare
    assert c["filter_abs_err_max"] < c["eps_mean"], c                 # the bound really bounds what the filter did


def test_c3_exact_rank_mode_vs_the_oracle_on_the_whole_corpus():
    """configs[2] in exact-rank mode against the CPU ORACLE directly (one hop, not via the f32 HIP path): 200 queries x the
    full 21 793-video corpus.  The HIP side is the whole product pass (ops.F16S model: split-f16 query encoder, bf16 K6
    filter, split-f16 re-score + certificate + second tier, split-f16 ConvSE, K9).  The oracle side is the reference
    formulation on the host cores -- query encoder, both (Nq, Nv, L) contractions, ConvSE, softmax, the (100, L, L) product
    and the full sort (xml/model_xml.py:291-295,436-502, xml/inference.py:317-386) -- on the context features the index was
    built from (the f32 outputs of the same HIP encoder, fetched batch by batch; the context encoder's own parity is
    tests/test_gpu_model.py's).  Same tie-aware rule and bounds as test_c2_full_shape_vs_oracle_fp32."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import bench
    import rank_agreement
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ops
    from tvretrieval_amd.model_xml import XML
    _, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
    nq = 200
    cfg = bench.model_config(hidden, dv, ds, dq, ctx_mode, l)
    torch.manual_seed(0)
    model = rank_agreement.perturb_weights(XML(cfg, compute_dtype=ops.F16S)).to(DEV).eval()
    qf, qm = bench.synth_queries(nq, dq, torch.device(DEV))
    host = dict(v1=[], v2=[], s1=[], s2=[])
    with torch.no_grad():
        raw = list(bench.context_batches(0, nv, l, dv, ds, True, True, torch.device(DEV)))
        index = inf.build_corpus_index(model, iter(raw), n_total=nv, l_ref=l, n_videos=nv, exact_filter=True)
        assert index.exact.mode == "f16s"
        for b in raw:           # the encoder is deterministic per batch: these are the rows the index was built from
            for k_, t in zip(("v1", "v2", "s1", "s2"), model.encode_context(*b)):
                host[k_].append(t.float().cpu())
        del raw
        out = inf.vcmr_search(model, index, qf, qm, max_vcmr_video=100, max_before_nms=200)
        assert out["exact"]["n_full_rows"] == 0
        del index
    torch.cuda.synchronize()
    f = {k_: torch.cat(v) for k_, v in host.items()}
    del host
    ones = torch.ones(nv, l)
    om = O.OracleXML(cfg, {k_: v.detach().float().cpu() for k_, v in model.state_dict().items()})
    with torch.no_grad():
        q2c, st, ed = om.get_pred_from_raw_query(qf.cpu(), qm.cpu(), f["v1"], f["v2"], ones, f["s1"], f["s2"], ones, cross=True)
    del f
    kv, kn, extra = 100, 200, 24
    ll = l * l
    gi, gw = out["top_indices"].cpu().numpy().astype(np.int64), out["top_scores"].cpu().numpy()
    gfi, gfs = out["flat_indices"].cpu().numpy().astype(np.int64), out["flat_scores"].cpu().numpy()
    n_vid_diff = n_mom_diff = n_rows = 0
    for c in range(0, nq, 25):
        sl = slice(c, c + 25)
        with torch.no_grad():
            tail = O.vcmr_tail(q2c[sl], st[sl], ed[sl], 20.0, kv, 2, 16, kn + extra)
            ww, wi = torch.topk(torch.exp(20.0 * q2c[sl]), kv + extra, dim=1)
        n_vid_diff += _tie_aware_equal(gi[sl], gw[sl], wi.numpy(), ww.numpy(), kv, 2e-4, "top-100 videos")
        wfi, wfs = tail["flat_indices"].numpy(), tail["flat_scores"].numpy()
        wkey = np.take_along_axis(tail["top_indices"].numpy(), wfi // ll, 1) * ll + wfi % ll
        gkey = np.take_along_axis(gi[sl], np.clip(gfi[sl] // ll, 0, kv - 1), 1) * ll + gfi[sl] % ll
        rows = np.nonzero((np.sort(gi[sl], 1) == np.sort(tail["top_indices"].numpy(), 1)).all(1))[0]
        n_rows += len(rows)
        assert (gfi[sl][rows] >= 0).all()
        n_mom_diff += _tie_aware_equal(gkey[rows], gfs[sl][rows], wkey[rows], wfs[rows], kn, 5e-4, "top-200 moments")
        assert (gi[sl][:, 0] == wi.numpy()[:, 0]).all(), "top-1 video"
    print("exact-rank vs oracle, %d queries x %d videos: %d video / %d moment positions swapped inside ties; %d queries "
          "with the oracle's top-100 set" % (nq, nv, n_vid_diff, n_mom_diff, n_rows))
    assert n_rows >= nq - 2, "video sets differ for %d queries" % (nq - n_rows)      # (a rank-100/101 tie at f32 rounding)
    assert n_vid_diff <= 0.01 * nq * kv and n_mom_diff <= 0.02 * n_rows * kn, (n_vid_diff, n_mom_diff)


@pytest.mark.parametrize("mode", ["bf16", "exact_f16s"])
def test_c4_eight_shard_walk_equals_the_single_pass(mode):
    """BASELINE configs[3] at its own size on ONE GPU: the 21 793-video corpus cut into the 8 `shard_range` slices an
    8-GPU node would hold, each shard walked in turn through the rank's side of the pass (dist._local_scores_topk: local
    K6 + local top-100, global ids), the eight lists laid out the way the grouped receive of xml_rccl_topk_by_owner leaves
    them, merged by the kernels that run behind the wire (xml_merge_shard_topk), and the owner's K7 / K9 on the merged
    list -- for every query owner.  The reference takes moments only from the GLOBAL top-100 videos of a query
    (xml/inference.py:347-348,365-367): the merged lists must be the single pass's lists BIT FOR BIT (scores, ids, order),
    for the query-owner rerank and (bf16) for the video-owner scheme whose per-rank moment lists are merged the same way.
    mode "exact_f16s": every shard is an exact-rank index of an ops.F16S model (f32-grade local lists)."""
    sys.path.insert(0, ROOT)
    import bench
    from tvretrieval_amd import dist as xd
    from tvretrieval_amd import inference as inf
    from tvretrieval_amd import ops
    from tvretrieval_amd.model_xml import XML
    nq, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["c3"]
    world, k, n_out = 8, 100, 200
    dev = torch.device(DEV)
    exact = mode != "bf16"
    torch.manual_seed(0)
    model = XML(bench.model_config(hidden, dv, ds, dq, ctx_mode, l),
                compute_dtype=ops.F16S if exact else torch.bfloat16).to(dev).eval()
    kw = dict(exact_filter=True) if exact else {}
    qf, qm = bench.synth_queries(nq, dq, dev)
    ranges = [xd.shard_range(nv, r, world, align=bench.SHARD_ALIGN) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == nv and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    with torch.no_grad():
        # phase 0: every owner encodes its query slice (dist.encode_queries_sharded), the all-gather is a concatenation
        parts = [inf.stage_query_vectors(model, qf[lo:hi].contiguous(), qm[lo:hi].contiguous())
                 for lo, hi, _ in (xd.query_slice(nq, r, world) for r in range(world))]
        qvec = {m: torch.cat([p[m] for p in parts]).contiguous() for m in parts[0]}
        # The single pass it must equal: ONE index over the whole corpus encoded in the bench's own batches of 2 048 videos
        # (the shards encode 2 724-video ranges in their own batches), one vcmr_search over all 10 000 queries encoded as ONE
        # batch (the owners encode 1 250 each).  The encoders' bits do not depend on the batch
        # (test_index_bits_do_not_depend_on_the_context_batch), so nothing is fed across: both sides run end to end.
        full = inf.build_corpus_index(model, bench.context_batches(0, nv, l, dv, ds, True, True, dev), n_total=nv, l_ref=l, **kw)
        want = inf.vcmr_search(model, full, qf, qm, max_vcmr_video=k, max_before_nms=n_out)
        if exact:
            assert want["exact"]["n_fail"] <= nq // 20
        whole = inf.stage_query_vectors(model, qf, qm)       # the same vectors from ONE batch of 10 000: bit for bit
        for m in qvec:
            assert torch.equal(whole[m], qvec[m]), (m, float((whole[m].float() - qvec[m].float()).abs().max()))
        # phase 1 on every shard in turn
        shards, loc = [], []
        for r in range(world):
            lo, hi = ranges[r]
            idx = inf.build_corpus_index(model, bench.context_batches(lo, hi, l, dv, ds, True, True, dev), video_offset=lo,
                                         n_total=nv, l_ref=l, **kw)
            assert idx.n_videos == hi - lo
            _, (loc_s, loc_i) = xd._local_scores_topk(idx, qvec, k, ops)
            loc.append((loc_s, loc_i))
            shards.append(idx if not exact else None)       # (the video-owner leg below is bf16 only)
        # the owner's merge behind the wire + the owner's K7 / K9 against the corpus-wide feat2 copy
        full.feat2_all, full.mask_all = full.feat2, full.mask
        top_w, top_gid, fs, fi = [], [], [], []
        for o in range(world):
            q_lo, q_hi, per = xd.query_slice(nq, o, world)
            recv_s = torch.stack([s[q_lo:q_hi] for s, _ in loc]).contiguous()              # [p][row][c]
            recv_i = torch.stack([i[q_lo:q_hi] for _, i in loc]).contiguous()
            own_w, own_gid = ops.merge_shard_topk(recv_s, recv_i, k, alpha=20.0)
            st, ed = inf.stage_span_probs(model, full, {m: v[q_lo:q_hi] for m, v in qvec.items()}, own_gid, ops, replicated=True)
            s_, f_ = ops.moment_topk(st, ed, own_w, full.l_ref, 2, 16, n_out)
            top_w.append(own_w), top_gid.append(own_gid), fs.append(s_), fi.append(f_)
        top_w, top_gid, fs, fi = (torch.cat(t) for t in (top_w, top_gid, fs, fi))
        torch.cuda.synchronize()
        assert torch.equal(top_gid, want["top_indices"]), "global top-100 video ids differ from the single pass"
        assert torch.equal(top_w, want["top_scores"]), "global top-100 weights differ from the single pass"
        assert torch.equal(fi, want["flat_indices"]), "top-200 moments (query-owner rerank) differ from the single pass"
        assert torch.equal(fs, want["flat_scores"])
        if exact:
            return
        # video-owner scheme: every rank reranks the global top-100 videos IT holds; the per-rank top-200 lists (flat
        # indices in the global slot order) are merged by the same kernels (score desc, flat asc)
        loc_m = []
        for r in range(world):
            a, b = xd.video_owner_local_moments(model, shards[r], qvec, top_w, top_gid, n_out, 2, 16, ops)
            loc_m.append((a.contiguous(), xd.moment_merge_payload(b)))
        ms, mi = [], []
        for o in range(world):
            q_lo, q_hi, per = xd.query_slice(nq, o, world)
            a, b = ops.merge_shard_topk(torch.stack([s[q_lo:q_hi] for s, _ in loc_m]).contiguous(),
                                        torch.stack([i[q_lo:q_hi] for _, i in loc_m]).contiguous(), n_out, alpha=0.0)
            ms.append(a), mi.append(torch.where(a > 0, b, torch.full_like(b, -1)))
        ms, mi = torch.cat(ms), torch.cat(mi)
        torch.cuda.synchronize()
        assert torch.equal(mi, want["flat_indices"]), "top-200 moments (video-owner scheme) differ from the single pass"
        assert torch.equal(ms, want["flat_scores"])


def test_tvr_val_shape_vs_oracle_fp32():
    """The reference's AS-TRAINED shape (xml/config.py:60-63,86-88,143: hidden 256, max_ctx_l 100; TVR val: 2 179 videos with
    their real clip counts, resnet_i3d + subtitles, cross attention, merged ConvSE) against the oracle on the GPU box's host
    cores, fp32: the WHOLE corpus (length-bucketed K6 image, ragged K7 / K9 rows -- the paths only this shape exercises at
    size) x 640 of the 10 895 queries (the oracle materialises (Nq, Nv, L) like the reference: 640 queries = 1.1 GB).
    q2c within 1e-4, top-100 videos and top-200 (video, st, ed) identical up to groups of scores tied within rounding."""
    sys.path.insert(0, ROOT)
    import bench
    from tvretrieval_amd import inference as inf
    _, nv, l, hidden, dv, ds, dq, ctx_mode, _ = bench.WORKLOADS["tvr_val"]
    nq = 640
    m, cfg = _synthetic_model("video_sub", hidden, dv, ds, dq, l, torch.float32, seed=23)
    lens = bench.real_clip_counts(nv, l)
    g = torch.Generator().manual_seed(2018)
    vm = (torch.arange(l)[None] < lens[:, None]).float()
    norm = lambda x: x / (x.norm(dim=-1, keepdim=True) + 1e-5)                   # noqa: E731
    vf = norm(torch.randn(nv, l, dv, generator=g)) * vm[..., None]
    sf = norm(torch.randn(nv, l, ds, generator=g)) * vm[..., None]
    qlens = torch.randint(5, 31, (nq,), generator=g)
    qm = (torch.arange(30)[None] < qlens[:, None]).float()
    qf = norm(torch.randn(nq, 30, dq, generator=g)) * qm[..., None]
    bs = 200                                                                     # eval_context_bsz, xml/config.py:63
    om = O.OracleXML(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        # both sides encode batch by batch at the batch's own padded length and zero-fill beyond it (cat_tensor,
        # xml/inference.py:71-87): the padded-row semantics the 5-tap filter can see
        batches, f1v, f2v, f1s, f2s = [], [], [], [], []
        for b in range(0, nv, bs):
            lb = int(lens[b:b + bs].max())
            batches.append((vf[b:b + bs, :lb].to(DEV), vm[b:b + bs, :lb].to(DEV), sf[b:b + bs, :lb].to(DEV), vm[b:b + bs, :lb].to(DEV)))
            v1, v2, s1, s2 = om.encode_context(vf[b:b + bs, :lb], vm[b:b + bs, :lb], sf[b:b + bs, :lb], vm[b:b + bs, :lb])
            pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, l - lb))           # noqa: E731
            f1v.append(pad(v1)), f2v.append(pad(v2)), f1s.append(pad(s1)), f2s.append(pad(s2))
        index = inf.build_corpus_index(m, batches, l_ref=l)
        assert index.ragged and getattr(index.feat1n["video"], "plan", None) is not None      # the ragged paths are the ones on
        out = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), max_vcmr_video=100, max_before_nms=200)
        torch.cuda.synchronize()
        f1v, f2v, f1s, f2s = (torch.cat(t) for t in (f1v, f2v, f1s, f2s))
        q2c, st, ed = om.get_pred_from_raw_query(qf, qm, f1v, f2v, vm, f1s, f2s, vm, cross=True)
    err = float((out["q2c"].cpu() - q2c).abs().max())
    assert err <= 1e-4, "q2c max abs err %g" % err
    kv, kn, extra = 100, 200, 24
    gi, gw = out["top_indices"].cpu().numpy().astype(np.int64), out["top_scores"].cpu().numpy()
    gfi, gfs = out["flat_indices"].cpu().numpy().astype(np.int64), out["flat_scores"].cpu().numpy()
    n_vid = n_mom = n_rows = 0
    ll = l * l
    for c in range(0, nq, 32):
        sl = slice(c, c + 32)
        with torch.no_grad():
            tail = O.vcmr_tail(q2c[sl], st[sl], ed[sl], 20.0, kv, 2, 16, kn + extra)
            ww, wi = torch.topk(torch.exp(20.0 * q2c[sl]), kv + extra, dim=1)
        n_vid += _tie_aware_equal(gi[sl], gw[sl], wi.numpy(), ww.numpy(), kv, 2e-4, "top-100 videos")
        wfi, wfs = tail["flat_indices"].numpy(), tail["flat_scores"].numpy()
        wkey = np.take_along_axis(tail["top_indices"].numpy(), wfi // ll, 1) * ll + wfi % ll
        gkey = np.take_along_axis(gi[sl], np.clip(gfi[sl] // ll, 0, kv - 1), 1) * ll + gfi[sl] % ll
        rows = np.nonzero((np.sort(gi[sl], 1) == np.sort(tail["top_indices"].numpy(), 1)).all(1))[0]
        n_rows += len(rows)
        assert (gfi[sl][rows] >= 0).all()
        n_mom += _tie_aware_equal(gkey[rows], gfs[sl][rows], wkey[rows], wfs[rows], kn, 5e-4, "top-200 moments")
    print("tvr_val shape, fp32: q2c max err %.2e; %d / %d video and %d / %d moment positions swapped inside tie groups; "
          "%d of %d queries compared on moments" % (err, n_vid, nq * kv, n_mom, n_rows * kn, n_rows, nq))
    assert n_rows >= nq - 3 and n_vid <= 100 and n_mom <= 400, (n_rows, n_vid, n_mom)
