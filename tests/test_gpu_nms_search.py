"""Temporal NMS on the device, end to end: the three search entry points with nms_thd / opt.nms_on_device return exactly what
host NMS (postproc.post_processing_*_nms) makes of their own pre-NMS records, and leave the default path untouched."""
import argparse
import copy

import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model
from tvretrieval_amd import inference as inf
from tvretrieval_amd import ops, postproc
from tvretrieval_amd.results import MOMENT_DTYPE, MomentResults

pytestmark = pytest.mark.gpu

NV, NQ, L, KV, N_MOM, CLIP = 12, 9, 24, 5, 60, 1.5
KW = dict(max_vcmr_video=KV, max_before_nms=N_MOM)
_WORLD = {}


def _world():
    """The small two-stream model: H = 128, 12 videos of at most 24 clips, 9 queries; built once."""
    if _WORLD:
        return _WORLD
    m, cfg = _synthetic_model("video_sub", 128, 256, 128, 128, L, torch.float32, seed=61)
    rng = np.random.default_rng(62)
    lens = rng.integers(8, L + 1, NV)
    lens[0] = L
    vf, vm = _feats(NV, lens, 256, 63)
    sf, sm = _feats(NV, lens, 128, 64)
    qlens = np.concatenate([[30], rng.integers(2, 31, NQ - 1)])
    qf, qm = _feats(NQ, qlens, 128, 65)
    with torch.no_grad():
        index = inf.build_corpus_index(m, [(vf.to(DEV), vm.to(DEV), sf.to(DEV), sm.to(DEV))])
    meta2vid = torch.from_numpy((np.arange(NV) * 7 + 3).astype(np.int32)).to(DEV)
    gt = torch.from_numpy(rng.integers(0, NV, NQ).astype(np.int32)).to(DEV)
    _WORLD.update(m=m, index=index, qf=qf.to(DEV), qm=qm.to(DEV), qlens=qlens, meta2vid=meta2vid, gt=gt)
    return _WORLD


def _results(rec_dev, cnt_dev, scale=None):
    rec = rec_dev.cpu().numpy().view(MOMENT_DTYPE)[..., 0]
    n = rec.shape[0]
    return MomentResults.from_records(list(range(n)), [""] * n, rec, cnt_dev.cpu().numpy(), scale=scale)


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got.count, want.count, err_msg=what + ": counts")
    for col in ("vid", "st", "ed", "score"):
        np.testing.assert_array_equal(getattr(got, col), getattr(want, col), err_msg="%s: %s" % (what, col))


def _check_nms_outputs(out, prefix, task, thd, max_after, scale, what):
    """out[prefix + nms_*] == host NMS of out[prefix + records]: index, count, records gathered bitwise."""
    raw = _results(out[prefix + "records"], out[prefix + "record_count"], scale=scale)
    fn = postproc.post_processing_vcmr_nms if task == "VCMR" else postproc.post_processing_svmr_nms
    want = fn(raw.copy(), nms_thd=thd, max_before_nms=N_MOM, max_after_nms=max_after)
    idx, cnt = out[prefix + "nms_index"].cpu().numpy(), out[prefix + "nms_count"].cpu().numpy()
    _assert_same(raw.take(idx, cnt), want, what)
    words = out[prefix + "records"].cpu().numpy()
    rec = out[prefix + "nms_records"].cpu().numpy()
    for q in range(rec.shape[0]):
        np.testing.assert_array_equal(rec[q, :cnt[q]], words[q, idx[q, :cnt[q]]], err_msg=what + ": records are bitwise copies")
        assert (rec[q, cnt[q]:] == np.array([-1, 0, 0, 0])).all() and (idx[q, cnt[q]:] == -1).all()
    return int(raw.count.sum()), int(cnt.sum())


@pytest.mark.parametrize("thd", [0.5, 0.3])
def test_vcmr_search_ends_in_the_final_lists_eager_and_graphed(thd):
    w = _world()
    m, index = w["m"], w["index"]
    nkw = dict(nms_thd=thd, max_after_nms=20, meta2vid=w["meta2vid"], clip_length=CLIP, svmr_video=w["gt"])
    with torch.no_grad():
        plain = inf.vcmr_search(m, index, w["qf"], w["qm"], svmr_video=w["gt"], **KW)
        out = inf.vcmr_search(m, index, w["qf"], w["qm"], **KW, **nkw)
    assert "nms_records" not in plain and "records" not in plain
    for k in plain:          # everything the search returned before is unchanged
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], out[k]), k
    n_in, n_out = _check_nms_outputs(out, "", "VCMR", thd, 20, None, "vcmr_search VCMR")
    assert 0 < n_out < n_in
    n_in, n_out = _check_nms_outputs(out, "svmr_", "SVMR", thd, 20, CLIP, "vcmr_search SVMR")
    assert 0 < n_out < n_in
    want = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    with torch.no_grad():
        gt_static = w["gt"].clone()
        g = inf.GraphedVcmrSearch(m, index, NQ, 30, 128, **KW, **dict(nkw, svmr_video=gt_static))
        for rep in range(2):
            got = g(w["qf"], w["qm"])
            torch.cuda.synchronize()
            for k in ("records", "record_count", "nms_records", "nms_index", "nms_count", "svmr_records", "svmr_record_count",
                      "svmr_nms_records", "svmr_nms_index", "svmr_nms_count", "flat_scores", "flat_indices"):
                assert torch.equal(got[k], want[k]), "%s (replay %d)" % (k, rep)


def test_host_to_host_with_nms_carries_the_kept_records_only():
    """vcmr_search_host(nms_thd=0.5, max_after_nms=20): records and counts == the plain pass's records through
    post_processing_vcmr_nms, at a chunk size that splits the queries (256 + 344) and one that does not; the plain pass is
    bit for bit K10 of one vcmr_search -- what it was before."""
    w = _world()
    m, index, meta2vid = w["m"], w["index"], w["meta2vid"]
    nq = 600
    rng = np.random.default_rng(66)
    qf, qm = _feats(nq, np.concatenate([[30], rng.integers(2, 31, nq - 1)]), 128, 67)
    host = dict(query_feat=qf.pin_memory(), query_mask=qm.pin_memory())
    with torch.no_grad():
        one = inf.vcmr_search(m, index, qf.to(DEV), qm.to(DEV), **KW)
        rec1, cnt1 = ops.moments_decode(one["flat_scores"], flat=one["flat_indices"], top_idx=one["top_indices"],
                                        meta2vid=meta2vid, l_ref=index.l_ref, clip_length=CLIP, seconds=True)
        base = _results(rec1, cnt1)
        want = postproc.post_processing_vcmr_nms(base.copy(), nms_thd=0.5, max_before_nms=N_MOM, max_after_nms=20)
        for chunk, chunks in ((256, [256, 344]), (1024, [600])):
            tm = {}
            rec, cnt = inf.vcmr_search_host(m, index, meta2vid=meta2vid, chunk=chunk, clip_length=CLIP, timings=tm, **host, **KW)
            assert tm["chunk_queries"] == chunks and rec.shape == (nq, N_MOM)
            plain = MomentResults.from_records(list(range(nq)), [""] * nq, rec.copy(), cnt.copy())
            _assert_same(plain, base, "plain host-to-host pass, chunk %d" % chunk)
            np.testing.assert_array_equal(rec.view(np.int32).reshape(nq, N_MOM, 4), rec1.cpu().numpy())   # bitwise, padding included
            for rep in range(2):
                tm = {}
                nrec, ncnt = inf.vcmr_search_host(m, index, meta2vid=meta2vid, chunk=chunk, clip_length=CLIP, timings=tm,
                                                  nms_thd=0.5, max_after_nms=20, **host, **KW)
                assert nrec.shape == (nq, 20) and tm["chunk_queries"] == chunks and tm["nms_s"] > 0
                got = MomentResults.from_records(list(range(nq)), [""] * nq, nrec, ncnt)
                got = got.take(np.tile(np.arange(20), (nq, 1)), ncnt)          # (zeros behind the count, like take() leaves)
                _assert_same(got, want, "host-to-host with NMS, chunk %d pass %d" % (chunk, rep))
                behind = np.arange(20)[None, :] >= ncnt[:, None]
                assert (nrec["vid"][behind] == -1).all() and (nrec["score"][behind] == 0).all()
            # and the plain pass after it is still the plain pass (its own buffers, its own width)
            rec, cnt = inf.vcmr_search_host(m, index, meta2vid=meta2vid, chunk=chunk, clip_length=CLIP, **host, **KW)
            _assert_same(MomentResults.from_records(list(range(nq)), [""] * nq, rec, cnt), base, "plain pass again")
    assert 0 < int(want.count.sum()) < int(base.count.sum()) and int(want.count.max()) <= 20


class _Queries(object):
    """The reference's eval-dataset contract in "query" mode over the world's queries."""

    def __init__(self, w):
        self.qf = w["qf"].cpu().numpy()
        self.lens = w["qlens"]
        self.gt_video = w["gt"].cpu().numpy()
        self.video2idx = {"v%03d" % i: 7 * i + 3 for i in range(NV)}
        self.gt = False

    def set_data_mode(self, mode):
        assert mode == "query"

    def load_gt_vid_name_for_query(self, flag):
        self.gt = flag

    def __len__(self):
        return NQ

    def __getitem__(self, i):
        meta = dict(desc_id=700 + i, desc="query %d" % i, vid_name="v%03d" % self.gt_video[i] if self.gt else None)
        return dict(meta=meta, model_inputs=dict(query_feat=self.qf[i, :self.lens[i]]))


@pytest.mark.parametrize("full_lists", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_eval_epoch_with_nms_on_device_is_eval_epoch(graph, full_lists):
    w = _world()
    ds = _Queries(w)
    ctx = dict(index=w["index"], video_metas=[dict(vid_name="v%03d" % i) for i in range(NV)])
    gt = [dict(desc_id=700 + i, desc="", type=["v", "t", "vt"][i % 3], vid_name="v%03d" % ds.gt_video[i], ts=[3.0, 9.0])
          for i in range(NQ)]
    opt = argparse.Namespace(eval_query_bsz=4, device=torch.device(DEV), q2c_alpha=20.0, min_pred_l=2, max_pred_l=16,
                             clip_length=CLIP, debug=False, external_inference_vr_res_path=None, max_ctx_l=L,
                             max_before_nms=N_MOM, max_vcmr_video=KV, nms_thd=0.5, dset_name="tvr", graph_search=graph,
                             max_desc_l=30, nms_on_full_lists=full_lists)
    runs = {}
    for on_device in (False, True):
        o = copy.copy(opt)
        if on_device:
            o.nms_on_device = True
        with torch.no_grad():
            runs[on_device] = inf.eval_epoch(w["m"], ds, o, tasks=("SVMR", "VCMR", "VR"), max_after_nms=20, ground_truth=gt,
                                             as_arrays=True, ctx_info=ctx)
    (sub_h, met_h, nms_h, mnms_h), (sub_d, met_d, nms_d, mnms_d) = runs[False], runs[True]
    assert set(sub_d) == set(sub_h) == {"video2idx", "SVMR", "VCMR", "VR"} and set(nms_d) == set(nms_h)
    for k in ("SVMR", "VCMR", "VR"):
        _assert_same(sub_d[k], sub_h[k], "raw submission " + k)
    assert met_d == met_h
    for k in ("SVMR", "VCMR"):
        _assert_same(nms_d[k], nms_h[k], "sub_nms " + k)
        assert nms_d[k].width == nms_h[k].width and 0 < int(nms_h[k].count.sum())
    assert mnms_d == mnms_h and mnms_h is not None


def test_sinks_keep_their_keys_without_the_option():
    """compute_query2ctx_info: "VCMR_nms" / "SVMR_nms" appear only with opt.nms_on_device and a threshold."""
    w = _world()
    ds = _Queries(w)
    ctx = dict(index=w["index"], video_metas=[dict(vid_name="v%03d" % i) for i in range(NV)])
    opt = argparse.Namespace(eval_query_bsz=4, device=torch.device(DEV), q2c_alpha=20.0, min_pred_l=2, max_pred_l=16,
                             clip_length=CLIP, debug=False, external_inference_vr_res_path=None, max_ctx_l=L,
                             max_before_nms=N_MOM, nms_thd=0.5)
    with torch.no_grad():
        plain = inf.compute_query2ctx_info(w["m"], ds, opt, ctx, max_before_nms=N_MOM, max_n_videos=KV, tasks=("SVMR", "VCMR"),
                                           as_arrays=True)
        opt.nms_on_device = True
        both = inf.compute_query2ctx_info(w["m"], ds, opt, ctx, max_before_nms=N_MOM, max_n_videos=KV, tasks=("SVMR", "VCMR"),
                                          as_arrays=True, max_after_nms=20)
        only = inf.compute_query2ctx_info_svmr_only(w["m"], ds, opt, ctx, max_before_nms=N_MOM, as_arrays=True, max_after_nms=20)
        opt.nms_thd = -1
        off = inf.compute_query2ctx_info(w["m"], ds, opt, ctx, max_before_nms=N_MOM, max_n_videos=KV, tasks=("SVMR", "VCMR"),
                                         as_arrays=True)
    assert set(plain) == set(off) == {"SVMR", "VCMR"} and set(both) == {"SVMR", "VCMR", "SVMR_nms", "VCMR_nms"}
    assert set(only) == {"SVMR", "SVMR_nms"}
    for k in ("SVMR", "VCMR"):
        _assert_same(both[k], plain[k], "raw " + k)
        fn = postproc.post_processing_vcmr_nms if k == "VCMR" else postproc.post_processing_svmr_nms
        # eval_epoch's order of events: the raw lists are cut to max_after_nms first (the reference's quirk)
        _assert_same(both[k + "_nms"], fn(plain[k].copy().truncate(20), nms_thd=0.5, max_before_nms=N_MOM, max_after_nms=20),
                     k + "_nms")
    _assert_same(only["SVMR"], plain["SVMR"], "svmr-only raw")
    _assert_same(only["SVMR_nms"], both["SVMR_nms"], "svmr-only kept")
