"""CPU-side checks of xml_eval_moments (retrieval metrics on the device): the symbol is declared, exported and bound, and the
entry rejects every argument outside its limits before any launch (no GPU here, so a launch would fail differently)."""
import ctypes
import os

import numpy as np
import pytest

BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbol_is_exported_bound_and_declared(lib):
    from tvretrieval_amd import _lib, ops
    assert hasattr(lib, "xml_eval_moments")
    res, args = _lib.SIGNATURES["xml_eval_moments"]
    assert res is ctypes.c_int and len(args) == 21
    assert lib.xml_eval_moments.argtypes == args
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int xml_eval_moments(const xml_moment* rec," in open(os.path.join(root, "include", "xmlhip.h")).read()
    assert lib.xml_abi_version() == 6          # additive: nothing existing changed signature
    assert callable(ops.eval_moments) and ops.EVAL_TASKS == {"VCMR": 0, "SVMR": 1, "VR": 2}


def _call(lib, rec=0x1000, ld_rec=8, count=0, nq=2, n=8, task=0, scale=1.0, max_pred=100, gt_vid=0x2000, gt_ts=0x3000, n_ts=1,
          n_gt=0x4000, desc_type=0x5000, iou_thd=(0.5, 0.7), n_thd=None, topk=(1, 5, 10, 100), n_k=None, first_hit=0x6000,
          hits=0x7000, rows=0x8000):
    p = ctypes.c_void_p
    thd = np.asarray(iou_thd, dtype=np.float32) if iou_thd is not None else None
    ks = np.asarray(topk, dtype=np.int32) if topk is not None else None
    return lib.xml_eval_moments(p(rec), ld_rec, p(count), nq, n, task, scale, max_pred, p(gt_vid), p(gt_ts), n_ts, p(n_gt),
                                p(desc_type), p(thd.ctypes.data) if thd is not None else p(0),
                                len(thd) if n_thd is None else n_thd, p(ks.ctypes.data) if ks is not None else p(0),
                                len(ks) if n_k is None else n_k, p(first_hit), p(hits), p(rows), p(0))


@pytest.mark.parametrize("bad", [
    dict(n=0),                                          # 1 <= n
    dict(n=1025, ld_rec=1025),                          # n <= 1024
    dict(iou_thd=(), n_thd=0),                          # 1 <= n_thd
    dict(iou_thd=(0.1, 0.3, 0.5, 0.7, 0.9)),            # n_thd <= 4
    dict(topk=(), n_k=0),                               # 1 <= n_k
    dict(topk=tuple(range(1, 10))),                     # n_k <= 8
    dict(topk=(0, 5)),                                  # topk positive
    dict(topk=(5, 1)),                                  # topk ascending
    dict(n_ts=0),                                       # 1 <= n_ts
    dict(n_ts=17),                                      # n_ts <= 16
    dict(max_pred=-1),
    dict(scale=float("nan")),
    dict(task=-1),
    dict(task=3),
    dict(rec=0x1008),                                   # records not 16-byte aligned
    dict(ld_rec=7),                                     # row stride below n
    dict(nq=-1),
    dict(rec=0),
    dict(gt_vid=0),
    dict(gt_ts=0),
    dict(n_gt=0),
    dict(iou_thd=None, n_thd=2),                        # thresholds are needed for VCMR / SVMR
    dict(topk=None, n_k=4),
    dict(first_hit=0),
    dict(hits=0),
    dict(rows=0),
], ids=["n_0", "n_1025", "n_thd_0", "n_thd_5", "n_k_0", "n_k_9", "topk_zero", "topk_descending", "n_ts_0", "n_ts_17",
        "max_pred_neg", "nan_scale", "task_neg", "task_3", "misaligned", "ld_rec", "nq_neg", "rec_null", "gt_vid_null",
        "gt_ts_null", "n_gt_null", "iou_thd_null", "topk_null", "first_hit_null", "hits_null", "rows_null"])
def test_bad_arguments_are_rejected_before_any_launch(lib, bad):
    assert _call(lib, **bad) == BAD_ARG


def test_empty_query_set_is_a_no_op(lib):
    assert _call(lib, nq=0) == 0
    assert _call(lib, nq=0, task=2, iou_thd=None, n_thd=1) == 0       # VR needs no thresholds
    assert _call(lib, nq=0, count=0, desc_type=0) == 0                # count and desc_type are optional


def test_metrics_from_hits_restates_the_host_formatting():
    """Counters -> the host's OrderedDicts: keys, order, rounding, NaN for an empty description type, the ratio string."""
    from tvretrieval_amd import evaluate
    hits = np.zeros((4, 2, 4), dtype=np.int32)
    hits[0] = [[1, 2, 3, 7], [0, 1, 1, 3]]
    hits[1] = [[1, 1, 2, 4], [0, 1, 1, 2]]
    hits[3] = [[0, 1, 1, 3], [0, 0, 0, 1]]
    rows = np.array([7, 4, 0, 3], dtype=np.int32)
    m, mt = evaluate.metrics_from_hits(hits, rows, "VCMR", (0.5, 0.7), (1, 5, 10, 100), True)
    assert list(m) == ["%s-r%d" % (t, k) for t in (0.5, 0.7) for k in (1, 5, 10, 100)]
    assert m["0.5-r1"] == round(np.float64(1) / 7 * 100, 2) == 14.29 and m["0.7-r100"] == 42.86
    assert list(mt) == ["%s-%s-r%d" % (d, t, k) for d in ("v", "t", "vt") for t in (0.5, 0.7) for k in (1, 5, 10, 100)] \
        + ["desc_type_ratio"]
    assert mt["v-0.5-r100"] == 100.0 and np.isnan(mt["t-0.5-r1"]) and mt["vt-0.7-r100"] == 33.33
    assert mt["desc_type_ratio"] == "v 57.14 t 0.0 vt 42.86"
    m, mt = evaluate.metrics_from_hits(hits[:, :1], rows, "VR", (0.5, 0.7), (1, 5, 10, 100), False)
    assert list(m) == ["r1", "r5", "r10", "r100"] and m["r100"] == 100.0 and len(mt) == 0
