"""The part plan of videos longer than max_ctx_l (ingest.plan_parts / PartTable) and the argument checks of the three C entries
of the parts path (xml_group_best_allow, xml_best_part_rows, xml_moments_decode_parts) -- all on the host: the entries reject
bad arguments before any launch."""
import ctypes
import os

import numpy as np
import pytest

from tvretrieval_amd.ingest import PartTable, plan_parts

BAD_ARG = -1
CASES = [(w, o) for w in (8, 32, 100) for o in (0, 3, 16) if o < w]


@pytest.mark.parametrize("w,o", CASES)
def test_plan_covers_every_video_and_every_short_window(w, o):
    """Every n in 1 .. 3W + 5 as one corpus: part count, parts inside the video, full length beyond W, adjacency and order,
    and by brute force that every window of <= O clips (at least the single clips) lies inside some part."""
    ns = np.arange(1, 3 * w + 6)
    t = plan_parts(ns, w, o)
    s = w - o
    assert t.n_videos == len(ns) and t.group_start[0] == 0 and t.group_start[-1] == t.n_parts
    assert t.max_ctx_len == w and t.overlap == o
    for v, n in enumerate(ns):
        b, e = int(t.group_start[v]), int(t.group_start[v + 1])
        off, ln = t.part_offset[b:e].astype(np.int64), t.part_len[b:e].astype(np.int64)
        assert (t.part_video[b:e] == v).all()
        want = 1 if n <= w else 1 + -(-(n - w) // s)
        assert e - b == want, (n, e - b, want)
        assert off[0] == 0 and (np.diff(off) > 0).all()                       # offset order
        assert (off >= 0).all() and (off + ln <= n).all() and (off + ln).max() == n        # inside the video, up to its end
        if n > w:
            assert (ln == w).all()
            assert off[:-1].tolist() == [j * s for j in range(want - 1)] and off[-1] == n - w
            assert all(x + w < n for x in off[:-1])
        else:
            assert ln.tolist() == [n]
        # cover[a, l - 1]: some part holds the window [a, a + l)
        for l in range(1, max(o, 1) + 1):
            starts = np.arange(0, n - l + 1)
            inside = (off[None, :] <= starts[:, None]) & (starts[:, None] + l <= (off + ln)[None, :])
            assert inside.any(1).all(), "n = %d: a window of %d clips lies in no part" % (n, l)
    assert np.array_equal(t.n_clips(), ns)


def test_meta2vid_and_arrays():
    t = plan_parts(np.array([5, 32, 33, 80]), 32, 8)
    assert t.part_video.tolist() == [0, 1, 2, 2, 3, 3, 3]
    assert t.part_offset.tolist() == [0, 0, 0, 1, 0, 24, 48]
    assert t.part_len.tolist() == [5, 32, 32, 32, 32, 32, 32]
    assert t.group_start.tolist() == [0, 1, 2, 4, 7]
    assert all(a.dtype == np.int32 for a in (t.part_video, t.part_offset, t.part_len, t.group_start))
    assert t.meta2vid() is t.part_video
    assert t.meta2vid(np.array([7, 9, 11, 13])).tolist() == [7, 9, 11, 11] + [13] * (t.n_parts - 4)
    with pytest.raises(ValueError, match="ids"):
        t.meta2vid(np.array([1, 2]))
    d = t.to("cpu")                                       # the "device" copy: int32 tensors
    import torch
    assert torch.is_tensor(d.part_video) and d.part_video.dtype == torch.int32 and d.n_parts == t.n_parts
    assert d.meta2vid(torch.tensor([7, 9, 11, 13], dtype=torch.int32)).tolist() == t.meta2vid(np.array([7, 9, 11, 13])).tolist()


def test_plan_of_80_clips_at_32_8():
    """80 clips, W 32, O 8 (S 24): offsets 0 and 24 (24 + 32 < 80), not 48 (48 + 32 = 80), and the last part at 48."""
    t = plan_parts(np.array([80]), 32, 8)
    assert t.part_offset.tolist() == [0, 24, 48] and t.part_len.tolist() == [32, 32, 32]
    t = plan_parts(np.array([81]), 32, 8)
    assert t.part_offset.tolist() == [0, 24, 48, 49]


def test_default_overlap_is_the_reference_max_pred_l():
    assert plan_parts(np.array([300]), 100).overlap == 16


@pytest.mark.parametrize("kw,match", [
    (dict(overlap=32), "overlap"),
    (dict(overlap=-1), "overlap"),
    (dict(max_ctx_len=0), "overlap"),
    (dict(group_start=[0, 2, 2, 5]), "group_start"),                 # a video without a part
    (dict(group_start=[0, 2, 1, 5]), "group_start"),                 # not monotone
    (dict(group_start=[0, 2, 4]), "group_start"),                    # does not end at n_parts
    (dict(group_start=[1, 2, 3, 5]), "group_start"),
    (dict(part_video=[0, 1, 0, 2, 2]), "adjacent"),                  # parts of video 0 are not adjacent rows
    (dict(part_video=[0, 0, 2, 1, 1]), "adjacent"),
    (dict(part_len=[32, 33, 5, 32, 32]), "part_len"),
    (dict(part_len=[32, 0, 5, 32, 32]), "part_len"),
    (dict(part_offset=[0, 24, 0, 24, 0]), "offset"),                 # not in rising order inside a video
    (dict(part_offset=[1, 24, 0, 0, 24]), "offset"),                 # first part not at 0
    (dict(part_offset=[0, 24, 0, 0]), "one entry per part"),
    (dict(part_video=[[0, 0, 1, 2, 2]]), "1-D"),
    (dict(part_video=np.array([0, 0, 1, 2, 2], dtype=np.float32)), "integer"),
])
def test_part_table_validation(kw, match):
    good = dict(part_video=[0, 0, 1, 2, 2], part_offset=[0, 24, 0, 0, 24], part_len=[32, 32, 5, 32, 32],
                group_start=[0, 2, 3, 5], max_ctx_len=32, overlap=8)
    PartTable(**{k: (np.asarray(v) if isinstance(v, list) else v) for k, v in good.items()})
    bad = dict(good, **kw)
    with pytest.raises(ValueError, match=match):
        PartTable(**{k: (np.asarray(v) if isinstance(v, list) else v) for k, v in bad.items()})


@pytest.mark.parametrize("args", [(np.array([], dtype=np.int64), 32, 8), (np.array([5, 0]), 32, 8), (np.array([5.0]), 32, 8),
                                  (np.array([[5]]), 32, 8), (np.array([5]), 32, 32), (np.array([5]), 0, 0)])
def test_plan_parts_rejects_bad_input(args):
    with pytest.raises(ValueError):
        plan_parts(*args)


def test_context_feeder_iterates_parts(tmp_path):
    """ContextFeeder(parts=) hands out the sub-ranges of the store's rows (a CPU stand-in of xml_ingest_rows records what it is
    asked for); stores whose clip counts differ from the plan are refused."""
    import torch
    from tvretrieval_amd.ingest import ContextFeeder, FeatureStore, write_feature_store
    ns = dict(a=5, b=80, c=33)
    rng = np.random.default_rng(0)
    feats = {k: rng.standard_normal((n, 4)).astype(np.float32) for k, n in ns.items()}
    write_feature_store(str(tmp_path / "v"), feats, "float32")
    write_feature_store(str(tmp_path / "s"), {k: v[:, :2] for k, v in feats.items()}, "float32")
    write_feature_store(str(tmp_path / "s_short"), {k: v[:-1, :2] for k, v in feats.items()}, "float32")
    vs, ss = FeatureStore(str(tmp_path / "v")), FeatureStore(str(tmp_path / "s"))
    names = list(ns)
    t = plan_parts(np.array([ns[k] for k in names]), 32, 8)

    class Ops(object):
        @staticmethod
        def ingest_rows(src, row_start, n, lmax, max_len, normalize=True, eps=1e-5, out_dtype=torch.float32):
            rs = row_start.tolist()
            return [src[rs[i]:rs[i + 1]].clone() for i in range(n)], lmax

    fd = ContextFeeder(names, vs, ss, max_ctx_len=32, batch_size=4, device="cpu", ops=Ops, parts=t, host_threads=1)
    assert len(fd) == 2
    got_v, got_s = [], []
    for vf, lv, sf, ls in fd:
        assert lv == ls
        got_v += vf
        got_s += sf
    assert len(got_v) == t.n_parts == 6
    for p in range(t.n_parts):
        name, o, l = names[t.part_video[p]], int(t.part_offset[p]), int(t.part_len[p])
        assert np.array_equal(got_v[p].numpy(), feats[name][o:o + l]), p
        assert np.array_equal(got_s[p].numpy(), feats[name][o:o + l, :2]), p
    with pytest.raises(ValueError, match="same clip count"):
        ContextFeeder(names, vs, FeatureStore(str(tmp_path / "s_short")), max_ctx_len=32, device="cpu", ops=Ops, parts=t)
    with pytest.raises(ValueError, match="part table covers"):
        ContextFeeder(names[:2], vs, ss, max_ctx_len=32, device="cpu", ops=Ops, parts=t)
    with pytest.raises(ValueError, match="part table covers"):
        ContextFeeder(names, vs, ss, max_ctx_len=64, device="cpu", ops=Ops, parts=t)


# ---------------------------------------------------------------------------------------------------------
# the C entries: exported, bound, and bad arguments rejected before any launch
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tvretrieval_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbols_are_exported_bound_and_declared(lib):
    from tvretrieval_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "xmlhip.h")).read()
    for name, n_args in (("xml_group_best_allow", 13), ("xml_best_part_rows", 8), ("xml_moments_decode_parts", 17)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args
        assert "int %s(" % name in header
    assert len(_lib.SIGNATURES["xml_moments_decode_parts"][1]) == len(_lib.SIGNATURES["xml_moments_decode"][1]) + 1
    assert lib.xml_abi_version() == 6          # additive: nothing existing changed signature


def _fold(lib, scores=0x1000, ld=70, rows=3, n_parts=70, part_video=0x2000, group_start=0x3000, n_videos=20, allow=0,
          allow_ld=0, allow_rows=0, out=0x4000, out_ld=3):
    p = ctypes.c_void_p
    return lib.xml_group_best_allow(p(scores), ld, rows, n_parts, p(part_video), p(group_start), n_videos, p(allow), allow_ld,
                                    allow_rows, p(out), out_ld, p(0))


@pytest.mark.parametrize("bad", [
    dict(scores=0), dict(part_video=0), dict(group_start=0), dict(out=0),
    dict(rows=-1), dict(n_parts=0), dict(n_parts=-5), dict(n_videos=0), dict(n_videos=-1),
    dict(n_videos=71),                                   # more videos than parts
    dict(ld=69),                                         # row stride below n_parts
    dict(out_ld=2),                                      # 70 parts need 3 words
    dict(allow=0x5000, allow_ld=0, allow_rows=1),        # 20 videos need 1 word
    dict(allow=0x5000, allow_ld=1, allow_rows=2),        # allow rows neither 1 nor rows
    dict(allow=0x5000, allow_ld=-1, allow_rows=1),
], ids=["scores_null", "part_video_null", "group_start_null", "out_null", "rows_neg", "n_parts_0", "n_parts_neg", "n_videos_0",
        "n_videos_neg", "n_videos_gt_parts", "ld", "out_ld", "allow_ld", "allow_rows", "allow_ld_neg"])
def test_group_best_allow_rejects_bad_arguments(lib, bad):
    assert _fold(lib, **bad) == BAD_ARG


def _best(lib, scores=0x1000, ld=70, rows=3, group_start=0x3000, n_videos=20, video=0x5000, out=0x4000):
    p = ctypes.c_void_p
    return lib.xml_best_part_rows(p(scores), ld, rows, p(group_start), n_videos, p(video), p(out), p(0))


@pytest.mark.parametrize("bad", [dict(scores=0), dict(group_start=0), dict(video=0), dict(out=0), dict(rows=-1),
                                 dict(n_videos=0), dict(n_videos=-3), dict(ld=19), dict(ld=-1)],
                         ids=["scores_null", "group_start_null", "video_null", "out_null", "rows_neg", "n_videos_0",
                              "n_videos_neg", "ld", "ld_neg"])
def test_best_part_rows_rejects_bad_arguments(lib, bad):
    assert _best(lib, **bad) == BAD_ARG


def test_empty_row_sets_are_no_ops(lib):
    assert _fold(lib, rows=0) == 0
    assert _best(lib, rows=0) == 0


def _decode(lib, flat=0x1000, score=0x2000, top_idx=0x3000, row_vid=0, meta2vid=0x4000, part_offset=0x5000, nq=4, n=8,
            ld_in=8, k=2, l_ref=16, clip=1.5, seconds=1, out=0x6000, ld_out=8, out_count=0):
    p = ctypes.c_void_p
    return lib.xml_moments_decode_parts(p(flat), p(score), p(top_idx), p(row_vid), p(meta2vid), p(part_offset), nq, n, ld_in,
                                        k, l_ref, clip, seconds, p(out), ld_out, p(out_count), p(0))


@pytest.mark.parametrize("bad,code", [
    (dict(part_offset=0), -1), (dict(score=0), -1), (dict(out=0), -1), (dict(nq=0), -1), (dict(nq=-1), -1), (dict(n=0), -1),
    (dict(ld_in=7), -1), (dict(ld_out=7), -1), (dict(l_ref=0), -1), (dict(k=0), -1), (dict(flat=0, top_idx=0), -1),
    (dict(out=0x6008), -1),
    (dict(l_ref=40000, k=2), -2),                        # the INT32_MAX guard of xml_moments_decode, unchanged
], ids=["part_offset_null", "score_null", "out_null", "nq_0", "nq_neg", "n_0", "ld_in", "ld_out", "l_ref_0", "k_0", "no_list",
        "misaligned", "int32_guard"])
def test_moments_decode_parts_rejects_bad_arguments(lib, bad, code):
    assert _decode(lib, **bad) == code
