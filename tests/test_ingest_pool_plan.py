"""The host side of ingest from frame- and word-level stores (tvretrieval_amd/ingest.py: frame_clip_boundaries,
sentence_word_ranges, PooledStore, ContextFeeder over a PooledStore) without a GPU.  The two helpers are checked against loop
restatements of the reference lines they cite; the feeder's staging buffers and seg arrays against pooling straight from the
stores, through a CPU stand-in of ops.ingest_pool_rows (in the manner of tests/test_parts_plan.py)."""
import math

import numpy as np
import pytest
import torch

from tvretrieval_amd.ingest import (ContextFeeder, FeatureStore, PooledStore, frame_clip_boundaries, plan_parts,
                                    sentence_word_ranges, write_feature_store)


# ---- loop restatements of the reference's index arithmetic ---------------------------------------------------------------------
def ref_boundaries(clip_length=1.5, max_video_length=300):
    """utils/video_feature/convert_feature_frm_to_clip.py:55-62: feature row j of second s shows s + {3, 13, 23}[j] / 30;
    boundary c = the first row whose time is not before c * clip_length (searchsorted, side left)."""
    times = []
    for second in range(max_video_length):
        for f in (3, 13, 23):
            times.append(f / 30. + second)
    out, c = [], 0
    while c * clip_length < max_video_length:                  # np.arange(0, max_video_length, clip_length)
        bound = c * clip_length
        j = 0
        while j < len(times) and times[j] < bound:
            j += 1
        out.append(j)
        c += 1
    return out


def ref_word_ranges(sub, sentence_lengths, n_clips, clip_length=1.5):
    """utils/text_feature/convert_sub_feature_word_to_clip.py:19-32 (which sentences a clip takes) and :62-86 (their words):
    -> [(lo, hi) or None per clip]."""
    sen2clips = {}
    for s, (st, ed) in enumerate(sub):
        a = int(math.floor(np.float32(st) / np.float32(clip_length)))
        b = int(math.ceil(np.float32(ed) / np.float32(clip_length)))
        sen2clips[s] = set(range(a, b))
    clip2sen = {}
    for s, clips in sen2clips.items():
        for c in clips:
            clip2sen.setdefault(c, []).append(s)
    num_sens = len(sentence_lengths)
    length_indices = [0]
    for i in range(num_sens):
        length_indices.append(length_indices[i] + int(sentence_lengths[i]))
    out = []
    for c in range(n_clips):
        got = None
        if c in clip2sen:
            sen = [min(e, num_sens - 1) for e in sorted(clip2sen[c])]
            lo, hi = length_indices[sen[0]], length_indices[sen[-1] + 1]
            if lo != hi:
                got = (lo, hi)
        out.append(got)
    return out


def as_pairs(r):
    return [None if lo == hi else (int(lo), int(hi)) for lo, hi in r]


def test_default_frame_boundaries():
    b = frame_clip_boundaries()
    assert b.tolist() == ref_boundaries()
    assert len(b) == 200 and b[:8].tolist() == [0, 5, 9, 14, 18, 23, 27, 32]
    seg = np.diff(b)
    assert sorted(set(seg.tolist())) == [4, 5] and int((seg == 4).sum()) == 99 and int((seg == 5).sum()) == 100


@pytest.mark.parametrize("clip_length,max_len", [(1.5, 300), (1.0, 40), (2.5, 61), (0.5, 10)])
def test_frame_boundaries_match_the_restatement(clip_length, max_len):
    assert frame_clip_boundaries(clip_length, max_len).tolist() == ref_boundaries(clip_length, max_len)


def test_frame_boundaries_of_another_extractor():
    b = frame_clip_boundaries(clip_length=1.0, max_video_length=5, frames_in_second=(0, 15), video_fps=30.)
    assert b.tolist() == [0, 2, 4, 6, 8]


SUBS = {
    # a sentence spanning two clips (1.0 .. 2.0 s: clips 0 and 1), and clip 3 that no sentence touches
    "span": ([(1.0, 2.0), (2.2, 2.9), (6.1, 7.4)], [4, 3, 5], 6),
    # more sentences in the subtitle file than in the word store: the last two are clamped to num_sens - 1 = 1
    "clamp": ([(0.1, 1.0), (1.6, 2.5), (3.2, 4.0), (4.6, 5.5)], [2, 6], 5),
    # a sentence of zero words: clip 2 is touched by it alone -> empty; clip 1 by it and a neighbour -> the neighbour's words
    "zero_words": ([(0.2, 1.9), (2.0, 4.4), (4.5, 5.9)], [3, 0, 2], 5),
    # sentences beyond the video's clips, a negative start, exact multiples of the clip length
    "edges": ([(-0.4, 1.5), (1.5, 3.0), (3.0, 3.0), (7.5, 30.0)], [1, 2, 3, 4], 6),
    "none": ([], [], 4),
}


@pytest.mark.parametrize("name", sorted(SUBS))
def test_sentence_word_ranges_match_the_restatement(name):
    sub, lens, n_clips = SUBS[name]
    got = sentence_word_ranges(np.array(sub, dtype=np.float64).reshape(-1, 2), lens, n_clips)
    assert got.shape == (n_clips, 2) and got.dtype == np.int64
    assert as_pairs(got) == ref_word_ranges(sub, lens, n_clips)


def test_sentence_word_ranges_named_cases():
    sub, lens, n = SUBS["span"]
    assert as_pairs(sentence_word_ranges(sub, lens, n)) == [(0, 4), (0, 7), None, None, (7, 12), None]
    sub, lens, n = SUBS["clamp"]
    assert as_pairs(sentence_word_ranges(sub, lens, n)) == [(0, 2), (2, 8), (2, 8), (2, 8), None]
    sub, lens, n = SUBS["zero_words"]
    assert as_pairs(sentence_word_ranges(sub, lens, n)) == [(0, 3), (0, 3), None, (3, 5), None]


def test_random_subtitles_match_the_restatement():
    rng = np.random.default_rng(5)
    for _ in range(30):
        n_sub = int(rng.integers(1, 25))
        st = np.sort(rng.uniform(0, 60, n_sub))
        sub = [(float(a), float(a + rng.uniform(0.2, 4.0))) for a in st]
        lens = rng.integers(0, 9, n_sub - int(rng.integers(0, min(3, n_sub)))).tolist()
        n_clips = int(rng.integers(1, 45))
        assert as_pairs(sentence_word_ranges(sub, lens, n_clips)) == ref_word_ranges(sub, lens, n_clips)


# ---- PooledStore ---------------------------------------------------------------------------------------------------------------
FRAMES = dict(a=23, b=14, c=200, d=4, e=33)        # frame rows per video


def ref_clip_count(n_frames, b):
    """convert_feature_frm_to_clip.py:29-32: clips until the first empty slice of the frame rows."""
    n = 0
    for idx in range(len(b) - 1):
        if len(range(n_frames)[b[idx]:b[idx + 1]]) == 0:
            break
        n += 1
    return n


@pytest.fixture
def stores(tmp_path):
    rng = np.random.default_rng(1)
    res = {k: rng.standard_normal((n, 16)).astype(np.float16) for k, n in FRAMES.items()}
    i3d = {k: rng.standard_normal((n, 8)).astype(np.float16) for k, n in FRAMES.items()}
    write_feature_store(str(tmp_path / "res"), res)
    write_feature_store(str(tmp_path / "i3d"), i3d)
    write_feature_store(str(tmp_path / "i3d_short"), {k: v[:-4] for k, v in i3d.items()})
    return dict(res=FeatureStore(str(tmp_path / "res")), i3d=FeatureStore(str(tmp_path / "i3d")),
                i3d_short=FeatureStore(str(tmp_path / "i3d_short")), res_np=res, i3d_np=i3d, tmp=tmp_path)


def test_pooled_store_clip_counts(stores):
    b = frame_clip_boundaries()
    ps = PooledStore([(stores["res"], b, True), (stores["i3d"], b, True)])
    assert ps.dim == 24 and ps.pool == "max"
    want = dict(a=5, b=3, c=45, d=1, e=8)          # 23 frames: [0,5) [5,9) [9,14) [14,18) [18,23); 14 frames: the fourth is empty
    for k, n in FRAMES.items():
        assert ps.n_rows(k) == ref_clip_count(n, b) == want[k], k
        r = ps.clip_ranges(k)[0]
        assert r[:, 0].tolist() == b[:len(r)].tolist() and r[-1, 1] == n and (r[:-1, 1] == b[1:len(r)]).all()
    assert "a" in ps and "zz" not in ps
    # a boundary array that ends before the video does: at most len(b) - 1 clips
    assert PooledStore([(stores["res"], b[:4], False)]).n_rows("c") == 3
    # the break at the FIRST empty clip: boundaries that repeat end the video there
    assert PooledStore([(stores["res"], np.array([0, 5, 5, 9, 14]), False)]).n_rows("c") == 1


def test_pooled_store_mapping_and_refusals(stores):
    b = frame_clip_boundaries()
    words = {k: np.array([[0, 3], [0, 0], [2, 4]]) for k in FRAMES}
    ps = PooledStore([(stores["res"], words, False)], pool="mean")
    assert ps.n_rows("d") == 3 and ps.clip_ranges("d")[0].dtype == np.int64
    with pytest.raises(ValueError, match="outside"):
        PooledStore([(stores["res"], dict(d=np.array([[0, 5]])), False)]).n_rows("d")        # video d has 4 rows
    with pytest.raises(ValueError, match="outside"):
        PooledStore([(stores["res"], dict(d=np.array([[3, 2]])), False)]).n_rows("d")
    two = PooledStore([(stores["res"], b, True), (stores["i3d_short"], b, True)])
    assert two.n_rows("a") == 5                        # 23 and 19 frames: the fifth clip is [18, 23) and [18, 19)
    with pytest.raises(ValueError, match="disagree on the clip count of 'e': 8 / 7"):
        two.n_rows("e")                                # 33 frames: the eighth clip is [32, 33); 29 frames end in the seventh
    with pytest.raises(ValueError, match="1 or 2 sources"):
        PooledStore([])
    with pytest.raises(ValueError, match="pool"):
        PooledStore([(stores["res"], b, True)], pool="sum")
    with pytest.raises(ValueError, match="boundary array"):
        PooledStore([(stores["res"], np.array([0, 5, 3]), True)])


# ---- the feeder's staging and seg arrays, through a CPU stand-in of ops.ingest_pool_rows ---------------------------------------
class Ops(object):
    """Records what the feeder hands to ingest_pool_rows and pools it in numpy: per video the (len, sum d) clip rows."""
    calls = []

    @classmethod
    def ingest_pool_rows(cls, sources, row_start, n, lmax, max_len, pool="max", normalize=True, eps=1e-5,
                         out_dtype=torch.float32):
        rs = row_start.tolist()
        assert len(rs) == n + 1 and rs[0] == 0 and lmax == max(min(rs[i + 1] - rs[i], max_len) for i in range(n))
        blocks = []
        for src, seg, norm in sources:
            src, seg = src.numpy().astype(np.float32), seg.numpy()
            assert seg.shape == (rs[-1], 2) and seg.dtype == np.int64
            assert ((seg[:, 0] >= 0) & (seg[:, 0] <= seg[:, 1]) & (seg[:, 1] <= len(src))).all(), "a range outside the staged rows"
            f = np.max if pool == "max" else np.mean
            blocks.append(np.stack([f(src[lo:hi], axis=0) if hi > lo else np.zeros(src.shape[1], np.float32) for lo, hi in seg])
                          if len(seg) else np.zeros((0, src.shape[1]), np.float32))
        rows = np.concatenate(blocks, axis=1)
        cls.calls.append(dict(rows=[int(s[0].shape[0]) for s in sources], norms=[s[2] for s in sources], normalize=normalize,
                              pool=pool, used=[int((s[1][:, 1] - s[1][:, 0]).sum()) for s in sources]))
        return [rows[rs[i]:rs[i + 1]] for i in range(n)], lmax


def pooled_clip_rows(arrays, ranges, pool):
    f = np.max if pool == "max" else np.mean
    out = []
    for a, r in zip(arrays, ranges):
        a = a.astype(np.float32)
        out.append(np.stack([f(a[lo:hi], axis=0) if hi > lo else np.zeros(a.shape[1], np.float32) for lo, hi in r]))
    return np.concatenate(out, axis=1)


def word_store(stores, n_clips):
    """a word-level store with TVR-like ranges: overlapping neighbours, empty clips, a range that ends at the last row"""
    rng = np.random.default_rng(2)
    words, ranges = {}, {}
    for k, nc in n_clips.items():
        lo = np.sort(rng.integers(0, 3 * nc, nc))
        hi = lo + rng.integers(0, 7, nc)                      # 0: an empty clip
        n_words = int(hi.max()) + (0 if k == "a" else 3)
        words[k] = rng.standard_normal((max(n_words, 1), 6)).astype(np.float32)
        ranges[k] = np.where((hi > lo)[:, None], np.stack([lo, hi], 1), 0)
    write_feature_store(str(stores["tmp"] / "words"), words, "float32")
    return FeatureStore(str(stores["tmp"] / "words")), words, ranges


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_feeder_stages_the_fine_rows_and_their_ranges(stores, pool):
    b = frame_clip_boundaries()
    vs = PooledStore([(stores["res"], b, True), (stores["i3d"], b, False)], pool=pool)
    names = ["c", "a", "e", "b", "d"]                   # not the store's order: 'a', 'e' are no neighbours there
    n_clips = {k: vs.n_rows(k) for k in names}
    wstore, words, wranges = word_store(stores, n_clips)
    ss = PooledStore([(wstore, wranges, False)], pool=pool)
    w = 8                                               # video c (45 clips) and e (8) are cut / kept whole at max_ctx_len
    Ops.calls = []
    fd = ContextFeeder(names, vs, ss, max_ctx_len=w, batch_size=3, device="cpu", ops=Ops, host_threads=1,
                       normalize_vfeat=True, normalize_tfeat=False)
    assert len(fd) == 2
    got_v, got_s = [], []
    for vf, lv, sf, ls in fd:
        assert lv == ls
        got_v += vf
        got_s += sf
    assert len(got_v) == len(names)
    for k, gv, gs in zip(names, got_v, got_s):
        ln = min(n_clips[k], w)
        want_v = pooled_clip_rows([stores["res_np"][k], stores["i3d_np"][k]], [r[:ln] for r in vs.clip_ranges(k)], pool)
        want_s = pooled_clip_rows([words[k]], [wranges[k][:ln]], pool)
        assert gv.shape == (ln, 24) and np.array_equal(gv, want_v), k
        assert gs.shape == (ln, 6) and np.array_equal(gs, want_s), k
    video_calls = [c for c in Ops.calls if len(c["rows"]) == 2]
    assert [c["norms"] for c in video_calls] == [[True, False]] * 2 and all(c["normalize"] is True for c in video_calls)
    assert all(c["normalize"] is False and c["pool"] == pool for c in Ops.calls if len(c["rows"]) == 1)
    # only the rows the first max_ctx_len clips need are staged: video c contributes b[8] = 36 of its 200 frames
    first = video_calls[0]
    assert first["rows"] == [int(b[8]) + 23 + 33] * 2 and first["used"] == first["rows"]
    fine = sum(min(FRAMES[k], int(b[min(n_clips[k], w)])) for k in names)
    staged_words = sum(c["rows"][0] for c in Ops.calls if len(c["rows"]) == 1)
    # stats count the staged rows; a batch with no word at all still hands over one (unread) row
    assert fd.stats["rows"] == 2 * fine + sum(_span(wranges[k][:min(n_clips[k], w)]) for k in names)
    assert staged_words >= sum(_span(wranges[k][:min(n_clips[k], w)]) for k in names)
    assert fd.stats["h2d_bytes"] == fine * (16 + 8) * 2 + (fd.stats["rows"] - 2 * fine) * 6 * 4


def _span(r):
    full = r[:, 1] > r[:, 0]
    return int(r[full, 1].max() - r[full, 0].min()) if full.any() else 0


def test_feeder_iterates_parts_of_pooled_stores(stores):
    b = frame_clip_boundaries()
    vs = PooledStore([(stores["res"], b, True), (stores["i3d"], b, True)])
    names = ["a", "c", "e"]
    n_clips = {k: vs.n_rows(k) for k in names}                  # 5, 45, 8
    wstore, words, wranges = word_store(stores, n_clips)
    ss = PooledStore([(wstore, wranges, False)])
    t = plan_parts(np.array([n_clips[k] for k in names]), 16, 4)          # the long video: parts at 0, 12, 24, 29
    assert t.part_offset.tolist() == [0, 0, 12, 24, 29, 0]
    Ops.calls = []
    fd = ContextFeeder(names, vs, ss, max_ctx_len=16, batch_size=4, device="cpu", ops=Ops, parts=t, host_threads=1)
    got_v, got_s = [], []
    for vf, lv, sf, ls in fd:
        got_v += vf
        got_s += sf
    assert len(got_v) == t.n_parts == 6
    for p in range(t.n_parts):
        k, o, ln = names[t.part_video[p]], int(t.part_offset[p]), int(t.part_len[p])
        want_v = pooled_clip_rows([stores["res_np"][k], stores["i3d_np"][k]], [r[o:o + ln] for r in vs.clip_ranges(k)], "max")
        assert np.array_equal(got_v[p], want_v), p
        assert np.array_equal(got_s[p], pooled_clip_rows([words[k]], [wranges[k][o:o + ln]], "max")), p
    # a part stages its own frames only: part 2 of video c is clips 12 .. 27 = frames b[12] .. b[28]
    assert Ops.calls[0]["rows"][0] == 23 + int(b[16]) + int(b[28] - b[12]) + int(b[40] - b[24])
    with pytest.raises(ValueError, match="same clip count"):
        ContextFeeder(names, vs, ss, max_ctx_len=16, device="cpu", ops=Ops, parts=plan_parts(np.array([5, 44, 8]), 16, 4))


def test_clip_stores_take_the_old_path(stores):
    """A feeder over clip stores never asks for ingest_pool_rows."""
    class Old(object):
        @staticmethod
        def ingest_rows(src, row_start, n, lmax, max_len, normalize=True, eps=1e-5, out_dtype=torch.float32):
            return src.clone(), lmax
    fd = ContextFeeder(["a", "b"], stores["res"], None, max_ctx_len=100, batch_size=2, device="cpu", ops=Old, host_threads=1)
    (vf, lmax, sf, sm), = list(fd)
    assert lmax == 23 and sf is None and np.array_equal(vf.numpy(), np.concatenate([stores["res_np"]["a"], stores["res_np"]["b"]]))
