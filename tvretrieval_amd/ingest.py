"""Feature ingest ("next" row 8f-3): replacement for the h5py-backed StartEndEvalDataset feature lookup + collate
(xml/start_end_dataset.py:208-232,297-359) on a box without h5py.

  FeatureStore        flat binary container: <path>.bin (all rows, float16 / float32, memory-mapped) + <path>.json
                      ({"dim", "dtype", "index": {name: [first_row, n_rows]}}).  `write_feature_store` converts a
                      {name: (n_clips, D) array} mapping (e.g. exported from the reference's h5 files elsewhere).
  ContextFeeder       iterator of (video_feat, video_mask, sub_feat, sub_mask) DEVICE batches with the reference's
                      semantics: truncate to max_ctx_len (start_end_dataset.py:311,320), pad with zeros to the batch
                      maximum + float mask (pad_sequences_1d), L2-normalise each clip x / (||x|| + 1e-5)
                      (utils/basic_utils.py:82-84).  The host only moves bytes: raw rows go from the memory map into
                      pinned staging buffers (two, alternating) in the store's dtype and back to back, are copied
                      asynchronously on a side stream (the H2D copy of batch i+1 overlaps the encoder kernels of batch
                      i), and ONE device launch (xml_ingest_rows) truncates, pads, converts, normalises and writes
                      the mask.  ctx_mode="video_sub_tef" / "video_tef" / "sub_tef": the launch (xml_ingest_rows_tef,
                      xml_ingest_pool_rows_tef) also appends the reference's two temporal endpoint columns
                      (start_end_dataset.py:328-342); the parts of a long video get WHOLE-VIDEO time.
  PooledStore         1-2 FRAME- or WORD-level FeatureStores (what a feature extractor emits) + the source-row range of every
                      clip; ContextFeeder takes one in place of a clip store: it stages the fine rows, and ONE launch
                      (xml_ingest_pool_rows) pools them into clips (max / mean), normalises each source, concatenates,
                      and does the rest of the collate -- the reference's three offline numpy + h5py conversion scripts
                      (utils/video_feature/convert_feature_frm_to_clip.py, normalize_and_concat.py,
                      utils/text_feature/convert_sub_feature_word_to_clip.py) and their clip-level copy of the corpus on
                      disk are not needed.  frame_clip_boundaries / sentence_word_ranges restate their index arithmetic.
                      train_data.DeviceTrainStore takes one too (the fine rows resident, pooled in the batch gather), and
                      PooledStore[name] pools on the host for StoreTrainDataset / StoreEvalDataset.
  StoreEvalDataset    the reference's eval-dataset contract (set_data_mode / load_gt_vid_name_for_query / items with
                      "meta" + "model_inputs") over FeatureStores, for compute_context_info / compute_query2ctx_info.
"""
import json
import os

import numpy as np
import torch

from . import ops as hip_ops
from .train_data import CTX_MODES

_DT = {"float16": np.float16, "float32": np.float32}


class FeatureStoreWriter(object):
    """Streaming writer of a FeatureStore: add(name, (n_clips, D) array) one video at a time, close() writes the index."""

    def __init__(self, path, dim, dtype="float16"):
        self.path, self.dim, self.dtype = path, int(dim), dtype
        self.index, self.row = {}, 0
        self.f = open(path + ".bin", "wb")

    def add(self, name, a):
        a = np.asarray(a)
        assert a.ndim == 2 and a.shape[1] == self.dim
        self.f.write(np.ascontiguousarray(a, dtype=_DT[self.dtype]).tobytes())
        self.index[name] = [self.row, int(a.shape[0])]
        self.row += int(a.shape[0])

    def add_block(self, names, block):
        """Several videos of equal length at once: block (len(names), n_clips, D) -- one write."""
        block = np.ascontiguousarray(block, dtype=_DT[self.dtype])
        assert block.ndim == 3 and block.shape[0] == len(names) and block.shape[2] == self.dim
        self.f.write(memoryview(block).cast("B"))
        for n in names:
            self.index[n] = [self.row, int(block.shape[1])]
            self.row += int(block.shape[1])

    def close(self):
        self.f.close()
        with open(self.path + ".json", "w") as f:
            json.dump(dict(dim=self.dim, dtype=self.dtype, rows=self.row, index=self.index), f)


def write_feature_store(path, features, dtype="float16"):
    names = list(features)
    w = FeatureStoreWriter(path, int(np.asarray(features[names[0]]).shape[1]), dtype)
    for n in names:
        w.add(n, features[n])
    w.close()


class FeatureStore(object):
    def __init__(self, path):
        meta = json.load(open(path + ".json"))
        self.dim, self.index, self.dtype = meta["dim"], meta["index"], meta["dtype"]
        self.data = np.memmap(path + ".bin", dtype=_DT[meta["dtype"]], mode="r", shape=(meta["rows"], self.dim))

    def __contains__(self, name):
        return name in self.index

    def __getitem__(self, name):
        first, n = self.index[name]
        return self.data[first:first + n]

    def n_rows(self, name):
        return self.index[name][1]


_TORCH_DT = {"float16": torch.float16, "float32": torch.float32}


def frame_clip_boundaries(clip_length=1.5, max_video_length=300, frames_in_second=(3, 13, 23), video_fps=30.):
    """Clip boundaries in frame-feature rows (get_clip2frm_idx_mapping, utils/video_feature/convert_feature_frm_to_clip.py:
    40-62): the extractor kept frames `frames_in_second` of every second of a `video_fps` video, so feature row j shows second
    j // k + frames_in_second[j % k] / video_fps; boundary c is the number of rows before c * clip_length seconds, and clip c is
    rows [b[c], b[c + 1]).  The defaults give 200 boundaries 0 5 9 14 18 23 27 32 ...: clips of 4 or 5 frames."""
    sec = np.arange(0, max_video_length)
    times = (np.asarray(frames_in_second)[None, :] / video_fps + sec[:, None]).reshape(-1)
    return np.searchsorted(times, np.arange(0, max_video_length, clip_length))


def sentence_word_ranges(sub_times, sentence_lengths, n_clips, clip_length=1.5):
    """Word-row range of every clip of one video (process_single_vid_sub + the range logic of convert_h5,
    utils/text_feature/convert_sub_feature_word_to_clip.py:19-32,68-86).  sub_times (n_sub, 2): start / end seconds of the
    subtitle sentences in file order; sentence_lengths (num_sens,): word rows per sentence in the word store (num_sens may be
    below n_sub).  Sentence s is taken by clips floor(st / clip_length) .. ceil(ed / clip_length) - 1 (float32 arithmetic, as
    there); sentence numbers are clamped to num_sens - 1; a clip's words run from the start of its first sentence to the end of
    its last.  -> (n_clips, 2) int64 [lo, hi) relative to the video's first word row; [0, 0] where no sentence touches the
    clip or the range holds no words."""
    n_clips = int(n_clips)
    out = np.zeros((n_clips, 2), dtype=np.int64)
    t = np.asarray(sub_times, dtype=np.float32).reshape(-1, 2) / clip_length
    lens = np.asarray(sentence_lengths, dtype=np.int64).reshape(-1)
    num_sens = len(lens)
    if n_clips == 0 or len(t) == 0 or num_sens == 0:
        return out
    word_start = np.concatenate([[0], np.cumsum(lens)])
    st = np.floor(t[:, 0]).astype(np.int64)
    ed = np.ceil(t[:, 1]).astype(np.int64)
    first = np.full(n_clips, -1, dtype=np.int64)          # lowest and highest sentence that touches each clip
    last = np.full(n_clips, -1, dtype=np.int64)
    for s in range(len(t)):
        a, b = max(int(st[s]), 0), min(int(ed[s]), n_clips)
        if a < b:
            first[a:b] = np.where(first[a:b] < 0, s, np.minimum(first[a:b], s))
            last[a:b] = np.maximum(last[a:b], s)
    hit = first >= 0
    lo = word_start[np.minimum(first[hit], num_sens - 1)]
    hi = word_start[np.minimum(last[hit], num_sens - 1) + 1]
    lo, hi = np.where(lo == hi, 0, lo), np.where(lo == hi, 0, hi)
    out[hit, 0], out[hit, 1] = lo, hi
    return out


class PooledStore(object):
    """Clip rows that are POOLED on the device from finer rows: sources = 1 or 2 tuples (FeatureStore, ranges, normalize), in
    column order (ResNet, then I3D).  ranges is either
      a 1-D boundary array b shared by every video (frame_clip_boundaries): clip c of a video of F rows is rows
        [b[c], min(b[c + 1], F)); the video has the clips before the first empty one, as convert_for_single_h5 breaks there
        (convert_feature_frm_to_clip.py:29-32) -- at most len(b) - 1;
      or a mapping name -> (n_clips, 2) [lo, hi) relative to the video's first row (sentence_word_ranges); lo == hi: no rows,
        the clip's block is zero.
    normalize: x / (||x|| + 1e-5) on that source's pooled block (normalize_and_concat.py).  pool: "max" or "mean".
    ContextFeeder(video_store= / sub_store=) takes a PooledStore in place of a FeatureStore; n_rows / dim are in CLIPS and
    output columns, like a clip store's."""

    def __init__(self, sources, pool="max"):
        sources = list(sources)
        if len(sources) not in (1, 2):
            raise ValueError("PooledStore: 1 or 2 sources expected, got %d" % len(sources))
        if pool not in ("max", "mean"):
            raise ValueError("PooledStore: pool must be 'max' or 'mean', got %r" % (pool,))
        self.pool, self.stores, self.ranges, self.norms = pool, [], [], []
        for store, ranges, normalize in sources:
            if not isinstance(ranges, dict):
                ranges = np.asarray(ranges)
                if ranges.ndim != 1 or len(ranges) < 2 or not np.issubdtype(ranges.dtype, np.integer) or \
                        ranges[0] < 0 or (np.diff(ranges) < 0).any():
                    raise ValueError("PooledStore: a shared boundary array must be 1-D, integer, non-negative and rising, with "
                                     "at least 2 entries")
                ranges = ranges.astype(np.int64)
            self.stores.append(store)
            self.ranges.append(ranges)
            self.norms.append(bool(normalize))
        self.dim = sum(int(s.dim) for s in self.stores)
        self._cache = {}

    def __contains__(self, name):
        return all(name in s for s in self.stores)

    def _source_ranges(self, si, name):
        store, rg = self.stores[si], self.ranges[si]
        rows = int(store.index[name][1])
        if isinstance(rg, dict):
            r = np.asarray(rg[name], dtype=np.int64).reshape(-1, 2)
            if ((r[:, 0] < 0) | (r[:, 0] > r[:, 1]) | (r[:, 1] > rows)).any():
                raise ValueError("PooledStore: a range of %r lies outside 0 <= lo <= hi <= %d rows of source %d" % (name, rows, si))
            return r
        lo, hi = rg[:-1], np.minimum(rg[1:], rows)
        empty = hi - lo <= 0
        n = int(np.argmax(empty)) if empty.any() else len(lo)
        return np.stack([lo[:n], hi[:n]], axis=1)

    def clip_ranges(self, name):
        """Per source the (n_clips, 2) int64 [lo, hi) ranges of the video's clips, relative to its first row in that source."""
        got = self._cache.get(name)
        if got is None:
            got = [self._source_ranges(si, name) for si in range(len(self.stores))]
            if len({len(r) for r in got}) != 1:
                raise ValueError("PooledStore: the sources disagree on the clip count of %r: %s"
                                 % (name, " / ".join(str(len(r)) for r in got)))
            self._cache[name] = got
        return got

    def n_rows(self, name):
        """clips of the video"""
        return len(self.clip_ranges(name)[0])

    def __getitem__(self, name):
        """The video's clip rows, (n_clips, dim) float32, pooled on the HOST: the reference's scripts stage by stage in the numpy
        expressions of tests/ingest_pool_ref.py -- np.max / np.mean over each range in float32, a zero block for an empty range,
        x / (||x|| + 1e-5) per normalised source, concatenation.  StoreTrainDataset / StoreEvalDataset take a PooledStore through
        it (store[name][:max_len], then their own row norm); it is the host statement of the device paths."""
        f = np.max if self.pool == "max" else np.mean
        blocks = []
        for store, rg, norm in zip(self.stores, self.clip_ranges(name), self.norms):
            src = store[name]
            block = np.zeros((len(rg), int(store.dim)), dtype=np.float32)
            for c in range(len(rg)):
                lo, hi = int(rg[c, 0]), int(rg[c, 1])
                x = f(src[lo:hi].astype(np.float32), axis=0) if lo < hi else block[c]
                block[c] = x / (np.sqrt((x * x).sum(dtype=np.float32), dtype=np.float32) + np.float32(1e-5)) if norm else x
            blocks.append(block)
        return np.concatenate(blocks, axis=1)


class PartTable(object):
    """Which index rows make up which video, for corpora with videos longer than max_ctx_len.
    A long video is stored as several overlapping PARTS, each an ordinary index row of <= max_ctx_len clips; the parts of a
    video are adjacent rows, in offset order.
      part_video  (n_parts,)      int32  source video of each index row
      part_offset (n_parts,)      int32  first clip of the row in its source video
      part_len    (n_parts,)      int32  clips of the row
      group_start (n_videos + 1,) int32  CSR over the index rows: video v owns rows group_start[v] : group_start[v + 1]
    plan_parts() makes the host table (numpy arrays); .to(device) returns the copy with int32 tensors on that device, which is
    what build_corpus_index(parts=) keeps on the index and the device ops take."""

    def __init__(self, part_video, part_offset, part_len, group_start, max_ctx_len, overlap):
        on_device = torch.is_tensor(part_video)
        if on_device:
            pv, po, pl, gs = (t.detach().cpu().numpy() for t in (part_video, part_offset, part_len, group_start))
        else:
            pv, po, pl, gs = (np.asarray(a) for a in (part_video, part_offset, part_len, group_start))
        self.max_ctx_len, self.overlap = int(max_ctx_len), int(overlap)
        if self.max_ctx_len < 1 or not 0 <= self.overlap < self.max_ctx_len:
            raise ValueError("PartTable: 0 <= overlap < max_ctx_len is required, got overlap %d, max_ctx_len %d"
                             % (self.overlap, self.max_ctx_len))
        for a, name in ((pv, "part_video"), (po, "part_offset"), (pl, "part_len"), (gs, "group_start")):
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("PartTable: %s must be a 1-D integer array" % name)
        n_parts, n_videos = len(pv), len(gs) - 1
        if n_videos < 1 or len(po) != n_parts or len(pl) != n_parts:
            raise ValueError("PartTable: part_video / part_offset / part_len must have one entry per part and group_start "
                             "n_videos + 1 >= 2 entries; got %d / %d / %d / %d" % (len(pv), len(po), len(pl), len(gs)))
        if gs[0] != 0 or gs[-1] != n_parts or (np.diff(gs) < 1).any():
            raise ValueError("PartTable: group_start must rise strictly from 0 to n_parts = %d (every video has a part)"
                             % n_parts)
        if not np.array_equal(pv, np.repeat(np.arange(n_videos), np.diff(gs))):
            raise ValueError("PartTable: the parts of a video must be adjacent index rows, videos in order: part_video must "
                             "equal the video of each row's group_start range")
        if (pl < 1).any() or (pl > self.max_ctx_len).any() or (po < 0).any():
            raise ValueError("PartTable: every part needs 1 <= part_len <= max_ctx_len = %d and part_offset >= 0"
                             % self.max_ctx_len)
        first = gs[:-1]
        inner = np.ones(n_parts, dtype=bool)
        inner[first] = False
        if (po[first] != 0).any() or (np.diff(po)[inner[1:]] < 1).any():
            raise ValueError("PartTable: the parts of a video must start at offset 0 and follow in rising offset order")
        if on_device:
            self.part_video, self.part_offset, self.part_len, self.group_start = (
                t.to(torch.int32).contiguous() for t in (part_video, part_offset, part_len, group_start))
        else:
            self.part_video, self.part_offset, self.part_len, self.group_start = (
                np.ascontiguousarray(a, dtype=np.int32) for a in (pv, po, pl, gs))
        self.n_parts, self.n_videos = int(n_parts), int(n_videos)

    @property
    def device(self):
        return self.part_video.device if torch.is_tensor(self.part_video) else None

    def n_clips(self):
        """(n_videos,) clips of each source video = end of its last part (host array)."""
        po, pl, gs = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in (self.part_offset, self.part_len, self.group_start))
        last = gs[1:] - 1
        return (po[last] + pl[last]).astype(np.int32)

    def to(self, device):
        """The table with int32 tensors on `device` (already validated: the copy is not checked again)."""
        t = object.__new__(PartTable)
        t.__dict__.update(self.__dict__)
        t.part_video, t.part_offset, t.part_len, t.group_start = (
            torch.as_tensor(a, dtype=torch.int32).to(device).contiguous()
            for a in (self.part_video, self.part_offset, self.part_len, self.group_start))
        return t

    def meta2vid(self, video_ids=None):
        """K10's table for an index of parts: index row -> the caller's id of its source video.  video_ids (n_videos,)
        int32, source video -> id (None: the source-video number itself); array or tensor on the table's side."""
        if video_ids is None:
            return self.part_video
        if torch.is_tensor(self.part_video):
            ids = torch.as_tensor(video_ids, dtype=torch.int32).to(self.part_video.device)
            if ids.dim() != 1 or ids.numel() != self.n_videos:
                raise ValueError("PartTable.meta2vid: %d ids for %d source videos" % (ids.numel(), self.n_videos))
            return ids.index_select(0, self.part_video.long()).contiguous()
        ids = np.asarray(video_ids.cpu() if torch.is_tensor(video_ids) else video_ids, dtype=np.int32)
        if ids.ndim != 1 or len(ids) != self.n_videos:
            raise ValueError("PartTable.meta2vid: %d ids for %d source videos" % (ids.size, self.n_videos))
        return np.ascontiguousarray(ids[self.part_video])


def plan_parts(n_clips, max_ctx_len, overlap=16):
    """The part plan of a corpus: n_clips (n_videos,) clips per video -> PartTable (host).
    W = max_ctx_len, O = overlap, S = W - O.  A video of n <= W clips is one part (0, n); a video of n > W clips gets parts of
    W clips at offsets 0, S, 2S, ... for every offset with offset + W < n, and one last part at n - W: 1 + ceil((n - W) / S)
    parts.  Every window of <= O clips of the video (K9's candidates: at most max_pred_l <= O clips) lies inside a part."""
    w, o = int(max_ctx_len), int(overlap)
    if w < 1 or not 0 <= o < w:
        raise ValueError("plan_parts: 0 <= overlap < max_ctx_len is required, got overlap %d, max_ctx_len %d" % (o, w))
    n = np.asarray(n_clips)
    if n.ndim != 1 or n.size < 1 or not np.issubdtype(n.dtype, np.integer) or (n < 1).any():
        raise ValueError("plan_parts: n_clips must be a non-empty 1-D integer array of clip counts >= 1")
    n = n.astype(np.int64)
    s = w - o
    count = np.where(n > w, 1 + (np.maximum(n - w, 0) + s - 1) // s, 1)
    gs = np.concatenate([[0], np.cumsum(count)])
    if gs[-1] > np.iinfo(np.int32).max:
        raise ValueError("plan_parts: %d parts do not fit int32 row numbers" % gs[-1])
    pv = np.repeat(np.arange(len(n)), count)
    j = np.arange(gs[-1]) - gs[:-1][pv]                       # number of the part inside its video
    nv = n[pv]
    po = np.where(j == count[pv] - 1, np.maximum(nv - w, 0), j * s)
    pl = np.minimum(nv, w)
    return PartTable(pv.astype(np.int32), po.astype(np.int32), pl.astype(np.int32), gs.astype(np.int32), w, o)


def _resolve_ctx_mode(who, ctx_mode, video_store, sub_store):
    """ctx_mode=None: the streams are those whose stores are given, no endpoint columns.  Else one of train_data.CTX_MODES, which
    must name exactly the streams whose stores are given.  -> whether the mode appends the temporal endpoint columns."""
    if ctx_mode is None:
        return False
    if ctx_mode not in CTX_MODES:
        raise ValueError("%s: ctx_mode %r: the model has %s (the endpoint columns ride on a video or subtitle stream)"
                         % (who, ctx_mode, ", ".join(CTX_MODES)))
    parts = ctx_mode.split("_")
    for tag, store in (("video", video_store), ("sub", sub_store)):
        if tag in parts and store is None:
            raise ValueError("%s: ctx_mode %r needs a %s store" % (who, ctx_mode, tag))
        if tag not in parts and store is not None:
            raise ValueError("%s: a %s store is given, ctx_mode %r has no %s stream" % (who, tag, ctx_mode, tag))
    return "tef" in parts


class ContextFeeder(object):
    """Raw clip rows leave the host in the STORE's dtype (f16 on disk: half the PCIe bytes of the reference's f32 batches)
    and back to back -- runs of videos that are adjacent in the store are ONE copy from the memory map into the pinned
    staging buffer, spread over `host_threads` threads --; truncation, padding, the mask, the conversion and the per-clip
    normalisation happen in one device launch (xml_ingest_rows).  Two staging buffers alternate, the copy runs on a side
    stream: the H2D of batch i + 1 overlaps the encoder kernels of batch i.
    stats (after iterating): rows / bytes moved and the seconds the host spent gathering."""

    def __init__(self, video_names, video_store=None, sub_store=None, max_ctx_len=100, batch_size=200,
                 normalize_vfeat=True, normalize_tfeat=True, device="cuda:0", ops=hip_ops, feature_dtype=torch.float32,
                 host_threads=8, parts=None, ctx_mode=None):
        """feature_dtype=torch.bfloat16 (bf16 models only): the normalised features are handed over in bf16 -- the encoder's
        input LayerNorm reads half the bytes (the C ABI takes f32 or the compute dtype); the reference's contract is f32.
        parts (PartTable of plan_parts over these videos' clip counts, host): nothing is cut off -- the feeder iterates batches
        of PARTS, each the rows [offset, offset + len) of its video in the store; rows that two parts share are copied twice.
        video_store / sub_store may be a PooledStore (frame- / word-level rows): the fine rows a batch's clips name are staged
        and copied instead, and xml_ingest_pool_rows pools them into clips in the collate launch; stats then count fine rows.
        ctx_mode (None, or one of train_data.CTX_MODES naming exactly the given stores): with a *_tef mode every feature tensor
        is two columns wider -- the reference's temporal endpoint feature (start_end_dataset.py:328-342), written by the same
        launch (xml_ingest_rows_tef / xml_ingest_pool_rows_tef).  The time axis is the truncated video, as there; with parts it
        is the WHOLE video: a part's columns are the columns the unsplit video has at those clips."""
        self.use_tef = _resolve_ctx_mode("ContextFeeder", ctx_mode, video_store, sub_store)
        self.ctx_mode = ctx_mode
        self.feature_dtype = feature_dtype
        self.names, self.vs, self.ss = list(video_names), video_store, sub_store
        self.max_ctx_len, self.bsz = int(max_ctx_len), int(batch_size)
        if self.use_tef and parts is None and video_store is not None and sub_store is not None:
            for n in self.names:       # one endpoint feature serves both streams: the reference fails in torch.cat here
                lv, ls = (min(int(st.n_rows(n)), self.max_ctx_len) for st in (video_store, sub_store))
                if lv != ls:
                    raise ValueError("ContextFeeder: video %r has %d video and %d subtitle clips after truncation; ctx_mode %r "
                                     "appends one temporal endpoint feature to both" % (n, lv, ls, ctx_mode))
        self.parts = parts
        if parts is not None:
            if torch.is_tensor(parts.part_video):
                raise ValueError("ContextFeeder: parts must be the host table (plan_parts), not its device copy")
            if parts.n_videos != len(self.names) or parts.max_ctx_len != self.max_ctx_len:
                raise ValueError("ContextFeeder: the part table covers %d videos at max_ctx_len %d, the feeder %d at %d"
                                 % (parts.n_videos, parts.max_ctx_len, len(self.names), self.max_ctx_len))
            counts = parts.n_clips()
            self._part_total = counts
            for tag, store in (("video", video_store), ("sub", sub_store)):
                if store is None:
                    continue
                if isinstance(store, PooledStore):
                    have = np.array([store.n_rows(n) for n in self.names], dtype=np.int64)
                else:
                    have = np.array([store.index[n][1] for n in self.names], dtype=np.int64)
                if (have != counts).any():
                    i = int(np.nonzero(have != counts)[0][0])
                    raise ValueError("ContextFeeder: the part table was planned for %d clips of %r, the %s store holds %d "
                                     "(with parts, the video and subtitle stores must hold the same clip count per video)"
                                     % (counts[i], self.names[i], tag, have[i]))
        self.norm = dict(video=normalize_vfeat, sub=normalize_tfeat)
        self.device, self.ops = torch.device(device), ops
        self._stage = {}
        self._slot_done = {}     # (tag, slot) -> event recorded after the H2D copy that last read this pinned slot
        self._pool = None
        self.host_threads = max(1, int(host_threads))
        self.stats = dict(rows=0, h2d_bytes=0, gather_s=0.0)

    def _n_items(self):
        return len(self.names) if self.parts is None else self.parts.n_parts

    def _tef_kw(self, items, moved=None):
        """Keywords of the ingest op for this batch: none without a *_tef mode (the op is called as ever); tef=True, and with
        parts each part's place in its video (offset, whole clip count) as two (n,) int32 arrays -- copied like row_start: the
        caller is inside the copy stream's context and record_stream()s what is appended to `moved`."""
        if not self.use_tef:
            return {}
        if self.parts is None:
            return dict(tef=True)
        pt = self.parts
        rows = np.arange(items.start, items.stop)
        pos = torch.from_numpy(np.ascontiguousarray(pt.part_offset[rows], dtype=np.int32))
        tot = torch.from_numpy(np.ascontiguousarray(self._part_total[pt.part_video[rows]], dtype=np.int32))
        if self.device.type == "cuda":
            pos, tot = pos.to(self.device, non_blocking=True), tot.to(self.device, non_blocking=True)
            moved += [pos, tot]
        return dict(tef=True, tef_pos=pos, tef_len=tot)

    def __len__(self):
        return (self._n_items() + self.bsz - 1) // self.bsz

    def _staging(self, key, rows, store):
        buf = self._stage.get(key)
        if buf is None or buf.shape[0] < rows:
            cap = max(rows, min(self.bsz, self._n_items()) * self.max_ctx_len)
            buf = torch.empty((cap, store.dim), dtype=_TORCH_DT[store.dtype])
            if self.device.type == "cuda":
                buf = buf.pin_memory()
            self._stage[key] = buf
        return buf

    def _gather(self, store, items, slot, tag):
        """items: the batch's video names, or with a part table its range of index rows -> (pinned (rows, D) buffer in the
        store dtype holding the batch's truncated videos (or parts) back to back, rows, row_start (n + 1) int64, lmax)"""
        import time
        t0 = time.perf_counter()
        if self.parts is None:
            idx = [store.index[n] for n in items]
        else:       # a part is the sub-range [first + offset, + len) of its video's rows
            pt = self.parts
            idx = [[store.index[self.names[pt.part_video[p]]][0] + int(pt.part_offset[p]), int(pt.part_len[p])] for p in items]
        lens = np.minimum(np.array([i[1] for i in idx], dtype=np.int64), self.max_ctx_len)
        start = np.concatenate([[0], np.cumsum(lens)])
        rows = int(start[-1])
        ev = self._slot_done.get((tag, slot))
        if ev is not None:       # batch i - 2 was copied from this pinned slot asynchronously: the host must not rewrite it
            ev.synchronize()     # before that copy has actually read it
        buf = self._staging((tag, slot), rows, store)
        out = buf.numpy()
        # runs: consecutive videos that are adjacent in the store and taken whole collapse into one copy
        runs, i = [], 0
        while i < len(idx):
            src, dst, n = idx[i][0], int(start[i]), int(lens[i])
            while i + 1 < len(idx) and lens[i] == idx[i][1] and idx[i + 1][0] == idx[i][0] + idx[i][1]:
                i += 1
                n += int(lens[i])
            runs.append((src, dst, n))
            i += 1
        chunk = max(1, (8 << 20) // (store.dim * out.itemsize))              # ~8 MB pieces
        jobs = [(s + o, d + o, min(chunk, n - o)) for s, d, n in runs for o in range(0, n, chunk)]

        def copy(j):
            out[j[1]:j[1] + j[2]] = store.data[j[0]:j[0] + j[2]]             # (numpy releases the GIL inside the copy loop)
        if len(jobs) > 1 and self.host_threads > 1:
            if self._pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(self.host_threads)
            list(self._pool.map(copy, jobs))
        else:
            for j in jobs:
                copy(j)
        self.stats["gather_s"] += time.perf_counter() - t0
        return buf, rows, torch.from_numpy(start), int(lens.max())

    def _gather_pooled(self, pstore, items, slot, tag):
        """The batch of a PooledStore: per source only the fine rows that the items' clips (a video's first max_ctx_len, or a
        part's) name -- per item the span from the first to the last of them -- go back to back into the pinned buffer, and seg
        (R, 2) int64 holds each clip row's range RELATIVE TO THAT BUFFER ([0, 0]: no rows).  -> ([(buffer, rows, seg)] per
        source, row_start (n + 1) int64 over the clip rows, lmax)"""
        import time
        t0 = time.perf_counter()
        if self.parts is None:
            clips = [(n, 0, min(pstore.n_rows(n), self.max_ctx_len)) for n in items]
        else:
            pt = self.parts
            clips = [(self.names[pt.part_video[p]], int(pt.part_offset[p]), int(pt.part_len[p])) for p in items]
        lens = np.array([c[2] for c in clips], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(lens)])
        per_source = []
        for si, store in enumerate(pstore.stores):
            seg = np.zeros((int(start[-1]), 2), dtype=np.int64)
            runs, rows = [], 0
            for k, (name, c0, ln) in enumerate(clips):
                r = pstore.clip_ranges(name)[si][c0:c0 + ln]
                full = r[:, 1] > r[:, 0]
                if not full.any():
                    continue
                lo, hi = int(r[full, 0].min()), int(r[full, 1].max())
                seg[int(start[k]):int(start[k + 1])] = np.where(full[:, None], r - lo + rows, 0)
                src = int(store.index[name][0]) + lo
                if runs and runs[-1][0] + runs[-1][2] == src:          # adjacent in the store: one copy
                    runs[-1] = (runs[-1][0], runs[-1][1], runs[-1][2] + hi - lo)
                else:
                    runs.append((src, rows, hi - lo))
                rows += hi - lo
            key = (tag, slot, si)
            ev = self._slot_done.get(key)
            if ev is not None:       # the copy that last read this pinned slot must have finished before it is rewritten
                ev.synchronize()
            buf = self._stage.get(key)
            if buf is None or buf.shape[0] < max(rows, 1):
                buf = torch.empty((max(int(rows * 1.25), 1), store.dim), dtype=_TORCH_DT[store.dtype])
                if self.device.type == "cuda":
                    buf = buf.pin_memory()
                self._stage[key] = buf
            out = buf.numpy()
            chunk = max(1, (8 << 20) // (store.dim * out.itemsize))              # ~8 MB pieces
            jobs = [(s + o, d + o, min(chunk, n - o)) for s, d, n in runs for o in range(0, n, chunk)]

            def copy(j, out=out, store=store):
                out[j[1]:j[1] + j[2]] = store.data[j[0]:j[0] + j[2]]
            if len(jobs) > 1 and self.host_threads > 1:
                if self._pool is None:
                    from concurrent.futures import ThreadPoolExecutor
                    self._pool = ThreadPoolExecutor(self.host_threads)
                list(self._pool.map(copy, jobs))
            else:
                for j in jobs:
                    copy(j)
            per_source.append((buf, rows, torch.from_numpy(seg)))
        self.stats["gather_s"] += time.perf_counter() - t0
        return per_source, torch.from_numpy(start), int(lens.max())

    def _pooled_batch(self, pstore, items, slot, tag, copy_stream):
        """[features, mask] of one batch of a PooledStore: stage, copy on the side stream, one xml_ingest_pool_rows launch."""
        per_source, start, lmax = self._gather_pooled(pstore, items, slot, tag)
        cuda = self.device.type == "cuda"
        sources = []
        if cuda:
            cur = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(copy_stream):
                dstart = start.to(self.device, non_blocking=True)
                moved = [dstart]
                for si, (host, rows, seg) in enumerate(per_source):
                    dev = host[:max(rows, 1)].to(self.device, non_blocking=True)      # (no rows: one unread row, never NULL)
                    dseg = seg.to(self.device, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(copy_stream)
                    self._slot_done[(tag, slot, si)] = done
                    sources.append((dev, dseg, pstore.norms[si]))
                    moved += [dev, dseg]
                tef_kw = self._tef_kw(items, moved)
            cur.wait_stream(copy_stream)
            for t in moved:                      # allocated on the copy stream, consumed on the compute stream
                t.record_stream(cur)
        else:
            dstart = start
            for si, (host, rows, seg) in enumerate(per_source):
                sources.append((host[:max(rows, 1)].clone(), seg, pstore.norms[si]))
            tef_kw = self._tef_kw(items)
        for si, (host, rows, seg) in enumerate(per_source):
            self.stats["rows"] += rows
            self.stats["h2d_bytes"] += rows * pstore.stores[si].dim * host.element_size()
        feat, mask = self.ops.ingest_pool_rows(sources, dstart, len(items), lmax, self.max_ctx_len, pool=pstore.pool,
                                               normalize=self.norm[tag], eps=1e-5, out_dtype=self.feature_dtype, **tef_kw)
        return [feat, mask]

    def __iter__(self):
        cuda = self.device.type == "cuda"
        copy_stream = torch.cuda.Stream(self.device) if cuda else None
        for bi, b in enumerate(range(0, self._n_items(), self.bsz)):
            names = self.names[b:b + self.bsz] if self.parts is None else range(b, min(b + self.bsz, self.parts.n_parts))
            out = []
            for tag, store in (("video", self.vs), ("sub", self.ss)):
                if store is None:
                    out += [None, None]
                    continue
                if isinstance(store, PooledStore):
                    out += self._pooled_batch(store, names, bi & 1, tag, copy_stream)
                    continue
                host, rows, start, lmax = self._gather(store, names, bi & 1, tag)
                self.stats["rows"] += rows
                self.stats["h2d_bytes"] += rows * store.dim * host.element_size()
                if cuda:
                    with torch.cuda.stream(copy_stream):
                        dev = host[:rows].to(self.device, non_blocking=True)
                        dstart = start.to(self.device, non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(copy_stream)
                        moved = [dev, dstart]
                        tef_kw = self._tef_kw(names, moved)
                    self._slot_done[(tag, bi & 1)] = done
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_stream(copy_stream)
                    for t in moved:                 # allocated on the copy stream and consumed on the compute stream: keep
                        t.record_stream(cur)        # the allocator from recycling them early
                else:
                    dev, dstart = host[:rows].clone(), start
                    tef_kw = self._tef_kw(names)
                feat, mask = self.ops.ingest_rows(dev, dstart, len(names), lmax, self.max_ctx_len, normalize=self.norm[tag],
                                                  eps=1e-5, out_dtype=self.feature_dtype, **tef_kw)
                out += [feat, mask]
            yield tuple(out)


class StoreEvalDataset(object):
    """Reference eval-dataset contract over FeatureStores.  query_data: list of dicts with desc_id, desc, vid_name
    (+ ts/type for evaluation); video_data: list of dicts with vid_name, duration; video2idx: name -> int."""

    def __init__(self, query_data, video_data, video2idx, desc_store, video_store=None, sub_store=None, max_desc_len=30,
                 max_ctx_len=100, normalize_vfeat=True, normalize_tfeat=True, ctx_mode=None):
        """ctx_mode (None, or one of train_data.CTX_MODES naming exactly the given stores): with a *_tef mode the context items
        end in the two temporal endpoint columns, computed as the reference does (start_end_dataset.py:328-342)."""
        self.use_tef = _resolve_ctx_mode("StoreEvalDataset", ctx_mode, video_store, sub_store)
        self.ctx_mode = ctx_mode
        self.query_data, self.video_data, self.video2idx = query_data, video_data, video2idx
        self.desc, self.vs, self.ss = desc_store, video_store, sub_store
        self.max_desc_len, self.max_ctx_len = max_desc_len, max_ctx_len
        self.nv, self.nt = normalize_vfeat, normalize_tfeat
        self.data_mode, self.load_gt_video = "query", False

    def set_data_mode(self, mode):
        assert mode in ("context", "query")
        self.data_mode = mode

    def load_gt_vid_name_for_query(self, flag):
        self.load_gt_video = flag

    def __len__(self):
        return len(self.query_data) if self.data_mode == "query" else len(self.video_data)

    @staticmethod
    def _norm(a):
        a = np.asarray(a, dtype=np.float32)
        return a / (np.linalg.norm(a, axis=-1, keepdims=True) + 1e-5)

    def __getitem__(self, i):
        if self.data_mode == "context":
            v = self.video_data[i]
            mi = {}
            ctx_l = 0
            if self.vs is not None:
                f = self.vs[v["vid_name"]][:self.max_ctx_len]
                mi["video_feat"] = self._norm(f) if self.nv else np.asarray(f, dtype=np.float32)
                ctx_l = len(f)
            if self.ss is not None:
                f = self.ss[v["vid_name"]][:self.max_ctx_len]
                mi["sub_feat"] = self._norm(f) if self.nt else np.asarray(f, dtype=np.float32)
                ctx_l = len(f)
            if self.use_tef:           # the reference's lines, on the stream it takes the length from (the subtitles' if any)
                tef_st = torch.arange(0, ctx_l, 1.0) / ctx_l
                tef = torch.stack([tef_st, tef_st + 1.0 / ctx_l], dim=1).numpy()
                for k in list(mi):
                    if len(mi[k]) != ctx_l:
                        raise ValueError("StoreEvalDataset: video %r has %d %s rows and %d endpoint rows after truncation; "
                                         "ctx_mode %r appends one temporal endpoint feature to both streams"
                                         % (v["vid_name"], len(mi[k]), k, ctx_l, self.ctx_mode))
                    mi[k] = np.concatenate([mi[k], tef], axis=1)
            return dict(meta=dict(vid_name=v["vid_name"], duration=v.get("duration", 0.0)), model_inputs=mi)
        q = self.query_data[i]
        f = self.desc[str(q["desc_id"])][:self.max_desc_len]
        meta = dict(desc_id=q["desc_id"], desc=q.get("desc", ""),
                    vid_name=q["vid_name"] if self.load_gt_video else None)
        return dict(meta=meta, model_inputs=dict(query_feat=self._norm(f) if self.nt else np.asarray(f, dtype=np.float32)))
