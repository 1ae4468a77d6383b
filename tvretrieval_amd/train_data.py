"""Training data path: the reference's StartEndDataset + start_end_collate + prepare_batch_inputs
(xml/start_end_dataset.py:21-168,346-370) and its train_epoch (xml/train.py:42-119) over `ingest.FeatureStore`s.

  StoreTrainDataset   the reference's training-dataset contract on the host (numpy): items with "meta" + "model_inputs"
                      (query_feat, video_feat, sub_feat, tef_feat, st_ed_indices), for users of the reference's own loop --
                      and the host statement the device path is tested against.  `collate` is start_end_collate +
                      prepare_batch_inputs for those items.
  DeviceTrainStore    the stores' rows uploaded ONCE in the store's dtype, plus the example tables (example -> description /
                      video item, row prefixes, the (N, 2) start / end labels).  `batch(ids)` builds the keyword dict
                      xml_forward_train takes with one xml_gather_feature_rows launch per stream and one xml_gather_index_rows
                      for the labels; `fill(static, ids)` writes the same batch into existing tensors (GraphedTrainStep.static).
                      Per step the host sends the example ids, nothing else.  The video and / or the subtitle store may
                      be an ingest.PooledStore (frame- / word-level rows): its fine rows stay resident with the absolute
                      source-row range of every clip, and that stream's launch is xml_gather_pool_feature_rows -- the clip
                      pooling, the per-source norms and the collate in the gather.
  train_epoch         the reference's epoch loop on a DeviceTrainStore, eager (train_step) or through a captured
                      GraphedTrainStep (fill + replay, losses read once at the end).

Fixed shapes (a captured step, `batch(ids, lmax=..., lq=...)`): a fixed lmax above a batch's own maximum differs from the
reference at the last conv_kernel_size // 2 clips of the batch's longest videos -- the ConvSE taps read encoder outputs at
padded positions where the reference's shorter tensor has the convolution's zero padding (the effect build_corpus_index's
docstring describes for the corpus).  This is inherent to fixed-shape capture and applies to GraphedTrainStep as such.
"""
import collections
import json
import math

import numpy as np
import torch

from . import ops as hip_ops

CTX_MODES = ("video", "sub", "video_sub", "video_tef", "sub_tef", "video_sub_tef")
LOSS_KEYS = ("loss_st_ed", "loss_neg_ctx", "loss_neg_q", "loss_overall")
_TORCH_DT = {"float16": torch.float16, "float32": torch.float32}


def didemo_agreed_ts(times_list):
    """get_didemo_agreed_ts: the most frequent (st, ed) pair; the first seen wins a tie."""
    counts = collections.OrderedDict()
    for e in times_list:
        counts[tuple(e)] = counts.get(tuple(e), 0) + 1
    best = max(counts.values())
    return next(k for k, c in counts.items() if c == best)


def st_ed_label(ts, clip_length, length):
    """get_st_ed_label (xml/start_end_dataset.py:147-162) in float64; `length` is the context length AFTER truncation."""
    return (min(int(math.floor(float(ts[0]) / clip_length)), length - 1),
            min(int(math.ceil(float(ts[1]) / clip_length)), length - 1))


def _load_examples(examples, data_ratio):
    if isinstance(examples, str):
        with open(examples) as f:
            examples = [json.loads(line) for line in f if line.strip()]
    examples = list(examples)
    if data_ratio != 1:
        examples = examples[:int(len(examples) * data_ratio)]
    return examples


def _l2norm(a, eps=1e-5):
    """l2_normalize_np_array (utils/basic_utils.py:82-84)"""
    return a / (np.linalg.norm(a, axis=-1, keepdims=True) + eps)


class StoreTrainDataset(object):
    """examples: list of dicts (or a jsonl path) with desc_id, desc, vid_name, duration, ts.  Items hold torch tensors that
    share memory with the numpy arrays they were computed in, so the reference's start_end_collate takes them as they are."""

    def __init__(self, examples, desc_store, video_store=None, sub_store=None, dset_name="tvr", max_desc_len=30,
                 max_ctx_len=100, clip_length=1.5, ctx_mode="video_sub", normalize_vfeat=True, normalize_tfeat=True,
                 data_ratio=1.0):
        if ctx_mode not in CTX_MODES:
            raise ValueError("ctx_mode %r: the model has %s" % (ctx_mode, ", ".join(CTX_MODES)))
        self.data = _load_examples(examples, data_ratio)
        self.dset_name, self.ctx_mode = dset_name, ctx_mode
        self.desc, self.vs, self.ss = desc_store, video_store, sub_store
        self.max_desc_len, self.max_ctx_len, self.clip_length = int(max_desc_len), int(max_ctx_len), clip_length
        self.use_video, self.use_sub, self.use_tef = "video" in ctx_mode, "sub" in ctx_mode, "tef" in ctx_mode
        if (self.use_video and video_store is None) or (self.use_sub and sub_store is None):
            raise ValueError("ctx_mode %r needs a %s store" % (ctx_mode, "video" if video_store is None else "sub"))
        self.normalize_vfeat, self.normalize_tfeat = normalize_vfeat, normalize_tfeat

    def __len__(self):
        return len(self.data)

    def _ts(self, raw):
        return raw["ts"] if self.dset_name != "didemo" else didemo_agreed_ts(raw["ts"])

    def _feat(self, store, name, max_len, normalize):
        a = np.array(store[name][:max_len], dtype=np.float32)           # (a copy: the memory map is read-only)
        return np.ascontiguousarray(_l2norm(a), dtype=np.float32) if normalize else a

    def __getitem__(self, index):
        raw = self.data[index]
        meta = dict(desc_id=raw["desc_id"], desc=raw.get("desc", ""), vid_name=raw["vid_name"],
                    duration=raw.get("duration", 0.0), ts=self._ts(raw))
        mi = dict(query_feat=torch.from_numpy(self._feat(self.desc, str(meta["desc_id"]), self.max_desc_len,
                                                         self.normalize_tfeat)))
        ctx_l = 0
        for key, use, store, norm in (("video_feat", self.use_video, self.vs, self.normalize_vfeat),
                                      ("sub_feat", self.use_sub, self.ss, self.normalize_tfeat)):
            if use:
                mi[key] = torch.from_numpy(self._feat(store, meta["vid_name"], self.max_ctx_len, norm))
                ctx_l = len(mi[key])
            else:
                mi[key] = torch.zeros((2, 2))
        if self.use_tef:
            tef_st = torch.arange(0, ctx_l, 1.0) / ctx_l
            mi["tef_feat"] = torch.stack([tef_st, tef_st + 1.0 / ctx_l], dim=1)
            for key, use in (("video_feat", self.use_video), ("sub_feat", self.use_sub)):
                if use:
                    mi[key] = torch.cat([mi[key], mi["tef_feat"]], dim=1)
        else:
            mi["tef_feat"] = torch.zeros((2, 2))
        mi["st_ed_indices"] = torch.LongTensor(list(st_ed_label(meta["ts"], self.clip_length, ctx_l)))
        return dict(meta=meta, model_inputs=mi)


def collate(items, use_video=True, use_sub=True, lmax=None, lq=None):
    """start_end_collate + prepare_batch_inputs on the host: zero padding to the batch maximum (or to lmax / lq) and float
    masks -> (list of meta, dict of numpy arrays keyed like XML.forward's arguments; None for an unused modality)."""
    def pad(seqs, fixed):
        seqs = [np.asarray(s, dtype=np.float32) for s in seqs]
        length = max(len(s) for s in seqs) if fixed is None else int(fixed)
        out = np.zeros((len(seqs), length) + seqs[0].shape[1:], np.float32)
        mask = np.zeros((len(seqs), length), np.float32)
        for i, s in enumerate(seqs):
            out[i, :len(s)] = s
            mask[i, :len(s)] = 1
        return out, mask
    mi = [e["model_inputs"] for e in items]
    batch = {}
    for key, use, fixed in (("query", True, lq), ("video", use_video, lmax), ("sub", use_sub, lmax)):
        batch[key + "_feat"], batch[key + "_mask"] = pad([m[key + "_feat"] for m in mi], fixed) if use else (None, None)
    batch["st_ed_indices"] = np.stack([np.asarray(m["st_ed_indices"], dtype=np.int64) for m in mi])
    return [e["meta"] for e in items], batch


# ---------------------------------------------------------------------------------------------------------
# device-resident store
# ---------------------------------------------------------------------------------------------------------
def _store_items(store, what):
    """-> (names in row order, row_start (n_items + 1) int64).  A FeatureStore's rows lie back to back."""
    names = sorted(store.index, key=lambda k: store.index[k][0])
    first = np.array([store.index[k][0] for k in names], dtype=np.int64)
    rows = np.array([store.index[k][1] for k in names], dtype=np.int64)
    empty = np.flatnonzero(rows <= 0)
    if len(empty):
        raise ValueError("%s store: item %r has zero rows" % (what, names[int(empty[0])]))
    start = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    if not np.array_equal(first, start[:-1]):
        raise ValueError("%s store: rows are not laid back to back" % what)
    return names, start


def _upload_rows(store, total, device, chunk_bytes):
    """The first `total` rows of a FeatureStore -> a device tensor in the store's dtype."""
    dim, dt = int(store.dim), _TORCH_DT[store.dtype]
    rows = torch.empty((total, dim), dtype=dt, device=device)
    # memory map -> pinned chunks (two, alternating) -> device
    step = max(1, chunk_bytes // (dim * rows.element_size()))
    cuda = torch.device(device).type == "cuda"
    stage = [torch.empty((min(step, total), dim), dtype=dt, pin_memory=cuda) for _ in range(2 if cuda else 1)]
    done = [None, None]
    for ci, a in enumerate(range(0, total, step)):
        b, s = min(a + step, total), ci % len(stage)
        if done[s] is not None:
            done[s].synchronize()
        stage[s].numpy()[:b - a] = store.data[a:b]
        rows[a:b].copy_(stage[s][:b - a], non_blocking=True)
        if cuda:
            done[s] = torch.cuda.Event()
            done[s].record()
    if cuda:
        torch.cuda.current_stream(device).synchronize()
    return rows


class _Resident(object):
    """One FeatureStore on the device: rows in the store's dtype + the row prefix."""
    pooled = False

    def __init__(self, store, what, device, chunk_bytes=64 << 20):
        self.names, start = _store_items(store, what)
        self.item = {k: i for i, k in enumerate(self.names)}
        self.rows_of = np.diff(start)
        self.dim = int(store.dim)
        self.row_start = torch.from_numpy(start).to(device)
        self.rows = _upload_rows(store, int(start[-1]), device, chunk_bytes)
        self.nbytes = self.rows.numel() * self.rows.element_size() + self.row_start.numel() * 8


class _PooledResident(object):
    """One ingest.PooledStore on the device: every source's FINE rows in the store's dtype, the items (the names all sources
    hold, in the first source's row order), clip_start (n_items + 1) over one clip numbering, and per source the (clips, 2)
    table of ABSOLUTE source-row ranges: PooledStore.clip_ranges(name) plus the item's first row in that source.  Raises
    ValueError, by name, where the sources disagree on a clip count or a range lies outside its source (clip_ranges)."""
    pooled = True

    def __init__(self, pstore, what, device, chunk_bytes=64 << 20):
        first = pstore.stores[0]
        self.names = [k for k in sorted(first.index, key=lambda k: first.index[k][0]) if k in pstore]
        if not self.names:
            raise ValueError("%s store: the sources share no item" % what)
        self.item = {k: i for i, k in enumerate(self.names)}
        self.dim, self.pool = int(pstore.dim), pstore.pool
        ranges = [pstore.clip_ranges(k) for k in self.names]
        self.rows_of = np.array([len(r[0]) for r in ranges], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(self.rows_of)]).astype(np.int64)
        self.clip_start = torch.from_numpy(start).to(device)
        self.sources = []
        self.nbytes = self.clip_start.numel() * 8
        for si, (store, norm) in enumerate(zip(pstore.stores, pstore.norms)):
            seg = np.zeros((max(int(start[-1]), 1), 2), dtype=np.int64)
            for k, r, a in zip(self.names, ranges, start[:-1]):
                f0, n_rows = int(store.index[k][0]), int(store.index[k][1])
                if len(r[si]) and (r[si].min() < 0 or r[si].max() > n_rows):
                    raise ValueError("%s store: a range of %r lies outside the %d rows it has in source %d" % (what, k, n_rows, si))
                seg[a:a + len(r[si])] = r[si] + f0
            rows = _upload_rows(store, int(store.data.shape[0]), device, chunk_bytes)
            seg = torch.from_numpy(seg).to(device)
            self.sources.append((rows, seg, bool(norm)))
            self.nbytes += rows.numel() * rows.element_size() + seg.numel() * 8


def plan_examples(examples, desc_store, video_store, sub_store, dset_name, max_desc_len, max_ctx_len, clip_length, ctx_mode):
    """Host tables of a training set: per example the description / video names' presence is checked, the lengths after
    truncation and the (st, ed) labels are computed (get_st_ed_label on the context length the reference uses: the subtitle
    stream's when the mode has one, else the video's).  Raises ValueError on what the reference's dataset would fail on."""
    if ctx_mode not in CTX_MODES:
        raise ValueError("ctx_mode %r: the model has %s" % (ctx_mode, ", ".join(CTX_MODES)))
    use_video, use_sub, use_tef = "video" in ctx_mode, "sub" in ctx_mode, "tef" in ctx_mode
    if (use_video and video_store is None) or (use_sub and sub_store is None):
        raise ValueError("ctx_mode %r needs a %s store" % (ctx_mode, "video" if use_video and video_store is None else "sub"))
    n = len(examples)
    q_len, ctx_len, labels = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, 2), np.int64)
    for i, e in enumerate(examples):
        did, vid = str(e["desc_id"]), e["vid_name"]
        if did not in desc_store:
            raise ValueError("example %d: description %s is missing from the description store" % (i, did))
        if desc_store.n_rows(did) <= 0:
            raise ValueError("example %d: description %s has zero rows" % (i, did))
        q_len[i] = min(desc_store.n_rows(did), max_desc_len)
        lens = []
        for use, store, what in ((use_video, video_store, "video"), (use_sub, sub_store, "sub")):
            if not use:
                continue
            if vid not in store:
                raise ValueError("example %d: video %s is missing from the %s store" % (i, vid, what))
            if store.n_rows(vid) <= 0:
                raise ValueError("example %d: video %s has zero rows in the %s store" % (i, vid, what))
            lens.append(min(store.n_rows(vid), max_ctx_len))
        if use_tef and len(set(lens)) > 1:
            raise ValueError("example %d: video %s has %d video and %d subtitle clips after truncation; ctx_mode %r appends "
                             "one temporal endpoint feature to both" % (i, vid, lens[0], lens[1], ctx_mode))
        ctx_len[i] = lens[-1]
        ts = e["ts"] if dset_name != "didemo" else didemo_agreed_ts(e["ts"])
        labels[i] = st_ed_label(ts, clip_length, int(lens[-1]))
    return q_len, ctx_len, labels


class DeviceTrainStore(object):
    """See the module docstring.  feature_dtype: torch.float32 (the reference's contract) or torch.bfloat16."""

    def __init__(self, examples, desc_store, video_store=None, sub_store=None, dset_name="tvr", max_desc_len=30,
                 max_ctx_len=100, clip_length=1.5, ctx_mode="video_sub", normalize_vfeat=True, normalize_tfeat=True,
                 data_ratio=1.0, device="cuda:0", feature_dtype=torch.float32, ops=hip_ops):
        self.examples = _load_examples(examples, data_ratio)
        self.max_desc_len, self.max_ctx_len, self.ctx_mode = int(max_desc_len), int(max_ctx_len), ctx_mode
        self.q_len, self.ctx_len, labels = plan_examples(self.examples, desc_store, video_store, sub_store, dset_name,
                                                         self.max_desc_len, self.max_ctx_len, clip_length, ctx_mode)
        self.use_video, self.use_sub, self.use_tef = "video" in ctx_mode, "sub" in ctx_mode, "tef" in ctx_mode
        self.labels_host = labels
        self.device, self.ops, self.feature_dtype = torch.device(device), ops, feature_dtype
        self.norm = dict(query=bool(normalize_tfeat), video=bool(normalize_vfeat), sub=bool(normalize_tfeat))
        self.res, self.item_of = {}, {}
        for tag, use, store in (("query", True, desc_store), ("video", self.use_video, video_store),
                                ("sub", self.use_sub, sub_store)):
            if not use:
                continue
            pooled = tag != "query" and hasattr(store, "clip_ranges")        # an ingest.PooledStore: frame- / word-level rows
            r = self.res[tag] = (_PooledResident if pooled else _Resident)(store, tag, self.device)
            key = (lambda e: str(e["desc_id"])) if tag == "query" else (lambda e: e["vid_name"])
            self.item_of[tag] = torch.tensor([r.item[key(e)] for e in self.examples], dtype=torch.int32).to(self.device)
        self.labels = torch.from_numpy(labels).to(self.device)

    def __len__(self):
        return len(self.examples)

    def batch_max(self, ids):
        """(lmax, lq) of a batch as pad_sequences_1d gives them, from the host's lengths."""
        ids = np.asarray(ids, dtype=np.int64)
        return int(self.ctx_len[ids].max()), int(self.q_len[ids].max())

    def _host_ids(self, ids):
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
        if ids.ndim != 1 or ids.size == 0 or ids.dtype.kind not in "iu":
            raise IndexError("ids: expected a non-empty 1-d sequence of integers")
        bad = np.flatnonzero((ids < 0) | (ids >= len(self)))
        if len(bad):
            raise IndexError("example id %d out of range [0, %d)" % (int(ids[bad[0]]), len(self)))
        return ids.astype(np.int64)

    def _spec(self, n, lmax, lq):
        """key -> (shape, dtype) of the batch dict for n examples"""
        spec = collections.OrderedDict()
        for tag, length in (("query", lq), ("video", lmax), ("sub", lmax)):
            if tag in self.res:
                dd = self.res[tag].dim + (2 if self.use_tef and tag != "query" else 0)
                spec[tag + "_feat"] = ((n, length, dd), self.feature_dtype)
                spec[tag + "_mask"] = ((n, length), torch.float32)
        spec["st_ed_indices"] = ((n, 2), torch.int64)
        return spec

    def _gather(self, ids_dev, lmax, lq, out):
        n = int(ids_dev.numel())
        batch = dict(video_feat=None, video_mask=None, sub_feat=None, sub_mask=None)
        for tag, length, max_len in (("query", lq, self.max_desc_len), ("video", lmax, self.max_ctx_len),
                                     ("sub", lmax, self.max_ctx_len)):
            r = self.res.get(tag)
            if r is None:
                continue
            kw = dict(item_of=self.item_of[tag], normalize=self.norm[tag], eps=1e-5, tef=self.use_tef and tag != "query",
                      out_dtype=self.feature_dtype, out=None if out is None else out[tag + "_feat"],
                      mask_out=None if out is None else out[tag + "_mask"], want_len=False)
            if r.pooled:
                f, m, _ = self.ops.gather_pool_feature_rows(r.sources, r.clip_start, ids_dev, length, max_len, pool=r.pool, **kw)
            else:
                f, m, _ = self.ops.gather_feature_rows(r.rows, r.row_start, ids_dev, length, max_len, **kw)
            batch[tag + "_feat"], batch[tag + "_mask"] = f, m
        batch["st_ed_indices"] = self.ops.gather_index_rows(self.labels, ids_dev, out=None if out is None
                                                            else out["st_ed_indices"])
        return batch

    def batch(self, ids, lmax=None, lq=None, out=None):
        """-> the keyword dict xml_forward_train takes.  ids: a host sequence (validated: IndexError) or a device int32 tensor
        (lmax and lq must then be given; ids out of range give empty examples).  lmax / lq None: the batch maximum."""
        if out is not None:
            return self.fill(out, ids)
        if torch.is_tensor(ids) and ids.is_cuda:
            if lmax is None or lq is None:
                raise ValueError("ids on the device: lmax and lq must be given (nothing is read back)")
            if ids.dtype != torch.int32 or ids.dim() != 1:
                raise ValueError("ids on the device: expected a 1-d int32 tensor")
            ids_dev = ids.contiguous()
        else:
            host = self._host_ids(ids)
            bl, bq = self.batch_max(host)
            lmax, lq = bl if lmax is None else int(lmax), bq if lq is None else int(lq)
            ids_dev = torch.from_numpy(host.astype(np.int32)).to(self.device)
        return self._gather(ids_dev, int(lmax), int(lq), None)

    def fill(self, static, ids):
        """Writes the batch of `ids` into existing tensors (e.g. GraphedTrainStep.static): shapes and dtypes are checked
        against the request (ValueError).  The launches run on the current stream."""
        if torch.is_tensor(ids) and ids.is_cuda:
            if ids.dtype != torch.int32 or ids.dim() != 1:
                raise ValueError("ids on the device: expected a 1-d int32 tensor")
            ids_dev = ids.contiguous()
        else:
            ids_dev = torch.from_numpy(self._host_ids(ids).astype(np.int32)).to(self.device)
        n = int(ids_dev.numel())
        q = static.get("query_feat")
        c = static.get("video_feat") if self.use_video else static.get("sub_feat")
        if not torch.is_tensor(q) or not torch.is_tensor(c) or q.dim() != 3 or c.dim() != 3:
            raise ValueError("fill: the static batch has no (n, l, d) query / context features for ctx_mode %r" % self.ctx_mode)
        for key, (shape, dtype) in self._spec(n, int(c.shape[1]), int(q.shape[1])).items():
            t = static.get(key)
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError("fill: %s must be a contiguous %s tensor of shape %s, got %s" % (
                    key, dtype, shape, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
        for key in ("video_feat", "sub_feat"):
            if key[:-5] not in self.res and static.get(key) is not None:
                raise ValueError("fill: %s given, ctx_mode is %r" % (key, self.ctx_mode))
        return self._gather(ids_dev, int(c.shape[1]), int(q.shape[1]), static)


# ---------------------------------------------------------------------------------------------------------
# epoch driver
# ---------------------------------------------------------------------------------------------------------
def plan_epoch(n_examples, bsz, generator=None, order=None, rank=0, world=1, debug=False):
    """-> (the epoch's order (n_examples,) int64 numpy, this rank's batches: list of int64 arrays).  The order is
    torch.randperm on a CPU generator of its own (the global generator's sequence stays what draw_negative_ranks alone would
    see); rank r of `world` takes positions r::world of every batch; debug: four batches (xml/train.py:96-97)."""
    if order is None:
        if generator is None:
            generator = torch.Generator()
            generator.seed()
        order = torch.randperm(int(n_examples), generator=generator).numpy()
    order = np.asarray(order, dtype=np.int64)
    if not 0 <= rank < world:
        raise ValueError("rank %d of world %d" % (rank, world))
    batches = [order[b:b + bsz][rank::world] for b in range(0, len(order), int(bsz))]
    batches = [b for b in batches if len(b)]
    return order, batches[:4] if debug else batches


def train_epoch(model, optimizer, store, opt, epoch_i, training=True, step=None, generator=None, order=None, rank=0, world=1,
                history=None):
    """The reference's train_epoch (xml/train.py:42-119) on a DeviceTrainStore -> OrderedDict of the averaged loss terms.
    step: a GraphedTrainStep built on store.batch(ids0, lmax=max_ctx_len, lq=max_desc_len): full batches go through
    fill + replay, the partial last batch runs eagerly at the same fixed shapes, and the losses stay on the device until the
    end of the epoch (set_train_st_ed changes which tensors train: re-create the captured step when it switches on).
    history: a list that receives every step's loss dict."""
    from .train import train_step, xml_forward_train
    model.train(mode=training)
    if opt.hard_negtiave_start_epoch != -1 and epoch_i >= opt.hard_negtiave_start_epoch:
        model.set_hard_negative(True, opt.hard_pool_size)
    if opt.train_span_start_epoch != -1 and epoch_i >= opt.train_span_start_epoch:
        model.set_train_st_ed(opt.lw_st_ed)
    _, batches = plan_epoch(len(store), opt.bsz, generator, order, rank, world, bool(getattr(opt, "debug", False)))
    if not batches:
        return collections.OrderedDict((k, 0.0) for k in LOSS_KEYS)
    # the whole epoch's order goes to the device once; a step's ids are a slice of it
    flat = np.concatenate(batches)
    bad = np.flatnonzero((flat < 0) | (flat >= len(store)))
    if len(bad):
        raise IndexError("example id %d out of range [0, %d)" % (int(flat[bad[0]]), len(store)))
    ids_all = torch.from_numpy(flat.astype(np.int32)).to(store.device)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in batches])])
    graphed = step is not None and training
    if graphed:
        n_static = int(step.static["query_feat"].shape[0])
        lq_fix = int(step.static["query_feat"].shape[1])
        lmax_fix = int(step.static["video_feat" if store.use_video else "sub_feat"].shape[1])
        on_dev = torch.zeros((len(batches), len(LOSS_KEYS)), dtype=torch.float32, device=store.device)
    rows = []
    for bi, host_ids in enumerate(batches):
        ids = ids_all[int(offs[bi]):int(offs[bi + 1])]
        if graphed and len(host_ids) == n_static:
            store.fill(step.static, ids)
            _, parts = step(None)
            torch.stack([parts[k] for k in LOSS_KEYS], out=on_dev[bi])
            rows.append(None)
            continue
        lmax, lq = (lmax_fix, lq_fix) if graphed else store.batch_max(host_ids)
        batch = store.batch(ids, lmax=lmax, lq=lq)
        if training:
            _, parts = train_step(model, optimizer, batch, grad_clip=opt.grad_clip)
        else:
            with torch.no_grad():
                _, parts = xml_forward_train(model, **batch)
        rows.append([float(parts[k]) for k in LOSS_KEYS])
    if graphed:
        dev_rows = on_dev.tolist()           # the one host read of the captured steps' losses
        rows = [dev_rows[i] if r is None else r for i, r in enumerate(rows)]
    if history is not None:
        history.extend(dict(zip(LOSS_KEYS, r)) for r in rows)
    return collections.OrderedDict((k, float(np.mean([r[j] for r in rows]))) for j, k in enumerate(LOSS_KEYS))
