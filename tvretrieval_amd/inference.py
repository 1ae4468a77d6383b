"""Corpus-level retrieval drivers: host-side mirror of the hot loops of the reference's
baselines/crossmodal_moment_localization/inference.py ("xml/inference.py").

  compute_context_info     <- xml/inference.py:32-97     (HOT LOOP A: encode the corpus once)
  compute_query2ctx_info   <- xml/inference.py:252-445   (HOT LOOP B: per query batch, VCMR / SVMR / VR)
  vcmr_search              the device part of HOT LOOP B (:302-386) on resident tensors, used by bench.py

What changed by design (outputs are the same lists):
  * the corpus lives in HBM as a `CorpusIndex`: feat1 stored L2-normalised (the reference re-normalises it for
    every query batch, xml/model_xml.py:447), feat2 and masks padded to a multiple of 16 clips;
  * the (Nq, Nv, L) st/ed tensors are never built: ConvSE runs only on the top-k (and GT) videos per query;
  * the (Nq, k, L, L) product + full sort is replaced by a banded top-n kernel.
Everything on the device goes through tvretrieval_amd.ops (HIP); numpy only formats the result lists.

The `ops` argument of the functions here and in tvretrieval_amd.dist is the kernel backend.  tvretrieval_amd.ops is its
definition; a backend is any object with the names of OPS_CONTRACT, each taking the parameter names tvretrieval_amd.ops
gives it (tests/test_backend_contract.py holds the CPU stand-in of the gloo tests to that).  Nothing here asks a backend what
it can do: every keyword is passed, None / False being each callee's default, and a stand-in may raise NotImplementedError
for a non-default value it does not implement.  What OPS_CONTRACT lists is what index build, plain and f32 exact-rank search
and the sharded drivers call:
  l2norm_rows(x)                                          round_bf16_rows_err(y)
  q2c_pack_plan(masks)                                    q2c_tiled_ok(lpad, hidden, dtype)
  q2c_tiled_numel(rows, hidden, dtype)                    pack_q2c_corpus(feat1n, mask, plan, normalize=, out=)
  q2c_scores_fused(qn, cn, masks, normalize_q=)           q2c_rescore(qn, cn, masks, pair_vid)
  topk_rows(scores, k, alpha=, idx_in=, allow=)           select_ge_rows(scores, thr, cap, allow=)
  exact_certificate(filter_scores, top_val, eq, ec, slack, alpha, outside)
  convse_rerank(q_lin, feat2, masks, pair_vid, conv_w, l_ref, merged, ksize, softmax=, zero_skipped=, pair_w=, band=, vid_len=)
  moment_topk(st, ed, w, l_ref, min_l, max_l, n_out, summ=, pair_vid=, vid_len=)
  F16S                                                    the dtype sentinel of split-f16 models and rows
The split-f16 exact mode (split_f16_rows, SplitRows, F16_UNIT_LOG2), explain_moments (span_evidence), the device-side result
records (moments_decode, nms_moments), vcmr_search_host (ingest_rows) and searches on an index whose long videos take several
rows -- the drivers see index.fold and ask it alone: PartsFold for an index of parts (group_best_allow, best_part_rows),
ChainFold for chains of slots (chain_best_allow, chain_best_rows; exact-rank: cand_best_part, chain_spread_allow,
chain_members), both moments_decode(part_offset=) -- and the updates of an index_update.MutableCorpusIndex (index_put_rows,
index_clear_rows; with chains index_set_chains) and of an exact-rank one (index_put_rows_exact, exact_certificate_dev,
index_exact_bound; with the packed filter image index_put_rows_packed_exact) and the subset views of
video_subset (index_gather_blocks; HIP only, a search with subset= refuses any other backend) and a ContextFeeder over
ingest.PooledStore frame- / word-level stores (ingest_pool_rows; HIP only) or with a *_tef ctx_mode (ingest_rows /
ingest_pool_rows with tef=True; HIP only) call further entries of tvretrieval_amd.ops; a backend without them serves every search that does not ask for those.
"""
import types

import numpy as np
import torch

from . import ops as hip_ops

OPS_CONTRACT = ("l2norm_rows", "round_bf16_rows_err", "q2c_pack_plan", "q2c_tiled_ok", "q2c_tiled_numel", "pack_q2c_corpus",
                "q2c_scores_fused", "q2c_rescore", "topk_rows", "select_ge_rows", "exact_certificate", "convse_rerank",
                "moment_topk", "F16S")


def _round_up(x, m):
    return (x + m - 1) // m * m


class CorpusIndex(object):
    """Encoded corpus resident in HBM.

    modalities : list of "video" / "sub" in model order
    feat1n[m]  : (Nv, lpad, H) compute dtype, L2-normalised rows (zero rows beyond each batch's own length); on the
                 HIP backend at lpad == 128 an ops.TiledRows (K6's slice-major tile layout) -- feat1n_rows(m) gives
                 the row-major tensor back
    feat2[m]   : (Nv, lpad, H) compute dtype
    mask[m]    : (Nv, lpad) float32
    l_ref      : the reference's context length = global max clip count (xml/inference.py:71-87)
    video_offset : global index of local video 0 (corpus shards, tvretrieval_amd.dist)
    """

    def __init__(self, modalities, feat1n, feat2, mask, l_ref, video_offset=0, n_total=None):
        self.modalities = list(modalities)
        self.feat1n, self.feat2, self.mask = feat1n, feat2, mask
        self.l_ref = int(l_ref)
        self.lpad = int(feat2[self.modalities[0]].shape[1])
        self.n_videos = int(feat2[self.modalities[0]].shape[0])
        self.video_offset = int(video_offset)
        self.n_total = int(n_total if n_total is not None else self.n_videos)
        self.feat2_all = self.mask_all = None      # corpus-wide copies of feat2 / mask (dist.replicate_rerank_features)
        self.exact = None                          # ExactFilter: feat1n is the bf16 FILTER image of an f32 index (exact-rank mode)
        # ragged corpora: valid clips per video (1 + index of the last unmasked clip over the modalities) -- K7 neither
        # fetches the clip rows nor writes the (exactly zero) probabilities beyond it, K9 does not read them
        self.vlen = self.vlen_all = None
        self.ragged = False
        # long videos held as several rows: None (every row is a whole video), a PartsFold or a ChainFold.  The search drivers
        # ask the fold; the attributes of the two forms below serve ops.chain_*, the update path, subset views and tools.
        self.fold = None
        # long videos indexed in parts (build_corpus_index(parts=)): the device ingest.PartTable; rows
        # of the index are then PARTS (n_videos keeps meaning index rows) and n_source_videos the videos they fold back into.
        # index.parts is the table the PartsFold holds -- one fact, kept once (the property below)
        self.n_source_videos = self.n_videos
        # an index that takes updates (index_update.MutableCorpusIndex): rows are SLOTS, live the
        # (1, ceil(n_videos / 32)) int32 words of the occupied ones -- every search sees live AND video_allow -- and slot_ids
        # the slot -> caller's id table (the meta2vid of a search that passes none).  None on every other index.
        self.live = self.slot_ids = None
        # long videos on such an index (MutableCorpusIndex.create(..., part_overlap=O)): a video is a
        # CHAIN of slots, one part each; (n_videos,) int32 device tables slot -> head slot / next slot (-1) / first clip of the
        # slot's part in its video.  A video's number -- in top_videos, in a caller's video_allow -- is its HEAD slot.
        self.chain_head = self.chain_next = self.chain_offset = None
        self.part_overlap = self.max_parts = None

    @property
    def parts(self):
        """The device PartTable of a parts index, None on every other index."""
        return self.fold._parts if isinstance(self.fold, PartsFold) else None

    @parts.setter
    def parts(self, table):
        """Only cleared: index.parts = None on a (copy of a) parts index leaves an index of plain rows, each a video."""
        if table is not None:
            raise AttributeError("index.parts is made by build_corpus_index(parts=); it can only be set to None")
        if self.parts is not None:
            self.fold = None

    def set_valid_lengths(self):
        """Per-video valid length from the masks (one small device pass + one host read at build time)."""
        pos = None
        for m in self.modalities:
            mk = self.mask[m]
            if not isinstance(mk, torch.Tensor):
                return self
            last = ((mk != 0).to(torch.int32) * torch.arange(1, mk.shape[1] + 1, device=mk.device, dtype=torch.int32)).amax(1)
            pos = last if pos is None else torch.maximum(pos, last)
        # The maximum over modalities is exact, also when one modality of a video has no valid clip: the reference averages
        # the masked LOGITS of the two streams, (video + sub) / 2 with -1e10 at masked positions, and takes the softmax
        # afterwards (xml/model_xml.py:436-453, xml/inference.py:365-370) -- a position masked in one stream sits at -5e9, in
        # both at -1e10, and exp() of either against a valid position is exactly 0
        # (tests/test_gpu_model.py::test_video_with_one_empty_modality_matches_the_reference_lists).
        pos = torch.where(pos == 0, torch.full_like(pos, self.l_ref), pos)     # no valid clip at all: the masked softmax is
        self.vlen = pos.clamp_max(self.l_ref).to(torch.int32).contiguous()     # uniform, not zero -> nothing is skipped
        self.ragged = bool((self.vlen < self.l_ref).any().item())
        return self

    def feat1n_rows(self, m):
        t = self.feat1n[m]
        return t.to_rows() if hasattr(t, "to_rows") else t

    @property
    def device(self):
        return self.feat2[self.modalities[0]].device

    def hbm_bytes(self):
        tot = 0
        for d in (self.feat1n, self.feat2, self.mask, self.feat2_all or {}, self.mask_all or {},
                  self.exact.feat1n_f32 if self.exact is not None else {}):
            for t in d.values():
                tot += t.numel() * t.element_size()
                if hasattr(t, "inv"):
                    tot += t.inv.numel() * 4
        if self.exact is not None:
            tot += self.exact.hbm_bytes_extra()
        return tot


class ExactFilter(object):
    """Exact-rank mode of a CorpusIndex (include/xmlhip.h "Exact-rank mode"): the model runs in f32, `index.feat1n` holds the
    similarity operand ROUNDED ONCE to bf16 (K6 is a filter), and this object holds what turns the filter's candidates into
    the f32 path's lists:
      feat1n_f32[m]  (Nv, lpad, H) f32 row-major, L2-normalised -- re-scoring operand, and the f32 K6 operand of the fallback
      e_c[m]         largest bf16 rounding-error norm || c - c_b ||_2 over the corpus rows of modality m
      n_candidates   M: candidates per query proposed by the bf16 pass (K8 emits at most 256)"""

    def __init__(self, feat1n_f32, e_c, n_candidates=256, mode="f32"):
        self.feat1n_f32, self.e_c, self.n_candidates, self.mode = feat1n_f32, e_c, int(n_candidates), mode
        # mode "f32"  : bf16 filter image, f32 rows re-scored with the exact-f32 MFMA (round 3)
        # mode "f16s" : f16 filter image (the hi planes), feat1n_f32 holds ops.SplitRows (hi + lo halves at the fixed unit
        #               scale) re-scored as split-f16 products, index.feat2 are SplitRows too: every f32-grade stage on the
        #               16-bit MFMA pipe (include/xmlhip.h "Exact-rank mode on the 16-bit pipe")
        self.tier2_rows = None        # capacity of the on-device second tier (None: sized from the batch); tests shrink it
        self.tier2_cap = 1024         # candidates per second-tier query
        # an index that takes updates (index_update.MutableCorpusIndex.create(..., exact_rank=True)):
        #   e_c_dev      (n_mod,) f32 device, the RUNNING bound: every put raises it (atomic max), the certificate reads it
        #                through a pointer -- no update reads anything back, a captured search sees the bound of its replay;
        #                e_c is then a read-back of these cells, for diagnostics only
        #   err_rows[m]  (capacity, lpad) f32: the rounding-error norm of every stored row (tighten_error_bound)
        # None on a one-shot index, whose e_c stays the host dict.
        self.e_c_dev = self.err_rows = None

    def hbm_bytes_extra(self):
        """Bytes of the tensors only an updatable exact-rank index holds."""
        if self.e_c_dev is None:
            return 0
        return self.e_c_dev.numel() * 4 + sum(t.numel() * 4 for t in self.err_rows.values())


class _DeviceBound(object):
    """ExactFilter.e_c of an updatable index: a mapping modality -> the float read back from e_c_dev (one small device ->
    host copy per access; the search never uses it)."""

    def __init__(self, cells, modalities):
        self._cells, self._mods = cells, list(modalities)

    def __getitem__(self, m):
        return float(self._cells[self._mods.index(m)].item())

    def keys(self):
        return list(self._mods)

    __iter__ = lambda self: iter(self._mods)
    __len__ = lambda self: len(self._mods)

    def items(self):
        vals = self._cells.cpu().tolist()
        return list(zip(self._mods, vals))


def _exact_certificate(ex, mods, ops, cand_s, top_w, eq, hidden, alpha, outside, split):
    """The certificate of an exact-rank search.  split (the split-f16 chain): three product sums per re-scored value, one per
    filter value -- the f32 accumulation bound of each + the second-order terms of the two error norms (e_q e_c) the
    first-order formula of xml_exact_certificate leaves out; else the f32 chain's exact_slack.  A one-shot index hands its
    host e_c by value (xml_exact_certificate); an updatable one its device cells, and the slack's e_c term is evaluated in
    the kernel (xml_exact_certificate_dev)."""
    if ex.e_c_dev is not None:
        base = 2.0 * exact_slack(hidden) + 2.0 ** -20 if split else exact_slack(hidden)
        return ops.exact_certificate_dev(cand_s, top_w, eq, ex.e_c_dev, base, 4.0 if split else 0.0, alpha, outside)
    ec = [ex.e_c[m] for m in mods]
    slack = 2.0 * exact_slack(hidden) + 4.0 * max(ec) ** 2 + 2.0 ** -20 if split else exact_slack(hidden)
    return ops.exact_certificate(cand_s, top_w, eq, ec, slack, alpha, outside)


# Filter operand of the split-f16 exact mode.  The K6 kernel is power-limited and every mantissa bit of its operands costs
# ~0.85 ms of a 65 ms launch (tools/bench_k6_dtype.py: bf16 64.8, f16 69.3 ms on one box); an f16 filter needs 128
# candidates per query, a bf16 filter 256 -- and the 128-row re-score chunks make the second 128 candidates cheap.
EXACT_F16S_FILTER = "bf16"          # "bf16" (256 candidates) or "f16" (128 candidates)


def _exact_filter_operands(f1_raw, mask, plan, ops, mode="f32", filter_dtype=None):
    """raw f32 feat1 (Nv, lpad, H) -> (filter image for K6, re-score operand, largest rounding-error norm).
    mode "f32": bf16 tiles + f32 normalised rows; mode "f16s": bf16 or f16 tiles + SplitRows."""
    if f1_raw.dtype != torch.float32:
        raise ValueError("exact-rank mode needs f32 activations (XML(cfg, compute_dtype=torch.float32 or ops.F16S)); got %s"
                         % f1_raw.dtype)
    fn = ops.l2norm_rows(f1_raw)
    if mode == "f16s" and (filter_dtype or EXACT_F16S_FILTER) == "f16":
        sr, hi, err = ops.split_f16_rows(fn, ops.F16_UNIT_LOG2, want_hi=True, want_err=True)
        e_c = float(err.max()) if err.numel() else 0.0
        return ops.pack_q2c_corpus(hi, mask, plan, normalize=False), sr, e_c
    if mode == "f16s":
        sr = ops.split_f16_rows(fn, ops.F16_UNIT_LOG2)
        fb, err = ops.round_bf16_rows_err(fn)
        e_c = float(err.max()) if err.numel() else 0.0
        return ops.pack_q2c_corpus(fb, mask, plan, normalize=False), sr, e_c
    fb, err = ops.round_bf16_rows_err(fn)
    e_c = float(err.max()) if err.numel() else 0.0
    return ops.pack_q2c_corpus(fb, mask, plan, normalize=False), fn, e_c


def exact_mode_of(model, ops=hip_ops):
    """which exact-rank pipeline an index built from this model gets"""
    return "f16s" if getattr(model, "compute_dtype", None) is ops.F16S else "f32"


def index_lpad(l_ref, model, ops=hip_ops):
    """Padded clip count of the index tensors: l_ref rounded up to 16 -- or 128 when that lets K6 take its persistent tiled
    kernel (which is built for 128-column video groups): the reference's as-trained shape, max_ctx_l = 100
    (xml/config.py:86-88), pads 100 -> 128 (the length-bucketed layout then packs the videos of <= 64 / <= 32 clips 4 / 8 to
    a tile, so the padding rows of SHORT videos cost no MFMA work) instead of 112 on the slow per-modality kernels."""
    lp = _round_up(int(l_ref), 16)
    dt = getattr(model, "compute_dtype", torch.float32)
    if dt is ops.F16S:
        dt = torch.float16            # (its K6 operand is the f16 hi plane)
    if 64 < lp < 128 and model is not None and ops.q2c_tiled_ok(128, model.config.hidden_size, dt):
        return 128
    return lp


def pad_batch(seqs, device=None, dtype=torch.float32):
    """pad_sequences_1d (utils/tensor_utils.py:5-53) for a list of (L_i, D) arrays -> (N, Lmax, D), (N, Lmax).
    One concatenate + one masked assignment instead of a Python loop of per-sequence tensor copies (50 ms -> 2 ms for a
    batch of 50 queries: the loop, not the device, was what eval_epoch waited for)."""
    n = len(seqs)
    arrs = [s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s) for s in seqs]
    lens = np.fromiter((len(a) for a in arrs), dtype=np.int64, count=n)
    lmax = int(lens.max())
    valid = np.arange(lmax)[None, :] < lens[:, None]
    np_dtype = torch.empty(0, dtype=dtype).numpy().dtype
    out = np.zeros((n, lmax) + tuple(arrs[0].shape[1:]), dtype=np_dtype)
    out[valid] = np.concatenate(arrs, axis=0)
    out, mask = torch.from_numpy(out), torch.from_numpy(valid.astype(np.float32))
    if device is not None:
        out, mask = out.to(device, non_blocking=True), mask.to(device, non_blocking=True)
    return out, mask


class IndexStorage(object):
    """Device memory of a corpus index, allocated (and zero-filled: touched) BEFORE the encode -- a resident engine maps its
    index once; hipMalloc + first touch of tens of GB inside the encode loop is what a fresh process pays, not the encoder
    (bench.py times the two separately).  f1 / f2 / mk: per-modality (n_videos, lpad, H) compute dtype x2 and (n_videos,
    lpad) f32; tiles: per-modality flat buffer of the K6 tile image (full-length corpora: the size is known up front)."""

    def __init__(self, model, n_videos, l_ref, ops=hip_ops, device=None, tiles=True):
        # tiles=False: an exact-rank index builds its filter image itself (from the normalised f32 rows)
        mods = [n for n, u in (("video", model.use_video), ("sub", model.use_sub)) if u]
        dev = device if device is not None else next(model.parameters()).device
        dt, h = getattr(model, "act_dtype", model.compute_dtype), model.config.hidden_size
        self.n_videos, self.l_ref, self.lpad = int(n_videos), int(l_ref), index_lpad(l_ref, model, ops)
        self.f1 = {m: torch.zeros((self.n_videos, self.lpad, h), dtype=dt, device=dev) for m in mods}
        self.f2 = {m: torch.zeros((self.n_videos, self.lpad, h), dtype=dt, device=dev) for m in mods}
        self.mk = {m: torch.zeros((self.n_videos, self.lpad), dtype=torch.float32, device=dev) for m in mods}
        self.tiles = {}
        if tiles and self.lpad == 128 and dt in (torch.float32, torch.bfloat16):
            n = ops.q2c_tiled_numel(self.n_videos * self.lpad, h, dt)
            if n:
                self.tiles = {m: torch.zeros(n, dtype=dt, device=dev) for m in mods}

    def nbytes(self):
        return sum(t.numel() * t.element_size() for d in (self.f1, self.f2, self.mk, self.tiles) for t in d.values())


def build_corpus_index(model, context_batches, ops=hip_ops, keep_raw=False, video_offset=0, n_total=None,
                        l_ref=None, n_videos=None, exact_filter=False, storage=None, length_buckets=True, parts=None):
    """Encode context batches and assemble the resident index.

    context_batches: iterable of (video_feat, video_mask, sub_feat, sub_mask) device tensors (unused modality:
    None).  Each batch is encoded at its own padded length and zero-filled beyond it in the index, exactly
    like cat_tensor (xml/inference.py:71-87), so rows >= a batch's max length are 0 and rows between a video's
    length and its batch max hold the encoder's outputs at padded positions (both observable through the 5-tap
    ConvSE).
    l_ref + n_videos (a resident engine knows its corpus) or storage=IndexStorage: the index tensors exist before the loop
    (allocated from the first batch's dtype and width, or handed in) and every encoded batch is written into its rows -- no
    growing list of per-batch outputs, no concatenation pass, the per-batch activations are recycled by the allocator; a
    batch of full padded length is encoded STRAIGHT into its rows (the last layer of each branch writes there).  Otherwise
    the encoded batches are collected, n_videos / l_ref (the batch maximum) follow from them, and the same rows are filled.
    exact_filter=True (f32 model): exact-rank mode -- feat1n becomes the bf16 filter image, index.exact the f32 operands
    (ExactFilter); vcmr_search then returns the f32 path's lists at close to the bf16 path's speed.
    length_buckets=False: a ragged corpus keeps the plain two-videos-per-tile K6 image (A/B against the bucketed one).
    parts (ingest.PartTable, host or device): the batches hold the PARTS of videos longer than max_ctx_l, in the table's row
    order (ingest.ContextFeeder(parts=)); every part is encoded and stored as a stand-alone video.  The index gets
    index.parts (the table on the device) and index.n_source_videos; index.n_videos stays the number of index rows.  Searches
    then rank a video by its best part and report moments in whole-video time (vcmr_search)."""
    if parts is not None:
        if exact_filter:
            raise ValueError("build_corpus_index: parts= and exact_filter=True exclude each other -- exact-rank mode never "
                             "forms the f32 (Nq, rows) score matrix that the best part of a video is taken from")
        if video_offset or (n_total is not None and int(n_total) != parts.n_parts):
            raise ValueError("build_corpus_index: a parts index is not a corpus shard (video_offset / n_total)")
        if n_videos is not None and int(n_videos) != parts.n_parts:
            raise ValueError("build_corpus_index: n_videos = %d, but the part table has %d index rows (n_videos counts rows)"
                             % (n_videos, parts.n_parts))
    mods = [n for n, u in (("video", model.use_video), ("sub", model.use_sub)) if u]
    dst = None                    # (feat1, feat2, mask): per-modality (n_videos, lpad, H) x2 and (n_videos, lpad) f32
    if storage is not None:       # (zero-filled by IndexStorage; used for ONE build)
        assert l_ref is None or int(l_ref) == storage.l_ref
        assert n_videos is None or int(n_videos) == storage.n_videos
        l_ref, n_videos = storage.l_ref, storage.n_videos
        dst = dict(storage.f1), dict(storage.f2), dict(storage.mk)
    known = n_videos is not None and l_ref is not None
    lpad = index_lpad(l_ref, model, ops) if known else None
    collected, r = [], 0
    for video_feat, video_mask, sub_feat, sub_mask in context_batches:
        feats = dict(video=video_feat, sub=sub_feat)
        outs = [None, None, None, None]
        direct = dst is not None and all(feats[m] is not None and feats[m].shape[1] == lpad
                                         and r + feats[m].shape[0] <= n_videos for m in mods)
        if direct:
            for i, m in enumerate(("video", "sub")):
                if m in mods:
                    b = feats[m].shape[0]
                    outs[2 * i], outs[2 * i + 1] = dst[0][m][r:r + b], dst[1][m][r:r + b]
        v1, v2, s1, s2 = model.encode_context(video_feat, video_mask, sub_feat, sub_mask, outs=tuple(outs))
        enc = {m: e for m, e in (("video", (v1, v2, video_mask)), ("sub", (s1, s2, sub_mask))) if m in mods}
        if not known:
            collected.append(enc)
            continue
        if dst is None:
            dst = _alloc_index_rows(enc, n_videos, lpad)
        r = _fill_index_rows(dst, r, enc, l_ref, copy=not direct)
    if not known:
        batch_max = max(enc[mods[0]][1].shape[1] for enc in collected)
        l_ref = batch_max if l_ref is None else int(l_ref)
        assert l_ref >= batch_max
        n_videos = sum(enc[mods[0]][1].shape[0] for enc in collected)
        dst = _alloc_index_rows(collected[0], n_videos, index_lpad(l_ref, model, ops))
        for enc in collected:
            r = _fill_index_rows(dst, r, enc, l_ref)
        del collected          # (the per-batch outputs are not held through the packing passes)
    assert r == n_videos, "n_videos=%d but the batches held %d" % (n_videos, r)
    if parts is not None and r != parts.n_parts:
        raise ValueError("build_corpus_index: the batches held %d rows, the part table has %d parts" % (r, parts.n_parts))
    index = _finish_index(model, ops, mods, dst, int(l_ref), video_offset, n_total, keep_raw, exact_filter, length_buckets,
                          storage.tiles if storage is not None else {})
    if parts is not None:
        if index.l_ref > parts.max_ctx_len:
            raise ValueError("build_corpus_index: rows of %d clips, but the part table was planned for max_ctx_len = %d"
                             % (index.l_ref, parts.max_ctx_len))
        index.fold = PartsFold(parts.to(index.device))          # (index.parts reads the table from it)
        index.n_source_videos = parts.n_videos
    return index


def _alloc_index_rows(enc, n_videos, lpad):
    """Zero-filled index tensors for n_videos videos, dtype / width / device of the encoded batch enc."""
    f1 = {m: a1.new_zeros((n_videos, lpad, a1.shape[2])) for m, (a1, _, _) in enc.items()}
    f2 = {m: a2.new_zeros((n_videos, lpad, a2.shape[2])) for m, (_, a2, _) in enc.items()}
    mk = {m: torch.zeros((n_videos, lpad), dtype=torch.float32, device=a1.device) for m, (a1, _, _) in enc.items()}
    return f1, f2, mk


def _fill_index_rows(dst, r, enc, l_ref, copy=True):
    """One encoded batch, enc[m] = (feat1, feat2, mask), into rows r : r + b, columns : lb of the index tensors; returns
    r + b.  copy=False: the encoder already wrote feat1 / feat2 there."""
    f1, f2, mk = dst
    for m, (a1, a2, am) in enc.items():
        b, lb = a1.shape[0], a1.shape[1]
        assert r + b <= mk[m].shape[0] and lb <= l_ref
        if copy:
            f1[m][r:r + b, :lb] = a1
            f2[m][r:r + b, :lb] = a2
        mk[m][r:r + b, :lb] = am.float()
    return r + b


def _finish_index(model, ops, mods, dst, l_ref, video_offset, n_total, keep_raw, exact_filter, length_buckets, tile_bufs):
    """Filled index tensors -> CorpusIndex: K6's resident operand (and the exact-rank ones), valid lengths."""
    f1, f2, mk = dst
    # ragged corpora: one length-bucketed layout shared by the modalities (2 / 4 / 8 videos per K6 tile)
    plan = ops.q2c_pack_plan([mk[m] for m in mods]) if (length_buckets and mk[mods[0]].shape[1] == 128) else None
    mode = exact_mode_of(model, ops)
    feat1n, ex_f32, ex_ec = {}, {}, {}
    for m in mods:
        if exact_filter:
            feat1n[m], ex_f32[m], ex_ec[m] = _exact_filter_operands(f1[m], mk[m], plan, ops, mode)
            if mode == "f16s":
                f2[m] = ops.split_f16_rows(f2[m])
        else:       # normalised, in slice-major tiles where the persistent K6 kernel takes them (a storage's buffer: no plan)
            feat1n[m] = ops.pack_q2c_corpus(f1[m], mk[m], plan, normalize=True,
                                            out=tile_bufs.get(m) if plan is None else None)
    idx = CorpusIndex(mods, feat1n, f2, mk, l_ref, video_offset, n_total).set_valid_lengths()
    idx.raw_feat1 = dict(f1) if keep_raw else {}
    if exact_filter:        # f16 filter: rounding errors 8x smaller than bf16's -> the certificate holds with half the candidates
        idx.exact = ExactFilter(ex_f32, ex_ec, n_candidates=128 if (mode == "f16s" and EXACT_F16S_FILTER == "f16") else 256,
                                mode=mode)
    return idx


def compute_context_info(model, eval_dataset, opt, ops=hip_ops):
    """Mirror of compute_context_info (xml/inference.py:32-97): same dict keys, plus "index" (CorpusIndex).
    `eval_dataset` follows the reference's dataset contract (set_data_mode("context"), items with "meta" and
    "model_inputs" {video_feat, sub_feat}); batches of opt.eval_context_bsz in dataset order."""
    eval_dataset.set_data_mode("context")
    device = opt.device
    metas = []

    def batches():
        n = len(eval_dataset)
        for b in range(0, n, opt.eval_context_bsz):
            items = [eval_dataset[i] for i in range(b, min(n, b + opt.eval_context_bsz))]
            metas.extend(e["meta"] for e in items)
            vf = vm = sf = sm = None
            if model.use_video:
                vf, vm = pad_batch([e["model_inputs"]["video_feat"] for e in items], device)
            if model.use_sub:
                sf, sm = pad_batch([e["model_inputs"]["sub_feat"] for e in items], device)
            yield vf, vm, sf, sm

    index = build_corpus_index(model, batches(), ops=ops, keep_raw=True)
    lr = index.l_ref
    g = lambda d, m: d[m][:, :lr] if m in d else None
    return dict(video_metas=metas,
                video_feat1=g(index.raw_feat1, "video"), video_feat2=g(index.feat2, "video"),
                video_mask=g(index.mask, "video"),
                sub_feat1=g(index.raw_feat1, "sub"), sub_feat2=g(index.feat2, "sub"), sub_mask=g(index.mask, "sub"),
                index=index)


# ---------------------------------------------------------------------------------------------------------
# device stages of HOT LOOP B
# ---------------------------------------------------------------------------------------------------------
def stage_query_vectors(model, query_feat, query_mask, n_valid_tokens=None):
    """encode_query -> per-modality modular query vectors, in index.modalities order.
    n_valid_tokens: see XML.encode_query (host-known token count: no read-back in the packed encoder)."""
    vq, sq = model.encode_query(query_feat, query_mask, n_valid_tokens=n_valid_tokens)
    out = {}
    if model.use_video:
        out["video"] = vq
    if model.use_sub:
        out["sub"] = sq
    return out


# Measured in round 4 (profiles/r04_notes.md) and NOT the default: handing K9 its selection threshold from K7 takes K9 from
# 0.65 to 0.45-0.53 ms at the TVR shape, but the extra epilogue work costs K7 as much or more (+0.2 ms with one maximum per
# group of 16 rows, +0.45 ms with the 8 largest rows of a pair), and at the as-trained shape the weaker bound makes K9 slower.
K7_SUMMARIES = False   # vcmr_search: K7 emits per-pair candidate summaries for K9 (False: K9 makes its own first pass); a tool may set it
K6_TIMER = None   # bench.py: callable returning (start, end) torch.cuda.Event pair recorded around each K6 launch


def _k6(index, qn, ops, normalize_q=False, subset=None):
    """One fused K6 launch over the local corpus (both modalities), bracketed by the bench's HIP events.
    subset (a subset.VideoSubset of this index): the launch runs xml_q2c_scores_packed over the VIEW's image, codes and mask
    bits; the matrix keeps its (Nq, Nv) shape and only the columns of the view's videos are written."""
    mods = index.modalities
    ev = K6_TIMER() if K6_TIMER is not None else None
    if ev:
        ev[0].record()
    q2c = ops.q2c_scores_fused(qn, [(index.feat1n if subset is None else subset.k6)[m] for m in mods],
                               [index.mask[m] for m in mods], normalize_q=normalize_q)
    if ev:
        ev[1].record()
    return q2c


def stage_q2c(index, qvec, ops=hip_ops, subset=None):
    """K6 over the local corpus: (Nq, Nv_local) f32 = mean over modalities of max-over-clips cosine (one launch).
    subset (video_subset): K6 over the view; the matrix is defined on the columns of the view's videos only."""
    if index.exact is not None:
        raise ValueError("this index is an exact-rank FILTER image (bf16 operands of an f32 model): use stage_exact_topk")
    return _k6(index, [qvec[m].contiguous() for m in index.modalities], ops, normalize_q=True, subset=subset)


def video_subset(index, allowed, tiles=None, n_clips=None):
    """A subset view of a resident index (subset.VideoSubset): the K6 blocks of the allowed videos,
    gathered on the device into a small packed image of their own, so that a search restricted to them --
    vcmr_search(..., subset=view), stage_video_topk, vcmr_search_host, GraphedVcmrSearch -- pays K6 for those videos only and
    returns bitwise what vcmr_search(..., video_allow=view.allow) returns.
    allowed: a (Nv,) bool array / tensor or an ascending list of video numbers (slots of an index that takes updates).
    tiles=None: exactly the tiles the placement needs; tiles=N: N tiles (room for view.reset(another set)).
    n_clips (an index that takes updates, tiles=None form): the members' valid lengths, which saves the one host read.
    Refused with a ValueError that names its reason: a parts index, chains of slots, a corpus shard, a parent whose K6 operand
    is not the tiled image (lpad != 128, a hidden size or dtype xml_q2c_tiled_ok refuses), float non-binary masks."""
    from .subset import VideoSubset
    return VideoSubset(index, allowed, tiles=tiles, n_clips=n_clips)


def _check_subset(subset, index, ops, external_top=None, pad_tail=False):
    """What a search through a subset view refuses, before any launch, each with its reason."""
    from . import subset as _subset
    if ops is not hip_ops:
        raise ValueError("subset=: a subset view is a HIP-only operand (xml_index_gather_blocks, xml_q2c_scores_packed); a "
                         "non-HIP ops backend cannot search it")
    if getattr(subset, "index", None) is not index:
        raise ValueError("subset=: this is a view of another index -- its codes name that index's videos and its blocks are "
                         "copies of that index's rows")
    if external_top is not None:
        raise ValueError("subset= and external_top exclude each other: a caller's video lists replace the ranking the view "
                         "restricts (filter the lists instead)")
    if pad_tail:
        raise ValueError("subset= and pad_tail=True exclude each other: the reference-shaped tail would have to invent rows in "
                         "the empty video slots of a restricted list")
    _subset.check_parent(index)
    subset.check_fresh()


def _subset_allow(subset, video_allow):
    """The allow rows of a search through a view: the view's row, ANDed with the caller's (1 or Nq rows)."""
    if video_allow is None:
        return subset.allow
    return video_allow[:, :subset.allow.shape[1]] & subset.allow


EXACT_TIER2_CAP = 4096        # second-tier candidates per failing query beyond which the f32 K6 row is computed instead


def exact_slack(hidden):
    """f32 accumulation bound of the two dot products a certificate compares: the filter's (exact bf16 products, f32
    accumulate) and the f32 path's own (fma chain): each |fl(sum) - sum| <= n u |x| |y|, u = 2^-24."""
    return 2.0 * (hidden + 1) * 2.0 ** -24


def pack_video_allow(allowed):
    """The allow-bit matrix of a restricted search (vcmr_search(video_allow=)) from booleans.
    allowed: (Nv,) or (R, Nv) bool array or tensor, host or device -> (R, ceil(Nv / 32)) int32 words on the same side (a numpy
    array for host input, numpy or CPU tensor alike; a device tensor for a device tensor): video v is allowed when bit v & 31
    of word v >> 5 is set; the padding bits of the last word are 0."""
    on_device = torch.is_tensor(allowed) and allowed.is_cuda
    a = allowed if on_device else (allowed.numpy() if torch.is_tensor(allowed) else np.asarray(allowed))
    if (a.dtype != torch.bool) if on_device else (a.dtype != np.bool_):
        raise ValueError("pack_video_allow: a bool array is expected, got dtype %s" % (a.dtype,))
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("pack_video_allow: (Nv,) or (R, Nv) with Nv >= 1 expected, got shape %s" % (tuple(allowed.shape),))
    r, nv = int(a.shape[0]), int(a.shape[1])
    nw = (nv + 31) // 32
    if not on_device:
        bits = np.zeros((r, nw * 32), dtype=np.uint8)
        bits[:, :nv] = a
        words = (bits.reshape(r, nw, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
        return np.ascontiguousarray(words).view(np.int32)
    bits = torch.zeros((r, nw * 32), dtype=torch.bool, device=a.device)
    bits[:, :nv] = a
    return hip_ops._pack_bits32(bits)


def _check_video_allow(video_allow, index, nq):
    """video_allow of a search over index for nq queries: int32 words on the index's device, 1 or nq rows.  On an index with a
    fold the bits number the fold's videos (a parts index: SOURCE videos)."""
    nv = index.fold.n_videos if index.fold is not None else index.n_videos
    nw = (nv + 31) // 32
    if not torch.is_tensor(video_allow) or video_allow.dtype != torch.int32 or video_allow.dim() != 2:
        raise ValueError("video_allow must be a 2-D int32 tensor of bit words (pack_video_allow)")
    if video_allow.shape[1] < nw or video_allow.shape[0] not in (1, nq):
        raise ValueError("video_allow must be (1 | %d, >= %d) words for %d videos and %d queries, got %s"
                         % (nq, nw, nv, nq, tuple(video_allow.shape)))
    return video_allow


class PartsFold(object):
    """index.fold of a parts index (build_corpus_index(parts=)): the rows of a long video are the CSR
    ranges of the device ingest.PartTable.  A fold is what the search drivers know about long videos held as several rows:
      overlap, n_videos (the bits a caller's video_allow must cover), part_offset (K10's operand: first clip of each row)
      best_allow(ops, scores, allow)  (rows, Nv) scores -> allow words over index rows: each allowed video's best part
      best_rows(ops, scores, video)   a video per row -> the index row of its best part
      video_of(top_i)                 listed index rows -> their videos (out["top_videos"])
      meta2vid(meta2vid)              a caller's video -> id table -> K10's index row -> id table"""

    def __init__(self, parts):
        self._parts, self._meta2vid = parts, None
        self.overlap, self.n_videos, self.part_offset = parts.overlap, parts.n_videos, parts.part_offset

    def best_allow(self, ops, scores, allow):
        return ops.group_best_allow(scores, self._parts, allow)

    def best_rows(self, ops, scores, video):
        return ops.best_part_rows(scores, self._parts, video)

    def video_of(self, top_i):
        return torch.where(top_i >= 0, self._parts.part_video[top_i.clamp_min(0).long()], top_i)

    def meta2vid(self, meta2vid):
        """PartTable.meta2vid, composed once per ids tensor and kept: the same tensor, unchanged since (same object, same
        version), is served from here."""
        if meta2vid is None or not torch.is_tensor(meta2vid):
            return self._parts.meta2vid(meta2vid)
        kept = self._meta2vid
        if kept is None or kept[0] is not meta2vid or kept[1] != meta2vid._version:
            kept = self._meta2vid = (meta2vid, meta2vid._version, self._parts.meta2vid(meta2vid))
        return kept[2]


class ChainFold(object):
    """index.fold of an index that takes updates and holds long videos as chains of slots (MutableCorpusIndex.create(...,
    part_overlap=O)): PartsFold's members over the index's chain tables, which updates rewrite in
    place -- a video's number is its HEAD slot, meta2vid is per slot already.  The last three members serve the exact-rank
    chain (section 20g), which folds re-scored candidate lists, not a score matrix; only this fold has them."""

    def __init__(self, index):
        self._index = index       # (the tables are allocated once: the operands may be bound here)
        self.overlap, self.n_videos, self.part_offset = index.part_overlap, index.n_videos, index.chain_offset

    def best_allow(self, ops, scores, allow):
        return ops.chain_best_allow(scores, self._index, allow)

    def best_rows(self, ops, scores, video):
        return ops.chain_best_rows(scores, self._index, video)

    def video_of(self, top_i):
        return torch.where(top_i >= 0, self._index.chain_head[top_i.clamp_min(0).long()], top_i)

    def meta2vid(self, meta2vid):
        return meta2vid

    def slot_allow(self, ops, allow):
        """The allow words of an exact-rank search: (per-slot words for the selections that propose candidate SLOTS, head-bit
        words for the fold of a full row).  allow is what stage_video_topk hands on: the live words themselves -- they carry
        every bit of a chain, nothing is launched -- or a caller's mask ANDed with them, whose bits number videos by their head
        slot: ops.chain_spread_allow gives every slot its head's bit."""
        live = self._index.live
        if allow is None or allow is live:
            return live, live
        return ops.chain_spread_allow(allow, self._index) & live, allow

    def fold_candidates(self, ops, scores, ids):
        """Candidate lists of SLOTS -> the same lists with every video reduced to its best candidate part (the others
        (-inf, -1))."""
        return ops.cand_best_part(scores, ids, self._index.chain_head, self._index.chain_offset)

    def members(self, ops, video):
        return ops.chain_members(self._index, video)


def _check_parts_search(index, max_pred_l, external_top=None, pad_tail=False):
    """What a search on an index with a fold cannot do, each with its reason."""
    fold = index.fold
    if external_top is not None:
        raise ValueError("external_top on a parts index: a caller's lists name index rows and would bypass the fold that lets "
                         "only the best part of a video compete (rank the source videos with the index instead)")
    if index.exact is not None and not hasattr(fold, "fold_candidates"):     # (no fold of re-scored candidate lists)
        raise ValueError("a parts index cannot be an exact-rank index (exact_filter=True): no f32 score matrix exists to "
                         "take the best part of a video from")
    if int(max_pred_l) > fold.overlap:
        raise ValueError("max_pred_l = %d exceeds the part overlap of %d clips: a moment of that length need not lie inside "
                         "one part (plan_parts(overlap=) must be >= max_pred_l)" % (max_pred_l, fold.overlap))
    if pad_tail:
        raise ValueError("pad_tail=True on a parts index: the reference-shaped tail would have to invent rows in the video "
                         "slots that stay empty once every video is counted once")


def _decode_operands(index, meta2vid):
    """K10's (meta2vid table, keywords) for this index: the slot -> id table of an index that takes updates unless the
    caller has one; with a fold, the fold's table and the first clip of every row, so that records carry the video's id and
    whole-video times."""
    if meta2vid is None and index.live is not None:
        meta2vid = index.slot_ids
    if index.fold is None:
        return meta2vid, {}
    return index.fold.meta2vid(meta2vid), dict(part_offset=index.fold.part_offset)


def _allow_rows(video_allow, rows):
    """The allow rows of a subset / permutation `rows` of the queries (a shared row serves every subset)."""
    if video_allow is None or video_allow.shape[0] == 1:
        return video_allow
    return video_allow.index_select(0, rows).contiguous()


def _exact_allow(index, k, video_allow, ops):
    """How every exact-rank search begins: the k check, then the allow words.  -> t with t.fold (index.fold: None or the
    ChainFold), t.allow (the words of every selection over corpus columns; per slot with chains) and t.head_allow (with chains:
    the head-bit words a full row is folded under)."""
    ex = index.exact
    if k > min(ex.n_candidates, index.n_videos):
        raise ValueError("exact-rank mode: top-%d videos asked of %d candidates per query (ExactFilter.n_candidates; K8 "
                         "proposes at most 256) -- lower max_vcmr_video or raise n_candidates" % (k, ex.n_candidates))
    t = types.SimpleNamespace(fold=index.fold, allow=video_allow, head_allow=video_allow)
    if t.fold is not None:
        t.allow, t.head_allow = t.fold.slot_allow(ops, video_allow)
    return t


def _exact_first_tier(t, index, q_filter, q_rescore, eq, k, alpha, ops, subset, split):
    """What the two exact-rank modes share behind their query preparation (per modality: the FILTER operand, the re-score
    operand, the rounding-error norms): K6 over the filter image, K8's M candidates, their re-score, the fold of an index with
    chains, K8 again for the top-k, the certificate, the info dict.  Returns (top_w (Nq, k) -- the raw re-scored values --,
    top_i, info) and leaves in t what the later tiers read: filt, rows_c, masks, fail, thr, n_fail, outside."""
    ex, mods = index.exact, index.modalities
    t.masks = [index.mask[m] for m in mods]
    t.filt = _k6(index, q_filter, ops, subset=subset)
    m_c = min(ex.n_candidates, index.n_videos)
    cand_s, cand_i = ops.topk_rows(t.filt, m_c, alpha=0.0, allow=t.allow)
    t.rows_c = [ex.feat1n_f32[m] for m in mods]                  # f32 rows / SplitRows (Nv, lpad, H)
    cand_r = ops.q2c_rescore(q_rescore, t.rows_c, t.masks, cand_i)
    fold_r, fold_i = t.fold.fold_candidates(ops, cand_r, cand_i) if t.fold is not None else (cand_r, cand_i)
    top_w, top_i = ops.topk_rows(fold_r, k, alpha=0.0, idx_in=fold_i)
    t.outside = index.n_videos > m_c
    t.fail, eps, t.thr, t.n_fail = _exact_certificate(ex, mods, ops, cand_s, top_w, eq, q_filter[0].shape[1], alpha,
                                                      t.outside, split)
    info = dict(fail=t.fail, eps=eps, q2c_filter=t.filt, cand_indices=cand_i, cand_filter=cand_s, cand_scores=cand_r,
                n_candidates=m_c, n_full_rows=0)
    if t.fold is not None:
        info.update(cand_folded_indices=fold_i, cand_folded_scores=fold_r, q_rescore=q_rescore)
    return top_w, top_i, info


def _exact_full_rows(t, scores, rows, k, alpha, ops):
    """The last tier of both modes: scores (len(rows), Nv), the f32-grade scores of EVERY video for the query rows `rows` ->
    their (top_w = exp(alpha s), top_i); on an index with chains the row is folded (the fold of index_parts.hip) under the
    head-bit words."""
    row_allow = _allow_rows(t.allow, rows)
    if t.fold is not None:
        row_allow = t.fold.best_allow(ops, scores, _allow_rows(t.head_allow, rows))
    return ops.topk_rows(scores, k, alpha=alpha, allow=row_allow)


def stage_exact_topk(index, qvec, k, alpha, ops=hip_ops, defer_check=False, video_allow=None, subset=None):
    """Exact-rank replacement of K6 + K8: dispatches on index.exact.mode (round-3 f32 re-score / split-f16 pipeline).
    subset (video_subset; video_allow must then carry the view's row): the FILTER pass runs over the view's image -- the
    filter matrix (info["q2c_filter"]) is defined on the view's columns only, which is all a selection under the allow row
    reads; the re-score operands and the tiers behind the filter are the parent's."""
    if index.exact.mode == "f16s":
        return stage_exact_topk_f16s(index, qvec, k, alpha, ops, defer_check, video_allow, subset)
    return stage_exact_topk_f32(index, qvec, k, alpha, ops, video_allow, subset)


def stage_exact_topk_f16s(index, qvec, k, alpha, ops=hip_ops, defer_check=False, video_allow=None, subset=None):
    """The exact-rank chain on the 16-bit MFMA pipe, with no host read-back on the common path (capturable):
      1. q normalised (f32) and split: hi plane (f16) -> K6 FILTER over the corpus's hi planes; rounding-error norms e_q;
      2. K8: the M best filter scores per query (M = 128: the f16 filter's error bound is 8x tighter than bf16's);
      3. xml_q2c_rescore on split-f16 rows (hi.hi + lo.hi + hi.lo): f32-grade scores of the candidates; K8 -> top-k;
      4. certificate  b_M + eps_q < T_k  per query (eps from the rounding-error norms, as in the f32 mode);
      5. ON-DEVICE second tier, fixed capacity: the failing queries are brought to the front by a stable sort of the fail
         flags, the first R slots get every video whose filter score reaches T_k - eps (<= C per query), re-scored and
         re-selected, and written back through a select on the fail flag -- slots of passing queries change nothing;
      6. only if more than R queries fail or a query has more than C such videos (scores closer together than any 16-bit
         filter resolves) the overflow flag is raised: eager callers (defer_check=False) read it -- one 4-byte read-back
         after everything is enqueued -- and re-score those queries against the whole corpus; graphed callers get the flag.
    video_allow (pack_video_allow's words, 1 or Nq rows): every selection over corpus columns -- the candidate K8, the second
    tier's select_ge_rows, the third tier's full row -- takes the mask; candidate slots a short row leaves empty are id -1,
    which the re-score turns into -inf.  The certificate is unchanged (conservative: a -inf at the candidates' end passes).
    An index with chains of slots (index.fold a ChainFold): the lists are of VIDEOS, each ranked by its
    best part, top_i the slots of those parts.  Candidates are proposed as slots under per-slot allow words (fold.slot_allow);
    every re-scored list is folded (fold.fold_candidates) before its top-k, so T_k is the k-th value over k DISTINCT videos and
    the certificate holds unchanged; the third tier's full row is folded by fold.best_allow under the head-bit words.
    info then also holds cand_folded_indices / cand_folded_scores and q_rescore (the query operands of ops.q2c_rescore).
    Returns (top_w = exp(alpha s) (Nq, k) f32, top_i (Nq, k) int32, info dict)."""
    t = _exact_allow(index, k, video_allow, ops)
    q_sr, q_hi, eq = [], [], []
    for m in index.modalities:
        q = qvec[m].contiguous()
        if q.dtype != torch.float32:
            raise ValueError("exact-rank mode needs f32 query vectors (an f32 / ops.F16S model)")
        qn = ops.l2norm_rows(q)
        if index.feat1n[m].dtype == torch.float16:              # f16 filter: the hi plane of the split
            sr, hi, e = ops.split_f16_rows(qn, ops.F16_UNIT_LOG2, want_hi=True, want_err=True)
        else:                                                   # bf16 filter
            sr = ops.split_f16_rows(qn, ops.F16_UNIT_LOG2)
            hi, e = ops.round_bf16_rows_err(qn)
        q_sr.append(sr), q_hi.append(hi), eq.append(e)
    top_w, top_i, info = _exact_first_tier(t, index, q_hi, q_sr, eq, k, alpha, ops, subset, True)
    ex, nq, fail, n_fail = index.exact, top_w.shape[0], t.fail, t.n_fail
    info.update(n_fail_dev=n_fail, overflow_dev=None)
    if t.outside:
        r_cap = min(nq, ex.tier2_rows if ex.tier2_rows is not None else max(32, nq // 64))
        c_cap = min(int(ex.tier2_cap), index.n_videos)
        if c_cap < k:
            raise ValueError("exact-rank mode: tier2_cap %d < k %d" % (c_cap, k))
        order = torch.argsort(fail, descending=True, stable=True)[:r_cap]          # failing queries first; a permutation
        is_fail = fail.index_select(0, order) != 0
        inf_ = torch.full((), float("inf"), device=fail.device)
        thr = torch.where(is_fail, t.thr.index_select(0, order), inf_).contiguous()        # passing slots select nothing
        cand2, cnt2 = ops.select_ge_rows(t.filt.index_select(0, order).contiguous(), thr, c_cap,
                                         allow=_allow_rows(t.allow, order))
        q_sub = [sr[order] for sr in q_sr]
        q_sub = [ops.SplitRows(sr.data.contiguous(), sr.inv.contiguous()) for sr in q_sub]
        full = ops.q2c_rescore(q_sub, t.rows_c, t.masks, cand2)
        if t.fold is not None:
            full, cand2 = t.fold.fold_candidates(ops, full, cand2)
        # slots of PASSING queries selected nothing: their rows are c_cap times -inf, and the top-k of an all-tied row with
        # payloads takes K8's one-block-minimum-per-element path (0.46 ms for 156 such rows -- more than the second tier's
        # re-score).  Their results are discarded below; a ramp of distinct values keeps them on the fast path.
        ramp = -torch.arange(c_cap, dtype=torch.float32, device=full.device)
        full = torch.where(is_fail[:, None], full, ramp[None, :])
        fw, fi = ops.topk_rows(full, k, alpha=alpha, idx_in=cand2)
        top_w.index_copy_(0, order, torch.where(is_fail[:, None], fw, top_w.index_select(0, order)))
        top_i.index_copy_(0, order, torch.where(is_fail[:, None], fi, top_i.index_select(0, order)))
        overflow = ((cnt2 > c_cap) & is_fail).any() | (n_fail[0] > r_cap)
        info["overflow_dev"] = overflow
        if not defer_check:
            nf = int(n_fail.item())
            info["n_fail"] = nf
            if bool(overflow.item()):        # third tier: the overflowing queries against the whole corpus
                bad = torch.nonzero(fail, as_tuple=False).reshape(-1)
                if nf <= r_cap:              # only the second-tier slots whose candidate list overflowed
                    bad = order[:nf][(cnt2[:nf] > c_cap)]
                every = torch.arange(index.n_videos, dtype=torch.int32, device=fail.device)
                for b0 in range(0, bad.numel(), 16):
                    rows = bad[b0:b0 + 16]
                    qs = [ops.SplitRows(sr.data.index_select(0, rows).contiguous(), sr.inv.index_select(0, rows).contiguous())
                          for sr in q_sr]
                    allv = ops.q2c_rescore(qs, t.rows_c, t.masks, every.repeat(rows.numel(), 1).contiguous())
                    fw, fi = _exact_full_rows(t, allv, rows, k, alpha, ops)
                    top_w.index_copy_(0, rows, fw)
                    top_i.index_copy_(0, rows, fi)
                info["n_full_rows"] = int(bad.numel())
    elif not defer_check:
        info["n_fail"] = 0
    return top_w, top_i, info


def stage_exact_topk_f32(index, qvec, k, alpha, ops=hip_ops, video_allow=None, subset=None):
    """Exact-rank replacement of K6 + K8 (index.exact is set, f32 query vectors): the f32 path's top-k videos per query.
      1. q_b = rne_bf16(normalize(q)) with its rounding-error norm e_q; bf16 K6 over the filter image (the timed K6);
      2. K8 proposes the M best filter scores per query (raw values + ids);
      3. xml_q2c_rescore: those (q, v) pairs against the f32 operands -> f32 scores of the candidates;
      4. K8 again on the (Nq, M) re-scored values with the ids as payload: top-k by (score desc, id asc);
      5. per-query certificate  b_M + eps_q < T_k ; the few queries that fail get a second tier -- every video whose filter
         score reaches T_k - eps_q (nothing below that line can enter the top-k) is re-scored too -- or, when the scores are
         too close together for that (> EXACT_TIER2_CAP such videos), a full f32 K6 row (the f32 path itself).
    video_allow: as in stage_exact_topk_f16s -- the candidate K8, both select_ge_rows calls and the fallback's full row.
    An index with chains of slots: as in stage_exact_topk_f16s -- every re-scored list is folded before its top-k, the
    fallback's full f32 row by fold.best_allow.
    Returns (top_w = exp(alpha s) (Nq, k) f32, top_i (Nq, k) int32, info dict)."""
    t = _exact_allow(index, k, video_allow, ops)
    qn = [ops.l2norm_rows(qvec[m].contiguous()) for m in index.modalities]
    if qn[0].dtype != torch.float32:
        raise ValueError("exact-rank mode needs f32 query vectors (an f32 model)")
    qb, eq = [], []
    for q in qn:
        b, e = ops.round_bf16_rows_err(q)
        qb.append(b), eq.append(e)
    top_w, top_i, info = _exact_first_tier(t, index, qb, qn, eq, k, alpha, ops, subset, False)
    nf = int(t.n_fail.item())        # (host sync: the launch shapes below depend on it)
    info["n_fail"] = nf
    if nf:
        rows = torch.nonzero(t.fail, as_tuple=False).reshape(-1)
        qsub = [q.index_select(0, rows).contiguous() for q in qn]
        # Second tier: T_k (the k-th re-scored value) is a LOWER bound of the final k-th score, so only videos whose filter
        # score reaches T_k - eps can still enter: usually a few dozen more than M.  Re-score exactly those.
        thr = t.thr.index_select(0, rows).contiguous()
        frows = t.filt.index_select(0, rows).contiguous()
        cap = int(ops.select_ge_rows(frows, thr, allow=_allow_rows(t.allow, rows)).max())
        if t.allow is not None:
            cap = max(cap, k)          # (rows with fewer than k allowed videos: the list is filled up with id -1 = -inf)
        if cap <= EXACT_TIER2_CAP:
            cand2, _ = ops.select_ge_rows(frows, thr, cap, allow=_allow_rows(t.allow, rows))
            full = ops.q2c_rescore(qsub, t.rows_c, t.masks, cand2)                    # (-inf where a row has fewer candidates)
            if t.fold is not None:
                full, cand2 = t.fold.fold_candidates(ops, full, cand2)
            fw, fi = ops.topk_rows(full, k, alpha=alpha, idx_in=cand2)
        else:   # scores so close together that the filter cannot separate them: the f32 K6 row itself
            info["n_full_rows"] = nf
            fw, fi = _exact_full_rows(t, ops.q2c_scores_fused(qsub, t.rows_c, t.masks), rows, k, alpha, ops)
        top_w.index_copy_(0, rows, fw)
        top_i.index_copy_(0, rows, fi)
    return top_w, top_i, info


def ragged_lengths(index, ops=hip_ops, replicated=False):
    """The valid-length array K7 / K9 take for a ragged corpus (None: every video has the full length -- full rows)."""
    if not index.ragged:
        return None
    return index.vlen_all if replicated else index.vlen


def query_linears(model, index, qvec):
    """{video,sub}_query_linear of the modular query vectors (xml/model_xml.py:459-460,507): K7's query operand."""
    return [getattr(model, m + "_query_linear")(qvec[m].contiguous()) for m in index.modalities]


SMALL_BATCH_FORK = 256      # query batches up to this size: the query linears run beside K6 + K8 on a second stream
_FORK_STREAMS = {}


def _fork_stream(device):
    key = str(torch.device(device))
    if key not in _FORK_STREAMS:
        _FORK_STREAMS[key] = torch.cuda.Stream(device=device)
    return _FORK_STREAMS[key]


def fork_query_linears(model, index, qvec, ops=hip_ops):
    """Small batches (the reference's eval_query_bsz = 50: ~20 short kernels in a chain, K6 on a handful of the 256 CUs):
    K7's query operand needs only the query vectors, so its two projections are issued on a second stream next to K6 + K8
    instead of between K8 and K7.  Returns (q_lin, event to wait for) or None; capturable (the fork and the join become
    graph edges)."""
    q0 = qvec[index.modalities[0]]
    if ops is not hip_ops or not q0.is_cuda or q0.shape[0] > SMALL_BATCH_FORK:
        return None
    main = torch.cuda.current_stream(q0.device)
    side = _fork_stream(q0.device)
    fork = torch.cuda.Event()
    fork.record(main)
    side.wait_event(fork)
    with torch.cuda.stream(side):
        q_lin = query_linears(model, index, qvec)
        done = torch.cuda.Event()
        done.record(side)
    for t in q_lin:
        t.record_stream(main)           # allocated on the side stream, consumed (and freed) on the main one
    for m in index.modalities:
        qvec[m].record_stream(side)
    return q_lin, done


def stage_span_probs(model, index, qvec, pair_vid, ops=hip_ops, zero_skipped=True, replicated=False, pair_w=None,
                     band=None, vid_len=None, q_lin=None):
    """K7 on the listed (query, local video) pairs -> softmaxed st / ed (Nq, K, lpad).
    replicated=True: pair_vid holds GLOBAL video ids into the corpus-wide copies index.feat2_all / index.mask_all
    (tvretrieval_amd.dist.replicate_rerank_features).
    vid_len (ragged_lengths(index)): the entries beyond a video's valid length are left unwritten -- hand the same array to
    ops.moment_topk(..., pair_vid=pair_vid, vid_len=vid_len)."""
    mods = index.modalities
    if q_lin is None:
        q_lin = query_linears(model, index, qvec)
    merged = bool(model.config.merge_two_stream and len(mods) == 2)
    feat2, mask = (index.feat2_all, index.mask_all) if replicated else (index.feat2, index.mask)
    if feat2[mods[0]].dtype is ops.F16S:
        q_lin = [ops.split_f16_rows(q.float().contiguous()) for q in q_lin]      # per-row scales: q' is not normalised
    # band = (min_l, max_l) [+ pair_w]: K7 also returns the per-pair candidate summaries K9 starts from (st, ed, summ)
    return ops.convse_rerank(q_lin, [feat2[m] for m in mods], [mask[m] for m in mods], pair_vid,
                             model._conv_weights(), index.l_ref, merged, model.config.conv_kernel_size, softmax=True,
                             zero_skipped=zero_skipped, pair_w=pair_w, band=band, vid_len=vid_len)


def pad_moment_tail(flat_scores, flat_indices, k_videos, l_ref, min_pred_l=None, max_pred_l=None):
    """Opt-in reference-shaped tail of a moment list.  The reference sorts the WHOLE (k, L, L) product tensor and always
    returns max_before_nms rows (xml/inference.py:381-386; SVMR: utils/tensor_utils.py:133-141): when fewer candidates
    have a positive score -- short videos, the length mask -- its tail is rows of score exactly 0 in an order torch.sort
    leaves unspecified.  The kernels mark those rows flat = -1; this fills them with the lowest flat positions of the
    (k, L, L) tensor that are NOT in the list (a list with empty rows holds every positive-score candidate, so every other
    position scores exactly 0 in the reference too) -- the order a stable descending sort would produce.
    Index plumbing on the device, in place; returns (flat_scores, flat_indices)."""
    n_out = flat_indices.shape[1]
    dev = flat_indices.device
    total = int(k_videos) * l_ref * l_ref
    cnt = (flat_indices >= 0).sum(1)
    rows = torch.nonzero(cnt < n_out, as_tuple=False).reshape(-1)
    if rows.numel() == 0:
        return flat_scores, flat_indices
    if total < n_out:          # (the reference itself fails when max_before_nms exceeds k * L * L)
        raise ValueError("pad_tail: max_before_nms = %d exceeds the %d positions of the (k, L, L) tensor" % (n_out, total))
    # among the first 2 n_out positions at least n_out are not in a list of < n_out entries
    cand = torch.arange(min(total, 2 * n_out), device=dev, dtype=flat_indices.dtype)
    pos = torch.arange(n_out, device=dev)
    for c in range(0, rows.numel(), 256):
        r = rows[c:c + 256]
        have = flat_indices[r]                                                        # (b, n_out), -1 = empty
        # membership by scatter, O(b (|cand| + n_out)) memory (a (b, |cand|, n_out) comparison is 512 MB per chunk at the
        # evaluation default max_before_nms = 1000): list entries inside [0, |cand|) mark their position as taken
        taken = torch.zeros((r.numel(), cand.numel() + 1), dtype=torch.bool, device=dev)
        slot = torch.where((have >= 0) & (have < cand.numel()), have, torch.full_like(have, cand.numel())).long()
        taken.scatter_(1, slot, True)
        free = ~taken[:, :cand.numel()]                                               # (b, |cand|): not in the list
        order = torch.argsort((~free).to(torch.int8), dim=1, stable=True)             # free positions first, ascending
        fill = cand[order[:, :n_out]]                                                 # (b, n_out)
        k = (pos[None, :] - cnt[r][:, None])                                          # index into fill for the empty rows
        empty = k >= 0
        flat_indices[r] = torch.where(empty, torch.gather(fill, 1, k.clamp_min(0)), have)
        flat_scores[r] = flat_scores[r].masked_fill(empty, 0.0)
    return flat_scores, flat_indices


def stage_video_topk(model, index, qvec, max_vcmr_video=100, q2c_alpha=20.0, ops=hip_ops, external_top=None,
                     defer_exact_check=False, video_allow=None, subset=None):
    """K6 + K8 (or the exact-rank chain, or a caller's video lists): (q2c or None, top_w (Nq, K) f32 = exp(alpha s) desc,
    top_i (Nq, K) int32, exact-rank info or None).  Per query independent of the rest of the batch.
    video_allow (pack_video_allow's words, 1 or Nq rows, on the device): every query's list is the list of the corpus that
    holds only its allowed videos (indices in this index's numbering); a query with a < K of them ends in K - a empty slots
    (top_i -1, top_w 0, or -inf when alpha == 0), which yield no moments.  K6 still scores every video.
    subset (video_subset(index, allowed)): the same lists as video_allow=subset.allow, bitwise, but K6 runs over the view's
    packed image -- its cost follows the allowed videos.  The allow row is the view's, ANDed with a caller's video_allow (1 or
    Nq rows) and with index.live; the returned q2c matrix (the exact-rank filter matrix alike) is defined on the columns of the
    view's videos only -- the others are never written.  subset=None is the path above, unchanged.
    A parts index: K6, then ops.group_best_allow (each video's best part AND the caller's mask over source videos), then K8 under
    those bits -- top_i are index rows, one per video; slots beyond the number of allowed videos are empty.
    An index that takes updates (index.live): the allow words are ANDed with the live words -- one small (rows, words) int32
    pass, part of a captured search -- so the lists are those of the corpus of the live videos, in slot numbering.
    One with chains (index.chain_head): K6, then ops.chain_best_allow under those words (each video's best part; a caller's
    video_allow bit for a video is the bit of its HEAD slot), then K8 under the fold's bits -- top_i are slots, one per video.
    One with chains in exact-rank mode (create(..., exact_rank=True, exact_part_overlap=O)): the exact-rank chain with the fold
    on its candidate lists (stage_exact_topk_f16s) -- the same lists of videos, f32-grade; q2c is None."""
    exact = None
    if subset is not None:
        _check_subset(subset, index, ops, external_top)
    if video_allow is not None:
        if external_top is not None:
            raise ValueError("video_allow and external_top exclude each other: a caller's video lists replace the ranking "
                             "the mask restricts (filter the lists instead)")
        _check_video_allow(video_allow, index, qvec[index.modalities[0]].shape[0])
    if subset is not None:
        video_allow = _subset_allow(subset, video_allow)
    if index.live is not None and external_top is None:
        video_allow = index.live if video_allow is None else video_allow[:, :index.live.shape[1]] & index.live
    if index.fold is not None:
        _check_parts_search(index, 0, external_top)
    k = min(max_vcmr_video, index.n_videos)
    if external_top is not None:    # external video-retrieval results replace K6/K8 (xml/inference.py:349-355):
        q2c = None                  # (meta idx int32, exp(alpha*s))
        top_i, top_w = external_top
    elif index.exact is not None:
        q2c = None          # (the f32 (Nq, Nv) matrix is never formed; exact["q2c_filter"] is the bf16 pass's)
        # defer_exact_check (split-f16 exact mode): no host read-back inside the pass; out["exact"]["overflow_dev"] (device
        # bool, None when every video is a candidate) says whether the on-device second tier's capacity was exceeded.
        # With a fold (chains) there is no f32 matrix to fold: the exact-rank chain folds its candidate lists itself
        top_w, top_i, exact = stage_exact_topk(index, qvec, k, q2c_alpha, ops, bool(defer_exact_check), video_allow, subset)
    else:
        q2c = stage_q2c(index, qvec, ops, subset)
        if index.fold is not None:
            # long videos in several rows: K6 scored every row, the fold keeps each video's best part (and the caller's mask,
            # which numbers videos as the fold does), K8 ranks those -- the restricted search over the rows, one per video
            video_allow = index.fold.best_allow(ops, q2c, video_allow)
        top_w, top_i = ops.topk_rows(q2c, k, alpha=q2c_alpha, allow=video_allow)
    return q2c, top_w, top_i, exact


def stage_moments(model, index, qvec, top_w, top_i, min_pred_l=2, max_pred_l=16, max_before_nms=200, ops=hip_ops,
                  pad_tail=False, q_lin=None):
    """K7 + K9 on the selected (query, video) pairs -> (flat_scores (Nq, n) f32 desc, flat_indices (Nq, n) int32).
    q_lin: the query linears' outputs when the caller already has them (fork_query_linears)."""
    if K7_SUMMARIES:
        # K7 hands K9 the 8 largest row maxima of every pair (taken while the rows were in its registers): K9 reads the
        # 1 GB of span probabilities once instead of twice
        st, ed, summ = stage_span_probs(model, index, qvec, top_i, ops, pair_w=top_w.contiguous(), band=(min_pred_l, max_pred_l))
        fs, fi = ops.moment_topk(st, ed, top_w, index.l_ref, min_pred_l, max_pred_l, max_before_nms, summ=summ)
    else:
        vl = ragged_lengths(index, ops)
        st, ed = stage_span_probs(model, index, qvec, top_i, ops, vid_len=vl, q_lin=q_lin)
        fs, fi = ops.moment_topk(st, ed, top_w, index.l_ref, min_pred_l, max_pred_l, max_before_nms, pair_vid=top_i,
                                 vid_len=vl)
    if pad_tail:
        pad_moment_tail(fs, fi, top_i.shape[1], index.l_ref, min_pred_l, max_pred_l)
    return fs, fi


def vcmr_search(model, index, query_feat, query_mask, max_vcmr_video=100, max_before_nms=200, q2c_alpha=20.0,
                min_pred_l=2, max_pred_l=16, svmr_video=None, ops=hip_ops, external_top=None, pad_tail=False,
                defer_exact_check=False, n_valid_tokens=None, video_allow=None, nms_thd=None, max_after_nms=100,
                meta2vid=None, clip_length=1.5, subset=None):
    """Device part of compute_query2ctx_info for one query batch (xml/inference.py:308-386), single GPU.

    Returns device tensors:
      top_scores (Nq,K) f32 = exp(alpha*q2c) desc, top_indices (Nq,K) int32 video (meta) indices,
      flat_scores (Nq,n) f32 desc, flat_indices (Nq,n) int32 into (K, l_ref, l_ref)  [-1 = no candidate]
      and, if svmr_video (Nq,) int32 is given, svmr_scores / svmr_flat (Nq,n) over (l_ref, l_ref).
    external_top = (indices (Nq,K) int32, weights (Nq,K) f32): use these videos / weights instead of K6 + K8.
    pad_tail=True: always max_before_nms rows, the reference's shape -- missing candidates become zero-score rows at
    length-masked positions (pad_moment_tail) instead of flat = -1.
    n_valid_tokens (host int): query_mask.sum() when the masks were built on the host (prefix masks) -- the packed query
    encoder of large batches then needs no read-back and the whole pass is enqueued without a host synchronisation.
    video_allow (pack_video_allow: (1 | Nq, ceil(Nv / 32)) int32 words on the device): the search restricted to each query's
    allowed videos -- exactly the unrestricted result on the corpus of those videos, in this index's numbering (see
    stage_video_topk for queries with fewer than K allowed videos).  Not with external_top or pad_tail=True.
    subset (video_subset(index, allowed)): the search restricted to the view's videos -- bitwise the result of
    video_allow=subset.allow (ANDed with video_allow when both are given), with K6 over the view's own packed image instead of
    the corpus.  out["q2c"] (out["exact"]["q2c_filter"] on an exact-rank index) is defined on the columns of the view's videos
    only; everything behind K6 runs on the index unchanged.  Refused with a ValueError before any launch: a view of another
    index, a stale view (the index was updated: view.refresh()), external_top, pad_tail=True, a non-HIP ops; see video_subset
    for the indexes that take no view.
    nms_thd (None: off): the search ends in the FINAL list on the device -- K10 (xml_moments_decode, meta2vid / clip_length as
    in vcmr_search_host) and temporal NMS (xml_nms_moments) follow on the same stream.  out additionally holds records /
    record_count (K10 of flat_scores / flat_indices: (Nq, n, 4) int32 xml_moment rows in seconds, (Nq,) int32) and nms_records
    (Nq, max_after_nms, 4) / nms_index (Nq, max_after_nms) positions in `records` / nms_count (Nq,) = filter_vcmr_by_nms of
    them; with svmr_video also svmr_records / svmr_record_count (clip units) and svmr_nms_records / svmr_nms_index /
    svmr_nms_count = post_processing_svmr_nms on the spans scaled by clip_length in float64.
    A parts index (build_corpus_index(parts=): videos longer than max_ctx_l stored as overlapping parts): a video is ranked by
    its best part, and the result is by definition the restricted search over the index rows that allows exactly each query's
    best parts (ANDed with video_allow, whose bits then number SOURCE videos).  top_indices / flat_indices stay in index rows
    (K7, K9 and explain_moments need them); out["top_videos"] (Nq, K) int32 names the source videos; records carry the source
    video's id (meta2vid: source video -> id) and whole-video times (the part's clip offset is added in K10); svmr_video names
    source videos, out["svmr_rows"] the index rows that stood for them.  Refused with a ValueError: external_top, pad_tail=True,
    an exact-rank index, max_pred_l > parts.overlap (such a moment need not lie inside one part).
    An index that takes updates with chains of slots (MutableCorpusIndex.create(..., part_overlap=O)): the same with slots for
    index rows -- the fold walks the chain tables (ops.chain_best_allow), top_videos names each listed slot's HEAD slot, which
    is also the bit a caller's video_allow carries for the video; svmr_video names a video by any of its slots; records carry
    the video's id (slot_ids) and whole-video times (chain_offset).  Refused alike: external_top, pad_tail=True, max_pred_l >
    part_overlap.  In exact-rank mode (create(..., exact_rank=True, exact_part_overlap=O)) all of this holds with the f32
    path's lists: the fold runs on the re-scored candidate lists (stage_exact_topk_f16s), out["q2c"] is None, and svmr_video
    re-scores the slots of the named video (ops.chain_members) to find its best part."""
    if subset is not None:
        _check_subset(subset, index, ops, external_top, pad_tail)
    if video_allow is not None and pad_tail:
        raise ValueError("video_allow and pad_tail=True exclude each other: the reference-shaped tail would have to invent "
                         "rows in the empty video slots of a restricted list")
    fold = index.fold
    if index.live is not None and pad_tail:
        raise ValueError("pad_tail=True on an index that takes updates: the reference-shaped tail would have to invent rows "
                         "in the video slots that stay empty when fewer than K videos are live")
    if fold is not None:
        _check_parts_search(index, max_pred_l, external_top, pad_tail)
    meta2vid, pkw = _decode_operands(index, meta2vid)
    qvec = stage_query_vectors(model, query_feat, query_mask, n_valid_tokens)
    forked = fork_query_linears(model, index, qvec, ops) if not K7_SUMMARIES else None
    q2c, top_w, top_i, exact = stage_video_topk(model, index, qvec, max_vcmr_video, q2c_alpha, ops, external_top,
                                                defer_exact_check, video_allow, subset)
    q_lin = None
    if forked is not None:
        q_lin, lin_done = forked
        torch.cuda.current_stream(q_lin[0].device).wait_event(lin_done)
    fs, fi = stage_moments(model, index, qvec, top_w, top_i, min_pred_l, max_pred_l, max_before_nms, ops, pad_tail, q_lin=q_lin)
    out = dict(q2c=q2c, top_scores=top_w, top_indices=top_i, flat_scores=fs, flat_indices=fi)
    if exact is not None:
        out["exact"] = exact
    if fold is not None:        # (the source video / the head slot of every listed row, -1 in the empty slots)
        out["top_videos"] = fold.video_of(top_i)
    if nms_thd is not None:
        rec, cnt = ops.moments_decode(fs, flat=fi, top_idx=top_i, meta2vid=meta2vid, l_ref=index.l_ref,
                                      clip_length=clip_length, seconds=True, **pkw)
        nrec, nidx, ncnt = ops.nms_moments(rec, cnt, True, nms_thd, max_before=max_before_nms, max_after=max_after_nms)
        out.update(records=rec, record_count=cnt, nms_records=nrec, nms_index=nidx, nms_count=ncnt)
    if svmr_video is not None:
        pv = svmr_video.to(torch.int32).reshape(-1).contiguous()
        if fold is not None and index.exact is not None:
            # no q2c matrix: the slots of each video, re-scored with the query operands the exact-rank chain made, folded to
            # the best part.  The fold leaves one slot per row (the head for a chain of nothing but -inf, where a top-1 by
            # value would find an empty list): the largest id is that slot, -1 for a slot outside the index.
            members = fold.members(ops, pv)
            sc = ops.q2c_rescore(exact["q_rescore"], [index.exact.feat1n_f32[m] for m in index.modalities],
                                 [index.mask[m] for m in index.modalities], members)
            pv = fold.fold_candidates(ops, sc, members)[1].amax(1).to(torch.int32)
        elif fold is not None:      # a video per query (a SOURCE video; any slot of a chain): the index row of its best part
            pv = fold.best_rows(ops, q2c, pv)      # for that query stands for it (-1: unknown id / outside the index)
        if fold is not None:
            out["svmr_rows"] = pv
        pv = pv.reshape(-1, 1)
        st1, ed1 = stage_span_probs(model, index, qvec, pv, ops, q_lin=q_lin)
        ss, sf = ops.moment_topk(st1, ed1, None, index.l_ref, min_pred_l, max_pred_l, max_before_nms)
        if pad_tail:
            pad_moment_tail(ss, sf, 1, index.l_ref, min_pred_l, max_pred_l)
        out.update(svmr_scores=ss, svmr_flat=sf, svmr_st=st1[:, 0], svmr_ed=ed1[:, 0])
        if nms_thd is not None:
            rec, cnt = ops.moments_decode(ss, flat=sf, row_vid=pv.reshape(-1), meta2vid=meta2vid, l_ref=index.l_ref,
                                          seconds=False, **pkw)
            nrec, nidx, ncnt = ops.nms_moments(rec, cnt, False, nms_thd, scale=clip_length, max_before=max_before_nms,
                                               max_after=max_after_nms)
            out.update(svmr_records=rec, svmr_record_count=cnt, svmr_nms_records=nrec, svmr_nms_index=nidx,
                       svmr_nms_count=ncnt)
    return out


def _as_pairs(t, name, device):
    t = torch.as_tensor(t)
    if t.dim() != 1 or (t.numel() and t.dtype.is_floating_point):
        raise ValueError("explain_moments: %s must be a 1-D integer array" % name)
    return t.to(device=device, dtype=torch.int32).contiguous()


def explain_moments(model, index, query_feat, query_mask, pair_q, pair_vid, ops=hip_ops, with_q2c=True, to_host=False):
    """Why did video v rank / localise where it did for query q: the arrays of the reference's XML.get_visualization_data
    (xml/model_xml.py:253-289) for P listed (query, video) pairs against the RESIDENT index -- the corpus is not re-encoded.

      pair_q (P,)   row of query_feat; pair_vid (P,) index-LOCAL video row (a record's video_idx - index.video_offset)

    The queries are encoded once (packed when encode_query would pack them) with K5 keeping its softmax weights, the query
    linears are applied, and K7's evidence variant reads index.feat2 / index.mask in place (bf16, f32 or split-f16 rows).
    Returns a dict of device tensors (to_host=True: numpy arrays):
      modular_att (Nq, Lq, n_mod)  pooling weight of every query token per stream, 0 at padded tokens
      video_similarity, sub_similarity, similarity (P, l_ref)  per-clip q' . feat2 of each stream (unmasked; the stream a
                    model does not have is None) and their mean -- what the span filters run over in a merged model
      st_logits, ed_logits (P, l_ref)  masked logits, bitwise K7's (ops.convse_rerank(softmax=False)): -1e10 at masked clips
      ctx_len (P,)  valid clips of the pair's video (1 + its last unmasked clip); columns beyond it hold what K7 holds there
      q2c (P,)      video-level score of the pair: its entry of stage_q2c's matrix, or the re-scored f32-grade value on an
                    exact-rank index (with_q2c=False: None -- on a plain index the score costs a K6 pass over the corpus)
    Corpus shards (tvretrieval_amd.dist) are not handled: every pair_vid must lie in [0, index.n_videos)."""
    mods = index.modalities
    dev = index.device
    pq, pv = _as_pairs(pair_q, "pair_q", dev), _as_pairs(pair_vid, "pair_vid", dev)
    if pq.shape != pv.shape:
        raise ValueError("explain_moments: pair_q and pair_vid differ in length (%d, %d)" % (pq.numel(), pv.numel()))
    nq, n_pairs = int(query_feat.shape[0]), int(pq.numel())
    if n_pairs:
        lo_v, hi_v, lo_q, hi_q = (int(x) for x in torch.stack([pv.min(), pv.max(), pq.min(), pq.max()]).tolist())
        if lo_v < 0 or hi_v >= index.n_videos:
            raise ValueError("explain_moments: pair_vid must be index-local rows in [0, %d) (a record's video_idx minus "
                             "index.video_offset = %d); got values in [%d, %d]"
                             % (index.n_videos, index.video_offset, lo_v, hi_v))
        if lo_q < 0 or hi_q >= nq:
            raise ValueError("explain_moments: pair_q must be rows of query_feat in [0, %d); got values in [%d, %d]"
                             % (nq, lo_q, hi_q))
    l_ref, lq, n_mod = index.l_ref, int(query_feat.shape[1]), len(mods)
    finish = lambda d: {k: (v.cpu().numpy() if (to_host and v is not None) else v) for k, v in d.items()}   # noqa: E731
    if nq:            # (an out-of-range check above: no queries means no pairs)
        with torch.no_grad():
            vq, sq, att = model.encode_query(query_feat, query_mask, return_modular_att=True)
        qvec = {m: q for m, q in (("video", vq), ("sub", sq)) if m in mods}
    else:
        att = torch.zeros((0, lq, n_mod), dtype=torch.float32, device=dev)
    if n_pairs == 0:
        rows = lambda m: torch.zeros((0, l_ref), dtype=torch.float32, device=dev) if m in mods else None   # noqa: E731
        return finish(dict(modular_att=att, video_similarity=rows("video"), sub_similarity=rows("sub"),
                           similarity=rows(mods[0]), st_logits=rows(mods[0]), ed_logits=rows(mods[0]),
                           ctx_len=torch.zeros((0,), dtype=torch.int32, device=dev),
                           q2c=torch.zeros((0,), dtype=torch.float32, device=dev) if with_q2c else None))
    with torch.no_grad():
        q_lin = query_linears(model, index, qvec)
        split = index.feat2[mods[0]].dtype is ops.F16S
        if split:
            q_lin = [ops.split_f16_rows(q.float().contiguous()) for q in q_lin]      # per-row scales, as stage_span_probs
        merged = bool(model.config.merge_two_stream and n_mod == 2)
        ev = ops.span_evidence(q_lin, [index.feat2[m] for m in mods], [index.mask[m] for m in mods], pq, pv,
                               model._conv_weights(), l_ref, merged, model.config.conv_kernel_size)
        per_stream = dict(zip(mods, (ev.video_similarity, ev.sub_similarity)))     # (operand order = index.modalities)
        cut = lambda t: None if t is None else t[:, :l_ref]          # noqa: E731
        ar = torch.arange(1, index.lpad + 1, device=dev, dtype=torch.int32)
        ctx_len = None
        for m in mods:
            last = ((index.mask[m].index_select(0, pv.long()) != 0).to(torch.int32) * ar).amax(1)
            ctx_len = last if ctx_len is None else torch.maximum(ctx_len, last)
        q2c = None
        if with_q2c and index.exact is not None:
            pv1 = pv.reshape(-1, 1).contiguous()
            qn = [ops.l2norm_rows(qvec[m].float().contiguous()).index_select(0, pq.long()).contiguous() for m in mods]
            if index.exact.mode == "f16s":
                qn = [ops.split_f16_rows(q, ops.F16_UNIT_LOG2) for q in qn]
            q2c = ops.q2c_rescore(qn, [index.exact.feat1n_f32[m] for m in mods], [index.mask[m] for m in mods], pv1)[:, 0]
        elif with_q2c:
            q2c = stage_q2c(index, qvec, ops)[pq.long(), pv.long()]
    out = dict(modular_att=att, video_similarity=cut(per_stream.get("video")), sub_similarity=cut(per_stream.get("sub")),
               similarity=cut(ev.similarity), st_logits=cut(ev.st_logits), ed_logits=cut(ev.ed_logits),
               ctx_len=ctx_len.clamp_max(l_ref), q2c=q2c)
    return finish(out)


_HOST_STREAMS = {}


def _host_streams(device):
    key = str(torch.device(device))
    if key not in _HOST_STREAMS:
        _HOST_STREAMS[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
    return _HOST_STREAMS[key]


class HostSearchBuffers(object):
    """Pinned host memory + device staging of vcmr_search_host, allocated once and reused across calls (pinning a gigabyte of
    queries is a page-locking system call, not part of a search)."""

    def __init__(self, n_queries, width, chunk, lq, d_in, ragged_rows, device, dtype, nms_width=None):
        """nms_width: the pass ends in temporal NMS on the device -- the pinned records and the device -> host copy have this
        (max_after_nms) width; the pre-NMS records (width = max_before_nms) stay on the device."""
        host_width = width if nms_width is None else nms_width
        self.rec = torch.empty((n_queries, host_width, 4), dtype=torch.int32, pin_memory=True)      # xml_moment records
        self.cnt = torch.empty((n_queries,), dtype=torch.int32, pin_memory=True)
        self.rec_dev = torch.empty((n_queries, width, 4), dtype=torch.int32, device=device)
        self.cnt_dev = torch.zeros((n_queries,), dtype=torch.int32, device=device)
        self.nms_dev = self.nms_cnt_dev = None
        if nms_width is not None:
            self.nms_dev = torch.empty((n_queries, nms_width, 4), dtype=torch.int32, device=device)
            self.nms_cnt_dev = torch.zeros((n_queries,), dtype=torch.int32, device=device)
        # two staging sets: chunk c + 1 is copied in while chunk c is searched
        if ragged_rows:
            self.stage = [dict(rows=torch.empty((ragged_rows, d_in), dtype=dtype, device=device),
                               start=torch.empty((chunk + 1,), dtype=torch.int64, device=device)) for _ in range(2)]
        else:
            self.stage = [dict(qf=torch.empty((chunk, lq, d_in), dtype=dtype, device=device),
                               qm=torch.empty((chunk, lq), dtype=torch.float32, device=device)) for _ in range(2)]
        # ONE pair of copy streams per device, shared by every buffer set: the runtime multiplexes streams onto a few hardware
        # queues (four by default) and a stream that lands on the compute stream's queue executes in order WITH it -- a fifth
        # stream made copies and K6 take turns instead of overlapping (profiles/r06_h2h_notes.md)
        self.copy_stream, self.back_stream = _host_streams(device)   # host -> device, device -> host (PCIe is full duplex)
        self.last_done = None                                       # event: the pass that last used these buffers has finished
        self.freed = [None, None]                                   # events: staging set i has been read by its chunk


class PendingHostSearch(object):
    """A vcmr_search_host pass that has been enqueued (wait=False).  result() blocks until its records are in host memory."""

    def __init__(self, buffers, done, fill_timings):
        self.buffers, self.done, self._fill = buffers, done, fill_timings

    def result(self):
        from .results import MOMENT_DTYPE
        self.done.synchronize()
        if self._fill is not None:
            self._fill()
            self._fill = None
        return self.buffers.rec.numpy().view(MOMENT_DTYPE)[..., 0], self.buffers.cnt.numpy()


def host_chunks(nq, first=1024, growth=3, largest=16384):
    """Query ranges of vcmr_search_host: a small first chunk (its copy is the only one nothing overlaps), then chunks growing
    by `growth` -- a chunk's copy (PCIe: ~1.7 ms per 1 024 padded f32 queries) hides behind the previous chunk's K6 (~6.5 ms
    per 1 024 queries on the TVR corpus) as long as it is not more than ~4 x as long.  Boundaries are multiples of 1 024
    queries = four of K6's 256-row query tiles."""
    first = max(256, (int(first) // 256) * 256)
    out, b, n = [], 0, first
    while b < nq:
        e = min(nq, b + n)
        if nq - e < first // 2:          # no sliver at the end
            e = nq
        out.append((b, e))
        b, n = e, min(n * growth, largest)          # (bounded staging memory for very large query sets)
    return out


def vcmr_search_host(model, index, query_feat, query_mask=None, row_start=None, meta2vid=None, chunk=1024, lq=None,
                     clip_length=1.5, buffers=None, timings=None, ops=hip_ops, max_vcmr_video=100, max_before_nms=200,
                     q2c_alpha=20.0, min_pred_l=2, max_pred_l=16, pad_tail=False, chunk_growth=3, wait=True, video_allow=None,
                     nms_thd=None, max_after_nms=100, subset=None):
    """VCMR from host memory to host memory: the path of the reference's query loop (xml/inference.py:302-314 moves every
    batch host -> device, :383-386 moves the lists device -> host; start_end_dataset.py:362-370) for a whole query set.

    Queries arrive in one of two host layouts (pinned for the copies to be asynchronous):
      * query_feat (Nq, Lq, D) f32 + query_mask (Nq, Lq) f32 -- what the reference's collate delivers (padded);
      * query_feat (rows, D) f16 / f32 + row_start (Nq + 1,) int64 -- the feature store's layout (ingest.FeatureStore): the
        queries' token rows back to back, un-normalised; the collate (truncate to lq, l2-normalise, pad, mask) runs on the
        device (xml_ingest_rows).
    The set is cut into growing chunks (host_chunks).  Chunk c + 1 is copied host -> device on a side stream while chunk c
    runs the per-query half of the search -- query encoder, K6 against the whole corpus, K8.  The pair half (K7 reads every
    selected video's feat2 tile once per launch whatever the number of queries: 8.6 GB on the TVR corpus -- one launch, not
    one per chunk) and K9 then run once over all queries, xml_moments_decode turns the lists into [video_idx, st, ed,
    score] records and ONE device -> host copy returns them.  Per query the arithmetic is that of vcmr_search on the whole
    set: the records are bitwise the single-launch records.
    meta2vid (Nv,) int32 device: meta index -> video2idx value (None: the meta index itself).
    Returns (records (Nq, n) numpy view of results.MOMENT_DTYPE on the pinned buffer, count (Nq,) int32 numpy).
    wait=False: returns a PendingHostSearch as soon as the pass is enqueued; its result() gives the same pair.  Two passes can
    be in flight (two buffer sets are kept on the index): the first copy of pass i + 1 then runs under the pair half of pass
    i and the device never idles between query sets -- an idle gap of a few milliseconds costs the next K6 launch 2-3 % by
    itself (clock / cache state; tools/bench_idle_effect.py).  The records of a pass stay valid until the second next pass.
    timings (dict, optional): h2d_s / device_s / decode_s / d2h_s from HIP events (copy and compute overlap: the wall clock
    is the caller's to take).
    video_allow: DEVICE-resident allow words (pack_video_allow), 1 row or one per query of the whole set; every chunk uses
    its own rows.  Not with pad_tail=True.
    subset (video_subset(index, allowed)): every chunk's K6 runs over the view (see vcmr_search); the records are those of
    video_allow=subset.allow.
    nms_thd (None: off, the records are the pre-NMS lists): temporal NMS per video (filter_vcmr_by_nms at this threshold, first
    max_before_nms candidates in, at most max_after_nms out) runs on the device behind K10 (xml_nms_moments, same stream); the
    pinned buffer and the device -> host copy then carry (Nq, max_after_nms) records -- the kept ones, best first, {-1, 0, 0, 0}
    behind each row's count -- instead of (Nq, max_before_nms).  timings gains nms_s."""
    from .results import MOMENT_DTYPE
    import time as _time
    t_enter = _time.perf_counter()
    if subset is not None:
        _check_subset(subset, index, ops, None, pad_tail)
    dev = next(model.parameters()).device
    ragged = row_start is not None
    nq = (row_start.numel() - 1) if ragged else query_feat.shape[0]
    if index.fold is not None:
        _check_parts_search(index, max_pred_l, None, pad_tail)
    if index.live is not None and pad_tail:
        raise ValueError("pad_tail=True on an index that takes updates (see vcmr_search)")
    if video_allow is not None:
        if pad_tail:
            raise ValueError("video_allow and pad_tail=True exclude each other (see vcmr_search)")
        _check_video_allow(video_allow, index, nq)
        if not video_allow.is_cuda:
            raise ValueError("vcmr_search_host: video_allow must already be on the device (a mask is part of the request's "
                             "state, not of the query stream)")
    d_in = query_feat.shape[-1]
    lq = int(lq if lq is not None else (model.config.max_desc_l if ragged else query_feat.shape[1]))
    width = int(max_before_nms)
    nms_width = None if nms_thd is None else max(int(max_after_nms), 1)
    bounds = host_chunks(nq, chunk, chunk_growth)
    rs_host = row_start.numpy() if ragged else None
    max_q = max(e - b for b, e in bounds)
    max_rows = max(int(rs_host[e] - rs_host[b]) for b, e in bounds) if ragged else 0
    if buffers is None:
        # kept on the index between calls: pinning host pages and mapping device memory are system calls, not search time
        key = (nq, width, max_q, lq, d_in, max_rows, str(dev), query_feat.dtype) + (() if nms_width is None else (nms_width,))
        cache = index.__dict__.setdefault("_host_search_buffers", {})
        if key not in cache:
            cache.clear()
            nkw = {} if nms_width is None else dict(nms_width=nms_width)
            cache[key] = [[HostSearchBuffers(nq, width, max_q, lq, d_in, max_rows, dev, query_feat.dtype, **nkw)
                           for _ in range(2)], 0]
        ring = cache[key]
        buffers = ring[0][ring[1]]
        ring[1] ^= 1
    if buffers.last_done is not None:
        buffers.last_done.synchronize()                  # (the pass before the previous one: normally long finished)
    main = torch.cuda.current_stream(dev)
    side = buffers.copy_stream
    meta2vid, pkw = _decode_operands(index, meta2vid)       # (with a fold: the video's id, whole-video times; see vcmr_search)
    if meta2vid is None:
        meta2vid = torch.arange(index.n_videos, dtype=torch.int32, device=dev)
    copied, freed = [None, None], buffers.freed
    ev_h2d = []

    def evt():
        return torch.cuda.Event(enable_timing=timings is not None)

    def send(c):
        b, e = bounds[c]
        st = buffers.stage[c & 1]
        with torch.cuda.stream(side):
            if freed[c & 1] is not None:
                side.wait_event(freed[c & 1])          # the chunk that read this staging set is done with it
            t0, t1 = evt(), evt()
            t0.record(side)
            if ragged:
                r0, r1 = int(rs_host[b]), int(rs_host[e])
                st["rows"][:r1 - r0].copy_(query_feat[r0:r1], non_blocking=True)
                st["start"][:e - b + 1].copy_(row_start[b:e + 1], non_blocking=True)
            else:
                st["qf"][:e - b].copy_(query_feat[b:e], non_blocking=True)
                st["qm"][:e - b].copy_(query_mask[b:e], non_blocking=True)
            t1.record(side)
            ev_h2d.append((t0, t1))
            copied[c & 1] = t1

    with torch.no_grad():
        send(0)
        t_sent = _time.perf_counter()
        qvecs, tws, tis = [], [], []
        t_first = evt()
        for c, (b, e) in enumerate(bounds):
            if c + 1 < len(bounds):
                send(c + 1)
            st = buffers.stage[c & 1]
            main.wait_event(copied[c & 1])
            if c == 0:
                t_first.record(main)
            # the host holds the queries' lengths: the packed encoder is told its token count instead of reading it back
            # (a read-back per chunk is a host synchronisation per chunk)
            if ragged:
                r0 = int(rs_host[b])
                qf, qm = ops.ingest_rows(st["rows"], st["start"][:e - b + 1] - r0, e - b, lq, lq, normalize=True)
                ln = np.minimum(np.diff(rs_host[b:e + 1]), lq)
                n_tok = int(ln.sum()) if (e > b and ln.min() >= 1) else None
            else:
                qf, qm = st["qf"][:e - b], st["qm"][:e - b]
                mh = query_mask[b:e].numpy()
                prefix = bool((mh[:, 0] == 1).all() and ((mh == 0) | (mh == 1)).all() and (mh[:, 1:] <= mh[:, :-1]).all())
                n_tok = int(mh.sum()) if prefix else None
            qvec = stage_query_vectors(model, qf, qm, n_tok)
            done = evt()
            done.record(main)                            # the staging set is free once the query encoder has read it
            freed[c & 1] = done
            allow = video_allow if (video_allow is None or video_allow.shape[0] == 1) else video_allow[b:e]
            _, tw, ti, _ = stage_video_topk(model, index, qvec, max_vcmr_video, q2c_alpha, ops, video_allow=allow,
                                            subset=subset)
            qvecs.append(qvec), tws.append(tw), tis.append(ti)
        one = len(bounds) == 1
        qvec = {m: (qvecs[0][m] if one else torch.cat([q[m] for q in qvecs])) for m in qvecs[0]}
        top_w = tws[0] if one else torch.cat(tws)
        top_i = tis[0] if one else torch.cat(tis)
        fs, fi = stage_moments(model, index, qvec, top_w, top_i, min_pred_l, max_pred_l, max_before_nms, ops, pad_tail)
        t1, t2, t2b, t3 = evt(), evt(), evt(), torch.cuda.Event(enable_timing=timings is not None)
        t1.record(main)
        ops.moments_decode(fs, flat=fi, top_idx=top_i, meta2vid=meta2vid, l_ref=index.l_ref, clip_length=clip_length,
                           seconds=True, out=buffers.rec_dev, out_count=buffers.cnt_dev, **pkw)
        t2.record(main)
        rec_src, cnt_src, t_out = buffers.rec_dev, buffers.cnt_dev, t2
        if nms_thd is not None:
            if buffers.nms_dev is None or buffers.nms_dev.shape[1] != nms_width:
                raise ValueError("vcmr_search_host: buffers were not made for nms_width = %d" % nms_width)
            ops.nms_moments(buffers.rec_dev, buffers.cnt_dev, True, nms_thd, max_before=max_before_nms,
                            max_after=max_after_nms, want_index=False, out=buffers.nms_dev, out_count=buffers.nms_cnt_dev)
            t_out = evt()
            t_out.record(main)
            rec_src, cnt_src = buffers.nms_dev, buffers.nms_cnt_dev
        back = buffers.back_stream                       # the records leave on their own stream: `main` is free for the next pass
        back.wait_event(t_out)
        with torch.cuda.stream(back):
            t2b.record(back)
            buffers.rec.copy_(rec_src, non_blocking=True)
            buffers.cnt.copy_(cnt_src, non_blocking=True)
            t3.record(back)
        buffers.last_done = t3
    t_enq = _time.perf_counter()

    def fill():
        timings.update(host_before_first_copy_s=t_sent - t_enter, host_enqueue_s=t_enq - t_sent,
                       h2d_s=sum(a.elapsed_time(b) for a, b in ev_h2d) * 1e-3,
                       h2d_exposed_s=ev_h2d[0][0].elapsed_time(ev_h2d[0][1]) * 1e-3,
                       device_s=t_first.elapsed_time(t1) * 1e-3, decode_s=t1.elapsed_time(t2) * 1e-3,
                       d2h_s=t2b.elapsed_time(t3) * 1e-3, chunks=len(bounds), chunk_queries=[e - b for b, e in bounds])
        if nms_thd is not None:
            timings.update(nms_s=t2.elapsed_time(t_out) * 1e-3)
    pending = PendingHostSearch(buffers, t3, fill if timings is not None else None)
    return pending.result() if wait else pending


class GraphedVcmrSearch(object):
    """vcmr_search for ONE fixed query-batch shape, captured once into a HIP graph and replayed.

    The reference serves queries in batches of `eval_query_bsz` = 50 (xml/config.py); at that size the pass is a
    chain of ~25 short kernels and the time goes to launch latency, not to the kernels.  One graph launch replaces
    the chain.  Inputs are copied into static buffers, the returned tensors are the graph's static outputs
    (overwritten by the next call: copy them if they must outlive it).  Weights are packed and workspaces sized by
    two eager warm-up passes before the capture; the corpus index and the model weights must not be re-allocated
    afterwards (re-create the object after load_state_dict / an optimizer step).  An index_update.MutableCorpusIndex never
    re-allocates and takes no data-dependent launch decision, so it may be updated (add / replace / remove) between replays:
    the live words are read by the captured pass, and a replay after an update returns the updated result.  On an exact-rank
    one (create(..., exact_rank=True), ops.F16S model) the captured certificate also reads the bound cells index.exact.e_c_dev:
    replays depend on that tensor, like the live words, never being re-allocated (updates and tighten_error_bound() write it
    in place).
    subset=view (video_subset): the captured pass bakes in the view's n_tiles and the pointers of its image, codes, mask words
    and allow row; view.reset(another set) / view.refresh() rewrite those buffers in place, so the next replay searches the
    new set.  A call through a stale view raises ValueError, as the eager search does."""

    def __init__(self, model, index, nq, lq, d_in, video_allow_rows=None, **search_kwargs):
        """video_allow_rows = None | 1 | nq: a restricted search -- a static (rows, ceil(Nv / 32)) allow-word buffer (all videos
        allowed until a call passes a mask) is part of the captured pass; __call__(..., video_allow=) copies into it."""
        if video_allow_rows not in (None, 1, nq):
            raise ValueError("GraphedVcmrSearch: video_allow_rows must be None, 1 or nq = %d, got %r" % (nq, video_allow_rows))
        if "video_allow" in search_kwargs:
            raise ValueError("GraphedVcmrSearch: pass video_allow_rows= here and the mask itself to every call")
        if index.fold is not None:
            raise ValueError("GraphedVcmrSearch: a parts index (build_corpus_index(parts=)) is not captured yet -- the fold and "
                             "K10 with offsets need no host round trip, but the captured pass has not been verified; use "
                             "vcmr_search or vcmr_search_host")
        if index.exact is not None and index.exact.mode != "f16s":
            raise ValueError("the f32 exact-rank mode reads its certificate on the host (the fallback's launch shape "
                             "depends on it): not capturable -- build the index from an ops.F16S model")
        search_kwargs = dict(search_kwargs)
        self.exact = index.exact is not None
        if self.exact:           # split-f16 exact mode: second tier on the device, overflow flag checked after the replay
            search_kwargs["defer_exact_check"] = True
        dev = next(model.parameters()).device
        self.query_feat = torch.zeros((nq, lq, d_in), dtype=torch.float32, device=dev)
        self.query_mask = torch.zeros((nq, lq), dtype=torch.float32, device=dev)
        self.query_mask[:, 0] = 1.0
        self.video_allow = None
        if video_allow_rows is not None:
            self.video_allow = torch.full((video_allow_rows, (index.n_videos + 31) // 32), -1, dtype=torch.int32, device=dev)
            search_kwargs["video_allow"] = self.video_allow
        self._args = (model, index)
        self._kw = search_kwargs
        # the packed-token query encoder (large batches) reads its plan back on the host and launches shapes that depend on
        # the batch's valid-token count: the graph keeps the padded path -- in the warm-ups too, so that the workspaces they
        # size are the captured path's
        from . import model_xml
        pack_was, model_xml.PACK_QUERY_TOKENS = model_xml.PACK_QUERY_TOKENS, False
        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(2):
                    vcmr_search(model, index, self.query_feat, self.query_mask, **self._kw)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph), torch.no_grad():
                self.out = vcmr_search(model, index, self.query_feat, self.query_mask, **self._kw)
        finally:
            model_xml.PACK_QUERY_TOKENS = pack_was

    def __call__(self, query_feat, query_mask, video_allow=None):
        if tuple(query_feat.shape) != tuple(self.query_feat.shape) or tuple(query_mask.shape) != tuple(self.query_mask.shape):
            raise ValueError("GraphedVcmrSearch was captured for queries %s / masks %s, got %s / %s"
                             % (tuple(self.query_feat.shape), tuple(self.query_mask.shape), tuple(query_feat.shape),
                                tuple(query_mask.shape)))
        if self._kw.get("subset") is not None:
            self._kw["subset"].check_fresh()
        if video_allow is not None:
            if self.video_allow is None:
                raise ValueError("GraphedVcmrSearch was captured without a video mask (video_allow_rows=None)")
            if tuple(video_allow.shape) != tuple(self.video_allow.shape) or video_allow.dtype != torch.int32:
                raise ValueError("GraphedVcmrSearch was captured for an int32 video mask of shape %s, got %s %s"
                                 % (tuple(self.video_allow.shape), video_allow.dtype, tuple(video_allow.shape)))
            self.video_allow.copy_(video_allow)
        elif self.video_allow is not None:
            self.video_allow.fill_(-1)          # no mask for this call: every video allowed
        self.query_feat.copy_(query_feat)
        self.query_mask.copy_(query_mask)
        self.graph.replay()
        if self.exact and self.out["exact"]["overflow_dev"] is not None and bool(self.out["exact"]["overflow_dev"].item()):
            # more failing queries / closer scores than the captured second tier holds: this batch through the eager pass
            model, index = self._args
            kw = {k: v for k, v in self._kw.items() if k != "defer_exact_check"}
            with torch.no_grad():
                return vcmr_search(model, index, self.query_feat, self.query_mask, **kw)
        return self.out


def decode_flat(flat, l_ref):
    """(r, st_idx, ed_idx) of the reference's flat index over (K, L, L) (np.unravel_index, :423-425)."""
    flat = np.asarray(flat).astype(np.int64)
    r = flat // (l_ref * l_ref)
    rem = flat - r * l_ref * l_ref
    return r, rem // l_ref, rem % l_ref


class _GraphedBatches(object):
    """compute_query2ctx_info's per-batch search through ONE captured graph (opt.graph_search): batches are padded on the host
    into pinned buffers of the captured shape (eval_query_bsz, max_desc_l, D), sent in one asynchronous copy each, and replayed.
    A batch of 50 queries is ~25 short kernels: issued one by one the host, not the device, sets the pace (TVR val, 218
    batches: 0.19 s of search of which 0.09 s device time)."""

    def __init__(self, model, index, bsz, lq, d_in, with_gt, **search_kwargs):
        dev = next(model.parameters()).device
        self.gt = torch.zeros(bsz, dtype=torch.int32, device=dev) if with_gt else None
        self.g = GraphedVcmrSearch(model, index, bsz, lq, d_in, svmr_video=self.gt, **search_kwargs)
        self.bsz, self.lq, self.d = bsz, lq, d_in
        self.ring = [dict(qf=torch.zeros((bsz, lq, d_in), dtype=torch.float32, pin_memory=True),
                          qm=torch.zeros((bsz, lq), dtype=torch.float32, pin_memory=True),
                          gt=torch.zeros(bsz, dtype=torch.int32, pin_memory=True), ev=None) for _ in range(3)]
        for r in self.ring:
            r["np"] = (r["qf"].numpy(), r["qm"].numpy(), r["gt"].numpy())
        self.i = 0

    def fits(self, seqs):
        return len(seqs) <= self.bsz and max(len(a) for a in seqs) <= self.lq and seqs[0].shape[1] == self.d

    def __call__(self, seqs, gt_rows):
        r = self.ring[self.i]
        self.i = (self.i + 1) % len(self.ring)
        if r["ev"] is not None:
            r["ev"].synchronize()                  # the copies that last read this pinned set are done
        qf, qm, gt = r["np"]
        n = len(seqs)
        lens = np.fromiter((len(a) for a in seqs), dtype=np.int64, count=n)
        valid = np.arange(self.lq)[None, :] < lens[:, None]
        qf[:] = 0.0
        qf[:n][valid] = np.concatenate(seqs, axis=0)
        qm[:] = 0.0
        qm[:n] = valid
        qm[n:, 0] = 1.0                            # filler rows of the last batch: one valid (zero) token, results ignored
        g = self.g
        g.query_feat.copy_(r["qf"], non_blocking=True)
        g.query_mask.copy_(r["qm"], non_blocking=True)
        if self.gt is not None:
            gt[:] = 0
            gt[:n] = gt_rows
            self.gt.copy_(r["gt"], non_blocking=True)
        r["ev"] = torch.cuda.Event()
        r["ev"].record()
        g.graph.replay()
        return g.out


class _ResultSink(object):
    """Device-side result buffer of one task for a whole query set: K10 writes each batch's 16-byte records into its rows,
    the host fetches the buffer ONCE at the end (no per-batch synchronisation, no per-query Python)."""

    def __init__(self, n_queries, width, device):
        self.rec = torch.empty((n_queries, width, 4), dtype=torch.int32, device=device)
        self.cnt = torch.zeros((n_queries,), dtype=torch.int32, device=device)
        self.n = 0
        self.nms_scale = 1.0         # float64 factor on st / ed in front of NMS (SVMR records are in clip units)

    def rows(self, b, nb):
        self.n = max(self.n, b + nb)
        return dict(out=self.rec[b:b + nb], out_count=self.cnt[b:b + nb])

    def nms(self, task, opt, max_after_nms):
        """opt.nms_on_device: ONE xml_nms_moments launch over the whole buffer; the kept records stay on the device until
        fetch_nms.  The reference quirk of eval_epoch is kept: unless opt.nms_on_full_lists is set, NMS sees only the first
        max_after_nms candidates of a list (get_submission_top_n has truncated it in place by then)."""
        max_before = int(opt.max_before_nms)
        if not getattr(opt, "nms_on_full_lists", False):
            max_before = min(max_before, int(max_after_nms))
        n = self.n
        self.kept_rec, _, self.kept_cnt = hip_ops.nms_moments(
            self.rec[:n], self.cnt[:n], task == "VCMR", opt.nms_thd, scale=self.nms_scale,
            max_before=min(max_before, self.rec.shape[1]), max_after=max_after_nms, want_index=False)

    def fetch_nms(self, desc_ids, descs):
        """The kept lists as a MomentResults -- what MomentResults.take makes of the raw lists and host NMS's index lists
        (zeros behind each row's count), without the gather on the host: the device has copied the records."""
        from .results import MOMENT_DTYPE, MomentResults
        n = self.n
        rec = self.kept_rec.cpu().numpy().view(MOMENT_DTYPE)[..., 0]
        cnt = self.kept_cnt.cpu().numpy()
        res = MomentResults.from_records(desc_ids[:n], descs[:n], rec, cnt, scale=None if self.nms_scale == 1.0 else self.nms_scale)
        res.vid[np.arange(res.width)[None, :] >= cnt[:, None]] = 0
        return res

    def eval_raw(self, top_n):
        """(records, count) of the raw lists as eval_epoch evaluates them: cut to the first top_n entries (a view)."""
        n = self.n
        return self.rec[:n, :max(min(int(top_n), self.rec.shape[1]), 1)], self.cnt[:n]

    def eval_kept(self):
        """(records, count, scale) of K11's kept lists."""
        return self.kept_rec, self.kept_cnt, self.nms_scale

    def fetch(self, desc_ids, descs, scale=None, int_spans=False):
        from .results import MOMENT_DTYPE, MomentResults
        n = self.n
        rec = self.rec[:n].cpu().numpy().view(MOMENT_DTYPE)[..., 0]
        return MomentResults.from_records(desc_ids[:n], descs[:n], rec, self.cnt[:n].cpu().numpy(), scale=scale,
                                          int_spans=int_spans)


def _nms_on_device(opt):
    return bool(getattr(opt, "nms_on_device", False)) and getattr(opt, "nms_thd", -1) != -1


def compute_query2ctx_info(model, eval_dataset, opt, ctx_info, max_before_nms=1000, max_n_videos=100,
                           tasks=("SVMR",), ops=hip_ops, as_arrays=False, max_after_nms=100, _sinks=None):
    """Mirror of compute_query2ctx_info (xml/inference.py:252-445).  Same result dict:
    {"VCMR"|"SVMR"|"VR": [dict(desc_id, desc, predictions=[[video_idx, st, ed, score], ...]), ...]}.
    opt.external_inference_vr_res_path (xml/inference.py:264-273,349-355): re-rank the videos of another model's VR
    submission instead of this model's own top-k.
    opt.pad_tail=True (not a reference option): every list has max_before_nms rows like the reference's -- zero-score rows
    where fewer candidates exist -- instead of the positive-score prefix.
    as_arrays=True: each task as a results.MomentResults (the (Nq, n) columns K10 produced) instead of nested lists; the
    reference's "numpy tail" (:391-445) is the device epilogue xml_moments_decode either way -- the lists, when asked for,
    are built from the columns in one C call (results.MomentResults.to_list).
    opt.nms_on_device=True with opt.nms_thd != -1 (not reference options): temporal NMS runs on the device, one launch per
    task over the whole result buffer after the last batch; the kept lists (at most max_after_nms entries each) come back next
    to the raw ones as "VCMR_nms" / "SVMR_nms" -- what post_processing_{vcmr,svmr}_nms makes of the raw lists in eval_epoch.
    _sinks (eval_epoch's, for opt.eval_on_device): "also" adds the device-resident result buffers to the result under
    "_sinks"; "only" returns nothing else -- no record buffer is fetched."""
    is_svmr, is_vr, is_vcmr = "SVMR" in tasks, "VR" in tasks, "VCMR" in tasks
    index = ctx_info["index"]
    video2idx = eval_dataset.video2idx
    video_metas = ctx_info["video_metas"]
    external_query2video = None
    if getattr(opt, "external_inference_vr_res_path", None) is not None:
        # load_external_vr_res2 (xml/inference.py:244-249,264-273): desc_id -> top video predictions of another model
        import json
        from .postproc import get_submission_top_n
        with open(opt.external_inference_vr_res_path, "r") as f:
            ext = get_submission_top_n(json.load(f), top_n=max_n_videos)["VR"]
        external_query2video = {e["desc_id"]: e["predictions"] for e in ext}
        video_idx2meta_idx = {video2idx[m["vid_name"]]: i for i, m in enumerate(video_metas)}
    meta_vid = np.array([video2idx[m["vid_name"]] for m in video_metas])
    meta2vid = torch.from_numpy(meta_vid.astype(np.int32)).to(opt.device)
    eval_dataset.set_data_mode("query")
    eval_dataset.load_gt_vid_name_for_query(is_svmr)
    name2meta = {e["vid_name"]: i for i, e in enumerate(video_metas)}
    clip = opt.clip_length
    l_ref = index.l_ref
    n = len(eval_dataset)
    sink_vcmr = _ResultSink(n, max_before_nms, opt.device) if is_vcmr else None
    sink_svmr = _ResultSink(n, max_before_nms, opt.device) if is_svmr else None
    sink_vr = None
    desc_ids, descs = [], []
    search_kw = dict(max_vcmr_video=max_n_videos, max_before_nms=max_before_nms, q2c_alpha=opt.q2c_alpha,
                     min_pred_l=opt.min_pred_l, max_pred_l=opt.max_pred_l, ops=ops, pad_tail=getattr(opt, "pad_tail", False))
    graphed = None          # opt.graph_search (not a reference option): the batches through one captured graph
    want_graph = (getattr(opt, "graph_search", False) and external_query2video is None and ops is hip_ops and n > 0
                  and torch.device(opt.device).type == "cuda" and not getattr(opt, "debug", False))
    def emit(out, b, nb, gt):
        """K10 on the device: (flat index, local rank) -> [video_idx, st, ed, score] records (xml/inference.py:402-439)"""
        nonlocal sink_vr
        if is_vr:
            n_vr = min(100, out["top_indices"].shape[1])
            if sink_vr is None:
                sink_vr = _ResultSink(n, n_vr, opt.device)
            ops.moments_decode(out["top_scores"], top_idx=out["top_indices"], meta2vid=meta2vid, n=n_vr,
                               **sink_vr.rows(b, nb))
        if is_vcmr:
            ops.moments_decode(out["flat_scores"], flat=out["flat_indices"], top_idx=out["top_indices"], meta2vid=meta2vid,
                               l_ref=l_ref, clip_length=clip, seconds=True, **sink_vcmr.rows(b, nb))
        if is_svmr:     # clip units on the device; the float64 scaling of get_svmr_res_from_st_ed_probs (:229-233) on the host
            ops.moments_decode(out["svmr_scores"], flat=out["svmr_flat"], row_vid=gt, meta2vid=meta2vid, l_ref=l_ref,
                               seconds=False, **sink_svmr.rows(b, nb))

    # Replayed batches of a split-f16 exact-rank index: the captured second tier can overflow (more failing queries / closer
    # scores than it holds).  GraphedVcmrSearch.__call__ reads the flag back after every replay; here that would put a host
    # synchronisation into every batch, so each batch's flag is kept on the device and the flagged batches are searched
    # again eagerly -- and their records overwritten -- before the sinks are fetched.
    exact_flags = []        # (first query, device flag)
    for b in range(0, n, opt.eval_query_bsz):
        items = [eval_dataset[i] for i in range(b, min(n, b + opt.eval_query_bsz))]
        metas = [e["meta"] for e in items]
        nb = len(metas)
        desc_ids.extend(m["desc_id"] for m in metas)
        descs.extend(m["desc"] for m in metas)
        seqs = [e["model_inputs"]["query_feat"] for e in items]
        if want_graph and graphed is None:
            want_graph = False
            arr0 = seqs[0].detach().cpu().numpy() if isinstance(seqs[0], torch.Tensor) else np.asarray(seqs[0])
            try:
                lq = min(int(getattr(opt, "max_desc_l", 30)), int(model.config.max_desc_l))
                graphed = _GraphedBatches(model, index, opt.eval_query_bsz, lq, int(arr0.shape[1]), is_svmr, **search_kw)
            except ValueError:      # (an index whose exact-rank mode is not capturable: the eager pass)
                graphed = None
        if graphed is not None:
            seqs = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in seqs]
        if graphed is not None and graphed.fits(seqs):
            gt_rows = np.fromiter((name2meta[m["vid_name"]] for m in metas), dtype=np.int32, count=nb) if is_svmr else None
            out = graphed(seqs, gt_rows)
            gt = graphed.gt[:nb] if is_svmr else None
            if out.get("exact") is not None and out["exact"].get("overflow_dev") is not None:
                exact_flags.append((b, out["exact"]["overflow_dev"].reshape(-1)[:1].clone()))
            out = {k: (v[:nb] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == graphed.bsz else v)
                   for k, v in out.items()}
            qf = None
        else:
            qf, qm = pad_batch(seqs, opt.device)
            gt = None
            if is_svmr:
                gt = torch.tensor([name2meta[m["vid_name"]] for m in metas], dtype=torch.int32, device=opt.device)
        external_top = None
        if external_query2video is not None:
            info = [external_query2video[m["desc_id"]] for m in metas]
            ext_i = torch.tensor([[video_idx2meta_idx[p[0]] for p in e] for e in info], dtype=torch.int32)
            ext_w = torch.exp(opt.q2c_alpha * torch.tensor([[p[3] for p in e] for e in info], dtype=torch.float32))
            external_top = (ext_i.to(opt.device).contiguous(), ext_w.to(opt.device).contiguous())
        if qf is not None:
            out = vcmr_search(model, index, qf, qm, svmr_video=gt, external_top=external_top, **search_kw)
        emit(out, b, nb, gt)
        if getattr(opt, "debug", False):
            break
    if exact_flags:
        flagged = torch.cat([f for _, f in exact_flags]).cpu().numpy()            # ONE read-back for the whole query set
        for (b, _), over in zip(exact_flags, flagged):
            if not over:
                continue
            items = [eval_dataset[i] for i in range(b, min(n, b + opt.eval_query_bsz))]
            qf, qm = pad_batch([e["model_inputs"]["query_feat"] for e in items], opt.device)
            gt = None
            if is_svmr:
                gt = torch.tensor([name2meta[e["meta"]["vid_name"]] for e in items], dtype=torch.int32, device=opt.device)
            emit(vcmr_search(model, index, qf, qm, svmr_video=gt, **search_kw), b, len(items), gt)
    res = {}
    kept = {}
    if _nms_on_device(opt):         # enqueued before the first fetch
        if is_svmr:
            sink_svmr.nms_scale = float(clip)
            kept["SVMR"] = sink_svmr
        if is_vcmr:
            kept["VCMR"] = sink_vcmr
        for k, sink in kept.items():
            sink.nms(k, opt, max_after_nms)
    handed = None
    if _sinks is not None:
        handed = dict(desc_ids=desc_ids, descs=descs, kept=kept, raw={
            k: (s, sc) for k, s, sc in (("SVMR", sink_svmr, float(clip)), ("VCMR", sink_vcmr, 1.0), ("VR", sink_vr, 1.0))
            if s is not None and s.n > 0})
        if _sinks == "only":
            return {"_sinks": handed}
    if is_svmr:
        res["SVMR"] = sink_svmr.fetch(desc_ids, descs, scale=clip)
    if is_vcmr:
        res["VCMR"] = sink_vcmr.fetch(desc_ids, descs)
    for k, sink in kept.items():
        res[k + "_nms"] = sink.fetch_nms(desc_ids, descs)
    if is_vr and sink_vr is not None:
        res["VR"] = sink_vr.fetch(desc_ids, descs, int_spans=True)
    res = {k: v for k, v in res.items() if len(v) != 0}
    if not as_arrays:
        from .results import to_lists
        res = to_lists(res)
    if handed is not None:
        res["_sinks"] = handed
    return res


def compute_query2ctx_info_svmr_only(model, eval_dataset, opt, ctx_info, max_before_nms=1000, max_n_videos=200,
                                     tasks=("SVMR",), ops=hip_ops, as_arrays=False, max_after_nms=100, _sinks=None):
    """Mirror of compute_query2ctx_info_svmr_only (xml/inference.py:107-167): every query is scored against its
    ground-truth video only (K7 with one pair per query + K9 with k = 1); no corpus-wide similarity.
    _sinks: as in compute_query2ctx_info."""
    index = ctx_info["index"]
    video2idx = eval_dataset.video2idx
    video_metas = ctx_info["video_metas"]
    name2meta = {e["vid_name"]: i for i, e in enumerate(video_metas)}
    meta2vid = torch.tensor([video2idx[m["vid_name"]] for m in video_metas], dtype=torch.int32).to(opt.device)
    eval_dataset.set_data_mode("query")
    eval_dataset.load_gt_vid_name_for_query(True)
    clip, l_ref = opt.clip_length, index.l_ref
    n = len(eval_dataset)
    sink = _ResultSink(n, max_before_nms, opt.device)
    desc_ids, descs = [], []
    for b in range(0, n, opt.eval_query_bsz):
        items = [eval_dataset[i] for i in range(b, min(n, b + opt.eval_query_bsz))]
        metas = [e["meta"] for e in items]
        desc_ids.extend(m["desc_id"] for m in metas)
        descs.extend(m["desc"] for m in metas)
        qf, qm = pad_batch([e["model_inputs"]["query_feat"] for e in items], opt.device)
        gt = torch.tensor([name2meta[m["vid_name"]] for m in metas], dtype=torch.int32, device=opt.device)
        qvec = stage_query_vectors(model, qf, qm)
        st1, ed1 = stage_span_probs(model, index, qvec, gt.reshape(-1, 1).contiguous(), ops)
        ss, sf = ops.moment_topk(st1, ed1, None, l_ref, opt.min_pred_l, opt.max_pred_l, max_before_nms)
        if getattr(opt, "pad_tail", False):
            pad_moment_tail(ss, sf, 1, l_ref, opt.min_pred_l, opt.max_pred_l)
        ops.moments_decode(ss, flat=sf, row_vid=gt, meta2vid=meta2vid, l_ref=l_ref, seconds=False, **sink.rows(b, len(metas)))
        if getattr(opt, "debug", False):
            break
    if _nms_on_device(opt):         # (see compute_query2ctx_info)
        sink.nms_scale = float(clip)
        sink.nms("SVMR", opt, max_after_nms)
    handed = None
    if _sinks is not None:
        handed = dict(desc_ids=desc_ids, descs=descs, kept=dict(SVMR=sink) if _nms_on_device(opt) else {},
                      raw=dict(SVMR=(sink, float(clip))) if sink.n > 0 else {})
        if _sinks == "only":
            return {"_sinks": handed}
    res = sink.fetch(desc_ids, descs, scale=clip)
    out = dict(SVMR=res)
    if _nms_on_device(opt):
        out["SVMR_nms"] = sink.fetch_nms(desc_ids, descs)
    out = out if as_arrays else {k: v.to_list() for k, v in out.items()}
    if handed is not None:
        out["_sinks"] = handed
    return out


def get_eval_res(model, eval_dataset, opt, tasks, max_after_nms, ops=hip_ops, as_arrays=False, _sinks=None):
    """Mirror of get_eval_res (xml/inference.py:448-464)."""
    context_info = compute_context_info(model, eval_dataset, opt, ops=ops)
    if "VCMR" in tasks or "VR" in tasks:
        eval_res = compute_query2ctx_info(model, eval_dataset, opt, context_info, max_before_nms=opt.max_before_nms,
                                          max_n_videos=opt.max_vcmr_video, tasks=tasks, ops=ops, as_arrays=as_arrays,
                                          max_after_nms=max_after_nms, _sinks=_sinks)
    else:
        eval_res = compute_query2ctx_info_svmr_only(model, eval_dataset, opt, context_info,
                                                    max_before_nms=opt.max_before_nms, max_n_videos=max_after_nms,
                                                    tasks=tasks, ops=ops, as_arrays=as_arrays, max_after_nms=max_after_nms,
                                                    _sinks=_sinks)
    eval_res["video2idx"] = eval_dataset.video2idx
    return eval_res


def eval_epoch(model, eval_dataset, opt, tasks=("SVMR",), max_after_nms=100, ground_truth=None, ops=hip_ops,
               as_arrays=False, timings=None, ctx_info=None):
    """The in-memory part of eval_epoch (xml/inference.py:473-531): raw results -> top-n submission -> metrics, and
    the same again after temporal NMS when opt.nms_thd != -1.  (File writing stays with the caller.)
    Returns (submission, metrics, submission_after_nms, metrics_after_nms).

    Everything between the device and the metrics works on (Nq, n) arrays (results.MomentResults: K10's records, one D2H per
    task; batched NMS; the evaluator's array path); the reference's nested lists are built once at the end for the two
    returned submissions -- or not at all with as_arrays=True (the tasks stay MomentResults; `.to_list()` on demand).
    timings: dict that receives the wall-clock split {search, top_n, eval, nms, eval_nms, lists} in seconds.
    ctx_info: a compute_context_info result to reuse (skips the corpus encode).

    Reference quirk kept on purpose: get_submission_top_n truncates the RAW lists in place (clip_alignment_with_language/
    inference.py:503-515), so the NMS stage (xml/inference.py:507-515) only ever sees the first max_after_nms (100)
    candidates, not max_before_nms, and the after-NMS metrics are computed with eval_retrieval's default
    use_desc_type=True.  opt.nms_on_full_lists=True runs NMS on the untruncated lists instead (not the reference).
    opt.nms_on_device=True (not a reference option; host NMS is the default): the after-NMS lists come from xml_nms_moments on
    the device-resident records (compute_query2ctx_info) instead of post_processing_*_nms on the fetched arrays -- the same
    lists, entry for entry.
    opt.eval_on_device=True (not a reference option; the host evaluator is the default): both metric sets come from
    xml_eval_moments on the device-resident records -- the sinks' records cut to max_after_nms, and K11's kept records (or,
    without opt.nms_on_device, the host's after-NMS lists sent back as records) -- against a DeviceGroundTruth built once;
    one small copy of counters per metric set.  The same numbers as evaluate.eval_retrieval, key for key.
    opt.metrics_only=True (needs eval_on_device, and nms_on_device when opt.nms_thd != -1): additionally no record buffer is
    fetched at all; returns (None, metrics, None, metrics_after_nms)."""
    import time
    from . import evaluate, postproc
    from .results import to_lists
    eval_on_device = bool(getattr(opt, "eval_on_device", False))
    metrics_only = bool(getattr(opt, "metrics_only", False))
    with_nms = getattr(opt, "nms_thd", -1) != -1
    if metrics_only and not eval_on_device:
        raise ValueError("opt.metrics_only needs opt.eval_on_device")
    if metrics_only and with_nms and not getattr(opt, "nms_on_device", False):
        raise ValueError("opt.metrics_only with opt.nms_thd != -1 needs opt.nms_on_device")
    if eval_on_device and ops is not hip_ops:
        raise ValueError("opt.eval_on_device needs the HIP ops")
    sinks_kw = dict(_sinks="only" if metrics_only else "also") if eval_on_device else {}
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        if timings is not None:
            timings[name] = timings.get(name, 0.0) + t[-1] - t[-2]
    if ctx_info is None:
        raw = get_eval_res(model, eval_dataset, opt, tasks, max_after_nms, ops=ops, as_arrays=True, **sinks_kw)
    elif "VCMR" in tasks or "VR" in tasks:
        raw = compute_query2ctx_info(model, eval_dataset, opt, ctx_info, max_before_nms=opt.max_before_nms,
                                     max_n_videos=opt.max_vcmr_video, tasks=tasks, ops=ops, as_arrays=True,
                                     max_after_nms=max_after_nms, **sinks_kw)
        raw["video2idx"] = eval_dataset.video2idx
    else:
        raw = compute_query2ctx_info_svmr_only(model, eval_dataset, opt, ctx_info, max_before_nms=opt.max_before_nms,
                                               max_n_videos=max_after_nms, tasks=tasks, ops=ops, as_arrays=True,
                                               max_after_nms=max_after_nms, **sinks_kw)
        raw["video2idx"] = eval_dataset.video2idx
    sinks = raw.pop("_sinks", None)
    # opt.nms_on_device: the kept lists were made on the device, next to the raw ones
    dev_nms = {k[:-4]: raw.pop(k) for k in [k for k in raw if k.endswith("_nms")]}
    lap("search")
    match_number = not getattr(opt, "debug", False)
    use_desc_type = getattr(opt, "dset_name", "tvr") == "tvr"
    dev_gt = None
    if sinks is not None and ground_truth is not None and sinks["raw"]:
        n_rows = max(s.n for s, _ in sinks["raw"].values())
        dev_gt = evaluate.DeviceGroundTruth(ground_truth, eval_dataset.video2idx, sinks["desc_ids"][:n_rows], opt.device,
                                            use_desc_type=use_desc_type or with_nms, match_number=match_number)
    if metrics_only:
        lap("top_n")
        metrics = metrics_nms = None
        if dev_gt is not None:
            metrics = evaluate.eval_retrieval_device(
                {k: s.eval_raw(max_after_nms) + (sc,) for k, (s, sc) in sinks["raw"].items()}, dev_gt,
                use_desc_type=use_desc_type)
        lap("eval")
        if with_nms:
            lap("nms")
            if dev_gt is not None:
                metrics_nms = evaluate.eval_retrieval_device({k: s.eval_kept() for k, s in sinks["kept"].items()}, dev_gt)
            lap("eval_nms")
        if not as_arrays:
            lap("lists")
        return None, metrics, None, metrics_nms
    full = None
    if getattr(opt, "nms_on_full_lists", False):
        full = {k: (v if k == "video2idx" else v.copy()) for k, v in raw.items()}
    submission = postproc.get_submission_top_n(raw, top_n=max_after_nms)      # truncates `raw` in place, like the reference
    if full is not None:
        raw = full
    lap("top_n")
    metrics = None
    if dev_gt is not None:
        metrics = evaluate.eval_retrieval_device(
            {k: s.eval_raw(max_after_nms) + (sc,) for k, (s, sc) in sinks["raw"].items()}, dev_gt,
            use_desc_type=use_desc_type)
    elif ground_truth is not None:
        metrics = evaluate.eval_retrieval(submission, ground_truth, iou_thds=(0.5, 0.7), verbose=False,
                                          match_number=match_number, use_desc_type=use_desc_type)
    lap("eval")
    sub_nms = metrics_nms = None
    if getattr(opt, "nms_thd", -1) != -1:
        sub_nms = dict(video2idx=raw["video2idx"])
        for k, fn in (("SVMR", postproc.post_processing_svmr_nms), ("VCMR", postproc.post_processing_vcmr_nms)):
            if k in dev_nms:
                sub_nms[k] = dev_nms[k]
            elif k in raw:
                sub_nms[k] = fn(raw[k], nms_thd=opt.nms_thd, max_before_nms=opt.max_before_nms,
                                max_after_nms=max_after_nms)         # (arrays in, new arrays out: nothing to deep-copy)
        lap("nms")
        if dev_gt is not None:
            on_dev = {}
            for k in ("SVMR", "VCMR"):
                if k in sinks["kept"]:
                    on_dev[k] = sinks["kept"][k].eval_kept()
                elif k in sub_nms:      # host NMS: its lists go back as records (f32 seconds, so scale = 1.0)
                    rec, cnt = evaluate.records_from_results(sub_nms[k])
                    on_dev[k] = (torch.from_numpy(rec).to(opt.device), torch.from_numpy(cnt).to(opt.device))
            metrics_nms = evaluate.eval_retrieval_device(on_dev, dev_gt)
        elif ground_truth is not None:
            metrics_nms = evaluate.eval_retrieval(sub_nms, ground_truth, iou_thds=(0.5, 0.7), verbose=False,
                                                  match_number=match_number)
        lap("eval_nms")
    if not as_arrays:
        submission = to_lists(submission)
        sub_nms = to_lists(sub_nms) if sub_nms is not None else None
        lap("lists")
    return submission, metrics, sub_nms, metrics_nms
