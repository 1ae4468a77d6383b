"""Fine-tuning the QUERY side of the model against a resident corpus index.

The index rows feat1n / feat2 / mask depend on the context-side parameters alone.  With those frozen, a training step needs no
context encoder pass: the context operands of the loss tail are GATHERED from the index rows of the batch's videos
(xml_index_gather_video_rows, one launch), and the loss tail writes query gradients only (xml_q2c_scores_arg_bwd_q,
xml_pair_sim_bwd_q; include/xmlhip_train_index.h).  The fine-tuned model searches the same index with no update to it.

  * `query_side_parameters(model)` freezes the context side and returns what is left, for BertAdam.
  * `xml_forward_train_index(model, index, ...)` is train.xml_forward_train with the context branches replaced by the gather.
  * `IndexTrainStore` is train_data.DeviceTrainStore without context features: a batch carries the videos' index slots.
  * `train.GraphedTrainStep(..., forward=xml_forward_train_index)` captures the step; `train_epoch_index` drives an epoch.
"""
import collections

import numpy as np
import torch

from . import ops
from . import train_data as _td
from . import train_ops as T
from .autograd import CombineLossFn, LinearFn, ModularPoolFn, RankLossFn, SpanLossFn
from .train import SHADOW_WEIGHTS, _encode_input, draw_negative_ranks, train_step

F32 = torch.float32

# what the index does NOT depend on (XML.__init__): the query encoder, the modular pooling, the per-modality query
# projections and the span predictors.  Everything else -- ctx_pos_embed, *_input_proj, *_encoder1/2/3, *_cross_att,
# *_cross_layernorm -- made the index rows.
QUERY_SIDE = ("query_input_proj.", "query_pos_embed.", "query_encoder.", "modular_vector_mapping.", "video_query_linear.",
              "sub_query_linear.", "video_st_predictor.", "video_ed_predictor.", "sub_st_predictor.", "sub_ed_predictor.",
              "merged_st_predictor.", "merged_ed_predictor.")


def split_parameters(model):
    """-> (query side, context side): two lists of (name, parameter) that together are model.named_parameters()."""
    q, c = [], []
    for name, p in model.named_parameters():
        (q if name.startswith(QUERY_SIDE) else c).append((name, p))
    return q, c


def query_side_parameters(model):
    """Freezes the context side (requires_grad_(False) on every parameter the index rows depend on) and returns the list of the
    others -- the parameters a resident index stays valid under.  Hand the list to train.BertAdam."""
    q, c = split_parameters(model)
    for _, p in c:
        p.requires_grad_(False)
    return [p for _, p in q]


# ---------------------------------------------------------------------------------------------------------
# autograd nodes: the loss tail with constant context operands
# ---------------------------------------------------------------------------------------------------------
class QueryScoresFn(torch.autograd.Function):
    """autograd.VideoLevelScoresFn for context rows that are ALREADY normalised and carry no gradient:
    forward(n_mod, queries..., cns..., masks...) -> (Nq, Nv) f32; backward writes the query gradients only."""

    @staticmethod
    def forward(ctx, n_mod, *rest):
        assert n_mod in (1, 2)
        saved, scores = [], None
        for i in range(n_mod):
            query, cn, mask = rest[i].contiguous(), rest[n_mod + i], rest[2 * n_mod + i]
            nv, l, hidden = cn.shape
            if l > 128 or not T.q2c_scores_l2norm_bwd_supported(query.shape[0], nv, l, hidden, query.dtype):
                raise ValueError("QueryScoresFn: xml_q2c_scores_arg / xml_q2c_scores_arg_bwd_q take up to 1024 queries and videos "
                                 "of up to 128 clips, f32 / bf16 rows of hidden %% 8 == 0, hidden <= 2048; got %d x %d x %d x %d %s"
                                 % (query.shape[0], nv, l, hidden, query.dtype))
            qn = ops.l2norm_rows(query)
            if scores is None:
                scores, arg = T.q2c_scores_arg(qn, cn, mask)
            else:
                _, arg = T.q2c_scores_arg(qn, cn, mask, out=scores, combine=True)
            saved += [query, qn, cn, mask, arg]
        ctx.n_mod = n_mod
        ctx.save_for_backward(*saved)
        return scores

    @staticmethod
    def backward(ctx, dscores):
        n_mod = ctx.n_mod
        sets = [ctx.saved_tensors[5 * i:5 * i + 5] for i in range(n_mod)]
        dq = T.q2c_scores_arg_bwd_q(sets, dscores.contiguous(), scale=1.0 / n_mod)
        return (None,) + tuple(dq) + (None,) * (2 * n_mod)


class QueryPairSimFn(torch.autograd.Function):
    """autograd.PairSimFn for a constant f2: sim[b][l] = q[b] . f2[b][l] -> f32; backward writes dq only."""

    @staticmethod
    def forward(ctx, q, f2):
        q = q.contiguous()
        ctx.save_for_backward(f2)
        return T.pair_sim(q, f2)

    @staticmethod
    def backward(ctx, dsim):
        f2, = ctx.saved_tensors
        return T.pair_sim_bwd_q(f2, dsim.contiguous()), None


# ---------------------------------------------------------------------------------------------------------
# the index as a source of training operands
# ---------------------------------------------------------------------------------------------------------
def index_form(model, index):
    """What an index cannot be trained against, each a ValueError with its reason (host only, before any launch); returns the
    form of its K6 operand: "rows" (row-major) | "fixed" | "plan" | "packed" (block images)."""
    why = None
    if index.exact is not None:
        why = ("an exact-rank index (index.exact): its K6 operand is a bf16 FILTER image of an f32 model, not the rows the "
               "scores are made of -- training runs in f32 / bf16 on an index of the same dtype")
    elif model is not None and model.compute_dtype is ops.F16S:
        why = "an ops.F16S model is inference-only (the exact-rank mode's split-f16 model): train in torch.bfloat16 or torch.float32"
    elif index.fold is not None:
        why = ("a parts or chain index (index.fold): a video is several rows, and the row that holds a labelled moment is "
               "not defined")
    elif index.video_offset or index.n_total != index.n_videos:
        why = "a corpus shard (video_offset / n_total): a batch's videos may live on another rank"
    if why is None:
        mods = index.modalities
        dts = {index.feat2[m].dtype for m in mods} | {index.feat1n[m].dtype for m in mods}
        if model is not None and (dts != {model.act_dtype} or mods != [n for n, u in (("video", model.use_video),
                                                                                      ("sub", model.use_sub)) if u]):
            why = ("the model computes %s rows for the modalities %s, the index holds %s rows for %s: the gathered rows would "
                   "not be what this model's context side produces" % (
                       model.act_dtype, [n for n, u in (("video", model.use_video), ("sub", model.use_sub)) if u],
                       sorted(str(d) for d in dts), mods))
    if why is not None:
        raise ValueError("training on a resident index: " + why)
    tiled = [isinstance(index.feat1n[m], ops.TiledRows) for m in mods]
    if not any(tiled):
        return "rows"
    if getattr(index, "blocks", None) is not None:
        return "packed"
    t0 = index.feat1n[mods[0]]
    if t0.plan is not None:
        return "plan"
    for m in mods:
        t = index.feat1n[m]
        if not t.all_valid and t.mask_bits is None:
            raise ValueError("training on a resident index: float, non-binary clip masks (modality %s) on a block image -- the "
                             "gather hands the loss tail one mask per clip, K6 multiplied the scores by the float mask" % m)
    return "fixed"


def slot_first_blocks(index, form, slots):
    """slot -> first block of its run in the block image (numpy int64; zeros for a row-major index): 8 * slot in the fixed
    image, the plan's run in the length-bucketed one, BlockTable.run_of in the packed one."""
    slots = np.asarray(slots, dtype=np.int64)
    if form == "packed":
        return np.asarray([index.blocks.run_of(int(s))[0] for s in slots], dtype=np.int64)
    if form == "plan":
        from .subset import invert_pack_plan
        return invert_pack_plan(index.feat1n[index.modalities[0]].plan)[0][slots]
    return 8 * slots if form == "fixed" else np.zeros_like(slots)


def _n_blocks(index, form):
    if form == "rows":
        return 0
    return 8 * index.n_videos if form == "fixed" else 16 * index.feat1n[index.modalities[0]].plan.n_tiles


def _valid_lengths(index):
    if index.vlen is not None:
        return index.vlen
    full = index.__dict__.get("_vlen_full")
    if full is None:
        full = index._vlen_full = torch.full((index.n_videos,), index.l_ref, dtype=torch.int32, device=index.device)
    return full


def gather_context(index, form, ctx_slots, ctx_first_block, length, out=None):
    """The batch's (cn, feat2, mask) per modality of the index, one launch (ops.index_gather_video_rows)."""
    mods = index.modalities
    return ops.index_gather_video_rows(ctx_slots, ctx_first_block if form != "rows" else None, _valid_lengths(index),
                                       [index.feat1n[m] for m in mods], [index.feat2[m] for m in mods],
                                       [index.mask[m] for m in mods], length, n_blocks=_n_blocks(index, form), out=out)


def xml_forward_train_index(model, index, query_feat, query_mask, ctx_slots, ctx_first_block, st_ed_indices,
                            neg_ctx_rank=None, neg_q_rank=None, as_tensors=False, ctx_len=None):
    """train.xml_forward_train with the context side read from a resident index -> (loss, loss dict), same conventions.

    ctx_slots (N,) int32 device: the index row / slot of every example's video; ctx_first_block (N,) int32 device: the first
    block of its run in a block image (IndexTrainStore makes both; ignored by a row-major index); ctx_len: the batch's context
    length (default and maximum: index.l_ref).  The query branch, the losses and the in-batch negatives are those of the full
    step.  The ONE intended difference: the context rows are the index's -- encoded in eval mode, so without dropout, and
    rounded to the index dtype -- and are constants: no context encoder runs, no context gradient is written.  The model's
    context-side parameters must be frozen (query_side_parameters): a step that moved them would leave the index stale."""
    form = index_form(model, index)
    moving = [name for name, p in split_parameters(model)[1] if p.requires_grad]
    if moving:
        raise ValueError("training on a resident index: the context-side parameters still require gradients (%s, ... %d in all) "
                         "-- a step would move them and the index rows would go stale; freeze them with "
                         "train_index.query_side_parameters(model)" % (moving[0], len(moving)))
    length = index.l_ref if ctx_len is None else int(ctx_len)
    if not 0 < length <= index.l_ref:
        raise ValueError("training on a resident index: ctx_len %d outside (0, l_ref = %d]" % (length, index.l_ref))
    cfg = model.config
    dev = query_feat.device
    query_mask = query_mask.float().contiguous()
    if SHADOW_WEIGHTS and model.compute_dtype == torch.bfloat16 and torch.is_grad_enabled():
        reg = getattr(model.modular_vector_mapping.weight, "_xml_sink", None)
        if reg is not None:             # an optimizer owns the query side: its bf16 / transposed weight copies for this step
            reg.opt.refresh_shadows(model.compute_dtype)
    enc = _encode_input(model, query_feat, query_mask, model.query_input_proj, model.query_encoder, model.query_pos_embed)
    mq = ModularPoolFn.apply(enc, query_mask, model.modular_vector_mapping.weight)
    video_query, sub_query = mq.unbind(0) if mq.shape[0] == 2 else (mq[0], mq[0])

    names = index.modalities
    qs = dict(video=video_query, sub=sub_query)
    ctx = dict(zip(names, gather_context(index, form, ctx_slots, ctx_first_block, length)))
    ms = {n: ctx[n][2] for n in names}
    bsz = query_feat.shape[0]
    zero = torch.zeros((), dtype=F32, device=dev)

    loss_st_ed = zero
    if cfg.lw_st_ed != 0:
        sims = []
        for n in names:
            lin = getattr(model, n + "_query_linear")
            sims.append(QueryPairSimFn.apply(LinearFn.apply(qs[n], lin.weight, lin.bias, False), ctx[n][1]))
        merged = bool(cfg.merge_two_stream and len(names) == 2)
        if merged:
            masks = [ms["video"], ms["video"]]
            filters = [model.merged_st_predictor.weight, model.merged_ed_predictor.weight]
        else:
            masks = [ms[n] for n in names]
            filters = [getattr(model, n + "_st_predictor").weight for n in names] + \
                      [getattr(model, n + "_ed_predictor").weight for n in names]
        loss_st_ed = SpanLossFn.apply(merged, cfg.conv_kernel_size, st_ed_indices.long().contiguous(), len(sims),
                                      *sims, *masks, *filters)

    losses = None
    if cfg.lw_neg_ctx != 0 or cfg.lw_neg_q != 0:
        q2c = QueryScoresFn.apply(len(names), *[qs[n] for n in names], *[ctx[n][0] for n in names], *[ms[n] for n in names])
        if neg_ctx_rank is None or neg_q_rank is None:
            neg_ctx_rank, neg_q_rank = draw_negative_ranks(model, bsz)
        to_dev = lambda r: torch.as_tensor(r).to(device=dev, dtype=torch.int32).contiguous()   # noqa: E731
        if cfg.ranking_loss_type not in ("hinge", "lse"):
            raise NotImplementedError("Only support 'hinge' and 'lse'")
        losses = RankLossFn.apply(q2c, to_dev(neg_ctx_rank), to_dev(neg_q_rank), float(cfg.margin),
                                  cfg.ranking_loss_type == "lse")

    if cfg.lw_st_ed == 0 and losses is None:
        raise ValueError("training on a resident index: every loss weight is zero")
    loss, parts = CombineLossFn.apply(loss_st_ed if cfg.lw_st_ed != 0 else None, losses, cfg.lw_st_ed, cfg.lw_neg_ctx,
                                      cfg.lw_neg_q)
    if not as_tensors:
        parts = parts.tolist()                # one host read for the four numbers
    return loss, {"loss_st_ed": parts[0], "loss_neg_ctx": parts[1], "loss_neg_q": parts[2], "loss_overall": parts[3]}


# ---------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------
class _IndexLengths(object):
    """What train_data.plan_examples asks of a context store -- membership and the row count of a video -- answered from the
    index: a video's rows in a modality are its clips up to the last unmasked one."""

    def __init__(self, row_of, lengths):
        self.row_of, self.lengths = row_of, lengths

    def __contains__(self, name):
        return self.row_of(name) is not None

    def n_rows(self, name):
        return int(self.lengths[self.row_of(name)])


class IndexTrainStore(object):
    """train_data.DeviceTrainStore for xml_forward_train_index: query features and labels resident on the device, and per
    example the index row / slot of its video instead of context features.

    examples / desc_store / dset_name / max_desc_len / clip_length / normalize_tfeat / data_ratio / feature_dtype: as in
    DeviceTrainStore.  index: an inference.CorpusIndex or index_update.MutableCorpusIndex (index_form names what is refused).
    row_of: vid_name -> index row / slot, a dict or a callable (a mutable index: lambda name: index.slot_of(id_of[name])).
    max_ctx_len must be index.l_ref: the (st, ed) labels are clip numbers of the video as the index truncated it; they are
    made by train_data.plan_examples from the index's own clip counts (the subtitle stream's when the index has one).
    batch(ids) / fill(static, ids) -> query_feat, query_mask, ctx_slots, ctx_first_block, st_ed_indices (+ ctx_len, the
    context length as a host integer).  Ids out of range give empty examples (slot -1).

    On a MutableCorpusIndex the store records index.version and raises after an add / replace / remove until refresh();
    compact() moves runs without raising the version: the store compares BlockTable.compactions and re-derives its first
    blocks by itself."""

    def __init__(self, examples, desc_store, index, row_of, dset_name="tvr", max_desc_len=30, max_ctx_len=100, clip_length=1.5,
                 normalize_tfeat=True, data_ratio=1.0, device=None, feature_dtype=torch.float32, model=None):
        self.index = index
        self.form = index_form(model, index)
        if int(max_ctx_len) != index.l_ref:
            raise ValueError("IndexTrainStore: max_ctx_len = %d, the index was built for l_ref = %d -- the labels are clip numbers "
                             "of the video as the index truncated it" % (max_ctx_len, index.l_ref))
        self.examples = _td._load_examples(examples, data_ratio)
        self.max_desc_len, self.max_ctx_len = int(max_desc_len), int(max_ctx_len)
        self.device = torch.device(device) if device is not None else index.device
        self.feature_dtype, self.norm_query = feature_dtype, bool(normalize_tfeat)
        self._row_of = row_of.get if isinstance(row_of, dict) else row_of
        self._desc_store, self._dset_name, self._clip_length = desc_store, dset_name, clip_length
        self.use_video, self.use_sub = "video" in index.modalities, "sub" in index.modalities
        r = self.res = _td._Resident(desc_store, "query", self.device)
        self.item_of = torch.tensor([r.item[str(e["desc_id"])] if str(e["desc_id"]) in r.item else -1 for e in self.examples],
                                    dtype=torch.int32).to(self.device)
        self.refresh()

    def __len__(self):
        return len(self.examples)

    # ---- host side ----------------------------------------------------------------------------------------------------------
    def _slot(self, name):
        """The live index row / slot of a video, None when it has none."""
        try:
            s = self._row_of(name)
        except (KeyError, ValueError, IndexError):
            return None
        if s is None or isinstance(s, bool) or int(s) != s or not 0 <= int(s) < self.index.n_videos:
            return None
        if self.index.live is not None and not self.index.table.is_live(int(s)):
            return None
        return int(s)

    def first_blocks(self, slots):
        return slot_first_blocks(self.index, self.form, slots)

    def refresh(self):
        """(Re)reads the index: slots, liveness, clip counts -> labels, first blocks.  ValueError, by example, for a video
        that is not live in the index."""
        index = self.index
        slots = [self._slot(e["vid_name"]) for e in self.examples]
        dead = [i for i, s in enumerate(slots) if s is None]
        if dead:
            raise ValueError("IndexTrainStore: example %d: video %s is not live in the index (%d such examples)"
                             % (dead[0], self.examples[dead[0]]["vid_name"], len(dead)))
        self.slots_host = np.asarray(slots, dtype=np.int64)
        pos = torch.arange(1, index.lpad + 1, dtype=torch.int32, device=index.device)
        lens = {m: ((index.mask[m] != 0).to(torch.int32) * pos).amax(1).clamp_max(index.l_ref).cpu().numpy() for m in index.modalities}
        stores = {m: _IndexLengths(self._slot, lens[m]) for m in index.modalities}
        self.q_len, self.ctx_len, labels = _td.plan_examples(
            self.examples, self._desc_store, stores.get("video"), stores.get("sub"), self._dset_name, self.max_desc_len,
            self.max_ctx_len, self._clip_length, "_".join(index.modalities))
        self.labels_host = labels
        self.labels = torch.from_numpy(labels).to(self.device)
        self._version = getattr(index, "version", None)
        self._upload_ctx()
        return self

    def _upload_ctx(self):
        """The (n_examples, 2) int64 device table [slot + 1, first block + 1] (xml_gather_index_rows gives zero rows for ids
        out of range: 0 - 1 = -1 is the gather's empty example)."""
        fb = self.first_blocks(self.slots_host)
        self.first_block_host = fb
        self._ctx = torch.from_numpy(np.stack([self.slots_host + 1, fb + 1], 1)).to(self.device)
        self._compactions = self.index.blocks.compactions if self.form == "packed" else None

    @property
    def stale(self):
        return getattr(self.index, "version", None) != self._version

    def _check_fresh(self):
        if self.stale:
            raise ValueError("this IndexTrainStore is stale: the index was updated (version %s, the store read it at version %s) "
                             "-- call store.refresh()" % (getattr(self.index, "version", None), self._version))
        if self.form == "packed" and self.index.blocks.compactions != self._compactions:
            self._upload_ctx()                # compact() moved runs: same videos, same slots, other first blocks

    batch_max = _td.DeviceTrainStore.batch_max
    _host_ids = _td.DeviceTrainStore._host_ids

    def _spec(self, n, lq):
        return collections.OrderedDict([
            ("query_feat", ((n, lq, self.res.dim), self.feature_dtype)), ("query_mask", ((n, lq), F32)),
            ("ctx_slots", ((n,), torch.int32)), ("ctx_first_block", ((n,), torch.int32)), ("st_ed_indices", ((n, 2), torch.int64))])

    # ---- device side --------------------------------------------------------------------------------------------------------
    def _gather(self, ids_dev, lq, out):
        o = out or {}
        f, m, _ = ops.gather_feature_rows(self.res.rows, self.res.row_start, ids_dev, lq, self.max_desc_len, item_of=self.item_of,
                                          normalize=self.norm_query, eps=1e-5, tef=False, out_dtype=self.feature_dtype,
                                          out=o.get("query_feat"), mask_out=o.get("query_mask"), want_len=False)
        st_ed = ops.gather_index_rows(self.labels, ids_dev, out=o.get("st_ed_indices"))
        ctx = ops.gather_index_rows(self._ctx, ids_dev).sub_(1)
        if out is None:
            ctx = ctx.to(torch.int32)
            slots, fb = ctx[:, 0].contiguous(), ctx[:, 1].contiguous()
        else:
            slots, fb = out["ctx_slots"].copy_(ctx[:, 0]), out["ctx_first_block"].copy_(ctx[:, 1])
        return dict(query_feat=f, query_mask=m, ctx_slots=slots, ctx_first_block=fb, st_ed_indices=st_ed)

    def batch(self, ids, lmax=None, lq=None, out=None):
        """-> the keyword dict xml_forward_train_index takes beside model and index.  ids: a host sequence (validated:
        IndexError) or a device int32 tensor (lq must then be given).  lmax / lq None: the batch maximum (ids on the device:
        lmax = l_ref)."""
        if out is not None:
            return self.fill(out, ids)
        self._check_fresh()
        if torch.is_tensor(ids) and ids.is_cuda:
            if lq is None:
                raise ValueError("ids on the device: lq must be given (nothing is read back)")
            if ids.dtype != torch.int32 or ids.dim() != 1:
                raise ValueError("ids on the device: expected a 1-d int32 tensor")
            ids_dev, lmax = ids.contiguous(), self.max_ctx_len if lmax is None else int(lmax)
        else:
            host = self._host_ids(ids)
            bl, bq = self.batch_max(host)
            lmax, lq = bl if lmax is None else int(lmax), bq if lq is None else int(lq)
            ids_dev = torch.from_numpy(host.astype(np.int32)).to(self.device)
        if not 0 < lmax <= self.max_ctx_len:
            raise ValueError("lmax %d outside (0, l_ref = %d]" % (lmax, self.max_ctx_len))
        b = self._gather(ids_dev, int(lq), None)
        b["ctx_len"] = int(lmax)
        return b

    def fill(self, static, ids):
        """Writes the batch of `ids` into existing tensors (GraphedTrainStep.static): shapes and dtypes are checked against
        the request (ValueError).  The launches run on the current stream; static["ctx_len"] stays what the step was
        captured with."""
        self._check_fresh()
        if torch.is_tensor(ids) and ids.is_cuda:
            if ids.dtype != torch.int32 or ids.dim() != 1:
                raise ValueError("ids on the device: expected a 1-d int32 tensor")
            ids_dev = ids.contiguous()
        else:
            ids_dev = torch.from_numpy(self._host_ids(ids).astype(np.int32)).to(self.device)
        q = static.get("query_feat")
        if not torch.is_tensor(q) or q.dim() != 3:
            raise ValueError("fill: the static batch has no (n, lq, d) query features")
        for key, (shape, dtype) in self._spec(int(ids_dev.numel()), int(q.shape[1])).items():
            t = static.get(key)
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError("fill: %s must be a contiguous %s tensor of shape %s, got %s" % (
                    key, dtype, shape, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
        return self._gather(ids_dev, int(q.shape[1]), static)


def train_epoch_index(model, optimizer, store, opt, epoch_i, training=True, step=None, generator=None, order=None, rank=0,
                      world=1, history=None):
    """train_data.train_epoch on an IndexTrainStore -> OrderedDict of the averaged loss terms.  step: a
    GraphedTrainStep(model, optimizer, dict(index=store.index, **store.batch(ids0, lmax=l_ref, lq=max_desc_len)),
    forward=xml_forward_train_index): full batches go through fill + replay, the partial last batch runs eagerly at the same
    fixed shapes; the losses stay on the device until the end of the epoch."""
    keys = _td.LOSS_KEYS
    model.train(mode=training)
    if opt.hard_negtiave_start_epoch != -1 and epoch_i >= opt.hard_negtiave_start_epoch:
        model.set_hard_negative(True, opt.hard_pool_size)
    if opt.train_span_start_epoch != -1 and epoch_i >= opt.train_span_start_epoch:
        model.set_train_st_ed(opt.lw_st_ed)
    _, batches = _td.plan_epoch(len(store), opt.bsz, generator, order, rank, world, bool(getattr(opt, "debug", False)))
    if not batches:
        return collections.OrderedDict((k, 0.0) for k in keys)
    flat = np.concatenate(batches)
    store._host_ids(flat)
    ids_all = torch.from_numpy(flat.astype(np.int32)).to(store.device)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in batches])])
    graphed = step is not None and training
    if graphed:
        n_static, lq_fix = int(step.static["query_feat"].shape[0]), int(step.static["query_feat"].shape[1])
        lmax_fix = int(step.static.get("ctx_len") or store.max_ctx_len)
        on_dev = torch.zeros((len(batches), len(keys)), dtype=F32, device=store.device)
    rows = []
    for bi, host_ids in enumerate(batches):
        ids = ids_all[int(offs[bi]):int(offs[bi + 1])]
        if graphed and len(host_ids) == n_static:
            store.fill(step.static, ids)
            _, parts = step(None)
            torch.stack([parts[k] for k in keys], out=on_dev[bi])
            rows.append(None)
            continue
        lmax, lq = (lmax_fix, lq_fix) if graphed else store.batch_max(host_ids)
        batch = dict(store.batch(ids, lmax=lmax, lq=lq), index=store.index)
        if training:
            _, parts = train_step(model, optimizer, batch, grad_clip=opt.grad_clip, forward=xml_forward_train_index)
        else:
            with torch.no_grad():
                _, parts = xml_forward_train_index(model, **batch)
        rows.append([float(parts[k]) for k in keys])
    if graphed:
        dev_rows = on_dev.tolist()           # the one host read of the captured steps' losses
        rows = [dev_rows[i] if r is None else r for i, r in enumerate(rows)]
    if history is not None:
        history.extend(dict(zip(keys, r)) for r in rows)
    return collections.OrderedDict((k, float(np.mean([r[j] for r in rows]))) for j, k in enumerate(keys))
