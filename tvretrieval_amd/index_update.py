"""A resident corpus index that takes updates: videos are added, replaced and removed in place.

  SlotTable            the host side: which of the `capacity` slots are live, the caller's id of each (no GPU needed)
  MutableCorpusIndex   a CorpusIndex of `capacity` slots allocated once; every update is a stream-ordered launch
                       (ops.index_put_rows / ops.index_clear_rows) that reads nothing back and re-allocates nothing

Slot numbers are what top_indices, flat_indices, video_allow bits, svmr_video and explain_moments pairs mean on such an
index.  A search sees `live AND video_allow` (inference.stage_video_topk), i.e. by the definition of a restricted search the
unrestricted search over the corpus of the live videos, in slot numbering.  What depends on the data in a one-shot build is
fixed here for the index's lifetime: K6 always reads mask bits (never the mask-free kernel, no length-bucketed image), K7 / K9
always take the valid lengths (ragged = True), l_ref is set at creation -- so a GraphedVcmrSearch captured on the index stays
valid across updates."""
import heapq

import torch

from . import _lib
from . import ops as hip_ops
from .inference import CorpusIndex, index_lpad


def _int_list(x, what):
    """Slots or ids as a list of Python ints (a tensor, an array, a sequence or one integer)."""
    if hasattr(x, "tolist"):
        x = x.tolist()
    if not isinstance(x, (list, tuple, range)):
        x = [x]
    for v in x:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be integers, got %r" % (what, v))
    return [int(v) for v in x]


class SlotTable(object):
    """Host bookkeeping of a fixed number of video slots: a slot is live or free, free slots are handed out lowest first
    (the numbering is deterministic), every live slot carries the caller's video id (ids are distinct int32 values; a video
    added without one gets its slot number).  The check_* methods validate a whole call and change nothing; the commit_*
    methods are called once the device launch is enqueued."""

    def __init__(self, capacity):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("SlotTable: capacity must be positive, got %d" % capacity)
        self.capacity = capacity
        self._id = [None] * capacity          # slot -> id, None = free
        self._slot = {}                       # id -> slot
        self._free = list(range(capacity))    # heap of the free slots

    @property
    def n_live(self):
        return len(self._slot)

    def is_live(self, slot):
        return 0 <= slot < self.capacity and self._id[slot] is not None

    def live_slots(self):
        return [s for s in range(self.capacity) if self._id[s] is not None]

    def id_of(self, slot):
        if not self.is_live(slot):
            raise ValueError("slot %r is free (or outside [0, %d))" % (slot, self.capacity))
        return self._id[slot]

    def slot_of(self, vid):
        try:
            return self._slot[int(vid)]
        except KeyError:
            raise ValueError("unknown video id %r" % (vid,))

    def _check_slots(self, slots, what):
        for s in slots:
            if not 0 <= s < self.capacity:
                raise ValueError("%s: slot %d is outside [0, %d)" % (what, s, self.capacity))
        if len(set(slots)) != len(slots):
            raise ValueError("%s: duplicate slots in one call: %s" % (what, sorted(s for s in set(slots) if slots.count(s) > 1)))

    def _check_ids(self, slots, ids, what):
        if len(ids) != len(slots):
            raise ValueError("%s: %d ids for %d videos" % (what, len(ids), len(slots)))
        if len(set(ids)) != len(ids):
            raise ValueError("%s: duplicate video ids in one call" % what)
        for v in ids:
            if not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s: video id %d does not fit int32" % (what, v))
            held = self._slot.get(v)
            if held is not None and held not in slots:
                raise ValueError("%s: video id %d is already held by slot %d" % (what, v, held))

    def resolve(self, slots=None, ids=None, what="slots"):
        """The live slots a call names, by slot number or by id: validated (in range, distinct, live / known)."""
        if (slots is None) == (ids is None):
            raise ValueError("%s: name the videos by slots or by ids=, not both" % what)
        if ids is not None:
            slots = [self.slot_of(v) for v in _int_list(ids, what)]
        else:
            slots = _int_list(slots, what)
        self._check_slots(slots, what)
        for s in slots:
            if self._id[s] is None:
                raise ValueError("%s: slot %d is free" % (what, s))
        return slots

    def check_add(self, n, ids=None):
        """The n lowest free slots and the ids their videos will carry."""
        n = int(n)
        if n > len(self._free):
            raise ValueError("add: %d videos into an index with %d free slots of %d (the index is full)"
                             % (n, len(self._free), self.capacity))
        slots = heapq.nsmallest(n, self._free)
        return self.check_put(slots, ids, "add")

    def check_put(self, slots, ids=None, what="put"):
        """slots (any mix of free and live ones) and the ids they will carry: ids=None keeps a live slot's id and gives a free
        slot its own number."""
        slots = _int_list(slots, what)
        self._check_slots(slots, what)
        if ids is None:
            ids = [self._id[s] if self._id[s] is not None else s for s in slots]
        else:
            ids = _int_list(ids, what)
        self._check_ids(slots, ids, what)
        return slots, ids

    def commit_put(self, slots, ids):
        for s in slots:
            if self._id[s] is not None:
                del self._slot[self._id[s]]
                self._id[s] = None
            else:
                self._free.remove(s)
        heapq.heapify(self._free)
        for s, v in zip(slots, ids):
            self._id[s] = v
            self._slot[v] = s

    def commit_remove(self, slots):
        for s in slots:
            del self._slot[self._id[s]]
            self._id[s] = None
            heapq.heappush(self._free, s)


class MutableCorpusIndex(CorpusIndex):
    """A CorpusIndex of `capacity` video slots whose rows are rewritten on the stream (module docstring).  Besides the
    CorpusIndex fields:
      live       (1, ceil(capacity / 32)) int32 device, bit s = slot s holds a video; never re-allocated
      slot_ids   (capacity,) int32 device, slot -> the caller's id: the meta2vid of a search that passes none
      mask_bits  {modality: (capacity, 4) int32}: K6's mask-bit operand (on the tiled layout also feat1n[m].mask_bits)
      n_live     host counter; table: the SlotTable
    n_videos == capacity: the kernels run over all slots."""

    def __init__(self, *a, **kw):
        raise TypeError("use MutableCorpusIndex.create(model, capacity) or MutableCorpusIndex.from_batches(...)")

    @classmethod
    def create(cls, model, capacity, l_ref=None, exact_filter=False, parts=None, video_offset=0, n_total=None):
        """An empty index (all slots free) for `capacity` videos of up to l_ref clips (default model.config.max_ctx_l)."""
        dt = getattr(model, "compute_dtype", torch.float32)
        if dt is hip_ops.F16S or exact_filter:
            raise ValueError("MutableCorpusIndex: no exact-rank mode (an ops.F16S model / exact_filter=True) -- its certificate "
                             "rests on e_c, a bound over the WHOLE corpus that a one-video update cannot maintain")
        if parts is not None:
            raise ValueError("MutableCorpusIndex: no parts table -- the fold of parts into videos is planned for a fixed corpus")
        if video_offset or n_total is not None:
            raise ValueError("MutableCorpusIndex: not a corpus shard (video_offset / n_total): the sharded drivers number "
                             "videos by position in a fixed global corpus")
        table = SlotTable(capacity)
        l_ref = int(model.config.max_ctx_l if l_ref is None else l_ref)
        if l_ref <= 0:
            raise ValueError("MutableCorpusIndex: l_ref must be positive, got %d" % l_ref)
        act = getattr(model, "act_dtype", dt)
        h = int(model.config.hidden_size)
        lpad = index_lpad(l_ref, model, hip_ops)
        if act not in (torch.float32, torch.bfloat16) or lpad > 128 or \
                not _lib.load().xml_q2c_tile_rows_l2norm_ok(h, hip_ops.dt_of(act)):
            raise ValueError("MutableCorpusIndex: xml_index_put_rows takes f32 / bf16 rows of up to 128 clips and a hidden size "
                             "of whole 64-byte slices; got %s, lpad %d, hidden %d" % (act, lpad, h))
        dev = next(model.parameters()).device
        mods = [n for n, u in (("video", model.use_video), ("sub", model.use_sub)) if u]
        cap = table.capacity
        self = object.__new__(cls)
        feat2 = {m: torch.zeros((cap, lpad, h), dtype=act, device=dev) for m in mods}
        mask = {m: torch.zeros((cap, lpad), dtype=torch.float32, device=dev) for m in mods}
        self.mask_bits = {m: torch.zeros((cap, 4), dtype=torch.int32, device=dev) for m in mods}
        feat1n = {}
        for m in mods:
            if hip_ops.q2c_tiled_ok(lpad, h, act):      # the plain two-slots-per-tile image; K6 in mask-bit mode, always
                data = torch.zeros(hip_ops.q2c_tiled_numel(cap * lpad, h, act), dtype=act, device=dev)
                feat1n[m] = hip_ops.TiledRows(data, cap * lpad, h, (cap, lpad, h), all_valid=False)
                feat1n[m].mask_bits = self.mask_bits[m]
            else:
                feat1n[m] = torch.zeros((cap, lpad, h), dtype=act, device=dev)
        CorpusIndex.__init__(self, mods, feat1n, feat2, mask, l_ref)
        self.raw_feat1 = {}
        self.vlen = torch.full((cap,), l_ref, dtype=torch.int32, device=dev)
        self.ragged = True                   # K7 / K9 always take vlen: the launch shape does not depend on the data
        self.live = torch.zeros((1, (cap + 31) // 32), dtype=torch.int32, device=dev)
        self.slot_ids = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.table = table
        self.model = model
        return self

    @classmethod
    def from_batches(cls, model, context_batches, capacity, l_ref=None, ids=None, **kw):
        """create + one add per (video_feat, video_mask, sub_feat, sub_mask) batch; ids: the videos' ids, in order."""
        self = cls.create(model, capacity, l_ref, **kw)
        ids = None if ids is None else _int_list(ids, "ids")
        r = 0
        for vf, vm, sf, sm in context_batches:
            b = int((vf if vf is not None else sf).shape[0])
            self.add(vf, vm, sf, sm, ids=None if ids is None else ids[r:r + b])
            r += b
        return self

    capacity = property(lambda self: self.table.capacity)
    n_live = property(lambda self: self.table.n_live)

    def set_valid_lengths(self):
        return self                           # vlen is maintained per slot by the update kernels; ragged stays True

    def slot_of(self, vid):
        return self.table.slot_of(vid)

    def hbm_bytes(self):
        extra = list(self.mask_bits.values()) + [self.vlen, self.live, self.slot_ids]
        return CorpusIndex.hbm_bytes(self) + sum(t.numel() * t.element_size() for t in extra)

    # ---- updates --------------------------------------------------------------------------------------------------------
    def _to_device(self, values):
        """Host integers -> int32 device tensor by an asynchronous copy from pinned memory (the only traffic of an update,
        host -> device)."""
        return torch.tensor(values, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)

    def _check_batch(self, video_feat, video_mask, sub_feat, sub_mask, what):
        feats = dict(video=(video_feat, video_mask), sub=(sub_feat, sub_mask))
        b = None
        for m in self.modalities:
            f, k = feats[m]
            if f is None or k is None:
                raise ValueError("%s: the index holds the %s modality, the batch does not" % (what, m))
            if f.dim() != 3 or tuple(k.shape) != tuple(f.shape[:2]):
                raise ValueError("%s: %s features (b, l, D) and mask (b, l) expected" % (what, m))
            if f.shape[1] > self.l_ref:
                raise ValueError("%s: a batch of padded width %d into an index of l_ref = %d clips" % (what, f.shape[1], self.l_ref))
            if b is not None and f.shape[0] != b:
                raise ValueError("%s: the modalities hold %d and %d videos" % (what, b, f.shape[0]))
            b = int(f.shape[0])
        if not b:
            raise ValueError("%s: an empty batch" % what)
        return b

    def encode(self, video_feat, video_mask, sub_feat, sub_mask):
        with torch.no_grad():
            v1, v2, s1, s2 = self.model.encode_context(video_feat, video_mask, sub_feat, sub_mask)
        enc = dict(video=(v1, v2, video_mask), sub=(s1, s2, sub_mask))
        return {m: enc[m] for m in self.modalities}

    def put(self, slots, enc, ids=None):
        """Write an ENCODED batch, enc[m] = (feat1, feat2, mask) of (b, lb <= l_ref) rows as model.encode_context returns them,
        into the b distinct slots; a live slot is replaced, a free one becomes live.  ids=None keeps / assigns ids as
        SlotTable.check_put says.  Returns the slots."""
        slots, ids = self.table.check_put(slots, ids)
        mods = self.modalities
        if set(enc) != set(mods):
            raise ValueError("put: the batch holds modalities %s, the index %s" % (sorted(enc), mods))
        for m in mods:
            a1, a2, am = enc[m]
            if a1.shape[0] != len(slots) or a1.shape[1] > self.l_ref:
                raise ValueError("put: %d slots and l_ref = %d for a batch of shape %s" % (len(slots), self.l_ref, tuple(a1.shape)))
        both = self._to_device([slots, ids])
        hip_ops.index_put_rows([enc[m][0].contiguous() for m in mods], [enc[m][1].contiguous() for m in mods],
                               [enc[m][2].float().contiguous() for m in mods], both[0], both[1],
                               [self.feat1n[m] for m in mods], [self.feat2[m] for m in mods], [self.mask[m] for m in mods],
                               [self.mask_bits[m] for m in mods], self.vlen, self.slot_ids, self.live.view(-1), self.l_ref)
        self.table.commit_put(slots, ids)
        return slots

    def add(self, video_feat, video_mask, sub_feat, sub_mask, ids=None):
        """Encode a context batch and store its videos in the lowest free slots; returns the slots (a list, batch order)."""
        b = self._check_batch(video_feat, video_mask, sub_feat, sub_mask, "add")
        slots, ids = self.table.check_add(b, ids)
        return self.put(slots, self.encode(video_feat, video_mask, sub_feat, sub_mask), ids)

    def replace(self, slots, video_feat, video_mask, sub_feat, sub_mask, ids=None, new_ids=None):
        """Encode a context batch over the LIVE slots named by `slots` (or, slots=None, by ids=); the videos keep their ids
        unless new_ids gives others.  Returns the slots."""
        slots = self.table.resolve(slots, ids, "replace")
        b = self._check_batch(video_feat, video_mask, sub_feat, sub_mask, "replace")
        if b != len(slots):
            raise ValueError("replace: %d slots for a batch of %d videos" % (len(slots), b))
        slots, new_ids = self.table.check_put(slots, new_ids, "replace")
        return self.put(slots, self.encode(video_feat, video_mask, sub_feat, sub_mask), new_ids)

    def remove(self, slots=None, ids=None):
        """Free the LIVE slots named by `slots` (or by ids=): searches enqueued afterwards no longer see them.  Returns them."""
        slots = self.table.resolve(slots, ids, "remove")
        if slots:
            mods = self.modalities
            hip_ops.index_clear_rows(self._to_device(slots), [self.mask[m] for m in mods], [self.mask_bits[m] for m in mods],
                                     self.vlen, self.live.view(-1), self.l_ref)
            self.table.commit_remove(slots)
        return slots
