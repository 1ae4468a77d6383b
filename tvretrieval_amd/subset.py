"""Subset views of a resident corpus index: a restricted search at the cost of the allowed videos.

`vcmr_search(..., video_allow=bits)` restricts a search exactly, but K6 still scores every video.  A VideoSubset holds COPIES
of the K6 blocks of the allowed videos in a small packed image of its own (xml_index_gather_blocks, one device pass), with a
code table that names each block's video IN THE PARENT'S NUMBERING: xml_q2c_scores_packed over the view writes out[q, v] into
the video's own column of the usual (Nq, Nv) matrix, bitwise the value the parent's K6 writes there, and everything behind K6
-- K8 under the view's allow row, the exact-rank chain, K7 - K11 -- runs on the parent unchanged.

Every resident K6 operand is the same slice-major image in blocks of 16 rows; what differs is where a video's blocks lie:
  fixed tiled image (one-shot, IndexStorage, MutableCorpusIndex(tiles=None), exact-rank filter image)   blocks 8 v .. 8 v + nb - 1
  length-bucketed one-shot image (ops.PackPlan)      the run the plan gave the video (inverted once from plan.slot_ids)
  packed MutableCorpusIndex(tiles=N)                 the BlockTable's run of the slot
with nb = max(1, ceil(valid length / 16)) blocks in 1..8.  place_members lays the members' runs into the view's tiles with
index_update.BlockTable's placement rule, in member order.

Host traffic of a creation / reset: one asynchronous upload of the tables (source block per destination block, codes, allow
words) from pinned memory, and -- only where the lengths are not known on the host -- one read of vlen.
"""
import numpy as np
import torch

from . import ops as hip_ops
from .index_update import BlockTable, blocks_of


def _view_error(msg):
    return ValueError("video_subset: " + msg)


def place_members(members, n_blocks, first_src, tiles=None):
    """Pure host placement of a view.  members: the videos' numbers in the parent index, ascending; n_blocks: blocks of each
    (1..8); first_src: the first SOURCE block of each.  Every member gets one run of n_blocks consecutive blocks inside one
    tile (a run may cross blocks 7|8, never a tile boundary; runs do not overlap), by BlockTable's rule in member order -- so
    the view uses exactly the tiles an in-order BlockTable uses.  tiles=None: as many tiles as that takes (at least one);
    tiles=N: N tiles, ValueError when the members do not fit.
    Returns (src_block (16 T,) int32: source block per destination block, -2 = unused; codes (2 T, 8) int32 as
    xml_q2c_scores_packed reads them: -1 inside a run, the member's number at its last block, -3 at block 7 of a run that goes
    on in block 8, -2 elsewhere; firsts (n,) int64: each member's first destination block)."""
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    nb = np.asarray(n_blocks, dtype=np.int64).reshape(-1)
    src = np.asarray(first_src, dtype=np.int64).reshape(-1)
    n = members.size
    if nb.size != n or src.size != n:
        raise _view_error("%d members, %d block counts, %d source blocks" % (n, nb.size, src.size))
    if n and (nb.min() < 1 or nb.max() > 8):
        raise _view_error("a video occupies 1..8 blocks of 16 clips, got %d..%d" % (nb.min(), nb.max()))
    if n > 1 and (np.diff(members) <= 0).any():
        raise _view_error("the member videos must be distinct and ascending")
    if tiles is not None and (isinstance(tiles, bool) or int(tiles) != tiles or int(tiles) <= 0):
        raise _view_error("tiles must be a positive number of 256-row tiles, got %r" % (tiles,))
    # a tile that holds ONE run has a free run of >= 8 blocks behind it, which takes any video: a new tile is opened only when
    # every open one holds two runs or more -- ceil(n / 2) tiles always suffice
    table = BlockTable(int(tiles) if tiles is not None else max(1, (n + 1) // 2))
    firsts = np.empty(n, dtype=np.int64)
    for i in range(n):
        f = table._place(int(nb[i]))
        if f is None:
            raise _view_error("the set does not fit: no room for member %d (video %d, %d blocks) in a view of %d tiles -- %d "
                              "of its %d blocks are free, the largest free run holds %d"
                              % (i, members[i], nb[i], table.n_tiles, table.free_blocks, table.n_tiles * 16,
                                 table.largest_free_run()))
        table._take(f, int(nb[i]), i)
        firsts[i] = f
    n_tiles = table.n_tiles if tiles is not None else max(1, int((firsts + nb - 1).max()) // 16 + 1 if n else 1)
    src_block = np.full(n_tiles * 16, -2, dtype=np.int32)
    codes = np.full(n_tiles * 16, -2, dtype=np.int32)
    if n:
        seg = np.repeat(np.arange(n), nb)
        within = np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)
        dst = firsts[seg] + within
        src_block[dst] = (src[seg] + within).astype(np.int32)
        codes[dst] = -1
        codes[firsts + nb - 1] = members.astype(np.int32)
        straddles = ((firsts & 15) < 8) & ((firsts & 15) + nb > 8)
        codes[(firsts[straddles] & ~15) + 7] = -3
    return src_block, codes.reshape(2 * n_tiles, 8), firsts


def invert_pack_plan(plan):
    """(first block (Nv,) int64, blocks (Nv,) int64) of every video of a length-bucketed one-shot image, read once from the
    plan's code table and kept beside the plan."""
    kept = plan.__dict__.get("_video_runs")
    if kept is None:
        codes = plan.slot_ids.cpu().numpy().reshape(-1).astype(np.int64)
        cont = (codes == -1) | (codes == -3)                      # a block whose video goes on in the next block
        pos = np.arange(codes.size)
        stop = np.maximum.accumulate(np.where(cont, -1, pos))     # the last block <= g that does NOT continue
        last = np.nonzero(codes >= 0)[0]
        before = np.where(last > 0, stop[np.maximum(last - 1, 0)], -1)
        first = np.full(plan.n_videos, -1, dtype=np.int64)
        nb = np.zeros(plan.n_videos, dtype=np.int64)
        first[codes[last]] = before + 1
        nb[codes[last]] = last - before
        kept = (first, nb)
        plan._video_runs = kept
    return kept


def check_parent(index):
    """What a view cannot be made of (or searched through), each with its reason; returns the parent's form:
    "fixed" | "plan" | "packed"."""
    if getattr(index, "parts", None) is not None:
        raise _view_error("a parts index (build_corpus_index(parts=)): its rows are PARTS that the fold ranks by the best of "
                          "each video over the whole score row -- a view would have to hold every part of a member")
    if getattr(index, "chain_head", None) is not None:
        raise _view_error("an index with chains of slots (part_overlap=): a video is several slots that the fold ranks by "
                          "the best part -- a view would have to hold every slot of a member's chain")
    if index.video_offset or index.n_total != index.n_videos:
        raise _view_error("a corpus shard (video_offset / n_total): the sharded drivers number videos by their position in "
                          "the global corpus and take no view")
    mods = index.modalities
    t0 = index.feat1n[mods[0]]
    if index.lpad != 128 or not all(isinstance(index.feat1n[m], hip_ops.TiledRows) for m in mods):
        raise _view_error("the parent's K6 operand is not the tiled image (lpad = %d; the tiled kernel takes 128-clip slots and "
                          "f32 / bf16 rows of whole 64-byte slices): there are no 16-row blocks to gather" % index.lpad)
    if t0.dtype not in (torch.float32, torch.bfloat16) or not hip_ops.q2c_tiled_ok(128, t0.hidden, t0.dtype):
        raise _view_error("the parent's K6 operand is not the tiled image xml_index_gather_blocks copies (f32 / bf16 rows of a "
                          "hidden size xml_q2c_tiled_ok takes); got %s, hidden %d" % (t0.dtype, t0.hidden))
    if getattr(index, "blocks", None) is not None:
        return "packed"
    if t0.plan is not None:
        return "plan"
    for m in mods:
        t = index.feat1n[m]
        if not t.all_valid and t.mask_bits is None:
            raise _view_error("float, non-binary clip masks (modality %s): the packed kernel reads one mask BIT per clip, the "
                              "parent's K6 multiplies by the float mask" % m)
    return "fixed"


def member_list(index, allowed):
    """allowed -- a (Nv,) bool array / tensor or an ascending list of video numbers -- as an ascending int64 numpy array."""
    nv = index.n_videos
    if torch.is_tensor(allowed):
        allowed = allowed.detach().cpu().numpy()
    a = np.asarray(allowed)
    if a.dtype == np.bool_:
        if a.shape != (nv,):
            raise _view_error("a bool array of shape (%d,) expected, got %s" % (nv, a.shape))
        return np.nonzero(a)[0].astype(np.int64)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise _view_error("allowed must be a (Nv,) bool array or an ascending list of video numbers")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= nv or (np.diff(a) <= 0).any():
        raise _view_error("video numbers must be distinct, ascending and in [0, %d)" % nv)
    return a


class _ViewPlan(object):
    """What ops.q2c_scores_fused asks of a PackPlan: the code table, the tiles, and the columns of the matrix it writes."""

    def __init__(self, codes, n_tiles, n_videos):
        self.slot_ids, self.n_tiles, self.n_videos = codes, int(n_tiles), int(n_videos)


class VideoSubset(object):
    """A subset view of `index` (inference.video_subset): a packed K6 image of the allowed videos' blocks.
      video_ids  (n_videos,) int32 device: the members, ascending, in the parent's numbering
      allow      (1, ceil(Nv / 32)) int32 device: the row inference.pack_video_allow gives for the set
      n_videos, n_tiles, hbm_bytes()
      k6         per modality an ops.TiledRows over n_tiles * 256 rows whose plan carries the view's codes: the operand
                 ops.q2c_scores_fused runs xml_q2c_scores_packed on
    The view holds COPIES.  On an index_update.MutableCorpusIndex it records index.version and a search through it after an
    add / put / replace / remove raises ValueError until refresh() (or reset) has gathered again; compact() moves blocks
    inside the parent and leaves a view valid.  reset / refresh rewrite the same device buffers in place, on the current stream."""

    def __init__(self, index, allowed, tiles=None, n_clips=None):
        self.index = index
        self.form = check_parent(index)
        mods = index.modalities
        t0 = index.feat1n[mods[0]]
        self.hidden, self.dtype = int(t0.hidden), t0.dtype
        members = member_list(index, allowed)
        src_block, codes, _ = self._plan(members, tiles, n_clips)
        dev = index.device
        self.n_tiles = int(codes.shape[0]) // 2
        self._words = (index.n_videos + 31) // 32
        t = self.n_tiles
        per_tile = hip_ops.q2c_tiled_numel(256, self.hidden, self.dtype)
        self._tables = torch.zeros(32 * t + self._words, dtype=torch.int32, device=dev)
        self.src_block, self.codes = self._tables[:16 * t], self._tables[16 * t:32 * t].view(2 * t, 8)
        self.allow = self._tables[32 * t:].view(1, self._words)
        self.bits = {m: torch.zeros((2 * t, 4), dtype=torch.int32, device=dev) for m in mods}
        self.k6 = {}
        plan = _ViewPlan(self.codes, t, index.n_videos)
        for m in mods:      # (zero-filled once: the rows of unused blocks are never read -- their code is -2 -- but defined)
            data = torch.zeros(t * per_tile, dtype=self.dtype, device=dev)
            self.k6[m] = hip_ops.TiledRows(data, index.n_videos * 128, self.hidden, (index.n_videos, 128, self.hidden))
            self.k6[m].mask_bits, self.k6[m].plan = self.bits[m], plan
        self._gather(members, src_block, codes)

    # ---- host side ----------------------------------------------------------------------------------------------------------
    def _lengths(self, members, n_clips):
        """Valid lengths of the members of a FIXED image as host integers: n_clips when given, else vlen -- the host copy a
        one-shot index keeps after its first use, one device -> host read on an index that takes updates."""
        index = self.index
        if n_clips is not None:
            n_clips = np.asarray([int(x) for x in n_clips], dtype=np.int64)
            if n_clips.size != members.size:
                raise _view_error("%d valid lengths (n_clips) for %d member videos" % (n_clips.size, members.size))
            return n_clips
        if all(index.feat1n[m].all_valid for m in index.modalities) or index.vlen is None:
            return np.full(members.size, 128, dtype=np.int64)
        if index.live is not None:
            ids = torch.from_numpy(members).to(index.device)
            return index.vlen.index_select(0, ids).cpu().numpy().astype(np.int64)
        host = index.__dict__.get("_vlen_host")
        if host is None:
            host = index._vlen_host = index.vlen.cpu().numpy().astype(np.int64)
        return host[members]

    def _plan(self, members, tiles, n_clips):
        """Validation and placement of a member set, host only (nothing of the view changes)."""
        index = self.index
        if index.live is not None:
            dead = [int(v) for v in members if not index.table.is_live(int(v))]
            if dead:
                raise _view_error("slots %s hold no video" % (dead[:8],))
        if self.form == "packed":
            runs = [index.blocks.run_of(int(v)) for v in members]
            first = np.asarray([r[0] for r in runs], dtype=np.int64)
            nb = np.asarray([r[1] for r in runs], dtype=np.int64)
        elif self.form == "plan":
            pf, pn = invert_pack_plan(index.feat1n[index.modalities[0]].plan)
            first, nb = pf[members], pn[members]
        else:
            first = 8 * members
            try:
                nb = np.asarray([blocks_of(n) for n in self._lengths(members, n_clips)], dtype=np.int64)
            except ValueError as e:
                raise _view_error(str(e))
        return place_members(members, nb, first, tiles)

    def _n_blocks_src(self):
        index = self.index
        if self.form == "fixed":
            return 8 * index.n_videos
        return 16 * index.feat1n[index.modalities[0]].plan.n_tiles

    # ---- device side --------------------------------------------------------------------------------------------------------
    def _gather(self, members, src_block, codes):
        """Upload the tables (one asynchronous copy from pinned memory) and gather the blocks: one launch."""
        index, mods = self.index, self.index.modalities
        words = np.zeros(self._words * 32, dtype=np.uint8)
        words[members] = 1
        words = (words.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
        host = np.concatenate([src_block, codes.reshape(-1), words.view(np.int32)])
        self._tables.copy_(torch.from_numpy(host).pin_memory(), non_blocking=True)
        self.video_ids = torch.from_numpy(members.astype(np.int32)).pin_memory().to(index.device, non_blocking=True)
        self.n_videos = int(members.size)
        self._members = members
        src = [index.feat1n[m] for m in mods]
        bits_src = [None if (self.form == "fixed" and t.all_valid) else t.mask_bits for t in src]
        hip_ops.index_gather_blocks(self.src_block, [t.data for t in src], bits_src, self._n_blocks_src(),
                                    [self.k6[m].data for m in mods], [self.bits[m] for m in mods], self.hidden)
        self.blocks_used = int((src_block >= 0).sum())
        self._version = getattr(index, "version", None)

    def reset(self, allowed, n_clips=None):
        """The view of another set in the SAME buffers (n_tiles stays): tables uploaded, blocks gathered, on the current
        stream.  ValueError -- and the view as it was -- when the set does not fit into n_tiles tiles."""
        members = member_list(self.index, allowed)
        src_block, codes, _ = self._plan(members, self.n_tiles, n_clips)
        self._gather(members, src_block, codes)
        return self

    def refresh(self):
        """After updates of the parent: gather the members that are still live again, drop the others."""
        index = self.index
        members = self._members
        if index.live is not None:
            members = np.asarray([v for v in members if index.table.is_live(int(v))], dtype=np.int64)
        src_block, codes, _ = self._plan(members, self.n_tiles, None)
        self._gather(members, src_block, codes)
        return self

    @property
    def stale(self):
        return getattr(self.index, "version", None) != self._version

    def check_fresh(self):
        if self.stale:
            raise ValueError("this subset view is stale: the index was updated (version %s, the view holds copies made at "
                             "version %s) -- call view.refresh() or view.reset(allowed)"
                             % (getattr(self.index, "version", None), self._version))

    def hbm_bytes(self):
        ts = [self._tables, self.video_ids] + list(self.bits.values()) + [t.data for t in self.k6.values()]
        return sum(t.numel() * t.element_size() for t in ts)
