"""A resident corpus index that takes updates: videos are added, replaced and removed in place.

  SlotTable            the host side: which of the `capacity` slots are live, the caller's id of each (no GPU needed)
  MutableCorpusIndex   a CorpusIndex of `capacity` slots allocated once; every update is a stream-ordered launch
                       (ops.index_put_rows / ops.index_clear_rows) that reads nothing back and re-allocates nothing
  ChainTable           the SlotTable of an index created with part_overlap=O: a video longer than l_ref clips is a CHAIN of
                       slots, one overlapping part each (ops.index_set_chains keeps the device tables chain_head / chain_next /
                       chain_offset in step; searches fold a chain to its best part, ops.chain_best_allow)
  BlockTable           the host side of the packed form (create(..., tiles=N)): which run of 16-row blocks of the packed K6
                       image each live slot owns (ops.index_put_rows_packed / ops.index_clear_rows_packed keep the image,
                       its code table and its mask words in step); check_compact / commit_compact plan the moves that
                       MutableCorpusIndex.compact() enqueues (ops.index_move_blocks_packed)

Slot numbers are what top_indices, flat_indices, video_allow bits, svmr_video and explain_moments pairs mean on such an
index.  A search sees `live AND video_allow` (inference.stage_video_topk), i.e. by the definition of a restricted search the
unrestricted search over the corpus of the live videos, in slot numbering.  What depends on the data in a one-shot build is
fixed here for the index's lifetime: K6 always reads mask bits (never the mask-free kernel, no length-bucketed image), K7 / K9
always take the valid lengths (ragged = True), l_ref is set at creation -- so a GraphedVcmrSearch captured on the index stays
valid across updates."""
import bisect
import heapq

import torch

from . import _lib
from . import inference as _inference
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

    def _check_ids(self, leaving, ids, what, n=None):
        """ids for the n videos of a call; an id that is held already must be held by one of the slots in `leaving`."""
        n = len(leaving) if n is None else n
        if len(ids) != n:
            raise ValueError("%s: %d ids for %d videos" % (what, len(ids), n))
        if len(set(ids)) != len(ids):
            raise ValueError("%s: duplicate video ids in one call" % what)
        for v in ids:
            if not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s: video id %d does not fit int32" % (what, v))
            held = self._slot.get(v)
            if held is not None and held not in leaving:
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


class ChainTable(SlotTable):
    """SlotTable of an index whose long videos are CHAINS of slots (MutableCorpusIndex.create(..., part_overlap=O); DESIGN.md
    section 20c): a video of several parts takes one slot per part, every slot of it carries the video's id, and an id maps
    to the HEAD slot (the part at offset 0), which is the video's number in results and in a caller's video_allow.  The table
    mirrors the device tables chain_head / chain_next / chain_offset: a free slot and a video of one part are in the SINGLE
    state (head = itself, next = -1, offset = 0).  A chain is added, replaced and removed whole; chains are built here from
    free slots only, each slot once, so the tables never hold a cycle.
    check_chains / check_remove_chains validate a whole call, change nothing and return a plan; commit_chains applies it once
    the launches are enqueued.  plan["records"] is the operand of xml_index_set_chains: {slot, head, next, offset} of every
    touched slot whose state changes.  SlotTable's own calls keep working for videos of one part and refuse a slot that is
    a part of a longer video."""

    def __init__(self, capacity, max_parts=32):
        SlotTable.__init__(self, capacity)
        max_parts = int(max_parts)
        if max_parts < 1:
            raise ValueError("ChainTable: max_parts must be >= 1, got %d" % max_parts)
        self.max_parts = max_parts
        self._head = list(range(self.capacity))       # the mirror of the device tables
        self._next = [-1] * self.capacity
        self._off = [0] * self.capacity

    n_live = property(lambda self: self.capacity - len(self._free))
    n_videos_live = property(lambda self: len(self._slot))

    def state(self, slot):
        """(head, next, offset) of a slot as the device tables hold it."""
        return self._head[slot], self._next[slot], self._off[slot]

    def head_of(self, slot):
        if not self.is_live(slot):
            raise ValueError("slot %r is free (or outside [0, %d))" % (slot, self.capacity))
        return self._head[slot]

    def chain_of(self, slot):
        """The slots of the video that `slot` (any of its parts) belongs to, in offset order."""
        s, out = self.head_of(slot), []
        while s != -1:
            out.append(s)
            s = self._next[s]
        return out

    def heads(self):
        return sorted(self._slot.values())

    def resolve_videos(self, slots=None, ids=None, what="slots"):
        """The head slots of the videos a call names, by any slot of each or by id: validated, one entry per video."""
        heads = [self._head[s] for s in self.resolve(slots, ids, what)]
        if len(set(heads)) != len(heads):
            raise ValueError("%s: a video is named twice in one call (head slots %s)"
                             % (what, sorted(h for h in set(heads) if heads.count(h) > 1)))
        return heads

    # ---- SlotTable's calls: videos of one part only --------------------------------------------------------------------------
    def check_put(self, slots, ids=None, what="put"):
        slots = _int_list(slots, what)
        self._check_slots(slots, what)
        for s in slots:
            if self._head[s] != s or self._next[s] != -1:
                raise ValueError("%s: slot %d is a part of the video at head slot %d; replace or remove the whole video"
                                 % (what, s, self._head[s]))
        return SlotTable.check_put(self, slots, ids, what)

    # ---- chains ------------------------------------------------------------------------------------------------------------
    def check_chains(self, counts, offsets, ids=None, old_heads=None, what="add"):
        """Slots for the videos of one call: counts[i] parts for video i, offsets[i] their first clips (rising from 0).
        old_heads=None (add): every part takes a free slot, lowest first, videos in call order.  old_heads (replace): video i
        takes over the slots of the video at old_heads[i], in order -- the head keeps its number --, the slots it does not
        need are freed, and the parts it has beyond them take the lowest free slots, those just freed included.
        ids: one per video (None: add gives a video its head slot's number, replace keeps the id).  Returns the plan
          heads, ids          per video
          chains              per video the slots of its parts, in offset order
          put_slots, put_ids  per PART, in batch order: where each row of the batch goes and the id it carries
          surplus             the slots a replace frees and no video of the call takes
          records             [[slot, head, next, offset], ...] for xml_index_set_chains
        Nothing changes; ValueError when the call does not fit."""
        counts = [int(c) for c in counts]
        n = len(counts)
        if len(offsets) != n or any(len(o) != c for o, c in zip(offsets, counts)):
            raise ValueError("%s: one offset per part expected" % what)
        for c in counts:
            if c < 1:
                raise ValueError("%s: a video of %d parts" % (what, c))
            if c > self.max_parts:
                raise ValueError("%s: a video of %d parts; the index was created with max_parts = %d (the fold walks a chain "
                                 "per slot: its cost grows with the square of the parts)" % (what, c, self.max_parts))
        old = [[] for _ in range(n)]
        if old_heads is not None:
            if len(old_heads) != n:
                raise ValueError("%s: %d slots for a batch of %d videos" % (what, len(old_heads), n))
            old = [self.chain_of(h) for h in old_heads]
        keep = [o[:c] for o, c in zip(old, counts)]
        freed = sorted(s for o, c in zip(old, counts) for s in o[c:])
        need = sum(c - len(k) for c, k in zip(counts, keep))
        if need > len(self._free) + len(freed):
            raise ValueError("%s: %d parts of %d videos into an index with %d free slots of %d (the index is full)"
                             % (what, need, n, len(self._free) + len(freed), self.capacity))
        pool = sorted(heapq.nsmallest(need, self._free) + freed)[:need]
        chains, at = [], 0
        for c, k in zip(counts, keep):
            chains.append(k + pool[at:at + c - len(k)])
            at += c - len(k)
        heads = [ch[0] for ch in chains]
        if ids is None:
            ids = [self._id[h] if self._id[h] is not None else h for h in heads]
        else:
            ids = _int_list(ids, what)
        self._check_ids(set(s for o in old for s in o), ids, what, n)
        taken = set(s for ch in chains for s in ch)
        surplus = [s for s in freed if s not in taken]
        want = {s: (s, -1, 0) for s in surplus}
        for ch, offs in zip(chains, offsets):
            for j, s in enumerate(ch):
                want[s] = (ch[0], ch[j + 1] if j + 1 < len(ch) else -1, int(offs[j]))
        records = [[s] + list(w) for s, w in sorted(want.items()) if w != self.state(s)]
        return dict(heads=heads, ids=ids, chains=chains, put_slots=[s for ch in chains for s in ch],
                    put_ids=[v for v, ch in zip(ids, chains) for _ in ch], surplus=surplus, records=records,
                    old=[s for o in old for s in o])

    def check_remove_chains(self, heads):
        """The plan that frees the whole videos at `heads` (resolve_videos): slots = every slot of them, records = the single
        state for each of those that is not in it."""
        slots = [s for h in heads for s in self.chain_of(h)]
        return dict(heads=list(heads), slots=slots, records=[[s, s, -1, 0] for s in sorted(slots) if self.state(s) != (s, -1, 0)])

    def _free_slot(self, s):
        self._slot.pop(self._id[s], None)
        self._id[s] = None
        heapq.heappush(self._free, s)

    def commit_remove_chains(self, plan):
        for s in plan["slots"]:
            self._free_slot(s)
            self._head[s], self._next[s], self._off[s] = s, -1, 0

    def commit_chains(self, plan):
        for s in plan["old"]:
            self._free_slot(s)
        for s in plan["put_slots"]:
            self._free.remove(s)
        heapq.heapify(self._free)
        for v, ch in zip(plan["ids"], plan["chains"]):
            for s in ch:
                self._id[s] = v
            self._slot[v] = ch[0]
        for s, h, nx, off in plan["records"]:
            self._head[s], self._next[s], self._off[s] = h, nx, off


def blocks_of(n_clips):
    """Blocks of 16 clips a video of this valid length (last valid clip + 1 over the modalities' masks) occupies in the packed
    K6 image: max(ceil(len / 16), 1), ops.PackPlan's rule."""
    n = int(n_clips)
    if not 0 <= n <= 128:
        raise ValueError("a valid length of %d clips: the packed K6 image holds videos of 0..128 clips (1..8 blocks)" % n)
    return max((n + 15) // 16, 1)


class NoRunError(ValueError):
    """BlockTable.check_put found no free run for a video.  blocks_asked: the blocks of the call's videos that need a run;
    blocks_free: the free blocks once the call's moving videos have left theirs -- when blocks_free >= blocks_asked the space
    may exist without being contiguous, and compaction can help."""

    def __init__(self, message, blocks_asked, blocks_free):
        ValueError.__init__(self, message)
        self.blocks_asked, self.blocks_free = int(blocks_asked), int(blocks_free)


class BlockTable(object):
    """Host bookkeeping of the packed K6 image of a MutableCorpusIndex(tiles=N): n_tiles tiles of 16 blocks (16 clip rows
    each).  A live slot owns one RUN of nb consecutive blocks inside one tile; a run may cross the boundary between blocks 7
    and 8 of its tile (the two wave tiles: a straddle), never a tile boundary.  first = tile * 16 + block numbers the blocks.
    Placement (deterministic): of the maximal free runs that hold nb blocks the SHORTEST; among those of that length one in
    which the video does not straddle before one in which it does; then the lowest (tile, block).  The video sits at the
    start of the chosen free run, so the run is never split in two.  (Moving a video that would straddle up to block 8 was
    tried: no straddle among the TVR clip counts loaded in corpus order, but 5 448 tiles instead of 5 128 -- K6's time follows
    the tiles, a straddle costs one barrier per tile and modality.)  The free runs are the maximal runs of free blocks of each
    tile, so a freed run is one with its free neighbours at once.
    The check_* methods validate a whole call and change nothing; the commit_* methods apply what a check returned, once the
    device launches are enqueued."""

    def __init__(self, n_tiles):
        n_tiles = int(n_tiles)
        if n_tiles <= 0:
            raise ValueError("BlockTable: n_tiles must be positive, got %d" % n_tiles)
        self.n_tiles = n_tiles
        self._owner = [None] * (n_tiles * 16)                     # block -> slot, None = free
        self._run = {}                                            # slot -> (first, nb)
        self._free = [[] for _ in range(17)]                      # length -> sorted first blocks of the maximal free runs
        self._free[16] = [t * 16 for t in range(n_tiles)]
        self.free_blocks = n_tiles * 16
        self.compactions = 0              # raised by every commit_compact that moved a run: a cached slot -> run table is stale

    # ---- queries ----------------------------------------------------------------------------------------------------------
    def run_of(self, slot):
        """(first, nb) of a slot's run, None when it has none."""
        return self._run.get(slot)

    def runs(self):
        """{slot: (first, nb)} of the live runs."""
        return dict(self._run)

    def free_runs(self):
        """The maximal free runs as sorted (first, length) pairs."""
        return sorted((f, n) for n in range(1, 17) for f in self._free[n])

    def largest_free_run(self):
        return max([n for n in range(1, 17) if self._free[n]] or [0])

    def tiles_used(self):
        """Tiles up to and including the last one that holds a block of a video."""
        for b in range(self.n_tiles * 16 - 1, -1, -1):
            if self._owner[b] is not None:
                return b // 16 + 1
        return 0

    def stats(self):
        """Free blocks, the largest free run per tile class (in an empty tile it is 16; `largest_free_run_partial`: in a tile
        that holds a video), live runs, tiles by class, straddling videos."""
        empty = len(self._free[16])
        full = sum(1 for t in range(self.n_tiles) if all(o is not None for o in self._owner[t * 16:t * 16 + 16]))
        return dict(n_tiles=self.n_tiles, free_blocks=self.free_blocks, live_runs=len(self._run),
                    largest_free_run=self.largest_free_run(),
                    largest_free_run_partial=max([n for n in range(1, 16) if self._free[n]] or [0]),
                    tiles_empty=empty, tiles_full=full, tiles_partial=self.n_tiles - empty - full, tiles_used=self.tiles_used(),
                    straddles=sum(1 for f, nb in self._run.values() if (f & 15) < 8 < (f & 15) + nb))

    def row_map(self):
        """(n_tiles * 256,) int32 CPU tensor: packed row -> slot * 128 + clip, -1 where no video lies -- what
        ops.TiledRows.to_rows() needs (tests only: the search never reads it)."""
        rows = torch.full((self.n_tiles * 256,), -1, dtype=torch.int32)
        for slot, (first, nb) in self._run.items():
            rows[first * 16:(first + nb) * 16] = torch.arange(slot * 128, slot * 128 + nb * 16, dtype=torch.int32)
        return rows

    # ---- the free runs ----------------------------------------------------------------------------------------------------
    def _drop_free(self, first, n):
        lst = self._free[n]
        del lst[bisect.bisect_left(lst, first)]

    def _take(self, first, nb, slot):
        """Blocks [first, first + nb), all free, now belong to slot."""
        lo, hi, t0 = first, first + nb, first & ~15
        while lo > t0 and self._owner[lo - 1] is None:
            lo -= 1
        while hi < t0 + 16 and self._owner[hi] is None:
            hi += 1
        self._drop_free(lo, hi - lo)
        if first > lo:
            bisect.insort(self._free[first - lo], lo)
        if hi > first + nb:
            bisect.insort(self._free[hi - first - nb], first + nb)
        self._owner[first:first + nb] = [slot] * nb
        self._run[slot] = (first, nb)
        self.free_blocks -= nb

    def _release(self, slot):
        """The exact inverse of _take: the slot's blocks are free again, one run with their free neighbours."""
        first, nb = self._run.pop(slot)
        lo, hi, t0 = first, first + nb, first & ~15
        while lo > t0 and self._owner[lo - 1] is None:
            lo -= 1
        while hi < t0 + 16 and self._owner[hi] is None:
            hi += 1
        if first > lo:
            self._drop_free(lo, first - lo)
        if hi > first + nb:
            self._drop_free(first + nb, hi - first - nb)
        bisect.insort(self._free[hi - lo], lo)
        self._owner[first:first + nb] = [None] * nb
        self.free_blocks += nb

    def _place(self, nb):
        """First block for a run of nb blocks by the placement rule, None when no free run holds it."""
        for n in range(nb, 17):
            lst = self._free[n]
            if not lst:
                continue
            for f in lst:
                if (f & 15) >= 8 or (f & 15) + nb <= 8:
                    return f
            return lst[0]
        return None

    # ---- calls ------------------------------------------------------------------------------------------------------------
    def check_put(self, slots, n_blocks, what="put"):
        """Runs for the videos of one call: slots (distinct) and the block count of each.  A slot that has a run of that many
        blocks keeps it; any other run of a named slot is freed first -- its blocks may serve the call -- and the videos are
        placed in call order.  Returns (runs, clears): runs[i] = (first, nb) of slots[i], clears = the freed (first, nb) runs.
        Nothing changes; ValueError when a video finds no room."""
        n_blocks = [int(n) for n in n_blocks]
        if len(n_blocks) != len(slots) or len(set(slots)) != len(slots):
            raise ValueError("%s: %d block counts for %d distinct slots" % (what, len(n_blocks), len(set(slots))))
        for nb in n_blocks:
            if not 1 <= nb <= 8:
                raise ValueError("%s: a run of %d blocks; a video occupies 1..8 blocks of 16 clips" % (what, nb))
        moved = [(s, self._run[s]) for s, nb in zip(slots, n_blocks) if s in self._run and self._run[s][1] != nb]
        for s, _ in moved:
            self._release(s)
        taken, runs, err = [], [], None
        for s, nb in zip(slots, n_blocks):
            if s in self._run:
                runs.append(self._run[s])
                continue
            first = self._place(nb)
            if first is None:
                err = ("%s: no room for a video of %d blocks (%d clip rows) in the packed K6 image: %d free blocks of %d, the "
                       "largest free run holds %d (tiles=%d; compact() gathers the free blocks of the tiles, the image does "
                       "not grow)"
                       % (what, nb, nb * 16, self.free_blocks, self.n_tiles * 16, self.largest_free_run(), self.n_tiles))
                # what the call asks for against what is free once its moving videos have left their runs
                asked = sum(n for s2, n in zip(slots, n_blocks) if s2 not in self._run or s2 in taken)
                free = self.free_blocks + sum(self._run[s2][1] for s2 in taken)
                break
            self._take(first, nb, s)
            taken.append(s)
            runs.append((first, nb))
        for s in reversed(taken):                                 # back to the state before the call
            self._release(s)
        for s, (first, nb) in reversed(moved):
            self._take(first, nb, s)
        if err is not None:
            raise NoRunError(err, asked, free)
        return runs, [r for _, r in moved]

    def commit_put(self, slots, runs):
        for s, r in zip(slots, runs):
            if s in self._run and self._run[s] != r:
                self._release(s)
        for s, (first, nb) in zip(slots, runs):
            if s not in self._run:
                self._take(first, nb, s)

    def check_remove(self, slots):
        """The runs of the slots (each must have one)."""
        for s in slots:
            if s not in self._run:
                raise ValueError("remove: slot %d has no run in the packed K6 image" % s)
        return [self._run[s] for s in slots]

    def commit_remove(self, slots):
        for s in slots:
            self._release(s)

    # ---- compaction ---------------------------------------------------------------------------------
    def check_compact(self):
        """A plan that makes the free blocks of every partial tile one run at its end and empties the tiles whose videos fit
        into the ends of others; changes nothing.  The plan is a list of ROUNDS, each a dict
          records  one [tile, src[0..15]] per touched tile: the operand of ONE xml_index_move_blocks_packed launch
                   (src >= 0: the block received, -1: stays, -2: becomes unused); its launch contract holds
          clears   the (first, nb) runs vacated in OTHER tiles: ONE xml_index_clear_rows_packed launch (slot -1) behind it
          moves    {slot: ((first, nb) before, (first, nb) after)} of the round, for commit_compact
        Policy per round (deterministic).  Donors: the partial tiles in order of fewest used blocks, ties to the highest tile;
        all runs of a tile, largest first (ties: lowest slot), are placed tentatively into the space other partial tiles have
        at their END once slid -- best fit: the smallest such tail that holds the run, ties to the lowest tile; never into an
        empty tile, a donor or the tile itself; if every run fits the tile is a donor and the moves are taken, else none of
        them.  A receiver is never a donor of the same round.  Slide: every other partial tile whose runs are not packed at
        its start gets them slid left in block order, received runs behind them; one record per touched tile, none for a
        donor (its blocks are sources).  Rounds repeat on the resulting state until one finds no donor and nothing to slide;
        a round with a donor empties a tile and nothing is ever placed into an empty tile, so this ends.  An empty plan is []."""
        tiles = {}                                                # tile -> [(first, nb, slot)] in block order
        for slot, (first, nb) in self._run.items():
            tiles.setdefault(first >> 4, []).append((first, nb, slot))
        for runs in tiles.values():
            runs.sort()
        plan = []
        while True:
            used = {t: sum(nb for _, nb, _ in runs) for t, runs in tiles.items()}
            partial = [t for t in tiles if 0 < used[t] < 16]
            tail = {t: 16 - used[t] for t in partial}             # free blocks at the end of a tile once it is slid
            donors, received = set(), {}                          # received: tile -> [(first, nb, slot)] in order of placement
            by_size = [[] for _ in range(16)]                     # tail length -> sorted tiles that have it (0: no target)
            for t in sorted(partial):
                by_size[tail[t]].append(t)

            def resize(u, size):                                  # tile u's tail is `size` blocks from now on
                del by_size[tail[u]][bisect.bisect_left(by_size[tail[u]], u)]
                bisect.insort(by_size[size], u)
                tail[u] = size

            for t in sorted(partial, key=lambda t: (used[t], -t)):
                if t in received:
                    continue
                own = tail[t]
                resize(t, 0)                                      # not a target of its own runs; of nobody's once a donor
                got = []
                for first, nb, slot in sorted(tiles[t], key=lambda r: (-r[1], r[2])):
                    size = next((n for n in range(nb, 16) if by_size[n]), None)      # best fit, then the lowest tile
                    if size is None:
                        break
                    u = by_size[size][0]
                    resize(u, size - nb)
                    got.append((u, (first, nb, slot)))
                if len(got) < len(tiles[t]):                      # not all of it fits: nothing of it is taken
                    for u, (_, nb, _) in reversed(got):
                        resize(u, tail[u] + nb)
                    resize(t, own)
                    continue
                donors.add(t)
                for u, run in got:
                    received.setdefault(u, []).append(run)
            records, moves = [], {}
            for t in sorted(partial):
                if t in donors:
                    continue
                src, at = [-1] * 16, 0
                for first, nb, slot in tiles[t] + received.get(t, []):
                    new = t * 16 + at
                    if new != first:
                        src[at:at + nb] = range(first, first + nb)
                        moves[slot] = ((first, nb), (new, nb))
                    at += nb
                if all(s == -1 for s in src):
                    continue                                      # packed at its start already, and receives nothing
                for b in range(at, 16):                           # blocks of its own runs behind the new end: unused now
                    if self._owner_in(tiles[t], t * 16 + b):
                        src[b] = -2
                records.append([t] + src)
            if not records:
                break
            clears = [(first, nb) for t in sorted(donors) for first, nb, _ in tiles[t]]
            plan.append(dict(records=records, clears=clears, moves=moves))
            for t in donors:
                del tiles[t]
            for t in list(tiles):
                if 0 < used[t] < 16:
                    at, out = 0, []
                    for first, nb, slot in tiles[t] + received.get(t, []):
                        out.append((t * 16 + at, nb, slot))
                        at += nb
                    tiles[t] = out
        return plan

    @staticmethod
    def _owner_in(runs, block):
        return any(first <= block < first + nb for first, nb, _ in runs)

    def commit_compact(self, plan):
        """Apply what check_compact returned (the table must be the one it was computed on)."""
        for rnd in plan:
            moves = rnd["moves"]
            for slot, (old, _) in moves.items():
                if self._run.get(slot) != old:
                    raise ValueError("commit_compact: the table changed since check_compact (slot %d)" % slot)
            for slot in moves:
                self._release(slot)
            for slot, (_, (first, nb)) in moves.items():
                self._take(first, nb, slot)
            self.compactions += bool(moves)


class _TablePlan(object):
    """What ops.q2c_scores_fused and ops.TiledRows.to_rows ask of a PackPlan, for the packed image of a MutableCorpusIndex:
    slot_ids = the device code table the update kernels maintain, n_tiles and n_videos fixed; row_map is made from the
    host BlockTable when somebody asks (to_rows: tests)."""

    def __init__(self, blocks, codes, n_videos):
        self.blocks, self.slot_ids, self.n_tiles, self.n_videos = blocks, codes, blocks.n_tiles, int(n_videos)

    @property
    def row_map(self):
        return self.blocks.row_map().to(self.slot_ids.device)


class MutableCorpusIndex(CorpusIndex):
    """A CorpusIndex of `capacity` video slots whose rows are rewritten on the stream (module docstring).  Besides the
    CorpusIndex fields:
      live       (1, ceil(capacity / 32)) int32 device, bit s = slot s holds a video; never re-allocated
      slot_ids   (capacity,) int32 device, slot -> the caller's id: the meta2vid of a search that passes none
      mask_bits  {modality: (capacity, 4) int32}: K6's mask-bit operand (on the tiled layout also feat1n[m].mask_bits)
      n_live     host counter; table: the SlotTable
      version    host counter, raised by every committed add / put / replace / remove (not by compact(), which moves blocks
                 but changes no video): what a subset view (inference.video_subset) compares to know its copies are current
    n_videos == capacity: the kernels run over all slots.

    The packed form, create(..., tiles=N) (addendum): the K6 operand is the packed image of
    xml_q2c_scores_packed over N tiles of 256 rows instead of capacity / 2, every video in a run of ceil(len / 16) blocks of
    16 rows -- K6's time follows N, not capacity.  Then
      blocks     the BlockTable: which run each live slot owns
      codes      (2 N, 8) int32 device, K6's per-block code table (feat1n[m].plan.slot_ids); a video's code is its SLOT
      mask_bits  {modality: (2 N, 4) int32}: the packed mask words (= feat1n[m].mask_bits)
    feat2, mask, vlen, slot_ids and live stay per slot.  K6 then writes the score columns of the LIVE slots only: the columns
    of free slots of stage_q2c's matrix (vcmr_search's out["q2c"]) are unspecified -- every search tests the live / allow bit
    before the value (topk.hip); explain_moments' q2c of a pair that names a free slot is unspecified too.
    Updates take the videos' valid lengths (last valid clip + 1 over the modalities) as n_clips=; without it they are read
    from the masks with one small device -> host copy, the one synchronising path of an update.  Given up, beyond what the
    plain form gives up: `tiles` does not grow (an update that finds no run is refused; compact() -- or auto_compact=True -- makes the free blocks
    of the tiles contiguous first), K6 costs N tiles whatever the occupancy.

    Long videos, create(..., part_overlap=O): a video of more than l_ref clips is stored as the
    overlapping parts of ingest.plan_parts(n_clips, l_ref, overlap=O), one slot (and, packed, one run) per part; then
      chain_head / chain_next / chain_offset  (capacity,) int32 device: slot -> the slot of its video's first part, the slot
                 of the next part (-1), the part's first clip in the video; a free slot and a one-part video: (itself, -1, 0)
      table      a ChainTable; n_videos_live counts videos, n_live slots
    A video is numbered by its HEAD slot: add(..., parts=) returns it, slot_of(id) gives it, a caller's video_allow bit for
    the video is the head's bit, out["top_videos"] lists it.  Chains are added, replaced and removed whole.

    Exact-rank mode, create(..., exact_rank=True) with an f32 or ops.F16S model: feat1n[m] is the bf16
    FILTER image (tiled where ops.q2c_tiled_ok takes bf16 rows of that width, else row-major), feat2[m] f32 rows or
    ops.SplitRows, and `exact` an inference.ExactFilter whose feat1n_f32[m] are the (capacity, lpad, H) re-score rows (f32 or
    SplitRows), err_rows[m] the (capacity, lpad) rounding-error norm of every stored row and e_c_dev the (n_mod,) running
    bound on the device: every put raises it (ops.index_put_rows_exact, one launch for all operands of the slots), the
    certificate of a search reads it through a pointer.  remove leaves it alone -- a bound that is too large only sends more
    queries to the second tier --; tighten_error_bound() recomputes it over the live slots.  Searches run the exact-rank
    chains of inference under `live AND video_allow`; a GraphedVcmrSearch (ops.F16S model) stays valid across updates.
    create(..., exact_rank=True, filter_tiles=N): the bf16 filter image ALONE is the packed image over
    N tiles, with blocks / codes / mask_bits as in the packed form (ops.index_put_rows_packed_exact: the filter rows, codes
    and mask words of a video go to its run, everything else to its slot, one launch); re-score rows, feat2, err_rows and the
    bound are those of the plain exact-rank index bit for bit, mask and vlen follow the effective mask of the packed form.
    n_clips=, compact() and auto_compact work as there; the filter then costs N tiles, not capacity / 2.
    create(..., exact_rank=True, exact_part_overlap=O) (with or without filter_tiles=N): long videos on
    an exact-rank index -- chains of slots with everything part_overlap=O gives (parts=, the ChainTable, chain_head /
    chain_next / chain_offset, videos numbered by their head slot, added, replaced and removed whole).  Every part is an
    ordinary exact-rank slot to the put kernels; a search folds the parts of a video on its re-scored candidate lists
    (ops.cand_best_part) and returns the f32 path's lists of VIDEOS, each ranked by its best part."""

    def __init__(self, *a, **kw):
        raise TypeError("use MutableCorpusIndex.create(model, capacity) or MutableCorpusIndex.from_batches(...)")

    @classmethod
    def create(cls, model, capacity, l_ref=None, exact_filter=False, parts=None, video_offset=0, n_total=None, tiles=None,
               auto_compact=False, part_overlap=None, max_parts=32, exact_rank=False, filter_tiles=None,
               exact_part_overlap=None):
        """An empty index (all slots free) for `capacity` videos of up to l_ref clips (default model.config.max_ctx_l).
        tiles=None: the plain K6 image, two slots per tile; tiles=N: the packed image over N tiles (class docstring).
        auto_compact (the packed form): an add / put / replace that finds no run although enough blocks are free runs
        compact() once and tries again.
        part_overlap=O (None: off, nothing changes): videos longer than l_ref clips are taken as CHAINS of slots (class
        docstring), cut by ingest.plan_parts(n_clips, l_ref, overlap=O); max_parts bounds the parts of one video.
        exact_rank=True (an f32 or ops.F16S model; tiles=None, no part_overlap -- exact_part_overlap instead): exact-rank mode
        (class docstring) -- the index holds the bf16 filter image, the f32-grade re-score rows and the running error bound, and searches return the
        f32 path's lists.
        filter_tiles=N (with exact_rank=True only): the bf16 FILTER image alone is the packed image over N tiles -- re-score
        rows, feat2 and error norms stay per slot --; updates then take n_clips=, compact() and auto_compact work as in the
        packed form (class docstring).
        exact_part_overlap=O (with exact_rank=True only, with or without filter_tiles=N): what part_overlap=O is on an index
        without exact-rank mode -- long videos as chains of slots, max_parts parts at the most; searches fold the parts of
        a video on their re-scored candidate lists (class docstring)."""
        dt = getattr(model, "compute_dtype", torch.float32)
        if exact_part_overlap is not None:
            cls._check_exact_part_overlap(model, exact_part_overlap, exact_rank, tiles, part_overlap, l_ref)
        if filter_tiles is not None:
            cls._check_filter_tiles(filter_tiles, exact_rank, tiles, part_overlap)
        if exact_filter or (dt is hip_ops.F16S and not exact_rank):
            raise ValueError("MutableCorpusIndex: no exact-rank mode (an ops.F16S model / exact_filter=True) -- its certificate "
                             "rests on e_c, a bound over the WHOLE corpus that a one-video update cannot maintain by value; "
                             "create(..., exact_rank=True) keeps that bound on the device instead")
        if exact_rank:
            cls._check_exact_rank(model, dt, l_ref, tiles, part_overlap, filter_tiles)
        if parts is not None:
            raise ValueError("MutableCorpusIndex: no parts table -- the fold of parts into videos is planned for a fixed corpus")
        if video_offset or n_total is not None:
            raise ValueError("MutableCorpusIndex: not a corpus shard (video_offset / n_total): the sharded drivers number "
                             "videos by position in a fixed global corpus")
        l_ref = int(model.config.max_ctx_l if l_ref is None else l_ref)
        if l_ref <= 0:
            raise ValueError("MutableCorpusIndex: l_ref must be positive, got %d" % l_ref)
        if exact_part_overlap is not None:       # (validated above, with exact_rank=True)
            table = ChainTable(capacity, max_parts)
        elif part_overlap is None:
            table = SlotTable(capacity)
        else:
            if isinstance(part_overlap, bool) or int(part_overlap) != part_overlap or not 0 <= int(part_overlap) < l_ref:
                raise ValueError("MutableCorpusIndex: part_overlap must be a number of clips in [0, l_ref = %d), got %r"
                                 % (l_ref, part_overlap))
            table = ChainTable(capacity, max_parts)
        act = getattr(model, "act_dtype", hip_ops.act_dtype(dt))
        h = int(model.config.hidden_size)
        lpad = index_lpad(l_ref, model, hip_ops)
        if act not in (torch.float32, torch.bfloat16) or lpad > 128 or \
                not _lib.load().xml_q2c_tile_rows_l2norm_ok(h, hip_ops.dt_of(act)):
            raise ValueError("MutableCorpusIndex: xml_index_put_rows takes f32 / bf16 rows of up to 128 clips and a hidden size "
                             "of whole 64-byte slices; got %s, lpad %d, hidden %d" % (act, lpad, h))
        blocks = None
        if tiles is not None:
            if isinstance(tiles, bool) or int(tiles) != tiles or int(tiles) <= 0:
                raise ValueError("MutableCorpusIndex: tiles must be a positive number of 256-row tiles, got %r" % (tiles,))
            if lpad != 128 or not hip_ops.q2c_tiled_ok(lpad, h, act):
                raise ValueError("MutableCorpusIndex: the packed form (tiles=%d) needs the tiled K6 operand -- 128-clip slots and "
                                 "f32 / bf16 rows the tiled kernel takes; got %s, lpad %d, hidden %d.  Use tiles=None"
                                 % (tiles, act, lpad, h))
            blocks = BlockTable(tiles)
        dev = next(model.parameters()).device
        mods = [n for n, u in (("video", model.use_video), ("sub", model.use_sub)) if u]
        cap = table.capacity
        self = object.__new__(cls)
        if exact_rank:
            self._init_exact(model, table, mods, l_ref, lpad, h, dev, filter_tiles, auto_compact)
            if exact_part_overlap is not None:
                self._init_chains(int(exact_part_overlap), table, dev)
            return self
        feat2 = {m: torch.zeros((cap, lpad, h), dtype=act, device=dev) for m in mods}
        mask = {m: torch.zeros((cap, lpad), dtype=torch.float32, device=dev) for m in mods}
        self.blocks, self.codes, self.auto_compact = blocks, None, bool(auto_compact) and blocks is not None
        n_words = cap if blocks is None else 2 * blocks.n_tiles
        self.mask_bits = {m: torch.zeros((n_words, 4), dtype=torch.int32, device=dev) for m in mods}
        plan = None
        if blocks is not None:                          # the packed image: every block unused, K6 skips all of them
            self.codes = torch.full((2 * blocks.n_tiles, 8), -2, dtype=torch.int32, device=dev)
            plan = _TablePlan(blocks, self.codes, cap)
        feat1n = {m: self._alloc_k6_image(m, (cap, lpad, h), act, dev, plan) for m in mods}
        CorpusIndex.__init__(self, mods, feat1n, feat2, mask, l_ref)
        self._init_slot_state(model, table, l_ref, dev)
        if part_overlap is not None:
            self._init_chains(int(part_overlap), table, dev)
        return self

    def _init_chains(self, overlap, table, dev):
        """The chain tables of an index that holds long videos: every slot in the single state -- an add of short videos
        never touches these."""
        cap = table.capacity
        self.part_overlap, self.max_parts = overlap, table.max_parts
        self.chain_head = torch.arange(cap, dtype=torch.int32, device=dev)
        self.chain_next = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.chain_offset = torch.zeros((cap,), dtype=torch.int32, device=dev)
        self.fold = _inference.ChainFold(self)

    def _alloc_k6_image(self, m, shape, dtype, dev, plan=None):
        """The zero-filled K6 operand of modality m for (capacity, lpad, H) rows of `dtype`: the packed image of `plan` (a
        _TablePlan), else the plain two-slots-per-tile image where the tiled kernel takes the rows (K6 in mask-bit mode,
        always), else row-major."""
        cap, lpad, h = shape
        if plan is None and not hip_ops.q2c_tiled_ok(lpad, h, dtype):
            return torch.zeros(shape, dtype=dtype, device=dev)
        rows = cap * lpad if plan is None else plan.n_tiles * 256
        data = torch.zeros(hip_ops.q2c_tiled_numel(rows, h, dtype), dtype=dtype, device=dev)
        image = hip_ops.TiledRows(data, cap * lpad, h, shape, all_valid=False)
        image.mask_bits = self.mask_bits[m]
        if plan is not None:
            image.plan = plan
        return image

    @staticmethod
    def _check_exact_part_overlap(model, overlap, exact_rank, tiles, part_overlap, l_ref):
        """What create(..., exact_part_overlap=O) refuses about the keyword itself, before any device allocation."""
        if not exact_rank:
            raise ValueError("MutableCorpusIndex: exact_part_overlap=%r without exact_rank=True -- it is the chains of slots of "
                             "exact-rank mode; an index without that mode takes long videos with part_overlap=O" % (overlap,))
        if tiles is not None or part_overlap is not None:
            raise ValueError("MutableCorpusIndex: exact_part_overlap=%r together with %s -- exact-rank mode (exact_rank=True) "
                             "packs its filter image alone (filter_tiles=N, tiles=None), and its chains are asked for with "
                             "exact_part_overlap= alone" % (overlap, "tiles=" if tiles is not None else "part_overlap="))
        l_ref = int(model.config.max_ctx_l if l_ref is None else l_ref)
        if isinstance(overlap, bool) or int(overlap) != overlap or not 0 <= int(overlap) < l_ref:
            raise ValueError("MutableCorpusIndex: exact_part_overlap must be a number of clips in [0, l_ref = %d), got %r"
                             % (l_ref, overlap))

    @staticmethod
    def _check_filter_tiles(filter_tiles, exact_rank, tiles, part_overlap):
        """What create(..., filter_tiles=N) refuses about the keyword itself, before any device allocation."""
        if not exact_rank:
            raise ValueError("MutableCorpusIndex: filter_tiles=%r without exact_rank=True -- it packs the bf16 FILTER image of "
                             "exact-rank mode; an index without that mode packs its K6 image with tiles=N" % (filter_tiles,))
        if tiles is not None or part_overlap is not None:
            raise ValueError("MutableCorpusIndex: filter_tiles=%r together with %s -- exact-rank mode (exact_rank=True) keeps "
                             "re-score rows and error norms per slot and packs the filter image alone (tiles=None), and its "
                             "chains of slots are asked for with exact_part_overlap=O"
                             % (filter_tiles, "tiles=" if tiles is not None else "part_overlap="))
        if isinstance(filter_tiles, bool) or int(filter_tiles) != filter_tiles or int(filter_tiles) <= 0:
            raise ValueError("MutableCorpusIndex: filter_tiles must be a positive integer number of 256-row tiles, got %r"
                             % (filter_tiles,))

    @staticmethod
    def _check_exact_rank(model, dt, l_ref, tiles, part_overlap, filter_tiles=None):
        """What create(..., exact_rank=True) refuses, before any device allocation."""
        if tiles is not None:
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True) on the packed K6 image (tiles=%r) is not "
                             "built -- the filter image, the re-score rows and the error norms are kept per slot; use "
                             "tiles=None (filter_tiles=N packs the filter image alone)" % (tiles,))
        if part_overlap is not None:
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True) and part_overlap= exclude each other -- "
                             "exact-rank mode never forms the f32 (Nq, slots) score matrix that the best part of a video is "
                             "taken from; exact_part_overlap=O holds long videos as chains of slots there, folded on the "
                             "re-scored candidate lists")
        if dt is not hip_ops.F16S and dt != torch.float32:
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True) needs f32 activations (XML(cfg, "
                             "compute_dtype=torch.float32 or ops.F16S)); got a %s model" % (dt,))
        mode = _inference.exact_mode_of(model)
        if mode == "f16s" and _inference.EXACT_F16S_FILTER != "bf16":
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True) builds the bf16 filter image only; "
                             "inference.EXACT_F16S_FILTER is %r" % (_inference.EXACT_F16S_FILTER,))
        h = int(model.config.hidden_size)
        lpad = index_lpad(int(model.config.max_ctx_l if l_ref is None else l_ref), model, hip_ops)
        if lpad > 128 or not _lib.load().xml_q2c_tile_rows_l2norm_ok(h, _lib.XML_F32) or (mode == "f16s" and h % 32):
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True): xml_index_put_rows_exact takes f32 rows of up "
                             "to 128 clips and a hidden size of whole 64-byte slices (a multiple of 32 for an ops.F16S "
                             "model); got lpad %d, hidden %d" % (lpad, h))
        if filter_tiles is not None and (lpad != 128 or not hip_ops.q2c_tiled_ok(128, h, torch.bfloat16)):
            raise ValueError("MutableCorpusIndex: exact-rank mode (exact_rank=True) with the packed filter image "
                             "(filter_tiles=%d) needs the tiled bf16 K6 operand -- 128-clip slots and bf16 rows the tiled "
                             "kernel takes; got lpad %d, hidden %d.  Use filter_tiles=None" % (filter_tiles, lpad, h))

    def _init_exact(self, model, table, mods, l_ref, lpad, h, dev, filter_tiles=None, auto_compact=False):
        """The tensors of an exact-rank index (create(..., exact_rank=True)): allocated once, zero-filled.  filter_tiles=N:
        the filter image is the packed one, with the BlockTable, the code table and the packed mask words of the packed
        form; everything else stays per slot."""
        cap = table.capacity
        blocks = None if filter_tiles is None else BlockTable(filter_tiles)
        mode = _inference.exact_mode_of(model)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)         # noqa: E731

        def rows():          # f32-grade rows: f32, or split-f16 data + one inv_scale per row
            if mode == "f16s":
                return hip_ops.SplitRows(torch.zeros((cap, lpad, h), dtype=torch.int32, device=dev), f32(cap, lpad))
            return f32(cap, lpad, h)
        feat2 = {m: rows() for m in mods}
        mask = {m: f32(cap, lpad) for m in mods}
        self.blocks, self.codes, self.auto_compact = blocks, None, bool(auto_compact) and blocks is not None
        n_words = cap if blocks is None else 2 * blocks.n_tiles
        self.mask_bits = {m: torch.zeros((n_words, 4), dtype=torch.int32, device=dev) for m in mods}
        plan = None
        if blocks is not None:                          # the packed filter image: every block unused
            self.codes = torch.full((2 * blocks.n_tiles, 8), -2, dtype=torch.int32, device=dev)
            plan = _TablePlan(blocks, self.codes, cap)
        # the bf16 FILTER image: packed, else in the layout create chooses for bf16 rows of this width
        feat1n = {m: self._alloc_k6_image(m, (cap, lpad, h), torch.bfloat16, dev, plan) for m in mods}
        CorpusIndex.__init__(self, mods, feat1n, feat2, mask, l_ref)
        cells = f32(len(mods))
        self.exact = _inference.ExactFilter({m: rows() for m in mods}, _inference._DeviceBound(cells, mods), n_candidates=256,
                                            mode=mode)
        self.exact.e_c_dev, self.exact.err_rows = cells, {m: f32(cap, lpad) for m in mods}
        self._init_slot_state(model, table, l_ref, dev)
        return self

    def _init_slot_state(self, model, table, l_ref, dev):
        """The per-slot state every form of the index has: every slot free."""
        cap = table.capacity
        self.raw_feat1 = {}
        self.vlen = torch.full((cap,), l_ref, dtype=torch.int32, device=dev)
        self.ragged = True                   # K7 / K9 always take vlen: the launch shape does not depend on the data
        self.live = torch.zeros((1, (cap + 31) // 32), dtype=torch.int32, device=dev)
        self.slot_ids = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.table = table
        self.model = model
        self.version = 0

    def tighten_error_bound(self):
        """An exact-rank index: recompute the running bound e_c_dev as the maximum of err_rows over the LIVE slots (one launch,
        nothing read back).  After removals the bound may be larger than the live rows need -- still valid, it only sends
        more queries to the second tier -- and this makes it tight again."""
        if self.exact is None:
            raise ValueError("tighten_error_bound: not an exact-rank index (MutableCorpusIndex.create(..., exact_rank=True))")
        hip_ops.index_exact_bound([self.exact.err_rows[m] for m in self.modalities], self.live.view(-1), self.exact.e_c_dev)
        return self

    @classmethod
    def from_batches(cls, model, context_batches, capacity, l_ref=None, ids=None, n_clips=None, parts=None, **kw):
        """create + one add per (video_feat, video_mask, sub_feat, sub_mask) batch; ids: the videos' ids, in order; n_clips:
        their valid lengths, in order (the packed form, tiles=N; None: read from the masks, one host read per batch).
        parts (an index created with part_overlap=): the ingest.PartTable of the batch, or a list of them, one per batch --
        the batch rows are then parts, ids one per SOURCE video, n_clips one per part."""
        self = cls.create(model, capacity, l_ref, **kw)
        ids = None if ids is None else _int_list(ids, "ids")
        n_clips = None if n_clips is None else _int_list(n_clips, "n_clips")
        tables = None if parts is None else (list(parts) if isinstance(parts, (list, tuple)) else [parts])
        r = v = 0
        for i, (vf, vm, sf, sm) in enumerate(context_batches):
            b = int((vf if vf is not None else sf).shape[0])
            kw_add, nv = {}, b
            if tables is not None:
                if i >= len(tables):
                    raise ValueError("from_batches: %d part tables for more batches (parts= takes one table per batch)" % len(tables))
                kw_add, nv = dict(parts=tables[i]), int(tables[i].n_videos)
            self.add(vf, vm, sf, sm, ids=None if ids is None else ids[v:v + nv], n_clips=None if n_clips is None else n_clips[r:r + b],
                     **kw_add)
            r += b
            v += nv
        return self

    capacity = property(lambda self: self.table.capacity)
    n_live = property(lambda self: self.table.n_live)
    n_videos_live = property(lambda self: getattr(self.table, "n_videos_live", self.table.n_live))

    def set_valid_lengths(self):
        return self                           # vlen is maintained per slot by the update kernels; ragged stays True

    def slot_of(self, vid):
        return self.table.slot_of(vid)

    def hbm_bytes(self):
        extra = list(self.mask_bits.values()) + [self.vlen, self.live, self.slot_ids] + ([] if self.codes is None else [self.codes])
        if self.chain_head is not None:
            extra += [self.chain_head, self.chain_next, self.chain_offset]
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

    @staticmethod
    def _valid_lengths(masks):
        """(last valid clip + 1) over the modalities' (b, lb) masks as host integers: one small device -> host copy that waits
        for the stream -- the one synchronising path of an update (pass n_clips= to avoid it)."""
        pos = None
        for mk in masks:
            last = ((mk != 0).to(torch.int32) * torch.arange(1, mk.shape[1] + 1, device=mk.device, dtype=torch.int32)).amax(1)
            pos = last if pos is None else torch.maximum(pos, last)
        return pos.cpu().tolist()

    @staticmethod
    def _n_blocks(n_clips, b, what):
        """Blocks per video of a batch in the packed image from its valid lengths (host integers)."""
        n_clips = _int_list(n_clips, what + ": n_clips")
        if len(n_clips) != b:
            raise ValueError("%s: %d valid lengths (n_clips) for %d videos" % (what, len(n_clips), b))
        try:
            return [blocks_of(n) for n in n_clips]
        except ValueError as e:
            raise ValueError("%s: %s" % (what, e))

    def put(self, slots, enc, ids=None, n_clips=None):
        """Write an ENCODED batch, enc[m] = (feat1, feat2, mask) of (b, lb <= l_ref) rows as model.encode_context returns them,
        into the b distinct slots; a live slot is replaced, a free one becomes live.  ids=None keeps / assigns ids as
        SlotTable.check_put says.  n_clips (the packed form; ignored by the plain one): the videos' valid lengths, class
        docstring -- a mask that is longer than its n_clips rounded up to whole blocks is cut there.  Returns the slots.
        (An index with chains: videos of one part only; a slot of a longer video is refused.)"""
        slots, ids = self.table.check_put(slots, ids)
        self._check_enc(slots, enc)
        nbs = runs = clears = None
        if self.blocks is not None:
            nbs = self._n_blocks(self._valid_lengths([enc[m][2] for m in self.modalities]) if n_clips is None else n_clips,
                                 len(slots), "put")
            runs, clears = self._find_runs(slots, nbs, "put")
        self._launch_put(slots, ids, enc, nbs, runs, clears)
        self.table.commit_put(slots, ids)
        self.version += 1
        return slots

    def _check_enc(self, slots, enc):
        """Everything a put launch could refuse about an encoded batch, before anything is enqueued."""
        mods = self.modalities
        if set(enc) != set(mods):
            raise ValueError("put: the batch holds modalities %s, the index %s" % (sorted(enc), mods))
        for m in mods:
            a1, a2, am = enc[m]
            if a1.shape[0] != len(slots) or a1.shape[1] > self.l_ref:
                raise ValueError("put: %d slots and l_ref = %d for a batch of shape %s" % (len(slots), self.l_ref, tuple(a1.shape)))
        if self.blocks is not None or self.exact is not None:
            b = len(slots)
            for m in mods:      # everything the put launch could refuse, before the clear launch of the moving videos
                a1, a2, am = enc[m]
                want = (b, a1.shape[1], self.feat2[m].shape[2])
                want_dt = torch.float32 if self.exact is not None else self.feat2[m].dtype
                if not (a1.is_cuda and a2.is_cuda and am.is_cuda) or a1.dtype != want_dt or a2.dtype != a1.dtype or \
                        tuple(a1.shape) != want or tuple(a2.shape) != want or tuple(am.shape) != want[:2]:
                    raise ValueError("put: %s rows (b, lb, %d) of %s on the device and a (b, lb) mask expected"
                                     % (m, want[2], want_dt))

    def _launch_put(self, slots, ids, enc, nbs, runs, clears):
        """The launches of a validated put (the packed form: with the runs _find_runs returned, committed to the BlockTable
        here); the slot table is the caller's to commit."""
        b = len(slots)
        batch = [[enc[m][k].contiguous() for m in self.modalities] for k in (0, 1)] + \
            [[enc[m][2].float().contiguous() for m in self.modalities]]
        if self.blocks is not None:
            if clears:     # videos that move: their old runs become unused blocks BEFORE the put, whose runs may reuse them
                self._clear([-1] * len(clears), clears)
            rec = self._to_device(slots + ids + [x for r in runs for x in r])
            records = (rec[:b], rec[b:2 * b], rec[2 * b:].view(b, 2), max(nbs))
            if self.exact is not None:     # the packed FILTER image: its runs and every per-slot operand, one launch
                ex = self.exact
                hip_ops.index_put_rows_packed_exact(*batch, *records,
                                                    *self._sides(self.feat1n, ex.feat1n_f32, self.feat2, ex.err_rows, self.mask,
                                                                 self.mask_bits),
                                                    self.codes, ex.e_c_dev, self.vlen, self.slot_ids, self.live.view(-1),
                                                    self.l_ref)
            else:
                hip_ops.index_put_rows_packed(*batch, *records,
                                              *self._sides(self.feat1n, self.feat2, self.mask, self.mask_bits), self.codes,
                                              self.vlen, self.slot_ids, self.live.view(-1), self.l_ref)
            self.blocks.commit_put(slots, runs)
            return
        both = self._to_device([slots, ids])
        if self.exact is not None:     # every operand of the slots and the running bound, one launch
            ex = self.exact
            hip_ops.index_put_rows_exact(*batch, both[0], both[1],
                                         *self._sides(self.feat1n, ex.feat1n_f32, self.feat2, ex.err_rows, self.mask,
                                                      self.mask_bits),
                                         ex.e_c_dev, self.vlen, self.slot_ids, self.live.view(-1), self.l_ref)
            return
        hip_ops.index_put_rows(*batch, both[0], both[1], *self._sides(self.feat1n, self.feat2, self.mask, self.mask_bits),
                               self.vlen, self.slot_ids, self.live.view(-1), self.l_ref)

    def _sides(self, *tensors):
        """Per-modality dicts -> the per-modality lists the ops entries take."""
        return [[t[m] for m in self.modalities] for t in tensors]

    def _clear(self, slots, runs=None):
        """One clear launch over host lists: the plain entry frees `slots`; the packed one takes (slot, run) records -- a run
        becomes unused blocks, its slot is freed unless it is -1.  `slots` may be a device tensor already (then runs is too)."""
        if not torch.is_tensor(slots):
            slots, runs = self._to_device(slots), None if runs is None else self._to_device(runs)
        state = (self.vlen, self.live.view(-1), self.l_ref)
        if self.blocks is None:
            hip_ops.index_clear_rows(slots, *self._sides(self.mask, self.mask_bits), *state)
        else:
            hip_ops.index_clear_rows_packed(slots, runs, 8, *self._sides(self.mask, self.mask_bits), self.codes, *state)

    def _room(self, slots, masks, n_clips, b, what):
        """The packed form: refuse a batch that finds no runs BEFORE it is encoded; returns n_clips for put (the lengths read
        from the masks, so that they are read once)."""
        if self.blocks is None:
            return None
        if n_clips is None:
            n_clips = self._valid_lengths([mk for m, mk in zip(("video", "sub"), masks) if m in self.modalities])
        self._find_runs(slots, self._n_blocks(n_clips, b, what), what)
        return n_clips

    def _find_runs(self, slots, n_blocks, what, freed=()):
        """BlockTable.check_put; with auto_compact a refusal for lack of a RUN while enough blocks are free is answered by one
        compact() and one more try.  freed: slots the same call frees first (the surplus parts of a replaced chain) -- their
        runs count as room; the table is back in its state when this returns."""
        def attempt():
            gone = self.blocks.check_remove(freed) if freed else []
            self.blocks.commit_remove(freed)
            try:
                return self.blocks.check_put(slots, n_blocks, what)
            finally:
                for s, (first, nb) in reversed(list(zip(freed, gone))):
                    self.blocks._take(first, nb, s)
        try:
            return attempt()
        except NoRunError as e:
            if not self.auto_compact or e.blocks_free < e.blocks_asked:
                raise
        self.compact()
        try:
            return attempt()
        except NoRunError as e:
            raise NoRunError(str(e) + " after compaction", e.blocks_asked, e.blocks_free)

    def compact(self):
        """The packed form: move runs inside the image so that the free blocks of every partial tile are one run at its end,
        and empty the tiles whose videos fit into the ends of others (BlockTable.check_compact).  Per
        round one xml_index_move_blocks_packed launch and, when runs crossed tiles, one xml_index_clear_rows_packed launch
        (slot -1) over the vacated runs, on the current stream; nothing is read back, no tensor is re-allocated, slots keep
        their numbers, n_tiles and every pointer stay -- a captured GraphedVcmrSearch stays valid.  Returns what was done."""
        if self.blocks is None:
            raise ValueError("compact: the plain form (tiles=None) has nothing to compact -- every slot owns its 128 rows; "
                             "only the packed form (create(..., tiles=N)) hands out runs of blocks")
        mods = self.modalities
        before = self.blocks.stats()
        plan = self.blocks.check_compact()
        for rnd in plan:
            recs, clears = rnd["records"], rnd["clears"]
            flat = [x for r in recs for x in r] + [-1] * len(clears) + [x for r in clears for x in r]
            dev = self._to_device(flat)
            n, c = 17 * len(recs), len(clears)
            records, runs = dev[:n].view(-1, 17), dev[n + c:].view(c, 2)
            # an entry takes 65535 records; a part of a launch that keeps the contract keeps it too (tiles are independent,
            # cross-tile sources lie in donor tiles, which no record writes)
            for i in range(0, len(recs), 65535):
                hip_ops.index_move_blocks_packed(records[i:i + 65535], *self._sides(self.feat1n, self.mask_bits), self.codes)
            for i in range(0, c, 65535):     # the runs vacated in other tiles: until here their slots' codes stood twice
                self._clear(dev[n + i:n + min(i + 65535, c)], runs[i:i + 65535])
        self.blocks.commit_compact(plan)
        after = self.blocks.stats()
        moved = sum(nb for rnd in plan for (_, nb), _ in rnd["moves"].values())
        row_bytes = sum(self.feat1n[m].hidden * self.feat1n[m].element_size() for m in mods)      # the image's rows move
        return dict(rounds=len(plan), blocks_moved=moved, tiles_touched=len({r[0] for rnd in plan for r in rnd["records"]}),
                    tiles_emptied=after["tiles_empty"] - before["tiles_empty"],
                    largest_free_run_before=before["largest_free_run"], largest_free_run_after=after["largest_free_run"],
                    bytes_moved=moved * 16 * row_bytes)

    def add(self, video_feat, video_mask, sub_feat, sub_mask, ids=None, n_clips=None, parts=None):
        """Encode a context batch and store its videos in the lowest free slots; returns the slots (a list, batch order).
        n_clips: put.  parts (an index created with part_overlap=O): the ingest.PartTable of THIS batch,
        ingest.plan_parts(clip counts, index.l_ref, overlap=O) -- the batch rows are its parts in table order (what
        ingest.ContextFeeder(parts=table) yields), ids has one entry per source video, n_clips (default: the table's part
        lengths) one per part; returns the HEAD slots, one per video."""
        if parts is not None:
            return self._put_chains(None, video_feat, video_mask, sub_feat, sub_mask, ids, n_clips, parts, "add")
        b = self._check_batch(video_feat, video_mask, sub_feat, sub_mask, "add")
        slots, ids = self.table.check_add(b, ids)
        n_clips = self._room(slots, (video_mask, sub_mask), n_clips, b, "add")
        return self.put(slots, self.encode(video_feat, video_mask, sub_feat, sub_mask), ids, n_clips)

    def replace(self, slots, video_feat, video_mask, sub_feat, sub_mask, ids=None, new_ids=None, n_clips=None, parts=None):
        """Encode a context batch over the LIVE slots named by `slots` (or, slots=None, by ids=); the videos keep their ids
        unless new_ids gives others.  The packed form: a video whose block count does not change keeps its run, any other
        moves (its old run is freed first).  n_clips: put.  Returns the slots.
        An index created with part_overlap=: the slots name VIDEOS (by any slot of each); the old chains are freed and the new
        ones placed in one validated call -- a new video takes over its predecessor's slots in order (the head keeps its
        number), frees those it does not need and takes the lowest free slots for further parts; parts as in add (None: every
        row of the batch is a whole video).  Returns the head slots."""
        if self.chain_head is not None:
            heads = self.table.resolve_videos(slots, ids, "replace")
            return self._put_chains(heads, video_feat, video_mask, sub_feat, sub_mask, new_ids, n_clips, parts, "replace")
        if parts is not None:
            self._part_lists(parts, 0, "replace")
        slots = self.table.resolve(slots, ids, "replace")
        b = self._check_batch(video_feat, video_mask, sub_feat, sub_mask, "replace")
        if b != len(slots):
            raise ValueError("replace: %d slots for a batch of %d videos" % (len(slots), b))
        slots, new_ids = self.table.check_put(slots, new_ids, "replace")
        n_clips = self._room(slots, (video_mask, sub_mask), n_clips, b, "replace")
        return self.put(slots, self.encode(video_feat, video_mask, sub_feat, sub_mask), new_ids, n_clips)

    def remove(self, slots=None, ids=None):
        """Free the LIVE slots named by `slots` (or by ids=): searches enqueued afterwards no longer see them.  Returns them.
        The packed form frees their runs too.  An index created with part_overlap=: a video is named by any of its slots or by
        its id and its whole chain is freed (all its slots are returned); one xml_index_set_chains launch puts every freed
        slot of a longer video back into the single state."""
        plan = None
        if self.chain_head is not None:
            plan = self.table.check_remove_chains(self.table.resolve_videos(slots, ids, "remove"))
            slots = plan["slots"]
        else:
            slots = self.table.resolve(slots, ids, "remove")
        if slots:
            self._free_slots(slots)
        if plan is not None:
            self._set_chains(plan["records"])
            self.table.commit_remove_chains(plan)
        elif slots:
            self.table.commit_remove(slots)
        if slots:
            self.version += 1
        return slots

    def _free_slots(self, slots):
        """The clear launch that frees live slots; the packed form frees their runs too (BlockTable committed here)."""
        if self.blocks is None:
            return self._clear(slots)
        self._clear(slots, self.blocks.check_remove(slots))
        self.blocks.commit_remove(slots)

    # ---- long videos: chains of slots ---------------------------------------------------------------
    def _set_chains(self, records):
        if records:
            hip_ops.index_set_chains(self._to_device(records).view(-1, 4), self.chain_head, self.chain_next, self.chain_offset)

    def _part_lists(self, table, b, what):
        """A batch's part table against this index: (parts per video, their offsets per video, clips per part) as host lists.
        table=None: every row of the batch is a whole video."""
        if table is None:
            return [1] * b, [[0]] * b, None
        if self.chain_head is None:
            raise ValueError("%s: parts= on an index created without part_overlap= -- it holds videos of up to l_ref = %d clips "
                             "only (MutableCorpusIndex.create(..., part_overlap=O); in exact-rank mode exact_part_overlap=O)"
                             % (what, self.l_ref))
        for name in ("max_ctx_len", "overlap", "n_parts", "n_videos", "group_start", "part_offset", "part_len"):
            if not hasattr(table, name):
                raise ValueError("%s: parts must be the ingest.PartTable of the batch (ingest.plan_parts), got %s"
                                 % (what, type(table).__name__))
        if int(table.max_ctx_len) != self.l_ref:
            raise ValueError("%s: the part table was planned for parts of %d clips, the index holds l_ref = %d "
                             "(ingest.plan_parts(n_clips, index.l_ref, overlap=%d))"
                             % (what, table.max_ctx_len, self.l_ref, self.part_overlap))
        if int(table.overlap) != self.part_overlap:
            raise ValueError("%s: the part table overlaps its parts by %d clips, the index was created with part_overlap = %d "
                             "(searches rely on it: a moment of up to part_overlap clips lies inside one part)"
                             % (what, table.overlap, self.part_overlap))
        if int(table.n_parts) != b:
            raise ValueError("%s: the batch holds %d rows, the part table has %d parts" % (what, b, table.n_parts))
        gs, po, pl = (_int_list(t.cpu() if torch.is_tensor(t) else t, what)
                      for t in (table.group_start, table.part_offset, table.part_len))
        counts = [gs[i + 1] - gs[i] for i in range(len(gs) - 1)]
        return counts, [po[gs[i]:gs[i + 1]] for i in range(len(counts))], pl

    def _put_chains(self, old_heads, video_feat, video_mask, sub_feat, sub_mask, ids, n_clips, parts, what):
        """add (old_heads=None) / replace of whole videos on an index with chains: one validated call -- ChainTable.check_chains,
        in the packed form the runs of every part with the freed slots' runs counted as room -- then the launches: clear of the
        surplus slots, put of all parts, xml_index_set_chains over the slots whose link state changes."""
        b = self._check_batch(video_feat, video_mask, sub_feat, sub_mask, what)
        counts, offsets, part_len = self._part_lists(parts, b, what)
        plan = self.table.check_chains(counts, offsets, ids, old_heads, what)
        slots, surplus, mods = plan["put_slots"], plan["surplus"], self.modalities
        nbs = runs = clears = None
        if self.blocks is not None:
            if n_clips is None:
                n_clips = part_len if part_len is not None else \
                    self._valid_lengths([mk for m, mk in zip(("video", "sub"), (video_mask, sub_mask)) if m in mods])
            nbs = self._n_blocks(n_clips, b, what)
            runs, clears = self._find_runs(slots, nbs, what, freed=surplus)
        enc = self.encode(video_feat, video_mask, sub_feat, sub_mask)
        self._check_enc(slots, enc)
        if surplus:
            self._free_slots(surplus)
        self._launch_put(slots, plan["put_ids"], enc, nbs, runs, clears)
        self._set_chains(plan["records"])
        self.table.commit_chains(plan)
        self.version += 1
        return plan["heads"]
