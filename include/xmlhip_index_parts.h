/* xmlhip_index_parts.h -- companion of xmlhip.h, xmlhip_index.h and xmlhip_index_compact.h: videos longer than l_ref clips
 * on an updatable index (index_update.MutableCorpusIndex.create(..., part_overlap=O)).  Same library
 * (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers are device memory,
 * every entry validates its arguments before any launch and returns an xml_status, is one stream-ordered launch (the fold:
 * one per 2 097 120 score rows), takes no workspace, allocates nothing and reads nothing back; rows == 0 / n == 0 returns
 * XML_OK and launches nothing.  (A header of its own because the symbol sets of the other index headers are pinned by their
 * test files.)
 */
#ifndef XMLHIP_INDEX_PARTS_H
#define XMLHIP_INDEX_PARTS_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * A long video is stored as overlapping PARTS (ingest.plan_parts), each part in a slot of its own -- an ordinary video to
 * the encoders, K6, K7, K9, NMS and the update entries.  The slots of one video form a CHAIN, described by three per-slot
 * tables of `capacity` int32 each:
 *   chain_head[s]    the slot of the first part (offset 0) of slot s's video
 *   chain_next[s]    the slot of the next part in rising offset order, -1 at the end
 *   chain_offset[s]  the first clip of slot s's part within its source video: the part_offset of xml_moments_decode_parts
 *                    (whose meta2vid is the slot -> id table: all slots of a chain carry their video's id)
 * INVARIANT (the caller's, index_update.ChainTable keeps it): a slot that is free, or that holds a video of one part, is in
 * the SINGLE state head == itself, next == -1, offset == 0; all slots of a chain are live; a chain has no cycle.
 *
 * BOUNDED WALK.  No entry trusts the tables: a walk visits at most max_parts slots, stops at a next outside [0, capacity)
 * and ignores a head outside that range.  A damaged table can give a wrong bit / slot, never an access outside the tables
 * or a score row and never a kernel that does not end.
 *
 * BEST PART of a chain for one score row: the running best starts as (head, -inf); following next, a later part replaces it
 * when its score is strictly greater.  Ties go to the lowest offset, a NaN never wins, a chain of nothing but -inf / NaN is
 * represented by its head -- the rule of xml_group_best_allow with row order replaced by chain order.
 * --------------------------------------------------------------------------------------------- */

/* n records of four int32 {slot, head, next, offset}: chain_head[slot] = head, chain_next[slot] = next, chain_offset[slot]
 * = offset.  Links a new chain, and resets the slots of a removed one to the single state {s, s, -1, 0}.  The slots of one
 * call are distinct (the caller's).  A record whose slot is outside [0, capacity) writes nothing (checked on the device).
 * XML_ERR_BAD_ARG: a NULL pointer, n < 0, capacity <= 0. */
int xml_index_set_chains(const int32_t* records, int n, int32_t* chain_head, int32_t* chain_next, int32_t* chain_offset,
                         int capacity, xml_stream_t stream);

/* The fold between K6 and K8.  scores (rows, capacity) f32 with row stride ld; video_allow (1 | rows, allow_ld >=
 * ceil(capacity / 32)) words, never NULL (a caller always has the live words); out_bits (rows, out_ld >= ceil(capacity / 32))
 * words in the bit layout of xml_topk_rows_allowed.  Bit s of a row is set iff the allow bit of chain_head[s] is set for that
 * row and s is the best part of its chain.  ONLY THE HEAD'S BIT IS TESTED: a caller's mask numbers a video by its head slot,
 * and ANDed with the live words such a mask has the other bits of a chain at 0 while the live words alone have them at 1.
 * A free slot is single with a clear live bit: its bit is 0.  A chain of one slot is its own best part whatever it scores --
 * its score is NOT READ (the packed K6 leaves the columns of free slots unspecified).  Padding bits of the last word are 0;
 * words beyond ceil(capacity / 32) are not written.
 * XML_ERR_BAD_ARG: a NULL pointer, rows < 0, capacity <= 0, max_parts < 1, ld < capacity, out_ld or allow_ld <
 * ceil(capacity / 32), allow_rows other than 1 or rows. */
int xml_chain_best_allow(const float* scores, int64_t ld, int rows, int capacity, const int32_t* chain_head,
                         const int32_t* chain_next, int max_parts, const uint32_t* video_allow, int64_t allow_ld,
                         int allow_rows, uint32_t* out_bits, int64_t out_ld, xml_stream_t stream);

/* xml_best_part_rows for chains: video (rows,) names one video per row by ANY slot of it; out (rows,) = the slot of that
 * video's best part for the row, -1 for a slot outside [0, capacity) (or whose head lies outside it).  SVMR and ground-truth
 * videos use it.
 * XML_ERR_BAD_ARG: a NULL pointer, rows < 0, capacity <= 0, max_parts < 1, ld < capacity. */
int xml_chain_best_rows(const float* scores, int64_t ld, int rows, int capacity, const int32_t* chain_head,
                        const int32_t* chain_next, int max_parts, const int32_t* video, int32_t* out, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_PARTS_H */
