/* xmlhip_index_parts_exact.h -- companion of xmlhip_index_parts.h and xmlhip_index_exact.h: videos longer than l_ref clips on
 * an EXACT-RANK updatable index (index_update.MutableCorpusIndex.create(..., exact_rank=True, exact_part_overlap=O); DESIGN.md
 * section 20g).  Same library (libxmlhip.so), same ABI version (an added function breaks no caller), the conventions of
 * xmlhip_index_parts.h: all pointers are device memory, every entry validates its arguments before any launch and returns
 * an xml_status, is one stream-ordered launch, takes no workspace, allocates nothing and reads nothing back; rows == 0
 * validates, returns XML_OK and launches nothing.  (A header of its own because the symbol sets of the other index headers are
 * pinned by their test files.)
 *
 * Exact-rank mode never forms the f32 (Nq, slots) score matrix that xml_chain_best_allow folds.  What it has are CANDIDATE
 * LISTS: per query m slots with their re-scored, f32-grade values.  The fold of a chain index runs on those lists (a), under
 * per-slot allow words made from a caller's head-bit mask (b); SVMR gets the slots of one video as a list to re-score (c).
 * The chain tables are those of xmlhip_index_parts.h, and its BOUNDED WALK holds here too: no table value is used as an index
 * without a range check.
 */
#ifndef XMLHIP_INDEX_PARTS_EXACT_H
#define XMLHIP_INDEX_PARTS_EXACT_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The widest candidate list xml_cand_best_part folds (4 096: the widest list the exact-rank chains re-score). */
int xml_cand_best_part_max_m(void);

/* (a) The fold on a candidate list.  scores / ids (rows, m) f32 / int32 with row stride ld (both); group / order (n,) int32
 * per-slot tables (for chains: chain_head, chain_offset); out_scores / out_ids (rows, m) with row stride out_ld.  IN PLACE is
 * allowed (out_scores == scores and out_ids == ids with out_ld == ld); any other overlap is not.
 * A candidate whose id lies outside [0, n) (-1 by convention) is EMPTY and passes through unchanged.  Two candidates belong
 * together when both ids are in range and their group values are equal; a group value outside [0, n) makes the candidate a
 * group of its own.  Within a group the winner is chosen by v = isnan(s) ? -inf : s: the greatest v wins, ties go to the
 * smallest order, a further tie to the lower position in the row.  The winner keeps its score bits and its id, every other
 * member becomes (-inf, -1).
 * On a list that holds ALL slots of a chain the winner is the slot xml_chain_best_allow marks for the same scores -- maximum,
 * ties to the lowest offset, a NaN never wins --, including the chain of nothing but -inf / NaN, which its head (offset 0)
 * represents.
 * One workgroup per row; a candidate that is the only one of its group in the row costs no scan of the row.
 * XML_ERR_BAD_ARG: a NULL pointer, rows < 0, m < 1, m > xml_cand_best_part_max_m(), ld or out_ld < m, n <= 0. */
int xml_cand_best_part(const float* scores, const int32_t* ids, int64_t ld, int rows, int m, const int32_t* group,
                       const int32_t* order, int n, float* out_scores, int32_t* out_ids, int64_t out_ld, xml_stream_t stream);

/* (b) A caller's head-bit mask made per-slot.  video_allow (1 | rows, allow_ld >= ceil(capacity / 32)) words in which a video
 * is numbered by its HEAD slot; out_bits (rows, out_ld >= ceil(capacity / 32)) words: bit s = the allow bit of chain_head[s]
 * for that row, 0 for a head outside [0, capacity).  Padding bits of the last word are 0; words beyond ceil(capacity / 32)
 * are not written.  ANDed with the live words the result is the allow= of every selection over slots.
 * XML_ERR_BAD_ARG: a NULL pointer, rows < 0, capacity <= 0, allow_ld or out_ld < ceil(capacity / 32), allow_rows other than 1
 * or rows. */
int xml_chain_spread_allow(const uint32_t* video_allow, int64_t allow_ld, int allow_rows, int rows, int capacity,
                           const int32_t* chain_head, uint32_t* out_bits, int64_t out_ld, xml_stream_t stream);

/* (c) The slots of one video per row.  video (rows,) names a video by ANY slot of it; out (rows, out_ld >= max_parts): the
 * chain's slots in rising offset order, -1 beyond its end; all -1 for a slot outside [0, capacity) or whose head lies outside
 * it.  The walk visits at most max_parts slots and stops at a next outside [0, capacity): a chain longer than max_parts is
 * cut there, a damaged table gives a wrong slot, never an access outside the tables and never a kernel that does not end.
 * XML_ERR_BAD_ARG: a NULL pointer, rows < 0, capacity <= 0, max_parts < 1, out_ld < max_parts. */
int xml_chain_members(const int32_t* video, int rows, int capacity, const int32_t* chain_head, const int32_t* chain_next,
                      int max_parts, int32_t* out, int64_t out_ld, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_PARTS_EXACT_H */
