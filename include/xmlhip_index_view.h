/* xmlhip_index_view.h -- companion of xmlhip.h, xmlhip_index.h and xmlhip_index_compact.h: SUBSET VIEWS of a resident index
 * (inference.video_subset, tvretrieval_amd/subset.py).  A view is a small packed K6 image that holds
 * copies of the blocks of the allowed videos only, so that xml_q2c_scores_packed over it costs what the allowed videos cost.
 * Same library (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers are
 * device memory, the entry validates its arguments before any launch and returns an xml_status, is one stream-ordered
 * launch, takes no workspace and reads nothing back.  (A header of its own because the symbol sets of the sibling headers
 * are pinned by their test files.)
 */
#ifndef XMLHIP_INDEX_VIEW_H
#define XMLHIP_INDEX_VIEW_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Images, block numbering and mask words are those of xmlhip_index.h / xmlhip_index_compact.h: tiles of 16 BLOCKS of 16 rows,
 * blocks numbered g = tile * 16 + block; k6 the slice-major tile image (the 16 rows of a block, for one 64-byte slice, are
 * 1 KiB contiguous at tile * slices * 16384 + slice * 16384 + block * 1024); the 16 mask bits of block g are in word g >> 1
 * of a modality's bits, in the upper half for odd g.  Every resident K6 operand -- the fixed image of two videos per tile
 * (video v = blocks 8 v .. 8 v + 7), the length-bucketed image, the packed image of an updatable index -- is such an image.
 *
 * xml_index_gather_blocks: src_block holds 16 * n_tiles_dst int32, one per DESTINATION block:
 *   s >= 0   the destination block receives source block s: its 16 image rows of every slice and modality and its 16 mask
 *            bits of every modality
 *   -2       the destination block is unused: its mask bits become 0, its image rows are not written
 * An entry outside {-2} u [0, n_blocks_src) is handled as -2.  bits_src_m == NULL: that modality of the source is all-valid
 * (mask mode 1 of the fixed image) -- every copied block gets 16 one bits.  EVERY destination mask word (8 per tile and
 * modality) is stored, whole, with a plain store by the one thread that owns both of its halves.  Nothing outside the
 * destination images (n_tiles_dst * slices * 16384 bytes each) and mask words (n_tiles_dst * 8 each) is written.  The code
 * table of the destination is the caller's (it is built on the host with the placement).
 * Source and destination must not overlap (the caller's contract): the copy goes through registers only.
 *
 * XML_ERR_BAD_ARG: a NULL required operand (src_block, k6_src_a, k6_dst_a, bits_dst_a; with n_mod == 2 also k6_src_b,
 * k6_dst_b, bits_dst_b -- with n_mod == 1 the _b operands are ignored), n_mod outside 1..2, n_tiles_dst <= 0,
 * n_blocks_src <= 0, dt other than XML_F32 / XML_BF16.
 * XML_ERR_UNSUPPORTED: hidden / dt that xml_q2c_tiled_ok(128, hidden, dt) refuses.
 * --------------------------------------------------------------------------------------------- */
int xml_index_gather_blocks(int n_mod, const int32_t* src_block, int n_tiles_dst, const void* k6_src_a,
                            const uint32_t* bits_src_a, const void* k6_src_b, const uint32_t* bits_src_b,
                            int64_t n_blocks_src, void* k6_dst_a, int32_t* bits_dst_a, void* k6_dst_b, int32_t* bits_dst_b,
                            int hidden, int dt, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_VIEW_H */
