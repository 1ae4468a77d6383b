/* xmlhip_index_compact.h -- companion of xmlhip.h and xmlhip_index.h: compaction of the PACKED image of an updatable index
 * (index_update.MutableCorpusIndex(tiles=N).compact()).  Same library (libxmlhip.so), same ABI
 * version (an added function breaks no caller), same conventions: all pointers are device memory, the entry validates its
 * arguments before any launch and returns an xml_status, is one stream-ordered launch, takes no workspace and reads nothing
 * back.  (A header of its own because the symbol set of xmlhip_index.h is pinned by its test file.)
 */
#ifndef XMLHIP_INDEX_COMPACT_H
#define XMLHIP_INDEX_COMPACT_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The image, the code table and the mask words are those of xmlhip_index.h: n_tiles tiles of 16 BLOCKS of 16 rows, blocks
 * numbered g = tile * 16 + block; k6 the slice-major tile image (the 16 rows of a block, for one 64-byte slice, are 1 KiB
 * contiguous at tile * slices * 16384 + slice * 16384 + block * 1024); codes (2 * n_tiles, 8) int32; bits (2 * n_tiles, 4)
 * int32 per modality.  The per-slot state (feat2, imask, vlen, slot_ids, live) is no operand: a slot keeps its number.
 *
 * xml_index_move_blocks_packed: n records of 17 int32 {tile, src[16]}.  For destination block b of `tile`:
 *   src[b] >= 0    the block receives block number src[b] (of any tile, this one included): its 16 image rows of every slice
 *                  and modality, its 16 mask bits per modality, and its code -- the source's code c when c >= 0 (the SLOT, at
 *                  the last block of a run), else -3 when b == 7 and -1 otherwise (a non-last block at position 7 continues
 *                  in block 8: the straddle marker is regenerated wherever a run lands)
 *   src[b] == -1   the block stays as it is
 *   src[b] == -2   the block becomes unused: code -2, mask bits 0 (its image rows stay, as after xml_index_clear_rows_packed)
 * All sources of a tile are read before anything of the tile is written (the image through LDS, per (tile, slice)), so a
 * record may permute the blocks of its own tile in any way -- a run may slide left over its own old blocks.  The tile's 8
 * mask words are stored whole, with plain stores.
 *
 * LAUNCH CONTRACT (the caller's; index_update.BlockTable.check_compact guarantees it).  Within one launch:
 *   - there is at most one record per tile;
 *   - every destination block (src >= 0 or -2) was free before the launch or is a block of the same tile that the record
 *     itself moves, i.e. one of its sources: no block of a video is lost;
 *   - a source block that lies in a DIFFERENT tile than its destination is not written by any record of the launch: it is
 *     neither a destination nor freed (-2);
 *   - the blocks mapped from one run are contiguous and in order.
 * After a launch that moved a run across tiles the slot's code stands TWICE in the table (old and new place) until the
 * caller has cleared the vacated run with xml_index_clear_rows_packed (slot -1, "the run alone") on the same stream; nothing
 * may read the table between the two launches.
 *
 * A record whose tile is outside [0, n_tiles) or with a src outside {-2, -1} u [0, 16 * n_tiles) is dropped whole on the
 * device: nothing of it is written.  XML_ERR_BAD_ARG: a NULL operand (k6_b / bits_b are required when n_mod == 2 and ignored
 * when n_mod == 1), n_mod outside 1..2, n <= 0 or n > 65535, n_tiles <= 0 or > 1 << 26, dt other than XML_F32 / XML_BF16.
 * XML_ERR_UNSUPPORTED: hidden / dt that xml_q2c_tiled_ok(128, hidden, dt) refuses.
 * --------------------------------------------------------------------------------------------- */
int xml_index_move_blocks_packed(int n_mod, const int32_t* records, int n, void* k6_a, int32_t* bits_a, void* k6_b,
                                 int32_t* bits_b, int32_t* codes, int n_tiles, int hidden, int dt, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_COMPACT_H */
