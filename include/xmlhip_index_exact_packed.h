/* xmlhip_index_exact_packed.h -- companion of xmlhip_index_exact.h and xmlhip_index.h: exact-rank mode on an updatable index
 * whose bf16 FILTER image is the packed image of xml_q2c_scores_packed (index_update.MutableCorpusIndex.create(...,
 * exact_rank=True, filter_tiles=N)).  Same library (libxmlhip.so), same ABI version (an added function
 * breaks no caller), same conventions: all pointers are device memory, the entry validates its arguments before any launch
 * and returns an xml_status, is one stream-ordered launch, takes no workspace, allocates nothing and reads nothing back.  (A
 * header of its own because the symbol sets of the other headers are pinned by their test files.)
 */
#ifndef XMLHIP_INDEX_EXACT_PACKED_H
#define XMLHIP_INDEX_EXACT_PACKED_H

#include "xmlhip_index_exact.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The put of an exact-rank slot (xmlhip_index_exact.h, "An exact-rank slot") whose filter rows lie in a RUN of the packed
 * image (xmlhip_index.h): the operands of xml_index_put_rows_exact with, per modality,
 *   k6     the packed bf16 tile image over n_tiles * 256 rows
 *   bits   (2 * n_tiles, 4) int32, the packed mask words (16 bits per block)
 * and once codes (2 * n_tiles, 8) int32 and runs (b, 2) int32 = (first block, blocks) per video, as for
 * xml_index_put_rows_packed.  Only the filter image is packed: rescore, rescore_inv, feat2, feat2_inv, err and imask stay
 * (capacity, 128, ..) per slot.  For video i with run {first, nb} and keep = 16 nb:
 *   filter image  rows [0, keep) of the run hold rne_bf16(F.normalize(f1[i, r])), bitwise what xml_index_put_rows_exact stores
 *                 for the same row; zero from the batch's width lb on.  No row outside the run is written.
 *   codes, bits   exactly xml_index_put_rows_packed: -1 inside the run, the SLOT at its last block, -3 at block 7 of a tile
 *                 when the run goes on into block 8; the run's 16-bit mask fields by atomicAnd then atomicOr (two videos may
 *                 share a word); codes are written by modality 0 only.
 *   rescore, rescore_inv, feat2, feat2_inv, err
 *                 all 128 rows of the slot, bitwise xml_index_put_rows_exact's values WHATEVER the run: the rows [keep, lb)
 *                 that the filter does not hold are stored here too.
 *   ec[m]         raised by the same atomicMax over the err of EVERY row of the slot (a NaN norm: +inf), a superset of the rows
 *                 the filter scores -- the bound stays valid, and bit for bit that of xml_index_put_rows_exact after the
 *                 same batch.
 *   imask, bits, vlen   follow the EFFECTIVE mask, mask AND (clip < keep), as for xml_index_put_rows_packed: the filter, the
 *                 re-score and K7 / K9 see one valid length.  slot_ids, live: xml_index_put_rows.
 * A record with a slot outside [0, capacity), nb outside 1..nb_max, a run outside the image or across a tile boundary is
 * dropped whole on the device: nothing of it is written.  Slots of one call are distinct, runs do not overlap (the host's
 * tables guarantee both).  b <= 65535.
 * XML_ERR_BAD_ARG: mode other than XML_EXACT_F32 | XML_EXACT_F16S, n_mod other than 1 | 2, a NULL operand (ids may be NULL;
 * rescore_inv / feat2_inv only in XML_EXACT_F16S), lpad != 128, b <= 0 or b > capacity, lb outside 1..lpad, l_ref outside
 * 1..lpad, capacity <= 0, nb_max outside 1..8, n_tiles <= 0.
 * XML_ERR_UNSUPPORTED: dt other than XML_F32, a hidden that xml_q2c_tiled_ok(128, hidden, XML_BF16) or
 * xml_q2c_tile_rows_l2norm_ok(hidden, XML_F32) refuses, hidden % 32 != 0 in XML_EXACT_F16S.
 * (Runs are freed by xml_index_clear_rows_packed and moved by xml_index_move_blocks_packed with dt = XML_BF16.)
 * --------------------------------------------------------------------------------------------- */
int xml_index_put_rows_packed_exact(int n_mod, int mode, const void* f1_a, const void* f2_a, const float* mask_a,
                                    const void* f1_b, const void* f2_b, const float* mask_b, const int32_t* slots,
                                    const int32_t* ids, const int32_t* runs, int b, int lb, int nb_max, void* k6_a,
                                    void* rescore_a, float* rescore_inv_a, void* feat2_a, float* feat2_inv_a, float* err_a,
                                    float* imask_a, int32_t* bits_a, void* k6_b, void* rescore_b, float* rescore_inv_b,
                                    void* feat2_b, float* feat2_inv_b, float* err_b, float* imask_b, int32_t* bits_b,
                                    int32_t* codes, float* ec, int32_t* vlen, int32_t* slot_ids, int32_t* live, int capacity,
                                    int n_tiles, int lpad, int l_ref, int hidden, int dt, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_EXACT_PACKED_H */
