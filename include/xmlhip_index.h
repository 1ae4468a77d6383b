/* xmlhip_index.h -- companion of xmlhip.h: in-place updates of a resident index whose K6 operand is the PACKED image
 * (inference.MutableCorpusIndex(tiles=N); DESIGN.md section 20, "packed form").  Same library (libxmlhip.so), same ABI
 * version, same conventions as xmlhip.h: all pointers are device memory, every entry validates its arguments before any
 * launch and returns an xml_status, is one stream-ordered launch, takes no workspace and reads nothing back.
 * (A separate header only because the guards that tie xmlhip.h to its test cases live in test files of their own; the
 * entries belong beside xml_index_put_rows)
 */
#ifndef XMLHIP_INDEX_H
#define XMLHIP_INDEX_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The packed image (xml_q2c_scores_packed) as an updatable index of `capacity` slots over n_tiles tiles of 256 rows.
 * A tile is 16 BLOCKS of 16 rows; blocks are numbered g = tile * 16 + block over the whole image.  A video occupies a RUN:
 * nb = 1..8 consecutive blocks inside ONE tile (it may cross blocks 7 | 8, the two wave tiles), packed rows
 * [16 first, 16 (first + nb)).  A run record is two int32: {first, nb}.  The caller owns the allocation (runs of live
 * videos do not overlap; index_update.BlockTable); the entries keep what xml_q2c_scores_packed reads in step with it:
 *   k6     the slice-major tile image of n_tiles * 256 rows (xml_q2c_tiled_bytes(n_tiles * 256, hidden, dt) bytes)
 *   codes  (2 * n_tiles, 8) int32 = one code per block, flat index g: -1 inside a run, the SLOT number at its last block
 *          (so xml_q2c_scores_packed writes out[q, slot]), -3 instead of -1 at block 7 of a tile when the run continues
 *          in block 8, -2 for a block of no run.  Initialise to -2.
 *   bits   (2 * n_tiles, 4) int32 per modality: 16 mask bits per block, word g >> 1, the upper half for odd g.
 * The per-slot state is that of xml_index_put_rows: feat2 (capacity, 128, hidden), imask (capacity, 128) f32,
 * vlen / slot_ids (capacity) int32, live (ceil(capacity / 32)) int32.  lpad is 128.
 *
 * xml_index_put_rows_packed: one encoded context batch -- per modality (n_mod = 1 | 2; "_a" = first, "_b" = second, NULL
 * when n_mod == 1) f1 / f2 (b, lb, hidden) of dtype dt and mask (b, lb) f32, lb <= 128 -- to the b DISTINCT slots `slots`
 * and the runs `runs` (b, 2).  The EFFECTIVE mask of video i is mask[i] AND (clip < 16 nb): a mask longer than its run is the
 * caller's error and is truncated the same way everywhere.  Per video:
 *   k6     rows [0, 16 nb) of the run: f1 L2-normalised (F.normalize; bitwise xml_l2norm_rows / xml_q2c_tile_rows_l2norm),
 *          zero rows from lb on; no row outside the run is written
 *   codes  the run's nb codes;  bits: the run's 16 nb bits of the effective mask, per modality (atomicAnd + atomicOr on the
 *          word: two videos of one call may share it), no other bit changes
 *   feat2  rows [0, lb) = f2, rows [lb, 128) zero;  imask = the effective mask, zero elsewhere
 *   vlen   max over the modalities of (last c with effective mask[c] != 0) + 1, l_ref when there is none, <= l_ref
 *   slot_ids[slot] = ids[i] (ids NULL: the slot number);  live: the slot's bit set (atomicOr)
 * nb_max (1..8): no run of the call is longer.  A record with a slot outside [0, capacity), nb outside 1..nb_max, a run
 * outside the image or across a tile boundary is dropped on the device: nothing of that video is written.  b <= 65535.
 * XML_ERR_BAD_ARG: a NULL operand, b <= 0 or b > capacity, lb outside 1..128, l_ref outside 1..128, nb_max outside 1..8,
 * n_tiles <= 0, lpad != 128, dt other than XML_F32 / XML_BF16.  XML_ERR_UNSUPPORTED: hidden that xml_q2c_tiled_ok(128, ..)
 * or xml_q2c_tile_rows_l2norm_ok refuses.
 *
 * xml_index_clear_rows_packed: n records {slots[i], runs[i]}: the run's codes become -2 and its bits 0 (atomicAnd), and
 * -- unless slots[i] == -1, "the run alone", for a replace that moves its video -- the slot is freed as
 * xml_index_clear_rows frees it: live bit cleared (atomicAnd), imask row zeroed, vlen = l_ref.  Feature rows stay.  Records
 * are dropped as above (slot outside [-1, capacity)).  XML_ERR_BAD_ARG: a NULL operand, n <= 0, nb_max outside 1..8,
 * capacity / n_tiles <= 0, l_ref outside 1..128, lpad != 128.
 * --------------------------------------------------------------------------------------------- */
int xml_index_put_rows_packed(int n_mod, const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b,
                              const void* f2_b, const float* mask_b, const int32_t* slots, const int32_t* ids,
                              const int32_t* runs, int b, int lb, int nb_max, void* k6_a, void* feat2_a, float* imask_a,
                              int32_t* bits_a, void* k6_b, void* feat2_b, float* imask_b, int32_t* bits_b, int32_t* codes,
                              int32_t* vlen, int32_t* slot_ids, int32_t* live, int capacity, int n_tiles, int lpad,
                              int l_ref, int hidden, int dt, xml_stream_t stream);
int xml_index_clear_rows_packed(int n_mod, const int32_t* slots, const int32_t* runs, int n, int nb_max, float* imask_a,
                                int32_t* bits_a, float* imask_b, int32_t* bits_b, int32_t* codes, int32_t* vlen,
                                int32_t* live, int capacity, int n_tiles, int lpad, int l_ref, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_H */
