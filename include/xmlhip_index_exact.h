/* xmlhip_index_exact.h -- companion of xmlhip.h, xmlhip_index.h, xmlhip_index_compact.h and xmlhip_index_parts.h: exact-rank
 * mode on an index that takes updates (index_update.MutableCorpusIndex.create(..., exact_rank=True)).
 * Same library (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers are
 * device memory, every entry validates its arguments before any launch and returns an xml_status, is one stream-ordered
 * launch, takes no workspace, allocates nothing and reads nothing back.  (A header of its own because the symbol sets of the
 * other headers are pinned by their test files.)
 */
#ifndef XMLHIP_INDEX_EXACT_H
#define XMLHIP_INDEX_EXACT_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which f32-grade operands a slot holds beside the bf16 filter image (inference.exact_mode_of) */
#define XML_EXACT_F32 0  /* f32 model: re-score rows and feat2 are f32 rows                                                 */
#define XML_EXACT_F16S 1 /* XML_F16S model: both are split-f16 rows (xml_split_f16_rows) with one inv_scale float per row    */

/* ---------------------------------------------------------------------------------------------
 * An exact-rank slot.  Per modality (n_mod = 1 | 2; "_a" = first, "_b" = second, NULL when n_mod == 1) the index holds, for
 * `capacity` slots of lpad clip rows (lpad % 16 == 0, lpad <= 128):
 *   k6           the FILTER image in bf16: the slice-major tile image of xml_q2c_scores_tiled over capacity * lpad rows
 *                (tiled != 0; lpad == 128) or (capacity, lpad, hidden) row-major
 *   rescore      the re-score operand of xml_q2c_rescore: XML_EXACT_F32 (capacity, lpad, hidden) f32;  XML_EXACT_F16S the
 *                split-f16 rows, 4 bytes per element, with rescore_inv (capacity, lpad) f32
 *   feat2        K7's operand, f32 rows or split-f16 rows with feat2_inv (capacity, lpad) f32
 *   err          (capacity, lpad) f32: the bf16 rounding-error norm of every stored row
 *   imask, bits  (capacity, lpad) f32 and (capacity, 4) int32, as for xml_index_put_rows
 * and once: ec (n_mod) f32, the RUNNING BOUND e_c -- at least the largest err of the rows put so far, per modality --,
 * vlen / slot_ids (capacity) int32, live (ceil(capacity / 32)) int32.  rescore_inv / feat2_inv are NULL in XML_EXACT_F32.
 *
 * xml_index_put_rows_exact: one encoded context batch -- f1 / f2 (b, lb, hidden) F32 and mask (b, lb) f32 per modality,
 * lb <= lpad -- to the b DISTINCT slots `slots`.  Every one of a slot's lpad rows is written in every operand; row r < lb of
 * video i holds, with y = F.normalize(f1[i, r]) (bitwise xml_l2norm_rows),
 *   k6       rne_bf16(y) (bitwise xml_round_bf16_rows_err)
 *   err      || y - rne_bf16(y) ||_2 in f32, bitwise xml_round_bf16_rows_err's value (its reduction order: one wave per row)
 *   rescore  y, or what xml_split_f16_rows(y, fixed_log2 = XML_F16_UNIT_LOG2) writes (data and inv_scale = 2^-14)
 *   feat2    f2[i, r], or what xml_split_f16_rows(f2[i, r], fixed_log2 = -1) writes (data and the row's inv_scale)
 * and a row r >= lb what the same arithmetic makes of a zero row (zeros; inv_scale 2^-14 and 1; err 0).  The mask row, the 4
 * mask-bit words, vlen, slot_ids[slot] = ids[i] (ids NULL: the slot number) and the live bit: exactly xml_index_put_rows.
 * ec[m] is raised by an integer atomicMax on the float's bits of every row's err: the norms are non-negative, for which the
 * unsigned order of the bits is the order of the values, so the cell ends as the maximum whatever the order of the rows --
 * bit for bit max(ec before, the batch's err values).  A NaN norm (a row with a non-finite element) raises the cell to +inf
 * instead of leaving a NaN there: the certificate then fails for every query and the search re-scores against the whole corpus,
 * which is the safe answer; err itself keeps the NaN.  The cell is never lowered here.
 * A slot outside [0, capacity) is dropped on the device: nothing of that video is written.  The source rows are read from
 * memory once (the normalisation and the rounding walk a row in two lane orders; the second walk hits the cache), loads and
 * stores are 16 bytes per lane.  b <= 65535.
 * XML_ERR_BAD_ARG: mode other than the two above, n_mod other than 1 | 2, a NULL operand (rescore_inv / feat2_inv only in
 * XML_EXACT_F16S), b <= 0 or b > capacity, lb outside 1..lpad, l_ref outside 1..lpad, capacity <= 0.
 * XML_ERR_UNSUPPORTED: dt other than XML_F32, lpad % 16 != 0 or lpad > 128, tiled with lpad != 128 or with a hidden that
 * xml_q2c_tiled_ok(128, hidden, XML_BF16) refuses, hidden that xml_q2c_tile_rows_l2norm_ok(hidden, XML_F32) refuses,
 * hidden % 32 != 0 in XML_EXACT_F16S.
 * (Slots are freed by xml_index_clear_rows; ec is left alone -- a bound that is too large costs second-tier work, never a
 * wrong list -- until xml_index_exact_bound recomputes it.)
 * --------------------------------------------------------------------------------------------- */
int xml_index_put_rows_exact(int n_mod, int mode, const void* f1_a, const void* f2_a, const float* mask_a, const void* f1_b,
                             const void* f2_b, const float* mask_b, const int32_t* slots, const int32_t* ids, int b, int lb,
                             void* k6_a, void* rescore_a, float* rescore_inv_a, void* feat2_a, float* feat2_inv_a,
                             float* err_a, float* imask_a, int32_t* bits_a, void* k6_b, void* rescore_b, float* rescore_inv_b,
                             void* feat2_b, float* feat2_inv_b, float* err_b, float* imask_b, int32_t* bits_b, float* ec,
                             int32_t* vlen, int32_t* slot_ids, int32_t* live, int capacity, int lpad, int l_ref, int hidden,
                             int dt, int tiled, xml_stream_t stream);

/* xml_exact_certificate (xmlhip.h) with the corpus bound read from the device when the kernel runs: ec points to n_mod
 * floats (the cells xml_index_put_rows_exact maintains), and the slack is slack_base + slack_ec2 * max_m(ec[m])^2, evaluated
 * in f32 in the kernel (slack_ec2 == 0: slack_base alone, no product is formed).  A cell at +inf -- a NaN norm was put --
 * gives eps = +inf and thr = -inf whatever slack_ec2 is: every query fails (outside != 0) and a second tier that selects
 * filter scores >= thr takes every video.  A captured search sees the bound of the moment of its replay.  Everything else -- eps,
 * fail, thr, n_fail (the caller zeroes it), the exp(alpha s) transform of top_val in place -- is xml_exact_certificate's.
 * XML_ERR_BAD_ARG: as xml_exact_certificate, and a NULL ec. */
int xml_exact_certificate_dev(const float* filter_scores, int m, float* top_val, int k, const float* eq0, const float* eq1,
                              const float* ec, int n_mod, float slack_base, float slack_ec2, float alpha, int outside,
                              int32_t* fail, float* eps_out, float* thr_out, int32_t* n_fail, int nq, xml_stream_t stream);

/* ec[m] = max over the LIVE slots s and their rows r of err_m[s, r] (err_b NULL when n_mod == 1): tightens the running bound
 * after removals.  Writes all n_mod cells; 0 when no slot is live.  A NaN counts as +inf, a negative value as 0.  One launch
 * of one workgroup per modality (a maintenance call, not part of a search: it streams capacity * lpad floats).
 * XML_ERR_BAD_ARG: n_mod other than 1 | 2, a NULL operand, capacity <= 0, lpad <= 0. */
int xml_index_exact_bound(int n_mod, const float* err_a, const float* err_b, const int32_t* live, float* ec, int capacity,
                          int lpad, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INDEX_EXACT_H */
