/* xmlhip_train_pool.h -- companion of xmlhip.h, xmlhip_ingest_pool.h and xmlhip_ingest_tef.h: TRAINING BATCHES FROM RESIDENT
 * FRAME- AND WORD-LEVEL STORES (tvretrieval_amd/train_data.py DeviceTrainStore over ingest.PooledStore).
 * The batch gather of xml_gather_feature_rows with the segmented reduction of xml_ingest_pool_rows in front of it: the fine rows
 * of a whole store stay on the device, a step sends its example ids and each clip row of the batch is pooled in the gather
 * launch.  Same library (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers
 * are device memory, the entry validates its arguments before any launch and returns an xml_status, is one stream-ordered
 * launch, takes no workspace, allocates nothing, reads nothing back and may be captured.  (A header of its own because the
 * symbol sets of the sibling headers are pinned by their test files.)
 */
#ifndef XMLHIP_TRAIN_POOL_H
#define XMLHIP_TRAIN_POOL_H

#include "xmlhip_ingest_tef.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * xml_gather_pool_feature_rows: n_src = 1 or 2 SOURCES (a, and b); source x is src_x, (rows_x, d_x) row-major of src_dt_x =
 * XML_F16 or XML_F32 -- the RESIDENT fine rows of a whole store.  clip_start, (n_items + 1) int64: item j owns the clip rows
 * clip_start[j] .. clip_start[j + 1] - 1 of one clip numbering that both sources share.  seg_x, (clip_start[n_items], 2) int64:
 * the ABSOLUTE half-open range of source rows of every clip of every item (the sources may order their items differently).
 * ids (n,) int32, item_of (n_examples,) int32 or NULL, n_examples: as in xml_gather_feature_rows.
 *
 * Written: dst, (n, lmax, d_a + d_b + 2 * tef) of dst_dt = XML_F32 or XML_BF16, every element; mask (n, lmax) f32 unless NULL;
 * len_out (n,) int32 unless NULL.  For batch position i: item = item_of ? item_of[ids[i]] : ids[i]; an id or an item out of
 * range gives len = 0 (zero rows, zero mask, nothing read); else len = min(clips of the item, max_len, lmax), a negative count
 * counting as 0.  len_out[i] = len.
 *   l >= len   the row is zero in every column, mask 0.
 *   l <  len   mask 1; with r = clip_start[item] + l the d_a + d_b feature columns are BITWISE the row xml_ingest_pool_rows
 *              writes for the ranges seg_a[r], seg_b[r] under the same pool, norm_a, norm_b, normalize and eps: an empty,
 *              inverted or out-of-range range reads nothing and gives a zero block.  With tef = 1 the row ends in
 *              (float)l / (float)len and that plus (float)(1.0 / (double)len) -- the columns of xml_gather_feature_rows(tef = 1)
 *              and of xml_ingest_pool_rows_tef without tef_pos; they are not normalised.
 * A row's bits depend on its own ranges alone: not on the batch position, n, lmax, its neighbours or the launch.  16-byte loads
 * are used under the conditions of xml_ingest_pool_rows (with tef: of xml_ingest_pool_rows_tef, where the destination decides
 * the store width only); any other shape or alignment takes the element-wise path with the same results.
 *
 * XML_ERR_BAD_ARG: a NULL required operand (src_a, seg_a, clip_start, ids, dst; with n_src == 2 also src_b, seg_b), n_src
 * outside 1..2, n / lmax / max_len / d_a / rows_a / n_items <= 0 (with n_src == 2 also d_b / rows_b), n_examples <= 0 with
 * item_of, a source dtype other than XML_F16 / XML_F32, a dst_dt other than XML_F32 / XML_BF16, a pool other than XML_POOL_MAX /
 * XML_POOL_MEAN, tef or normalize other than 0 / 1, eps NaN.  XML_ERR_UNSUPPORTED: d_a + d_b > 4096.  With n_src == 1 every _b
 * argument is ignored and d_b counts as 0.
 * --------------------------------------------------------------------------------------------- */
int xml_gather_pool_feature_rows(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a, int norm_a,
                                 const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                                 const int64_t* clip_start, int64_t n_items, const int32_t* ids, int n, const int32_t* item_of,
                                 int64_t n_examples, void* dst, int dst_dt, float* mask, int32_t* len_out, int lmax, int max_len,
                                 float eps, int normalize, int pool, int tef, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_TRAIN_POOL_H */
