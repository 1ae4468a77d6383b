/* xmlhip_ingest_pool.h -- companion of xmlhip.h: FEATURE INGEST FROM FRAME- AND WORD-LEVEL STORES (tvretrieval_amd/ingest.py
 * PooledStore / ContextFeeder).  The context collate of xml_ingest_rows (truncate, pad, normalise,
 * mask) on rows FINER than clips: each clip row of the batch is pooled, in the same launch, over a range of source rows.
 * Same library (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers are
 * device memory, the entry validates its arguments before any launch and returns an xml_status, is one stream-ordered
 * launch, takes no workspace and reads nothing back.  (A header of its own because the symbol sets of the sibling headers
 * are pinned by their test files.)
 */
#ifndef XMLHIP_INGEST_POOL_H
#define XMLHIP_INGEST_POOL_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pool: how the source rows of a clip become one row */
#define XML_POOL_MAX 0  /* column-wise maximum */
#define XML_POOL_MEAN 1 /* column-wise f32 sum in row order, divided by the row count */

/* ---------------------------------------------------------------------------------------------
 * xml_ingest_pool_rows: n videos; video i owns the clip rows row_start[i] .. row_start[i + 1] - 1 of the batch (row_start:
 * n + 1 int64, as in xml_ingest_rows), R = row_start[n] clip rows in all.  There are n_src = 1 or 2 SOURCES (a, and b);
 * source x is src_x, (rows_x, d_x) row-major of src_dt_x = XML_F16 or XML_F32, and seg_x, (R, 2) int64: clip row r is pooled
 * over the source rows seg_x[r][0] <= j < seg_x[r][1].  With n_src == 1 every _b argument is ignored and d_b counts as 0.
 *
 * Written: dst, (n, lmax, d_a + d_b) of dst_dt = XML_F32 or XML_BF16, every element; mask (n, lmax) f32 unless NULL; filled
 * (n, lmax) f32 unless NULL.  For destination row (i, l), with len = min(max_len, row_start[i + 1] - row_start[i]):
 *   l >= len   the row is zero, mask 0, filled 0; nothing is read for it.
 *   l <  len   mask 1; r = row_start[i] + l.  Per source the column block (a: columns 0 .. d_a - 1, b: d_a .. d_a + d_b - 1)
 *              is the pool (XML_POOL_MAX / XML_POOL_MEAN) of its range.  A range that is empty (lo == hi) or not within
 *              0 <= lo <= hi <= rows_x reads NOTHING and gives a zero block.  filled is 1 where at least one source's range
 *              was valid and non-empty, else 0.  Then, with norm_x != 0, the block becomes x / (||x||_2 + eps); then, with
 *              normalize != 0, the whole row of d_a + d_b columns becomes x / (||x||_2 + eps); then the row is stored once.
 * Each source row of a range is read once per clip row that names it; sums of squares are f32; nothing is accumulated with
 * atomics: a clip row's value depends on its own ranges only and is bitwise the same in every launch.  16-byte accesses are
 * used when d_a and d_b are multiples of 8 and src_a, src_b and dst are 16-byte aligned; any other shape or alignment
 * (elements need their natural alignment only) takes an element-wise path with the same results.
 *
 * XML_ERR_BAD_ARG: a NULL required operand (src_a, seg_a, row_start, dst; with n_src == 2 also src_b, seg_b), n_src outside
 * 1..2, n / lmax / max_len / d_a / rows_a <= 0 (with n_src == 2 also d_b / rows_b), a source dtype other than XML_F16 /
 * XML_F32, a dst_dt other than XML_F32 / XML_BF16, a pool other than XML_POOL_MAX / XML_POOL_MEAN.
 * XML_ERR_UNSUPPORTED: d_a + d_b > 4096 (the widest input row of xml_pack_plan).
 * --------------------------------------------------------------------------------------------- */
int xml_ingest_pool_rows(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a, int norm_a,
                         const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                         const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled, int n, int lmax,
                         int max_len, float eps, int normalize, int pool, xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INGEST_POOL_H */
