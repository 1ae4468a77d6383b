/* xmlhip_ingest_tef.h -- companion of xmlhip.h and xmlhip_ingest_pool.h: FEATURE INGEST FOR *_tef MODELS (ctx_mode =
 * video_sub_tef / video_tef / sub_tef; tvretrieval_amd/ingest.py ContextFeeder(ctx_mode=)).  The two
 * ingest launches with the reference dataset's TEMPORAL ENDPOINT FEATURE (xml/start_end_dataset.py:127-142, 328-342)
 * appended to every clip row: two more columns, tef_st and tef_ed, after the feature columns.  Same library (libxmlhip.so),
 * same ABI version (an added function breaks no caller), same conventions: all pointers are device memory, each entry
 * validates its arguments before any launch and returns an xml_status, is one stream-ordered launch, takes no workspace,
 * reads nothing back and may be captured.  (A header of its own because the symbol sets of the sibling headers are pinned
 * by their test files.)
 *
 * Both entries write dst, (n, lmax, D + 2) of dst_dt, every element; D = d, or d_a + d_b for the pooled entry.  With
 * len = min(max_len, row_start[i + 1] - row_start[i]) as in the entries without the columns:
 *   l >= len   the row is zero in all D + 2 columns (mask 0, filled 0).
 *   l <  len   columns 0 .. D - 1 are BITWISE what xml_ingest_rows / xml_ingest_pool_rows write for the same arguments: the
 *              per-source norm and the whole-row `normalize` see the D feature columns only, never the endpoint columns.
 *              With P = tef_pos ? tef_pos[i] : 0 and L = tef_len ? tef_len[i] : len,
 *                column D      tef_st = (float)(P + l) / (float)L            one correctly rounded f32 division
 *                column D + 1  tef_ed = tef_st + (float)(1.0 / (double)L)    the double quotient rounded to f32, one f32 sum
 *              With P = 0, L = len these are bit for bit torch.arange(0, L, 1.0) / L and tef_st + 1.0 / L on the CPU.  With a
 *              bf16 dst the two values are rounded to nearest even like every other column.
 * mask and filled are as in the entries without the columns.
 *
 * tef_pos / tef_len, (n,) int32 each, place item i on a longer time axis: item i is the clips P .. P + len - 1 of a video of
 * L clips (the PARTS of a long video: P = part offset, L = clips of the whole video -- a part's columns are then bitwise
 * the columns the unsplit video has at those clips).  Both or neither are given.  An item with tef_pos[i] < 0 or
 * tef_pos[i] + len > tef_len[i] is a caller's error that the device cannot report: its two columns are computed with P = 0,
 * L = len.  No read depends on these values.
 *
 * The destination row pitch (D + 2) * size is never a multiple of 16 bytes: source loads are 16 bytes wide wherever the
 * entry without the columns takes its vector path (for the pooled entry: d_a and d_b multiples of 8, src_a and src_b 16-byte
 * aligned -- whatever the alignment of dst); stores are as wide as the destination base and pitch allow (8 bytes for f32, 4
 * for bf16 on an aligned base); elements need their natural alignment only.
 *
 * XML_ERR_BAD_ARG: every bad-argument condition of the entry without the columns; one of tef_pos / tef_len given without the
 * other.  XML_ERR_UNSUPPORTED: the conditions of the entry without the columns; D + 2 > 4098.
 */
#ifndef XMLHIP_INGEST_TEF_H
#define XMLHIP_INGEST_TEF_H

#include "xmlhip_ingest_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xml_ingest_rows (xmlhip.h) with the two endpoint columns: src (rows, d), dst (n, lmax, d + 2). */
int xml_ingest_rows_tef(const void* src, int src_dt, const int64_t* row_start, const int32_t* tef_pos, const int32_t* tef_len,
                        void* dst, int dst_dt, float* mask, int n, int lmax, int d, int max_len, float eps, int normalize,
                        xml_stream_t stream);

/* xml_ingest_pool_rows (xmlhip_ingest_pool.h) with the two endpoint columns: dst (n, lmax, d_a + d_b + 2). */
int xml_ingest_pool_rows_tef(int n_src, const void* src_a, int src_dt_a, int64_t rows_a, int d_a, const int64_t* seg_a, int norm_a,
                             const void* src_b, int src_dt_b, int64_t rows_b, int d_b, const int64_t* seg_b, int norm_b,
                             const int64_t* row_start, void* dst, int dst_dt, float* mask, float* filled, int n, int lmax,
                             int max_len, float eps, int normalize, int pool, const int32_t* tef_pos, const int32_t* tef_len,
                             xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_INGEST_TEF_H */
