/* xmlhip_train_index.h -- companion of xmlhip.h, xmlhip_index_view.h and xmlhip_train_pool.h: TRAINING THE QUERY SIDE ON A
 * RESIDENT INDEX (tvretrieval_amd/train_index.py).  The context operands of a training step are
 * gathered from the index rows of the batch's videos, and the loss tail writes query gradients only.  Same library
 * (libxmlhip.so), same ABI version (an added function breaks no caller), same conventions: all pointers are device memory,
 * every entry validates its arguments before any launch and returns an xml_status, is one stream-ordered launch, takes no
 * workspace, allocates nothing, reads nothing back and may be captured.  (A header of its own because the symbol sets of
 * the sibling headers are pinned by their test files.)
 */
#ifndef XMLHIP_TRAIN_INDEX_H
#define XMLHIP_TRAIN_INDEX_H

#include "xmlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the two source forms of the K6 operand (`form` below) */
enum { XML_INDEX_ROW_MAJOR = 0, XML_INDEX_BLOCK_IMAGE = 1 };

/* ---------------------------------------------------------------------------------------------
 * xml_index_gather_video_rows: the context operands of a batch of n videos from the index, for the n_mod (1 or 2)
 * modalities of the model in one launch.  slot (n,) int32: the index row / slot of every batch item.  vlen (n_videos,)
 * int32: valid clips per slot.  Per modality x = a, b the index holds
 *   cn_src_x    the K6 operand, L2-normalised rows of dt = XML_F32 or XML_BF16:
 *               form XML_INDEX_ROW_MAJOR    (n_videos, lpad, hidden) row-major; first_block is ignored (may be NULL)
 *               form XML_INDEX_BLOCK_IMAGE  the slice-major image of n_blocks blocks of 16 rows (layout: xmlhip_index_view.h);
 *                                           first_block (n,) int32: the first block of every batch item's run -- clip l of
 *                                           the item is image row 16 * first_block[i] + l.  The fixed image (video v =
 *                                           blocks 8 v ..), the length-bucketed image and the packed image of an index
 *                                           that takes updates (a run may cross blocks 7 | 8 of its tile) are all read so.
 *   f2_src_x    (n_videos, lpad, hidden) dt row-major
 *   mask_src_x  (n_videos, lpad) f32
 * Written, every element exactly once, with 16-byte stores (4-byte for the masks): cn_x, f2_x (n, l, hidden) dt and mask_x
 * (n, l) f32, l <= lpad.  Row (i, c) is a copy of clip c of slot[i] -- bit for bit what the index holds -- when
 * 0 <= slot[i] < n_videos and c < vlen[slot[i]] (and, block image: first_block[i] >= 0 and the row's block < n_blocks);
 * every other row is zero in cn_x and f2_x with mask 0: an item out of range is an empty example, as in
 * xml_gather_feature_rows.  Nothing outside the sources is read for any value of slot / first_block / vlen.
 *
 * XML_ERR_BAD_ARG: a NULL required operand (slot, vlen, cn_src_a, f2_src_a, mask_src_a, cn_a, f2_a, mask_a; with the block
 * image first_block; with n_mod == 2 the _b operands too -- with n_mod == 1 they are ignored), n_mod outside 1..2, a form
 * other than the two above, n / l / lpad / hidden / n_videos <= 0, l > lpad, n_blocks <= 0 with the block image, dt other
 * than XML_F32 / XML_BF16, a feature pointer that is not 16-byte aligned.
 * XML_ERR_UNSUPPORTED: block image: rows that are not whole 64-byte slices (every width xml_q2c_tiled_ok(128, hidden, dt) takes
 * is one: the layout formula holds for any number of slices); row-major: hidden % 8 != 0; hidden > 4096.
 * --------------------------------------------------------------------------------------------- */
int xml_index_gather_video_rows(int n_mod, int form, const int32_t* slot, const int32_t* first_block, int n,
                                const int32_t* vlen, int64_t n_videos, int64_t n_blocks, int lpad, const void* cn_src_a,
                                const void* f2_src_a, const float* mask_src_a, const void* cn_src_b, const void* f2_src_b,
                                const float* mask_src_b, void* cn_a, void* f2_a, float* mask_a, void* cn_b, void* f2_b,
                                float* mask_b, int l, int hidden, int dt, xml_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * xml_q2c_scores_arg_bwd_q: the QUERY gradient of the in-batch video-level scores of xml_q2c_scores_arg, for the n_mod (1 or
 * 2) modalities in one launch; the calling form is that of xml_q2c_scores_l2norm_bwd_multi (every per-modality argument a
 * HOST array of n_mod entries).  query (nq, hidden): the un-normalised query rows; qn (nq, hidden) and cn (nv, l[m], hidden):
 * what the forward pass scored; mask (nv, l[m]) f32; arg (nq, nv) int32 row stride ld_arg: the arg-max clips the forward
 * pass kept; dscores (nq, nv) f32 row stride ld_ds, multiplied by `scale`.  Written: dq[m] (nq, hidden) dt, every element:
 *   dqn[q] = sum over v, in ascending v, of scale dscores[q, v] mask[v, arg[q, v]] cn[v, arg[q, v], :]
 *   dq[q]  = the F.normalize backward of row query[q] applied to dqn[q]
 * the sums, in the order, of the dq of xml_q2c_scores_l2norm_bwd_multi.  cn is taken as already normalised: there is no raw
 * feat, no second normalisation and no dfeat.  An arg entry outside [0, l[m]) contributes nothing.  No float
 * atomics: the sum of a row has a fixed order.  (qn is part of the calling form and is not read: arg replaces it.)
 *
 * XML_ERR_BAD_ARG: a NULL array or entry (query, qn, cn, mask, arg, dq, l), NULL dscores, n_mod outside 1..2, ld_ds < nv,
 * ld_arg < nv.  XML_ERR_UNSUPPORTED: what xml_q2c_scores_l2norm_bwd_supported(nq, nv, l[m], hidden, dt) refuses.
 * --------------------------------------------------------------------------------------------- */
int xml_q2c_scores_arg_bwd_q(int n_mod, const void* const* query, const void* const* qn, const void* const* cn,
                             const float* const* mask, const float* dscores, int64_t ld_ds, float scale, void* const* dq,
                             int nq, int nv, const int* l, int hidden, const int32_t* const* arg, int64_t ld_arg, int dt,
                             xml_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * xml_pair_sim_bwd_q: the query gradient of xml_pair_sim alone, dq[b, :] = sum over c, in the clip order of
 * xml_pair_sim_bwd, of dsim[b, c] f2[b, c, :], without df2.  f2 (n, l, hidden) dt, dsim (n, l) f32,
 * dq (n, hidden) dt, every element written.
 * XML_ERR_BAD_ARG: a NULL operand, n / l / hidden <= 0, dt other than XML_F32 / XML_BF16.
 * XML_ERR_UNSUPPORTED: hidden % 8 != 0 or hidden > 2048.
 * --------------------------------------------------------------------------------------------- */
int xml_pair_sim_bwd_q(const void* f2, const float* dsim, void* dq, int64_t n, int l, int hidden, int dt,
                       xml_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* XMLHIP_TRAIN_INDEX_H */
