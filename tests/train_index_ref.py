"""The float64 statement of train_index.xml_forward_train_index -- TEST INFRASTRUCTURE: the query branch of the model in
float64 (oracle/f64.py: K1 + K2, the query encoder, train_modular_pool), then q2c_scores on the ALREADY normalised rows the
index holds, train_pair_sim, train_span_loss and train_rank_loss, with plain float64 autograd for the query-side gradients.

The context operands are the index's own rows (index.feat1n_rows(m), index.feat2[m], index.mask[m]) of the batch's slots, the
first `length` clips, with the rows at or beyond a video's valid length (index.vlen) zero and masked -- the contract of
xml_index_gather_video_rows, and how K7 treats them at search time."""
import torch
import torch.nn.functional as F

from oracle import f64

QUERY_SIDE = ("query_input_proj.", "query_pos_embed.", "query_encoder.", "modular_vector_mapping.", "video_query_linear.",
              "sub_query_linear.", "video_st_predictor.", "video_ed_predictor.", "sub_st_predictor.", "sub_ed_predictor.",
              "merged_st_predictor.", "merged_ed_predictor.")


def index_rows(index, slots, length):
    """-> {modality: (cn, f2, mask)} float64 CPU tensors (n, length, H) x 2 and (n, length) of the batch's slots; a slot
    outside [0, n_videos) is an empty example."""
    slots = torch.as_tensor(slots, dtype=torch.long)
    ok = (slots >= 0) & (slots < index.n_videos)
    sl = slots.clamp(0, index.n_videos - 1).to(index.device)
    vlen = (index.vlen if index.vlen is not None else torch.full((index.n_videos,), index.l_ref, device=index.device))[sl].cpu()
    keep = ((torch.arange(length)[None, :] < vlen[:, None]) & ok[:, None]).double()
    out = {}
    for m in index.modalities:
        cn = index.feat1n_rows(m)[sl, :length].cpu().double() * keep[:, :, None]
        f2 = index.feat2[m][sl, :length].cpu().double() * keep[:, :, None]
        out[m] = (cn, f2, index.mask[m][sl, :length].cpu().double() * keep)
    return out


def forward64(model, ctx, query_feat, query_mask, st_ed, ranks_ctx, ranks_q):
    """-> (terms: dict of float64 0-d tensors loss_st_ed / loss_neg_ctx / loss_neg_q (weighted) / loss_overall, scores (N, N),
    sims list, grads: {query-side parameter name: float64 gradient of loss_overall})."""
    cfg = model.config
    sd = {k: v.detach().cpu().double().requires_grad_(k.startswith(QUERY_SIDE)) for k, v in model.named_parameters()}
    w = f64.Weights64(sd)
    qm = query_mask.detach().cpu().double()
    x = f64.linear_ln_relu_pos(query_feat.detach().cpu().double(), w.sub("query_input_proj"), w.sub("query_pos_embed"))
    enc = f64.bert_attention(x, qm.unsqueeze(1), w.sub("query_encoder"), cfg.n_heads)
    mq = f64.train_modular_pool(enc, qm, w["modular_vector_mapping.weight"])
    names = [n for n in ("video", "sub") if n in ctx]
    qs = dict(zip(names, mq.unbind(0)))
    zero = torch.zeros((), dtype=torch.float64)
    span = zero
    sims = []
    if cfg.lw_st_ed != 0:
        for n in names:
            lin = w.sub(n + "_query_linear")
            sims.append(f64.train_pair_sim(F.linear(qs[n], lin["weight"], lin["bias"]), ctx[n][1]))
        merged = bool(cfg.merge_two_stream and len(names) == 2)
        if merged:
            masks, filters = [ctx["video"][2]] * 2, [w["merged_st_predictor.weight"], w["merged_ed_predictor.weight"]]
        else:
            masks = [ctx[n][2] for n in names]
            filters = [w[n + "_st_predictor.weight"] for n in names] + [w[n + "_ed_predictor.weight"] for n in names]
        span = f64.train_span_loss(sims, filters, masks, st_ed.detach().cpu().long(), merged, cfg.conv_kernel_size)
    scores = sum(f64.q2c_scores(F.normalize(qs[n], dim=-1), ctx[n][0], ctx[n][2])[0] for n in names) / len(names)
    rank = f64.train_rank_loss(scores, torch.as_tensor(ranks_ctx), torch.as_tensor(ranks_q), float(cfg.margin),
                               cfg.ranking_loss_type == "lse")
    terms = dict(loss_st_ed=cfg.lw_st_ed * span, loss_neg_ctx=cfg.lw_neg_ctx * rank[0], loss_neg_q=cfg.lw_neg_q * rank[1])
    terms["loss_overall"] = terms["loss_st_ed"] + terms["loss_neg_ctx"] + terms["loss_neg_q"]
    terms["loss_overall"].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items() if v.requires_grad}
    return {k: v.detach() for k, v in terms.items()}, scores.detach(), [s.detach() for s in sims], grads
