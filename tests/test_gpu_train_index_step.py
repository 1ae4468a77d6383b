"""The training step on a resident index (tvretrieval_amd/train_index.py) end to end: video_sub model, H = 128, 4 heads,
dropout off (eval mode), batch 5, 7 query tokens, an index of 8 ragged videos at l_ref = 24 (row-major K6 operand) and at
l_ref = 128 (block images: fixed, length-bucketed, the plain updatable index and the packed one, tiles=N, with a run across
blocks 7 | 8), f32 and bf16, merged / hinge and unmerged / lse.  (The tiled K6 kernel takes rows of 384 bytes and more: the
bf16 model of the l_ref = 128 cases has H = 256, as in tests/test_gpu_index_packed.py; every other case H = 128.)

(a) loss terms and every query-side gradient against the float64 statement tests/train_index_ref.py on the rows the index
    holds.  f32: the bounds of tests/test_gpu_train.py for the same terms -- |span term| 5e-5, |rank terms| 2e-5, every parameter
    gradient within 5e-4 of max(max|ref|, floor) (test_golden_train_steps_fp32; the floor: see the test).  bf16: the yardstick of
    test_c5_shape_bf16_gradients_vs_fp32 -- loss terms within 2 %, and for every tensor that carries a real gradient
    (norm >= 1e-4 of the largest) cosine >= 0.97 and a norm within 10 %.  The context side is absent from the optimizer and
    bit-identical after a step.
(b) three GraphedTrainStep replays against three eager steps with injected negatives (f32): per-step losses within 5e-5 and the
    parameters after the third step within 2e-5, what test_graphed_train_step_reproduces_the_reference_steps requires.
(c) every tensor of the index is bit-identical after the steps; (d) vcmr_search on the same index with the fine-tuned model
    equals, list for list, the search of a fresh model loaded from its state_dict.
No parts or chain index is made in this module."""
import numpy as np
import pytest
import torch

import train_index_ref as R
from test_gpu_kernels import DEV
from test_gpu_model import _feats, _synthetic_model

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
H, DV, DS, DQ, BSZ, LQ = 128, 256, 128, 128, 5, 7
LENS = {24: [24, 5, 17, 16, 1, 9, 20, 12], 128: [128, 40, 100, 16, 17, 64, 90, 1]}
FORMS = [("oneshot", 24), ("mutable", 24), ("plan", 128), ("fixed", 128), ("mutable", 128), ("tiles", 128)]
IDS = [100 + i for i in range(8)]
BATCH_VIDEOS = [5, 6, 2, 7, 3]                 # index positions of the batch's videos (5: the run across 7 | 8 when packed)
SEARCH_KEYS = ("top_scores", "top_indices", "flat_scores", "flat_indices")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def make_index(m, form, l_ref):
    from tvretrieval_amd import inference, ops
    from tvretrieval_amd.index_update import MutableCorpusIndex
    lens = LENS[l_ref]
    vf, vm = _feats(len(lens), lens, DV, 11)
    sf, sm = _feats(len(lens), lens, DS, 12)
    batch = tuple(t.to(DEV) for t in (vf, vm, sf, sm))
    with torch.no_grad():
        if form in ("oneshot", "plan", "fixed"):
            index = inference.build_corpus_index(m, [batch], length_buckets=form != "fixed")
            row_of = {"v%d" % i: i for i in range(len(lens))}
        else:
            index = MutableCorpusIndex.create(m, 10, l_ref, tiles=4 if form == "tiles" else None)
            index.add(*batch, ids=IDS, n_clips=list(lens) if form == "tiles" else None)
            row_of = lambda name: index.slot_of(IDS[int(name[1:])])          # noqa: E731
    tiled = isinstance(index.feat1n["video"], ops.TiledRows)
    assert index.l_ref == l_ref and tiled == (l_ref == 128)
    if form == "plan":
        assert index.feat1n["video"].plan is not None
    if form == "fixed":
        assert index.feat1n["video"].plan is None
    if form == "tiles":
        first, nb = index.blocks.run_of(index.slot_of(IDS[5]))
        assert first % 16 < 8 < first % 16 + nb, "the batch holds a run across blocks 7 | 8"
    return index, row_of, lens


def make_store(tmp_path, index, row_of, lens, model):
    from tvretrieval_amd import ingest
    from tvretrieval_amd import train_index as TI
    g = np.random.default_rng(3)
    qlens = [LQ, 3, 5, 1, 6, 4]
    videos = BATCH_VIDEOS + [1]
    feats, examples = {}, []
    for i, (v, ql) in enumerate(zip(videos, qlens)):
        feats[str(900 + i)] = g.standard_normal((ql, DQ)).astype(np.float32)
        st = float(g.integers(0, lens[v])) * 1.5
        ed = min(st + 1.5 * float(g.integers(1, 4)), lens[v] * 1.5)
        examples.append(dict(desc_id=900 + i, vid_name="v%d" % v, ts=[st, ed], duration=lens[v] * 1.5))
    ingest.write_feature_store(str(tmp_path / "desc"), feats, dtype="float32")
    store = TI.IndexTrainStore(examples, ingest.FeatureStore(str(tmp_path / "desc")), index, row_of, max_desc_len=LQ,
                               max_ctx_len=index.l_ref, model=model)
    return store, examples


def setup(tmp_path, dtype, form, l_ref, merged, lse, seed=60):
    m, cfg = _synthetic_model("video_sub", 256 if (dtype == BF16 and l_ref == 128) else H, DV, DS, DQ, l_ref, dtype, seed=seed,
                              merge=merged)
    m.config.ranking_loss_type = "lse" if lse else "hinge"
    m.config.lw_st_ed = 1.0
    index, row_of, lens = make_index(m, form, l_ref)
    store, examples = make_store(tmp_path, index, row_of, lens, m)
    return m, cfg, index, store


def index_tensors(index):
    """name -> every device tensor the index holds (the K6 images through TiledRows.data)."""
    out = {}
    for k, v in vars(index).items():
        for kk, t in (v.items() if isinstance(v, dict) else [("", v)]):
            t = getattr(t, "data", t) if not torch.is_tensor(t) else t
            if torch.is_tensor(t) and t.is_cuda:
                out["%s/%s" % (k, kk)] = t
    return out


RANKS = [([1, 2, 3, 4, 1], [2, 1, 4, 3, 2]), ([4, 4, 1, 2, 3], [1, 3, 2, 1, 4]), ([2, 3, 4, 1, 2], [3, 4, 1, 2, 1])]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,l_ref,merged,lse", [FORMS[0] + (True, False), FORMS[0] + (False, True)] +
                         [f + (i % 2 == 0, i % 2 == 1) for i, f in enumerate(FORMS[1:])],
                         ids=lambda v: str(v))
def test_losses_and_query_gradients_against_float64(tmp_path, dtype, form, l_ref, merged, lse):
    from tvretrieval_amd import train_index as TI
    from tvretrieval_amd.train import BertAdam
    m, cfg, index, store = setup(tmp_path, dtype, form, l_ref, merged, lse)
    params = TI.query_side_parameters(m)
    opt = BertAdam(params, lr=1e-3, warmup=-1, t_total=-1, schedule="none")
    q_named, c_named = TI.split_parameters(m)
    assert {id(p) for p in opt.params} == {id(p) for _, p in q_named} and not {id(p) for p in opt.params} & {id(p) for _, p in c_named}
    ids = [0, 1, 2, 3, 4]
    batch = store.batch(ids)
    assert sorted(batch) == ["ctx_first_block", "ctx_len", "ctx_slots", "query_feat", "query_mask", "st_ed_indices"]
    assert batch["ctx_slots"].dtype == batch["ctx_first_block"].dtype == torch.int32
    assert batch["ctx_len"] == max(LENS[l_ref][v] for v in BATCH_VIDEOS) and batch["query_feat"].shape == (BSZ, LQ, DQ)
    assert (batch["st_ed_indices"].cpu().numpy() == store.labels_host[ids]).all()
    slots = batch["ctx_slots"].cpu().numpy()
    assert (slots == store.slots_host[ids]).all() and (batch["ctx_first_block"].cpu().numpy() == store.first_block_host[ids]).all()
    before_ctx = {n: p.detach().clone() for n, p in c_named}
    before_idx = {k: t.clone() for k, t in index_tensors(index).items()}
    rc, rq = RANKS[0]
    loss, parts = TI.xml_forward_train_index(m, index, neg_ctx_rank=rc, neg_q_rank=rq, **batch)
    opt.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    # the float64 statement, on the rows the index holds
    ctx = R.index_rows(index, slots, batch["ctx_len"])
    assert all(float(ctx[k][2].sum()) > 0 for k in ctx)
    terms, _, _, grads = R.forward64(m, ctx, batch["query_feat"], batch["query_mask"], batch["st_ed_indices"], rc, rq)
    print("LOSSES %s %s: kernel %s float64 %s" % (form, dtype, {k: round(v, 6) for k, v in parts.items()},
                                                  {k: round(float(v), 6) for k, v in terms.items()}))
    assert abs(float(loss.detach()) - parts["loss_overall"]) < 1e-6 and float(terms["loss_st_ed"]) > 0 and float(terms["loss_overall"]) > 0
    for k, tol in (("loss_st_ed", 5e-5), ("loss_neg_ctx", 2e-5), ("loss_neg_q", 2e-5)):
        a, b = parts[k], float(terms[k])
        if dtype == F32:
            assert abs(a - b) < tol, (k, a, b)
        else:
            assert abs(a - b) <= 2e-2 * max(abs(b), 1e-3), (k, a, b)
    got = {n: p.grad.detach().double().cpu() for n, p in q_named}
    assert set(got) == set(grads)
    if dtype == F32:
        # key biases have an analytically ZERO gradient (softmax is shift invariant): both sides hold rounding noise there,
        # hence the floor.  test_golden_train_steps_fp32 states it as 1e-4 absolute at steps whose largest gradient element is
        # 0.118 and 2.87 (tests/golden/train_step_*.npz); the noise scales with the gradients that flow through the node, so
        # here -- the span loss unweighted -- it is the stricter of the two as a share of the largest element: 1e-4 / 2.87
        gtop = max(float(v.abs().max()) for v in grads.values())
        floor = 1e-4 / 2.87 * gtop
        worst = sorted(((float((got[n] - grads[n]).abs().max()) / max(float(grads[n].abs().max()), floor), n) for n in grads), reverse=True)
        print("largest gradient element %.3e, floor %.3e; worst gradient errors:" % (gtop, floor), worst[:4])
        assert worst[0][0] < 5e-4, worst[:5]
    else:
        gmax = max(float(v.norm()) for v in grads.values())
        rows = []
        for n, gf in grads.items():
            nf, nb = float(gf.norm()), float(got[n].norm())
            if nf < 1e-4 * gmax:
                continue
            rows.append((float((gf * got[n]).sum()) / (nf * nb + 1e-30), nb / nf, n))
        rows.sort()
        print("bf16 vs float64 gradients: worst cosine %.4f (%s), norm ratio %.3f..%.3f over %d tensors"
              % (rows[0][0], rows[0][2], min(r[1] for r in rows), max(r[1] for r in rows), len(rows)))
        assert len(rows) > 10 and rows[0][0] >= 0.97, rows[:5]
        assert all(0.9 <= r[1] <= 1.1 for r in rows), sorted(rows, key=lambda r: abs(r[1] - 1))[-5:]
    assert max(float(g.abs().max()) for g in got.values()) > 0
    # the context side: no gradient, not in the optimizer, the same bits after a step; the index untouched
    assert all(p.grad is None for _, p in c_named)
    moved_from = {n: p.detach().clone() for n, p in q_named}
    opt.step()
    torch.cuda.synchronize()
    for n, p in c_named:
        assert torch.equal(_bits(p.detach()), _bits(before_ctx[n])), n
    assert any(not torch.equal(p.detach(), moved_from[n]) for n, p in q_named)
    for k, t in index_tensors(index).items():
        assert torch.equal(t.view(torch.uint8), before_idx[k].view(torch.uint8)), k


@pytest.mark.parametrize("form,l_ref", [FORMS[0], FORMS[5]], ids=lambda v: str(v))
def test_graphed_replays_against_eager_steps(tmp_path, form, l_ref):
    from tvretrieval_amd import train_index as TI
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep, train_step
    runs = []
    for graphed in (False, True):
        (tmp_path / str(graphed)).mkdir()
        m, cfg, index, store = setup(tmp_path / str(graphed), F32, form, l_ref, True, False)
        opt = BertAdam(TI.query_side_parameters(m), lr=5e-4, warmup=-1, t_total=-1, schedule="none")
        batch = dict(store.batch([0, 1, 2, 3, 4], lmax=l_ref, lq=LQ), index=index)
        losses = []
        if graphed:
            before = opt.flat_p.clone()
            step = GraphedTrainStep(m, opt, batch, forward=TI.xml_forward_train_index)
            assert torch.equal(opt.flat_p, before) and opt.step_count == 0
            assert step.static["index"] is index and step.static["ctx_slots"].dtype == torch.int32
            assert not any(k.startswith(("video_", "sub_")) for k in step.static)
            store.fill(step.static, [4, 3, 2, 1, 0])            # another batch through the static buffers, then this one again
            store.fill(step.static, [0, 1, 2, 3, 4])
            for k in ("query_feat", "query_mask", "ctx_slots", "ctx_first_block", "st_ed_indices"):
                assert torch.equal(step.static[k], batch[k]), k
        for rc, rq in RANKS:
            if graphed:
                loss, parts = step(None, neg_ctx_rank=rc, neg_q_rank=rq)
                assert abs(float(parts["loss_overall"]) - float(loss)) < 1e-6
            else:
                loss, parts = train_step(m, opt, dict(batch, neg_ctx_rank=rc, neg_q_rank=rq), forward=TI.xml_forward_train_index)
            losses.append(float(loss))
        assert opt.step_count == 3
        runs.append((losses, {n: p.detach().cpu().clone() for n, p in m.named_parameters()}))
    (l0, p0), (l1, p1) = runs
    print("eager", l0, "graphed", l1)
    for a, b in zip(l0, l1):
        assert abs(a - b) < 5e-5, (l0, l1)
    assert len({round(x, 5) for x in l0}) == 3
    worst = max(float((p0[n] - p1[n]).abs().max()) for n in p0)
    assert worst < 2e-5, worst


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,l_ref", [FORMS[0], FORMS[2], FORMS[4], FORMS[5]], ids=lambda v: str(v))
def test_index_untouched_and_search_with_the_fine_tuned_model(tmp_path, dtype, form, l_ref):
    from tvretrieval_amd import inference, train_index as TI
    from tvretrieval_amd.model_xml import XML
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep
    m, cfg, index, store = setup(tmp_path, dtype, form, l_ref, True, False)
    qf, qm = (t.to(DEV) for t in _feats(6, [LQ, 3, 5, 1, 6, 4], DQ, 21))
    kw = dict(max_vcmr_video=4, max_before_nms=20)
    with torch.no_grad():
        first = inference.vcmr_search(m, index, qf, qm, **kw)       # fills the packed-weight caches a step must invalidate
    first = {k: first[k].clone() for k in SEARCH_KEYS}
    before_idx = {k: t.clone() for k, t in index_tensors(index).items()}
    assert len(before_idx) >= 7
    opt = BertAdam(TI.query_side_parameters(m), lr=2e-2, warmup=-1, t_total=-1, schedule="none")
    step = GraphedTrainStep(m, opt, dict(store.batch([0, 1, 2, 3, 4], lmax=l_ref, lq=LQ), index=index),
                            forward=TI.xml_forward_train_index)
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    for rc, rq in RANKS:
        store.fill(step.static, [0, 1, 2, 3, 4])
        step(None, neg_ctx_rank=rc, neg_q_rank=rq)
    if form == "tiles":                                        # compact() moves runs; the store follows, the step goes on
        index.remove(ids=[IDS[4]])
        store.refresh()
        index.compact()
        store.fill(step.static, [0, 1, 2, 3, 4])
        fb = [index.blocks.run_of(int(s))[0] for s in store.slots_host[:5]]
        assert step.static["ctx_first_block"].cpu().tolist() == fb
        before_idx = {k: t.clone() for k, t in index_tensors(index).items()}
        step(None, neg_ctx_rank=RANKS[0][0], neg_q_rank=RANKS[0][1])
    torch.cuda.synchronize()
    for k, t in index_tensors(index).items():
        assert torch.equal(t.view(torch.uint8), before_idx[k].view(torch.uint8)), k
    q_named, c_named = TI.split_parameters(m)
    assert all(torch.equal(_bits(p.detach()), _bits(start[n])) for n, p in c_named)
    assert sum(not torch.equal(p.detach(), start[n]) for n, p in q_named) > 10
    fresh = XML(cfg, compute_dtype=dtype)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        got = inference.vcmr_search(m, index, qf, qm, **kw)
        want = inference.vcmr_search(fresh, index, qf, qm, **kw)
    for k in SEARCH_KEYS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    if form != "tiles":
        assert any(not torch.equal(_bits(got[k]), _bits(first[k])) for k in SEARCH_KEYS), "the steps changed no list"


def test_train_epoch_index_eager_and_graphed(tmp_path):
    """train_epoch_index over the six examples in two batches of three: fill + replay of a captured step against the eager
    loop at each batch's own length, same order, same negatives (the CPU generator is seeded alike) -- the averaged loss terms
    within the 5e-5 of (b); and an evaluation pass (training=False) leaves the parameters alone."""
    import types
    from tvretrieval_amd import train_index as TI
    from tvretrieval_amd.train import BertAdam, GraphedTrainStep
    opt_ns = types.SimpleNamespace(bsz=3, grad_clip=-1, debug=False, hard_negtiave_start_epoch=-1, hard_pool_size=20,
                                   train_span_start_epoch=-1, lw_st_ed=1.0)
    order = np.asarray([0, 1, 2, 3, 4, 5])
    got = []
    for graphed in (False, True):
        (tmp_path / str(graphed)).mkdir()
        m, cfg, index, store = setup(tmp_path / str(graphed), F32, "oneshot", 24, True, False)
        for mod in m.modules():                                 # the epoch driver switches to train mode: dropout 0 by p
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        opt = BertAdam(TI.query_side_parameters(m), lr=5e-4, warmup=-1, t_total=-1, schedule="none")
        step = None
        if graphed:
            step = GraphedTrainStep(m, opt, dict(store.batch([0, 1, 2], lmax=24, lq=LQ), index=index),
                                    forward=TI.xml_forward_train_index)
        torch.manual_seed(11)
        history = []
        got.append((TI.train_epoch_index(m, opt, store, opt_ns, 0, step=step, order=order, history=history), history))
        assert opt.step_count == 2 and len(history) == 2
        before = opt.flat_p.clone()
        val = TI.train_epoch_index(m, opt, store, opt_ns, 1, training=False, order=order)
        assert torch.equal(opt.flat_p, before) and opt.step_count == 2 and val["loss_overall"] > 0
        m.eval()
    (avg0, h0), (avg1, h1) = got
    print("eager", h0, "graphed", h1)
    for a, b in zip(h0 + [avg0], h1 + [avg1]):
        for k in a:
            assert abs(a[k] - b[k]) < 5e-5, (k, a, b)
