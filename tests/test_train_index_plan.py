"""Host side of training on a resident index (tvretrieval_amd/train_index.py) without a GPU: the split of the model's
parameters, the slot -> first block tables of the three block images against subset.VideoSubset._plan's sources, every
refusal with its reason, staleness of an IndexTrainStore after updates of the index and after compact().

The indexes are DESCRIPTIONS: inference.CorpusIndex objects over small CPU tensors with the K6 operand an ops.TiledRows whose
image is never read here; the updatable ones carry the SlotTable / BlockTable / version an index_update.MutableCorpusIndex
carries and are driven through the same table calls its add / replace / remove / compact make."""
import numpy as np
import pytest
import torch

from test_train_store import load_collate_fixture
from tvretrieval_amd import inference, ops, subset
from tvretrieval_amd import train_data as td
from tvretrieval_amd import train_index as TI
from tvretrieval_amd.index_update import BlockTable, SlotTable, _TablePlan, blocks_of
from tvretrieval_amd.model_xml import XML, xml_base_config

H, L_REF = 128, 100
LENS = [7, 1, 44, 40, 23]                      # clips of vid_0 .. vid_4 of tests/golden/train_collate.npz


def _model(ctx_mode="video_sub", cross=True, merge=True, dtype=torch.bfloat16, hidden=H):
    cfg = dict(xml_base_config)
    cfg.update(visual_input_size=32, sub_input_size=32, query_input_size=32, hidden_size=hidden, max_ctx_l=L_REF, max_desc_l=30,
               ctx_mode=ctx_mode, cross_att=cross and ctx_mode == "video_sub", merge_two_stream=merge and ctx_mode == "video_sub")
    return XML(cfg, compute_dtype=dtype)


# ---- the parameter split ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx_mode,cross,merge", [("video_sub", True, True), ("video_sub", False, True), ("video_sub", True, False),
                                                  ("video_sub", False, False), ("video", False, False), ("sub", False, False)])
def test_query_side_parameters_split_the_model(ctx_mode, cross, merge):
    m = _model(ctx_mode, cross, merge)
    named = dict(m.named_parameters())
    q, c = TI.split_parameters(m)
    assert not {n for n, _ in q} & {n for n, _ in c} and {n for n, _ in q} | {n for n, _ in c} == set(named)
    assert [n for n, _ in q] + [n for n, _ in c] != [] and len(q) + len(c) == len(named)
    mods = [x for x in ("video", "sub") if x in ctx_mode]
    want_q = {"query_input_proj", "query_pos_embed", "query_encoder", "modular_vector_mapping"} | {x + "_query_linear" for x in mods}
    want_q |= {"merged_st_predictor", "merged_ed_predictor"} if (merge and ctx_mode == "video_sub") else \
        {x + s for x in mods for s in ("_st_predictor", "_ed_predictor")}
    want_c = {"ctx_pos_embed"} | {x + s for x in mods for s in ("_input_proj", "_encoder1", "_encoder2")}
    want_c |= {x + s for x in mods for s in (("_cross_att", "_cross_layernorm") if (cross and ctx_mode == "video_sub") else
                                             ("_encoder3",))}
    assert {n.split(".")[0] for n, _ in q} == want_q and {n.split(".")[0] for n, _ in c} == want_c
    assert all(p.requires_grad for p in named.values())
    got = TI.query_side_parameters(m)
    assert [id(p) for p in got] == [id(p) for _, p in q]
    assert all(p.requires_grad for _, p in q) and not any(p.requires_grad for _, p in c)
    assert TI.QUERY_SIDE == __import__("train_index_ref").QUERY_SIDE           # the float64 statement differentiates the same set


# ---- index descriptions -----------------------------------------------------------------------------------------------------
def _describe(lens, form, dtype=torch.bfloat16, hidden=H, l_ref=L_REF, mods=("video", "sub"), tiles=3, **kw):
    """form: rows | fixed | plan | packed (an updatable index, every slot free) | slots (updatable, row-major)."""
    nv = len(lens)
    lpad = 128 if form in ("fixed", "plan", "packed") else (l_ref + 15) // 16 * 16
    mask = (torch.arange(lpad)[None, :] < torch.as_tensor(lens)[:, None]).float()
    if form in ("packed", "slots"):
        mask = torch.zeros_like(mask)
    plan = ops.PackPlan([mask]) if form == "plan" else None
    blocks = BlockTable(tiles) if form == "packed" else None
    if blocks is not None:
        plan = _TablePlan(blocks, torch.full((2 * tiles, 8), -2, dtype=torch.int32), nv)
    feat1n = {}
    for m in mods:
        if form in ("rows", "slots"):
            feat1n[m] = torch.zeros((nv, lpad, hidden), dtype=dtype)
            continue
        rows = nv * 128 if form == "fixed" else plan.n_tiles * 256
        t = ops.TiledRows(torch.zeros((rows + 255) // 256 * 256 * hidden, dtype=dtype), nv * 128, hidden, (nv, 128, hidden))
        t.mask_bits, t.plan = torch.zeros((nv, 4), dtype=torch.int32), plan
        feat1n[m] = t
    index = inference.CorpusIndex(list(mods), feat1n, {m: torch.zeros((nv, lpad, hidden), dtype=dtype) for m in mods},
                                  {m: mask.clone() for m in mods}, l_ref, **kw)
    index.set_valid_lengths()
    if form in ("packed", "slots"):
        index.blocks, index.table, index.version = blocks, SlotTable(nv), 0
        index.live = torch.zeros((1, (nv + 31) // 32), dtype=torch.int32)
        index.slot_of = index.table.slot_of
    return index


def _put(index, slots, ids, lens):
    """The host half of MutableCorpusIndex.add / replace: tables, masks, version."""
    slots, ids = index.table.check_put(slots, ids)
    if index.blocks is not None:
        runs, _ = index.blocks.check_put(slots, [blocks_of(n) for n in lens])
        index.blocks.commit_put(slots, runs)
    index.table.commit_put(slots, ids)
    for s, n in zip(slots, lens):
        for m in index.modalities:
            index.mask[m][s] = (torch.arange(index.lpad) < n).float()
    index.version += 1


def _remove(index, slots):
    if index.blocks is not None:
        index.blocks.check_remove(slots)
        index.blocks.commit_remove(slots)
    index.table.commit_remove(slots)
    for m in index.modalities:
        index.mask[m][slots] = 0
    index.version += 1


def _view_sources(index, form, members):
    """The first source block of every member as subset.VideoSubset._plan hands it to place_members."""
    view = object.__new__(subset.VideoSubset)
    view.index, view.form = index, form
    src_block, _, firsts = view._plan(np.asarray(members, dtype=np.int64), None, None)
    return src_block[firsts].astype(np.int64)


_FIXTURE = {}


def _store(tmp_path, index, row_of, model=None, **kw):
    if tmp_path not in _FIXTURE:
        _FIXTURE[tmp_path] = load_collate_fixture(tmp_path)
    z, examples, st = _FIXTURE[tmp_path]
    a = dict(max_desc_len=int(z["max_desc_len"]), max_ctx_len=L_REF, clip_length=float(z["clip_length"]), device="cpu", model=model)
    a.update(kw)
    return TI.IndexTrainStore(examples, st["desc"], index, row_of, **a), examples, st


ROW_OF = {"vid_%d" % i: i for i in range(len(LENS))}


@pytest.mark.parametrize("form", ["fixed", "plan"])
def test_first_blocks_of_the_one_shot_images_are_the_views_sources(tmp_path, form):
    lens = LENS + [128, 16, 17, 64, 65, 100, 3, 90]
    index = _describe(lens, form)
    assert TI.index_form(_model(), index) == form
    store, examples, st = _store(tmp_path, index, ROW_OF)
    slots = np.asarray([ROW_OF[e["vid_name"]] for e in examples])
    assert (store.slots_host == slots).all()
    assert (store.first_block_host == _view_sources(index, form, np.unique(slots))[np.searchsorted(np.unique(slots), slots)]).all()
    every = np.arange(len(lens))
    assert (store.first_blocks(every) == _view_sources(index, form, every)).all()
    if form == "fixed":
        assert (store.first_blocks(every) == 8 * every).all()
    else:
        rm = index.feat1n["video"].plan.row_map.numpy()
        assert (rm[store.first_blocks(every) * 16] == every * 128).all()           # row 0 of every video by the plan's own map
    assert (store._ctx.numpy() == np.stack([slots + 1, store.first_block_host + 1], 1)).all()
    # the labels are plan_examples' on the index's own clip counts: those of a DeviceTrainStore over the raw stores
    _, ctx_len, labels = td.plan_examples(examples, st["desc"], st["video"], st["sub"], "tvr", store.max_desc_len, L_REF, 1.5, "video_sub")
    assert (store.labels_host == labels).all() and (store.ctx_len == ctx_len).all() and store.labels.dtype == torch.int64
    assert not store.stale


def test_packed_index_staleness_and_compaction(tmp_path):
    index = _describe([0] * 12, "packed", tiles=3)
    ids = [50, 51, 52, 53, 54]
    id_of = {"vid_%d" % i: ids[i] for i in range(5)}
    row_of = lambda name: index.slot_of(id_of[name])            # noqa: E731
    with pytest.raises(ValueError, match=r"example 0: video vid_0 is not live in the index \(9 such examples\)"):
        _store(tmp_path, index, row_of)
    _put(index, [0, 1, 2], [90, 91, 92], [100, 70, 40])       # fillers in front: the videos do not start at block 0
    _put(index, [3, 4, 5, 6, 7], ids, LENS)
    assert TI.index_form(_model(), index) == "packed"
    store, examples, _ = _store(tmp_path, index, row_of)
    slots = np.asarray([index.slot_of(id_of[e["vid_name"]]) for e in examples])

    def check():
        fb = np.asarray([index.blocks.run_of(int(s))[0] for s in slots])
        assert (store.slots_host == slots).all() and (store.first_block_host == fb).all()
        assert (store._ctx.numpy() == np.stack([slots + 1, fb + 1], 1)).all()
        live = np.unique(slots)
        assert (store.first_blocks(live) == _view_sources(index, "packed", live)).all()
        return fb
    before = check()
    assert not store.stale
    store._check_fresh()
    # remove -> stale until refresh; the removed filler is no example's video, so refresh succeeds
    _remove(index, [1])
    assert store.stale
    for call in (lambda: store.batch([0, 1]), lambda: store.fill({}, [0, 1])):
        with pytest.raises(ValueError, match="stale: the index was updated .* call store.refresh\\(\\)"):
            call()
    assert store.refresh() is store and not store.stale
    check()
    # add -> stale; replace (a video of the store moves to a longer run) -> stale, and the refreshed labels follow its length
    _put(index, [1], [93], [30])
    assert store.stale and not store.refresh().stale
    old = store.labels_host.copy()
    _put(index, [5], [ids[2]], [20])                           # vid_2: 44 -> 20 clips
    assert store.stale and not store.refresh().stale
    check()
    ex2 = [i for i, e in enumerate(examples) if e["vid_name"] == "vid_2"]
    assert (store.labels_host[ex2] <= 19).all() and (np.delete(store.labels_host, ex2, 0) == np.delete(old, ex2, 0)).all()
    assert store.ctx_len[ex2[0]] == 20
    # a removed video of the store: refresh names it
    _remove(index, [3])
    with pytest.raises(ValueError, match="video vid_0 is not live"):
        store.refresh()
    _put(index, [3], [ids[0]], [LENS[0]])
    store.refresh()
    # compact(): the version stays, runs move, and the table a batch gathers from carries the moved runs' first blocks
    _remove(index, [0])
    store.refresh()
    before, version = check(), index.version
    plan = index.blocks.check_compact()
    assert any(rnd["moves"] for rnd in plan), "the removed filler left a hole in front of the videos"
    index.blocks.commit_compact(plan)
    assert index.version == version and not store.stale and index.blocks.compactions == sum(bool(r["moves"]) for r in plan)
    assert (store.first_block_host == before).all()            # not yet looked at
    store._check_fresh()                                       # what batch() and fill() call first
    after = check()
    assert (after != before).any()
    store._check_fresh()
    assert store._compactions == index.blocks.compactions


def test_row_major_and_plain_updatable_indexes(tmp_path):
    index = _describe(LENS + [9], "rows")
    assert TI.index_form(_model(), index) == "rows"
    store, examples, _ = _store(tmp_path, index, lambda name: ROW_OF[name])
    assert (store.first_block_host == 0).all() and store._compactions is None
    slots = _describe([0] * 8, "slots")
    _put(slots, [2, 3, 4, 5, 6], [7, 8, 9, 10, 11], LENS)
    store2, _, _ = _store(tmp_path, slots, lambda name: slots.slot_of(7 + ROW_OF[name]))
    assert (store2.slots_host == np.asarray([2 + ROW_OF[e["vid_name"]] for e in examples])).all()
    _put(slots, [0], [30], [5])
    assert store2.stale and not store2.refresh().stale


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(tmp_path):
    m = _model()
    ok = _describe(LENS, "fixed")
    assert TI.index_form(m, ok) == "fixed"
    exact = _describe(LENS, "fixed"); exact.exact = object()
    parts = _describe(LENS, "fixed"); parts.fold = object()
    shard = _describe(LENS, "fixed", video_offset=5, n_total=100)
    shard2 = _describe(LENS, "fixed", n_total=100)
    f32 = _describe(LENS, "fixed", dtype=torch.float32)
    one = _describe(LENS, "fixed", mods=("video",))
    floats = _describe(LENS, "fixed")
    for t in floats.feat1n.values():
        t.mask_bits = None
    m16 = _model(dtype=ops.F16S)
    cases = [(m, exact, "an exact-rank index"), (m16, f32, "an ops.F16S model is inference-only"), (m, parts, "a parts or chain index"),
             (m, shard, "a corpus shard"), (m, shard2, "a corpus shard"), (m, f32, "the model computes torch.bfloat16 rows"),
             (_model(dtype=torch.float32), ok, "the model computes torch.float32 rows"), (m, one, r"the index holds .* rows for \['video'\]"),
             (m, floats, "float, non-binary clip masks \\(modality video\\) on a block image")]
    for model, index, why in cases:
        with pytest.raises(ValueError, match="training on a resident index: .*" + why):
            TI.index_form(model, index)
        with pytest.raises(ValueError, match=why):
            TI.xml_forward_train_index(model, index, None, None, None, None, None)      # before anything is touched
        with pytest.raises(ValueError, match=why):
            _store(tmp_path, index, ROW_OF, model=model)
    floats_rows = _describe(LENS, "rows")
    floats_rows.mask["video"][0, 0] = 0.5
    assert TI.index_form(m, floats_rows) == "rows"             # a row-major index multiplies by its float masks: taken
    # a model whose context side still trains
    q = torch.zeros((2, 3, 32))
    with pytest.raises(ValueError, match=r"context-side parameters still require gradients \(ctx_pos_embed.*index rows would go stale"):
        TI.xml_forward_train_index(m, ok, q, torch.ones((2, 3)), None, None, None)
    TI.query_side_parameters(m)
    with pytest.raises(ValueError, match=r"ctx_len 101 outside \(0, l_ref = 100\]"):
        TI.xml_forward_train_index(m, ok, q, torch.ones((2, 3)), None, None, None, ctx_len=101)
    # the store: labels are clip numbers of the truncated video
    with pytest.raises(ValueError, match="max_ctx_len = 40, the index was built for l_ref = 100"):
        _store(tmp_path, ok, ROW_OF, max_ctx_len=40)
    with pytest.raises(ValueError, match="example 1: video vid_1 is not live in the index"):
        _store(tmp_path, ok, {k: v for k, v in ROW_OF.items() if k != "vid_1"})
    with pytest.raises(ValueError, match="video vid_0 is not live"):
        _store(tmp_path, ok, lambda name: 5 + ROW_OF[name])    # rows outside the index
    store, _, _ = _store(tmp_path, ok, ROW_OF)
    with pytest.raises(IndexError, match="example id 9 out of range"):
        store.batch([0, 9])
    with pytest.raises(ValueError, match="lmax 101 outside"):
        store.batch([0, 1], lmax=101)


def test_graphed_step_and_train_step_take_a_forward():
    import inspect
    from tvretrieval_amd import train
    assert inspect.signature(train.GraphedTrainStep.__init__).parameters["forward"].default is None
    assert inspect.signature(train.train_step).parameters["forward"].default is train.xml_forward_train
    assert list(inspect.signature(TI.xml_forward_train_index).parameters)[:10] == [
        "model", "index", "query_feat", "query_mask", "ctx_slots", "ctx_first_block", "st_ed_indices", "neg_ctx_rank", "neg_q_rank",
        "as_tensors"]
