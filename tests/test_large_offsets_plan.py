"""CPU checks of the large-offset tests (tests/large_offsets.py, tests/test_gpu_large_offsets.py): the shape crosses what it
claims to, the sample set straddles every threshold, and every symbol of the four public headers has a large-offset case
or one of the four stated reasons -- so that a new entry point cannot skip the question."""
import inspect

import numpy as np
import pytest

import large_offsets as LO


def test_the_shape_is_the_smallest_round_corpus_past_t3():
    per = LO.LPAD * LO.HIDDEN
    assert LO.NV_BIG * per == 2151677952 > 2 ** 31 > 21793 * per == 2142339072          # the headline corpus: 0.24 % below T3
    assert 21793 * per * 2 == 4284678144 < 2 ** 32                                      # ... and, in bf16, below T2
    assert LO.NV_BIG % 64 == 0 and (LO.NV_BIG - 64) * per < 2 ** 31                     # no smaller multiple of 64 crosses
    assert LO.thresholds(2) == {"T1": 2 ** 30, "T2": 2 ** 31, "T3": 2 ** 31}
    assert LO.thresholds(4) == {"T1": 2 ** 29, "T2": 2 ** 30, "T3": 2 ** 31}
    for es in (2, 4):
        LO.assert_crosses(LO.NV_BIG * per, es, ("T1", "T2", "T3"))
    with pytest.raises(AssertionError, match="ends below T3"):
        LO.assert_crosses(21793 * per, 2, "T3")
    with pytest.raises(AssertionError, match="ends below T2"):
        LO.assert_crosses(21793 * per, 2, ("T1", "T2"))
    LO.assert_crosses(21793 * per, 2, "T1")                                             # (what the C3 tests cross today)


@pytest.mark.parametrize("es", [2, 4])
def test_every_threshold_is_straddled_by_a_sampled_video(es):
    nv, l, h = LO.NV_BIG, LO.LPAD, LO.HIDDEN
    s = LO.sample_videos(nv, l, h, es)
    assert s == sorted(set(s)) and s[0] == 0 and s[-1] == nv - 1
    per = l * h
    for name, t in LO.thresholds(es).items():
        v = LO.straddler(t, per)
        assert v * per < t < (v + 1) * per, name                   # the rows of v lie on both sides
        assert {v - 1, v, v + 1} <= set(s), name
    assert LO.missed_thresholds(s, nv, l, h, es) == []
    want = {2: {10922, 21845}, 4: {5461, 10922, 21845}}[es]
    assert {LO.straddler(t, per) for t in LO.thresholds(es).values()} == want


@pytest.mark.parametrize("es", [2, 4])
def test_a_sample_set_that_misses_a_threshold_is_noticed(es):
    nv, l, h = LO.NV_BIG, LO.LPAD, LO.HIDDEN
    s = LO.sample_videos(nv, l, h, es)
    assert LO.missed_thresholds([v for v in s if v != 21845], nv, l, h, es) == (["T2", "T3"] if es == 2 else ["T3"])
    assert LO.missed_thresholds([v for v in s if v != 10923], nv, l, h, es) == (["T1"] if es == 2 else ["T2"])
    assert LO.missed_thresholds([0, nv - 1], nv, l, h, es) == ["T1", "T2", "T3"]
    assert LO.missed_thresholds([0, 99], 100, l, h, es) == []        # an operand below every threshold has none to miss


def test_tile_layout_restatement():
    """[tile][slice][row][64 B]: byte b of row r of tile t stands at t * 256 * row_bytes + (b // 64) * 16384 + r * 64 + b % 64."""
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 256, (512, 192), dtype=np.uint8)
    img = LO.tile_image_bytes(rows, 192)
    assert img.shape == (2, 256 * 192)
    for t, r, b in ((0, 0, 0), (0, 255, 191), (1, 17, 64), (1, 200, 130)):
        assert img[t, (b // 64) * 16384 + r * 64 + b % 64] == rows[t * 256 + r, b]


def _registry():
    import test_gpu_large_offsets as G
    return G


def test_every_header_symbol_has_a_large_case_or_one_of_the_four_reasons():
    G = _registry()
    syms = set(LO.header_symbols())
    assert len(syms) >= 130 and {"xml_index_move_blocks_packed", "xml_chain_best_rows", "xml_index_put_rows_packed"} <= syms
    covered, exempt = set(G.LARGE_CASES), set(G.LARGE_EXEMPT)
    assert covered <= syms, "cases for symbols no header declares: %s" % sorted(covered - syms)
    assert exempt <= syms, "exemptions for symbols no header declares: %s" % sorted(exempt - syms)
    assert not covered & exempt, "symbols that are both covered and exempt: %s" % sorted(covered & exempt)
    missing = syms - covered - exempt
    assert not missing, "header symbols with neither a large-offset case nor a stated reason: %s" % sorted(missing)
    for s, why in G.LARGE_EXEMPT.items():
        assert why in LO.REASONS, (s, why)
    for s, cases in G.LARGE_CASES.items():
        assert cases, s
        for name in cases:
            fn = getattr(G, name, None)
            assert name.startswith("test_") and callable(fn), (s, name)
            assert "assert_crosses(" in inspect.getsource(fn), "%s does not say which threshold its operand crosses" % name
    assert G.pytestmark.name == "gpu"


def test_completeness_bites_when_a_symbol_is_deleted(monkeypatch):
    G = _registry()
    for gone in ("xml_index_put_rows", "xml_span_evidence", "xml_index_move_blocks_packed"):
        cases = dict(G.LARGE_CASES)
        del cases[gone]
        monkeypatch.setattr(G, "LARGE_CASES", cases)
        with pytest.raises(AssertionError, match=gone):
            test_every_header_symbol_has_a_large_case_or_one_of_the_four_reasons()
    monkeypatch.undo()
    monkeypatch.setitem(G.LARGE_EXEMPT, "xml_abi_version", "too small to matter")
    with pytest.raises(AssertionError, match="too small to matter"):
        test_every_header_symbol_has_a_large_case_or_one_of_the_four_reasons()


def test_corpus_operands_are_never_exempt():
    """The rule of the registry, spelled out for the entries the issue names: anything that reads or writes an operand of
    nv x lpad x hidden, nv x lpad, rows x d with corpus-sized rows, a feature store or a strided score matrix has a case."""
    G = _registry()
    need = """xml_index_put_rows xml_index_put_rows_packed xml_index_clear_rows xml_index_clear_rows_packed
        xml_index_move_blocks_packed xml_index_set_chains xml_chain_best_allow xml_group_best_allow xml_span_evidence
        xml_q2c_rescore xml_split_f16_rows xml_unsplit_f16_rows xml_q2c_tile_rows xml_q2c_tile_rows_gather
        xml_q2c_tile_rows_l2norm xml_ingest_rows xml_gather_feature_rows xml_gather_index_rows xml_q2c_scores_packed
        xml_q2c_scores xml_q2c_scores_fused xml_q2c_scores_tiled xml_l2norm_rows xml_l2norm_rows_eps xml_convert
        xml_round_bf16_rows_err xml_convse_rerank xml_convse_rerank_f16s xml_convse_rerank_ex xml_topk_rows
        xml_topk_rows_allowed xml_select_ge_rows xml_select_ge_rows_allowed xml_best_part_rows""".split()
    assert set(need) <= set(G.LARGE_CASES), sorted(set(need) - set(G.LARGE_CASES))


def test_the_sample_sets_of_the_gpu_cases_cover_both_element_sizes():
    G = _registry()
    for es in (2, 4):
        assert LO.missed_thresholds(G.SAMPLE, G.NV, G.L, G.H, es) == []
        assert LO.missed_thresholds(G.SAMPLE_TILES, G.N_TILES, 256, G.H, es) == []          # tiles of 256 rows as units
    assert G.N_TILES * 256 * G.H == G.NV * G.L * G.H and G.HALF * G.L * G.H < 2 ** 31
    assert 2 * G.LD_BIG > 2 ** 31 and len(G.STORE_PERM) == len(G.SAMPLE) and sorted(G.STORE_PERM) == list(range(len(G.SAMPLE)))
