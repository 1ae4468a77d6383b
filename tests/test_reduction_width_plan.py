"""The plan of tests/test_gpu_reduction_width.py, checked without a GPU: from the same tables (tests/reduction_width_cases.py)
* every case lands on the kernel it is meant for, by the library's own dispatch rules (tests/kernel_forms.py);
* every residue class of the slice count modulo the ring depth, every minimum count and a count above the model's largest
  width is present for every form -- a table edit that empties a class fails here with the class named;
* the thresholds the tables were laid out for are the ones the library reports, so a kernel change that moves a threshold
  cannot silently move the cases to another kernel."""
import kernel_forms as DM
import reduction_width_cases as RC


def need(present, required, what):
    """one line per required class that `present` lacks."""
    return ["%s: no case with %s" % (what, r) for r in required if r not in present]


def report(problems):
    assert not problems, "classes missing from tests/reduction_width_cases.py:\n  " + "\n  ".join(problems)


def residues(slices, depth):
    return {"n_slices = %d (mod %d)" % (s % depth, depth) for s in slices}


def all_residues(depth, step=2):
    """the slice count is even (K bytes % 128 == 0), so a four-slot ring sees 0 and 2, a five-slot ring every residue."""
    return sorted({"n_slices = %d (mod %d)" % (s % depth, depth) for s in range(0, 2 * depth * step, step)})


# ---- every case lands in its form -------------------------------------------------------------------------------------------
def test_gemm_cases_reach_their_kernels():
    for form, dt, (m, n), s in RC.gemm256_cases() + RC.gemm256p_cases():
        assert DM.gemm_form(m, n, RC.k_of(s, dt), RC.ES[dt]) == form, (form, dt, m, n, s)
        assert RC.k_of(s, dt) * RC.ES[dt] == s * DM.SLICE_BYTES
    (m, n), = RC.GEMM256P_SHAPES
    tiles = DM.cdiv(m, 256) * DM.cdiv(n, 256)
    assert DM.GEMM256P_MIN_TILES <= tiles < DM.GEMM256P_MIN_TILES + 8 and m % 256 == 1      # just over the threshold, ragged last row tile
    assert tiles > 2 * 256, "every workgroup of the persistent kernel must walk several tiles"
    for m, n in RC.GEMM256_SHAPES:
        assert DM.FEW_TILES <= DM.cdiv(m, 256) * DM.cdiv(n, 256) < DM.GEMM256P_MIN_TILES // 4
    assert any(m % 256 and n % 256 for m, n in RC.GEMM256_SHAPES), "gemm256: no ragged M with an N that is no multiple of 256"
    for form, dt, (m, n), ns, k in RC.small_cases():
        es = RC.ES[dt]
        assert DM.few(m, n) or not (DM.gemm256_ok(m, n, k, es) or DM.gemm256p_ok(m, n, k, es)), (form, dt, m, n, k)
        assert DM.gemm_form(m, n, k, es).startswith(form + "-") and DM.cdiv(k * es, 128) == ns and k % (16 // es) == 0
    for form, dt, h, s in RC.ln_cases():
        assert DM.gemm_ln_fused(RC.LN_SEQS * RC.LN_LEN, h, RC.k_of(s, dt), RC.ES[dt]), (form, dt, h, s)
    for form, dt, h, nh in RC.ATTENTION_BLOCK_CASES:
        assert DM.gemm_ln_fused(RC.LN_SEQS * RC.LN_LEN, h, h, RC.ES[dt]) and DM.attn_form(RC.LN_LEN, RC.LN_LEN, h, nh, RC.ES[dt]) == "large"
    assert RC.LN_SEQS * RC.LN_LEN >= DM.LN_FUSED_MIN_ROWS
    for form, m, k in RC.f16s_cases():
        assert DM.f16s_form(m, RC.F16S_N, k) == ("gemm256-f16s" if m >= 256 else "small%d-f16s" % DM.small_bmn(m, RC.F16S_N))


def test_k6_cases_reach_their_kernels():
    for form, dt, s, (nq, nv), n_mod in RC.k6_persist_cases():
        hidden, es = RC.k_of(s, dt), RC.ES[dt]
        assert hidden * es == s * DM.SLICE_BYTES and hidden % 8 == 0
        assert DM.q2c_tiled_ok(128, hidden, es), (form, dt, s)
        if form == "rowmajor":
            assert DM.q2c_fused_forms(n_mod, 128, hidden, es, f16=dt == "f16") == ["persist"], (form, dt, s)
            assert DM.q2c_form(128, hidden, es, combine=False, f16=dt == "f16") == "persist"
        assert DM.q2c_persist_slots(RC.K6_TILED[form], RC.K6_MASK[form]) == (5 if form in ("nomask", "bitmask") else 4)
    (nq, nv), (nq2, nv2) = RC.K6_PERSIST_SHAPES
    assert DM.q2c_persist_qsh(nq, nv) == 2 and DM.q2c_persist_tiles_per_workgroup(nq, nv) == 3, "the ring phase must carry across tiles"
    assert nv2 % 2 == 1, "an odd number of videos leaves half a clip tile"
    for form, dt, lpad, s in RC.k6_ring_cases():
        hidden, es = RC.k_of(s, dt), RC.ES[dt]
        persist = lpad == 128 and s * DM.SLICE_BYTES >= DM.K6_PERSIST_MIN_KB
        assert DM.q2c_form(lpad, hidden, es, combine=False) == ("persist" if persist else "ring"), (dt, lpad, s)
        assert DM.q2c_form(lpad, hidden, es, combine=True) == "ring", (dt, lpad, s)
    for form, dt, lpad, hidden in RC.k6_staged_cases():
        assert [DM.q2c_form(lpad, hidden, RC.ES[dt], combine=c) for c in (False, True)] == ["staged", "staged"], (dt, lpad, hidden)
    for form, dt, d in RC.l2n_cases():
        es = RC.ES[dt]
        lim, beyond = RC.L2N_WIDTHS[dt]
        assert lim // (16 // es) == 32 * DM.L2N_MAXJ and beyond == lim + 8 and beyond % (16 // es) == 0      # refused for its width alone
        assert DM.l2n_vec_ok(lim, es) and not DM.l2n_vec_ok(beyond, es)
        assert DM.tile_rows_l2norm_ok(lim, es) and not DM.tile_rows_l2norm_ok(beyond, es)


def test_attention_cases_reach_both_kernels():
    problems = []
    for dt in RC.GEMM_DTYPES:
        forms = {}
        for _, _, dh, nh, (n, lq, lk) in RC.attention_cases((dt,)):
            forms.setdefault((DM.attn_form(lq, lk, dh * nh, nh, RC.ES[dt]), dh), set()).add(nh)
        for dh in DM.ATTN_DH:
            for kern in ("small", "large"):
                heads = forms.get((kern, dh), set())
                problems += need(heads, [h for h in RC.ATTN_HEADS], "attention %s kernel, %s, DH = %d, n_heads" % (kern, dt, dh))
        refused = sorted(k for k in forms if k[0].startswith("refused"))
        assert not refused, refused                  # (a refusal would show as a skipped GPU case with its reason in the id)
    assert set(RC.ATTN_HEADS) - {4} and 96 in DM.ATTN_DH
    # the whole block: both kernels x every DH x every head count, BertSelfOutput on its unfused tail, hidden sizes beyond the model's
    for dt in RC.GEMM_DTYPES:
        forms, hidden = {}, set()
        for _, _, dh, nh, (n, l) in RC.attention_block_cases((dt,)):
            assert not DM.gemm_ln_fused(n * l, dh * nh, dh * nh, RC.ES[dt]) and (dh * nh) % 8 == 0, (dt, dh, nh, n, l)
            form = DM.attn_form(l, l, dh * nh, nh, RC.ES[dt])
            assert not form.startswith("refused"), (dt, dh, nh, l, form)
            forms.setdefault((form, dh), set()).add(nh)
            hidden.add(dh * nh)
        for dh in DM.ATTN_DH:
            for kern in ("small", "large"):
                problems += need(forms.get((kern, dh), set()), list(RC.ATTN_HEADS),
                                 "attention_block %s kernel, %s, DH = %d, n_heads" % (kern, dt, dh))
        problems += need(hidden, [96, 288, 576, 1536], "attention_block %s unfused BertSelfOutput, hidden" % dt)
    # the small kernel packs four (sequence, head) units per workgroup: the unit counts leave every remainder
    rem = {(n * nh) % 4 for _, _, _, nh, (n, lq, lk) in RC.attention_cases(("bf16",)) if max(lq, lk) <= DM.ATTN_SMALL_MAX_L}
    problems += need(rem, [0, 1, 2, 3], "attention small kernel, units % 4")
    for _, _, dh, nh, (n, lq, lk) in RC.attention_cases(("bf16",)):
        assert DM.attn_train_ok(lq, lk, dh * nh, nh)
    report(problems)


# ---- no class is missing ------------------------------------------------------------------------------------------------------
def test_every_slice_class_of_the_gemm_forms_is_present():
    problems = []
    for dt in RC.GEMM_DTYPES:
        for mn in RC.GEMM256P_SHAPES:
            sl = [s for f, d, shp, s in RC.gemm256p_cases() if d == dt and shp == mn]
            problems += need(residues(sl, 4), all_residues(4), "gemm256p %s %s" % (dt, mn))
            problems += need(sl, [DM.GEMM_MIN_KB // DM.SLICE_BYTES], "gemm256p %s %s: the minimum n_slices =" % (dt, mn))
        for mn in RC.GEMM256_SHAPES:
            sl = [s for f, d, shp, s in RC.gemm256_cases() if d == dt and shp == mn]
            main = {"no steady-state step (n_slices = 4)" if s == 4 else "one steady-state pair (n_slices = 6)" if s == 6
                    else "several steady-state pairs, n_slices = %d (mod 4)" % (s % 4) for s in sl}
            problems += need(main, ["no steady-state step (n_slices = 4)", "one steady-state pair (n_slices = 6)",
                                    "several steady-state pairs, n_slices = 0 (mod 4)",
                                    "several steady-state pairs, n_slices = 2 (mod 4)"], "gemm256 %s %s" % (dt, mn))
            problems += need(sl, [10, 14], "gemm256 %s %s: n_slices =" % (dt, mn))
        for h in RC.LN_WIDTHS:
            sl = [s for f, d, n, s in RC.ln_cases() if d == dt and n == h]
            problems += need(residues(sl, 4), all_residues(4), "LayerNorm-epilogue GEMM %s N = %d" % (dt, h))
            problems += need(sl, [DM.GEMM_MIN_KB // DM.SLICE_BYTES], "LayerNorm-epilogue GEMM %s N = %d: the minimum n_slices =" % (dt, h))
        for bmn in (32, 64, 128):
            loops = {}
            for f, d, (m, n), ns, k in RC.small_cases():
                if d == dt and f == "small%d" % bmn:
                    loops.setdefault(DM.small_kloop(k, RC.ES[dt], bmn), set()).add((ns, (k * RC.ES[dt]) % 128 != 0))
            for loop in (("plain",) if bmn == 128 else ("deep3", "deep2", "plain")):
                got = loops.get(loop, set())
                if len({ns for ns, _ in got}) < 2:
                    problems.append("small-tile GEMM %d %s: fewer than two step counts on the %s K loop" % (bmn, dt, loop))
                problems += need({p for _, p in got}, [False, True], "small-tile GEMM %d %s, %s K loop, partial last step =" % (bmn, dt, loop))
    forms = {DM.f16s_form(m, RC.F16S_N, k).split("-")[0].rstrip("0123456789") for _, m, k in RC.f16s_cases()}
    problems += need(forms, ["gemm", "small"], "split-f16 GEMM, kernel")
    problems += need(residues([6 * k // 64 for k in RC.F16S_KS], 4), all_residues(4), "split-f16 GEMM")
    report(problems)


def test_every_slice_class_of_the_k6_forms_is_present():
    problems = []
    for form in RC.K6_FORMS:
        depth = DM.q2c_persist_slots(RC.K6_TILED[form], RC.K6_MASK[form])
        for dt in RC.K6_DTYPES[form]:
            for shp in RC.K6_PERSIST_SHAPES:
                for n_mod in RC.K6_N_MOD:
                    what = "q2c_persist %s (%d slots) %s %s n_mod %d" % (form, depth, dt, shp, n_mod)
                    sl = [s for f, d, s, sh, nm in RC.k6_persist_cases() if (f, d, sh, nm) == (form, dt, shp, n_mod)]
                    problems += need(residues(sl, depth), all_residues(depth), what)
                    problems += need(sl, [DM.K6_PERSIST_MIN_KB // DM.SLICE_BYTES], what + ": the minimum n_slices =")
                    if not any(s > RC.MODEL_MAX_SLICES for s in sl):
                        problems.append("%s: no case with n_slices > %d (the largest model width)" % (what, RC.MODEL_MAX_SLICES))
    problems += need([f for f in RC.K6_FORMS if "f16" in RC.K6_DTYPES[f]], [f for f in RC.K6_FORMS if RC.K6_TILED[f]],
                     "q2c_persist f16 operands, tiled form")
    for dt in RC.GEMM_DTYPES:
        for lpad in (16, 48, 112):
            sl = [s for f, d, lp, s in RC.k6_ring_cases() if d == dt and lp == lpad]
            problems += need(sl, [2, 4, 6, 8, 10, 12, 14], "q2c_ring %s lpad %d: n_slices =" % (dt, lpad))
        sl = [s for f, d, lp, s in RC.k6_ring_cases() if d == dt and lp == 128]
        problems += need(sl, [2, 4], "q2c_ring %s lpad 128 below the persistent kernel's minimum: n_slices =" % dt)
        problems += need(sl, [6, 8, 10, 12, 14], "q2c_ring %s lpad 128 combine pass: n_slices =" % dt)
        for lpad in RC.K6_STAGED_LPADS:
            hs = [h for f, d, lp, h in RC.k6_staged_cases() if d == dt and lp == lpad]
            steps = {"%s 128-byte steps" % ("<= 1" if h * RC.ES[dt] <= 128 else "2" if h * RC.ES[dt] <= 256 else "> 2") for h in hs}
            problems += need(steps, ["<= 1 128-byte steps", "2 128-byte steps", "> 2 128-byte steps"],
                             "register-staged q2c %s lpad %d" % (dt, lpad))
        problems += need(RC.K6_STAGED_LPADS, [16, 48, 128], "register-staged q2c %s: lpad =" % dt)
    report(problems)


def test_a_removed_class_is_named(monkeypatch):
    """the failure message names the form and the class: drop every count = 0 (mod 5) from the K6 sweep."""
    import pytest
    monkeypatch.setattr(RC, "K6_PERSIST_SLICES", tuple(s for s in RC.K6_PERSIST_SLICES if s % 5))
    with pytest.raises(AssertionError) as e:
        test_every_slice_class_of_the_k6_forms_is_present()
    assert "q2c_persist nomask (5 slots) bf16 (520, 300) n_mod 2: no case with n_slices = 0 (mod 5)" in str(e.value)
    assert "q2c_persist rowmajor" not in str(e.value)        # the four-slot forms keep both of their classes


# ---- the thresholds the tables were laid out for ----------------------------------------------------------------------------------
def test_pinned_thresholds():
    """moving a threshold is one edit in csrc/dispatch.h and one here -- and a look at the tables above."""
    c = DM.const
    assert (DM.FEW_TILES, DM.GEMM256P_MIN_TILES, DM.LN_FUSED_MIN_ROWS, DM.GEMM_MIN_KB) == (64, 3072, 2048, 256)
    assert [c(n) for n in ("GEMM256_MIN_M", "GEMM256_MIN_N", "GEMM_TILE128_MIN_WG", "GEMM_TILE64_MIN_WG")] == [256, 128, 512, 192]
    # the small tiles' K loop: deep 3, then deep 2, by the number of 128-byte steps; 128-wide tiles and f16 operands stay plain
    assert [DM.small_kloop(32 * ns, 4, 64) for ns in (1, 2, 3, 4, 6)] == ["plain", "deep2", "deep3", "deep2", "deep3"]
    assert DM.small_kloop(96, 4, 128) == "plain" and DM.small_kloop(192, 2, 32) == "deep3"
    assert DM.K6_PERSIST_MIN_KB == 384 and (DM.L2N_MAXJ, DM.L2N_LANES) == (8, 32) and DM.ATTN_DH == (32, 64, 96, 128, 192)
    assert (DM.ATTN_SMALL_MAX_L, DM.ATTN_MAX_L, DM.LDS_BYTES, DM.ATTN_SMALL_UNITS) == (32, 128, 160 * 1024, 4)
    assert DM.SLICE_BYTES == 64 and (c("RING_SLOTS"), c("RING_SLOTS_NOMASK"), c("RING_LEAD")) == (4, 5, 5)
    assert [DM.q2c_persist_slots(t, m) for t in (False, True) for m in DM.K6_MASK_FORMS] == [4, 4, 4, 4, 4, 5, 5, 4]
    # the numbers are the rules' own: each predicate flips exactly at its constant
    assert DM.few(63 * 256, 256) and not DM.few(63 * 256 + 1, 256)
    assert not DM.gemm256p_ok(3071 * 256, 256, 64, 4) and DM.gemm256p_ok(3071 * 256 + 1, 256, 64, 4)
    assert not DM.gemm256_ok(255, 128, 64, 4) and not DM.gemm256_ok(256, 127, 64, 4) and DM.gemm256_ok(256, 128, 64, 4)
    assert not DM.gemm256_ok(256, 128, 32, 4) and not DM.gemm256_ok(256, 128, 80, 4)       # 128 bytes; 320 bytes: an odd slice count
    assert [DM.small_bmn(128 * wg, 128) for wg in (47, 48, 511, 512)] == [32, 64, 64, 128]
    assert not DM.q2c_tiled_ok(128, 64, 4) and DM.q2c_tiled_ok(128, 96, 4) and not DM.q2c_tiled_ok(112, 96, 4)
    assert DM.attn_form(32, 32, 64, 1, 2) == "small" and DM.attn_form(33, 32, 64, 1, 2) == DM.attn_form(32, 33, 64, 1, 2) == "large"
    assert DM.attn_form(128, 128, 64, 1, 2) == "large" and DM.attn_form(129, 128, 64, 1, 2) == "refused: longer than 128"
    # K7 / span evidence / re-score (convse.hip)
    assert (DM.CONVSE_TM, DM.RESCORE_TM_BIG, DM.CONVSE_SMALL_P, DM.CONVSE_SMALL_NV) == (64, 128, 32768, 4096)
    assert (DM.CONVSE_SUB_MIN_PAIRS_PER_VIDEO, DM.CONVSE_STEP_BYTES, c("CONVSE_SUB_MAX")) == (128, 128, 16)
    assert (c("CONVSE_MAX_KSIZE"), c("CONVSE_FAST_KSIZE")) == (15, 5)
    for entry in ("k7", "evidence"):
        assert [DM.convse_inversion(entry, p, nv) for p, nv in ((32768, 4096), (32769, 4096), (32768, 4097))] == \
            ["one-workgroup", "global", "global"]
        assert [DM.convse_inversion(entry, p, 257) for p in (128 * 257 - 1, 128 * 257)] == ["global", "sub"]
        assert [DM.convse_epilogue(entry, ks) for ks in (1, 3, 5, 7, 15)] == ["general", "general", "fast", "general", "general"]
        assert DM.convse_chunk_pairs(entry, 10 ** 6, 2, "f16s") == 64
    assert DM.convse_epilogue("k7", 5, summ=True) == "general" and DM.convse_epilogue("evidence", 5, summ=True) == "fast"
    assert [DM.convse_inversion("rescore", p, 2) for p in (1, 255, 256)] == ["global", "global", "sub"]
    assert [DM.convse_chunk_pairs("rescore", p, 2, dt) for dt in ("f32", "bf16", "f16s") for p in (128, 129)] == [64, 64, 64, 64, 64, 128]
    assert DM.convse_max_chunks("k7", 129, 13) == 2 + 13 and DM.convse_max_chunks("k7", 5, 13) == 5
    assert DM.convse_max_chunks("rescore", 129, 2, "f16s") == 1 + 2 and DM.convse_max_chunks("rescore", 128, 2, "f16s") == 2 + 2
    # the DMA mainloop: whole 128-byte rows, and both 32-bit row-offset conditions (query rows; a video's lpad clip rows)
    loop = lambda nq, lpad, h, dt, e="k7": DM.convse_mainloop(e, nq, lpad, lpad, h, 5, dt)       # noqa: E731
    assert [loop(4, 16, h, "f32") for h in (8, 24, 32, 40, 64)] == ["staged", "staged", "dma", "staged", "dma"]
    assert [loop(4, 16, h, "bf16") for h in (32, 64, 72, 96, 128)] == ["staged", "dma", "staged", "staged", "dma"]
    assert [loop(4, 16, h, "f16s") for h in (32, 96)] == ["dma", "dma"] and loop(4, 16, 48, "f16s") == "refused"
    for e in ("k7", "evidence", "rescore"):
        assert loop(2 ** 32 // 128 - 1, 16, 32, "f32", e) == "dma" and loop(2 ** 32 // 128, 16, 32, "f32", e) == "staged"
        assert loop(2 ** 32 // 128, 16, 32, "f16s", e) == "refused"
        assert loop(4, 128, 2 ** 23 - 32, "f32", e) == "dma" and loop(4, 128, 2 ** 23, "f32", e) == "staged"
        assert loop(4, 24, 32, "f32", e) == loop(4, 144, 32, "f32", e) == loop(4, 16, 12, "f32", e) == "refused"
    assert [DM.convse_mainloop("k7", 4, 16, l_ref, 32, ks, "f32") for l_ref, ks in ((17, 5), (0, 5), (16, 4), (16, 17), (16, 15))] == \
        ["refused"] * 4 + ["dma"]
    assert DM.convse_mainloop("rescore", 4, 16, 99, 32, 4, "f32") == "dma"          # (no filter, no l_ref)
