"""The three kernels of include/xmlhip_index_parts_exact.h against numpy loops, bitwise: the fold on a candidate list
(xml_cand_best_part), the head-bit mask made per-slot (xml_chain_spread_allow) and the slots of a video (xml_chain_members).
Synthetic tables of n = 70 slots (three words, the last one partial) with chains of 1, 2, 3, max_parts = 8 and max_parts + 1
slots scattered across the word boundaries; the fold out of place and in place, on contiguous lists through the wrapper and
on rows with wider leading dimensions through the entry itself."""
import types

import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from tvretrieval_amd import _lib, ops

pytestmark = pytest.mark.gpu

N, MAX_PARTS = 70, 8
CHAINS = [[30, 33], [62, 5, 66], [31, 32, 63, 64, 1, 40, 69, 10], [20, 21, 22, 23, 24, 25, 26, 27, 28]]
LIMIT = 4096
INF, NAN = float("inf"), float("nan")


def _tables(n=N, chains=CHAINS):
    head, nxt, off = np.arange(n, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for ch in chains:
        for i, s in enumerate(ch):
            head[s], off[s] = ch[0], 16 * i
            nxt[s] = ch[i + 1] if i + 1 < len(ch) else -1
    return head, nxt, off


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ref_fold(scores, ids, group, order):
    """The header's rule as a loop."""
    n = len(group)
    out_s, out_i = scores.copy(), ids.copy()
    for r in range(scores.shape[0]):
        groups = {}
        for p in range(scores.shape[1]):
            s = int(ids[r, p])
            if not 0 <= s < n:
                continue                                                   # empty: passes through
            g = int(group[s])
            groups.setdefault(g if 0 <= g < n else ("own", p), []).append(p)
        for ps in groups.values():
            if len(ps) == 1:
                continue
            v = [(-INF if np.isnan(scores[r, p]) else float(scores[r, p])) for p in ps]
            best = min(range(len(ps)), key=lambda i: (-v[i], int(order[ids[r, ps[i]]]), ps[i]))
            for i, p in enumerate(ps):
                if i != best:
                    out_s[r, p], out_i[r, p] = -INF, -1
    return out_s, out_i


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_fold(scores, ids, group, order):
    want_s, want_i = _ref_fold(scores, ids, group, order)
    ds, di, dg, do = _dev(scores), _dev(ids), _dev(group), _dev(order)
    got_s, got_i = ops.cand_best_part(ds, di, dg, do)                       # out of place: the inputs stay
    assert (_bits(ds.cpu().numpy()) == _bits(scores)).all() and (di.cpu().numpy() == ids).all()
    assert (_bits(got_s.cpu().numpy()) == _bits(want_s)).all(), "scores"
    assert (got_i.cpu().numpy() == want_i).all(), "ids"
    back = ops.cand_best_part(ds, di, dg, do, out=(ds, di))                 # in place
    assert back[0] is ds and back[1] is di
    assert (_bits(ds.cpu().numpy()) == _bits(want_s)).all(), "scores in place"
    assert (di.cpu().numpy() == want_i).all(), "ids in place"
    return want_s, want_i


def _plant(scores, ids, r, places, slots, values):
    """Candidates at chosen places of row r; with 130 rows the row holds nothing else, so that the planted ones decide."""
    r %= scores.shape[0]
    if scores.shape[0] == 130:
        ids[r] = -1
    for p, s, v in zip(places, slots, values):
        if p < scores.shape[1]:
            ids[r, p], scores[r, p] = s, v


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 256, 257, 1024, LIMIT])
def test_the_fold_equals_the_loop(m):
    head, nxt, off = _tables()
    group = head.copy()
    group[50], group[51] = 99, -3                                           # group values outside [0, n): groups of their own
    rng = np.random.default_rng(100 + m)
    pool = np.array(list(range(N)) + [-1] * 25 + [70, 1000, -5, 2 ** 31 - 1], dtype=np.int64)   # ids outside [0, n) too
    for rows in (1, 5, 130):
        ids = rng.choice(pool, size=(rows, m)).astype(np.int32)
        if m >= 64:                                                         # rows with few candidates: most groups are single
            ids[rows // 2:] = np.where(rng.random((rows - rows // 2, m)) < 0.9, -1, ids[rows // 2:])
        scores = (rng.integers(-3, 6, size=(rows, m)) / 4.0).astype(np.float32)       # few values: many ties
        special = rng.random((rows, m))
        scores[special < 0.03] = NAN
        scores[(special >= 0.03) & (special < 0.06)] = -INF
        scores[(special >= 0.06) & (special < 0.08)] = INF
        last = m - 1
        a, b, c = CHAINS[0], CHAINS[1], CHAINS[2]
        # two members of one chain at the ends of the row, the lower offset LATER with an equal score: it wins
        _plant(scores, ids, 0, [0, last], [a[1], a[0]], [7.0, 7.0])
        # three members on either side of 63 / 64 with an empty slot between them; the middle offset scores highest
        _plant(scores, ids, 1, [62, 63, 64, 65], [b[2], -1, b[1], b[0]], [1.0, 9.0, 8.0, 1.0])
        # ... and of 255 / 256, the lower offset later with an equal score
        _plant(scores, ids, 2, [254, 255, 256, 257], [c[5], c[7], c[2], -1], [8.5, 8.0, 8.5, 8.5])
        # a chain of nothing but NaN / -inf: the lowest offset represents it; NaN against +inf and -inf
        _plant(scores, ids, 3, [0, 1, last], [c[3], c[1], c[6]], [NAN, -INF, NAN])
        _plant(scores, ids, 4, [0, 1, last], [b[1], b[0], b[2]], [NAN, -INF, INF])
        # candidates whose group value is outside the table stay, both of them; an id outside it passes through
        _plant(scores, ids, 5, [0, 1, 2, last], [50, 50, 51, 70], [1.0, 2.0, 3.0, 4.0])
        want_s, want_i = _check_fold(scores, ids, group, off)
        if rows == 130 and m >= 2:
            assert want_i[0, 0] == -1 and want_i[0, last] == a[0] and want_s[0, last] == 7.0
        if rows == 130 and m >= 66:
            assert want_i[1, 64] == b[1] and want_i[1, 62] == -1 and want_i[1, 65] == -1 and want_i[1, 63] == -1
        if rows == 130 and m >= 257:
            assert want_i[2, 254] == -1 and want_i[2, 256] == c[2] and want_i[2, 255] == -1
        if rows == 130 and m >= 3:
            assert want_i[3, 1] == c[1] and np.isneginf(want_s[3, 1]) and want_i[3, 0] == -1 and want_i[3, last] == -1
            assert want_i[4, last] == b[2] and want_i[4, 0] == -1 and want_i[4, 1] == -1
        if rows == 130 and m >= 5:
            assert want_i[5, :3].tolist() == [50, 50, 51] and want_i[5, last] == 70 and want_s[5, last] == 4.0


def test_the_fold_on_many_distinct_groups():
    """A wide table: rows of the widest list whose candidates are almost all the only ones of their group (the path that
    scans nothing), with chains of two and three among them."""
    n = 6000
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).tolist()
    chains, at = [], 0
    while at + 3 <= 1500:
        k = int(rng.integers(2, 4))
        chains.append(perm[at:at + k])
        at += k
    head, nxt, off = _tables(n, chains)
    ids = np.stack([rng.permutation(n)[:LIMIT] for _ in range(3)]).astype(np.int32)
    ids[1, rng.random(LIMIT) < 0.5] = -1
    scores = rng.standard_normal((3, LIMIT)).astype(np.float32)
    scores[2] = np.round(scores[2])                                        # ties inside chains
    want_s, want_i = _check_fold(scores, ids, head, off)
    assert ((want_i == -1) & (ids >= 0)).sum() > 300                       # parts really lost to better ones


def test_the_fold_of_all_slots_of_a_chain_marks_chain_best_allows_slot():
    head, nxt, off = _tables()
    rng = np.random.default_rng(3)
    rows = 40
    scores = (rng.integers(-2, 3, size=(rows, N)) / 2.0).astype(np.float32)
    scores[rng.random((rows, N)) < 0.2] = NAN
    scores[rng.random((rows, N)) < 0.2] = -INF
    scores[:3, CHAINS[1]] = NAN                                            # chains of nothing but NaN: the head stands for them
    ids = np.tile(np.arange(N, dtype=np.int32), (rows, 1))
    ch = types.SimpleNamespace(chain_head=_dev(head), chain_next=_dev(nxt), max_parts=16)
    live = torch.full((1, 3), -1, dtype=torch.int32, device=DEV)
    bits = ops.chain_best_allow(_dev(scores), ch, live).cpu().numpy().view(np.uint32)
    marked = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(rows, 96)[:, :N].astype(bool)
    _, got_i = ops.cand_best_part(_dev(scores), _dev(ids), ch.chain_head, _dev(off))
    assert ((got_i.cpu().numpy() >= 0) == marked).all()


def _ref_spread(allow_words, head, n):
    words = (n + 31) // 32
    out = np.zeros((allow_words.shape[0], words), dtype=np.uint32)
    for r in range(allow_words.shape[0]):
        for s in range(n):
            h = int(head[s])
            if 0 <= h < n and (int(allow_words[r, h >> 5]) >> (h & 31)) & 1:
                out[r, s >> 5] |= np.uint32(1 << (s & 31))
    return out


@pytest.mark.parametrize("rows", [1, 5, 130])
def test_spread_gives_every_slot_its_heads_bit(rows):
    head, nxt, off = _tables()
    head[52], head[53] = 70, -1                                             # heads outside the table: bit 0
    rng = np.random.default_rng(rows)
    allowed = rng.random((rows, N)) < 0.5
    allowed[0, [30, 62, 31, 20]] = True                                     # heads in each of the three words ...
    allowed[0, [33, 5, 66, 32, 63, 64, 1, 40, 69, 10]] = False              # ... whose other slots' bits mean nothing
    allowed[-1, [30, 62, 31]] = [False, True, False]
    allowed[-1, [33, 5, 66]] = [True, False, False]
    pad = np.zeros((rows, 96), dtype=bool)
    pad[:, :N] = allowed
    pad[:, N:] = True                                                       # a caller's padding bits must not leak
    words = (pad.reshape(rows, 3, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
    want = _ref_spread(words, head, N)
    assert not (want[:, 2] >> np.uint32(N - 64)).any()                      # padding bits of the last word are 0
    ch = types.SimpleNamespace(chain_head=_dev(head))
    got = ops.chain_spread_allow(_dev(words.view(np.int32)), ch)
    assert tuple(got.shape) == (rows, 3) and (got.cpu().numpy().view(np.uint32) == want).all()
    for s in (33, 5, 66, 32, 69):
        assert ((want[:, s >> 5] >> np.uint32(s & 31)) & 1 == allowed[:, head[s]]).all()
    # the entry itself: a shared row spread to `rows` rows, wider row strides, and words beyond ceil(capacity / 32) untouched
    guard = 0x5A5A5A5A
    out = torch.full((rows, 5), guard, dtype=torch.int32, device=DEV)
    wide = torch.full((rows, 4), -1, dtype=torch.int32, device=DEV)
    wide[:, :3] = _dev(words.view(np.int32))
    lib = _lib.load()
    for allow_rows in sorted({1, rows}):
        out.fill_(guard)
        _lib.check(lib.xml_chain_spread_allow(ops._p(wide), 4, allow_rows, rows, N, ops._p(ch.chain_head), ops._p(out), 5,
                                              ops._stream()), "xml_chain_spread_allow")
        res = out.cpu().numpy()
        assert (res[:, 3:] == guard).all()
        assert (res[:, :3].view(np.uint32) == (want if allow_rows == rows else np.repeat(want[:1], rows, 0))).all()


def test_members_lists_a_chain_and_stops():
    head, nxt, off = _tables()
    nxt[5] = 1000                                                           # a next outside the table ends the walk
    head[53] = 70                                                           # a head outside it: no video
    ch = types.SimpleNamespace(chain_head=_dev(head), chain_next=_dev(nxt), max_parts=MAX_PARTS)
    video = np.array([30, 33, 62, 66, 5, 31, 10, 64, 20, 28, 0, 69, 53, -1, 70, 10 ** 6, -2 ** 31] + list(range(N)),
                     dtype=np.int32)
    want = np.full((len(video), MAX_PARTS), -1, dtype=np.int32)
    by_head = {c[0]: c for c in CHAINS}
    by_head[62] = [62, 5]
    for r, v in enumerate(video):
        if 0 <= v < N and 0 <= head[v] < N:
            c = by_head.get(int(head[v]), [int(v)])[:MAX_PARTS]             # nine slots: cut at max_parts
            want[r, :len(c)] = c
    got = ops.chain_members(ch, _dev(video)).cpu().numpy()
    assert (got == want).all()
    assert got[5].tolist() == CHAINS[2] and got[8].tolist() == CHAINS[3][:8] and got[9].tolist() == CHAINS[3][:8]
    assert got[2].tolist()[:4] == [62, 5, -1, -1] and got[3].tolist()[:3] == [62, 5, -1] and (got[12:17] == -1).all()
    assert ops.chain_members(ch, _dev(video[:0])).shape == (0, MAX_PARTS)


def test_row_strides_are_respected_and_nothing_else_is_written():
    """The entries themselves with leading dimensions wider than the rows: the gaps are neither read as candidates nor
    written, out of place and in place."""
    head, nxt, off = _tables()
    lib = _lib.load()
    rng = np.random.default_rng(21)
    rows, m = 7, 65
    ld, out_ld = m + 3, m + 5
    ids = (rng.integers(0, N + 6, size=(rows, m)) - 3).astype(np.int32)               # some outside [0, n)
    scores = (rng.integers(-3, 6, size=(rows, m)) / 4.0).astype(np.float32)
    want_s, want_i = _ref_fold(scores, ids, head, off)
    assert (want_i != ids).any()
    guard_f, guard_i = 123.5, 0x5A5A5A5A
    s_in = torch.full((rows, ld), 99.0, dtype=torch.float32, device=DEV)              # a gap that would win every group ...
    i_in = torch.full((rows, ld), CHAINS[2][0], dtype=torch.int32, device=DEV)        # ... of a chain, were it read
    s_in[:, :m], i_in[:, :m] = _dev(scores), _dev(ids)
    s_out = torch.full((rows, out_ld), guard_f, dtype=torch.float32, device=DEV)
    i_out = torch.full((rows, out_ld), guard_i, dtype=torch.int32, device=DEV)
    dh, do = _dev(head), _dev(off)

    def fold(a, b, lda, c, d, ldc):
        _lib.check(lib.xml_cand_best_part(ops._p(a), ops._p(b), lda, rows, m, ops._p(dh), ops._p(do), N, ops._p(c), ops._p(d), ldc,
                                          ops._stream()), "xml_cand_best_part")
    fold(s_in, i_in, ld, s_out, i_out, out_ld)
    assert (_bits(s_out[:, :m].cpu().numpy()) == _bits(want_s)).all() and (i_out[:, :m].cpu().numpy() == want_i).all()
    assert bool((s_out[:, m:] == guard_f).all()) and bool((i_out[:, m:] == guard_i).all())
    assert (_bits(s_in[:, :m].cpu().numpy()) == _bits(scores)).all() and (i_in[:, :m].cpu().numpy() == ids).all()
    fold(s_in, i_in, ld, s_in, i_in, ld)                                              # in place
    assert (_bits(s_in[:, :m].cpu().numpy()) == _bits(want_s)).all() and (i_in[:, :m].cpu().numpy() == want_i).all()
    assert bool((s_in[:, m:] == 99.0).all()) and bool((i_in[:, m:] == CHAINS[2][0]).all())
    # xml_chain_members with out_ld > max_parts
    video = _dev(np.array([33, 66, 10, 28, 0, -1, 70], dtype=np.int32))
    out = torch.full((7, MAX_PARTS + 2), guard_i, dtype=torch.int32, device=DEV)
    dn = _dev(nxt)
    _lib.check(lib.xml_chain_members(ops._p(video), 7, N, ops._p(dh), ops._p(dn), MAX_PARTS, ops._p(out), MAX_PARTS + 2,
                                     ops._stream()), "xml_chain_members")
    ch = types.SimpleNamespace(chain_head=dh, chain_next=dn, max_parts=MAX_PARTS)
    assert torch.equal(out[:, :MAX_PARTS], ops.chain_members(ch, video)) and bool((out[:, MAX_PARTS:] == guard_i).all())
    assert out[0, :3].tolist() == [30, 33, -1] and out[3, :MAX_PARTS].tolist() == CHAINS[3][:MAX_PARTS]
