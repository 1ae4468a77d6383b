"""The chain entries of include/xmlhip_index_parts.h on the GPU against a numpy restatement, with ==: the fold
(ops.chain_best_allow), its one-video-per-row form (ops.chain_best_rows) and the table scatter (ops.index_set_chains).
Capacity 300: ten bit words, the last one with 12 valid bits, and two workgroups of 256 threads; the chain 5 -> 290 -> 31 -> 32
crosses both the word and the workgroup edge.  No table here holds a cycle: the bound on the walk is read off the kernel
(csrc/index_parts.hip), and tests/test_index_chains.py shows that the host table never emits one."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from tvretrieval_amd import _lib, ops
from tvretrieval_amd import inference as inf

pytestmark = pytest.mark.gpu

CAP, MAX_PARTS = 300, 8
WORDS = (CAP + 31) // 32
# chains of 4, 2, 3, max_parts, max_parts - 1 and 5 slots (the last three are longer than the four slot numbers the kernel
# keeps in registers); slot 40 and 299 are live videos of one part; every other slot is free
CHAINS = [[5, 290, 31, 32], [64, 63], [100, 7, 255], [299 - 1, 256, 0, 33, 96, 95, 128, 200], [10, 11, 12, 13, 14, 15, 16],
          [288, 287, 286, 257, 1]]
SINGLES = [40, 299]


class Tables(object):
    def __init__(self, chains=CHAINS, max_parts=MAX_PARTS):
        self.head, self.next = np.arange(CAP, dtype=np.int32), np.full(CAP, -1, dtype=np.int32)
        for ch in chains:
            for j, s in enumerate(ch):
                self.head[s] = ch[0]
                self.next[s] = ch[j + 1] if j + 1 < len(ch) else -1
        self.chains, self.max_parts = chains, max_parts
        self.live = np.zeros(CAP, dtype=bool)
        self.live[[s for ch in chains for s in ch] + SINGLES] = True
        self.chain_head, self.chain_next = torch.from_numpy(self.head).to(DEV), torch.from_numpy(self.next).to(DEV)


def _best(srow, chain):
    """The best part of a chain for one score row: the first maximum in chain order, NaN as -inf, nothing finite: the head."""
    v = np.asarray(srow[chain], dtype=np.float32).copy()
    v[np.isnan(v)] = -np.inf
    return chain[int(np.argmax(v))]


def _fold(scores, t, allow):
    """numpy restatement of xml_chain_best_allow: allow (rows, CAP) bool, tested at the HEAD only."""
    rows = scores.shape[0]
    out = np.zeros((rows, CAP), dtype=bool)
    in_chain = {s for ch in t.chains for s in ch}
    for r in range(rows):
        for ch in t.chains:
            if allow[r, ch[0]]:
                out[r, _best(scores[r], ch)] = True
        for s in range(CAP):
            if s not in in_chain and allow[r, s]:
                out[r, s] = True                                   # a slot alone is its own best part, whatever it scores
    return out


def _words(mask):
    return inf.pack_video_allow(np.ascontiguousarray(mask))


def _scores(rows, seed, t, nan_singles):
    rng = np.random.default_rng(seed)
    ld = CAP + 7                                                   # ld > capacity
    buf = rng.standard_normal((rows, ld)).astype(np.float32)
    s = buf[:, :CAP]
    s[:, 63] = s[:, 64]                                            # a tie between head and second part: the lowest offset wins
    s[:, 32] = s[:, 31] = 9.0                                      # ... and at the maximum between the last two of four
    s[:, [100, 7, 255]] = -np.inf                                  # a chain of nothing but -inf -> its head
    s[:, 0] = np.nan                                               # NaN in the middle of the longest chain
    s[:, 200] = 8.0                                                # its best part is the LAST one, behind the register slots
    s[:, [10, 12, 14]] = np.nan
    s[:, [11, 13, 15, 16]] = -np.inf                               # nothing but NaN / -inf -> the head, slot 10
    if rows > 1:
        s[1, [288, 287, 286, 257, 1]] = 0.5                        # all parts tied in one row
        s[-1, 63] = np.nan                                         # NaN in a chain of two: the other part wins
    if nan_singles:                                                # every free slot and every one-slot video: must not be read
        alone = np.ones(CAP, dtype=bool)
        alone[[x for ch in t.chains for x in ch]] = False
        s[:, alone] = np.nan
    return buf, s


@pytest.mark.parametrize("rows", [1, 32, 33])
@pytest.mark.parametrize("allow", ["live", "shared", "per_row"])
def test_chain_best_allow_matches_the_restatement(rows, allow):
    t = Tables()
    rng = np.random.default_rng(rows * 11 + len(allow))
    if allow == "live":
        a = t.live[None].copy()                                    # the live words alone: the non-head bits of a chain are 1
    else:
        a = np.broadcast_to(t.live, (1 if allow == "shared" else rows, CAP)).copy()
        a &= rng.random(a.shape) < 0.7                             # a caller's mask ANDed with live
        a[:, 298] = True
        a[:, [256, 0, 33, 96, 95, 128, 200]] = False               # ... numbers a video by its head: the other bits are 0
        a[-1, 5] = False                                           # a cleared head: no part of that chain is listed
        a[-1, [290, 31, 32]] = True                                # (bits of its other slots mean nothing)
    results = []
    for nan_singles in (False, True):
        buf, s = _scores(rows, rows, t, nan_singles)
        dev = torch.from_numpy(buf).to(DEV)[:, :CAP]
        assert dev.stride(0) == CAP + 7
        got = ops.chain_best_allow(dev, t, torch.from_numpy(_words(a)).to(DEV))
        assert got.dtype == torch.int32 and tuple(got.shape) == (rows, WORDS)
        g = got.cpu().numpy()
        want = _fold(s, t, np.broadcast_to(a, (rows, CAP)))
        assert (g == _words(want)).all(), nan_singles
        assert ((g[:, -1].view(np.uint32) >> np.uint32(CAP % 32)) == 0).all()      # padding bits of the last word
        results.append(g)
    assert (results[0] == results[1]).all()                        # NaN in the columns that are not read changes nothing
    want = _fold(s, t, np.broadcast_to(a, (rows, CAP)))
    assert not want[:, ~t.live].any()                              # a free slot: single, live bit clear -> 0
    assert want[:, SINGLES].all() if allow == "live" else True
    if allow != "live":
        assert not want[-1, [5, 290, 31, 32]].any()
        return
    assert want[0, 31] and not want[0, [5, 290, 32]].any() and want[0, 64] and not want[0, 63]
    assert want[0, 100] and want[0, 200] and want[0, 10]
    assert want.sum(1).tolist() == [len(CHAINS) + len(SINGLES)] * rows
    if rows > 1:
        assert want[1, 288] and want[-1, 64] and not want[-1, 63]


def test_the_word_behind_the_last_one_is_not_written():
    t = Tables()
    rows, out_ld = 33, WORDS + 1
    buf, s = _scores(rows, 3, t, True)
    dev = torch.from_numpy(buf).to(DEV)
    allow = torch.from_numpy(_words(t.live[None])).to(DEV)
    out = torch.full((rows, out_ld), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    st = _lib.load().xml_chain_best_allow(ctypes.c_void_p(dev.data_ptr()), CAP + 7, rows, CAP, ctypes.c_void_p(t.chain_head.data_ptr()),
                                          ctypes.c_void_p(t.chain_next.data_ptr()), MAX_PARTS, ctypes.c_void_p(allow.data_ptr()),
                                          WORDS, 1, ctypes.c_void_p(out.data_ptr()), out_ld, ops._stream())
    assert st == 0
    g = out.cpu().numpy()
    assert (g[:, WORDS] == 0x5A5A5A5A).all()
    assert (g[:, :WORDS] == _words(_fold(s, t, np.broadcast_to(t.live, (rows, CAP))))).all()


@pytest.mark.parametrize("max_parts,lengths", [(8, [8, 7]), (4, [4, 3]), (1, [1])])
def test_chains_of_max_parts_and_one_less(max_parts, lengths):
    """Chains of exactly max_parts and max_parts - 1 slots are folded whole, for a max_parts above, at and below the number of
    slot numbers the kernel keeps in registers."""
    rng = np.random.default_rng(max_parts)
    slots = rng.permutation(CAP)[:sum(lengths)].tolist()
    chains, at = [], 0
    for n in lengths:
        chains.append(slots[at:at + n])
        at += n
    t = Tables([ch for ch in chains if len(ch) > 1], max_parts)
    t.live[:] = True
    rows = 33
    s = rng.standard_normal((rows, CAP)).astype(np.float32)
    for ch in t.chains:
        s[0, ch[-1]] = 7.0                                          # the last slot of the chain wins row 0
    got = ops.chain_best_allow(torch.from_numpy(s).to(DEV), t, torch.from_numpy(_words(t.live[None])).to(DEV)).cpu().numpy()
    want = _fold(s, t, np.broadcast_to(t.live, (rows, CAP)))
    assert (got == _words(want)).all()
    for ch in t.chains:
        assert want[0, ch[-1]] and want[:, ch].sum(1).tolist() == [1] * rows


def test_chain_best_rows_matches_the_restatement():
    t = Tables()
    rows = 33
    buf, s = _scores(rows, 5, t, True)
    dev = torch.from_numpy(buf).to(DEV)[:, :CAP]
    video = np.random.default_rng(9).integers(0, CAP, rows).astype(np.int32)
    video[:12] = [32, 5, -1, CAP, 255, 200, 40, 41, 13, 63, 1, CAP + 1000]     # any slot of a chain; outside; single; free
    got = ops.chain_best_rows(dev, t, torch.from_numpy(video).to(DEV)).cpu().numpy()
    by_slot = {x: ch for ch in t.chains for x in ch}
    for r, v in enumerate(video.tolist()):
        want = -1 if not 0 <= v < CAP else (_best(s[r], by_slot[v]) if v in by_slot else v)
        assert got[r] == want, (r, v)
    assert got[0] == 31 and got[1] == 31 and got[4] == 100 and got[5] == 200 and got[8] == 10


def test_index_set_chains_links_and_resets():
    head = torch.arange(CAP, dtype=torch.int32, device=DEV)
    nxt = torch.full((CAP,), -1, dtype=torch.int32, device=DEV)
    off = torch.zeros(CAP, dtype=torch.int32, device=DEV)
    rec = [[5, 5, 290, 0], [290, 5, 31, 16], [31, 5, 32, 32], [32, 5, -1, 41], [CAP, 1, 2, 3], [-1, 1, 2, 3], [299, 298, -1, 16]]
    ops.index_set_chains(torch.tensor(rec, dtype=torch.int32, device=DEV), head, nxt, off)
    want = Tables([[5, 290, 31, 32]])
    want.head[299] = 298
    w_off = np.zeros(CAP, dtype=np.int32)
    w_off[[290, 31, 32, 299]] = [16, 32, 41, 16]
    assert (head.cpu().numpy() == want.head).all() and (nxt.cpu().numpy() == want.next).all() and (off.cpu().numpy() == w_off).all()
    ops.index_set_chains(torch.tensor([[s, s, -1, 0] for s in (5, 290, 31, 32, 299)], dtype=torch.int32, device=DEV), head, nxt, off)
    assert (head.cpu().numpy() == np.arange(CAP)).all() and (nxt == -1).all() and (off == 0).all()
    ops.index_set_chains(torch.zeros((0, 4), dtype=torch.int32, device=DEV), head, nxt, off)          # n == 0: no launch


def test_the_wrappers_validate_their_arguments():
    t = Tables()
    s = torch.zeros((3, CAP), device=DEV)
    live = torch.from_numpy(_words(t.live[None])).to(DEV)
    with pytest.raises(ValueError, match="slots"):
        ops.chain_best_allow(s[:, :-1].contiguous(), t, live)
    with pytest.raises(ValueError, match="required"):
        ops.chain_best_allow(s, t, None)
    with pytest.raises(ValueError, match="allow"):
        ops.chain_best_allow(s, t, torch.zeros((2, WORDS), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="allow"):
        ops.chain_best_allow(s, t, torch.zeros((1, WORDS - 1), dtype=torch.int32, device=DEV))
    with pytest.raises(Exception, match="float32"):
        ops.chain_best_allow(s.double(), t, live)
    with pytest.raises(ValueError, match="video"):
        ops.chain_best_rows(s, t, torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(Exception, match="chain_head"):
        ops.chain_best_allow(s, object(), live)
    with pytest.raises(Exception, match="records"):
        ops.index_set_chains(torch.zeros((2, 3), dtype=torch.int32, device=DEV), t.chain_head, t.chain_next, t.chain_head.clone())
