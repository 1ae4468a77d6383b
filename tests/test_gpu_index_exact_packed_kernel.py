"""ops.index_put_rows_packed_exact (xml_index_put_rows_packed_exact) called directly, bitwise against
  * the composition of the existing ops l2norm_rows -> round_bf16_rows_err -> split_f16_rows on the batch's rows, and
  * ops.index_put_rows_exact of the same batch, under the EFFECTIVE masks (mask AND clip < 16 nb), into a scratch per-slot
    index -- every per-slot operand, the slot state and the running bound;
the code table and the packed mask words against what the header says, written out in numpy.
Capacity 9, 3 tiles, b = 4, lb = 37 (no multiple of 4: the last workgroup of a video holds one batch row and three padding
rows); hidden 768 (the second 512-element trip of the row walk, lanes 32..63 of the first) and 256; one and two modalities,
both exact modes.  Runs: blocks 0 and 1 | 2 | 3 (two videos in mask word 0; the first with keep = 16 < lb), 6 | 7 | 8 (across
the wave tiles: -3 at block 7), the image's last three blocks.  Every tensor of the index is pre-filled with sentinels, so
that whatever the call must not write shows."""
import numpy as np
import pytest
import torch

from test_gpu_index_update import _bits
from test_gpu_kernels import DEV
from tvretrieval_amd import ops

pytestmark = pytest.mark.gpu

CAP, TILES, B, LB, L_REF = 9, 3, 4, 37, 100
SLOTS, IDS = [2, 0, 8, 5], [70, 71, 72, 73]
RUNS = [(0, 1), (1, 3), (6, 3), (45, 3)]
LENS = ([37, 30, 37, 5], [20, 37, 0, 37])                 # valid clips per video, modality a | b (video 2 of b: none)
CASES = [pytest.param(mode, h, n_mod, id="%s-h%d-mod%d" % (mode, h, n_mod))
         for mode in ("f32", "f16s") for h in (768, 256) for n_mod in (1, 2)]


def _batch(h, n_mod, seed=0):
    g = torch.Generator().manual_seed(410 + seed)
    f1 = [torch.randn(B, LB, h, generator=g).to(DEV) for _ in range(n_mod)]
    f2 = [(3.0 * torch.randn(B, LB, h, generator=g)).to(DEV) for _ in range(n_mod)]
    f2[0][1, 4] = 0.0                                      # a zero row inside the batch: scale 1, halves 0
    masks = [(torch.arange(LB)[None] < torch.tensor(LENS[m])[:, None]).float().to(DEV) for m in range(n_mod)]
    return f1, f2, masks


class Index(object):
    """The tensors of an exact-rank index, sentinel-filled: per-slot (tiles=None) or with the packed filter image."""

    def __init__(self, mode, h, n_mod, tiles=None, seed=1):
        g = torch.Generator().manual_seed(420 + seed)
        rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)                               # noqa: E731
        ints = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).to(torch.int32).to(DEV)     # noqa: E731
        self.split, self.h, self.n_mod, self.tiles = mode == "f16s", h, n_mod, tiles

        def rows():
            if self.split:
                return ops.SplitRows(ints(-2 ** 31, 2 ** 31, CAP, 128, h), rnd(CAP, 128).abs())
            return rnd(CAP, 128, h)
        image_rows = CAP * 128 if tiles is None else tiles * 256
        self.k6 = []
        for _ in range(n_mod):
            data = rnd(ops.q2c_tiled_numel(image_rows, h, torch.bfloat16)).to(torch.bfloat16)
            self.k6.append(ops.TiledRows(data, CAP * 128, h, (CAP, 128, h)))
        self.rescore, self.feat2 = [rows() for _ in range(n_mod)], [rows() for _ in range(n_mod)]
        self.err = [rnd(CAP, 128).abs() * 1e-3 for _ in range(n_mod)]
        self.imask = [(rnd(CAP, 128) > 0).float() for _ in range(n_mod)]
        n_words = CAP if tiles is None else 2 * tiles
        self.bits = [ints(-2 ** 31, 2 ** 31, n_words, 4) for _ in range(n_mod)]
        self.codes = None if tiles is None else ints(-3, CAP, 2 * tiles, 8)
        self.ec = torch.tensor([0.0, 0.5][:n_mod], device=DEV)          # cell 0 is raised; cell 1 is above every norm: it stays
        self.vlen, self.slot_ids = ints(1, 129, CAP), ints(0, 10 ** 6, CAP)
        self.live = torch.tensor([0b100000], dtype=torch.int32, device=DEV)      # slot 5 is live already

    def put(self, batch, masks, slots, ids, runs=None, nb_max=None):
        f1, f2, _ = batch
        rec = (torch.tensor(slots, dtype=torch.int32, device=DEV), torch.tensor(ids, dtype=torch.int32, device=DEV))
        side = (self.k6, self.rescore, self.feat2, self.err, self.imask, self.bits)
        state = (self.ec, self.vlen, self.slot_ids, self.live, L_REF)
        if runs is None:
            ops.index_put_rows_exact(f1, f2, masks, *rec, *side, *state)
        else:
            ops.index_put_rows_packed_exact(f1, f2, masks, *rec, torch.tensor(runs, dtype=torch.int32, device=DEV), nb_max,
                                            *side, self.codes, *state)
        torch.cuda.synchronize()

    def per_slot(self):
        """name -> tensor, everything indexed by slot"""
        out = {"vlen": self.vlen, "slot_ids": self.slot_ids}
        for m in range(self.n_mod):
            out["err%d" % m], out["imask%d" % m] = self.err[m], self.imask[m]
            for nm, t in (("rescore", self.rescore[m]), ("feat2", self.feat2[m])):
                out["%s%d" % (nm, m)] = t.data if self.split else t
                if self.split:
                    out["%s_inv%d" % (nm, m)] = t.inv
        return out

    def image(self, m):
        """(image rows, H) bf16 rows of the flat tile image"""
        h = self.h
        return self.k6[m].data.view(-1, h // 32, 256, 32).permute(0, 2, 1, 3).reshape(-1, h)

    def snapshot(self):
        t = dict(self.per_slot(), ec=self.ec, live=self.live)
        for m in range(self.n_mod):
            t["image%d" % m], t["bits%d" % m] = self.image(m), self.bits[m]
        if self.codes is not None:
            t["codes"] = self.codes
        return {k: v.clone() for k, v in t.items()}


def _effective(masks, runs):
    out = [mk.clone() for mk in masks]
    for i, (_, nb) in enumerate(runs):
        for mk in out:
            mk[i, 16 * nb:] = 0
    return out


def _want_tables(before, masks_eff, slots, runs, n_mod):
    """The code table and the packed mask words after the put, from those before it (numpy; the header's words)."""
    codes = before["codes"].cpu().numpy().reshape(-1).copy()
    words = [before["bits%d" % m].cpu().numpy().reshape(-1).view(np.uint32).copy() for m in range(n_mod)]
    for i, (slot, (first, nb)) in enumerate(zip(slots, runs)):
        for k in range(nb):
            blk = first + k
            codes[blk] = slot if k == nb - 1 else (-3 if blk % 16 == 7 else -1)
            for m in range(n_mod):
                clip = masks_eff[m][i].cpu().numpy()[16 * k:16 * k + 16] != 0
                field = sum(1 << j for j in range(clip.size) if clip[j])
                sh = 16 * (blk & 1)
                words[m][blk >> 1] = (int(words[m][blk >> 1]) & ~(0xFFFF << sh) & 0xFFFFFFFF) | (field << sh)
    return codes, words


@pytest.mark.parametrize("mode,h,n_mod", CASES)
def test_put_equals_the_exact_put_and_the_composition(mode, h, n_mod):
    batch = _batch(h, n_mod)
    f1, f2, masks = batch
    P = Index(mode, h, n_mod, tiles=TILES)
    R = Index(mode, h, n_mod)                                    # the scratch per-slot index
    before = P.snapshot()
    eff = _effective(masks, RUNS)
    assert int(eff[0][0].sum()) == 16 < LB and int(masks[0][0].sum()) == 37      # video 0: keep < lb, the mask is cut
    P.put(batch, masks, SLOTS, IDS, RUNS, 3)
    R.put(batch, eff, SLOTS, IDS)
    after, ref = P.snapshot(), R.snapshot()
    sl = torch.tensor(SLOTS, device=DEV)
    rest = torch.tensor([s for s in range(CAP) if s not in SLOTS], device=DEV)
    # ---- every per-slot operand, the slot state and the bound: the plain exact put's, bitwise; other slots keep theirs
    for name in P.per_slot():
        assert torch.equal(_bits(after[name][sl]), _bits(ref[name][sl])), name
        assert torch.equal(_bits(after[name][rest]), _bits(before[name][rest])), name
    assert torch.equal(_bits(after["ec"]), _bits(ref["ec"])) and float(after["ec"][0]) > 0
    if n_mod == 2:
        assert float(after["ec"][1]) == 0.5                      # the other modality's cell: above every norm, untouched
    assert torch.equal(after["live"], ref["live"]) and int(after["live"][0]) == 0b100100101
    assert after["vlen"][sl].tolist() == [16, 37 if n_mod == 2 else 30, 37, 37 if n_mod == 2 else 5]      # video 0: cut at 16
    assert after["slot_ids"][sl].tolist() == IDS
    # ---- the composition of the existing ops on the batch's rows
    for m in range(n_mod):
        y = ops.l2norm_rows(f1[m])
        fb, err = ops.round_bf16_rows_err(y)
        assert torch.equal(_bits(after["err%d" % m][sl][:, :LB]), _bits(err)) and not bool(after["err%d" % m][sl][:, LB:].any())
        assert torch.equal(_bits(after["ec"][m:m + 1]), _bits(torch.maximum(err.max(), before["ec"][m]).reshape(1)))
        if mode == "f16s":
            rs, s2 = ops.split_f16_rows(y, ops.F16_UNIT_LOG2), ops.split_f16_rows(f2[m])
            for nm, sr in (("rescore", rs), ("feat2", s2)):
                assert torch.equal(after["%s%d" % (nm, m)][sl][:, :LB], sr.data), (nm, m)
                assert torch.equal(_bits(after["%s_inv%d" % (nm, m)][sl][:, :LB]), _bits(sr.inv)), (nm, m)
        else:
            assert torch.equal(_bits(after["rescore%d" % m][sl][:, :LB]), _bits(y))
            assert torch.equal(_bits(after["feat2%d" % m][sl][:, :LB]), _bits(f2[m]))
        # ---- the filter image: rows [0, 16 nb) of each run are the rounded rows, zero from lb on; nothing outside the runs
        image, was = after["image%d" % m], before["image%d" % m]
        ref_rows = R.k6[m].to_rows()
        in_run = torch.zeros(TILES * 256, dtype=torch.bool, device=DEV)
        for i, (slot, (first, nb)) in enumerate(zip(SLOTS, RUNS)):
            run = image[first * 16:(first + nb) * 16]
            in_run[first * 16:(first + nb) * 16] = True
            have = min(16 * nb, LB)
            assert torch.equal(_bits(run[:have]), _bits(fb[i, :have])), (m, slot)
            assert torch.equal(_bits(run), _bits(ref_rows[slot, :16 * nb])) and not bool(run[have:].any()), (m, slot)
        assert torch.equal(_bits(image[~in_run]), _bits(was[~in_run])), m
    # ---- codes and mask words
    codes, words = _want_tables(before, eff, SLOTS, RUNS, n_mod)
    assert (after["codes"].cpu().numpy().reshape(-1) == codes).all()
    assert codes[0] == 2 and codes[1:4].tolist() == [-1, -1, 0] and codes[6:9].tolist() == [-1, -3, 8] and codes[45:48].tolist() == [-1, -1, 5]
    for m in range(n_mod):
        got = after["bits%d" % m].cpu().numpy().reshape(-1).view(np.uint32)
        assert (got == words[m]).all(), m
    w0 = after["bits0"].cpu().numpy().reshape(-1).view(np.uint32)
    assert w0[0] == 0xFFFFFFFF and w0[1] == 0x3FFF                 # blocks 0 | 1 of two videos in one word; 30 clips: 16 + 14 + 0


@pytest.mark.parametrize("mode", ["f32", "f16s"])
def test_bad_records_are_dropped_whole(mode):
    """A slot outside the capacity, a run across a tile boundary, a run longer than nb_max and a run beyond the image:
    nothing of those videos is written; the good record of the same call is."""
    h, n_mod = 256, 2
    batch = _batch(h, n_mod, seed=1)
    P = Index(mode, h, n_mod, tiles=TILES, seed=2)
    before = P.snapshot()
    slots, runs = [CAP, 3, 4, 6], [(20, 2), (14, 3), (24, 4), (47, 2)]
    P.put(batch, batch[2], slots, IDS, runs, 3)
    assert all(torch.equal(_bits(v), _bits(before[k])) for k, v in P.snapshot().items())
    P.put(batch, batch[2], [-1, 3, 4, 6], IDS, [(20, 2), (-1, 2), (24, 0), (48, 1)], 3)
    assert all(torch.equal(_bits(v), _bits(before[k])) for k, v in P.snapshot().items())
    one = Index(mode, h, n_mod, tiles=TILES, seed=2)
    runs[2] = (24, 2)                                                # slot 4: two blocks now, a good record among bad ones
    one.put(batch, batch[2], slots, IDS, runs, 3)
    after = one.snapshot()
    rest = torch.tensor([s for s in range(CAP) if s != 4], device=DEV)
    assert int(after["vlen"][4]) == 32 and int(after["slot_ids"][4]) == IDS[2]      # 37 clips cut at two blocks
    for name in one.per_slot():
        assert torch.equal(_bits(after[name][rest]), _bits(before[name][rest])), name
        assert name in ("vlen", "slot_ids") or not torch.equal(_bits(after[name][4]), _bits(before[name][4])), name
    codes, was = after["codes"].view(-1), before["codes"].view(-1)
    assert codes[24:26].tolist() == [-1, 4]
    keep = torch.ones(TILES * 16, dtype=torch.bool, device=DEV)
    keep[24:26] = False
    assert torch.equal(codes[keep], was[keep])
    for m in range(n_mod):
        rows = torch.ones(TILES * 256, dtype=torch.bool, device=DEV)
        rows[24 * 16:26 * 16] = False
        assert torch.equal(_bits(after["image%d" % m][rows]), _bits(before["image%d" % m][rows])), m
        words = torch.ones(TILES * 8, dtype=torch.bool, device=DEV)
        words[12] = False
        assert torch.equal(after["bits%d" % m].view(-1)[words], before["bits%d" % m].view(-1)[words]), m
    assert int(after["live"][0]) == 0b110000


def test_the_wrapper_checks_shapes_before_the_call():
    from tvretrieval_amd._lib import XmlHipError
    h, n_mod = 256, 2
    batch = _batch(h, n_mod)
    P = Index("f32", h, n_mod, tiles=TILES)
    before = P.snapshot()
    for breakage, match in ((lambda: setattr(P, "bits", [b[:-1] for b in P.bits]), "bits"),
                            (lambda: setattr(P, "codes", P.codes[:-2]), "n_tiles"),
                            (lambda: setattr(P, "ec", P.ec[:1]), "ec"),
                            (lambda: setattr(P, "err", [e[:, :100] for e in P.err]), "err")):
        P_saved = (P.bits, P.codes, P.ec, P.err)
        breakage()
        with pytest.raises(XmlHipError, match=match):
            P.put(batch, batch[2], SLOTS, IDS, RUNS, 3)
        P.bits, P.codes, P.ec, P.err = P_saved
    with pytest.raises(XmlHipError, match="run"):
        P.put(batch, batch[2], SLOTS, IDS, RUNS[:3], 3)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(v), _bits(before[k])) for k, v in P.snapshot().items())
