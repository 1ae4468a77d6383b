"""The per-slot state that a put and a clear of an updatable index leave (include/xmlhip.h "In-place updates of a resident
index", include/xmlhip_index.h, include/xmlhip_index_exact.h), at the ops level and on masks the index suites never put: no
valid clip at all, a valid clip in the upper 64 clips only, holes, the two sides of the 64-clip boundary, a valid length that
only the OTHER modality gives, and one beyond l_ref.  The index tensors are the test's own, pre-filled with sentinels; the
expectation is computed in torch on the host from the headers' rule:
  imask   the batch mask (the packed form: AND clip < 16 nb), 0 from lb on        bits   bit c = imask[c] != 0
  vlen    max over the modalities of (last c with imask[c] != 0) + 1, l_ref when there is none, at most l_ref
  slot_ids = the id given, else the slot; the slot's live bit set; feat2 rows [0, lb) = f2, zero from lb on
  K6 rows  F.normalize(f1) (to rounding; the bitwise pin is the index suites'), zero from lb on
  a clear: live bit off, mask row and mask bits 0, vlen = l_ref -- slot_ids and the feature rows stay
and EVERY element of every tensor is compared, so a slot that no record names must still hold its sentinel."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import DEV, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

CAP, H = 70, 128                                   # three live words
SLOTS = [0, 31, 32, 33, 63, 69]
IDS = [1000, -3, 7, 2 ** 31 - 1, 12, 70]
S_MASK, S_BITS, S_VLEN, S_ID, S_FEAT, S_CODE = -7.0, 0x5A5A5A5A, -5, -9, 3.5, -7
S_LIVE = [1 << 1, 1 << (34 - 32), 1 << (68 - 64)]  # slots 1, 34 and 68 live from the start: their bits must survive

# (video modality clips, sub modality clips, the vlen the headers' rule gives with two modalities)
L128 = dict(lpad=128, lb=112, l_ref=100, masks=[
    ((), (), 100),                  # no valid clip -> l_ref; all bits 0
    ((0,), (), 1),                  # lower ballot word
    ((), (111,), 100),              # clip lb - 1 of the OTHER modality only: min(lb, l_ref)
    ((3, 70), (), 71),              # holes, upper ballot word
    ((63,), (), 64),                # word boundary, lower side
    ((64,), (), 65),                # word boundary, upper side
    ((110,), (), 100)])             # the clamp to l_ref
L48 = dict(lpad=48, lb=37, l_ref=40, masks=[
    ((), (), 40), ((0,), (), 1), ((), (36,), 37), ((3, 30), (), 31), ((31,), (), 32), ((32,), (), 33)])


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _live_bit(slot):
    """The slot's bit of its live word as an int32 value."""
    return (1 << (slot & 31)) - (2 ** 32 if (slot & 31) == 31 else 0)


def _words(bits01):
    """(..., 32 k) 0 / 1 -> (..., k) int32 words, bit j of word w = element 32 w + j."""
    b = bits01.to(torch.int64).reshape(bits01.shape[:-1] + (-1, 32))
    w = (b << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


class _Index(object):
    """The tensors of one updatable index on the device (`dev`) and what the rule says they hold (`want`, on the host)."""

    def __init__(self, ops, n_mod, lpad, l_ref, form, n_tiles=2):
        self.ops, self.n_mod, self.lpad, self.l_ref, self.form, self.n_tiles = ops, n_mod, lpad, l_ref, form, n_tiles
        kdt = torch.bfloat16 if form == "exact" else torch.float32
        self.tiled = lpad == 128 and ops.q2c_tiled_ok(128, H, kdt)      # (the bf16 filter image of H = 128 is row-major)
        assert self.tiled or lpad != 128 or form == "exact"
        rows = n_tiles * 256 if form == "packed" else CAP * lpad
        mods = range(n_mod)
        w = self.want = dict(
            k6=[torch.full((rows if self.tiled else CAP * lpad, H), S_FEAT) for _ in mods],
            feat2=[torch.full((CAP, lpad, H), S_FEAT) for _ in mods],
            imask=[torch.full((CAP, lpad), S_MASK) for _ in mods],
            bits=[torch.full((2 * n_tiles if form == "packed" else CAP, 4), S_BITS, dtype=torch.int32) for _ in mods],
            vlen=torch.full((CAP,), S_VLEN, dtype=torch.int32), slot_ids=torch.full((CAP,), S_ID, dtype=torch.int32),
            live=torch.tensor(S_LIVE, dtype=torch.int32))
        if form == "packed":
            w["codes"] = torch.full((2 * n_tiles, 8), S_CODE, dtype=torch.int32)
        d = self.dev = {k: [t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV) for k, v in w.items()}
        if self.tiled:      # the sentinel is the same in every element, so the tile image of the sentinel rows is flat
            d["k6"] = [ops.TiledRows(torch.full((ops.q2c_tiled_numel(rows, H, kdt),), S_FEAT, dtype=kdt, device=DEV),
                                     CAP * lpad, H, (CAP, lpad, H)) for _ in mods]
        else:
            d["k6"] = [t.to(kdt).view(CAP, lpad, H) for t in d["k6"]]
        if form == "exact":
            d["rescore"] = [torch.full((CAP, lpad, H), S_FEAT, device=DEV) for _ in mods]
            d["err"] = [torch.full((CAP, lpad), S_FEAT, device=DEV) for _ in mods]
            d["ec"] = torch.zeros((n_mod,), device=DEV)

    # ---- the library
    def put(self, f1, f2, masks, slots, ids, runs=None):
        o, d = self.ops, self.dev
        dev = lambda ts: [t.to(DEV) for t in ts]                                          # noqa: E731
        batch = (dev(f1), dev(f2), dev(masks), _i32(slots), None if ids is None else _i32(ids))
        state = (d["vlen"], d["slot_ids"], d["live"], self.l_ref)
        if self.form == "packed":
            o.index_put_rows_packed(*batch, _i32(runs), max(nb for _, nb in runs), d["k6"], d["feat2"], d["imask"], d["bits"],
                                    d["codes"], *state)
        elif self.form == "exact":
            o.index_put_rows_exact(*batch, d["k6"], d["rescore"], d["feat2"], d["err"], d["imask"], d["bits"], d["ec"], *state)
        else:
            o.index_put_rows(*batch, d["k6"], d["feat2"], d["imask"], d["bits"], *state)
        self._want_put(f1, f2, masks, slots, ids, runs)

    def clear(self, slots, runs=None):
        d = self.dev
        if self.form == "packed":
            self.ops.index_clear_rows_packed(_i32(slots), _i32(runs), 8, d["imask"], d["bits"], d["codes"], d["vlen"], d["live"],
                                             self.l_ref)
        else:
            self.ops.index_clear_rows(_i32(slots), d["imask"], d["bits"], d["vlen"], d["live"], self.l_ref)
        w = self.want
        for i, s in enumerate(slots):
            if runs is not None:
                first, nb = runs[i]
                w["codes"].view(-1)[first:first + nb] = -2
                for m in range(self.n_mod):
                    w["bits"][m].view(-1).view(torch.int16)[first:first + nb] = 0      # (little endian: half b of the words)
            if s < 0:
                continue
            for m in range(self.n_mod):
                w["imask"][m][s] = 0.
                if runs is None:
                    w["bits"][m][s] = 0
            w["vlen"][s] = self.l_ref
            w["live"][s >> 5] &= ~_live_bit(s)

    # ---- the rule
    def _want_put(self, f1, f2, masks, slots, ids, runs):
        w, lpad, lb = self.want, self.lpad, masks[0].shape[1]
        last = torch.zeros(len(slots), dtype=torch.int64)
        for m in range(self.n_mod):
            for i, s in enumerate(slots):
                keep = lpad if runs is None else 16 * runs[i][1]
                row = torch.zeros(128)
                row[:min(lb, keep)] = masks[m][i, :min(lb, keep)]
                w["imask"][m][s] = row[:lpad]
                valid = (row != 0).nonzero().view(-1)
                last[i] = max(int(last[i]), int(valid[-1]) + 1 if valid.numel() else 0)
                if runs is None:
                    w["bits"][m][s] = _words(row != 0)
                    base = s * lpad
                else:
                    first, nb = runs[i]
                    w["bits"][m].view(-1).view(torch.int16)[first:first + nb] = self._halves(row != 0, nb)
                    base = first * 16
                w["feat2"][m][s] = 0.
                w["feat2"][m][s, :lb] = f2[m][i]
                k = min(lpad, keep)
                w["k6"][m][base:base + k] = 0.
                w["k6"][m][base:base + min(lb, k)] = F.normalize(f1[m][i, :min(lb, k)], dim=-1)
        for i, s in enumerate(slots):
            w["vlen"][s] = min(int(last[i]) or self.l_ref, self.l_ref)
            w["slot_ids"][s] = s if ids is None else ids[i]
            w["live"][s >> 5] |= _live_bit(s)
            if runs is not None:
                first, nb = runs[i]
                for b in range(first, first + nb):
                    w["codes"].view(-1)[b] = s if b == first + nb - 1 else (-3 if (b & 15) == 7 else -1)

    @staticmethod
    def _halves(bits01, nb):
        """The 16 bits of each of the run's nb blocks as int16 half-words."""
        h = (bits01[:16 * nb].to(torch.int64).view(nb, 16) << torch.arange(16)).sum(-1)
        return torch.where(h >= 2 ** 15, h - 2 ** 16, h).to(torch.int16)

    # ---- the comparison: every element of every tensor
    def k6_rows(self, m):
        k6 = self.dev["k6"][m]
        if not self.tiled:
            return k6.float().reshape(-1, H).cpu()
        per = 64 // k6.data.element_size()
        return k6.data.view(-1, H // per, 256, per).permute(0, 2, 1, 3).reshape(-1, H).float().cpu()

    def check(self, what):
        torch.cuda.synchronize()
        w, d = self.want, self.dev
        for name in ("vlen", "slot_ids", "live") + (("codes",) if self.form == "packed" else ()):
            assert torch.equal(d[name].cpu(), w[name]), "%s: %s\n%s\n%s" % (what, name, d[name].cpu(), w[name])
        for m in range(self.n_mod):
            for name in ("imask", "bits", "feat2"):
                got = d[name][m].cpu()
                bad = (got != w[name][m]).nonzero()
                assert not bad.numel(), "%s: %s[%d] differs at %s ..." % (what, name, m, bad[:4].tolist())
            tol = 2 ** -8 if self.form == "exact" else 1e-6      # unit-norm rows: bf16 rounding / f32 rounding of the division
            err = (self.k6_rows(m) - w["k6"][m]).abs()
            assert float(err.max()) <= tol, "%s: k6[%d] off by %g at row %d" % (what, m, err.max(), int(err.amax(1).argmax()))


def _batch(spec, n_mod, rows=None, seed=0):
    """f1, f2, masks (per-modality lists of host tensors) of the spec's mask rows `rows` (default: the first six)."""
    g = torch.Generator().manual_seed(seed)
    rows = list(range(len(SLOTS))) if rows is None else rows
    lb = spec["lb"]
    f1 = [torch.randn((len(rows), lb, H), generator=g) for _ in range(n_mod)]
    f2 = [torch.randn((len(rows), lb, H), generator=g) for _ in range(n_mod)]
    masks = [torch.zeros((len(rows), lb)) for _ in range(n_mod)]
    for i, r in enumerate(rows):
        for m in range(n_mod):
            for c in spec["masks"][r][m]:
                masks[m][i, c] = 1.
    return f1, f2, masks


def test_mask_table_is_the_rule():
    """The vlen column of the tables above is what the rule gives (two modalities), so the tables say what they claim."""
    for spec in (L128, L48):
        for v, s, vlen in spec["masks"]:
            last = max([c + 1 for c in v + s] or [0])
            assert min(last or spec["l_ref"], spec["l_ref"]) == vlen


@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noids"])
@pytest.mark.parametrize("n_mod", [1, 2])
@pytest.mark.parametrize("spec", [L128, L48], ids=["lpad128_tiled", "lpad48_rowmajor"])
def test_put_and_clear_plain(ops, spec, n_mod, with_ids):
    ix = _Index(ops, n_mod, spec["lpad"], spec["l_ref"], "plain")
    ix.put(*_batch(spec, n_mod), SLOTS, IDS if with_ids else None)
    ix.check("put")
    if len(spec["masks"]) > len(SLOTS):      # the seventh mask (the clamp), over live slots and out of slot order
        ix.put(*_batch(spec, n_mod, rows=[6, 0, 3], seed=1), [63, 0, 32], [5, 6, 8] if with_ids else None)
        ix.check("replace")
    ix.clear([69, 0, 32])
    ix.check("clear")


@pytest.mark.parametrize("n_mod", [1, 2])
@pytest.mark.parametrize("spec", [L128, L48], ids=["lpad128_tiled", "lpad48_rowmajor"])
def test_put_exact_state_is_the_plain_put_state(ops, spec, n_mod):
    """Exact-rank mode (f32 re-score rows): the per-slot state is bitwise the plain form's for the same batch."""
    plain = _Index(ops, n_mod, spec["lpad"], spec["l_ref"], "plain")
    exact = _Index(ops, n_mod, spec["lpad"], spec["l_ref"], "exact")
    rows = [6, 1, 2, 3, 4, 5] if len(spec["masks"]) > len(SLOTS) else None
    for ix in (plain, exact):
        ix.put(*_batch(spec, n_mod, rows), SLOTS, IDS)
    exact.check("exact put")
    for name in ("vlen", "slot_ids", "live"):
        assert torch.equal(exact.dev[name], plain.dev[name]), name
    for m in range(n_mod):
        for name in ("imask", "bits", "feat2"):
            assert torch.equal(exact.dev[name][m], plain.dev[name][m]), name


@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noids"])
@pytest.mark.parametrize("n_mod", [1, 2])
def test_put_and_clear_packed(ops, n_mod, with_ids):
    """Runs (first block, blocks): (6, 4) straddles blocks 7 and 8 -- codes -1, -3, -1, slot; (2, 1) and (3, 1) share one bits
    word; the mask {3, 70} of the 4-block run is valid beyond 16 nb = 64 and is cut there (vlen 4)."""
    runs = [(6, 4), (2, 1), (3, 1), (16, 8)]
    slots, rows = [69, 0, 33, 63], [3, 1, 2, 6]
    ix = _Index(ops, n_mod, 128, L128["l_ref"], "packed")
    f1, f2, masks = _batch(L128, n_mod, rows)
    if n_mod == 2:
        masks[1][2, 111], masks[1][2, 10] = 0., 1.      # the one-block video: its sub mask alone gives the length, inside the run
    ix.put(f1, f2, masks, slots, [IDS[0], IDS[1], IDS[3], IDS[2]] if with_ids else None, runs)
    ix.check("put")
    assert ix.want["codes"].view(-1)[6:10].tolist() == [-1, -3, -1, 69]
    assert ix.want["vlen"][[69, 0, 33, 63]].tolist() == [4, 1, 11 if n_mod == 2 else 100, 100]
    ix.clear([0, -1, 63], [(2, 1), (3, 1), (16, 8)])    # slot -1: the run alone, slot 33 stays live
    ix.check("clear")
