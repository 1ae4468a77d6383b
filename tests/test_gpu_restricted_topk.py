"""K8 over an allowed set of columns (xml_topk_rows_allowed, xml_select_ge_rows_allowed).  Every comparison is bitwise.

The yardstick is the unmasked xml_topk_rows, pinned by test_gpu_kernels.py / test_gpu_fuzz.py: a row's allowed columns are
gathered into a dense row with their column numbers (or payloads) as idx_in, short rows padded with (-inf, 2^31 - 1) as the
sharded merge pads, and the unmasked kernel runs on that.  The first cnt outputs of the masked kernel must be those; the
rest must be the empty-slot values; out_cnt must be the popcount clipped to k."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV, dev, ops  # noqa: F401
from tvretrieval_amd.inference import pack_video_allow

pytestmark = pytest.mark.gpu

ROWS = 6
# 3072 / 3073: the register-resident dispatch; 4095 / 4096: the pre-filter; 8200 with k = 100: the pre-filter is taken
SHAPES = [(n, k) for n in (37, 300, 3072, 3073, 4095, 4096, 8200) for k in (1, 5, 100, 256) if k <= n]
INT_MAX = 2 ** 31 - 1


def _masks(n, k, rng):
    """name -> (ROWS, n) bool"""
    out = {"ones": np.ones((ROWS, n), dtype=bool)}
    for d in (2, 6, 64):
        out["1/%d" % d] = rng.random((ROWS, n)) < 1.0 / d
    for name, a in (("exactly k", k), ("k - 1", k - 1), ("one", 1), ("none", 0)):
        m = np.zeros((ROWS, n), dtype=bool)
        for r in range(ROWS):
            m[r, rng.permutation(n)[:a]] = True
        out[name] = m
    late = np.zeros((ROWS, n), dtype=bool)          # the first 2048 columns (a long row's sample) see nothing
    late[:, min(2048, n // 2):] = rng.random((ROWS, n - min(2048, n // 2))) < 0.5
    out["late only"] = late
    last = np.zeros((ROWS, n), dtype=bool)
    last[:, -1] = True
    out["last column"] = last
    return out


def _scores(kind, mask, rng):
    rows, n = mask.shape
    if kind == "gauss":
        return rng.standard_normal((rows, n)).astype(np.float32)
    if kind == "const":                             # every tie is broken by the column; the mask decides who is in
        return np.full((rows, n), 0.25, dtype=np.float32)
    if kind == "ascending":
        return np.sort(rng.standard_normal((rows, n)).astype(np.float32), axis=1)
    if kind == "allowed -inf":                      # an allowed -inf still ranks above every disallowed column
        return np.where(mask, -np.inf, 10.0 + rng.standard_normal((rows, n))).astype(np.float32)
    raise KeyError(kind)


def _bits(mask, col0, rng, shared=False):
    """Allow words whose bit col0 + c is mask[., c]; the bits before col0 and after col0 + n are noise to be ignored."""
    rows, n = mask.shape
    wide = rng.random((rows, col0 + n + 77)) < 0.5
    wide[:, col0:col0 + n] = mask
    return dev(torch.from_numpy(pack_video_allow(wide[:1] if shared else wide)))


def _want(ops, s, mask, k, alpha, pay=None):
    """The unmasked kernel on the gathered rows: (values, indices, counts)."""
    rows, n = mask.shape
    a = mask.sum(1)
    width = int(max(k, a.max()))
    order = np.argsort(~mask, axis=1, kind="stable")[:, :width]           # allowed columns first, ascending
    if order.shape[1] < width:
        order = np.pad(order, ((0, 0), (0, width - order.shape[1])))
    live = np.arange(width)[None, :] < a[:, None]
    ds = np.where(live, np.take_along_axis(s, order, 1), -np.inf).astype(np.float32)
    src = order if pay is None else np.take_along_axis(pay, order, 1)
    di = np.where(live, src, INT_MAX).astype(np.int32)
    v, i = ops.topk_rows(dev(torch.from_numpy(ds)), k, alpha=alpha, idx_in=dev(torch.from_numpy(di)))
    return v.cpu(), i.cpu(), torch.from_numpy(np.minimum(a, k).astype(np.int32))


def _check(what, got_v, got_i, got_c, want_v, want_i, want_c, k, alpha):
    got_v, got_i, got_c = got_v.cpu(), got_i.cpu(), got_c.cpu()
    assert torch.equal(got_c, want_c), "%s: out_cnt %s vs %s" % (what, got_c.tolist(), want_c.tolist())
    live = torch.arange(k)[None, :] < want_c[:, None].long()
    assert torch.equal(got_i[live], want_i[live]), "%s: indices differ" % what
    assert torch.equal(got_v[live].view(torch.int32), want_v[live].view(torch.int32)), "%s: value bits differ" % what
    assert bool((got_i[~live] == -1).all()), "%s: empty slots must carry index -1" % what
    empty = 0.0 if alpha != 0 else -np.inf
    assert bool((got_v[~live] == empty).all()), "%s: empty slots must carry %r" % (what, empty)


@pytest.mark.parametrize("col0", [0, 1, 31, 45])
@pytest.mark.parametrize("n,k", SHAPES)
def test_masked_topk_equals_unmasked_topk_of_the_allowed_columns(ops, n, k, col0):
    rng = np.random.default_rng(1000 * n + 10 * k + col0)
    names, masks, scores = [], [], []
    for mname, m in _masks(n, k, rng).items():
        for kind in ("gauss", "const", "ascending", "allowed -inf"):
            names.append("%s / %s" % (mname, kind))
            masks.append(m)
            scores.append(_scores(kind, m, rng))
    mask, s = np.concatenate(masks), np.concatenate(scores)
    bits = _bits(mask, col0, rng)
    sd = dev(torch.from_numpy(s))
    for alpha in (0.0, 20.0):
        wv, wi, wc = _want(ops, s, mask, k, alpha)
        gv, gi, gc = ops.topk_rows(sd, k, alpha=alpha, allow=bits, col0=col0, return_count=True)
        for b, name in enumerate(names):
            r = slice(b * ROWS, (b + 1) * ROWS)
            _check("n=%d k=%d col0=%d alpha=%g %s" % (n, k, col0, alpha, name), gv[r], gi[r], gc[r], wv[r], wi[r], wc[r], k, alpha)
        # all ones: also the unmasked kernel on the row itself, bit for bit
        r = slice(0, 4 * ROWS)
        assert names[0].startswith("ones") and names[3].startswith("ones")
        uv, ui = ops.topk_rows(sd[r].contiguous(), k, alpha=alpha)
        assert torch.equal(gi[r], ui) and torch.equal(gv[r].view(torch.int32), uv.view(torch.int32))
        # without out_cnt the lists are the same
        hv, hi = ops.topk_rows(sd, k, alpha=alpha, allow=bits, col0=col0)
        assert torch.equal(hi, gi) and torch.equal(hv.view(torch.int32), gv.view(torch.int32))


@pytest.mark.parametrize("col0", [0, 45])
@pytest.mark.parametrize("n,k", SHAPES)
def test_one_shared_allow_row_serves_every_score_row(ops, n, k, col0):
    rng = np.random.default_rng(77 * n + k + col0)
    s = rng.standard_normal((ROWS, n)).astype(np.float32)
    for d in (1, 2, 6, 64):
        one = rng.random((1, n)) < 1.0 / d
        mask = np.repeat(one, ROWS, axis=0)
        shared = _bits(mask, col0, rng, shared=True)
        assert shared.shape[0] == 1
        for alpha in (0.0, 20.0):
            wv, wi, wc = _want(ops, s, mask, k, alpha)
            gv, gi, gc = ops.topk_rows(dev(torch.from_numpy(s)), k, alpha=alpha, allow=shared, col0=col0, return_count=True)
            _check("shared 1/%d n=%d k=%d col0=%d" % (d, n, k, col0), gv, gi, gc, wv, wi, wc, k, alpha)


@pytest.mark.parametrize("n,k", [(300, 5), (300, 100), (3073, 100), (8200, 100), (8200, 256)])
def test_the_bit_tests_the_column_also_with_payloads(ops, n, k):
    """idx_in payloads repeat on allowed AND disallowed columns (values 0 .. 4, and the scores are coarse, so the threshold
    ties exceed the need): which entries take part is decided by the column's bit, never by the payload's."""
    rng = np.random.default_rng(5 * n + k)
    for d in (1, 2, 6):
        mask = rng.random((ROWS, n)) < 1.0 / d
        s = (np.round(rng.standard_normal((ROWS, n)) * 4) / 4).astype(np.float32)
        pay = rng.integers(0, 5, (ROWS, n)).astype(np.int32)
        bits = _bits(mask, 3, rng)
        for alpha in (0.0, 20.0):
            wv, wi, wc = _want(ops, s, mask, k, alpha, pay=pay)
            gv, gi, gc = ops.topk_rows(dev(torch.from_numpy(s)), k, alpha=alpha, idx_in=dev(torch.from_numpy(pay)), allow=bits,
                                       col0=3, return_count=True)
            _check("payloads 1/%d n=%d k=%d" % (d, n, k), gv, gi, gc, wv, wi, wc, k, alpha)


@pytest.mark.parametrize("col0", [0, 1, 31, 45])
@pytest.mark.parametrize("n", [37, 300, 5000])
def test_masked_select_ge_rows(ops, n, col0):
    rng = np.random.default_rng(31 * n + col0)
    rows = 9
    s = rng.standard_normal((rows, n)).astype(np.float32)
    thr = rng.standard_normal(rows).astype(np.float32)
    thr[0] = -np.inf                                     # exactly the allowed columns
    thr[1] = np.inf
    mask = rng.random((rows, n)) < np.array([1, 1 / 2, 1 / 6, 1 / 64, 0, 1, 1 / 2, 1 / 6, 1 / 2])[:, None]
    want = [np.nonzero(mask[r] & (s[r] >= thr[r]))[0].tolist() for r in range(rows)]
    want_cnt = np.array([len(w) for w in want], dtype=np.int32)
    assert want[0] == np.nonzero(mask[0])[0].tolist() and want_cnt[1] == 0 and want_cnt[4] == 0
    for shared in (False, True):
        m = np.repeat(mask[2:3], rows, axis=0) if shared else mask
        w = [np.nonzero(m[r] & (s[r] >= thr[r]))[0].tolist() for r in range(rows)]
        wc = np.array([len(x) for x in w], dtype=np.int32)
        bits = _bits(m, col0, rng, shared=shared)
        sd, td = dev(torch.from_numpy(s)), dev(torch.from_numpy(thr))
        cnt = ops.select_ge_rows(sd, td, allow=bits, col0=col0).cpu().numpy()
        assert np.array_equal(cnt, wc)
        cap = int(max(1, wc.max()))
        idx, cnt2 = ops.select_ge_rows(sd, td, cap, allow=bits, col0=col0)
        assert np.array_equal(cnt2.cpu().numpy(), wc)
        idx = idx.cpu().numpy()
        for r in range(rows):
            assert sorted(idx[r, :wc[r]].tolist()) == w[r], (r, shared)
            assert (idx[r, wc[r]:] == -1).all()
        small = max(1, cap // 3)                         # a cap smaller than the count: counts stay, cap entries are listed
        idx, cnt3 = ops.select_ge_rows(sd, td, small, allow=bits, col0=col0)
        assert np.array_equal(cnt3.cpu().numpy(), wc)
        idx = idx.cpu().numpy()
        for r in range(rows):
            got = idx[r, :min(small, wc[r])].tolist()
            assert len(set(got)) == len(got) and set(got) <= set(w[r]), (r, shared)
            assert (idx[r, min(small, wc[r]):] == -1).all()


def test_allow_argument_validation(ops):
    s = torch.zeros((4, 100), device=DEV)
    thr = torch.zeros((4,), device=DEV)
    ok = torch.full((4, 4), -1, dtype=torch.int32, device=DEV)
    calls = [lambda **kw: ops.topk_rows(s, 5, **kw), lambda **kw: ops.select_ge_rows(s, thr, **kw)]
    for call in calls:
        call(allow=ok)
        call(allow=ok[:1])
        call(allow=torch.full((4, 5), -1, dtype=torch.int32, device=DEV), col0=45)
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok.to(torch.int64))                                       # dtype
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok.cpu())                                                 # device
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok[:, :3].contiguous())                                   # too few words for 100 columns
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok, col0=29)                                              # ... and for columns 29 .. 128
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok[:3])                                                   # neither 1 nor `rows` rows
        with pytest.raises(ValueError, match="allow"):
            call(allow=ok.reshape(-1))                                           # not a matrix
        with pytest.raises(ValueError, match="col0"):
            call(allow=ok, col0=-1)
        with pytest.raises(ValueError, match="col0"):
            call(col0=3)                                                         # col0 without a mask
    with pytest.raises(ValueError, match="return_count"):
        ops.topk_rows(s, 5, return_count=True)
