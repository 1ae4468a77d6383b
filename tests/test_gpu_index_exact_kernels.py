"""The two small entries of include/xmlhip_index_exact.h against what they replace: xml_exact_certificate_dev against
xml_exact_certificate on the same inputs (the bound by pointer instead of by value), xml_index_exact_bound against torch."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from tvretrieval_amd import ops

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    """distance in units of the last place between two positive finite f32 tensors"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


@pytest.mark.parametrize("n_mod", [1, 2])
@pytest.mark.parametrize("alpha", [0.0, 20.0])
def test_certificate_dev_equals_the_certificate_by_value(n_mod, alpha):
    nq, m, k = 500, 64, 10
    g = torch.Generator().manual_seed(2)
    filt = torch.sort(torch.rand(nq, m, generator=g) * 0.02 + 0.3, dim=1, descending=True)[0].contiguous().to(DEV)
    top = torch.sort(torch.rand(nq, k, generator=g) * 0.02 + 0.3, dim=1, descending=True)[0].contiguous().to(DEV)
    eq = [(torch.rand(nq, generator=g) * 1e-3).to(DEV) for _ in range(n_mod)]
    ec = [0.9e-3, 1.1e-3][:n_mod]
    base, c2 = 1e-4, 4.0
    tv_a, tv_b = top.clone(), top.clone()
    # the same inputs: the by-value entry takes its bound as f32 arguments and ONE slack, the sum the other entry forms in
    # f32 from the same cells (4 x is exact, so the f32 sum is one rounding whether or not the kernel fuses it)
    ec32 = [np.float32(x) for x in ec]
    slack = float(np.float32(base) + np.float32(c2) * (max(ec32) * max(ec32)))
    want = ops.exact_certificate(filt, tv_a, eq, ec, slack, alpha, True)
    got = ops.exact_certificate_dev(filt, tv_b, eq, torch.tensor(ec, dtype=torch.float32, device=DEV), base, c2, alpha, True)
    (fail_w, eps_w, thr_w, nf_w), (fail_g, eps_g, thr_g, nf_g) = want, got
    worst = int(_ulps(eps_g, eps_w).max())
    dbl = ops.exact_certificate(filt, top.clone(), eq, ec, base + c2 * max(ec) ** 2, alpha, True)
    print("eps: %d ulp apart at most; %d ulp from the slack summed in double on the host" % (worst, int(_ulps(eps_g, dbl[1]).max())))
    assert worst <= 2 and int(_ulps(eps_g, dbl[1]).max()) <= 2
    assert torch.equal(fail_g, fail_w) and int(nf_g.item()) == int(nf_w.item()) == int(fail_g.sum().item())
    assert 0 < int(nf_g.item()) < nq
    assert torch.equal(tv_a, tv_b)                              # exp(alpha s), or the raw values at alpha == 0
    assert torch.equal(tv_b, top) == (alpha == 0.0)
    assert torch.equal(thr_g, thr_w)
    # the bound is read when the kernel runs: a changed cell changes the next call, with no new argument
    cells = torch.tensor(ec, dtype=torch.float32, device=DEV)
    a = ops.exact_certificate_dev(filt, top.clone(), eq, cells, base, c2, alpha, True)
    cells.fill_(10.0)
    b = ops.exact_certificate_dev(filt, top.clone(), eq, cells, base, c2, alpha, True)
    assert int(b[3].item()) == nq > int(a[3].item()) and bool((b[1] > 10.0).all())
    # no videos outside the candidate set: nothing can fail
    c = ops.exact_certificate_dev(filt, top.clone(), eq, cells, base, c2, alpha, False)
    assert int(c[3].item()) == 0 and not bool(c[0].any())


@pytest.mark.parametrize("n_mod", [1, 2])
@pytest.mark.parametrize("slack_ec2", [0.0, 4.0])
def test_an_infinite_cell_fails_every_certificate_and_selects_everything(n_mod, slack_ec2):
    """A NaN norm raises a cell to +inf (the header): eps must then be +inf and the second tier's line -inf in both exact modes
    -- slack_ec2 = 0 is mode "f32", where 0 * inf^2 would be a NaN that selects nothing."""
    nq, m, k = 70, 20, 10
    g = torch.Generator().manual_seed(4)
    filt = torch.sort(torch.rand(nq, m, generator=g), dim=1, descending=True)[0].contiguous().to(DEV)
    top = torch.sort(torch.rand(nq, k, generator=g) + 1.0, dim=1, descending=True)[0].contiguous().to(DEV)   # passes a finite bound
    eq = [(torch.rand(nq, generator=g) * 1e-3).to(DEV) for _ in range(n_mod)]
    eq[0][3] = 0.0                                              # a query without rounding error: still 0 * inf nowhere
    inf_ = float("inf")
    for hot in range(n_mod):                                    # either cell alone is enough
        cells = torch.full((n_mod,), 1e-3, device=DEV)
        tv_ok = top.clone()
        ok = ops.exact_certificate_dev(filt, tv_ok, eq, cells, 1e-4, slack_ec2, 20.0, True) + (tv_ok,)
        assert int(ok[3].item()) == 0 and bool(torch.isfinite(ok[1]).all())
        cells[hot] = inf_
        tv = top.clone()
        fail, eps, thr, n_fail = ops.exact_certificate_dev(filt, tv, eq, cells, 1e-4, slack_ec2, 20.0, True)
        assert bool((eps == inf_).all()) and bool((thr == -inf_).all()), (hot, eps[:4], thr[:4])
        assert bool((fail == 1).all()) and int(n_fail.item()) == nq
        assert torch.equal(tv, ok[4])                           # the transform is untouched by the bound
        cand, cnt = ops.select_ge_rows(filt, thr, m)            # the line the second tier selects by: every column
        assert bool((cnt == m).all()) and bool((cand >= 0).all())


@pytest.mark.parametrize("cap,lpad,n_mod", [(70, 128, 2), (37, 48, 1), (1000, 112, 2)])
def test_exact_bound_equals_torch(cap, lpad, n_mod):
    g = torch.Generator().manual_seed(cap)
    err = [(torch.rand(cap, lpad, generator=g) * 1e-2).to(DEV) for _ in range(n_mod)]
    live = torch.rand(cap, generator=g) < 0.5
    live[cap - 1] = True                                        # the last slot, in the ragged last word
    top = int(torch.argmax(err[0].amax(1)))
    live[top] = False                                           # the slot with the largest norm is free: not counted
    from tvretrieval_amd.inference import pack_video_allow
    words = pack_video_allow(live.to(DEV)).view(-1)
    ec = torch.full((n_mod,), -1.0, device=DEV)
    ops.index_exact_bound(err, words, ec)
    want = torch.stack([e[live.to(DEV)].max() for e in err])
    assert torch.equal(ec, want) and float(ec[0]) < float(err[0].max())
    # an empty live set: 0 in every cell
    ops.index_exact_bound(err, torch.zeros_like(words), ec)
    assert torch.equal(ec, torch.zeros(n_mod, device=DEV))
    # a NaN norm counts as +inf (the certificate then fails for every query), a free slot's NaN does not count
    err[0][cap - 1, 3] = float("nan")
    err[n_mod - 1][top, 0] = float("nan")
    ops.index_exact_bound(err, words, ec)
    assert float(ec[0]) == float("inf") and (n_mod == 1 or float(ec[1]) == float(want[1]))
