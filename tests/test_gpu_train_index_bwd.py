"""The query-gradient entries of include/xmlhip_train_index.h -- xml_q2c_scores_arg_bwd_q and xml_pair_sim_bwd_q -- on the
operand lists of tests/train_bf16_cases.py (scores_cases: a fully masked video, an all-zero clip row, one and two modalities;
pair_sim_case) against float64:
* bf16: the block-wise yardstick train_bf16_cases.check_blocks with C_TRAIN_CHAIN of tests/test_gpu_train_bf16.py for the
  scores' dq (a chain: the normalised rows are a bf16 store) -- against the block's own staged error, exactly W where the staged
  reference is exactly W --, and for the pair similarity's dq (one store from exact operands) that module's
  check_bf16_rounding with C_ALLOW besides;
* f32: max|G - W| / max|W| within tests/test_gpu_train.py's figures for the same gradients (5e-5 scores, 2e-5 pair-sim), and
  within its 1e-6 of the dq the existing one-launch entries write on the same operands;
* exactly zero wherever the exact gradient is exactly zero, and equal bits from two runs of the same call (no atomics: a
  row's sum has one order)."""
import pytest
import torch

import numerics_regimes as NR
import train_bf16_cases as TC
from test_gpu_kernels import DEV
from test_gpu_train import check
from test_gpu_train_bf16 import C_ALLOW, C_TRAIN_CHAIN, _d

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SCORES = [c for c in TC.scores_cases() if c.cfg["fused"]]          # (the padded variants hold the same operands)
DH = 32                                                            # column block of check_blocks: divides 64 and 128


def _scores_dq(case, dt):
    """-> (dq per modality from xml_q2c_scores_arg_bwd_q, the sets, dscores, scale) on the case's operands in dtype dt."""
    from tvretrieval_amd import ops, train_ops as TO
    n_mod = case.cfg["n_mod"]
    sets, feats, scores = [], [], None
    for i in range(n_mod):
        query, feat = case.leaves[i].to(DEV).to(dt), case.leaves[n_mod + i].to(DEV).to(dt)
        mask = case.cfg["masks"][i].to(DEV).contiguous()
        qn, cn = ops.l2norm_rows(query), ops.l2norm_rows(feat)
        if scores is None:
            scores, arg = TO.q2c_scores_arg(qn, cn, mask)
        else:
            _, arg = TO.q2c_scores_arg(qn, cn, mask, out=scores, combine=True)
        sets.append((query, qn, cn, mask, arg))
        feats.append(feat)
    ds = case.gouts[0].to(DEV).contiguous()
    return TO.q2c_scores_arg_bwd_q(sets, ds, scale=1.0 / n_mod), sets, feats, ds, 1.0 / n_mod


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", SCORES, ids=TC.ids(SCORES))
def test_q2c_scores_arg_bwd_q_against_float64(case, dt):
    from tvretrieval_amd import train_ops as TO
    n_mod = case.cfg["n_mod"]
    dq, sets, feats, ds, scale = _scores_dq(case, dt)
    again = TO.q2c_scores_arg_bwd_q(sets, ds, scale=scale)
    (_, Wg), (_, Sg) = case.refs()["W"], case.refs()["S"]
    for i in range(n_mod):
        G, W, S = dq[i], Wg[i], Sg[i]
        assert G.dtype == dt and G.shape == W.shape and bool(torch.isfinite(G).all())
        assert torch.equal(G.view(torch.int16 if dt == BF16 else torch.int32), again[i].view(torch.int16 if dt == BF16 else torch.int32))
        assert bool((_d(G)[W == 0] == 0).all())
        name = "xml_q2c_scores_arg_bwd_q.dq%d" % i
        if dt == BF16:
            TC.check_blocks(name, case.name, G[None], W[None], S[None], DH, C_TRAIN_CHAIN)
        else:
            check(name, G, W, 5e-5)
            # the existing one-launch entry on the same saved tensors (its dfeat half is what the new entry leaves out)
            query, qn, cn, mask, arg = sets[i]
            old_dq, _ = TO.q2c_scores_l2norm_bwd(query, feats[i], qn, cn, mask, ds, scale=scale, arg=arg)
            check(name + " vs xml_q2c_scores_l2norm_bwd", G, old_dq, 1e-6)
    assert float(dq[0].float().abs().max()) > 0


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_pair_sim_bwd_q_against_float64(dt):
    from tvretrieval_amd import train_ops as TO
    case = TC.pair_sim_case()
    q, f2 = (t.to(DEV).to(dt) for t in case.leaves)
    dsim = case.gouts[0].to(DEV).contiguous()
    G = TO.pair_sim_bwd_q(f2, dsim)
    assert G.dtype == dt and G.shape == q.shape and torch.equal(G.view(torch.uint8), TO.pair_sim_bwd_q(f2, dsim).view(torch.uint8))
    refs = case.refs()
    W, S, R = refs["W"][1][0], refs["S"][1][0], refs["R"][1][0]
    name = "xml_pair_sim_bwd_q.dq"
    if dt == BF16:
        NR.check_bf16_rounding(name, case.name, _d(G), W, R, C_ALLOW, strict=True, cap=False)
        TC.check_blocks(name, case.name, G[None], W[None], S[None], DH, C_TRAIN_CHAIN)
    else:
        check(name, G, W, 2e-5)
        old_dq, _ = TO.pair_sim_bwd(q, f2, dsim)
        check(name + " vs xml_pair_sim_bwd", G, old_dq, 1e-6)
