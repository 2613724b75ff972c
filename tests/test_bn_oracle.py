"""tests/bn_oracle.py pinned on the CPU: the BatchNorm references against torch autograd in fp64, the loss references against
oracle.psmnet_oracle.psm_loss and its autograd, launch_plan against the grids the GPU cases are meant to reach, and the strength of
the GPU tests' input (a mis-weighted or dropped chunk must move the statistics by >= 10x their tolerance)."""
import pytest
import torch
from torch import nn

from oracle import psmnet_oracle as O
from disprcnn_amd.utils import synth
from tests import bn_oracle as B

F64 = torch.float64
REL = 1e-12


def _close(got, ref, what):
    err = float((got - ref).abs().max())
    bar = REL * max(float(ref.abs().max()), 1e-300)
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("shape", [(2, 5, 3, 4, 6), (3, 7, 1, 5, 9)])
@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, False), (True, True)])
def test_bn_oracle_vs_torch_autograd_fp64(shape, with_res, relu):
    N, C, D, H, W = shape
    M = N * D * H * W
    x = (synth.hash_uniform("bno:x", shape).to(F64) * 1.5 + torch.arange(C, dtype=F64).view(1, -1, 1, 1, 1) * 0.3).requires_grad_()
    res = synth.hash_uniform("bno:r", shape).to(F64).requires_grad_() if with_res else None
    dy = synth.hash_uniform("bno:dy", shape, 0.1, 1.0).to(F64)
    bn = nn.BatchNorm3d(C, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(synth.hash_uniform("bno:g", (C,), 0.5, 1.5)); bn.bias.copy_(synth.hash_uniform("bno:b", (C,), -0.5, 0.5))
        bn.running_mean.copy_(synth.hash_uniform("bno:rm", (C,))); bn.running_var.copy_(synth.hash_uniform("bno:rv", (C,), 0.5, 2.0))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    z = bn(x)
    if with_res:
        z = z + res
    y = torch.relu(z) if relu else z
    y.backward(dy)

    mean, var = B.stats(x.detach())
    invstd, rm, rv = B.finalize(mean, var * M, M, bn.eps, bn.momentum, rm0, rv0)
    _close(rm, bn.running_mean, "running_mean")
    _close(rv, bn.running_var, "running_var")
    assert int(bn.num_batches_tracked) == 1
    y_o = B.apply(x.detach(), mean, invstd, bn.weight.detach(), bn.bias.detach(), res.detach() if with_res else None, relu)
    _close(y_o, y.detach(), "forward")
    g = B.bwd(dy, y.detach(), x.detach(), mean, invstd, bn.weight.detach(), relu)
    _close(g["draw"], x.grad, "d raw")
    _close(g["sum_dz"], bn.bias.grad, "d beta")
    _close(g["sum_dz_xhat"], bn.weight.grad, "d gamma")
    if with_res:
        _close(g["dres"], res.grad, "d res")
    assert (g["sum_abs_dz"] >= g["sum_dz"].abs()).all() and (g["sum_abs_dz_xhat"] >= g["sum_dz_xhat"].abs()).all()
    # `sums` handed in replace the reference sums inside draw
    g2 = B.bwd(dy, y.detach(), x.detach(), mean, invstd, bn.weight.detach(), relu, sums=torch.stack([g["sum_dz"], g["sum_dz_xhat"]]))
    assert torch.equal(g2["draw"], g["draw"])


def _loss_case(n, mask_kind):
    tgt = synth.hash_uniform("bno:lt", (n,), 0.0, 48.0).to(F64)
    preds = [(tgt + synth.hash_uniform(f"bno:lp{k}", (n,), -2.5, 2.5).to(F64)).requires_grad_() for k in range(3)]
    mask = {"ones": torch.ones(n, dtype=torch.bool), "zero": torch.zeros(n, dtype=torch.bool),
            "rand": synth.hash_uniform("bno:lm", (n,), 0.0, 1.0) < 0.6}[mask_kind]
    return preds, tgt, mask


@pytest.mark.parametrize("mask_kind", ["ones", "zero", "rand"])
@pytest.mark.parametrize("n", [1, 77, 1000])
def test_loss_oracle_vs_psm_loss_and_its_autograd(n, mask_kind):
    preds, tgt, mask = _loss_case(n, mask_kind)
    s = B.loss_sums(*[p.detach() for p in preds], tgt, mask)
    assert float(s[3]) == float(mask.sum())
    denom = s[3] if s[3] != 0 else torch.ones((), dtype=F64)
    ref = O.psm_loss(preds, tgt, mask)
    _close((0.5 * s[0] + 0.7 * s[1] + s[2]) / denom, ref.detach(), "train loss")
    (ref * 0.37).backward()
    for p, w in zip(preds, (0.5, 0.7, 1.0)):
        g = B.loss_grad(p.detach(), tgt, mask, w, 0.37)
        _close(g, p.grad, f"grad w={w}") if mask.any() else None
        assert torch.equal(g[~mask], torch.zeros_like(g[~mask])) and torch.isfinite(g).all()
    # eval form: the other heads absent
    se = B.loss_sums(preds[0].detach(), None, None, tgt, mask)
    assert float(se[1]) == 0 and float(se[2]) == 0 and torch.equal(se[[0, 3, 4]], s[[0, 3, 4]])
    ref_e = O.psm_loss(preds[0].detach(), tgt, mask)
    got_e = se[4] / se[3] if se[3] != 0 else torch.zeros((), dtype=F64)
    _close(got_e, ref_e, "eval loss") if mask.any() else None
    assert mask.any() or (float(got_e) == 0 and float(ref_e) == 0 and float(ref.detach()) == 0)


def test_loss_oracle_at_the_smooth_l1_knee():
    one = torch.tensor(1.0, dtype=torch.float32)
    d = torch.stack([one, -one, torch.nextafter(one, one * 0), torch.nextafter(one, one * 2), one * 0, one * 3, -one * 3]).to(F64)
    tgt, mask = torch.zeros(7, dtype=F64), torch.ones(7, dtype=torch.bool)
    s = B.loss_sums(d, None, None, tgt, mask)
    ref = torch.nn.functional.smooth_l1_loss(d, tgt, reduction="sum")
    _close(s[0], ref, "knee")
    g = B.loss_grad(d, tgt, mask, 1.0, 1.0) * 7
    assert torch.equal(g, torch.tensor([1.0, -1.0, float(d[2]), 1.0, 0.0, 1.0, -1.0], dtype=F64))


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_launch_plan_reaches_the_intended_grid(name):
    (N, C, D, H, W), _, want = B.CASES[name]
    p = B.launch_plan(N, D, H, W)
    rows = N * D * H
    # the ranges partition [0, rows) in order; empty blocks only at the end
    assert p["rows"] == rows and len(p["ranges"]) == p["blocks"] and p["ranges"][0][0] == 0
    at = 0
    for r0, r1 in p["ranges"]:
        assert r0 == at and r1 >= r0 and (r1 > r0 or at == rows)
        at = r1
    assert at == rows
    assert all(r1 - r0 == p["chunk"] for r0, r1 in p["ranges"][: p["blocks"] - B.grid_of(p)[1] - 1])
    assert p["chunk"] % p["rpb"] == 0
    assert B.grid_of(p) == (want["blocks"], want["empty"], want["last"])
    if "rpb" in want:
        assert p["rpb"] == want["rpb"]


def test_launch_plan_named_regimes():
    P = B.launch_plan
    assert P(1, 1, 3, 5)["rpb"] == 12 and P(1, 1, 3, 5)["chunk"] == 12                       # a: rows in flight exceed the rows
    assert P(2, 12, 112, 112)["chunk"] == 6 and -(-2 * 12 * 112 * 112 // 512) == 588         # k: 588 chunks asked, 512 given
    assert P(2, 12, 112, 112, cap=1 << 20)["blocks"] == 588
    assert P(1, 1, 2, 700)["blocks"] == 2                                                     # l: never more blocks than rows
    assert P(0, 3, 4, 5)["blocks"] == 1 and P(0, 3, 4, 5)["ranges"] == [(0, 0)]              # the launchers return before this
    assert [B.is_ragged(P(*[B.CASES[k][0][i] for i in (0, 2, 3, 4)])) for k in "abcdefghijklmn"] == \
        [False, True, False, True, True, True, True, False, True, False, True, False, True, False]


@pytest.mark.parametrize("name", ["b", "d", "e", "f", "g", "m"])
def test_trend_input_makes_every_chunk_matter(name):
    """The condition the GPU test re-evaluates for every ragged case (here: the ones that cost nothing): both wrong merges sit
    >= 10x the tolerance of the statistics test (1e-5 * max|ref|) from the truth, in mean and in variance."""
    shape = B.CASES[name][0]
    x = B.trend_input(f"trend:{name}", shape)
    p = B.launch_plan(shape[0], *shape[2:])
    mean, var = B.stats(x)
    ns, means, m2s = B.chunk_stats(x, p)
    m_all, m2_all = B.merge_chunks(ns, means, m2s)                     # the exact merge gives the truth back
    assert (m_all - mean).abs().max() <= 1e-12 * mean.abs().max() and (m2_all / ns.sum() - var).abs().max() <= 1e-12 * var.max()
    for mname, (mm, mv) in B.stat_mutants(x, p).items():
        assert (mm - mean).abs().max() >= 10 * 1e-5 * mean.abs().max(), mname
        assert (mv - var).abs().max() >= 10 * 1e-5 * var.abs().max(), mname
