"""The BatchNorm kernels of pts/pn2_bn.hip (layers/pn2_mlp.py:bn_act_train) on the MI355X against torch on the CPU in fp64, forward and
backward, at the shapes where each path can break: row length 1, n = 2, one past a wavefront and a workgroup with odd rows (the scalar
path), aligned rows (the 16-byte path), a partial chunk and exact chunks.

Bound (the one tests/test_hip_rpn.py applies to kernels): err <= 2 * e32 + 1e-6 * max|ref| per compared tensor, e32 the error of
torch.nn.BatchNorm1d's own fp32 CPU run (+ ReLU, + autograd) against the fp64 run.  Compared: z, gy, ggamma, gbeta, the saved mean and
the updated running_mean / running_var.  gamma has a zero and a negative entry where the shape has the channels for them, and the last
channel of a shape with four or more is constant (with a constant upstream gradient): there x_hat = 0, z = act(beta) and gy = 0 exactly.
"""
import numpy as np
import pytest
import torch

from tests import rpn_train_oracle as TO

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOMENTUM = 1e-5, 0.1


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()


def chunk():
    from disprcnn_amd.layers import pn2_mlp
    from disprcnn_amd.pts import _lib
    assert _lib.lib().drc_pn2_bn_chunk() == pn2_mlp.BN_CHUNK
    return pn2_mlp.BN_CHUNK


def shapes():
    from disprcnn_amd.layers.pn2_mlp import BN_CHUNK
    return [(2, 1, 1), (3, 3, 1), (1, 5, 2), (2, 7, 65), (1, 4, 257), (2, 16, 64), (3, 33, BN_CHUNK + 4), (1, 2, 2 * BN_CHUNK)]


def make_case(shape, seed):
    B, C, N = shape
    rs = np.random.RandomState(seed)
    y = (rs.normal(0.0, 1.0, shape) * rs.uniform(0.5, 2.0, (1, C, 1)) + rs.normal(0.0, 1.0, (1, C, 1))).astype(np.float32)
    gz = rs.normal(0.0, 1.0, shape).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rs.normal(0.0, 0.5, C).astype(np.float32)
    if C >= 2:
        gamma[1] = 0.0
    if C >= 3:
        gamma[2] = -0.8
    const = C - 1 if C >= 4 else None
    if const is not None:
        y[:, const] = 0.75
        gz[:, const] = 0.5
    rm = rs.normal(0.0, 0.1, C).astype(np.float32)
    rv = rs.uniform(0.75, 1.25, C).astype(np.float32)
    settle(y, gamma, beta)
    return dict(y=y, gz=gz, gamma=gamma, beta=beta, rm=rm, rv=rv, const=const)


def pre_activation(y, gamma, beta):
    y = y.astype(np.float64)
    xh = (y - y.mean((0, 2), keepdims=True)) / np.sqrt(y.var((0, 2), keepdims=True) + EPS)
    return gamma.astype(np.float64)[None, :, None] * xh + beta.astype(np.float64)[None, :, None]


def settle(y, gamma, beta):
    """A condition on the inputs, not a tolerance: no pre-ReLU value (fp64) within 1e-5 of the tensor's largest, so that the ReLU mask
    cannot differ between fp32 and fp64 and pass for, or hide, an arithmetic error.  Offending inputs are moved by 0.01 until none is
    left; asserted at the end."""
    for _ in range(50):
        pre = np.abs(pre_activation(y, gamma, beta))
        near = pre < TO.COND_REL * pre.max()
        if not near.any():
            return
        y[near] += np.float32(0.01)
    raise AssertionError("the inputs keep a pre-ReLU value next to zero")


def torch_fp32(case, relu):
    """torch.nn.BatchNorm1d's own fp32 run on the CPU: the error unit"""
    bn = torch.nn.BatchNorm1d(case["y"].shape[1], eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(case["gamma"]))
        bn.bias.copy_(torch.from_numpy(case["beta"]))
        bn.running_mean.copy_(torch.from_numpy(case["rm"]))
        bn.running_var.copy_(torch.from_numpy(case["rv"]))
    y = torch.from_numpy(case["y"]).clone().requires_grad_()
    z = bn.train()(y)
    if relu:
        z = torch.relu(z)
    z.backward(torch.from_numpy(case["gz"]))
    return dict(z=z.detach().numpy(), gy=y.grad.numpy(), ggamma=bn.weight.grad.numpy(), gbeta=bn.bias.grad.numpy(),
                mean=case["y"].astype(np.float32).mean((0, 2), dtype=np.float32), running_mean=bn.running_mean.numpy(),
                running_var=bn.running_var.numpy())


def hip(case, relu):
    from disprcnn_amd.layers import pn2_mlp
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    y = t(case["y"]).requires_grad_()
    g, b = t(case["gamma"]).requires_grad_(), t(case["beta"]).requires_grad_()
    rm, rv = t(case["rm"]), t(case["rv"])
    z, stats = pn2_mlp.bn_act_train(y, g, b, rm, rv, MOMENTUM, EPS, relu, return_stats=True)
    z.backward(t(case["gz"]))
    torch.cuda.synchronize()
    return dict(z=z.detach().cpu().numpy(), gy=y.grad.cpu().numpy(), ggamma=g.grad.cpu().numpy(), gbeta=b.grad.cpu().numpy(),
                mean=stats[0].cpu().numpy(), invstd=stats[1].cpu().numpy(), running_mean=rm.cpu().numpy(), running_var=rv.cpu().numpy())


NAMES = ("z", "gy", "ggamma", "gbeta", "mean", "running_mean", "running_var")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "identity"])
@pytest.mark.parametrize("k", range(8))
def test_forward_and_backward_match_fp64(k, relu):
    chunk()
    shape = shapes()[k]
    case = make_case(shape, 300 + k)
    ref = TO.bn_step(case["y"], case["gamma"], case["beta"], case["rm"], case["rv"], case["gz"], relu, MOMENTUM, EPS)
    r32 = torch_fp32(case, relu)
    got = hip(case, relu)
    bad = []
    for name in NAMES:
        e32 = np.abs(r32[name].astype(np.float64) - ref[name]).max()
        err = np.abs(got[name].astype(np.float64) - ref[name]).max()
        bound = 2 * e32 + 1e-6 * np.abs(ref[name]).max()
        print(f"{shape} relu={relu} {name}: err {err:.3g}, torch fp32 {e32:.3g}, bound {bound:.3g}")
        assert np.isfinite(got[name]).all(), name
        if err > bound:
            bad.append(name)
    assert not bad, bad
    c = case["const"]
    if c is not None:
        want = max(case["beta"][c], 0) if relu else case["beta"][c]
        assert (got["z"][:, c] == np.float32(want)).all(), "x_hat = 0 on the constant channel"
        assert (got["gy"][:, c] == 0).all() and got["ggamma"][c] == 0
    if shape[1] >= 2:
        assert (got["z"][:, 1] == (np.float32(max(case["beta"][1], 0)) if relu else case["beta"][1])).all(), "gamma = 0"
        assert (got["gy"][:, 1] == 0).all()


def test_variance_of_a_channel_far_from_zero():
    """30 + 0.01 N(0,1) over 4096 columns: an fp32 E[x^2] - E[x]^2 is off by tens of percent here, fixed-order fp64 sums by about 1e-9.
    The saved variance and the running_var update within a relative 1e-5 of fp64.  (z is not compared: rounding the mean to fp32
    dominates it, here and in the fp32 reference.)"""
    from disprcnn_amd.layers import pn2_mlp
    rs = np.random.RandomState(11)
    y = (30.0 + 0.01 * rs.normal(0.0, 1.0, (2, 3, 2048))).astype(np.float32)
    n = 4096
    var = y.astype(np.float64).var((0, 2))
    yt = torch.from_numpy(y).to(DEV)
    rm, rv = torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    _, stats = pn2_mlp.bn_act_train(yt, torch.ones(3, device=DEV), torch.zeros(3, device=DEV), rm, rv, MOMENTUM, EPS, False, return_stats=True)
    saved = 1.0 / stats[1].cpu().numpy().astype(np.float64) ** 2 - EPS
    rel_saved = np.abs(saved - var).max() / var.min()
    want_rv = MOMENTUM * var * n / (n - 1)
    rel_rv = (np.abs(rv.cpu().numpy().astype(np.float64) - want_rv) / want_rv).max()
    naive = (y ** 2).mean((0, 2), dtype=np.float32) - y.mean((0, 2), dtype=np.float32) ** 2
    print(f"variance {var}, saved {saved} (relative error {rel_saved:.3g}), running_var relative error {rel_rv:.3g}; an fp32 E[x^2] - E[x]^2 "
          f"gives {naive}")
    assert rel_saved <= 1e-5 and rel_rv <= 1e-5
    assert np.abs(rm.cpu().numpy() - MOMENTUM * y.astype(np.float64).mean((0, 2))).max() <= 1e-6 * 3.0


@pytest.mark.parametrize("k", [3, 5, 6])
def test_two_runs_give_the_same_bits(k):
    case = make_case(shapes()[k], 400 + k)
    a, b = hip(case, True), hip(case, True)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_one_value_per_channel_is_refused():
    from disprcnn_amd.layers import pn2_mlp
    y = torch.zeros(1, 4, 1, device=DEV)
    w, b = torch.ones(4, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        pn2_mlp.bn_act_train(y, w, b, torch.zeros(4, device=DEV), torch.ones(4, device=DEV), MOMENTUM, EPS, True)
