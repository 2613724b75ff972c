"""The backward kernels of the shared MLPs on the MI355X (pts/pn2_mlp_bwd.hip through layers/pn2_mlp.py): input, weight and bias
gradients of one pointwise layer, the max over a neighbourhood with its winner, and the training form of an SA scale.

Bound, per gradient tensor, the one tests/test_hip_rpn.py::check_bound applies: err <= 2 * e32 + 1e-6 * max|ref|, ref being
tests/rcnn_train_oracle.py's fp64 autograd result and e32 the error of the same oracle run in fp32 on the CPU.  The upstream gradient is
one seeded tensor per case, the same for all three runs.  Exact properties (ReLU at zero, the max and its winner, reproducibility) are
checked bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import rcnn_train_oracle as TO
from tests import rpn_oracle as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import __graft_entry__ as g
    g.build()
    yield
    release_cached_blocks()


def release_cached_blocks():
    """Hand this module's freed blocks back to the driver: autograd's graphs die with the garbage collector, and what they held would
    otherwise stay split up in the caching allocator, where the tests of other modules that count allocated bytes would be served from it."""
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def P():
    from disprcnn_amd.layers import pn2_mlp
    return pn2_mlp


def t(a, dtype=torch.float32, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)
    return x.requires_grad_() if grad else x


def check_bound(name, got, ref, e32):
    err = (got.double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
    m = ref.abs().max().item() if ref.numel() else 0.0
    print(f"{name}: max|err| {err:.3e} (fp32 chain {e32:.3e}), max|ref| {m:.3e}")
    assert err <= 2.0 * e32 + 1e-6 * m, (name, err, e32)


def cpu_leaves(arrays, dtype):
    return [None if a is None else torch.from_numpy(a).to(dtype).requires_grad_() for a in arrays]


def grads_of(leaves):
    return [None if x is None else x.grad.double() for x in leaves]


# ---- one pointwise layer
def pointwise_case(seed, B, N, C0, C1, cout, relu):
    rs = np.random.RandomState(seed)
    cin = C0 + C1
    in0 = rs.normal(0, 1, (B, C0, N)).astype(f32)
    in1 = rs.normal(0, 1, (B, C1, N)).astype(f32) if C1 else None
    w = rs.normal(0, np.sqrt(2.0 / cin), (cout, cin, 1)).astype(f32)
    b = rs.normal(0, 0.1, cout).astype(f32)
    gout = rs.normal(0, 1, (B, cout, N)).astype(f32)
    return in0, in1, w, b, gout


def pointwise_oracle(case, relu, dtype):
    in0, in1, w, b, gout = case
    leaves = cpu_leaves([in0, in1, w, b], dtype)
    y = TO.pointwise(leaves[0], leaves[1], leaves[2], leaves[3], relu)
    y.backward(torch.from_numpy(gout).to(dtype))
    return y.detach().double(), grads_of(leaves)


def pointwise_gpu(case, relu):
    in0, in1, w, b, gout = case
    leaves = [t(in0, grad=True), t(in1, grad=True) if in1 is not None else None, t(w, grad=True), t(b, grad=True)]
    y = P().pointwise_mlp_train(leaves[0], leaves[1], leaves[2], leaves[3], relu)
    y.backward(t(gout))
    return y.detach(), [None if x is None else x.grad for x in leaves]


def chunk_shapes():
    c = P().WGRAD_CHUNK
    return [(1, c - 1, 16, 0, 40, True), (1, c, 16, 0, 40, True), (1, c + 1, 16, 0, 40, True), (3, c // 2 + 1, 16, 0, 40, True)]


SHAPES = [(1, 1, 1, 0, 1, False), (2, 33, 5, 0, 128, True), (3, 70, 128, 128, 128, True), (1, 37, 512, 0, 46, False),
          (2, 257, 131, 0, 128, True)]


def run_pointwise(shape):
    B, N, C0, C1, cout, relu = shape
    case = pointwise_case(1000 + N + cout, B, N, C0, C1, cout, relu)
    y64, g64 = pointwise_oracle(case, relu, torch.float64)
    y32, g32 = pointwise_oracle(case, relu, torch.float32)
    y, g = pointwise_gpu(case, relu)
    check_bound(f"{shape} out", y, y64, (y32 - y64).abs().max().item())
    assert g[2].shape == case[2].shape and g[3].shape == case[3].shape
    for name, got, r64, r32 in zip(("in0", "in1", "W", "b"), g, g64, g32):
        if r64 is None:
            assert got is None
            continue
        assert got.shape == r64.shape
        check_bound(f"{shape} d{name}", got, r64, (r32 - r64).abs().max().item())


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_pointwise_layer_gradients(shape):
    run_pointwise(shape)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_pointwise_layer_gradients_across_a_chunk_boundary(which):
    shape = chunk_shapes()[which]
    c = P().WGRAD_CHUNK
    assert shape[0] * shape[1] > c or which < 2             # the later cases need a second partial; the last one crosses a batch boundary
    run_pointwise(shape)


def test_needs_input_grad_is_respected():
    case = pointwise_case(5, 2, 40, 8, 0, 16, True)
    x, w, b = t(case[0]), t(case[2], grad=True), t(case[3])
    y = P().pointwise_mlp_train(x, None, w, b, True)
    y.backward(t(case[4]))
    assert x.grad is None and b.grad is None and w.grad is not None and w.grad.shape == w.shape
    w4 = t(case[2][..., None], grad=True)                   # the Conv2d parameter's shape
    P().pointwise_mlp_train(x, None, w4, b, True).backward(t(case[4]))
    assert w4.grad.shape == w4.shape and torch.equal(w4.grad.reshape(-1), w.grad.reshape(-1))


def test_relu_at_exactly_zero_passes_no_gradient():
    rs = np.random.RandomState(9)
    B, N, cin, cout = 2, 70, 12, 40
    in0 = rs.normal(0, 1, (B, cin, N)).astype(f32)
    w = rs.normal(0, 0.5, (cout, cin)).astype(f32)
    b = rs.normal(0, 0.1, cout).astype(f32)
    zero_rows = [0, 17, 39]
    w[zero_rows], b[zero_rows] = 0, 0                       # pre-activation exactly 0 at every column of these rows
    gout = rs.normal(0, 1, (B, cout, N)).astype(f32)
    x, wt, bt = t(in0, grad=True), t(w, grad=True), t(b, grad=True)
    y = P().pointwise_mlp_train(x, None, wt, bt, True)
    assert (y[:, zero_rows] == 0).all()
    y.backward(t(gout))
    assert (wt.grad[zero_rows] == 0).all() and (bt.grad[zero_rows] == 0).all()
    # a layer made of such rows only passes an exact zero into its input, and the whole layer's input gradient is that of its other rows
    x2, w2, b2 = t(in0, grad=True), t(w[zero_rows], grad=True), t(b[zero_rows], grad=True)
    P().pointwise_mlp_train(x2, None, w2, b2, True).backward(t(gout[:, zero_rows]))
    assert (x2.grad == 0).all() and (w2.grad == 0).all() and (b2.grad == 0).all()
    gz = gout.astype(np.float64) * (y.detach().cpu().numpy() > 0)
    ref = np.einsum("oc,bon->bcn", w.astype(np.float64), gz)
    assert np.abs(x.grad.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- the max over the neighbourhood
@pytest.mark.parametrize("ns", [1, 16, 33, 64])
def test_group_max_forward_and_backward(ns):
    rs = np.random.RandomState(ns)
    B, C, M = 2, 5, 37
    x = rs.normal(0, 1, (B, C, M, ns)).astype(f32)
    x[0, 0, 0] = 0.25                                        # a row of equal values
    x[1, 2, 3] = -1.5
    if ns > 1:
        x[:, :, 5, ns // 2:] = x[:, :, 5, :ns - ns // 2]     # duplicated columns, as a padded neighbourhood has
        x[0, 1, 6, ns - 1] = x[0, 1, 6].max()                # a tie that includes the last sample
    xt = t(x, grad=True)
    out, arg = P().group_max(xt, return_arg=True)
    want = torch.from_numpy(x).max(3)[0]
    assert torch.equal(out.detach().cpu(), want)
    a = arg.cpu().numpy()
    assert a[0, 0, 0] == 0 and a[1, 2, 3] == 0
    first = (x == x.max(3, keepdims=True)).argmax(3)         # the lowest index among equal maxima
    assert np.array_equal(a, first)
    gout = rs.normal(0, 1, (B, C, M)).astype(f32)
    gout[gout == 0] = 1.0
    out.backward(t(gout))
    g = xt.grad.cpu().numpy()
    assert g.shape == x.shape
    nz = g != 0
    assert (nz.sum(3) == 1).all()                            # exactly one sample per (b, c, m) ...
    assert np.array_equal(g.sum(3), gout)                    # ... carries gout, the rest is exact zero
    assert (x[nz] == np.broadcast_to(x.max(3, keepdims=True), x.shape)[nz]).all()       # ... and its value is the maximum
    assert (g[0, 0, 0, 1:] == 0).all() and g[0, 0, 0, 0] == gout[0, 0, 0]


# ---- the SA chain
def sa_inputs(rs, B, N, M, C, ns, radius, group_all=False):
    from disprcnn_amd.layers import pointnet2 as L
    xyz = np.stack([RO.make_cloud("surface", int(rs.randint(1 << 30)), N) for _ in range(B)])
    if group_all:
        new_xyz = np.zeros((B, 1, 3), f32)
        idx = np.broadcast_to(np.arange(N, dtype=np.int32), (B, 1, N)).copy()
    else:
        new_xyz = np.stack([xyz[b][rs.permutation(N)[:M]] for b in range(B)])
        idx = L.ball_query(radius, ns, t(xyz), t(new_xyz)).cpu().numpy()
    feats = rs.normal(0, 1, (B, C, N)).astype(f32) if C else None
    return xyz, new_xyz, feats, idx


def rand_layers(rs, cin, widths):
    out = []
    for w in widths:
        out.append((rs.normal(0, np.sqrt(2.0 / cin), (w, cin, 1, 1)).astype(f32), rs.normal(0, 0.1, w).astype(f32)))
        cin = w
    return out


def sa_oracle(xyz, new_xyz, feats, idx, layers, gout, dtype):
    f = cpu_leaves([feats], dtype)[0]
    ls = [tuple(cpu_leaves([w, b], dtype)) for w, b in layers]
    y = TO.sa_chain(xyz, new_xyz, f, idx, ls, dtype)
    y.backward(torch.from_numpy(gout).to(dtype))
    return y.detach().double(), grads_of([f] + [p for l in ls for p in l])


def sa_gpu(xyz, new_xyz, feats, idx, layers, gout):
    f = t(feats, grad=True) if feats is not None else None
    ls = [(t(w, grad=True), t(b, grad=True)) for w, b in layers]
    y = P().sa_mlp_max_train(t(xyz), t(new_xyz), f, t(idx, torch.int32), ls)
    y.backward(t(gout))
    return y.detach(), [None if f is None else f.grad] + [p.grad for l in ls for p in l]


SA_CASES = {"nofeat_ns1": (2, 40, 5, 0, 1, [16, 32], False), "nofeat_ns16": (2, 40, 5, 0, 16, [16, 32], False),
            "nofeat_ns64": (2, 40, 5, 0, 64, [16, 32], False), "feat128": (2, 40, 5, 128, 16, [128, 128, 128], False),
            "group_all": (3, 32, 1, 256, 32, [256, 256, 512], True)}


@pytest.mark.parametrize("name", list(SA_CASES))
def test_sa_chain_gradients(name):
    B, N, M, C, ns, widths, group_all = SA_CASES[name]
    rs = np.random.RandomState(len(name) + ns)
    xyz, new_xyz, feats, idx = sa_inputs(rs, B, N, M, C, ns, 0.25, group_all)
    if not group_all and ns > 1:
        padded = [(idx[b, m] == idx[b, m, 0]).sum() > 1 for b in range(B) for m in range(M)]
        assert any(padded), "no neighbourhood is padded with repeats: the radius is too large for this case"
    layers = rand_layers(rs, C + 3, widths)
    gout = rs.normal(0, 1, (B, widths[-1], M)).astype(f32)
    y64, g64 = sa_oracle(xyz, new_xyz, feats, idx, layers, gout, torch.float64)
    y32, g32 = sa_oracle(xyz, new_xyz, feats, idx, layers, gout, torch.float32)
    y, g = sa_gpu(xyz, new_xyz, feats, idx, layers, gout)
    e_fwd = (y32 - y64).abs().max().item()
    check_bound(f"{name} out", y, y64, e_fwd)
    ev = P().sa_mlp_max(t(xyz), t(new_xyz), t(feats) if feats is not None else None, t(idx, torch.int32),
                        [(t(w.reshape(w.shape[0], -1)), t(b)) for w, b in layers])
    bound = 2 * e_fwd + 1e-6 * y64.abs().max().item()
    print(f"{name}: training forward vs eval sa_mlp_max {(y - ev).abs().max().item():.3e} (2 x bound {2 * bound:.3e})")
    assert (y - ev).abs().max().item() <= 2 * bound
    names = ["feats"] + [f"{k}{i}" for i in range(len(layers)) for k in ("W", "b")]
    for nm, got, r64, r32 in zip(names, g, g64, g32):
        if r64 is None:
            assert got is None
            continue
        assert got.shape == r64.shape
        check_bound(f"{name} d{nm}", got, r64, (r32 - r64).abs().max().item())


def test_backward_is_bit_reproducible():
    case = pointwise_case(1000 + 257 + 128, 2, 257, 131, 0, 128, True)
    _, a = pointwise_gpu(case, True)
    _, b = pointwise_gpu(case, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)
    B, N, M, C, ns, widths, _ = SA_CASES["feat128"]
    rs = np.random.RandomState(77)
    xyz, new_xyz, feats, idx = sa_inputs(rs, B, N, M, C, ns, 0.25)
    layers = rand_layers(rs, C + 3, widths)
    gout = rs.normal(0, 1, (B, widths[-1], M)).astype(f32)
    _, a = sa_gpu(xyz, new_xyz, feats, idx, layers, gout)
    _, b = sa_gpu(xyz, new_xyz, feats, idx, layers, gout)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_empty_problems_give_zero_gradients():
    for B, N in ((0, 5), (2, 0)):
        x = torch.zeros(B, 4, N, device=DEV, requires_grad=True)
        w, b = torch.randn(6, 4, 1, device=DEV, requires_grad=True), torch.randn(6, device=DEV, requires_grad=True)
        y = P().pointwise_mlp_train(x, None, w, b, True)
        assert y.shape == (B, 6, N)
        y.sum().backward()
        assert x.grad.shape == x.shape and w.grad.shape == w.shape and (w.grad == 0).all() and (b.grad == 0).all()
    xyz, feats = torch.randn(2, 10, 3, device=DEV), torch.randn(2, 4, 10, device=DEV, requires_grad=True)
    w, b = torch.randn(6, 7, 1, 1, device=DEV, requires_grad=True), torch.randn(6, device=DEV, requires_grad=True)
    y = P().sa_mlp_max_train(xyz, torch.zeros(2, 0, 3, device=DEV), feats, torch.zeros(2, 0, 8, dtype=torch.int32, device=DEV), [(w, b)])
    assert y.shape == (2, 6, 0)
    y.sum().backward()
    assert (feats.grad == 0).all() and feats.grad.shape == feats.shape and (w.grad == 0).all() and (b.grad == 0).all()
    g = P().group_max(torch.zeros(2, 3, 0, 4, device=DEV, requires_grad=True))
    assert g.shape == (2, 3, 0)


def test_training_forms_refuse_cpu_tensors():
    with pytest.raises(RuntimeError):
        P().pointwise_mlp_train(torch.zeros(1, 4, 8), None, torch.zeros(6, 4, device=DEV), torch.zeros(6, device=DEV), True)
    with pytest.raises(RuntimeError):
        P().group_max(torch.zeros(1, 2, 3, 4))
