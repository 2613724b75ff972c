"""The layer tables of disprcnn_amd/modeling/psmnet/schedule.py against the CPU oracle (no GPU, no built library).

Each table is EXECUTED with the oracle's own per-layer helpers and must reproduce the oracle's hand-written network bit for bit: the same
torch ops run on the same operands, so a difference is a wiring error (a wrong input, residual, stride or ReLU), never rounding.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from disprcnn_amd.modeling.psmnet import schedule as S
from disprcnn_amd.modeling.psmnet.runtime import PSMNetRuntime
from disprcnn_amd.modeling.psmnet.stackhourglass import PSMNet
from disprcnn_amd.modeling.psmnet.submodule import SPP_BRANCHES
from oracle import psmnet_oracle as O
from tests.helpers import state_for


@pytest.fixture(scope="module")
def sd():
    return state_for("A")


def _ramp(*shape):
    """Values that differ per element (no two voxels or channels alike), of unit scale."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float32)
    return (torch.sin(0.37 * i) + 0.001 * (i % 97)).reshape(shape)


def _run_regressor(sd, cost, training):
    """REGRESSOR_SITES + REGRESSOR_HEADS evaluated with the oracle's convbn3d / deconvbn3d; -> {tensor name: value}."""
    T = {"cost": cost}
    full = tuple(cost.shape[2:])
    dims = (full, tuple(s // 2 for s in full), tuple(s // 4 for s in full))
    for s in S.REGRESSOR_SITES:
        x = T[s.x]
        assert tuple(x.shape[1:]) == (s.cin,) + dims[s.level], s.plan
        y = O.deconvbn3d(sd, s.prefix, x, training) if s.kind == "up" else O.convbn3d(sd, s.prefix, x, S.STRIDE[s.kind], training)
        assert y.shape[1] == s.cout, s.plan
        if s.res:
            y = y + T[s.res]
        T[s.y] = F.relu(y) if s.relu else y
    prev = None
    for h in S.REGRESSOR_HEADS:
        assert h.site.y == h.cls_t and h.site.plan == f"classif{h.k}.0"
        c = F.conv3d(T[h.cls_t], sd[h.weight + ".weight"].to(cost.dtype), None, 1, 1)
        T[h.costk] = prev = c if prev is None else c + prev
    return T


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_regressor_tables_reproduce_the_oracle_exactly(sd, training):
    cost = _ramp(1, 64, 4, 8, 8)                 # the smallest volume whose quarter level is non-empty
    ref = O.regressor3d(sd, cost, training=training, want_intermediates=True)
    T = _run_regressor(sd, cost, training)
    names = dict(cost0="cost0", out1="out1", out2="out2", out3="out3", pre1="hg1.pre", post1="hg1.post", post2="hg2.post",
                 cost1="costk1", cost2="costk2", cost3="costk3")
    assert set(names) == set(ref)
    for k, name in names.items():
        assert torch.equal(T[name], ref[k]), f"{k} ({name}) differs from the oracle"


def test_regressor_tables_are_complete_and_named_as_the_workspaces_are():
    assert len(S.REGRESSOR_SITES) == 25 and len({s.plan for s in S.REGRESSOR_SITES}) == 25 and len({s.wname for s in S.REGRESSOR_SITES}) == 25
    assert [s.plan for s in S.REGRESSOR_SITES if s.costvol] == ["dres0.0"]
    tensors = {n: (c, lvl) for n, c, lvl in S.REGRESSOR_TENSORS}
    assert len(tensors) == len(S.REGRESSOR_TENSORS) == 25
    out_level = {"s1": 0, "s2": 1, "up": -1}
    for s in S.REGRESSOR_SITES:
        assert tensors[s.y] == (s.cout, s.level + out_level[s.kind]), s.plan
        assert s.costvol or tensors[s.x] == (s.cin, s.level), s.plan
        assert s.res is None or tensors[s.res] == tensors[s.y], s.plan
    for name in ("d0a", "cost0a", "hg2.pre", "out3", "cls_t1", "hg3.c4"):
        assert name in tensors
    assert [h[2:] for h in S.REGRESSOR_HEADS] == [(f"classif{k}.2", f"cls_t{k}", f"costk{k}") for k in (1, 2, 3)]


def _run_trunk(sd, img, training):
    trunk = S.trunk_sites()
    T = {"img": img}
    for s in trunk.stem + trunk.blocks:
        x = T[s.x]
        assert x.shape[1] == s.cin and tuple(x.shape[2:]) == tuple(d * s.stride // (1 << s.level) for d in img.shape[2:]), s.wname
        y = O._convbn2d(sd, "feature_extraction." + s.prefix, x, s.stride, s.pad, s.dilation, training)
        if s.res:
            y = y + T[s.res]
        T[s.y] = F.relu(y) if s.relu else y
    return T[trunk.raw], T[trunk.skip]


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_trunk_table_reproduces_the_oracle_blocks_exactly(sd, training):
    img = _ramp(1, 3, 32, 48)                    # the trunk has no size floor (only the SPP pools do)
    P = "feature_extraction"
    o = img
    for i, stride in ((0, 2), (2, 1), (4, 1)):
        o = F.relu(O._convbn2d(sd, f"{P}.firstconv.{i}", o, stride, 1, 1, training))
    for name, nblk, stride, dil in (("layer1", 3, 1, 1), ("layer2", 16, 2, 1), ("layer3", 3, 1, 1), ("layer4", 3, 1, 2)):
        for b in range(nblk):
            o = O._basic_block(sd, f"{P}.{name}.{b}", o, stride if b == 0 else 1, 1, dil, training)
        if name == "layer2":
            raw = o
    got_raw, got_skip = _run_trunk(sd, img, training)
    assert tuple(got_raw.shape) == (1, 64, 8, 12) and tuple(got_skip.shape) == (1, 128, 8, 12)
    assert torch.equal(got_raw, raw), "output_raw differs from the oracle"
    assert torch.equal(got_skip, o), "output_skip differs from the oracle"


def test_concat_slots():
    assert [name for name, _, _ in S.CONCAT] == ["raw", "skip", "branch4", "branch3", "branch2", "branch1"]
    assert sum(ch for _, _, ch in S.CONCAT) == 320
    off = 0
    for _, first, ch in S.CONCAT:                # the parts tile the 320 channels in order
        assert first == off
        off += ch
    assert list(S.concat_slots(16).values()) == [0, 4, 12, 14, 16, 18]
    assert list(S.concat_slots(32).values()) == [0, 2, 6, 7, 8, 9]
    assert S.concat_slots(16)["branch1"] == 18 and S.concat_slots(32)["skip"] == 2


def test_s16_layers_are_the_distinct_layer_shapes():
    full, half, quart = (12, 28, 28), (6, 14, 14), (3, 7, 7)
    assert PSMNetRuntime._s16_layers(12, 28, 28) == [
        ("s1", 64, 32, full), ("s1", 32, 32, full), ("s2", 32, 64, full), ("s1", 64, 64, half), ("s2", 64, 64, half),
        ("s1", 64, 64, quart), ("up", 64, 64, quart), ("up", 64, 32, half)]


def test_every_site_resolves_to_its_module_and_compile_builds_exactly_these_weights():
    model = PSMNet(48)
    trunk = S.trunk_sites()
    for s in S.REGRESSOR_SITES:
        conv, bn = model.get_submodule(s.prefix)
        up = isinstance(conv, nn.ConvTranspose3d)
        assert up == (s.kind == "up") and isinstance(conv, nn.ConvTranspose3d if up else nn.Conv3d) and isinstance(bn, nn.BatchNorm3d), s.plan
        assert (conv.in_channels, conv.out_channels) == (s.cin, s.cout), s.plan
        assert conv.stride == (S.STRIDE[s.kind],) * 3 and conv.dilation == (1, 1, 1) and conv.kernel_size == (3, 3, 3), s.plan
    for h in S.REGRESSOR_HEADS:
        conv = model.get_submodule(h.weight)
        assert isinstance(conv, nn.Conv3d) and (conv.in_channels, conv.out_channels) == (32, 1)
    for s in trunk.stem + trunk.blocks:
        conv, bn = model.feature_extraction.get_submodule(s.prefix)
        assert isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d), s.wname
        assert (conv.in_channels, conv.out_channels, conv.kernel_size) == (s.cin, s.cout, (s.k, s.k)), s.wname
        assert (conv.stride, conv.padding, conv.dilation) == ((s.stride,) * 2, (s.pad,) * 2, (s.dilation,) * 2), s.wname
    names = ({s.wname for s in S.REGRESSOR_SITES} | {h.weight for h in S.REGRESSOR_HEADS} | {s.wname for s in trunk.stem + trunk.blocks} |
             {f"fe.{name}" for name, _ in SPP_BRANCHES} | {"fe.lastconv.0", "fe.lastconv.2"})
    W = PSMNetRuntime(model, torch.device("cpu"))._compile()
    assert set(W) == names and len(W) == 89
    for s in S.REGRESSOR_SITES:
        assert W[s.wname].conv is model.get_submodule(s.prefix)[0] and W[s.wname].transposed == (s.kind == "up"), s.plan
    for s in trunk.stem + trunk.blocks:
        assert W[s.wname].conv is model.feature_extraction.get_submodule(s.prefix)[0], s.wname
