"""PSMNet's topology as data: the ONE description of the 3D regressor and of the 2D trunk behind the fp32, fp16-storage and split-f16
schedules of runtime.py (which adds storage, plans and launches -- nothing about the wiring).  Pure Python: no GPU, no built library, so
the tables are checked on a CPU against oracle/psmnet_oracle.py (tests/test_psmnet_schedule.py).

Reference: stackhourglass.py:32-51 (hourglass), :130-144 (regressor), submodule.py:25-48, 60-104 (BasicBlock, trunk), :134-135 (concat).
"""
from collections import namedtuple

from .submodule import TRUNK_STAGES

# ------------------------------------------------------------------------------------------- 3D regressor
# One conv(+BN)(+res)(+ReLU) site.  plan: key in ws["p"]; wname: key of the packed weights; prefix: state-dict prefix of the [conv, bn] pair;
# kind: "s1" / "s2" 3x3x3 conv of stride 1 / 2, "up" the stride-2 transposed conv; level: resolution of the INPUT (0 full, 1 half, 2 quarter
# volume); x, y, res: tensor names; costvol: the layer that reads the cost volume (dres0[0])
Site3d = namedtuple("Site3d", "plan wname prefix kind cin cout level x y res relu costvol")
Head = namedtuple("Head", "k site weight cls_t costk")
STRIDE = {"s1": 1, "s2": 2, "up": 2}

# (name, channels, level) in allocation order
REGRESSOR_TENSORS = (tuple((n, 32, 0) for n in ("d0a", "cost0a", "d1a", "cost0", "out1", "out2", "out3", "cls_t1", "cls_t2", "cls_t3")) +
                     tuple((f"hg{k}.{n}", 64, lvl) for k in (1, 2, 3) for n, lvl in (("c1", 1), ("pre", 1), ("post", 1), ("c3", 2), ("c4", 2))))


def _regressor_sites():
    def S(plan, wname, prefix, kind, cin, cout, level, x, y, res=None, relu=True, costvol=False):
        return Site3d(plan, wname, prefix, kind, cin, cout, level, x, y, res, relu, costvol)

    sites = [S("dres0.0", "dres0.0", "dres0.0", "s1", 64, 32, 0, "cost", "d0a", costvol=True),
             S("dres0.2", "dres0.2", "dres0.2", "s1", 32, 32, 0, "d0a", "cost0a"),
             S("dres1.0", "dres1.0", "dres1.0", "s1", 32, 32, 0, "cost0a", "d1a"),
             S("dres1.2", "dres1.2", "dres1.2", "s1", 32, 32, 0, "d1a", "cost0", res="cost0a", relu=False)]     # dres1(cost0)+cost0, no relu
    for k, hg in ((1, "dres2"), (2, "dres3"), (3, "dres4")):
        h = f"hg{k}"
        src = "cost0" if k == 1 else f"out{k - 1}"
        postsqu = None if k == 1 else f"hg{k - 1}.post"               # dres3(.., post1), dres4(.., post2)
        presqu = h + ".pre" if k == 1 else "hg1.pre"                  # pre1 reused by dres3 AND dres4 (:136,:139)
        sites += [S(h + ".conv1", hg + ".conv1", hg + ".conv1.0", "s2", 32, 64, 0, src, h + ".c1"),
                  S(h + ".conv2", hg + ".conv2", hg + ".conv2", "s1", 64, 64, 1, h + ".c1", h + ".pre", res=postsqu),      # relu(conv2 + postsqu)
                  S(h + ".conv3", hg + ".conv3", hg + ".conv3.0", "s2", 64, 64, 1, h + ".pre", h + ".c3"),
                  S(h + ".conv4", hg + ".conv4", hg + ".conv4.0", "s1", 64, 64, 2, h + ".c3", h + ".c4"),
                  S(h + ".conv5", hg + ".conv5", hg + ".conv5", "up", 64, 64, 2, h + ".c4", h + ".post", res=presqu),      # relu(conv5 + presqu|pre)
                  S(h + ".conv6", hg + ".conv6", hg + ".conv6", "up", 64, 32, 1, h + ".post", f"out{k}", res="cost0", relu=False),   # out_k = conv6 + cost0
                  S(f"classif{k}.0", f"classif{k}.0", f"classif{k}.0", "s1", 32, 32, 0, f"out{k}", f"cls_t{k}")]
    return tuple(sites)


# in plan order: classif{k}[0] follows its hourglass here; it is LAUNCHED with the heads, after the last hourglass
REGRESSOR_SITES = _regressor_sites()
# cost_k = classif{k}[2](cls_t{k}) + cost_{k-1}: the cumulative 32 -> 1 heads
REGRESSOR_HEADS = tuple(Head(k, next(s for s in REGRESSOR_SITES if s.plan == f"classif{k}.0"), f"classif{k}.2", f"cls_t{k}", f"costk{k}")
                        for k in (1, 2, 3))


# ------------------------------------------------------------------------------------------- 2D trunk
# prefix: relative to feature_extraction; pad: the conv's own padding; level: resolution of the OUTPUT (0: H, 1: H/2, 2: H/4); halo: what
# the output tensor carries (the maps of layer3 / layer4 are read by the dilated layer4)
Site2d = namedtuple("Site2d", "wname prefix cin cout k stride pad dilation relu x y res level halo")
Trunk = namedtuple("Trunk", "stem blocks raw skip")     # firstconv sites, residual-block sites, names of output_raw / output_skip


def trunk_sites():
    stem = tuple(Site2d(f"fe.firstconv.{i}", f"firstconv.{i}", cin, 32, 3, s, 1, 1, True, x, y, None, 1, 1)
                 for i, cin, s, x, y in ((0, 3, 2, "img", "f0"), (2, 32, 1, "f0", "f1"), (4, 32, 1, "f1", "f2")))
    blocks, outs = [], {}
    cur, width, level = "f2", 32, 1
    for name, planes, nblk, stride, dil in TRUNK_STAGES:
        halo = 2 if name in ("layer3", "layer4") else 1
        for b in range(nblk):
            s = stride if b == 0 else 1
            level += s - 1
            u, pre = f"fe.{name}.{b}", f"{name}.{b}"
            blocks.append(Site2d(u + ".conv1", pre + ".conv1.0", width, planes, 3, s, dil, dil, True, cur, u + ".mid", None, level, halo))
            res = cur
            if b == 0 and (s != 1 or width != planes):
                blocks.append(Site2d(u + ".down", pre + ".downsample", width, planes, 1, s, 0, 1, False, cur, u + ".sc", None, level, halo))
                res = u + ".sc"
            blocks.append(Site2d(u + ".conv2", pre + ".conv2", planes, planes, 3, 1, dil, dil, False, u + ".mid", u + ".out", res, level, halo))   # out += x, no trailing relu
            cur, width = u + ".out", planes
        outs[name] = cur
    return Trunk(stem, tuple(blocks), outs["layer2"], outs["layer4"])


# ------------------------------------------------------------------------------------------- concat (submodule.py:134-135)
# (part, first channel, channels) of the 320-channel input of lastconv
CONCAT = (("raw", 0, 64), ("skip", 64, 128), ("branch4", 192, 32), ("branch3", 224, 32), ("branch2", 256, 32), ("branch1", 288, 32))


def concat_slots(cb):
    """{part: index of its first channel block} for storage in blocks of `cb` channels (16: Blocked, 32: Blocked16)."""
    return {name: off // cb for name, off, _ in CONCAT}
