"""GPU tests of the input pipeline (pts/input_ops.hip behind disprcnn_amd/data): drc_input_batch_fwd bit for bit against the NumPy oracle
at the edges of its quads (odd widths, tails, quads that straddle rows / planes / images, unaligned outputs, the strided grid), with the
output pre-filled with NaN so that an unwritten element or a non-zero pad shows; drc_mask_resize_flip_fwd against the oracle's exact
rule and pinned to the reference's F.interpolate; and DeviceBatchCollator against the host path (build_transforms per sample,
DoubleViewBatchCollator, .to(device)).

The file's name sorts behind every other test file on purpose.  The suite runs its GPU tests in one process and in collection order, and
tests/test_hip_rcnn.py::test_pooling_and_group_all_allocate_only_their_outputs compares torch's peak allocation with the size of the
outputs, which holds only while the caching allocator's best cached block for the 8 MiB output is not one it hands out whole (up to 1 MiB larger).  Tests that come
before it move the garbage collector's schedule and with it the blocks that are cached when it runs; collected last, these tests leave
every older test behind the same history as before, and they hand their own blocks back when they are done."""
import gc
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import input_oracle as O
from .test_input_host import MEAN, MEAN01, P2, P3, STD, STD01, make_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from disprcnn_amd.pts import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _hand_blocks_back():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _images(sizes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


def _run(dev, images, out_hws, flips, div=0, bgr=True, mean=MEAN, std=STD, max_blocks=None, shift=0):
    """The kernel on NaN-filled memory; `shift` moves the output off its 16-byte boundary by that many floats."""
    from disprcnn_amd.data import device_input as D
    tables = D.build_tables([im.shape[:2] for im in images], out_hws, flips, div)
    lut, chan = D.make_lut(mean, std, bgr)
    n = len(images) * 3 * tables.hp * tables.wp
    store = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=dev)
    out = store[shift: shift + n].view(len(images), 3, tables.hp, tables.wp)
    got = D.input_batch(images, tables, lut, chan, out=out, max_blocks=max_blocks)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    rest = torch.cat((store[:shift], store[shift + n:]))
    assert bool(torch.isnan(rest).all()), "the kernel wrote outside its output"
    return got.cpu().numpy(), tables


def _check_images(dev, images, out_hws, flips, div=0, bgr=True, mean=MEAN, std=STD, **kw):
    got, tables = _run(dev, images, out_hws, flips, div, bgr, mean, std, **kw)
    ref = O.image_batch(images, out_hws, flips, mean, std, bgr, div)
    assert got.shape == ref.shape and tables.image_sizes == [tuple(s) for s in out_hws]
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} elements were never written"
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))          # bit for bit: the pad is +0.0, not -0.0
    return got


def test_unresized_5x7_tail_of_two(dev):
    ims = _images([(5, 7), (5, 7)], 0)
    got = _check_images(dev, ims, [(5, 7), (5, 7)], [False, False])
    assert got.size == 210 and got.size % 4 == 2


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("src,dst", [((11, 37), (17, 57)), ((30, 100), (15, 50)), ((11, 37), (11, 37))])
def test_single_image_resize_and_flip(dev, src, dst, flip):
    _check_images(dev, _images([src], 1), [dst], [flip])


@pytest.mark.parametrize("div", [0, 1, 32])
def test_three_pairs_of_different_sizes(dev, div):
    """One image is smaller than the others in both dimensions: padding to the right, below, and both."""
    sizes, outs = [(11, 37), (9, 21), (13, 30)], [(17, 57), (9, 21), (19, 43)]
    for view, seed in (("left", 2), ("right", 3)):
        got = _check_images(dev, _images(sizes, seed), outs, [False, True, True], div=div)
        assert got.shape[2:] == ((32, 64) if div == 32 else (19, 57))


@pytest.mark.parametrize("bgr,mean,std", [(True, MEAN, STD), (False, MEAN01, STD01)])
def test_ramp_of_every_byte_in_every_channel(dev, bgr, mean, std):
    r = np.arange(256)
    img = np.stack([r, r[::-1], (r * 7) % 256], axis=-1).astype(np.uint8).reshape(16, 16, 3)
    got = _check_images(dev, [img], [(16, 16)], [False], bgr=bgr, mean=mean, std=std)
    assert len(np.unique(got[0, 0])) == 256
    _check_images(dev, [img], [(23, 19)], [True], bgr=bgr, mean=mean, std=std)


@pytest.mark.parametrize("cap", [1, 2])
def test_lowered_grid_cap_strides(dev, cap):
    ims = _images([(11, 37), (9, 21)], 4)                                     # 2 * 3 * 17 * 57 = 5814 elements = 1454 quads > 256 * cap
    _check_images(dev, ims, [(17, 57), (9, 21)], [True, False], max_blocks=cap)
    from disprcnn_amd.data import device_input as D
    old = D.GRID_CAP
    D.GRID_CAP = cap                                                          # the module constant reaches the launch too
    try:
        _check_images(dev, ims, [(17, 57), (9, 21)], [True, False])
    finally:
        D.GRID_CAP = old


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_output_off_the_16_byte_boundary(dev, shift):
    _check_images(dev, _images([(5, 7), (5, 7)], 5), [(5, 7), (5, 7)], [False, True], shift=shift)
    _check_images(dev, _images([(11, 37)], 6), [(17, 57)], [False], shift=shift)


def test_empty_batch_launches_nothing_and_bad_arguments_raise(dev):
    from disprcnn_amd.data import device_input as D
    lut, chan = D.make_lut(MEAN, STD, True)
    out = D.input_batch([], D.build_tables([], [], []), lut, chan, device=dev)
    assert tuple(out.shape) == (0, 3, 0, 0)
    ims = _images([(5, 7)], 7)
    t = D.build_tables([(5, 7)], [(5, 7)], [False])
    with pytest.raises(ValueError):
        D.input_batch(ims, t, lut, chan, out=torch.empty(1, 3, 5, 8, device=dev))
    with pytest.raises(RuntimeError):
        D.input_batch(ims, t, lut, (0, 1, 3), device=dev)
    with pytest.raises(ValueError):
        D.input_batch(_images([(5, 8)], 7), t, lut, chan, device=dev)


# ---- masks
MASK_CASES = [("11x37", 3, (11, 37), (17, 57), False), ("37x123", 3, (37, 123), (59, 196), False), ("down", 2, (30, 100), (15, 50), False),
              ("equal", 3, (11, 37), (11, 37), False), ("equal_flip", 3, (11, 37), (11, 37), True), ("11x37_flip", 3, (11, 37), (17, 57), True)]


@pytest.fixture(scope="module")
def mask_refs():
    """Inputs and oracle outputs of every mask case, computed once."""
    out = {}
    for name, G, (H, W), (oh, ow), flip in MASK_CASES:
        m = O.blobs(G, H, W, seed=11)
        out[name] = (m, O.mask_resize_flip(m, oh, ow, flip), O.torch_bilinear(m, oh, ow))
    return out


@pytest.mark.parametrize("name,G,src,dst,flip", MASK_CASES)
def test_masks_equal_the_exact_rule_and_pin_the_reference(dev, mask_refs, name, G, src, dst, flip):
    from disprcnn_amd.structures.segmentation_mask import SegmentationMask
    m, ref, t = mask_refs[name]
    s = SegmentationMask(torch.from_numpy(m).to(dev), (src[1], src[0]))
    r = s.resize((dst[1], dst[0]))
    if flip:
        r = r.transpose(0)
    assert r.masks.is_cuda and r.masks.dtype == torch.uint8 and r.size == (dst[1], dst[0])
    got = r.masks.cpu().numpy()
    assert np.array_equal(got, ref)
    if flip:
        t = t[:, :, ::-1]
    diff = got != t.astype(np.uint8)                                          # the reference truncates torch's fp32 sum
    assert (np.abs(t[diff] - 1.0) <= 2.0 ** -20).all(), "differs from the reference where its blend is not a rounded 1.0"
    assert diff.mean() <= 0.01
    if src == dst:
        assert np.array_equal(got, m[:, :, ::-1] if flip else m)


@pytest.mark.parametrize("cap", [None, 1])
def test_ragged_mask_jobs_in_one_launch(dev, mask_refs, cap):
    """Every case as one job of a single launch, flips fused, plus an empty list and an unaligned destination size (G * oh * ow odd)."""
    from disprcnn_amd.structures.segmentation_mask import resize_flip_batch
    odd = O.blobs(1, 5, 9, seed=12)
    srcs = [torch.from_numpy(mask_refs[n][0]).to(dev) for n, *_ in MASK_CASES] + [torch.zeros(0, 11, 37, dtype=torch.uint8, device=dev),
                                                                                 torch.from_numpy(odd).to(dev)]
    sizes = [(d[1], d[0]) for _, _, _, d, _ in MASK_CASES] + [(57, 17), (31, 13)]
    flips = [f for *_, f in MASK_CASES] + [True, True]
    outs = resize_flip_batch(srcs, sizes, flips, max_blocks=cap)
    for (n, *_), o in zip(MASK_CASES, outs):
        assert np.array_equal(o.cpu().numpy(), mask_refs[n][1]), n
    assert tuple(outs[-2].shape) == (0, 17, 57)
    assert np.array_equal(outs[-1].cpu().numpy(), O.mask_resize_flip(odd, 13, 31, True))


def test_no_masks_is_a_no_op(dev):
    from disprcnn_amd.structures.segmentation_mask import SegmentationMask, mask_jobs
    s = SegmentationMask(torch.zeros(0, 11, 37, dtype=torch.uint8, device=dev), (37, 11))
    r = s.resize((57, 17)).transpose(0)
    assert tuple(r.masks.shape) == (0, 17, 57) and r.masks.is_cuda
    rows, quads = mask_jobs([(s.masks, r.masks)], [False])
    assert rows.shape == (0, 10) and quads == 0


# ---- the collator against the host path
def _sample(rng, w, h, g, as_tensor=False):
    imgs, targets = {}, {}
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.calib import Calib
    from disprcnn_amd.structures.disparity import DisparityMap
    from disprcnn_amd.structures.segmentation_mask import SegmentationMask
    for k in ("left", "right"):
        a = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        imgs[k] = torch.from_numpy(a) if as_tensor else a
        x1, y1 = rng.uniform(0, w / 2, g), rng.uniform(0, h / 2, g)
        box = np.stack([x1, y1, x1 + rng.uniform(2, w / 2 - 1, g), y1 + rng.uniform(2, h / 2 - 1, g)], axis=1).astype(np.float32)
        t = BoxList(torch.from_numpy(box), (w, h))
        t.add_field("labels", torch.ones(g, dtype=torch.int64))
        t.add_field("masks", SegmentationMask(torch.from_numpy(O.blobs(g, h, w, seed=int(rng.randint(1 << 30)))), (w, h)))
        t.add_field("calib", Calib(SimpleNamespace(P2=P2, P3=P3), (w, h)))
        t.add_map("disparity", DisparityMap(torch.from_numpy(rng.uniform(0, 40, size=(h, w)).astype(np.float32))))
        targets[k] = t
    return imgs, targets


COLLATE_CASES = [("train_seed0", dict(min_size=(17, 20, 23), max_size=70, flip=0.5), 0), ("train_seed1", dict(min_size=(17, 20, 23), max_size=70, flip=0.5), 1),
                 ("flip_div32_rgb", dict(min_size=(20,), flip=1.0, div=32, bgr=False, mean=MEAN01, std=STD01), 2),
                 ("no_resize_flip", dict(flip=1.0, do_resize=False), 3), ("max_size", dict(min_size=(30,), max_size=50, flip=0.0, div=1), 4)]


@pytest.mark.parametrize("name,kw,seed", COLLATE_CASES)
def test_collator_equals_the_host_path(dev, name, kw, seed):
    from disprcnn_amd.data.collate_batch import DeviceBatchCollator, DoubleViewBatchCollator
    from disprcnn_amd.data.transforms import build_transforms
    cfg = make_cfg(**kw)
    rng = np.random.RandomState(seed)
    raw = [_sample(rng, 37, 11, 3) + (100,), _sample(rng, 30, 13, 2, as_tensor=True) + (101,)]

    random.seed(seed)
    tr = build_transforms(cfg, True)
    host = DoubleViewBatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)([tr(im, tg) + (i,) for im, tg, i in raw])
    random.seed(seed)
    collate = DeviceBatchCollator(cfg, True, dev)
    images, targets, ids = collate(raw)
    torch.cuda.synchronize()
    assert tuple(ids) == (100, 101)
    n_flipped = 0
    for k in ("left", "right"):
        want = host[0][k].tensors
        assert images[k].tensors.is_cuda and images[k].image_sizes == host[0][k].image_sizes
        assert tuple(images[k].tensors.shape) == tuple(want.shape)
        assert np.array_equal(images[k].tensors.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32))
        for i, (t, h) in enumerate(zip(targets[k], host[1][k])):
            src = raw[i][1][k]
            assert t.size == h.size and t.mode == h.mode and t.fields() == h.fields() and t.bbox.is_cuda
            assert np.array_equal(t.bbox.cpu().numpy().view(np.uint32), h.bbox.numpy().view(np.uint32))
            assert torch.equal(t.get_field("labels").cpu(), h.get_field("labels"))
            gm, hm = t.get_field("masks"), h.get_field("masks")
            assert gm.masks.is_cuda and gm.size == hm.size == t.size and torch.equal(gm.masks.cpu(), hm.masks)
            assert 0.02 < gm.masks.float().mean().item() < 0.98
            want_disp = src.get_map("disparity").to(dev).resize(t.size) if cfg.INPUT.DO_RESIZE else src.get_map("disparity").to(dev)
            gd = t.get_map("disparity").data
            assert gd.is_cuda and np.array_equal(gd.cpu().numpy().view(np.uint32), want_disp.data.cpu().numpy().view(np.uint32))
            gc, hc = t.get_field("calib"), h.get_field("calib")
            assert gc.size == hc.size == t.size and np.array_equal(gc.calib.P2, hc.calib.P2) and np.array_equal(gc.calib.P3, hc.calib.P3)
            if cfg.INPUT.DO_RESIZE and t.size != src.size:
                assert gc.calib.P2[0, 0] != src.get_field("calib").calib.P2[0, 0]
            n_flipped += int(not torch.equal(h.bbox, src.resize(h.size).bbox if cfg.INPUT.DO_RESIZE else src.bbox))
    if kw.get("flip") == 1.0:
        assert n_flipped == 4
    if kw.get("flip") == 0.0:
        assert n_flipped == 0

    random.seed(seed)
    again, targets2, _ = collate(raw)                                          # the staging buffers are reused: same bits
    torch.cuda.synchronize()
    for k in ("left", "right"):
        assert torch.equal(again[k].tensors, images[k].tensors) and again[k].image_sizes == images[k].image_sizes
        for a, b in zip(targets2[k], targets[k]):
            assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("masks").masks, b.get_field("masks").masks)
            assert torch.equal(a.get_map("disparity").data, b.get_map("disparity").data)


def test_collator_five_tuple_and_refusals(dev):
    from disprcnn_amd.data.collate_batch import DeviceBatchCollator
    cfg = make_cfg(min_size=(17,), flip=0.0)
    rng = np.random.RandomState(9)
    collate = DeviceBatchCollator(cfg, False, dev, rng=random.Random(0))
    s = _sample(rng, 37, 11, 1)
    images, targets, extra = collate([s + (7, "lp", "rp")])
    assert tuple(extra[0]) == (7,) and extra[1] == {"left": ["lp"], "right": ["rp"]} and tuple(images["left"].tensors.shape) == (1, 3, 17, 57)
    with pytest.raises(ValueError):
        collate([({"left": np.zeros((11, 37), np.uint8), "right": s[0]["right"]}, s[1], 0)])
    with pytest.raises(NotImplementedError):
        collate([(s[0]["left"], s[1]["left"], 0)])
