"""Host tests of the input pipeline: the size rule, the NEAREST index tables against tables recorded from Pillow, the LUT against torch's
CPU ops, the order of the random draws, SegmentationMask / Calib semantics on hand-computed values, and the shape of the new module tree
and C ABI.  No GPU."""
import copy
import os
import random
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from . import input_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEAN, STD = [102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0]
MEAN01, STD01 = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def make_cfg(min_size=(600,), max_size=10000, flip=0.5, do_resize=True, bgr=True, div=0, mean=MEAN, std=STD):
    return SimpleNamespace(INPUT=SimpleNamespace(DO_RESIZE=do_resize, MIN_SIZE_TRAIN=min_size, MAX_SIZE_TRAIN=max_size, MIN_SIZE_TEST=min_size[0],
                                                 MAX_SIZE_TEST=max_size, FLIP_PROB_TRAIN=flip, TO_BGR255=bgr, PIXEL_MEAN=mean, PIXEL_STD=std),
                           DATALOADER=SimpleNamespace(SIZE_DIVISIBILITY=div))


# ---- get_size
@pytest.mark.parametrize("wh,size,max_size,expect", [
    ((1242, 375), 600, 10000, (600, 1987)),
    ((100, 30), 20, 50, (15, 50)),                 # the max_size branch: 100 / 30 * 20 > 50 -> size = round(50 * 30 / 100) = 15
    ((1242, 375), 375, 10000, (375, 1242)),        # equal size: early return
    ((375, 1242), 600, 10000, (1987, 600)),        # portrait
    ((30, 100), 30, None, (100, 30)),
])
def test_get_size(wh, size, max_size, expect):
    from disprcnn_amd.data.device_input import get_size
    from disprcnn_amd.data.transforms import Resize
    assert get_size(wh, size, max_size) == expect
    assert O.get_size(wh[0], wh[1], size, max_size) == expect
    assert Resize(size, max_size).get_size(wh) == expect


# ---- index tables
@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "input_nearest_tables.npz"))


def test_fixture_holds_eight_shapes_of_arrays_only(recorded):
    assert recorded["shapes"].shape == (8, 4)
    assert [1242, 375, 1987, 600] in recorded["shapes"].tolist()
    assert all(recorded[k].dtype == np.int32 for k in recorded.files)
    assert os.path.getsize(os.path.join(HERE, "golden", "input_nearest_tables.npz")) < 1 << 20


@pytest.mark.parametrize("k", range(8))
def test_tables_equal_the_recorded_pillow_tables(recorded, k):
    from disprcnn_amd.data.device_input import axis_tables, nearest_table
    iw, ih, ow, oh = (int(v) for v in recorded["shapes"][k])
    assert np.array_equal(nearest_table(ih, oh), recorded[f"y{k}"])
    assert np.array_equal(nearest_table(iw, ow), recorded[f"x{k}"])
    assert np.array_equal(O.nearest_table(ih, oh), recorded[f"y{k}"])
    assert np.array_equal(O.nearest_table(iw, ow), recorded[f"x{k}"])
    yt, xt = axis_tables((ih, iw), (oh, ow), flip=True)
    assert yt.dtype == np.int32 and xt.dtype == np.int32
    assert np.array_equal(yt, recorded[f"y{k}"]) and np.array_equal(xt, recorded[f"x{k}"][::-1])


def test_identity_table_and_bounds():
    from disprcnn_amd.data.device_input import nearest_table
    assert np.array_equal(nearest_table(7, 7), np.arange(7))
    for n_in, n_out in [(3, 1000), (1000, 3), (1, 17), (17, 1), (1242, 1987)]:
        t = nearest_table(n_in, n_out)
        assert t.shape == (n_out,) and t.min() >= 0 and t.max() <= n_in - 1 and (np.diff(t) >= 0).all()


def test_resize_transform_equals_pillow_nearest_when_it_imports(recorded):
    Image = pytest.importorskip("PIL.Image")
    from disprcnn_amd.data.transforms import Resize
    from disprcnn_amd.structures.bounding_box import BoxList
    nearest = getattr(Image, "Resampling", Image).NEAREST
    rng = np.random.RandomState(0)
    for iw, ih, ow, oh in [(37, 11, 57, 17), (100, 30, 50, 15), (123, 37, 196, 59), (1242, 375, 1987, 600)]:
        a = rng.randint(0, 256, size=(ih, iw, 3)).astype(np.uint8)
        pil = Image.fromarray(a)
        ref = np.asarray(pil.resize((ow, oh), nearest))
        tr = Resize(oh, 10000)
        assert tr.get_size((iw, ih)) == (oh, ow)
        for img in (pil, a):
            got, tgt = tr(img, BoxList(torch.zeros(0, 4), (iw, ih)))
            assert np.array_equal(got, ref) and tgt.size == (ow, oh)


# ---- LUT
@pytest.mark.parametrize("bgr,mean,std", [(True, MEAN, STD), (False, MEAN01, STD01)])
def test_lut_equals_the_torch_ops_on_every_byte(bgr, mean, std):
    from disprcnn_amd.data.device_input import make_lut
    from disprcnn_amd.data.transforms import Normalize, ToTensor
    lut, chan = make_lut(mean, std, bgr)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and chan == ((2, 1, 0) if bgr else (0, 1, 2))
    ref, rchan = O.lut(mean, std, bgr)
    assert rchan == chan and np.array_equal(lut.numpy().view(np.uint32), ref.view(np.uint32))
    # and the host transforms on an image that holds every byte in every channel, with channels that differ
    img = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256], axis=-1).astype(np.uint8).reshape(16, 16, 3)
    t = {"left": img, "right": img}
    x, _ = Normalize(mean, std, bgr)(*ToTensor()(t, dict(t)))
    want = np.stack([ref[c][img[:, :, chan[c]]] for c in range(3)])
    assert np.array_equal(x["left"].numpy().view(np.uint32), want.view(np.uint32))


def test_bytes_survive_div_255_times_255():
    u = torch.arange(256).to(torch.uint8)
    assert torch.equal(u.float().div(255) * 255, u.float())


# ---- random draws
class CountingRng:
    def __init__(self, seed):
        self.r, self.calls = random.Random(seed), []

    def choice(self, seq):
        self.calls.append("choice")
        return self.r.choice(seq)

    def random(self):
        self.calls.append("random")
        return self.r.random()


def _collator(cfg, rng):
    """A DeviceBatchCollator for its plan only: the draws need no GPU."""
    from disprcnn_amd.data.collate_batch import DeviceBatchCollator
    c = DeviceBatchCollator.__new__(DeviceBatchCollator)
    from disprcnn_amd.data.transforms.build import transform_params
    c.min_size, c.max_size, c.flip_prob = transform_params(cfg, True)
    c.do_resize, c.rng = bool(cfg.INPUT.DO_RESIZE), rng
    return c


def test_rng_call_order():
    sizes = [[(40, 12), (40, 12)], [(37, 11), (37, 11)], [(50, 20), (50, 20)]]
    rng = CountingRng(3)
    plans = _collator(make_cfg(min_size=(16, 20, 24), flip=0.0), rng).plan(sizes)
    assert rng.calls == ["choice", "choice", "random"] * 3              # the flip is drawn even at probability 0
    assert not any(p.flip for p in plans)
    rng = CountingRng(3)
    _collator(make_cfg(min_size=(16, 20, 24), do_resize=False), rng).plan(sizes)
    assert rng.calls == ["random"] * 3


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_seed_gives_the_sizes_and_flips_of_the_host_path(seed):
    from disprcnn_amd.data.transforms import build_transforms
    from disprcnn_amd.structures.bounding_box import BoxList
    cfg = make_cfg(min_size=(16, 20, 24, 28), max_size=70, flip=0.5)
    rng = np.random.RandomState(seed)
    samples = []
    for w, h in [(40, 12), (37, 11), (50, 20), (23, 31)]:
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        img[:, 0] = 0
        img[:, -1] = 255                                                   # a flip shows in the first column
        samples.append(img)
    random.seed(seed)
    tr = build_transforms(cfg, True)
    host = []
    for img in samples:
        x, t = tr({"left": img, "right": img.copy()}, {k: BoxList(torch.zeros(0, 4), (img.shape[1], img.shape[0])) for k in ("left", "right")})
        flipped = bool(x["left"][0, 0, 0] > x["left"][0, 0, -1])
        host.append(([tuple(x[k].shape[-2:]) for k in ("left", "right")], flipped))
        assert t["left"].size == (x["left"].shape[-1], x["left"].shape[-2])
    random.seed(seed)
    plans = _collator(cfg, random).plan([[(s.shape[1], s.shape[0])] * 2 for s in samples])
    assert [([tuple(s) for s in p.sizes], p.flip) for p in plans] == host
    assert len({tuple(h[0][0]) for h in host}) > 1 or len({h[1] for h in host}) > 1


# ---- SegmentationMask on the CPU
def test_segmentation_mask_cpu_semantics():
    from disprcnn_amd.structures.segmentation_mask import BinaryMaskList, SegmentationMask
    m = torch.zeros(2, 4, 6, dtype=torch.uint8)
    m[0, 1:3, 1:4] = 1
    m[1, :, 5] = 1
    s = SegmentationMask(m, (6, 4), mode="mask")
    assert len(s) == 2 and s.size == (6, 4) and s.mode == "mask" and s.masks.dtype == torch.uint8
    assert isinstance(s.instances, BinaryMaskList) and torch.equal(s.masks, m) and s.convert("mask") is s
    assert torch.equal(s.transpose(0).masks, m.flip(2)) and torch.equal(s.transpose(1).masks, m.flip(1))
    # x2 in both axes: taps of output 2k+1 / 2k+2 are (k, k+1) with weights .25 / .75, so a pixel survives only inside a run of ones
    r = s.resize((12, 8))
    assert r.size == (12, 8) and tuple(r.masks.shape) == (2, 8, 12)
    want0 = np.zeros((8, 12), np.uint8)
    want0[3:5, 3:7] = 1                                                   # rows 1..2 -> 3..4, columns 1..3 -> 3..6
    assert np.array_equal(r.masks[0].numpy(), want0)
    assert np.array_equal(r.masks.numpy(), O.mask_resize_flip(m.numpy(), 8, 12, False))
    assert torch.equal(s.resize((6, 4)).masks, m)                         # equal size: a copy
    p = s.resize((3, 2), use_max_pooling=True)
    assert torch.equal(p.masks, torch.nn.functional.adaptive_max_pool2d(m[None].float(), (2, 3))[0].to(torch.uint8))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert torch.equal(s.resize((-1, -1)).masks, m) and s.resize((-1, -1)).size == (6, 4)
    assert w
    # crop: rounded half to even, clamped, at least one pixel (mask_resize.h:crop_bounds)
    c = s.crop([0.5, 1.5, 3.5, 2.6])                                      # -> x 0..4, y 2..3
    assert c.size == (4, 1) and torch.equal(c.masks, m[:, 2:3, 0:4])
    assert s.crop([7, 7, 9, 9]).size == (1, 1)
    assert torch.equal(s[1].masks, m[1:2]) and torch.equal(s[[1, 0]].masks, m[[1, 0]]) and len(s[torch.tensor([True, False])]) == 1
    assert tuple(s.get_mask_tensor().shape) == (2, 4, 6) and tuple(s[0].get_mask_tensor().shape) == (4, 6)
    assert torch.equal(s.get_full_image_mask_tensor(), (m.sum(0) > 0).long())
    assert torch.equal(s.to("cpu").masks, m) and [tuple(x.masks.shape) for x in s] == [(1, 4, 6)] * 2
    assert len(SegmentationMask([], (6, 4))) == 0 and tuple(SegmentationMask([], (6, 4)).resize((12, 8)).masks.shape) == (0, 8, 12)
    with pytest.raises(NotImplementedError):
        SegmentationMask([[[0, 0, 1, 1, 2, 2]]], (6, 4), mode="poly")
    with pytest.raises(NotImplementedError):
        SegmentationMask([{"counts": b"", "size": [4, 6]}], (6, 4), mode="mask")
    with pytest.raises(ValueError):
        SegmentationMask(m, (4, 6))


@pytest.mark.parametrize("shape", [(3, 11, 37, 17, 57), (3, 37, 123, 59, 196), (2, 30, 100, 15, 50), (2, 5, 9, 13, 31)])
def test_cpu_mask_rule_equals_the_oracle_and_pins_the_reference(shape):
    """The exact rule may differ from the reference's truncated fp32 sum only where that sum is within 2^-20 of 1.0, on at most 1 %."""
    from disprcnn_amd.structures.segmentation_mask import SegmentationMask
    G, H, W, oh, ow = shape
    m = O.blobs(G, H, W, seed=1)
    got = SegmentationMask(torch.from_numpy(m), (W, H)).resize((ow, oh)).masks.numpy()
    assert np.array_equal(got, O.mask_resize_flip(m, oh, ow, False))
    t = O.torch_bilinear(m, oh, ow)
    diff = got != t.astype(np.uint8)
    assert (np.abs(t[diff] - 1.0) <= 2.0 ** -20).all() and diff.mean() <= 0.01
    assert 0.05 < got.mean() < 0.95


# ---- Calib
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]], dtype=np.float32)
P3 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]], dtype=np.float32)


def test_calib_resize_and_crop():
    from disprcnn_amd.structures.calib import Calib
    src = SimpleNamespace(P0=P2.copy(), P2=P2.copy(), P3=P3.copy(), tag="kept")
    c = Calib(src, (1242, 375))
    r = c.resize((1987, 600))
    assert r is not c and r.size == (1987, 600) and r.calib.tag == "kept"
    for name, m in (("P0", P2), ("P2", P2), ("P3", P3)):
        want = m.copy()
        want[0] = want[0] / 1242 * 1987                                   # float32 throughout, as the stored matrices
        want[1] = want[1] / 375 * 600
        got = np.asarray(getattr(r.calib, name))
        assert want.dtype == np.float32 and np.array_equal(got.astype(np.float32), want) and np.array_equal(got, want.astype(got.dtype))
    assert r.fu.item() == np.float32(np.float32(721.5377) / np.float32(1242) * np.float32(1987))
    assert r.stereo_fuxbaseline == float(np.float32(np.float32(44.85728) / 1242 * 1987) - np.float32(np.float32(-339.5242) / 1242 * 1987))
    assert torch.equal(r.P2[2], torch.from_numpy(P2[2]))
    assert np.array_equal(c.calib.P2, P2.astype(np.float64)) and np.array_equal(src.P2, P2)      # the original is untouched
    # a small case by hand, float64 storage, no P0
    d = Calib(SimpleNamespace(P2=[[10.0, 0, 4, 2], [0, 20, 6, 8], [0, 0, 1, 0]], P3=[[10.0, 0, 4, -2], [0, 20, 6, 8], [0, 0, 1, 0]]), (8, 4))
    e = d.resize((4, 8))
    assert e.calib.P2.tolist() == [[5, 0, 2, 1], [0, 40, 12, 16], [0, 0, 1, 0]] and e.calib.P3[0].tolist() == [5, 0, 2, -1]
    assert (e.fu.item(), e.fv.item(), e.cu.item(), e.cv.item()) == (5, 40, 2, 12) and not hasattr(e.calib, "P0")
    k = d.crop((1, 2, 7, 4))
    assert k.size == (6, 2) and k.calib.P2.tolist() == [[10, 0, 3, 2], [0, 20, 4, 8], [0, 0, 1, 0]] and k.calib.P3[0].tolist() == [10, 0, 3, -2]
    assert d.calib.P2[0, 2] == 4
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert d.resize((-1, -1)) is d
    assert w
    q = copy.deepcopy(c)
    assert q is not c and q.calib is not c.calib and np.array_equal(q.calib.P2, c.calib.P2) and q.calib.tag == "kept"


def test_boxlist_resize_carries_masks_and_calib_along():
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.calib import Calib
    from disprcnn_amd.structures.disparity import DisparityMap
    from disprcnn_amd.structures.segmentation_mask import SegmentationMask
    W, H, ow, oh = 37, 11, 57, 17
    m = O.blobs(2, H, W, seed=2)
    t = BoxList(torch.tensor([[1.0, 2.0, 20.0, 9.0], [5.0, 0.0, 30.0, 10.0]]), (W, H))
    t.add_field("labels", torch.tensor([1, 1]))
    t.add_field("masks", SegmentationMask(torch.from_numpy(m), (W, H)))
    t.add_field("calib", Calib(SimpleNamespace(P2=P2, P3=P3), (W, H)))
    t.add_map("disparity", DisparityMap(torch.rand(H, W)))
    r = t.resize((ow, oh))
    assert r.size == (ow, oh) and r.get_field("masks").size == (ow, oh) and tuple(r.get_field("masks").masks.shape) == (2, oh, ow)
    assert np.array_equal(r.get_field("masks").masks.numpy(), O.mask_resize_flip(m, oh, ow, False))
    assert r.get_field("calib").size == (ow, oh) and r.get_field("calib").fu.item() == np.float32(np.float32(721.5377) / np.float32(W) * np.float32(ow))
    assert r.get_map("disparity").size == (ow, oh) and torch.equal(r.get_field("labels"), t.get_field("labels"))
    f = r.transpose(0)
    assert torch.equal(f.get_field("masks").masks, r.get_field("masks").masks.flip(2)) and f.get_field("calib") is r.get_field("calib")
    c = t.crop((2, 1, 30, 9))
    assert c.get_field("masks").size == (28, 8) and c.get_field("calib").size == (28, 8)
    # the 3D stage's reader and the mask loss accept the new field
    from disprcnn_amd.modeling.roi_heads.mask_head_loss import _mask_tensor
    assert torch.equal(_mask_tensor(r.get_field("masks")), r.get_field("masks").masks)


# ---- collators on the host
def test_double_view_batch_collator():
    from disprcnn_amd.data.collate_batch import BatchCollator, DoubleViewBatchCollator
    a, b = torch.ones(3, 5, 7), torch.full((3, 4, 9), 2.0)
    batch = [({"left": a, "right": a + 1}, {"left": "tl0", "right": "tr0"}, 10), ({"left": b, "right": b + 1}, {"left": "tl1", "right": "tr1"}, 11)]
    images, targets, ids = DoubleViewBatchCollator(4)(batch)
    assert tuple(images["left"].tensors.shape) == (2, 3, 8, 12) and images["left"].image_sizes == [(5, 7), (4, 9)]
    assert torch.equal(images["right"].tensors[1, :, :4, :9], b + 1) and images["right"].tensors[1, :, 4:].abs().sum() == 0
    assert targets == {"left": ["tl0", "tl1"], "right": ["tr0", "tr1"]} and tuple(ids) == (10, 11)
    five = [s + ("lp%d" % i, "rp%d" % i) for i, s in enumerate(batch)]
    images, targets, extra = DoubleViewBatchCollator(0)(five)
    assert tuple(images["left"].tensors.shape) == (2, 3, 5, 9) and tuple(extra[0]) == (10, 11)
    assert extra[1] == {"left": ["lp0", "lp1"], "right": ["rp0", "rp1"]}
    images, targets, ids = BatchCollator(0)([(a, "t0", 0), (b, "t1", 1)])
    assert tuple(images.tensors.shape) == (2, 3, 5, 9) and tuple(targets) == ("t0", "t1")


def test_refusals():
    from disprcnn_amd.data.device_input import as_rgb_array, build_tables
    with pytest.raises(ValueError):
        as_rgb_array(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        as_rgb_array(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        as_rgb_array(np.zeros((4, 4, 3), np.float32))
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with pytest.raises(ValueError):
            as_rgb_array(Image.new("L", (4, 4)))
        assert as_rgb_array(Image.new("RGB", (5, 4))).shape == (4, 5, 3)
    t = build_tables([(5, 7), (3, 4)], [(5, 7), (6, 8)], [False, True], 4)
    assert (t.n_images, t.hp, t.wp, t.src_bytes) == (2, 8, 8, 5 * 7 * 3 + 3 * 4 * 3) and t.ints.dtype == np.int32
    d = t.ints[:16].reshape(2, 8)
    assert d[0].tolist() == [0, 5, 7, 5, 7, 16, 21, 0] and d[1].tolist() == [105, 3, 4, 6, 8, 28, 34, 0] and t.ints.size == 16 + 12 + 14
    assert t.ints[34:42].tolist() == [3, 3, 2, 2, 1, 1, 0, 0]


# ---- the module tree and the C ABI
def test_alias_imports():
    import disprcnn  # noqa: F401
    from disprcnn.data.collate_batch import DeviceBatchCollator, DoubleViewBatchCollator, input_batch
    from disprcnn.data.transforms import Compose, Normalize, RandomHorizontalFlip, Resize, ToTensor, build_transforms
    from disprcnn.data.transforms.build import build_transforms as bt2
    from disprcnn.structures.segmentation_mask import BinaryMaskList, SegmentationMask
    import disprcnn_amd.data.collate_batch as cb
    import disprcnn_amd.data.transforms as tr
    import disprcnn_amd.structures.segmentation_mask as sm
    assert DeviceBatchCollator is cb.DeviceBatchCollator and DoubleViewBatchCollator is cb.DoubleViewBatchCollator and input_batch is cb.input_batch
    assert (Compose, Resize, RandomHorizontalFlip, ToTensor, Normalize) == (tr.Compose, tr.Resize, tr.RandomHorizontalFlip, tr.ToTensor, tr.Normalize)
    assert build_transforms is tr.build_transforms and bt2 is tr.build_transforms
    assert SegmentationMask is sm.SegmentationMask and BinaryMaskList is sm.BinaryMaskList
    steps = build_transforms(make_cfg(), True).transforms
    assert [type(s).__name__ for s in steps] == ["Resize", "RandomHorizontalFlip", "ToTensor", "Normalize"]
    steps = build_transforms(make_cfg(do_resize=False), False).transforms
    assert [type(s).__name__ for s in steps] == ["RandomHorizontalFlip", "ToTensor", "Normalize"] and steps[0].prob == 0


def test_new_symbols_are_declared_bound_and_built():
    from disprcnn_amd.pts import _lib, build
    names = ("drc_input_batch_fwd", "drc_mask_resize_flip_fwd", "drc_input_default_max_blocks", "drc_mask_job_cols")
    with open(os.path.join(ROOT, "include", "disprcnn_pts.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(drc_\w+)\s*\(([^)]*)\)\s*;", text)}
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and n in decls
        params = [p for p in decls[n].split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_lib._SIGS[n][1]), n
    assert "input_ops.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "disprcnn_amd", "pts", "input_ops.hip")).read()
    for n in names:
        assert re.search(r'extern "C" \w+ ' + n + r"\(", src), n
    assert "float4" in src and "hipMemset" not in src
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()                                                    # every bound symbol resolves, or this raises
        assert L.drc_mask_job_cols() == 10 and L.drc_input_default_max_blocks() >= 1
