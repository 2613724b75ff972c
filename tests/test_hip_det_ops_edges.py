"""GPU parity of the 2D stage's two elementwise box kernels (csrc/det_ops.hip) past their grid cap and over their channel pairing,
against the same operation in float64 (oracle.det_oracle.decode / clip on float64 inputs, a float64 softmax over the reference's
view(N, 2, -1, W) pairing).

grid_for caps the launch at 8,192 blocks x 256 threads = 2,097,152 threads; beyond that the kernels' grid-stride loop takes a second trip.
The softmax pairs channel c1 = 2a + 1 with c1 + A or c1 - A, which differs for odd and even A.

Bounds: boxes |got - ref| / max(|ref|, 1) <= 2e-5 (test_box_decode_vs_oracle), objectness 3e-5 (test_stereo_rpn_vs_oracle_and_reference).
Over 10^7 coordinates the box bound cannot hold for ANY fp32 evaluation: a corner is center -+ half a width, both of a few hundred
to a few thousand px (ulp 3e-5 .. 2.4e-4), and thousands of corners fall within a pixel of 0, where the bound is absolute.  There the
bound is twice the worst error, against float64 on the same inputs, of the same expression evaluated in torch float32 on the CPU
(`_bound`; the figures are in the tests' docstrings) -- taken from fp32 itself, never from the kernel."""
import functools

import pytest
import torch

from oracle import det_oracle as D
from disprcnn_amd.utils import synth

pytestmark = pytest.mark.gpu

CAP = 8192 * 256
BOX_TOL, OBJ_TOL = 2e-5, 3e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(got, ref):
    return ((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max().item() if ref.numel() else 0.0


def _bound(ref64, ref32, what):
    e32 = _rel(ref32, ref64)
    bound = max(BOX_TOL, 2 * e32)
    print(f"{what}: fp32-on-CPU vs float64 {e32:.3e} -> bound {bound:.3e}")
    return bound


# ------------------------------------------------------------------------------------------------ drc_box_decode_fwd
DECODE_BASE = {(3, 4): 700_100, (2, 4): 1_048_576, (2, 6): 1_049_676}
# rows, groups, per, clip_to: rows * groups just below, at, one above and well above the cap
DECODE_CASES = [(699_050, 3, 4, None), (1_048_576, 2, 4, (1242, 375)), (699_051, 3, 4, None), (699_051, 3, 4, (1242, 375)),
                (700_100, 3, 4, (1242, 375)), (1_049_676, 2, 6, None), (1_049_676, 2, 6, (1242, 375))]


@functools.lru_cache(maxsize=None)
def _decode_base(groups, per):
    """Inputs of DECODE_BASE rows and their per-row references (float64 and float32 on the CPU, unclipped); a case takes the first `rows`.
    Codes as in test_box_decode_vs_oracle, with dw / dh above the log(1000/16) clamp at every case's first and last row."""
    rows = DECODE_BASE[(groups, per)]
    w = (10.0, 10.0, 5.0, 5.0) if per == 4 else (1.0, 1.0, 1.0, 1.0)
    codes = synth.hash_uniform(f"edge{groups}x{per}", (rows, groups * per), -3.0, 3.0) * (4.0 if per == 4 else 1.0)
    for r in {0, rows - 1} | {c[0] - 1 for c in DECODE_CASES if (c[1], c[2]) == (groups, per)}:
        codes[r, 2::per] = 50.0
        codes[r, 3] = 31.0
        if per == 6:
            codes[r, 5] = 4.2
    b = synth.hash_uniform(f"edgeb{groups}x{per}", (rows, 4), 0.0, 1.0)
    boxes = torch.stack([b[:, 0] * 300, b[:, 1] * 150, b[:, 0] * 300 + b[:, 2] * 200, b[:, 1] * 150 + b[:, 3] * 100], 1)

    def ref(c, bx):
        return torch.cat([D.decode(c[:, g * per:(g + 1) * per], bx, w) for g in range(groups)], 1)
    return w, codes, boxes, ref(codes.double(), boxes.double()), ref(codes, boxes)


def _clip_rows(ref, per, clip):
    if clip is None:
        return ref
    r = ref.reshape(-1, per).clone()
    xs = [0, 2] + ([4, 5] if per == 6 else [])
    r[:, xs] = r[:, xs].clamp(0, clip[0] - 1)
    r[:, [1, 3]] = r[:, [1, 3]].clamp(0, clip[1] - 1)
    return r.reshape(ref.shape)


@pytest.mark.parametrize("rows,groups,per,clip", DECODE_CASES)
def test_box_decode_past_the_grid_cap(dev, rows, groups, per, clip):
    """BoxCoder.decode with rows * groups = cap - 2, cap, cap + 1 and cap + 3,148 (4 codes) and cap + 2,200 (6 codes), with and without
    clip_to.  The last 1,000 rows -- the rows of the second grid-stride trip where there is one -- are compared on their own.
    fp32 on the CPU against float64, this metric, these inputs (measured): 1.02e-4 for the 3 x 4 cases with and without clip_to, 6.6e-5
    for 2 x 4 clipped, 8.7e-5 / 7.6e-5 for 2 x 6 without / with clip_to (a corner within a pixel of 0 under a width of ~2,000 px); over
    the last 1,000 rows alone 1.7e-5 .. 5.1e-5.  So the bound is twice the whole tensor's figure, 1.3e-4 .. 2.0e-4, instead of 2e-5."""
    from disprcnn_amd.modeling.box_coder import BoxCoder
    w, codes, boxes, ref64, ref32 = _decode_base(groups, per)
    assert ref64.dtype == torch.float64
    codes, boxes = codes[:rows], boxes[:rows]
    ref64, ref32 = _clip_rows(ref64[:rows], per, clip), _clip_rows(ref32[:rows], per, clip)
    bound = _bound(ref64, ref32, f"decode {rows}x{groups}x{per} clip={clip}")
    got = BoxCoder(w).decode(codes.to(dev), boxes.to(dev), clip_to=clip, per=per).cpu()
    assert got.shape == codes.shape and torch.isfinite(got).all()
    tail, head = _rel(got[-1000:], ref64[-1000:]), _rel(got[:-1000], ref64[:-1000])
    print(f"  kernel vs float64: head {head:.3e}, last 1,000 rows {tail:.3e}")
    assert tail <= bound, "the last 1,000 rows (second grid-stride trip)"
    assert head <= bound, "rows of the first trip"
    # the clamp: rows 0 and rows - 1 carry dw = 50 / ww: the decoded width is exp(log(1000/16)) = 62.5 reference widths, not exp(10)
    if clip is None:
        for r in (0, rows - 1):
            bw = float(boxes[r, 2] - boxes[r, 0] + 1)
            assert abs(float(got[r, 2] - got[r, 0]) - 62.5 * bw) <= 1e-4 * 62.5 * bw


# ------------------------------------------------------------------------------------------------ drc_srpn_proposals_fwd
def _srpn_inputs(tag, n, a, h, w):
    logits = synth.hash_uniform(f"srpn{tag}:l", (n, 2 * a, h, w), -6.0, 6.0)
    reg = synth.hash_uniform(f"srpn{tag}:r", (n, 6 * a, h, w), -1.5, 1.5)
    reg[:, 2::6][:, :, 0, 0] = 9.0                         # dw above the clamp at the first position ...
    reg[:, 5::6][:, :, -1, -1] = 7.0                       # ... and dw' at the last
    u = synth.hash_uniform(f"srpn{tag}:a", (h * w * a, 4), 0.0, 1.0)
    anchors = torch.stack([u[:, 0] * 1100 - 50, u[:, 1] * 330 - 30, u[:, 0] * 1100 - 50 + 8 + u[:, 2] * 400, u[:, 1] * 330 - 30 + 8 + u[:, 3] * 250], 1)
    return logits, reg, anchors


def _srpn_ref(logits, reg, anchors, image_wh, dtype):
    """(scores [N, HWA], left [N, HWA, 4], right [N, HWA, 4]) in `dtype` on the CPU, restated from oracle.det_oracle.srpn_head / srpn_select."""
    n = logits.shape[0]
    lg, rg, an = logits.to(dtype), reg.to(dtype), anchors.to(dtype)
    obj = lg.view(n, 2, -1, lg.shape[3]).softmax(1).view(*lg.shape)          # pairs channel c with channel c +- A
    sc = obj.permute(0, 2, 3, 1).reshape(n, -1, 2)[:, :, 1]
    rg = rg.permute(0, 2, 3, 1).reshape(n, -1, 6)
    left, right = [], []
    for i in range(n):
        p = D.decode(rg[i], an, (1.0, 1.0, 1.0, 1.0))
        assert p.dtype == dtype
        left.append(D.clip(p[:, 0:4], *image_wh[i]))
        right.append(D.clip(p[:, [4, 1, 5, 3]], *image_wh[i]))
    return sc, torch.stack(left), torch.stack(right)


def _srpn_call(dev, logits, reg, anchors, image_wh, total, off, sc, left, right):
    from disprcnn_amd import _lib
    from disprcnn_amd import engine as E
    n, a2, h, w = logits.shape
    t = [x.to(dev).contiguous() for x in (logits, reg, anchors, torch.tensor(image_wh, dtype=torch.float32))]
    return _lib.lib().drc_srpn_proposals_fwd(E._ptr(t[0]), E._ptr(t[1]), E._ptr(t[2]), E._ptr(t[3]), n, a2 // 2, h, w, total, off, D.XFORM_CLIP,
                                             E._ptr(sc), E._ptr(left), E._ptr(right), E._stream_ptr(dev))


SENTINEL = -12345.0
IMAGE_WH = [(1242.0, 375.0), (1000.0, 300.0)]


@pytest.mark.parametrize("a", [1, 2, 3, 4, 5])
def test_srpn_proposals_channel_pairing_and_level_offsets(dev, a):
    """A = 1..5 (c2 = c1 + A or c1 - A: odd and even A pair channels differently), N = 2 with two image sizes, H != W, and two levels
    written into one sentinel-filled output at level offsets 3 and 3 + H1*W1*A + 2 with total_anchors larger than their sum: the slack
    entries stay untouched.  fp32 on the CPU against float64 on these inputs (measured): objectness 9e-8; boxes 1.8e-6 .. 9.4e-6, so the
    bound is 2e-5, except A = 4 at the first level: 1.65e-5, bound 3.3e-5."""
    levels = [(7, 11), (4, 5)]
    counts = [h * w * a for h, w in levels]
    offs = [3, 3 + counts[0] + 2]
    total = offs[1] + counts[1] + 4
    sc = torch.full((2, total), SENTINEL, device=dev)
    left, right = torch.full((2, total, 4), SENTINEL, device=dev), torch.full((2, total, 4), SENTINEL, device=dev)
    refs = []
    for lvl, (h, w) in enumerate(levels):
        inp = _srpn_inputs(f"{a}:{lvl}", 2, a, h, w)
        assert _srpn_call(dev, *inp, IMAGE_WH, total, offs[lvl], sc, left, right) == 0
        refs.append((_srpn_ref(*inp, IMAGE_WH, torch.float64), _srpn_ref(*inp, IMAGE_WH, torch.float32)))
    sc, left, right = sc.cpu(), left.cpu(), right.cpu()
    used = torch.zeros(total, dtype=torch.bool)
    for lvl in range(2):
        sl = slice(offs[lvl], offs[lvl] + counts[lvl])
        used[sl] = True
        (s64, l64, r64), (_, l32, r32) = refs[lvl]
        assert (sc[:, sl].double() - s64).abs().max().item() <= OBJ_TOL, f"objectness, A={a}, level {lvl}"
        assert 0.01 < s64.mean().item() < 0.99 and l64[1].max().item() == 999.0 and l64[0].max().item() == 1241.0      # each image's own clip
        bound = _bound(torch.cat((l64, r64)), torch.cat((l32, r32)), f"srpn A={a} level {lvl}")
        assert _rel(left[:, sl], l64) <= bound and _rel(right[:, sl], r64) <= bound, f"boxes, A={a}, level {lvl}"
    assert (sc[:, ~used] == SENTINEL).all() and (left[:, ~used] == SENTINEL).all() and (right[:, ~used] == SENTINEL).all()


def test_srpn_proposals_past_the_grid_cap(dev):
    """N = 2, A = 3, H = W = 600: 2,160,000 anchors, 62,848 of them in the second grid-stride trip (the end of image 1, compared on its
    own).  fp32 on the CPU against float64 on these inputs (measured): objectness 9.1e-8, boxes 9.6e-5 (a corner within a pixel of 0
    under a width of a few thousand px) -> box bound 1.9e-4 instead of 2e-5."""
    n, a, h, w = 2, 3, 600, 600
    per_img = h * w * a
    assert n * per_img > CAP > per_img
    inp = _srpn_inputs("cap", n, a, h, w)
    sc = torch.full((n, per_img), SENTINEL, device=dev)
    left, right = torch.full((n, per_img, 4), SENTINEL, device=dev), torch.full((n, per_img, 4), SENTINEL, device=dev)
    assert _srpn_call(dev, *inp, IMAGE_WH, per_img, 0, sc, left, right) == 0
    sc, left, right = sc.cpu(), left.cpu(), right.cpu()
    s64, l64, r64 = _srpn_ref(*inp, IMAGE_WH, torch.float64)
    _, l32, r32 = _srpn_ref(*inp, IMAGE_WH, torch.float32)
    bound = _bound(torch.cat((l64, r64)), torch.cat((l32, r32)), "srpn past the cap")
    trip2 = CAP - per_img                                   # image 1's first anchor of the second trip
    assert (sc[1, trip2:].double() - s64[1, trip2:]).abs().max().item() <= OBJ_TOL, "objectness, second grid-stride trip"
    assert _rel(left[1, trip2:], l64[1, trip2:]) <= bound and _rel(right[1, trip2:], r64[1, trip2:]) <= bound, "boxes, second grid-stride trip"
    assert (sc.double() - s64).abs().max().item() <= OBJ_TOL
    assert _rel(left, l64) <= bound and _rel(right, r64) <= bound


def test_srpn_proposals_argument_errors(dev):
    """A level that does not fit total_anchors, and A = 0: -2 before any launch (the output keeps its sentinel)."""
    inp = _srpn_inputs("err", 2, 3, 4, 5)
    sc = torch.full((2, 64), SENTINEL, device=dev)
    left, right = torch.full((2, 64, 4), SENTINEL, device=dev), torch.full((2, 64, 4), SENTINEL, device=dev)
    assert _srpn_call(dev, *inp, IMAGE_WH, 64, 5, sc, left, right) == -2           # 5 + 60 > 64
    assert _srpn_call(dev, *inp, IMAGE_WH, 59, 0, sc, left, right) == -2
    assert _srpn_call(dev, inp[0][:, :0], inp[1][:, :0], inp[2], IMAGE_WH, 64, 0, sc, left, right) == -2      # A = 0
    assert _srpn_call(dev, *inp, IMAGE_WH, 64, -1, sc, left, right) == -2
    torch.cuda.synchronize(dev)
    assert (sc.cpu() == SENTINEL).all() and (left.cpu() == SENTINEL).all() and (right.cpu() == SENTINEL).all()
    assert _srpn_call(dev, *inp, IMAGE_WH, 64, 4, sc, left, right) == 0            # 4 + 60 = 64 fits
    assert (sc.cpu()[:, 4:] != SENTINEL).all() and (sc.cpu()[:, :4] == SENTINEL).all()
