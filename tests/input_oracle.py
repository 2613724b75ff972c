"""NumPy restatement of the input pipeline, written from the reference and from Pillow's Geometry.c, not from the package's code:

  get_size          data/transforms/transforms.py:44-64 (after its random.choice)
  nearest_table     Pillow's NEAREST scale: xo = 0.5 * a, then xo += a once per output index, in double; the source index is int(xo)
  lut               ToTensor + Normalize on all 256 bytes by torch CPU ops in the reference's order (transforms.py:144, 183-189)
  image_batch       the gather with to_image_list's zero padding (structures/image_list.py)
  resize_axis       pts/mask_resize.h:resize_axis, scalar, with the fused multiply-add taken in double and rounded once
  mask_resize_flip  a pixel is 1 iff every tap with a non-zero fp32 weight is 1; flip reads the resized column ow-1-x
"""
import numpy as np
import torch

F32 = np.float32


def get_size(w, h, size, max_size):
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def nearest_table(n_in, n_out):
    a = float(n_in) / float(n_out)
    xo, tab = 0.5 * a, []
    for _ in range(n_out):
        tab.append(int(xo))
        xo += a
    return np.asarray(tab, dtype=np.int32)


def lut(mean, std, to_bgr255):
    """fp32 [3,256] and the source channel of each output channel."""
    u = torch.arange(256).to(torch.uint8)
    img = u.reshape(1, 1, 256).repeat(3, 1, 1)                     # a [3,1,256] "image" whose every channel holds every byte
    t = img.float().div(255)
    if to_bgr255:
        t = t[[2, 1, 0]] * 255
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    t = t.sub(m[:, None, None]).div(s[:, None, None])
    return t[:, 0].numpy(), ((2, 1, 0) if to_bgr255 else (0, 1, 2))


def padded(sizes, div):
    hp, wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if div > 0:
        hp, wp = -(-hp // div) * div, -(-wp // div) * div
    return hp, wp


def image_batch(images, out_hws, flips, mean, std, to_bgr255, div):
    """uint8 [H,W,3] arrays -> fp32 [I,3,Hp,Wp]."""
    table, chan = lut(mean, std, to_bgr255)
    hp, wp = padded(out_hws, div)
    out = np.zeros((len(images), 3, hp, wp), dtype=F32)
    for i, (im, (oh, ow), flip) in enumerate(zip(images, out_hws, flips)):
        yt, xt = nearest_table(im.shape[0], oh), nearest_table(im.shape[1], ow)
        if flip:
            xt = xt[::-1]
        g = im[yt][:, xt]                                           # [oh, ow, 3]
        for c in range(3):
            out[i, c, :oh, :ow] = table[c][g[:, :, chan[c]]]
    return out


def resize_axis(o, n_in, n_out):
    """-> (i0, i1, l0, l1) of output index o."""
    if n_in == n_out:
        return o, o, F32(1), F32(0)
    scale = F32(n_in) / F32(n_out)
    src = F32(float(scale) * float(F32(o) + F32(0.5)) - 0.5)        # the product of two floats is exact in double: one rounding
    src = max(src, F32(0))
    i0 = min(int(np.floor(src)), n_in - 1)
    l1 = min(max(F32(src - F32(i0)), F32(0)), F32(1))
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    return i0, i1, F32(1) - l1, l1


def mask_resize_flip(masks, oh, ow, flip):
    """uint8 [G,H,W] -> uint8 [G,oh,ow] by the exact rule."""
    G, H, W = masks.shape
    on = masks != 0
    ys = [resize_axis(y, H, oh) for y in range(oh)]
    xs = [resize_axis(x, W, ow) for x in range(ow)]
    rows = np.ones((G, oh, W), dtype=bool)
    for y, (i0, i1, l0, l1) in enumerate(ys):
        if l0 != 0:
            rows[:, y] &= on[:, i0]
        if l1 != 0:
            rows[:, y] &= on[:, i1]
    out = np.ones((G, oh, ow), dtype=bool)
    for x, (i0, i1, l0, l1) in enumerate(xs):
        if l0 != 0:
            out[:, :, x] &= rows[:, :, i0]
        if l1 != 0:
            out[:, :, x] &= rows[:, :, i1]
    if flip:
        out = out[:, :, ::-1]
    return out.astype(np.uint8)


def torch_bilinear(masks, oh, ow):
    """The reference's resize before its cast: F.interpolate(bilinear, align_corners=False) on the CPU, fp32 [G,oh,ow]."""
    import torch.nn.functional as F
    return F.interpolate(torch.from_numpy(masks)[None].float(), size=(oh, ow), mode="bilinear", align_corners=False)[0].numpy()


def blobs(G, H, W, seed, speckle=0.02):
    """0/1 masks: an ellipse per instance with a 2 % speckle of flipped pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((G, H, W), dtype=np.uint8)
    for g in range(G):
        cy, cx = rng.uniform(0.25, 0.75) * H, rng.uniform(0.25, 0.75) * W
        ry, rx = rng.uniform(0.2, 0.45) * H, rng.uniform(0.2, 0.45) * W
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        out[g] = m ^ (rng.uniform(size=(H, W)) < speckle)
    return out
