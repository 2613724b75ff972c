"""The host side of the device input path: everything drc_input_batch_fwd (pts/input_ops.hip) reads besides the pixels.

The reference transforms a sample on the host (data/transforms/transforms.py): PIL `Image.resize`, `hflip`, `to_tensor`, `[[2,1,0]] * 255`,
`normalize`, then `to_image_list` pads the batch.  Per output pixel that is a gather and a function of one byte, so it is described
here by

  index tables   int32, out_h + out_w entries per image: the source row of every output row and the source column of every output column.
                 They carry the resize and the flip.  The resize is Pillow's NEAREST (the reference's environment pins Pillow < 7, whose
                 `Image.resize` default is NEAREST): the source index of output x is int(xo) after xo = 0.5 * a, then xo += a, x times, in
                 double, a = in / out.  The repeated addition is part of the definition (np.add.accumulate adds in order).
  a LUT          fp32 [3][256]: the reference's torch CPU ops applied to all 256 bytes, in its order, per output channel
  a channel map  the source channel of each output channel ((2, 1, 0) with TO_BGR255)

`Resize` on the host (transforms.py) gathers with the same tables, so the two paths cannot disagree about a pixel.
"""
import numpy as np
import torch

DESC_INTS = 8          # src_off, src_h, src_w, out_h, out_w, ytab_off, xtab_off, 0  (input_ops.hip:kDescInts)
GRID_CAP = None        # workgroups of a launch; None = the library's default.  Tests lower it to make the kernels stride


def get_size(image_size, size, max_size):
    """(w, h) of the image, the drawn min size, the max size -> (oh, ow): Resize.get_size of the reference after its random.choice."""
    w, h = image_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def nearest_table(in_size, out_size):
    """Source index of every output index of Pillow's NEAREST resize of an axis from in_size to out_size: int32 [out_size]."""
    if in_size < 1 or out_size < 1:
        raise ValueError("nearest_table: sizes must be positive")
    if in_size == out_size:
        return np.arange(out_size, dtype=np.int32)
    a = float(in_size) / float(out_size)
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = 0.5 * a
    xo = np.add.accumulate(steps)                          # xo_0 = 0.5 a; xo_x = xo_{x-1} + a, each sum rounded to double in turn
    return np.minimum(xo.astype(np.int64), in_size - 1).astype(np.int32)


def axis_tables(src_hw, out_hw, flip=False):
    """-> (ytab [out_h], xtab [out_w]) int32; the flip reverses the x table (the reference flips after it resizes)."""
    ytab = nearest_table(src_hw[0], out_hw[0])
    xtab = nearest_table(src_hw[1], out_hw[1])
    return ytab, (xtab[::-1].copy() if flip else xtab)


def make_lut(mean, std, to_bgr255=True):
    """-> (lut fp32 [3,256] CPU tensor, chan): lut[c][u] is what ToTensor + Normalize make of byte u in output channel c, by the reference's
    torch CPU ops in its order -- u.float().div(255), * 255 with TO_BGR255, (t - mean[c]) / std[c] -- and chan[c] is the source channel."""
    t = torch.arange(256, dtype=torch.int32).to(torch.uint8).float().div(255)
    t = t[None].repeat(3, 1)
    if to_bgr255:
        t = t * 255
    mean = torch.as_tensor(mean, dtype=torch.float32)
    std = torch.as_tensor(std, dtype=torch.float32)
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError("make_lut: three channel means and deviations are expected")
    t = t.sub(mean[:, None]).div(std[:, None])
    return t.contiguous(), ((2, 1, 0) if to_bgr255 else (0, 1, 2))


def as_rgb_array(image):
    """PIL image, uint8 HWC array or uint8 HWC tensor -> contiguous uint8 [H,W,3] array; anything that is not 8-bit RGB raises."""
    if hasattr(image, "mode") and hasattr(image, "size") and not isinstance(image, np.ndarray) and not torch.is_tensor(image):
        if image.mode != "RGB":
            raise ValueError(f"input images must be RGB, got a PIL image of mode {image.mode!r}")
        image = np.asarray(image)
    elif torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"input images must be uint8 [H,W,3] RGB, got {image.dtype} {tuple(image.shape)}")
    if image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("input images must not be empty")
    return np.ascontiguousarray(image)


def padded_size(out_hws, size_divisible=0):
    """(Hp, Wp) of to_image_list over images of sizes out_hws."""
    hp = max(h for h, _ in out_hws)
    wp = max(w for _, w in out_hws)
    if size_divisible > 0:
        hp = -(-hp // size_divisible) * size_divisible
        wp = -(-wp // size_divisible) * size_divisible
    return hp, wp


class InputTables:
    """The tables of one launch: `ints` int32 (I descriptors, then the index tables), the padded size and the image sizes (h, w)."""

    def __init__(self, ints, n_images, hp, wp, image_sizes, src_bytes):
        self.ints, self.n_images, self.hp, self.wp, self.image_sizes, self.src_bytes = ints, n_images, hp, wp, list(image_sizes), src_bytes


def build_tables(src_hws, out_hws, flips, size_divisible=0):
    """Images of sizes src_hws (h, w), packed one after the other as HWC bytes, resized to out_hws and flipped where flips says
    -> InputTables."""
    n = len(src_hws)
    if not (n == len(out_hws) == len(flips)):
        raise ValueError("build_tables: one output size and one flip flag per image")
    desc = np.zeros((n, DESC_INTS), dtype=np.int64)
    tabs, pos, src_off = [], n * DESC_INTS, 0
    for i, (s, o, f) in enumerate(zip(src_hws, out_hws, flips)):
        ytab, xtab = axis_tables(s, o, f)
        desc[i] = (src_off, s[0], s[1], o[0], o[1], pos, pos + len(ytab), 0)
        tabs += [ytab, xtab]
        pos += len(ytab) + len(xtab)
        src_off += int(s[0]) * int(s[1]) * 3
    if src_off > 0x7fffffff or pos > 0x7fffffff:
        raise ValueError("build_tables: more than 2 GiB of pixels in one launch")
    hp, wp = padded_size(out_hws, size_divisible) if n else (0, 0)
    ints = np.concatenate([desc.astype(np.int32).reshape(-1)] + tabs) if n else np.zeros(0, np.int32)
    return InputTables(ints, n, hp, wp, [tuple(int(v) for v in o) for o in out_hws], src_off)


def pack_images(images):
    """uint8 [H,W,3] arrays -> one uint8 [sum H*W*3] array, in order."""
    return np.concatenate([im.reshape(-1) for im in images]) if len(images) else np.zeros(0, np.uint8)


def launch_input_batch(bytes_dev, ints_dev, tables, lut_dev, chan, out, max_blocks=None):
    """drc_input_batch_fwd over packed bytes and table ints that already lie on the device; `out` is fp32 [I,3,Hp,Wp], contiguous,
    every element of it is written."""
    from .. import engine as E
    from ..pts import _lib as P
    t = tables
    if not (bytes_dev.is_cuda and ints_dev.is_cuda and lut_dev.is_cuda and out.is_cuda):
        raise RuntimeError("input_batch: expected CUDA/HIP tensors on an MI355X; the HIP path has no CPU fallback")
    if bytes_dev.dtype != torch.uint8 or ints_dev.dtype != torch.int32 or lut_dev.dtype != torch.float32 or out.dtype != torch.float32:
        raise RuntimeError("input_batch: bytes are uint8, tables int32, the LUT and the output fp32")
    if tuple(out.shape) != (t.n_images, 3, t.hp, t.wp) or not out.is_contiguous():
        raise ValueError(f"input_batch: out must be contiguous [{t.n_images},3,{t.hp},{t.wp}], got {tuple(out.shape)}")
    if bytes_dev.numel() < t.src_bytes or ints_dev.numel() < t.ints.size or tuple(lut_dev.shape) != (3, 256):
        raise ValueError("input_batch: the device buffers are smaller than the tables say")
    if not (bytes_dev.is_contiguous() and ints_dev.is_contiguous() and lut_dev.is_contiguous()):
        raise ValueError("input_batch: contiguous buffers are expected")
    L = P.lib()
    cap = max_blocks if max_blocks is not None else (GRID_CAP if GRID_CAP is not None else L.drc_input_default_max_blocks())
    st = L.drc_input_batch_fwd(E._ptr(bytes_dev), int(t.src_bytes), E._ptr(ints_dev), int(t.ints.size), E._ptr(lut_dev), int(chan[0]),
                               int(chan[1]), int(chan[2]), t.n_images, t.hp, t.wp, E._ptr(out), int(cap), E._stream_ptr(out.device))
    P.check(st, "drc_input_batch_fwd")
    return out


def input_batch(images, tables, lut, chan, out=None, device=None, max_blocks=None):
    """uint8 [H,W,3] images (host arrays / PIL / tensors, or one packed uint8 GPU tensor) + InputTables + LUT + channel map -> the padded
    fp32 [I,3,Hp,Wp] batch on the GPU.  `out` may be any contiguous fp32 tensor of that shape, uninitialised: every element is written."""
    if torch.is_tensor(images) and images.is_cuda:
        bytes_dev = images
    else:
        arrays = [as_rgb_array(im) for im in images]
        if [a.shape[:2] for a in arrays] != [tuple(d[1:3]) for d in tables.ints[: tables.n_images * DESC_INTS].reshape(-1, DESC_INTS)]:
            raise ValueError("input_batch: the images do not have the sizes the tables were built for")
        if device is None:
            device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
        bytes_dev = torch.from_numpy(pack_images(arrays)).to(device)
    dev = bytes_dev.device
    if out is None:
        out = torch.empty((tables.n_images, 3, tables.hp, tables.wp), dtype=torch.float32, device=dev)
    if tables.n_images == 0 or out.numel() == 0:
        return out
    ints_dev = torch.from_numpy(tables.ints).to(dev)
    lut_dev = lut if lut.is_cuda else lut.to(dev)
    return launch_input_batch(bytes_dev, ints_dev, tables, lut_dev.contiguous(), chan, out, max_blocks)
