"""SegmentationMask / BinaryMaskList: the instance masks of one image as a uint8 [G,H,W] tensor of 0/1 that follows the image through
resize, flip and crop (reference: disprcnn/structures/segmentation_mask.py:34-191, 460-578).

Only binary masks are built: KITTI's masks are binary, and polygons / RLE need pycocotools (`mode='poly'` and RLE input raise).

`resize` resamples with the taps and weights of torch's bilinear interpolation (align_corners=False) -- pts/mask_resize.h:resize_axis --
and sets a pixel iff EVERY tap whose fp32 weight is non-zero is set.  That is what the reference's `interpolate(...).type_as(uint8)`
computes in exact arithmetic; its fp32 sum rounds some all-ones neighbourhoods to 0.99999994 and truncates them to 0, at pixels that
depend on the shape and on torch's summation order, so the rule is stated without a floating-point sum.  A GPU tensor goes through the
HIP kernel (drc_mask_resize_flip_fwd, pts/input_ops.hip; `resize_flip_batch` runs many mask lists in one launch).  A CPU tensor (the
data side in front of the device path, as DisparityMap._resize_cpu) applies the same rule with torch indexing: a GPU tensor never takes
that route.
"""
import warnings

import numpy as np
import torch

FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1


def resize_axis(in_size, out_size):
    """mask_resize.h:resize_axis for every output index at once -> (i0, i1 int64 [out], l0, l1 float32 [out]).  The source coordinate is
    one fused multiply-add in fp32: the double product of two floats minus 0.5 is exact, so rounding it once is the same value."""
    idx = np.arange(out_size, dtype=np.int64)
    if in_size == out_size:
        return idx, idx.copy(), np.ones(out_size, np.float32), np.zeros(out_size, np.float32)
    scale = np.float32(in_size) / np.float32(out_size)
    src = (np.float64(scale) * (idx.astype(np.float32) + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, np.float32(1) - l1, l1


def _resize_cpu(masks, oh, ow):
    """The rule of drc_mask_resize_flip_fwd on a CPU tensor: rows first, then columns (the conjunction over the taps is separable)."""
    on = masks != 0
    for dim, (n_in, n_out) in ((1, (masks.shape[1], oh)), (2, (masks.shape[2], ow))):
        i0, i1, l0, l1 = resize_axis(n_in, n_out)
        shape = [1, 1, 1]
        shape[dim] = n_out
        skip0 = torch.from_numpy(l0 == 0).reshape(shape)
        skip1 = torch.from_numpy(l1 == 0).reshape(shape)
        on = (on.index_select(dim, torch.from_numpy(i0)) | skip0) & (on.index_select(dim, torch.from_numpy(i1)) | skip1)
    return on.to(torch.uint8)


def mask_jobs(pairs, flips):
    """Job rows of drc_mask_resize_flip_fwd for (src [G,H,W] uint8 GPU, dst [G,oh,ow] uint8 GPU) pairs -> (int64 array [J,cols], quads).
    Pairs without output elements get no row."""
    from ..pts import _lib as P
    cols = P.lib().drc_mask_job_cols()
    rows, quads = [], 0
    for (src, dst), flip in zip(pairs, flips):
        for t in (src, dst):
            if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.is_contiguous()):
                raise RuntimeError("mask resize: contiguous uint8 [G,H,W] tensors on the GPU are expected; the HIP path has no CPU fallback")
        if src.shape[0] != dst.shape[0]:
            raise ValueError("mask resize: source and destination hold different numbers of masks")
        n = dst.numel()
        if n == 0:
            continue
        if src.numel() == 0:
            raise ValueError("mask resize: an empty source cannot fill a non-empty destination")
        q = (n + 3) // 4
        rows.append([src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], src.shape[2], dst.shape[1], dst.shape[2], int(bool(flip)),
                     quads, q])
        quads += q
    return np.asarray(rows, dtype=np.int64).reshape(len(rows), cols), quads


def launch_mask_jobs(jobs_dev, n_jobs, quads, device, max_blocks=None):
    """One launch over job rows that already lie on the device (int64, contiguous)."""
    from .. import engine as E
    from ..pts import _lib as P
    if n_jobs == 0 or quads == 0:
        return
    L = P.lib()
    cap = L.drc_input_default_max_blocks() if max_blocks is None else int(max_blocks)
    P.check(L.drc_mask_resize_flip_fwd(E._ptr(jobs_dev), int(n_jobs), int(quads), cap, E._stream_ptr(device)), "drc_mask_resize_flip_fwd")


def resize_flip_batch(masks, sizes, flips, max_blocks=None):
    """[G_k,H_k,W_k] uint8 GPU tensors, (width, height) per tensor, flip flag per tensor -> the resized (then left-right flipped) tensors,
    all in ONE launch (none when there is nothing to write)."""
    masks = [m.contiguous() for m in masks]
    outs = [torch.empty((m.shape[0], int(h), int(w)), dtype=torch.uint8, device=m.device) for m, (w, h) in zip(masks, sizes)]
    rows, quads = mask_jobs(list(zip(masks, outs)), flips)
    if len(rows):
        dev = masks[0].device
        launch_mask_jobs(torch.from_numpy(rows).to(dev), len(rows), quads, dev, max_blocks)
    return outs


class BinaryMaskList(object):
    """The binary masks of all objects of one image: `masks` uint8 [G,H,W], `size` = (width, height)."""

    def __init__(self, masks, size):
        size = tuple(size)
        if isinstance(masks, BinaryMaskList):
            masks = masks.masks.clone()
        elif torch.is_tensor(masks):
            masks = masks.clone()
        elif isinstance(masks, np.ndarray):
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        elif isinstance(masks, (list, tuple)):
            if len(masks) == 0:
                masks = torch.empty((0, int(size[1]), int(size[0])), dtype=torch.uint8)
            elif torch.is_tensor(masks[0]):
                masks = torch.stack(list(masks), dim=0)
            elif isinstance(masks[0], np.ndarray):
                masks = torch.from_numpy(np.stack(masks))
            elif isinstance(masks[0], dict) and "counts" in masks[0]:
                raise NotImplementedError("BinaryMaskList: RLE masks need pycocotools, which is not part of this implementation")
            else:
                raise TypeError(f"BinaryMaskList: masks of {type(masks[0])} cannot be interpreted")
        else:
            raise TypeError(f"BinaryMaskList: {type(masks)} cannot be interpreted")
        if masks.dim() == 2:
            masks = masks[None]
        if masks.dim() != 3 or masks.shape[1] != size[1] or masks.shape[2] != size[0]:
            raise ValueError(f"BinaryMaskList: masks {tuple(masks.shape)} do not have the image size (w, h) = {size}")
        self.masks = masks.to(torch.uint8)
        self.size = size

    @classmethod
    def owning(cls, masks, size):
        """A list over a uint8 [G,H,W] tensor that nobody else holds (a fresh result): no copy is made."""
        out = cls.__new__(cls)
        out.masks, out.size = masks.to(torch.uint8), tuple(size)
        return out

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        if method == FLIP_LEFT_RIGHT and self.masks.is_cuda:
            return BinaryMaskList.owning(resize_flip_batch([self.masks], [self.size], [True])[0], self.size)
        return BinaryMaskList.owning(self.masks.flip(1 if method == FLIP_TOP_BOTTOM else 2), self.size)

    def crop(self, box):
        """box = xyxy, rounded half to even and clamped as mask_resize.h:crop_bounds (reference :97-116)."""
        w, h = self.size
        xmin, ymin, xmax, ymax = (round(float(b)) for b in box)
        if xmin > xmax or ymin > ymax:
            raise ValueError(f"BinaryMaskList.crop: {tuple(box)} is not a forward window")
        xmin, ymin = min(max(xmin, 0), w - 1), min(max(ymin, 0), h - 1)
        xmax, ymax = min(max(xmax, 0), w), min(max(ymax, 0), h)
        xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
        return BinaryMaskList(self.masks[:, ymin:ymax, xmin:xmax], (xmax - xmin, ymax - ymin))

    def resize(self, size, use_max_pooling=False):
        try:
            iter(size)
        except TypeError:
            size = size, size
        width, height = map(int, size)
        if width < 0 or height < 0:
            warnings.warn("dst size < 0, size will not change.")
            return BinaryMaskList(self.masks, self.size)
        if width == 0 or height == 0:
            raise ValueError("BinaryMaskList.resize: the destination is empty")
        if use_max_pooling:
            import torch.nn.functional as F
            out = F.adaptive_max_pool2d(self.masks[None].float(), (height, width))[0].to(torch.uint8)
        elif self.masks.is_cuda:
            out = resize_flip_batch([self.masks], [(width, height)], [False])[0]
        else:
            out = _resize_cpu(self.masks, height, width)
        return BinaryMaskList.owning(out, (width, height))

    def to(self, *args, **kwargs):
        """Unlike the reference's (which stays where it is), the masks move: the device collator and the 3D stage read them on the GPU."""
        moved = self.masks.to(*args, **kwargs)             # the same tensor when nothing changes, as Tensor.to
        return self if moved is self.masks else BinaryMaskList.owning(moved, self.size)

    def __len__(self):
        return len(self.masks)

    def __getitem__(self, index):
        if self.masks.numel() == 0:
            return self
        return BinaryMaskList(self.masks[index], self.size)

    def __iter__(self):
        return iter(self.masks)

    def __repr__(self):
        return f"{self.__class__.__name__}(num_instances={len(self.masks)}, image_width={self.size[0]}, image_height={self.size[1]})"


def invalid_size(size):
    return (isinstance(size, int) and size < 0) or (isinstance(size, (tuple, list)) and any(a < 0 for a in size))


class SegmentationMask(object):
    """The segmentations of all objects of one image (reference :460-578), over a BinaryMaskList."""

    def __init__(self, instances, size, mode="mask"):
        if not isinstance(size, (list, tuple)) or len(size) != 2:
            raise ValueError(f"expect {size} to be a (width, height) list or tuple")
        size = tuple(s.item() if torch.is_tensor(s) else s for s in size)
        if mode == "poly":
            raise NotImplementedError("SegmentationMask: polygon masks need pycocotools, which is not part of this implementation; "
                                      "pass binary masks with mode='mask'")
        if mode != "mask":
            raise NotImplementedError(f"Unknown mode: {mode}")
        self.instances = instances if isinstance(instances, BinaryMaskList) and instances.size == size else BinaryMaskList(instances, size)
        self.mode = mode
        self.size = size

    @property
    def masks(self):
        """The uint8 [G,H,W] tensor (what mask_head_loss._mask_tensor and the 3D stage read)."""
        return self.instances.masks

    def transpose(self, method):
        return SegmentationMask(self.instances.transpose(method), self.size, self.mode)

    def crop(self, box):
        cropped = self.instances.crop(box)
        return SegmentationMask(cropped, cropped.size, self.mode)

    def resize(self, size, use_max_pooling=False):
        if invalid_size(size):
            warnings.warn("dst size < 0, size will not change.")
            return SegmentationMask(self.instances, self.size, self.mode)
        resized = self.instances.resize(size, use_max_pooling)
        return SegmentationMask(resized, resized.size, self.mode)

    def to(self, *args, **kwargs):
        return SegmentationMask(self.instances.to(*args, **kwargs), self.size, self.mode)

    def convert(self, mode):
        if mode == self.mode:
            return self
        raise NotImplementedError("SegmentationMask.convert: only 'mask' is built (polygons need pycocotools)")

    def get_mask_tensor(self, squeeze=True):
        t = self.instances.masks
        return t.squeeze(0) if squeeze else t

    def get_full_image_mask_tensor(self):
        t = self.get_mask_tensor()
        if t.dim() == 3:
            t = t.sum(dim=0)
        return t.clamp(max=1)

    def __len__(self):
        return len(self.instances)

    def __getitem__(self, item):
        return SegmentationMask(self.instances[item], self.size, self.mode)

    def __iter__(self):
        self.iter_idx = 0
        return self

    def __next__(self):
        if self.iter_idx < len(self):
            out = self[self.iter_idx]
            self.iter_idx += 1
            return out
        raise StopIteration()

    def __repr__(self):
        return (f"{self.__class__.__name__}(num_instances={len(self.instances)}, image_width={self.size[0]}, "
                f"image_height={self.size[1]}, mode={self.mode})")

    @property
    def width(self):
        return self.size[0]

    @property
    def height(self):
        return self.size[1]
