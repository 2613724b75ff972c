"""Batch collators (reference: disprcnn/data/collate_batch.py) and the device collator that replaces transforms + collate + upload.

BatchCollator / DoubleViewBatchCollator take samples that are ALREADY transformed, as the reference's do.

DeviceBatchCollator(cfg, is_train, device) takes RAW samples `(imgs, targets, idx[, left_pred, right_pred])` -- imgs = {'left', 'right'}
of PIL images or uint8 [H,W,3] arrays / tensors, targets = {'left', 'right'} of BoxLists at the original size -- and returns what
DoubleViewBatchCollator would have returned after build_transforms(cfg, is_train), on the device:

  * one host-to-device copy of the packed uint8 pixels of both views and one of all tables (index tables, image descriptors, mask jobs),
    both from pinned staging buffers; nothing is read back;
  * one drc_input_batch_fwd launch per view writes the padded fp32 batch (resize, flip, channel order, normalisation, padding);
  * one drc_mask_resize_flip_fwd launch per view resizes and flips the instance masks of every target of the view;
  * boxes, calibration and the disparity map follow through BoxList.resize / transpose (DisparityMap.resize is drc_disparity_resize_fwd).

Random draws come from `rng` (the `random` module, or a random.Random) in the reference's calls and order, sample by sample:
choice(min_size) for the left view, again for the right view (both only with INPUT.DO_RESIZE), then one random() per pair for the flip,
drawn even when the probability is 0.  So random.seed(k) gives the sizes and flips of the host path.

It runs in the process that owns the GPU (a DataLoader worker has none): give the DataLoader `collate_fn=list` and call this on its
batches, or call it directly.
"""
import random as _random

import numpy as np
import torch

from ..structures.bounding_box import FLIP_LEFT_RIGHT, BoxList
from ..structures.image_list import ImageList, to_image_list
from ..structures.segmentation_mask import BinaryMaskList, SegmentationMask, launch_mask_jobs, mask_jobs
from . import device_input as D
from .device_input import input_batch  # noqa: F401  -- the lower-level entry, re-exported next to the collators
from .transforms.build import transform_params

VIEWS = ("left", "right")


class BatchCollator(object):
    """From a list of samples from the dataset, returns the batched images and targets."""

    def __init__(self, size_divisible=0):
        self.size_divisible = size_divisible

    def __call__(self, batch):
        transposed_batch = list(zip(*batch))
        images = to_image_list(list(transposed_batch[0]), self.size_divisible)
        return images, transposed_batch[1], transposed_batch[2]


class DoubleViewBatchCollator(BatchCollator):
    def __call__(self, batch):
        transposed_batch = list(zip(*batch))
        images = {k: to_image_list([b[k] for b in transposed_batch[0]], self.size_divisible) for k in VIEWS}
        targets = {k: [t[k] for t in transposed_batch[1]] for k in VIEWS}
        img_ids = transposed_batch[2]
        if len(transposed_batch) == 5:
            preds2d = {"left": list(transposed_batch[3]), "right": list(transposed_batch[4])}
            return images, targets, [img_ids, preds2d]
        return images, targets, img_ids


class SamplePlan(object):
    """What the random draws decided for one pair: the output size (h, w) of each view and whether the pair flips."""

    def __init__(self, sizes, flip):
        self.sizes, self.flip = sizes, flip


class _Staging(object):
    """A pinned host buffer that grows; the copy out of it is asynchronous, so it is handed out again only after that copy is done."""

    def __init__(self, dtype):
        self.dtype, self.buf, self.done = dtype, None, None

    def take(self, n):
        if self.done is not None:
            self.done.synchronize()
            self.done = None
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(max(n, 1), dtype=self.dtype, pin_memory=True)
        return self.buf[:n]

    def upload(self, host, device):
        dev = host.to(device, non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(device))
        return dev


class DeviceBatchCollator(object):
    def __init__(self, cfg, is_train=True, device="cuda", rng=None):
        self.min_size, self.max_size, self.flip_prob = transform_params(cfg, is_train)
        self.do_resize = bool(cfg.INPUT.DO_RESIZE)
        self.size_divisible = int(cfg.DATALOADER.SIZE_DIVISIBILITY)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceBatchCollator: expected a CUDA/HIP device (an MI355X); the HIP path has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.rng = _random if rng is None else rng
        lut, self.chan = D.make_lut(cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255)
        self.lut = lut.to(self.device)
        self._bytes, self._ints = _Staging(torch.uint8), _Staging(torch.int32)

    # ---- the draws
    def plan(self, image_sizes):
        """[(w, h) of the left image, (w, h) of the right image] per sample -> [SamplePlan], drawing from rng like the host transforms."""
        plans = []
        for pair in image_sizes:
            if self.do_resize:
                sizes = [D.get_size(wh, self.rng.choice(self.min_size), self.max_size) for wh in pair]
            else:
                sizes = [(wh[1], wh[0]) for wh in pair]
            plans.append(SamplePlan(sizes, self.rng.random() < self.flip_prob))
        return plans

    # ---- targets
    def _follow(self, target, out_hw, flip, masks):
        """The target after Resize and RandomHorizontalFlip; its masks were resampled by the batched launch and are put back in place."""
        if not isinstance(target, BoxList):
            raise TypeError(f"DeviceBatchCollator: targets are BoxLists, got {type(target)}")
        if masks is not None:
            rest = BoxList(target.bbox, target.size, target.mode)
            rest.extra_fields = {k: v for k, v in target.extra_fields.items() if k != "masks"}
            rest.PixelWise_map = dict(target.PixelWise_map)
        else:
            rest = target
        if self.do_resize:
            rest = rest.resize((out_hw[1], out_hw[0]))
        if flip:
            rest = rest.transpose(FLIP_LEFT_RIGHT)
        if masks is not None:
            size = (masks.shape[2], masks.shape[1])
            masks = SegmentationMask(BinaryMaskList.owning(masks, size), size, "mask")
            fields = {k: (masks if k == "masks" else rest.extra_fields[k]) for k in target.extra_fields}
            rest.extra_fields = fields
        return rest

    def __call__(self, batch):
        if len(batch) == 0:
            raise ValueError("DeviceBatchCollator: an empty batch")
        cols = list(zip(*batch))
        if len(cols) not in (3, 5) or not all(isinstance(c, dict) for c in cols[0]) or not all(isinstance(c, dict) for c in cols[1]):
            raise NotImplementedError("DeviceBatchCollator: samples are (imgs, targets, idx[, left_pred, right_pred]) with {'left', 'right'} "
                                      "dicts; only the double-view form is built")
        dev = self.device
        arrays = {k: [D.as_rgb_array(s[k]) for s in cols[0]] for k in VIEWS}
        plans = self.plan([[(arrays[k][i].shape[1], arrays[k][i].shape[0]) for k in VIEWS] for i in range(len(batch))])
        targets = {k: [s[k].to(dev) for s in cols[1]] for k in VIEWS}

        # tables of both views, then the mask jobs, in one int32 buffer; pixels of both views in one uint8 buffer
        tables, mask_out, jobs = {}, {}, {}
        for v, k in enumerate(VIEWS):
            tables[k] = D.build_tables([a.shape[:2] for a in arrays[k]], [p.sizes[v] for p in plans], [p.flip for p in plans],
                                       self.size_divisible)
            pairs, flips, mask_out[k] = [], [], []
            for t, p in zip(targets[k], plans):
                m = t.get_field("masks") if isinstance(t, BoxList) and t.has_field("masks") else None
                if not isinstance(m, SegmentationMask) or not (self.do_resize or p.flip):
                    mask_out[k].append(None)           # tensors pass through BoxList.resize untouched, as they always did
                    continue
                src = m.masks.contiguous()
                oh, ow = p.sizes[v]
                dst = torch.empty((src.shape[0], oh, ow), dtype=torch.uint8, device=dev)
                pairs.append((src, dst))
                flips.append(p.flip)
                mask_out[k].append(dst)                # wrapped after the launch: only then does it hold the masks
            jobs[k] = mask_jobs(pairs, flips)
        parts, pos, where = [], 0, {}
        for k in VIEWS:
            where["t" + k] = pos
            parts.append(tables[k].ints)
            pos += tables[k].ints.size
        pos += pos & 1                                   # the int64 job rows start on 8 bytes
        pad = pos - sum(p.size for p in parts)
        if pad:
            parts.append(np.zeros(pad, np.int32))
        for k in VIEWS:
            where["j" + k] = pos
            parts.append(jobs[k][0].reshape(-1).view(np.int32))
            pos += parts[-1].size
        host_ints = self._ints.take(pos)
        np.concatenate(parts, out=host_ints.numpy())
        n_bytes = sum(tables[k].src_bytes for k in VIEWS)
        host_bytes = self._bytes.take(n_bytes)
        np.concatenate([a.reshape(-1) for k in VIEWS for a in arrays[k]], out=host_bytes.numpy())
        ints_dev = self._ints.upload(host_ints, dev)
        bytes_dev = self._bytes.upload(host_bytes, dev)

        images, off = {}, 0
        for k in VIEWS:
            t = tables[k]
            out = torch.empty((t.n_images, 3, t.hp, t.wp), dtype=torch.float32, device=dev)
            D.launch_input_batch(bytes_dev[off: off + t.src_bytes], ints_dev[where["t" + k]: where["t" + k] + t.ints.size], t, self.lut,
                                 self.chan, out)
            off += t.src_bytes
            images[k] = ImageList(out, t.image_sizes)
            rows, quads = jobs[k]
            if len(rows):
                launch_mask_jobs(ints_dev[where["j" + k]: where["j" + k] + rows.size * 2].view(torch.int64), len(rows), quads, dev)
        out_targets = {k: [self._follow(t, p.sizes[v], p.flip, m) for t, p, m in zip(targets[k], plans, mask_out[k])]
                       for v, k in enumerate(VIEWS)}
        img_ids = cols[2]
        if len(cols) == 5:
            return images, out_targets, [img_ids, {"left": list(cols[3]), "right": list(cols[4])}]
        return images, out_targets, img_ids
