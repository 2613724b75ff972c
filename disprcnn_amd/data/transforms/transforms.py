"""Per-sample host transforms under the reference's names (disprcnn/data/transforms/transforms.py): Compose, Resize,
RandomHorizontalFlip, ToTensor, Normalize.  Each takes (image, target) -- single view, or {'left', 'right'} dicts of both -- and draws from
the `random` module in the reference's calls and order.  Images are PIL images or uint8 [H,W,3] arrays; without torchvision they travel
as uint8 arrays from the first transform that touches them and become a float [3,H,W] tensor in ToTensor.

`Resize` is Pillow's NEAREST (the `Image.resize` default of the Pillow < 7 the reference pins), gathered with the index tables of
data/device_input.py -- the same tables DeviceBatchCollator hands to the HIP kernel.

Not built: ColorJitter, FixSizeCrop, ToRGB255, ToPILImage, ImageNetNormalize (no shipped KITTI config uses them).
"""
import random

import numpy as np
import torch

from ..device_input import as_rgb_array, get_size, nearest_table


def _double(image, target):
    return isinstance(image, dict) and isinstance(target, dict)


def _image_size(image):
    """(w, h) of a PIL image or an [H,W,3] array."""
    if isinstance(image, np.ndarray) or torch.is_tensor(image):
        return image.shape[1], image.shape[0]
    return image.size


class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join(f"\n    {t}" for t in self.transforms) + "\n)"


class _PerView(object):
    """call_single_view on each view of a pair, left first, unless a transform defines call_double_view itself."""

    def call_double_view(self, image, target):
        left_image, left_target = self.call_single_view(image["left"], target["left"])
        right_image, right_target = self.call_single_view(image["right"], target["right"])
        return {"left": left_image, "right": right_image}, {"left": left_target, "right": right_target}

    def __call__(self, image, target):
        if _double(image, target):
            return self.call_double_view(image, target)
        return self.call_single_view(image, target)


class Resize(_PerView):
    def __init__(self, min_size, max_size):
        if not isinstance(min_size, (list, tuple)):
            min_size = (min_size,)
        self.min_size = min_size
        self.max_size = max_size

    def get_size(self, image_size):
        """(w, h) -> (oh, ow); one random.choice over the min sizes, like the reference."""
        return get_size(image_size, random.choice(self.min_size), self.max_size)

    def call_single_view(self, image, target):
        h, w = self.get_size(_image_size(image))
        a = as_rgb_array(image)
        image = a[nearest_table(a.shape[0], h)][:, nearest_table(a.shape[1], w)]
        return image, target.resize((w, h))


class RandomHorizontalFlip(_PerView):
    def __init__(self, prob=0.5):
        self.prob = prob

    def call_single_view(self, image, target):
        if random.random() < self.prob:
            image = as_rgb_array(image)[:, ::-1]
            target = target.transpose(0)
        return image, target

    def call_double_view(self, image, target):
        """One draw for the pair: both views flip or neither."""
        if random.random() < self.prob:
            image = {k: as_rgb_array(image[k])[:, ::-1] for k in ("left", "right")}
            target = {k: target[k].transpose(0) for k in ("left", "right")}
        return image, target


class ToTensor(_PerView):
    def call_single_view(self, image, target):
        a = np.ascontiguousarray(as_rgb_array(image))
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div(255), target


class Normalize(_PerView):
    def __init__(self, mean, std, to_bgr255=True):
        self.mean = mean
        self.std = std
        self.to_bgr255 = to_bgr255

    def _normalize(self, image):
        mean = torch.as_tensor(self.mean, dtype=image.dtype)
        std = torch.as_tensor(self.std, dtype=image.dtype)
        return image.sub(mean[:, None, None]).div(std[:, None, None])

    def call_single_view(self, image, target):
        """As the reference's single-view form, which leaves the channel order and range alone whatever to_bgr255 says."""
        return self._normalize(image), target

    def call_double_view(self, image, target):
        out = {}
        for k in ("left", "right"):
            t = image[k]
            if self.to_bgr255:
                t = t[[2, 1, 0]] * 255
            out[k] = self._normalize(t)
        return out, {"left": target["left"], "right": target["right"]}
