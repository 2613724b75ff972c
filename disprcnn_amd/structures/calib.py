"""Calib: the per-image camera calibration the 3D stage reads (reference: disprcnn/structures/calib.py:10-122 over
utils/kitti_utils.py:Calibration).

`Calib(calibration, image_size)` takes any object with 3x4 `P2` / `P3` projection matrices -- the reference's
`kitti_utils.Calibration`, or a plain namespace.  `.calib` exposes the intrinsics the reference reads off it (`fu, fv, cu, cv, tx,
ty`, float64 as NumPy computes them) and forwards any other attribute to the wrapped object.  `img_to_rect` / `depthmap_to_rect` on
torch tensors have the reference's arithmetic: fp32 tensors with the intrinsics as scalars, points in the x-major order of
meshgrid(x, y).

`resize` / `crop` return a new Calib whose projection matrices follow the image (reference :48-76), so a target that went through
`BoxList.resize` carries the intrinsics of the image it now describes.
"""
import warnings

import numpy as np
import torch

_MATRICES = ("P0", "P2", "P3")


class _Replaced:
    """A calibration source with some projection matrices replaced; every other attribute comes from the original."""

    def __init__(self, source, matrices):
        self._source = source
        self.__dict__.update(matrices)

    def __getattr__(self, name):
        if name.startswith("__") or name == "_source":
            raise AttributeError(name)
        return getattr(self._source, name)


class CameraIntrinsics:
    """fu, fv, cu, cv, tx, ty of the left colour camera from P2 (kitti_utils.py:28-49); other attributes come from `source`."""

    def __init__(self, source):
        self.source = source
        self.P2 = np.asarray(source.P2, dtype=np.float64).reshape(3, 4)
        self.P3 = np.asarray(source.P3, dtype=np.float64).reshape(3, 4)

    def __getattr__(self, name):
        if name == "source" or name.startswith("__"):   # no special method is borrowed from the source: copy / pickle see this class
            raise AttributeError(name)
        return getattr(self.source, name)

    def stored_matrices(self):
        """{name: [3,4] array} of the projection matrices the source has among P0 / P2 / P3: copies, in the floating dtype the source
        stores them in (the reference divides its float32 matrices in float32), float64 for anything that is not floating."""
        out = {}
        for name in _MATRICES:
            if name in ("P2", "P3") or hasattr(self.source, name):
                m = np.array(getattr(self.source, name)).reshape(3, 4)
                out[name] = m if np.issubdtype(m.dtype, np.floating) else m.astype(np.float64)
        return out

    def replaced(self, matrices):
        """-> a copy of these intrinsics over the same source with `matrices` ({name: [3,4]}) in place of its own."""
        return CameraIntrinsics(_Replaced(self.source, matrices))

    @property
    def cu(self):
        return self.P2[0, 2]

    @property
    def cv(self):
        return self.P2[1, 2]

    @property
    def fu(self):
        return self.P2[0, 0]

    @property
    def fv(self):
        return self.P2[1, 1]

    @property
    def tx(self):
        return self.P2[0, 3] / (-self.fu)

    @property
    def ty(self):
        return self.P2[1, 3] / (-self.fv)

    def img_to_rect(self, u, v, depth_rect):
        """NumPy form (kitti_utils.Calibration.img_to_rect): u, v, depth [N] -> [N,3]."""
        x = ((u - self.cu) * depth_rect) / self.fu + self.tx
        y = ((v - self.cv) * depth_rect) / self.fv + self.ty
        return np.concatenate((x.reshape(-1, 1), y.reshape(-1, 1), depth_rect.reshape(-1, 1)), axis=1)

    def depthmap_to_rect(self, depth_map):
        x_idxs, y_idxs = np.meshgrid(np.arange(0, depth_map.shape[1]), np.arange(0, depth_map.shape[0]), indexing="ij")
        x_idxs, y_idxs = x_idxs.reshape(-1), y_idxs.reshape(-1)
        depth = depth_map[y_idxs, x_idxs]
        return self.img_to_rect(x_idxs, y_idxs, depth), x_idxs, y_idxs


class Calib:
    def __init__(self, calibration, image_size):
        self.calib = calibration if isinstance(calibration, CameraIntrinsics) else CameraIntrinsics(calibration)
        self.size = tuple(image_size)

    @property
    def P2(self):
        return torch.tensor(self.calib.P2).float()

    @property
    def P3(self):
        return torch.tensor(self.calib.P3).float()

    @property
    def width(self):
        return self.size[0]

    @property
    def height(self):
        return self.size[1]

    @property
    def stereo_fuxbaseline(self):
        """fu * baseline = P2[0,3] - P3[0,3], taken in fp32 as the reference does (its P2 / P3 are float tensors)."""
        return float(np.float32(self.calib.P2[0, 3]) - np.float32(self.calib.P3[0, 3]))

    @property
    def fu(self):
        return self.P2[0, 0]

    @property
    def fv(self):
        return self.P2[1, 1]

    @property
    def cu(self):
        return self.P2[0, 2]

    @property
    def cv(self):
        return self.P2[1, 2]

    @property
    def tx(self):
        return self.P2[0, 3] / (-self.fu)

    @property
    def ty(self):
        return self.P2[1, 3] / (-self.fv)

    def __getitem__(self, item):
        return self

    def transpose(self, method):
        return self

    def resize(self, dst_size):
        """dst_size = (width, height) -> the calibration of the resampled image: row 0 of P0 / P2 / P3 / width * new width, row 1
        / height * new height, in that order and in the dtype the matrices are stored in (reference :59-76).  A negative size returns
        self with a warning, like the reference."""
        if len(dst_size) != 2:
            raise ValueError("dst_size is (width, height)")
        if any(a < 0 for a in dst_size):
            warnings.warn("dst size < 0, size will not change")
            return self
        width, height = dst_size
        mats = self.calib.stored_matrices()
        for m in mats.values():
            m[0] = m[0] / self.width * width
            m[1] = m[1] / self.height * height
        return Calib(self.calib.replaced(mats), (width, height))

    def crop(self, box):
        """box = (x1, y1, x2, y2) -> the calibration of the window: the principal point of P0 / P2 / P3 moves by (-x1, -y1), the size is
        the window's.  This is what reference :48-57 spells out; there the six assignments land on tensors that its P0 / P2 / P3
        properties build afresh, so only the size changes.  The shift is applied here."""
        x1, y1, x2, y2 = (v.item() if torch.is_tensor(v) else v for v in box)
        mats = self.calib.stored_matrices()
        for m in mats.values():
            m[0, 2] = m[0, 2] - x1
            m[1, 2] = m[1, 2] - y1
        return Calib(self.calib.replaced(mats), (x2 - x1, y2 - y1))

    def img_to_rect(self, u, v, depth_rect):
        """Image coordinates + depth -> rectified camera coordinates [N,3]."""
        if isinstance(u, torch.Tensor):
            c = self.calib
            x = ((u.float() - c.cu) * depth_rect) / c.fu + c.tx
            y = ((v.float() - c.cv) * depth_rect) / c.fv + c.ty
            return torch.cat((x.reshape(-1, 1), y.reshape(-1, 1), depth_rect.reshape(-1, 1)), dim=1)
        return self.calib.img_to_rect(u, v, depth_rect)

    def depthmap_to_rect(self, depth_map):
        """[H,W] depth -> ([H*W,3] points, x indices, y indices), x-major (meshgrid(x, y) with 'ij' indexing)."""
        if isinstance(depth_map, torch.Tensor):
            x_range = torch.arange(0, depth_map.shape[1], device=depth_map.device)
            y_range = torch.arange(0, depth_map.shape[0], device=depth_map.device)
            x_idxs, y_idxs = torch.meshgrid(x_range, y_range, indexing="ij")
            x_idxs, y_idxs = x_idxs.reshape(-1), y_idxs.reshape(-1)
            depth = depth_map[y_idxs, x_idxs]
            return self.img_to_rect(x_idxs, y_idxs, depth), x_idxs, y_idxs
        return self.calib.depthmap_to_rect(depth_map)
