"""Calib: the per-image camera calibration the 3D stage reads (reference: disprcnn/structures/calib.py:10-122 over
utils/kitti_utils.py:Calibration).

`Calib(calibration, image_size)` takes any object with 3x4 `P2` / `P3` projection matrices -- the reference's
`kitti_utils.Calibration`, or a plain namespace.  `.calib` exposes the intrinsics the reference reads off it (`fu, fv, cu, cv, tx,
ty`, float64 as NumPy computes them) and forwards any other attribute to the wrapped object.  `img_to_rect` / `depthmap_to_rect` on
torch tensors have the reference's arithmetic: fp32 tensors with the intrinsics as scalars, points in the x-major order of
meshgrid(x, y).
"""
import numpy as np
import torch


class CameraIntrinsics:
    """fu, fv, cu, cv, tx, ty of the left colour camera from P2 (kitti_utils.py:28-49); other attributes come from `source`."""

    def __init__(self, source):
        self.source = source
        self.P2 = np.asarray(source.P2, dtype=np.float64).reshape(3, 4)
        self.P3 = np.asarray(source.P3, dtype=np.float64).reshape(3, 4)

    def __getattr__(self, name):
        if name == "source":
            raise AttributeError(name)
        return getattr(self.source, name)

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
