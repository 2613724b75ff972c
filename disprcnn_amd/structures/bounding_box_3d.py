"""Box3DList: a set of 3D boxes in the rectified camera frame (reference: disprcnn/structures/bounding_box_3d.py).

Modes, as the reference's:
    'xyzhwl_ry'  (N,7)  x, y, z of the bottom-face centre, h, w, l, rotation about y
    'ry_lhwxyz'  (N,7)  the same values in the order ry, l, h, w, x, y, z
    'corners'    (N,24) eight corners x, y, z each, in the reference's order (0-3: z = +w/2 side, 4-7: z = -w/2 side)
Every conversion between two different modes goes through the corners, as the reference's does, so 'xyzhwl_ry' -> 'ry_lhwxyz' is not a
permutation: the sizes come back as corner distances and the angle as -atan2(dz, dx) of the edge 0 -> 3 (a zero-size box has angle 0).
Values are kept in fp32.  The 'alpha_lhwxyz' mode, the velodyne frame, flips and the projection helpers of the reference are not built.
"""
import torch

_MODES = ("ry_lhwxyz", "xyzhwl_ry", "corners")


class Box3DList(object):
    def __init__(self, bbox_3d, size, mode="corners", frame="rect"):
        if frame != "rect":
            raise NotImplementedError(f"Box3DList: frame {frame!r} is not built, only the rectified camera frame")
        if mode not in _MODES:
            raise ValueError("mode should be 'ry_lhwxyz', 'xyzhwl_ry' or 'corners'")
        device = bbox_3d.device if isinstance(bbox_3d, torch.Tensor) else torch.device("cpu")
        bbox_3d = torch.as_tensor(bbox_3d, dtype=torch.float32, device=device)
        if bbox_3d.ndimension() == 1:
            bbox_3d = bbox_3d.unsqueeze(0)
        if bbox_3d.ndimension() == 3:
            bbox_3d = bbox_3d.reshape(-1, 24)
        if bbox_3d.ndimension() != 2 and bbox_3d.numel() != 0:
            raise ValueError("bbox_3d should have 2 dimensions, got {} {}".format(bbox_3d.ndimension(), bbox_3d.size()))
        width = 24 if mode == "corners" else 7
        if bbox_3d.size(-1) != width:
            if bbox_3d.numel() != 0:
                raise ValueError("last dimension of bbox_3d in the {} mode should have a size of {}, got {}".format(mode, width,
                                                                                                                   bbox_3d.size(-1)))
            bbox_3d = torch.empty((0, width), dtype=torch.float32, device=device)
        self.device = device
        self.frame = frame
        self.bbox_3d = bbox_3d
        self.size = (int(size[0]), int(size[1]))        # (image_width, image_height)
        self.mode = mode

    def __getitem__(self, item):
        return Box3DList(self.bbox_3d[item], self.size, self.mode)

    def __len__(self):
        return self.bbox_3d.shape[0]

    def to(self, device):
        return Box3DList(self.bbox_3d.to(device), self.size, self.mode)

    def _split_into_corners(self):
        """-> 8 tensors (N,3)"""
        if self.mode == "corners":
            return self.bbox_3d.split(3, dim=-1)
        if self.mode == "xyzhwl_ry":
            x, y, z, h, w, l, ry = self.bbox_3d.split(1, dim=-1)
        else:
            ry, l, h, w, x, y, z = self.bbox_3d.split(1, dim=-1)
        zero_col, ones_col = torch.zeros_like(ry), torch.ones_like(ry)
        x_corners = torch.cat((-l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2), dim=1)
        y_corners = torch.cat((zero_col, -h, -h, zero_col, zero_col, -h, -h, zero_col), dim=1)
        z_corners = torch.cat((w / 2, w / 2, w / 2, w / 2, -w / 2, -w / 2, -w / 2, -w / 2), dim=1)
        corners_obj = torch.stack((x_corners, y_corners, z_corners), dim=1)                     # (N,3,8)
        R = torch.cat([torch.cos(ry), zero_col, torch.sin(ry), zero_col, ones_col, zero_col, -torch.sin(ry), zero_col, torch.cos(ry)],
                      dim=1).view(-1, 3, 3)
        corners_cam = torch.matmul(R, corners_obj) + torch.cat((x, y, z), dim=-1).view(-1, 3, 1)
        return corners_cam.transpose(1, 2).reshape(-1, 24).split(3, dim=-1)

    def convert(self, mode):
        if mode not in _MODES:
            raise ValueError("mode should be 'ry_lhwxyz', 'xyzhwl_ry' or 'corners'")
        if mode == self.mode:
            return self
        corners = self._split_into_corners()
        if mode == "corners":
            return Box3DList(torch.cat(corners, dim=-1), self.size, mode=mode)
        dif = corners[3] - corners[0]
        ry = -(torch.atan2(dif[:, 2], dif[:, 0])).view(-1, 1)
        xyz = ((corners[7] + corners[0]) / 2).view(-1, 3)
        l = torch.norm(corners[0] - corners[3], dim=1).view(-1, 1)
        h = torch.norm(corners[0] - corners[1], dim=1).view(-1, 1)
        w = torch.norm(corners[0] - corners[4], dim=1).view(-1, 1)
        bbox_3d = torch.cat((xyz, h, w, l, ry), dim=-1) if mode == "xyzhwl_ry" else torch.cat((ry, l, h, w, xyz), dim=-1)
        return Box3DList(bbox_3d, self.size, mode=mode)

    def enlarge_box3d(self, extra_width):
        """The boxes grown by extra_width on every side (h, w, l + 2 extra_width, the bottom centre moved down by extra_width), in this
        list's mode; through 'xyzhwl_ry' and back, as the reference's."""
        large_boxes3d = self.convert("xyzhwl_ry").bbox_3d.clone()
        large_boxes3d[:, 3:6] += extra_width * 2
        large_boxes3d[:, 1] += extra_width
        return Box3DList(large_boxes3d, self.size, mode="xyzhwl_ry").convert(self.mode)

    def __repr__(self):
        return "{}(num_boxes_3d={}, image_width={}, image_height={}, mode={})".format(self.__class__.__name__, len(self), self.size[0],
                                                                                      self.size[1], self.mode)
