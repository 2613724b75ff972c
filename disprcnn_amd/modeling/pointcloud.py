"""InstancePointCloud: per-ROI disparity maps -> the instance point clouds PointRCNN's RPN consumes
(reference: pointnet_module/point_rcnn/lib/net/point_rcnn.py:189-241 process_input_eval, :37-83 back_project with fix_seed=True,
called from _forward_val with a 0.5 mask threshold, :286-294).

Per ROI: the disparity resampled to the integer box (+ x1 - x1p), depth = fuxb / (disp + 1e-6) clamped at 1 inside the box, the Masker
paste of the mask probabilities (padding 1, threshold 0.5) applied only when it meets the box, img_to_rect, points with z > 0 in
x-major order, a draw of exactly `npoints` of them, z clamped at `max_depth`, a rotation about y by atan2(box centre x - W/2, fu)
(W: the first image's width, as the reference) and the per-ROI mean subtracted.

Device work is two HIP kernels (libdisprcnn_pts.so): A compacts the kept pixels of every ROI of every image in one launch, B gathers,
rotates and centres the drawn points.  The host reads the per-ROI counts once -- the call's only sync -- to build the draw.

The draw.  The reference reseeds NumPy's global legacy generator to 0 before each choice and each shuffle, so the chosen indices
depend only on the count n and npoints.  Here a private ``np.random.RandomState(0)`` per ROI gives the same stream and leaves NumPy's
global state alone (the reference leaves it reseeded to 0); the arrays are cached by n.

The training form (``InstancePointCloud.train_clouds``; reference :97-187 process_input with back_project's fix_seed=False): the mask
threshold is the caller's (MODEL.POINTRCNN.MASK_THRESH), depth has no lower clamp (a pixel of negative depth falls to the z > 0
filter), the draw is not reseeded but reads a generator `rng` -- NumPy's global legacy generator by default, as the reference, or any
``RandomState`` -- with the reference's calls in the reference's order (``draw_choice_train`` per ROI, then ``draw_augmentation``), and
kernel B applies the augmentation in the reference's order: z clamped at `max_depth`, times `scale`, x negated when flipped, the
rotation by the angle negated when flipped, the mean subtracted.  The returned `rot_angle` is the signed angle that was used.  The
counts still come to the host in the call's one read; a caller may append int64 slots to that buffer and fill them on the device before
the read (PointRCNN puts the 2D matcher's indices there).
"""
import numpy as np
import torch

from .. import engine as E
from ..ops import integer_roi_boxes
from ..pts import _lib
from ..structures.calib import Calib


def draw_choice(n, npoints):
    """back_project's fix_seed draw (point_rcnn.py:52-70) for n kept points: int64 [npoints] indices into them."""
    if n <= 0:
        raise ValueError("draw_choice needs n >= 1")
    rs = np.random.RandomState(0)
    if n > npoints:
        choice = rs.choice(n, npoints, replace=False)
    else:
        choice = rs.choice(n, npoints - n, replace=True)
        choice = np.concatenate((np.arange(n), choice))
    np.random.RandomState(0).shuffle(choice)
    return choice


def draw_choice_train(n, npoints, rng=None):
    """back_project's draw without fix_seed (point_rcnn.py:59-73) for n kept points, read from `rng` (default: the numpy.random module,
    as the reference): choice, then shuffle.  int64 [npoints] indices."""
    if n <= 0:
        raise ValueError("draw_choice_train needs n >= 1")
    rng = np.random if rng is None else rng
    if n > npoints:
        choice = rng.choice(n, npoints, replace=False)
    else:
        choice = rng.choice(n, npoints - n, replace=True)
        choice = np.concatenate((np.arange(n), choice))
    rng.shuffle(choice)
    return choice


def draw_augmentation(rng=None):
    """process_input's draws after the clouds (point_rcnn.py:145-154): uniform(0.95, 1.05) for the scale, then random() < 0.5 for the
    flip -> (scale, flip)."""
    rng = np.random if rng is None else rng
    scale = float(rng.uniform(0.95, 1.05))
    flip = bool(rng.random() < 0.5)
    return scale, flip


class InstancePointCloud:
    def __init__(self, npoints=768, mask_threshold=0.5, mask_padding=1, max_depth=160.0):
        self.npoints = int(npoints)
        self.mask_threshold = float(mask_threshold)
        self.mask_padding = int(mask_padding)
        self.max_depth = float(max_depth)
        self._choices = {}
        self._ws = {}
        self.last_counts = None
        self.last_src_pix = None

    def choice(self, n):
        """The cached draw for n kept points, int32 [npoints]."""
        c = self._choices.get(n)
        if c is None:
            c = draw_choice(n, self.npoints).astype(np.int32)
            self._choices[n] = c
        return c

    def _workspace(self, dev, need):
        ws = self._ws.get(dev)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(need, 1 << 20, 0 if ws is None else 2 * ws.numel()), dtype=torch.int32, device=dev)
            self._ws[dev] = ws
        return ws

    def __call__(self, left_result, right_result, calibs):
        """left_result / right_result: per-image BoxLists (left ones carry 'disparity' [R,S,S] and 'mask' [R,1,M,M]); calibs: one Calib
        (or P2/P3 calibration object) per image.  Returns pts [R,npoints,3] (centred), pts_mean [R,3], rot_angle [R] (float64)."""
        return self._run(left_result, right_result, calibs, None)[:3]

    def train_clouds(self, left_result, right_result, calibs, rng=None, augment=True, tail=0, fill_tail=None):
        """The training form (see the module's docstring).  rng: numpy.random (default) or a RandomState; augment: draw a scale and a flip
        after the clouds (False with RPN.FIXED: scale 1, no flip, no draw).  tail / fill_tail: `tail` int64 slots appended to the buffer
        the counts are read through; fill_tail(view) is called once, before the read, to fill them on the device.
        Returns pts [R,npoints,3], pts_mean [R,3], rot_angle [R] (float64, signed), scale, flip, the tail as a CPU int64 tensor."""
        return self._run(left_result, right_result, calibs, dict(rng=rng, augment=augment, tail=int(tail), fill_tail=fill_tail))

    def _run(self, left_result, right_result, calibs, train):
        counts = [len(lr) for lr in left_result]
        R = sum(counts)
        if len(right_result) != len(left_result) or len(calibs) < len(left_result):
            raise ValueError("InstancePointCloud needs one right BoxList and one calibration per image")
        dev = left_result[0].bbox.device if left_result else torch.device("cuda")
        if R == 0:
            return (torch.empty(0, self.npoints, 3, device=dev), torch.empty(0, 3, device=dev),
                    torch.empty(0, dtype=torch.float64, device=dev), 1.0, False, torch.empty(0, dtype=torch.int64))
        if not dev.type == "cuda":
            raise RuntimeError("InstancePointCloud: expected CUDA/HIP boxes on an MI355X; the HIP path has no CPU fallback")
        parts = [i for i, c in enumerate(counts) if c]
        lb = torch.cat([left_result[i].bbox for i in parts]).to(dev).float().contiguous()
        rb = torch.cat([right_result[i].bbox for i in parts]).to(dev).float().contiguous()
        disp = torch.cat([left_result[i].get_field("disparity") for i in parts]).to(dev).float().contiguous()
        mask = torch.cat([left_result[i].get_field("mask") for i in parts]).to(dev).float()
        E.require_gpu(disp, "InstancePointCloud disparity")
        if disp.dim() != 3 or disp.shape[0] != R or disp.shape[1] != disp.shape[2]:
            raise ValueError("'disparity' must be [R,S,S]")
        if mask.dim() == 4:
            mask = mask[:, 0]
        mask = mask.contiguous()
        if mask.dim() != 3 or mask.shape[0] != R or mask.shape[1] != mask.shape[2]:
            raise ValueError("'mask' must be [R,1,M,M]")
        S, M = disp.shape[1], mask.shape[1]

        # host constants of every ROI in one pinned buffer, uploaded in one asynchronous copy:
        #   int32 [R,2] (H, W) | fp32 [R,8] (fu, fv, cu, cv, tx, ty, fuxb, W0/2) | fp64 [R] fu
        half_w0 = left_result[0].size[0] / 2
        hw = np.zeros((R, 2), np.int32)
        cam = np.zeros((R, 8), np.float32)
        fu64 = np.zeros(R, np.float64)
        r = 0
        for i in parts:
            c = calibs[i] if isinstance(calibs[i], Calib) else Calib(calibs[i], left_result[i].size)
            k = c.calib
            w, h = left_result[i].size
            n = counts[i]
            hw[r:r + n] = (h, w)
            cam[r:r + n] = (k.fu, k.fv, k.cu, k.cv, k.tx, k.ty, c.stereo_fuxbaseline, half_w0)
            fu64[r:r + n] = k.fu
            r += n
        raw = np.concatenate([fu64.view(np.uint8), cam.reshape(-1).view(np.uint8), hw.reshape(-1).view(np.uint8)])
        up = torch.from_numpy(raw).pin_memory().to(dev, non_blocking=True)
        roi_d = up[:8 * R].view(torch.float64)
        cam_d = up[8 * R:40 * R].view(torch.float32).view(R, 8)
        hw_d = up[40 * R:48 * R].view(torch.int32).view(R, 2)
        roi_i = torch.cat([integer_roi_boxes(lb, rb), hw_d], dim=1).contiguous()
        roi_f = torch.cat([lb, cam_d], dim=1).contiguous()

        tail = train["tail"] if train else 0
        info = torch.empty(2 * R + 1 + tail, dtype=torch.int64, device=dev)
        if tail:
            train["fill_tail"](info[2 * R + 1:])
        stream = E._stream_ptr(dev)
        ws = self._workspace(dev, 0)
        L = _lib.lib()
        kernel_a, name_a = (L.drc_instance_points_train_fwd, "drc_instance_points_train_fwd") if train else \
            (L.drc_instance_points_fwd, "drc_instance_points_fwd")
        for _ in range(2):                      # a second pass only when the boxes outgrow the cached workspace
            st = kernel_a(E._ptr(disp), S, E._ptr(roi_i), E._ptr(roi_f), E._ptr(mask), M, self.mask_padding,
                          self.mask_threshold, R, E._ptr(info), E._ptr(ws), ws.numel(), stream)
            _lib.check(st, name_a)
            info_h = info.cpu()
            if int(info_h[2 * R]) <= ws.numel():
                break
            ws = self._workspace(dev, int(info_h[2 * R]))
        n_kept = info_h[:R].tolist()
        self.last_counts = n_kept
        if min(n_kept) == 0:
            raise EOFError("mask is nonvalid")

        scale, flip = 1.0, False
        if train:
            rng = train["rng"]
            choice = np.stack([draw_choice_train(n, self.npoints, rng).astype(np.int32) for n in n_kept])
            if train["augment"]:
                scale, flip = draw_augmentation(rng)
        else:
            choice = np.stack([self.choice(n) for n in n_kept])
        choice = torch.from_numpy(choice).pin_memory().to(dev, non_blocking=True)
        pts = torch.empty(R, self.npoints, 3, dtype=torch.float32, device=dev)
        mean = torch.empty(R, 3, dtype=torch.float32, device=dev)
        rot = torch.empty(R, dtype=torch.float64, device=dev)
        src = torch.empty(R, self.npoints, dtype=torch.int32, device=dev)
        if train:
            st = L.drc_instance_points_gather_train_fwd(E._ptr(disp), S, E._ptr(roi_i), E._ptr(roi_f), E._ptr(roi_d), R, E._ptr(info),
                                                        E._ptr(ws), E._ptr(choice), self.npoints, self.max_depth, scale, int(flip),
                                                        E._ptr(pts), E._ptr(mean), E._ptr(rot), E._ptr(src), stream)
            _lib.check(st, "drc_instance_points_gather_train_fwd")
        else:
            st = L.drc_instance_points_gather_fwd(E._ptr(disp), S, E._ptr(roi_i), E._ptr(roi_f), E._ptr(roi_d), R, E._ptr(info), E._ptr(ws),
                                                  E._ptr(choice), self.npoints, self.max_depth, E._ptr(pts), E._ptr(mean), E._ptr(rot),
                                                  E._ptr(src), stream)
            _lib.check(st, "drc_instance_points_gather_fwd")
        self.last_src_pix = src
        return pts, mean, rot, scale, flip, info_h[2 * R + 1:].clone()

    @staticmethod
    def rotate_back(pts, rot_angle):
        """Inverse of the rotation about y (rotate_pc_along_y.rotate_back, utils_3d.py:106-114): pts [R,N,3] -> [R,N,3]."""
        a = -rot_angle
        cosval, sinval = torch.cos(a).unsqueeze(1), torch.sin(a).unsqueeze(1)
        rotmat = torch.cat([cosval, -sinval, sinval, cosval], dim=1).view(-1, 2, 2)
        out = pts.clone()
        out[:, :, [0, 2]] = torch.bmm(pts[:, :, [0, 2]], torch.transpose(rotmat, 1, 2).float())
        return out
