"""tests/disp_tail_oracle.py pinned on the CPU: its fp64 functions against the maps recorded from the reference (tests/golden/post_golden.npz,
the resize entries of structures_golden.npz) and against oracle/post_oracle.py in fp32, each within the rule the GPU tests apply
(err <= 2 * e32 + 1e-6 * max|ref|, e32 from the oracle's own fp32 evaluation); F.interpolate in fp64 against the written-out bilinear rule."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from disprcnn_amd.utils import synth
from oracle import post_oracle as P
from tests import disp_tail_oracle as T

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "post_golden.npz"))
GS = np.load(os.path.join(GOLD, "structures_golden.npz"))
_spec = importlib.util.spec_from_file_location("disp_tail_structures_cases", os.path.join(GOLD, "_structures_cases.py"))
_cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cases)
POST = sorted({k.split(":")[0] for k in G.files})
H, W, S = 96, 320, 224


def _within(name, other, ref64, ref32):
    bound, e32 = T.e32_bound(ref64, ref32)
    err = (other.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{name}: err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}")
    assert tuple(other.shape) == tuple(ref64.shape)
    assert err <= bound, (name, err, bound)


def _post_case(name):
    lb, rb = torch.from_numpy(G[f"{name}:left"]).reshape(-1, 4), torch.from_numpy(G[f"{name}:right"]).reshape(-1, 4)
    return lb, rb, synth.hash_uniform(f"post:{name}", (len(lb), S, S), -48.0, 48.0)


@pytest.mark.parametrize("name", POST)
def test_disparity_map_reproduces_the_recorded_maps(name):
    lb, rb, disp = _post_case(name)
    ref64 = T.disparity_map(lb, rb, disp, H, W)
    assert ref64.dtype == torch.float64
    _within(name, torch.from_numpy(G[f"{name}:map"]), ref64, T.disparity_map(lb, rb, disp, H, W, dtype=torch.float32))


@pytest.mark.parametrize("name", [n for n in POST if len(G[f"{n}:left"].reshape(-1, 4))])
@pytest.mark.parametrize("clamp0,with_masks", [(False, False), (True, True)])
def test_disparity_map_and_depth_agree_with_post_oracle_fp32(name, clamp0, with_masks):
    lb, rb, disp = _post_case(name)
    masks = (synth.hash_uniform(f"tail:mask:{name}", (len(lb), H, W), 0.0, 1.0) > 0.3).float() if with_masks else None
    ref64 = T.disparity_map(lb, rb, disp, H, W, clamp0, masks)
    _within(f"{name} map", P.disparity_map(lb, rb, disp, H, W, clamp0, masks), ref64,
            T.disparity_map(lb, rb, disp, H, W, clamp0, masks, dtype=torch.float32))
    if with_masks:
        return
    pos = disp.abs() + 8.0                                         # depth: away from the pole at disparity 0
    rb0 = torch.stack([torch.minimum(rb[:, 0], lb[:, 0]), rb[:, 1], rb[:, 2], rb[:, 3]], 1)
    d64, dd = T.roi_depth_maps(lb, rb0, pos, H, W, 389.34, return_disparity=True)
    assert dd[~dd.isnan()].min().item() >= 1.0
    _within(f"{name} depth", P.roi_depth_maps(lb, rb0, pos, H, W, 389.34), d64, T.roi_depth_maps(lb, rb0, pos, H, W, 389.34, dtype=torch.float32))
    assert (d64 == 0).eq(P.roi_depth_maps(lb, rb0, pos, H, W, 389.34) == 0).all() and (d64 == 0).eq(dd.isnan()).all()


@pytest.mark.parametrize("name,hw,dst", _cases.RESIZE)
def test_disparity_resize_reproduces_the_recorded_maps(name, hw, dst):
    d = synth.hash_uniform(f"structures:resize:{name}", hw, -48.0, 48.0)
    for mode, key in ((False, "bilinear"), (True, "maxpool")):
        ref64 = T.disparity_resize(d, dst[0], dst[1], mode)
        assert ref64.dtype == torch.float64 and tuple(ref64.shape) == (dst[1], dst[0])
        _within(f"{name} {key}", torch.from_numpy(GS[f"resize:{name}:{key}"]), ref64, T.disparity_resize(d, dst[0], dst[1], mode, dtype=torch.float32))


@pytest.mark.parametrize("ih,iw,oh,ow", [(56, 56, 150, 200), (37, 53, 10, 7), (1, 17, 5, 9), (8, 1, 3, 4), (5, 5, 5, 5), (9, 9, 1, 1)])
def test_interpolate_fp64_is_the_written_out_rule(ih, iw, oh, ow):
    d = synth.hash_uniform(f"tail:interp:{ih}x{iw}", (ih, iw), -48.0, 48.0).double()
    a = F.interpolate(d[None, None], (oh, ow), mode="bilinear", align_corners=True)[0, 0]
    b = T.bilinear_align_corners(d, oh, ow)
    assert (a - b).abs().max().item() <= 1e-12 * 48.0


def test_softargmin_is_fp64_and_hits_a_one_hot_column():
    """A column whose cost peaks by 1e4 at one coarse slice puts all the mass on the fine disparity that lands on it."""
    cost = torch.zeros(1, 5, 2, 2)
    cost[:, 3] = 1e4
    out = T.upsample_softargmin(cost, 7 + 9, 7, 2, 2)          # D = 9 = 2 * (5 - 1) + 1: fine sample 6 is coarse slice 3
    assert out.dtype == torch.float64 and torch.equal(out, torch.full((1, 2, 2), 13.0, dtype=torch.float64))
    assert T.upsample_softargmin(cost[:, None], 16, 7, 2, 2).equal(out)
