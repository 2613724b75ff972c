"""The algebra under the cost-volume layer's kernel (csrc/s16_cvrows.h), on the CPU in fp64.

dres0[0] is convbn_3d 64 -> 32 k3 s1 p1 on the concat cost volume (reference stackhourglass.py:115-130).  The volume's left half is one 2D map
masked per plane, its right half one 2D map moved by one column per plane, and the layer is linear, so with s_j = lo4 + j and L~, R~ zero outside
the map

    A[kd][kw](y, v) = sum_{kh,c} w[o, c,      kd, kh, kw] L~[c, y+kh-1, v]
    B[kd][kw](y, v) = sum_{kh,c} w[o, 32 + c, kd, kh, kw] R~[c, y+kh-1, v]
    pre(o, j, y, x) = sum_{kd: 0 <= j+kd-1 < D} sum_{kw} [0 <= x+kw-1 < W] [0 <= x-s_j+kw-kd < W] (A[kd][kw](y, x+kw-1) + B[kd][kw](y, x-s_j+kw-kd))

equals F.conv3d of the materialised volume: 18 vertical 3 x 1 convolutions per image row instead of a 3D convolution per plane.  The depth
edges, the x edges, the band around the mask edge and fully masked planes all come out of the two predicates.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_s16 import _ref_costvol

CASES = [(0, 12, 28, 28), (-12, 24, 10, 56), (-6, 12, 28, 28), (-5, 12, 28, 28), (2, 8, 12, 40), (-1, 4, 6, 64), (0, 1, 2, 16), (-12, 6, 5, 28),
         (9, 6, 5, 28)]


def rows_identity(L, R, w, lo4, D):
    """pre-activation [N, O, D, H, W] by the identity above (any float dtype)."""
    N, Cc, H, W = L.shape
    Oc = w.shape[0]
    # the 18 maps: a (3, 1) convolution per (side, kd, kw), vertical zero padding only
    A = [[F.conv2d(L, w[:, :Cc, kd, :, kw].unsqueeze(-1), padding=(1, 0)) for kw in range(3)] for kd in range(3)]
    B = [[F.conv2d(R, w[:, Cc:, kd, :, kw].unsqueeze(-1), padding=(1, 0)) for kw in range(3)] for kd in range(3)]
    x = torch.arange(W)
    out = torch.zeros(N, Oc, D, H, W, dtype=L.dtype)
    for j in range(D):
        s = lo4 + j
        for kd in range(3):
            if not 0 <= j + kd - 1 < D:
                continue
            for kw in range(3):
                ca, cb = x + kw - 1, x - s + kw - kd
                ok = (ca >= 0) & (ca < W) & (cb >= 0) & (cb < W)
                xs = x[ok]
                out[:, :, j, :, xs] += A[kd][kw][:, :, :, ca[ok]] + B[kd][kw][:, :, :, cb[ok]]
    return out


@pytest.mark.parametrize("lo4,D,H,W", CASES)
def test_row_maps_identity_equals_conv3d_of_the_volume_fp64(lo4, D, H, W):
    g = torch.Generator().manual_seed(1000 + 7 * D + W + lo4)
    L = torch.randn(2, 32, H, W, generator=g, dtype=torch.float64)
    R = torch.randn(2, 32, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(32, 64, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv3d(_ref_costvol(L, R, lo4, D), w, padding=1)
    got = rows_identity(L, R, w, lo4, D)
    m = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"lo4={lo4} D={D} {H}x{W}: max|err| {err:.3e} at max|ref| {m:.1f}")
    # fp64 re-association of 27 x 64 products of N(0,1) values: a few hundred ulps of the largest value at most
    assert err <= 1e-11 * max(m, 1.0)


def test_fully_masked_planes_are_zero_before_the_epilogue():
    """|s_j| >= W: no pixel of the plane has a partner, the volume's plane is zero -- and a plane next to it still sees it through kd."""
    g = torch.Generator().manual_seed(5)
    L = torch.randn(1, 32, 4, 16, generator=g, dtype=torch.float64)
    R = torch.randn(1, 32, 4, 16, generator=g, dtype=torch.float64)
    w = torch.randn(32, 64, 3, 3, 3, generator=g, dtype=torch.float64)
    lo4, D = -18, 6                     # s_j = -18 .. -13: planes 0..2 fully masked, plane 1's neighbours too
    got = rows_identity(L, R, w, lo4, D)
    ref = F.conv3d(_ref_costvol(L, R, lo4, D), w, padding=1)
    assert (got - ref).abs().max().item() <= 1e-11 * max(ref.abs().max().item(), 1.0)
    assert not got[:, :, 0].any() and not got[:, :, 1].any() and got[:, :, 3].any()
