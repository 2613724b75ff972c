"""Host only, fp64: the rows layout of the fused cout-1 heads is the same sum as the 12-float layout (csrc/convs16.hip HEAD form,
include/disprcnn_hip.h `drc_s16conv_params.head_rows`, drc_head_gather_rows_fwd).

From random pointwise products P[27][D][H][W] (tap t = kd*9 + kh*3 + kw; out[o] = sum_t P[t][o + off(t)], zero outside the volume):
  slots   S[j = kh*3+kw] of a SOURCE voxel = sum_kd P[kd, j] on the plane z + kd - 1     + the nine-term gather of drc_head_gather_fwd,
  rows    (T0, T1a, T1b, T2) of a source row and OUTPUT column, built the way the kernel does -- per 64-lane wave, five values per lane,
          one-lane whole-wave shifts with the idle lanes 28..31 of each half zeroed first   + the three-row gather,
and both equal conv3d of the taps.  The lane emulation puts NaN into the idle lanes: the zeroing is what keeps lane 31 out of column 0 of
the second half and lane 28 out of column 27."""
import numpy as np
import pytest

W = 28


def _taps(D, H, seed):
    return np.random.default_rng(seed).standard_normal((27, D, H, W))


def _conv(P):
    """out[z, y, x] = sum_t P[t][z + kd - 1, y + kh - 1, x + kw - 1]"""
    _, D, H, _ = P.shape
    Pp = np.pad(P, ((0, 0), (1, 1), (1, 1), (1, 1)))
    out = np.zeros((D, H, W))
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                out += Pp[kd * 9 + kh * 3 + kw, kd:kd + D, kh:kh + H, kw:kw + W]
    return out


def _slots(P):
    """S[j][z, y, x] (output plane z, source row y, source column x)"""
    _, D, H, _ = P.shape
    Pp = np.pad(P, ((0, 0), (1, 1), (0, 0), (0, 0)))
    return np.stack([sum(Pp[kd * 9 + j, kd:kd + D] for kd in range(3)) for j in range(9)])


def _gather9(S):
    _, D, H, _ = S.shape
    Sp = np.pad(S, ((0, 0), (0, 0), (1, 1), (1, 1)))
    return sum(Sp[kh * 3 + kw, :, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3))


def _wave_rows(S_row):
    """One wave = one row of 28 voxels.  S_row: [9][28].  Lane l: column l & 31, half g = l >> 5; half 0 holds j = 0..4, half 1 j = 5..8 (its
    fifth value is the unused MFMA row).  Returns (T0, T1a, T1b, T2) [4][28] as the two halves store them."""
    o = np.full((5, 64), np.nan)
    o[:, 0:28] = S_row[0:5]
    o[:4, 32:60] = S_row[5:9]
    o[4, 32:60] = 0.0
    live = (np.arange(64) & 31) < 28
    v = np.where(live, o, 0.0)
    left = lambda a: np.concatenate([[0.0], a[:-1]])          # lane i reads lane i - 1 (x - 1); lane 0 reads zero
    right = lambda a: np.concatenate([a[1:], [0.0]])          # lane i reads lane i + 1 (x + 1); lane 63 reads zero
    a0 = (left(v[0]) + v[1]) + right(v[2])
    a1 = left(v[3]) + v[4]
    b0 = right(v[0])
    b1 = (left(v[1]) + v[2]) + right(v[3])
    return np.stack([a0[0:28], a1[0:28], b0[32:60], b1[32:60]])


def _rows(S):
    _, D, H, _ = S.shape
    T = np.empty((4, D, H, W))
    for z in range(D):
        for y in range(H):
            T[:, z, y] = _wave_rows(S[:, z, y])
    return T


def _gather_rows(T):
    _, D, H, _ = T.shape
    out = np.zeros((D, H, W))
    for y in range(H):
        s = T[1][:, y] + T[2][:, y]
        if y - 1 >= 0:
            s = T[0][:, y - 1] + s
        if y + 1 < H:
            s = s + T[3][:, y + 1]
        out[:, y] = s
    return out


@pytest.mark.parametrize("D,H", [(6, 28), (3, 5), (2, 1), (1, 2)])
def test_rows_layout_equals_slot_layout_equals_conv(D, H):
    P = _taps(D, H, 100 * D + H)
    ref = _conv(P)
    S = _slots(P)
    nine = _gather9(S)
    T = _rows(S)
    assert np.isfinite(T).all()
    rows = _gather_rows(T)
    tol = 1e-12 * np.abs(ref).max()
    assert np.abs(nine - ref).max() <= tol
    assert np.abs(rows - ref).max() <= tol
    for sl in (np.s_[:, :, 0], np.s_[:, :, W - 1], np.s_[:, 0, :], np.s_[:, H - 1, :]):       # x = 0, x = 27, y = 0, y = H - 1
        assert np.abs(rows[sl] - ref[sl]).max() <= tol and np.abs(rows[sl] - nine[sl]).max() <= tol


def test_edge_columns_take_no_tap_from_outside_the_row():
    """x = 0 has no kw = 0 source, x = 27 no kw = 2 source: with a single non-zero source column the row sums say exactly which outputs it feeds."""
    S = np.zeros((9, 1, 1, W))
    S[:, 0, 0, 0] = np.arange(1.0, 10.0)                 # source column 0: tap kw feeds output column 1 - kw
    T = _rows(S)[:, 0, 0]
    assert T[0, 0] == 2.0 and T[0, 1] == 1.0 and T[1, 0] == 5.0 and T[1, 1] == 4.0 and T[2, 0] == 0.0 and T[2, 1] == 0.0
    assert T[3, 0] == 8.0 and T[3, 1] == 7.0 and not T[:, 2:].any()
    S = np.zeros((9, 1, 1, W))
    S[:, 0, 0, W - 1] = np.arange(1.0, 10.0)             # source column 27 feeds outputs 26 (kw = 2) and 27 (kw = 1)
    T = _rows(S)[:, 0, 0]
    assert T[0, 27] == 2.0 and T[0, 26] == 3.0 and T[1, 27] == 5.0 and T[2, 26] == 6.0 and T[2, 27] == 0.0
    assert T[3, 27] == 8.0 and T[3, 26] == 9.0 and not T[:, :26].any()
