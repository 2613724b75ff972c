"""CPU checks of the 3D stage's host side: the point-cloud draw, Calib, and the PointNet++ oracle on hand-computed cases."""
import os

import numpy as np
import pytest

from tests import pn2_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "points_ref_golden.npz")


def _reference_draw(n, npoints):
    """back_project's fix_seed draw through NumPy's global generator, as the reference makes it (point_rcnn.py:52-70)."""
    np.random.seed(0)
    if n > npoints:
        choice = np.random.choice(n, npoints, replace=False)
    else:
        choice = np.concatenate((np.arange(n), np.random.choice(n, npoints - n, replace=True)))
    np.random.seed(0)
    np.random.shuffle(choice)
    return choice


@pytest.mark.parametrize("n", [1, 600, 767, 768, 769, 5000])
def test_cached_draw_equals_the_reference_sequence(n):
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    state = np.random.get_state()
    ref = _reference_draw(n, 768)
    np.random.set_state(state)
    ipc = InstancePointCloud()
    got = ipc.choice(n)
    assert got.dtype == np.int32 and got.shape == (768,)
    assert np.array_equal(got, ref)
    assert ipc.choice(n) is got                       # cached by n


def test_draw_leaves_numpy_global_state_alone():
    from disprcnn_amd.modeling.pointcloud import InstancePointCloud
    np.random.seed(1234)
    before = np.random.get_state()
    InstancePointCloud().choice(5000)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_calib_matches_the_golden():
    import torch
    from types import SimpleNamespace
    import disprcnn.structures.calib as alias
    from disprcnn_amd.structures.calib import Calib
    assert alias.Calib is Calib
    g = np.load(GOLDEN)
    c = Calib(SimpleNamespace(P2=g["P2"], P3=g["P3"]), (int(g["W"]), int(g["H"])))
    P2 = g["P2"]
    assert c.calib.fu == P2[0, 0] and c.calib.fv == P2[1, 1] and c.calib.cu == P2[0, 2] and c.calib.cv == P2[1, 2]
    assert c.calib.tx == P2[0, 3] / -P2[0, 0] and c.calib.ty == P2[1, 3] / -P2[1, 1]
    assert c.stereo_fuxbaseline == g["fuxb"][0]
    assert Calib(SimpleNamespace(P2=g["P2B"], P3=g["P3B"]), (1, 1)).stereo_fuxbaseline == g["fuxb"][1]
    dm = torch.zeros(4, 5)
    dm[1, 3] = 10.0
    pts, xs, ys = c.depthmap_to_rect(dm)
    assert xs.tolist()[:5] == [0, 0, 0, 0, 1] and ys.tolist()[:5] == [0, 1, 2, 3, 0]        # x-major
    k = int(np.flatnonzero(pts[:, 2].numpy() > 0)[0])
    assert (xs[k].item(), ys[k].item()) == (3, 1)
    expect = ((np.float32(3.0) - np.float32(c.calib.cu)) * np.float32(10.0)) / np.float32(c.calib.fu) + np.float32(c.calib.tx)
    assert pts[k, 0].item() == pytest.approx(float(expect), rel=1e-6)


def test_oracle_fps_ties_follow_the_reference_tree():
    # N = 4 -> block size 4.  From point 0, points 1..3 are all at distance 1: the tree pairs slot 0 with 2 and 1 with 3, then 0 with 1;
    # slot 1 (point 1) and slot 2 (point 2) tie and slot 2 wins: the smallest bit-reversed slot (0b10 -> 0b01) beats 0b01 -> 0b10
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    assert O.fps(xyz, 2).tolist() == [[0, 2]]
    # N = 6 -> block size 4: point 4 sits in slot 0 behind point 0; a tie between points 4 and 1 goes to slot 0 (point 4)
    xyz = np.array([[[0, 0, 0], [2, 0, 0], [0, 0, 0], [0, 0, 0], [-2, 0, 0], [0, 0, 0]]], np.float32)
    assert O.fps(xyz, 3).tolist() == [[0, 4, 1]]
    assert O.opt_n_threads(6) == 4 and O.opt_n_threads(16384) == 1024 and O.opt_n_threads(1) == 1


def test_oracle_ball_query_without_hit_stays_zero_and_pads_with_first_hit():
    xyz = np.array([[[0, 0, 0], [5, 0, 0], [0.1, 0, 0], [0.2, 0, 0]]], np.float32)
    new = np.array([[[0, 0, 0], [100, 0, 0], [5, 0, 0]]], np.float32)
    idx = O.ball_query(0.5, 4, xyz, new)
    assert idx.tolist() == [[[0, 2, 3, 0], [0, 0, 0, 0], [1, 1, 1, 1]]]


def test_oracle_three_nn_keeps_the_first_of_duplicates():
    known = np.array([[[1, 0, 0], [1, 0, 0], [0, 2, 0], [1, 0, 0]]], np.float32)
    unknown = np.array([[[0, 0, 0]]], np.float32)
    d2, idx = O.three_nn(unknown, known)
    assert idx.tolist() == [[[0, 1, 3]]] and d2.tolist() == [[[1, 1, 1]]]
    d2, idx = O.three_nn(unknown, known[:, :2])
    assert idx[0, 0, :2].tolist() == [0, 1] and np.isinf(d2[0, 0, 2])


def test_oracle_gather_group_interpolate_and_scatter():
    pts = np.arange(2 * 2 * 5, dtype=np.float32).reshape(2, 2, 5)
    idx = np.array([[4, 0, 4], [1, 1, 2]], np.int32)
    assert O.gather(pts, idx)[1].tolist() == [[11, 11, 12], [16, 16, 17]]
    g = np.ones((2, 2, 3), np.float32)
    assert O.scatter_grad(g, idx, 5)[0, 0].tolist() == [1, 0, 0, 0, 2]
    gi = idx.reshape(2, 3, 1)
    assert O.group(pts, gi).shape == (2, 2, 3, 1)
    w = np.full((2, 1, 3), 0.5, np.float32)
    i3 = np.array([[[0, 1, 1]], [[2, 2, 2]]], np.int32)
    assert O.three_interpolate(pts, i3, w)[:, 0, 0].tolist() == [0.5 * 0 + 0.5 * 1 + 0.5 * 1, 1.5 * 12]
    assert O.scatter_grad(np.ones((2, 2, 1), np.float32), i3, 5, w)[0, 0].tolist() == [0.5, 1.0, 0, 0, 0]


# d^2 = 9 from the origin for every point but point 0: a cloud whose first FPS step ties in every slot
_TIE9 = np.array([[[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3], [-3, 0, 0], [0, -3, 0], [0, 0, -3], [2, 2, 1], [-2, -2, -1], [2, 1, 2],
                   [1, 2, 2], [-2, -1, -2]]], np.float32)


def test_oracle_fps_tie_order_at_block_size_8_with_ties_in_every_slot():
    # N = 12 -> block size 8: slot s holds points s and s + 8 (s < 4).  Step 1: every point but 0 is at d^2 = 9, so all eight slots
    # tie; slot 0 (bit-reversed 0) wins with its first point at the maximum, point 8.  Step 2 from point 8 leaves
    # temp = [0,9,9,9,6,6,9,9,0,9,9,2]: slots 1,2,3,6,7 tie at 9 with bit-reversed keys 4,2,6,3,7 -> slot 2, and of its points 2 and 10
    # (both 9) the first, 2.  Lowest-slot order would give point 1, last-in-slot order point 10.
    idx, temp = O.fps(_TIE9, 3, return_temp=True)
    assert O.opt_n_threads(12) == 8
    assert idx.tolist() == [[0, 8, 2]]
    assert temp.tolist() == [[0, 9, 9, 9, 6, 6, 9, 9, 0, 9, 9, 2]]        # the last step's running minimum (from point 8)


def test_oracle_fps_tie_order_at_block_size_4_and_m_beyond_n():
    # N = 4 -> block size 4.  From 0: slots 1,2,3 tie at 1 -> keys 2,1,3 -> point 2.  temp [0,1,1,1] -> from 2 (0,1,0): [0,1,0,1]
    # -> slots 1 and 3 tie -> point 1.  -> from 1: [0,0,0,1] -> point 3.  Then every distance is 0: slot 0, point 0, for ever.
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)
    idx, temp = O.fps(xyz, 7, return_temp=True)
    assert idx.tolist() == [[0, 2, 1, 3, 0, 0, 0]]
    assert temp.tolist() == [[0, 0, 0, 0]]
    # m = 1: the kernel never updates temp
    idx, temp = O.fps(xyz, 1, return_temp=True)
    assert idx.tolist() == [[0]] and (temp == np.float32(1e10)).all()


def test_oracle_ball_query_at_the_radius_without_hits_and_with_nsample_beyond_the_hits():
    # 0.5-grid coordinates: every squared distance is exact.  (1,0,0), (0,-1,0) and (0,0,1) sit on the unit sphere: `d2 < r2` is
    # strict, so they are not neighbours; points 1, 3 and 5 are (d2 0.25, 0.75, 0.5).
    xyz = np.array([[[1, 0, 0], [0.5, 0, 0], [0, -1, 0], [0.5, 0.5, 0.5], [0, 0, 1], [-0.5, 0, 0.5]]], np.float32)
    new = np.array([[[0, 0, 0], [10, 10, 10], [1, 0, 0]]], np.float32)
    idx = O.ball_query(1.0, 5, xyz, new)
    assert idx[0, 0].tolist() == [1, 3, 5, 1, 1]                 # nsample 5 > 3 hits: padded with the first hit
    assert idx[0, 1].tolist() == [0] * 5                         # no neighbour: the row stays as the caller zeroed it
    assert idx[0, 2].tolist() == [0, 1, 3, 0, 0]                 # (1,0,0): itself, (0.5,0,0) and (0.5,0.5,0.5) (d2 0.75); rest >= 2
    idx = O.ball_query(1.0, 8, xyz, new[:, 2:])
    assert idx[0, 0].tolist() == [0, 1, 3, 0, 0, 0, 0, 0]
    assert O.ball_query(0.0, 3, xyz, xyz).tolist() == np.zeros((1, 6, 3)).tolist()   # radius 0: d2 < 0 never holds


def test_oracle_three_nn_with_fewer_than_three_known_points_and_exact_ties():
    u = np.array([[[0, 0, 0]]], np.float32)
    d2, idx = O.three_nn(u, np.array([[[1, 0, 0]]], np.float32))
    assert idx.tolist() == [[[0, 0, 0]]] and d2[0, 0, 0] == 1 and np.isinf(d2[0, 0, 1:]).all()   # (float)1e40 = inf, index 0
    d2, idx = O.three_nn(u, np.array([[[0, 2, 0], [1, 0, 0]]], np.float32))
    assert idx.tolist() == [[[1, 0, 0]]] and d2[0, 0, :2].tolist() == [1, 4] and np.isinf(d2[0, 0, 2])
    # four known points at d2 = 1 (exact ties) behind a farther one: the first three in index order win
    d2, idx = O.three_nn(u, np.array([[[2, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1], [1, 0, 0]]], np.float32))
    assert idx.tolist() == [[[1, 2, 3]]] and d2.tolist() == [[[1, 1, 1]]]


def test_oracle_out_of_range_indices_read_zero_and_are_skipped_in_backward():
    pts = np.arange(1, 11, dtype=np.float32).reshape(1, 2, 5)
    idx = np.array([[-1, 5, 2147483647, 3]], np.int32)
    assert O.gather(pts, idx).tolist() == [[[0, 0, 0, 4], [0, 0, 0, 9]]]
    assert O.group(pts, idx.reshape(1, 2, 2)).tolist() == [[[[0, 0], [0, 4]], [[0, 0], [0, 9]]]]
    w = np.array([[[0.5, 0.25, 2.0]]], np.float32)
    assert O.three_interpolate(pts, np.array([[[1, -1, 4]]], np.int32), w).tolist() == [[[0.5 * 2 + 2.0 * 5], [0.5 * 7 + 2.0 * 10]]]
    g = O.scatter_grad(np.ones((1, 2, 4), np.float32), idx, 5)
    assert g.tolist() == [[[0, 0, 0, 1, 0], [0, 0, 0, 1, 0]]]
