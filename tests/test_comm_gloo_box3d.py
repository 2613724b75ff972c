"""world_size-2 gloo tests (CPU) of the 3D results on the N>1 path: `box3d` travels through gather_predictions as its rows plus its mode,
and sharded_inference hands a sample's targets to the model."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from disprcnn_amd.utils import comm

FIELDS = ("scores", "box3d", "scores_3d", "random")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _spawn(worker, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=worker, args=(r, 2, port) + args + (q,)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r[0])


def _image(img, r, mode="ry_lhwxyz"):
    """Image `img` with r ROIs: every value is a function of (img, row), so rank 0 can rebuild what the other rank sent."""
    from disprcnn_amd.structures.bounding_box import BoxList
    from disprcnn_amd.structures.bounding_box_3d import Box3DList
    size = (1242 - img, 375 + img)
    bl = BoxList(torch.arange(r * 4, dtype=torch.float32).reshape(r, 4) + 100 * img, size)
    bl.add_field("scores", torch.linspace(0.1, 0.9, r) + img)
    bl.add_field("box3d", Box3DList(torch.arange(r * 7, dtype=torch.float32).reshape(r, 7) / 7 - 3 * img, size, mode))
    bl.add_field("scores_3d", -torch.linspace(0.5, 2.5, r) * (img + 1))
    bl.add_field("random", (torch.arange(r) + img) % 2)
    bl.add_field("note", "not a tensor")                                  # stays untransported
    return bl


def _gather_worker(rank, world, port, layout, q):
    _init(rank, world, port)
    try:
        from disprcnn_amd.structures.bounding_box_3d import Box3DList
        preds = {img: _image(img, r) for img, r in layout[rank]}
        got = comm.gather_predictions(preds, FIELDS)
        if rank != 0:
            assert got is None
            q.put((rank, "none"))
            return
        everything = sorted(layout[0] + layout[1])
        assert len(got) == len(everything)
        for b, (img, r) in zip(got, everything):
            want = _image(img, r)
            assert b.size == want.size and len(b) == r and sorted(b.fields()) == sorted(FIELDS)
            b3 = b.get_field("box3d")
            assert type(b3) is Box3DList and b3.mode == "ry_lhwxyz" and b3.size == want.size and len(b3) == r
            assert b3.bbox_3d.dtype == torch.float32 and torch.equal(b3.bbox_3d, want.get_field("box3d").bbox_3d)
            for f in ("scores", "scores_3d", "random"):
                assert b.get_field(f).dtype == want.get_field(f).dtype and torch.equal(b.get_field(f), want.get_field(f))
        q.put((rank, [len(b) for b in got]))
    finally:
        dist.destroy_process_group()


def test_box3d_travels_with_its_mode_and_each_images_size():
    res = _spawn(_gather_worker, {0: [(0, 2), (3, 4)], 1: [(1, 0), (2, 3)]})          # image 1 has no ROI
    assert res == [(0, [2, 0, 3, 4]), (1, "none")]


def test_a_rank_without_images_still_takes_part():
    res = _spawn(_gather_worker, {0: [(0, 3), (1, 1)], 1: []})
    assert res == [(0, [3, 1]), (1, "none")]


def _mismatch_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        preds = {rank: _image(rank, 2, "ry_lhwxyz" if rank == 0 else "xyzhwl_ry")}
        try:
            comm.gather_predictions(preds, FIELDS)
            q.put((rank, "no error"))
        except RuntimeError as ex:
            q.put((rank, "box3d" in str(ex) and "different dtypes / trailing shapes" in str(ex)))
    finally:
        dist.destroy_process_group()


def test_a_mode_mismatch_between_ranks_raises_on_every_rank():
    assert _spawn(_mismatch_worker) == [(0, True), (1, True)]


def _sharded_worker(rank, world, port, with_targets, q):
    _init(rank, world, port)
    try:
        seen = []

        class FakeDet3D:
            """image i: its 2D results get the 3D fields of _image(i, r); remembers what it was handed as targets"""

            def __call__(self, lr_images, lr_result, lr_targets="absent"):
                i = int(lr_images["left"])
                seen.append((i, lr_targets))
                b = lr_result["left"][0]
                src = _image(i, len(b))
                for f in ("box3d", "scores_3d", "random"):
                    b.add_field(f, src.get_field(f))
                return {"left": [b], "right": lr_result["right"]}

        def sample(i):
            src = _image(i, i % 3)
            b = src.copy_with_fields(["scores"])
            item = (i, {"left": i, "right": i}, {"left": [b], "right": [b]})
            return item + ({"left": [f"calib{i}"]},) if with_targets else item

        n = 5
        got = comm.sharded_inference(FakeDet3D(), [sample(i) for i in range(n)], fields=FIELDS)
        lo, hi = comm.shard_range(n)
        assert seen == [(i, {"left": [f"calib{i}"]} if with_targets else "absent") for i in range(lo, hi)]
        if rank == 0:
            assert len(got) == n
            for i, b in enumerate(got):
                want = _image(i, i % 3)
                assert len(b) == i % 3 and b.size == want.size and b.get_field("box3d").mode == "ry_lhwxyz"
                assert torch.equal(b.get_field("box3d").bbox_3d, want.get_field("box3d").bbox_3d) and b.get_field("box3d").size == want.size
                assert torch.equal(b.get_field("random"), want.get_field("random")) and b.get_field("random").dtype == torch.int64
                assert torch.equal(b.get_field("scores"), want.get_field("scores"))
        else:
            assert got is None
        q.put((rank, len(seen)))
    finally:
        dist.destroy_process_group()


def test_sharded_inference_hands_the_targets_over():
    assert _spawn(_sharded_worker, True) == [(0, 3), (1, 2)]


def test_sharded_inference_with_three_item_samples_is_unchanged():
    assert _spawn(_sharded_worker, False) == [(0, 3), (1, 2)]
