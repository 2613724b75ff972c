"""bench.py's multi-rank control flow on CPU (gloo, world size 2): `python bench.py --gpus 2` must launch 2 ranks by itself,
every rank must enter the collective-bearing extra (the gradient all-reduce), timing is max-over-ranks, rank 0 prints ONE
JSON line with n_gpus = 2 (--gpus was ignored and a rank-0-only all-reduce would have hung)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env,
                          cwd=ROOT)


def _json_lines(out):
    lines = []
    for ln in out.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            try:
                lines.append(json.loads(ln))
            except ValueError:
                pass
    return lines


def test_gpus_flag_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run-cpu", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout                       # ONE line, from rank 0
    d = lines[0]
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["extra"]["dry_run_cpu"] and d["extra"]["grad_sync_ok"]          # both ranks took part in the all-reduce
    # max over ranks: rank 1's stand-in step sleeps 4 ms, rank 0's 2 ms
    assert d["ms_per_step"] >= 3.9, d["ms_per_step"]
    assert d["config"]["parallelism"].startswith("roi-shard x2")


def test_single_rank_dry_run_and_world_mismatch():
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "0", "--dry-run-cpu", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_lines(r.stdout)[0]
    assert d["n_gpus"] == 1 and d["extra"]["grad_sync_ok"]
    # launched by an external torchrun with another world size than --gpus: refuse instead of mislabelling the line
    r = _run(["--gpus", "4", "--dry-run-cpu"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_plain_run_leaves_the_extras_to_full():
    """Without --full the line carries the headline only: the collective-bearing extra is not entered, no roofline, no CPU baseline."""
    r = _run(["--gpus", "2", "--steps", "4", "--warmup", "1", "--dry-run-cpu"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] >= 3.9
    assert d["extra"] == {"dry_run_cpu": True} and d["roofline"] is None and d["cpu_baseline"] is None
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k


def test_dump_outputs_writes_float32_and_samples_above_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: the last step's disparity maps as DIR/disparity.npy (float32); above the byte limit a fixed seeded sample of
    whole ROIs, ascending, with their indices (float64) -- the same sample on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    disp = torch.arange(10 * 4 * 4, dtype=torch.float32).reshape(10, 4, 4)
    bench.dump_outputs(str(tmp_path / "all"), disp)
    got = np.load(tmp_path / "all" / "disparity.npy")
    assert got.dtype == np.float32 and np.array_equal(got, disp.numpy())
    assert not (tmp_path / "all" / "disparity_roi_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 300)                # 64 bytes per ROI (+ 8 for its index): 4 ROIs fit
    for sub in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / sub), disp)
    d1, i1 = np.load(tmp_path / "s1" / "disparity.npy"), np.load(tmp_path / "s1" / "disparity_roi_index.npy")
    assert d1.shape == (4, 4, 4) and i1.dtype == np.float64 and d1.nbytes + i1.nbytes <= 300
    assert np.all(np.diff(i1) > 0) and np.array_equal(d1, disp.numpy()[i1.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "s2" / "disparity_roi_index.npy"), i1)


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    """A plain GPU run: the headline line without the --full parts, and DIR/disparity.npy = forward_from_features of the bench's model
    on the bench's inputs (rank 0's tag), as this process computes it."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from disprcnn_amd.utils import synth
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rois", "16", "--dump-outputs", str(tmp_path)], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["extra"] == {}
    got = np.load(tmp_path / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == (16, 112, 112)
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dev, 48, 0, "A")
    fl, fr = synth.synth_features(16, 32, 28, 28, tag="bench0")
    with torch.no_grad():
        want = model.forward_from_features(fl.to(dev), fr.to(dev), (112, 112)).cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-4, np.abs(got - want).max()
