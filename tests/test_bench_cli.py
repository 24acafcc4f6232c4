"""bench.py's rank handling (no GPU): `--gpus N` must mean N ranks.

Under a launcher (WORLD_SIZE set) --gpus has to agree with it; started directly with
--gpus N > 1, bench.py launches N ranks itself through torch.distributed.run (a child
process, never an exec) -- here, with no GPU, every RCCL rank refuses to start and the
launcher's failure is bench.py's exit status.  The GPU form of this test, which renders with
two ranks and checks the assembled frame, is tests/test_gpu_bench.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_gpus_must_match_world_size():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE=3" in r.stderr


def test_gpus_spawns_ranks():
    r = _run(["--gpus", "2", "--config", "c2", "--steps", "1", "--warmup", "0",
              "--dist-backend", "nccl", "--no-cpu-baseline"])
    # the launcher started two ranks, and each refused: 2 RCCL ranks on a machine without GPUs
    assert "[launcher] 2 ranks" in r.stderr
    assert "--nproc-per-node=2" in r.stderr
    assert "2 RCCL ranks need 2 GPUs" in r.stderr
    assert r.returncode != 0
    assert r.stdout.strip() == ""


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs' writer: float32 files, whole frames while they fit the byte budget,
    otherwise the same seeded pixel sample of every array (with the pixel numbers) that stays
    within the budget and is identical from call to call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench

    W, H = 48, 32
    rng = np.random.default_rng(1)
    arrays = {"framebuffer_rgba8": rng.integers(0, 256, (W * H, 4), dtype=np.uint8),
              "accum_rgba": rng.random((W * H, 4), dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "whole"), W, H, arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "whole" / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (H, W, 4)
        assert np.array_equal(got.reshape(-1, 4), a.astype(np.float32))
    assert not (tmp_path / "whole" / "pixel_index.npy").exists()

    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), W, H, arrays)
    idx = np.load(tmp_path / "s1" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < W * H
    assert sum(f.stat().st_size - 128 for f in (tmp_path / "s1").iterdir()) <= 4000
    assert len(idx) == 4000 // 40
    for name, a in arrays.items():
        got = np.load(tmp_path / "s1" / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (len(idx), 4)
        assert np.array_equal(got, a[idx.astype(np.int64)].astype(np.float32))
        assert np.array_equal(got, np.load(tmp_path / "s2" / (name + ".npy")))
