"""bench.py --dump-outputs on CPU tensors: the arrays written, their dtypes, the fixed env sample and the
size bound.  The engine's side of the timed path is the GPU tests'; what is checked here is the dump."""
import os
import types

import numpy as np
import torch


def _outputs(n, agents=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(
        obs=torch.randint(0, 200, (n, agents, 3, 21, 21), dtype=torch.int64, generator=g),
        rewards=torch.rand((n, agents), dtype=torch.float64, generator=g),
        done=torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g),
        trunc=torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g),
        listed=torch.randint(0, 2, (n, agents), dtype=torch.uint8, generator=g),
        was_reset=torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_every_output(tmp_path):
    import bench
    assert bench.DUMP_OBS_BYTES < 64 * 10 ** 6
    src = _outputs(37)
    bench.dump_outputs(str(tmp_path / "a"), src)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == ["done", "listed", "obs", "obs_env_index", "rewards", "truncated", "was_reset"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    # small enough: every env, in order, values exact
    assert np.array_equal(got["obs_env_index"], np.arange(37))
    assert np.array_equal(got["obs"], src.obs.numpy()) and got["obs"].dtype == np.float32
    assert np.array_equal(got["rewards"], src.rewards.numpy()) and got["rewards"].dtype == np.float64
    assert np.array_equal(got["truncated"], src.trunc.numpy()) and np.array_equal(got["done"], src.done.numpy())
    assert np.array_equal(got["listed"], src.listed.numpy()) and np.array_equal(got["was_reset"], src.was_reset.numpy())


def test_dump_outputs_samples_the_same_envs_within_the_bound(tmp_path, monkeypatch):
    import bench
    src = _outputs(300)
    per_env = src.obs[0].numel() * 4
    monkeypatch.setattr(bench, "DUMP_OBS_BYTES", 64 * per_env + 5)  # room for 64 of the 300 envs
    bench.dump_outputs(str(tmp_path / "a"), src)
    bench.dump_outputs(str(tmp_path / "b"), src, suffix="_rank1")
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["obs_env_index"].astype(np.int64)
    assert len(idx) == 64 and len(set(idx)) == 64 and np.all(np.diff(idx) > 0) and idx.max() < 300
    assert np.array_equal(a["obs"], src.obs.numpy()[idx])
    assert a["rewards"].shape == (300, 2) and a["done"].shape == (300,)
    # the sample is fixed: a second dump picks the same envs
    assert sorted(b) == sorted(k + "_rank1" for k in a)
    assert all(np.array_equal(a[k], b[k + "_rank1"]) for k in a)
    assert a["obs"].nbytes <= bench.DUMP_OBS_BYTES
