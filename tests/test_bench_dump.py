"""bench.py --dump-outputs: what the headline window's last step returned, written as .npy under a 64 MB budget."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 64 * 10**6


def _outputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"stacked": torch.rand((n, 6, 3, 13, 26), generator=g), "mask": (torch.rand((n, 6), generator=g) < 0.5).to(torch.uint8),
            "reward": torch.randn((n,), generator=g), "info": torch.randint(-2**31, 2**31 - 1, (n, 4), generator=g, dtype=torch.int32)}


def _sizes(paths):
    return sum(os.path.getsize(p) for p in paths)


def test_large_outputs_are_sampled_under_the_budget_with_the_same_rows(tmp_path):
    out = _outputs(4096, 0)   # 100 MB of stacked observations alone
    paths = bench.dump_outputs(str(tmp_path / "a"), out, env_index_base=8192)
    assert sorted(os.path.basename(p) for p in paths) == ["env_index.npy", "info.npy", "mask.npy", "reward.npy", "stacked.npy"]
    assert _sizes(paths) <= BUDGET
    got = {os.path.basename(p)[:-4]: np.load(p) for p in paths}
    idx = got["env_index"].astype(np.int64) - 8192
    assert 0 < len(idx) < 4096 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 4096
    assert got["stacked"].dtype == np.float32 and got["reward"].dtype == np.float32
    assert got["mask"].dtype == np.float64 and got["info"].dtype == np.float64 and got["env_index"].dtype == np.float64
    for k, t in out.items():   # every array holds the same env rows, integers exactly
        np.testing.assert_array_equal(got[k], t.numpy()[idx].astype(got[k].dtype))
    again = bench.dump_outputs(str(tmp_path / "b"), _outputs(4096, 0), env_index_base=8192)
    for p, q in zip(paths, again):
        np.testing.assert_array_equal(np.load(p), np.load(q))


def test_small_outputs_are_written_whole(tmp_path):
    out = _outputs(64, 1)
    paths = bench.dump_outputs(str(tmp_path), out)
    np.testing.assert_array_equal(np.load(paths[-1]), np.arange(64, dtype=np.float64))
    for p, (k, t) in zip(paths, out.items()):
        assert os.path.basename(p) == f"{k}.npy"
        np.testing.assert_array_equal(np.load(p), t.numpy())


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--envs-per-gpu", "4096",
                        "--headline-only", "--no-cpu-baseline", "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_dump_is_the_last_timed_step_and_repeats(tmp_path):
    """The dump equals a rollout of exactly warmup + steps env.step calls on the same inputs, and two runs (with and without the event
    replay after the window) write the same arrays."""
    a = _bench(tmp_path / "a")
    b = _bench(tmp_path / "b", "--no-profile-events")
    assert sorted(a) == ["done", "env_index", "inertial", "info", "last_action", "lidar", "reward"]
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert sum(v.nbytes for v in a.values()) <= BUDGET

    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    cfg = default_config("stage03", n_envs=4096, env_index_base=0, motor_noise=1, seed=0)
    env = BatchedEnv(cfg, "cuda:0")
    env.reset()
    act = torch.empty((4096, 4), dtype=torch.float32, device="cuda:0")
    for i in range(3 + 7):
        env.random_actions(1234, i, out=act)
        res = env.step(act, terminal=True)
    torch.cuda.synchronize()
    idx = a["env_index"].astype(np.int64)
    for k, t in zip(("lidar", "inertial", "last_action", "reward", "done", "info"), res):
        np.testing.assert_array_equal(a[k], t.cpu().numpy()[idx].astype(a[k].dtype), err_msg=k)
    env.close()
