#!/usr/bin/env python3
"""PPO collect on exp05 with the ally flown by a frozen policy snapshot, fused_forward on throughout:
  (a) te_drive_wingman inside the captured rollout graph (PPOConfig.wingman_driver="snapshot", use_graph=True), and the same eager;
  (b) the VecEnv-style sequence per step, eager: observe_ally -> PolicyDriver(fused=True).predict -> set_ally_actions;
  (c) stage03 (no ally), graph, for reference.
Then collect + n_epochs of update with fused_update for (a) and (c), and te_drive_wingman alone against observe_wingman +
te_policy_act.  One JSON document on stdout.
    python tools/exp05_collect_bench.py [n_envs] [n_steps] [epochs]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, PolicyDriver, PPOConfig

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = int(sys.argv[2]) if len(sys.argv) > 2 else 32
E = int(sys.argv[3]) if len(sys.argv) > 3 else 2


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def vecenv_style(ppo):
    """ThreatEngageVecEnv._drive_ally's four calls in place of te_drive_wingman."""
    driver = PolicyDriver(ppo.wingman.policy, fused=True)
    env = ppo.env

    def drive():
        lidar, inertial, last_action, _ = env.observe_ally()
        a, _ = driver.predict({"lidar": lidar, "inertial_data": inertial, "last_action": last_action}, deterministic=True)
        env.set_ally_actions(a.contiguous())
    ppo._drive_wingmen = drive


def run(task, graph, style, update):
    env = BatchedEnv(default_config(task, n_envs=N), "cuda:0")
    kw = dict(wingman_driver="snapshot") if task == "exp05" else {}
    ppo = PPO(env, PPOConfig(n_steps=T, batch_size=N, n_epochs=E, use_graph=graph, fused_forward=True, fused_update=True, **kw), seed=3)
    if style == "vecenv":
        vecenv_style(ppo)
    ppo.collect()                                  # graph capture
    if update:
        ppo.update()                               # workspace
    t_col = timed(ppo.collect, 3)
    rec = {"task": task, "use_graph": graph, "ally": style, "collect_us_per_step": t_col / T * 1e6, "collect_Msteps_per_s": T * N / t_col / 1e6}
    if update:
        t_upd = timed(ppo.update, 2)
        stats = ppo.update()
        rec.update(update_s=t_upd, collect_plus_update_Msteps_per_s=T * N / (t_col + t_upd) / 1e6,
                   finite=all(v == v and abs(v) < 1e30 for v in stats.values()), last_update=stats)
    env.close(); del ppo
    torch.cuda.empty_cache()
    return rec


out = {"n_envs": N, "n_steps": T, "n_epochs": E, "batch_size": N, "fused_forward": True, "fused_update": True}
out["a_drive_wingman_graph"] = run("exp05", True, "drive_wingman", True)
out["a_drive_wingman_eager"] = run("exp05", False, "drive_wingman", False)
out["b_vecenv_sequence_eager"] = run("exp05", False, "vecenv", False)
out["c_stage03_graph"] = run("stage03", True, None, True)

# the ally's part of one step alone: te_drive_wingman against observe_wingman + te_policy_act (no clamp, no set)
env = BatchedEnv(default_config("exp05", n_envs=N), "cuda:0")
env.reset()
ppo = PPO(env, PPOConfig(n_steps=1, wingman_driver="snapshot"), seed=3)
ppo._drive_wingmen()
t_drive = timed(ppo._drive_wingmen, 50)


def observe_and_act():
    lidar, inertial, last_action, _ = env.observe_wingman(1)
    ppo.wingman.forward({"lidar": lidar, "inertial_data": inertial, "last_action": last_action})


observe_and_act()
t_obs_act = timed(observe_and_act, 50)
out["ally_alone"] = {"te_drive_wingman_ms": t_drive * 1e3, "observe_wingman_plus_te_policy_act_ms": t_obs_act * 1e3}
env.close()
print(json.dumps(out, indent=1))
