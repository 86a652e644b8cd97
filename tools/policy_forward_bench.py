#!/usr/bin/env python3
"""The policy's inference: PyTorch's op-by-op forward + sampling against te_policy_act (one launch, te_policy.hpp) at 8 192, 16 384 and
65 536 rows, then the PPO collect split (tools/ppo_split.py's way) with PPOConfig.fused_forward off and on.  One JSON document on stdout.
    python tools/policy_forward_bench.py [n_envs_for_collect] [n_steps]
Bound: 267 k MACs per row -> 65 536 rows = 35.0 GFLOP = 0.22 ms at the 157.3 TF fp32 MFMA peak."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, FusedPolicy, LidarInertialActionPolicy, PPOConfig

N_COLLECT = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = int(sys.argv[2]) if len(sys.argv) > 2 else 32
MACS_PER_ROW = 32 * 48 * 12 + 64 * 128 * 3 + (15 * 128 + 2 * 128 * 128) + (4 * 128 + 2 * 128 * 128) + 448 * 256 + 2 * (256 * 64 + 64 * 64) + 64 * 5
PEAK_TFLOPS = 157.3


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


out = {"macs_per_row": MACS_PER_ROW, "forward": []}
torch.manual_seed(0)
policy = LidarInertialActionPolicy().to("cuda:0")
fused = FusedPolicy(policy)
for n in (8192, 16384, 65536):
    obs = {"lidar": torch.rand(n, 3, 13, 26, device="cuda:0"), "inertial_data": torch.rand(n, 15, device="cuda:0") * 2 - 1,
           "last_action": torch.rand(n, 4, device="cuda:0")}
    eps = torch.randn(n, 4, device="cuda:0")

    @torch.no_grad()
    def torch_act():
        mu, v = policy(obs)
        a = mu + policy.log_std.exp() * eps
        return a, (-0.5 * eps * eps - policy.log_std - 0.9189385332046727).sum(-1), v

    for _ in range(5):
        torch_act(); fused.act(obs, eps)
    t_torch = timed(torch_act, 50)
    t_fwd = timed(lambda: fused.forward(obs), 200)
    t_act = timed(lambda: fused.act(obs, eps), 200)
    flop = 2.0 * MACS_PER_ROW * n
    out["forward"].append({"rows": n, "pytorch_forward_sample_ms": t_torch * 1e3, "te_policy_act_forward_ms": t_fwd * 1e3,
                           "te_policy_act_sample_ms": t_act * 1e3, "speedup": t_torch / t_act,
                           "te_policy_act_TFLOPS": flop / t_act / 1e12, "fraction_of_fp32_mfma_peak": flop / t_act / 1e12 / PEAK_TFLOPS,
                           "bound_ms": flop / (PEAK_TFLOPS * 1e12) * 1e3})
    del obs, eps
del fused, policy
torch.cuda.empty_cache()

env = BatchedEnv(default_config("stage03", n_envs=N_COLLECT), "cuda:0")
env.reset()
a = env.random_actions(1, 0)
for _ in range(20):
    env.step(a, terminal=False)
t_env = timed(lambda: env.step(a, terminal=False), 200)
env.close()
out["collect"] = {"n_envs": N_COLLECT, "n_steps": T, "env_step_us": t_env * 1e6}
for ff in (False, True):
    env = BatchedEnv(default_config("stage03", n_envs=N_COLLECT), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=T, batch_size=N_COLLECT, n_epochs=1, use_graph=True, fused_forward=ff), seed=3)
    ppo.collect()                          # graph capture
    t_col = timed(ppo.collect, 3)
    out["collect"]["fused_forward" if ff else "pytorch_forward"] = {
        "collect_us_per_step": t_col / T * 1e6, "collect_Msteps_per_s": T * N_COLLECT / t_col / 1e6,
        "policy_share_of_collect": 1.0 - t_env * T / t_col}
    env.close(); del ppo
    torch.cuda.empty_cache()
print(json.dumps(out, indent=1))
