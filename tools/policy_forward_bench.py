#!/usr/bin/env python3
"""The policy's inference: PyTorch's op-by-op forward + sampling against te_policy_act (one launch, te_policy.hpp) at 8 192, 16 384 and
65 536 rows, then the PPO collect split (tools/ppo_split.py's way) with PPOConfig.fused_forward off and on.  One JSON document on stdout.
    python tools/policy_forward_bench.py [n_envs_for_collect] [n_steps] [--features-dim F] [--net-arch 128,256,512] [--no-collect]
--features-dim / --net-arch: the shape of the policy of those two parts (default 256 and 64,64).
Then every served shape at 65 536 rows: the fused launch (forward only, FusedPolicy.forward) against the op-by-op PyTorch forward of
the same module, five alternating repeats each (median, min and max), written to profiles/policy_shapes.json as well.
Bound, default shape: 267 k MACs per row -> 65 536 rows = 35.0 GFLOP = 0.22 ms at the 157.3 TF fp32 MFMA peak."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, FusedPolicy, LidarInertialActionPolicy, PPOConfig

ap = argparse.ArgumentParser()
ap.add_argument("n_collect", nargs="?", type=int, default=65536)
ap.add_argument("n_steps", nargs="?", type=int, default=32)
ap.add_argument("--features-dim", type=int, default=256)
ap.add_argument("--net-arch", type=lambda s: tuple(int(w) for w in s.split(",")), default=(64, 64))
ap.add_argument("--no-collect", action="store_true", help="skip the PPO collect split")
args = ap.parse_args()
N_COLLECT, T = args.n_collect, args.n_steps
SERVED = {"default": (256, (64, 64)), "reference BO": (512, (128, 256, 512)), "reference learn": (512, (512, 128, 256))}


def macs_per_row(features_dim, net_arch, c=3):
    widths = (features_dim,) + tuple(net_arch)
    return 32 * 16 * c * 12 + 64 * 128 * 3 + (15 * 128 + 2 * 128 * 128) + (4 * 128 + 2 * 128 * 128) + 448 * features_dim + \
        2 * sum(a * b for a, b in zip(widths, widths[1:])) + net_arch[-1] * 5


MACS_PER_ROW = macs_per_row(args.features_dim, args.net_arch)
PEAK_TFLOPS = 157.3


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


out = {"features_dim": args.features_dim, "net_arch": list(args.net_arch), "macs_per_row": MACS_PER_ROW, "forward": []}
torch.manual_seed(0)
policy = LidarInertialActionPolicy(features_dim=args.features_dim, net_arch=args.net_arch).to("cuda:0")
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

# ---- every served shape at 65 536 rows: the fused launch against the PyTorch forward it replaces, alternating repeats
ROWS, REPEATS = 65536, 5
shapes = {"rows": ROWS, "repeats": REPEATS, "peak_fp32_mfma_TFLOPS": PEAK_TFLOPS, "shapes": []}
obs = {"lidar": torch.rand(ROWS, 3, 13, 26, device="cuda:0"), "inertial_data": torch.rand(ROWS, 15, device="cuda:0") * 2 - 1,
       "last_action": torch.rand(ROWS, 4, device="cuda:0")}
for name, (fdim, arch) in SERVED.items():
    torch.manual_seed(0)
    policy = LidarInertialActionPolicy(features_dim=fdim, net_arch=arch).to("cuda:0")
    fused = FusedPolicy(policy)

    @torch.no_grad()
    def torch_forward():
        return policy(obs)

    for _ in range(5):
        torch_forward(); fused.forward(obs)
    t_f, t_t = [], []
    for _ in range(REPEATS):
        t_f.append(timed(lambda: fused.forward(obs), 100) * 1e3)
        t_t.append(timed(torch_forward, 30) * 1e3)
    flop = 2.0 * macs_per_row(fdim, arch) * ROWS
    med_f, med_t = statistics.median(t_f), statistics.median(t_t)
    shapes["shapes"].append({
        "name": name, "features_dim": fdim, "net_arch": list(arch), "param_words": fused.params.numel(), "macs_per_row": macs_per_row(fdim, arch),
        "fused_forward_ms": {"median": med_f, "min": min(t_f), "max": max(t_f)},
        "pytorch_forward_ms": {"median": med_t, "min": min(t_t), "max": max(t_t)},
        "pytorch_over_fused": med_t / med_f, "fused_TFLOPS": flop / med_f / 1e9,
        "fused_fraction_of_fp32_mfma_peak": flop / med_f / 1e9 / PEAK_TFLOPS, "bound_ms": flop / (PEAK_TFLOPS * 1e12) * 1e3})
    del fused, policy
del obs
torch.cuda.empty_cache()
out["shapes"] = shapes
with open(os.path.join(ROOT, "profiles", "policy_shapes.json"), "w") as f:
    json.dump(shapes, f, indent=1)
    f.write("\n")

if args.no_collect:
    print(json.dumps(out, indent=1))
    sys.exit(0)

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
    ppo = PPO(env, PPOConfig(n_steps=T, batch_size=N_COLLECT, n_epochs=1, use_graph=True, fused_forward=ff, features_dim=args.features_dim,
                             net_arch=args.net_arch), seed=3)
    ppo.collect()                          # graph capture
    t_col = timed(ppo.collect, 3)
    out["collect"]["fused_forward" if ff else "pytorch_forward"] = {
        "collect_us_per_step": t_col / T * 1e6, "collect_Msteps_per_s": T * N_COLLECT / t_col / 1e6,
        "policy_share_of_collect": 1.0 - t_env * T / t_col}
    env.close(); del ppo
    torch.cuda.empty_cache()
print(json.dumps(out, indent=1))
