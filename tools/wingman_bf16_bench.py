#!/usr/bin/env python3
"""The ally's precision on exp05: te_drive_wingman_shaped (fp32) against te_drive_wingman_bf16, for every served policy shape.
  (1) the bare call, BatchedEnv.drive_wingman with a FusedPolicy of either precision on one env a few steps into an episode;
      te_observe_wingman alone beside it (both calls contain it);
  (2) PPO collect, graph-captured, fused_forward + fused_forward_bf16, wingman_driver="snapshot", with PPOConfig.wingman_bf16 off and on;
  (3) what the switch costs numerically: over the rows of one collected rollout (eager, bf16 ally), the fp32 launch on the very rows the
      bf16 drive read: mean and max |mu_bf16 - mu_fp32|, and the share of envs whose clamped ally action differs.
The two precisions alternate within the run; five repeats, median [min, max].  Writes one JSON document (default
profiles/wingman_bf16.json) and prints it.
    python tools/wingman_bf16_bench.py [n_envs] [n_steps] [--out PATH] [--resources FILE.json]
--resources: the compiler's resource report of the six policy_drive_bf16_kernel instances (a JSON list made from the build's
-Rpass-analysis=kernel-resource-usage remarks: build_library(extra_flags=("-Rpass-analysis=kernel-resource-usage",))), copied into the
document as "resources"."""
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
ap.add_argument("n_envs", nargs="?", type=int, default=65536)
ap.add_argument("n_steps", nargs="?", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wingman_bf16.json"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()
N, T, REPEATS = args.n_envs, args.n_steps, 5
SERVED = {"default": (256, (64, 64)), "reference BO": (512, (128, 256, 512)), "reference learn": (512, (512, 128, 256))}
if not torch.cuda.is_available():
    sys.exit("wingman_bf16_bench: no GPU visible; this is a measurement, it has no CPU path")

stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def alternate(runs):
    """runs: {name: (fn, calls per window)}; REPEATS windows of each, the variants taking turns: {name: [seconds per call]}."""
    for _ in range(3):
        for fn, _reps in runs.values():
            fn()
    t = {k: [] for k in runs}
    for _ in range(REPEATS):
        for k, (fn, reps) in runs.items():
            t[k].append(timed(fn, reps))
    return t


def bare_calls(fdim, arch):
    env = BatchedEnv(default_config("exp05", n_envs=N, seed=3), "cuda:0")
    env.reset()
    torch.manual_seed(0)
    policy = LidarInertialActionPolicy(features_dim=fdim, net_arch=arch).to("cuda:0").requires_grad_(False)
    f32, b16 = FusedPolicy(policy), FusedPolicy(policy, precision="bf16")
    for s in range(4):          # a few steps in: the ally sees the others
        env.drive_wingman(1, f32)
        env.step(env.random_actions(8, s), terminal=False)
    mu = torch.empty((N, 4), device="cuda:0")
    t = alternate({"te_drive_wingman_shaped": (lambda: env.drive_wingman(1, f32, mu=mu), 50),
                   "te_drive_wingman_bf16": (lambda: env.drive_wingman(1, b16, mu=mu), 100),
                   "te_observe_wingman": (lambda: env.observe_wingman(1), 200)})
    rec = {k + "_ms": stat([x * 1e3 for x in v]) for k, v in t.items()}
    rec["fp32_over_bf16"] = rec["te_drive_wingman_shaped_ms"]["median"] / rec["te_drive_wingman_bf16_ms"]["median"]
    env.close()
    return rec


def collect(fdim, arch):
    ppos = {}
    for k, bf16 in (("ally_fp32", False), ("ally_bf16", True)):
        env = BatchedEnv(default_config("exp05", n_envs=N, seed=3), "cuda:0")
        ppos[k] = PPO(env, PPOConfig(n_steps=T, batch_size=N, n_epochs=1, use_graph=True, fused_forward=True, fused_forward_bf16=True,
                                     wingman_driver="snapshot", wingman_bf16=bf16, features_dim=fdim, net_arch=arch), seed=3)
        assert ppos[k].wingman.precision == ("bf16" if bf16 else "fp32")
        ppos[k].collect()                          # graph capture
    t = alternate({k: (p.collect, 3) for k, p in ppos.items()})
    rec = {k: {"collect_us_per_step": stat([x / T * 1e6 for x in v]), "collect_Msteps_per_s": T * N / statistics.median(v) / 1e6}
           for k, v in t.items()}
    rec["fp32_over_bf16"] = rec["ally_fp32"]["collect_us_per_step"]["median"] / rec["ally_bf16"]["collect_us_per_step"]["median"]
    for p in ppos.values():
        p.env.close()
    return rec


def numerics(fdim, arch):
    """One eager collect with the bf16 ally; after every drive the fp32 launch runs on the rows the drive just read."""
    env = BatchedEnv(default_config("exp05", n_envs=N, seed=3), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=T, batch_size=N, n_epochs=1, use_graph=False, fused_forward=True, fused_forward_bf16=True,
                             wingman_driver="snapshot", wingman_bf16=True, features_dim=fdim, net_arch=arch), seed=3)
    f32 = FusedPolicy(ppo.wingman.policy)
    low, high = torch.tensor([-1.0, -1.0, -1.0, 0.0], device="cuda:0"), torch.ones(4, device="cuda:0")
    clamp = lambda m: torch.max(torch.min(m, high), low)
    acc = {"rows": 0, "sum": 0.0, "max": 0.0, "differ": 0, "differ_1e-3": 0, "clamped_sum": 0.0, "clamped_max": 0.0, "mu_abs_sum": 0.0}
    drive = ppo._drive_wingmen

    def drive_and_compare():
        drive()
        f32.refresh()                               # the snapshot was synced at the start of this collect
        lidar, inertial, last_action = env.wingman_scratch(1)
        mu32, _ = f32.forward({"lidar": lidar, "inertial_data": inertial, "last_action": last_action})
        mu16 = ppo._wingman_mu[1]
        d, dc = (mu16 - mu32).abs(), (clamp(mu16) - clamp(mu32)).abs()
        acc["rows"] += N
        acc["sum"] += float(d.sum()); acc["max"] = max(acc["max"], float(d.max()))
        acc["clamped_sum"] += float(dc.sum()); acc["clamped_max"] = max(acc["clamped_max"], float(dc.max()))
        acc["differ"] += int((dc > 0).any(dim=1).sum()); acc["differ_1e-3"] += int((dc > 1e-3).any(dim=1).sum())
        acc["mu_abs_sum"] += float(mu32.abs().sum())
    ppo._drive_wingmen = drive_and_compare
    ppo.collect()
    env.close()
    r = acc["rows"]
    return {"rows": r, "mean_abs_mu_gap": acc["sum"] / (4 * r), "max_abs_mu_gap": acc["max"], "mean_abs_mu_fp32": acc["mu_abs_sum"] / (4 * r),
            "mean_abs_clamped_action_gap": acc["clamped_sum"] / (4 * r), "max_abs_clamped_action_gap": acc["clamped_max"],
            "share_of_envs_whose_clamped_action_differs": acc["differ"] / r,
            "share_of_envs_whose_clamped_action_differs_by_more_than_1e-3": acc["differ_1e-3"] / r}


doc = {"n_envs": N, "n_steps": T, "repeats": REPEATS, "task": "exp05", "device": torch.cuda.get_device_name(0),
       "collect_config": "use_graph, fused_forward, fused_forward_bf16, wingman_driver=snapshot", "shapes": []}
for name, (fdim, arch) in SERVED.items():
    rec = {"name": name, "features_dim": fdim, "net_arch": list(arch)}
    for part, fn in (("bare_call", bare_calls), ("collect", collect), ("numerics", numerics)):
        rec[part] = fn(fdim, arch)
        torch.cuda.empty_cache()
    doc["shapes"].append(rec)
    print(json.dumps(rec), flush=True)
if args.resources:
    with open(args.resources) as f:
        doc["resources"] = json.load(f)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc, indent=1))
