#!/usr/bin/env python3
"""The policy's inference: PyTorch's op-by-op forward + sampling against te_policy_act (one launch, te_policy.hpp) at 8 192, 16 384 and
65 536 rows, then the PPO collect split (tools/ppo_split.py's way) with PPOConfig.fused_forward off and on.  One JSON document on stdout.
    python tools/policy_forward_bench.py [n_envs_for_collect] [n_steps] [--features-dim F] [--net-arch 128,256,512] [--no-collect]
--features-dim / --net-arch: the shape of the policy of those two parts (default 256 and 64,64).
Then every served shape at 65 536 rows: the fused launch (forward only, FusedPolicy.forward) against the op-by-op PyTorch forward of
the same module, five alternating repeats each (median, min and max), written to profiles/policy_shapes.json as well.
Then te_policy_act_bf16 (FusedPolicy(precision="bf16")) for every served shape at 8 192 and 65 536 rows against the fp32 fused launch, the
PyTorch fp32 forward and the PyTorch forward under torch.autocast(bfloat16), five alternating repeats each (median, min, max), and the PPO
collect split of net_arch (128, 256, 512) with PPOConfig.fused_forward_bf16 off and on, written to profiles/policy_bf16.json; --only-bf16 runs
this part alone.  TE_POLICY_BF16_RECORD=<path>: the JSON lines tests/test_policy_bf16.py wrote there become the file's "numerics".
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
ap.add_argument("--only-bf16", action="store_true", help="only the bf16 part (profiles/policy_bf16.json)")
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


def bf16_part():
    """te_policy_act_bf16 against the three forwards it competes with, and the collect split; profiles/policy_bf16.json."""
    REPEATS = 5
    stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
    doc = {"repeats": REPEATS, "rows": [8192, 65536], "forward_ms": [], "collect": None, "numerics": []}
    for rows in doc["rows"]:
        obs = {"lidar": torch.rand(rows, 3, 13, 26, device="cuda:0"), "inertial_data": torch.rand(rows, 15, device="cuda:0") * 2 - 1,
               "last_action": torch.rand(rows, 4, device="cuda:0")}
        for name, (fdim, arch) in SERVED.items():
            torch.manual_seed(0)
            policy = LidarInertialActionPolicy(features_dim=fdim, net_arch=arch).to("cuda:0")
            f32, b16 = FusedPolicy(policy), FusedPolicy(policy, precision="bf16")

            @torch.no_grad()
            def torch_forward():
                return policy(obs)

            @torch.no_grad()
            def torch_autocast():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return policy(obs)

            runs = {"fused_bf16": (lambda: b16.forward(obs), 100), "fused_fp32": (lambda: f32.forward(obs), 50),
                    "pytorch_fp32": (torch_forward, 30), "pytorch_autocast_bf16": (torch_autocast, 30)}
            for _ in range(5):
                for fn, _reps in runs.values():
                    fn()
            t = {k: [] for k in runs}
            for _ in range(REPEATS):
                for k, (fn, reps) in runs.items():
                    t[k].append(timed(fn, reps * (65536 // rows)) * 1e3)     # the same work per window at either size
            med = {k: statistics.median(v) for k, v in t.items()}
            flop = 2.0 * macs_per_row(fdim, arch) * rows
            doc["forward_ms"].append({
                "rows": rows, "name": name, "features_dim": fdim, "net_arch": list(arch), "bf16_halfwords": b16.weights_bf16.numel(),
                **{k: stat(v) for k, v in t.items()},
                "pytorch_fp32_over_fused_bf16": med["pytorch_fp32"] / med["fused_bf16"],
                "pytorch_autocast_over_fused_bf16": med["pytorch_autocast_bf16"] / med["fused_bf16"],
                "fused_fp32_over_fused_bf16": med["fused_fp32"] / med["fused_bf16"], "fused_bf16_TFLOPS": flop / med["fused_bf16"] / 1e9})
            del f32, b16, policy
        del obs
        torch.cuda.empty_cache()

    fdim, arch = SERVED["reference BO"]
    env = BatchedEnv(default_config("stage03", n_envs=N_COLLECT), "cuda:0")
    env.reset()
    a = env.random_actions(1, 0)
    for _ in range(20):
        env.step(a, terminal=False)
    t_env = timed(lambda: env.step(a, terminal=False), 200)
    env.close()
    col = {"n_envs": N_COLLECT, "n_steps": T, "features_dim": fdim, "net_arch": list(arch), "env_step_us": t_env * 1e6}
    variants = {"pytorch_forward": {}, "fused_forward": {"fused_forward": True}, "fused_forward_bf16": {"fused_forward": True, "fused_forward_bf16": True}}
    ppos, t_col = {}, {k: [] for k in variants}
    for k, kw in variants.items():
        env = BatchedEnv(default_config("stage03", n_envs=N_COLLECT), "cuda:0")
        ppos[k] = PPO(env, PPOConfig(n_steps=T, batch_size=N_COLLECT, n_epochs=1, use_graph=True, features_dim=fdim, net_arch=arch, **kw), seed=3)
        ppos[k].collect()                          # graph capture
    for _ in range(REPEATS):
        for k in variants:
            t_col[k].append(timed(ppos[k].collect, 2))
    for k in variants:
        m = statistics.median(t_col[k])
        col[k] = {"collect_us_per_step": stat([x / T * 1e6 for x in t_col[k]]), "collect_Msteps_per_s": T * N_COLLECT / m / 1e6,
                  "policy_share_of_collect": 1.0 - t_env * T / m}
    # what the switch costs PPO: old_logp is the bf16 forward's, update()'s forward is fp32, so log(ratio) of the first epoch is not 0
    b = ppos["fused_forward_bf16"].buf
    with torch.no_grad():
        t0 = slice(0, 2)                            # two steps of the rollout: 131 072 rows at the default size
        d, v = ppos["fused_forward_bf16"].policy.dist({k: o[t0].reshape(-1, *o.shape[2:]) for k, o in b.obs.items()})
        lr = (d.log_prob(b.actions[t0].reshape(-1, 4)).sum(-1) - b.logp[t0].reshape(-1)).abs()
        dv = (v - b.values[t0].reshape(-1)).abs()
    col["first_epoch_abs_log_ratio"] = {"max": float(lr.max()), "mean": float(lr.mean())}
    col["value_abs_gap_to_fp32_module"] = {"max": float(dv.max()), "mean": float(dv.mean())}
    for p in ppos.values():
        p.env.close()
    doc["collect"] = col
    rec = os.environ.get("TE_POLICY_BF16_RECORD")
    if rec and os.path.exists(rec):
        doc["numerics"] = [json.loads(line) for line in open(rec) if line.strip()]
    with open(os.path.join(ROOT, "profiles", "policy_bf16.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if args.only_bf16:
    print(json.dumps({"bf16": bf16_part()}, indent=1))
    sys.exit(0)

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
out["bf16"] = bf16_part()
print(json.dumps(out, indent=1))
