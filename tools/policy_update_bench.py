#!/usr/bin/env python3
"""The PPO learner's minibatch: autograd fp32 (plain Adam), PPOConfig.fast_learner (bf16 autocast + fused Adam),
PPOConfig.fused_update (te_policy_ppo_grad, te_policy_grad.hpp) and fused_update + PPOConfig.fused_optimizer (te_policy_adam_step,
te_policy_opt.hpp) at 2 048 (PPOConfig.batch_size's default), 8 192, 16 384 and 65 536 rows, each one update() of one
minibatch (gradient + clip + Adam) on a collected stage03 rollout; the te_policy_ppo_grad call alone against its fp32 MFMA bound;
then tools/ppo_split.py's 65 536-env collect + update with fused_forward=True, fused_update=True.  One JSON document on stdout.
    python tools/policy_update_bench.py [n_envs_for_split] [n_steps] [epochs]
    python tools/policy_update_bench.py --shapes [--rows 8192,65536] [--repeats 5] [--features-dim 512 --net-arch 128,256,512]
--shapes: the same minibatch for the wide shapes the gradient kernel serves (both, or the one given): autograd fp32 against
fused_update + fused_update_wide, and te_policy_ppo_grad_shaped alone, the three forms alternating, median [min, max] over the repeats.
--bf16 [--rows 8192,65536] [--repeats 5] [--split-envs 65536]: the three served shapes with PPOConfig.fused_update_bf16
(te_policy_ppo_grad_bf16, te_policy_grad_bf16.hpp) next to autograd fp32, fast_learner and fused_update: the full minibatch of each and
the fp32 and bf16 gradient calls alone, all forms alternating inside one process, median [min, max]; then one collect() + update() at
--split-envs envs (0: skip) with fused_forward_bf16 and fused_update_bf16 both on.
Bound: forward + activation gradients (all but conv1's, inertial.0's and action.0's inputs) + weight gradients, 2 FLOP per MAC, at
the 157.3 TF fp32 MFMA peak."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, PPOConfig

_pos = [] if "--shapes" in sys.argv or "--bf16" in sys.argv else sys.argv[1:]
N_SPLIT = int(_pos[0]) if len(_pos) > 0 else 65536
T = int(_pos[1]) if len(_pos) > 1 else 32
E = int(_pos[2]) if len(_pos) > 2 else 2
FWD = 32 * 48 * 12 + 64 * 128 * 3 + (15 * 128 + 2 * 128 * 128) + (4 * 128 + 2 * 128 * 128) + 448 * 256 + 2 * (256 * 64 + 64 * 64) + 64 * 5
MACS_PER_ROW = 3 * FWD - (32 * 48 * 12 + 15 * 128 + 4 * 128)
PEAK_TFLOPS = 157.3


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def shapes_mode(argv):
    """One minibatch per form and repeat, the forms alternating; ms, median [min, max]."""
    import statistics
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    rows_list = [int(r) for r in opt("--rows", "8192,65536").split(",")]
    repeats = int(opt("--repeats", "5"))
    shapes = {"reference BO": (512, (128, 256, 512)), "reference learn": (512, (512, 128, 256))}
    if "--features-dim" in argv or "--net-arch" in argv:
        shapes = {"given": (int(opt("--features-dim", "256")), tuple(int(w) for w in opt("--net-arch", "64,64").split(",")))}
    res = {"repeats": repeats, "unit": "ms per minibatch (gradient + clip + Adam), median [min, max]", "shapes": []}
    for name, (f, arch) in shapes.items():
        widths = (f,) + arch
        fwd = 32 * 48 * 12 + 64 * 128 * 3 + (15 * 128 + 2 * 128 * 128) + (4 * 128 + 2 * 128 * 128) + 448 * f + \
            2 * sum(a * b for a, b in zip(widths, widths[1:])) + arch[-1] * 5
        macs = 3 * fwd - (32 * 48 * 12 + 15 * 128 + 4 * 128)
        for rows in rows_list:
            forms, envs = {}, []
            for key, kw in (("autograd_fp32", {}), ("fused_update_wide", {"fused_update": True, "fused_update_wide": True})):
                env = BatchedEnv(default_config("stage03", n_envs=rows), "cuda:0")
                ppo = PPO(env, PPOConfig(n_steps=1, batch_size=rows, n_epochs=1, use_graph=False, features_dim=f, net_arch=arch, **kw), seed=3)
                ppo.collect()
                for _ in range(3):
                    ppo.update()
                forms[key] = ppo.update
                envs.append((env, ppo))
            ppo = envs[1][1]
            b = ppo.buf
            obs = {k: v.reshape(rows, *v.shape[2:]) for k, v in b.obs.items()}
            idx = torch.randperm(rows, device="cuda:0")
            ms = torch.tensor([0.0, 1.0], device="cuda:0")
            st = torch.empty(4, device="cuda:0")
            grad = torch.empty_like(ppo._flat_grad)
            forms["te_policy_ppo_grad_shaped"] = lambda: ppo.fused_grad.ppo_grad(obs, idx, b.actions.reshape(rows, 4), b.logp.reshape(-1),
                                                                                 b.adv.reshape(-1), b.ret.reshape(-1), ms, 0.2, 0.5, 0.0, grad, st)
            forms["te_policy_ppo_grad_shaped"]()
            times = {k: [] for k in forms}
            for _ in range(repeats):
                for k, fn in forms.items():
                    times[k].append(timed(fn, 10) * 1e3)
            rec = {"shape": name, "features_dim": f, "net_arch": list(arch), "rows": rows, "macs_per_row": macs,
                   "bound_ms": 2.0 * macs * rows / (PEAK_TFLOPS * 1e12) * 1e3}
            for k, ts in times.items():
                rec[k] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            rec["autograd_over_fused"] = rec["autograd_fp32"]["median"] / rec["fused_update_wide"]["median"]
            rec["te_policy_ppo_grad_shaped_TFLOPS"] = 2.0 * macs * rows / (rec["te_policy_ppo_grad_shaped"]["median"] * 1e-3) / 1e12
            res["shapes"].append(rec)
            for env, _ in envs:
                env.close()
            del envs, forms, ppo, b, obs, grad
            torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))


def bf16_mode(argv):
    """The bf16 gradient call next to every other form of the minibatch, the forms alternating; ms, median [min, max]."""
    import statistics
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    rows_list = [int(r) for r in opt("--rows", "8192,65536").split(",")]
    repeats, split_envs = int(opt("--repeats", "5")), int(opt("--split-envs", "65536"))
    shapes = {"default": (256, (64, 64)), "reference BO": (512, (128, 256, 512)), "reference learn": (512, (512, 128, 256))}
    res = {"repeats": repeats, "unit": "ms, median [min, max]; *_minibatch: gradient + clip + Adam, *_call: the gradient call alone", "shapes": []}
    fused = {"fused_update": True, "fused_update_wide": True}
    for name, (f, arch) in shapes.items():
        for rows in rows_list:
            forms, made = {}, {}
            for key, kw in (("autograd_fp32_minibatch", {}), ("fast_learner_minibatch", {"fast_learner": True}), ("fused_update_minibatch", fused),
                            ("fused_update_bf16_minibatch", {**fused, "fused_update_bf16": True})):
                env = BatchedEnv(default_config("stage03", n_envs=rows), "cuda:0")
                ppo = PPO(env, PPOConfig(n_steps=1, batch_size=rows, n_epochs=1, use_graph=False, features_dim=f, net_arch=arch, **kw), seed=3)
                ppo.collect()
                for _ in range(3):
                    ppo.update()
                forms[key] = ppo.update
                made[key] = (env, ppo)
            idx = torch.randperm(rows, device="cuda:0")
            ms = torch.tensor([0.0, 1.0], device="cuda:0")
            st = torch.empty(4, device="cuda:0")

            def alone(ppo):
                b = ppo.buf
                obs = {k: v.reshape(rows, *v.shape[2:]) for k, v in b.obs.items()}
                grad = torch.empty_like(ppo._flat_grad)
                return lambda: ppo.fused_grad.ppo_grad(obs, idx, b.actions.reshape(rows, 4), b.logp.reshape(-1), b.adv.reshape(-1),
                                                       b.ret.reshape(-1), ms, 0.2, 0.5, 0.0, grad, st)
            forms["te_policy_ppo_grad_shaped_call"] = alone(made["fused_update_minibatch"][1])
            forms["te_policy_ppo_grad_bf16_call"] = alone(made["fused_update_bf16_minibatch"][1])
            times = {k: [] for k in forms}
            for k, fn in forms.items():
                fn()
            for _ in range(repeats):
                for k, fn in forms.items():
                    times[k].append(timed(fn, 5) * 1e3)
            rec = {"shape": name, "features_dim": f, "net_arch": list(arch), "rows": rows}
            for k, ts in times.items():
                rec[k] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
            med = lambda k: rec[k]["median"]
            rec["bf16_call_speedup_vs_fp32_call"] = med("te_policy_ppo_grad_shaped_call") / med("te_policy_ppo_grad_bf16_call")
            rec["bf16_call_faster_beyond_spread"] = rec["te_policy_ppo_grad_bf16_call"]["max"] < rec["te_policy_ppo_grad_shaped_call"]["min"]
            rec["bf16_minibatch_speedup_vs_fast_learner"] = med("fast_learner_minibatch") / med("fused_update_bf16_minibatch")
            rec["bf16_minibatch_speedup_vs_autograd_fp32"] = med("autograd_fp32_minibatch") / med("fused_update_bf16_minibatch")
            res["shapes"].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
            for env, _ in made.values():
                env.close()
            del made, forms, ppo
            torch.cuda.empty_cache()
    if split_envs:
        f, arch = shapes["reference BO"]
        env = BatchedEnv(default_config("stage03", n_envs=split_envs), "cuda:0")
        ppo = PPO(env, PPOConfig(n_steps=T, batch_size=split_envs, n_epochs=E, use_graph=True, features_dim=f, net_arch=arch, fused_forward=True,
                                 fused_forward_bf16=True, fused_update=True, fused_update_wide=True, fused_update_bf16=True, fused_optimizer=True,
                                 fused_advantages=True), seed=3)
        ppo.collect(); ppo.update()
        t_col, t_upd = timed(ppo.collect, 3), timed(ppo.update, 2)
        stats = ppo.update()
        res["split"] = {"shape": "reference BO", "n_envs": split_envs, "n_steps": T, "batch_size": split_envs, "n_epochs": E,
                        "switches": "fused_forward(_bf16), fused_update(_wide, _bf16), fused_optimizer, fused_advantages",
                        "collect_s": t_col, "collect_Msteps_per_s": T * split_envs / t_col / 1e6, "update_s": t_upd,
                        "update_ms_per_minibatch": t_upd / (E * T) * 1e3, "collect_plus_update_Msteps_per_s": T * split_envs / (t_col + t_upd) / 1e6,
                        "finite": all(v == v and abs(v) < 1e30 for v in stats.values()), "last_update": stats}
        env.close()
    print(json.dumps(res, indent=1))


if "--shapes" in sys.argv:
    shapes_mode(sys.argv)
    sys.exit(0)
if "--bf16" in sys.argv:
    bf16_mode(sys.argv)
    sys.exit(0)

out = {"macs_per_row": MACS_PER_ROW, "minibatch": []}
for rows in (2048, 8192, 16384, 65536):
    rec = {"rows": rows, "bound_ms": 2.0 * MACS_PER_ROW * rows / (PEAK_TFLOPS * 1e12) * 1e3}
    for key, kw in (("autograd_fp32_ms", {}), ("fast_learner_ms", {"fast_learner": True}), ("fused_update_ms", {"fused_update": True}),
                    ("fused_optimizer_ms", {"fused_update": True, "fused_optimizer": True})):
        env = BatchedEnv(default_config("stage03", n_envs=rows), "cuda:0")
        ppo = PPO(env, PPOConfig(n_steps=1, batch_size=rows, n_epochs=1, use_graph=False, **kw), seed=3)
        ppo.collect()
        for _ in range(3):
            ppo.update()                     # warm-up: MIOpen algorithm search, the fused path's workspace
        rec[key] = timed(ppo.update, 20) * 1e3
        if key == "fused_update_ms":        # the gradient call alone, on the same rows
            b = ppo.buf
            obs = {k: v.reshape(rows, *v.shape[2:]) for k, v in b.obs.items()}
            idx = torch.randperm(rows, device="cuda:0")
            ms = torch.tensor([0.0, 1.0], device="cuda:0")
            st = torch.empty(4, device="cuda:0")
            call = lambda: ppo.fused_grad.ppo_grad(obs, idx, b.actions.reshape(rows, 4), b.logp.reshape(-1), b.adv.reshape(-1),
                                                   b.ret.reshape(-1), ms, 0.2, 0.5, 0.0, ppo._flat_grad, st)
            call()
            t = timed(call, 50)
            rec["te_policy_ppo_grad_ms"] = t * 1e3
            rec["te_policy_ppo_grad_TFLOPS"] = 2.0 * MACS_PER_ROW * rows / t / 1e12
            rec["fraction_of_fp32_mfma_peak"] = rec["te_policy_ppo_grad_TFLOPS"] / PEAK_TFLOPS
        env.close(); del ppo
        torch.cuda.empty_cache()
    rec["speedup_vs_autograd_fp32"] = rec["autograd_fp32_ms"] / rec["fused_update_ms"]
    rec["speedup_vs_fast_learner"] = rec["fast_learner_ms"] / rec["fused_update_ms"]
    rec["fused_optimizer_speedup_vs_fused_update"] = rec["fused_update_ms"] / rec["fused_optimizer_ms"]
    out["minibatch"].append(rec)

# tools/ppo_split.py's measurement with both fused paths on
env = BatchedEnv(default_config("stage03", n_envs=N_SPLIT), "cuda:0")
ppo = PPO(env, PPOConfig(n_steps=T, batch_size=N_SPLIT, n_epochs=E, use_graph=True, fused_forward=True, fused_update=True), seed=3)
ppo.collect(); ppo.update()                  # graph capture, workspace
t_col = timed(ppo.collect, 3)
t_upd = timed(ppo.update, 2)
stats = ppo.update()
mbs = E * ((T * N_SPLIT + N_SPLIT - 1) // N_SPLIT)
out["split"] = {"n_envs": N_SPLIT, "n_steps": T, "batch_size": N_SPLIT, "n_epochs": E, "fused_forward": True, "fused_update": True,
                "collect_s": t_col, "collect_us_per_step": t_col / T * 1e6, "collect_Msteps_per_s": T * N_SPLIT / t_col / 1e6,
                "update_s": t_upd, "update_ms_per_minibatch": t_upd / mbs * 1e3, "update_Msamples_per_s": E * T * N_SPLIT / t_upd / 1e6,
                "collect_plus_update_Msteps_per_s": T * N_SPLIT / (t_col + t_upd) / 1e6,
                "finite": all(v == v and abs(v) < 1e30 for v in stats.values()), "last_update": stats}
env.close()
print(json.dumps(out, indent=1))
