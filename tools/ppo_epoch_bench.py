#!/usr/bin/env python3
"""PPOConfig.fused_epoch (te_policy_ppo_epoch) against update()'s Python loop, both in one process, on the MI355X.

Per shape (default, reference BO, reference learn) and minibatch size (2 048, 8 192, 65 536 rows): two PPO objects on a stage03
rollout of 8 steps x `rows` envs, batch_size = rows, one epoch, i.e. 8 minibatches per update(); all four fused switches
(fused_forward, fused_update, fused_optimizer, fused_advantages) with the bf16 forward and gradient, the wide shapes through
fused_update_wide.  One has fused_epoch off (the Python loop: per minibatch five ABI calls, a slice and two tensor adds), the other
on (one ABI call per epoch).  Each repeat times one update() of each, alternating, between two stream events (and by the wall clock,
which agrees: update() ends with its host read); ms per minibatch = that / 8; median [min, max] over the repeats after a warm-up.
The gradient call alone on the same rows is timed next to them: what a minibatch cannot go below.
Then the README's reference-BO configuration (65 536 envs x 32 steps, batch_size 65 536, 2 epochs, graph-captured collect):
collect() + update() with fused_epoch off and on.  One JSON document on stdout (profiles/ppo_epoch.json).
    python tools/ppo_epoch_bench.py [--rows 2048,8192,65536] [--repeats 9] [--split-envs 65536]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, PPOConfig

opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
ROWS = [int(r) for r in opt("--rows", "2048,8192,65536").split(",")]
REPEATS, SPLIT_ENVS = int(opt("--repeats", "9")), int(opt("--split-envs", "65536"))
STEPS = 8           # minibatches per update()
SHAPES = {"default": (256, (64, 64)), "reference BO": (512, (128, 256, 512)), "reference learn": (512, (512, 128, 256))}
SWITCHES = dict(fused_forward=True, fused_forward_bf16=True, fused_update=True, fused_update_wide=True, fused_update_bf16=True,
                fused_optimizer=True, fused_advantages=True)


def timed(fn):
    """(ms between two stream events around fn, ms by the wall clock), fn's work finished in both."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


res = {"unit": "ms per minibatch, median [min, max] over the repeats; one update() = 8 minibatches of `rows` rows", "repeats": REPEATS,
       "switches": "fused_forward(_bf16), fused_update(_wide, _bf16), fused_optimizer, fused_advantages; fused_epoch off / on", "points": []}
for name, (f, arch) in SHAPES.items():
    for rows in ROWS:
        made = {}
        for key, on in (("python_loop", False), ("fused_epoch", True)):
            env = BatchedEnv(default_config("stage03", n_envs=rows), "cuda:0")
            ppo = PPO(env, PPOConfig(n_steps=STEPS, batch_size=rows, n_epochs=1, use_graph=False, features_dim=f, net_arch=arch, fused_epoch=on,
                                     **SWITCHES), seed=3)
            ppo.collect()
            for _ in range(3):
                ppo.update()          # warm-up: the workspace, the kernels' first launches
            made[key] = (env, ppo)
        ppo = made["python_loop"][1]
        b = ppo.buf
        n = STEPS * rows
        obs = {k: v.reshape(n, *v.shape[2:]) for k, v in b.obs.items()}
        idx = torch.randperm(n, device="cuda:0")[:rows].contiguous()
        ms, st, grad = torch.tensor([0.0, 1.0], device="cuda:0"), torch.empty(4, device="cuda:0"), torch.empty_like(ppo._flat_grad)

        def call():
            for _ in range(STEPS):
                ppo.fused_grad.ppo_grad(obs, idx, b.actions.reshape(n, 4), b.logp.reshape(-1), b.adv.reshape(-1), b.ret.reshape(-1), ms, 0.2, 0.5,
                                        0.0, grad, st)
        forms = {"python_loop": made["python_loop"][1].update, "fused_epoch": made["fused_epoch"][1].update, "gradient_call_alone": call}
        ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
        call()
        for _ in range(REPEATS):
            for k, fn in forms.items():
                e, w = timed(fn)
                ev[k].append(e / STEPS); wall[k].append(w / STEPS)
        rec = {"shape": name, "features_dim": f, "net_arch": list(arch), "rows": rows}
        for k in forms:
            rec[k] = summary(ev[k])
            rec[k + "_wall"] = summary(wall[k])
        rec["loop_over_epoch"] = rec["python_loop"]["median"] / rec["fused_epoch"]["median"]
        rec["outside_the_gradient_call_ms"] = {k: rec[k]["median"] - rec["gradient_call_alone"]["median"] for k in ("python_loop", "fused_epoch")}
        rec["gain_beyond_spread"] = rec["fused_epoch"]["max"] < rec["python_loop"]["min"]
        res["points"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        for env, _ in made.values():
            env.close()
        del made, forms, ppo, b, obs, grad
        torch.cuda.empty_cache()

if SPLIT_ENVS:
    f, arch = SHAPES["reference BO"]
    T, E = 32, 2
    res["split"] = {"shape": "reference BO", "n_envs": SPLIT_ENVS, "n_steps": T, "batch_size": SPLIT_ENVS, "n_epochs": E}
    for key, on in (("python_loop", False), ("fused_epoch", True)):
        env = BatchedEnv(default_config("stage03", n_envs=SPLIT_ENVS), "cuda:0")
        ppo = PPO(env, PPOConfig(n_steps=T, batch_size=SPLIT_ENVS, n_epochs=E, use_graph=True, features_dim=f, net_arch=arch, fused_epoch=on,
                                 **SWITCHES), seed=3)
        ppo.collect(); ppo.update()
        col = [timed(ppo.collect)[1] for _ in range(3)]
        upd = [timed(ppo.update)[1] for _ in range(5)]
        stats = ppo.update()
        c, u = statistics.median(col), statistics.median(upd)
        res["split"][key] = {"collect_ms": summary(col), "update_ms": summary(upd), "update_ms_per_minibatch": u / (E * T),
                             "collect_plus_update_Msteps_per_s": T * SPLIT_ENVS / ((c + u) * 1e-3) / 1e6,
                             "finite": all(v == v and abs(v) < 1e30 for k, v in stats.items() if k != "explained_variance")}
        env.close()
        del ppo, env
        torch.cuda.empty_cache()
print(json.dumps(res, indent=1))
