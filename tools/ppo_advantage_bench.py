#!/usr/bin/env python3
"""PPOConfig.fused_advantages against today's PyTorch code, the two forms alternating in one process:
  * RolloutBuffer.finish (the Python loop over n_steps) against finish(fused=True) (te_rollout_gae), T = 128, N = 8 192 and 65 536;
  * the minibatch's advantage statistics, a = adv[idx]; torch.stack((a.mean(), a.std())), against ppo.adv_stats (te_adv_stats),
    B = 2 048 and 65 536 rows drawn at random from a 128 x 65 536 rollout.
Every figure is the time of one call, from a host clock around `reps` calls that end in a device synchronise; WINDOWS windows per form,
reported as the median with min and max.  One JSON document on stdout (profiles/ppo_advantages.json is one run of it).
    python tools/ppo_advantage_bench.py [windows]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dronechase_amd.ppo import RolloutBuffer, adv_stats, adv_stats_workspace

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
T, GAMMA, LAM = 128, 0.99, 0.95
DEV = torch.device("cuda:0")


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def alternate(forms, reps):
    """{name: [ms per call] * WINDOWS}, the forms taking turns window by window after a warm-up of each."""
    for fn in forms.values():
        fn(); fn()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(timed(fn, reps[k]) * 1e3)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms)}


def record(times, base, new):
    rec = {k: summary(v) for k, v in times.items()}
    rec["speedup_of_medians"] = rec[base]["median_ms"] / rec[new]["median_ms"]
    return rec


out = {"device": torch.cuda.get_device_name(0), "n_steps": T, "gae": [], "stats": []}
gen = torch.Generator(device=DEV).manual_seed(3)
for n_envs in (8192, 65536):
    buf = RolloutBuffer(T, n_envs, {}, DEV)
    buf.rewards.normal_(generator=gen); buf.values.normal_(generator=gen)
    buf.dones.copy_((torch.rand((T, n_envs), generator=gen, device=DEV) < 0.01).float())
    last = torch.randn(n_envs, generator=gen, device=DEV)
    forms = {"finish_pytorch": lambda: buf.finish(last, GAMMA, LAM), "finish_fused": lambda: buf.finish(last, GAMMA, LAM, fused=True)}
    buf.finish(last, GAMMA, LAM)
    want = (buf.adv.clone(), buf.ret.clone())
    buf.finish(last, GAMMA, LAM, fused=True)
    same = torch.equal(buf.adv.view(torch.int32), want[0].view(torch.int32)) and torch.equal(buf.ret.view(torch.int32), want[1].view(torch.int32))
    rec = {"n_envs": n_envs, "bitwise_equal": same, "bytes_moved": 5 * 4 * T * n_envs,
           **record(alternate(forms, {"finish_pytorch": 20, "finish_fused": 1000}), "finish_pytorch", "finish_fused")}
    rec["fused_GBps"] = rec["bytes_moved"] / (rec["finish_fused"]["median_ms"] * 1e-3) / 1e9
    out["gae"].append(rec)
    del buf, want
    torch.cuda.empty_cache()

adv = torch.randn(T * 65536, generator=gen, device=DEV)
ws = adv_stats_workspace(adv.numel(), DEV)
ms_out = torch.zeros(2, device=DEV)
for rows in (2048, 65536):
    idx = torch.randperm(adv.numel(), generator=gen, device=DEV)[:rows].contiguous()

    def stats_pytorch():
        a = adv[idx]
        return torch.stack((a.mean(), a.std()))

    forms = {"stats_pytorch": stats_pytorch, "stats_fused": lambda: adv_stats(adv, idx, ms_out, ws)}
    want = stats_pytorch()
    adv_stats(adv, idx, ms_out, ws)
    rec = {"rows": rows, "largest_relative_gap_to_pytorch": float(((ms_out - want).abs() / want.abs()).max()),
           **record(alternate(forms, {"stats_pytorch": 2000, "stats_fused": 2000}), "stats_pytorch", "stats_fused")}
    out["stats"].append(rec)
print(json.dumps(out, indent=1))
