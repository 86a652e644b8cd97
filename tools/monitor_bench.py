#!/usr/bin/env python3
"""What PPOConfig.episode_stats costs: PPO collect (fused_forward, graph path, 32-step rollout) on stage03 with the episode monitor
off and on, alternating in one process, and the monitor kernel's own duration set against its bytes.

    python tools/monitor_bench.py collect [n_envs] [n_steps] [reps]         one JSON document on stdout
    rocprofv3 --kernel-trace --stats -d DIR -o monitor -- python tools/monitor_bench.py kernel [n_envs]
    python tools/monitor_bench.py merge collect.json DIR/.../monitor_kernel_stats.csv [n_envs]   -> both in one JSON document

`kernel` is the workload of the profiler run (a run of its own: tracing slows the host, so `collect` is timed without it): four
collects with the monitor on.  The kernel moves, per env and step, reward 4 + done 1 + ret 8 + len 8 = 21 bytes, + 16 of info on an env
that finishes: 37 B at most, 2.4 MB at 65 536 envs; at the 6.29 TB/s a float4 copy reaches on this GPU that is 0.39 us, far below a launch."""
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED = 6.29e12     # bytes/s, float4 copy
BYTES_PER_ENV = 37


def make(n_envs, n_steps, stats):
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=n_envs), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=n_steps, n_epochs=1, use_graph=True, fused_forward=True, episode_stats=stats), seed=3)
    ppo.collect()              # graph capture
    ppo.collect()
    return ppo


def collect(n_envs, n_steps, reps):
    import torch
    ppos = {False: make(n_envs, n_steps, False), True: make(n_envs, n_steps, True)}
    times = {False: [], True: []}
    last = {}
    for _ in range(reps):      # alternate, so that drift of the shared host hits both alike
        for on in (False, True):
            torch.cuda.synchronize(); t = time.perf_counter()
            last[on] = ppos[on].collect()
            torch.cuda.synchronize()
            times[on].append((time.perf_counter() - t) / n_steps * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(times[False]), med(times[True])
    return {"n_envs": n_envs, "n_steps": n_steps, "reps": reps, "collect_ms_per_step_off": off, "collect_ms_per_step_on": on,
            "collect_ms_per_step_off_all": times[False], "collect_ms_per_step_on_all": times[True],
            "overhead_us_per_step": (on - off) * 1e3, "overhead_fraction": on / off - 1, "last_log_on": last[True], "last_log_off": last[False]}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "collect"
    if mode == "collect":
        n, t, r = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 65536), (3, 32), (4, 9)))
        print(json.dumps(collect(n, t, r), indent=1))
    elif mode == "kernel":
        import torch
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
        ppo = make(n, 32, True)
        for _ in range(4):
            ppo.collect()
        torch.cuda.synchronize()
    elif mode == "merge":
        doc = json.load(open(sys.argv[2]))
        n = int(sys.argv[4]) if len(sys.argv) > 4 else doc["n_envs"]
        rows = [r for r in csv.DictReader(open(sys.argv[3])) if "monitor_" in r["Name"]]
        doc["kernels"] = [{"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                           "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3} for r in rows]
        step = [k for k in doc["kernels"] if "monitor_step_kernel" in k["name"]]
        if not step:
            raise SystemExit("no monitor_step_kernel row in the kernel stats")
        by = BYTES_PER_ENV * n
        doc["monitor_step_kernel"] = {"bytes_per_launch_at_most": by, "hbm_bound_us": by / HBM_MEASURED * 1e6, "average_us": step[0]["average_us"],
                                      "achieved_TB_per_s_at_most": by / (step[0]["average_us"] * 1e-6) / 1e12}
        print(json.dumps(doc, indent=1))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
