#!/usr/bin/env python3
"""The imitation dataset (csrc/te_dataset.hpp, dronechase_amd/imitation.py) against the PyTorch formulation of the same work.
    python tools/imitation_dataset_bench.py [--envs 2048,8192] [--batches 1024,8192] [--steps 20]
Inputs: real BatchedEnv.step_students() outputs of `level5_dumb` (seven wingmen per env, so 14 336 and 57 344 source rows), taken after
ten steps so that the snapshots' ring is full.
  (a) te_dataset_append (ImitationDataset.append_students) against torch: keep.nonzero() (a host synchronisation, included: a user pays
      it), five index_selects, slice assignment with the ring's wrap split in two.  Both append the same step over and over into a ring
      of twice the source rows, so every other call wraps.
  (b) te_dataset_gather (ImitationDataset.batch, "noise" branch, the index given) against five index_selects + torch.randn noise
      and clamp, over the same random slots; and the gather drawing its own slots (index=None).
  (c) ImitationDataset.collect against bare step_students(), steps per second.
Per item: warm-up, then five alternating repeats of a window of calls each ending in a device synchronise; median, min and max per
call.  Moved bytes: rows x 24 434 read and as many written (the scan's 7 bytes per source row on top), next to the 6.29 TB/s a float4
copy reaches on this device.  Before timing, the Gaussian branch is compared with the float64 restatement of tests/_dataset_cases.py.
One JSON document on stdout and in profiles/imitation_dataset.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.imitation import ImitationDataset

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=lambda s: tuple(int(w) for w in s.split(",")), default=(2048, 8192))
ap.add_argument("--batches", type=lambda s: tuple(int(w) for w in s.split(",")), default=(1024, 8192))
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()
DEV = torch.device("cuda:0")
REPEATS = 5
ROW_BYTES = 6 * 3 * 13 * 26 * 4 + 6 + (15 + 4 + 4) * 4
COPY_TBPS = 6.29


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def compare(runs, warmup=3):
    """{name: (fn, reps)} -> {name: [ms per call] x REPEATS}, the runs taking turns."""
    for _ in range(warmup):
        for fn, _reps in runs.values():
            fn()
    t = {k: [] for k in runs}
    for _ in range(REPEATS):
        for k, (fn, reps) in runs.items():
            t[k].append(timed(fn, reps) * 1e3)
    return t


stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


class TorchRing:
    """The same ring as five tensors, appended to and sampled with PyTorch calls."""

    def __init__(self, capacity):
        f32 = dict(dtype=torch.float32, device=DEV)
        self.capacity, self.total = capacity, 0
        self.rings = [torch.zeros((capacity, 6, 3, 13, 26), **f32), torch.zeros((capacity, 6), dtype=torch.uint8, device=DEV),
                      torch.zeros((capacity, 15), **f32), torch.zeros((capacity, 4), **f32), torch.zeros((capacity, 4), **f32)]

    def append_students(self, out):
        stacked, mask, inertial, last_action, active = (t.flatten(0, 1) for t in out[:5])
        keep = (active != 0) & (mask != 0).any(dim=1)
        idx = keep.nonzero().squeeze(1)                 # the host waits here
        k = int(idx.numel())
        start = self.total % self.capacity
        first = min(k, self.capacity - start)
        for ring, src in zip(self.rings, (stacked, mask, inertial, last_action, last_action)):
            rows = src.index_select(0, idx)
            ring[start:start + first] = rows[:first]
            if first < k:
                ring[:k - first] = rows[first:]
        self.total += k
        return k

    def batch(self, index, noise_std=0.2):
        stacked, mask, inertial, last_action, teacher = (r.index_select(0, index) for r in self.rings)
        last_action = (last_action + noise_std * torch.randn_like(last_action)).clamp_(-1.0, 1.0)
        return {"stacked_spheres": stacked, "validity_mask": mask, "inertial_data": inertial, "last_action": last_action}, teacher


def noise_gap():
    """max |te_dataset_gather's Gaussian branch - the float64 restatement| over 8 192 rows of a small ring."""
    from tests import _dataset_cases as D
    r = D.rows(range(80))
    ds = ImitationDataset(96, DEV, 80)
    t = {k: torch.tensor(v).to(DEV) for k, v in r.items()}
    ds.append({"stacked_spheres": t["stacked"], "validity_mask": t["mask"], "inertial_data": t["inertial"], "last_action": t["last_action"]}, t["teacher"])
    worst = 0.0
    for seed, draw in ((123456789, 5), (1, 0), (2 ** 63 + 7, 2 ** 40)):
        obs, _teacher = ds.batch(8192, last_action_mode="noise", seed=seed, draw=draw)
        want = D.la_noise(r["last_action"][D.philox_slots(8192, 80, seed, draw)], seed, draw)
        worst = max(worst, float(np.abs(obs["last_action"].cpu().numpy().astype(np.float64) - want).max()))
    return worst


doc = {"repeats": REPEATS, "row_bytes": ROW_BYTES, "float4_copy_TBps": COPY_TBPS, "noise_max_abs_gap_to_float64": noise_gap(), "noise_bound": 4e-6,
       "sizes": []}
for n_envs in args.envs:
    env = BatchedEnv(default_config("level5_dumb", n_envs=n_envs, seed=11), DEV)
    env.reset()
    for _ in range(10):
        out = env.step_students()
    rows = n_envs * int(env.cfg.n_pursuers)
    capacity = 2 * rows
    ds, ring = ImitationDataset(capacity, DEV, rows), TorchRing(capacity)
    kept = ring.append_students(out)
    ds.append_students(out)
    assert ds.total() == kept
    for a, b in zip((ds.stacked, ds.mask, ds.inertial, ds.last_action, ds.teacher), ring.rings):
        assert torch.equal(a[:kept], b[:kept])
    entry = {"envs": n_envs, "source_rows": rows, "kept_rows": kept, "capacity": capacity}

    # (a) append
    t = compare({"hip": (lambda: ds.append_students(out), 10), "torch": (lambda: ring.append_students(out), 10)})
    moved = 2 * kept * ROW_BYTES + 7 * rows
    med = {k: statistics.median(v) for k, v in t.items()}
    entry["append"] = {"hip_ms": stat(t["hip"]), "torch_ms": stat(t["torch"]), "torch_over_hip": med["torch"] / med["hip"], "moved_bytes": moved,
                       "hip_TBps": moved / med["hip"] / 1e9, "hip_fraction_of_float4_copy": moved / med["hip"] / 1e9 / COPY_TBPS}

    # (b) gather
    entry["gather"] = []
    gen = torch.Generator(device=DEV).manual_seed(n_envs)
    for B in args.batches:
        index = torch.randint(0, capacity, (B,), device=DEV, generator=gen)
        draws = iter(range(10 ** 9))
        t = compare({"hip": (lambda: ds.batch(B, index=index, last_action_mode="noise", seed=1, draw=next(draws)), 20),
                     "hip_own_slots": (lambda: ds.batch(B, last_action_mode="noise", seed=1, draw=next(draws)), 20),
                     "torch": (lambda: ring.batch(index), 20)})
        moved = 2 * B * ROW_BYTES + 8 * B
        med = {k: statistics.median(v) for k, v in t.items()}
        entry["gather"].append({"batch": B, "hip_ms": stat(t["hip"]), "hip_own_slots_ms": stat(t["hip_own_slots"]), "torch_ms": stat(t["torch"]),
                                "torch_over_hip": med["torch"] / med["hip"], "moved_bytes": moved, "hip_TBps": moved / med["hip"] / 1e9,
                                "hip_fraction_of_float4_copy": moved / med["hip"] / 1e9 / COPY_TBPS})

    # (c) collect against the bare step
    def bare():
        for _ in range(args.steps):
            env.step_students()

    t = compare({"step_students": (bare, 1), "collect": (lambda: ds.collect(env, args.steps), 1)}, warmup=1)
    med = {k: statistics.median(v) / args.steps for k, v in t.items()}
    entry["collect"] = {"steps_per_window": args.steps, "step_students_ms_per_step": stat([x / args.steps for x in t["step_students"]]),
                        "collect_ms_per_step": stat([x / args.steps for x in t["collect"]]), "step_students_steps_per_s": 1e3 / med["step_students"],
                        "collect_steps_per_s": 1e3 / med["collect"], "append_share_of_collect": 1.0 - med["step_students"] / med["collect"]}
    doc["sizes"].append(entry)
    print(json.dumps(entry), file=sys.stderr, flush=True)
    env.close()
    del ds, ring, env, out
    torch.cuda.empty_cache()
with open(os.path.join(ROOT, "profiles", "imitation_dataset.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc, indent=1))
