#!/usr/bin/env python3
"""The level5 student's sphere encoder: te_sphere_encode (one launch, csrc/te_sphere.hpp) and te_sphere_encode_bf16 (one launch,
csrc/te_sphere_bf16.hpp) against the PyTorch formulation of the same
two blocks (F.pad circular + F.pad constant + conv2d, twice: the reference's SphereCNN.block1 / block2, as FLIAStudent runs them) on the
same inputs, at 2 048, 8 192 and 65 536 rows of 6 spheres.
    python tools/student_encode_bench.py [--rows 2048,8192,65536] [--envs 2048] [--out profiles/student_encode_bf16.json]
Inputs: the stacked observations and validity masks of a real `level5` rollout (--envs environments, random actions, rows / envs steps),
timed twice: with every sphere valid (mask of ones) and with the rollout's own masks.  The PyTorch side has no way to skip a sphere and
computes all of them either way.  Per size and mask: warm-up, then five alternating repeats of a window of launches each ending in a
device synchronise; median, min and max per call.  Before timing, the outputs are compared on the counting spheres at that size;
the PyTorch reference of that comparison is computed 8 192 rows at a time, and the one-call PyTorch result is compared with it as well.
In the same alternation a whole StudentDriver.predict is timed once per encoder (PyTorch, fp32 fused, bf16 fused; seeded inertial_data
and last_action), which shows the encoder's share of a policy call.  The bf16 launch is also given in GB/s on the counting spheres'
bytes (4 056 read + 7 168 written each) against the 8 TB/s of the HBM, its floor.
One JSON document on stdout and in --out (profiles/student_encode.json is the run before the bf16 column existed).
Count: 7 x 13 x 32 x 75 + 4 x 7 x 64 x 288 = 734 496 MACs per sphere -> 65 536 rows of 6 valid spheres = 0.578 TFLOP =
3.7 ms at the 157.3 TF fp32 MFMA peak."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from dronechase_amd import default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.student import FLIAStudent, StudentDriver, counting_spheres

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=lambda s: tuple(int(w) for w in s.split(",")), default=(2048, 8192, 65536))
ap.add_argument("--envs", type=int, default=2048)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "student_encode_bf16.json"))
args = ap.parse_args()
DEV = torch.device("cuda:0")
MACS_PER_SPHERE = 7 * 13 * 32 * 75 + 4 * 7 * 64 * 288
PEAK_TFLOPS = 157.3
BYTES_PER_SPHERE = 3 * 13 * 26 * 4 + 1792 * 4
HBM_GBPS = 8000.0
REPEATS = 5
CHUNK = 8192


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def rollout(rows):
    """rows stacked observations and masks of a level5 rollout under random actions, from its second step on."""
    n = min(args.envs, rows)
    steps = rows // n
    env = BatchedEnv(default_config("level5", n_envs=n, seed=11), DEV)
    env.reset()
    stacked = torch.empty((rows, 6, 3, 13, 26), dtype=torch.float32, device=DEV)
    mask = torch.empty((rows, 6), dtype=torch.uint8, device=DEV)
    for s in range(steps + 8):          # 8 steps ahead: the ring of snapshots fills
        obs = env.step_stacked(env.random_actions(3, s), terminal=False)
        if s >= 8:
            stacked[(s - 8) * n:(s - 7) * n].copy_(obs[0]); mask[(s - 8) * n:(s - 7) * n].copy_(obs[1])
    torch.cuda.synchronize()
    env.close()
    return stacked, mask


torch.manual_seed(0)
student = FLIAStudent().to(DEV).requires_grad_(False).eval()
driver = StudentDriver(student, fused_encoder=True)
driver_bf16 = StudentDriver(student, fused_encoder=True, encoder_precision="bf16")
driver_torch = StudentDriver(student)
cnn = student.sphere_cnn
w1, b1, w2, b2 = (cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias)


@torch.no_grad()
def pytorch_blocks(stacked):
    x = stacked.reshape(-1, 3, 13, 26)
    x = F.relu(F.conv2d(F.pad(F.pad(x, (2, 2, 0, 0), mode="circular"), (0, 0, 2, 2), mode="constant", value=1.0), w1, b1, stride=2))
    x = F.relu(F.conv2d(F.pad(F.pad(x, (1, 1, 0, 0), mode="circular"), (0, 0, 1, 1), mode="constant", value=1.0), w2, b2, stride=2))
    return x.flatten(1)


stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
doc = {"repeats": REPEATS, "macs_per_sphere": MACS_PER_SPHERE, "peak_fp32_mfma_TFLOPS": PEAK_TFLOPS, "bytes_per_counting_sphere": BYTES_PER_SPHERE,
       "hbm_GBps": HBM_GBPS, "envs": args.envs, "sizes": []}
for rows in args.rows:
    stacked, real_mask = rollout(rows)
    scale = max(1, 65536 // rows)
    gen = torch.Generator(device=DEV).manual_seed(rows)
    rest = {"inertial_data": torch.randn((rows, 15), device=DEV, generator=gen), "last_action": torch.rand((rows, 4), device=DEV, generator=gen) * 2 - 1}
    for mask_name, mask in (("all_valid", torch.ones_like(real_mask)), ("rollout", real_mask)):
        counts = counting_spheres(mask)
        n_counting = int(counts.sum())
        # the reference in chunks of CHUNK rows: above 2^31 bytes per tensor the one-call PyTorch result is compared with it too
        got = driver.encode(stacked, mask).reshape(-1, 1792)[counts.reshape(-1)]
        ref_all = torch.cat([pytorch_blocks(stacked[i:i + CHUNK]) for i in range(0, rows, CHUNK)])
        one_call_gap = float((pytorch_blocks(stacked) - ref_all).abs().max())
        ref = ref_all[counts.reshape(-1)]
        gap = float((got - ref).abs().max())
        worst = float(((got - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max())
        got_bf16 = driver_bf16.encode(stacked, mask).reshape(-1, 1792)[counts.reshape(-1)]
        gap_bf16 = float((got_bf16 - ref).abs().max())
        gap_bf16_fp32 = float((got_bf16 - got).abs().max())
        del got, got_bf16, ref, ref_all
        obs = dict(rest, stacked_spheres=stacked, validity_mask=mask)
        runs = {"te_sphere_encode": (lambda: driver.encode(stacked, mask), 20 * scale),
                "te_sphere_encode_bf16": (lambda: driver_bf16.encode(stacked, mask), 20 * scale),
                "pytorch": (lambda: pytorch_blocks(stacked), 5 * scale),
                "predict_pytorch": (lambda: driver_torch.predict(obs), 3 * scale), "predict_fp32": (lambda: driver.predict(obs), 3 * scale),
                "predict_bf16": (lambda: driver_bf16.predict(obs), 3 * scale)}
        for _ in range(3):
            for fn, _reps in runs.values():
                fn()
        t = {k: [] for k in runs}
        for _ in range(REPEATS):
            for k, (fn, reps) in runs.items():
                t[k].append(timed(fn, reps) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        flop = 2.0 * MACS_PER_SPHERE * n_counting
        doc["sizes"].append({"rows": rows, "mask": mask_name, "spheres": rows * 6, "counting_spheres": n_counting,
                             "max_abs_gap_to_pytorch_chunked": gap, "gap_share_of_1e-4_bound": worst,
                             "pytorch_one_call_max_abs_gap_to_pytorch_chunked": one_call_gap,
                             "te_sphere_encode_ms": stat(t["te_sphere_encode"]), "pytorch_ms": stat(t["pytorch"]),
                             "pytorch_over_te_sphere_encode": med["pytorch"] / med["te_sphere_encode"],
                             "te_sphere_encode_TFLOPS_on_counting_spheres": flop / med["te_sphere_encode"] / 1e9,
                             "fraction_of_fp32_mfma_peak": flop / med["te_sphere_encode"] / 1e9 / PEAK_TFLOPS,
                             "bound_ms": flop / (PEAK_TFLOPS * 1e12) * 1e3,
                             "te_sphere_encode_bf16_ms": stat(t["te_sphere_encode_bf16"]),
                             "te_sphere_encode_over_bf16": med["te_sphere_encode"] / med["te_sphere_encode_bf16"],
                             "bf16_GBps_on_counting_spheres": n_counting * BYTES_PER_SPHERE / med["te_sphere_encode_bf16"] / 1e6,
                             "bf16_fraction_of_hbm": n_counting * BYTES_PER_SPHERE / med["te_sphere_encode_bf16"] / 1e6 / HBM_GBPS,
                             "bf16_max_abs_gap_to_pytorch_chunked": gap_bf16, "bf16_max_abs_gap_to_te_sphere_encode": gap_bf16_fp32,
                             "predict_ms": {"pytorch": stat(t["predict_pytorch"]), "fp32_fused": stat(t["predict_fp32"]),
                                            "bf16_fused": stat(t["predict_bf16"])},
                             "encoder_share_of_predict": {"fp32_fused": med["te_sphere_encode"] / med["predict_fp32"],
                                                          "bf16_fused": med["te_sphere_encode_bf16"] / med["predict_bf16"]}})
        print(json.dumps(doc["sizes"][-1]), file=sys.stderr, flush=True)
    del stacked, real_mask
    driver._out = driver_bf16._out = None
    torch.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc, indent=1))
