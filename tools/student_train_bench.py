#!/usr/bin/env python3
"""Training the level5 student's sphere encoder: te_sphere_encode + te_sphere_encode_grad (csrc/te_sphere.hpp) against autograd through
the PyTorch formulation of the same two blocks (FLIAStudent.sphere_cnn.conv_stack), and StudentTrainer.step with and without
fused_encoder, at 1 024 rows (the reference loader's batch) and 8 192 rows of 6 spheres.
    python tools/student_train_bench.py [--rows 1024,8192] [--envs 1024] [--record FILE]
Inputs: as tools/student_encode_bench.py, the stacked observations and validity masks of a real `level5` rollout, timed with every
sphere valid and with the rollout's own masks; the other observation parts and the teacher's action are seeded noise.  The PyTorch
side cannot skip a sphere; past 8 192 rows it runs 8 192 rows at a time (its intermediates pass 2^31 bytes).
  (a) encoder forward + backward: the two launches' calls, against conv_stack + torch.autograd.grad for the four conv tensors only;
  (b) StudentTrainer.step (train mode, Adam, clip_grad_norm_), fused_encoder=True against False, on two copies of one student.
Per size and mask: warm-up, then five alternating repeats of a window of calls each ending in a device synchronise; median, min and
max per call.  Before timing, the fused gradient and PyTorch's fp32 gradient are both compared with PyTorch's float64 one at that size,
and the float64 pre-activations within 1e-5 of zero and the block2 ReLU decisions that differ from float64's are counted (a rollout's
inputs are not kink-free: a decision that differs moves a gradient by a whole term, not by a rounding error).
--record: the JSON lines that tests/test_gpu_student_grad.py appends under TE_STUDENT_GRAD_RECORD, copied into the document.
One JSON document on stdout and in profiles/student_train.json.
Count: the backward's four GEMMs (block1 again, dW2, the column matrix, dW1) are 2 x 734 496 MACs per sphere, the forward 734 496."""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dronechase_amd import _lib, default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.student import FLIAStudent, StudentTrainer, counting_spheres

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=lambda s: tuple(int(w) for w in s.split(",")), default=(1024, 8192))
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--record", default=None)
args = ap.parse_args()
DEV = torch.device("cuda:0")
MACS_FORWARD = 7 * 13 * 32 * 75 + 4 * 7 * 64 * 288
MACS_BACKWARD = 2 * MACS_FORWARD
PEAK_TFLOPS = 157.3
REPEATS = 5
CHUNK = 8192


def timed(fn, reps):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def rollout(rows):
    """rows stacked observations and masks of a level5 rollout under random actions, from its ninth step on."""
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
student = FLIAStudent().to(DEV)
cnn = student.sphere_cnn
conv = [cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias]
params = torch.cat([p.detach().reshape(-1) for p in conv])


class Fused:
    """te_sphere_encode + te_sphere_encode_grad on buffers of its own."""

    def __init__(self, rows):
        need = C.c_size_t()
        _lib.call("te_sphere_encode_grad_workspace_bytes", 3, rows, 6, C.byref(need))
        self.ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        self.out = torch.empty((rows, 6, 1792), dtype=torch.float32, device=DEV)
        self.grad = torch.empty_like(params)
        self.rows = rows

    def __call__(self, stacked, mask, d_out):
        _lib.call_on(DEV, "te_sphere_encode", params.data_ptr(), 3, self.rows, 6, stacked.data_ptr(), mask.data_ptr(), self.out.data_ptr())
        _lib.call_on(DEV, "te_sphere_encode_grad", params.data_ptr(), 3, self.rows, 6, stacked.data_ptr(), mask.data_ptr(), self.out.data_ptr(),
                     d_out.data_ptr(), self.grad.data_ptr(), self.ws.data_ptr(), self.ws.numel())
        return self.grad


def pytorch_grads(stacked, d_out, net=cnn, chunk=CHUNK):
    """autograd through conv_stack, gradients of the four conv tensors only; `chunk` rows at a time, in the dtype of `net`."""
    tensors = [net.block1[0].conv.weight, net.block1[0].conv.bias, net.block2[0].conv.weight, net.block2[0].conv.bias]
    total = None
    for i in range(0, stacked.shape[0], chunk):
        out = net.conv_stack(stacked[i:i + chunk].reshape(-1, 3, 13, 26).to(tensors[0].dtype))
        g = torch.autograd.grad(out, tensors, d_out[i:i + chunk].reshape(-1, 1792).to(tensors[0].dtype))
        total = g if total is None else [a + b for a, b in zip(total, g)]
    return torch.cat([t.reshape(-1) for t in total])


cnn64 = copy.deepcopy(cnn).double()


def gaps(got, ref64):
    """max |d| and its largest share of 1e-4 + 1e-4 |ref| against the float64 gradient."""
    d = (got.double() - ref64).abs()
    return {"max_abs": float(d.max()), "share_of_1e-4_bound": float((d / (1e-4 + 1e-4 * ref64.abs())).max())}


stat = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
doc = {"repeats": REPEATS, "macs_per_sphere_forward": MACS_FORWARD, "macs_per_sphere_backward": MACS_BACKWARD, "peak_fp32_mfma_TFLOPS": PEAK_TFLOPS,
       "envs": args.envs, "sizes": []}
if args.record and os.path.exists(args.record):
    with open(args.record) as f:
        doc["kinkfree_ratios"] = [json.loads(line) for line in f if line.strip()]
for rows in args.rows:
    stacked, real_mask = rollout(rows)
    gen = torch.Generator(device=DEV).manual_seed(rows)
    d_out = torch.randn((rows, 6, 1792), device=DEV, generator=gen)
    inertial = torch.randn((rows, 15), device=DEV, generator=gen)
    last_action = torch.rand((rows, 4), device=DEV, generator=gen) * 2 - 1
    teacher = torch.rand((rows, 4), device=DEV, generator=gen) * 2 - 1
    fused = Fused(rows)
    scale = max(1, 8192 // rows)
    for mask_name, mask in (("all_valid", torch.ones_like(real_mask)), ("rollout", real_mask)):
        counts = counting_spheres(mask)
        n_counting = int(counts.sum())
        # the gradient of the counting spheres: the PyTorch side gets zeros upstream at the others
        d_counting = d_out * counts.unsqueeze(-1)
        # both fp32 gradients against the same function in float64 (PyTorch, 1 024 rows at a time), and what stands between fp32 and
        # float64 besides rounding: ReLU decisions that differ, each of which moves a gradient by a whole term
        ref64 = pytorch_grads(stacked, d_counting, cnn64, 1024)
        gap_fused, gap_pytorch = gaps(fused(stacked, mask, d_out), ref64), gaps(pytorch_grads(stacked, d_counting), ref64)
        near1 = near2 = flips_fused = flips_pytorch = 0
        with torch.no_grad():
            for i in range(0, rows, 1024):
                x, c = stacked[i:i + 1024].reshape(-1, 3, 13, 26), counts[i:i + 1024].reshape(-1)
                z1 = cnn64.block1[0](x.double())
                z2 = cnn64.block2[0](torch.relu(z1)).flatten(1)
                near1 += int(((z1.abs() < 1e-5).flatten(1) & c[:, None]).sum()); near2 += int(((z2.abs() < 1e-5) & c[:, None]).sum())
                flips_fused += int((((fused.out[i:i + 1024].reshape(-1, 1792) > 0) != (z2 > 0)) & c[:, None]).sum())
                flips_pytorch += int((((cnn.conv_stack(x) > 0) != (z2 > 0)) & c[:, None]).sum())
        kinks = {"fp64_preactivations_within_1e-5_of_zero": {"block1": near1, "block2": near2},
                 "block2_relu_decisions_differing_from_fp64": {"fused": flips_fused, "pytorch_fp32": flips_pytorch}}
        obs = {"stacked_spheres": stacked, "validity_mask": mask, "inertial_data": inertial, "last_action": last_action}
        trainers = {k: StudentTrainer(copy.deepcopy(student), fused_encoder=(k == "fused")) for k in ("fused", "pytorch")}
        runs = {"encoder_fused": (lambda: fused(stacked, mask, d_out), 10 * scale), "encoder_pytorch": (lambda: pytorch_grads(stacked, d_counting), 3 * scale),
                "step_fused": (lambda: trainers["fused"].step(obs, teacher), 3 * scale), "step_pytorch": (lambda: trainers["pytorch"].step(obs, teacher), 3 * scale)}
        for _ in range(3):
            for fn, _reps in runs.values():
                fn()
        t = {k: [] for k in runs}
        for _ in range(REPEATS):
            for k, (fn, reps) in runs.items():
                t[k].append(timed(fn, reps) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        flop = 2.0 * (MACS_FORWARD + MACS_BACKWARD) * n_counting
        doc["sizes"].append({"rows": rows, "mask": mask_name, "spheres": rows * 6, "counting_spheres": n_counting,
                             "grad_max_abs_fp64": float(ref64.abs().max()), "fused_grad_gap_to_fp64": gap_fused, "pytorch_fp32_grad_gap_to_fp64": gap_pytorch, "kinks_on_counting_spheres": kinks,
                             "encoder_fused_ms": stat(t["encoder_fused"]), "encoder_pytorch_ms": stat(t["encoder_pytorch"]),
                             "encoder_pytorch_over_fused": med["encoder_pytorch"] / med["encoder_fused"],
                             "encoder_fused_TFLOPS_on_counting_spheres": flop / med["encoder_fused"] / 1e9,
                             "encoder_fraction_of_fp32_mfma_peak": flop / med["encoder_fused"] / 1e9 / PEAK_TFLOPS,
                             "step_fused_ms": stat(t["step_fused"]), "step_pytorch_ms": stat(t["step_pytorch"]),
                             "step_pytorch_over_fused": med["step_pytorch"] / med["step_fused"]})
        print(json.dumps(doc["sizes"][-1]), file=sys.stderr, flush=True)
        del trainers, obs
    del stacked, real_mask, fused, d_out
    torch.cuda.empty_cache()
with open(os.path.join(ROOT, "profiles", "student_train.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc, indent=1))
