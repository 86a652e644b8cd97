"""The imitation dataset of the level5 student: the middle of the reference's line between its collector
(apps/threatsense_runner/collect_and_save.py: step Level5DumbMultiObs, drop the rows whose validity mask is all false) and its trainer
(SupervisedImitationTrainer._train_ppo, core/rl_framework/utils/sl_pipeline.py:172-207).

ImitationDataset is a ring of student rows (stacked_spheres, validity_mask, inertial_data, last_action, teacher action) in ONE device
buffer, filled by te_dataset_append from BatchedEnv.step_students' outputs as they are and sampled by te_dataset_gather into the
contiguous batch tensors StudentTrainer.step reads (dronechase_amd/csrc/te_dataset.hpp; the ABI is in include/threatengage.h).  A row is
24 434 bytes and never leaves HBM between the collector and the trainer; appending and sampling make no host read.
StudentTrainer.fit(dataset, ...) (student.py) is the reference's training loop on top, kill_high_correlation included.

to_dump / from_dump go through dump.ObservationDump and dump.load_part: the reference's file layout loads into the ring, and a ring
can be written out.  CUDA / ROCm only: there is no CPU form of the kernels."""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import config as K
from .student import OBS_KEYS

LAST_ACTION_MODES = {"keep": 0, "random": 1, "noise": 2}
NOISE_STD = 0.2                     # kill_high_correlation's alpha = 0.1: noise = randn * 2 * alpha
SPHERE_SHAPE = (K.LIDAR_CHANNELS, K.LIDAR_NTHETA, K.LIDAR_NPHI)


class ImitationDataset:
    """A ring of `capacity` student rows on `device`; `max_append_rows` bounds the rows of one append (N * P of the collector's env).

    append / append_students / collect enqueue two launches and read nothing back: the kept rows (active and any mask byte set, the
    collector's armed rows behind drop_invalid_student_obs) are placed in source-row order behind the rows already there, the oldest
    rows are overwritten once the ring is full.  size() and total() are the only host reads, 8 bytes each.  batch() gathers rows into
    fresh contiguous tensors: by `index` (slots; the caller keeps them below size()), or drawn on the device from (seed, draw).

    The typed views `stacked` [capacity, S, 3, 13, 26], `mask` [capacity, S] u8, `inertial` [capacity, 15], `last_action`,
    `teacher` [capacity, 4] alias the buffer `buf`; slot (total + k) mod capacity holds the k-th row appended after `total` others."""

    def __init__(self, capacity: int, device, max_append_rows: int, n_spheres: int = K.STACK_SPHERES):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ImitationDataset: device must be a GPU ('cuda:N'): the dataset is filled and sampled by the HIP kernels "
                             "te_dataset_append and te_dataset_gather, there is no CPU form")
        self.capacity, self.max_append_rows, self.n_spheres = int(capacity), int(max_append_rows), int(n_spheres)
        if not 1 <= self.capacity <= 2 ** 31 - 1:
            raise ValueError(f"ImitationDataset: capacity must be in 1 .. 2^31 - 1, not {capacity}")
        if not 1 <= self.max_append_rows <= self.capacity:
            raise ValueError(f"ImitationDataset: max_append_rows must be in 1 .. capacity ({self.capacity}), not {max_append_rows}")
        if not 1 <= self.n_spheres <= 8:
            raise ValueError(f"ImitationDataset: n_spheres must be in 1 .. 8, not {n_spheres}")
        self._geom = _lib.DatasetGeom(self.capacity, self.max_append_rows, self.n_spheres, SPHERE_SHAPE[0])
        o = self.offsets = _lib.DatasetOffsets()
        _lib.call("te_dataset_layout", C.byref(self._geom), C.byref(o))
        self.buf = torch.empty(int(o.bytes), dtype=torch.uint8, device=self.device)
        self.device = self.buf.device        # "cuda" -> "cuda:N": the device the callers' tensors report
        cap, S = self.capacity, self.n_spheres

        def view(at, dtype, *shape):
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            return self.buf[at:at + n].view(dtype).view(*shape)

        self._total = view(o.header, torch.int64, 1)
        self.stacked = view(o.stacked, torch.float32, cap, S, *SPHERE_SHAPE)
        self.mask = view(o.mask, torch.uint8, cap, S)
        self.inertial = view(o.inertial, torch.float32, cap, K.OBS_INERTIAL_WORDS)
        self.last_action = view(o.last_action, torch.float32, cap, 4)
        self.teacher = view(o.teacher, torch.float32, cap, 4)
        self.clear()

    # ------------------------------------------------------------------ plumbing
    def _args(self):
        return self.buf.data_ptr(), self.buf.numel(), C.byref(self._geom)

    def _rows(self, who: str, obs: Dict[str, torch.Tensor], teacher: torch.Tensor, active: Optional[torch.Tensor]):
        """The five row arrays and `active` as te_dataset_append reads them; M rows."""
        missing = [k for k in OBS_KEYS if k not in obs]
        if missing:
            raise ValueError(f"{who}: obs lacks {missing}: it must hold {list(OBS_KEYS)}")
        M, S = int(obs["stacked_spheres"].shape[0]) if obs["stacked_spheres"].dim() else 0, self.n_spheres
        if not 1 <= M <= self.max_append_rows:
            raise ValueError(f"{who}: {M} rows: an append takes 1 .. max_append_rows ({self.max_append_rows}) rows")
        _lib.require_f32(who, "stacked_spheres", obs["stacked_spheres"], (M, S, *SPHERE_SHAPE), self.device)
        _lib.require_f32(who, "inertial_data", obs["inertial_data"], (M, K.OBS_INERTIAL_WORDS), self.device)
        _lib.require_f32(who, "last_action", obs["last_action"], (M, 4), self.device)
        _lib.require_f32(who, "teacher", teacher, (M, 4), self.device)
        mask = _lib.require_bytes(who, "validity_mask", obs["validity_mask"], (M, S), self.device)
        if active is not None:
            active = _lib.require_bytes(who, "active", active, (M,), self.device)
        return M, obs["stacked_spheres"], mask, obs["inertial_data"], obs["last_action"], teacher, active

    # ------------------------------------------------------------------ filling
    def clear(self) -> None:
        """te_dataset_init: forget every row (the whole buffer is zeroed)."""
        _lib.call_on(self.device, "te_dataset_init", *self._args())

    def append(self, obs: Dict[str, torch.Tensor], teacher: torch.Tensor, active: Optional[torch.Tensor] = None) -> None:
        """obs: the four level5 keys as [M, ...] tensors on the device, teacher [M, 4] (may be obs["last_action"] itself), active [M]
        uint8 / bool or None (every row active).  The rows that are not kept may hold anything, NaN included.  No host read."""
        M, stacked, mask, inertial, last_action, teacher, active = self._rows("ImitationDataset.append", obs, teacher, active)
        _lib.call_on(self.device, "te_dataset_append", *self._args(), M, stacked.data_ptr(), mask.data_ptr(), inertial.data_ptr(),
                     last_action.data_ptr(), teacher.data_ptr(), _lib._ptr(active))

    def append_students(self, step_students_result) -> None:
        """BatchedEnv.step_students()'s tuple as it is: (stacked [N, P, S, 3, 13, 26], mask [N, P, S], inertial [N, P, 15], last_action
        [N, P, 4], active [N, P], ...).  The teacher's action of the all-scripted collector is the wingman's own command: last_action."""
        stacked, mask, inertial, last_action, active = step_students_result[:5]
        if stacked.dim() != 6:
            raise ValueError("ImitationDataset.append_students: stacked_spheres must be [N, P, S, 3, 13, 26], as BatchedEnv.step_students gives it")
        la = last_action.flatten(0, 1)
        self.append({"stacked_spheres": stacked.flatten(0, 1), "validity_mask": mask.flatten(0, 1), "inertial_data": inertial.flatten(0, 1),
                     "last_action": la}, la, active.flatten(0, 1))

    def collect(self, env, n_steps: int) -> None:
        """n_steps of env.step_students() (a BatchedEnv of an all-scripted stacked task: level5_dumb), each appended.  The env is
        stepped from where it stands (reset it first); nothing is read back."""
        for _ in range(int(n_steps)):
            self.append_students(env.step_students())

    # ------------------------------------------------------------------ reading
    def total(self) -> int:
        """The number of rows ever appended (one 8-byte host read)."""
        return int(self._total.item())

    def size(self) -> int:
        """The number of rows the ring holds: min(total, capacity) (one 8-byte host read)."""
        return min(self.total(), self.capacity)

    def batch(self, batch_size: int, index: Optional[torch.Tensor] = None, last_action_mode: str = "keep", seed: int = 0, draw: int = 0,
              noise_std: float = NOISE_STD, return_index: bool = False):
        """(obs dict of the four level5 keys, teacher [B, 4]) as fresh contiguous tensors; with return_index=True also the slots used
        (int64 [B]; -1 from an empty ring).  index: int64 [B] slots on the device (values outside the ring are clamped into it; below
        size() is the caller's business), or None: row j draws its slot on the device from Philox(seed, draw, j) and the ring's size,
        so no host read is needed; an empty ring gives zeros.  last_action_mode is kill_high_correlation's branch for this batch: "keep",
        "random" (uniform in [-1, 1)) or "noise" (+ noise_std * N(0, 1), clamped to [-1, 1]), drawn from the same (seed, draw)."""
        who = "ImitationDataset.batch"
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"{who}: batch_size must be >= 1, not {batch_size}")
        if last_action_mode not in LAST_ACTION_MODES:
            raise ValueError(f"{who}: last_action_mode must be one of {list(LAST_ACTION_MODES)}, not {last_action_mode!r}")
        if not float(noise_std) >= 0.0:
            raise ValueError(f"{who}: noise_std must be >= 0, not {noise_std}")
        if index is not None:
            _lib.require_index(who, index, self.device)
            if index.numel() != B:
                raise ValueError(f"{who}: index has {index.numel()} entries, batch_size is {B}")
        S, dev = self.n_spheres, self.device
        obs = {"stacked_spheres": torch.empty((B, S, *SPHERE_SHAPE), dtype=torch.float32, device=dev),
               "validity_mask": torch.empty((B, S), dtype=torch.uint8, device=dev),
               "inertial_data": torch.empty((B, K.OBS_INERTIAL_WORDS), dtype=torch.float32, device=dev),
               "last_action": torch.empty((B, 4), dtype=torch.float32, device=dev)}
        teacher = torch.empty((B, 4), dtype=torch.float32, device=dev)
        used = torch.empty((B,), dtype=torch.int64, device=dev) if return_index else None
        mask64 = (1 << 64) - 1
        _lib.call_on(dev, "te_dataset_gather", *self._args(), B, _lib._ptr(index), int(seed) & mask64, int(draw) & mask64,
                     LAST_ACTION_MODES[last_action_mode], float(noise_std), obs["stacked_spheres"].data_ptr(), obs["validity_mask"].data_ptr(),
                     obs["inertial_data"].data_ptr(), obs["last_action"].data_ptr(), teacher.data_ptr(), _lib._ptr(used))
        return (obs, teacher, used) if return_index else (obs, teacher)

    def logical_index(self) -> torch.Tensor:
        """The slots of the ring's rows, oldest first (int64 [size] on the device; one host read, of total)."""
        total = self.total()
        size = min(total, self.capacity)
        return (torch.arange(size, dtype=torch.int64, device=self.device) + (total - size)) % self.capacity

    # ------------------------------------------------------------------ files
    def to_dump(self, directory: str, rows_per_file: int = 1000, use_hdf5: Optional[bool] = None, chunk: int = 1024):
        """Write the ring's rows, oldest first, as dump.ObservationDump part files (the reference collector's layout); returns the
        closed ObservationDump.  The rows travel to the host `chunk` at a time."""
        from .dump import ObservationDump
        out = ObservationDump(directory, rows_per_file=rows_per_file, use_hdf5=use_hdf5)
        order = self.logical_index()
        for at in range(0, int(order.numel()), int(chunk)):
            idx = order[at:at + int(chunk)].contiguous()
            obs, teacher = self.batch(int(idx.numel()), index=idx)
            out.add(obs, teacher)
        out.close()
        return out

    @classmethod
    def from_dump(cls, directory: str, device, capacity: Optional[int] = None, max_append_rows: int = 1024, n_spheres: int = K.STACK_SPHERES):
        """A dataset holding the rows of every part file in `directory` (part0, part1, ... of dump.ObservationDump or of the
        reference's collector, .npz or .h5), in file order.  capacity: the ring's (default: the number of rows in the files); a smaller one keeps
        the newest rows."""
        from .dump import load_part
        names = sorted((f for f in os.listdir(directory) if re.fullmatch(r"part\d+\.(npz|h5)", f)), key=lambda f: int(re.findall(r"\d+", f)[0]))
        if not names:
            raise ValueError(f"ImitationDataset.from_dump: no part files (partK.npz / partK.h5) in {directory}")
        parts = [load_part(os.path.join(directory, f)) for f in names]
        rows = sum(len(p["teacher_actions"]) for p in parts)
        capacity = max(rows, 1) if capacity is None else int(capacity)
        ds = cls(capacity, device, min(int(max_append_rows), capacity), n_spheres)
        for p in parts:
            for at in range(0, len(p["teacher_actions"]), ds.max_append_rows):
                cut = slice(at, at + ds.max_append_rows)
                obs = {k: torch.from_numpy(np.ascontiguousarray(p[f"student/{k}"][cut])).to(ds.device) for k in OBS_KEYS}
                ds.append(obs, torch.from_numpy(np.ascontiguousarray(p["teacher_actions"][cut], dtype=np.float32)).to(ds.device))
        return ds


def last_action_mode(p: float) -> str:
    """kill_high_correlation's branch for a batch from its uniform draw p (sl_pipeline.py): p < 0.2 replaces last_action by uniform
    noise, p < 0.6 keeps it, anything else adds Gaussian noise."""
    return "random" if p < 0.2 else "keep" if p < 0.6 else "noise"
