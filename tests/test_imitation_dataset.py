"""te_dataset_* and dronechase_amd.imitation without a GPU: the ABI's declarations, te_dataset_layout against sizes computed by hand,
the host-side refusals of all four calls (they return before anything is launched: the pointers are fake and never dereferenced), the
properties of the numpy restatement in tests/_dataset_cases.py the GPU tests lean on, and the Python front-end's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _dataset_cases as D

FAKE = 1 << 20          # never dereferenced: every call below fails a check first
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "threatengage.h")
NAMES = ("te_dataset_layout", "te_dataset_init", "te_dataset_append", "te_dataset_gather")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _geom(capacity=1000, max_append_rows=100, n_spheres=6, channels=3):
    from dronechase_amd import _lib
    return _lib.DatasetGeom(capacity, max_append_rows, n_spheres, channels)


def test_header_declares_and_the_binding_exports_every_entry(lib):
    from dronechase_amd import _lib, build
    with open(HEADER) as f:
        body = f.read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert lib.te_abi_version() == 5
    assert "te_dataset.hpp" in {os.path.basename(d) for d in build.deps()}
    assert C.sizeof(_lib.DatasetOffsets) == 8 * C.sizeof(C.c_size_t) and C.sizeof(_lib.DatasetGeom) == 16


@pytest.mark.parametrize("capacity,max_append_rows,n_spheres", [(1, 1, 1), (32, 21, 6), (1000, 7, 5), (14336, 14336, 6), (180000, 21, 6),
                                                                (2 ** 31 - 1, 2 ** 31 - 1, 8)])
def test_layout_is_aligned_ordered_disjoint_and_sized_by_hand(lib, capacity, max_append_rows, n_spheres):
    from dronechase_amd import _lib
    o = _lib.DatasetOffsets()
    assert lib.te_dataset_layout(C.byref(_geom(capacity, max_append_rows, n_spheres)), C.byref(o)) == 0, lib.te_last_error()
    want, sizes = D.layout(capacity, max_append_rows, n_spheres)
    got = {k: getattr(o, k) for k in ("header", "dst", "stacked", "mask", "inertial", "last_action", "teacher", "bytes")}
    assert got == want
    order = ["dst", "stacked", "mask", "inertial", "last_action", "teacher"]
    assert got["header"] == 0 and got["dst"] >= 64
    for name, nxt in zip(order, order[1:] + ["bytes"]):
        assert got[name] % 16 == 0 and got[name] + sizes[name] <= got[nxt], (name, nxt)
    assert got["bytes"] % 16 == 0 and got["bytes"] - (64 + sum(sizes.values())) < 16 * len(order)
    if n_spheres == 6:
        assert sizes["stacked"] + sizes["mask"] + sizes["inertial"] + sizes["last_action"] + sizes["teacher"] == capacity * 24434 == capacity * D.row_bytes(6)


GEOM_REFUSALS = [(dict(channels=2), b"channels must be 3, not 2"), (dict(n_spheres=0), b"n_spheres must be in 1 .. 8, not 0"),
                 (dict(n_spheres=9), b"n_spheres must be in 1 .. 8, not 9"), (dict(capacity=0), b"capacity must be in 1 .. 2^31 - 1, not 0"),
                 (dict(capacity=-5), b"capacity must be in 1 .. 2^31 - 1"), (dict(max_append_rows=0), b"max_append_rows must be in 1 .. capacity"),
                 (dict(max_append_rows=1001), b"max_append_rows must be in 1 .. capacity (1000), not 1001")]


def _refused(lib, fn, args, who, msg):
    assert getattr(lib, fn)(*args) != 0, (fn, msg)
    err = lib.te_last_error()
    assert err.startswith(who.encode() + b": ") and msg in err, (fn, msg, err)


def test_layout_refusals(lib):
    from dronechase_amd import _lib
    o = _lib.DatasetOffsets()
    for kw, msg in GEOM_REFUSALS:
        _refused(lib, "te_dataset_layout", (C.byref(_geom(**kw)), C.byref(o)), "te_dataset_layout", msg)
    _refused(lib, "te_dataset_layout", (None, C.byref(o)), "te_dataset_layout", b"null argument geom")
    _refused(lib, "te_dataset_layout", (C.byref(_geom()), None), "te_dataset_layout", b"null argument out")


def _bytes(lib, **kw):
    from dronechase_amd import _lib
    o = _lib.DatasetOffsets()
    assert lib.te_dataset_layout(C.byref(_geom(**kw)), C.byref(o)) == 0
    return o.bytes


def _buffer_refusals(need):
    return [(dict(ds=None), b"null argument ds"), (dict(ds=FAKE + 8), b"ds must be 16-byte aligned"),
            (dict(bytes=need - 1), b"ds too small"), (dict(bytes=0), b"te_dataset_layout says " + str(need).encode())]


def test_init_refusals_come_from_the_host(lib):
    need = _bytes(lib)
    base = dict(ds=FAKE, bytes=need, geom=None, stream=None)
    for kw, msg in _buffer_refusals(need) + [(dict(geom=kw), msg) for kw, msg in GEOM_REFUSALS]:
        a = dict(base, **kw)
        a["geom"] = C.byref(_geom(**(a["geom"] or {})))
        _refused(lib, "te_dataset_init", list(a.values()), "te_dataset_init", msg)
    _refused(lib, "te_dataset_init", [FAKE, need, None, None], "te_dataset_init", b"null argument geom")


def test_append_refusals_come_from_the_host(lib):
    need = _bytes(lib)
    base = dict(ds=FAKE, bytes=need, geom=None, n_rows=100, stacked=FAKE, mask=FAKE, inertial=FAKE, last_action=FAKE, teacher=FAKE, active=None,
                stream=None)
    cases = _buffer_refusals(need) + [(dict(geom=kw), msg) for kw, msg in GEOM_REFUSALS]
    cases += [(dict(n_rows=101), b"n_rows must be in 1 .. max_append_rows (100), not 101"), (dict(n_rows=0), b"n_rows must be in 1 .. max_append_rows"),
              (dict(n_rows=-3), b"n_rows must be in 1 .. max_append_rows"), (dict(stacked=FAKE + 4), b"stacked must be 16-byte aligned"),
              (dict(inertial=FAKE + 2), b"inertial must be 4-byte aligned"), (dict(last_action=FAKE + 1), b"last_action must be 4-byte aligned"),
              (dict(teacher=FAKE + 3), b"teacher must be 4-byte aligned")]
    cases += [({name: None}, b"null argument " + name.encode()) for name in ("stacked", "mask", "inertial", "last_action", "teacher")]
    for kw, msg in cases:
        a = dict(base, **kw)
        a["geom"] = C.byref(_geom(**(a["geom"] or {})))
        _refused(lib, "te_dataset_append", list(a.values()), "te_dataset_append", msg)


def test_gather_refusals_come_from_the_host(lib):
    need = _bytes(lib)
    base = dict(ds=FAKE, bytes=need, geom=None, batch=8, index=None, seed=1, draw=2, mode=0, noise_std=0.2, out_stacked=FAKE, out_mask=FAKE,
                out_inertial=FAKE, out_last_action=FAKE, out_teacher=FAKE, out_index=None, stream=None)
    cases = _buffer_refusals(need) + [(dict(geom=kw), msg) for kw, msg in GEOM_REFUSALS]
    cases += [(dict(batch=0), b"batch must be >= 1, not 0"), (dict(batch=-1), b"batch must be >= 1"),
              (dict(mode=3), b"last_action_mode must be 0 (keep), 1 (random) or 2 (noise), not 3"), (dict(mode=-1), b"last_action_mode must be"),
              (dict(noise_std=-0.5), b"noise_std must be finite and >= 0"), (dict(noise_std=float("nan")), b"noise_std must be finite and >= 0"),
              (dict(noise_std=float("inf")), b"noise_std must be finite and >= 0"),
              (dict(index=FAKE + 4), b"index must be 8-byte aligned"), (dict(out_index=FAKE + 4), b"out_index must be 8-byte aligned"),
              (dict(out_stacked=FAKE + 8), b"out_stacked must be 16-byte aligned"), (dict(out_inertial=FAKE + 2), b"out_inertial must be 4-byte aligned")]
    cases += [({name: None}, b"null argument " + name.encode()) for name in ("out_stacked", "out_mask", "out_inertial", "out_last_action", "out_teacher")]
    for kw, msg in cases:
        a = dict(base, **kw)
        a["geom"] = C.byref(_geom(**(a["geom"] or {})))
        _refused(lib, "te_dataset_gather", list(a.values()), "te_dataset_gather", msg)


def test_mode_1_is_exact_in_fp32():
    f32, f64 = D.la_random(4096, seed=0x1234_5678_9ABC_DEF0, draw=3)
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), f64)
    assert f32.min() >= -1.0 and f32.max() < 1.0 and len(np.unique(f32)) > 16000
    # the extremes of u: 0 and 2^24 - 1
    for u, want in ((0, -1.0), (2 ** 24 - 1, 1.0 - 2.0 ** -23)):
        assert float(np.float32(u) * np.float32(2.0 ** -23) - np.float32(1)) == want


def test_the_restatements_noise_is_standard_normal():
    z = D.normals(8192, seed=11, draw=5)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.8          # sqrt(-2 ln 2^-24) = 5.77
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.std() - 1.0) < 5 / np.sqrt(2 * n)
    la = np.zeros((8192, 4), np.float32)
    noise = D.la_noise(la, 11, 5)
    assert np.abs(noise).max() <= 0.2 * 5.8 and ((noise >= -1) & (noise <= 1)).all()
    assert not np.array_equal(z, D.normals(8192, seed=11, draw=6))


def test_philox_slots_cover_the_ring_and_nothing_else():
    for size in (1, 7, 80, 2 ** 31 - 1):
        s = D.philox_slots(4096, size, seed=9, draw=1)
        assert s.min() >= 0 and s.max() < size
    assert len(np.unique(D.philox_slots(4096, 80, 9, 1))) == 80
    assert (D.philox_slots(16, 0, 9, 1) == -1).all()


def test_the_keep_rule_is_observation_dumps(tmp_path):
    from dronechase_amd import dump
    pool = D.rows(range(200))
    rng = np.random.default_rng(4)
    r, active = D.with_pattern(pool, rng.random(200) < 0.6)
    assert np.array_equal(D.keep_rule(r["mask"], active), D.keep_rule(r["mask"]))   # the pattern's inactive rows have zero masks
    d = dump.ObservationDump(str(tmp_path), rows_per_file=10 ** 6, use_hdf5=False)
    kept = d.add({"stacked_spheres": r["stacked"], "validity_mask": r["mask"], "inertial_data": r["inertial"], "last_action": r["last_action"]},
                 r["teacher"])
    d.close()
    keep = D.keep_rule(r["mask"], active)
    assert kept == keep.sum() > 0
    part = dump.load_part(d.files[0])
    assert np.array_equal(part["student/stacked_spheres"].view(np.uint32), r["stacked"][keep].view(np.uint32))
    assert np.array_equal(part["teacher_actions"].view(np.uint32), r["teacher"][keep].view(np.uint32))
    # the ring on the host places them in that order
    ring = D.Ring(32)
    slots = ring.append({k: v[:21] for k, v in r.items()}, active[:21])
    assert list(slots) == list(range(keep[:21].sum())) and ring.total == keep[:21].sum()
    # active matters on its own: an armed row needs a mask, a masked row needs to be armed
    assert not D.keep_rule(np.array([[0, 0]]), np.array([1]))[0] and not D.keep_rule(np.array([[0, 7]]), np.array([0]))[0]
    assert D.keep_rule(np.array([[0, 7]]), np.array([2]))[0]


def test_synthetic_rows_are_all_different():
    r = D.rows(range(1021), n_spheres=8)
    flat = np.concatenate([r["stacked"].reshape(1021, -1), r["inertial"], np.abs(r["last_action"]), r["teacher"]], axis=1)
    assert len(np.unique(flat.view(np.uint32))) == flat.size and flat.min() >= 0.5 and flat.max() < 1.0
    assert (r["mask"] != 0).any(axis=1).all() and (r["last_action"][1] < 0).all() and (r["last_action"][0] > 0).all()


def test_the_front_end_refuses_a_cpu():
    from dronechase_amd.imitation import ImitationDataset, last_action_mode
    from dronechase_amd.student import FLIAStudent, StudentTrainer
    with pytest.raises(ValueError, match="device must be a GPU.*te_dataset_append"):
        ImitationDataset(100, "cpu", 10)
    with pytest.raises(ValueError, match="dataset must be an imitation.ImitationDataset"):
        StudentTrainer(FLIAStudent()).fit({"stacked_spheres": torch.zeros(4, 6, 3, 13, 26)})
    assert [last_action_mode(p) for p in (0.0, 0.19, 0.2, 0.59, 0.6, 0.99)] == ["random", "random", "keep", "keep", "noise", "noise"]
