"""Shared by tests/golden/gen_student_flia.py (which runs the reference's StudentWithFLIA) and the student tests: the seeded weight
recipe, the fixture's inputs, and the tolerance.  The reference network has 4 265 412 parameters (17 MB), too large to commit, so the
fixture holds results only and both sides rebuild the same weights from this recipe."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "student_flia.npz")
KEYS = os.path.join(GOLDEN, "student_flia_keys.json")

SEED = 20261021
GAIN = 2.0            # on 1 / sqrt(fan_in): with torch's default init the 8 output rows are nearly identical and would hide a wrong mask rule
MASKS = ("000000", "100000", "000001", "111111", "110010", "011100", "101010", "001000")
CONV_SPHERES = ((1, 0), (3, 5), (4, 1), (6, 2))      # (row, slot) of the four spheres whose conv stack the fixture holds
RTOL = ATOL = 1e-4    # |d| <= 1e-4 + 1e-4 |ref|: the bound of tests/test_policy_fused.py for fp32 kernels against a reference


def keys_and_shapes():
    with open(KEYS) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def recipe_weights(keys_shapes, seed=SEED):
    """{name: float64 array}: numpy.random.default_rng(seed), one draw per tensor in key order.  A weight is normal * GAIN /
    sqrt(fan_in) (fan_in = the product of its dimensions after the first), a bias normal * 0.1, a LayerNorm gain 1 + 0.1 * normal."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in keys_shapes:
        x = rng.standard_normal(shape)
        if name.endswith("layer_norm.weight"):
            x = 1.0 + 0.1 * x
        elif name.endswith("bias"):
            x = 0.1 * x
        else:
            x = x * (GAIN / np.sqrt(np.prod(shape[1:])))
        out[name] = x
    return out


def mask_array():
    return np.array([[int(c) for c in m] for m in MASKS], np.uint8)


def counting(mask):
    """The spheres the network looks at: mask != 0, or sphere 0 of a row whose mask is all zero."""
    c = mask != 0
    c[:, 0] |= ~c.any(axis=1)
    return c


def fixture_inputs(seed=SEED + 1):
    """The 8 rows: LIDAR-like cells in [0, 1], inertial rows ~ N(0, 1), last actions in [-1, 1]."""
    rng = np.random.default_rng(seed)
    n = len(MASKS)
    return {"stacked_spheres": rng.uniform(0.0, 1.0, (n, 6, 3, 13, 26)), "validity_mask": mask_array(),
            "inertial_data": rng.standard_normal((n, 15)), "last_action": rng.uniform(-1.0, 1.0, (n, 4))}


def loss_pairs(seed=SEED + 2):
    """Three (pred, target) batches for loss_mae_direction: generic, nearly opposite directions, and a zero direction row."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((16, 4)), rng.standard_normal((16, 4)))
    t = rng.standard_normal((8, 4))
    b = (-t + 0.01 * rng.standard_normal((8, 4)), t)
    p = rng.standard_normal((4, 4)); p[0, :3] = 0.0
    c = (p, rng.standard_normal((4, 4)))
    return [a, b, c]


def within(got, ref):
    """(ok, max |d|, max |d| / (ATOL + RTOL |ref|)) of got against ref."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    ratio = d / (ATOL + RTOL * np.abs(ref))
    return bool(np.all(np.isfinite(got)) and ratio.max() <= 1.0), float(d.max()), float(ratio.max())
