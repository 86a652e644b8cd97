"""The imitation dataset restated in numpy: te_dataset_append's keep rule and ring placement, te_dataset_gather's Philox slots and its
three last_action branches (include/threatengage.h), on the oracle's Philox.  The reference of tests/test_gpu_imitation_dataset.py; its
own properties are checked without a GPU in tests/test_imitation_dataset.py.

Synthetic rows: every float of pool row `i` is a distinct number in [0.5, 1) whose bits hold (i mod 1021, the float's position in the
row), so a row that lands in the wrong slot, or is assembled from two rows, or is shifted by a float, differs somewhere."""
import functools

import numpy as np

from oracle import te_oracle as O

SPHERE = (3, 13, 26)
SPHERE_FLOATS = 3 * 13 * 26
FIELDS = ("stacked", "mask", "inertial", "last_action", "teacher")
NOISE_STD = np.float32(0.2)


def row_bytes(n_spheres):
    return n_spheres * SPHERE_FLOATS * 4 + n_spheres + (15 + 4 + 4) * 4


def layout(capacity, max_append_rows, n_spheres):
    """te_dataset_layout by hand: a 64-byte header, then every array at the next multiple of 16."""
    sizes = [("dst", max_append_rows * 4), ("stacked", capacity * n_spheres * SPHERE_FLOATS * 4), ("mask", capacity * n_spheres),
             ("inertial", capacity * 15 * 4), ("last_action", capacity * 4 * 4), ("teacher", capacity * 4 * 4)]
    at, out = 64, {"header": 0}
    for name, n in sizes:
        out[name] = at
        at = (at + n + 15) // 16 * 16
    out["bytes"] = at
    return out, dict(sizes)


def coded(row_ids, first, count):
    """float32 [len(row_ids), count]: bits 0x3F000000 | (id mod 1021) << 13 | (first + k)."""
    ids = (np.asarray(row_ids, np.int64) % 1021).astype(np.uint32)[:, None]
    pos = np.arange(first, first + count, dtype=np.uint32)[None, :]
    assert first + count <= 8192
    return (np.uint32(0x3F000000) | (ids << np.uint32(13)) | pos).view(np.float32)


def rows(row_ids, n_spheres=6, mask_seed=0):
    """Pool rows `row_ids` (any integers): every mask has at least one non-zero byte (of value 1, 2 or 255), last_action is negative on
    odd ids."""
    ids = np.asarray(row_ids, np.int64)
    n, words = len(ids), n_spheres * SPHERE_FLOATS
    rng = np.random.default_rng(mask_seed)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=(n, n_spheres))
    mask[np.arange(n), rng.integers(0, n_spheres, n)] = 1
    sign = np.where(ids % 2 == 1, np.float32(-1), np.float32(1))[:, None]
    return {"stacked": coded(ids, 0, words).reshape(n, n_spheres, *SPHERE), "mask": mask, "inertial": coded(ids, 8130, 15),
            "last_action": coded(ids, 8150, 4) * sign, "teacher": coded(ids, 8160, 4)}


def with_pattern(pool, keep, inactive_but_valid=(), active_but_empty=()):
    """(rows, active): the rows of `pool` where keep, the others not kept and full of NaN: inactive with a zero mask, except
    `inactive_but_valid` (active = 0, the mask left on) and `active_but_empty` (active = 1, the mask all zero)."""
    keep = np.asarray(keep, bool)
    out = {k: v.copy() for k, v in pool.items()}
    active = keep.astype(np.uint8)
    drop = ~keep
    for k in ("stacked", "inertial", "last_action", "teacher"):
        out[k][drop] = np.nan
    out["mask"][drop] = 0
    for i in inactive_but_valid:
        assert drop[i]
        out["mask"][i] = pool["mask"][i]
    for i in active_but_empty:
        assert drop[i]
        active[i] = 1
    return out, active


def keep_rule(mask, active=None):
    """te_dataset_append's: active != 0 and any mask byte != 0."""
    k = (np.asarray(mask) != 0).any(axis=1)
    return k if active is None else k & (np.asarray(active) != 0)


class Ring:
    """The dataset's rings and `total` on the host."""

    def __init__(self, capacity, n_spheres=6):
        self.capacity, self.n_spheres, self.total = capacity, n_spheres, 0
        self.a = {"stacked": np.zeros((capacity, n_spheres, *SPHERE), np.float32), "mask": np.zeros((capacity, n_spheres), np.uint8),
                  "inertial": np.zeros((capacity, 15), np.float32), "last_action": np.zeros((capacity, 4), np.float32),
                  "teacher": np.zeros((capacity, 4), np.float32)}

    @property
    def size(self):
        return min(self.total, self.capacity)

    def append(self, r, active=None):
        keep = np.flatnonzero(keep_rule(r["mask"], active))
        slots = (self.total + np.arange(len(keep))) % self.capacity
        for k in FIELDS:
            self.a[k][slots] = r[k][keep]        # one append keeps at most capacity rows: the slots are distinct
        self.total += len(keep)
        return slots


@functools.lru_cache(maxsize=None)
def _philox_words(n, seed, draw, purpose):
    key = (seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([O.philox((j, draw & 0xFFFFFFFF, draw >> 32, purpose), key) for j in range(n)])


def philox_slots(batch, size, seed, draw):
    """slot_j = mulhi32(w.x, size), w = philox4x32_10((j, draw_lo, draw_hi, 1), (seed_lo, seed_hi)); -1 from an empty ring."""
    if size == 0:
        return np.full(batch, -1, np.int64)
    w0 = _philox_words(batch, seed, draw, 1)[:, 0].astype(np.uint64)
    return ((w0 * np.uint64(size)) >> np.uint64(32)).astype(np.int64)


def la_random(batch, seed, draw):
    """Mode 1 in float32 arithmetic, and the same in float64: the two must agree bit for bit (every step is exact)."""
    u = (_philox_words(batch, seed, draw, 2) >> np.uint32(8))
    f32 = u.astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1)
    f64 = u.astype(np.float64) * 2.0 ** -23 - 1.0
    return f32, f64


def normals(batch, seed, draw):
    """z [batch, 4] float64: the two Box-Muller pairs of mode 2."""
    u = (_philox_words(batch, seed, draw, 2) >> np.uint32(8)).astype(np.float64)
    z = np.empty((batch, 4))
    for a in (0, 2):
        u1, u2 = (u[:, a] + 1.0) * 2.0 ** -24, u[:, a + 1] * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, a], z[:, a + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return z


def la_noise(la, seed, draw, noise_std=NOISE_STD):
    """Mode 2 in float64 on the float32 inputs (la as stored, noise_std as the ABI's float carries it)."""
    la = np.asarray(la, np.float32)
    return np.clip(la.astype(np.float64) + float(np.float32(noise_std)) * normals(len(la), seed, draw), -1.0, 1.0)
