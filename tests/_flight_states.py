"""Crafted flight states for the paths of the sub-step that no rollout reaches (te_device.hpp substep(): the general attitude read, the
gimbal guard, the fast-rotation update), and the bookkeeping that holds the kernel to the oracle there.

Families (every one writes QUAT, OMEGA and VEL of EVERY armed drone of every env, so a slot flies them whatever its mode):
  central     40 oracle steps out of reset: what every rollout of the suite flies (tilt < 0.25 rad)
  tilted      roll +-U(0.5, 1.2), pitch +-U(0.6, 1.2): both inverse functions off their central branch
  inverted    roll +-U(2, 3), pitch +-0.4: R22 < 0, the x < 0 and ay > ax selects of atan2
  near_guard  pitch +-(pi/2 - U(0.1, 0.3)): asin's square-root branch, never the guard.  (Not U(0.02, 0.3): roll and yaw carry the rounding of the
              rotation matrix times 1 / cos(pitch), up to 50 there, and with that heavy a tail the pair's maximum and the kernel's sit on a handful
              of drones each: after 16 sub-steps the agents' attitude row missed 4 G at 5.8e-6 against G = 1.2e-6 on the MI355X while the same
              drones passed inside OBS_EULER, whose G comes from three times as many.  From 0.1 on the factor is 3 to 10 for every drone.)
  guard       pitch +-(pi/2 - U(0, 0.004)), slow: |sarg| >= 0.99999, roll = 0, yaw by the double angle of (q.x, q.y)
  spin        |omega| = U(245, 300) rad/s: (dt |w| / 2)^2 >= 0.25, the native sin / cos in revolutions
Every family draws yaw U(-3, 3), omega U(-2, 2)^3 unless it says otherwise, and VEL as BODY-frame components +-U(1.2, 2) each, rotated into the
world frame.  Why the velocity is not U(-2, 2)^3 in the world frame: the velocity loop's derivative term (kd / T = 60 next to kp = 0.8) leaves
its +-0.4 clamp only while |set-point - body velocity| < 0.0065 m/s, and inside that window the commanded rate is 2 x 61 times the rounding of
the body velocity.  With world-frame U(-2, 2)^3 two or three of 768 drones land in the window, the pair's largest PID_AV_E gap is the
maximum over those two or three (2.1e-6 for `inverted` at one sub-step, 4.5e-5 for `tilted`), and a correct kernel missed 4 G at 1.7e-5 on one of
them (MI355X; its body velocity differed from float64 by 1.4e-7, two ulps).  Body components of at least 1.2 m/s keep every drone whose set-point is at
most 1 m/s (all but stage01's mode-7 slot) out of the window at the first controller sub-step: away from the ill-conditioning, not from any of
the attitude or rotation paths, which do not look at the velocity.  The window itself is what every rollout of the suite flies through.
The builders are deterministic: numpy.random.default_rng seeded per (family, task).

The bounds of the GPU test come from the oracle's own float32 / float64 pair on the same inputs (pair(), gaps(), G / NEAR below), never from
the kernel; drones whose guard decision sits within 1e-6 of the threshold (OracleEnv.flight_census) are left out, and so are envs in which
a discrete decision that changes state or done sat within 1e-4 of its threshold (OracleEnv.state_margins; integer words, done and info
follow OracleEnv.margins, the rule of tests/test_gpu_parity.py)."""
import functools
import zlib

import numpy as np

from dronechase_amd import config as K
from oracle import te_oracle as O

N_ENVS = 256          # four waves of lanes per slot
SEED = 17
ACTION_SEED = 5
GUARD_MARGIN = 1e-6   # ~16 float32 ulps of sarg, against a guard band 1e-5 wide
MARGIN = 1e-4         # discrete decisions (tests/test_gpu_parity.py)
ULP_FLOOR = 16 * 2.0 ** -24
FAMILIES = ("tilted", "inverted", "near_guard", "guard", "spin")
SUBSTEPS = {"tilted": (1, 2, 16), "inverted": (1, 2, 16), "near_guard": (1, 2, 16), "guard": (1, 2), "spin": (1,)}
INTENDED = {"tilted": O.CENSUS_GENERAL, "inverted": O.CENSUS_GENERAL, "near_guard": O.CENSUS_GENERAL, "guard": O.CENSUS_GUARD,
            "spin": O.CENSUS_FAST}

# word groups of a drone record that are compared (SETPOINT / FORMATION / PENDING are inputs or logic words held by other tests)
GROUPS = {name: (K.D[name], n) for name, n in (
    ("POS", 3), ("QUAT", 4), ("VEL", 3), ("OMEGA", 3), ("THROTTLE", 4), ("PID_AV_I", 3), ("PID_AV_E", 3), ("PID_LV_I", 2), ("PID_LV_E", 2),
    ("PID_ZV_I", 1), ("PID_ZV_E", 1), ("OBS_POS", 3), ("OBS_EULER", 3), ("OBS_VEL", 3), ("OBS_RATE", 3))}
# the agent's inertial observation row (normalised position, velocity, attitude / pi, rates / 2 pi, gun state)
INERTIAL_GROUPS = {"INERTIAL_POS": (0, 3), "INERTIAL_VEL": (3, 3), "INERTIAL_EULER": (6, 3), "INERTIAL_RATE": (9, 3), "INERTIAL_GUN": (12, 3)}
ALL_GROUPS = tuple(GROUPS) + tuple(INERTIAL_GROUPS)


def config(task, substeps=16, noise=0, **over):
    return O.default_config(task, n_envs=N_ENVS, seed=SEED, motor_noise=noise, substeps=substeps, **over)


def _quat_of_euler(roll, pitch, yaw):
    """getQuaternionFromEuler (ZYX), (x, y, z, w), float64."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _norm2_f32(q):
    """|q|^2 as the kernel's prologue computes it: fma(w, w, fma(z, z, fma(y, y, x * x))) in float32 (products of float32 are exact in float64)."""
    q = q.astype(np.float32).astype(np.float64)
    d = (q[..., 0] * q[..., 0]).astype(np.float32)
    for i in (1, 2, 3):
        d = (q[..., i] * q[..., i] + d.astype(np.float64)).astype(np.float32)
    return d


def _unit_in_float32(q):
    """The float32 quaternion next to `q` (a few ulps per component) whose float32 |q|^2 is exactly 1.  The kernel normalises
    every quaternion that comes in through te_set_state (fly(): b.q * rsq(|q|^2)); on such a quaternion that is the identity, so the kernel and
    both oracle builds start from the same float32 attitude.  Otherwise the kernel flies a state up to an ulp per component away from the
    oracle's, a difference the float32 / float64 pair cannot know and which near the guard is amplified by 1 / cos(pitch) (up to 50 here)."""
    q = q.astype(np.float32).copy()
    order = np.argsort(-np.abs(q), axis=-1)
    ks = list(range(1, 33)) + list(range(40, 257, 8)) + list(range(320, 4097, 64))
    for k in (k * sgn for k in ks for sgn in (1, -1)):      # k ulps on one component (at most 1e-6), the fewest and the largest component first
        if (_norm2_f32(q) == 1.0).all():
            break
        for rank in range(4):
            idx = order[..., rank:rank + 1]
            v = np.take_along_axis(q, idx, -1)
            c = (v.view(np.int32) + k).view(np.float32)
            trial = q.copy()
            np.put_along_axis(trial, idx, c, -1)
            take = (_norm2_f32(q) != 1.0) & (_norm2_f32(trial) == 1.0) & (np.abs(c.astype(np.float64) - v)[..., 0] <= 1e-6)
            q[take] = trial[take]
    for at in map(tuple, np.argwhere(_norm2_f32(q) != 1.0)):   # the rest: a few ulps on several components at once
        bits = q[at].view(np.int32).astype(np.int64)
        hits = [o for o in np.ndindex(9, 9, 9, 9) if _norm2_f32((bits + (np.array(o) - 4)).astype(np.int32).view(np.float32)) == 1.0]
        q[at] = (bits + (np.array(min(hits, key=lambda o: np.abs(np.array(o) - 4).sum())) - 4)).astype(np.int32).view(np.float32)
    assert (_norm2_f32(q) == 1.0).all()
    return q


def _matrix_of_quat(q):
    x, y, z, w = (q[..., i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


@functools.lru_cache(maxsize=None)
def draws(family, task, D):
    """(quat [N,D,4], omega [N,D,3] world frame, vel [N,D,3]) of `family`, the same for every call with the same (family, task); shared, read-only."""
    rng = np.random.default_rng(zlib.crc32(f"{family}/{task}".encode()))
    shape = (N_ENVS, D)
    sign = lambda: rng.choice([-1.0, 1.0], shape)
    u = lambda lo, hi, s=shape: rng.uniform(lo, hi, s)
    yaw, omega = u(-3, 3), u(-2, 2, shape + (3,))
    vel_body = rng.choice([-1.0, 1.0], shape + (3,)) * u(1.2, 2.0, shape + (3,))   # (see VEL in the module's docstring)
    if family == "tilted":
        roll, pitch = sign() * u(0.5, 1.2), sign() * u(0.6, 1.2)
    elif family == "inverted":
        roll, pitch = sign() * u(2, 3), sign() * 0.4
    elif family == "near_guard":
        roll, pitch = u(-0.5, 0.5), sign() * (np.pi / 2 - u(0.1, 0.3))
    elif family == "guard":
        roll, pitch, omega = u(-0.5, 0.5), sign() * (np.pi / 2 - u(0, 0.004)), u(-0.2, 0.2, shape + (3,))
    elif family == "spin":
        roll, pitch = u(-0.2, 0.2), u(-0.2, 0.2)
        axis = rng.normal(size=shape + (3,))
        omega = axis / np.linalg.norm(axis, axis=-1, keepdims=True) * u(245, 300)[..., None]
    else:
        raise ValueError(family)
    q = _unit_in_float32(_quat_of_euler(roll, pitch, yaw)).astype(np.float64)
    return q, omega, np.einsum("...ij,...j->...i", _matrix_of_quat(q), vel_body)


@functools.lru_cache(maxsize=None)
def _reset_blob(task, noise, over):
    orc = O.OracleEnv(config(task, 16, noise, **dict(over)), "f64", threads=8)
    orc.reset()
    w = orc.get_state()
    orc.close()
    return w


@functools.lru_cache(maxsize=None)
def _central_blob(task, noise, over):
    """40 oracle steps out of reset with random actions, at the task's own 16 sub-steps."""
    orc = O.OracleEnv(config(task, 16, noise, **dict(over)), "f64", threads=8)
    orc.reset()
    step = orc.step_stacked if orc.cfg.stacked_obs else orc.step
    for s in range(40):
        step(orc.random_actions(ACTION_SEED + 1, s), terminal=False)
    w = orc.get_state()
    orc.close()
    return w


def armed(blob, D):
    return blob[: N_ENVS * D * K.DRONE_WORDS].reshape(N_ENVS, D, K.DRONE_WORDS)[..., K.D["ARMED"]] != 0


def build(task, family, noise=0, over=(), base="reset", envs=None):
    """State blob (uint32 words, a copy) of `task` with `family` written onto every armed drone of the envs in `envs` (all by default) of
    the base blob: "reset" (the reset state) or "central".  `family` may be a sequence of N_ENVS names, one per env.  `central` leaves the
    central blob as it is."""
    cfg = config(task, 16, noise, **dict(over))
    D = cfg.n_drones
    w = (_reset_blob if base == "reset" else _central_blob)(task, noise, tuple(over)).copy()
    if family == "central":
        return _central_blob(task, noise, tuple(over)).copy()
    fam_of_env = [family] * N_ENVS if isinstance(family, str) else list(family)
    dr = w[: N_ENVS * D * K.DRONE_WORDS].reshape(N_ENVS, D, K.DRONE_WORDS)
    on = armed(w, D)
    sel = np.zeros(N_ENVS, bool)
    sel[np.arange(N_ENVS) if envs is None else np.asarray(envs)] = True
    for fam in sorted(set(fam_of_env)):
        q, om, v = draws(fam, task, D)
        m = on & (sel & (np.array(fam_of_env) == fam))[:, None]
        for name, val in (("QUAT", q), ("OMEGA", om), ("VEL", v)):
            o = K.D[name]
            dr[..., o:o + val.shape[-1]][m] = val.astype(np.float32).view(np.uint32)[m]
    return w


def actions(cfg):
    orc = O.OracleEnv(cfg, "f64")
    a = orc.random_actions(ACTION_SEED, 0)
    orc.close()
    return a


def oracle_step(cfg, blob, acts, precision):
    """One step of the `precision` oracle from `blob` with the census on -> dict(state, inertial, reward, done, info, margins,
    state_margins, branches, guard_margin)."""
    orc = O.OracleEnv(cfg, precision, threads=8)
    orc.set_state(blob)
    orc.set_flight_census(True)
    out = (orc.step_stacked if cfg.stacked_obs else orc.step)(acts)
    branches, guard_margin = orc.flight_census()
    r = dict(state=orc.get_state(), inertial=orc.inertial.copy(), reward=out[-3].copy(), done=out[-2].copy(), info=out[-1].copy(),
             margins=orc.margins(), state_margins=orc.state_margins(), branches=branches, guard_margin=guard_margin)
    orc.close()
    return r


def drone_words(state, D):
    return state[: N_ENVS * D * K.DRONE_WORDS].reshape(N_ENVS, D, K.DRONE_WORDS)


def gaps(state, inertial, ref_state, ref_inertial, D):
    """{group: per-drone (per-env for the inertial rows) largest |x - ref| over the group's words, in units of max(1, |ref|)}; angles modulo
    2 pi (2 in the inertial row's units of pi), quaternions up to sign."""
    a, b = drone_words(state, D), drone_words(ref_state, D)
    out = {}

    def rel(x, y, wrap=None, axis=-1):
        d = x.astype(np.float64) - y
        if wrap:
            d = (d + wrap / 2) % wrap - wrap / 2
        return (np.abs(d) / np.maximum(1.0, np.abs(y))).max(axis)

    for name, (o, n) in GROUPS.items():
        x, y = a[..., o:o + n].view(np.float32), b[..., o:o + n].view(np.float32).astype(np.float64)
        if name == "QUAT":
            out[name] = np.minimum(rel(x, y), rel(-x, y))
        else:
            out[name] = rel(x, y, 2 * np.pi if name == "OBS_EULER" else None)
    for name, (o, n) in INERTIAL_GROUPS.items():
        out[name] = rel(inertial[:, o:o + n], ref_inertial[:, o:o + n].astype(np.float64), 2.0 if name == "INERTIAL_EULER" else None)
    return out


def masks(f64, crafted):
    """(kept [N,D], comparable [N,D]): kept = crafted drones whose every IMU read stayed more than GUARD_MARGIN from the guard's threshold in
    the float64 oracle; comparable = kept drones of envs in which no discrete decision that changes state or done sat within MARGIN of its
    threshold (a kill, a reset: float words of such an env say nothing about the flight)."""
    kept = crafted & (f64["guard_margin"] > GUARD_MARGIN)
    return kept, kept & (f64["state_margins"] > MARGIN)[:, None]


def per_group(g, name, comparable):
    """The figures of `name` over the comparable drones (inertial rows: over the envs whose agent, drone 0, is comparable)."""
    return g[name][comparable[:, 0]] if name in INERTIAL_GROUPS else g[name][comparable]


@functools.lru_cache(maxsize=None)
def pair(task, family, substeps, noise, over=()):
    """The float32 / float64 oracle pair of one case, computed once and shared (read-only): dict(cfg, blob, actions, f32, f64, crafted, kept,
    comparable, G {group: max}, NEAR {group: 90th percentile})."""
    cfg = config(task, substeps, noise, **dict(over))
    D = cfg.n_drones
    blob = build(task, family, noise, over)
    acts = actions(cfg)
    f64, f32 = oracle_step(cfg, blob, acts, "f64"), oracle_step(cfg, blob, acts, "f32")
    crafted = armed(blob, D)
    kept, comparable = masks(f64, crafted)
    g = gaps(f32["state"], f32["inertial"], f64["state"], f64["inertial"], D)
    G, NEAR = {}, {}
    for name in ALL_GROUPS:
        x = per_group(g, name, comparable)
        G[name] = float(x.max()) if x.size else 0.0
        NEAR[name] = float(np.percentile(x, 90)) if x.size else 0.0
    return dict(cfg=cfg, D=D, blob=blob, actions=acts, f32=f32, f64=f64, crafted=crafted, kept=kept, comparable=comparable, G=G, NEAR=NEAR)
