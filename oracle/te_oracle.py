"""ctypes front-end of the TEST oracle (oracle/te_oracle.c).  Test infrastructure only:
importable from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg — never from
dronechase_amd/."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from dronechase_amd import config as K

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS: dict = {}


def _sources():
    """What the two oracle libraries are made of (oracle/Makefile): the restatement, the shared config table and the ABI header."""
    root = os.path.dirname(_HERE)
    return [os.path.join(_HERE, "te_oracle.c"), os.path.join(_HERE, "Makefile"), os.path.join(root, "dronechase_amd", "csrc", "te_config.c"),
            os.path.join(root, "include", "threatengage.h")]


def build(force: bool = False) -> None:
    """Compile both precisions with gcc (oracle/Makefile) when a library is missing or older than one of its sources."""
    outs = [os.path.join(_HERE, "_build", f"libte_oracle_{p}.so") for p in ("f64", "f32")]
    newest = max(os.path.getmtime(f) for f in _sources() if os.path.exists(f))
    if force or any(not os.path.exists(o) or os.path.getmtime(o) < newest for o in outs):
        subprocess.run(["make", "-C", _HERE, "-s", "-B"], check=True)


def lib(precision: str = "f64") -> C.CDLL:
    if precision not in _LIBS:
        path = os.path.join(_HERE, "_build", f"libte_oracle_{precision}.so")
        build()   # no-op when the libraries are newer than their sources
        L = C.CDLL(path)
        L.ote_create.restype = C.c_void_p
        L.ote_create.argtypes = [C.POINTER(K.Config)]
        L.ote_destroy.argtypes = [C.c_void_p]
        L.ote_state_words.restype = C.c_size_t
        L.ote_state_words.argtypes = [C.c_void_p]
        for name in ("ote_get_state", "ote_set_state"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.ote_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_observe.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        L.ote_step.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_int]
        L.ote_margins.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_stack_margins.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_ring_lookup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ote_step_stacked.argtypes = [C.c_void_p] + [C.c_void_p] * 12 + [C.c_int]
        L.ote_observe_stacked.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.ote_step_students.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int]
        L.ote_observe_ally.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.ote_set_ally_actions.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_observe_wingman.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.ote_set_wingman_actions.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ote_wingman_info.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_stack_draws.argtypes = [C.POINTER(K.Config), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        L.ote_state_margins.argtypes = [C.c_void_p, C.c_void_p]
        L.ote_random_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
        L.ote_set_flight_census.argtypes = [C.c_void_p, C.c_int]
        L.ote_flight_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ote_set_lidar_margins.argtypes = [C.c_void_p, C.c_int]
        L.ote_lidar_margins.argtypes = [C.c_void_p, C.c_void_p]
        L.te_config_default.argtypes = [C.POINTER(K.Config), C.c_int32]
        L.te_quad_preset.argtypes = [C.POINTER(K.Config), C.c_int32]
        L.ote_degrees_between.restype = C.c_double
        L.ote_normalize_distance.restype = C.c_double
        L.ote_normalize_distance.argtypes = [C.c_double, C.c_double]
        L.ote_theta_index.argtypes = [C.c_double]
        L.ote_phi_index.argtypes = [C.c_double]
        _LIBS[precision] = L
    return _LIBS[precision]


def default_config(task, **overrides) -> K.Config:
    cfg = K.Config()
    t = K.TASKS[task] if isinstance(task, str) else int(task)
    rc = lib("f64").te_config_default(C.byref(cfg), t)
    if rc:
        raise ValueError(f"te_config_default({task}) -> {rc}")
    if "quad_preset" in overrides:
        if lib("f64").te_quad_preset(C.byref(cfg), int(overrides.pop("quad_preset"))):
            raise ValueError("unknown quad_preset")
    return K.apply_overrides(cfg, **overrides)


# bits of OracleEnv.flight_census() (OTE_CENSUS_* in te_oracle.c)
CENSUS_GENERAL, CENSUS_GUARD, CENSUS_SATURATED, CENSUS_FLOORED, CENSUS_FAST, CENSUS_GROUND = 1, 2, 4, 8, 16, 32


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class OracleEnv:
    """N scalar environments stepped on the CPU (optionally OpenMP over envs)."""

    def __init__(self, cfg: K.Config, precision: str = "f64", threads: int = 1):
        self.L = lib(precision)
        self.cfg = cfg.copy()
        self.N = int(cfg.n_envs)
        self.D = cfg.n_drones
        self.threads = threads
        self.h = self.L.ote_create(C.byref(self.cfg))
        if not self.h:
            raise RuntimeError("ote_create failed (bad config)")
        N = self.N
        self.lidar = np.empty((N, int(cfg.lidar_channels), K.LIDAR_NTHETA, K.LIDAR_NPHI), np.float32)
        self.inertial = np.empty((N, K.OBS_INERTIAL_WORDS), np.float32)
        self.last_action = np.empty((N, 4), np.float32)
        self.t_lidar = np.zeros_like(self.lidar)
        self.t_inertial = np.zeros_like(self.inertial)
        self.t_last_action = np.zeros_like(self.last_action)
        self.reward = np.empty(N, np.float32)
        self.done = np.empty(N, np.uint8)
        self.info = np.empty((N, 4), np.int32)
        if cfg.stacked_obs:  # level5
            self.stacked = np.empty((N, K.STACK_SPHERES, K.LIDAR_CHANNELS, K.LIDAR_NTHETA, K.LIDAR_NPHI), np.float32)
            self.mask = np.empty((N, K.STACK_SPHERES), np.uint8)
            self.t_stacked = np.zeros_like(self.stacked)
            self.t_mask = np.zeros_like(self.mask)

    def close(self):
        if self.h:
            self.L.ote_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, mask: Optional[np.ndarray] = None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.L.ote_reset(self.h, _p(m))
        return self.observe()

    def observe(self):
        self.L.ote_observe(self.h, _p(self.lidar), _p(self.inertial), _p(self.last_action))
        return self.lidar, self.inertial, self.last_action

    def step(self, actions: np.ndarray, terminal: bool = True):
        a = np.ascontiguousarray(actions, np.float32)
        assert a.shape == (self.N, 4)
        t = (self.t_lidar, self.t_inertial, self.t_last_action) if terminal else (None, None, None)
        self.L.ote_step(self.h, _p(a), _p(self.lidar), _p(self.inertial), _p(self.last_action), _p(self.reward),
                        _p(self.done), _p(self.info), _p(t[0]), _p(t[1]), _p(t[2]), self.threads)
        return self.lidar, self.inertial, self.last_action, self.reward, self.done, self.info

    # level5 ---------------------------------------------------------------------------------
    def observe_stacked(self):
        self.L.ote_observe_stacked(self.h, _p(self.stacked), _p(self.mask), _p(self.inertial), _p(self.last_action))
        return self.stacked, self.mask, self.inertial, self.last_action

    def step_stacked(self, actions: np.ndarray, terminal: bool = True):
        a = np.ascontiguousarray(actions, np.float32)
        assert a.shape == (self.N, 4)
        t = (self.t_stacked, self.t_mask, self.t_inertial, self.t_last_action) if terminal else (None,) * 4
        rc = self.L.ote_step_stacked(self.h, _p(a), _p(self.stacked), _p(self.mask), _p(self.inertial), _p(self.last_action),
                                     _p(self.reward), _p(self.done), _p(self.info), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]),
                                     self.threads)
        assert rc == 0
        return self.stacked, self.mask, self.inertial, self.last_action, self.reward, self.done, self.info

    def step_students(self):
        """Level5DumbMultiObs: one all-scripted step; (stacked [N,P,6,3,13,26], mask [N,P,6], inertial [N,P,15], last_action [N,P,4],
        active [N,P], reward, done, info)."""
        N, P = self.N, int(self.cfg.n_pursuers)
        if not hasattr(self, "st"):
            self.st = (np.empty((N, P, K.STACK_SPHERES, K.LIDAR_CHANNELS, K.LIDAR_NTHETA, K.LIDAR_NPHI), np.float32), np.empty((N, P, K.STACK_SPHERES), np.uint8),
                       np.empty((N, P, K.OBS_INERTIAL_WORDS), np.float32), np.empty((N, P, 4), np.float32), np.empty((N, P), np.uint8))
        st = self.st
        rc = self.L.ote_step_students(self.h, _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3]), _p(st[4]), _p(self.reward), _p(self.done), _p(self.info), self.threads)
        assert rc == 0, "step_students needs cfg.stacked_obs and an all-scripted task (level5_dumb, evaluation)"
        return (*st, self.reward, self.done, self.info)

    # exp05 ----------------------------------------------------------------------------------
    def observe_wingman(self, wingman: int):
        """(lidar [N,3,13,26], inertial [N,15], last_action [N,4], active [N] u8) of a caller-driven pursuer on the current state."""
        lidar, inertial = np.empty_like(self.lidar), np.empty_like(self.inertial)
        last_action, active = np.empty_like(self.last_action), np.empty(self.N, np.uint8)
        rc = self.L.ote_observe_wingman(self.h, wingman, _p(lidar), _p(inertial), _p(last_action), _p(active))
        assert rc == 0, "observe_wingman: this pursuer is not driven by the caller"
        return lidar, inertial, last_action, active

    def set_wingman_actions(self, wingman: int, actions: np.ndarray):
        a = np.ascontiguousarray(actions, np.float32)
        assert a.shape == (self.N, 4)
        rc = self.L.ote_set_wingman_actions(self.h, wingman, _p(a))
        assert rc == 0, "set_wingman_actions: this pursuer is not driven by the caller"

    def observe_ally(self):
        assert self.cfg.ally_policy == K.ALLY_EXTERNAL, "observe_ally needs cfg.ally_policy == ALLY_EXTERNAL with 2 pursuers"
        return self.observe_wingman(1)

    def set_ally_actions(self, actions: np.ndarray):
        assert self.cfg.ally_policy == K.ALLY_EXTERNAL, "set_ally_actions needs cfg.ally_policy == ALLY_EXTERNAL with 2 pursuers"
        self.set_wingman_actions(1, actions)

    def wingman_info(self) -> np.ndarray:
        """[N,P,5] i32 rows (lw_kills, lw_alive, lw_munitions, current_wave, step) (Evaluation_Task.compute_info)."""
        out = np.empty((self.N, self.cfg.n_pursuers, 5), np.int32)
        rc = self.L.ote_wingman_info(self.h, _p(out))
        assert rc == 0, "wingman_info needs cfg.evaluation"
        return out

    def stack_margins(self) -> np.ndarray:
        """Smallest angular distance (rad) of any feature binned during the last step to a LIDAR cell boundary."""
        out = np.empty(self.N, np.float64)
        self.L.ote_stack_margins(self.h, _p(out))
        return out

    def ring_lookup(self, env: int, pursuer: int, age: int) -> int:
        """Step stamp of the snapshot of `pursuer` that has `age` now (1 = freshest), 0 if there is none."""
        return int(self.L.ote_ring_lookup(self.h, env, pursuer, age))

    def ring(self, words: Optional[np.ndarray] = None) -> np.ndarray:
        w = self.get_state() if words is None else words
        base = self.N * (self.D * K.DRONE_WORDS + K.ENV_WORDS)
        return w[base:].reshape(self.N, self.cfg.n_pursuers, K.RING_DEPTH, K.ring_entry_words(self.D))

    def margins(self) -> np.ndarray:
        out = np.empty(self.N, np.float64)
        self.L.ote_margins(self.h, _p(out))
        return out

    def state_margins(self) -> np.ndarray:
        """Like margins() but only over decisions that change state or done (not reward-only thresholds)."""
        out = np.empty(self.N, np.float64)
        self.L.ote_state_margins(self.h, _p(out))
        return out

    def set_flight_census(self, on: bool = True):
        """Record, from the next step on, which sub-step paths every drone takes (CENSUS_* bits).  Off by default."""
        assert self.L.ote_set_flight_census(self.h, int(bool(on))) == 0

    def flight_census(self):
        """(branches [N,D] uint32, guard_margin [N,D] float64) of the last step: the CENSUS_* bits ORed over its sub-steps, and the
        smallest | |sarg| - 0.99999 | over every IMU read of the step (1e30 for a drone that did not fly)."""
        branches = np.empty((self.N, self.D), np.uint32)
        margin = np.empty((self.N, self.D), np.float64)
        assert self.L.ote_flight_census(self.h, _p(branches), _p(margin)) == 0, "flight_census needs set_flight_census(True)"
        return branches, margin

    def set_lidar_margins(self, on: bool = True):
        """Record, from the next step / observe on, how decidable the agent's LIDAR tile is (lidar_margins).  Off by default."""
        assert self.L.ote_set_lidar_margins(self.h, int(bool(on))) == 0

    def lidar_margins(self) -> np.ndarray:
        """[N] float64, metres: how far some drone of the env would have to move for the agent's tile of the last step / observe (the
        terminal tile when one was produced) to change: the distance to the nearest cell edge, to the rim r = lidar_radius, or between
        two ranges of one cell (own_sphere_margins).  1e30 for the reset observation."""
        out = np.empty(self.N, np.float64)
        assert self.L.ote_lidar_margins(self.h, _p(out)) == 0, "lidar_margins needs set_lidar_margins(True)"
        return out

    def random_actions(self, seed: int, step_index: int) -> np.ndarray:
        a = np.empty((self.N, 4), np.float32)
        self.L.ote_random_actions(self.h, _p(a), seed, step_index)
        return a

    def state_words(self) -> int:
        return int(self.L.ote_state_words(self.h))

    def get_state(self) -> np.ndarray:
        w = np.empty(self.state_words(), np.uint32)
        self.L.ote_get_state(self.h, _p(w))
        return w

    def set_state(self, words: np.ndarray):
        w = np.ascontiguousarray(words, np.uint32)
        assert w.size == self.state_words()
        self.L.ote_set_state(self.h, _p(w))

    # convenience views of a state blob
    def drones(self, words: Optional[np.ndarray] = None) -> np.ndarray:
        w = self.get_state() if words is None else words
        return w[: self.N * self.D * K.DRONE_WORDS].reshape(self.N, self.D, K.DRONE_WORDS)

    def envrecs(self, words: Optional[np.ndarray] = None) -> np.ndarray:
        w = self.get_state() if words is None else words
        base = self.N * self.D * K.DRONE_WORDS
        return w[base: base + self.N * K.ENV_WORDS].reshape(self.N, K.ENV_WORDS)


# ---------------------------------------------------------------------------------------------
# unit-level entry points (pinned by tests/test_oracle_golden.py against tests/golden/*.npz)
# ---------------------------------------------------------------------------------------------
def _d(a):
    return np.ascontiguousarray(a, np.float64)


def philox(ctr, key, precision="f64", rounds=10):
    c = np.asarray(ctr, np.uint32); k = np.asarray(key, np.uint32); o = np.zeros(4, np.uint32)
    getattr(lib(precision), {10: "ote_philox4x32_10", 7: "ote_philox4x32_7"}[rounds])(_p(c), _p(k), _p(o))
    return o


def vec_fn(name, v, n_out, precision="f64"):
    a = _d(v); o = np.zeros(n_out)
    getattr(lib(precision), name)(_p(a), _p(o))
    return o


def rotate_vector(q, v, precision="f64"):
    a, b, o = _d(q), _d(v), np.zeros(3)
    lib(precision).ote_rotate_vector(_p(a), _p(b), _p(o))
    return o


def theta_index(x, precision="f64"):
    return int(lib(precision).ote_theta_index(float(x)))


def phi_index(x, precision="f64"):
    return int(lib(precision).ote_phi_index(float(x)))


def normalize_distance(d, rmax, precision="f64"):
    return float(lib(precision).ote_normalize_distance(float(d), float(rmax)))


def add_features(feats, invert=False, precision="f64"):
    f = _d(feats).reshape(-1, 5)
    sphere = np.ones((K.LIDAR_CHANNELS, K.LIDAR_NTHETA, K.LIDAR_NPHI), np.float32)
    lib(precision).ote_add_features(_p(sphere), C.c_int(len(f)), _p(f), C.c_int(int(invert)))
    return sphere


def gun_trace(steps, shoot, draws, munition, cooldown=60, hit_prob=0.9, precision="f64"):
    n = len(steps)
    s = np.ascontiguousarray(steps, np.int32); sh = np.ascontiguousarray(shoot, np.int32); dr = _d(draws)
    hit = np.zeros(n, np.int32); mun = np.zeros(n, np.int32); st = np.zeros((n, 3))
    lib(precision).ote_gun_trace(C.c_int(n), _p(s), _p(sh), _p(dr), C.c_int32(munition), C.c_int32(cooldown),
                                 C.c_double(hit_prob), _p(hit), _p(mun), _p(st))
    return hit, mun, st


def kamikaze_scenario(P, I, positions, mask, nav_in, speed=0.4, cone_check=0, building=(0, 0, 0.1), precision="f64"):
    pos = _d(positions); nin = np.ascontiguousarray(nav_in, np.int32); b = _d(building)
    nout = nin.copy(); sp = np.zeros((P + I, 4))
    lib(precision).ote_kamikaze_scenario(C.c_int(P), C.c_int(I), _p(pos), C.c_uint32(int(mask)), _p(nin),
                                         C.c_double(speed), C.c_int(cone_check), _p(b), _p(nout), _p(sp))
    return nout, sp


def wingman_scenario(P, I, positions, formation, mask, slot, munition, last_fired, step, cooldown=60, speed=0.6,
                     precision="f64"):
    pos = _d(positions); f = _d(formation); sp = np.zeros(4)
    lib(precision).ote_wingman_scenario(C.c_int(P), C.c_int(I), _p(pos), _p(f), C.c_uint32(int(mask)), C.c_int(slot),
                                        C.c_int32(munition), C.c_int32(last_fired), C.c_int32(step),
                                        C.c_int32(cooldown), C.c_double(speed), _p(sp))
    return sp


def point_inside_cone(p, apex, base, degrees, precision="f64"):
    a, b, c = _d(p), _d(apex), _d(base)
    return int(lib(precision).ote_point_inside_cone(_p(a), _p(b), _p(c), C.c_double(degrees)))


def degrees_between(a, b, precision="f64"):
    x, y = _d(a), _d(b)
    return float(lib(precision).ote_degrees_between(_p(x), _p(y)))


def normalize_inertial(pos, vel, att, rate, max_speed, dome_radius, precision="f64"):
    a, b, c, d = _d(pos), _d(vel), _d(att), _d(rate)
    out = np.zeros(12, np.float32)
    lib(precision).ote_normalize_inertial(_p(a), _p(b), _p(c), _p(d), C.c_double(max_speed), C.c_double(dome_radius),
                                          _p(out))
    return out


def own_sphere_from_poses(pos, euler_own, own, armed, P, lidar_radius, precision="f64"):
    p = _d(pos); e = _d(euler_own); a = np.ascontiguousarray(armed, np.uint8)
    sphere = np.zeros((K.LIDAR_CHANNELS, K.LIDAR_NTHETA, K.LIDAR_NPHI), np.float32)
    lib(precision).ote_own_sphere_from_poses(C.c_int(len(p)), C.c_int(P), _p(p), _p(e), C.c_int(own), _p(a),
                                             C.c_double(lidar_radius), _p(sphere))
    return sphere


def own_sphere_margins(pos, euler_own, own, armed, P, lidar_radius, precision="f64"):
    """(cell [D] int32, rhat [D], margin [D] metres) of every other armed drone in the own sphere of `own`, in the build's arithmetic: cell =
    theta index * 26 + phi index (-1: not a target), margin = how far the drone would have to move for the tile to change (te_oracle.c:
    sphere_margins; 1e30 for a slot that is no target)."""
    p = _d(pos); e = _d(euler_own); a = np.ascontiguousarray(armed, np.uint8)
    cell = np.empty(len(p), np.int32); rhat = np.empty(len(p)); margin = np.empty(len(p))
    lib(precision).ote_own_sphere_margins(C.c_int(len(p)), C.c_int(P), _p(p), _p(e), C.c_int(own), _p(a), C.c_double(lidar_radius),
                                          _p(cell), _p(rhat), _p(margin))
    return cell, rhat, margin


def level4_position(r, min_z, u_theta, u_phi, precision="f64"):
    o = np.zeros(3)
    lib(precision).ote_level4_position(C.c_double(r), C.c_double(min_z), C.c_double(u_theta), C.c_double(u_phi), _p(o))
    return o


def fly(cfg, mode, setpoint, n_substeps, pos0, precision="f64"):
    sp, p0 = _d(setpoint), _d(pos0)
    pos = np.zeros((n_substeps, 3)); vel = np.zeros((n_substeps, 3)); eul = np.zeros((n_substeps, 3))
    thr = np.zeros((n_substeps, 4))
    lib(precision).ote_fly(C.byref(cfg), C.c_int(mode), _p(sp), C.c_int(n_substeps), _p(p0), _p(pos), _p(vel), _p(eul),
                           _p(thr))
    return pos, vel, eul, thr


def fly_from(cfg, mode, setpoint, n_substeps, pos0, zv_i0, precision="f64"):
    """IMU reads (position, body velocity, euler, body rates) seen at the top of each of n sub-steps, starting at rest
    with the z-velocity integrator pre-loaded."""
    sp, p0 = _d(setpoint), _d(pos0)
    out = [np.zeros((n_substeps, 3)) for _ in range(4)]
    lib(precision).ote_fly_from(C.byref(cfg), C.c_int(mode), _p(sp), C.c_int(n_substeps), _p(p0), C.c_double(zv_i0), *[_p(o) for o in out])
    return out


def fly_hidden(cfg, mode, setpoints, sp_start, n_substeps, pos0, hidden, noise_env=-1, precision="f64"):
    """The general form of fly_from: set-point schedule, hidden controller / motor state at release, optional motor noise.
    Returns the IMU reads (position, body velocity, euler, body rates) at the top of each sub-step."""
    sp = _d(setpoints).reshape(-1, 4); st = np.ascontiguousarray(sp_start, np.int32); p0 = _d(pos0); h = _d(hidden)
    assert h.size == 16 and len(st) == len(sp)
    out = [np.zeros((n_substeps, 3)) for _ in range(4)]
    lib(precision).ote_fly_hidden(C.byref(cfg), C.c_int(mode), _p(sp), _p(st), C.c_int(len(sp)), C.c_int(n_substeps), _p(p0), _p(h),
                                  C.c_int(noise_env), *[_p(o) for o in out])
    return out


def stack_draws(cfg: K.Config, env_local: int, episode: int, step: int, armed_pursuers: int) -> dict:
    """The random choices of one stacked observation: n, the chosen wingmen, their ages, the shuffle."""
    out = np.zeros(15, np.int32)
    lib("f64").ote_stack_draws(C.byref(cfg), env_local, episode, step, armed_pursuers, _p(out))
    n = int(out[0])
    return {"n": n, "who": out[1:1 + n].tolist(), "age": out[5:5 + n].tolist(), "perm": out[9:15].tolist()}

