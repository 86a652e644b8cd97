"""Crafted task-logic states for the discrete decisions of one env.step (shoot / explosion / origin ranges, the dome, the floor, the closest-target
searches, the gun's and the clock's integer edges), and the bookkeeping that holds the step kernels to the float64 oracle there.

Every case is a state blob of a few hundred envs (at most 700, never a multiple of 64) stepped ONCE without physics (substeps = 0, observe_lag = 0,
no motor noise, no auto-reset: the positions a kernel decides on are exactly the float32 words loaded), ranges ON.  An env holds ONE decision under
test; every other decision of the env sits at least 0.05 m (or 2 steps) from its threshold, which audit() proves in numpy float64 from the float32
words and the builder asserts.  Unused slots are parked disarmed and far away (stage01 / stage02 keep every drone armed: parked inside the dome);
one spare invader is armed far from everything, because a kill that empties the wave would advance the round and re-arm the slot.  Rungs and signs
are shuffled over the envs.  The margin of an env is audit()'s figure for the decision under test: |value - threshold|, or |d1 - d2| for a tie.

Oracle call sites (oracle/te_oracle.c) -> family.  level4_step_env:
  d vs shoot_range                       shoot_rim (pursuer 0; pursuer 1 in its own envs)
  d vs explosion_range                   explosion_rim (with munition left: deads; MUNITION = 0: suicide; agent and ally)
  |p| vs origin_range                    origin_rim (evaluation drops the rule: the invader must stay, exact; level5_2bt keeps it)
  |p| vs dome_radius (reward, pursuers)  dome_rim (agent, ally): the 1000 penalty
  |p| vs dome_radius (termination)       dome_rim (agent, ally, invader; evaluation: every armed drone)
  z vs -5.99                             floor
  last_dist - cur vs 0.01                reward_edges / approach (reward model exp03)
  |p0| vs born_radius - 2                reward_edges / born (reward model exp03: the literal term jumps by 4; Level5Dumb's is continuous: left out)
  d1 vs last_dist (Level5C1)             reward_edges / c1
  cur - last_dist vs 0.01 (Level5Dumb)   reward_edges / retreat
  cur vs SAFE (Level5Dumb)               left out: (SAFE - cur) / SAFE * 500 is 0 at cur = SAFE, continuous
  z vs -5 (both models)                  left out: (-5 - z) * 1000 is 0 at z = -5, continuous
  drone_contacts: d vs 2 contact_radius  left out: opt-in, off in every preset
stage02_step_env: shoot_range -> shoot_rim (a kill triggers the respawn); explosion_range -> explosion_rim; dome_radius -> dome_rim (agent, supporter,
  invader); last - cur vs 0.01 -> reward_edges / approach.  stage01_step_env: catch_distance -> catch_rim; d, |p0|, |p2| vs dome_radius -> dome_rim
  (sep, agent, invader); d vs last_dist -> reward_edges / progress.
The searches (strict < in slot order; the oracle notes no margin for them) are the `ties` family: which of two / three invaders inside shoot range
dies, the scripted wingman's target (its SETPOINT words after the step), the kamikaze's closest pursuer (the invader's SETPOINT words), each down the
ladder and as exact mirror images (one component of the separation negated: bitwise equal sums of squares, the lower slot must win), a double shot
and a shot plus an explosion on one target.  `integers`: cooldown expiry, the last round of munition, STEP + 1 against MAX_STEP, the last invader of
the last and of the last-but-one round, evaluation's unlimited clock.  `central`: 200 envs of a plain rollout, the control.

The bound is measured on the oracle's own float32 / float64 builds, never on a kernel: G(family) = the largest margin at which the two builds decide an
env differently, pooled over SHAPES; a kernel may differ from float64 only where margin <= M = 4 max(G, 2^-23 s), s the magnitude of the compared
quantity (one float32 ulp of it: v_sqrt_f32's 1 ulp and the rounding of the fused sum of squares, which the float32 oracle does not share, and
thresholds that are no float32 numbers: -5.99, 0.01).  Exact and integer envs excuse nothing."""
import functools
import zlib

import numpy as np

from dronechase_amd import config as K
from oracle import te_oracle as O
from tests._blob import Blob

SEED = 29
STEP = 3
FACTOR = 4.0            # the project's standing factor for "an implementation in another order" (tests/_flight_states.py)
ULP = 2.0 ** -23
CLEAR = 0.05            # metres: every decision that is not under test keeps this distance from its threshold
RUNGS = (3e-1, 1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7, 1e-7)
BASE = dict(substeps=0, observe_lag=0, motor_noise=0, auto_reset=0)
STATE_BAR = 1e-4        # the single-step bar of a float state word (tests/test_gpu_parity.py STATE_TOL)
REWARD_RTOL, REWARD_ATOL = 1e-5, 1e-3      # the scenarios' bar (tests/test_gpu_scenarios.py)
TARGET = 300            # envs a rung family is repeated up to

# the shapes the bound is pooled over: the step kernels' forms of tests/test_gpu_decision_edges.py
SHAPES = {
    "exp03": ("exp03", ()), "wide": ("exp03", (("n_invaders", 9), ("n_pursuers", 5))), "stage02": ("stage02", (("n_invaders", 8),)),
    "stage01": ("stage01", ()), "level5": ("level5", ()), "level5_c1": ("level5_c1", ()), "level5_dumb": ("level5_dumb", ()),
    "evaluation": ("evaluation", ()), "level5_2bt": ("level5_2bt", ()),
}
THRESHOLD_FAMILIES = ("shoot_rim", "explosion_rim", "origin_rim", "dome_rim", "floor", "catch_rim")


def families(shape):
    task = SHAPES[shape][0]
    if task == "stage01":
        return ("catch_rim", "dome_rim", "reward_edges", "integers", "central")
    if task == "stage02":
        return ("shoot_rim", "explosion_rim", "dome_rim", "reward_edges", "ties", "integers", "central")
    if task in ("evaluation", "level5_2bt"):       # reward 0, no floor rule
        return ("shoot_rim", "explosion_rim", "origin_rim", "dome_rim", "ties", "integers", "central")
    return ("shoot_rim", "explosion_rim", "origin_rim", "dome_rim", "floor", "reward_edges", "ties", "integers", "central")


FAMILIES = ("shoot_rim", "explosion_rim", "origin_rim", "dome_rim", "floor", "catch_rim", "reward_edges", "ties", "integers", "central")


def f32(x):
    """x rounded to float32, as float64."""
    return np.asarray(x, np.float32).astype(np.float64)


def _dist(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def _norm(a):
    return _dist(a, (0.0, 0.0, 0.0))


def _dir(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _other_dir(rng, u):
    """A direction at least 40 degrees from u and from -u."""
    while True:
        v = _dir(rng)
        if abs(float(v @ u)) < 0.75:
            return v


class Ctx:
    """One shape's constants, thresholds as the float32 numbers of the config."""

    def __init__(self, shape, family):
        self.shape, self.family = shape, family
        self.task, over = SHAPES[shape]
        self.over = dict(over)
        self.over.update(BASE)
        self.over["hit_prob"] = 0.0 if family == "explosion_rim" else 1.0
        c = self.config(1)
        self.P, self.D = int(c.n_pursuers), int(c.n_drones)
        self.kind = {"stage01": "s01", "stage02": "s02"}.get(self.task, "l4")
        self.shoot, self.expl, self.orig, self.dome = float(c.shoot_range), float(c.explosion_range), float(c.origin_range), float(c.dome_radius)
        self.born, self.catch = float(c.born_radius) - 2.0, float(c.catch_distance)
        self.ev, self.model, self.scripted = int(c.evaluation), int(c.reward_model), bool(c.evaluation or c.agent_scripted)
        self.origin_rule = (not self.ev) or bool(self.ev & K.EVAL_ORIGIN_RULE)
        self.cooldown, self.munition, self.n_rounds, self.max_step = int(c.cooldown_steps), int(c.munition), int(c.n_rounds), int(c.max_step)
        self.spare = self.D - 1

    def config(self, n):
        return O.default_config(self.task, n_envs=n, seed=SEED, **self.over)


# ---------------------------------------------------------------------------------------------------------------------------------
# audit: every decision of one env.step, in numpy float64 from the float32 words.  {key: (margin, class, scale)}, class = "state" (noted by
# the oracle's state_margins), "reward" (margins() only), "tie" (a search: the gap of its two smallest distances; the oracle notes none)
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_smallest(ds):
    s = sorted(ds)
    return (s[1] - s[0], s[1]) if len(s) > 1 else None


def audit(ctx, pos, armed, last_dist, prev_min, ready=True):
    out = {}
    P, D = ctx.P, ctx.D
    if ctx.kind == "s01":
        d = _dist(pos[2], pos[0])
        out[("catch",)] = (abs(d - ctx.catch), "state", ctx.catch)
        out[("sep",)] = (abs(d - ctx.dome), "state", ctx.dome)
        out[("dome", 0)] = (abs(_norm(pos[0]) - ctx.dome), "state", ctx.dome)
        out[("dome", 2)] = (abs(_norm(pos[2]) - ctx.dome), "state", ctx.dome)
        out[("progress",)] = (abs(d - last_dist), "reward", max(d, last_dist))
        return out
    pursuers = [p for p in range(P) if armed[p]]
    invaders = [j for j in range(P, D) if armed[j]]
    for p in pursuers:
        ds = {j: _dist(pos[p], pos[j]) for j in invaders}
        for j, d in ds.items():
            out[("shoot", p, j)] = (abs(d - ctx.shoot), "state", ctx.shoot)
            out[("explode", p, j)] = (abs(d - ctx.expl), "state", ctx.expl)
        t = _two_smallest(ds.values())
        if t:
            out[("tie_inv", p)] = (t[0], "tie", t[1])
    for s in pursuers + invaders:
        out[("dome", s)] = (abs(_norm(pos[s]) - ctx.dome), "state", ctx.dome)
    if ctx.kind == "s02":
        first = pursuers[0] if pursuers else None
        cur = min((_dist(pos[first], pos[j]) for j in invaders), default=0.0) if first is not None else 0.0
        out[("approach",)] = (abs((prev_min - cur) - 0.01), "reward", max(prev_min, cur))
        return out
    for j in invaders:
        if ctx.origin_rule:
            out[("origin", j)] = (abs(_norm(pos[j]) - ctx.orig), "state", ctx.orig)
        t = _two_smallest([_dist(pos[p], pos[j]) for p in pursuers])
        if t:
            out[("tie_pur", j)] = (t[0], "tie", t[1])
    if armed[0]:
        t = _two_smallest([_dist(pos[0], pos[p]) for p in pursuers if p != 0])
        if t:
            out[("tie_ally",)] = (t[0], "tie", t[1])
    if not ctx.ev:
        out[("floor",)] = (abs(pos[0][2] + 5.99), "state", 5.99)
        cur, d1 = current_distance(ctx, pos, armed)
        if ctx.model == K.REWARD_L5_C1:
            out[("c1",)] = (abs(d1 - last_dist), "reward", max(d1, last_dist))
        else:
            out[("z5",)] = (abs(pos[0][2] + 5.0), "reward", 5.0)
            out[("born",)] = (abs(_norm(pos[0]) - ctx.born), "reward", ctx.born)
            if ctx.model == K.REWARD_L5_DUMB:
                out[("retreat",)] = (abs((cur - last_dist) - 0.01), "reward", max(cur, last_dist))
                if not ready:
                    out[("safe",)] = (abs(cur - 5.0), "reward", 5.0)
            else:
                out[("approach",)] = (abs((last_dist - cur) - 0.01), "reward", max(cur, last_dist))
    return out


def _closest(pos, frm, slots):
    best, bd = -1, 0.0
    for s in slots:
        d = _dist(pos[frm], pos[s])
        if best < 0 or d < bd:
            best, bd = s, d
    return best, bd


def current_distance(ctx, pos, armed):
    """(cur, d1) of the level4 reward: the agent's distance to the closest invader of its closest ally (of itself without one), and to its own."""
    P, D = ctx.P, ctx.D
    invaders = [j for j in range(P, D) if armed[j]]
    ally = _closest(pos, 0, [p for p in range(1, P) if armed[p]])[0] if armed[0] else -1
    frm = ally if ally >= 0 else 0
    target = _closest(pos, frm, invaders)[0] if armed[frm] else -1
    cur = _dist(pos[0], pos[target]) if target >= 0 else _norm(pos[0])
    t1, bd = _closest(pos, 0, invaders) if armed[0] else (-1, 0.0)
    return cur, (bd if t1 >= 0 else _norm(pos[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# env recipes: dict(pos {slot: xyz}, armed set, di {(slot, name): int}, ei {name: int}, vel {slot: xyz}, last (LAST_DIST / PREV_SNAP_MIN; None:
# one metre clear), under (audit keys under test), exact, tag, want_armed {slot: 0 / 1}, want_done, want_info, want_dir (slot, target slot))
# ---------------------------------------------------------------------------------------------------------------------------------
def _park(s):
    return np.array([300.0 + 10.0 * s, 100.0, 50.0])


def _skeleton(ctx, rng, pursuers=(0,), box=8.0):
    """The quiet env every recipe starts from."""
    P, D = ctx.P, ctx.D
    r = dict(pos={}, armed=set(), di={}, ei={"STEP": STEP, "MAX_STEP": 300, "ROUND": 1, "INFO_WAVE": 1}, vel={}, last=None, under=(), exact=False,
             tag="", in_range=set(), want_armed={}, want_done=None, want_info=None, want_dir=None, ready=True)
    if ctx.kind == "s01":
        r["ei"]["ROUND"] = 0
        r["armed"] = {0, 1, 2}
        r["pos"] = {0: f32(rng.uniform(-3, 3, 3)), 1: f32([0.5, -6.0, 1.0]), 2: f32(rng.uniform(-3, 3, 3))}
        return r
    if ctx.kind == "s02":       # everybody armed, inside the 8 m dome: agent above, supporter below, invaders on a ring of 6 m
        r["ei"]["ROUND"] = 0
        r["armed"] = set(range(D))
        r["pos"][0] = f32(rng.uniform([-2, -2, 0.5], [2, 2, 2.5]))
        r["pos"][1] = f32(np.array([0.0, 0.0, -3.5]) + rng.uniform(-0.5, 0.5, 3))
        for k, j in enumerate(range(P, D)):
            a = 2 * np.pi * (k + rng.uniform(0.2, 0.8)) / (D - P)
            r["pos"][j] = f32([6.0 * np.cos(a), 6.0 * np.sin(a), rng.uniform(-1.0, 1.0)])
        r["di"][(0, "MUNITION")] = ctx.munition; r["di"][(1, "MUNITION")] = 10
        for p in range(P):
            r["di"][(p, "LAST_FIRED")] = -ctx.cooldown
        return r
    for s in range(D):
        r["pos"][s] = _park(s)
    for p in pursuers:
        r["pos"][p] = f32(rng.uniform([-box, -box, -4.0], [box, box, box]))
        r["armed"].add(p)
        r["di"][(p, "MUNITION")] = ctx.munition; r["di"][(p, "LAST_FIRED")] = -ctx.cooldown
    r["pos"][ctx.spare] = f32([0.5, -0.25, 15.0])
    r["armed"].add(ctx.spare)
    for j in range(P, D):
        r["di"][(j, "NAV_STATE")] = 1        # TE_NAV_COLLIDE_WINGMAN: the kamikaze flies at its closest pursuer
    return r


def _team(ctx, p):
    """The armed pursuers of an env whose decision belongs to pursuer p: the agent always lives (its death ends the episode)."""
    return (0,) if p == 0 else (0, p)


def _free_invader(ctx, r, k=0):
    """The k-th invader slot a recipe may move: stage02's ring slots are all armed, level4's parked ones get armed."""
    j = ctx.P + k
    assert j < ctx.spare or ctx.kind == "s02"
    r["armed"].add(j)
    return j


def _axis(k, length):
    v = np.zeros(3)
    v[k % 3] = length if (k // 3) % 2 == 0 else -length
    return v


def _grid(rng, lo, hi, step, zero_axis=None):
    """A position of multiples of `step` (exact in float32, and so are its sums with such offsets); one coordinate 0 on request."""
    p = np.round(rng.uniform(lo, hi, 3) / step) * step
    if zero_axis is not None:
        p[zero_axis % 3] = 0.0
    return p


def _rim_recipes(ctx, rng, what):
    """[(maker(rng) -> recipe)] of a threshold family: every rung and sign per variant, plus the exact cases the geometry allows."""
    P = ctx.P
    makers = []
    rungs = [(d, s) for d in RUNGS for s in (-1.0, 1.0)]
    if what in ("shoot_rim", "explosion_rim"):
        thr, key = (ctx.shoot, "shoot") if what == "shoot_rim" else (ctx.expl, "explode")
        muns = (None,) if what == "shoot_rim" else (None, 0)
        for p in ((0, 1) if P >= 2 else (0,)):
            for mun in muns:
                def make(rng, d=None, s=None, p=p, mun=mun, k=None):
                    r = _skeleton(ctx, rng, _team(ctx, p))
                    j = _free_invader(ctx, r)
                    if k is None:
                        r["pos"][j] = f32(r["pos"][p] + _dir(rng) * (thr + s * d))
                    else:        # bitwise d == threshold: axis-aligned, the pursuer's coordinate on that axis 0 (0.2f + x is no float32 number)
                        r["pos"][p] = _grid(rng, [-2, -2, 0.5] if ctx.kind == "s02" else -6, [2, 2, 2.5] if ctx.kind == "s02" else 6, 0.25, k)
                        r["pos"][j] = r["pos"][p] + _axis(k, thr)
                        r["exact"] = True
                    if mun is not None:
                        r["di"][(p, "MUNITION")] = mun
                    r["under"] = ((key, p, j),)
                    r["in_range"] = {(p, j)}
                    r["tag"] = f"{key}/p{p}" + ("/empty" if mun == 0 else "") + ("/exact" if k is not None else "")
                    hit = _dist(r["pos"][p], r["pos"][j]) < thr
                    if what == "shoot_rim":
                        r["want_armed"] = {j: 0 if hit else 1, p: 1}
                        r["want_info"] = (int(hit), 0, 0, 0) if ctx.kind == "s02" else None
                    else:       # (stage02's suicide rule: an empty gun inside shoot range removes the target without a shot)
                        r["want_armed"] = {j: 0 if (hit or (mun == 0 and ctx.kind == "s02")) else 1, p: 0 if hit else 1}
                        r["want_info"] = (int(mun == 0), 0, int(hit), 0) if ctx.kind == "s02" else None
                    return r
                makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
                makers += [functools.partial(make, k=k) for k in range(6)]
    elif what == "origin_rim":
        def make(rng, d=None, s=None, k=None):
            r = _skeleton(ctx, rng)
            j = _free_invader(ctx, r)
            r["pos"][j] = f32(_dir(rng) * (ctx.orig + s * d)) if k is None else _axis(k, ctx.orig)
            while _dist(r["pos"][0], r["pos"][j]) < ctx.shoot + 1.0:       # pursuers out of shoot range
                r["pos"][0] = f32(rng.uniform([-8, -8, -4], [8, 8, 8]))
            r["exact"] = k is not None or not ctx.origin_rule       # a form without the rule: the invader stays, whatever its distance
            r["under"] = (("origin", j),) if ctx.origin_rule else ()
            r["tag"] = "origin" + ("/exact" if k is not None else "")
            r["want_armed"] = {j: 0 if (ctx.origin_rule and _norm(r["pos"][j]) < ctx.orig) else 1}
            return r
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs] + [functools.partial(make, k=k) for k in range(6)]
    elif what == "dome_rim":
        if ctx.kind == "s01":
            whos = (("sep", None), ("dome", 0), ("dome", 2))
        else:
            whos = (("dome", 0),) + ((("dome", 1),) if P >= 2 else ()) + (("dome", P),)
        for key, slot in whos:
            def make(rng, d=None, s=None, k=None, key=key, slot=slot):
                r = _skeleton(ctx, rng, (0,) if slot in (None, 0) or slot >= P else (0, slot), box=5.0)
                rad = ctx.dome + s * d if k is None else ctx.dome
                u = _dir(rng) if k is None else _axis(k, 1.0)
                if ctx.kind == "l4" and slot == 0:
                    u[2] = abs(u[2])        # (the agent stays above the floor rule's z = -5.99)
                if key == "sep":        # stage01: invader and agent `dome_radius` apart, both inside the dome
                    r["pos"][0] = f32(-u * 0.5 * rad + rng.uniform(-0.5, 0.5, 3)) if k is None else _grid(rng, -1, 1, 0.25, k) - u * 5.0
                    r["pos"][2] = f32(r["pos"][0] + u * rad) if k is None else r["pos"][0] + u * rad
                    r["under"] = (("sep",),)
                    out = _dist(r["pos"][2], r["pos"][0]) > ctx.dome
                    r["want_done"] = 0
                else:
                    if ctx.kind == "l4" and slot >= P:
                        _free_invader(ctx, r)
                    if ctx.kind == "s01" and slot == 0:      # (keep the invader clear of catch_distance and of the dome-wide separation)
                        r["pos"][2] = f32(u * (rad - 3.0))
                    if ctx.kind == "s01" and slot == 2:
                        r["pos"][0] = f32(u * (rad - 3.0))
                    r["pos"][slot] = f32(u * rad) if k is None else u * rad
                    r["under"] = ((key, slot),)
                    out = _norm(r["pos"][slot]) > ctx.dome
                    r["want_done"] = int(out)
                r["exact"] = k is not None
                r["tag"] = f"dome/{key}{'' if slot is None else slot}" + ("/exact" if k is not None else "")
                return r
            makers += [functools.partial(make, d=d, s=s) for d, s in rungs] + [functools.partial(make, k=k) for k in range(6)]
    elif what == "floor":
        def make(rng, d, s):
            r = _skeleton(ctx, rng)
            r["pos"][0][2] = f32(-5.99 + s * d)
            r["under"] = (("floor",),)
            r["tag"] = "floor"
            r["want_done"] = int(r["pos"][0][2] < -5.99)
            return r
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
    elif what == "catch_rim":
        def make(rng, d=None, s=None, k=None):
            r = _skeleton(ctx, rng)
            if k is None:
                r["pos"][2] = f32(r["pos"][0] + _dir(rng) * (ctx.catch + s * d))
            else:
                r["pos"][0] = _grid(rng, -3, 3, 0.25, k)
                r["pos"][2] = r["pos"][0] + _axis(k, ctx.catch)
            r["exact"] = k is not None
            r["under"] = (("catch",),)
            r["tag"] = "catch" + ("/exact" if k is not None else "")
            r["want_info"] = (int(_dist(r["pos"][2], r["pos"][0]) < ctx.catch), 0, 0, 0)
            return r
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs] + [functools.partial(make, k=k) for k in range(6)]
    else:
        raise ValueError(what)
    return makers


VEL = (1.5, -1.0, 0.5)      # the agent's speed in the reward cases: |v| = 1.87 m/s, so that the approach bonus is gain x 1.87 >= 1.87


def _reward_recipes(ctx, rng):
    """Reward-only thresholds whose term jumps: (makers, {tag: jump})."""
    rungs = [(d, s) for d in RUNGS for s in (-1.0, 1.0)]
    makers, jumps = [], {}
    gain = float(ctx.config(1).approach_bonus_gain)
    speed = float(np.linalg.norm(VEL))

    def near(rng, r, far):
        """An invader `far` metres from the agent (the spare is further)."""
        j = _free_invader(ctx, r)
        r["pos"][j] = f32(r["pos"][0] + _dir(rng) * far)
        return j
    if ctx.kind == "s01":
        def make(rng, d, s):
            r = _skeleton(ctx, rng)
            r["vel"][0] = VEL
            r["last"] = float(f32(_dist(r["pos"][2], r["pos"][0]) + s * d))
            r["under"] = (("progress",),); r["tag"] = "progress"
            return r
        jumps["progress"] = gain * speed
        return [functools.partial(make, d=d, s=s) for d, s in rungs], jumps
    if ctx.kind == "s02" or ctx.model == K.REWARD_EXP03:
        def make(rng, d, s):
            r = _skeleton(ctx, rng, box=4.0)
            r["vel"][0] = VEL
            if ctx.kind == "l4":
                near(rng, r, rng.uniform(3.0, 6.0))
            r["last"] = ("cur", 0.01 + s * d)
            r["under"] = (("approach",),); r["tag"] = "approach"
            return r
        jumps["approach"] = gain * speed
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
    if ctx.kind == "l4" and ctx.model == K.REWARD_EXP03:      # (Level5Dumb's term is min(dist_origin - (born_radius - 2), 1000): continuous, left out)
        def make(rng, d, s):
            r = _skeleton(ctx, rng)
            r["pos"][0] = f32(_dir(rng) * np.array([1.0, 1.0, 0.5]) * 1.0)
            r["pos"][0] = f32(r["pos"][0] / _norm(r["pos"][0]) * (ctx.born + s * d))
            r["under"] = (("born",),); r["tag"] = "born"
            return r
        jumps["born"] = 4.0         # dist_origin - born_radius - 2 at dist_origin = born_radius - 2: the literal term is -4
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
    if ctx.kind == "l4" and ctx.model == K.REWARD_L5_C1:
        def make(rng, d, s):
            r = _skeleton(ctx, rng, box=4.0)
            r["vel"][0] = VEL
            near(rng, r, rng.uniform(3.0, 6.0))
            r["last"] = ("d1", s * d)
            r["under"] = (("c1",),); r["tag"] = "c1"
            return r
        jumps["c1"] = gain * speed
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
    if ctx.kind == "l4" and ctx.model == K.REWARD_L5_DUMB:
        def make(rng, d, s):
            r = _skeleton(ctx, rng, box=4.0)
            near(rng, r, rng.uniform(5.5, 7.0))          # (clear of SAFE = 5)
            r["di"][(0, "LAST_FIRED")] = STEP - 1          # the gun cools down, munition left: the retreat bonus is on
            r["ready"] = False
            r["last"] = ("cur", -(0.01 + s * d))
            r["under"] = (("retreat",),); r["tag"] = "retreat"
            return r
        jumps["retreat"] = 100.0
        makers += [functools.partial(make, d=d, s=s) for d, s in rungs]
    return makers, jumps


def _tie_recipes(ctx, rng):
    P = ctx.P
    makers = []
    lo_hi = ([-2, -2, 0.5], [2, 2, 2.5]) if ctx.kind == "s02" else (-6, 6)

    def kill(rng, d=None, n=2, order=0, p=0, mirror=None):
        """n invaders inside shoot range of pursuer p, distances d apart (mirror: two bitwise equal ones); `order` rotates who is closest."""
        r = _skeleton(ctx, rng, _team(ctx, p))
        slots = [_free_invader(ctx, r, k) for k in range(n)]
        if mirror is None:
            d0 = 0.3 if d >= 0.1 else rng.uniform(0.35, 0.8)
            u = _dir(rng)
            for i in range(n):
                r["pos"][slots[(i + order) % n]] = f32(r["pos"][p] + u * (d0 + i * d))
                u = _other_dir(rng, u)
        else:
            r["pos"][p] = _grid(rng, lo_hi[0], lo_hi[1], 0.125)
            off = np.array([0.5, 0.25, 0.375])[[(mirror + i) % 3 for i in range(3)]] * (1 if mirror < 3 else -1)
            flip = np.ones(3); flip[mirror % 3] = -1.0
            r["pos"][slots[0]], r["pos"][slots[1]] = r["pos"][p] + off, r["pos"][p] + off * flip
            r["exact"] = True
        r["under"] = (("tie_inv", p),)
        r["in_range"] = {(p, j) for j in slots}
        r["tag"] = f"kill{n}/p{p}" + ("/mirror" if mirror is not None else "")
        dead = _closest(r["pos"], p, slots)[0]
        r["want_armed"] = {j: int(j != dead) for j in slots}
        return r

    def wingman(rng, d=None, order=0, mirror=None):
        """The scripted wingman's target among two invaders about 5 m away: its command for the next step."""
        p = 0 if ctx.scripted else 1
        r = _skeleton(ctx, rng, _team(ctx, p), box=5.0)
        a, b = _free_invader(ctx, r, order), _free_invader(ctx, r, 1 - order)
        if mirror is None:
            u = _dir(rng)
            r["pos"][a], r["pos"][b] = f32(r["pos"][p] + u * 5.0), f32(r["pos"][p] + _other_dir(rng, u) * (5.0 + d))
        else:
            r["pos"][p] = _grid(rng, -4, 4, 0.125)
            off = np.array([3.0, 4.0, 0.5])[[(mirror + i) % 3 for i in range(3)]]
            flip = np.ones(3); flip[(mirror + 1) % 3] = -1.0
            r["pos"][a], r["pos"][b] = r["pos"][p] + off, r["pos"][p] + off * flip
            r["exact"] = True
        r["under"] = (("tie_inv", p),)
        r["tag"] = "wingman" + ("/mirror" if mirror is not None else "")
        r["want_dir"] = (p, _closest(r["pos"], p, sorted((a, b)))[0])
        return r

    def kamikaze(rng, d=None, order=0, mirror=None):
        """An invader between the two pursuers: the kamikaze's closest pursuer, in its set-point after the step."""
        r = _skeleton(ctx, rng, (0, 1))
        j = _free_invader(ctx, r)
        a, b = (0, 1) if order == 0 else (1, 0)
        if mirror is None:
            r["pos"][j] = f32(rng.uniform(-5, 5, 3))
            u = _dir(rng)
            r["pos"][a], r["pos"][b] = f32(r["pos"][j] + u * 3.0), f32(r["pos"][j] + _other_dir(rng, u) * (3.0 + d))
        else:
            r["pos"][j] = _grid(rng, -4, 4, 0.125)
            off = np.array([2.0, 1.5, 1.0])[[(mirror + i) % 3 for i in range(3)]]
            flip = np.ones(3); flip[(mirror + 2) % 3] = -1.0
            r["pos"][a], r["pos"][b] = r["pos"][j] + off, r["pos"][j] + off * flip
            r["exact"] = True
        r["under"] = (("tie_pur", j),)
        r["tag"] = "kamikaze" + ("/mirror" if mirror is not None else "")
        r["want_dir"] = (j, _closest(r["pos"], j, (0, 1))[0])
        return r

    def double_shot(rng):
        """Both pursuers with the same invader as their closest, in range: the second shot hits the dead target again."""
        r = _skeleton(ctx, rng, (0, 1))
        j = _free_invader(ctx, r)
        u = _dir(rng)
        r["pos"][j] = f32(r["pos"][0] + u * 0.5)
        r["pos"][1] = f32(r["pos"][j] + _other_dir(rng, u) * 0.7)
        r["in_range"] = {(0, j), (1, j)}
        r["exact"] = True; r["tag"] = "double_shot"
        r["want_armed"] = {j: 0, 0: 1, 1: 1}
        return r

    def shot_and_explosion(rng, p):
        r = _skeleton(ctx, rng, _team(ctx, p))
        j = _free_invader(ctx, r)
        r["pos"][j] = f32(r["pos"][p] + _dir(rng) * 0.1)
        r["in_range"] = {(p, j)}
        r["exact"] = True; r["tag"] = f"shot_and_explosion/p{p}"
        r["want_armed"] = {j: 0, p: 0}
        return r
    ps = (0, 1) if P >= 2 else (0,)
    for d in RUNGS:
        for order in (0, 1):
            makers += [functools.partial(kill, d=d, n=2, order=order, p=p) for p in ps]
            makers += [functools.partial(kill, d=d, n=3, order=order + 1, p=ps[-1])]
            if ctx.kind == "l4":
                makers += [functools.partial(wingman, d=d, order=order)]
                if P >= 2:
                    makers += [functools.partial(kamikaze, d=d, order=order)]
    for m in range(6):
        makers += [functools.partial(kill, p=p, mirror=m) for p in ps]
        if ctx.kind == "l4":
            makers += [functools.partial(wingman, order=m % 2, mirror=m)]
            if P >= 2:
                makers += [functools.partial(kamikaze, order=m % 2, mirror=m)]
    if P >= 2:
        makers += [double_shot] * 4
    makers += [functools.partial(shot_and_explosion, p=p) for p in ps for _ in range(3)]
    return makers


def _integer_recipes(ctx, rng):
    makers = []

    def clock(rng, k):
        r = _skeleton(ctx, rng)
        r["ei"]["MAX_STEP"] = STEP + 1 + k
        r["exact"] = True; r["tag"] = f"max_step{k:+d}"
        r["want_done"] = int(k < 0 and not (ctx.ev and ctx.max_step == 0))      # evaluation with max_step = 0: unlimited
        return r
    makers += [functools.partial(clock, k=k) for k in (-1, 0, 1)]
    if ctx.kind == "s01":
        return makers

    def in_range(rng, r):
        j = _free_invader(ctx, r)
        r["pos"][j] = f32(r["pos"][0] + _dir(rng) * 0.6)
        r["in_range"] = {(0, j)}
        return j

    def cooldown(rng, k):
        r = _skeleton(ctx, rng)
        j = in_range(rng, r)
        r["di"][(0, "LAST_FIRED")] = STEP + 1 - (ctx.cooldown + k)
        r["exact"] = True; r["tag"] = f"cooldown{k:+d}"
        r["want_armed"] = {j: int(k < 0)}
        return r

    def munition(rng, n):
        r = _skeleton(ctx, rng)
        j = in_range(rng, r)
        r["di"][(0, "MUNITION")] = n
        r["exact"] = True; r["tag"] = f"munition{n}"
        r["want_armed"] = {j: int(n == 0 and ctx.kind != "s02")}     # (stage02's suicide rule: an empty gun in range still removes the target)
        return r
    makers += [functools.partial(cooldown, k=k) for k in (-1, 0, 1)] + [functools.partial(munition, n=n) for n in (1, 0)]
    if ctx.kind == "l4":
        def last_invader(rng, back):
            r = _skeleton(ctx, rng)
            r["armed"].discard(ctx.spare)       # no spare: the kill empties the wave
            r["pos"][ctx.spare] = _park(ctx.spare)
            j = in_range(rng, r)
            r["ei"]["ROUND"] = ctx.n_rounds - back; r["ei"]["INFO_WAVE"] = ctx.n_rounds - back
            r["exact"] = True; r["tag"] = f"last_invader/round-{back}"
            r["want_done"] = int(back == 0)
            r["round_may_advance"] = True
            return r
        makers += [functools.partial(last_invader, back=b) for b in (0, 1)]
    return makers


def _recipes(ctx, rng):
    f = ctx.family
    if f in THRESHOLD_FAMILIES:
        return _rim_recipes(ctx, rng, f), {}
    if f == "reward_edges":
        return _reward_recipes(ctx, rng)
    if f == "ties":
        return _tie_recipes(ctx, rng), {}
    if f == "integers":
        return _integer_recipes(ctx, rng), {}
    raise ValueError(f)


def _resolve_last(ctx, r):
    """LAST_DIST / PREV_SNAP_MIN of a recipe as a float32 number: one metre clear of every reward threshold unless the recipe states it."""
    pos, armed = r["pos"], [s in r["armed"] for s in range(ctx.D)]
    if ctx.kind == "s01":
        base = _dist(pos[2], pos[0])
        return float(f32(base + 1.0)) if r["last"] is None else r["last"]
    if ctx.kind == "s02":
        cur = min(_dist(pos[0], pos[j]) for j in range(ctx.P, ctx.D))
        d1 = cur
    else:
        cur, d1 = current_distance(ctx, pos, armed)
    if r["last"] is None:
        return float(f32((d1 if ctx.model == K.REWARD_L5_C1 and ctx.kind == "l4" else cur) + 1.0))
    which, off = r["last"]
    return float(f32((cur if which == "cur" else d1) + off))


def _quiet_elsewhere(ctx, r):
    """Nothing but the decision under test happens: only the pairs the recipe names are inside shoot range, and no drone that is not under test
    is inside origin_range, outside the dome or below the floor."""
    if ctx.kind == "s01":
        return all(("dome", s) in r["under"] or _norm(r["pos"][s]) < ctx.dome for s in (0, 2))
    pos, armed = r["pos"], r["armed"]
    for p in range(ctx.P):
        for j in range(ctx.P, ctx.D):
            if p in armed and j in armed and _dist(pos[p], pos[j]) < ctx.shoot and (p, j) not in r["in_range"]:
                return False
    for s in armed:
        if ("dome", s) not in r["under"] and _norm(pos[s]) > ctx.dome:
            return False
        if ctx.kind == "l4" and s >= ctx.P and ctx.origin_rule and ("origin", s) not in r["under"] and _norm(pos[s]) < ctx.orig:
            return False
    return ctx.kind != "l4" or bool(ctx.ev) or ("floor",) in r["under"] or pos[0][2] > -5.99


def _reward_want(ctx, r, last):
    """(the reward numpy expects, whether the term under test is on) of a reward_edges recipe."""
    pos, armed = r["pos"], [s in r["armed"] for s in range(ctx.D)]
    tag = r["tag"]
    gain = float(ctx.config(1).approach_bonus_gain) * float(np.linalg.norm(VEL))
    if tag == "progress":
        d = _dist(pos[2], pos[0])
        return -d + (gain if d < last else 0.0), d < last
    cur, d1 = (min(_dist(pos[0], pos[j]) for j in range(ctx.P, ctx.D)), 0.0) if ctx.kind == "s02" else current_distance(ctx, pos, armed)
    n0 = _norm(pos[0])
    if ctx.kind == "l4" and ctx.model == K.REWARD_EXP03:       # the literal term: dist_origin - born_radius - 2 beyond born_radius - 2
        beyond = -((n0 - (ctx.born + 2.0) - 2.0) if n0 > ctx.born else 0.0)
    elif ctx.kind == "l4" and ctx.model == K.REWARD_L5_DUMB:
        beyond = -max(0.0, n0 - ctx.born)
    else:
        beyond = 0.0
    if tag == "approach":
        return -cur + (gain if 0.01 < last - cur else 0.0) + beyond, 0.01 < last - cur
    if tag == "born":
        return -cur + beyond, n0 > ctx.born
    if tag == "c1":
        return (gain if d1 < last else 0.0), d1 < last
    assert tag == "retreat"
    return cur + (100.0 if cur - last > 0.01 else 0.0) + beyond, cur - last > 0.01


@functools.lru_cache(maxsize=None)
def case(shape, family):
    """One case: dict(cfg, N, D, P, blob, margin / scale / exact / real [N], tag [N], want [N] (the recipe), jumps)."""
    if family == "central":
        return _central(shape)
    ctx = Ctx(shape, family)
    rng = np.random.default_rng(zlib.crc32(f"{shape}/{family}".encode()))
    makers, jumps = _recipes(ctx, rng)
    reps = max(1, -(-TARGET // len(makers))) if family != "integers" else max(1, 200 // len(makers))
    makers = makers * reps
    assert len(makers) <= 700, (shape, family, len(makers))
    recipes = []
    for make in makers:
        for attempt in range(200):
            r = make(rng)
            last = _resolve_last(ctx, r)
            a = audit(ctx, r["pos"], [s in r["armed"] for s in range(ctx.D)], last, last, r["ready"])
            if all(m >= CLEAR for k, (m, _, _) in a.items() if k not in r["under"]) and _quiet_elsewhere(ctx, r):
                break
        else:
            raise AssertionError(f"{shape}/{family}/{r['tag']}: no geometry keeps the other decisions {CLEAR} m clear: "
                                 f"{ {k: v for k, v in a.items() if v[0] < CLEAR and k not in r['under']} }")
        r["last"] = last
        r["want_reward"] = _reward_want(ctx, r, last) if family == "reward_edges" else None
        r["margin"] = min((a[k][0] for k in r["under"]), default=np.inf)
        r["scale"] = max((a[k][2] for k in r["under"]), default=0.0)
        r["real"] = True
        recipes.append(r)
    while len(recipes) % 64 == 0:       # never a multiple of 64: one quiet env more
        r = _skeleton(ctx, rng)
        r.update(last=_resolve_last(ctx, r), margin=np.inf, scale=0.0, real=False, exact=True, tag="quiet")
        recipes.append(r)
    recipes = [recipes[i] for i in rng.permutation(len(recipes))]
    N, D, P = len(recipes), ctx.D, ctx.P
    cfg = ctx.config(N)
    orc = O.OracleEnv(cfg, "f64")
    orc.reset()
    b = Blob(orc.get_state(), N, D)
    orc.close()
    for e, r in enumerate(recipes):
        for s in range(D):
            b.place(e, s, r["pos"][s], armed=int(s in r["armed"]))
            b.set_f(e, s, "SETPOINT", [0, 0, 0, 0])
            b.set_f(e, s, "PENDING", [0] * 6)      # (stage01's reset leaves the invader a wrench for its first sub-step; a step of none is not its subject)
            b.set_i(e, s, "MUNITION", 10 if s >= P else ctx.munition); b.set_i(e, s, "LAST_FIRED", -ctx.cooldown); b.set_i(e, s, "NAV_STATE", 0)
        for (s, name), v in r["di"].items():
            b.set_i(e, s, name, v)
        for s, v in r["vel"].items():
            b.set_f(e, s, "VEL", v); b.set_f(e, s, "OBS_VEL", v)
        for name in ("AGENT_KILLS", "ALLIES_KILLS", "DEADS"):
            b.set_ei(e, name, 0)
        for name, v in r["ei"].items():
            b.set_ei(e, name, v)
        b.set_ef(e, "LAST_DIST", [r["last"]]); b.set_ef(e, "PREV_SNAP_MIN", [r["last"]]); b.set_ef(e, "LAST_ACTION", [0, 0, 0, 0])
        b.refresh_snapshot(e)
    # a bitwise d == threshold that is no tie; rim_rounded: the square of the threshold is no float32 number (0.2f, 0.4f), so a float32 sum of
    # squares is rounded before the root is taken: sqrtf (correctly rounded) still returns the threshold, a root good to 1 ulp need not.  Where
    # the square is exact (1, 8, 10, 20 m) the root's argument is the perfect square itself
    scale = np.array([r["scale"] for r in recipes])
    rim_exact = np.array([r["exact"] and len(r["under"]) > 0 and not r["under"][0][0].startswith("tie") for r in recipes], bool)
    return dict(cfg=cfg, ctx=ctx, shape=shape, family=family, N=N, D=D, P=P, blob=b.w, jumps=jumps, want=recipes,
                margin=np.array([r["margin"] for r in recipes]), scale=np.array([r["scale"] for r in recipes]),
                exact=np.array([r["exact"] for r in recipes], bool),
                rim_exact=rim_exact, rim_rounded=rim_exact & (scale.astype(np.float32).astype(np.float64) ** 2 != (scale * scale).astype(np.float32)), real=np.array([r["real"] for r in recipes], bool),
                tag=np.array([r["tag"] for r in recipes]))


def _central(shape):
    """200 envs of a plain reset-and-rollout state, 40 steps in, stepped once without physics: the control.  The margin of an env is audit()'s
    smallest figure over every decision and search of the env."""
    N = 200
    ctx = Ctx(shape, "central")
    task, over = SHAPES[shape]
    orc = O.OracleEnv(O.default_config(task, n_envs=N, seed=SEED, **dict(over)), "f64", threads=4)
    orc.reset()
    for s in range(40):
        orc.step(orc.random_actions(SEED, s), terminal=False)
    w = orc.get_state()
    orc.close()
    b = Blob(w, N, ctx.D)
    margin, scale = np.zeros(N), np.zeros(N)
    for e in range(N):
        pos = [b.f(e, s, "POS", 3).astype(np.float64) for s in range(ctx.D)]
        for s in range(ctx.D):       # (observe_lag = 0: the step reads the IMU first; no physics: the read is the loaded position)
            b.set_f(e, s, "OBS_POS", pos[s])
        armed = [bool(b.i(e, s, "ARMED")) for s in range(ctx.D)]
        ready = b.i(e, 0, "MUNITION") == 0 or ctx.cooldown <= b.ei(e, "STEP") + 1 - b.i(e, 0, "LAST_FIRED")
        a = audit(ctx, pos, armed, float(b.ef(e, "LAST_DIST")[0]), float(b.ef(e, "PREV_SNAP_MIN")[0]), ready)
        k = min(a, key=lambda k: a[k][0])
        margin[e], scale[e] = a[k][0], a[k][2]
    return dict(cfg=ctx.config(N), ctx=ctx, shape=shape, family="central", N=N, D=ctx.D, P=ctx.P, blob=b.w, jumps={}, want=[None] * N,
                margin=margin, scale=scale, exact=np.zeros(N, bool), rim_exact=np.zeros(N, bool), rim_rounded=np.zeros(N, bool), real=np.ones(N, bool), tag=np.array(["central"] * N))


# ---------------------------------------------------------------------------------------------------------------------------------
# stepping and comparing
# ---------------------------------------------------------------------------------------------------------------------------------
def state_part(c, words):
    """The drone and env records of a blob (level5: the ring that follows is left to the stacked-observation tests)."""
    return np.asarray(words, np.uint32)[: c["N"] * (c["D"] * K.DRONE_WORDS + K.ENV_WORDS)]


def oracle_step(c, precision):
    """dict(reward, done, info, state, margins, state_margins) of one oracle step on the case's blob."""
    orc = O.OracleEnv(c["cfg"], precision)
    orc.set_state(c["blob"])
    out = orc.step(np.zeros((c["N"], 4), np.float32), terminal=False)
    r = dict(reward=out[3].copy(), done=out[4].copy(), info=out[5].copy(), state=state_part(c, orc.get_state()), margins=orc.margins(),
             state_margins=orc.state_margins())
    orc.close()
    return r


def differs(c, a, b):
    """[N] bool: envs in which step results a and b differ: done, info, any integer state word, reward beyond the scenarios' bar, a float state
    word beyond the single-step bar (b is the reference of the reward's relative part)."""
    from tests.test_gpu_parity import _compare_states
    fdiff, imis = _compare_states(b["state"], a["state"], c["N"], c["D"])
    bad = (a["done"] != b["done"]) | (a["info"] != b["info"]).any(1) | imis | (fdiff > STATE_BAR)
    ra, rb = a["reward"].astype(np.float64), b["reward"].astype(np.float64)
    return bad | (np.abs(ra - rb) > REWARD_ATOL + REWARD_RTOL * np.abs(rb))


@functools.lru_cache(maxsize=None)
def reference(shape, family):
    """The float64 / float32 oracle steps of one case, computed once and shared (read-only), and G of this case."""
    c = case(shape, family)
    f64, f32_ = oracle_step(c, "f64"), oracle_step(c, "f32")
    bad = differs(c, f32_, f64)
    G = float(c["margin"][bad & ~c["exact"]].max(initial=0.0))
    return dict(case=c, f64=f64, f32=f32_, pair_differs=bad, G=G)


@functools.lru_cache(maxsize=None)
def family_G(family):
    """G per family from the oracle pair alone, pooled over every shape that has the family."""
    return max(reference(shape, family)["G"] for shape in SHAPES if family in families(shape))


def bound(c):
    """[N]: M = 4 max(G, 2^-23 s) per env."""
    return FACTOR * np.maximum(family_G(c["family"]), ULP * c["scale"])


def figures(c, bad, report_only=None):
    """The per-case record: M (largest over the envs), share of envs held (margin above M, or exact), largest margin of an env that disagrees,
    smallest margin of an inexact env that agrees, and the disagreeing envs that nothing excuses.  report_only [N]: envs that are counted
    (rim_exact_disagreeing) but not held: a bitwise d == threshold on a form whose square root is v_sqrt_f32."""
    M = bound(c)
    real, exact = c["real"], c["exact"]
    held = exact | (c["margin"] > M)
    reported = 0
    if report_only is not None:
        reported = int((bad & report_only).sum())
        held = held & ~report_only
        bad = bad & ~report_only
    loose = real & ~exact
    return dict(shape=c["shape"], family=c["family"], n_envs=int(c["N"]), M=float(M[real].max()), G_family=family_G(c["family"]),
                held_share=float(held[real].mean()), disagreeing=int(bad.sum()),
                largest_disagreeing_margin=float(np.where(exact, np.inf, c["margin"])[bad].max(initial=0.0)),
                smallest_agreeing_margin=float(c["margin"][loose & ~bad].min()) if (loose & ~bad).any() else None,
                rim_exact_disagreeing=reported, unexcused=[int(e) for e in np.flatnonzero(bad & held)])
