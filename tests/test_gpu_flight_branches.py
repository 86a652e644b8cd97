"""The sub-step kernel on the paths that no rollout flies (te_device.hpp substep(): the general attitude read with its range reductions
and quadrant selects, the gimbal guard with its double-angle yaw, the fast-rotation update on the native sin / cos in revolutions), held
to the float64 oracle from a common float32 state.  Run on an MI355X: `pytest -m gpu`.

The bounds are not chosen here and never come from the kernel: every case computes the oracle's own float32 / float64 pair on the same
inputs (tests/_flight_states.py pair(); tests/test_oracle_flight_branches.py holds that pair to its conditions on the CPU) and asks, per
word group and in units of max(1, |float64 value|), angles modulo 2 pi and quaternions up to sign,
    |kernel - f64| <= max(4 G[group], 16 * 2^-24)        on every kept drone   (G = the pair's largest gap; 4 = the factor of
                                                                               tests/test_policy_bf16.py: a maximum over rare rounding
                                                                               flips is heavy-tailed; 16 ulps: G can be 0, v_rcp / v_rsq
                                                                               are 1-ulp where the oracle divides)
    share of kept drones beyond NEAR[group] <= 30 %                            (NEAR = the pair's 90th percentile; three times its own 10 %)
A drone is kept when every IMU read of the step stayed more than 1e-6 from the guard's threshold |sarg| = 0.99999 in the float64 oracle (the
guard band is 1e-5 wide and leaving it is a real discontinuity: roll jumps from 0 to its value); integer words, done and info are equal
wherever OracleEnv.margins() > 1e-4.  Where 4 G <= 1e-4 this implies the STATE_TOL of tests/test_gpu_parity.py; each case prints the groups
whose pair exceeds it.

The second test is bitwise and needs no oracle: a lane's result does not depend on what its wave-mates fly (the wave-uniform central-branch
test and the ballot-guarded saturation branch of substep()).

TE_FLIGHT_BRANCHES_RECORD=<path>: every parity case appends one JSON line (both kernels' names where the helpers apply) (profiles/flight_branches.json is such a record)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CES0, LAG0, PRESET0 = {"control_every_substep": 0}, {"observe_lag": 0}, {"quad_preset": 0}


def _cases():
    from tests import _flight_states as F
    out = []
    for noise in (0, 1):
        out += [("exp03", fam, s, noise, {}) for fam in F.FAMILIES for s in F.SUBSTEPS[fam]]
        # PyFlyt's own controller rate: S = 2 is one controller sub-step (CTRL == 0) and one coasting, capturing one (CTRL == 2)
        out += [("exp03", fam, 2, noise, CES0) for fam in ("tilted", "inverted", "near_guard", "guard")]
        out += [("exp03", "tilted", 16, noise, CES0), ("exp03", "spin", 1, noise, CES0)]
        # the epilogue's euler_of(b.q)
        out += [("exp03", fam, s, noise, LAG0) for fam in ("guard", "near_guard") for s in F.SUBSTEPS[fam]]
        # mode 7 with the pending wrench
        out += [("stage01", fam, max(x for x in F.SUBSTEPS[fam] if x <= 2), noise, {}) for fam in F.FAMILIES]
        out += [("level5", "tilted", 16, noise, {})]
        out += [("exp03", "tilted", s, noise, PRESET0) for s in (1, 2, 16)]
    return out


def _id(case):
    task, fam, s, noise, over = case
    return "-".join([task, fam, f"S{s}", "noise" if noise else "quiet"] + [f"{k}{v}" for k, v in over.items()])


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box (no CPU fallback exists)")
    return torch


def _kernel_step(cfg, blob, acts):
    """One step of the HIP path from `blob` -> (state words, outputs as numpy, the plan's substeps= name)."""
    torch = _gpu()
    from dronechase_amd._lib import kernel_plan
    from dronechase_amd.batched_env import BatchedEnv
    name = kernel_plan(cfg)["substeps"]
    gpu = BatchedEnv(cfg, "cuda:0")
    gpu.set_state(torch.from_numpy(blob.view(np.int32)).cuda())
    step = gpu.step_stacked if cfg.stacked_obs else gpu.step
    out = [x.cpu().numpy() for x in step(torch.from_numpy(acts).cuda())]
    state = gpu.get_state().cpu().numpy().view(np.uint32)
    gpu.close()
    return state, out, name


def _check(p, state, out, label):
    """-> (per-group figures of the kernel, list of violated bounds)."""
    from dronechase_amd import config as K
    from tests import _flight_states as F
    D, f64 = p["D"], p["f64"]
    inertial, done, info = out[-5], out[-2], out[-1]
    bad = []
    # integer words, done, info: wherever no discrete decision sat near its threshold
    ok = f64["margins"] > F.MARGIN
    a, b = F.drone_words(state, D), F.drone_words(f64["state"], D)
    idw = list(K.D_INT_WORDS)
    base = F.N_ENVS * D * K.DRONE_WORDS
    ea, eb = (w[base: base + F.N_ENVS * K.ENV_WORDS].reshape(F.N_ENVS, K.ENV_WORDS)[:, list(K.E_INT_WORDS)] for w in (state, f64["state"]))
    imis = (a[..., idw] != b[..., idw]).any(axis=(1, 2)) | (ea != eb).any(axis=1) | (done.astype(bool) != f64["done"].astype(bool)) | (info != f64["info"]).any(axis=1)
    if (imis & ok).any():
        bad.append(f"integer words / done / info differ in {int((imis & ok).sum())} unambiguous envs")
    # float words
    g = F.gaps(state, inertial, f64["state"], f64["inertial"], D)
    figures = {}
    for name in F.ALL_GROUPS:
        x = F.per_group(g, name, p["comparable"])
        gap = float(x.max()) if x.size else 0.0
        share = float((x > p["NEAR"][name]).mean()) if x.size else 0.0
        bound = max(4 * p["G"][name], F.ULP_FLOOR)
        figures[name] = {"gap": gap, "share": share}
        if not np.isfinite(x).all() or gap > bound:
            bad.append(f"{name}: kernel gap {gap:.3e} > max(4 G, 16 ulp) = {bound:.3e} (G {p['G'][name]:.3e})")
        if share > 0.30:
            bad.append(f"{name}: {share:.3f} of the kept drones beyond NEAR = {p['NEAR'][name]:.3e}")
    worst = max(F.ALL_GROUPS, key=lambda n: figures[n]["gap"] / max(4 * p["G"][n], F.ULP_FLOOR))
    print(f"{label}: kept {p['kept'].sum() / p['crafted'].sum():.3f}, comparable {int(p['comparable'].sum())}; worst {worst} gap "
          f"{figures[worst]['gap']:.2e} vs G {p['G'][worst]:.2e}; pair beyond STATE_TOL/4: {[n for n in F.ALL_GROUPS if 4 * p['G'][n] > 1e-4]}")
    return figures, bad


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_rare_paths_against_the_float64_oracle(case, monkeypatch):
    """Measured on the MI355X: profiles/flight_branches.json, one line per run of a case.
    What the share rule found: `tilted` at one sub-step, where the captured angles are those of the input attitude, had 31.2 % of its drones
    beyond NEAR = 1.146e-7 (one ulp) in OBS_EULER - 14.8 % in pitch alone.  x_asin's square-root branch subtracted from a pi/2 rounded to
    float32, 4.37e-8 too large: 0.73 ulp of a pitch in [0.5, 1), always to the same side.  The attitude read now takes that error off after the rounding
    (x_asin_pitch, te_device.hpp; one ulp for a pitch below 1 rad, nothing above): 22.4 % of the drones, 4.9 % in pitch; every case holds both rules, the largest share of any family is 27 %."""
    from tests import _flight_states as F
    task, family, substeps, noise, over = case
    p = F.pair(task, family, substeps, noise, tuple(sorted(over.items())))
    cfg = p["cfg"]
    monkeypatch.delenv("TE_K1_HELP", raising=False)
    runs = [("as created", *_kernel_step(cfg, p["blob"], p["actions"]))]
    if noise and substeps >= 2 and cfg.n_pursuers <= 4:   # the noise-helper instantiation and the plain one (te_env.hip: help_ok)
        monkeypatch.setenv("TE_K1_HELP", "0")
        runs.append(("TE_K1_HELP=0", *_kernel_step(cfg, p["blob"], p["actions"])))
        monkeypatch.delenv("TE_K1_HELP")
        assert runs[0][3].endswith(", true>") and runs[1][3].endswith(", false>"), (runs[0][3], runs[1][3])
    kept_share = float(p["kept"].sum() / p["crafted"].sum())
    failures = [] if kept_share >= 0.85 else [f"only {kept_share:.3f} of the crafted drones are kept"]
    record = {"task": task, "family": family, "substeps": substeps, "motor_noise": noise, "variant": over, "kernels": [r[3] for r in runs],
              "kept_share": kept_share, "comparable_drones": int(p["comparable"].sum())}
    for i, (label, state, out, name) in enumerate(runs):
        figures, bad = _check(p, state, out, f"{_id(case)} [{label}: {name}]")
        failures += [f"[{label}] {b}" for b in bad]
        groups = {n: {"G": p["G"][n], "NEAR": p["NEAR"][n], "kernel_gap": figures[n]["gap"], "kernel_share_beyond_NEAR": figures[n]["share"]}
                  for n in F.ALL_GROUPS}
        if i == 0:
            record["groups"] = groups
        elif groups != record["groups"]:     # (the helped flights are the plain ones bit for bit: tests/test_gpu_noise_helper.py)
            record["groups_of_second_kernel"] = groups
    path = os.environ.get("TE_FLIGHT_BRANCHES_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")
    assert not failures, "\n".join(failures)


CYCLE = ("tilted", "inverted", "guard", "near_guard", "spin")


@pytest.mark.parametrize("ces", [1, 0])
@pytest.mark.parametrize("noise,helper", [(0, None), (1, "1"), (1, "0")])
@pytest.mark.parametrize("substeps", [2, 16])
def test_a_lane_does_not_depend_on_its_wave_mates(substeps, noise, helper, ces, monkeypatch):
    """A: every env central.  B: A with every 8th env on a rare state, so every wave takes the general attitude read (and the wave-uniform
    saturation test) while most of its lanes are central.  C: every env rare, the same draws.  An env that two blobs share comes out of one
    step with the same bits in both: the central-branch polynomials ARE x_atan2 / x_asin on their central branch (te_device.hpp substep()),
    and the ballot in front of the saturation branch only skips work."""
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd._lib import kernel_plan
    from dronechase_amd.batched_env import BatchedEnv
    from tests import _flight_states as F
    if helper is None:
        monkeypatch.delenv("TE_K1_HELP", raising=False)
    else:
        monkeypatch.setenv("TE_K1_HELP", helper)
    cfg = F.config("exp03", substeps, noise, control_every_substep=ces)
    if helper is not None:
        assert kernel_plan(cfg)["substeps"].endswith(", true>" if helper == "1" else ", false>")
    D, N = cfg.n_drones, F.N_ENVS
    cycle = [f for f in CYCLE if not (f == "spin" and substeps == 16)]   # the explicit integrator diverges within 16 sub-steps of a spin
    rare = np.arange(0, N, 8)
    fams = [cycle[(e // 8) % len(cycle)] for e in range(N)]   # by the ordinal of the rare env: 8 consecutive families per wave of 64 lanes
    for wave in range(N // 64):
        assert {fams[e] for e in rare if e // 64 == wave} == set(cycle), "a wave of B misses a family"
    blobs = {"A": F.build("exp03", "central", noise), "B": F.build("exp03", fams, noise, base="central", envs=rare),
             "C": F.build("exp03", fams, noise, base="central")}
    on = F.armed(blobs["A"], D)
    assert on[rare].any(axis=1).all() and (F.drone_words(blobs["B"], D)[rare] == F.drone_words(blobs["C"], D)[rare]).all()
    assert (F.drone_words(blobs["A"], D)[rare] != F.drone_words(blobs["B"], D)[rare]).any()
    acts = torch.from_numpy(F.actions(cfg)).cuda()
    gpu = BatchedEnv(cfg, "cuda:0")
    res = {}
    for k, w in blobs.items():
        gpu.set_state(torch.from_numpy(w.view(np.int32)).cuda())
        out = [x.cpu().numpy().reshape(N, -1) for x in gpu.step(acts)]
        s = gpu.get_state().cpu().numpy().view(np.uint32)
        per_env = [F.drone_words(s, D).reshape(N, -1), s[N * D * K.DRONE_WORDS:].reshape(N, K.ENV_WORDS)]
        res[k] = [np.ascontiguousarray(x).view(np.uint8).reshape(N, -1) for x in per_env + out]
    gpu.close()
    shared_ab = np.setdiff1d(np.arange(N), rare)
    for i, (x, y) in enumerate(zip(res["A"], res["B"])):
        assert np.array_equal(x[shared_ab], y[shared_ab]), f"A / B: part {i} of a central env depends on its rare wave-mates"
    for i, (x, y) in enumerate(zip(res["B"], res["C"])):
        assert np.array_equal(x[rare], y[rare]), f"B / C: part {i} of a rare env depends on its wave-mates"
    # the rare envs did fly something else than the central ones
    assert not np.array_equal(res["A"][0][rare], res["B"][0][rare])
