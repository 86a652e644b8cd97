"""The own-sphere tile that te_step returns, held to float64 at cell edges, the rim and closer-wins ties.

Every kernel that te_step can pick for the level4 family, stage02 and stage01 bins with lidar_cell_fast (te_engage.hpp: native rsq / rcp, polynomial
asin / atan2, a multiply by 1 / pi, truncation); the reference-made fixtures reached only observe_kernel's libm lidar_cell, and the step kernels
were compared with each other, not with anything else.  Here every form takes ONE step without physics on the crafted states of
tests/_lidar_states.py and its tile is compared with the float64 oracle's: a cell that differs (hit or not, who won, r_hat beyond 2e-6, flag or
time beyond 1e-7) must lie in the neighbourhood of a target whose decision margin is at most M = 4 G, G from the oracle's own float32 / float64
pair on these states (tests/test_oracle_lidar_edges.py, tests/_lidar_states.py: family_G); exact cases excuse nothing.  TE_LIDAR_EDGES_RECORD=<path> appends one JSON line per
case: the largest margin at which the kernel disagreed, the smallest at which it agreed, the share of targets held (profiles/lidar_edges.json)."""
import json
import os

import numpy as np
import pytest

from dronechase_amd import config as K
from tests import _lidar_states as L
from tests._blob import Blob

pytestmark = pytest.mark.gpu

# (task, config overrides, environment knobs, the engage kernel the plan must name, env limit of the case)
FORMS = {
    "slots": ("exp03", (), {}, "engage_slots_kernel<16>", 700),
    "regs": ("exp03", (), {"TE_ENGAGE": "regs"}, "engage_kernel<2, 9, false>", 700),
    "spw2": ("exp03", (), {"TE_SLOT_SPW": "2"}, "engage_slots_multi_kernel<2, true, false>", 700),
    "lds": ("exp03", (), {"TE_ENGAGE": "lds"}, "engage_observe_kernel<0, 256>", 700),       # libm lidar_cell: a control on the same states
    "wide": ("exp03", (("n_invaders", 9), ("n_pursuers", 5)), {}, "engage_kernel<6, 12, false>", 700),
    "wide_lds": ("exp03", (("n_invaders", 9), ("n_pursuers", 5)), {"TE_ENGAGE": "lds"}, "engage_observe_kernel<0, 256>", 700),      # (the control again)
    "stage02": ("stage02", (("n_invaders", 8),), {}, "engage_slots_stage02_kernel<16>", 700),
    "stage02_regs": ("stage02", (("n_invaders", 8),), {"TE_ENGAGE": "regs"}, "engage_stage02_kernel<2, 8>", 700),
    "stage02_lds": ("stage02", (("n_invaders", 8),), {"TE_ENGAGE": "lds"}, None, 700),
    "stage01": ("stage01", (), {}, "engage_stage01_kernel", 320),
    "two_planes": ("exp03", (("lidar_channels", 2),), {}, "engage_slots_kernel<16>", 700),
    "stage02_two_planes": ("stage02", (("lidar_channels", 2), ("n_invaders", 8)), {}, "engage_slots_stage02_kernel<16>", 700),
}
CASES = [(form, family) for form in FORMS for family in L.FAMILIES + (("crowd",) if form.startswith("wide") else ())]
EULER_BAR = 1e-4     # rad: the single-step parity bar of a state word (tests/test_gpu_parity.py STATE_TOL); the read itself belongs to the flight tests


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _env(monkeypatch, cfg, knobs, role, kernel):
    from dronechase_amd._lib import kernel_plan
    from dronechase_amd.batched_env import BatchedEnv
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    plan = kernel_plan(cfg)
    assert plan[role] == kernel or (kernel is None and "engage_observe_kernel" in plan[role]), plan
    env = BatchedEnv(cfg, "cuda:0")
    for k in knobs:
        monkeypatch.delenv(k)
    return env


def _record(fig, **more):
    path = os.environ.get("TE_LIDAR_EDGES_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(fig, **more)) + "\n")


def _hold(r, tile, label, **more):
    """The assertion of this file: `tile` [N, planes, 13, 26] against the float64 tiles of reference `r`."""
    bad = L.mismatch(tile, r["f64"])
    M = L.bound(r["case"]["family"])
    fig = L.figures(r, bad, M)
    print(f"{label}: M = {M:.3g} m, held = {fig['kept_share']:.3f}, kernel disagrees up to "
          f"{fig['largest_disagreeing_margin']:.3g} m in {fig['disagreeing_cells']} cells, agrees down to {fig['smallest_agreeing_margin']}")
    _record(fig, form=label, G_family=L.family_G(r["case"]["family"]), **more)
    assert fig["largest_disagreeing_margin"] <= M, f"{label}: the kernel's tile differs from float64 at a margin of {fig['largest_disagreeing_margin']:.3g} m > M = {M:.3g} m"
    assert fig["kept_share"] >= 2.0 / 3.0


@pytest.mark.parametrize("form,family", CASES)
def test_step_tile_against_float64(monkeypatch, form, family):
    torch = _torch()
    task, over, knobs, kernel, limit = FORMS[form]
    r = L.reference(task, family, 0, over, limit)
    c = r["case"]
    N, D = c["N"], c["D"]
    env = _env(monkeypatch, c["cfg"], knobs, "engage", kernel)
    env.set_state(torch.from_numpy(c["blob"].view(np.int32)).cuda())
    lidar, _, _, _, done, _ = env.step(torch.zeros((N, 4), dtype=torch.float32, device="cuda:0"), terminal=False)
    tile, done = lidar.cpu().numpy(), done.cpu().numpy()
    after = Blob(env.get_state().cpu().numpy().view(np.uint32), N, D)
    env.close()
    # the config kept every task event away from the armed set; the tile is held on the poses the kernel itself read: positions as loaded, and
    # the agents' OBS_EULER words as the sub-step kernel left them, which must be the float64 read up to the parity bar of a state word
    before = Blob(c["blob"], N, D)
    assert not done.any() and np.array_equal(after.dr[:, :, K.D["ARMED"]], before.dr[:, :, K.D["ARMED"]])
    armed = before.dr[:, :, K.D["ARMED"]] != 0
    assert np.array_equal(after.dr[:, :, K.D["OBS_POS"]:K.D["OBS_POS"] + 3][armed], before.dr[:, :, K.D["POS"]:K.D["POS"] + 3][armed])
    assert tile.shape == (N, int(c["cfg"].lidar_channels), K.LIDAR_NTHETA, K.LIDAR_NPHI)
    o = K.D["OBS_EULER"]
    euler = after.dr[:, 0, o:o + 3].view(np.float32)
    gap = np.abs((euler.astype(np.float64) - before.dr[:, 0, o:o + 3].view(np.float32) + np.pi) % (2 * np.pi) - np.pi)
    assert gap.max() < EULER_BAR, f"the kernel's attitude read is {gap.max():.3g} rad from float64's"
    _hold(L.refer(c, euler), tile, f"{form}/{family}", euler_read_gap=float(gap.max()))


@pytest.mark.parametrize("n,kernel", [(None, "observe_ally_kernel"), (4096, "ally_view_kernel+ally_patch_kernel")])
@pytest.mark.parametrize("family", ["theta_edge", "phi_edge", "seam", "poles", "rim", "ties", "coincident"])
def test_ally_tile_against_float64(monkeypatch, n, kernel, family):
    """exp05: the ally's tile from te_observe_wingman against own_sphere_from_poses(own = 1): the one-launch form, and the two-launch form at exactly
    4 096 envs (the case's envs repeated to fill it)."""
    torch = _torch()
    r = L.reference("exp05", family, 1, (), 700)
    c = r["case"]
    N, D = c["N"], c["D"]
    n = n or N
    idx = np.arange(n) % N
    before = Blob(c["blob"], N, D)
    words = np.concatenate([before.dr[idx].reshape(-1), before.er[idx].reshape(-1)])
    env = _env(monkeypatch, L.config("exp05", n), {}, "wingman_view", kernel)
    assert words.size == env.state_words()
    env.set_state(torch.from_numpy(words.view(np.int32)).cuda())
    tile = env.observe_wingman(1)[0].cpu().numpy()
    env.close()
    assert np.array_equal(tile[N:], tile[idx[N:]])       # (the repeated envs see what their originals see)
    _hold(r, tile[:N], f"ally{n if n != N else ''}/{family}")


def _quat(rpy):
    from tests._flight_states import _quat_of_euler, _unit_in_float32
    rpy = np.atleast_2d(np.asarray(rpy, np.float64))
    return _unit_in_float32(_quat_of_euler(rpy[:, 0], rpy[:, 1], rpy[:, 2]))


PLANS = [({}, "engage_slots_kernel<16>"), ({"TE_ENGAGE": "regs"}, "engage_kernel<2, 9, false>")]


@pytest.mark.parametrize("knobs,kernel", PLANS)
def test_lidar_binning_fixture_through_te_step(monkeypatch, golden, knobs, kernel):
    """tests/golden/lidar_math.npz (the reference's LidarMath on 1 000 body-frame vectors) through te_step, i.e. through lidar_cell_fast, with the
    exclusions and bars of test_lidar_binning_fixture_through_te_observe unchanged."""
    torch = _torch()
    from tests.test_gpu_fixtures import _angle_margin
    g = golden("lidar_math.npz")
    vecs, n = g["vecs"], len(g["vecs"])
    cfg = L.config("exp02", n, n_invaders=1, lidar_radius=float(g["max_radius"]))
    env = _env(monkeypatch, cfg, knobs, "engage", kernel)
    b = Blob(np.zeros(env.state_words(), np.uint32), n, 2)
    for e in range(n):
        b.place(e, 0, (0, 0, 0)); b.place(e, 1, vecs[e]); b.set_ei(e, "STEP", 3); b.set_ei(e, "MAX_STEP", 300); b.set_ei(e, "ROUND", 1); b.refresh_snapshot(e)
    env.set_state(torch.from_numpy(b.w.view(np.int32)).cuda())
    lidar = env.step(torch.zeros((n, 4), dtype=torch.float32, device="cuda:0"), terminal=False)[0].cpu().numpy()
    after = Blob(env.get_state().cpu().numpy().view(np.uint32), n, 2)
    assert np.array_equal(after.dr[:, :, K.D["ARMED"]], b.dr[:, :, K.D["ARMED"]])
    checked = 0
    for e in range(n):
        sph = g["sph"][e]
        mt, mp = _angle_margin(sph[1], sph[2])
        rn = float(g["norm_dist"][e])
        hits = np.argwhere(lidar[e, 0] < 1.0)
        if rn >= 1.0:
            if sph[0] > float(g["max_radius"]) * (1 + 1e-6):
                assert len(hits) == 0, e
                checked += 1
            continue
        if min(mt, mp) < 1e-5 or sph[0] < 1e-6:
            continue
        assert len(hits) == 1 and tuple(hits[0]) == (int(g["th_idx"][e]), int(g["ph_idx"][e])), (e, hits, g["th_idx"][e], g["ph_idx"][e])
        t, p = hits[0]
        assert abs(lidar[e, 0, t, p] - rn) < 1e-6 and abs(lidar[e, 1, t, p] - 0.2) < 1e-7 and abs(lidar[e, 2, t, p] - 0.1) < 1e-7
        checked += 1
    assert checked > 950
    env.close()


@pytest.mark.parametrize("knobs,kernel", PLANS)
def test_normalization_fixture_through_te_step(monkeypatch, golden, knobs, kernel):
    """tests/golden/normalization.npz through te_step: the step re-reads the IMU from the world state, so position, velocity and rates are loaded
    there (level attitude: body = world) and the attitude row is left to the flight tests; bar as in test_normalization_fixture_through_te_observe."""
    torch = _torch()
    g = golden("normalization.npz")
    n = len(g["pos"])
    cfg = L.config("exp02", n, n_invaders=1, dome_radius=float(g["dome_radius"]), max_speed=float(g["max_speed"]))
    env = _env(monkeypatch, cfg, knobs, "engage", kernel)
    b = Blob(np.zeros(env.state_words(), np.uint32), n, 2)
    for e in range(n):
        b.place(e, 0, g["pos"][e]); b.place(e, 1, (3, 3, 3))
        b.set_f(e, 0, "VEL", g["vel"][e]); b.set_f(e, 0, "OMEGA", g["rate"][e])
        b.set_i(e, 0, "MUNITION", 20); b.set_i(e, 0, "LAST_FIRED", -60); b.set_ei(e, "STEP", 3); b.set_ei(e, "MAX_STEP", 300); b.set_ei(e, "ROUND", 1)
        b.refresh_snapshot(e)
    env.set_state(torch.from_numpy(b.w.view(np.int32)).cuda())
    inertial = env.step(torch.zeros((n, 4), dtype=torch.float32, device="cuda:0"), terminal=False)[1].cpu().numpy()
    keep = [0, 1, 2, 3, 4, 5, 9, 10, 11]
    np.testing.assert_allclose(inertial[:, keep], g["out"][:, keep], atol=1e-6)
    env.close()


@pytest.mark.parametrize("knobs,kernel", [({}, "engage_slots_multi_kernel<2, true, false>"), ({"TE_ENGAGE": "regs"}, "engage_kernel<6, 12, false>")])
def test_closer_wins_fixture_through_te_step(monkeypatch, golden, knobs, kernel):
    """The closer-wins lists of tests/golden/lidar_math.npz that fit a served shape (at most 5 LOYALWINGMAN and 12 LOITERINGMUNITION features: 6 + 12
    slots: the slot waves and engage_kernel<6, 12>) through te_step, cell for cell as test_closer_wins_fixture_through_te_observe asserts."""
    torch = _torch()
    from tests.test_gpu_fixtures import _angle_margin, _rot_zyx
    g = golden("lidar_math.npz")
    feats, nf, want = g["feats"], g["n_feats"], g["closer"]
    Rr = float(g["max_radius"])
    P, I = 6, 12
    fits = [e for e in range(len(nf)) if sum(abs(feats[e, k, 3] - 0.6) < 1e-9 for k in range(int(nf[e]))) <= P - 1
            and sum(abs(feats[e, k, 3] - 0.6) >= 1e-9 for k in range(int(nf[e]))) <= I]
    n = len(fits)
    print(f"closer-wins lists that fit 6 + 12 slots: {n} of {len(nf)}")
    assert n >= 10
    cfg = L.config("exp03", n, n_pursuers=P, n_invaders=I, lidar_radius=Rr)
    env = _env(monkeypatch, cfg, knobs, "engage", kernel)
    D = P + I
    b = Blob(np.zeros(env.state_words(), np.uint32), n, D)
    rng = np.random.RandomState(1)
    risky = np.zeros(n, bool)
    for i, e in enumerate(fits):
        rpy = np.zeros(3) if i < n // 2 else rng.uniform([-3, -1.2, -3], [3, 1.2, 3])
        own = np.zeros(3) if i < n // 2 else rng.uniform(-5, 5, 3)
        Rm = _rot_zyx(rpy)
        for s in range(D):
            b.place(i, s, (500.0 + s, 0, 0), armed=0)
        b.place(i, 0, own); b.set_f(i, 0, "QUAT", _quat(rpy)[0])
        np_, ni_ = 1, 0
        for k in range(int(nf[e])):
            r, th, ph, flag = feats[e, k, :4]
            local = (r * Rr if r < 1.0 else 1.001 * Rr) * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            if abs(flag - 0.6) < 1e-9: s = np_; np_ += 1
            else: s = P + ni_; ni_ += 1
            b.place(i, s, own + Rm @ local)
            mt, mp = _angle_margin(th, ph)
            risky[i] |= min(mt, mp) < 2e-5 or r * Rr < 1e-3
        if ni_ == 0:
            b.place(i, D - 1, (0.0, 0.0, 3 * Rr + 20.0))     # (an env without an armed invader would advance its round)
        b.set_ei(i, "STEP", 3); b.set_ei(i, "MAX_STEP", 300); b.set_ei(i, "ROUND", 1); b.refresh_snapshot(i)
    env.set_state(torch.from_numpy(b.w.view(np.int32)).cuda())
    lidar = env.step(torch.zeros((n, 4), dtype=torch.float32, device="cuda:0"), terminal=False)[0].cpu().numpy()
    after = Blob(env.get_state().cpu().numpy().view(np.uint32), n, D)
    assert np.array_equal(after.dr[:, :, K.D["ARMED"]], b.dr[:, :, K.D["ARMED"]])
    checked = 0
    for i, e in enumerate(fits):
        if risky[i]:
            continue
        assert np.array_equal(lidar[i, 0] < 1.0, want[e, 0] < 1.0), e
        np.testing.assert_allclose(lidar[i], want[e], atol=2e-6, err_msg=str(e))
        checked += 1
    resolved = sum(int(nf[e]) - int((want[e, 0] < 1.0).sum()) for i, e in enumerate(fits) if not risky[i])
    print(f"checked {checked} of {n}, collisions resolved {resolved}")
    assert checked >= 0.8 * n      # (the te_observe test: >= 40 of 50)
    assert resolved >= 20 * n // 50      # collisions were resolved (the te_observe test: >= 20 among 50 lists)
    env.close()
