"""te_drive_wingman: a caller-driven pursuer (exp05's ally, the evaluation task's "nn" drivers) flown by a packed
LidarInertialActionPolicy in one ABI call (observe, deterministic forward, clamp, drive), and PPO on exp05 with that ally inside
the rollout (PPOConfig.wingman_driver, PPO(wingman_policy=...)).

The main check is bitwise: te_drive_wingman leaves the env state of te_observe_wingman -> te_policy_act (eps NULL) -> clamp ->
te_set_wingman_actions, step after step, and its mu is te_policy_act's."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests._policy_cases import StubEnv


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbol_is_exported(lib):
    from dronechase_amd import _lib
    assert "te_drive_wingman" in _lib.EXPORTS
    assert hasattr(lib, "te_drive_wingman")


def test_null_env_is_an_error(lib):
    rc = lib.te_drive_wingman(None, 1, None, 3, None, None, None, None, None)
    assert rc != 0
    assert b"te_drive_wingman" in lib.te_last_error()


def test_ppo_config_default_has_no_wingman_driver():
    from dronechase_amd.ppo import PPOConfig
    assert PPOConfig().wingman_driver == "none" and PPOConfig().wingman_sync_every == 1


def test_caller_driven_pursuers(lib):
    from dronechase_amd import default_config
    from dronechase_amd.ppo import caller_driven_pursuers
    assert caller_driven_pursuers(default_config("exp05")) == [1]
    assert caller_driven_pursuers(default_config("stage03")) == []
    assert caller_driven_pursuers(None) == []


def test_ppo_wingman_driver_argument_errors(lib):
    from dronechase_amd.ppo import PPO, LidarInertialActionPolicy, PPOConfig
    with pytest.raises(ValueError, match="PPO drives the agent only"):
        PPO(StubEnv("exp05"), PPOConfig(n_steps=2))
    with pytest.raises(ValueError, match="needs a GPU device"):
        PPO(StubEnv("exp05"), PPOConfig(n_steps=2, wingman_driver="snapshot"))
    with pytest.raises(ValueError, match="no caller-driven pursuer"):
        PPO(StubEnv("stage03"), PPOConfig(n_steps=2, wingman_driver="snapshot"))
    with pytest.raises(ValueError, match="wingman_driver must be"):
        PPO(StubEnv("exp05"), PPOConfig(n_steps=2, wingman_driver="latest"))
    with pytest.raises(ValueError, match="pass wingman_policy with wingman_driver='none'"):
        PPO(StubEnv("exp05"), PPOConfig(n_steps=2, wingman_driver="snapshot"), wingman_policy=LidarInertialActionPolicy())


# ---------------------------------------------------------------------------------------------------------- GPU
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _policy(seed, c=3):
    """Random weights whose mean leaves [-1, 1] in a share of the rows, so the clamp matters."""
    torch = _gpu()
    from dronechase_amd.ppo import LidarInertialActionPolicy
    torch.manual_seed(seed)
    p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26))
    with torch.no_grad():
        p.mu.weight.mul_(8.0)
        p.mu.bias.copy_(torch.tensor([0.5, -0.5, 0.2, 0.3]))
    return p.cuda().requires_grad_(False)


def _drone_words(env, state):
    from dronechase_amd import config as K
    return state[: env.N * env.D * K.DRONE_WORDS].view(env.N, env.D, K.DRONE_WORDS)


def _clamp(torch, mu):
    low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device=mu.device)
    return torch.max(torch.min(mu, torch.ones_like(mu)), low)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 16384])
def test_drive_matches_the_four_call_sequence_bitwise(n):
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    cfg = default_config("exp05", n_envs=n, motor_noise=1, seed=17, max_step=14)   # short episodes: auto-resets inside 40 steps
    A, B = BatchedEnv(cfg, "cuda:0"), BatchedEnv(cfg, "cuda:0")
    A.reset(); B.reset()
    fp = FusedPolicy(_policy(5))
    mu_a = torch.full((n, 4), float("nan"), device="cuda:0")
    kill = torch.arange(n, device="cuda:0") % 7 == 3
    ARMED, SP, ACT = K.D["ARMED"], K.D["SETPOINT"], K.D["ALLY_ACTION"]
    dead_rows = resets = 0
    for step in range(40):
        if step == 6:   # kill the ally in every 7th env of both (the same words): dead allies from here on, until their env resets
            for env in (A, B):
                s = env.get_state()
                _drone_words(env, s)[kill, 1, ARMED] = 0
                env.set_state(s)
        before = _drone_words(A, A.get_state()).clone()
        A.drive_wingman(1, fp, mu=mu_a)
        lidar, inertial, last_action, _active = B.observe_wingman(1)
        mu_b, _ = fp.forward({"lidar": lidar, "inertial_data": inertial, "last_action": last_action})
        B.set_wingman_actions(1, _clamp(torch, mu_b).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(mu_a.view(torch.int32), mu_b.view(torch.int32)), f"mu differs from te_policy_act's at step {step}"
        after = _drone_words(A, A.get_state())
        assert torch.equal(after, _drone_words(B, B.get_state())), f"state after the drive differs at step {step}"
        dead = before[:, 1, ARMED] == 0
        dead_rows += int(dead.sum())
        # a dead ally is not driven: its set-point and last action stay
        assert torch.equal(after[dead, 1, SP:SP + 4], before[dead, 1, SP:SP + 4])
        assert torch.equal(after[dead, 1, ACT:ACT + 4], before[dead, 1, ACT:ACT + 4])
        live = ~dead
        assert torch.equal(after[live, 1, ACT:ACT + 4].view(torch.float32), _clamp(torch, mu_a)[live])
        acts = A.random_actions(29, step)
        A.step(acts, terminal=False); B.step(acts, terminal=False)
        resets += int(A.done.sum())
        assert torch.equal(A.get_state(), B.get_state()), f"state after te_step differs at step {step}"
    assert dead_rows > 0 and resets > 0, (dead_rows, resets)
    A.close(); B.close()


@pytest.mark.gpu
def test_graph_capture_and_weight_sync():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    n = 1024
    cfg = default_config("exp05", n_envs=n, motor_noise=1, seed=3)
    G, R = BatchedEnv(cfg, "cuda:0"), BatchedEnv(cfg, "cuda:0")
    G.reset(); R.reset()
    p1, p2 = _policy(1), _policy(2)
    fg, fr = FusedPolicy(copy.deepcopy(p1)), FusedPolicy(copy.deepcopy(p1))
    mu_g, mu_r = torch.empty((n, 4), device="cuda:0"), torch.empty((n, 4), device="cuda:0")
    acts = G.random_actions(7, 0)
    for s in range(3):   # a few steps in: the ally sees the others
        a = G.random_actions(8, s)
        G.drive_wingman(1, fg); G.step(a, terminal=False)
    R.set_state(G.get_state())
    s0 = G.get_state().clone()

    def step_once():
        G.drive_wingman(1, fg, mu=mu_g)
        G.step(acts, terminal=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step_once()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step_once()
    G.set_state(s0)

    graph.replay()
    R.drive_wingman(1, fr, mu=mu_r); R.step(acts, terminal=False)
    torch.cuda.synchronize()
    assert torch.equal(G.get_state(), R.get_state()) and torch.equal(mu_g, mu_r)
    # sync new weights in place: the captured graph flies them
    address = fg.params.data_ptr()
    fg.load_from(p2); fr.load_from(p2)
    assert fg.params.data_ptr() == address
    graph.replay()
    R.drive_wingman(1, fr, mu=mu_r); R.step(acts, terminal=False)
    torch.cuda.synchronize()
    assert torch.equal(G.get_state(), R.get_state()) and torch.equal(mu_g, mu_r)
    ref, _ = FusedPolicy(p2).forward({k: v for k, v in zip(("lidar", "inertial_data", "last_action"), G.wingman_scratch(1))})
    assert torch.equal(mu_g, ref)
    G.close(); R.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("fused_forward", [False, True])
@pytest.mark.parametrize("driver", ["snapshot", "module"])
def test_ppo_trains_on_exp05(use_graph, fused_forward, driver):
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, pack_policy

    n, T = 4096, 8
    env = BatchedEnv(default_config("exp05", n_envs=n, seed=5), "cuda:0")
    frozen = _policy(9) if driver == "module" else None
    frozen_packed = None if frozen is None else pack_policy(frozen).clone()
    cfg = PPOConfig(n_steps=T, batch_size=8192, n_epochs=2, use_graph=use_graph, fused_forward=fused_forward,
                    wingman_driver="snapshot" if driver == "snapshot" else "none")
    ppo = PPO(env, cfg, seed=1, wingman_policy=frozen)
    assert ppo.wingmen == [1]
    before = [p.detach().clone() for p in ppo.policy.parameters()]
    ACT, ARMED = K.D["ALLY_ACTION"], K.D["ARMED"]
    ally_actions = []
    for it in range(2):
        ppo.collect()
        torch.cuda.synchronize()
        if driver == "snapshot":   # the copy was synced at the start of this collect
            assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
        else:
            assert torch.equal(ppo.wingman.params, frozen_packed)
        # the ally was driven by the frozen policy on the last state it observed: its remembered action is the clamped mean
        words = _drone_words(env, env.get_state())
        live = (words[:, 1, ARMED] != 0) & (ppo.buf.dones[-1] == 0)
        assert int(live.sum()) > 0
        mu = ppo._wingman_mu[1]
        lidar, inertial, last_action = env.wingman_scratch(1)
        ref, _ = ppo.wingman.forward({"lidar": lidar, "inertial_data": inertial, "last_action": last_action})
        assert torch.equal(mu, ref)
        assert torch.equal(words[live, 1, ACT:ACT + 4].view(torch.float32), _clamp(torch, mu)[live])
        ally_actions.append(words[:, 1, ACT:ACT + 4].clone())
        u = ppo.update()
        assert all(np.isfinite(v) for v in u.values()), u
        if driver == "snapshot":   # the learner moved, the ally did not
            assert not torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
    assert not torch.equal(ally_actions[0], ally_actions[1])
    assert any(not torch.equal(a, b) for a, b in zip(before, ppo.policy.parameters()))
    if frozen is not None:
        assert torch.equal(pack_policy(frozen), frozen_packed) and torch.equal(ppo.wingman.params, frozen_packed)
    assert all(p.grad is None for p in ppo.wingman.policy.parameters())
    # the env step counters advanced by exactly the collected steps (the graph's warm-up and capture steps were rolled back,
    # the ally's set-point with them: it lives in the state blob)
    w = env.get_state()
    steps = w[n * env.D * K.DRONE_WORDS:].view(n, K.ENV_WORDS)[:, K.E["STEP"]]
    assert int(steps.max()) <= 2 * T and int(steps.max()) >= T
    env.close()


@pytest.mark.gpu
def test_ppo_sync_every_and_explicit_sync():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, pack_policy

    env = BatchedEnv(default_config("exp05", n_envs=1024, seed=2), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=4, batch_size=4096, n_epochs=1, wingman_driver="snapshot", wingman_sync_every=2), seed=4)
    first = ppo.wingman.params.clone()
    ppo.collect(); ppo.update(); ppo.collect()         # one update: not yet synced
    assert torch.equal(ppo.wingman.params, first)
    ppo.update(); ppo.collect()                         # two updates: synced
    assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
    ppo.update(); ppo.sync_wingmen()
    assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
    env.close()


@pytest.mark.gpu
def test_ppo_without_a_wingman_driver_still_refuses_exp05():
    _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO

    env = BatchedEnv(default_config("exp05", n_envs=64), "cuda:0")
    with pytest.raises(ValueError, match="PPO drives the agent only: an environment with caller-driven wingmen"):
        PPO(env)
    env.close()


@pytest.mark.gpu
def test_ppo_on_exp05_at_full_size():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig

    n = 65536
    env = BatchedEnv(default_config("exp05", n_envs=n), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=4, batch_size=n, n_epochs=1, fused_forward=True, fused_update=True, wingman_driver="snapshot"), seed=2)
    r = ppo.collect()
    u = ppo.update()
    assert all(np.isfinite(v) for v in list(r.values()) + list(u.values())), (r, u)
    assert bool(torch.isfinite(ppo._wingman_mu[1]).all())
    env.close()


@pytest.mark.gpu
def test_drive_argument_errors_launch_nothing(lib):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    n = 256
    env = BatchedEnv(default_config("exp05", n_envs=n, seed=1), "cuda:0")
    env.reset()
    fp = FusedPolicy(_policy(3))
    lidar, inertial, last_action = env.wingman_scratch(1)
    for t in (lidar, inertial, last_action):
        t.fill_(float("nan"))
    mu = torch.full((n, 4), float("nan"), device="cuda:0")
    big = torch.empty(lidar.numel() + 4, device="cuda:0")        # misaligned views of the right size
    state = env.get_state().clone()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = [p(fp.params), 3, p(lidar), p(inertial), p(last_action), p(mu)]
    cases = {
        "null params": (1, [None] + base[1:]),
        "lidar_channels": (1, base[:1] + [2] + base[2:]),
        "misaligned lidar": (1, base[:2] + [C.c_void_p(big.data_ptr() + 4)] + base[3:]),
        "misaligned last_action": (1, base[:4] + [C.c_void_p(big.data_ptr() + 4)] + base[5:]),
        "not caller-driven (agent)": (0, base),
        "not caller-driven (pursuer 2)": (2, base),
        "out of range": (7, base),
    }
    for name, (wingman, args) in cases.items():
        rc = lib.te_drive_wingman(env._h, wingman, *args, stream)
        assert rc != 0, name
        assert lib.te_last_error().startswith(b"te_drive_wingman"), (name, lib.te_last_error())
    torch.cuda.synchronize()
    assert torch.equal(env.get_state(), state)
    for t in (lidar, inertial, last_action, mu):
        assert bool(torch.isnan(t).all())
    with pytest.raises(Exception, match="te_drive_wingman"):
        env.drive_wingman(0, fp)
    env.close()
    # a stage03 env has no caller-driven pursuer at all
    s3 = BatchedEnv(default_config("stage03", n_envs=n, seed=1), "cuda:0")
    s3.reset()
    state = s3.get_state().clone()
    for w in (0, 1, 2):
        assert lib.te_drive_wingman(s3._h, w, *base, stream) != 0
        assert b"not driven by the caller" in lib.te_last_error()
    torch.cuda.synchronize()
    assert torch.equal(s3.get_state(), state)
    s3.close()
