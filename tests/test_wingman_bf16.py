"""te_drive_wingman_bf16: te_drive_wingman_shaped with te_policy_act_bf16's forward (policy_drive_bf16_kernel, te_wingman.hpp), and
the layers above it: BatchedEnv.drive_wingman with a FusedPolicy(precision="bf16"), PPOConfig.wingman_bf16, evaluate_policy.

The main check is bitwise, as in tests/test_wingman_policy.py: the call leaves the env state of te_observe_wingman ->
te_policy_act_bf16 (eps NULL) -> clamp -> te_set_wingman_actions, step after step, and its mu is te_policy_act_bf16's.  1 000 envs
are a multiple of neither tile height (32 rows for the default shape, 48 for the wide ones): the last workgroup has rows past n."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests._policy_cases import DEFAULT, StubEnv, _shape
from tests.test_wingman_policy import _clamp, _drone_words, _gpu

BO = (512, (128, 256, 512))
LEARN = (512, (512, 128, 256))
FAKE = 1 << 20          # aligned to everything the entry asks for; never dereferenced


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbol_and_error_prefix(lib):
    from dronechase_amd import _lib
    assert "te_drive_wingman_bf16" in _lib.EXPORTS and hasattr(lib, "te_drive_wingman_bf16")
    bo = _shape(3, *BO)
    assert lib.te_drive_wingman_bf16(None, 1, FAKE, FAKE, C.byref(bo), FAKE, FAKE, FAKE, None, None) != 0
    assert lib.te_last_error().startswith(b"te_drive_wingman_bf16"), lib.te_last_error()
    # the shape is checked on the host before the env is looked at: an unserved one is refused with the served list
    for bad, field in ((_shape(3, 512, (128, 256)), b"hidden"), (_shape(3, 300, (64, 64)), b"features_dim"), (_shape(4, *BO), b"lidar_channels")):
        assert lib.te_drive_wingman_bf16(FAKE, 1, FAKE, FAKE, C.byref(bad), FAKE, FAKE, FAKE, None, None) != 0
        msg = lib.te_last_error()
        assert msg.startswith(b"te_drive_wingman_bf16") and field in msg, msg
        assert b"128, 256, 512" in msg and b"512, 128, 256" in msg and b"64, 64" in msg, msg
    assert lib.te_drive_wingman_bf16(FAKE, 1, FAKE, FAKE, None, FAKE, FAKE, FAKE, None, None) != 0
    assert lib.te_last_error().startswith(b"te_drive_wingman_bf16") and b"null shape" in lib.te_last_error()


def test_ppo_config_default():
    from dronechase_amd.ppo import PPOConfig
    assert PPOConfig().wingman_bf16 is False


def test_wingman_bf16_needs_a_driver_stub(lib):
    from dronechase_amd.ppo import PPO, PPOConfig
    for task in ("stage03", "exp05"):
        with pytest.raises(ValueError, match="wingman_bf16"):
            PPO(StubEnv(task), PPOConfig(n_steps=2, wingman_bf16=True))


# ---------------------------------------------------------------------------------------------------------- GPU
def _policy(seed, shape=DEFAULT, c=3):
    """Random weights whose mean leaves [-1, 1] in a share of the rows, so the clamp matters."""
    torch = _gpu()
    from dronechase_amd.ppo import LidarInertialActionPolicy
    torch.manual_seed(seed)
    p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=shape[0], net_arch=shape[1])
    with torch.no_grad():
        p.mu.weight.mul_(8.0)
        p.mu.bias.copy_(torch.tensor([0.5, -0.5, 0.2, 0.3]))
    return p.cuda().requires_grad_(False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape, c", [(DEFAULT, 3), (BO, 3), (LEARN, 3), (DEFAULT, 2)], ids=["default", "bo", "learn", "default-c2"])
def test_drive_bf16_matches_the_four_call_sequence_bitwise(shape, c):
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    n = 1000
    cfg = default_config("exp05", n_envs=n, motor_noise=1, seed=17, max_step=14, lidar_channels=c)   # short episodes: auto-resets inside 40 steps
    A, B = BatchedEnv(cfg, "cuda:0"), BatchedEnv(cfg, "cuda:0")
    A.reset(); B.reset()
    assert tuple(A.lidar.shape[1:]) == (c, 13, 26)
    policy = _policy(5, shape, c)
    fp, f32 = FusedPolicy(policy, precision="bf16"), FusedPolicy(policy)
    assert fp.precision == "bf16" and fp.weights_bf16 is not None
    mu_a = torch.full((n, 4), float("nan"), device="cuda:0")
    kill = torch.arange(n, device="cuda:0") % 7 == 3
    ARMED, SP, ACT = K.D["ARMED"], K.D["SETPOINT"], K.D["ALLY_ACTION"]
    dead_rows = resets = differs_from_fp32 = 0
    for step in range(40):
        if step == 6:   # kill the ally in every 7th env of both (the same words): dead allies from here on, until their env resets
            for env in (A, B):
                s = env.get_state()
                _drone_words(env, s)[kill, 1, ARMED] = 0
                env.set_state(s)
        before = _drone_words(A, A.get_state()).clone()
        A.drive_wingman(1, fp, mu=mu_a)
        lidar, inertial, last_action, _active = B.observe_wingman(1)
        obs = {"lidar": lidar, "inertial_data": inertial, "last_action": last_action}
        mu_b, _ = fp.forward(obs)
        B.set_wingman_actions(1, _clamp(torch, mu_b).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(mu_a.view(torch.int32), mu_b.view(torch.int32)), f"mu differs from te_policy_act_bf16's at step {step}"
        after = _drone_words(A, A.get_state())
        assert torch.equal(after, _drone_words(B, B.get_state())), f"state after the drive differs at step {step}"
        dead = before[:, 1, ARMED] == 0
        dead_rows += int(dead.sum())
        # a dead ally is not driven: its set-point and last action stay
        assert torch.equal(after[dead, 1, SP:SP + 4], before[dead, 1, SP:SP + 4])
        assert torch.equal(after[dead, 1, ACT:ACT + 4], before[dead, 1, ACT:ACT + 4])
        live = ~dead
        assert torch.equal(after[live, 1, ACT:ACT + 4].view(torch.float32), _clamp(torch, mu_a)[live])
        if step in (0, 5):   # the bf16 kernel really ran: on the same observation the fp32 launch gives other bits
            mu_32, _ = f32.forward(obs)
            differs_from_fp32 += int((mu_32.view(torch.int32) != mu_a.view(torch.int32)).any(dim=1).sum())
        acts = A.random_actions(29, step)
        A.step(acts, terminal=False); B.step(acts, terminal=False)
        resets += int(A.done.sum())
        assert torch.equal(A.get_state(), B.get_state()), f"state after te_step differs at step {step}"
    assert dead_rows > 0 and resets > 0, (dead_rows, resets)
    assert differs_from_fp32 > 0
    A.close(); B.close()


@pytest.mark.gpu
def test_graph_capture_and_weight_sync_bf16():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    n = 1024
    cfg = default_config("exp05", n_envs=n, motor_noise=1, seed=3)
    G, R = BatchedEnv(cfg, "cuda:0"), BatchedEnv(cfg, "cuda:0")
    G.reset(); R.reset()
    p1, p2 = _policy(1, BO), _policy(2, BO)
    fg, fr = FusedPolicy(copy.deepcopy(p1), precision="bf16"), FusedPolicy(copy.deepcopy(p1), precision="bf16")
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
    first = mu_g.clone()
    # sync new weights in place: the captured graph flies them, the fp32 buffer and the bf16 one
    address, address_bf16 = fg.params.data_ptr(), fg.weights_bf16.data_ptr()
    fg.load_from(p2); fr.load_from(p2)
    assert fg.params.data_ptr() == address and fg.weights_bf16.data_ptr() == address_bf16
    graph.replay()
    R.drive_wingman(1, fr, mu=mu_r); R.step(acts, terminal=False)
    torch.cuda.synchronize()
    assert torch.equal(G.get_state(), R.get_state()) and torch.equal(mu_g, mu_r)
    ref, _ = FusedPolicy(p2, precision="bf16").forward({k: v for k, v in zip(("lidar", "inertial_data", "last_action"), G.wingman_scratch(1))})
    assert torch.equal(mu_g, ref) and not torch.equal(mu_g, first)
    G.close(); R.close()


@pytest.mark.gpu
def test_drive_bf16_argument_errors_launch_nothing(lib):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy

    n = 256
    env = BatchedEnv(default_config("exp05", n_envs=n, seed=1), "cuda:0")
    env.reset()
    fp = FusedPolicy(_policy(3), precision="bf16")
    lidar, inertial, last_action = env.wingman_scratch(1)
    for t in (lidar, inertial, last_action):
        t.fill_(float("nan"))
    mu = torch.full((n, 4), float("nan"), device="cuda:0")
    big = torch.empty(lidar.numel() + 4, device="cuda:0")        # misaligned views of the right size
    state = env.get_state().clone()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    c2 = _shape(2, *DEFAULT)
    base = [p(fp.params), p(fp.weights_bf16), C.byref(fp.shape), p(lidar), p(inertial), p(last_action), p(mu)]
    cases = {
        "null weights_bf16": (1, base[:1] + [None] + base[2:]),
        "misaligned weights_bf16": (1, base[:1] + [C.c_void_p(fp.weights_bf16.data_ptr() + 8)] + base[2:]),
        "null params": (1, [None] + base[1:]),
        "lidar_channels": (1, base[:2] + [C.byref(c2)] + base[3:]),
        "misaligned lidar": (1, base[:3] + [C.c_void_p(big.data_ptr() + 4)] + base[4:]),
        "misaligned last_action": (1, base[:5] + [C.c_void_p(big.data_ptr() + 4)] + base[6:]),
        "not caller-driven (agent)": (0, base),
        "not caller-driven (pursuer 2)": (2, base),
        "out of range": (7, base),
    }
    for name, (wingman, args) in cases.items():
        rc = lib.te_drive_wingman_bf16(env._h, wingman, *args, stream)
        assert rc != 0, name
        assert lib.te_last_error().startswith(b"te_drive_wingman_bf16"), (name, lib.te_last_error())
    torch.cuda.synchronize()
    assert torch.equal(env.get_state(), state)
    for t in (lidar, inertial, last_action, mu):
        assert bool(torch.isnan(t).all())
    with pytest.raises(Exception, match="te_drive_wingman_bf16"):
        env.drive_wingman(0, fp)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("driver", ["snapshot", "module"])
def test_ppo_trains_on_exp05_with_a_bf16_wingman(use_graph, driver):
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, pack_policy

    n, T = 4096, 8
    env = BatchedEnv(default_config("exp05", n_envs=n, seed=5), "cuda:0")
    frozen = _policy(9) if driver == "module" else None
    frozen_packed = None if frozen is None else pack_policy(frozen).clone()
    cfg = PPOConfig(n_steps=T, batch_size=8192, n_epochs=2, use_graph=use_graph, wingman_bf16=True,
                    wingman_driver="snapshot" if driver == "snapshot" else "none")
    ppo = PPO(env, cfg, seed=1, wingman_policy=frozen)
    assert ppo.wingmen == [1] and ppo.wingman.precision == "bf16" and ppo.wingman.weights_bf16 is not None
    address, address_bf16 = ppo.wingman.params.data_ptr(), ppo.wingman.weights_bf16.data_ptr()
    ACT, ARMED = K.D["ALLY_ACTION"], K.D["ARMED"]
    ally_actions = []
    for it in range(2):
        ppo.collect()
        torch.cuda.synchronize()
        if driver == "snapshot":   # the copy was synced at the start of this collect
            assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
        else:
            assert torch.equal(ppo.wingman.params, frozen_packed)
        # the ally was driven by the frozen policy on the last state it observed: its remembered action is the clamped bf16 mean.
        # ppo.wingman.forward reads the bf16 buffer the drive read, so this also holds the repack after the sync to account
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
    assert (ppo.wingman.params.data_ptr(), ppo.wingman.weights_bf16.data_ptr()) == (address, address_bf16)
    if frozen is not None:
        assert torch.equal(pack_policy(frozen), frozen_packed) and torch.equal(ppo.wingman.params, frozen_packed)
    w = env.get_state()
    steps = w[n * env.D * K.DRONE_WORDS:].view(n, K.ENV_WORDS)[:, K.E["STEP"]]
    assert int(steps.max()) <= 2 * T and int(steps.max()) >= T
    env.close()


@pytest.mark.gpu
def test_wingman_bf16_needs_a_driver():
    _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig

    env = BatchedEnv(default_config("stage03", n_envs=64), "cuda:0")
    with pytest.raises(ValueError, match="wingman_bf16"):
        PPO(env, PPOConfig(n_steps=2, wingman_bf16=True))
    env.close()


@pytest.mark.gpu
def test_evaluate_policy_on_exp05_with_a_bf16_wingman():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.ppo import FusedPolicy

    n = 256
    env = BatchedEnv(default_config("exp05", n_envs=n, seed=4, max_step=20), "cuda:0")
    wingman = FusedPolicy(_policy(6), precision="bf16")
    calls = []
    drive = env.drive_wingman
    env.drive_wingman = lambda w, fp, **kw: (calls.append(fp), drive(w, fp, **kw))[1]
    returns, lengths = evaluate_policy(_policy(7), env, n_eval_episodes=16, wingman_policy=wingman)
    assert returns.shape == (16,) and lengths.shape == (16,)
    assert bool(np.isfinite(returns).all()) and bool((lengths > 0).all())
    assert calls and all(fp is wingman for fp in calls)      # the object is passed through: the drive was te_drive_wingman_bf16's
    env.close()
