"""te_policy_act (dronechase_amd/csrc/te_policy.hpp): the PPO policy's forward, sample, log-prob and action clamp in one HIP
launch, and the layers above it (FusedPolicy, PPOConfig.fused_forward, PolicyDriver(fused=True)).

Tolerance: |d| <= 1e-4 + 1e-4 |ref| against the PyTorch module in fp32.  The kernel sums in another order than rocBLAS / MIOpen, so
it is not bit-exact; the measured gap over every parity case below is printed (pytest -s): on the MI355X the largest |d| was
1.5e-7 on mu and 1.2e-7 on value, 0.1 % of the bound."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from tests._policy_cases import _gpu, _obs, _policy, _trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = RTOL = 1e-4

# the layout include/threatengage.h documents for te_policy_act's parameter buffer
LAYOUT = ["lidar.0.weight", "lidar.0.bias", "lidar.2.weight", "lidar.2.bias"] + \
    [f"{m}.{i}.{w}" for m in ("inertial", "action") for i in (0, 2, 4) for w in ("weight", "bias")] + \
    ["final.0.weight", "final.0.bias"] + [f"{m}.{i}.{w}" for m in ("pi", "vf") for i in (0, 2) for w in ("weight", "bias")] + \
    ["mu.weight", "mu.bias", "value.weight", "value.bias", "log_std"]


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_param_words(lib):
    from dronechase_amd.ppo import LidarInertialActionPolicy, policy_param_words
    assert policy_param_words(3) == 235049
    assert policy_param_words(2) == 235049 - 512 == 234537
    # from the layer shapes: conv1 32 * 16 C + 32, conv2 8 256, the inertial chain 35 072, the action chain 33 664, the trunk 114 944,
    # two heads of 20 608, mu 260, value 65, log_std 4
    for c in (2, 3):
        assert policy_param_words(c) == (32 * 16 * c + 32) + 8256 + 35072 + 33664 + 114944 + 2 * 20608 + 260 + 65 + 4
    for c in (2, 3):
        p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26))
        assert sum(x.numel() for x in p.parameters()) == policy_param_words(c)


def test_packed_layout_round_trips(lib):
    import torch
    from dronechase_amd.ppo import LidarInertialActionPolicy, pack_policy
    torch.manual_seed(0)
    for c in (2, 3):
        p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26))
        with torch.no_grad():
            p.log_std.copy_(torch.tensor([0.1, -0.2, 0.3, -0.4]))
        named = dict(p.named_parameters())
        assert sorted(named) == sorted(LAYOUT)
        buf = pack_policy(p)
        off = 0
        for name in LAYOUT:
            t = named[name]
            assert torch.equal(buf[off:off + t.numel()].view_as(t), t.detach()), name
            off += t.numel()
        assert off == buf.numel()
        out = torch.full_like(buf, float("nan"))
        ptr = out.data_ptr()
        assert pack_policy(p, out=out).data_ptr() == ptr and torch.equal(out, buf)   # in place: the address a graph captured


def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    header = open(os.path.join(ROOT, "include", "threatengage.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("te_policy_param_words", "te_policy_act"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None


def test_bad_arguments_fail_through_last_error(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    out = C.c_size_t()
    assert lib.te_policy_param_words(4, C.byref(out)) != 0 and b"lidar_channels" in lib.te_last_error()
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    args = lambda **kw: [kw.get(k, v) for k, v in dict(params=fake, ch=3, n=8, lidar=fake, inertial=fake, last_action=fake, eps=None,
                                                       mu=fake, value=fake, action=None, logp=None, action_env=None, stream=None).items()]
    cases = [(dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"), (dict(ch=1), b"lidar_channels"),
             (dict(ch=4), b"lidar_channels"), (dict(params=fake + 4), b"params must be 16-byte"), (dict(lidar=fake + 4), b"lidar must be 8-byte"),
             (dict(mu=fake + 2), b"4-byte"), (dict(mu=None), b"null"), (dict(eps=fake), b"eps given")]
    for kw, msg in cases:
        assert lib.te_policy_act(*args(**kw)) != 0, kw
        assert msg in lib.te_last_error(), (kw, lib.te_last_error())


# ---------------------------------------------------------------------------------------------------------- MI355X
MARGIN = {"mu": [0.0, 0.0], "value": [0.0, 0.0]}     # largest |d|, largest |d| / (ATOL + RTOL |ref|)


def _check(torch, got, ref, name):
    d = (got - ref).abs()
    m = MARGIN[name]
    m[0] = max(m[0], float(d.max()))
    m[1] = max(m[1], float((d / (ATOL + RTOL * ref.abs())).max()))
    torch.testing.assert_close(got, ref, atol=ATOL, rtol=RTOL, msg=lambda m: f"{name}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 2])
def test_parity_with_the_module(c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    trained, real = _trained_policy(torch, c, n_envs=512, batch_size=1024)      # 8 x 512 = 4 096 real te_step observations
    for label, policy in (("random", _policy(torch, c, 5)), ("trained", trained)):
        fused = FusedPolicy(policy)
        sources = [("random", n, _obs(torch, n, c, n)) for n in (1, 63, 64, 65, 4097, 65536)]
        sources.append(("te_step", 4096, real))
        sources.append(("te_step", 65, {k: v[1000:1065].contiguous() for k, v in real.items()}))
        for src, n, obs in sources:
            with torch.no_grad():
                mu_ref, v_ref = policy(obs)
            mu, v = fused.forward(obs)
            torch.cuda.synchronize()
            _check(torch, mu, mu_ref, "mu"); _check(torch, v, v_ref, "value")
    print(f"\nlidar_channels={c}: largest |d| so far: mu {MARGIN['mu'][0]:.2e}, value {MARGIN['value'][0]:.2e}; "
          f"largest fraction of the bound: mu {MARGIN['mu'][1]:.3f}, value {MARGIN['value'][1]:.3f}")


# SHA-256 of mu | value | action | logp | action_env of the call below, recorded from the library of commit 66a9492 on the MI355X:
# the kernel is bitwise deterministic for fixed inputs, so a refactor of the policy's description leaves these as they are
ACT_DIGEST = {2: "c65548f19cb5066403dce312d88165d7466a647245979699cef1607c3d57e068",
              3: "19215395f089bdf7311d472effa4f7e15abdde3eb5b38c24ffc96ea79bdf1aa4"}


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
def test_act_is_bitwise_the_recorded_one(lib, c):
    """n = 33: two tiles, the second with one live row and 31 padding rows.  Every input comes from numpy's PCG64, through the raw ABI."""
    torch = _gpu()
    n = 33
    rng = np.random.default_rng(1000 + c)
    u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32)).to("cuda:0")
    words = C.c_size_t()
    assert lib.te_policy_param_words(c, C.byref(words)) == 0
    params = u(-0.1, 0.1, words.value)
    lidar, inertial, last_action, eps = u(0, 1, n, c, 13, 26), u(-1, 1, n, 15), u(-1, 1, n, 4), u(-2, 2, n, 4)
    outs = [torch.full(s, float("nan"), device="cuda:0") for s in ((n, 4), (n,), (n, 4), (n,), (n, 4))]   # mu value action logp action_env
    rc = lib.te_policy_act(params.data_ptr(), c, n, lidar.data_ptr(), inertial.data_ptr(), last_action.data_ptr(), eps.data_ptr(),
                           *[t.data_ptr() for t in outs], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.te_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    digest = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in outs)).hexdigest()
    print(f"\nte_policy_act C={c}: {digest}")
    assert digest == ACT_DIGEST[c]


@pytest.mark.gpu
def test_sampling_matches_the_hand_formula():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 7)
    fused = FusedPolicy(p)
    obs = _obs(torch, 4097, 3, 1)
    eps = torch.randn(4097, 4, device="cuda:0") * 2
    a, logp, v, a_env = fused.act(obs, eps)
    mu, v2 = fused.forward(obs)
    assert torch.equal(v, v2)
    log_std = p.log_std.detach()
    torch.testing.assert_close(a, mu + log_std.exp() * eps, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(logp, (-0.5 * eps * eps - log_std - 0.9189385332046727).sum(-1), atol=1e-5, rtol=1e-6)
    low, high = torch.tensor([-1.0, -1.0, -1.0, 0.0], device="cuda:0"), torch.ones(4, device="cuda:0")
    assert torch.equal(a_env, torch.max(torch.min(a, high), low))
    assert bool((a_env != a).any())      # the draw is wide enough that the clamp does something
    with torch.no_grad():
        d, v_ref = p.dist(obs)
        torch.testing.assert_close(logp, d.log_prob(a).sum(-1), atol=ATOL, rtol=RTOL)


@pytest.mark.gpu
def test_rows_are_independent_and_calls_deterministic():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    fused = FusedPolicy(_policy(torch, 3, 9))
    n = 4097
    obs = _obs(torch, n, 3, 3)
    eps = torch.randn(n, 4, device="cuda:0")
    full = fused.act(obs, eps)
    again = fused.act(obs, eps)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    for s in (0, 17, 64, 2000, 4033, 4096):
        part = fused.act({k: v[s:s + 64].contiguous() for k, v in obs.items()}, eps[s:s + 64].contiguous())
        for x, y in zip(full, part):
            assert torch.equal(x[s:s + 64], y), s


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 2])
def test_unused_lidar_cells_change_nothing(c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    fused = FusedPolicy(_policy(torch, c, 11))
    obs = _obs(torch, 300, c, 4)
    eps = torch.randn(300, 4, device="cuda:0")
    ref = fused.act(obs, eps)
    poked = {k: v.clone() for k, v in obs.items()}
    poked["lidar"][:, :, 8:, :] = 1e6
    poked["lidar"][:, :, :, 24:] = -1e6
    for x, y in zip(ref, fused.act(poked, eps)):
        assert torch.equal(x, y)
    poked["lidar"][:, :, 7, 23] += 1.0     # ... and a used cell does
    assert not torch.equal(ref[0], fused.act(poked, eps)[0])


@pytest.mark.gpu
def test_graph_replay_sees_refreshed_weights():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 13)
    fused = FusedPolicy(p)
    obs = _obs(torch, 1000, 3, 5)
    eps = torch.randn(1000, 4, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.act(obs, eps)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fused.act(obs, eps)
    g.replay(); torch.cuda.synchronize()
    first = [t.clone() for t in out]
    with torch.no_grad():
        torch.testing.assert_close(out[2], p(obs)[1], atol=ATOL, rtol=RTOL)
        for q in p.parameters():
            q.add_(0.01 * torch.randn_like(q))
    g.replay(); torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, out))     # not refreshed: the buffer still holds the old weights
    fused.refresh()
    g.replay(); torch.cuda.synchronize()
    with torch.no_grad():
        mu_ref, v_ref = p(obs)
    torch.testing.assert_close(out[2], v_ref, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(out[0], mu_ref + p.log_std.detach().exp() * eps, atol=ATOL, rtol=RTOL)
    assert not torch.equal(first[2], out[2])


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False])
def test_ppo_fused_forward(use_graph):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=512, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=16, batch_size=2048, n_epochs=2, use_graph=use_graph, fused_forward=True), seed=1)
    before = [q.detach().clone() for q in ppo.policy.parameters()]
    logs = []
    ppo.learn(3 * 16 * 512, log=logs.append)     # the third collect replays the graph on weights two updates moved
    assert len(logs) == 3
    for rec in logs:
        assert all(np.isfinite(v) for v in rec.values() if isinstance(v, float)), rec
    assert any(not torch.equal(a, q.detach()) for a, q in zip(before, ppo.policy.parameters()))
    ppo.collect()          # learn() ended with update(): this rollout must run on the moved weights (collect() refreshes the buffer)
    b = ppo.buf
    T, N = b.rewards.shape
    with torch.no_grad():
        d, v = ppo.policy.dist({k: o.reshape(T * N, *o.shape[2:]) for k, o in b.obs.items()})
        logp = d.log_prob(b.actions.reshape(T * N, 4)).sum(-1)
    torch.testing.assert_close(b.values.reshape(-1), v, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(b.logp.reshape(-1), logp, atol=ATOL, rtol=RTOL)
    env.close()


@pytest.mark.gpu
def test_policy_driver_fused_on_exp05():
    torch = _gpu()
    from dronechase_amd.envs import Exp05vFinalEnvironment
    from dronechase_amd.pipeline import ReinforcementLearningPipeline
    from dronechase_amd.ppo import PolicyDriver
    n = 128
    v = ReinforcementLearningPipeline.create_vectorized_environment(Exp05vFinalEnvironment, {"dome_radius": 20, "rl_frequency": 15},
                                                                    n_envs=n, monitor=False)
    v.reset()
    policy = _policy(torch, 3, 17)
    plain, fused = PolicyDriver(policy), PolicyDriver(policy, fused=True)
    v.env_method("update_model", fused)
    a = np.tile(np.array([[0.3, -0.2, 0.1, 0.5]], np.float32), (n, 1))
    for _ in range(4):
        lidar, inertial, last_action, _active = v.backend.observe_ally()
        obs = {"lidar": lidar, "inertial_data": inertial, "last_action": last_action}
        got, _ = fused.predict(obs, deterministic=True)
        ref, _ = plain.predict(obs, deterministic=True)
        torch.testing.assert_close(got, ref, atol=ATOL, rtol=RTOL)
        sampled, _ = fused.predict(obs, deterministic=False)
        assert bool((sampled[:, :3] >= -1).all() and (sampled[:, 3] >= 0).all() and (sampled <= 1).all())
        v.step(a)
    v.close()
