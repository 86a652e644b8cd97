"""The fused policy inference over the served network shapes (te_policy_act_shaped, te_drive_wingman_shaped,
dronechase_amd/csrc/te_policy.hpp pol_shape): the default (features_dim 256, heads 64, 64) and the two the reference trains,
features_dim 512 with heads (128, 256, 512) ("reference BO") and (512, 128, 256) ("reference learn"); and the layers above them
(LidarInertialActionPolicy(net_arch=), FusedPolicy, PPOConfig.features_dim / net_arch, load_sb3_policy).

Tolerance: |d| <= 1e-4 + 1e-4 |ref| against the PyTorch module in fp32, the bound of tests/test_policy_fused.py.  The measured gap
over every parity case below is printed (pytest -s): on the MI355X the largest |d| was 1.8e-7 on mu and 1.9e-7 on value,
0.2 % of the bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._policy_cases import DEFAULT, StubEnv, _gpu, _obs, _policy, _shape, _trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = RTOL = 1e-4

BO = (512, (128, 256, 512))
LEARN = (512, (512, 128, 256))
SERVED = {"default": DEFAULT, "reference BO": BO, "reference learn": LEARN}
TILE_ROWS = {DEFAULT: 32, BO: 16, LEARN: 16}      # rows per workgroup (te_policy.hpp pol_lds_plan)


def layout(net_arch):
    """The packed order include/threatengage.h documents, for a head of len(net_arch) hidden layers."""
    return ["lidar.0.weight", "lidar.0.bias", "lidar.2.weight", "lidar.2.bias"] + \
        [f"{m}.{i}.{w}" for m in ("inertial", "action") for i in (0, 2, 4) for w in ("weight", "bias")] + \
        ["final.0.weight", "final.0.bias"] + \
        [f"{m}.{2 * i}.{w}" for m in ("pi", "vf") for i in range(len(net_arch)) for w in ("weight", "bias")] + \
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
    assert policy_param_words(3) == 235049 and policy_param_words(2) == 234537
    for c in (2, 3):
        for f, arch in SERVED.values():
            # conv1, conv2, the inertial chain, the action chain, the trunk, two heads, mu, value, log_std
            widths = (f,) + arch
            head = sum(a * b + b for a, b in zip(widths, widths[1:]))
            by_hand = (32 * 16 * c + 32) + 8256 + 35072 + 33664 + (448 * f + f) + 2 * head + (4 * arch[-1] + 4) + (arch[-1] + 1) + 4
            assert policy_param_words(c, f, arch) == by_hand, (c, f, arch)
            p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=f, net_arch=arch)
            assert sum(x.numel() for x in p.parameters()) == by_hand
    assert policy_param_words(3, *BO) == 771561 and policy_param_words(3, *LEARN) == 1032425


def test_packed_layout_round_trips(lib):
    import torch
    from dronechase_amd.ppo import LidarInertialActionPolicy, pack_policy
    torch.manual_seed(0)
    for c in (2, 3):
        for f, arch in (BO, LEARN):
            p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=f, net_arch=arch)
            with torch.no_grad():
                p.log_std.copy_(torch.tensor([0.1, -0.2, 0.3, -0.4]))
            named = dict(p.named_parameters())
            names = layout(arch)
            assert sorted(named) == sorted(names)
            buf = pack_policy(p)
            off = 0
            for name in names:
                t = named[name]
                assert torch.equal(buf[off:off + t.numel()].view_as(t), t.detach()), name
                off += t.numel()
            assert off == buf.numel()
            out = torch.full_like(buf, float("nan"))
            ptr = out.data_ptr()
            assert pack_policy(p, out=out).data_ptr() == ptr and torch.equal(out, buf)


def test_default_module_is_unchanged(lib):
    import torch
    from dronechase_amd.ppo import LidarInertialActionPolicy, policy_shape
    torch.manual_seed(3)
    a = LidarInertialActionPolicy()
    torch.manual_seed(3)
    b = LidarInertialActionPolicy(features_dim=256, net_arch=(64, 64))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == ["log_std"] + layout((64, 64))[:-1]      # a module's own parameter precedes its children's
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert policy_shape(a) == policy_shape(b) == (3, 256, (64, 64))
    assert policy_shape(LidarInertialActionPolicy(lidar_shape=(2, 13, 26), features_dim=512, net_arch=(512, 128, 256))) == (2, 512, (512, 128, 256))
    for bad in ((), (64,) * 4, (64, 0)):
        with pytest.raises(ValueError, match="net_arch"):
            LidarInertialActionPolicy(net_arch=bad)


def test_shape_check(lib):
    from dronechase_amd.ppo import check_policy_shape
    for c in (2, 3):
        for f, arch in SERVED.values():
            assert lib.te_policy_shape_check(C.byref(_shape(c, f, arch))) == 0, (c, f, arch)
    bad = [(_shape(3, 300, (64, 64)), b"features_dim"), (_shape(3, 256, (64, 64), n_hidden=0), b"n_hidden"),
           (_shape(3, 256, (64, 64, 64, 64)), b"n_hidden"), (_shape(3, 256, (64, 100)), b"hidden"),
           (_shape(3, 512, (128, 256, 100)), b"hidden"), (_shape(4, 256, (64, 64)), b"lidar_channels")]
    words = C.c_size_t()
    for shape, field in bad:
        assert lib.te_policy_shape_check(C.byref(shape)) != 0
        msg = lib.te_last_error()
        assert field in msg and b"128, 256, 512" in msg and b"512, 128, 256" in msg and b"64, 64" in msg, msg   # names the field, lists the served
        assert lib.te_policy_param_words_shaped(C.byref(shape), C.byref(words)) != 0
    assert lib.te_policy_shape_check(None) != 0 and b"null" in lib.te_last_error()
    with pytest.raises(ValueError, match="128, 256, 512"):
        check_policy_shape(3, 512, (128, 256))


def test_shaped_calls_reject_bad_arguments(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    bo = _shape(3, *BO)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(params=fake, shape=C.byref(bo), n=8, lidar=fake, inertial=fake, last_action=fake, eps=None,
                                                       mu=fake, value=fake, action=None, logp=None, action_env=None, stream=None).items()]
    cases = [(dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"), (dict(shape=None), b"null shape"),
             (dict(shape=C.byref(_shape(4, *BO))), b"lidar_channels"), (dict(shape=C.byref(_shape(3, 512, (128, 256)))), b"hidden"),
             (dict(params=fake + 4), b"params must be 16-byte"), (dict(lidar=fake + 4), b"lidar must be 8-byte"),
             (dict(mu=fake + 2), b"4-byte"), (dict(mu=None), b"null"), (dict(eps=fake), b"eps given")]
    for kw, msg in cases:
        assert lib.te_policy_act_shaped(*args(**kw)) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_act_shaped"), (kw, err)
    assert lib.te_drive_wingman_shaped(None, 1, fake, C.byref(bo), fake, fake, fake, None, None) != 0
    assert lib.te_last_error().startswith(b"te_drive_wingman_shaped")


def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    header = open(os.path.join(ROOT, "include", "threatengage.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("te_policy_shape_check", "te_policy_param_words_shaped", "te_policy_act_shaped", "te_drive_wingman_shaped"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None
    assert re.search(r"int32_t lidar_channels, features_dim, n_hidden, hidden\[4\];", body)
    assert C.sizeof(_lib.PolicyShape) == 28


def _sb3_state_dict(policy):
    """`policy`'s weights under the names SB3's MultiInputPolicy gives them, the shared extractor stored three times."""
    ext = {"lidar": "lidar_feature_extractor", "inertial": "inertial_feature_extractor", "action": "action_feature_extractor", "final": "final_layer"}
    top = {"pi": "mlp_extractor.policy_net", "vf": "mlp_extractor.value_net", "mu": "action_net", "value": "value_net"}
    sd = {}
    for name, t in policy.state_dict().items():
        head, _, rest = name.partition(".")
        if head == "log_std":
            sd["log_std"] = t.clone()
        elif head in ext:
            for pre in ("features_extractor", "pi_features_extractor", "vf_features_extractor"):
                sd[f"{pre}.{ext[head]}.{rest}"] = t.clone()
        else:
            sd[f"{top[head]}.{rest}"] = t.clone()
    return sd


def test_load_sb3_policy(lib, tmp_path):
    import io
    import zipfile
    import torch
    from dronechase_amd.ppo import LidarInertialActionPolicy, load_sb3_policy, policy_shape
    torch.manual_seed(11)
    src = LidarInertialActionPolicy(features_dim=BO[0], net_arch=BO[1])
    with torch.no_grad():
        src.log_std.copy_(torch.tensor([0.1, -0.2, 0.3, -0.4]))
    sd = _sb3_state_dict(src)
    assert "mlp_extractor.policy_net.4.weight" in sd and "pi_features_extractor.final_layer.0.bias" in sd and "action_net.bias" in sd
    path = tmp_path / "h[128, 256, 512]_model.zip"
    blob = io.BytesIO()
    torch.save(sd, blob)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", "{}")
        z.writestr("policy.pth", blob.getvalue())
    for source in (sd, str(path)):
        got = load_sb3_policy(source)
        assert policy_shape(got) == (3,) + BO
        want = src.state_dict()
        assert list(got.state_dict()) == list(want)
        for k, t in got.state_dict().items():
            assert torch.equal(t, want[k]), k
    only = {k: v for k, v in sd.items() if not k.startswith(("pi_features_extractor", "vf_features_extractor"))}
    assert policy_shape(load_sb3_policy(only)) == (3,) + BO          # the duplicates are optional
    for gone in ("mlp_extractor.value_net.2.bias", "action_net.weight", "log_std"):
        with pytest.raises(KeyError, match=re.escape(gone)):
            load_sb3_policy({k: v for k, v in only.items() if k != gone})
    with pytest.raises(KeyError, match="features_extractor.lidar_feature_extractor.0.weight"):
        load_sb3_policy({k: v for k, v in only.items() if k != "features_extractor.lidar_feature_extractor.0.weight"})
    for extra in ("mlp_extractor.policy_net.6.weight", "features_extractor.camera.0.weight", "optimizer.state"):
        with pytest.raises(KeyError, match=re.escape(extra)):
            load_sb3_policy({**sd, extra: torch.zeros(4, 4)})
    differs = dict(sd)
    differs["pi_features_extractor.final_layer.0.bias"] = sd["pi_features_extractor.final_layer.0.bias"] + 1
    with pytest.raises(ValueError, match="pi_features_extractor.final_layer.0.bias"):
        load_sb3_policy(differs)


def test_fused_update_refuses_other_shapes(lib):
    from dronechase_amd.ppo import PPO, LidarInertialActionPolicy, PPOConfig
    assert PPOConfig().features_dim == 256 and PPOConfig().net_arch == (64, 64)
    env = StubEnv()
    with pytest.raises(ValueError, match="gradient kernel.*default shape only"):
        PPO(env, PPOConfig(n_steps=2, fused_update=True, net_arch=(128, 256, 512), features_dim=512))
    with pytest.raises(ValueError, match="gradient kernel.*default shape only"):
        PPO(env, PPOConfig(n_steps=2, fused_update=True, fused_optimizer=True), policy=LidarInertialActionPolicy(features_dim=512, net_arch=LEARN[1]))
    assert env.resets == 0      # the shape check comes before the env is touched


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
@pytest.mark.parametrize("shape", [BO, LEARN], ids=["bo", "learn"])
def test_parity_with_the_module(shape, c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    trained, real = _trained_policy(torch, c, n_envs=512, batch_size=1024, shape=shape)      # 8 x 512 = 4 096 real te_step observations
    M = TILE_ROWS[shape]
    for label, policy in (("random", _policy(torch, c, 5, shape)), ("trained", trained)):
        fused = FusedPolicy(policy)
        assert (fused.features_dim, fused.net_arch) == shape
        sources = [("random", n, _obs(torch, n, c, n)) for n in (1, M - 1, M, M + 1, 2 * M + 1, 4097)]
        sources.append(("te_step", 4096, real))
        sources.append(("te_step", 2 * M + 1, {k: v[1000:1000 + 2 * M + 1].contiguous() for k, v in real.items()}))
        for src, n, obs in sources:
            with torch.no_grad():
                mu_ref, v_ref = policy(obs)
            mu, v = fused.forward(obs)
            torch.cuda.synchronize()
            _check(torch, mu, mu_ref, "mu"); _check(torch, v, v_ref, "value")
    print(f"\nfeatures_dim={shape[0]} net_arch={shape[1]} lidar_channels={c}: largest |d| so far: mu {MARGIN['mu'][0]:.2e}, value {MARGIN['value'][0]:.2e}; "
          f"largest fraction of the bound: mu {MARGIN['mu'][1]:.3f}, value {MARGIN['value'][1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
def test_shaped_entry_with_the_default_shape_is_te_policy_act(lib, c):
    """The inputs of test_policy_fused.py::test_act_is_bitwise_the_recorded_one (n = 33, numpy's PCG64), through both entries."""
    torch = _gpu()
    n = 33
    rng = np.random.default_rng(1000 + c)
    u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32)).to("cuda:0")
    words = C.c_size_t()
    assert lib.te_policy_param_words_shaped(C.byref(_shape(c, *DEFAULT)), C.byref(words)) == 0
    params = u(-0.1, 0.1, words.value)
    lidar, inertial, last_action, eps = u(0, 1, n, c, 13, 26), u(-1, 1, n, 15), u(-1, 1, n, 4), u(-2, 2, n, 4)
    new = lambda: [torch.full(s, float("nan"), device="cuda:0") for s in ((n, 4), (n,), (n, 4), (n,), (n, 4))]
    a, b = new(), new()
    stream = torch.cuda.current_stream().cuda_stream
    ins = (lidar.data_ptr(), inertial.data_ptr(), last_action.data_ptr(), eps.data_ptr())
    assert lib.te_policy_act(params.data_ptr(), c, n, *ins, *[t.data_ptr() for t in a], stream) == 0, lib.te_last_error()
    assert lib.te_policy_act_shaped(params.data_ptr(), C.byref(_shape(c, *DEFAULT)), n, *ins, *[t.data_ptr() for t in b], stream) == 0, lib.te_last_error()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.gpu
def test_rows_are_independent_and_calls_deterministic():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    fused = FusedPolicy(_policy(torch, 3, 9, BO))
    n = 4097
    obs = _obs(torch, n, 3, 3)
    eps = torch.randn(n, 4, device="cuda:0")
    full = fused.act(obs, eps)
    again = fused.act(obs, eps)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    for s in (0, 17, 64, 2000, 4033):
        part = fused.act({k: v[s:s + 64].contiguous() for k, v in obs.items()}, eps[s:s + 64].contiguous())
        for x, y in zip(full, part):
            assert torch.equal(x[s:s + 64], y), s


@pytest.mark.gpu
def test_sampling_matches_the_hand_formula():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 7, BO)
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


def _clamp(torch, mu):
    low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device=mu.device)
    return torch.max(torch.min(mu, torch.ones_like(mu)), low)


@pytest.mark.gpu
def test_drive_shaped_matches_the_four_call_sequence_bitwise():
    torch = _gpu()
    from dronechase_amd import config as K
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import FusedPolicy
    n = 128
    cfg = default_config("exp05", n_envs=n, motor_noise=1, seed=17, max_step=14)
    A, B = BatchedEnv(cfg, "cuda:0"), BatchedEnv(cfg, "cuda:0")
    A.reset(); B.reset()
    policy = _policy(torch, 3, 5, BO)
    with torch.no_grad():       # a mean that leaves [-1, 1] in a share of the rows, so the clamp matters
        policy.mu.weight.mul_(8.0)
        policy.mu.bias.copy_(torch.tensor([1.2, -1.2, 0.2, 0.3]))
    fp = FusedPolicy(policy.requires_grad_(False))
    words = lambda env: env.get_state()[: env.N * env.D * K.DRONE_WORDS].view(env.N, env.D, K.DRONE_WORDS)
    ACT = K.D["ALLY_ACTION"]
    mu_a = torch.full((n, 4), float("nan"), device="cuda:0")
    agent = torch.tensor([[0.3, -0.2, 0.1, 0.5]], device="cuda:0").repeat(n, 1)
    clamped = 0
    for step in range(6):
        A.drive_wingman(1, fp, mu=mu_a)
        lidar, inertial, last_action, _active = B.observe_wingman(1)
        mu_b, _ = fp.forward({"lidar": lidar, "inertial_data": inertial, "last_action": last_action})
        B.set_wingman_actions(1, _clamp(torch, mu_b).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(mu_a.view(torch.int32), mu_b.view(torch.int32)), f"mu differs from te_policy_act_shaped's at step {step}"
        after = words(A)
        assert torch.equal(after, words(B)), f"state after the drive differs at step {step}"
        assert torch.equal(after[:, 1, ACT:ACT + 4].view(torch.float32), _clamp(torch, mu_a))      # every ally is alive this early
        clamped += int((_clamp(torch, mu_a) != mu_a).sum())
        A.step(agent, terminal=False); B.step(agent, terminal=False)
    assert 0 < clamped < 6 * n * 4
    A.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False])
def test_ppo_fused_forward(use_graph):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, policy_shape
    env = BatchedEnv(default_config("stage03", n_envs=512, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=16, batch_size=2048, n_epochs=2, use_graph=use_graph, fused_forward=True, features_dim=512,
                             net_arch=(128, 256, 512)), seed=1)
    assert policy_shape(ppo.policy) == (3,) + BO and ppo.fused.net_arch == BO[1]
    before = [q.detach().clone() for q in ppo.policy.parameters()]
    logs = []
    ppo.learn(3 * 16 * 512, log=logs.append)     # the third collect replays the graph on weights two updates moved
    assert len(logs) == 3
    for rec in logs:
        assert all(np.isfinite(v) for v in rec.values() if isinstance(v, float)), rec
    assert any(not torch.equal(a, q.detach()) for a, q in zip(before, ppo.policy.parameters()))
    ppo.collect()          # learn() ended with update(): this rollout must run on the moved weights
    b = ppo.buf
    T, N = b.rewards.shape
    with torch.no_grad():
        d, v = ppo.policy.dist({k: o.reshape(T * N, *o.shape[2:]) for k, o in b.obs.items()})
        logp = d.log_prob(b.actions.reshape(T * N, 4)).sum(-1)
    torch.testing.assert_close(b.values.reshape(-1), v, atol=ATOL, rtol=RTOL)
    torch.testing.assert_close(b.logp.reshape(-1), logp, atol=ATOL, rtol=RTOL)
    env.close()


@pytest.mark.gpu
def test_ppo_on_exp05_flies_a_snapshot_of_the_learn_shape():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, pack_policy
    env = BatchedEnv(default_config("exp05", n_envs=128, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=8, batch_size=512, n_epochs=2, wingman_driver="snapshot", features_dim=LEARN[0], net_arch=LEARN[1]), seed=4)
    assert (ppo.wingman.features_dim, ppo.wingman.net_arch) == LEARN and ppo.wingman.policy is not ppo.policy
    ptr = ppo.wingman.params.data_ptr()
    for _ in range(2):
        log = ppo.collect()
        log.update(ppo.update())
        assert all(np.isfinite(v) for v in log.values() if isinstance(v, float)), log
    assert bool(torch.isfinite(ppo._wingman_mu[1]).all()) and bool((ppo._wingman_mu[1] != 0).any())     # the ally was driven
    ppo.sync_wingmen()
    torch.cuda.synchronize()
    assert ppo.wingman.params.data_ptr() == ptr
    assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
    env.close()


@pytest.mark.gpu
def test_fused_update_refuses_other_shapes_before_any_launch():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=64), "cuda:0")
    with pytest.raises(ValueError, match="gradient kernel.*default shape only"):
        PPO(env, PPOConfig(n_steps=2, fused_update=True, net_arch=(128, 256, 512), features_dim=512))
    env.close()
