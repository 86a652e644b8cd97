"""te_policy_act_bf16 (dronechase_amd/csrc/te_policy_bf16.hpp): the fused policy inference with bf16 operands on the bf16 MFMA, for the
three served shapes x lidar_channels 2 and 3, and the layers above it (te_policy_bf16_words, te_policy_pack_bf16,
FusedPolicy(precision="bf16"), PolicyDriver(precision="bf16"), PPOConfig.fused_forward_bf16).

The reference is reference() below, on the CPU: the numerics contract of include/threatengage.h applied to the PyTorch module.  The
weights of every layer below mu and value and the input of EVERY layer go through .float().bfloat16(); the sum, the bias and the
activation are in a chosen dtype, and the result is cast to fp32 between layers.  E64 accumulates in fp64, E32 in fp32.  Their gap is
what separates any two correct implementations (summation order, plus the rare activation that lands on the other side of a bf16
rounding boundary), so the bounds of the kernel come from it and never from the kernel:
  * per row, mu and value within 1e-5 of E64 except on at most 10 % of the rows: 3 x the pair's own worst share (at most 10 % / 3 of
    the rows differ between E64 and E32 by more than 1e-5, asserted without a GPU below), because the kernel's order differs from both;
  * every row within 4 x G, G = max |E64 - E32| on the same inputs (4: a maximum over rare rounding flips is heavy-tailed).
The inputs: default-initialised policies, torch.manual_seed(5) before building the six (shape, C) policies in turn; 2 048 uniform rows
(lidar in [0, 1), inertial_data and last_action in [-1, 1)).

PPO (test_ppo_collects_with_the_bf16_forward): buf.values, buf.logp AND buf.actions are bitwise what FusedPolicy(precision="bf16").act
gives on the stored observations with the rollout's own eps.  eps is not recovered from the action and the mean ((a - mu) / sigma
is eps only to rounding, and logp is a function of eps alone, so a recovered eps cannot give logp bit for bit): the device generator's
state from before collect() is restored and the draws are repeated.

Measured on the MI355X (profiles/policy_bf16.json): over the six instances G was 1.0e-4 to 2.4e-4, the kernel's largest gap to E64 1.1e-4 to
1.7e-4 (at most 1.6 x G), its share of rows beyond 1e-5 0.8 % to 3.7 %, and its largest gap to the fp32 module 2.3e-4 to 3.3e-4.

TE_POLICY_BF16_RECORD=<path>: every parity case appends one JSON line with its figures (G, the kernel's largest gap and share, its
largest gap to the fp32 module)."""
import copy
import ctypes as C
import functools
import json
import os

import pytest

from tests._policy_cases import StubEnv, _gpu, _shape

DEFAULT = (256, (64, 64))
BO = (512, (128, 256, 512))
LEARN = (512, (512, 128, 256))
SHAPES = {"default": DEFAULT, "bo": BO, "learn": LEARN}
TILE_ROWS = {DEFAULT: 32, BO: 48, LEARN: 48}      # rows per workgroup (te_policy_bf16.hpp pol_lds_plan_bf16)
INSTANCES = [(name, c) for name in SHAPES for c in (2, 3)]
ROWS = 2048
NEAR = 1e-5             # "the same" for one output
SHARE = 0.10            # of the rows may be further than NEAR from E64
G_FACTOR = 4.0


def _kp(k):
    return (k + 31) // 32 * 32


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _q(x):
    return x.float().bfloat16()         # round-to-nearest-even


def reference(policy, obs, dtype):
    """(mu [n, 4], value [n]) of the numerics contract on the CPU, accumulating in `dtype`."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    def seq(mods, x):
        for m in mods:
            if isinstance(m, nn.Conv2d):
                x = F.conv2d(_q(x).to(dtype), _q(m.weight).to(dtype), m.bias.to(dtype), stride=m.stride)
            elif isinstance(m, nn.Linear):
                x = F.linear(_q(x).to(dtype), _q(m.weight).to(dtype), m.bias.to(dtype))
            elif isinstance(m, nn.ReLU):
                x = torch.relu(x).float()
            elif isinstance(m, nn.Tanh):
                x = torch.tanh(x).float()
            else:
                assert isinstance(m, nn.Flatten), m
                x = x.flatten(1)
        return x

    def last(layer, x):                 # mu and value: fp32 weights over the bf16 last hidden tile
        return F.linear(_q(x).to(dtype), layer.weight.to(dtype), layer.bias.to(dtype)).float()

    with torch.no_grad():
        z = torch.cat((seq(policy.lidar, obs["lidar"]), seq(policy.inertial, obs["inertial_data"]), seq(policy.action, obs["last_action"])), dim=1)
        f = seq(policy.final, z)
        return last(policy.mu, seq(policy.pi, f)), last(policy.value, seq(policy.vf, f)).squeeze(-1)


def _row_gap(a, b):
    """Per row, the largest |difference| over mu's four components and the value."""
    import torch
    return torch.maximum((a[0] - b[0]).abs().max(dim=1).values, (a[1] - b[1]).abs())


def _references(policy, obs):
    import torch
    e64, e32 = reference(policy, obs, torch.float64), reference(policy, obs, torch.float32)
    with torch.no_grad():
        mod = policy(obs)
    gap = _row_gap(e64, e32)
    return {"e64": e64, "e32": e32, "module": mod, "G": float(gap.max()), "pair_share": float((gap > NEAR).float().mean())}


@functools.lru_cache(maxsize=None)
def _cases():
    """The six policies, their inputs and their references, computed once on the CPU and never changed."""
    import torch
    from dronechase_amd.ppo import LidarInertialActionPolicy
    g = torch.Generator().manual_seed(11)
    u = lambda *s: torch.rand(*s, generator=g)
    obs = {c: {"lidar": u(ROWS, c, 13, 26), "inertial_data": u(ROWS, 15) * 2 - 1, "last_action": u(ROWS, 4) * 2 - 1} for c in (2, 3)}
    torch.manual_seed(5)
    out = {}
    for name, c in INSTANCES:
        f, arch = SHAPES[name]
        policy = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=f, net_arch=arch)
        with torch.no_grad():
            policy.log_std.copy_(torch.tensor([0.2, -0.3, 0.1, -0.5]))
        out[name, c] = dict(policy=policy, obs=obs[c], **_references(policy, obs[c]))
    return out


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_bf16_words(lib):
    for name, c in INSTANCES:
        f, arch = SHAPES[name]
        widths = (f,) + arch
        by_hand = 32 * _kp(16 * c) + 64 * _kp(128) + (128 * _kp(15) + 2 * 128 * _kp(128)) + (128 * _kp(4) + 2 * 128 * _kp(128)) + f * _kp(448) + \
            2 * sum(b * _kp(a) for a, b in zip(widths, widths[1:]))
        out = C.c_size_t()
        assert lib.te_policy_bf16_words(C.byref(_shape(c, f, arch)), C.byref(out)) == 0, lib.te_last_error()
        assert out.value == by_hand, (name, c)
    assert lib.te_policy_bf16_words(C.byref(_shape(3, *DEFAULT)), None) != 0 and b"null" in lib.te_last_error()


def test_calls_reject_bad_arguments(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    bo = _shape(3, *BO)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(params=fake, weights=fake, shape=C.byref(bo), n=8, lidar=fake, inertial=fake, last_action=fake,
                                                       eps=None, mu=fake, value=fake, action=None, logp=None, action_env=None, stream=None).items()]
    unserved = [(_shape(3, 300, (64, 64)), b"features_dim"), (_shape(3, 512, (128, 256)), b"hidden"), (_shape(4, *BO), b"lidar_channels"),
                (_shape(3, 256, (64, 64, 64, 64)), b"n_hidden")]
    cases = [(dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"), (dict(shape=None), b"null shape"),
             (dict(params=None), b"null"), (dict(weights=None), b"null"), (dict(params=fake + 4), b"params must be 16-byte"),
             (dict(weights=fake + 2), b"weights_bf16 must be 16-byte"), (dict(weights=fake + 8), b"weights_bf16 must be 16-byte"),
             (dict(lidar=fake + 4), b"lidar must be 8-byte"), (dict(mu=fake + 2), b"4-byte"), (dict(mu=None), b"null"), (dict(eps=fake), b"eps given")]
    cases += [(dict(shape=C.byref(s)), field) for s, field in unserved]
    for kw, msg in cases:
        assert lib.te_policy_act_bf16(*args(**kw)) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_act_bf16"), (kw, err)
    words = C.c_size_t()
    for s, field in unserved:
        for rc in (lib.te_policy_act_bf16(*args(shape=C.byref(s))), lib.te_policy_bf16_words(C.byref(s), C.byref(words)),
                   lib.te_policy_pack_bf16(fake, C.byref(s), fake, None)):
            msg = lib.te_last_error()
            assert rc != 0 and field in msg and b"128, 256, 512" in msg and b"512, 128, 256" in msg and b"64, 64" in msg, msg
    for kw, msg in ((dict(params=None), b"null"), (dict(out=None), b"null"), (dict(params=fake + 4), b"params must be 16-byte"),
                    (dict(out=fake + 2), b"out must be 16-byte"), (dict(shape=None), b"null shape")):
        a = dict(params=fake, shape=C.byref(bo), out=fake, stream=None)
        a.update(kw)
        assert lib.te_policy_pack_bf16(*a.values()) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_pack_bf16"), (kw, err)


def test_switches_need_their_base(lib):
    from dronechase_amd.ppo import FusedPolicy, LidarInertialActionPolicy, PolicyDriver, PPOConfig
    assert PPOConfig().fused_forward_bf16 is False
    assert PPOConfig(fused_forward=True, fused_forward_bf16=True).fused_forward_bf16
    with pytest.raises(ValueError, match="fused_forward_bf16.*needs fused_forward"):
        PPOConfig(fused_forward_bf16=True)
    p = LidarInertialActionPolicy()
    with pytest.raises(ValueError, match="precision"):
        FusedPolicy(p, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        PolicyDriver(p, fused=False, precision="bf16")


def test_ppo_refuses_the_switch_set_after_the_config_check(lib):
    from dronechase_amd.ppo import PPO, PPOConfig
    cfg = PPOConfig(n_steps=2)
    cfg.fused_forward_bf16 = True
    with pytest.raises(ValueError, match="fused_forward_bf16.*needs fused_forward"):
        PPO(StubEnv(), cfg)


def test_the_reference_pair_agrees(lib):
    """The condition the kernel's bounds rest on: E64 and E32 differ by more than 1e-5 on at most 10 % / 3 of the rows."""
    for (name, c), case in _cases().items():
        mod_gap = float(_row_gap(case["e64"], case["module"]).max())
        print(f"\n{name} C={c}: G = max|E64 - E32| = {case['G']:.2e}; rows further than {NEAR:g}: {case['pair_share']:.2%}; max|E64 - fp32 module| = {mod_gap:.2e}")
        assert case["pair_share"] <= SHARE / 3, (name, c, case["pair_share"])
        assert 0.0 < case["G"] < 1e-2 and mod_gap < 1e-2, (name, c)      # the references are neither identical nor broken


# ---------------------------------------------------------------------------------------------------------- MI355X
def _to_gpu(obs):
    return {k: v.to("cuda:0").contiguous() for k, v in obs.items()}


def _fused(policy):
    from dronechase_amd.ppo import FusedPolicy
    return FusedPolicy(copy.deepcopy(policy).to("cuda:0"), precision="bf16")


def _hold_to_the_references(torch, label, got, refs):
    """The parity bounds of the module docstring; prints (and records) every figure before it asserts."""
    got = tuple(t.cpu() for t in got)
    gap = _row_gap(got, refs["e64"])
    share, worst, to_module = float((gap > NEAR).float().mean()), float(gap.max()), float(_row_gap(got, refs["module"]).max())
    rec = {"case": label, "rows": int(gap.numel()), "G": refs["G"], "reference_pair_share": refs["pair_share"], "kernel_max_gap_to_E64": worst,
           "kernel_share_beyond_1e-5": share, "kernel_max_gap_to_fp32_module": to_module}
    print("\n" + json.dumps(rec))
    if os.environ.get("TE_POLICY_BF16_RECORD"):
        with open(os.environ["TE_POLICY_BF16_RECORD"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert share <= SHARE, rec
    assert worst <= G_FACTOR * refs["G"], rec


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", INSTANCES)
def test_parity_with_the_reference(name, c):
    torch = _gpu()
    case = _cases()[name, c]
    fused = _fused(case["policy"])
    got = fused.forward(_to_gpu(case["obs"]))
    torch.cuda.synchronize()
    _hold_to_the_references(torch, f"{name} C={c} uniform", got, case)


@pytest.mark.gpu
def test_parity_on_real_observations():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, FusedPolicy, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=512, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=8, use_graph=False, features_dim=BO[0], net_arch=BO[1]), seed=2)
    ppo.collect(); ppo.collect()        # no update(): the observations are what this test is after, and autograd's first call takes seconds
    obs = {k: v[-1].clone() for k, v in ppo.buf.obs.items()}        # the 512 observations of the rollout's last step
    policy = ppo.policy
    env.close()
    got = FusedPolicy(policy, precision="bf16").forward(obs)
    torch.cuda.synchronize()
    refs = _references(copy.deepcopy(policy).cpu(), {k: v.cpu() for k, v in obs.items()})
    assert refs["pair_share"] <= SHARE / 3, refs["pair_share"]
    _hold_to_the_references(torch, "bo C=3 te_step", got, refs)


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("default", 3), ("bo", 2), ("learn", 3)])
def test_pack_is_the_rounded_weights_at_the_documented_offsets(name, c):
    torch = _gpu()
    import torch.nn as nn
    policy = _cases()[name, c]["policy"]
    fused = _fused(policy)
    torch.cuda.synchronize()
    buf = fused.weights_bf16.cpu()
    assert buf.dtype == torch.int16 and fused.weights_bf16.data_ptr() % 16 == 0
    off = 0
    for seq in (policy.lidar, policy.inertial, policy.action, policy.final, policy.pi, policy.vf):
        for m in seq:
            if not isinstance(m, (nn.Conv2d, nn.Linear)):
                continue
            w = m.weight.detach().reshape(m.weight.shape[0], -1)
            n, k = w.shape
            block = buf[off:off + n * _kp(k)].view(n, _kp(k))
            assert off * 2 % 64 == 0
            assert torch.equal(block[:, :k], w.bfloat16().view(torch.int16)), (name, m)
            assert bool((block[:, k:] == 0).all()), (name, m)
            off += n * _kp(k)
    assert off == buf.numel()


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", INSTANCES)
def test_rows_are_independent_and_calls_deterministic(name, c):
    torch = _gpu()
    case = _cases()[name, c]
    M = TILE_ROWS[SHAPES[name]]
    fused = _fused(case["policy"])
    n = 2 * M + 1
    obs = {k: v[:n].contiguous() for k, v in _to_gpu(case["obs"]).items()}
    eps = torch.randn(n, 4, device="cuda:0")
    full, again = fused.act(obs, eps), fused.act(obs, eps)
    for x, y in zip(full, again):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    for lo, hi in ((0, 1), (0, M - 1), (1, M + 2)):
        part = fused.act({k: v[lo:hi].contiguous() for k, v in obs.items()}, eps[lo:hi].contiguous())
        for x, y in zip(full, part):
            assert torch.equal(x[lo:hi], y), (lo, hi)
    mu, value = fused.forward(obs)
    assert torch.equal(value, full[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", INSTANCES)
def test_rows_past_n_are_not_written(lib, name, c):
    torch = _gpu()
    case = _cases()[name, c]
    M = TILE_ROWS[SHAPES[name]]
    fused = _fused(case["policy"])
    n = M + 1
    obs = {k: v[:n].contiguous() for k, v in _to_gpu(case["obs"]).items()}
    eps = torch.randn(n, 4, device="cuda:0")
    outs = [torch.full(s, float("nan"), device="cuda:0") for s in ((n + M, 4), (n + M,), (n + M, 4), (n + M,), (n + M, 4))]
    rc = lib.te_policy_act_bf16(fused.params.data_ptr(), fused.weights_bf16.data_ptr(), C.byref(fused.shape), n, obs["lidar"].data_ptr(),
                                obs["inertial_data"].data_ptr(), obs["last_action"].data_ptr(), eps.data_ptr(), *[t.data_ptr() for t in outs],
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.te_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all())


@pytest.mark.gpu
def test_sampling_matches_the_hand_formula(lib):
    torch = _gpu()
    case = _cases()["bo", 3]
    fused = _fused(case["policy"])
    obs = _to_gpu(case["obs"])
    eps = torch.randn(ROWS, 4, device="cuda:0") * 2
    a, logp, v, a_env = fused.act(obs, eps)
    mu, v2 = fused.forward(obs)
    assert torch.equal(v, v2)
    log_std = fused.policy.log_std.detach()
    torch.testing.assert_close(a, mu + log_std.exp() * eps, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(logp, (-0.5 * eps * eps - log_std - 0.9189385332046727).sum(-1), atol=1e-5, rtol=1e-6)
    low, high = torch.tensor([-1.0, -1.0, -1.0, 0.0], device="cuda:0"), torch.ones(4, device="cuda:0")
    assert torch.equal(a_env, torch.max(torch.min(a, high), low))
    assert bool((a_env != a).any())      # the draw is wide enough that the clamp does something
    d = torch.distributions.Normal(mu, log_std.exp().expand_as(mu), validate_args=False)      # around the kernel's own mean
    torch.testing.assert_close(logp, d.log_prob(a).sum(-1), atol=1e-4, rtol=1e-4)
    # eps = NULL: mu and value only
    outs = [torch.full(s, float("nan"), device="cuda:0") for s in ((ROWS, 4), (ROWS,), (ROWS, 4), (ROWS,), (ROWS, 4))]
    rc = lib.te_policy_act_bf16(fused.params.data_ptr(), fused.weights_bf16.data_ptr(), C.byref(fused.shape), ROWS, obs["lidar"].data_ptr(),
                                obs["inertial_data"].data_ptr(), obs["last_action"].data_ptr(), None, *[t.data_ptr() for t in outs],
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.te_last_error()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], mu) and torch.equal(outs[1], v)
    for t in outs[2:]:
        assert bool(torch.isnan(t).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [False, True])
def test_refresh_repacks_both_buffers_in_place(bound):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    case = _cases()["learn", 3]
    fused = _fused(case["policy"])
    if bound:
        fused.bind_parameters()
    obs = {k: v[:97].contiguous() for k, v in _to_gpu(case["obs"]).items()}
    ptrs = fused.params.data_ptr(), fused.weights_bf16.data_ptr()
    before = [t.clone() for t in fused.forward(obs)]
    with torch.no_grad():
        for p in fused.policy.parameters():
            p.mul_(1.03125)
    if not bound:       # bound: the fp32 buffer IS the weights (mu and value read it), only the bf16 copy is stale
        for x, y in zip(before, fused.forward(obs)):
            assert torch.equal(x, y)
    fused.refresh()
    assert (fused.params.data_ptr(), fused.weights_bf16.data_ptr()) == ptrs
    after = fused.forward(obs)
    fresh = FusedPolicy(fused.policy, precision="bf16").forward(obs)
    for x, y, z in zip(after, fresh, before):
        assert torch.equal(x, y) and not torch.equal(x, z)


def _replay(torch, ppo, rng_state, warmups):
    """The rollout in ppo.buf again: a fresh bf16 FusedPolicy on the stored observations with the rollout's own draws."""
    from dronechase_amd.ppo import FusedPolicy
    b = ppo.buf
    fresh = FusedPolicy(ppo.policy, precision="bf16")
    now = torch.cuda.get_rng_state("cuda:0")
    torch.cuda.set_rng_state(rng_state, "cuda:0")
    for _ in range(warmups):        # the two warm-up steps before the graph capture draw too
        torch.randn_like(b.actions[0])
    for t in range(b.actions.shape[0]):
        eps = torch.randn_like(b.actions[t])
        a, logp, v, _ = fresh.act({k: o[t] for k, o in b.obs.items()}, eps)
        assert torch.equal(a, b.actions[t]), f"step {t}: the replayed draw is not the rollout's"
        assert torch.equal(v, b.values[t]) and torch.equal(logp, b.logp[t]), t
    torch.cuda.set_rng_state(now, "cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False])
def test_ppo_collects_with_the_bf16_forward(use_graph):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig

    def make(bf16):
        env = BatchedEnv(default_config("stage03", n_envs=256, max_step=40), "cuda:0")
        return env, PPO(env, PPOConfig(n_steps=4, batch_size=512, n_epochs=1, use_graph=use_graph, fused_forward=True, fused_forward_bf16=bf16,
                                       features_dim=BO[0], net_arch=BO[1]), seed=1)

    env, ppo = make(True)
    assert ppo.fused.precision == "bf16" and ppo.fused.weights_bf16 is not None
    state = torch.cuda.get_rng_state("cuda:0")
    ppo.collect()
    _replay(torch, ppo, state, 2 if use_graph else 0)
    first = ppo.buf.values.clone(), ppo.buf.logp.clone(), ppo.buf.actions.clone()
    before = [q.detach().clone() for q in ppo.policy.parameters()]
    ppo.update()
    assert any(not torch.equal(a, q.detach()) for a, q in zip(before, ppo.policy.parameters()))
    state = torch.cuda.get_rng_state("cuda:0")
    ppo.collect()
    _replay(torch, ppo, state, 0)       # the new weights: _replay packs them afresh
    env.close()
    env, off = make(False)
    off.collect()
    assert not torch.equal(off.buf.values, first[0]) and not torch.equal(off.buf.actions, first[2])     # the same seed, another forward: the switch is live
    env.close()


@pytest.mark.gpu
def test_policy_driver_bf16():
    torch = _gpu()
    from dronechase_amd.ppo import PolicyDriver
    case = _cases()["default", 3]
    policy = copy.deepcopy(case["policy"]).to("cuda:0")
    obs = {k: v[:100].contiguous() for k, v in _to_gpu(case["obs"]).items()}
    a32, _ = PolicyDriver(policy, fused=True).predict(obs)
    driver = PolicyDriver(policy, fused=True, precision="bf16")
    a16, _ = driver.predict(obs)
    mu, _ = driver.fused.forward(obs)
    low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device="cuda:0")
    assert torch.equal(a16, torch.max(torch.min(mu, torch.ones_like(mu)), low))
    assert not torch.equal(a16, a32) and float((a16 - a32).abs().max()) < 1e-2
