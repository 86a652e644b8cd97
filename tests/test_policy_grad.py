"""te_policy_ppo_grad (dronechase_amd/csrc/te_policy_grad.hpp): the gradient of PPO's loss for the policy in one ABI call, and the
layers above it (FusedPolicy.ppo_grad, PPOConfig.fused_update).

Tolerance: per packed tensor, |d|_inf <= 1e-4 ||g||_inf + 1e-6 + 0.02 / B against autograd through the PyTorch module in fp32 (the
kernel sums in another order, so it is not bit-exact); the statistics to 1e-4 |s| + 1e-6.  The last term is one row's share of the
gradient at a ReLU kink: a pre-activation within rounding of 0 takes the other side in the other summation order, and its row's
dL/dY then enters the bias sum or not.  Measured on the MI355X (trained weights, te_step rows, B = 4 096): a pre-activation of 3.0e-9
moved inertial.4.bias by 1.78e-6 = its row's dL/dY exactly, while fp32 autograd was within 1.3e-10 of fp64 there.  The measured gaps
are printed (pytest -s).  The kink term is far above most tensors' norms at small B: tests/test_policy_kinkfree.py holds the same kernel to
fp64 per element on inputs that have no kink."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from tests._policy_cases import _compare, _gpu, _kernel, _obs, _policy, _ref, _rollout, _trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, ABS, KINK = 1e-4, 1e-6, 0.02


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _ws_bytes(lib, c, n):
    out = C.c_size_t()
    assert lib.te_policy_grad_workspace_bytes(c, n, C.byref(out)) == 0, lib.te_last_error()
    return out.value


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "threatengage.h")).read(), flags=re.S)
    for name in ("te_policy_grad_workspace_bytes", "te_policy_ppo_grad"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None


def test_workspace_bytes_monotone(lib):
    for c in (2, 3):
        sizes = [_ws_bytes(lib, c, n) for n in (1, 2, 31, 32, 33, 64, 1000, 4097, 65536, 1 << 20)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] > sizes[0] > 0
        assert 15_000 * 65536 < _ws_bytes(lib, c, 65536) < 25_000 * 65536     # ~17.5 KB per row
    assert _ws_bytes(lib, 2, 4096) < _ws_bytes(lib, 3, 4096)
    out = C.c_size_t()
    for c, n, msg in ((4, 8, b"lidar_channels"), (1, 8, b"lidar_channels"), (3, 0, b"n must be positive"), (3, -5, b"n must be positive"),
                      (3, (1 << 27) + 1, b"at most")):
        assert lib.te_policy_grad_workspace_bytes(c, n, C.byref(out)) != 0 and msg in lib.te_last_error(), (c, n)
    assert lib.te_policy_grad_workspace_bytes(3, 8, None) != 0 and b"null" in lib.te_last_error()


# te_policy_grad_workspace_bytes of commit 66a9492 (its library built and called on the host: the function touches no device); the
# order and the sizes of the workspace's buffers are part of what a caller's allocation relies on
WS_ROWS = (1, 32, 33, 161, 2048, 2049, 65536)
WS_BYTES = {2: (1467904, 1467904, 1996032, 4113664, 34868224, 36335104, 1115752192),
            3: (1494528, 1494528, 2047232, 4265216, 36465664, 37959168, 1166870272)}


def test_workspace_bytes_are_the_recorded_ones(lib):
    for c in (2, 3):
        assert tuple(_ws_bytes(lib, c, n) for n in WS_ROWS) == WS_BYTES[c]


def test_bad_arguments_fail_through_last_error(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    need = _ws_bytes(lib, 3, 8)
    base = dict(params=fake, ch=3, n=8, index=None, lidar=fake, inertial=fake, last_action=fake, action=fake, old_logp=fake, adv=fake,
                ret=fake, ms=None, clip=0.2, vf=0.5, ent=0.0, grad=fake, stats=fake, ws=fake, ws_bytes=need, stream=None)
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]
    cases = [(dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"), (dict(ch=1), b"lidar_channels"),
             (dict(ch=4), b"lidar_channels"), (dict(params=None), b"null"), (dict(lidar=None), b"null"), (dict(action=None), b"null"),
             (dict(ret=None), b"null"), (dict(grad=None), b"null"), (dict(stats=None), b"null"), (dict(ws=None), b"null"),
             (dict(params=fake + 4), b"params must be 16-byte"), (dict(grad=fake + 8), b"grad must be 16-byte"),
             (dict(lidar=fake + 4), b"lidar must be 8-byte"), (dict(adv=fake + 2), b"4-byte"), (dict(index=fake + 4), b"index must be 8-byte"),
             (dict(ws_bytes=need - 1), b"workspace too small"), (dict(ws_bytes=0), b"workspace too small"),
             (dict(n=4096), b"workspace too small"), (dict(clip=-0.1), b"clip_range")]
    for kw, msg in cases:
        assert lib.te_policy_ppo_grad(*args(**kw)) != 0, kw
        assert msg in lib.te_last_error(), (kw, lib.te_last_error())


# ---------------------------------------------------------------------------------------------------------- MI355X
GAP = {"grad": 0.0, "stats": 0.0}      # largest |d| / bound seen


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 2])
def test_gradient_parity_with_autograd(c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    trained, real = _trained_policy(torch, c, n_envs=512, batch_size=1024)      # 8 x 512 = 4 096 real te_step observations
    real_ro = _rollout(torch, trained, real, 99)
    for label, policy in (("random", _policy(torch, c, 5)), ("trained", trained)):
        fused = FusedPolicy(policy)
        cases = []      # (source, obs, rollout, index, normalise, ent_coef)
        for n, norm, ent in ((1, False, 0.0), (33, True, 0.01), (4097, True, 0.0), (65536, True, 0.01)):
            obs = _obs(torch, n, c, n)
            cases.append((f"random B={n}", obs, _rollout(torch, policy, obs, n), None, norm, ent))
        obs = _obs(torch, 10000, c, 7)
        idx = torch.randperm(10000, device="cuda:0")[:4097]
        cases.append(("random rows, index B=4097", obs, _rollout(torch, policy, obs, 7), idx, True, 0.02))
        ro = real_ro if policy is trained else _rollout(torch, policy, real, 98)
        cases.append(("te_step B=4096", real, ro, None, True, 0.0))
        cases.append(("te_step, index B=1000", real, ro, torch.randperm(4096, device="cuda:0")[:1000], True, 0.01))
        for src, obs, ro, idx, norm, ent in cases:
            ref, ref_stats, ms = _ref(torch, policy, obs, ro, idx, norm, 0.2, 0.5, ent)
            grad, stats = _kernel(torch, fused, obs, ro, idx, ms, 0.2, 0.5, ent)
            tag = f"C={c} {label} weights, {src}"
            ref64 = lambda: _ref(torch, policy, obs, ro, idx, norm, 0.2, 0.5, ent, dtype=torch.float64)[0]
            _compare(torch, policy, grad, ref, stats, ref_stats, tag, obs["lidar"].shape[0] if idx is None else idx.numel(), ref64,
                     tol=(REL, ABS, KINK), gap=GAP)
            if obs["lidar"].shape[0] > 1000 and idx is None:      # both clip branches were taken
                assert 0.1 < float(stats[3]) < 0.9, (tag, stats.tolist())
    print(f"\nlidar_channels={c}: largest |d| as a fraction of the bound so far: gradient {GAP['grad']:.3f}, statistics {GAP['stats']:.3f}")


# SHA-256 of (grad, stats) of the call below, recorded from the library of commit 66a9492 on the MI355X: every sum of the three
# kernels has a fixed order, so a refactor of the policy's description leaves these as they are
GRAD_DIGEST = {2: ("cb716a9248cff5e8911b3db8fb4e2ac8a2a220668657dfb73c923b24141e1248", "f36b37cf0a0e37c99eccf9f8a1a3e1900b2079949ef92b5636e22646021b6eee"),
               3: ("306c66bf3ebd710d914de046a77425eb19b9541cc3f8d6ec5357455dfd0839f0", "97e51954084fa257cfb3d0f54cf3f7af4e5d22387da3ffc5cb20940e456b6ca6")}


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
def test_ppo_grad_is_bitwise_the_recorded_one(lib, c):
    """2 049 rows picked by a permuted index out of 2 100: Bp = 2 080, so every layer's reduction crosses a kGradSlice = 2 048 boundary
    (conv1 has 13 slices) and the last tile has one live row.  Every input comes from numpy's PCG64, through the raw ABI."""
    torch = _gpu()
    n, m = 2049, 2100
    rng = np.random.default_rng(2000 + c)
    u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32)).to("cuda:0")
    words = C.c_size_t()
    assert lib.te_policy_param_words(c, C.byref(words)) == 0
    params = u(-0.1, 0.1, words.value)
    lidar, inertial, last_action = u(0, 1, m, c, 13, 26), u(-1, 1, m, 15), u(-1, 1, m, 4)
    action, old_logp, adv, ret = u(-1, 1, m, 4), u(-5, -3.5, m), u(-2, 2, m), u(-1, 1, m)
    index = torch.from_numpy(rng.permutation(m)[:n].astype(np.int64)).to("cuda:0")
    ms = torch.tensor([0.1, 1.3], device="cuda:0")
    grad = torch.full((words.value,), float("nan"), device="cuda:0")
    stats = torch.full((4,), float("nan"), device="cuda:0")
    ws = torch.empty(_ws_bytes(lib, c, n), dtype=torch.uint8, device="cuda:0")
    rc = lib.te_policy_ppo_grad(params.data_ptr(), c, n, index.data_ptr(), lidar.data_ptr(), inertial.data_ptr(), last_action.data_ptr(),
                                action.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), ms.data_ptr(), 0.2, 0.5, 0.01,
                                grad.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.te_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all())
    assert 0.0 < float(stats[3]) < 1.0        # both sides of the clip were taken
    digests = tuple(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (grad, stats))
    print(f"\nte_policy_ppo_grad C={c}: {digests}")
    assert digests == GRAD_DIGEST[c]


@pytest.mark.gpu
def test_index_gather_equals_pre_gathered_rows_bitwise():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 21)
    fused = FusedPolicy(p)
    obs = _obs(torch, 5000, 3, 21)
    ro = _rollout(torch, p, obs, 21)
    idx = torch.randint(0, 5000, (3001,), device="cuda:0")          # duplicates allowed
    ms = torch.tensor([0.3, 1.7], device="cuda:0")
    g1, s1 = _kernel(torch, fused, obs, ro, idx, ms, 0.2, 0.5, 0.01)
    g2, s2 = _kernel(torch, fused, {k: v[idx].contiguous() for k, v in obs.items()}, {k: v[idx].contiguous() for k, v in ro.items()},
                     None, ms, 0.2, 0.5, 0.01)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)


@pytest.mark.gpu
def test_repeated_calls_are_bitwise_equal():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 23)
    fused = FusedPolicy(p)
    obs = _obs(torch, 20000, 3, 23)
    ro = _rollout(torch, p, obs, 23)
    ms = torch.tensor([0.3, 1.7], device="cuda:0")
    g1, s1 = _kernel(torch, fused, obs, ro, None, ms, 0.2, 0.5, 0.01)
    _kernel(torch, fused, _obs(torch, 70000, 3, 1), _rollout(torch, p, _obs(torch, 70000, 3, 1), 1), None, ms, 0.2, 0.5, 0.0)  # grows the workspace
    g2, s2 = _kernel(torch, fused, obs, ro, None, ms, 0.2, 0.5, 0.01)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 2])
def test_unused_lidar_cells_change_nothing(c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy, policy_param_words
    p = _policy(torch, c, 25)
    fused = FusedPolicy(p)
    obs = _obs(torch, 300, c, 25)
    ro = _rollout(torch, p, obs, 25)
    ref, ref_s = _kernel(torch, fused, obs, ro, None, None, 0.2, 0.5, 0.0)
    poked = {k: v.clone() for k, v in obs.items()}
    poked["lidar"][:, :, 8:, :] = 1e6
    poked["lidar"][:, :, :, 24:] = -1e6
    g, s = _kernel(torch, fused, poked, ro, None, None, 0.2, 0.5, 0.0)
    assert torch.equal(ref, g) and torch.equal(ref_s, s)
    poked["lidar"][:, :, 7, 23] += 1.0     # ... and a used cell does
    assert not torch.equal(ref, _kernel(torch, fused, poked, ro, None, None, 0.2, 0.5, 0.0)[0])
    assert ref.numel() == policy_param_words(c)


@pytest.mark.gpu
def test_graph_replay_sees_refreshed_weights():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 27)
    fused = FusedPolicy(p)
    obs = _obs(torch, 3000, 3, 27)
    ro = _rollout(torch, p, obs, 27)
    idx = torch.randperm(3000, device="cuda:0")[:2048]
    ms = torch.tensor([0.3, 1.7], device="cuda:0")
    grad = torch.zeros_like(fused.params)
    stats = torch.zeros(4, device="cuda:0")
    call = lambda: fused.ppo_grad(obs, idx, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, 0.2, 0.5, 0.01, grad, stats)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                               # sizes the workspace outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay(); torch.cuda.synchronize()
    first = grad.clone()
    with torch.no_grad():
        for q in p.parameters():
            q.add_(0.01 * torch.randn_like(q))
    fused.refresh()
    g.replay(); torch.cuda.synchronize()
    eager, eager_s = _kernel(torch, fused, obs, ro, idx, ms, 0.2, 0.5, 0.01)
    assert torch.equal(grad, eager) and torch.equal(stats, eager_s)
    assert not torch.equal(first, grad)


def _ppo_pair(torch, fast, n_envs=1024):
    """Two PPOs on the same seed and rollout: autograd fp32 (with fused Adam when fast) and fused_update."""
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    cfg = dict(n_steps=8, batch_size=2048, n_epochs=2, use_graph=False)
    env_a = BatchedEnv(default_config("stage03", n_envs=n_envs, max_step=40), "cuda:0")
    env_b = BatchedEnv(default_config("stage03", n_envs=n_envs, max_step=40), "cuda:0")
    ref = PPO(env_a, PPOConfig(**cfg), seed=4)
    if fast:    # the fused path keeps fp32 gradients: compare against fp32 autograd with the same fused Adam
        ref.opt = torch.optim.Adam(ref.policy.parameters(), lr=ref.cfg.learning_rate, eps=1e-5, fused=True)
    new = PPO(env_b, PPOConfig(**cfg, fast_learner=fast, fused_update=True), seed=4)
    for a, b in zip(ref.policy.parameters(), new.policy.parameters()):
        assert torch.equal(a, b)
    ref.collect()
    for k in ref.buf.obs:
        new.buf.obs[k].copy_(ref.buf.obs[k])
    for name in ("actions", "logp", "values", "rewards", "dones", "adv", "ret"):
        getattr(new.buf, name).copy_(getattr(ref.buf, name))
    return ref, new, (env_a, env_b)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
def test_ppo_update_matches_autograd(fast):
    torch = _gpu()
    ref, new, envs = _ppo_pair(torch, fast)
    before = [q.detach().clone() for q in ref.policy.parameters()]
    torch.manual_seed(8); u_ref = ref.update()
    torch.manual_seed(8); u_new = new.update()
    moved = max(float((a - q.detach()).abs().max()) for a, q in zip(before, ref.policy.parameters()))
    gap = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(ref.policy.parameters(), new.policy.parameters()))
    print(f"\nfast_learner={fast}: parameters moved up to {moved:.3e}; fused_update vs autograd: largest |d| {gap:.3e}")
    assert moved > 1e-4
    # Adam's first steps move a weight by ~lr whatever the size of its gradient, so a near-zero entry of another summation order
    # can move differently: measured 1.6e-5 against moves of 1.8e-3
    assert gap <= 5e-5, gap
    for k in u_ref:
        assert abs(u_ref[k] - u_new[k]) <= REL * abs(u_ref[k]) + 1e-5, (k, u_ref[k], u_new[k])
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_learn_with_fused_forward_and_update():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=16384, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=4, batch_size=16384, n_epochs=2, fused_forward=True, fused_update=True), seed=6)
    before = [q.detach().clone() for q in ppo.policy.parameters()]
    logs = []
    ppo.learn(2 * 4 * 16384, log=logs.append)
    assert len(logs) == 2
    for rec in logs:
        assert all(np.isfinite(v) for v in rec.values() if isinstance(v, float)), rec
    assert all(not torch.equal(a, q.detach()) for a, q in zip(before, ppo.policy.parameters()))
    env.close()
