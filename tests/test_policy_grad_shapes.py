"""te_policy_ppo_grad_shaped / te_policy_grad_workspace_bytes_shaped (dronechase_amd/csrc/te_policy_grad.hpp): the fused PPO gradient for
every served network shape, the default (features_dim 256, heads 64, 64) and the two the reference trains, features_dim 512 with
heads (128, 256, 512) ("reference BO") and (512, 128, 256) ("reference learn"); and the layers above them (FusedPolicy.ppo_grad,
PPOConfig.fused_update_wide).

Tolerance: the bounds of tests/test_policy_grad.py, against autograd through the PyTorch module in fp32: per packed tensor
|d|_inf <= 1e-4 ||g||_inf + 1e-6 + 0.02 / B (the last term is one row's share of the gradient at a ReLU kink), the statistics to
1e-4 |s| + 1e-6.  The wide shapes run 16 rows per workgroup while the workspace is padded to 32: rows 1, 16, 17, 33 leave a whole
padding tile (n mod 32 in [1, 16]) or a partly filled one, and 2 081 rows pad to 2 112, two split-K slices for the one-position layers
(the second of 64 rows) and 13 for conv1.  The measured gaps are printed (pytest -s).  At these small B the kink term exceeds most
tensors' norms: tests/test_policy_kinkfree.py holds the same shapes and row counts to fp64 per element on inputs that have no kink."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests._policy_cases import DEFAULT, StubEnv, _compare, _gpu, _kernel, _obs, _policy, _ref, _rollout, _shape, _trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, ABS, KINK = 1e-4, 1e-6, 0.02

BO = (512, (128, 256, 512))
LEARN = (512, (512, 128, 256))
WIDE = {"reference BO": BO, "reference learn": LEARN}
GRAD_NAMES = ("te_policy_grad_workspace_bytes_shaped", "te_policy_ppo_grad_shaped")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _ws_bytes(lib, c, shape, n):
    out = C.c_size_t()
    assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(_shape(c, *shape)), n, C.byref(out)) == 0, lib.te_last_error()
    return out.value


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "threatengage.h")).read(), flags=re.S)
    for name in GRAD_NAMES:
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None, name


def test_workspace_bytes_default_shape_is_the_unshaped_size(lib):
    out = C.c_size_t()
    for c in (2, 3):
        for n in (1, 32, 33, 4097, 65536):
            assert lib.te_policy_grad_workspace_bytes(c, n, C.byref(out)) == 0, lib.te_last_error()
            assert _ws_bytes(lib, c, DEFAULT, n) == out.value, (c, n)


def _row_arrays(c, f, arch):
    """Floats per sample of every array the workspace holds per row, spelled out by hand: each weight layer's input X, then every
    layer's pre-activation gradient dZ (mu 4, value 1, and the two pseudo-layers log_std 4 and statistics 4)."""
    h0, h1, h2 = arch
    x = [12 * 16 * c, 3 * 128, 15, 128, 128, 4, 128, 128, 448, f, h0, h1, h2, h0, h1, h2]
    dz = [12 * 32, 3 * 64, 128, 128, 128, 128, 128, 128, f, h0, h1, h2, h0, h1, h2, 4, 1, 4, 4]
    return x + dz


def test_workspace_bytes_wide_shapes(lib):
    r256 = lambda b: (b + 255) // 256 * 256
    for c in (2, 3):
        for f, arch in WIDE.values():
            sizes = [_ws_bytes(lib, c, (f, arch), n) for n in (1, 2, 16, 17, 31, 32, 33, 64, 1000, 2081, 4097, 65536, 1 << 20)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
            small = {_ws_bytes(lib, c, (f, arch), n) for n in range(1, 33)}
            assert len(small) == 1 and _ws_bytes(lib, c, (f, arch), 33) > small.pop()          # padded to 32 rows, not to the 16-row tile
            arrays = _row_arrays(c, f, arch)
            assert sum(arrays) == 7904 - 192 * (3 - c)                                         # 31 616 B per row at 3 channels
            by_hand = sum(r256(64 * w * 4) - r256(32 * w * 4) for w in arrays)                 # the split-K partials do not grow below 2 048 rows
            assert _ws_bytes(lib, c, (f, arch), 64) - _ws_bytes(lib, c, (f, arch), 32) == by_hand, (c, f, arch)
            assert 0 <= 32 * 4 * sum(arrays) - by_hand < 256 * len(arrays)
            assert _ws_bytes(lib, c, (f, arch), 4096) > _ws_bytes(lib, c, DEFAULT, 4096)
    assert _ws_bytes(lib, 3, BO, 64) - _ws_bytes(lib, 3, BO, 32) == 32 * 31616 - 256      # inertial.0's input [15] and value's dZ [1] round up at 32 rows only


def test_bad_arguments_fail_through_last_error(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    out = C.c_size_t()
    unserved = [(_shape(3, 300, (64, 64)), b"features_dim"), (_shape(3, 512, (128, 256)), b"hidden"), (_shape(3, 512, (128, 256, 100)), b"hidden"),
                (_shape(4, *BO), b"lidar_channels"), (_shape(3, 256, (64, 64), n_hidden=0), b"n_hidden")]
    for shape, field in unserved:
        assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(shape), 8, C.byref(out)) != 0
        err = lib.te_last_error()
        assert err.startswith(b"te_policy_grad_workspace_bytes_shaped") and field in err and b"128, 256, 512" in err and b"64, 64" in err, err
    bo = _shape(3, *BO)
    for n, msg in ((0, b"n must be positive"), (-5, b"n must be positive"), ((1 << 27) + 1, b"at most")):
        assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(bo), n, C.byref(out)) != 0
        assert msg in lib.te_last_error() and lib.te_last_error().startswith(b"te_policy_grad_workspace_bytes_shaped")
    assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(bo), 8, None) != 0 and b"null" in lib.te_last_error()
    assert lib.te_policy_grad_workspace_bytes_shaped(None, 8, C.byref(out)) != 0 and b"null shape" in lib.te_last_error()

    need = _ws_bytes(lib, 3, BO, 8)
    base = dict(params=fake, shape=C.byref(bo), n=8, index=None, lidar=fake, inertial=fake, last_action=fake, action=fake, old_logp=fake,
                adv=fake, ret=fake, ms=None, clip=0.2, vf=0.5, ent=0.0, grad=fake, stats=fake, ws=fake, ws_bytes=need, stream=None)
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]
    cases = [(dict(shape=C.byref(s)), field) for s, field in unserved] + [
        (dict(shape=None), b"null shape"), (dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"),
        (dict(n=(1 << 27) + 1), b"at most"), (dict(params=None), b"null"), (dict(lidar=None), b"null"), (dict(action=None), b"null"),
        (dict(ret=None), b"null"), (dict(grad=None), b"null"), (dict(stats=None), b"null"), (dict(ws=None), b"null"),
        (dict(params=fake + 4), b"params must be 16-byte"), (dict(grad=fake + 8), b"grad must be 16-byte"),
        (dict(lidar=fake + 4), b"lidar must be 8-byte"), (dict(adv=fake + 2), b"4-byte"), (dict(index=fake + 4), b"index must be 8-byte"),
        (dict(ws=fake + 128), b"workspace must be 256-byte"), (dict(ws_bytes=need - 1), b"workspace too small"),
        (dict(ws_bytes=0), b"workspace too small"), (dict(n=4096), b"workspace too small"),
        (dict(ws_bytes=_ws_bytes(lib, 3, DEFAULT, 8)), b"te_policy_grad_workspace_bytes_shaped says"),      # the default's size does not do
        (dict(clip=-0.1), b"clip_range"), (dict(clip=float("nan")), b"clip_range")]
    for kw, msg in cases:
        assert lib.te_policy_ppo_grad_shaped(*args(**kw)) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_ppo_grad_shaped"), (kw, err)


def test_config_switch(lib):
    from dronechase_amd.ppo import PPO, LidarInertialActionPolicy, PPOConfig
    assert PPOConfig().fused_update_wide is False
    with pytest.raises(ValueError, match="fused_update_wide.*needs fused_update"):
        PPOConfig(fused_update_wide=True)
    cfg = PPOConfig(n_steps=2, fused_update=True, fused_update_wide=True)
    cfg.fused_update = False                                  # set after PPOConfig's own check
    with pytest.raises(ValueError, match="fused_update_wide.*needs fused_update"):
        PPO(StubEnv(), cfg)
    # past the shape refusal: the next check that fails on a CPU env is the device's
    for extra in (dict(), dict(fused_optimizer=True)):
        with pytest.raises(ValueError, match="needs a GPU device"):
            PPO(StubEnv(), PPOConfig(n_steps=2, fused_update=True, fused_update_wide=True, features_dim=512, net_arch=(128, 256, 512), **extra))
    with pytest.raises(ValueError, match="needs a GPU device"):     # with the default shape the switch changes nothing
        PPO(StubEnv(), PPOConfig(n_steps=2, fused_update=True, fused_update_wide=True))
    with pytest.raises(ValueError, match="gradient kernel.*default shape only.*fused_update_wide"):     # without it the refusal names it
        PPO(StubEnv(), PPOConfig(n_steps=2, fused_update=True, features_dim=512, net_arch=(128, 256, 512)))
    with pytest.raises(ValueError, match="128, 256, 512"):          # a shape no kernel serves: the list of served ones
        PPO(StubEnv(), PPOConfig(n_steps=2, fused_update=True, fused_update_wide=True),
            policy=LidarInertialActionPolicy(features_dim=512, net_arch=(128, 256)))


# ---------------------------------------------------------------------------------------------------------- MI355X
GAP = {"grad": 0.0, "stats": 0.0}      # largest |d| / bound seen


@pytest.mark.gpu
@pytest.mark.parametrize("c", [3, 2])
@pytest.mark.parametrize("name", list(WIDE))
def test_gradient_parity_with_autograd(name, c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    shape = WIDE[name]
    random = _policy(torch, c, 5, shape)
    cases = []      # (weights, source, obs, rollout, index, normalise, ent_coef)
    for n, norm, ent in ((1, False, 0.0), (16, True, 0.01), (17, False, 0.01), (33, True, 0.0), (2081, True, 0.01)):
        obs = _obs(torch, n, c, n)
        cases.append((random, f"random B={n}", obs, _rollout(torch, random, obs, n), None, norm, ent))
    obs = _obs(torch, 3000, c, 7)
    cases.append((random, "random rows, index B=1000", obs, _rollout(torch, random, obs, 7), torch.randperm(3000, device="cuda:0")[:1000], True, 0.01))
    trained, real = _trained_policy(torch, c, n_envs=64, batch_size=256, shape=shape)
    cases.append((trained, "trained weights, te_step B=512", real, _rollout(torch, trained, real, 99), None, True, 0.0))
    fused = {id(random): FusedPolicy(random), id(trained): FusedPolicy(trained)}
    for policy, src, obs, ro, idx, norm, ent in cases:
        ref, ref_stats, ms = _ref(torch, policy, obs, ro, idx, norm, 0.2, 0.5, ent)
        grad, stats = _kernel(torch, fused[id(policy)], obs, ro, idx, ms, 0.2, 0.5, ent)
        tag = f"{name} C={c}, {src}"
        ref64 = lambda: _ref(torch, policy, obs, ro, idx, norm, 0.2, 0.5, ent, dtype=torch.float64)[0]
        _compare(torch, policy, grad, ref, stats, ref_stats, tag, obs["lidar"].shape[0] if idx is None else idx.numel(), ref64,
                 tol=(REL, ABS, KINK), gap=GAP)
        if obs["lidar"].shape[0] == 2081:      # both clip branches were taken
            assert 0.1 < float(stats[3]) < 0.9, (tag, stats.tolist())
    print(f"\n{name} C={c}: largest |d| as a fraction of the bound so far: gradient {GAP['grad']:.3f}, statistics {GAP['stats']:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [DEFAULT, BO, LEARN], ids=["default", "BO", "learn"])
def test_poisoned_workspace_changes_nothing(lib, shape):
    """Every workspace row the split-K kernel reads is written by the tile kernel, the padding tiles' rows included: on a workspace
    of NaNs the result is finite and bitwise the one on a workspace of zeros."""
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 31, shape)
    fused = FusedPolicy(p)
    for b in (1, 17, 33):
        obs = _obs(torch, b, 3, 31 + b)
        ro = _rollout(torch, p, obs, 31 + b)
        need = _ws_bytes(lib, 3, shape, b)
        out = []
        for fill in (0xFF, 0x00):
            fused._grad_ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda:0")
            if fill:
                assert bool(torch.isnan(fused._grad_ws.view(torch.float32)).all())
            ws = fused._grad_ws
            out.append(_kernel(torch, fused, obs, ro, None, None, 0.2, 0.5, 0.01))
            assert fused._grad_ws is ws                       # exactly the required size: the call did not replace it
        (g1, s1), (g0, s0) = out
        assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(s1).all()), (shape, b)
        assert torch.equal(g1, g0) and torch.equal(s1, s0), (shape, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WIDE))
def test_bitwise_properties(name):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    shape = WIDE[name]
    p = _policy(torch, 3, 21, shape)
    fused = FusedPolicy(p)
    obs = _obs(torch, 600, 3, 21)
    ro = _rollout(torch, p, obs, 21)
    ms = torch.tensor([0.3, 1.7], device="cuda:0")
    # an index over a larger buffer (duplicates allowed) against the pre-gathered rows; 209 rows: 13 full tiles and one row
    idx = torch.randint(0, 600, (209,), device="cuda:0")
    g1, s1 = _kernel(torch, fused, obs, ro, idx, ms, 0.2, 0.5, 0.01)
    gathered = ({k: v[idx].contiguous() for k, v in obs.items()}, {k: v[idx].contiguous() for k, v in ro.items()})
    g2, s2 = _kernel(torch, fused, gathered[0], gathered[1], None, ms, 0.2, 0.5, 0.01)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    # two calls on the same inputs, a call of another size (which grows the workspace) between them
    _kernel(torch, fused, obs, ro, None, ms, 0.2, 0.5, 0.0)
    g3, s3 = _kernel(torch, fused, obs, ro, idx, ms, 0.2, 0.5, 0.01)
    assert torch.equal(g1, g3) and torch.equal(s1, s3)
    # LIDAR rows 8-12 and columns 24-25 are never read
    poked = {k: v.clone() for k, v in gathered[0].items()}
    poked["lidar"][:, :, 8:, :] = 1e6
    poked["lidar"][:, :, :, 24:] = -1e6
    g4, s4 = _kernel(torch, fused, poked, gathered[1], None, ms, 0.2, 0.5, 0.01)
    assert torch.equal(g2, g4) and torch.equal(s2, s4)
    poked["lidar"][:, :, 7, 23] += 1.0     # ... and a used cell is
    assert not torch.equal(g2, _kernel(torch, fused, poked, gathered[1], None, ms, 0.2, 0.5, 0.01)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
def test_default_shape_is_bitwise_the_unshaped_call(lib, c):
    torch = _gpu()
    n, m = 2049, 2100
    rng = np.random.default_rng(3000 + c)
    u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32)).to("cuda:0")
    words = C.c_size_t()
    assert lib.te_policy_param_words(c, C.byref(words)) == 0
    params = u(-0.1, 0.1, words.value)
    lidar, inertial, last_action = u(0, 1, m, c, 13, 26), u(-1, 1, m, 15), u(-1, 1, m, 4)
    action, old_logp, adv, ret = u(-1, 1, m, 4), u(-5, -3.5, m), u(-2, 2, m), u(-1, 1, m)
    index = torch.from_numpy(rng.permutation(m)[:n].astype(np.int64)).to("cuda:0")
    ms = torch.tensor([0.1, 1.3], device="cuda:0")
    ws = torch.empty(_ws_bytes(lib, c, DEFAULT, n), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for fn, first in ((lib.te_policy_ppo_grad, c), (lib.te_policy_ppo_grad_shaped, C.byref(_shape(c, *DEFAULT)))):
        grad = torch.full((words.value,), float("nan"), device="cuda:0")
        stats = torch.full((4,), float("nan"), device="cuda:0")
        rc = fn(params.data_ptr(), first, n, index.data_ptr(), lidar.data_ptr(), inertial.data_ptr(), last_action.data_ptr(), action.data_ptr(),
                old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), ms.data_ptr(), 0.2, 0.5, 0.01, grad.data_ptr(), stats.data_ptr(),
                ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, lib.te_last_error()
        torch.cuda.synchronize()
        out.append((grad, stats))
    assert bool(torch.isfinite(out[0][0]).all()) and 0.0 < float(out[0][1][3]) < 1.0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_graph_replay_sees_refreshed_weights():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy
    p = _policy(torch, 3, 27, BO)
    fused = FusedPolicy(p)
    obs = _obs(torch, 33, 3, 27)
    ro = _rollout(torch, p, obs, 27)
    ms = torch.tensor([0.3, 1.7], device="cuda:0")
    grad = torch.zeros_like(fused.params)
    stats = torch.zeros(4, device="cuda:0")
    call = lambda: fused.ppo_grad(obs, None, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, 0.2, 0.5, 0.01, grad, stats)
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
    eager, eager_s = _kernel(torch, fused, obs, ro, None, ms, 0.2, 0.5, 0.01)
    assert torch.equal(grad, eager) and torch.equal(stats, eager_s)
    assert not torch.equal(first, grad)


@pytest.mark.gpu
@pytest.mark.parametrize("fused_optimizer", [False, True])
def test_ppo_update_matches_autograd(fused_optimizer):
    """Reference BO on stage03: one update() of the autograd learner and of the fused one from the same rollout."""
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, _packed_order
    cfg = dict(n_steps=8, batch_size=256, n_epochs=1, use_graph=False, features_dim=BO[0], net_arch=BO[1])
    envs = [BatchedEnv(default_config("stage03", n_envs=64, max_step=40), "cuda:0") for _ in range(2)]
    ref = PPO(envs[0], PPOConfig(**cfg), seed=4)
    new = PPO(envs[1], PPOConfig(**cfg, fused_update=True, fused_update_wide=True, fused_optimizer=fused_optimizer, fused_forward=True), seed=4)
    assert new.fused_grad.net_arch == BO[1]
    for a, b in zip(ref.policy.parameters(), new.policy.parameters()):
        assert torch.equal(a, b)
    ref.collect()
    for k in ref.buf.obs:
        new.buf.obs[k].copy_(ref.buf.obs[k])
    for name in ("actions", "logp", "values", "rewards", "dones", "adv", "ret"):
        getattr(new.buf, name).copy_(getattr(ref.buf, name))
    before = [q.detach().clone() for q in ref.policy.parameters()]
    torch.manual_seed(8); u_ref = ref.update()
    torch.manual_seed(8); u_new = new.update()
    for log in (u_ref, u_new):
        assert all(np.isfinite(v) for v in log.values() if isinstance(v, float)), log
    moved = max(float((a - q.detach()).abs().max()) for a, q in zip(before, ref.policy.parameters()))
    assert all(not torch.equal(a, q.detach()) for a, q in zip(before, new.policy.parameters()))
    gap = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(ref.policy.parameters(), new.policy.parameters()))
    print(f"\nfused_optimizer={fused_optimizer}: parameters moved up to {moved:.3e}; fused_update_wide vs autograd: largest |d| {gap:.3e}")
    assert gap <= 5e-5, gap
    assert gap < 0.1 * moved, (gap, moved)
    if fused_optimizer:        # the module's parameters are the packed buffer
        off = 0
        for q in _packed_order(new.policy):
            assert q.data_ptr() == new.fused_grad.params.data_ptr() + 4 * off
            off += q.numel()
        assert off == new.fused_grad.params.numel()
    # the next rollout flies the updated weights through te_policy_act_shaped
    new.collect()
    b = new.buf
    T, N = b.rewards.shape
    flat = {k: o.reshape(T * N, *o.shape[2:]).contiguous() for k, o in b.obs.items()}
    with torch.no_grad():
        mu_ref, v_ref = new.policy(flat)
        mu, _ = new.fused.forward(flat)
    assert bool(((mu - mu_ref).abs() <= 1e-4 + 1e-4 * mu_ref.abs()).all())
    assert bool(((b.values.reshape(-1) - v_ref.reshape(-1)).abs() <= 1e-4 + 1e-4 * v_ref.reshape(-1).abs()).all())
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_ppo_on_exp05_trains_the_learn_shape_fused():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig, pack_policy
    env = BatchedEnv(default_config("exp05", n_envs=128, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=8, batch_size=512, n_epochs=2, wingman_driver="snapshot", fused_update=True, fused_update_wide=True,
                             fused_optimizer=True, features_dim=LEARN[0], net_arch=LEARN[1]), seed=4)
    assert (ppo.wingman.features_dim, ppo.wingman.net_arch) == LEARN and ppo.wingman.policy is not ppo.policy
    ptr = ppo.wingman.params.data_ptr()
    before = ppo.fused_grad.params.clone()
    for _ in range(2):
        log = ppo.collect()
        log.update(ppo.update())
        assert all(np.isfinite(v) for v in log.values() if isinstance(v, float)), log
    assert bool(torch.isfinite(ppo.fused_grad.params).all()) and not torch.equal(before, ppo.fused_grad.params)
    ppo.sync_wingmen()
    torch.cuda.synchronize()
    assert ppo.wingman.params.data_ptr() == ptr
    assert torch.equal(ppo.wingman.params, pack_policy(ppo.policy))
    env.close()
