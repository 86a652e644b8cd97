"""te_policy_adam_step (dronechase_amd/csrc/te_policy_opt.hpp): clip_grad_norm_ + Adam on one flat buffer in two launches, and the
layers above it (FusedPolicy.bind_parameters, PackedAdam, PPOConfig.fused_optimizer).

Tolerance of the parity test, per element after step k, against the same formulas in fp64 on the same fp32 inputs:
  |p - p64| <= k (1.2e-7 |p64| + 4e-5 lr)
The first term is one fp32 rounding of the stored parameter per step (2^-24, doubled).  The second is the largest possible update,
lr (1 - beta1) / sqrt(1 - beta2) ~ 3.2 lr, times a relative error budget of 1e-5 for the fp32 sum of 2.3e5 squares, the square root
and the divisions.  m and v: 1e-5 relative + 1e-12.  The inputs keep every element's sign over the K steps (m has no cancellation,
so a relative bound on it means something); clip_grad_norm_ + torch.optim.Adam(foreach=False) in fp32 on the same inputs must pass
the same bounds (else the inputs are wrong, not the kernel) and lands within twice the bounds of the kernel.  The measured gaps are
printed (pytest -s).  No bound depends on the word count, and the parity test also runs past 256 norm partials (LOOP_SIZES), where
policy_adam_kernel's threads re-sum more than one partial each: measured there as at the policy's size (kernel 0.354, m 0.027, v
0.002, norm 0.010 of the bounds; torch fp32 on the GPU 0.354).  torch's fp32 norm on a CPU is another matter at 2 101 251 words: it is
1.5e-5 off the fp64 norm whatever the seed (1.4e-6 at 1 048 577), so clip_grad_norm_ + Adam on the CPU misses m's bound there
(1.27) and could not be this test's witness; on the GPU torch's fp32 step passes every bound at both sizes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests._adam_ref import ref64_step
from tests._policy_cases import _gpu, _obs, _policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 4096                     # kOptSlice: the words one workgroup owns
HEADER_WORDS = 16
LR, B1, B2, EPS, MAX_NORM = 3e-4, 0.9, 0.999, 1e-5, 0.5
NORMS = (5.0, 0.1, 2.0, 0.3, 20.0)           # of the K = 5 gradients: steps 1, 3, 5 clip at 0.5, steps 2 and 4 do not
SIZES = (1, 5, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 234537, 235049)
# more than 256 norm partials: policy_adam_kernel's threads take a second (257: thread 0 alone) and a third trip round their re-sum.
# The lone 257th partial is one word's square, 1e-6 of the squared norm: at that size the 1e-5 bound holds the loop to reading nothing
# it should not, at 514 partials to reading all it should (the first 256 alone leave the norm 39 000 bounds low)
LOOP_SIZES = (256 * SLICE + 1, 513 * SLICE + 3)


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _state_bytes(lib, words):
    out = C.c_size_t()
    assert lib.te_policy_opt_state_bytes(words, C.byref(out)) == 0, lib.te_last_error()
    return out.value


def _align4(words):
    return (words + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "threatengage.h")).read(), flags=re.S)
    for name in ("te_policy_opt_state_bytes", "te_policy_adam_step"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None


def test_state_bytes(lib):
    sizes = (1, 2, 3, 4, 5, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 234537, 235049, 1 << 24)
    got = [_state_bytes(lib, w) for w in sizes]
    assert all(a <= b for a, b in zip(got, got[1:])), got
    for w, b in zip(sizes, got):
        assert b >= 8 * w and b % 16 == 0
        # the documented layout: 64-byte header, m and v padded to 16 bytes, one partial per 4 096 words padded to 16 bytes
        assert b == 64 + 2 * 4 * _align4(w) + 4 * _align4((w + SLICE - 1) // SLICE), (w, b)
    out = C.c_size_t()
    assert lib.te_policy_opt_state_bytes(0, C.byref(out)) != 0 and b"words must be positive" in lib.te_last_error()
    assert lib.te_policy_opt_state_bytes(8, None) != 0 and b"null" in lib.te_last_error()


def test_bad_arguments_fail_through_last_error(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    need = _state_bytes(lib, 100)
    base = dict(params=fake, grad=fake, state=fake, state_bytes=need, words=100, lr=LR, b1=B1, b2=B2, eps=EPS, max_norm=MAX_NORM,
                scale=1.0, stream=None)
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]
    inf, nan = float("inf"), float("nan")
    cases = [(dict(params=None), b"null"), (dict(grad=None), b"null"), (dict(state=None), b"null"),
             (dict(params=fake + 4), b"params must be 16-byte"), (dict(grad=fake + 8), b"grad must be 16-byte"),
             (dict(state=fake + 4), b"state must be 16-byte"), (dict(words=0), b"words must be positive"),
             (dict(state_bytes=need - 1), b"state too small"), (dict(state_bytes=0), b"state too small"),
             (dict(words=101), b"state too small"), (dict(lr=-1e-3), b"lr must be"), (dict(lr=nan), b"lr must be"),
             (dict(b1=1.0), b"beta1 must be in [0, 1)"), (dict(b1=-0.1), b"beta1 must be in [0, 1)"), (dict(b1=nan), b"beta1"),
             (dict(b2=1.0), b"beta2 must be in [0, 1)"), (dict(b2=-0.1), b"beta2 must be in [0, 1)"),
             (dict(eps=0.0), b"eps must be"), (dict(eps=-1e-5), b"eps must be"), (dict(max_norm=0.0), b"max_grad_norm must be > 0"),
             (dict(max_norm=-1.0), b"max_grad_norm must be > 0"), (dict(max_norm=nan), b"max_grad_norm must be > 0"),
             (dict(scale=inf), b"grad_scale must be finite"), (dict(scale=nan), b"grad_scale must be finite")]
    for kw, msg in cases:
        assert lib.te_policy_adam_step(*args(**kw)) != 0, kw
        assert msg in lib.te_last_error(), (kw, lib.te_last_error())


def test_fused_optimizer_needs_fused_update():
    from dronechase_amd.ppo import PPOConfig
    with pytest.raises(ValueError, match="fused_optimizer.*needs fused_update"):
        PPOConfig(fused_optimizer=True)
    assert PPOConfig().fused_optimizer is False
    assert PPOConfig(fused_update=True, fused_optimizer=True).fused_optimizer


# ---------------------------------------------------------------------------------------------------------- MI355X
def _zero_block(words):
    return slice(words // 5, 2 * words // 5)      # never-read cells: exact zeros in every gradient (empty for words == 1)


_INPUTS = {}


def _inputs(torch, words):
    """(p0 [words], grads: K tensors [words]) fp32 on the device, seeded; computed once per size and never written.  Every gradient is a
    tensor of its own: row k of one stacked [K, words] tensor would start 4 * k * words bytes in, 16-byte aligned only where words is
    a multiple of 4, and te_policy_adam_step refuses an unaligned gradient."""
    if words not in _INPUTS:
        rng = np.random.default_rng(4000 + words)
        p0 = (0.1 * rng.standard_normal(words)).astype(np.float32)
        sign = np.where(rng.random(words) < 0.5, -1.0, 1.0)
        grads = []
        for norm in NORMS:
            g = sign * (0.05 + np.abs(rng.standard_normal(words)))
            g[_zero_block(words)] = 0.0
            grads.append((g * (norm / np.linalg.norm(g))).astype(np.float32))
        _INPUTS[words] = (torch.from_numpy(p0).to("cuda:0"), tuple(torch.from_numpy(g).to("cuda:0") for g in grads))
        assert all(g.data_ptr() % 16 == 0 for g in _INPUTS[words][1])
    return _INPUTS[words]


def _fresh(lib, torch, words):
    p0, _ = _inputs(torch, words)
    return p0.clone(), torch.zeros(_state_bytes(lib, words) // 4, dtype=torch.float32, device="cuda:0")


def _m_v(state, words):
    a = _align4(words)
    return state[HEADER_WORDS:HEADER_WORDS + words], state[HEADER_WORDS + a:HEADER_WORDS + a + words]


def _step(lib, torch, p, g, state, max_norm=MAX_NORM, scale=1.0):
    rc = lib.te_policy_adam_step(p.data_ptr(), g.data_ptr(), state.data_ptr(), state.numel() * 4, p.numel(), LR, B1, B2, EPS, max_norm, scale,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.te_last_error()


def _ref64_step(torch, p, m, v, g32, k):
    """The issue's formulas in fp64 (tests/_adam_ref.py): p, m, v fp64, the gradient the fp32 input."""
    return ref64_step(torch, p, m, v, g32, k, LR, B1, B2, EPS, MAX_NORM)


@pytest.mark.gpu
@pytest.mark.parametrize("words", SIZES + LOOP_SIZES)
def test_parity_with_torch(lib, words):
    torch = _gpu()
    p0, grads = _inputs(torch, words)
    p, state = _fresh(lib, torch, words)
    m, v = _m_v(state, words)
    p64, m64, v64 = p0.double(), torch.zeros(words, dtype=torch.float64, device="cuda:0"), torch.zeros(words, dtype=torch.float64, device="cuda:0")
    pt = torch.nn.Parameter(p0.clone())
    adam = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    zb = _zero_block(words)
    worst = {"kernel": 0.0, "torch32": 0.0, "pair": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for k in range(1, len(NORMS) + 1):
        g = grads[k - 1]
        _step(lib, torch, p, g, state)
        p64, m64, v64 = _ref64_step(torch, p64, m64, v64, g, k)
        pt.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([pt], MAX_NORM)
        adam.step()
        torch.cuda.synchronize()
        bound = k * (1.2e-7 * p64.abs() + 4e-5 * LR)
        gap = lambda x: float(((x.detach().double() - p64).abs() / bound).max())
        worst["kernel"], worst["torch32"] = max(worst["kernel"], gap(p)), max(worst["torch32"], gap(pt))
        worst["pair"] = max(worst["pair"], float(((p.double() - pt.detach().double()).abs() / (2 * bound)).max()))
        st = adam.state[pt]
        for name, got, got32, ref in (("m", m, st["exp_avg"], m64), ("v", v, st["exp_avg_sq"], v64)):
            tol = 1e-5 * ref.abs() + 1e-12
            assert bool(((got32.double() - ref).abs() <= tol).all()), f"the inputs are wrong: torch fp32's {name} misses the bound at step {k}"
            worst[name] = max(worst[name], float(((got.double() - ref).abs() / tol).max()))
        # the header: the step, the norm before clipping and the coefficient that follows from it
        assert int(state[0:1].view(torch.int32)) == k
        norm, coef = float(state[1]), float(state[2])
        ref_norm = float(torch.linalg.vector_norm(g))
        worst["norm"] = max(worst["norm"], abs(norm - ref_norm) / (1e-5 * ref_norm))
        want = min(np.float32(1.0), np.float32(MAX_NORM) / (np.float32(norm) + np.float32(1e-6)))
        assert abs(coef - float(want)) <= 1e-6 * float(want), (k, coef, want)
        assert (coef < 1.0) == (NORMS[k - 1] > MAX_NORM) and (coef == 1.0) == (NORMS[k - 1] < MAX_NORM), (k, coef)
        # elements whose gradients are all zero: bitwise unchanged, no moments
        assert torch.equal(p[zb], p0[zb]) and not bool(m[zb].any()) and not bool(v[zb].any())
    print(f"\nwords={words}: largest gap / bound over {len(NORMS)} steps: " + ", ".join(f"{n} {x:.3f}" for n, x in worst.items()))
    assert worst["torch32"] <= 1.0, "the inputs are wrong: torch fp32 itself misses the bound"
    assert worst["kernel"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0 and worst["norm"] <= 1.0, worst
    assert worst["pair"] <= 1.0, worst
    assert bool((p != p0).any())


W = 2 * SLICE + 3               # three workgroups, a 3-word tail


def _run(lib, torch, steps=3, scale=1.0, gscale=1.0):
    _, grads = _inputs(torch, W)
    p, state = _fresh(lib, torch, W)
    for k in range(steps):
        _step(lib, torch, p, (grads[k] * gscale).contiguous(), state, scale=scale)
    torch.cuda.synchronize()
    return p, state


@pytest.mark.gpu
def test_repeated_runs_are_bitwise_equal(lib):
    torch = _gpu()
    (p1, s1), (p2, s2) = _run(lib, torch), _run(lib, torch)
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert int(s1[0:1].view(torch.int32)) == 3


@pytest.mark.gpu
def test_grad_scale_is_a_scaled_gradient(lib):
    torch = _gpu()
    (p1, s1), (p2, s2) = _run(lib, torch, scale=0.5), _run(lib, torch, gscale=0.5)
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert not torch.equal(p1, _run(lib, torch)[0])


@pytest.mark.gpu
def test_no_clipping_with_infinite_max_norm(lib):
    torch = _gpu()
    _, grads = _inputs(torch, W)
    p, state = _fresh(lib, torch, W)
    _step(lib, torch, p, grads[0], state, max_norm=float("inf"))
    torch.cuda.synchronize()
    assert float(state[2]) == 1.0 and abs(float(state[1]) - NORMS[0]) <= 1e-5 * NORMS[0]


@pytest.mark.gpu
def test_graph_replay_advances_the_step(lib):
    torch = _gpu()
    _, grads = _inputs(torch, W)
    eager_p, eager_s = _run(lib, torch)
    p, state = _fresh(lib, torch, W)
    p_start, g = p.clone(), grads[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(lib, torch, p, g, state)           # everything is loaded and sized outside the capture ...
    torch.cuda.current_stream().wait_stream(side)
    p.copy_(p_start); state.zero_()              # ... and undone: a zero state is a fresh optimiser
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(lib, torch, p, g, state)
    for k in range(3):
        g.copy_(grads[k])
        graph.replay()
    torch.cuda.synchronize()
    assert int(state[0:1].view(torch.int32)) == 3
    assert torch.equal(p, eager_p) and torch.equal(state.view(torch.int32), eager_s.view(torch.int32))


def _grad_like(torch, params, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return 0.01 * torch.randn(params.numel(), generator=g, device="cuda:0")


@pytest.mark.gpu
def test_checkpoint_continues_bitwise():
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy, PackedAdam
    a = FusedPolicy(_policy(torch, 3, 31))
    opt = PackedAdam(a, lr=LR)
    grads = [_grad_like(torch, a.params, s) for s in range(4)]
    for g in grads[:2]:
        opt.step(g, MAX_NORM)
    saved, weights = opt.state_dict(), a.params.clone()
    for g in grads[2:]:
        opt.step(g, MAX_NORM)
    b = FusedPolicy(_policy(torch, 3, 32))
    b.params.copy_(weights)
    opt_b = PackedAdam(b, lr=LR)
    assert int(opt_b.step_count) == 0
    opt_b.load_state_dict(saved)
    assert int(opt_b.step_count) == 2 and saved["state"].data_ptr() != opt_b.state.data_ptr()
    for g in grads[2:]:
        opt_b.step(g, MAX_NORM)
    torch.cuda.synchronize()
    assert int(opt.step_count) == int(opt_b.step_count) == 4
    assert torch.equal(a.params, b.params) and torch.equal(opt.state.view(torch.int32), opt_b.state.view(torch.int32))
    assert torch.equal(opt.exp_avg, opt_b.exp_avg) and bool(opt.exp_avg_sq.any()) and float(opt.grad_norm) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
def test_bound_parameters_are_the_packed_buffer(c):
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy, PackedAdam, _packed_order, pack_policy
    policy = _policy(torch, c, 41)
    fused = FusedPolicy(policy)
    packed = fused.params.clone()
    fused.bind_parameters()

    def assert_bound():
        off = 0
        for q in _packed_order(policy):
            assert q.data_ptr() == fused.params.data_ptr() + 4 * off
            off += q.numel()
        assert off == fused.params.numel()

    assert_bound()
    assert torch.equal(fused.params, packed)
    fused.refresh()
    assert torch.equal(fused.params, packed)
    PackedAdam(fused, lr=LR).step(_grad_like(torch, fused.params, 5), MAX_NORM)
    torch.cuda.synchronize()
    assert not torch.equal(fused.params, packed)
    assert torch.equal(pack_policy(policy), fused.params)
    obs = _obs(torch, 64, c, 9)
    with torch.no_grad():
        mu_ref, v_ref = policy(obs)
    mu, v = fused.forward(obs)
    torch.testing.assert_close(mu, mu_ref, atol=1e-4, rtol=1e-4)       # tests/test_policy_fused.py's tolerance
    torch.testing.assert_close(v, v_ref, atol=1e-4, rtol=1e-4)
    other = _policy(torch, c, 42)
    fused.load_from(other)
    assert torch.equal(fused.params, pack_policy(other)) and not torch.equal(fused.params, packed)
    assert_bound()


def _copy_rollout(src, dst):
    for k in src.buf.obs:
        dst.buf.obs[k].copy_(src.buf.obs[k])
    for name in ("actions", "logp", "values", "rewards", "dones", "adv", "ret"):
        getattr(dst.buf, name).copy_(getattr(src.buf, name))


@pytest.mark.gpu
def test_ppo_update_matches_the_torch_optimizer():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PackedAdam, PPOConfig
    cfg = dict(n_steps=8, batch_size=2048, n_epochs=2, use_graph=False, fused_update=True)
    envs = [BatchedEnv(default_config("stage03", n_envs=1024, max_step=40), "cuda:0") for _ in range(2)]
    ref = PPO(envs[0], PPOConfig(**cfg), seed=4)
    new = PPO(envs[1], PPOConfig(**cfg, fused_optimizer=True), seed=4)
    assert isinstance(new.opt, PackedAdam) and isinstance(ref.opt, torch.optim.Adam) and new.fused_grad.bound and not ref.fused_grad.bound
    for a, b in zip(ref.policy.parameters(), new.policy.parameters()):
        assert torch.equal(a, b)
    ref.collect()
    _copy_rollout(ref, new)
    before = [q.detach().clone() for q in new.policy.parameters()]
    torch.manual_seed(8); u_ref = ref.update()
    torch.manual_seed(8); u_new = new.update()
    moved = max(float((a - q.detach()).abs().max()) for a, q in zip(before, new.policy.parameters()))
    gap = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(ref.policy.parameters(), new.policy.parameters()))
    print(f"\nparameters moved up to {moved:.3e}; fused_optimizer vs clip_grad_norm_ + torch Adam: largest |d| {gap:.3e}; "
          f"grad_norm {u_new['grad_norm']:.4f}")
    assert moved > 1e-4
    assert gap <= 5e-5, gap                 # the bound the project holds between fused_update and autograd (1.6e-5 measured there)
    assert set(u_new) == set(u_ref) | {"grad_norm"} and "grad_norm" not in u_ref
    for k in u_ref:
        assert abs(u_ref[k] - u_new[k]) <= 1e-4 * abs(u_ref[k]) + 1e-5, (k, u_ref[k], u_new[k])
    assert math.isfinite(u_new["grad_norm"]) and u_new["grad_norm"] > 0.0
    assert int(new.opt.step_count) == 2 * 4
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_learn_with_every_fused_path():
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=1024, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=4, batch_size=2048, n_epochs=2, use_graph=True, fused_forward=True, fused_update=True,
                             fused_optimizer=True), seed=6)
    assert ppo.fused is ppo.fused_grad and ppo.fused.bound
    before = [q.detach().clone() for q in ppo.policy.parameters()]
    logs = []
    ppo.learn(2 * 4 * 1024, log=logs.append)
    assert len(logs) == 2
    for rec in logs:
        assert "grad_norm" in rec and all(np.isfinite(v) for v in rec.values() if isinstance(v, float)), rec
    assert all(not torch.equal(a, q.detach()) for a, q in zip(before, ppo.policy.parameters()))
    # the captured rollout graph flew the optimiser's weights with no repack: the module and the packed buffer are one
    with torch.no_grad():
        mu_ref, v_ref = ppo.policy(ppo._obs)
    mu, v = ppo.fused.forward(ppo._obs)
    torch.testing.assert_close(mu, mu_ref, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(v, v_ref, atol=1e-4, rtol=1e-4)
    env.close()
