"""What the fused policy kernels' test files (tests/test_policy_*.py) share: the C shape struct, random and trained policies on the GPU,
random observations and PPO minibatches, the autograd statement of PPO's loss, the call of the gradient kernel and its comparison with
that reference.  Seeds, row counts, tolerances and the record of the worst gap stay with each test file, which passes them in."""
import ctypes as C

import pytest

DEFAULT = (256, (64, 64))      # (features_dim, net_arch) of the default policy


class StubEnv:
    """What PPO.__init__ reads of an environment, on the CPU (no stepping, no GPU): `task`'s config (None: no cfg, as a backend without
    one) for n envs.  `resets` counts the reset() calls: a PPO(...) that refuses must leave it at 0."""

    def __init__(self, task="stage03", n=4):
        import torch
        from dronechase_amd import default_config
        self.cfg = None if task is None else default_config(task, n_envs=n)
        self.N, self.device, self.resets = n, torch.device("cpu"), 0
        self.lidar, self.inertial = torch.zeros(n, 3, 13, 26), torch.zeros(n, 15)

    def reset(self):
        self.resets += 1


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _shape(c, features_dim, net_arch, n_hidden=None):
    from dronechase_amd import _lib
    h = list(net_arch)[:4] + [0] * (4 - min(4, len(net_arch)))
    return _lib.PolicyShape(c, features_dim, len(net_arch) if n_hidden is None else n_hidden, (C.c_int32 * 4)(*h))


def _obs(torch, n, c, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, device="cuda:0")
    return {"lidar": u(n, c, 13, 26), "inertial_data": u(n, 15) * 2 - 1, "last_action": u(n, 4) * 2 - 1}


def _policy(torch, c, seed, shape=DEFAULT):
    from dronechase_amd.ppo import LidarInertialActionPolicy
    torch.manual_seed(seed)
    p = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=shape[0], net_arch=shape[1]).to("cuda:0")
    with torch.no_grad():
        p.log_std.copy_(torch.tensor([0.2, -0.3, 0.1, -0.5]))
    return p


def _trained_policy(torch, c, n_envs, batch_size, shape=DEFAULT):
    """Weights after a short PPO run (autograd update) on the real environment, and the 8 x n_envs te_step observations of that run's
    last rollout."""
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    env = BatchedEnv(default_config("stage03", n_envs=n_envs, max_step=40, lidar_channels=c), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=8, batch_size=batch_size, n_epochs=2, features_dim=shape[0], net_arch=shape[1]), seed=2)
    ppo.collect(); ppo.update(); ppo.collect()
    obs = {k: v.reshape(-1, *v.shape[2:]).clone() for k, v in ppo.buf.obs.items()}
    policy = ppo.policy
    env.close()
    return policy, obs


def _rollout(torch, policy, obs, seed, shift=0.3):
    """action, old_logp, adv, ret for the rows of obs: actions drawn from the policy, old_logp its log-prob shifted by
    N(0, shift) so that both branches of the clip are taken."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    n = obs["lidar"].shape[0]
    r = lambda *s: torch.randn(*s, generator=g, device="cuda:0")
    with torch.no_grad():
        d, v = policy.dist(obs)
        action = d.mean + d.stddev * r(n, 4)
        old_logp = d.log_prob(action).sum(-1) + shift * r(n)
    return {"action": action.contiguous(), "old_logp": old_logp.contiguous(), "adv": (r(n) * 2 + 0.3).contiguous(),
            "ret": (v + r(n)).contiguous()}


def _ref(torch, policy, obs, ro, index, norm, clip, vf, ent, dtype=None):
    """Autograd through the module (fp32; or a copy in `dtype`): (packed gradient, [pg, vl, ent, clip_frac], the [mean, std]
    the kernel gets)."""
    import copy
    from dronechase_amd.ppo import _packed_order
    if dtype is not None:
        policy = copy.deepcopy(policy).to(dtype)
        obs = {k: v.to(dtype) for k, v in obs.items()}
        ro = {k: v.to(dtype) for k, v in ro.items()}
    sel = (lambda t: t) if index is None else (lambda t: t[index])
    params = _packed_order(policy)
    mu, v = policy({k: sel(o) for k, o in obs.items()})
    d = torch.distributions.Normal(mu, policy.log_std.exp().expand_as(mu), validate_args=False)
    logp = d.log_prob(sel(ro["action"])).sum(-1)
    a = sel(ro["adv"])
    ms = torch.stack((a.mean(), a.std())) if norm else None
    if norm:
        a = (a - a.mean()) / (a.std() + 1e-8)
    ratio = (logp - sel(ro["old_logp"])).exp()
    pg = -torch.min(a * ratio, a * ratio.clamp(1 - clip, 1 + clip)).mean()
    vl = torch.nn.functional.mse_loss(v, sel(ro["ret"]))
    e = d.entropy().sum(-1).mean()
    loss = pg + vf * vl - ent * e
    grads = torch.autograd.grad(loss, params)
    stats = torch.stack((pg, vl, e, ((ratio - 1).abs() > clip).float().mean())).detach()
    return torch.cat([g.reshape(-1) for g in grads]).float(), stats.float(), (ms.detach().float().contiguous() if norm else None)


def _kernel(torch, fused, obs, ro, index, ms, clip, vf, ent):
    grad = torch.full_like(fused.params, float("nan"))
    stats = torch.full((4,), float("nan"), device="cuda:0")
    fused.ppo_grad(obs, index, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, clip, vf, ent, grad, stats)
    torch.cuda.synchronize()
    return grad, stats


def _compare(torch, policy, grad, ref, stats, ref_stats, label, rows, ref64, tol, gap):
    """Every packed tensor within REL ||g||_inf + ABS + KINK / B of the fp32 reference (tol: the caller's REL, ABS, KINK), the
    statistics within REL |s| + ABS; the gaps of all tensors that are not are reported together, with the fp64 module's view of them
    (ref64(): computed only then).  gap: the caller's {"grad", "stats"} record of the largest |d| / bound seen."""
    from dronechase_amd.ppo import _packed_order
    REL, ABS, KINK = tol
    names = [n for n, _ in policy.named_parameters() if n != "log_std"] + ["log_std"]
    off, bad, r64 = 0, [], None
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all()), label
    for name, p in zip(names, _packed_order(policy)):
        sl = slice(off, off + p.numel())
        g, r = grad[sl], ref[sl]
        off += p.numel()
        d, bound = float((g - r).abs().max()), REL * float(r.abs().max()) + ABS + KINK / rows
        gap["grad"] = max(gap["grad"], d / bound)
        if d > bound:
            r64 = ref64() if r64 is None else r64
            bad.append(f"{name}: |d| {d:.3e} > {bound:.3e} (||g|| {float(r.abs().max()):.3e}); vs fp64: kernel "
                       f"{float((g - r64[sl]).abs().max()):.3e}, fp32 autograd {float((r - r64[sl]).abs().max()):.3e}")
    assert off == grad.numel()
    ds = (stats - ref_stats).abs()
    sb = REL * ref_stats.abs() + ABS
    gap["stats"] = max(gap["stats"], float((ds / sb).max()))
    if not bool((ds <= sb).all()):
        bad.append(f"stats {stats.tolist()} vs {ref_stats.tolist()}")
    if bad:
        print(f"\n{label}:\n  " + "\n  ".join(bad))
    assert not bad, f"{label}: {bad}"
