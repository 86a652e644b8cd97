"""The numerics contract of te_policy_ppo_grad_bf16 (include/threatengage.h, dronechase_amd/csrc/te_policy_grad_bf16.hpp) stated as
PyTorch autograd on the CPU, and the fixed inputs of tests/test_policy_grad_bf16.py.  Three autograd functions carry the contract:
  RoundGrad   identity forward; the gradient is rounded to bf16 (nearest-even): one at every pre-activation, mu and value included
  ActQ        ReLU / tanh whose OUTPUT is rounded to bf16 where it is stored, differentiated on that stored output (y > 0, 1 - y^2)
  RoundSTE    the weights rounded to bf16 in the forward, the gradient passed straight through to the fp32 master weights
Everything else (the sums, the bias, the loss) runs in the dtype asked for: fp64 (E64) or fp32 (E32).  Nothing here sees a kernel."""
import copy
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from _kinkfree import CLIP, ENT_COEF, LOG_STD, LOGP_SHIFTS, SHAPES, VF_COEF

INSTANCES = [(name, c) for name in SHAPES for c in (2, 3)]
ROLLOUT, B = 96, 64
U = 2.0 ** -8            # half a bf16 ulp relative to the value: the size of one rounding
PAIR_CAP, KERNEL_CAP = 2.0, 6.0


def q(x):
    return x.float().bfloat16().to(x.dtype)         # round-to-nearest-even


class RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        return z.view_as(z)

    @staticmethod
    def backward(ctx, g):
        return q(g)


class ActQ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, tanh):
        y = q(torch.tanh(z) if tanh else torch.relu(z))
        ctx.save_for_backward(y)
        ctx.tanh = tanh
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return (g * (1 - y * y) if ctx.tanh else g * (y > 0).to(g.dtype)), None


class RoundSTE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w):
        return q(w)

    @staticmethod
    def backward(ctx, g):
        return g


def forward(policy, obs):
    """(mu, value) of the contract's forward in the dtype of `policy` and `obs`, differentiable by the contract's backward."""
    def seq(mods, x):
        for m in mods:
            if isinstance(m, nn.Conv2d):
                x = RoundGrad.apply(F.conv2d(x, RoundSTE.apply(m.weight), m.bias, stride=m.stride))
            elif isinstance(m, nn.Linear):
                x = RoundGrad.apply(F.linear(x, RoundSTE.apply(m.weight), m.bias))
            elif isinstance(m, (nn.ReLU, nn.Tanh)):
                x = ActQ.apply(x, isinstance(m, nn.Tanh))
            else:
                assert isinstance(m, nn.Flatten), m
                x = x.flatten(1)
        return x

    z = torch.cat((seq(policy.lidar, q(obs["lidar"])), seq(policy.inertial, q(obs["inertial_data"])), seq(policy.action, q(obs["last_action"]))), dim=1)
    f = seq(policy.final, z)
    last = lambda layer, x: RoundGrad.apply(F.linear(x, layer.weight, layer.bias))      # mu and value: fp32 weights, dmu / dv rounded
    return last(policy.mu, seq(policy.pi, f)), last(policy.value, seq(policy.vf, f)).squeeze(-1)


def row_terms(policy, obs, ro, ms):
    """Per row: (pg term, vl term, entropy, clipped) of PPO's loss, from the contract's forward."""
    mu, v = forward(policy, obs)
    d = torch.distributions.Normal(mu, policy.log_std.exp().expand_as(mu), validate_args=False)
    logp = d.log_prob(ro["action"]).sum(-1)
    a = ro["adv"] if ms is None else (ro["adv"] - ms[0]) / (ms[1] + 1e-8)
    ratio = (logp - ro["old_logp"]).exp()
    pg = -torch.min(a * ratio, a * ratio.clamp(1 - CLIP, 1 + CLIP))
    vl = (v - ro["ret"]) ** 2
    return pg, vl, d.entropy().sum(-1), ((ratio - 1).abs() > CLIP).to(pg.dtype), mu.detach(), v.detach()


def _cast(policy, obs, ro, ms, index, dtype):
    sel = (lambda t: t) if index is None else (lambda t: t[index])
    return (copy.deepcopy(policy).to(dtype), {k: sel(v).to(dtype) for k, v in obs.items()}, {k: sel(v).to(dtype) for k, v in ro.items()},
            None if ms is None else ms.to(dtype))


def gradient(policy, obs, ro, ms, index, dtype, n=None):
    """(packed gradient list, stats [4], per-row (pg, vl) terms) of the rows `index`, the loss a mean over n rows (default: all of them);
    results as fp64."""
    from dronechase_amd.ppo import _packed_order
    p, o, r, m = _cast(policy, obs, ro, ms, index, dtype)
    pg, vl, ent, clipped, _, _ = row_terms(p, o, r, m)
    n = n or pg.numel()
    loss = (pg.sum() + VF_COEF * vl.sum() - ENT_COEF * ent.sum()) / n
    grads = torch.autograd.grad(loss, _packed_order(p))
    stats = torch.stack((pg.sum(), vl.sum(), ent.sum(), clipped.sum())).detach() / n
    return [g.double() for g in grads], stats.double(), (pg.detach().double(), vl.detach().double())


def per_row(policy, obs, ro, ms, index):
    """E64 one row at a time: [rows][tensors] of each row's contribution to the gradient (the loss a mean over len(index) rows, the
    advantage normalisation fixed to ms).  Rows do not interact: every rounding of the contract is per row."""
    return [gradient(policy, obs, ro, ms, index[i:i + 1], torch.float64, n=len(index))[0] for i in range(len(index))]


def reference(policy, obs, ro, ms, index):
    """E64 (the sum of the per-row contributions, which is the batch's gradient), E32, R_t and the row that sets R_t, per tensor."""
    rows = per_row(policy, obs, ro, ms, index)
    nt = len(rows[0])
    e64 = [sum(r[t] for r in rows) for t in range(nt)]
    peak = [torch.stack([r[t].abs().max() for r in rows]) for t in range(nt)]
    _, stats64, terms = gradient(policy, obs, ro, ms, index, torch.float64)
    e32, stats32, _ = gradient(policy, obs, ro, ms, index, torch.float32)
    return dict(e64=e64, e32=e32, stats64=stats64, stats32=stats32, R=[float(p.max()) for p in peak], worst_row=[int(p.argmax()) for p in peak],
                rows=rows, pg_term=float(terms[0].abs().max()), vl_term=float(terms[1].abs().max()))


def make_policy(name, c, seed):
    from dronechase_amd.ppo import LidarInertialActionPolicy
    f, arch = SHAPES[name]
    torch.manual_seed(seed)
    policy = LidarInertialActionPolicy(lidar_shape=(c, 13, 26), features_dim=f, net_arch=arch)
    with torch.no_grad():
        policy.log_std.copy_(torch.tensor(LOG_STD))
    return policy


def make_rollout(policy, c, rows, seed):
    """Uniform observations; actions one sigma around the contract's mean; old_logp = logp - l with l from LOGP_SHIFTS in turn, so every
    ratio lies well away from 1 -+ clip; returns around the contract's value; normal advantages."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    obs = {"lidar": u(rows, c, 13, 26), "inertial_data": u(rows, 15) * 2 - 1, "last_action": u(rows, 4) * 2 - 1}
    with torch.no_grad():
        p64 = copy.deepcopy(policy).double()
        mu, v = forward(p64, {k: t.double() for k, t in obs.items()})
        action = (mu + p64.log_std.exp() * torch.randn(rows, 4, generator=g).double()).float()
        logp = torch.distributions.Normal(mu, p64.log_std.exp().expand_as(mu)).log_prob(action.double()).sum(-1)
        shifts = torch.tensor(LOGP_SHIFTS, dtype=torch.float64)[torch.arange(rows) % len(LOGP_SHIFTS)]
        ro = {"action": action, "old_logp": (logp - shifts).float(), "adv": torch.randn(rows, generator=g),
              "ret": (v + 0.3 * torch.randn(rows, generator=g).double()).float()}
    ms = torch.stack((ro["adv"].mean(), ro["adv"].std()))
    return obs, ro, ms


@functools.lru_cache(maxsize=None)
def case(name, c, seed=0, b=B):
    """One fixed case: the policy, a 96-row rollout, b rows of it through a shuffled index, and its references.  Computed once."""
    policy = make_policy(name, c, 5 + seed)
    obs, ro, ms = make_rollout(policy, c, ROLLOUT, 11 + 7 * seed + c)
    index = torch.randperm(ROLLOUT, generator=torch.Generator().manual_seed(3 + seed))[:b].contiguous()
    return dict(policy=policy, obs=obs, ro=ro, ms=ms, index=index, **reference(policy, obs, ro, ms, index))


def ratios(grads, ref):
    """Per tensor max |g - E64| / (2^-8 R_t)."""
    return [float((g.double().reshape(e.shape) - e).abs().max()) / (U * r) for g, e, r in zip(grads, ref["e64"], ref["R"])]
