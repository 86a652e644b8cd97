"""The fused learner (PPOConfig.fused_forward, fused_update, fused_advantages, with and without fused_optimizer) on two `gloo` ranks
that share cuda:0, as tests/test_gpu_two_ranks.py shares it: each rank owns 256 stage03 envs (env_index_base = rank * 256) and builds
its PPO with a seed of its own, so rank 0's broadcast, not a shared seed, is what makes the replicas equal.

One minibatch of PPO._fused_minibatch with fused_optimizer is pinned twice.  Bitwise: the packed parameters and the whole
PackedAdam.state after it are what a direct te_policy_adam_step call gives on the parameters and state from before, the gradient
g_0 + g_1 (each rank's own FusedPolicy.ppo_grad on its own rollout; fp32, two addends, so the order of the reduction cannot matter)
and grad_scale = 1 / 2: the same kernel on the same inputs, so any difference is the plumbing's (the all-reduce after the step, a
scale applied twice or not at all, a stale buffer).  Against fp64: the step is tests/_adam_ref.py's on the mean gradient
0.5 (g_0 + g_1), within tests/test_policy_opt.py's bound for one step, |p - p64| <= 1.2e-7 |p64| + 4e-5 lr, and the logged norm is
the mean gradient's to 1e-5 relative.  Then update() / collect() / update() with either optimiser: the replicas stay bitwise equal,
finite, and move.  The worker checks what one rank can see and exits non-zero on any miss; the parent compares the ranks' files."""
import os

import numpy as np
import pytest

from tests.test_gpu_two_ranks import _launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LOCAL, N_STEPS, BATCH = 256, 8, 512          # 2 048 rows per rank: four minibatches per epoch

WORKER = r"""
import math, os, sys
import numpy as np
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
if not torch.cuda.is_available():
    sys.exit("no GPU visible: the fused learner runs HIP kernels only")
from dronechase_amd import _lib, default_config
from dronechase_amd.batched_env import BatchedEnv
from dronechase_amd.ppo import PPO, PPOConfig, PackedAdam, _packed_order, adv_stats, pack_policy
from tests._adam_ref import ref64_step

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n_local, n_steps, batch, out_dir = {n_local}, {n_steps}, {batch}, {out_dir!r}
dev = torch.device("cuda:0")
fails, saved = [], {{}}


def check(ok, what):
    # every rank runs every collective whatever it found: the misses are reported together at the end
    if not ok:
        fails.append(what)
        print(f"rank {{rank}}: FAILED: {{what}}", file=sys.stderr, flush=True)


def make(seed, fused_optimizer):
    env = BatchedEnv(default_config("stage03", n_envs=n_local, env_index_base=rank * n_local, max_step=5), dev)   # episodes end inside a rollout
    cfg = PPOConfig(n_steps=n_steps, batch_size=batch, n_epochs=1, use_graph=False, fused_forward=True, fused_update=True,
                    fused_advantages=True, fused_optimizer=fused_optimizer)
    return env, PPO(env, cfg, seed=seed)


def gather(t):
    mine = t.detach().cpu().contiguous()
    bucket = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(bucket, mine)
    return [b.to(dev) for b in bucket]


def rollout(ppo):
    T, N = ppo.buf.rewards.shape
    flat = lambda x: x.reshape(T * N, *x.shape[2:])          # as update() builds them
    b = ppo.buf
    return {{k: flat(v) for k, v in b.obs.items()}}, flat(b.actions), flat(b.logp), flat(b.adv), flat(b.ret)


bits = lambda t: t.view(torch.int32)

# ------------------------------------------------------------------------------------------------ C1: one minibatch, pinned exactly
env, ppo = make(rank, True)
c = ppo.cfg
check(ppo.distributed and isinstance(ppo.opt, PackedAdam) and ppo.fused_grad.bound, "not a data-parallel PPO with the packed optimiser")
ppo.collect()
obs, actions, old_logp, adv, ret = rollout(ppo)
idx = torch.arange(batch, device=dev)
ms = torch.zeros(2, device=dev)
adv_stats(adv, idx, ms, ppo._adv_ws)                         # as _fused_minibatch does
g_mine, stats = torch.zeros_like(ppo._flat_grad), torch.zeros(4, device=dev)
ppo.fused_grad.ppo_grad(obs, idx, actions, old_logp, adv, ret, ms, c.clip_range, c.vf_coef, c.ent_coef, g_mine, stats)
p_before, s_before = ppo.fused_grad.params.clone(), ppo.opt.state.clone()
ppo._fused_minibatch(obs, idx, actions, old_logp, adv, ret)
torch.cuda.synchronize()
p_after, s_after, reduced = ppo.fused_grad.params.clone(), ppo.opt.state.clone(), ppo._flat_grad.clone()
g = gather(g_mine)
check(bool(torch.isfinite(g_mine).all()) and bool(g_mine.any()), "the rank's own gradient is not finite or all zero")
check(not torch.equal(g[0], g[1]), "(b) both ranks computed the same gradient: they did not see different rollouts")
g_sum = g[0] + g[1]
check(torch.equal(bits(reduced), bits(g_sum)), "the gradient bucket after the minibatch is not g_0 + g_1")
# (c) the same kernel, called directly
lib = _lib.load()
p_direct, s_direct = p_before.clone(), s_before.clone()
rc = lib.te_policy_adam_step(p_direct.data_ptr(), g_sum.data_ptr(), s_direct.data_ptr(), s_direct.numel() * 4, p_direct.numel(),
                             c.learning_rate, 0.9, 0.999, 1e-5, c.max_grad_norm, 0.5, torch.cuda.current_stream().cuda_stream)
check(rc == 0, f"te_policy_adam_step: {{lib.te_last_error()}}")
torch.cuda.synchronize()
check(torch.equal(bits(p_after), bits(p_direct)),
      f"(c) parameters differ from the direct step on g_0 + g_1 at grad_scale 0.5 in {{int((bits(p_after) != bits(p_direct)).sum())}} words")
check(torch.equal(bits(s_after), bits(s_direct)),
      f"(c) optimiser state differs from the direct step in {{int((bits(s_after) != bits(s_direct)).sum())}} words; "
      f"norm {{float(s_after[1])!r}} against {{float(s_direct[1])!r}}")
check(int(ppo.opt.step_count) == 1 and not torch.equal(p_after, p_before), "the minibatch did not take exactly one step")
# (d) the meaning of the step, in fp64
g_mean = 0.5 * (g[0].double() + g[1].double())
zeros = torch.zeros_like(g_mean)
p64, _, _ = ref64_step(torch, p_before.double(), zeros, zeros, g_mean, 1, c.learning_rate, 0.9, 0.999, 1e-5, c.max_grad_norm)
gap_p = float(((p_after.double() - p64).abs() / (1.2e-7 * p64.abs() + 4e-5 * c.learning_rate)).max())
norm64 = float(torch.linalg.vector_norm(g_mean))
gap_n = abs(float(ppo.opt.grad_norm) - norm64) / (1e-5 * norm64)
print(f"rank {{rank}}: one minibatch on two ranks: gap / bound: parameters {{gap_p:.3f}}, grad_norm {{gap_n:.3f}} "
      f"(norm {{float(ppo.opt.grad_norm)!r}}, fp64 {{norm64!r}}, clip coefficient {{float(ppo.opt.clip_coef)!r}})", flush=True)
check(gap_p <= 1.0, f"(d) parameters miss the fp64 step on the mean gradient: {{gap_p}} of the bound")
check(gap_n <= 1.0, f"(d) grad_norm {{float(ppo.opt.grad_norm)!r}} is not the mean gradient's {{norm64!r}}: {{gap_n}} of the bound")
saved.update(c1_before=p_before, c1_after=p_after, c1_state=s_after, c1_grad=g_mine)
env.close()

# ------------------------------------------------------------------------------------------------ C2: update() end to end
for tag, fused_optimizer in (("packed", True), ("torch", False)):
    env, ppo = make(10 * (1 + fused_optimizer) + rank, fused_optimizer)
    init = pack_policy(ppo.policy).clone()
    dicts = []
    for _ in range(2):
        ppo.collect()
        dicts.append(ppo.update())
    torch.cuda.synchronize()
    packed = pack_policy(ppo.policy).clone()
    check(bool(torch.isfinite(packed).all()) and not torch.equal(packed, init), f"{{tag}}: the weights are not finite or did not move")
    keys = {{"pg_loss", "v_loss", "entropy", "clip_frac", "explained_variance"}} | ({{"grad_norm"}} if fused_optimizer else set())
    for u in dicts:
        check(set(u) == keys, f"{{tag}}: update() returned {{sorted(u)}}, not {{sorted(keys)}}")
        check(all(math.isfinite(v) for v in u.values()), f"{{tag}}: update() returned a value that is not finite: {{u}}")
    if fused_optimizer:
        check(int(ppo.opt.step_count) == 2 * (n_steps * n_local // batch), f"{{tag}}: step_count {{int(ppo.opt.step_count)}}")
        check(ppo.fused_grad.bound and _packed_order(ppo.policy)[0].data_ptr() == ppo.fused_grad.params.data_ptr(),
              f"{{tag}}: the module's parameters no longer alias the packed buffer")
        check(torch.equal(bits(packed), bits(ppo.fused_grad.params)), f"{{tag}}: the module and the packed buffer hold different weights")
        saved[f"{{tag}}_state"] = ppo.opt.state.clone()
    else:
        check(isinstance(ppo.opt, torch.optim.Adam) and not ppo.fused_grad.bound, f"{{tag}}: not the torch optimiser")
    print(f"rank {{rank}}: {{tag}}: {{dicts[-1]}}", flush=True)
    saved[f"{{tag}}_init"], saved[f"{{tag}}_final"] = init, packed
    env.close()

np.savez(os.path.join(out_dir, f"rank{{rank}}.npz"), **{{k: v.cpu().numpy() for k, v in saved.items()}})
dist.barrier()
dist.destroy_process_group()
if fails:
    sys.exit(f"rank {{rank}}: {{len(fails)}} check(s) failed: " + "; ".join(fails))
"""


def test_fused_learner_on_two_ranks(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, n_local=N_LOCAL, n_steps=N_STEPS, batch=BATCH, out_dir=str(tmp_path)))
    out = _launch(2, [str(script)], {}, 300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stderr[-3000:]
    a, b = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    bits = lambda x: x.view(np.int32)
    assert set(a.files) == set(b.files) == {"c1_before", "c1_after", "c1_state", "c1_grad", "packed_init", "packed_final", "packed_state",
                                            "torch_init", "torch_final"}
    # (a) the seeds differ, the replicas do not: before the step by rank 0's broadcast, after it by the all-reduce
    for key in ("c1_before", "c1_after", "c1_state", "packed_init", "packed_final", "packed_state", "torch_init", "torch_final"):
        assert np.array_equal(bits(a[key]), bits(b[key])), f"{key} differs between the ranks in {int((bits(a[key]) != bits(b[key])).sum())} words"
        assert np.isfinite(a[key]).all(), key
    # (b) the ranks saw different rollouts
    assert not np.array_equal(a["c1_grad"], b["c1_grad"])
    for tag in ("packed", "torch"):
        assert not np.array_equal(a[f"{tag}_init"], a[f"{tag}_final"])
    assert not np.array_equal(a["c1_before"], a["packed_init"])      # another PPO, another seed: rank 0's own draw each time
