"""The fp64 statement of one te_policy_adam_step (clip_grad_norm_, then torch's non-fused Adam without weight decay or amsgrad), shared
by tests/test_policy_opt.py and the two-rank worker of tests/test_gpu_ppo_two_ranks.py."""
import math


def ref64_step(torch, p, m, v, g, k, lr, b1, b2, eps, max_norm):
    """Step k (from 1) on fp64 p, m, v with the gradient g (any float type: taken to fp64 as it is); returns the new (p, m, v)."""
    g = g.double()
    coef = min(1.0, max_norm / (float(torch.linalg.vector_norm(g)) + 1e-6))
    g = coef * g
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** k)) * m / (v.sqrt() / math.sqrt(1 - b2 ** k) + eps)
    return p, m, v
