"""te_policy_ppo_grad_bf16 (dronechase_amd/csrc/te_policy_grad_bf16.hpp): the fused PPO gradient with bf16 operands on the bf16 MFMA, for
the three served shapes x lidar_channels 2 and 3, and the layers above it (te_policy_bf16_grad_words, te_policy_pack_bf16_grad,
te_policy_grad_bf16_workspace_bytes, FusedPolicy(grad_precision="bf16"), PPOConfig.fused_update_bf16).

The reference is tests/_policy_grad_bf16_ref.py: the numerics contract of include/threatengage.h as PyTorch autograd on the CPU,
evaluated in fp64 (E64) and in fp32 (E32).  The bound is the flip model.  Any two correct implementations differ by summation order and
by the rare value that lands on the other side of a bf16 rounding boundary; one such flip changes one row's contribution to an element
by about 2^-8 of it.  So for tensor t, R_t = the largest |contribution of one row to one element| (from E64, one row at a time, the
advantage normalisation fixed), and
  * the pair: max |E64 - E32|_t <= 2 x 2^-8 R_t on the fixed inputs below, asserted without a GPU (measured on these inputs: at most 0.53);
  * the kernel: max |kernel - E64|_t <= 6 x 2^-8 R_t for every tensor, log_std included: three times the pair's cap, the convention
    of test_policy_bf16.py, because the kernel's summation order differs from both references;
  * pg and vl within 6 x 2^-8 x (largest per-row term) / B of E64's; ent and clip_frac within 1e-6 (every ratio lies well away from
    the clip thresholds: _kinkfree.LOGP_SHIFTS).
Every measured ratio is printed; TE_POLICY_GRAD_BF16_RECORD=<path> appends each as a JSON line (profiles/policy_grad_bf16.json).

Measured on the MI355X: the kernel's largest ratio over the ten parity cases was 1.39 (learn C=3, action.2.weight: one flip the pair does not
share; the pair's own 0.30 there), below 0.53 in every other case and below 1e-3 where no value flipped; pg and vl at most 0.003 of their
unit, ent 5.5e-8 and clip_frac at most 4.9e-9 from E64's."""
import copy
import ctypes as C
import json
import os

import pytest

from _kinkfree import CLIP, ENT_COEF, SHAPES, VF_COEF, packed_names
from _policy_cases import StubEnv, _gpu, _shape

DEFAULT, BO, LEARN = SHAPES["default"], SHAPES["BO"], SHAPES["learn"]
INSTANCES = [(name, c) for name in SHAPES for c in (2, 3)]
PARITY = [(name, c, 64) for name, c in INSTANCES] + [(name, 3, b) for name in ("default", "BO") for b in (1, 49)]


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _ref():
    import _policy_grad_bf16_ref as R
    return R


def _record(rec):
    print("\n" + json.dumps(rec))
    if os.environ.get("TE_POLICY_GRAD_BF16_RECORD"):
        with open(os.environ["TE_POLICY_GRAD_BF16_RECORD"], "a") as f:
            f.write(json.dumps(rec) + "\n")


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_the_reference_pair_agrees(lib):
    """The condition the kernel's bound rests on: E64 and E32 within 2 x 2^-8 R_t for every tensor of every parity case."""
    R = _ref()
    assert hasattr(lib, "te_policy_ppo_grad_bf16")      # the call these references are the contract of
    for name, c, b in PARITY:
        ref = R.case(name, c, 0, b)
        pair = R.ratios(ref["e32"], ref)
        print(f"\n{name} C={c} B={b}: max |E64 - E32|_t / (2^-8 R_t) = {max(pair):.3f}")
        assert max(pair) <= R.PAIR_CAP, (name, c, b, dict(zip(packed_names(ref["policy"]), pair)))
        assert all(r > 0.0 for r in ref["R"]), (name, c, b)
        gap = (ref["stats64"] - ref["stats32"]).abs()
        assert float(gap[0]) <= R.PAIR_CAP * R.U * ref["pg_term"] / b and float(gap[1]) <= R.PAIR_CAP * R.U * ref["vl_term"] / b
        assert float(gap[2:].max()) <= 1e-6


def test_the_bound_bites(lib):
    """E64 without the row that contributes most to a tensor is outside the kernel's bound for that tensor, in every instance."""
    R = _ref()
    assert hasattr(lib, "te_policy_ppo_grad_bf16")
    for name, c in INSTANCES:
        ref = R.case(name, c, 0, 64)
        broken = 0
        for t, row in enumerate(ref["worst_row"]):
            dropped = [g - r for g, r in zip(ref["e64"], ref["rows"][row])]
            broken += R.ratios(dropped, ref)[t] > R.KERNEL_CAP
        assert broken >= 1, (name, c)


def test_calls_reject_bad_arguments(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 20          # never dereferenced: every call below fails its argument check first
    bo = _shape(3, *BO)
    need = C.c_size_t()
    assert lib.te_policy_grad_bf16_workspace_bytes(C.byref(bo), 8, C.byref(need)) == 0
    base = dict(params=fake, weights=fake, weights_t=fake, shape=C.byref(bo), n=8, index=None, lidar=fake, inertial=fake, last_action=fake,
                action=fake, old_logp=fake, adv=fake, ret=fake, ms=None, clip=C.c_float(0.2), vf=C.c_float(0.5), ent=C.c_float(0.0), grad=fake,
                stats=fake, ws=fake, ws_bytes=need.value, stream=None)
    args = lambda **kw: list({**base, **kw}.values())
    unserved = [(_shape(3, 300, (64, 64)), b"features_dim"), (_shape(3, 512, (128, 256)), b"hidden"), (_shape(4, *BO), b"lidar_channels"),
                (_shape(3, 256, (64, 64, 64, 64)), b"n_hidden")]
    cases = [(dict(n=0), b"n must be positive"), (dict(n=-3), b"n must be positive"), (dict(shape=None), b"null shape"),
             (dict(params=None), b"null"), (dict(weights=None), b"null"), (dict(weights_t=None), b"null"), (dict(grad=None), b"null"),
             (dict(stats=None), b"null"), (dict(ws=None), b"null"), (dict(ret=None), b"null"),
             (dict(params=fake + 4), b"params must be 16-byte"), (dict(weights=fake + 2), b"weights_bf16 must be 16-byte"),
             (dict(weights_t=fake + 8), b"weights_bf16_t must be 16-byte"), (dict(grad=fake + 4), b"grad must be 16-byte"),
             (dict(lidar=fake + 4), b"lidar must be 8-byte"), (dict(ws=fake + 128), b"workspace must be 256-byte"), (dict(index=fake + 4), b"index must be 8-byte"),
             (dict(adv=fake + 2), b"4-byte"), (dict(ws_bytes=need.value - 1), b"workspace too small"), (dict(clip=C.c_float(-0.1)), b"clip_range")]
    cases += [(dict(shape=C.byref(s)), field) for s, field in unserved]
    for kw, msg in cases:
        assert lib.te_policy_ppo_grad_bf16(*args(**kw)) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_ppo_grad_bf16"), (kw, err)
    assert b"te_policy_grad_bf16_workspace_bytes says " + str(need.value).encode() in _err(lib, lib.te_policy_ppo_grad_bf16(*args(ws_bytes=16)))
    words = C.c_size_t()
    for s, field in unserved:
        for rc in (lib.te_policy_bf16_grad_words(C.byref(s), C.byref(words)), lib.te_policy_pack_bf16_grad(fake, C.byref(s), fake, None),
                   lib.te_policy_grad_bf16_workspace_bytes(C.byref(s), 8, C.byref(words))):
            msg = lib.te_last_error()
            assert rc != 0 and field in msg and b"128, 256, 512" in msg and b"512, 128, 256" in msg and b"64, 64" in msg, msg
    for kw, msg in ((dict(params=None), b"null"), (dict(out=None), b"null"), (dict(params=fake + 4), b"params must be 16-byte"),
                    (dict(out=fake + 2), b"out must be 16-byte"), (dict(shape=None), b"null shape")):
        a = dict(params=fake, shape=C.byref(bo), out=fake, stream=None)
        a.update(kw)
        assert lib.te_policy_pack_bf16_grad(*a.values()) != 0, kw
        err = lib.te_last_error()
        assert msg in err and err.startswith(b"te_policy_pack_bf16_grad"), (kw, err)
    assert lib.te_policy_bf16_grad_words(C.byref(bo), None) != 0 and b"null" in lib.te_last_error()
    assert lib.te_policy_grad_bf16_workspace_bytes(C.byref(bo), 8, None) != 0 and b"null" in lib.te_last_error()
    for n in (0, -1, (1 << 27) + 1):
        assert lib.te_policy_grad_bf16_workspace_bytes(C.byref(bo), n, C.byref(words)) != 0
        assert lib.te_last_error().startswith(b"te_policy_grad_bf16_workspace_bytes: n must be")


def _err(lib, rc):
    assert rc != 0
    return lib.te_last_error()


def _kp(k):
    return (k + 31) // 32 * 32


def test_transposed_words_and_workspace_size(lib):
    for name, c in INSTANCES:
        f, arch = SHAPES[name]
        widths = (f,) + arch
        # W^T [K][roundup(N, 32)] of conv2, inertial.2 / .4, action.2 / .4, final.0 and both heads' hidden layers
        by_hand = 128 * _kp(64) + 4 * 128 * _kp(128) + 448 * _kp(f) + 2 * sum(a * _kp(b) for a, b in zip(widths, widths[1:]))
        out = C.c_size_t()
        assert lib.te_policy_bf16_grad_words(C.byref(_shape(c, f, arch)), C.byref(out)) == 0, lib.te_last_error()
        assert out.value == by_hand, (name, c)
        last, bf16, fp32 = 0, C.c_size_t(), C.c_size_t()
        for n in (1, 31, 32, 33, 64, 2048, 2049, 8192, 65536):
            assert lib.te_policy_grad_bf16_workspace_bytes(C.byref(_shape(c, f, arch)), n, C.byref(bf16)) == 0, lib.te_last_error()
            assert bf16.value >= last and bf16.value % 256 == 0, (name, c, n)
            last = bf16.value
        assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(_shape(c, f, arch)), 65536, C.byref(fp32)) == 0
        print(f"\n{name} C={c}: workspace at 65 536 rows {bf16.value / 65536:.0f} B per row (fp32 call: {fp32.value / 65536:.0f})")
        assert bf16.value < fp32.value, (name, c)


def test_switches_need_their_base(lib):
    from dronechase_amd.ppo import FusedPolicy, LidarInertialActionPolicy, PPOConfig
    assert PPOConfig().fused_update_bf16 is False
    assert PPOConfig(fused_update=True, fused_update_bf16=True).fused_update_bf16
    assert PPOConfig(fused_update=True, fused_update_bf16=True, fused_optimizer=True, fused_advantages=True).fused_forward_bf16 is False
    with pytest.raises(ValueError, match="fused_update_bf16.*needs fused_update"):
        PPOConfig(fused_update_bf16=True)
    with pytest.raises(ValueError, match="fused_update_bf16.*needs fused_update"):
        PPOConfig(fused_forward=True, fused_forward_bf16=True, fused_update_bf16=True)
    with pytest.raises(ValueError, match="grad_precision"):
        FusedPolicy(LidarInertialActionPolicy(), grad_precision="fp16")


def test_ppo_refuses_the_switch_set_after_the_config_check(lib):
    from dronechase_amd.ppo import PPO, PPOConfig
    cfg = PPOConfig(n_steps=2)
    cfg.fused_update_bf16 = True
    with pytest.raises(ValueError, match="fused_update_bf16.*needs fused_update"):
        PPO(StubEnv(), cfg)
    # the wide shapes: the same rule as the fp32 call's
    with pytest.raises(ValueError, match="fused_update_wide"):
        PPO(StubEnv(), PPOConfig(n_steps=2, fused_update=True, fused_update_bf16=True, features_dim=BO[0], net_arch=BO[1]))


# ---------------------------------------------------------------------------------------------------------- MI355X
def _dev(d):
    return {k: v.to("cuda:0").contiguous() for k, v in d.items()}


def _fused(policy, precision="fp32"):
    from dronechase_amd.ppo import FusedPolicy
    return FusedPolicy(copy.deepcopy(policy).to("cuda:0"), precision=precision, grad_precision="bf16")


def _kernel(torch, fused, obs, ro, index, ms):
    """(packed gradient, stats) of one te_policy_ppo_grad_bf16 call; both start as NaN."""
    grad = torch.full_like(fused.params, float("nan"))
    stats = torch.full((4,), float("nan"), device="cuda:0")
    fused.ppo_grad(obs, index, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, CLIP, VF_COEF, ENT_COEF, grad, stats)
    torch.cuda.synchronize()
    return grad, stats


def _split(policy, grad):
    """The packed gradient as {parameter name: tensor}."""
    from dronechase_amd.ppo import _packed_order
    out, off = {}, 0
    for name, p in zip(packed_names(policy), _packed_order(policy)):
        out[name] = grad[off:off + p.numel()].view_as(p)
        off += p.numel()
    assert off == grad.numel()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,c,b", PARITY)
def test_parity_with_the_reference(name, c, b):
    torch = _gpu()
    R = _ref()
    ref = R.case(name, c, 0, b)
    fused = _fused(ref["policy"])
    grad, stats = _kernel(torch, fused, _dev(ref["obs"]), _dev(ref["ro"]), ref["index"].to("cuda:0"), ref["ms"].to("cuda:0"))
    names = packed_names(ref["policy"])
    got = list(_split(ref["policy"], grad.cpu()).values())
    kernel, pair = R.ratios(got, ref), R.ratios(ref["e32"], ref)
    gap = (stats.cpu().double() - ref["stats64"]).abs()
    rec = {"case": f"{name} C={c} B={b}", "kernel_max_ratio": max(kernel), "kernel_worst_tensor": names[kernel.index(max(kernel))],
           "pair_max_ratio": max(pair), "pg_ratio": float(gap[0]) / (R.U * ref["pg_term"] / b), "vl_ratio": float(gap[1]) / (R.U * ref["vl_term"] / b),
           "ent_gap": float(gap[2]), "clip_frac_gap": float(gap[3]), "clip_frac": float(stats[3]),
           "per_tensor": {n: round(k, 4) for n, k in zip(names, kernel)}}
    _record(rec)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all())
    assert max(kernel) <= R.KERNEL_CAP, rec
    assert rec["pg_ratio"] <= R.KERNEL_CAP and rec["vl_ratio"] <= R.KERNEL_CAP, rec
    assert rec["ent_gap"] <= 1e-6 and rec["clip_frac_gap"] <= 1e-6, rec
    if b > 1:
        assert 0.0 < rec["clip_frac"] < 1.0, rec       # both clip branches were taken


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("default", 3), ("learn", 2)])
def test_the_forward_is_the_bf16_inference(name, c):
    """With ret := the value te_policy_act_bf16 returns, the value loss and its gradients are exactly 0; with action := its mu, the
    policy head's are; with both only log_std has a gradient.  Anything but a bitwise equal forward leaves a non-zero."""
    torch = _gpu()
    R = _ref()
    policy = R.make_policy(name, c, 9)
    obs, ro, ms = R.make_rollout(policy, c, 200, 17)
    obs, ro, ms = _dev(obs), _dev(ro), ms.to("cuda:0")
    index = torch.randperm(200, generator=torch.Generator().manual_seed(4))[:49].to("cuda:0")
    fused = _fused(policy, precision="bf16")
    mu, value = fused.forward(obs)
    act_is_mu, ret_is_v = dict(ro, action=mu.contiguous()), dict(ro, ret=value.contiguous())
    groups = lambda g: ({k: v for k, v in g.items() if k.startswith(("vf.", "value."))}, {k: v for k, v in g.items() if k.startswith(("pi.", "mu."))})
    zero = lambda d: all(bool((v == 0).all()) for v in d.values())

    grad, stats = _kernel(torch, fused, obs, ret_is_v, index, ms)
    vf, pi = groups(_split(policy, grad))
    assert float(stats[1]) == 0.0 and zero(vf) and not zero(pi) and len(vf) == 2 * len(SHAPES[name][1]) + 2

    grad, stats = _kernel(torch, fused, obs, act_is_mu, index, ms)
    vf, pi = groups(_split(policy, grad))
    assert zero(pi) and not zero(vf) and float(stats[1]) > 0.0

    grad, stats = _kernel(torch, fused, obs, dict(act_is_mu, ret=value.contiguous()), index, ms)
    g = _split(policy, grad)
    assert zero({k: v for k, v in g.items() if k != "log_std"}) and bool((g["log_std"] != 0).all()) and float(stats[1]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_poisoned_workspace_changes_nothing(lib, name):
    """Rows past n contribute exactly 0 whatever the workspace held: on a workspace of NaNs the result is finite and bitwise the one
    on a workspace of zeros."""
    torch = _gpu()
    R = _ref()
    policy = R.make_policy(name, 3, 31)
    fused = _fused(policy)
    obs, ro, ms = R.make_rollout(policy, 3, 65, 31)
    obs, ro, ms = _dev(obs), _dev(ro), ms.to("cuda:0")
    need = C.c_size_t()
    for b in (1, 17, 33, 49, 65):
        assert lib.te_policy_grad_bf16_workspace_bytes(C.byref(fused.shape), b, C.byref(need)) == 0
        o, r = {k: v[:b].contiguous() for k, v in obs.items()}, {k: v[:b].contiguous() for k, v in ro.items()}
        out = []
        for fill in (0xFF, 0x00):
            ws = fused._grad_ws = torch.full((need.value,), fill, dtype=torch.uint8, device="cuda:0")
            if fill:
                assert bool(torch.isnan(ws.view(torch.bfloat16).float()).all())
            out.append(_kernel(torch, fused, o, r, None, ms))
            assert fused._grad_ws is ws                       # exactly the required size: the call did not replace it
        (g1, s1), (g0, s0) = out
        assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(s1).all()), (name, b)
        assert torch.equal(g1, g0) and torch.equal(s1, s0), (name, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("default", 2), ("BO", 3)])
def test_calls_are_deterministic_and_index_is_a_gather(name, c):
    torch = _gpu()
    R = _ref()
    policy = R.make_policy(name, c, 21)
    fused = _fused(policy)
    obs, ro, ms = R.make_rollout(policy, c, 300, 21)
    obs, ro, ms = _dev(obs), _dev(ro), ms.to("cuda:0")
    idx = torch.randint(0, 300, (209,), device="cuda:0")      # duplicates allowed; 6 full tiles and 17 rows
    g1, s1 = _kernel(torch, fused, obs, ro, idx, ms)
    g2, s2 = _kernel(torch, fused, {k: v[idx].contiguous() for k, v in obs.items()}, {k: v[idx].contiguous() for k, v in ro.items()}, None, ms)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    _kernel(torch, fused, obs, ro, None, ms)                  # a call of another size (which grows the workspace) in between
    g3, s3 = _kernel(torch, fused, obs, ro, idx, ms)
    assert torch.equal(g1, g3) and torch.equal(s1, s3) and bool((g1 != 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("default", 3), ("learn", 3)])
def test_two_split_k_slices_are_the_two_halves(name, c):
    """4 096 = 2 x 2 048 rows with an explicit adv_mean_std against the two halves called on their own.  The factor 2 in 1 / B commutes
    with every rounding, so only the association of the fp32 partial sums differs (the conv layers' slices group other rows)."""
    torch = _gpu()
    R = _ref()
    policy = R.make_policy(name, c, 41)
    fused = _fused(policy)
    obs, ro, ms = R.make_rollout(policy, c, 4096, 41)
    obs, ro, ms = _dev(obs), _dev(ro), ms.to("cuda:0")
    half = lambda lo: ({k: v[lo:lo + 2048].contiguous() for k, v in obs.items()}, {k: v[lo:lo + 2048].contiguous() for k, v in ro.items()})
    gf, sf = _kernel(torch, fused, obs, ro, None, ms)
    (ga, sa), (gb, sb) = (_kernel(torch, fused, *half(lo), None, ms) for lo in (0, 2048))
    worst = 0.0
    for (n, f), a, b in zip(_split(policy, gf).items(), _split(policy, ga).values(), _split(policy, gb).values()):
        gap, scale = float((f - (a + b) / 2).abs().max()), max(float(a.abs().max()), float(b.abs().max()))
        worst = max(worst, gap / scale)
        assert gap <= 1e-4 * scale, (n, gap, scale)
    print(f"\n{name} C={c}: largest |g_full - (g_a + g_b) / 2| / max(|g_a|, |g_b|) over the tensors: {worst:.2e}")
    mean = (sa + sb) / 2
    assert bool(((sf - mean).abs() <= 1e-6 * mean.abs()).all()), (sf.tolist(), mean.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("default", 3), ("BO", 2), ("learn", 3)])
def test_pack_is_the_transposed_rounded_weights_at_the_documented_offsets(name, c):
    torch = _gpu()
    import torch.nn as nn
    policy = _ref().make_policy(name, c, 5)
    fused = _fused(policy)
    torch.cuda.synchronize()
    buf = fused.weights_bf16_t.cpu()
    assert buf.dtype == torch.int16 and fused.weights_bf16_t.data_ptr() % 16 == 0 and fused.weights_bf16.data_ptr() % 16 == 0
    off = 0
    skipped = (policy.lidar[0], policy.inertial[0], policy.action[0])      # their inputs need no gradient
    for seq in (policy.lidar, policy.inertial, policy.action, policy.final, policy.pi, policy.vf):
        for m in seq:
            if not isinstance(m, (nn.Conv2d, nn.Linear)) or any(m is s for s in skipped):
                continue
            w = m.weight.detach().reshape(m.weight.shape[0], -1)
            n, k = w.shape
            block = buf[off:off + k * _kp(n)].view(k, _kp(n))
            assert off * 2 % 64 == 0
            assert torch.equal(block[:, :n], w.t().contiguous().bfloat16().view(torch.int16)), (name, m)
            assert bool((block[:, n:] == 0).all()), (name, m)
            off += k * _kp(n)
    assert off == buf.numel()


@pytest.mark.gpu
def test_graph_capture_and_replay():
    torch = _gpu()
    R = _ref()
    policy = R.make_policy("BO", 3, 27)
    fused = _fused(policy)
    obs, ro, ms = R.make_rollout(policy, 3, 33, 27)
    obs, ro, ms = _dev(obs), _dev(ro), ms.to("cuda:0")
    eager, eager_s = _kernel(torch, fused, obs, ro, None, ms)       # also sizes the workspace outside the capture
    grad, stats = torch.zeros_like(fused.params), torch.zeros(4, device="cuda:0")
    call = lambda: fused.ppo_grad(obs, None, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, CLIP, VF_COEF, ENT_COEF, grad, stats)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(grad, eager) and torch.equal(stats, eager_s)
    with torch.no_grad():
        for p in fused.policy.parameters():
            p.add_(0.01 * torch.randn_like(p))
    fused.refresh()                                                  # repacks all three buffers in place
    g.replay(); torch.cuda.synchronize()
    again, again_s = _kernel(torch, fused, obs, ro, None, ms)
    assert torch.equal(grad, again) and torch.equal(stats, again_s) and not torch.equal(grad, eager)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,fused_optimizer,bf16_forward", [("default", False, False), ("default", True, True), ("BO", True, False)])
def test_ppo_update_runs_the_bf16_gradient(shape, fused_optimizer, bf16_forward):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, FusedPolicy, PPOConfig
    f, arch = SHAPES[shape]
    env = BatchedEnv(default_config("stage03", n_envs=64, max_step=40), "cuda:0")
    ppo = PPO(env, PPOConfig(n_steps=4, batch_size=256, n_epochs=1, use_graph=False, features_dim=f, net_arch=arch, fused_update=True,
                             fused_update_wide=shape != "default", fused_update_bf16=True, fused_optimizer=fused_optimizer,
                             fused_forward=bf16_forward, fused_forward_bf16=bf16_forward), seed=4)
    fg = ppo.fused_grad
    assert fg.grad_precision == "bf16" and fg.precision == ("bf16" if bf16_forward else "fp32") and fg.weights_bf16_t is not None
    assert (ppo.fused is fg) == bf16_forward
    ppo.collect()
    before = copy.deepcopy(ppo.policy)          # a bound module's copy gets storage of its own
    seen = []
    inner = fg.ppo_grad

    def spy(obs, idx, actions, old_logp, adv, ret, ms, *rest):
        inner(obs, idx, actions, old_logp, adv, ret, ms, *rest)
        grad, stats = rest[-2], rest[-1]
        direct = FusedPolicy(before, grad_precision="bf16")
        g2, s2 = torch.full_like(grad, float("nan")), torch.full_like(stats, float("nan"))
        direct.ppo_grad(obs, idx, actions, old_logp, adv, ret, ms, *rest[:-2], g2, s2)
        seen.append((grad.clone(), stats.clone(), g2, s2))

    fg.ppo_grad = spy
    log = ppo.update()
    assert len(seen) == 1
    grad, stats, g2, s2 = seen[0]
    assert torch.equal(grad, g2) and torch.equal(stats, s2) and bool(torch.isfinite(grad).all()) and bool((grad != 0).any())
    assert all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert any(not torch.equal(a.detach(), b.detach()) for a, b in zip(before.parameters(), ppo.policy.parameters()))
    if bf16_forward:        # old_logp came from the same forward: no ratio is anywhere near the clip range before the first step
        assert float(stats[3]) == 0.0 and log["clip_frac"] == 0.0
    env.close()
