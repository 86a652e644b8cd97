"""te_rollout_gae and te_adv_stats (dronechase_amd/csrc/te_rollout.hpp) and the layers above them (RolloutBuffer.finish(fused=True),
ppo.adv_stats, PPOConfig.fused_advantages).

GAE is held bitwise to RolloutBuffer.finish: the kernel does the same fp32 operations in the same order, none of them fused.
The statistics are held to fp64 numpy on the same fp32 inputs:
  |mean - m64| <= 6e-8 |m64| + 1e-12 max|x|        (one fp32 rounding of the stored mean; the fp64 sums are far below the second term)
  |std  - s64| <= 1.2e-7 s64                        (one fp32 rounding, doubled for the square root)
Both bounds are held on all three input sets, normals shifted by 0, 1 and 100 (SHIFTS).  torch.mean / torch.std in fp32 on the same
inputs must pass twice these bounds (else the inputs are at fault, not the kernel); that clause is asserted on the set an fp32
reduction can be held to it, shift = 1, where both sums are well conditioned (sum|x| / |sum x| and mean / std are about 1).  At
shift = 0 the mean's condition number is about sqrt(n) and the relative bound on it is out of an fp32 sum's reach; at shift = 100
every x - mean carries the fp32 rounding of a number near 100 (4e-6 absolute against a std of 1), so an fp32 std is good to about
1e-6, not 2.4e-7.  Measured on the MI355X, as fractions of the (single) bounds: te_adv_stats at most 0.83 (mean) and 0.43 (std)
over every size and set; torch fp32 at most 1.93 and 0.85 at shift = 1, but 36 (mean, shift 0, n = 65) and 7.8 (std, shift 100,
n = 64), which is what the fp64 sums and the shifted set are there for.  The gaps of both are printed for every case (pytest -s).
Past 256 slices (LOOP_SIZES, test_stats_past_256_slices: the sizes at which the final kernel's threads take more than one partial
each, as they do at the workload's 2 048 slices) the same bounds hold on a trend plus noise, torch's fp32 sums held to nothing:
measured at most 0.86 (mean) and 0.40 (std)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 4096                     # kStatSlice: the elements one workgroup owns
GAE_SHAPES = ((1, 1), (7, 5), (3, 64), (5, 65), (128, 257))
STAT_SIZES = (1, 2, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 300000)
# adv_stats_final_kernel's 256 threads each take partials t, t + 256, ...: 256 slices is the last size with one trip, at 257 thread 0
# alone takes a second partial (of a one-element slice), at 514 every thread takes two trips or three and the last slice is ragged
LOOP_SIZES = (256 * SLICE, 256 * SLICE + 1, 513 * SLICE + 5)
GAMMA, LAM = 0.99, 0.95
SHIFTS = (0.0, 1.0, 100.0)
TORCH_SHIFT = 1.0                # the set torch's fp32 reductions are held to twice the bounds on (module docstring)


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _ws_bytes(lib, n):
    out = C.c_size_t()
    assert lib.te_adv_stats_workspace_bytes(n, C.byref(out)) == 0, lib.te_last_error()
    return out.value


# ---------------------------------------------------------------------------------------------------------- no GPU needed
def test_symbols_declared_and_exported(lib):
    from dronechase_amd import _lib
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "threatengage.h")).read(), flags=re.S)
    for name in ("te_rollout_gae", "te_adv_stats_workspace_bytes", "te_adv_stats"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None


def test_workspace_bytes(lib):
    sizes = (1, 2, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3, 300000, *LOOP_SIZES, 128 * 65536, 1 << 31, 1 << 40)
    got = [_ws_bytes(lib, n) for n in sizes]
    assert [_ws_bytes(lib, n) for n in LOOP_SIZES] == [16 * 256, 16 * 257, 16 * 514]
    assert all(a <= b for a, b in zip(got, got[1:])), got
    for n, b in zip(sizes, got):
        assert b % 16 == 0 and b == 16 * ((n + SLICE - 1) // SLICE), (n, b)      # the documented size: two fp64 partials per slice
    out = C.c_size_t()
    assert lib.te_adv_stats_workspace_bytes(0, C.byref(out)) != 0 and b"n must be positive" in lib.te_last_error()
    assert lib.te_adv_stats_workspace_bytes(-3, C.byref(out)) != 0 and b"n must be positive" in lib.te_last_error()
    assert lib.te_adv_stats_workspace_bytes((1 << 40) + 1, C.byref(out)) != 0 and b"at most 2^40" in lib.te_last_error()
    assert lib.te_adv_stats_workspace_bytes(8, None) != 0 and b"null" in lib.te_last_error()


def test_bad_arguments_fail_through_last_error(lib):
    """Rejected before anything touches a device (so these run without a GPU)."""
    fake = 1 << 30          # never dereferenced: every call below fails its argument check first
    mb = 1 << 20            # the fake arrays lie 1 MB apart: a 10 x 100 rollout's do not overlap
    inf, nan = float("inf"), float("nan")
    base = dict(n_steps=10, n_envs=100, rewards=fake, values=fake + mb, dones=fake + 2 * mb, last_value=fake + 3 * mb, gamma=GAMMA,
                lam=LAM, adv=fake + 4 * mb, ret=fake + 5 * mb, stream=None)
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]
    cases = [(dict(rewards=None), b"null"), (dict(values=None), b"null"), (dict(dones=None), b"null"), (dict(last_value=None), b"null"),
             (dict(adv=None), b"null"), (dict(ret=None), b"null"),
             (dict(n_steps=0), b"n_steps must be positive"), (dict(n_steps=-1), b"n_steps must be positive"),
             (dict(n_envs=0), b"n_envs must be positive"), (dict(n_envs=-7), b"n_envs must be positive"),
             (dict(n_steps=1 << 15, n_envs=1 << 16), b"at most 2^31 - 1"), (dict(n_steps=2, n_envs=1 << 30), b"at most 2^31 - 1"),
             (dict(gamma=-0.1), b"gamma must be in [0, 1]"), (dict(gamma=1.0001), b"gamma must be in [0, 1]"),
             (dict(gamma=nan), b"gamma must be in [0, 1]"), (dict(gamma=inf), b"gamma must be in [0, 1]"),
             (dict(lam=-0.1), b"gae_lambda must be in [0, 1]"), (dict(lam=1.5), b"gae_lambda must be in [0, 1]"),
             (dict(lam=nan), b"gae_lambda must be in [0, 1]"), (dict(lam=-inf), b"gae_lambda must be in [0, 1]"),
             (dict(values=fake + mb + 2), b"4-byte aligned"), (dict(ret=fake + 5 * mb + 1), b"4-byte aligned"),
             (dict(adv=fake), b"must not alias the inputs"), (dict(ret=fake + 2 * mb + 3996), b"must not alias the inputs"),
             (dict(adv=fake + 3 * mb + 396), b"must not alias the inputs"), (dict(ret=fake + 4 * mb + 3996), b"must not alias each other")]
    for kw, msg in cases:
        assert lib.te_rollout_gae(*args(**kw)) != 0, kw
        assert msg in lib.te_last_error(), (kw, lib.te_last_error())

    need = _ws_bytes(lib, 10000)
    base = dict(x=fake, index=fake + mb, n=10000, out=fake + 2 * mb, workspace=fake + 3 * mb, workspace_bytes=need, stream=None)
    cases = [(dict(x=None), b"null"), (dict(out=None), b"null"), (dict(workspace=None), b"null"),
             (dict(n=0), b"n must be positive"), (dict(n=-1), b"n must be positive"), (dict(n=(1 << 40) + 1), b"at most 2^40"),
             (dict(workspace_bytes=need - 1), b"workspace too small"), (dict(workspace_bytes=0), b"workspace too small"),
             (dict(n=3 * SLICE + 1), b"workspace too small"),
             (dict(x=fake + 2), b"4-byte aligned"), (dict(out=fake + 2 * mb + 1), b"4-byte aligned"),
             (dict(index=fake + mb + 4), b"index must be 8-byte aligned"), (dict(workspace=fake + 3 * mb + 4), b"workspace must be 8-byte aligned")]
    for kw, msg in cases:
        for drop_index in (False, True):        # the checks do not depend on whether there is an index
            kw2 = {**kw, "index": None} if drop_index and "index" not in kw else kw
            assert lib.te_adv_stats(*args(**kw2)) != 0, kw2
            assert msg in lib.te_last_error(), (kw2, lib.te_last_error())


def test_config_switch_needs_a_gpu():
    from dronechase_amd.ppo import PPO, PPOConfig
    from tests._policy_cases import StubEnv
    assert PPOConfig().fused_advantages is False
    cfg = PPOConfig(n_steps=2, batch_size=8, fused_advantages=True)          # does not need fused_update
    assert cfg.fused_advantages and not cfg.fused_update
    with pytest.raises(ValueError, match="fused_advantages.*needs a GPU"):
        PPO(StubEnv(None), cfg)
    ppo = PPO(StubEnv(None), PPOConfig(n_steps=2, batch_size=8))             # the same env is fine with the switch off
    assert not hasattr(ppo, "_adv_stats")


def test_fused_finish_refuses_a_cpu_buffer():
    import torch
    from dronechase_amd.ppo import RolloutBuffer
    buf = RolloutBuffer(3, 4, {}, "cpu")
    with pytest.raises(ValueError, match="te_rollout_gae"):
        buf.finish(torch.zeros(4), GAMMA, LAM, fused=True)


# ---------------------------------------------------------------------------------------------------------- MI355X
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _rollout(T, N, seed):
    """numpy-seeded rewards, values, last_value (normals) and dones (20 %; with N >= 2 env 0 never finishes and env N - 1 always does)."""
    rng = np.random.default_rng(seed)
    r, v = rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal((T, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.2).astype(np.float32)
    if N >= 2:
        d[:, 0], d[:, N - 1] = 0.0, 1.0
    return r, v, d, rng.standard_normal(N).astype(np.float32)


def _buffer(torch, T, N, data):
    from dronechase_amd.ppo import RolloutBuffer
    buf = RolloutBuffer(T, N, {}, torch.device("cuda:0"))
    r, v, d, last = data
    buf.rewards.copy_(torch.from_numpy(r)); buf.values.copy_(torch.from_numpy(v)); buf.dones.copy_(torch.from_numpy(d))
    buf.adv.fill_(float("nan")); buf.ret.fill_(float("nan"))
    return buf, torch.from_numpy(last).to("cuda:0")


def _bits(t):
    import torch
    return t.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,gamma,lam", [(T, N, GAMMA, LAM) for T, N in GAE_SHAPES] + [(7, 5, 1.0, 1.0), (7, 5, 0.0, 0.0)])
def test_gae_is_bitwise_finish(T, N, gamma, lam):
    torch = _gpu()
    data = _rollout(T, N, 1000 * T + N)
    ref, last = _buffer(torch, T, N, data)
    new, _ = _buffer(torch, T, N, data)
    ref.finish(last, gamma, lam)
    new.finish(last, gamma, lam, fused=True)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.adv).all() and torch.isfinite(ref.ret).all()
    assert torch.equal(_bits(new.adv), _bits(ref.adv)), int((_bits(new.adv) != _bits(ref.adv)).sum())
    assert torch.equal(_bits(new.ret), _bits(ref.ret)), int((_bits(new.ret) != _bits(ref.ret)).sum())
    # the inputs are untouched
    for got, want in zip((new.rewards, new.values, new.dones), data):
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    if N >= 2:
        assert torch.equal(new.adv[:, N - 1], new.rewards[:, N - 1] - new.values[:, N - 1])   # an env that always finishes: gae = delta = r - v


_STAT_INPUTS = {}


def _stat_inputs(torch, n, shift):
    """(x [n], big [m], idx [n] int64 into big with repeats) on the device, and the fp64 (mean, std, max|x|) of x and of big[idx];
    computed once per (n, shift) and never written."""
    key = (n, shift)
    if key not in _STAT_INPUTS:
        rng = np.random.default_rng(7000 + n)
        m = 2 * n + 5
        big = (shift + rng.standard_normal(m)).astype(np.float32)
        idx = rng.integers(0, m, n)
        if n >= 2:
            idx[1] = idx[0]         # at least one repeat
        x = big[:n].copy()

        def ref(a):
            a = a.astype(np.float64)
            return float(a.mean()), (float(a.std(ddof=1)) if a.size > 1 else float("nan")), float(np.abs(a).max())

        dev = lambda a: torch.from_numpy(a).to("cuda:0")
        _STAT_INPUTS[key] = (dev(x), dev(big), dev(idx.astype(np.int64)), ref(x), ref(big[idx]))
    return _STAT_INPUTS[key]


def _stats(torch, x, index, n_ws=None):
    from dronechase_amd.ppo import adv_stats, adv_stats_workspace
    n = x.numel() if index is None else index.numel()
    out = torch.full((2,), -7.0, device="cuda:0")
    adv_stats(x, index, out, adv_stats_workspace(n_ws or n, "cuda:0"))
    torch.cuda.synchronize()
    return out


def _gaps(mean, std, ref):
    """(mean gap, std gap) as fractions of the bounds in the module docstring."""
    m64, s64, amax = ref
    gm = abs(mean - m64) / (6e-8 * abs(m64) + 1e-12 * amax)
    gs = abs(std - s64) / (1.2e-7 * s64) if s64 > 0.0 else (0.0 if std == 0.0 else math.inf)
    return gm, gs


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", STAT_SIZES)
def test_stats_against_fp64(n, shift):
    torch = _gpu()
    x, big, idx, ref_x, ref_idx = _stat_inputs(torch, n, shift)
    cases = [("plain", x, None, ref_x)] + ([("indexed", big, idx, ref_idx)] if n >= 2 else [])
    for name, src, index, ref in cases:
        out = _stats(torch, src, index)
        mean, std = float(out[0]), float(out[1])
        rows = src if index is None else src[index]
        # the same call again, with a larger workspace: bitwise the same; an indexed call equals the call on the gathered rows
        assert torch.equal(_bits(out), _bits(_stats(torch, src, index, n_ws=2 * n + 7)))
        if index is not None:
            assert torch.equal(_bits(out), _bits(_stats(torch, rows.contiguous(), None)))
        if n == 1:
            assert mean == float(src[0]) and math.isnan(std)
            continue
        gm, gs = _gaps(mean, std, ref)
        tm, ts = _gaps(float(rows.mean()), float(rows.std()), ref)
        print(f"\nn={n} shift={shift:g} {name}: gap / bound: te_adv_stats mean {gm:.3f} std {gs:.3f}; torch fp32 mean {tm:.3f} std {ts:.3f}"
              f" (of twice the bound: {tm / 2:.3f}, {ts / 2:.3f})")
        if shift == TORCH_SHIFT:
            assert tm <= 2.0 and ts <= 2.0, "the inputs are wrong: torch fp32 itself misses twice the bound"
        assert gm <= 1.0 and gs <= 1.0, (name, mean, std, ref)


_TREND_INPUTS = {}


def _trend_inputs(torch, n):
    """As _stat_inputs, for the sizes past 256 slices, with a trend under the noise: x[i] = i / n + 0.1 N(0, 1) and big[j] = j / m +
    0.1 N(0, 1), m = 2 n + 5, in float32.  The slices of x then have different sums (a slice is worth about SLICE / n of the mean,
    2e-3 and more, against a bound near 3e-8), so a partial that is dropped, doubled or taken from another slice shows; the rows
    big[idx] lose the trend's order, not its spread.  Worked out in fp64 for these seeds: leaving any one slice out of the final sum,
    the one-element slice of 257 included, moves the mean or the std by at least 8 bounds (plain: 29), the first 256 partials alone
    at 514 slices by 1e6."""
    if n not in _TREND_INPUTS:
        rng = np.random.default_rng(9000 + n)
        m = 2 * n + 5
        x = (np.arange(n) / n + 0.1 * rng.standard_normal(n)).astype(np.float32)
        big = (np.arange(m) / m + 0.1 * rng.standard_normal(m)).astype(np.float32)
        idx = rng.integers(0, m, n)
        idx[1] = idx[0]             # at least one repeat

        def ref(a):
            a = a.astype(np.float64)
            return float(a.mean()), float(a.std(ddof=1)), float(np.abs(a).max())

        dev = lambda a: torch.from_numpy(a).to("cuda:0")
        _TREND_INPUTS[n] = (dev(x), dev(big), dev(idx.astype(np.int64)), ref(x), ref(big[idx]))
    return _TREND_INPUTS[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", LOOP_SIZES)
def test_stats_past_256_slices(n):
    """The second-level sum beyond one trip per thread (LOOP_SIZES), against fp64 numpy on the same fp32 elements and the bounds of the
    module docstring: the kernel sums in fp64 about a pivot and rounds once, so its error does not grow with n.  torch's fp32 sums do
    grow with n and are held to nothing here."""
    torch = _gpu()
    assert (n + SLICE - 1) // SLICE in (256, 257, 514)
    x, big, idx, ref_x, ref_idx = _trend_inputs(torch, n)
    for name, src, index, ref in (("plain", x, None, ref_x), ("indexed", big, idx, ref_idx)):
        out = _stats(torch, src, index)
        mean, std = float(out[0]), float(out[1])
        # the same call again, with a larger workspace: bitwise the same; an indexed call equals the call on the gathered rows
        assert torch.equal(_bits(out), _bits(_stats(torch, src, index, n_ws=2 * n + 7)))
        if index is not None:
            assert torch.equal(_bits(out), _bits(_stats(torch, src[index].contiguous(), None)))
        gm, gs = _gaps(mean, std, ref)
        print(f"\nn={n} ({(n + SLICE - 1) // SLICE} slices) {name}: gap / bound: te_adv_stats mean {gm:.3f} std {gs:.3f}")
        assert gm <= 1.0 and gs <= 1.0, (name, mean, std, ref)


@pytest.mark.gpu
def test_stats_of_a_constant_are_exact():
    torch = _gpu()
    x = torch.full((2 * SLICE + 3,), 0.1, device="cuda:0")
    out = _stats(torch, x, None)
    assert float(out[0]) == float(x[0]) and float(out[1]) == 0.0


@pytest.mark.gpu
def test_graph_replay_equals_eager():
    torch = _gpu()
    from dronechase_amd.ppo import adv_stats, adv_stats_workspace
    T, N = 5, 65
    sets = [_rollout(T, N, s) for s in (11, 12, 13)]
    buf, last = _buffer(torch, T, N, sets[0])
    out = torch.zeros(2, device="cuda:0")
    idx = torch.from_numpy(np.random.default_rng(5).integers(0, T * N, 200)).to("cuda:0")
    ws = adv_stats_workspace(T * N, "cuda:0")

    def run():
        buf.finish(last, GAMMA, LAM, fused=True)
        adv_stats(buf.adv.reshape(-1), idx, out, ws)

    def load(data):
        r, v, d, lv = data
        buf.rewards.copy_(torch.from_numpy(r)); buf.values.copy_(torch.from_numpy(v)); buf.dones.copy_(torch.from_numpy(d))
        last.copy_(torch.from_numpy(lv))

    eager = []
    for data in sets:
        load(data)
        run()
        torch.cuda.synchronize()
        eager.append((buf.adv.clone(), buf.ret.clone(), out.clone()))
    assert not torch.equal(eager[1][0], eager[2][0])
    load(sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (1, 2):
        load(sets[k])
        buf.adv.fill_(float("nan")); buf.ret.fill_(float("nan")); out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((buf.adv, buf.ret, out), eager[k]):
            assert torch.equal(_bits(got), _bits(want)), k


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_ppo_with_fused_advantages(use_graph):
    torch = _gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    cfg = dict(n_steps=8, batch_size=512, n_epochs=1, use_graph=use_graph, fused_update=True)      # 8 x 64 rows: one minibatch
    make_env = lambda: BatchedEnv(default_config("stage03", n_envs=64, max_step=5), "cuda:0")      # every env finishes inside the rollout
    env_a = make_env()
    a = PPO(env_a, PPOConfig(**cfg), seed=21)
    a.collect()
    env_b = make_env()
    b = PPO(env_b, PPOConfig(**cfg, fused_advantages=True), seed=21)
    b.collect()
    torch.cuda.synchronize()
    assert bool(b.buf.dones.any()) and not bool(b.buf.dones.all())
    assert torch.equal(_bits(a.buf.rewards), _bits(b.buf.rewards)) and torch.equal(_bits(a.buf.values), _bits(b.buf.values))
    assert torch.equal(_bits(a.buf.adv), _bits(b.buf.adv)) and torch.equal(_bits(a.buf.ret), _bits(b.buf.ret))
    before = [q.detach().clone() for q in b.policy.parameters()]
    u = b.update()
    assert set(u) == {"pg_loss", "v_loss", "entropy", "clip_frac", "explained_variance"}
    assert all(math.isfinite(u[k]) for k in ("pg_loss", "v_loss", "entropy", "clip_frac")), u
    adv64, ret64 = b.buf.adv.double().cpu().numpy().ravel(), b.buf.ret.double().cpu().numpy().ravel()
    ev64 = 1.0 - adv64.var(ddof=1) / ret64.var(ddof=1)
    assert abs(1.0 - ev64) < 10.0, "pick another seed: the 1e-5 bound below assumes Var(adv) / Var(ret) < 10"
    print(f"\nuse_graph={use_graph}: explained_variance {u['explained_variance']!r}, fp64 {ev64!r}")
    assert abs(u["explained_variance"] - ev64) <= 1e-5
    # the single minibatch is a permutation of all rows: its statistics are the buffer's
    ref = (float(adv64.mean()), float(adv64.std(ddof=1)), float(np.abs(adv64).max()))
    gm, gs = _gaps(float(b._adv_stats[0]), float(b._adv_stats[1]), ref)
    print(f"minibatch statistics: gap / bound: mean {gm:.3f} std {gs:.3f}")
    assert gm <= 1.0 and gs <= 1.0, (b._adv_stats.tolist(), ref)
    assert all(not torch.equal(p0, q.detach()) for p0, q in zip(before, b.policy.parameters()))
    assert "explained_variance" not in a.update()
    env_a.close(); env_b.close()
