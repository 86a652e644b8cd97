"""Episode monitor (dronechase_amd/monitor.py, te_monitor_* of include/threatengage.h): quotas, the CPU implementation and the
VecEnv's infos[i]["episode"] without a GPU; the HIP kernels, their capture in a graph, real env steps and PPO's episode_stats on
the MI355X.  The checker is an independent per-env loop in np.float32, written here."""
import ctypes as C

import numpy as np
import pytest

EPS64 = 2.0 ** -52


# ---------------------------------------------------------------------- the independent checker
def brute_force_quotas(N, n):
    return [(n + e) // N for e in range(N)]


def checker(rew, done, info, n_records, carry=None):
    """rew [T, N] f32, done [T, N] bool, info [T, N, 4] i32 -> every env's completed episodes in order, the record arrays
    (env-major, the first quota_e episodes of env e) and the partial episode left per env ((ret, len), to carry on)."""
    T, N = rew.shape
    quota = brute_force_quotas(N, n_records)
    episodes = [[] for _ in range(N)]            # (ret f32, len, info row, step it ended at)
    partial = []
    for e in range(N):
        ret, length = (np.float32(0), 0) if carry is None else carry[e]
        for t in range(T):
            ret = np.float32(ret + np.float32(rew[t, e]))
            length += 1
            if done[t, e]:
                episodes[e].append((ret, length, info[t, e].copy(), t))
                ret, length = np.float32(0), 0
        partial.append((ret, length))
    rec = [ep for e in range(N) for ep in episodes[e][:quota[e]]]
    slots = {}                                   # record slot -> episode, for the slots written so far
    at = 0
    for e in range(N):
        for k, ep in enumerate(episodes[e][:quota[e]]):
            slots[at + k] = ep
        at += quota[e]
    return dict(episodes=episodes, partial=partial, recorded=len(rec), slots=slots, quota=quota)


def window(episodes, t0, t1):
    """Exact window statistics of the episodes that ended in steps [t0, t1)."""
    eps = [ep for per_env in episodes for ep in per_env if t0 <= ep[3] < t1]
    rets = np.array([float(ep[0]) for ep in eps], np.float64)
    return dict(count=len(eps), sum_len=sum(ep[1] for ep in eps), sum_info=sum((ep[2].astype(np.int64) for ep in eps), np.zeros(4, np.int64)),
                rets=rets, rets32=np.array([ep[0] for ep in eps], np.float32))


def assert_window(summary, stats, want):
    """Integers exact; the fp64 sums within the reassociation bound count * 2^-52 * sum|x| (two orders of the same n-term fp64 sum
    differ by at most 2 (n - 1) u sum|x|, u = 2^-53); min / max exact; std from the same two sums."""
    n = want["count"]
    assert int(summary["count"]) == n == stats["count"]
    if n == 0:
        assert set(stats) == {"count"}
        return
    assert int(summary["sum_len"]) == want["sum_len"] and np.array_equal(summary["sum_info"], want["sum_info"])
    r = want["rets"]
    s1, s2 = float(np.sum(r)), float(np.sum(r * r))
    b1, b2 = n * EPS64 * float(np.sum(np.abs(r))), n * EPS64 * s2
    print(f"count {n}: sum_ret off by {abs(float(summary['sum_ret']) - s1):.3e} (bound {b1:.3e}), sum_ret2 by {abs(float(summary['sum_ret2']) - s2):.3e} (bound {b2:.3e})")
    assert abs(float(summary["sum_ret"]) - s1) <= b1 and abs(float(summary["sum_ret2"]) - s2) <= b2
    assert abs(stats["ep_rew_mean"] - s1 / n) <= b1 / n + EPS64 * abs(s1 / n)
    assert np.float32(summary["min_ret"]) == want["rets32"].min() and np.float32(summary["max_ret"]) == want["rets32"].max()
    assert stats["ep_rew_min"] == float(want["rets32"].min()) and stats["ep_rew_max"] == float(want["rets32"].max())
    assert stats["ep_len_mean"] == want["sum_len"] / n
    for k, v in zip(("ep_agent_kills_mean", "ep_allies_kills_mean", "ep_deads_mean", "ep_wave_mean"), want["sum_info"]):
        assert stats[k] == int(v) / n
    # var = E[x^2] - mean^2: each term carries a relative error of at most (2 n + 1) 2^-52, and mean^2 <= E[x^2]
    e2 = s2 / n
    assert abs(stats["ep_rew_std"] ** 2 - float(np.var(r))) <= (3 * n + 8) * EPS64 * e2


def assert_records(records, recorded, want, n_records):
    ret, length, info = records
    assert recorded == want["recorded"]
    assert ret.shape == (n_records,) and ret.dtype == np.float32 and length.shape == (n_records,) and info.shape == (n_records, 4)
    for at in range(n_records):
        if at in want["slots"]:
            r, l, i, _ = want["slots"][at]
            assert ret[at].tobytes() == np.float32(r).tobytes() and length[at] == l and np.array_equal(info[at], i), at
        else:
            assert length[at] == 0, at           # an unwritten slot


def script(T, N, seed, p=0.2):
    rng = np.random.default_rng(seed)
    rew = ((rng.random((T, N)) * 2 - 1) * 1000).astype(np.float32)
    done = rng.random((T, N)) < p
    info = rng.integers(0, 40, size=(T, N, 4)).astype(np.int32)
    return rew, done, info


def feed(mon, rew, done, info, t0, t1, device="cpu"):
    import torch
    for t in range(t0, t1):
        mon.step(torch.from_numpy(rew[t]).to(device), torch.from_numpy(done[t].astype(np.uint8)).to(device), torch.from_numpy(info[t]).to(device))


def run_and_check(N, R, T, device, seed):
    """Two windows (stats(reset=True) in the middle), records, partial-episode carry-over: the same equalities on either device."""
    from dronechase_amd.monitor import EpisodeMonitor, _summary_to_stats
    rew, done, info = script(T, N, seed)
    want = checker(rew, done, info, R)
    mon = EpisodeMonitor(N, device, n_records=R)
    half = T // 2
    feed(mon, rew, done, info, 0, half, device)
    peek = mon.summary(reset=False)
    s = mon.summary(reset=True)
    assert peek.tobytes() == s.tobytes()         # reset=False left the window alone
    assert_window(s, _summary_to_stats(s), window(want["episodes"], 0, half))
    empty = mon.stats(reset=True)
    assert empty == {"count": 0}                 # the window is empty now, and the keys are absent, not NaN
    feed(mon, rew, done, info, half, T, device)
    before_reset = mon.state()                   # the wave rows (the order-sensitive fp64 sums) are still in it
    s = mon.summary(reset=True)
    assert_window(s, _summary_to_stats(s), window(want["episodes"], half, T))   # episodes that straddle the reset are whole
    assert int(s["recorded"]) == want["recorded"]
    assert_records(mon.records(), mon.recorded(), want, R)
    return mon, want, before_reset


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("N,n", [(1, 1), (1, 5), (4, 10), (7, 3), (64, 100), (100, 64), (257, 1000)])
def test_quotas_are_evaluate_policys(N, n):
    import torch
    from dronechase_amd.monitor import EpisodeMonitor, episode_quotas
    quota, offset = episode_quotas(N, n)
    want = brute_force_quotas(N, n)
    assert list(quota) == want and int(quota.sum()) == n
    assert list(offset) == list(np.cumsum([0] + want[:-1]))
    # every env finishes an episode at every step: SB3's loop (step-major, env e counted while counts[e] < target[e]) against the records
    steps = max(want) + 2
    mon = EpisodeMonitor(N, "cpu", n_records=n)
    counts, sb3 = [0] * N, [[] for _ in range(N)]
    for t in range(steps):
        r = (np.arange(N) * 16 + t).astype(np.float32)
        mon.step(torch.from_numpy(r), torch.ones(N, dtype=torch.uint8), torch.zeros((N, 4), dtype=torch.int32))
        for e in range(N):
            if counts[e] < want[e]:
                sb3[e].append(float(r[e])); counts[e] += 1
    ret, length, _ = mon.records()
    assert mon.recorded() == n and list(ret) == [x for per_env in sb3 for x in per_env] and (length == 1).all()


def test_cpu_monitor_semantics():
    mon, want, _ = run_and_check(N=5, R=12, T=60, device="cpu", seed=11)
    # last_ret / last_len: the last completed episode of every env
    for e, eps in enumerate(want["episodes"]):
        if eps:
            assert mon.last_ret[e].numpy().tobytes() == np.float32(eps[-1][0]).tobytes() and int(mon.last_len[e]) == eps[-1][1]
    run_and_check(N=5, R=0, T=60, device="cpu", seed=12)      # n_records = 0 records nothing


def test_cpu_monitor_state_round_trip():
    from dronechase_amd.monitor import EpisodeMonitor
    rew, done, info = script(20, 3, 5)
    a, b = EpisodeMonitor(3, "cpu", n_records=4), EpisodeMonitor(3, "cpu", n_records=4)
    feed(a, rew, done, info, 0, 20)
    feed(b, rew, done, info, 0, 10)
    saved = b.state()
    feed(b, rew, done, info, 0, 7)               # wander off, then come back
    b.load_state(saved)
    feed(b, rew, done, info, 10, 20)
    assert a.stats() == b.stats() and all(np.array_equal(x, y) for x, y in zip(a.records(), b.records()))
    b.reset()
    assert b.recorded() == 0 and b.stats() == {"count": 0}


class ScriptedBackend:
    """Stands in for BatchedEnv on CPU tensors: env e's episodes last e + 1 steps and pay (e + 1) per step."""

    def __init__(self, n):
        import torch
        self.device, self.N = torch.device("cpu"), n
        self.lidar, self.inertial, self.last_action = torch.ones((n, 3, 13, 26)), torch.zeros((n, 15)), torch.zeros((n, 4))
        self.t_lidar, self.t_inertial, self.t_last_action = torch.zeros((n, 3, 13, 26)), torch.zeros((n, 15)), torch.zeros((n, 4))
        self.age = torch.zeros(n, dtype=torch.int64)

    def reset(self, mask=None):
        self.age.zero_()
        return self.lidar, self.inertial, self.last_action

    def step(self, actions, terminal=True):
        import torch
        e = torch.arange(self.N)
        self.age += 1
        done = self.age == e + 1
        self.age[done] = 0
        info = torch.stack((e, e * 2, e * 3, e * 4), dim=1).to(torch.int32)
        return self.lidar, self.inertial, self.last_action, (e + 1).float(), done.to(torch.uint8), info

    def close(self):
        pass


@pytest.mark.parametrize("output,infos", [("numpy", "dicts"), ("numpy", "lazy"), ("torch", "dicts"), ("torch", "lazy")])
def test_vecenv_episode_monitor_over_a_stub(output, infos):
    from dronechase_amd.vec_env import ThreatEngageVecEnv
    n = 4
    on = ThreatEngageVecEnv("stage03", num_envs=n, backend=ScriptedBackend(n), output=output, infos=infos, episode_monitor=True)
    off = ThreatEngageVecEnv("stage03", num_envs=n, backend=ScriptedBackend(n), output=output, infos=infos)
    on.reset(); off.reset()
    a = np.zeros((n, 4), np.float32)
    held = []
    for t in range(1, 9):
        _, _, dones, got = on.step(a)
        _, _, _, plain = off.step(a)
        held.append((t, got))
        for e in range(n):
            ended = t % (e + 1) == 0
            assert bool(dones[e]) == ended and ("episode" in got[e]) == ended and "episode" not in plain[e]
            if ended:      # env e's episodes: e + 1 steps of reward e + 1
                ep = got[e]["episode"]
                assert ep["r"] == float((e + 1) ** 2) and ep["l"] == e + 1 and type(ep["r"]) is float and type(ep["l"]) is int and ep["t"] >= 0
            assert {k: v for k, v in got[e].items() if k not in ("episode", "terminal_observation")} == \
                   {k: v for k, v in plain[e].items() if k != "terminal_observation"}
    # infos read late still show their own step's episode
    for t, got in held:
        for e in range(n):
            if t % (e + 1) == 0:
                assert got[e]["episode"]["l"] == e + 1
    on.reset()
    _, _, _, got = on.step(a)
    assert got[0]["episode"] == {"r": 1.0, "l": 1, "t": got[0]["episode"]["t"]} and "episode" not in got[1]


def test_pipeline_factory_forwards_the_flag():
    from dronechase_amd.pipeline import ReinforcementLearningPipeline as RLP
    v = RLP.create_vectorized_environment("stage03", {}, n_envs=3, monitor=False, backend=ScriptedBackend(3), episode_monitor=True)
    assert v.episode_monitor is not None
    v = RLP.create_vectorized_environment("stage03", {}, n_envs=3, monitor=False, backend=ScriptedBackend(3))
    assert v.episode_monitor is None


# ---------------------------------------------------------------------- GPU
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 600])
def test_kernel_against_the_checker(N):
    """A partial wave, a wave boundary, one and several workgroups; n_records 0, 3, N and 2 N + 1."""
    need_gpu()
    import torch
    for R in (0, 3, N, 2 * N + 1):
        mon, want, full = run_and_check(N, R, T=50, device="cuda:0", seed=100 + N)
        again, _, full_again = run_and_check(N, R, T=50, device="cuda:0", seed=100 + N)
        # two runs from init: bitwise the same buffer, with the second window's rows in it and after they are cleared
        assert torch.equal(full, full_again) and torch.equal(mon.buf, again.buf)
        for e, eps in enumerate(want["episodes"]):
            if eps:
                assert mon.last_ret[e].cpu().numpy().tobytes() == np.float32(eps[-1][0]).tobytes() and int(mon.last_len[e]) == eps[-1][1]


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    need_gpu()
    import torch
    from dronechase_amd import _lib
    from dronechase_amd.monitor import EpisodeMonitor
    L = _lib.load()
    N, R = 65, 7
    mon = EpisodeMonitor(N, "cuda:0", n_records=R)
    rew, done, info = script(4, N, 3)
    feed(mon, rew, done, info, 0, 4, "cuda:0")
    before = mon.buf.clone()
    r, d, i = torch.zeros(N, device="cuda:0"), torch.ones(N, dtype=torch.uint8, device="cuda:0"), torch.zeros((N, 4), dtype=torch.int32, device="cuda:0")
    out = torch.zeros(80, dtype=torch.uint8, device="cuda:0")
    p, nb = mon.buf.data_ptr(), mon.buf.numel()
    need = C.c_size_t()
    assert L.te_monitor_bytes(N, R, C.byref(need)) == 0 and need.value == nb
    bad = [lambda: L.te_monitor_step(None, nb, N, R, r.data_ptr(), d.data_ptr(), i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb, N, R, None, d.data_ptr(), i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb, N, R, r.data_ptr(), None, i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb, N, R, r.data_ptr(), d.data_ptr(), None, None),
           lambda: L.te_monitor_step(p, nb, 0, R, r.data_ptr(), d.data_ptr(), i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb, N, -1, r.data_ptr(), d.data_ptr(), i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb - 1, N, R, r.data_ptr(), d.data_ptr(), i.data_ptr(), None),
           lambda: L.te_monitor_step(p, nb, N + 64, R, r.data_ptr(), d.data_ptr(), i.data_ptr(), None),     # a larger monitor than the buffer holds
           lambda: L.te_monitor_init(None, nb, N, R, None), lambda: L.te_monitor_init(p, nb - 1, N, R, None),
           lambda: L.te_monitor_init(p, nb, -3, R, None),
           lambda: L.te_monitor_stats(p, nb, N, R, None, 1, None), lambda: L.te_monitor_stats(p, 16, N, R, out.data_ptr(), 1, None),
           lambda: L.te_monitor_stats(p, nb, N, -2, out.data_ptr(), 1, None),
           lambda: L.te_monitor_bytes(0, 0, C.byref(need)), lambda: L.te_monitor_bytes(4, -1, C.byref(need)), lambda: L.te_monitor_bytes(4, 4, None)]
    for k, call in enumerate(bad):
        assert call() != 0, k
        assert "te_monitor" in L.te_last_error().decode(), k
    torch.cuda.synchronize()
    assert torch.equal(mon.buf, before) and not out.any()
    # a device given without an index is the current one: tensors that report "cuda:0" are accepted
    bare = EpisodeMonitor(N, "cuda", n_records=R)
    feed(bare, rew, done, info, 0, 4, "cuda:0")
    assert torch.equal(bare.buf, before)


@pytest.mark.gpu
def test_monitor_step_is_capturable():
    need_gpu()
    import torch
    from dronechase_amd.monitor import EpisodeMonitor
    N, R, T = 257, 300, 10
    rew, done, info = script(T, N, 21, p=0.3)
    eager = EpisodeMonitor(N, "cuda:0", n_records=R)
    feed(eager, rew, done, info, 0, T, "cuda:0")
    mon = EpisodeMonitor(N, "cuda:0", n_records=R)
    s_r, s_d, s_i = torch.zeros(N, device="cuda:0"), torch.ones(N, dtype=torch.uint8, device="cuda:0"), torch.ones((N, 4), dtype=torch.int32, device="cuda:0")
    saved = mon.state()
    side = torch.cuda.Stream("cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mon.step(s_r, s_d, s_i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mon.step(s_r, s_d, s_i)
    mon.load_state(saved)                       # the warm-up steps did reach the monitor: roll them back
    for t in range(T):
        s_r.copy_(torch.from_numpy(rew[t])); s_d.copy_(torch.from_numpy(done[t].astype(np.uint8))); s_i.copy_(torch.from_numpy(info[t]))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mon.buf, eager.buf)
    assert mon.recorded() == checker(rew, done, info, R)["recorded"]


# stage03 with max_step = 20 ends an episode at its 21st step unless a shot raises the limit by step_increment = 100.  The CPU oracle
# (oracle/te_oracle.py) on this very config and action stream: every episode is 21 steps long and the last env finishes its second
# one at step index 41.  63 steps leave room for a third; the test asserts the property itself.
STEPS_FOR_TWO_EPISODES = 63


@pytest.mark.gpu
def test_monitor_on_real_steps():
    """256 stage03 envs with max_step = 20 under te_random_actions: the monitor's records and window against the checker fed with
    the reward, done and info of every step copied to the host."""
    need_gpu()
    import torch
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.monitor import EpisodeMonitor, _summary_to_stats
    N, R, T = 256, 512, STEPS_FOR_TWO_EPISODES
    env = BatchedEnv(default_config("stage03", n_envs=N, max_step=20), "cuda:0")
    env.reset()
    mon = EpisodeMonitor(N, "cuda:0", n_records=R)
    rew, done, info = np.zeros((T, N), np.float32), np.zeros((T, N), bool), np.zeros((T, N, 4), np.int32)
    for t in range(T):
        *_, r, d, i = env.step(env.random_actions(9, t), terminal=False)
        mon.step(r, d, i)
        rew[t], done[t], info[t] = r.cpu().numpy(), d.cpu().numpy().astype(bool), i.cpu().numpy()
    want = checker(rew, done, info, R)
    assert min(len(eps) for eps in want["episodes"]) >= 2, "every env must finish at least two episodes"
    assert_records(mon.records(), mon.recorded(), want, R)
    assert mon.recorded() == R
    s = mon.summary(reset=True)
    assert_window(s, _summary_to_stats(s), window(want["episodes"], 0, T))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_vecenv_episode_monitor_on_gpu(output):
    need_gpu()
    from dronechase_amd.vec_env import ThreatEngageVecEnv
    n, T = 96, 21      # max_step = 6: episodes end at steps 6, 13 and 20 (the last one, whose rows a torch-output read still gets)
    v = ThreatEngageVecEnv("stage03", num_envs=n, seed=4, max_step=6, output=output, infos="lazy", episode_monitor=True)
    v.reset()
    rew, done, got = np.zeros((T, n), np.float32), np.zeros((T, n), bool), []
    for t in range(T):
        _, r, d, infos = v.step(v.backend.random_actions(9, t))
        rew[t], done[t] = (r, d) if output == "numpy" else (r.cpu().numpy(), d.cpu().numpy())
        got.append(infos)
    want = checker(rew, done, np.zeros((T, n, 4), np.int32), 0)
    seen = 0
    for e in range(n):
        ends = {ep[3]: ep for ep in want["episodes"][e]}
        for t in range(T):                       # read after the run: every step's infos still show that step's episodes
            if t in ends:
                ep = got[t][e]["episode"] if output == "numpy" or t == T - 1 else None
                if ep is None:                   # (torch output: a late read of a done env's dict raises for its terminal rows; see test_vec_env.py)
                    continue
                assert np.float32(ep["r"]).tobytes() == np.float32(ends[t][0]).tobytes() and ep["l"] == ends[t][1]
                seen += 1
            else:
                assert "episode" not in got[t][e]
    assert seen > 0
    v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [True, False])
def test_ppo_episode_stats(use_graph):
    """collect()'s ep_* keys against the episodes recomputed from the rollout buffer (reward_scale 1: raw rewards), over two
    collects: the graph's warm-up and capture steps are not counted, and a partial episode carries over."""
    need_gpu()
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.ppo import PPO, PPOConfig
    N = 512
    env = BatchedEnv(default_config("stage03", n_envs=N, max_step=20), "cuda:0")
    ppo = PPO(env, PPOConfig(episode_stats=True, reward_scale=1.0, n_steps=32, n_epochs=1, use_graph=use_graph), seed=2)
    carry = None
    for _ in range(2):
        log = ppo.collect()
        rew, done = ppo.buf.rewards.cpu().numpy(), ppo.buf.dones.cpu().numpy() > 0.5
        want = checker(rew, done, np.zeros((32, N, 4), np.int32), 0, carry)
        carry = want["partial"]
        w = window(want["episodes"], 0, 32)
        n = w["count"]
        assert log["ep_count"] == n == log["episodes_finished"] and n > 0
        assert log["ep_len_mean"] == w["sum_len"] / n
        s1 = float(np.sum(w["rets"]))
        assert abs(log["ep_rew_mean"] - s1 / n) <= EPS64 * float(np.sum(np.abs(w["rets"]))) + EPS64 * abs(s1 / n)
        assert log["ep_rew_min"] == float(w["rets32"].min()) and log["ep_rew_max"] == float(w["rets32"].max())
        assert all(np.isfinite(v) for v in log.values())
    # (the second collect's episodes: one that is longer than the steps it took in this collect began in the first)
    assert any(ep[1] > ep[3] + 1 for eps in want["episodes"] for ep in eps), "no episode carried over from the first collect"
    env.close()
    env = BatchedEnv(default_config("stage03", n_envs=N, max_step=20), "cuda:0")
    plain = PPO(env, PPOConfig(reward_scale=1.0, n_steps=32, n_epochs=1, use_graph=use_graph), seed=2)
    assert set(plain.collect()) == {"mean_step_reward", "episodes_finished"} and plain.monitor is None
    env.close()
