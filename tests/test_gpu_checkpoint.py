"""PPO.save / PPO.load and the training callbacks on the device: a resumed run equals the uninterrupted one bit for bit.

Shapes: stage03 (exp05 for the wingman snapshot) x 66 envs: even, so the eager rollout writes its observations straight into the
buffer's slots, and no multiple of the kernels' 32-row tiles.  max_step=12: an episode ends, and its env auto-resets, at step 13 at the
latest (test_resume_is_bitwise_across_the_auto_reset runs that far).
n_steps=3 and batch_size=96: the 198 rows are two full minibatches and a ragged one of 6.  n_epochs=2.  One iteration is 198 timesteps.

Run A builds with seed 5, learns, saves, learns on.  Run B is PPO.load on a fresh env of the same config.  PPO.load builds with its own
seed (0), so nothing B ends with can come from the constructor: not the weights, not the wingman's snapshot, not a generator.
For the fused kernels the bound on |B - A| is zero (they are deterministic by contract).  With every switch off update() runs PyTorch's
autograd, whose determinism is PyTorch's: A is run a second time (A'), and the bound on |B - A| is the largest |A' - A| of that tensor,
the exact zero wherever A' equals A (that test says what PyTorch needs to be asked for, for A' to equal A)."""
import os

import numpy as np
import pytest

from tests._policy_cases import _gpu

pytestmark = pytest.mark.gpu

N_ENVS, MAX_STEP, N_STEPS, BATCH, EPOCHS = 66, 12, 3, 96, 2
ITER = N_STEPS * N_ENVS
FUSED = dict(fused_forward=True, fused_forward_bf16=True, fused_update=True, fused_update_bf16=True, fused_optimizer=True,
             fused_advantages=True, episode_stats=True)
CONFIGS = {"a: fused, graph, fused_epoch": dict(use_graph=True, fused_epoch=True, **FUSED),
           "b: fused, eager, python epoch": dict(use_graph=False, fused_epoch=False, **FUSED),
           "c: every switch off, graph": dict(use_graph=True),
           "c: every switch off, eager": dict(use_graph=False)}


@pytest.fixture(scope="module", autouse=True)
def lib():
    from dronechase_amd.build import build_library
    build_library()


def _env(task="stage03", n=N_ENVS, **kw):
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    return BatchedEnv(default_config(task, n_envs=n, max_step=MAX_STEP, **kw), "cuda:0")


def _cfg(**kw):
    from dronechase_amd.ppo import PPOConfig
    return PPOConfig(n_steps=N_STEPS, batch_size=BATCH, n_epochs=EPOCHS, **kw)


def _tensors(x, prefix=""):
    """{path: tensor} of every tensor below x."""
    torch = _gpu()
    if torch.is_tensor(x):
        return {prefix: x.detach().clone()}
    out = {}
    if isinstance(x, dict):
        for k, v in x.items():
            out.update(_tensors(v, f"{prefix}/{k}"))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            out.update(_tensors(v, f"{prefix}/{i}"))
    return out


def _snapshot(ppo):
    """Everything a run is compared by: every parameter, every optimiser state tensor, the env's state blob, the monitor's state."""
    torch = _gpu()
    torch.cuda.synchronize()
    out = _tensors(dict(ppo.policy.named_parameters()), "param")
    out.update(_tensors(ppo.opt.state_dict()["state"], "opt"))
    out["env"] = ppo.env.get_state().clone()
    if ppo.monitor is not None:
        out["monitor"] = ppo.monitor.state()
    if ppo.wingman is not None:
        out.update(_tensors(dict(ppo.wingman.policy.named_parameters()), "wingman"))
    torch.cuda.synchronize()
    return out


def _run_a(path, task="stage03", save_after=2, total=4, **switches):
    from dronechase_amd.ppo import PPO
    env = _env(task)
    ppo, logs = PPO(env, _cfg(**switches), seed=5), []
    ppo.learn(save_after * ITER, log=logs.append)
    ppo.save(path)
    ppo.learn(total * ITER, log=logs.append)
    snap = _snapshot(ppo)
    env.close()
    assert [l["timesteps"] for l in logs] == [ITER * k for k in range(1, total + 1)]
    return snap, logs


def _run_b(path, task="stage03", total=4):
    from dronechase_amd.ppo import PPO
    env = _env(task)
    ppo, logs = PPO.load(path, env), []
    ppo.learn(total * ITER, log=logs.append)
    snap = _snapshot(ppo)
    env.close()
    return snap, logs


def _assert_bitwise(a, b, label):
    torch = _gpu()
    assert a.keys() == b.keys(), label
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (label, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("name", [n for n in CONFIGS if n[0] in "ab"])
def test_resume_is_bitwise_on_the_fused_stack(name, tmp_path):
    path = str(tmp_path / "ckpt.pt")
    (a, logs_a), (b, logs_b) = _run_a(path, **CONFIGS[name]), _run_b(path)
    print(f"\n{name}: {os.path.getsize(path)} bytes; iterations 3, 4 of A {logs_a[2:]}\n of B {logs_b}")
    _assert_bitwise(a, b, name)
    assert len(logs_b) == 2 and logs_b[0] == logs_a[2] and logs_b[1] == logs_a[3]


@pytest.mark.parametrize("name", [n for n in CONFIGS if n[0] in "ab"])
def test_resume_is_bitwise_across_the_auto_reset(name, tmp_path):
    """An episode ends when its step count EXCEEDS max_step, so the 12 steps of the test above end none.  Six iterations are 18 steps:
    every env that did not end sooner ends and auto-resets at step 13, in iteration 5, after the save at iteration 2, so the resumed
    env draws its new episodes from the restored blob and the monitor closes episodes it was restored in the middle of."""
    path = str(tmp_path / "ckpt.pt")
    (a, logs_a), (b, logs_b) = _run_a(path, total=6, **CONFIGS[name]), _run_b(path, total=6)
    assert sum(l["ep_count"] for l in logs_a[:2]) == 0 and sum(l["ep_count"] for l in logs_a[2:]) >= N_ENVS, [l["ep_count"] for l in logs_a]
    _assert_bitwise(a, b, name)
    assert logs_b == logs_a[2:]


@pytest.fixture
def deterministic_convolutions():
    """torch.backends.cudnn.deterministic for one test (on ROCm: MIOpen's deterministic convolution algorithms), put back afterwards."""
    torch = _gpu()
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("name", [n for n in CONFIGS if n[0] == "c"])
def test_resume_with_every_switch_off_is_within_pytorchs_own_repeatability(name, tmp_path, deterministic_convolutions):
    """The bound on every tensor and log value is the |A' - A| of that tensor between two uninterrupted runs.  With PyTorch's defaults
    the convolutions' backward (MIOpen) does not repeat itself: measured on the MI355X, A' differed from A in 93 of 125 tensors after
    four iterations (the env state included: the trajectories part), and so did B, by amounts of the same size in either direction
    (|B - A| of pg_loss 1.3e-7 against |A' - A| 9.8e-9, of v_loss 7e-12 against 0), which one sample of |A' - A| cannot bound.  So the
    test asks PyTorch for its deterministic convolutions: then A' equals A in all 125 tensors and both logs, the bound is the exact
    zero everywhere, and B has to equal A bit for bit, as on the fused stack."""
    torch = _gpu()
    path, again = str(tmp_path / "ckpt.pt"), str(tmp_path / "again.pt")
    (a, logs_a), (a2, logs_a2), (b, logs_b) = _run_a(path, **CONFIGS[name]), _run_a(again, **CONFIGS[name]), _run_b(path)
    assert a.keys() == a2.keys() == b.keys() and len(logs_b) == 2
    worst = {}
    for k in a:
        f = lambda t: t.double()
        bound, gap = float((f(a2[k]) - f(a[k])).abs().max()), float((f(b[k]) - f(a[k])).abs().max())
        worst[k] = (gap, bound)
    for i in (2, 3):
        assert logs_a[i].keys() == logs_a2[i].keys() == logs_b[i - 2].keys()
        for key in logs_a[i]:
            worst[f"log{i + 1}/{key}"] = (abs(logs_b[i - 2][key] - logs_a[i][key]), abs(logs_a2[i][key] - logs_a[i][key]))
    print(f"\n{name}: largest |B - A| {max(g for g, _ in worst.values()):.3e}, largest |A' - A| {max(b for _, b in worst.values()):.3e}")
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_the_stale_wingman_snapshot_survives(tmp_path):
    """exp05, the ally flown by a snapshot that is synced every 3 updates, saved after ONE update: in iterations 2 and 3 the ally
    still flies the initial weights of seed 5, which are neither the learner's nor what PPO.load's constructor draws.  A load that
    re-syncs the wingman, rebuilds it from the learner, or loses the count (the sync before iteration 4 never comes, or comes early)
    ends with another env state."""
    torch = _gpu()
    path = str(tmp_path / "ckpt.pt")
    switches = dict(wingman_driver="snapshot", wingman_sync_every=3, **CONFIGS["a: fused, graph, fused_epoch"])
    (a, logs_a), (b, logs_b) = _run_a(path, "exp05", save_after=1, total=4, **switches), _run_b(path, "exp05", total=4)
    ck = torch.load(path, weights_only=True)
    assert ck["updates_since_sync"] == 1 and ck["wingman"]["snapshot"]
    assert not all(torch.equal(ck["wingman"]["policy"][k], ck["policy"][k]) for k in ck["policy"]), "the snapshot was not stale when saved"
    _assert_bitwise(a, b, "exp05 snapshot")
    assert logs_b == logs_a[1:]
    # the sync before iteration 4 happened in both: the wingman holds the learner's weights of after update 3, not the final ones
    assert not all(torch.equal(a[k], a["param" + k[len("wingman"):]]) for k in a if k.startswith("wingman"))


def test_save_between_collect_and_update_is_refused_and_harmless(tmp_path):
    from dronechase_amd.ppo import PPO
    switches = CONFIGS["b: fused, eager, python epoch"]
    outs = []
    for attempt in (False, True):
        env = _env()
        ppo = PPO(env, _cfg(**switches), seed=5)
        ppo.collect()
        if attempt:
            with pytest.raises(ValueError, match="update\\(\\) has not consumed"):
                ppo.save(str(tmp_path / "mid.pt"))
            assert not (tmp_path / "mid.pt").exists()
        log = ppo.update()
        ppo.save(str(tmp_path / "after.pt"))        # legal again
        outs.append((_snapshot(ppo), log))
        env.close()
    _assert_bitwise(outs[0][0], outs[1][0], "update after a refused save")
    assert outs[0][1] == outs[1][1]


def test_env_mismatch_and_fine_tuning_on_another_task(tmp_path):
    torch = _gpu()
    from dronechase_amd.ppo import PPO
    path = str(tmp_path / "ckpt.pt")
    switches = CONFIGS["a: fused, graph, fused_epoch"]
    env = _env()
    ppo = PPO(env, _cfg(**switches), seed=5)
    ppo.learn(2 * ITER)
    ppo.save(path)
    params = {k: v.detach().clone() for k, v in ppo.policy.named_parameters()}
    env.close()
    for other, field in ((_env(n=64), "te_config.n_envs"), (_env("stage02"), "te_config.task")):
        other.reset()
        before = other.get_state().clone()
        with pytest.raises(ValueError, match=field):
            PPO.load(path, other)
        assert torch.equal(other.get_state(), before), field        # not reset, not restored into
        other.close()
    stage02 = _env("stage02")
    tuned = PPO.load(path, stage02, restore_env=False)
    assert tuned.num_timesteps == 2 * ITER
    assert all(torch.equal(p, params[k]) for k, p in tuned.policy.named_parameters())
    logs = []
    tuned.learn(3 * ITER, log=logs.append)
    assert len(logs) == 1 and logs[0]["timesteps"] == 3 * ITER and all(np.isfinite(v) for k, v in logs[0].items() if k != "explained_variance")
    assert not all(torch.equal(p, params[k]) for k, p in tuned.policy.named_parameters())
    stage02.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused path", "module path"])
def test_deterministic_evaluation_leaves_the_generators_alone(fused):
    torch = _gpu()
    from dronechase_amd.ppo import PPO
    env, eval_env = _env(), _env(n=8, seed=1)
    ppo = PPO(env, _cfg(**(CONFIGS["a: fused, graph, fused_epoch"] if fused else {})), seed=5)
    ppo.learn(ITER)
    assert (ppo.fused is not None) == fused
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state("cuda:0")
    returns, lengths = ppo.evaluate(eval_env, n_eval_episodes=5, deterministic=True)
    assert returns.shape == (5,) and lengths.shape == (5,)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state("cuda:0"), gpu)
    env.close(); eval_env.close()


def test_callbacks_on_the_device_and_resuming_with_them(tmp_path):
    """learn() with callbacklist(...) evaluating and checkpointing every iteration, four iterations (fewer than min_evals, so the stop
    rule cannot end the run).  Then the run is resumed from the second checkpoint with a list of the same classes on a fresh evaluation
    env: the final weights and evaluations.npz are those of the uninterrupted run."""
    torch = _gpu()
    from dronechase_amd.callbacks import callbacklist
    from dronechase_amd.ppo import PPO, load_sb3_policy
    switches = CONFIGS["a: fused, graph, fused_epoch"]

    def lists(tag):
        eval_env = _env(n=8, seed=1)
        return eval_env, callbacklist(eval_env, log_path=str(tmp_path / tag / "logs"), model_path=str(tmp_path / tag / "models"),
                                      save_freq=ITER, n_eval_episodes=5)

    env = _env()
    eval_env, cb = lists("a")
    ppo, weights = PPO(env, _cfg(**switches), seed=5), []
    ppo.learn(4 * ITER, log=lambda l: weights.append({k: v.detach().cpu().clone() for k, v in ppo.policy.named_parameters()}), callback=cb)
    final_a = _snapshot(ppo)
    env.close(); eval_env.close()
    npz_a = dict(np.load(str(tmp_path / "a" / "logs" / "evaluations.npz")))
    assert set(npz_a) == {"timesteps", "results", "ep_lengths"}
    assert npz_a["timesteps"].tolist() == [ITER, 2 * ITER, 3 * ITER, 4 * ITER]
    assert npz_a["results"].shape == (4, 5) and npz_a["ep_lengths"].shape == (4, 5) and (npz_a["ep_lengths"] > 0).all()
    means = npz_a["results"].astype(np.float64).mean(axis=1)
    best = load_sb3_policy(str(tmp_path / "a" / "models" / "best_model.zip"))
    at = int(np.argmax(means))          # the first of equal maxima: a later equal mean does not exceed it
    print(f"\nevaluation means {means.tolist()}: best at evaluation {at + 1}")
    for k, p in best.named_parameters():
        assert torch.equal(p, weights[at][k]), k
    files = sorted(f for f in os.listdir(str(tmp_path / "a" / "models")) if f.endswith(".pt"))
    assert files == sorted(f"rl_model_{ITER * k}_steps.pt" for k in range(1, 5))

    env = _env()
    eval_env, cb = lists("b")
    resumed = PPO.load(str(tmp_path / "a" / "models" / f"rl_model_{2 * ITER}_steps.pt"), env, callback=cb)
    assert resumed.num_timesteps == 2 * ITER and cb.callbacks[0].evaluations_timesteps == [ITER, 2 * ITER]
    resumed.learn(4 * ITER, callback=cb)
    _assert_bitwise(final_a, _snapshot(resumed), "resumed with callbacks")
    env.close(); eval_env.close()
    npz_b = dict(np.load(str(tmp_path / "b" / "logs" / "evaluations.npz")))
    for k in npz_a:
        assert npz_a[k].dtype == npz_b[k].dtype and np.array_equal(npz_a[k], npz_b[k]), k
    assert sorted(f for f in os.listdir(str(tmp_path / "b" / "models")) if f.endswith(".pt")) == files[2:]
