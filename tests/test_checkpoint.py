"""PPO.save / PPO.load, save_sb3_policy and dronechase_amd.callbacks, as far as they need no GPU: the policy export's round trip and key
set, the stop rule against tables worked out by hand, the checkpoint file's safety, and every refusal of PPO.load with the count of
env.reset() calls it leaves behind (0: a refusal comes before the env is touched).  The envs are StubEnv (tests/_policy_cases.py),
which PPO can be built on but not stepped; bitwise resume is tests/test_gpu_checkpoint.py's."""
import io
import math
import zipfile

import numpy as np
import pytest
import torch

from tests._policy_cases import StubEnv

SHAPES = {"default": (256, (64, 64)), "BO": (512, (128, 256, 512)), "learn": (512, (512, 128, 256))}


class StateEnv(StubEnv):
    """StubEnv with a state blob of its own, so that a checkpoint with restore_env=True can be written and read on the CPU."""

    def __init__(self, task="stage03", n=4):
        super().__init__(task, n)
        self.words = torch.arange(3 * n, dtype=torch.int32)

    def get_state(self):
        return self.words.clone()

    def set_state(self, words):
        self.words = words.clone()


# ---------------------------------------------------------------------- export
def _sb3_keys(n_hidden):
    """The key set of an SB3 MultiInputPolicy with the reference's extractor, written out from the issue's list (not through the code
    under test): the extractor under three owners, the two head MLPs, the two output layers and log_std."""
    wb = lambda prefix: {prefix + ".weight", prefix + ".bias"}
    extractor = set()
    for layer in ("lidar_feature_extractor.0", "lidar_feature_extractor.2", "final_layer.0",
                  *(f"{m}_feature_extractor.{i}" for m in ("inertial", "action") for i in (0, 2, 4))):
        extractor |= wb(layer)
    keys = {"log_std"} | wb("action_net") | wb("value_net")
    for owner in ("features_extractor.", "pi_features_extractor.", "vf_features_extractor."):
        keys |= {owner + k for k in extractor}
    for net in ("policy_net", "value_net"):
        for i in range(n_hidden):
            keys |= wb(f"mlp_extractor.{net}.{2 * i}")
    return keys


@pytest.mark.parametrize("name", list(SHAPES))
def test_export_round_trip_and_key_set(name, tmp_path):
    from dronechase_amd.ppo import LidarInertialActionPolicy, load_sb3_policy, save_sb3_policy
    features_dim, net_arch = SHAPES[name]
    torch.manual_seed(7)
    policy = LidarInertialActionPolicy(features_dim=features_dim, net_arch=net_arch)
    with torch.no_grad():
        policy.log_std.copy_(torch.tensor([0.2, -0.3, 0.1, -0.5]))
    path = str(tmp_path / "policy.zip")
    save_sb3_policy(policy, path)
    with zipfile.ZipFile(path) as z:
        assert z.namelist() == ["policy.pth"]
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    assert set(sd) == _sb3_keys(len(net_arch))
    back = load_sb3_policy(path)
    ours, theirs = dict(policy.named_parameters()), dict(back.named_parameters())
    assert ours.keys() == theirs.keys()
    for k in ours:
        assert theirs[k].dtype == torch.float32 and torch.equal(ours[k], theirs[k]), k


# ---------------------------------------------------------------------- the stop rule
class ScriptedModel:
    """What EvalCallback asks of a PPO: evaluate() returns the next scripted mean as n equal episode returns."""

    def __init__(self, means, step=100):
        self.means, self.step, self.num_timesteps, self.saved, self.saved_at = list(means), step, 0, [], []

    def evaluate(self, env, n_eval_episodes, deterministic):
        m = self.means[len(self.saved_at)]
        self.saved_at.append(self.num_timesteps)
        return np.full(n_eval_episodes, m, dtype=np.float32), np.full(n_eval_episodes, 7, dtype=np.int32)

    def save_policy(self, path):
        self.saved.append(path)


def _stops_at(means):
    """The 1-based evaluation at which EvalCallback + StopTrainingOnNoModelImprovement(3, 5) ends training; None if it never does."""
    from dronechase_amd.callbacks import EvalCallback, StopTrainingOnNoModelImprovement
    model = ScriptedModel(means)
    cb = EvalCallback(None, n_eval_episodes=2, eval_freq=100, best_model_save_path=None, log_path=None,
                      callback_after_eval=StopTrainingOnNoModelImprovement(max_no_improvement_evals=3, min_evals=5))
    cb.init_callback(model)
    for k in range(1, len(means) + 1):
        model.num_timesteps += 100
        if not cb.on_iteration():
            return k, cb
    return None, cb


# Worked out by hand from the rule (count -> 0 when the parent's best exceeds the remembered one, else count + 1 and stop when
# n_calls > 5 and count > 3; then remember the best).
#   strictly improving: the count is 0 after every evaluation: never.
#   flat from the start (1, 1, 1, ...): evaluation 1 improves on -inf (count 0); evaluations 2..6 give counts 1..5.  count > 3 first at
#     evaluation 5, where n_calls = 5 is not > 5; at evaluation 6 both hold: 6.
#   improving for three, then flat (1, 2, 3, 3, ...): counts 0, 0, 0, 1, 2, 3, 4: count > 3 first at evaluation 7, n_calls = 7 > 5: 7.
#   worse after the first (5, 4, 3, ...): the best stays 5, so the counts are the flat case's: 6.
#   improving for six, then flat: counts 0 x 6, then 1, 2, 3, 4 at evaluations 7..10: 10.
STOP_TABLE = [
    ("strictly improving", [float(k) for k in range(1, 13)], None),
    ("flat from the start", [1.0] * 12, 6),
    ("improving then flat", [1.0, 2.0, 3.0] + [3.0] * 9, 7),
    ("worse after the first", [5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0], 6),
    ("improving for six, then flat", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0] + [6.0] * 6, 10),
]


@pytest.mark.parametrize("label,means,expected", STOP_TABLE, ids=[c[0] for c in STOP_TABLE])
def test_stop_rule(label, means, expected):
    stopped, cb = _stops_at(means)
    assert stopped == expected
    n = expected or len(means)
    assert len(cb.evaluations_timesteps) == n and cb.evaluations_timesteps == [100 * k for k in range(1, n + 1)]
    assert cb.best_mean_reward == max(means[:n])


def test_callbacks_fire_on_timesteps_and_keep_their_state(tmp_path):
    """Frequency in timesteps: with 100 timesteps per iteration and eval_freq 250 the evaluations fall on 300, 600, 900.  The state
    of a list goes through torch.save / torch.load(weights_only=True) into a fresh list, which then carries on as the first would."""
    from dronechase_amd.callbacks import CallbackList, EvalCallback, StopTrainingOnNoModelImprovement
    make = lambda: CallbackList([EvalCallback(None, n_eval_episodes=3, eval_freq=250, log_path=str(tmp_path / "log"),
                                              best_model_save_path=str(tmp_path / "best"),
                                              callback_after_eval=StopTrainingOnNoModelImprovement(3, 5))])
    model = ScriptedModel([1.0, 3.0, 2.0, 2.5, 4.0])
    a = make()
    a.init_callback(model)
    for _ in range(9):
        model.num_timesteps += 100
        assert a.on_iteration()
    assert model.saved_at == [300, 600, 900] and len(model.saved) == 2        # the best model: at 1.0 and at 3.0, not at 2.0
    npz = np.load(str(tmp_path / "log" / "evaluations.npz"))
    assert set(npz.files) == {"timesteps", "results", "ep_lengths"}
    assert npz["timesteps"].tolist() == [300, 600, 900] and npz["results"].shape == (3, 3) and npz["ep_lengths"].shape == (3, 3)
    torch.save(a.state_dict(), str(tmp_path / "cb.pt"))
    state = torch.load(str(tmp_path / "cb.pt"), weights_only=True)
    b = make()
    b.load_state_dict(state)
    b.init_callback(model)
    for cb in (a, b):
        t, saved_at = model.num_timesteps, list(model.saved_at)
        for _ in range(3):
            model.num_timesteps += 100
            assert cb.on_iteration()
        assert model.saved_at == saved_at + [1200]
        ev = cb.callbacks[0]
        assert ev.evaluations_timesteps == [300, 600, 900, 1200] and ev.best_mean_reward == 3.0 and ev.callback_after_eval.n_calls == 4
        assert ev.callback_after_eval.no_improvement_evals == 2
        model.num_timesteps, model.saved_at = t, saved_at
    with pytest.raises(ValueError, match="same classes in the same order"):
        make().callbacks[0].load_state_dict(state)


# ---------------------------------------------------------------------- the checkpoint file and PPO.load's refusals
def _saved(tmp_path, env=None, **cfg):
    from dronechase_amd.ppo import PPO, PPOConfig
    env = env or StateEnv()
    ppo = PPO(env, PPOConfig(n_steps=2, **cfg), seed=3)
    ppo.num_timesteps = 4096
    path = str(tmp_path / "ckpt.pt")
    ppo.save(path)
    return ppo, path


def _only_plain(x, path="ckpt"):
    """Tensors on the CPU, numbers, strings, None, lists, tuples and dicts: nothing else."""
    if torch.is_tensor(x):
        assert x.device.type == "cpu", path
    elif isinstance(x, dict):
        for k, v in x.items():
            assert isinstance(k, (str, int)), path
            _only_plain(v, f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _only_plain(v, f"{path}[{i}]")
    else:
        assert x is None or isinstance(x, (bool, int, float, str)), (path, type(x))


def test_checkpoint_is_plain_data_and_round_trips(tmp_path):
    from dronechase_amd.ppo import CHECKPOINT_FORMAT, CHECKPOINT_VERSION, PPO
    ppo, path = _saved(tmp_path, episode_stats=True)
    ck = torch.load(path, weights_only=True)
    _only_plain(ck)
    assert ck["format"] == CHECKPOINT_FORMAT and ck["version"] == CHECKPOINT_VERSION
    for key in ("cfg", "policy_shape", "policy", "optimizer", "num_timesteps", "updates_since_sync", "wingman", "obs", "env_config",
                "env_state", "abi_version", "monitor", "cpu_rng_state", "cuda_rng_state", "callbacks"):
        assert key in ck, key
    assert ck["policy_shape"] == [3, 256, [64, 64]] and ck["obs"] is None and ck["num_timesteps"] == 4096
    assert ck["env_config"].numpy().tobytes() == bytes(ppo.env.cfg)
    rng = torch.get_rng_state()
    env = StateEnv()
    env.words.zero_()
    torch.manual_seed(99)
    back = PPO.load(path, env)
    assert env.resets == 1 and back.num_timesteps == 4096 and back.cfg == ppo.cfg and back.monitor is not None
    assert torch.equal(env.words, ppo.env.words) and torch.equal(torch.get_rng_state(), rng)
    for (k, a), (_, b) in zip(ppo.policy.named_parameters(), back.policy.named_parameters()):
        assert torch.equal(a, b), k
    # restore_env=False into another task's env: the learner and the count, nothing of the env, no generator
    other = StateEnv("stage02", n=6)
    before = other.words.clone()
    torch.manual_seed(99)
    tuned = PPO.load(path, other, cfg=type(ppo.cfg)(n_steps=4, learning_rate=1e-5, episode_stats=True), restore_env=False)
    assert other.resets == 1 and torch.equal(other.words, before) and tuned.num_timesteps == 4096
    assert tuned.cfg.learning_rate == 1e-5 and tuned.opt.param_groups[0]["lr"] == 1e-5 and tuned.buf.rewards.shape == (4, 6)
    assert all(torch.equal(a, b) for a, b in zip(ppo.policy.parameters(), tuned.policy.parameters()))


def test_save_refuses_an_unconsumed_rollout(tmp_path):
    ppo, path = _saved(tmp_path)
    ppo._rollout_pending = True         # what collect() leaves and update() clears
    with pytest.raises(ValueError, match="update\\(\\) has not consumed"):
        ppo.save(str(tmp_path / "mid.pt"))
    assert not (tmp_path / "mid.pt").exists()


def _rewritten(path, tmp_path, **changes):
    ck = torch.load(path, weights_only=True)
    ck.update(changes)
    out = str(tmp_path / "changed.pt")
    torch.save(ck, out)
    return out


def test_load_refusals_come_before_the_env_is_touched(tmp_path):
    from dronechase_amd.callbacks import CallbackList, CheckpointCallback, EvalCallback, StopTrainingOnNoModelImprovement
    from dronechase_amd.ppo import PPO, PPOConfig
    ppo, path = _saved(tmp_path)
    ppo._callback = CallbackList([EvalCallback(None, 2, 100, None, None, callback_after_eval=StopTrainingOnNoModelImprovement(3, 5)),
                                  CheckpointCallback(100, str(tmp_path))])
    with_callbacks = str(tmp_path / "with_callbacks.pt")
    ppo.save(with_callbacks)
    lists = {"reordered": CallbackList([CheckpointCallback(100, str(tmp_path)), EvalCallback(None, 2, 100, None, None)]),
             "shorter": CallbackList([CheckpointCallback(100, str(tmp_path))]),
             "not a list": CheckpointCallback(100, str(tmp_path)),
             "no child": CallbackList([EvalCallback(None, 2, 100, None, None), CheckpointCallback(100, str(tmp_path))])}
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    cases = [
        ("format name", _rewritten(path, tmp_path / "a", format="somebody.elses"), {}, "somebody.elses"),
        ("newer version", _rewritten(path, tmp_path / "b", version=2), {}, "version 2"),
        ("features_dim", path, dict(cfg=PPOConfig(features_dim=512, net_arch=(64, 64))), "cfg.features_dim is 512"),
        ("net_arch", path, dict(cfg=PPOConfig(net_arch=(64, 32))), "cfg.net_arch is \\(64, 32\\)"),
        ("fused_optimizer", path, dict(cfg=PPOConfig(fused_update=True, fused_optimizer=True)), "cfg.fused_optimizer is True"),
        ("episode_stats", path, dict(cfg=PPOConfig(episode_stats=True)), "cfg.episode_stats is True"),
        ("wingman_driver", path, dict(cfg=PPOConfig(wingman_driver="snapshot")), "cfg.wingman_driver is 'snapshot'"),
        ("n_envs", path, dict(env=StateEnv(n=6)), "te_config.n_envs is 6, the checkpoint's env had 4"),
        ("task", path, dict(env=StateEnv("stage02")), "te_config.task"),
        ("no callback state", path, dict(callback=lists["shorter"]), "holds no callback state"),
        ("the constructor's own", path, dict(env=StateEnv("exp05"), restore_env=False), "caller-driven wingmen"),
    ] + [(f"callbacks {k}", with_callbacks, dict(callback=cb), "same classes in the same order|callback_after_eval is") for k, cb in lists.items()]
    for label, file, kw, text in cases:
        kw = dict(kw)
        env = kw.pop("env", None) or StateEnv()
        state = env.words.clone()
        with pytest.raises(ValueError, match=text):
            PPO.load(file, env, **kw)
        assert env.resets == 0 and torch.equal(env.words, state), label
    # a policy of another LIDAR channel count, and a file whose env had no state to give
    two = StateEnv()
    two.lidar = torch.zeros(4, 2, 13, 26)
    with pytest.raises(ValueError, match="reads 3 LIDAR channels, the environment has 2"):
        PPO.load(path, two, restore_env=False)
    _, stateless = _saved(tmp_path / "a", env=StubEnv())
    env = StateEnv()
    with pytest.raises(ValueError, match="holds no env state"):
        PPO.load(stateless, env)
    assert two.resets == 0 and env.resets == 0
    assert PPO.load(stateless, env, restore_env=False).num_timesteps == 4096 and env.resets == 1
    # and the accepted callback list takes its state
    good = CallbackList([EvalCallback(None, 2, 100, None, None, callback_after_eval=StopTrainingOnNoModelImprovement(3, 5)),
                         CheckpointCallback(100, str(tmp_path))])
    assert PPO.load(with_callbacks, StateEnv(), callback=good)._callback is good
    assert math.isinf(good.callbacks[0].best_mean_reward) and good.callbacks[1].last_fired is None
