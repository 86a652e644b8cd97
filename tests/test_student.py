"""dronechase_amd/student.py on the CPU: FLIAStudent against the reference's StudentWithFLIA (tests/golden/student_flia.npz, made by
tests/golden/gen_student_flia.py in float64 with the seeded weights of tests/_student_cases.py), the loss, the trainer, the driver,
and the host-side refusals of te_sphere_encode, which return before anything is launched.

Tolerance |d| <= 1e-4 + 1e-4 |ref| (tests/_student_cases.py).  Measured on the CPU in float32 against the float64 fixture:
outputs max |d| 8.1e-6 (0.080 of the bound), trunk 1.3e-5 (0.068), conv stack 1.9e-6 (0.012)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _student_cases as S

FAKE = 1 << 20          # never dereferenced: every call below fails a check first


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(S.FIXTURE))


@pytest.fixture(scope="module")
def student():
    from dronechase_amd.student import load_flia_student
    w = S.recipe_weights(S.keys_and_shapes())
    return load_flia_student({k: torch.from_numpy(v).float() for k, v in w.items()})


def _obs(fx, dtype=torch.float32):
    return {"stacked_spheres": torch.from_numpy(fx["stacked_spheres"]).to(dtype), "validity_mask": torch.from_numpy(fx["validity_mask"]),
            "inertial_data": torch.from_numpy(fx["inertial_data"]).to(dtype), "last_action": torch.from_numpy(fx["last_action"]).to(dtype)}


def test_state_dict_has_the_references_names_and_shapes():
    from dronechase_amd.student import FLIAStudent
    sd = FLIAStudent().state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == S.keys_and_shapes()
    assert len(sd) == 58 and sum(v.numel() for v in sd.values()) == 4_265_412


def test_load_is_strict_and_names_the_key():
    from dronechase_amd.student import FLIAStudent, load_flia_student
    sd = FLIAStudent().state_dict()
    missing = {k: v for k, v in sd.items() if k != "mlp_head.6.bias"}
    with pytest.raises(ValueError, match=r"missing \['mlp_head\.6\.bias'\]"):
        load_flia_student(missing)
    with pytest.raises(ValueError, match=r"unknown \['value_net\.weight'\]"):
        load_flia_student(dict(sd, **{"value_net.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match=r"mlp_head\.6\.bias: \(5,\), expected \(4,\)"):
        load_flia_student(dict(sd, **{"mlp_head.6.bias": torch.zeros(5)}))


def test_load_reads_a_checkpoint_file(tmp_path, student):
    from dronechase_amd.student import load_flia_student
    path = tmp_path / "student_last_model_0.pt"
    torch.save(student.state_dict(), path)
    again = load_flia_student(str(path))
    assert not again.training
    for (k, a), (_, b) in zip(student.state_dict().items(), again.state_dict().items()):
        assert torch.equal(a, b), k


def test_outputs_trunk_and_conv_stack_match_the_reference(fx, student):
    obs = _obs(fx)
    with torch.no_grad():
        out, trunk = student(obs).numpy(), student.trunk(obs).numpy()
        x = torch.stack([obs["stacked_spheres"][r, s] for r, s in fx["conv_spheres"]])
        conv = student.sphere_cnn.conv_stack(x).numpy()
        as_bool = student(dict(obs, validity_mask=obs["validity_mask"].bool())).numpy()
    for name, got, ref in (("out", out, fx["out"]), ("trunk", trunk, fx["trunk"]), ("conv", conv, fx["conv"])):
        ok, gap, ratio = S.within(got, ref)
        print(f"{name}: max |d| {gap:.3g}, {ratio:.3g} of the bound")
        assert ok, (name, gap, ratio)
    assert np.array_equal(as_bool, out)        # uint8 and bool masks are the same mask


def test_the_module_in_float64_is_the_reference_to_rounding(fx, student):
    import copy
    net = copy.deepcopy(student).double()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in S.recipe_weights(S.keys_and_shapes()).items()})
    with torch.no_grad():
        out = net(_obs(fx, torch.float64)).numpy()
    assert np.abs(out - fx["out"]).max() < 1e-12


def test_spheres_that_do_not_count_are_never_looked_at(fx, student):
    obs = _obs(fx)
    poked = dict(obs, stacked_spheres=obs["stacked_spheres"].clone())
    dead = torch.from_numpy(~S.counting(fx["validity_mask"]))
    assert dead.sum() == 48 - 19      # row 0 counts its sphere 0
    poked["stacked_spheres"][dead] = float("nan")
    with torch.no_grad():
        a, b = student(obs), student(poked)
    assert torch.isfinite(b).all() and torch.equal(a, b)


def test_imitation_loss_matches_the_reference(fx):
    from dronechase_amd.student import StudentTrainer, imitation_loss
    for i, (p, t) in enumerate(S.loss_pairs()):
        p, t = torch.from_numpy(p), torch.from_numpy(t)
        assert abs(float(imitation_loss(p, t)) - fx["loss_default"][i]) < 1e-12
        got = imitation_loss(p, t, w_dir=StudentTrainer.W_DIR, w_mag=StudentTrainer.W_MAG, w_raw_direction=StudentTrainer.W_RAW_DIRECTION)
        assert abs(float(got) - fx["loss_trainer"][i]) < 1e-10


def test_trainer_lowers_the_loss_on_a_fixed_batch():
    from dronechase_amd.student import FLIAStudent, StudentTrainer
    torch.manual_seed(5)
    rng = np.random.default_rng(11)
    obs = {"stacked_spheres": torch.from_numpy(rng.uniform(0, 1, (16, 6, 3, 13, 26))).float(),
           "validity_mask": torch.from_numpy((rng.uniform(size=(16, 6)) < 0.5).astype(np.uint8)),
           "inertial_data": torch.from_numpy(rng.standard_normal((16, 15))).float(),
           "last_action": torch.from_numpy(rng.uniform(-1, 1, (16, 4))).float()}
    target = torch.from_numpy(rng.uniform(-1, 1, (16, 4))).float()
    target[:, 3] = target[:, 3].abs()
    student = FLIAStudent()
    trainer = StudentTrainer(student, lr=1e-3)
    losses = [trainer.step(obs, target) for _ in range(20)]
    assert all(torch.is_tensor(v) and not v.requires_grad for v in losses) and student.training
    losses = [float(v) for v in losses]
    assert np.all(np.isfinite(losses)) and np.mean(losses[-3:]) < 0.8 * np.mean(losses[:3]), losses


def test_driver_clamps_and_refuses_sampling(fx, student):
    from dronechase_amd.student import StudentDriver
    obs = _obs(fx)
    driver = StudentDriver(student)
    a, state = driver.predict(obs)
    with torch.no_grad():
        raw = student(obs)
    assert state is None and a.shape == (8, 4)
    assert (raw.abs() > 1).any() and (raw[:, 3] < 0).any()          # the recipe's outputs do leave the box
    assert torch.equal(a, torch.max(torch.min(raw, torch.ones(4)), torch.tensor([-1.0, -1.0, -1.0, 0.0])))
    student.train()
    try:        # predict is the eval-mode network whatever mode the module is in, and leaves the mode as it was
        assert torch.equal(driver.predict(obs)[0], a) and student.training
    finally:
        student.eval()
    with pytest.raises(ValueError, match="deterministic must be True"):
        driver.predict(obs, deterministic=False)
    with pytest.raises(ValueError, match="must live on a GPU"):
        StudentDriver(student, fused_encoder=True)
    with pytest.raises(TypeError, match="FLIAStudent"):
        StudentDriver(torch.nn.Linear(2, 2))


class StackedBackend:
    """Stands in for a level5 BatchedEnv on CPU tensors: the fixture's 8 rows as the observation, env e's episodes last e + 1 steps
    and pay the clamped action's first component."""

    def __init__(self, fx, **cfg):
        import types
        self.device, self.N = torch.device("cpu"), 8
        self.obs = tuple(_obs(fx)[k] for k in ("stacked_spheres", "validity_mask", "inertial_data", "last_action"))
        self.cfg = types.SimpleNamespace(**dict(dict(stacked_obs=1, agent_scripted=0, evaluation=0, n_pursuers=6, ally_policy=0, task=6), **cfg))
        self.age, self.actions = torch.zeros(8, dtype=torch.int64), []

    def reset(self, mask=None):
        self.age.zero_()
        return self.obs[0][:, 0], self.obs[2], self.obs[3]      # the own sphere, as te_observe gives it

    def observe_stacked(self):
        return self.obs

    def step(self, *a, **k):
        raise AssertionError("a stacked env is stepped with step_stacked")

    def step_stacked(self, actions, terminal=True):
        assert terminal is False
        self.actions.append(actions.clone())
        self.age += 1
        done = self.age == torch.arange(8) + 1
        self.age[done] = 0
        return (*self.obs, actions[:, 0].clone(), done.to(torch.uint8), torch.zeros((8, 4), dtype=torch.int32))


def test_evaluate_policy_on_the_stacked_observation(fx, student):
    from dronechase_amd import config as K
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.pipeline import ReinforcementLearningPipeline as RLP
    from dronechase_amd.ppo import LidarInertialActionPolicy
    from dronechase_amd.student import StudentDriver
    want = StudentDriver(student).predict(_obs(fx))[0]
    for policy in (student, StudentDriver(student)):
        env = StackedBackend(fx)
        ret, length = evaluate_policy(policy, env, n_eval_episodes=12, poll_every=4)
        assert ret.shape == (12,) and list(length) == [1, 2, 3, 4, 5, 5, 6, 6, 7, 7, 8, 8]      # quotas (12 + e) // 8
        assert all(torch.equal(a, want) for a in env.actions)
        assert np.allclose(ret, np.repeat(want[:, 0].numpy(), [1, 1, 1, 1, 2, 2, 2, 2]) * length, rtol=1e-6)
    assert RLP.evaluate(student, StackedBackend(fx), n_eval_episodes=9)[2] == 9
    with pytest.raises(ValueError, match="stacked.*FLIAStudent or a StudentDriver"):
        evaluate_policy(LidarInertialActionPolicy(), StackedBackend(fx), n_eval_episodes=4)
    with pytest.raises(ValueError, match="deterministic must be True"):
        evaluate_policy(student, StackedBackend(fx), n_eval_episodes=4, deterministic=False)
    for task, flag in (("level5_dumb", "agent_scripted"), ("level5_2bt", "agent_scripted"), ("evaluation", "evaluation")):
        with pytest.raises(ValueError, match=rf"'{task}' has no agent.*cfg\.{flag}"):
            evaluate_policy(student, StackedBackend(fx, task=K.TASKS[task], **{flag: 1}), n_eval_episodes=4)
    # a student on an env that does not give the stacked observation
    flat = StackedBackend(fx, stacked_obs=0)
    with pytest.raises(ValueError, match="FLIAStudent / StudentDriver reads the stacked.*LidarInertialActionPolicy"):
        evaluate_policy(student, flat, n_eval_episodes=4)


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_sphere_encode_refusals_come_from_the_host(lib):
    from dronechase_amd import _lib
    assert "te_sphere_encode" in _lib.EXPORTS and "te_sphere_encode_param_words" in _lib.EXPORTS
    words = C.c_size_t()
    assert lib.te_sphere_encode_param_words(3, C.byref(words)) == 0
    assert words.value == 32 * 75 + 32 + 64 * 288 + 64
    assert lib.te_sphere_encode_param_words(2, C.byref(words)) != 0 and b"channels must be 3" in lib.te_last_error()
    assert lib.te_sphere_encode_param_words(3, None) != 0 and b"out_words" in lib.te_last_error()
    base = dict(params=FAKE, channels=3, n_rows=4, n_spheres=6, stacked=FAKE, mask=FAKE, out=FAKE, stream=None)
    cases = [(dict(params=None), b"null argument params"), (dict(stacked=None), b"null argument stacked"), (dict(out=None), b"null argument out"),
             (dict(params=FAKE + 4), b"params must be 16-byte aligned"), (dict(stacked=FAKE + 8), b"stacked must be 16-byte aligned"),
             (dict(out=FAKE + 4), b"out must be 16-byte aligned"), (dict(channels=2), b"channels must be 3"),
             (dict(n_spheres=0), b"n_spheres must be in 1 .. 8, not 0"), (dict(n_spheres=9), b"n_spheres must be in 1 .. 8, not 9"),
             (dict(n_rows=0), b"n_rows must be positive, not 0"), (dict(n_rows=-1), b"n_rows must be positive"),
             (dict(n_rows=1 << 30, n_spheres=8), b"n_rows * n_spheres must be at most")]
    for kw, msg in cases:
        args = [kw.get(k, v) for k, v in base.items()]
        assert lib.te_sphere_encode(*args) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_sphere_encode: ") and msg in err, (kw, err)
