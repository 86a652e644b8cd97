"""What PPOConfig.fused_epoch and PackedAdam.step(repack=True) refuse, and the host-side refusals of te_policy_ppo_epoch and
te_policy_adam_step_bf16 that need no device: every one of them returns before anything is launched, so all of this runs on a CPU."""
import ctypes as C
import types

import pytest

from tests._policy_cases import StubEnv, _shape

NEEDS = ("fused_update", "fused_optimizer", "fused_advantages")
FAKE = 1 << 20          # never dereferenced: every call below fails a check first


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_fused_epoch_is_off_by_default_and_names_each_missing_switch():
    from dronechase_amd.ppo import PPOConfig
    assert PPOConfig().fused_epoch is False
    assert PPOConfig(**{k: True for k in NEEDS}, fused_epoch=True).fused_epoch
    for missing in NEEDS:
        on = {k: True for k in NEEDS if k != missing}
        if missing == "fused_update":
            on.pop("fused_optimizer")       # PPOConfig refuses fused_optimizer without fused_update in its own right
        with pytest.raises(ValueError, match=rf"fused_epoch.*needs {missing}\b"):
            PPOConfig(fused_epoch=True, **on)
    with pytest.raises(ValueError, match=r"fused_epoch.*needs fused_update\b"):
        PPOConfig(fused_epoch=True)


def test_ppo_refuses_it_again_and_before_the_env_is_touched():
    from dronechase_amd.ppo import PPO, PPOConfig
    env = StubEnv()
    for missing in NEEDS:       # set on the object, past PPOConfig's own check
        cfg = PPOConfig(n_steps=2, **{k: True for k in NEEDS}, fused_epoch=True)
        setattr(cfg, missing, False)
        with pytest.raises(ValueError, match=rf"fused_epoch.*needs {missing}\b"):
            PPO(env, cfg)
    # a CPU device: fused_epoch's own text, in front of its three needs' "needs a GPU device"
    with pytest.raises(ValueError, match=r"PPOConfig\.fused_epoch runs the HIP kernels of te_policy_ppo_epoch: it needs a GPU device"):
        PPO(env, PPOConfig(n_steps=2, **{k: True for k in NEEDS}, fused_epoch=True))
    for extra in ("fused_update_wide", "fused_update_bf16"):      # it composes with both: still the same refusal, not another
        with pytest.raises(ValueError, match=r"fused_epoch.*needs a GPU device"):
            PPO(env, PPOConfig(n_steps=2, **{k: True for k in NEEDS}, fused_epoch=True, **{extra: True}))
    assert env.resets == 0


def test_packed_adam_repack_needs_bf16_buffers(lib):
    import torch
    from dronechase_amd.ppo import PackedAdam
    owner = types.SimpleNamespace(params=torch.zeros(100), device=torch.device("cpu"), weights_bf16=None, weights_bf16_t=None)
    opt = PackedAdam(owner, lr=3e-4)
    with pytest.raises(ValueError, match="repack=True.*owns none"):
        opt.step(torch.zeros(100), 0.5, repack=True)
    assert int(opt.step_count) == 0


def test_exports_and_the_struct_mirror(lib):
    from dronechase_amd import _lib
    for name in ("te_policy_adam_step_bf16", "te_policy_ppo_epoch"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.te_abi_version() == 5
    # the call checks the mirror's size against its own sizeof before anything else: a wrong one is refused, the right one gets past it
    a = _lib.PpoEpochArgs(struct_size=C.sizeof(_lib.PpoEpochArgs) - 8)
    assert lib.te_policy_ppo_epoch(C.byref(a), None) != 0 and b"struct_size" in lib.te_last_error()
    a.struct_size = C.sizeof(_lib.PpoEpochArgs)
    assert lib.te_policy_ppo_epoch(C.byref(a), None) != 0 and b"struct_size" not in lib.te_last_error()
    assert lib.te_last_error().startswith(b"te_policy_ppo_epoch: ")


def _epoch_args(lib, **kw):
    """Arguments that would pass every check (fp32, default shape, 200 rows in minibatches of 64), with fake pointers."""
    from dronechase_amd import _lib
    shape = _shape(3, 256, (64, 64))
    words, state, ws, aws = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.te_policy_param_words_shaped(C.byref(shape), C.byref(words)) == 0
    assert lib.te_policy_opt_state_bytes(words.value, C.byref(state)) == 0
    assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(shape), 64, C.byref(ws)) == 0
    assert lib.te_adv_stats_workspace_bytes(64, C.byref(aws)) == 0
    a = _lib.PpoEpochArgs(struct_size=C.sizeof(_lib.PpoEpochArgs), shape=shape, n_perm=200, batch=64, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
                          state_bytes=state.value, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_scale=1.0,
                          workspace_bytes=ws.value, adv_workspace_bytes=aws.value)
    for name in ("params", "lidar", "inertial", "last_action", "action", "old_logp", "adv", "ret", "perm", "grad", "state", "workspace",
                 "adv_workspace", "adv_mean_std", "stats", "sums"):
        setattr(a, name, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_epoch_refusals_come_from_the_host(lib):
    """Every check is made before the first launch, the inner calls' included, and the text starts with the entry's name."""
    ws = _epoch_args(lib).workspace_bytes
    cases = [(dict(batch=0), b"batch must be >= 1"), (dict(batch=-3), b"batch must be >= 1"), (dict(n_perm=0), b"n_perm must be >= 1"),
             (dict(perm=None), b"perm is required"), (dict(perm=FAKE + 4), b"perm must be 8-byte aligned"),
             (dict(weights_bf16=FAKE), b"go together"), (dict(weights_bf16_t=FAKE), b"go together"),
             (dict(sums=None), b"sums are required"), (dict(stats=None), b"are required"), (dict(adv_mean_std=None), b"are required"),
             (dict(lidar=None), b"null argument"), (dict(params=None), b"null argument"), (dict(state=None), b"null argument"),
             (dict(grad=FAKE + 4), b"grad must be 16-byte aligned"), (dict(workspace=FAKE + 16), b"workspace must be 256-byte aligned"),
             (dict(workspace_bytes=ws - 1), b"workspace too small"), (dict(adv_workspace_bytes=15), b"workspace too small"),
             (dict(state_bytes=100), b"state too small"), (dict(max_grad_norm=0.0), b"max_grad_norm must be > 0"),
             (dict(clip_range=-1.0), b"clip_range must be finite"), (dict(lr=-1.0), b"lr must be"),
             (dict(batch=(1 << 27) + 1, n_perm=1 << 28, adv_workspace_bytes=1 << 40), b"at most 2^27"),
             (dict(shape=_shape(3, 512, (128, 256))), b"is not served")]
    for kw, msg in cases:
        assert lib.te_policy_ppo_epoch(C.byref(_epoch_args(lib, **kw)), None) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_policy_ppo_epoch: ") and msg in err, (kw, err)
    assert lib.te_policy_ppo_epoch(None, None) != 0 and b"null argument" in lib.te_last_error()
    # the tail minibatch is checked as well as the first: 200 = 3 x 64 + 8, and a workspace that holds 8 rows but not 64 is refused
    small = C.c_size_t()
    assert lib.te_policy_grad_workspace_bytes_shaped(C.byref(_shape(3, 256, (64, 64))), 8, C.byref(small)) == 0
    if small.value < ws:
        assert lib.te_policy_ppo_epoch(C.byref(_epoch_args(lib, workspace_bytes=small.value)), None) != 0
        assert b"workspace too small" in lib.te_last_error()


def test_adam_step_bf16_refusals_come_from_the_host(lib):
    shape = _shape(3, 256, (64, 64))
    words, need = C.c_size_t(), C.c_size_t()
    assert lib.te_policy_param_words_shaped(C.byref(shape), C.byref(words)) == 0
    assert lib.te_policy_opt_state_bytes(words.value, C.byref(need)) == 0
    base = dict(params=FAKE, grad=FAKE, state=FAKE, state_bytes=need.value, shape=C.byref(shape), w=FAKE, wt=FAKE, lr=3e-4, b1=0.9, b2=0.999,
                eps=1e-5, max_norm=0.5, scale=1.0, stream=None)
    args = lambda **kw: [kw.get(k, v) for k, v in base.items()]
    bad = _shape(3, 512, (128, 256))
    cases = [(dict(params=None), b"null"), (dict(grad=None), b"null"), (dict(state=None), b"null"), (dict(w=None), b"weights_bf16 is required"),
             (dict(params=FAKE + 4), b"params must be 16-byte"), (dict(w=FAKE + 2), b"weights_bf16 must be 16-byte"),
             (dict(wt=FAKE + 8), b"weights_bf16_t must be 16-byte"), (dict(state_bytes=need.value - 1), b"state too small"),
             (dict(max_norm=0.0), b"max_grad_norm must be > 0"), (dict(max_norm=-1.0), b"max_grad_norm must be > 0"),
             (dict(shape=C.byref(bad)), b"the served shapes"), (dict(shape=None), b"null shape")]
    for kw, msg in cases:
        assert lib.te_policy_adam_step_bf16(*args(**kw)) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_policy_adam_step_bf16: ") and msg in err, (kw, err)
