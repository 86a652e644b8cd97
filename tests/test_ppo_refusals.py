"""What PPO(...) and PPOConfig(...) refuse, text by text: a sweep of constructor calls on CPU stub environments, each compared with
tests/golden/ppo_refusals.json (accepted or refused, the exception's type and its full text), and after every refused PPO(...) the
environment has not been reset.

The recording was made from the package of commit 36b7fb5, the last one whose PPO.__init__ interleaved its checks with construction:
with that commit's tree first on PYTHONPATH, `python tests/test_ppo_refusals.py --record FILE` runs the sweeps below and writes FILE.
At that commit 508 of the refusals came after env.reset(), so the resets assertion below fails there.

The switches are set by attribute on a PPOConfig(n_steps=2), past its own __post_init__ (a second, small sweep calls PPOConfig(**switches)
for that).  Every case runs on a CPU device, where the rule "the wingman driver needs a GPU device" fires in front of three others:
wingman_sync_every >= 1, fused_optimizer needing fused_update inside PPO, and the two checks of the wingman object itself.  The
recording does not hold those three."""
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_refusals.json")
N_CASES, N_ACCEPTED, N_CONFIG_CASES = 19008, 48, 176          # a case cannot drop out silently
SWITCHES = ("fused_forward", "fused_forward_bf16", "fused_update", "fused_update_wide", "fused_update_bf16", "fused_optimizer",
            "fused_advantages", "wingman_bf16", "fast_learner", "episode_stats")
SUBSETS = [s for k in range(4) for s in itertools.combinations(SWITCHES, k)]
POLICIES = {"default": (256, (64, 64)), "BO": (512, (128, 256, 512)), "unserved": (512, (128, 256))}

# one piece of every text the sweeps reach
FRAGMENTS = (
    "wingman_driver must be 'none' or 'snapshot', not 'latest'", "PPOConfig.wingman_bf16 is the wingman driver's forward",
    "PPO drives the agent only", "no caller-driven pursuer", "pass wingman_policy with wingman_driver='none'",
    "PPO's wingman driver runs the HIP kernels of te_drive_wingman: it needs a GPU device",
    "fused_update_wide widens fused_update to every served shape: it needs fused_update",
    "fused_update_bf16 is fused_update's call with bf16 operands: it needs fused_update", "serves the default shape only",
    "hidden [128, 256] is not served with features_dim 512", "PPOConfig.fused_forward runs the HIP kernel te_policy_act: it needs a GPU device",
    "PPOConfig.fused_optimizer runs", "PPOConfig.fused_update runs", "PPOConfig.fused_advantages runs",
    "fused_forward_bf16 is fused_forward's launch with bf16 operands: it needs fused_forward",
    "fused_optimizer steps on te_policy_ppo_grad's packed gradient: it needs fused_update")


def _outcome(make):
    """None when make() returns, else [the exception's type, its full text]."""
    try:
        make()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None


def _sweep():
    """([(label, outcome, env.reset() calls)] of every PPO(...) case, [(label, outcome)] of every PPOConfig(...) case), in a fixed order."""
    from _policy_cases import StubEnv
    from dronechase_amd.ppo import PPO, LidarInertialActionPolicy, PPOConfig
    policies = {k: LidarInertialActionPolicy(features_dim=f, net_arch=arch) for k, (f, arch) in POLICIES.items()}
    wingman = LidarInertialActionPolicy()
    ppo = []
    for task, driver, sync, given, shape in itertools.product(("stage03", "exp05", None), ("none", "snapshot", "latest"), (1, 0), (False, True),
                                                              POLICIES):
        env = StubEnv(task)
        for subset in SUBSETS:
            cfg = PPOConfig(n_steps=2)
            cfg.wingman_driver, cfg.wingman_sync_every = driver, sync
            for s in subset:
                setattr(cfg, s, True)
            env.resets = 0
            out = _outcome(lambda: PPO(env, cfg, policy=policies[shape], wingman_policy=wingman if given else None))
            ppo.append((f"{task} {driver} sync={sync} wingman_policy={given} {shape} {'+'.join(subset)}", out, env.resets))
    config = [("+".join(subset), _outcome(lambda: PPOConfig(**{s: True for s in subset}))) for subset in SUBSETS]
    return ppo, config


def _record(path):
    ppo, config = _sweep()
    assert len(ppo) == N_CASES and len(config) == N_CONFIG_CASES and len({k for k, _, _ in ppo}) == N_CASES
    outcomes = [None] + sorted({json.dumps(o) for _, o, _ in ppo if o} | {json.dumps(o) for _, o in config if o})      # 0: accepted
    at = lambda o: outcomes.index(json.dumps(o)) if o else 0
    rows = [ppo[i:i + len(SUBSETS)] for i in range(0, N_CASES, len(SUBSETS))]      # one line per env, driver and policy: its 176 subsets
    with open(path, "w") as f:
        f.write('{"outcomes": [null,\n' + ",\n".join(outcomes[1:]) + '],\n"ppo": [\n' +
                ",\n".join(",".join(str(at(o)) for _, o, _ in row) for row in rows) + '],\n"config": [' +
                ",".join(str(at(o)) for _, o in config) + "]}\n")
    late = sum(1 for _, o, resets in ppo if o and resets)
    print(f"{N_CASES} PPO cases, {sum(1 for _, o, _ in ppo if o is None)} accepted, {late} refused after env.reset(); "
          f"{len(outcomes) - 1} distinct refusals -> {path}")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_every_refusal_is_the_recorded_one_and_leaves_the_env_alone(lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    texts = [o[1] for o in golden["outcomes"][1:]]
    for fragment in FRAGMENTS:
        assert any(fragment in t for t in texts), fragment
    assert len(golden["ppo"]) == N_CASES and golden["ppo"].count(0) == N_ACCEPTED and len(golden["config"]) == N_CONFIG_CASES
    ppo, config = _sweep()
    assert len(ppo) == N_CASES and len(config) == N_CONFIG_CASES
    wrong = [(k, o, golden["outcomes"][i]) for (k, o, _), i in zip(ppo, golden["ppo"]) if o != golden["outcomes"][i]]
    assert not wrong, (len(wrong), wrong[:5])
    wrong = [(k, o, golden["outcomes"][i]) for (k, o), i in zip(config, golden["config"]) if o != golden["outcomes"][i]]
    assert not wrong, (len(wrong), wrong[:5])
    touched = [k for k, o, resets in ppo if o and resets]
    assert not touched, (len(touched), touched[:5])
    assert all(resets == 1 for _, o, resets in ppo if o is None)      # an accepted PPO(...) resets its env, once


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    _record(sys.argv[2])
