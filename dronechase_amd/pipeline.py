"""Mirror of ReinforcementLearningPipeline.create_vectorized_environment
(src/core/rl_framework/utils/pipeline.py:31-61): same arguments and kwarg white-list, but returns ONE
batched GPU VecEnv instead of VecMonitor(SubprocVecEnv([env]*n)); and of its evaluate (pipeline.py:374-414) over the
on-device evaluate_policy of monitor.py.  `episode_monitor=True` (forwarded to ThreatEngageVecEnv) is VecMonitor's
infos[i]["episode"] without stable-baselines3."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .envs import ENV_TASKS
from .vec_env import ThreatEngageVecEnv


class ReinforcementLearningPipeline:
    @staticmethod
    def create_vectorized_environment(environment, env_kwargs: Optional[dict] = None, n_envs: int = os.cpu_count() or 1,
                                      GUI: bool = False, env_args=None, device: str = "cuda:0", monitor: bool = True,
                                      **vec_kwargs):
        env_kwargs = dict(env_kwargs or {})
        n_envs = n_envs if not GUI else 1
        env_kwargs["GUI"] = GUI
        env_args = ["dome_radius", "rl_frequency", "GUI"] if env_args is None else env_args
        valid = {k: v for k, v in env_kwargs.items() if k in env_args}
        task = ENV_TASKS.get(environment, environment if isinstance(environment, str) else None)
        if task is None:
            raise ValueError(f"{environment!r} is not one of the environments of this hot path: {sorted(c.__name__ for c in ENV_TASKS)}")
        venv = ThreatEngageVecEnv(task=task, num_envs=n_envs, device=device, **valid, **vec_kwargs)
        if monitor:
            try:  # VecMonitor wraps any VecEnv (pipeline.py:61); optional because SB3 may be absent
                from stable_baselines3.common.vec_env import VecMonitor  # type: ignore
                return VecMonitor(venv)
            except Exception:
                pass
        return venv

    @staticmethod
    def evaluate(model, env, n_eval_episodes: int = 100, deterministic: bool = True):
        """(avg_reward, std_dev, n_eval_episodes, episode_rewards) over exactly n_eval_episodes episodes of `env` (reset first) flown
        by `model` (anything monitor.evaluate_policy takes): the mean and np.std (ddof 0) of the raw episode returns."""
        from .monitor import evaluate_policy

        episode_rewards, _ = evaluate_policy(model, env, n_eval_episodes=n_eval_episodes, deterministic=deterministic)
        avg_reward, std_dev = float(np.mean(episode_rewards, dtype=np.float64)), float(np.std(episode_rewards, dtype=np.float64))
        return avg_reward, std_dev, n_eval_episodes, episode_rewards
