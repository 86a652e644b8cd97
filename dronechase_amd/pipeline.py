"""Mirror of ReinforcementLearningPipeline.create_vectorized_environment
(src/core/rl_framework/utils/pipeline.py:31-61): same arguments and kwarg white-list, but returns ONE
batched GPU VecEnv instead of VecMonitor(SubprocVecEnv([env]*n)); and of its evaluate (pipeline.py:374-414) over the
on-device evaluate_policy of monitor.py; and of its create_callback_list / train_model / save_model (pipeline.py:122-149, 302-341) over
callbacks.py and PPO.save.  `episode_monitor=True` (forwarded to ThreatEngageVecEnv) is VecMonitor's
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

    @staticmethod
    def create_callback_list(vectorized_environment, model_dir: str, log_dir: str, callbacks_to_include=None, n_eval_episodes: int = 10,
                             debug: bool = False, steps: int = 1_000_000, step_size_save: int = 100_000):
        """pipeline.py:122-149 with its arguments: callbacks.callbacklist evaluating and checkpointing every step_size_save TIMESTEPS
        (steps // 10 when the whole run is no longer than that).  `vectorized_environment` is the EVALUATION env, a separate one from
        the env the model trains on (callbacks.py says why, and why the frequency is in timesteps, not in VecEnv.step calls)."""
        from .callbacks import callbacklist

        save_freq = max(step_size_save if steps > step_size_save else steps // 10, 1)
        return callbacklist(vectorized_environment, log_path=log_dir, model_path=model_dir, save_freq=int(save_freq),
                            callbacks_to_include=callbacks_to_include, n_eval_episodes=n_eval_episodes, debug=debug)

    @staticmethod
    def train_model(model, callback_list, n_timesteps: int = 1_000_000):
        """pipeline.py:302-306: model.learn(total_timesteps=n_timesteps, callback=callback_list); `model` is a ppo.PPO."""
        model.learn(total_timesteps=n_timesteps, callback=callback_list)
        return model

    @staticmethod
    def save_model(model, hidden_layers, rl_frequency: int, learning_rate: float, avg_reward: float, reward_std_dev: float,
                   models_dir: str, debug: bool = False, trial_number: int = 0) -> str:
        """pipeline.py:318-341 with its arguments and its file naming: models_dir/h{hidden_layers}_f{rl_frequency}_lr{learning_rate}/
        t{trial_number}_PPO_r{avg_reward:.2f} as TWO files: .pt, the full checkpoint of PPO.save (what PPO.load resumes or fine-tunes
        from), and .zip, the SB3-named policy of PPO.save_policy (what a user of the reference loads into a model of theirs).
        Returns the .pt path.  reward_std_dev and debug are accepted and unused, as in the reference."""
        folder = os.path.join(models_dir, f"h{list(hidden_layers)}_f{rl_frequency}_lr{learning_rate}")
        os.makedirs(folder, exist_ok=True)
        stem = os.path.join(folder, f"t{trial_number}_{type(model).__name__}_r{avg_reward:.2f}")
        model.save(stem + ".pt")
        model.save_policy(stem + ".zip")
        return stem + ".pt"
