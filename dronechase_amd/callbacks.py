"""Training callbacks for PPO.learn: the reference's callback_factory.callbacklist (src/core/rl_framework/utils/callback_factory.py:59-120:
EvalCallback with best_model_save_path, StopTrainingOnNoModelImprovement(3, 5) chained behind it, CheckpointCallback) without
stable-baselines3.

What differs from SB3, on purpose:
  * a callback is consulted once per ITERATION (after update()), not once per VecEnv.step, and frequencies are in TIMESTEPS: a
    callback fires at the first iteration boundary where PPO.num_timesteps has advanced by at least its frequency since it last
    fired (at the start: since learn() was first given it).  SB3 counts VecEnv.step calls, so the reference's save_freq=100_000 with
    65 536 envs would be 6.5 G timesteps; here it is 100 000, i.e. every iteration of a rollout that large;
  * EvalCallback evaluates on a SEPARATE env (PPO.evaluate refuses the training env: evaluating there would reset it mid-rollout);
  * the best model is the SB3-named policy zip of save_sb3_policy, checkpoints are PPO.save files (.pt), not SB3 model zips;
  * every callback has state_dict() / load_state_dict(): PPO.save stores the state of the callback learn() was last given and
    PPO.load(..., callback=...) restores it into one of the same classes in the same order, so a resumed run evaluates, stops and
    checkpoints where the uninterrupted run would have;
  * there is no progress bar.

In a CallbackList put the CheckpointCallback LAST: the file it writes holds the state of the whole list at that moment, and a
callback that fires after it in the same iteration would fire again after a resume."""
from __future__ import annotations

import os
from enum import Enum
from typing import List, Optional

import numpy as np
import torch


class BaseCallback:
    """on_iteration() -> bool after every update(); False ends learn().  `model` is the PPO, `parent` the callback this one is chained
    behind (EvalCallback's callback_after_eval).  n_calls counts the consultations."""

    def __init__(self):
        self.model, self.parent, self.n_calls = None, None, 0

    def init_callback(self, model) -> None:
        self.model = model

    def on_iteration(self) -> bool:
        self.n_calls += 1
        return bool(self._on_iteration())

    def _on_iteration(self) -> bool:
        return True

    def _own_state(self) -> dict:
        return {}

    def _load_own_state(self, state: dict) -> None:
        pass

    def state_dict(self) -> dict:
        """Numbers, strings, lists, dicts and CPU tensors only (what torch.load(weights_only=True) reads)."""
        return {"class": type(self).__name__, "n_calls": int(self.n_calls), **self._own_state()}

    def check_state(self, state) -> None:
        """A ValueError unless `state` is the state_dict() of a callback of this class (and, for the composite ones, of the same
        classes in the same order below it).  Reads only."""
        theirs = state.get("class") if isinstance(state, dict) else None
        if theirs != type(self).__name__:
            raise ValueError(f"callback state of a {theirs!r} cannot be loaded into a {type(self).__name__}: "
                             "PPO.load(callback=...) takes the same classes in the same order as the saved run's")

    def load_state_dict(self, state: dict) -> None:
        self.check_state(state)
        self.n_calls = int(state["n_calls"])
        self._load_own_state(state)


class _EveryTimesteps(BaseCallback):
    """Fires _fire() at the first iteration boundary where num_timesteps has advanced by at least `freq` since it last did."""

    def __init__(self, freq: int):
        super().__init__()
        if int(freq) <= 0:
            raise ValueError(f"{type(self).__name__}: the frequency must be a positive number of timesteps, not {freq!r}")
        self.freq, self.last_fired = int(freq), None

    def init_callback(self, model) -> None:
        super().init_callback(model)
        if self.last_fired is None:         # a restored state keeps its own
            self.last_fired = int(model.num_timesteps)

    def _on_iteration(self) -> bool:
        now = int(self.model.num_timesteps)
        if now - self.last_fired < self.freq:
            return True
        self.last_fired = now               # before firing: a checkpoint written by _fire holds the state after it
        return self._fire()

    def _fire(self) -> bool:
        return True

    def _own_state(self) -> dict:
        return {"last_fired": self.last_fired}

    def _load_own_state(self, state: dict) -> None:
        self.last_fired = None if state["last_fired"] is None else int(state["last_fired"])


class EvalCallback(_EveryTimesteps):
    """Every eval_freq timesteps: PPO.evaluate over n_eval_episodes episodes of eval_env (a BatchedEnv or ThreatEngageVecEnv other
    than the training env; it is reset each time), then
      * log_path/evaluations.npz rewritten with SB3's keys: timesteps [E], results [E, n_eval_episodes], ep_lengths [E, n_eval_episodes];
      * when the mean return exceeds best_mean_reward (initially -inf): best_model_save_path/best_model.zip through PPO.save_policy;
      * callback_after_eval consulted (its `parent` is this object); False from it ends training.
    deterministic=True draws nothing from any torch generator, on the fused path and on the module path, so evaluating does not move
    a run off the trajectory it would resume on.  The state holds the history, best_mean_reward and the evaluation env's state blob:
    te_reset derives an episode's draws from the env's episode counter, so the k-th evaluation of a resumed run sees the episodes it
    would have seen."""

    def __init__(self, eval_env, n_eval_episodes: int = 5, eval_freq: int = 10_000, best_model_save_path: Optional[str] = None,
                 log_path: Optional[str] = None, deterministic: bool = True, callback_after_eval: Optional[BaseCallback] = None):
        super().__init__(eval_freq)
        if int(n_eval_episodes) <= 0:
            raise ValueError("EvalCallback: n_eval_episodes must be positive")
        self.eval_env, self.n_eval_episodes, self.eval_freq = eval_env, int(n_eval_episodes), int(eval_freq)
        self.best_model_save_path, self.log_path, self.deterministic = best_model_save_path, log_path, bool(deterministic)
        self.callback_after_eval = callback_after_eval
        if callback_after_eval is not None:
            callback_after_eval.parent = self
        self.best_mean_reward, self.last_mean_reward = float("-inf"), float("-inf")
        self.evaluations_timesteps: List[int] = []
        self.evaluations_results: List[np.ndarray] = []
        self.evaluations_length: List[np.ndarray] = []

    def init_callback(self, model) -> None:
        super().init_callback(model)
        if self.callback_after_eval is not None:
            self.callback_after_eval.init_callback(model)

    def _fire(self) -> bool:
        returns, lengths = self.model.evaluate(self.eval_env, n_eval_episodes=self.n_eval_episodes, deterministic=self.deterministic)
        self.evaluations_timesteps.append(int(self.model.num_timesteps))
        self.evaluations_results.append(np.asarray(returns, dtype=np.float32).reshape(self.n_eval_episodes))
        self.evaluations_length.append(np.asarray(lengths, dtype=np.int32).reshape(self.n_eval_episodes))
        if self.log_path is not None:
            os.makedirs(self.log_path, exist_ok=True)
            np.savez(os.path.join(self.log_path, "evaluations.npz"), **self.evaluations())
        self.last_mean_reward = float(np.mean(self.evaluations_results[-1], dtype=np.float64))
        if self.last_mean_reward > self.best_mean_reward:
            self.best_mean_reward = self.last_mean_reward
            if self.best_model_save_path is not None:
                os.makedirs(self.best_model_save_path, exist_ok=True)
                self.model.save_policy(os.path.join(self.best_model_save_path, "best_model.zip"))
        return True if self.callback_after_eval is None else self.callback_after_eval.on_iteration()

    def evaluations(self) -> dict:
        """The arrays of evaluations.npz."""
        n = self.n_eval_episodes
        return {"timesteps": np.asarray(self.evaluations_timesteps, dtype=np.int64),
                "results": np.asarray(self.evaluations_results, dtype=np.float32).reshape(-1, n),
                "ep_lengths": np.asarray(self.evaluations_length, dtype=np.int32).reshape(-1, n)}

    def _own_state(self) -> dict:
        backend = getattr(self.eval_env, "backend", self.eval_env)
        state = super()._own_state()
        state.update({k: torch.from_numpy(v.copy()) for k, v in self.evaluations().items()})
        state.update(n_eval_episodes=self.n_eval_episodes, best_mean_reward=float(self.best_mean_reward),
                     last_mean_reward=float(self.last_mean_reward),
                     eval_env_state=backend.get_state().cpu() if hasattr(backend, "get_state") else None,
                     callback_after_eval=None if self.callback_after_eval is None else self.callback_after_eval.state_dict())
        return state

    def check_state(self, state) -> None:
        super().check_state(state)
        if int(state["n_eval_episodes"]) != self.n_eval_episodes:
            raise ValueError(f"EvalCallback: the saved history has {int(state['n_eval_episodes'])} episodes per evaluation, this callback "
                             f"{self.n_eval_episodes}")
        child = state["callback_after_eval"]
        if (child is None) != (self.callback_after_eval is None):
            raise ValueError("EvalCallback: callback_after_eval is " + ("absent from" if child is None else "present in") +
                             " the saved state and " + ("absent" if self.callback_after_eval is None else "present") + " here")
        if child is not None:
            self.callback_after_eval.check_state(child)

    def _load_own_state(self, state: dict) -> None:
        super()._load_own_state(state)
        self.evaluations_timesteps = [int(t) for t in state["timesteps"].tolist()]
        self.evaluations_results = [r.copy() for r in state["results"].numpy()]
        self.evaluations_length = [r.copy() for r in state["ep_lengths"].numpy()]
        self.best_mean_reward, self.last_mean_reward = float(state["best_mean_reward"]), float(state["last_mean_reward"])
        backend = getattr(self.eval_env, "backend", self.eval_env)
        if state["eval_env_state"] is not None and hasattr(backend, "set_state"):
            backend.set_state(state["eval_env_state"])
        if self.callback_after_eval is not None:
            self.callback_after_eval.load_state_dict(state["callback_after_eval"])


class StopTrainingOnNoModelImprovement(BaseCallback):
    """Behind an EvalCallback (callback_after_eval): stop when the best mean return has not improved for too many evaluations.  At
    every call, i.e. after every evaluation: if the parent's best_mean_reward is greater than the value remembered from the previous
    call, the count of evaluations without improvement goes to 0; otherwise it increases by one, and training stops when
    n_calls > min_evals and the count > max_no_improvement_evals.  Then the parent's best_mean_reward is remembered.
    The count runs from the first evaluation on, min_evals only holds the stop back: with (3, 5) a run that never improves after its
    first evaluation stops at evaluation 6.  (SB3 is not installed here to compare with; its published callback appears to leave the
    count alone during the first min_evals calls, which would stop the same run at evaluation 9.  Unpinned.)"""

    def __init__(self, max_no_improvement_evals: int, min_evals: int = 0):
        super().__init__()
        self.max_no_improvement_evals, self.min_evals = int(max_no_improvement_evals), int(min_evals)
        self.last_best_mean_reward, self.no_improvement_evals = float("-inf"), 0

    def _on_iteration(self) -> bool:
        if self.parent is None:
            raise ValueError("StopTrainingOnNoModelImprovement reads its parent's best_mean_reward: give it to an EvalCallback as callback_after_eval")
        go_on = True
        if self.parent.best_mean_reward > self.last_best_mean_reward:
            self.no_improvement_evals = 0
        else:
            self.no_improvement_evals += 1
            go_on = not (self.n_calls > self.min_evals and self.no_improvement_evals > self.max_no_improvement_evals)
        self.last_best_mean_reward = float(self.parent.best_mean_reward)
        return go_on

    def _own_state(self) -> dict:
        return {"last_best_mean_reward": float(self.last_best_mean_reward), "no_improvement_evals": int(self.no_improvement_evals)}

    def _load_own_state(self, state: dict) -> None:
        self.last_best_mean_reward, self.no_improvement_evals = float(state["last_best_mean_reward"]), int(state["no_improvement_evals"])


class CheckpointCallback(_EveryTimesteps):
    """Every save_freq timesteps: PPO.save to save_path/{name_prefix}_{num_timesteps}_steps.pt, a full checkpoint that PPO.load
    resumes bit for bit (the state of the callback list included).

    What it costs, measured on the MI355X at the size people train at (stage03 x 65 536 envs, features_dim 512 with net_arch
    (128, 256, 512), n_steps 32, batch_size 32 768, 4 epochs, every fused switch on; tools/ppo_checkpoint_bench.py,
    profiles/ppo_checkpoint.json): one save() takes 0.262 s (median of 5; 0.189 to 0.267 s) and writes 452.9 MB (the next
    rollout's observation 271 MB, the env's state blob 171 MB, the learner and Adam 11 MB), while one learn() iteration of 2 097 152
    timesteps with no checkpoint takes 0.389 s (0.388 to 0.389 s) in the same process: a save costs 0.67 of an iteration.  THAT IS
    NOT A FEW PERCENT: a checkpoint every iteration would slow training by two thirds.  save() is synchronous: it copies the state
    to the host and writes the file before learn() goes on, and there is no asynchronous path.  Choose save_freq so that a save is
    rare against the iterations between two of them: every 50 iterations (about 100 M timesteps at this size) it costs 1.3 %."""

    def __init__(self, save_freq: int, save_path: str, name_prefix: str = "rl_model"):
        super().__init__(save_freq)
        self.save_freq, self.save_path, self.name_prefix = int(save_freq), save_path, name_prefix

    def checkpoint_path(self, num_timesteps: int) -> str:
        return os.path.join(self.save_path, f"{self.name_prefix}_{int(num_timesteps)}_steps.pt")

    def _fire(self) -> bool:
        os.makedirs(self.save_path, exist_ok=True)
        self.model.save(self.checkpoint_path(self.model.num_timesteps))
        return True


class CallbackList(BaseCallback):
    """Every callback is consulted, in order, at every iteration; training goes on only if all of them say so."""

    def __init__(self, callbacks: List[BaseCallback]):
        super().__init__()
        self.callbacks = list(callbacks)

    def init_callback(self, model) -> None:
        super().init_callback(model)
        for cb in self.callbacks:
            cb.init_callback(model)

    def _on_iteration(self) -> bool:
        go_on = True
        for cb in self.callbacks:
            go_on = cb.on_iteration() and go_on
        return go_on

    def _own_state(self) -> dict:
        return {"callbacks": [cb.state_dict() for cb in self.callbacks]}

    def check_state(self, state) -> None:
        super().check_state(state)
        theirs, mine = [s.get("class") for s in state["callbacks"]], [type(cb).__name__ for cb in self.callbacks]
        if theirs != mine:
            raise ValueError(f"CallbackList: the saved list is {theirs}, this one {mine}: PPO.load(callback=...) takes the same classes in the same order")
        for cb, s in zip(self.callbacks, state["callbacks"]):
            cb.check_state(s)

    def _load_own_state(self, state: dict) -> None:
        for cb, s in zip(self.callbacks, state["callbacks"]):
            cb.load_state_dict(s)


class CallbackType(Enum):
    EVAL = "eval"
    CHECKPOINT = "checkpoint"
    PROGRESSBAR = "progressbar"     # accepted for the reference's call sites and ignored: there is no progress bar


def callbacklist(env, log_path: str = "./logs/", model_path: str = "./models/", save_freq: int = 100_000,
                 callbacks_to_include: Optional[List[CallbackType]] = None, n_eval_episodes: int = 10, debug: bool = False) -> CallbackList:
    """The reference's callbacklist with its argument names: an EvalCallback on `env` every save_freq TIMESTEPS (best model into
    model_path, evaluations.npz into log_path, StopTrainingOnNoModelImprovement(max_no_improvement_evals=3, min_evals=5) behind it),
    then a CheckpointCallback every save_freq timesteps into model_path.  `env` is the EVALUATION env: a separate one, not the
    training env the reference passes.  `debug` is accepted and unused (nothing here prints)."""
    if callbacks_to_include is None:
        callbacks_to_include = [CallbackType.EVAL, CallbackType.CHECKPOINT]
    if not isinstance(save_freq, int) or save_freq <= 0:
        raise ValueError("callbacklist: save_freq must be a positive integer (timesteps)")
    out: List[BaseCallback] = []
    if CallbackType.EVAL in callbacks_to_include:
        stop = StopTrainingOnNoModelImprovement(max_no_improvement_evals=3, min_evals=5)
        out.append(EvalCallback(env, n_eval_episodes=n_eval_episodes, eval_freq=save_freq, best_model_save_path=model_path,
                                log_path=log_path, deterministic=True, callback_after_eval=stop))
    if CallbackType.CHECKPOINT in callbacks_to_include:
        out.append(CheckpointCallback(save_freq=save_freq, save_path=model_path))
    return CallbackList(out)
