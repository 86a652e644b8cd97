"""On-device PPO for the batched environments (BASELINE.json config 5).

The reference trains SB3 PPO (`MultiInputPolicy` + `LidarInertialActionExtractor`,
src/core/rl_framework/agents/policies/ppo_policies.py:234-341; apps/threatengage_runner/stage03/...) against
`SubprocVecEnv`, i.e. every observation crosses process pipes and PCIe.  stable-baselines3 is not installed here, and
with 65 536 environments per GPU the rollout buffer is the thing to keep on the device: this module is a plain-PyTorch
PPO whose rollout storage, advantage estimation and minibatches never leave HBM (a 128-step rollout of 65 536 stage03
envs is 34 GB of observations — 288 GB per MI355X is what makes that layout possible).  PyTorch-ROCm is used for
autograd and the dense layers (rocBLAS/MIOpen): the environment side stays the HIP kernels of libthreatengage.so.

  * topology = the reference's extractor: LIDAR conv(k4,s4,32) -> conv(k2,s2,64) -> flatten; inertial and
    last_action 3 x Linear(128); concat -> Linear(features_dim); then pi / vf heads of net_arch widths with tanh (SB3's default
    2 x 64 and features_dim 256 unless told otherwise; the reference's trained networks are features_dim 512 with net_arch
    (128, 256, 512) or (512, 128, 256): load_sb3_policy below reads their checkpoints) and a state-independent log-std;
  * losses / GAE = the PPO of Schulman et al. 2017 with SB3's defaults (clip 0.2, gae_lambda 0.95, gamma 0.99,
    vf_coef 0.5, ent_coef 0, max_grad_norm 0.5, advantage normalisation per minibatch, 10 epochs);
  * PPOConfig.fused_forward: the rollout's forward, sampling and log-prob in one HIP launch (te_policy_act, FusedPolicy below)
    instead of ~40 PyTorch launches per step;
  * PPOConfig.fused_update: the minibatch's loss gradient in one ABI call (te_policy_ppo_grad, FusedPolicy.ppo_grad) instead of
    the PyTorch forward + autograd, reading the rollout rows through the minibatch index (no gather of the observations);
  * PPOConfig.fused_optimizer: gradient clipping and Adam in one ABI call (te_policy_adam_step, PackedAdam) on the packed buffer the
    kernels read, which the module's parameters are then views of (FusedPolicy.bind_parameters): no repack between minibatches;
  * PPOConfig.fused_advantages: GAE as one HIP launch over the whole rollout (te_rollout_gae, RolloutBuffer.finish(fused=True))
    instead of ~9 PyTorch launches per step, the minibatch's advantage mean and std as one te_adv_stats call (adv_stats below)
    into the two floats te_policy_ppo_grad reads, and "explained_variance" in update()'s log;
  * PPOConfig.wingman_driver / PPO(wingman_policy=...): exp05's ally (and the evaluation task's "nn" drivers) flown by a frozen
    policy inside the rollout, one te_drive_wingman call per caller-driven pursuer before every te_step (PPOConfig.wingman_bf16:
    te_drive_wingman_bf16, the bf16 MFMA forward in front of the same clamp and drive);
  * PPOConfig.episode_stats / PPO.evaluate: episode returns, lengths and final info rows accumulated on the device (monitor.py,
    te_monitor_step), and SB3's evaluate_policy over a separate evaluation env;
  * PPO.save / PPO.load: one torch.save file of plain data from which a run continues bit for bit on an env of the same config, or
    fine-tunes on another task (restore_env=False); PPO.save_policy / save_sb3_policy: the weights under SB3's names, load_sb3_policy's
    inverse; PPO.learn(callback=): the reference's evaluation, early-stop and checkpoint callbacks (callbacks.py);
  * multi-GPU: one process per GPU, each with its own env shard; gradients are averaged with
    torch.distributed all_reduce (RCCL) — the only collective of the whole system, once per minibatch.
"""
from __future__ import annotations

import copy
from dataclasses import asdict, dataclass, fields
from typing import Dict, List, Optional, Tuple

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from . import config as K
from ._lib import _ptr, require_f32, require_index    # require_f32: also this module's name for it (the callers' import)


class LidarInertialActionPolicy(nn.Module):
    """Actor-critic over {"lidar" [B,C,13,26], "inertial_data" [B,15], "last_action" [B,4]}.  net_arch: the widths of the 1-3 hidden
    layers (Linear + Tanh each) of the pi head and of the vf head, the reference's net_arch=dict(pi=hiddens, vf=hiddens)."""

    def __init__(self, lidar_shape=(3, 13, 26), inertial_dim: int = 15, action_dim: int = 4, features_dim: int = 256, net_arch=(64, 64)):
        super().__init__()
        net_arch = tuple(int(w) for w in net_arch)
        if not 1 <= len(net_arch) <= 3 or min(net_arch) < 1:
            raise ValueError(f"LidarInertialActionPolicy: net_arch must be 1 to 3 positive widths, not {net_arch}")
        c = lidar_shape[0]
        self.lidar = nn.Sequential(nn.Conv2d(c, 32, kernel_size=4, stride=4), nn.ReLU(),
                                   nn.Conv2d(32, 64, kernel_size=2, stride=2), nn.ReLU(), nn.Flatten())
        with torch.no_grad():
            n_lidar = self.lidar(torch.zeros(1, *lidar_shape)).shape[1]

        def mlp(n_in):
            return nn.Sequential(nn.Linear(n_in, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU())

        self.inertial, self.action = mlp(inertial_dim), mlp(action_dim)
        self.final = nn.Sequential(nn.Linear(n_lidar + 256, features_dim), nn.ReLU())

        def head():
            widths = (features_dim,) + net_arch
            return nn.Sequential(*(m for a, b in zip(widths, widths[1:]) for m in (nn.Linear(a, b), nn.Tanh())))

        self.pi, self.vf = head(), head()
        self.mu = nn.Linear(net_arch[-1], action_dim)
        self.value = nn.Linear(net_arch[-1], 1)
        self.log_std = nn.Parameter(torch.zeros(action_dim))

    def features(self, obs: Dict[str, torch.Tensor]) -> torch.Tensor:
        z = torch.cat((self.lidar(obs["lidar"]), self.inertial(obs["inertial_data"]), self.action(obs["last_action"])), dim=1)
        return self.final(z)

    def forward(self, obs):
        f = self.features(obs)
        return self.mu(self.pi(f)), self.value(self.vf(f)).squeeze(-1)

    def dist(self, obs):
        mu, v = self(obs)
        # validate_args=False: the argument check is a host synchronisation per call (and cannot be captured in a graph)
        return torch.distributions.Normal(mu, self.log_std.exp().expand_as(mu), validate_args=False), v


def _packed_order(policy: nn.Module):
    """The public layout of te_policy_act's parameter buffer (include/threatengage.h): the submodules' parameters in registration
    order, then log_std.  (parameters() itself yields log_std first: a module's own parameters precede its children's.)"""
    named = list(policy.named_parameters())
    return [p for n, p in named if n != "log_std"] + [policy.log_std]


@torch.no_grad()
def pack_policy(policy: nn.Module, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The policy's weights in te_policy_act's layout; into `out` in place (same storage) when given."""
    flat = [p.detach().reshape(-1).float() for p in _packed_order(policy)]
    return torch.cat(flat) if out is None else torch.cat(flat, out=out)


DEFAULT_FEATURES_DIM, DEFAULT_NET_ARCH = 256, (64, 64)


def policy_shape(policy: nn.Module) -> Tuple[int, int, Tuple[int, ...]]:
    """(lidar_channels, features_dim, net_arch) read from a LidarInertialActionPolicy's layers."""
    return (int(policy.lidar[0].in_channels), int(policy.final[0].out_features),
            tuple(int(m.out_features) for m in policy.pi if isinstance(m, nn.Linear)))


def _c_shape(lidar_channels: int, features_dim: int, net_arch) -> "_lib.PolicyShape":
    net_arch = tuple(int(w) for w in net_arch)
    # more than 3 widths cannot be written into the struct's 4 slots in full: n_hidden alone carries the count, and the check refuses it
    return _lib.PolicyShape(int(lidar_channels), int(features_dim), len(net_arch), (C.c_int32 * 4)(*(net_arch[:4])))


def check_policy_shape(lidar_channels: int, features_dim: int = DEFAULT_FEATURES_DIM, net_arch=DEFAULT_NET_ARCH) -> "_lib.PolicyShape":
    """The te_policy_shape of a shape the HIP kernels serve; a ValueError that lists the served shapes otherwise."""
    shape = _c_shape(lidar_channels, features_dim, net_arch)
    lib = _lib.load()
    if lib.te_policy_shape_check(C.byref(shape)) != 0:
        raise ValueError(lib.te_last_error().decode())
    return shape


def is_default_shape(features_dim: int, net_arch) -> bool:
    return int(features_dim) == DEFAULT_FEATURES_DIM and tuple(int(w) for w in net_arch) == DEFAULT_NET_ARCH


def policy_param_words(lidar_channels: int, features_dim: int = DEFAULT_FEATURES_DIM, net_arch=DEFAULT_NET_ARCH) -> int:
    """The words of the packed parameter buffer of a served shape (te_policy_param_words_shaped)."""
    shape = check_policy_shape(lidar_channels, features_dim, net_arch)
    out = C.c_size_t()
    _lib.call("te_policy_param_words_shaped", C.byref(shape), C.byref(out))
    return int(out.value)


# SB3's MultiInputPolicy names (stable-baselines3's ActorCriticPolicy; the extractor's attributes are the reference's,
# ppo_policies.py:245-256) -> this module's.  Taken from SB3's documentation, not checked against a checkpoint file.
_SB3_EXTRACTOR = {"lidar_feature_extractor": "lidar", "inertial_feature_extractor": "inertial", "action_feature_extractor": "action",
                  "final_layer": "final"}
_SB3_PREFIX = {"mlp_extractor.policy_net.": "pi.", "mlp_extractor.value_net.": "vf.", "action_net.": "mu.", "value_net.": "value."}


def _sb3_key(key: str) -> Optional[str]:
    """The module's name of SB3 state-dict key `key`; None for a key the module has no counterpart of."""
    if key == "log_std":
        return key
    if key.startswith("features_extractor."):
        attr, _, rest = key[len("features_extractor."):].partition(".")
        return f"{_SB3_EXTRACTOR[attr]}.{rest}" if attr in _SB3_EXTRACTOR and rest else None
    for pre, ours in _SB3_PREFIX.items():
        if key.startswith(pre):
            return ours + key[len(pre):]
    return None


def load_sb3_policy(path_or_state_dict, lidar_shape=(3, 13, 26)) -> LidarInertialActionPolicy:
    """A LidarInertialActionPolicy with the weights of an SB3 MultiInputPolicy checkpoint of the reference's extractor, without
    stable-baselines3: `path_or_state_dict` is the model's .zip (its policy.pth is read with torch.load(weights_only=True)) or the
    policy's state dict.  features_dim and net_arch are inferred from the tensors' shapes.  SB3 stores the extractor three times when
    it is shared (features_extractor, pi_features_extractor, vf_features_extractor): the copies must equal features_extractor's.
    Any other unknown key, and any key the module needs and the checkpoint lacks, is a KeyError naming it."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        import io
        import zipfile
        with zipfile.ZipFile(sd) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    mapped: Dict[str, torch.Tensor] = {}
    for key, t in sd.items():
        dup = next((d for d in ("pi_features_extractor.", "vf_features_extractor.") if key.startswith(d)), None)
        if dup is not None:
            shared = "features_extractor." + key[len(dup):]
            if _sb3_key(shared) is None:
                raise KeyError(f"load_sb3_policy: unknown key {key!r}")
            if shared in sd and not torch.equal(sd[shared], t):
                raise ValueError(f"load_sb3_policy: {key!r} differs from {shared!r}: the extractor is not shared, which this policy cannot express")
            if shared in sd:
                continue
            key = shared
        name = _sb3_key(key)
        if name is None:
            raise KeyError(f"load_sb3_policy: unknown key {key!r}")
        mapped[name] = t
    for need in ("final.0.weight", "pi.0.weight"):
        if need not in mapped:
            back = {"final.0.weight": "features_extractor.final_layer.0.weight", "pi.0.weight": "mlp_extractor.policy_net.0.weight"}[need]
            raise KeyError(f"load_sb3_policy: missing key {back!r}")
    net_arch = []
    while len(net_arch) < 3 and f"pi.{2 * len(net_arch)}.weight" in mapped:
        net_arch.append(int(mapped[f"pi.{2 * len(net_arch)}.weight"].shape[0]))
    policy = LidarInertialActionPolicy(lidar_shape=tuple(lidar_shape), features_dim=int(mapped["final.0.weight"].shape[0]), net_arch=tuple(net_arch))
    ours = policy.state_dict()
    back = {_sb3_key(k): k for k in sd if _sb3_key(k) is not None}
    for name in mapped:
        if name not in ours:
            raise KeyError(f"load_sb3_policy: unknown key {back.get(name, name)!r}")
    for name, t in ours.items():
        if name not in mapped:
            inv = {v: k for k, v in _SB3_EXTRACTOR.items()}
            head, _, rest = name.partition(".")
            sb3 = (f"features_extractor.{inv[head]}.{rest}" if head in inv else
                   next((pre + rest for pre, o in _SB3_PREFIX.items() if o == head + "."), name))
            raise KeyError(f"load_sb3_policy: missing key {sb3!r}")
        if tuple(mapped[name].shape) != tuple(t.shape):
            raise ValueError(f"load_sb3_policy: {back.get(name, name)!r} has shape {tuple(mapped[name].shape)}, the module's {name} {tuple(t.shape)}")
    policy.load_state_dict({k: mapped[k].float() for k in ours})
    return policy


def _to_sb3_keys(name: str) -> List[str]:
    """The SB3 state-dict keys of the module's parameter `name` (the inverse of _sb3_key): three for a parameter of the extractor,
    which SB3 stores once per owner when it is shared, one for every other."""
    if name == "log_std":
        return [name]
    head, _, rest = name.partition(".")
    inv = {v: k for k, v in _SB3_EXTRACTOR.items()}
    if head in inv:
        return [f"{pre}features_extractor.{inv[head]}.{rest}" for pre in ("", "pi_", "vf_")]
    return [next(pre for pre, ours in _SB3_PREFIX.items() if ours == head + ".") + rest]


def save_sb3_policy(policy: nn.Module, path) -> None:
    """The inverse of load_sb3_policy: a zip at `path` (a file name or a file object) whose policy.pth is the state dict of
    `policy` (a LidarInertialActionPolicy) under SB3's MultiInputPolicy key names, the extractor three times (features_extractor,
    pi_features_extractor, vf_features_extractor), CPU float32 tensors.  load_sb3_policy(path) gives the same parameters back, and a
    user of the reference reads it with model.policy.load_state_dict(torch.load(policy.pth)) on a model THEY construct: this is not a
    whole SB3 model zip (its `data` member holds cloudpickled SB3 objects, which nothing but SB3 can write).  The key names are taken
    from SB3's documentation, as load_sb3_policy's are."""
    import io
    import zipfile
    sd: Dict[str, torch.Tensor] = {}
    for name, t in policy.state_dict().items():
        host = t.detach().to("cpu", copy=True).contiguous()      # a bound parameter is a view of the packed buffer: no shared storage in the file
        for key in _to_sb3_keys(name):
            sd[key] = host
    blob = io.BytesIO()
    torch.save(sd, blob)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", blob.getvalue())


GRAD_DEFAULT_ONLY = ("the gradient kernel te_policy_ppo_grad serves the default shape only (features_dim 256, net_arch (64, 64)): "
                     "PPOConfig.fused_update and fused_optimizer are not available for this policy; without them update() runs autograd.  "
                     "PPOConfig.fused_update_wide (with fused_update) asks for te_policy_ppo_grad_shaped, which serves every shape FusedPolicy does")


class FusedPolicy:
    """Inference of a LidarInertialActionPolicy by te_policy_act_shaped: the forward pass, the Gaussian sample, its log-prob and the
    clamp of the action in one HIP launch, for every shape the kernels serve (features_dim 256 with net_arch (64, 64); features_dim
    512 with (128, 256, 512) or (512, 128, 256)); any other shape is a ValueError that lists them.  The weights are packed into ONE device buffer that keeps its address for the life of
    this object; refresh() repacks the module's current weights into it in place, so a HIP graph that captured a call sees them.
    Call refresh() after every change of the module's weights (PPO does, at the start of every collect()).
    After bind_parameters() the module's parameters are views of the packed buffer and there is nothing left to repack.
    precision="bf16": forward and act go to te_policy_act_bf16 (bf16 operands on the bf16 MFMA, fp32 accumulation; the numerics
    contract is in include/threatengage.h).  The object then owns a second buffer, the weights rounded to bf16 (te_policy_pack_bf16),
    at a stable address too; refresh() repacks it with one more launch, also after bind_parameters().  BatchedEnv.drive_wingman follows
    `precision` too: a bf16 object flies its pursuer through te_drive_wingman_bf16 (PPOConfig.wingman_bf16).  precision does not touch
    ppo_grad.
    grad_precision="bf16": ppo_grad goes to te_policy_ppo_grad_bf16 (the same contract, extended to the backward), whose forward is
    bitwise te_policy_act_bf16's.  The object then owns weights_bf16 (shared with precision="bf16") and weights_bf16_t, the transposed
    rounded weights (te_policy_pack_bf16_grad), both at stable addresses and both repacked by refresh(), also when bound.  forward,
    act and BatchedEnv.drive_wingman follow `precision` alone: precision="fp32", grad_precision="bf16" keeps the fp32 forward."""

    def __init__(self, policy: nn.Module, precision: str = "fp32", grad_precision: str = "fp32"):
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"FusedPolicy: precision must be 'fp32' or 'bf16', not {precision!r}")
        if grad_precision not in ("fp32", "bf16"):
            raise ValueError(f"FusedPolicy: grad_precision must be 'fp32' or 'bf16', not {grad_precision!r}")
        self.precision, self.grad_precision = precision, grad_precision
        self.policy = policy
        self.lidar_channels, self.features_dim, self.net_arch = policy_shape(policy)
        params = _packed_order(policy)
        self.device = params[0].device
        if self.device.type != "cuda":
            raise ValueError("FusedPolicy runs the HIP kernel te_policy_act: the policy must live on a GPU")
        self.shape = check_policy_shape(self.lidar_channels, self.features_dim, self.net_arch)    # the te_policy_shape of every call
        words = policy_param_words(self.lidar_channels, self.features_dim, self.net_arch)
        if sum(p.numel() for p in params) != words:
            raise ValueError(f"policy has {sum(p.numel() for p in params)} parameters, te_policy_act's layout {words}: not a LidarInertialActionPolicy")
        self.params = torch.empty(words, dtype=torch.float32, device=self.device)
        self.weights_bf16 = self.weights_bf16_t = None
        half = C.c_size_t()
        bf16, grad_bf16 = precision == "bf16", grad_precision == "bf16"
        if bf16 or grad_bf16:
            _lib.call("te_policy_bf16_words", C.byref(self.shape), C.byref(half))
            self.weights_bf16 = torch.empty(int(half.value), dtype=torch.int16, device=self.device)
        if grad_bf16:
            _lib.call("te_policy_bf16_grad_words", C.byref(self.shape), C.byref(half))
            self.weights_bf16_t = torch.empty(int(half.value), dtype=torch.int16, device=self.device)
        # the one place that tells fp32 from bf16: per kind of call the entry and its leading weight arguments.  A bf16 entry takes the
        # shaped entry's arguments with the rounded weights inserted after params (include/threatengage.h)
        fp32, rounded = (self.params,), (self.params, self.weights_bf16)
        self.act_entry = ("te_policy_act_bf16", rounded) if bf16 else ("te_policy_act_shaped", fp32)
        self.drive_entry = ("te_drive_wingman_bf16", rounded) if bf16 else ("te_drive_wingman_shaped", fp32)     # BatchedEnv.drive_wingman
        self.grad_entry = ("te_policy_ppo_grad_bf16", rounded + (self.weights_bf16_t,)) if grad_bf16 else ("te_policy_ppo_grad_shaped", fp32)
        self.grad_ws_entry = "te_policy_grad_bf16_workspace_bytes" if grad_bf16 else "te_policy_grad_workspace_bytes_shaped"
        self.bound = False
        self.refresh()

    def refresh(self) -> None:
        if not self.bound:      # bound: the parameters ARE the buffer (and torch.cat(out=) onto its own inputs raises)
            pack_policy(self.policy, out=self.params)
        if self.weights_bf16 is not None:       # the fp32 buffer is the master copy: round it again, in place, on the current stream
            _lib.call_on(self.device, "te_policy_pack_bf16", self.params.data_ptr(), C.byref(self.shape), self.weights_bf16.data_ptr())
        if self.weights_bf16_t is not None:
            _lib.call_on(self.device, "te_policy_pack_bf16_grad", self.params.data_ptr(), C.byref(self.shape), self.weights_bf16_t.data_ptr())

    @torch.no_grad()
    def bind_parameters(self) -> None:
        """Make every parameter of the module a view into the packed buffer, in _packed_order: from here on the buffer is the single
        copy of the weights.  What te_policy_adam_step (PackedAdam) writes into it is what the PyTorch module, state_dict(),
        te_policy_act and te_policy_ppo_grad read, and refresh() has nothing to do.  The offsets are multiples of 4 words except
        log_std's, one word off (PyTorch does not mind).  copy.deepcopy of a bound module gets storage of its own; a .to() or .float()
        that reallocates the parameters would detach them from the buffer: bind last."""
        if self.bound:
            return
        self.refresh()
        off = 0
        for p in _packed_order(self.policy):
            p.data = self.params[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.bound = True

    @torch.no_grad()
    def load_from(self, module: nn.Module) -> None:
        """Copy `module`'s weights into this object's policy and repack them in place (bound: the copy lands in the packed buffer
        through the views): the buffer keeps its address, so a
        HIP graph that captured a call flies the new weights.  A frozen snapshot of a learner is FusedPolicy(copy.deepcopy(learner))
        re-synced with load_from(learner)."""
        src, dst = _packed_order(module), _packed_order(self.policy)
        if len(src) != len(dst) or any(a.shape != b.shape for a, b in zip(src, dst)):
            raise ValueError("FusedPolicy.load_from: the module's parameters do not match this policy's layout")
        if module is not self.policy:
            for a, b in zip(src, dst):
                b.copy_(a)
        self.refresh()

    def ppo_grad(self, obs: Dict[str, torch.Tensor], index: Optional[torch.Tensor], action: torch.Tensor, old_logp: torch.Tensor,
                 adv: torch.Tensor, ret: torch.Tensor, adv_mean_std: Optional[torch.Tensor], clip: float, vf_coef: float,
                 ent_coef: float, grad_out: torch.Tensor, stats_out: torch.Tensor) -> None:
        """The gradient of PPO's loss over the minibatch rows `index` (int64 [B]; None: every row) of the rollout tensors obs,
        action [M, 4], old_logp, adv and ret [M], in the packed layout, into grad_out [te_policy_param_words] (16-byte aligned);
        stats_out [4] = pg, vl, ent, clip_frac.  adv_mean_std [2] (mean, unbiased std of adv over the minibatch) normalises the
        advantage; None uses it as it is.  One te_policy_ppo_grad_shaped call, for every shape FusedPolicy serves: three launches,
        no host synchronisation; for the default shape bitwise te_policy_ppo_grad.  The workspace (per row 17 280 B for the default
        shape, 31 616 B for features_dim 512 with net_arch (128, 256, 512) or (512, 128, 256), at 3 LIDAR channels; plus the split-K
        partials: 17.8 KB and 33.2 / 33.7 KB per row in all at 65 536 rows) is owned here and grows on demand, which a capturing stream does not allow:
        make the first call of a size outside capture.  grad_precision="bf16": one te_policy_ppo_grad_bf16 call instead, the same
        arguments and outputs, a workspace of about half the size."""
        lidar, inertial, last_action = obs["lidar"], obs["inertial_data"], obs["last_action"]
        m = lidar.shape[0]
        b = m if index is None else index.shape[0]
        checks = [("lidar", lidar, (m, self.lidar_channels, 13, 26)), ("inertial_data", inertial, (m, 15)), ("last_action", last_action, (m, 4)),
                  ("action", action, (m, 4)), ("old_logp", old_logp, (m,)), ("adv", adv, (m,)), ("ret", ret, (m,)),
                  ("adv_mean_std", adv_mean_std, (2,)), ("grad_out", grad_out, (self.params.numel(),)), ("stats_out", stats_out, (4,))]
        for name, t, shape in checks:
            if t is None:
                if name == "adv_mean_std":
                    continue
                raise ValueError(f"FusedPolicy.ppo_grad: {name} is required")
            require_f32("FusedPolicy.ppo_grad", name, t, shape, self.device)
        require_index("FusedPolicy.ppo_grad", index, self.device)
        if b == 0:
            raise ValueError("FusedPolicy.ppo_grad: the minibatch is empty")
        ws = self._grad_workspace("FusedPolicy.ppo_grad", b)
        entry, weights = self.grad_entry
        _lib.call_on(self.device, entry, *(w.data_ptr() for w in weights), C.byref(self.shape), b, _ptr(index), lidar.data_ptr(),
                     inertial.data_ptr(), last_action.data_ptr(), action.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                     _ptr(adv_mean_std), float(clip), float(vf_coef), float(ent_coef), grad_out.data_ptr(), stats_out.data_ptr(),
                     ws.data_ptr(), ws.numel())

    def _grad_workspace(self, who: str, rows: int) -> torch.Tensor:
        """The gradient workspace for minibatches of up to `rows` rows: owned here, grown on demand, never under capture."""
        need = C.c_size_t()
        _lib.call(self.grad_ws_entry, C.byref(self.shape), rows, C.byref(need))
        ws = getattr(self, "_grad_ws", None)
        if ws is None or ws.numel() < need.value:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{who}: the workspace must grow, which a capturing stream does not allow; "
                                   "call once with this minibatch size before capture")
            self._grad_ws = None           # free the old workspace before the larger one is allocated
            ws = self._grad_ws = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)
        return ws

    def ppo_epoch(self, obs: Dict[str, torch.Tensor], perm: torch.Tensor, batch: int, action: torch.Tensor, old_logp: torch.Tensor,
                  adv: torch.Tensor, ret: torch.Tensor, clip: float, vf_coef: float, ent_coef: float, grad_out: torch.Tensor,
                  opt: "PackedAdam", max_grad_norm: float, adv_workspace: torch.Tensor, adv_mean_std: torch.Tensor,
                  stats: torch.Tensor, sums: torch.Tensor, grad_scale: float = 1.0) -> None:
        """One epoch of PPO's update by ONE te_policy_ppo_epoch call: for every minibatch perm[s:s + batch] of the int64 row numbers
        `perm` (the last one may be shorter) the advantage statistics (adv_stats into adv_mean_std [2]), the gradient (ppo_grad's call
        into grad_out and stats [4]), `opt`'s clipped Adam step on this object's packed buffer, and sums [5] += (pg, vl, ent, clip_frac,
        the gradient's norm before clipping), enqueued back to back on PyTorch's current stream with no return to Python in between.
        Bitwise the same calls made one by one.  grad_precision="bf16": the bf16 gradient, and the step keeps weights_bf16 and
        weights_bf16_t current (te_policy_adam_step_bf16), so no refresh() is needed between the minibatches; they must be current
        when the call starts.  sums is added to, not cleared.  The gradient workspace is owned here, as ppo_grad's is;
        adv_workspace comes from adv_stats_workspace(n) with n >= batch."""
        who = "FusedPolicy.ppo_epoch"
        lidar, inertial, last_action = obs["lidar"], obs["inertial_data"], obs["last_action"]
        m = lidar.shape[0]
        for name, t, shape in (("lidar", lidar, (m, self.lidar_channels, 13, 26)), ("inertial_data", inertial, (m, 15)),
                               ("last_action", last_action, (m, 4)), ("action", action, (m, 4)), ("old_logp", old_logp, (m,)),
                               ("adv", adv, (m,)), ("ret", ret, (m,)), ("grad_out", grad_out, (self.params.numel(),)),
                               ("adv_mean_std", adv_mean_std, (2,)), ("stats", stats, (4,)), ("sums", sums, (5,))):
            require_f32(who, name, t, shape, self.device)
        if perm is None or perm.numel() == 0:
            raise ValueError(f"{who}: perm is required and must not be empty")
        require_index(who, perm, self.device)
        if opt.fused_policy is not self:
            raise ValueError(f"{who}: opt must be the PackedAdam of this FusedPolicy")
        if adv_workspace.dtype != torch.uint8 or adv_workspace.device != self.device or not adv_workspace.is_contiguous():
            raise ValueError(f"{who}: adv_workspace must be a contiguous uint8 tensor on {self.device} (adv_stats_workspace)")
        batch = int(batch)
        ws = self._grad_workspace(who, max(1, min(batch, perm.numel())))
        bf16 = self.weights_bf16_t is not None      # grad_precision == "bf16": the object owns both rounded copies
        a = _lib.PpoEpochArgs(
            struct_size=C.sizeof(_lib.PpoEpochArgs), shape=self.shape, params=self.params.data_ptr(),
            weights_bf16=self.weights_bf16.data_ptr() if bf16 else None, weights_bf16_t=self.weights_bf16_t.data_ptr() if bf16 else None,
            lidar=lidar.data_ptr(), inertial=inertial.data_ptr(), last_action=last_action.data_ptr(), action=action.data_ptr(),
            old_logp=old_logp.data_ptr(), adv=adv.data_ptr(), ret=ret.data_ptr(), perm=perm.data_ptr(), n_perm=perm.numel(), batch=batch,
            clip_range=float(clip), vf_coef=float(vf_coef), ent_coef=float(ent_coef), grad=grad_out.data_ptr(),
            state=opt.state.data_ptr(), state_bytes=opt.state.numel() * 4, lr=opt.lr, beta1=opt.betas[0], beta2=opt.betas[1], eps=opt.eps,
            max_grad_norm=float(max_grad_norm), grad_scale=float(grad_scale), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
            adv_workspace=adv_workspace.data_ptr(), adv_workspace_bytes=adv_workspace.numel(), adv_mean_std=adv_mean_std.data_ptr(),
            stats=stats.data_ptr(), sums=sums.data_ptr())
        _lib.call_on(self.device, "te_policy_ppo_epoch", C.byref(a))

    def _call(self, obs, eps, outs):
        lidar, inertial, last_action = obs["lidar"], obs["inertial_data"], obs["last_action"]
        n = lidar.shape[0]
        for name, t, shape in (("lidar", lidar, (n, self.lidar_channels, 13, 26)), ("inertial_data", inertial, (n, 15)),
                               ("last_action", last_action, (n, 4)), ("eps", eps, (n, 4))):
            if t is not None:
                require_f32("FusedPolicy", name, t, shape, self.device)
        entry, weights = self.act_entry
        _lib.call_on(self.device, entry, *(w.data_ptr() for w in weights), C.byref(self.shape), n, lidar.data_ptr(), inertial.data_ptr(),
                     last_action.data_ptr(), _ptr(eps), *(_ptr(o) for o in outs))

    def forward(self, obs: Dict[str, torch.Tensor]):
        """(mu [N, 4], value [N]) of the module's forward."""
        n = obs["lidar"].shape[0]
        mu = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        value = torch.empty((n,), dtype=torch.float32, device=self.device)
        self._call(obs, None, (mu, value, None, None, None))
        return mu, value

    __call__ = forward

    def act(self, obs: Dict[str, torch.Tensor], eps: torch.Tensor):
        """(a, logp, value, a_env) for the standard-normal draw eps [N, 4]: a = mu + exp(log_std) eps, logp its log-density summed
        over the 4 components, a_env = a clamped to [-1, 1]^3 x [0, 1]."""
        n = obs["lidar"].shape[0]
        f = dict(dtype=torch.float32, device=self.device)
        mu, value, a, logp, a_env = torch.empty((n, 4), **f), torch.empty((n,), **f), torch.empty((n, 4), **f), torch.empty((n,), **f), torch.empty((n, 4), **f)
        self._call(obs, eps, (mu, value, a, logp, a_env))
        return a, logp, value, a_env


class PackedAdam:
    """clip_grad_norm_ + torch.optim.Adam (non-fused form, no weight decay, no amsgrad: SB3's optimiser) on a FusedPolicy's packed
    buffer by te_policy_adam_step: two launches per step() on PyTorch's current stream, no host synchronisation, graph-capturable.
    The state (step, the last call's norm and clip coefficient, exp_avg, exp_avg_sq) is ONE device buffer in the layout of
    include/threatengage.h; zeros are a fresh optimiser.  Bind the policy's parameters (FusedPolicy.bind_parameters) for the module
    to see the steps: this object writes fused_policy.params only."""

    def __init__(self, fused_policy: FusedPolicy, lr: float, betas=(0.9, 0.999), eps: float = 1e-5):
        self.fused_policy, self.lr, self.betas, self.eps = fused_policy, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.words = fused_policy.params.numel()
        need = C.c_size_t()
        _lib.call("te_policy_opt_state_bytes", self.words, C.byref(need))
        self.state = torch.zeros(int(need.value) // 4, dtype=torch.float32, device=fused_policy.device)
        a = (self.words + 3) // 4 * 4            # m and v start on 16-byte boundaries behind the 64-byte header
        self.step_count = self.state[0:1].view(torch.int32)    # views of the state: reading them costs no host synchronisation
        self.grad_norm, self.clip_coef = self.state[1:2], self.state[2:3]
        self.exp_avg, self.exp_avg_sq = self.state[16:16 + self.words], self.state[16 + a:16 + a + self.words]

    def step(self, grad: torch.Tensor, max_grad_norm: float, grad_scale: float = 1.0, repack: bool = False) -> None:
        """One clipped Adam step on `grad` [words] (the packed order, 16-byte aligned); max_grad_norm = inf does not clip;
        grad_scale multiplies the gradient before the norm and the update (1 / world_size after an all-reduce).
        repack=True: te_policy_adam_step_bf16, the same step (params and state bitwise the same) that also leaves the FusedPolicy's
        weights_bf16 and, when it owns one, weights_bf16_t current, so no refresh() has to follow; a ValueError when the FusedPolicy
        owns no bf16 buffer."""
        f = self.fused_policy
        if repack and f.weights_bf16 is None:
            raise ValueError("PackedAdam.step: repack=True keeps the FusedPolicy's bf16 weights current, and this one owns none "
                             "(FusedPolicy(precision='bf16') or grad_precision='bf16')")
        require_f32("PackedAdam.step", "grad", grad, (self.words,), f.device)
        scalars = (self.lr, self.betas[0], self.betas[1], self.eps, float(max_grad_norm), float(grad_scale))
        if repack:
            _lib.call_on(f.device, "te_policy_adam_step_bf16", f.params.data_ptr(), grad.data_ptr(), self.state.data_ptr(),
                         self.state.numel() * 4, C.byref(f.shape), f.weights_bf16.data_ptr(), _ptr(f.weights_bf16_t), *scalars)
            return
        _lib.call_on(f.device, "te_policy_adam_step", f.params.data_ptr(), grad.data_ptr(), self.state.data_ptr(), self.state.numel() * 4,
                     self.words, *scalars)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"state": self.state.clone()}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        src = sd["state"]
        if tuple(src.shape) != tuple(self.state.shape) or src.dtype != self.state.dtype:
            raise ValueError(f"PackedAdam.load_state_dict: the state must be {self.state.numel()} float32 words (te_policy_opt_state_bytes)")
        self.state.copy_(src)


def adv_stats_workspace(n: int, device) -> torch.Tensor:
    """The workspace of adv_stats for up to n elements (te_adv_stats_workspace_bytes is monotone in n)."""
    need = C.c_size_t()
    _lib.call("te_adv_stats_workspace_bytes", int(n), C.byref(need))
    return torch.empty(int(need.value), dtype=torch.uint8, device=device)


def adv_stats(x: torch.Tensor, index: Optional[torch.Tensor], out: torch.Tensor, workspace: torch.Tensor) -> None:
    """out[0], out[1] = the mean and the unbiased std (torch.std's default) of x[index] (int64 [B]; None: all of x), x a contiguous
    float32 vector: one te_adv_stats call, two launches on PyTorch's current stream, fp64 sums in a fixed order (repeated calls are
    bitwise equal), no host synchronisation, graph-capturable.  `workspace` comes from adv_stats_workspace(n) with n >= the count."""
    dev = x.device
    if dev.type != "cuda":
        raise ValueError("adv_stats runs the HIP kernels of te_adv_stats: x must live on a GPU")
    if x.dim() != 1 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("adv_stats: x must be a contiguous 1-D float32 tensor")
    require_f32("adv_stats", "out", out, (2,), dev)
    require_index("adv_stats", index, dev)
    if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError(f"adv_stats: workspace must be a contiguous uint8 tensor on {dev} (adv_stats_workspace)")
    n = x.numel() if index is None else index.numel()
    _lib.call_on(dev, "te_adv_stats", x.data_ptr(), _ptr(index), n, out.data_ptr(), workspace.data_ptr(), workspace.numel())


class PolicyDriver:
    """SB3-style `predict` over a LidarInertialActionPolicy, on the device: what ThreatEngageVecEnv.update_model (exp05:
    the ally flown by a copy of the learning policy, apps/threatengage_runner/stage03/experiments/05/
    bo_exp05_vFinal_home_office_app.py:140,179) takes when the observations should not leave HBM.
    fused=True: the forward (and the sample) is one te_policy_act launch (FusedPolicy); the weights are repacked at every call,
    so a policy trained in between is always the one that flies.  precision="bf16" (with fused=True): te_policy_act_bf16."""
    accepts_torch = True

    def __init__(self, policy: nn.Module, fused: bool = False, precision: str = "fp32"):
        if precision != "fp32" and not fused:
            raise ValueError("PolicyDriver: precision other than 'fp32' is the fused kernel's: it needs fused=True")
        self.policy = policy
        self.fused = FusedPolicy(policy, precision=precision) if fused else None
        self.low = None

    @torch.no_grad()
    def predict(self, observation: Dict[str, torch.Tensor], state=None, episode_start=None, deterministic: bool = True):
        if self.fused is not None:
            self.fused.refresh()
            obs = {k: observation[k].contiguous() for k in ("lidar", "inertial_data", "last_action")}
            if deterministic:
                a = self.fused.forward(obs)[0]
            else:
                return self.fused.act(obs, torch.randn((obs["lidar"].shape[0], 4), device=self.fused.device))[3], None
        else:
            dist, _ = self.policy.dist(observation)
            a = dist.mean if deterministic else dist.sample()
        if self.low is None:
            self.low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device=a.device)
        return torch.max(torch.min(a, torch.ones_like(a)), self.low), None


@dataclass
class PPOConfig:
    n_steps: int = 128
    batch_size: int = 2048
    n_epochs: int = 10
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    vf_coef: float = 0.5
    ent_coef: float = 0.0
    max_grad_norm: float = 0.5
    learning_rate: float = 3e-4
    use_graph: bool = True       # collect(): policy forward + sampling + te_step captured once in a HIP graph and replayed per step
    # update(): fused Adam (one multi-tensor kernel instead of ~25 x 6 element-wise launches per minibatch) and bf16 autocast of the forward /
    # backward of the policy (fp32 master weights, fp32 losses and optimiser): measured + 16 % on the update at 32 768-sample minibatches
    # (tools/ppo_update_profile.py).  Off by default: fp32 / plain Adam is what SB3 runs.
    fast_learner: bool = False
    # collect() and the bootstrap value: the policy's forward + sampling + log-prob + clamp as ONE HIP launch (te_policy_act, FusedPolicy)
    # instead of the op-by-op PyTorch forward; eps still comes from torch.randn_like, update() still runs the PyTorch module.
    # Off by default: the outputs agree with the module's to ~1.5e-7 (measured), not bit for bit (another summation order)
    # It serves the shapes FusedPolicy lists, and pays for the default shape only: at 65 536 rows the launch takes 0.56 ms against PyTorch's
    # 1.14 ms for the default, but 3.06 against 1.84 ms for features_dim 512 with net_arch (128, 256, 512) and 3.83 against 2.04 ms with
    # (512, 128, 256) (measured, DESIGN.md 7, profiles/policy_shapes.json): for those, leave it off unless the single launch matters more, or add fused_forward_bf16
    fused_forward: bool = False
    # fused_forward through te_policy_act_bf16: weights and every layer's input rounded to bf16, the GEMMs on the bf16 MFMA with fp32
    # accumulation (FusedPolicy(precision="bf16"); the contract is in include/threatengage.h).  Needs fused_forward; applies to collect()
    # and to the bootstrap value, in both collect paths; update() is untouched.  What it costs: old_logp and the stored values come from
    # the bf16 mean and value while update()'s forward is fp32, so the first epoch's ratio is not exactly 1 (fused_update_bf16 below closes
    # that gap: its forward is this one).
    # Measured on the MI355X (profiles/policy_bf16.json): at 65 536 rows the launch takes 0.246 ms for the default shape, 0.548 ms
    # for features_dim 512 with net_arch (128, 256, 512) and 0.549 ms with (512, 128, 256), against PyTorch's fp32 forward at 1.158 / 1.849 /
    # 2.049 ms, PyTorch under autocast(bfloat16) at 0.886 / 1.064 / 1.070 ms and the fp32 launch at 0.563 / 3.069 / 3.817 ms; collect() of
    # (128, 256, 512) at 65 536 envs runs 1.02 ms per step against 2.38 (PyTorch) and 3.70 (fp32 launch).  The gap: mu and value differ from the
    # fp32 module's by at most 3.3e-4 on the test inputs (outputs of magnitude 0.02 to 0.2), and over 131 072 rows of that collect()
    # |log ratio| of the first epoch before any step was 1.1e-4 on average and 9.8e-4 at most, against clip_range 0.2.
    # Off by default
    fused_forward_bf16: bool = False
    # update(): the minibatch's loss gradient in ONE ABI call (te_policy_ppo_grad, FusedPolicy.ppo_grad: forward, loss, backward and
    # deterministic split-K weight gradients in HIP, the rows read through the minibatch index) instead of the PyTorch forward +
    # autograd; gradient clipping, the all-reduce and Adam stay as they are (with fast_learner: fused Adam, no autocast).
    # Off by default: the gradient agrees with autograd's to a tolerance (another summation order), not bit for bit
    fused_update: bool = False
    # update(): gradient clipping and Adam in ONE ABI call (te_policy_adam_step, PackedAdam: two launches) instead of clip_grad_norm_ +
    # torch.optim.Adam over 31 tensors.  Needs fused_update (the gradient already lies in the packed order) and a GPU.  The learner's
    # parameters become views of the FusedPolicy's packed buffer (bind_parameters), so no repack follows a step, and update()'s dict
    # gains "grad_norm" (the mean norm before clipping).  PPO.opt is then a PackedAdam (fast_learner's fused torch Adam is not used).
    # Off by default: the step agrees with torch's to rounding (the norm is summed in another order), not bit for bit
    fused_optimizer: bool = False
    reward_scale: float = 1e-3   # rewards reach +-1000 (exp03_vFinal_task.py:423-515); SB3 users wrap VecNormalize
    # who flies the caller-driven pursuers of the env (exp05's ally, the pursuers of cfg.evaluation's driver mask) during collect():
    # "none" = nobody, and PPO refuses such an env unless PPO(..., wingman_policy=module) gives a frozen policy to fly them;
    # "snapshot" = a frozen copy of the learner (bo_exp05_vFinal_home_office_app.py:140-175: update_model_path after every training
    # chunk), re-synced at the start of the first collect() after every wingman_sync_every updates.  Either way one te_drive_wingman
    # call per pursuer (observe, deterministic forward, clamp, drive) runs before every te_step, in both collect paths
    wingman_driver: str = "none"
    wingman_sync_every: int = 1
    # the wingmen's frozen policy through te_drive_wingman_bf16 (FusedPolicy(precision="bf16")): te_policy_act_bf16's forward in front of the
    # same clamp and drive.  Needs a wingman driver: wingman_driver="snapshot" or PPO(..., wingman_policy=module).  sync_wingmen() repacks
    # the bf16 weights in place with the fp32 ones, so the captured rollout graph flies them.  Independent of fused_forward_bf16 (the
    # learner's launch).  Measured on the MI355X at 65 536 exp05 envs (profiles/wingman_bf16.json): the call takes 0.321 ms for
    # the default shape, 0.645 ms for (128, 256, 512) and 0.630 ms for (512, 128, 256) against te_drive_wingman_shaped's 0.666 / 3.165 /
    # 3.922 ms, and a graph-captured collect step with fused_forward_bf16 1.03 / 1.71 / 1.70 ms against 1.40 / 4.32 / 5.06 ms.  What it
    # costs: over one rollout the ally's mean differs from the fp32 launch's on the same rows by 5e-5 to 6.5e-5 on average and 4.3e-4 at
    # most, so the ally does not fly the fp32 trajectory bit for bit.  Off by default
    wingman_bf16: bool = False
    # collect() also returns the statistics of the episodes that FINISHED during it (SB3's ep_rew_mean / ep_len_mean, plus the means of
    # the info row they ended with): an EpisodeMonitor (monitor.py, te_monitor_step) is fed the raw reward, done and info of every rollout
    # step on the device, one extra launch per step and one 80-byte host read per collect().  An episode still running at the end of a
    # collect() carries over to the next.  Keys other than "ep_count" are absent when no episode finished.  With several GPUs the
    # statistics are rank-local (each rank's own env shard; no collective).  Off by default: collect()'s dict is unchanged
    episode_stats: bool = False
    # the advantage arithmetic between the rollout and the gradient call in HIP (te_rollout.hpp).  collect(): GAE as ONE launch over the
    # whole rollout (te_rollout_gae, one thread per env) instead of RolloutBuffer.finish's ~9 PyTorch launches per step; adv and ret are
    # bitwise what finish() gives.  update() with fused_update: the minibatch's advantage mean and std by one te_adv_stats call (two
    # launches, fp64 sums in a fixed order) into the two floats te_policy_ppo_grad reads, instead of gather + mean + std + stack; they
    # agree with torch's to rounding, not bit for bit.  update()'s dict gains "explained_variance" = 1 - Var(ret - values) / Var(ret)
    # over the rollout (SB3's logger key; NaN when Var(ret) is 0), from two more te_adv_stats calls; with several GPUs it is rank-local
    # (each rank's own rollout; no collective).  Needs a GPU, not fused_update.  Off by default: every dict, tensor and launch is unchanged
    fused_advantages: bool = False
    # the shape of the policy PPO builds when it is given none: the trunk's width and the widths of the pi / vf heads' hidden layers
    # (LidarInertialActionPolicy).  The reference's trained networks are features_dim=512 with net_arch=(128, 256, 512) or (512, 128, 256).
    # fused_update and fused_optimizer serve the default shape, and the other two only with fused_update_wide
    features_dim: int = 256
    net_arch: tuple = (64, 64)
    # fused_update (and with it fused_optimizer) for a policy of the other served shapes: features_dim 512 with net_arch (128, 256, 512) or
    # (512, 128, 256), through te_policy_ppo_grad_shaped.  Needs fused_update; changes nothing for the default shape.  A switch of its own
    # because for these shapes the fused forward is slower than PyTorch's (fused_forward above), and the fused gradient pays at small
    # minibatches only.  Measured, one minibatch (gradient + clip + Adam) against autograd fp32 (DESIGN.md 7,
    # profiles/policy_grad_shapes.json): at 8 192 rows 1.65 against 3.47 ms for (128, 256, 512) and 1.93 against 4.07 ms for
    # (512, 128, 256), 2.1 x faster; at 65 536 rows 9.94 against 10.41 ms (1.05 x) and 11.78 against 10.25 ms: 0.87 x, SLOWER than autograd.
    # Off by default
    fused_update_wide: bool = False
    # fused_update through te_policy_ppo_grad_bf16 (FusedPolicy(grad_precision="bf16")): forward, backward and weight gradients on the bf16
    # MFMA with fp32 accumulation; the weights, every layer's input and every pre-activation gradient are rounded to bf16 once, the loss,
    # log_std's gradient, the statistics, the partial sums and the gradient itself stay fp32 (the contract is in include/threatengage.h).
    # Needs fused_update, and fused_update_wide for the wide shapes; independent of fused_forward_bf16; composes with fused_optimizer and
    # fused_advantages.  Its forward is bitwise te_policy_act_bf16's, so with fused_forward_bf16 as well the first epoch's ratio is
    # exactly 1 before any step.  What it costs: every tensor of the gradient is within 6 x 2^-8 of its largest per-row contribution of
    # the contract evaluated in fp64 (tests/test_policy_grad_bf16.py), which is bf16's resolution, not fp32's.
    # Measured on the MI355X (profiles/policy_grad_bf16.json), the call alone at 65 536 rows: 1.147 ms for the default shape, 2.688 ms
    # for features_dim 512 with net_arch (128, 256, 512) and 3.072 ms with (512, 128, 256), against te_policy_ppo_grad_shaped's 2.730 / 9.525 /
    # 11.515 ms in the same run (2.4 / 3.5 / 3.7 x; the spreads are below 1 %).  One minibatch (gradient + clip + Adam) at 65 536 rows: 1.57 /
    # 3.12 / 3.50 ms against fast_learner's (autocast bf16) 6.36 / 7.75 / 7.52 ms and autograd fp32's 7.24 / 10.47 / 10.31 ms: the wide shapes
    # no longer lose to fast_learner (2.5 x and 2.1 x faster).  At 8 192 rows 0.69 / 0.74 / 0.77 ms against fast_learner's 4.08 / 3.78 / 3.74 ms.
    # Off by default
    fused_update_bf16: bool = False
    # update(): every minibatch of an epoch enqueued by ONE ABI call (te_policy_ppo_epoch, FusedPolicy.ppo_epoch): per epoch one
    # torch.randperm and one call whose host loop, in C, launches the advantage statistics, the gradient, the Adam step and the log's
    # running sums of every minibatch back to back, instead of five ctypes calls, a slice and two tensor adds per minibatch from Python.
    # Needs fused_update, fused_optimizer and fused_advantages (the three calls it chains) and a GPU; composes with fused_update_wide and
    # fused_update_bf16, where the step itself keeps the bf16 weights current (te_policy_adam_step_bf16: no repack launches).  Refused
    # when torch.distributed has more than one rank: the all-reduce sits between the gradient and the step, and the Python loop stays the
    # path for that case.  The same kernels on the same inputs in the same order: the weights, the optimiser state and update()'s dict
    # are bitwise what the Python loop gives.
    # Measured on the MI355X (profiles/ppo_epoch.json), 8 minibatches per update(), ms per minibatch with the switch off
    # against on: 0.247 against 0.261 (default), 0.419 against 0.420 ((128, 256, 512)) and 0.420 against 0.432 ((512, 128, 256)) at 8 192 rows,
    # 1.260 / 2.762 / 3.122 against 1.266 / 2.762 / 3.135 at 65 536: no gain beyond the repeats' spread at any size, 3-5 % slower at some.
    # The Python loop already enqueues ahead of the device; what the switch buys is an update with no Python between its kernels, not time.
    # Off by default
    fused_epoch: bool = False

    def __post_init__(self):
        for switch in SWITCH_NEEDS:
            refusal = missing_switch(self, switch)
            if refusal:
                raise ValueError(refusal)
        refusal = fused_epoch_needs(self)
        if refusal:
            raise ValueError(refusal)


# switch: (the switch it needs, what it is to it), in the order PPOConfig checks them.  PPO checks them again, in its own order
# (PPO._refusal), for a switch set on the object after PPOConfig's own check
SWITCH_NEEDS = {"fused_update_bf16": ("fused_update", "is fused_update's call with bf16 operands"),
                "fused_optimizer": ("fused_update", "steps on te_policy_ppo_grad's packed gradient"),
                "fused_update_wide": ("fused_update", "widens fused_update to every served shape"),
                "fused_forward_bf16": ("fused_forward", "is fused_forward's launch with bf16 operands")}


def missing_switch(cfg: PPOConfig, switch: str) -> Optional[str]:
    """The refusal of `switch` when it is set without the switch it needs; None otherwise."""
    needs, what = SWITCH_NEEDS[switch]
    return f"PPOConfig.{switch} {what}: it needs {needs}" if getattr(cfg, switch) and not getattr(cfg, needs) else None


FUSED_EPOCH_NEEDS = ("fused_update", "fused_optimizer", "fused_advantages")    # the calls te_policy_ppo_epoch chains


def fused_epoch_needs(cfg: PPOConfig) -> Optional[str]:
    """The refusal of fused_epoch when one of the three switches it needs is off (the first one, by name); None otherwise."""
    if not cfg.fused_epoch:
        return None
    for needs in FUSED_EPOCH_NEEDS:
        if not getattr(cfg, needs):
            return (f"PPOConfig.fused_epoch enqueues te_adv_stats, the gradient call and te_policy_adam_step per minibatch from one "
                    f"te_policy_ppo_epoch call: it needs {needs}")
    return None


class RolloutBuffer:
    """[n_steps, N, ...] tensors on the environment's device."""

    def __init__(self, n_steps: int, n_envs: int, obs_shapes: Dict[str, tuple], device):
        f = dict(dtype=torch.float32, device=device)
        self.obs = {k: torch.empty((n_steps, n_envs, *s), **f) for k, s in obs_shapes.items()}
        self.actions = torch.empty((n_steps, n_envs, 4), **f)
        self.logp = torch.empty((n_steps, n_envs), **f)
        self.values = torch.empty((n_steps, n_envs), **f)
        self.rewards = torch.empty((n_steps, n_envs), **f)
        self.dones = torch.empty((n_steps, n_envs), **f)          # done AFTER this step
        self.adv = torch.empty((n_steps, n_envs), **f)
        self.ret = torch.empty((n_steps, n_envs), **f)

    def bytes(self) -> int:
        ts = list(self.obs.values()) + [self.actions, self.logp, self.values, self.rewards, self.dones, self.adv, self.ret]
        return sum(t.numel() * t.element_size() for t in ts)

    @torch.no_grad()
    def finish(self, last_value: torch.Tensor, gamma: float, lam: float, fused: bool = False) -> None:
        """GAE(lambda).  An env that auto-reset at step t starts a new episode at t+1: no bootstrap across it
        (terminations only: the reference never truncates, exp03_vFinal_environment.py:166).
        fused=True: the same recurrence, operation for operation, as ONE te_rollout_gae launch on PyTorch's current stream
        (bitwise the same adv and ret; GPU only)."""
        if fused:
            T, N = self.rewards.shape
            dev = self.rewards.device
            if dev.type != "cuda":
                raise ValueError("RolloutBuffer.finish(fused=True) runs the HIP kernel te_rollout_gae: the buffer must live on a GPU")
            require_f32("RolloutBuffer.finish", "last_value", last_value, (N,), dev)
            _lib.call_on(dev, "te_rollout_gae", T, N, self.rewards.data_ptr(), self.values.data_ptr(), self.dones.data_ptr(),
                         last_value.data_ptr(), float(gamma), float(lam), self.adv.data_ptr(), self.ret.data_ptr())
            return
        gae = torch.zeros_like(last_value)
        nxt = last_value
        for t in reversed(range(self.rewards.shape[0])):
            nonterminal = 1.0 - self.dones[t]
            delta = self.rewards[t] + gamma * nxt * nonterminal - self.values[t]
            gae = delta + gamma * lam * nonterminal * gae
            self.adv[t] = gae
            nxt = self.values[t]
        self.ret.copy_(self.adv + self.values)


def caller_driven_pursuers(ecfg) -> List[int]:
    """The pursuers of an env config that the caller flies (te_observe_wingman / te_set_wingman_actions): pursuer 1 of exp05
    (cfg.ally_policy == TE_ALLY_EXTERNAL) and every pursuer whose bit is set in cfg.evaluation's driver mask (bits 8..)."""
    if ecfg is None:
        return []
    mask = (int(ecfg.evaluation) & 0xFFFFFFFF) >> 8
    return [p for p in range(int(ecfg.n_pursuers)) if (int(ecfg.ally_policy) == K.ALLY_EXTERNAL and p == 1) or (mask >> p) & 1]


CHECKPOINT_FORMAT, CHECKPOINT_VERSION = "dronechase_amd.ppo.checkpoint", 1
# what the saved state means: a `cfg` given to PPO.load must agree with the saved one on these; every other field may differ
RESUME_FIELDS = ("features_dim", "net_arch", "fused_optimizer", "wingman_driver", "episode_stats")
_NO_DISTRIBUTED_CHECKPOINT = ("PPO.{}: a full checkpoint holds one rank's env shard, monitor and generators, and with more than one "
                              "torch.distributed rank it is refused; PPO.save_policy exports the weights on any rank")


def _host(x):
    """Tensors to the CPU (always a copy with storage of its own: a bound parameter is a view of the whole packed buffer), through
    dicts, lists and tuples; everything else as it is."""
    if torch.is_tensor(x):
        return x.detach().to("cpu", copy=True)
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_host(v) for v in x)
    return x


def _shape_lists(shape) -> list:
    c, features_dim, net_arch = shape
    return [int(c), int(features_dim), [int(w) for w in net_arch]]


def _module_of(saved: dict) -> LidarInertialActionPolicy:
    """The CPU module of a checkpoint's {"policy_shape", "policy"} pair; a ValueError when the tensors are not that shape's."""
    c, features_dim, net_arch = saved["policy_shape"]
    module = LidarInertialActionPolicy(lidar_shape=(int(c), K.LIDAR_NTHETA, K.LIDAR_NPHI), features_dim=int(features_dim),
                                       net_arch=tuple(int(w) for w in net_arch))
    try:
        module.load_state_dict(saved["policy"])
    except RuntimeError as e:
        raise ValueError(f"PPO.load: the saved weights are not those of the saved policy shape {saved['policy_shape']}: {e}") from None
    return module


def _load_checks(ck, env, cfg: Optional["PPOConfig"], wingman_policy, restore_env: bool, callback):
    """Every refusal of PPO.load that needs no more than the file, the arguments and what `env` says of itself, the first that fails
    as a ValueError; then (the config to build with, the learner's module with the saved weights on the CPU, the wingman module to
    give the constructor or None).  Reads only: the env is not reset and nothing is allocated on its device."""
    who = "PPO.load"
    name = ck.get("format") if isinstance(ck, dict) else None
    if name != CHECKPOINT_FORMAT:
        raise ValueError(f"{who}: the file's format is {name!r}, not {CHECKPOINT_FORMAT!r}")
    if int(ck["version"]) > CHECKPOINT_VERSION:
        raise ValueError(f"{who}: the file is version {int(ck['version'])} of {CHECKPOINT_FORMAT}, newer than version {CHECKPOINT_VERSION}, the last this package reads")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError(_NO_DISTRIBUTED_CHECKPOINT.format("load"))
    known = {f.name for f in fields(PPOConfig)}
    saved_cfg = PPOConfig(**{k: (tuple(v) if k == "net_arch" else v) for k, v in ck["cfg"].items() if k in known})
    if cfg is None:
        cfg = saved_cfg
    for f in RESUME_FIELDS:
        mine, theirs = getattr(cfg, f), getattr(saved_cfg, f)
        if f == "net_arch":
            mine, theirs = tuple(int(w) for w in mine), tuple(int(w) for w in theirs)
        if mine != theirs:
            raise ValueError(f"{who}: cfg.{f} is {mine!r}, the checkpoint was written with {theirs!r}: {', '.join(RESUME_FIELDS)} decide "
                             "what the saved state means and cannot change")
    policy = _module_of(ck)
    channels = int(env.lidar.shape[1])
    if int(ck["policy_shape"][0]) != channels:
        raise ValueError(f"{who}: the saved policy reads {int(ck['policy_shape'][0])} LIDAR channels, the environment has {channels}")
    ecfg = getattr(env, "cfg", None)
    if restore_env:
        if ck["env_state"] is None or ck["env_config"] is None:
            raise ValueError(f"{who}: the checkpoint holds no env state (its env had none to give): pass restore_env=False")
        abi = int(_lib.load().te_abi_version())
        if int(ck["abi_version"]) != abi:
            raise ValueError(f"{who}: the env state was written under ABI version {int(ck['abi_version'])}, the library's is {abi}: "
                             "restore_env=False takes the learner alone")
        if ecfg is None or not hasattr(env, "set_state"):
            raise ValueError(f"{who}: restore_env=True needs an env with a config and set_state")
        saved_bytes = ck["env_config"].numpy().tobytes()
        if saved_bytes != bytes(ecfg):
            if len(saved_bytes) != C.sizeof(K.Config):
                raise ValueError(f"{who}: the saved env config has te_config.struct_size {len(saved_bytes)}, this library's is {C.sizeof(K.Config)}")
            theirs = K.Config.from_buffer_copy(saved_bytes)
            field = K.first_difference(theirs, ecfg)
            if field is not None:
                values = dict(K.config_fields(theirs))[field], dict(K.config_fields(ecfg))[field]
                raise ValueError(f"{who}: the env's te_config.{field} is {values[1]!r}, the checkpoint's env had {values[0]!r}: restore_env=True "
                                 "continues the saved env, restore_env=False takes the learner alone")
    if callback is not None:
        if ck["callbacks"] is None:
            raise ValueError(f"{who}: a callback was given, but the checkpoint holds no callback state (learn() had none when it was saved)")
        callback.check_state(ck["callbacks"])
    saved = ck["wingman"]
    if wingman_policy is None and saved is not None and not saved["snapshot"] and caller_driven_pursuers(ecfg):
        wingman_policy = _module_of(saved).requires_grad_(False)     # the frozen module the saved run was given
    return cfg, policy, wingman_policy


LOSS_KEYS = ("pg_loss", "v_loss", "entropy", "clip_frac")        # update()'s log, in the order of te_policy_ppo_grad's stats_out
EV_KEYS = ("adv_mean", "adv_std", "ret_mean", "ret_std")         # PPO._ev_stats: read with the log, folded into "explained_variance"


class PPO:
    """`env` is a dronechase_amd.batched_env.BatchedEnv (classic own-sphere observation).  An env with caller-driven pursuers
    (exp05, the evaluation task's driver mask) needs PPOConfig.wingman_driver = "snapshot" or a frozen `wingman_policy`."""

    def __init__(self, env, cfg: Optional[PPOConfig] = None, policy: Optional[nn.Module] = None, seed: int = 0,
                 wingman_policy: Optional[nn.Module] = None):
        self.env, self.cfg = env, cfg or PPOConfig()
        self.device = env.device
        ecfg = getattr(env, "cfg", None)
        self.wingmen = caller_driven_pursuers(ecfg)
        torch.manual_seed(seed)
        self.policy = policy or LidarInertialActionPolicy(lidar_shape=tuple(env.lidar.shape[1:]), features_dim=self.cfg.features_dim,
                                                          net_arch=self.cfg.net_arch)
        refusal = self._refusal(wingman_policy is not None)      # before anything is allocated on the env's device or asked of the env
        if refusal:
            raise ValueError(refusal)
        self.policy = self.policy.to(self.device)
        fused = bool(self.cfg.fast_learner) and self.device.type == "cuda"
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=self.cfg.learning_rate, eps=1e-5, **({"fused": True} if fused else {}))
        shapes = {"lidar": tuple(env.lidar.shape[1:]), "inertial_data": (env.inertial.shape[1],), "last_action": (4,)}
        self.buf = RolloutBuffer(self.cfg.n_steps, env.N, shapes, self.device)
        self.low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device=self.device)
        self.high = torch.ones(4, device=self.device)
        self.distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if self.distributed:  # same initial weights on every rank
            for p in self.policy.parameters():
                torch.distributed.broadcast(p.data, src=0)
        # the frozen policy of the caller-driven pursuers: never trained, no gradient.  Its packed buffer keeps its address
        # (sync_wingmen repacks in place), so the captured rollout graph flies whatever was synced last
        self.wingman, self._wingman_snapshot, self._updates_since_sync = None, False, 0
        if self.wingmen:
            if wingman_policy is None:
                self._wingman_snapshot = True
                wingman_policy = copy.deepcopy(self.policy).requires_grad_(False)
            self.wingman = FusedPolicy(wingman_policy, precision="bf16" if self.cfg.wingman_bf16 else "fp32")
            if self.wingman.device != self.device:
                raise ValueError(f"PPO: wingman_policy lives on {self.wingman.device}, the environment on {self.device}")
            if self.wingman.lidar_channels != int(ecfg.lidar_channels):
                raise ValueError(f"PPO: wingman_policy reads {self.wingman.lidar_channels} LIDAR channels, the environment has {int(ecfg.lidar_channels)}")
            self._wingman_mu = {w: torch.zeros((env.N, 4), device=self.device) for w in self.wingmen}   # the last drive's mean
            for w in self.wingmen:
                env.wingman_scratch(w)      # allocated now, not inside a graph capture
        # ONE gradient bucket: every parameter's .grad is a view of this flat buffer, so data-parallel training averages the
        # gradients of a minibatch with a single all-reduce (RCCL over xGMI: a ring is per-link bound, 25 small collectives per
        # minibatch would be latency-bound; the policy has ~0.3 M parameters = 1.2 MB, one bucket)
        # fused_update: the bucket in te_policy_act's packed order, so te_policy_ppo_grad writes the .grad views directly
        params = _packed_order(self.policy) if self.cfg.fused_update else [p for p in self.policy.parameters() if p.requires_grad]
        self._flat_grad = torch.zeros(sum(p.numel() for p in params), dtype=params[0].dtype, device=self.device)
        off = 0
        for p in params:
            p.grad = self._flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        env.reset()
        precisions = dict(precision="bf16" if self.cfg.fused_forward_bf16 else "fp32",
                          grad_precision="bf16" if self.cfg.fused_update_bf16 else "fp32")     # one object serves both: the bf16 weights are shared
        self.fused = FusedPolicy(self.policy, **precisions) if self.cfg.fused_forward else None
        self.fused_grad = (self.fused or FusedPolicy(self.policy, **precisions)) if self.cfg.fused_update else None
        if self.cfg.fused_optimizer:    # the packed buffer becomes the single copy of the weights; the torch optimiser is dropped
            self.fused_grad.bind_parameters()
            self.opt = PackedAdam(self.fused_grad, lr=self.cfg.learning_rate, eps=1e-5)
        self._grad_stats = torch.zeros(4, device=self.device)
        if self.cfg.fused_epoch:        # te_policy_ppo_epoch's running sums: LOSS_KEYS and grad_norm, zeroed by every update()
            self._epoch_sums = torch.zeros(5, device=self.device)
        if self.cfg.fused_advantages:   # allocated once, for the whole rollout: nothing grows under graph capture
            self._adv_stats = torch.zeros(2, device=self.device)         # the minibatch's (mean, std): te_policy_ppo_grad's adv_mean_std
            self._ev_stats = torch.zeros(4, device=self.device)          # (mean, std) of adv and of ret over the rollout
            self._adv_ws = adv_stats_workspace(self.cfg.n_steps * env.N, self.device)
        self.direct = env.N % 2 == 0   # slot t of the LIDAR buffer starts on a 16-byte boundary (4 056 bytes per env)
        self._obs = None               # set by the first collect(): te_observe of the reset state
        self.monitor = None
        if self.cfg.episode_stats:
            from .monitor import EpisodeMonitor
            self.monitor = EpisodeMonitor(env.N, self.device, n_records=0)
        self.num_timesteps = 0
        self._rollout_pending = False  # collect() filled the buffer and update() has not consumed it: the one state save() refuses
        self._callback = None          # the callback learn() was last given: save() stores its state

    def _refusal(self, wingman_given: bool) -> Optional[str]:
        """Why this config, env and policy module cannot be trained together (the ValueError's text), or None: every rule that needs
        no more than them and whether a wingman_policy was given, the first that fails.  Reads only; nothing is allocated."""
        c, drv, on_gpu = self.cfg, self.cfg.wingman_driver, self.device.type == "cuda"
        if drv not in ("none", "snapshot"):
            return f"PPOConfig.wingman_driver must be 'none' or 'snapshot', not {drv!r}"
        driver = drv != "none" or wingman_given
        if c.wingman_bf16 and not driver:
            return ("PPOConfig.wingman_bf16 is the wingman driver's forward with bf16 operands: it needs wingman_driver='snapshot' "
                    "or PPO(..., wingman_policy=module)")
        if self.wingmen and not driver:
            # exp05 / Evaluation_Task "nn" drivers: somebody has to answer te_observe_wingman with te_set_wingman_actions
            # before every te_step; this rollout loop does not, and the wingman would fly a stale set-point
            return ("PPO drives the agent only: an environment with caller-driven wingmen (exp05, evaluation driver mask) "
                    "needs its wingman driver in the loop (ThreatEngageVecEnv.update_model), not this rollout")
        if driver:
            if not self.wingmen:
                return ("PPO: a wingman driver was given, but this environment has no caller-driven pursuer "
                        "(exp05's ally or cfg.evaluation's driver mask)")
            if drv == "snapshot" and wingman_given:
                return "PPO: wingman_driver='snapshot' flies a copy of the learner; pass wingman_policy with wingman_driver='none'"
            if not on_gpu:
                return "PPO's wingman driver runs the HIP kernels of te_drive_wingman: it needs a GPU device"
            if int(c.wingman_sync_every) < 1:
                return "PPOConfig.wingman_sync_every must be >= 1"
        early = missing_switch(c, "fused_update_wide") or missing_switch(c, "fused_update_bf16")     # set after PPOConfig's own check
        if early:
            return early
        if (c.fused_update or c.fused_optimizer) and not is_default_shape(*policy_shape(self.policy)[1:]):
            if not c.fused_update_wide:
                return GRAD_DEFAULT_ONLY
            try:
                check_policy_shape(*policy_shape(self.policy))      # an unserved shape: the text that lists the served ones
            except ValueError as e:
                return str(e)
        if c.fused_epoch:               # its own rules, in front of the rules of the switches it needs
            if fused_epoch_needs(c):
                return fused_epoch_needs(c)
            if not on_gpu:
                return "PPOConfig.fused_epoch runs the HIP kernels of te_policy_ppo_epoch: it needs a GPU device"
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                return ("PPOConfig.fused_epoch chains the gradient and the optimiser step in one call, and with more than one "
                        "torch.distributed rank the all-reduce sits between them: leave it off, update() then runs its Python loop")
        for switch, runs in (("fused_forward", "the HIP kernel te_policy_act"), ("fused_optimizer", "the HIP kernels of te_policy_adam_step"),
                             ("fused_update", "the HIP kernels of te_policy_ppo_grad"),
                             ("fused_advantages", "the HIP kernels of te_rollout_gae and te_adv_stats")):
            if getattr(c, switch) and not on_gpu:
                return f"PPOConfig.{switch} runs {runs}: it needs a GPU device"
        return missing_switch(c, "fused_optimizer") or missing_switch(c, "fused_forward_bf16")      # set after PPOConfig's own check

    def sync_wingmen(self) -> None:
        """Repack the wingmen's frozen policy in place: the learner's current weights with wingman_driver='snapshot', the given
        wingman_policy's otherwise (after the caller changed it)."""
        if self.wingman is None:
            raise ValueError("PPO.sync_wingmen: this PPO has no wingman driver")
        self.wingman.load_from(self.policy if self._wingman_snapshot else self.wingman.policy)
        self._updates_since_sync = 0

    def _drive_wingmen(self) -> None:
        """drive_lw_rl_agent of every caller-driven pursuer on the current state, before te_step (exp05_vFinal_task.py:252-260)."""
        for w in self.wingmen:
            self.env.drive_wingman(w, self.wingman, mu=self._wingman_mu[w])

    def _slot(self, t: int):
        b = self.buf
        return b.obs["lidar"][t], b.obs["inertial_data"][t], b.obs["last_action"][t]

    # ------------------------------------------------------------------ graph-captured rollout step
    def _capture_step(self) -> None:
        """One rollout step = ~40 small PyTorch launches (policy forward, sampling, clamps) + the two env kernels; at
        16 384 envs that is launch-bound in eager mode (1.9 ms per step, of which the kernels need ~0.8).  The step is
        captured once in a HIP graph on static tensors and replayed: te_step enqueues on PyTorch's current stream, so
        its launches are captured like any other."""
        b = self.buf
        self._g_obs = {k: torch.empty_like(v[0]) for k, v in b.obs.items()}
        self._g = dict(a=torch.empty_like(b.actions[0]), logp=torch.empty_like(b.logp[0]), v=torch.empty_like(b.values[0]),
                       reward=torch.empty_like(b.rewards[0]), done=torch.empty_like(b.dones[0]))
        for k in self._g_obs:
            self._g_obs[k].copy_(self._obs[k])

        def step_once():
            # the diagonal Gaussian by hand: torch.normal on expanded tensors checks its arguments on the host, which
            # a capturing stream does not permit.  log N(a; mu, sigma) = -(a - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi)
            if self.fused is not None:     # the same draw (randn_like of an [N, 4] float32 tensor), then one launch
                eps = torch.randn_like(self._g["a"])
                a, logp, v, a_env = self.fused.act(self._g_obs, eps)
            else:
                mu, v = self.policy(self._g_obs)
                log_std = self.policy.log_std
                eps = torch.randn_like(mu)
                a = mu + log_std.exp() * eps
                logp = (-0.5 * eps * eps - log_std - 0.9189385332046727).sum(-1)
                a_env = torch.max(torch.min(a, self.high), self.low).contiguous()
            self._g["a"].copy_(a); self._g["logp"].copy_(logp); self._g["v"].copy_(v)
            self._drive_wingmen()
            lidar, inertial, last_action, reward, done, _ = self.env.step(a_env, terminal=False)
            self._g["reward"].copy_(reward); self._g["done"].copy_(done)
            self._g_obs["lidar"].copy_(lidar); self._g_obs["inertial_data"].copy_(inertial); self._g_obs["last_action"].copy_(last_action)

        state = self.env.get_state().clone()          # warm-up and capture must not advance the environments (nor move the wingmen's set-points)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                step_once()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            step_once()
        self.env.set_state(state)
        for k in self._g_obs:
            self._g_obs[k].copy_(self._obs[k])

    @torch.no_grad()
    def _collect_graph(self) -> Dict[str, float]:
        b, c = self.buf, self.cfg
        if not hasattr(self, "_graph"):
            self._capture_step()
        ep_rew = torch.zeros((), device=self.device); ep_n = torch.zeros((), dtype=torch.int64, device=self.device)
        for t in range(c.n_steps):
            for k in b.obs:
                b.obs[k][t].copy_(self._g_obs[k])
            self._graph.replay()
            b.actions[t].copy_(self._g["a"]); b.logp[t].copy_(self._g["logp"]); b.values[t].copy_(self._g["v"])
            torch.mul(self._g["reward"], c.reward_scale, out=b.rewards[t]); b.dones[t].copy_(self._g["done"])
            ep_rew += self._g["reward"].mean(); ep_n += self._g["done"].sum().long()
            if self.monitor is not None:   # after replay(), outside the graph: the warm-up and capture steps never reach the monitor
                self.monitor.step(self.env.reward, self.env.done, self.env.info)
        self._obs = self._g_obs
        _, last_v = (self.fused or self.policy)(self._obs)
        b.finish(last_v, c.gamma, c.gae_lambda, fused=c.fused_advantages)
        self.num_timesteps += c.n_steps * self.env.N
        return {"mean_step_reward": float(ep_rew) / c.n_steps, "episodes_finished": int(ep_n), **self._episode_stats()}

    @torch.no_grad()
    def collect(self) -> Dict[str, float]:
        if self.fused is not None:   # update() moved the module's weights: repack them into the buffer the captured graph reads
            self.fused.refresh()
        if self._wingman_snapshot and self._updates_since_sync >= self.cfg.wingman_sync_every:
            self.sync_wingmen()
        if self._obs is None:
            self._obs = dict(zip(("lidar", "inertial_data", "last_action"), self.env.observe()))
        out = self._collect_graph() if self.cfg.use_graph and self.device.type == "cuda" else self._collect_eager()
        self._rollout_pending = True
        return out

    @torch.no_grad()
    def _collect_eager(self) -> Dict[str, float]:
        """The environment writes the observation of step t+1 straight into slot t+1 of the rollout buffer (te_step takes
        the destination pointers): no per-step copy of the 4 KB/env observation, and no host synchronisation inside the
        loop.  The observation after the last step goes to the env's own buffers and seeds slot 0 of the next rollout."""
        b, c = self.buf, self.cfg
        ep_rew = torch.zeros((), device=self.device); ep_n = torch.zeros((), dtype=torch.int64, device=self.device)
        for k in b.obs:
            b.obs[k][0].copy_(self._obs[k])
        for t in range(c.n_steps):
            if self.fused is not None:
                a, logp, v, a_env = self.fused.act({k: o[t] for k, o in b.obs.items()}, torch.randn_like(b.actions[t]))
                b.actions[t], b.logp[t], b.values[t] = a, logp, v
            else:
                dist, v = self.policy.dist({k: o[t] for k, o in b.obs.items()})
                a = dist.sample()
                b.actions[t], b.logp[t], b.values[t] = a, dist.log_prob(a).sum(-1), v
                a_env = torch.max(torch.min(a, self.high), self.low).contiguous()
            dest = self._slot(t + 1) if (self.direct and t + 1 < c.n_steps) else None
            self._drive_wingmen()
            lidar, inertial, last_action, reward, done, _info = self.env.step(a_env, terminal=False, out=dest)
            if dest is None and t + 1 < c.n_steps:   # odd n_envs: the slots are not 16-byte aligned, copy instead
                for k, src in zip(("lidar", "inertial_data", "last_action"), (lidar, inertial, last_action)):
                    b.obs[k][t + 1].copy_(src)
            b.rewards[t] = reward * c.reward_scale
            b.dones[t] = done.float()
            ep_rew += reward.mean(); ep_n += done.sum()   # stays on the device: one sync per rollout, not per step
            if self.monitor is not None:
                self.monitor.step(reward, done, _info)
        self._obs = {"lidar": lidar, "inertial_data": inertial, "last_action": last_action}
        _, last_v = (self.fused or self.policy)(self._obs)
        ep_rew, ep_n = float(ep_rew), int(ep_n)
        b.finish(last_v, c.gamma, c.gae_lambda, fused=c.fused_advantages)
        self.num_timesteps += c.n_steps * self.env.N
        return {"mean_step_reward": ep_rew / c.n_steps, "episodes_finished": ep_n, **self._episode_stats()}

    def _episode_stats(self) -> Dict[str, float]:
        """PPOConfig.episode_stats: the monitor's window (the episodes that finished during this collect()) as log keys, and a new window."""
        if self.monitor is None:
            return {}
        stats = self.monitor.stats(reset=True)
        stats["ep_count"] = stats.pop("count")
        return stats

    def evaluate(self, env, n_eval_episodes: int = 100, deterministic: bool = True, **kwargs):
        """SB3 EvalCallback's evaluate_policy of the learner on a SEPARATE evaluation env (monitor.evaluate_policy: it is reset and
        stepped; the training env is never touched): (episode_rewards, episode_lengths), raw rewards.  Caller-driven pursuers are flown
        by this PPO's own wingman object unless wingman_policy= says otherwise, in that object's precision (bf16 with
        PPOConfig.wingman_bf16)."""
        from .monitor import evaluate_policy

        if getattr(env, "backend", env) is self.env:
            raise ValueError("PPO.evaluate takes a separate evaluation env: evaluating on the training env would reset it mid-rollout")
        return evaluate_policy(self, env, n_eval_episodes=n_eval_episodes, deterministic=deterministic, **kwargs)

    def update(self) -> Dict[str, float]:
        b, c = self.buf, self.cfg
        T, N = b.rewards.shape
        flat = lambda x: x.reshape(T * N, *x.shape[2:])
        obs = {k: flat(v) for k, v in b.obs.items()}
        actions, old_logp, adv, ret = flat(b.actions), flat(b.logp), flat(b.adv), flat(b.ret)
        # running sums stay on the device: one host read per update(), not four per minibatch (each float() drains the stream)
        keys = LOSS_KEYS + (("grad_norm",) if c.fused_optimizer else ())      # grad_norm: the gradient's norm before clipping
        acc = torch.zeros(len(keys), device=self.device)
        n_batches = 0
        if c.fused_advantages:          # explained_variance's two stds, on the device: read with the accumulators below
            adv_stats(adv, None, self._ev_stats[0:2], self._adv_ws)
            adv_stats(ret, None, self._ev_stats[2:4], self._adv_ws)
        amp = bool(c.fast_learner) and self.device.type == "cuda" and not c.fused_update
        if c.fused_epoch:               # the weights Adam reads are the buffer; the bf16 copies are rounded once, then kept by the step
            self.fused_grad.refresh()
            acc = self._epoch_sums.zero_()
        for _ in range(c.n_epochs):
            perm = torch.randperm(T * N, device=self.device)
            if c.fused_epoch:           # every minibatch of the epoch: one call, no return to Python in between
                self.fused_grad.ppo_epoch(obs, perm, c.batch_size, actions, old_logp, adv, ret, c.clip_range, c.vf_coef, c.ent_coef,
                                          self._flat_grad, self.opt, c.max_grad_norm, self._adv_ws, self._adv_stats, self._grad_stats, acc)
                n_batches += -(-(T * N) // c.batch_size)
                continue
            for s in range(0, T * N, c.batch_size):
                idx = perm[s:s + c.batch_size]
                if self.fused_grad is not None:
                    self._fused_minibatch(obs, idx, actions, old_logp, adv, ret)
                    acc[:len(LOSS_KEYS)] += self._grad_stats
                    if c.fused_optimizer:
                        acc[len(LOSS_KEYS):] += self.opt.grad_norm
                    n_batches += 1
                    continue
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    mu, v = self.policy({k: o[idx] for k, o in obs.items()})
                mu, v = mu.float(), v.float()
                dist = torch.distributions.Normal(mu, self.policy.log_std.exp().expand_as(mu), validate_args=False)
                logp = dist.log_prob(actions[idx]).sum(-1)
                a = adv[idx]
                a = (a - a.mean()) / (a.std() + 1e-8)
                ratio = (logp - old_logp[idx]).exp()
                pg = -torch.min(a * ratio, a * ratio.clamp(1 - c.clip_range, 1 + c.clip_range)).mean()
                vl = torch.nn.functional.mse_loss(v, ret[idx])
                ent = dist.entropy().sum(-1).mean()
                loss = pg + c.vf_coef * vl - c.ent_coef * ent
                self._flat_grad.zero_()          # the parameters' .grad are views of it: backward accumulates in place
                loss.backward()
                self._step()
                with torch.no_grad():
                    acc += torch.stack((pg.detach(), vl.detach(), ent.detach(), ((ratio - 1).abs() > c.clip_range).float().mean()))
                n_batches += 1
        means = acc / max(n_batches, 1)
        if c.fused_advantages:
            keys, means = keys + EV_KEYS, torch.cat((means, self._ev_stats))
        out = dict(zip(keys, means.tolist()))      # the one host read
        self._updates_since_sync += 1
        self._rollout_pending = False
        if c.fused_advantages:          # ret - values is the advantage: 1 - Var(adv) / Var(ret), SB3's explained_variance
            _, std_adv, _, std_ret = (out.pop(k) for k in EV_KEYS)
            out["explained_variance"] = float("nan") if std_ret == 0.0 else 1.0 - (std_adv * std_adv) / (std_ret * std_ret)
        return out

    def _step(self) -> None:
        """The tail of every minibatch, on the gradient in the flat bucket: the system's only collective (the mean gradient over the
        ranks, one bucket), clipping and the optimiser's step.  fused_optimizer: the all-reduce and one te_policy_adam_step call on
        the buffer the next gradient reads (no repack, and no division: grad_scale)."""
        c = self.cfg
        world = 1
        if self.distributed:
            torch.distributed.all_reduce(self._flat_grad)
            world = torch.distributed.get_world_size()
        if c.fused_optimizer:
            self.opt.step(self._flat_grad, c.max_grad_norm, grad_scale=1.0 / world)
            return
        if self.distributed:
            self._flat_grad.div_(world)
        nn.utils.clip_grad_norm_(self.policy.parameters(), c.max_grad_norm)
        self.opt.step()

    def _fused_minibatch(self, obs, idx, actions, old_logp, adv, ret) -> None:
        """One minibatch of update() with fused_update: the gradient of the loss straight into the flat gradient bucket by
        te_policy_ppo_grad, then the autograd path's tail (_step)."""
        c = self.cfg
        self.fused_grad.refresh()            # Adam moved the weights: repack them (one 0.94 MB device copy; nothing when bound)
        if c.fused_advantages:
            adv_stats(adv, idx, self._adv_stats, self._adv_ws)
            ms = self._adv_stats
        else:
            a = adv[idx]
            ms = torch.stack((a.mean(), a.std()))
        self.fused_grad.ppo_grad(obs, idx, actions, old_logp, adv, ret, ms, c.clip_range, c.vf_coef, c.ent_coef,
                                 self._flat_grad, self._grad_stats)
        self._step()

    def learn(self, total_timesteps: int, log=None, callback=None):
        """collect() and update() until num_timesteps reaches total_timesteps.  callback (callbacks.py: a BaseCallback, usually a
        CallbackList) is consulted once per iteration, after update() and after log: when it returns False, learn returns."""
        if callback is not None:
            callback.init_callback(self)
            self._callback = callback
        while self.num_timesteps < total_timesteps:
            r = self.collect()
            u = self.update()
            if log:
                log({**r, **u, "timesteps": self.num_timesteps})
            if callback is not None and callback.on_iteration() is False:
                break
        return self

    # ------------------------------------------------------------------ save, resume, export
    def save_policy(self, path) -> None:
        """The learner's weights as an SB3-named policy zip (save_sb3_policy); works on any torch.distributed rank."""
        save_sb3_policy(self.policy, path)

    def save(self, path) -> None:
        """Everything the next collect() and update() read, as one torch.save file of CPU tensors, numbers, strings, lists and dicts
        (PPO.load reads it with weights_only=True): the config, the policy's shape and weights, the optimiser's state, num_timesteps,
        the wingman driver's frozen weights and the count of updates since their last sync, the observation the next rollout starts
        from, the env's config and state blob, the episode monitor, both torch generators and the state of learn()'s callback.  The
        rollout buffer is not saved: legal before the first collect() and between update() and the next collect(); with a collected
        rollout that update() has not consumed it is a ValueError and nothing is written.  Derived buffers (the packed fp32 copy, the
        bf16 weights and their transposes, the wingman's) are not saved: load() repacks them from the fp32 weights, which reproduces
        them bit for bit."""
        if self._rollout_pending:
            raise ValueError("PPO.save: collect() has filled a rollout that update() has not consumed, and the rollout buffer is not "
                             "part of a checkpoint: save between update() and the next collect()")
        if self.distributed:
            raise ValueError(_NO_DISTRIBUTED_CHECKPOINT.format("save"))
        torch.save(self._checkpoint(), path)

    def _checkpoint(self) -> dict:
        env, dev = self.env, self.device
        ecfg = getattr(env, "cfg", None)
        packed = isinstance(self.opt, PackedAdam)
        wingman = None
        if self.wingman is not None:
            wingman = {"policy_shape": _shape_lists(policy_shape(self.wingman.policy)), "policy": _host(self.wingman.policy.state_dict()),
                       "snapshot": bool(self._wingman_snapshot)}
        return {
            "format": CHECKPOINT_FORMAT, "version": CHECKPOINT_VERSION, "abi_version": int(_lib.load().te_abi_version()),
            "cfg": {**asdict(self.cfg), "net_arch": [int(w) for w in self.cfg.net_arch]},
            "policy_shape": _shape_lists(policy_shape(self.policy)), "policy": _host(self.policy.state_dict()),
            "optimizer_kind": "PackedAdam" if packed else "Adam", "optimizer": _host(self.opt.state_dict()),
            "num_timesteps": int(self.num_timesteps), "updates_since_sync": int(self._updates_since_sync), "wingman": wingman,
            "obs": None if self._obs is None else _host(dict(self._obs)),
            "env_config": None if ecfg is None else torch.frombuffer(bytearray(bytes(ecfg)), dtype=torch.uint8),
            "env_state": _host(env.get_state()) if hasattr(env, "get_state") else None,
            "monitor": None if self.monitor is None else self.monitor.saved_state(),
            "cpu_rng_state": torch.get_rng_state(),
            "cuda_rng_state": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,
            "callbacks": None if self._callback is None else self._callback.state_dict(),
        }

    @classmethod
    def load(cls, path, env, cfg: Optional[PPOConfig] = None, wingman_policy: Optional[nn.Module] = None, restore_env: bool = True,
             callback=None) -> "PPO":
        """The PPO that save() wrote, on `env`: read with torch.load(weights_only=True), built from the saved config (or `cfg`, which
        must agree with it on RESUME_FIELDS and may differ in everything else: a new learning rate, batch size or n_steps), then restored.
        restore_env=True: `env` must have the saved env's config (a ValueError names the first te_config field that differs); its state,
        the next rollout's observation, the episode monitor and both torch generators are restored, and learn() continues bit for bit
        as the saved run would have.  With use_graph the rollout step is captured here, BEFORE the generators are restored: the capture
        draws three times, which the saved run did before its first rollout.
        restore_env=False: the learner, the optimiser, num_timesteps and the wingman's weights are taken and the env is left freshly
        reset: the reference's stage03 continuing from a stage02 model (another task, the same observation shape).  No generator is
        restored then: the CPU generator is left as every PPO(...) leaves it (the constructor seeds it, here with 0).
        wingman_policy: flies the caller-driven pursuers as given, in place of the saved weights; without it a snapshot driver flies
        the saved frozen weights (NOT the learner's: the next sync comes when the saved count says so), and a driver that was given
        as a module is rebuilt from the file.  callback: a callback of the classes, in the order, of the one whose state the file
        holds; its state is restored, and it is what learn() should be given.
        Every refusal is a ValueError raised before the env is reset and before anything is allocated on its device."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        given = wingman_policy is not None
        cfg, policy, wingman_policy = _load_checks(ck, env, cfg, wingman_policy, restore_env, callback)
        probe = cls.__new__(cls)        # the constructor's own refusals, asked before a wingman module is moved to the env's device
        probe.cfg, probe.device, probe.wingmen, probe.policy = cfg, env.device, caller_driven_pursuers(getattr(env, "cfg", None)), policy
        refusal = probe._refusal(wingman_policy is not None)
        if refusal:
            raise ValueError(refusal)
        if wingman_policy is not None and not given:        # rebuilt from the file, on the CPU
            wingman_policy = wingman_policy.to(env.device)
        self = cls(env, cfg, policy=policy, seed=0, wingman_policy=wingman_policy)
        self._restore(ck, restore_env)
        if callback is not None:
            callback.load_state_dict(ck["callbacks"])
            self._callback = callback
        return self

    @torch.no_grad()
    def _restore(self, ck: dict, restore_env: bool) -> None:
        """The constructor was given the saved weights as its policy module, so the packed buffer, the bound parameters and the bf16
        copies already hold them.  Here: the optimiser, the counters, the wingman's frozen weights, and with restore_env the env."""
        dev = self.device
        if isinstance(self.opt, PackedAdam):
            self.opt.load_state_dict(ck["optimizer"])
        else:       # the state only: the hyper-parameters are this config's (a new learning rate is a reason to pass cfg)
            self.opt.load_state_dict({"state": ck["optimizer"]["state"], "param_groups": self.opt.state_dict()["param_groups"]})
        self.num_timesteps = int(ck["num_timesteps"])
        saved = ck["wingman"]
        if self._wingman_snapshot:
            if saved is not None and saved["snapshot"]:     # the frozen weights as they were: no sync, the saved count decides the next one
                self.wingman.load_from(_module_of(saved).to(dev))
                self._updates_since_sync = int(ck["updates_since_sync"])
            else:                                           # the saved run had no snapshot to keep: start from the restored learner
                self.sync_wingmen()
        if not restore_env:
            return
        self.env.set_state(ck["env_state"])
        if ck["obs"] is not None:
            self._obs = {k: ck["obs"][k].to(dev) for k in ("lidar", "inertial_data", "last_action")}
            if self.cfg.use_graph and dev.type == "cuda":
                self._capture_step()        # leaves the env state and _g_obs as they were given; draws from the CUDA generator
                self._obs = self._g_obs     # as after every graph collect(): the next rollout reads the static tensors
        if self.monitor is not None:
            self.monitor.load_saved_state(ck["monitor"])
        torch.set_rng_state(ck["cpu_rng_state"])
        if dev.type == "cuda":
            torch.cuda.set_rng_state(ck["cuda_rng_state"], dev)
