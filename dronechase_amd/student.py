"""The level5 student: the network that consumes the stacked observation (stacked_spheres [N,6,3,13,26], validity_mask [N,6],
inertial_data [N,15], last_action [N,4]) and imitates the teacher's action.

FLIAStudent restates the reference's StudentWithFLIA (core/rl_framework/agents/policies/ppo_policies.py:344-361) and what it is built
on (fused_lidar_extractor.py: FLIAExtractor -> CNNDeepSetAttentionNet -> SphereCNN + DeepSetAttentionNet) under the reference's 58
state_dict names, so a `student_last_model_0.pt` loads with strict=True.  The reference tree ships no student checkpoint; the names
and shapes are pinned from the reference module itself (tests/golden/student_flia_keys.json).

Everything is a PyTorch module of this package, trainable with autograd.  The one part PyTorch handles badly, the sphere CNN's two
oddly padded convolutions over N x 6 small spheres, also exists as a pair of HIP kernels (te_sphere_encode and its parameter gradient
te_sphere_encode_grad, csrc/te_sphere.hpp): StudentDriver(student, fused_encoder=True) runs inference through the first,
fused_conv_stack / StudentTrainer(student, fused_encoder=True) train through both.  The forward also exists with bf16 operands on the
bf16 MFMA (te_sphere_encode_bf16, csrc/te_sphere_bf16.hpp): StudentDriver(student, fused_encoder=True, encoder_precision="bf16"), for
inference only.

The data between the collector and the trainer lives in imitation.ImitationDataset (a ring in device memory filled from
BatchedEnv.step_students and sampled by HIP kernels); StudentTrainer.fit is the reference's training loop over it, kill_high_correlation
included.

Not here: bf16 in training (a bf16 forward needs a backward of the same forward) or behind the encoder, a gradient with respect to
the spheres, fusing Linear(1792, 512) / the DeepSet / trunk / heads, PPO on the stacked
observation, SB3 model.zip import of the MultiInputPolicy + FLIAExtractor form, and the reference file's unused CellGNN /
AttentionPooling / SingleWorldView* classes."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

OBS_KEYS = ("stacked_spheres", "validity_mask", "inertial_data", "last_action")
NO_VALUE = 1.0                      # HybridPadConv2d.NO_VALUE: the LIDAR's "no data", the constant of the padding in H
SPHERE_FEATURES = 64 * 4 * 7        # flatten(block2(block1(sphere))) of a [3, 13, 26] sphere


class _HybridPadConv2d(nn.Module):
    """Conv2d behind circular padding in W (azimuth) and constant NO_VALUE padding in H (fused_lidar_extractor.py:653-676)."""

    def __init__(self, in_ch: int, out_ch: int, kernel: int, stride: int):
        super().__init__()
        self.pad = (kernel - 1) // 2
        self.conv = nn.Conv2d(in_ch, out_ch, kernel_size=kernel, stride=stride, padding=0)

    def forward(self, x):
        x = F.pad(x, (self.pad, self.pad, 0, 0), mode="circular")
        x = F.pad(x, (0, 0, self.pad, self.pad), mode="constant", value=NO_VALUE)
        return self.conv(x)


class _SphereCNN(nn.Module):
    def __init__(self, shape: Tuple[int, int, int], output_dim: int):
        super().__init__()
        self.block1 = nn.Sequential(_HybridPadConv2d(shape[0], 32, 5, 2), nn.ReLU())
        self.block2 = nn.Sequential(_HybridPadConv2d(32, 64, 3, 2), nn.ReLU())
        with torch.no_grad():
            n_flatten = self.conv_stack(torch.zeros(1, *shape)).shape[1]
        self.linear = nn.Linear(n_flatten, output_dim)

    def conv_stack(self, x):
        """[M, C, H, W] -> [M, n_flatten]: the part te_sphere_encode computes."""
        return self.block2(self.block1(x)).flatten(1)


class _MLPBlock(nn.Module):
    """LayerNorm -> Linear(bias=False) -> activation -> dropout (fused_lidar_extractor.py:12-72)."""

    def __init__(self, input_dim: int, output_dim: int, prob: float, tanh: bool = True, dropout: bool = True):
        super().__init__()
        self.layer_norm = nn.LayerNorm(input_dim)
        self.linear = nn.Linear(input_dim, output_dim, bias=False)
        self.tanh = tanh
        self.p = prob if dropout else 0.0

    def forward(self, x):
        x = self.linear(self.layer_norm(x))
        if self.tanh:
            x = torch.tanh(x)
        return F.dropout(x, self.p, self.training) if self.p > 0.0 else x


class _MLPphi(nn.Module):
    def __init__(self, input_dim, output_dim, prob):
        super().__init__()
        self.phi_block_1 = _MLPBlock(input_dim, output_dim, prob)
        self.phi_block_2 = _MLPBlock(output_dim, output_dim, prob)
        self.phi_block_3 = _MLPBlock(output_dim, output_dim, prob)

    def forward(self, u):           # [B * N, input_dim]
        o1 = self.phi_block_1(u)
        i3 = self.phi_block_2(o1) + o1
        return self.phi_block_3(i3) + i3


class _MLPomega(nn.Module):
    def __init__(self, input_dim, output_dim, prob):
        super().__init__()
        self.omega_block_1 = _MLPBlock(input_dim, output_dim, prob)
        self.omega_block_2 = _MLPBlock(output_dim, output_dim, prob)
        self.omega_block_3 = _MLPBlock(output_dim, output_dim, prob, tanh=False)

    def forward(self, u, counts):   # [B * N, input_dim], [B, N] bool -> attention weights [B, N, output_dim]
        o1 = self.omega_block_1(u)
        o3 = self.omega_block_3(self.omega_block_2(o1) + o1)
        o3 = o3.masked_fill(~counts.reshape(-1, 1), torch.finfo(o3.dtype).min)
        return torch.softmax(o3.reshape(counts.shape[0], counts.shape[1], -1), dim=1).nan_to_num(0.0)


class _MLPtheta(nn.Module):
    def __init__(self, input_dim, hidden, output_dim, prob):
        super().__init__()
        self.theta_block_1 = _MLPBlock(input_dim, hidden, prob)
        self.theta_block_2 = _MLPBlock(hidden, hidden, prob)
        self.theta_block_3 = _MLPBlock(hidden, hidden, prob)
        self.theta_block_4 = _MLPBlock(hidden, output_dim, prob, tanh=False, dropout=False)

    def forward(self, x):
        i2 = self.theta_block_1(x) + x
        i3 = self.theta_block_2(i2) + i2
        return self.theta_block_4(self.theta_block_3(i3) + i3)


class _DeepSetAttentionNet(nn.Module):
    def __init__(self, input_dim, hidden, output_dim, prob=0.5):
        super().__init__()
        self.mlp_phi = _MLPphi(input_dim, hidden, prob)
        self.mlp_omega = _MLPomega(input_dim, hidden, prob)
        self.mlp_theta = _MLPtheta(hidden, hidden, output_dim, prob)

    def forward(self, features, counts):    # [B, N, input_dim], [B, N] bool
        B, N, _ = features.shape
        flat = features.reshape(B * N, -1)
        weighted = self.mlp_phi(flat).reshape(B, N, -1) * self.mlp_omega(flat, counts)
        return self.mlp_theta(weighted.sum(dim=1))


def counting_spheres(mask: torch.Tensor) -> torch.Tensor:
    """[B, N] uint8 or bool -> bool: the spheres the network looks at.  MLPomega._grant_at_least_one_valid as arithmetic (the
    reference branches on `all_invalid.any()`, a host read): sphere 0 of a row whose mask is all zero is turned on."""
    m = mask != 0
    first = torch.arange(m.shape[1], device=m.device) == 0
    return m | (~m.any(dim=1, keepdim=True) & first)


class _CNNDeepSetAttentionNet(nn.Module):
    def __init__(self, input_shape, hidden=512, output_dim=512, prob=0.5):
        super().__init__()
        self.sphere_cnn = _SphereCNN(input_shape, hidden)
        self.deepset = _DeepSetAttentionNet(hidden, hidden, output_dim, prob)

    def forward(self, spheres, mask, encoded=None):
        """spheres [B, N, C, H, W]; encoded [B, N, n_flatten]: the conv stack's output when something else computed it
        (te_sphere_encode), `spheres` is then not read.  The features of a sphere that does not count are taken as zeros, as the
        kernel writes them: the attention gives that sphere the weight 0, so the output does not depend on them, but an input that
        holds NaN there would otherwise reach the sum as 0 * NaN."""
        counts = counting_spheres(mask)
        B, N = counts.shape
        if encoded is None:
            encoded = self.sphere_cnn.conv_stack(spheres.reshape(B * N, *spheres.shape[2:]))
        encoded = encoded.reshape(B * N, -1)
        encoded = torch.where(counts.reshape(-1, 1), encoded, torch.zeros((), dtype=encoded.dtype, device=encoded.device))
        return self.deepset(self.sphere_cnn.linear(encoded).reshape(B, N, -1), counts)


def _mlp3(n_in: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(n_in, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU())


class _FLIAExtractor(nn.Module):
    def __init__(self, lidar_shape, features_dim):
        super().__init__()
        self.lidar_feature_extractor = _CNNDeepSetAttentionNet(lidar_shape, hidden=512, output_dim=512, prob=0.5)
        self.inertial_feature_extractor = _mlp3(15)
        self.action_feature_extractor = _mlp3(4)
        self.final_layer = nn.Sequential(nn.Linear(512 + 128 + 128, features_dim), nn.ReLU())

    def forward(self, obs, encoded=None):
        z = torch.cat((self.lidar_feature_extractor(obs["stacked_spheres"], obs["validity_mask"], encoded),
                       self.inertial_feature_extractor(obs["inertial_data"].flatten(start_dim=1)),
                       self.action_feature_extractor(obs["last_action"])), dim=1)
        return self.final_layer(z)


class FLIAStudent(nn.Module):
    """StudentWithFLIA: FLIAExtractor -> Linear(128) tanh Linear(256) tanh Linear(512) tanh Linear(4).  58 tensors, 4 265 412
    parameters under the reference's names.  eval() is the reference's eval mode; train() keeps its dropout (p = 0.5 after every
    DeepSet block but the last).  forward makes no host read."""

    def __init__(self, lidar_shape: Tuple[int, int, int] = (3, 13, 26), n_spheres: int = 6, features_dim: int = 512):
        super().__init__()
        self.lidar_shape, self.n_spheres, self.features_dim = tuple(int(v) for v in lidar_shape), int(n_spheres), int(features_dim)
        self.feature_extractor = _FLIAExtractor(self.lidar_shape, self.features_dim)
        self.mlp_head = nn.Sequential(nn.Linear(self.features_dim, 128), nn.Tanh(), nn.Linear(128, 256), nn.Tanh(), nn.Linear(256, 512), nn.Tanh(),
                                      nn.Linear(512, 4))

    @property
    def sphere_cnn(self) -> _SphereCNN:
        return self.feature_extractor.lidar_feature_extractor.sphere_cnn

    def trunk(self, obs: Dict[str, torch.Tensor], encoded: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The FLIAExtractor part alone: obs (the four level5 keys; the mask uint8 or bool) -> [B, features_dim].  `encoded`
        [B, n_spheres, 1792]: the sphere CNN's conv stack computed elsewhere (StudentDriver's fused encoder)."""
        return self.feature_extractor(obs, encoded)

    def forward(self, obs: Dict[str, torch.Tensor], encoded: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.mlp_head(self.trunk(obs, encoded))


def load_flia_student(path_or_state_dict, **kwargs) -> FLIAStudent:
    """A FLIAStudent with the weights of a reference checkpoint (`torch.save(student.state_dict(), ...)` of a StudentWithFLIA): a
    path, read with torch.load(weights_only=True), or the state_dict itself.  Strict: a missing key, an unknown key or a tensor of
    another shape is a ValueError that names it.  kwargs go to FLIAStudent."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    student = FLIAStudent(**kwargs)
    own = student.state_dict()
    missing, unknown = [k for k in own if k not in sd], [k for k in sd if k not in own]
    if missing or unknown:
        raise ValueError(f"load_flia_student: not a StudentWithFLIA state_dict: missing {missing}, unknown {unknown}")
    wrong = [f"{k}: {tuple(sd[k].shape)}, expected {tuple(v.shape)}" for k, v in own.items() if tuple(sd[k].shape) != tuple(v.shape)]
    if wrong:
        raise ValueError(f"load_flia_student: tensors of another shape: {wrong}")
    student.load_state_dict(sd, strict=True)
    return student.eval()


def imitation_loss(pred: torch.Tensor, target: torch.Tensor, w_dir: float = 0.8, w_mag: float = 0.2, w_raw_direction: float = 0.1,
                   eps: float = 1e-8) -> torch.Tensor:
    """loss_mae_direction (core/rl_framework/utils/sl_pipeline.py:87-111) on [B, 4] rows (dx, dy, dz, magnitude):
    w_dir * mean(1 - cos(direction)) + w_mag * MAE(magnitude) + w_raw_direction * MAE(raw direction)."""
    d_pred, d_true = pred[:, :3], target[:, :3]
    cos = (F.normalize(d_pred, dim=1, eps=eps) * F.normalize(d_true, dim=1, eps=eps)).sum(dim=1).clamp(-1.0, 1.0)
    return w_dir * (1.0 - cos).mean() + w_mag * F.l1_loss(pred[:, 3:4], target[:, 3:4]) + w_raw_direction * F.l1_loss(d_pred, d_true)


def _conv_tensors(student: FLIAStudent):
    """The four tensors of the two conv blocks, in the order of te_sphere_encode's parameter buffer."""
    cnn = student.sphere_cnn
    return [cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias]


def _conv_layout_words(who: str, student: FLIAStudent) -> int:
    """te_sphere_encode's parameter count, which the student's two conv blocks must have."""
    words = C.c_size_t()
    _lib.call("te_sphere_encode_param_words", student.lidar_shape[0], C.byref(words))
    if sum(p.numel() for p in _conv_tensors(student)) != words.value:
        raise ValueError(f"{who}: the student's conv blocks do not have te_sphere_encode's layout")
    return int(words.value)


def _sphere_encode(params, weights_bf16, stacked, mask, out) -> None:
    """The forward launch over stacked [B, N, C, 13, 26] into out: te_sphere_encode, or te_sphere_encode_bf16 when bf16 weights are given."""
    B, N, channels = (int(v) for v in stacked.shape[:3])
    if weights_bf16 is not None:
        _lib.call_on(stacked.device, "te_sphere_encode_bf16", params.data_ptr(), weights_bf16.data_ptr(), channels, B, N, stacked.data_ptr(),
                     _lib._ptr(mask), out.data_ptr())
    else:
        _lib.call_on(stacked.device, "te_sphere_encode", params.data_ptr(), channels, B, N, stacked.data_ptr(), _lib._ptr(mask), out.data_ptr())


# te_sphere_encode_grad's workspaces, (device, stream, B, N) -> buffer, most recently used last.  A workspace is scratch of one call, so
# calls that may overlap must not share one: the key holds the stream the call is enqueued on (two calls on one stream run in order).
# At most _GRAD_WORKSPACES_MAX are kept (a workspace is up to 21 MB); the least recently used one is dropped, which is safe while its
# call is still queued because PyTorch's allocator hands a freed block of a stream only to later work on that stream.
_GRAD_WORKSPACES: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()
_GRAD_WORKSPACES_MAX = 8


def _grad_workspace(device, channels: int, B: int, N: int) -> torch.Tensor:
    key = (device, torch.cuda.current_stream(device).cuda_stream, B, N)
    ws = _GRAD_WORKSPACES.get(key)
    if ws is None:
        need = C.c_size_t()
        _lib.call("te_sphere_encode_grad_workspace_bytes", channels, B, N, C.byref(need))
        ws = _GRAD_WORKSPACES[key] = torch.empty(int(need.value), dtype=torch.uint8, device=device)
        while len(_GRAD_WORKSPACES) > _GRAD_WORKSPACES_MAX:
            _GRAD_WORKSPACES.popitem(last=False)
    _GRAD_WORKSPACES.move_to_end(key)
    return ws


class _FusedConvStack(torch.autograd.Function):
    """te_sphere_encode forward, te_sphere_encode_grad backward, over the packed parameter buffer."""

    @staticmethod
    def forward(ctx, params, stacked, mask):
        B, N = int(stacked.shape[0]), int(stacked.shape[1])
        out = torch.empty((B, N, SPHERE_FEATURES), dtype=torch.float32, device=stacked.device)
        _sphere_encode(params, None, stacked, mask, out)
        ctx.save_for_backward(params, stacked, mask, out)
        return out

    @staticmethod
    def backward(ctx, d_out):
        params, stacked, mask, out = ctx.saved_tensors
        B, N, channels = int(stacked.shape[0]), int(stacked.shape[1]), int(stacked.shape[2])
        d_out = d_out.contiguous()
        grad = torch.empty_like(params)
        ws = _grad_workspace(stacked.device, channels, B, N)      # of the stream call_on enqueues on
        _lib.call_on(stacked.device, "te_sphere_encode_grad", params.data_ptr(), channels, B, N, stacked.data_ptr(), _lib._ptr(mask),
                     out.data_ptr(), d_out.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel())
        return grad, None, None


def fused_conv_stack(student: FLIAStudent, stacked: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """The student's two conv blocks over stacked [B, N, 3, 13, 26] f32 as HIP launches that autograd can differentiate:
    te_sphere_encode forward, te_sphere_encode_grad backward -> encoded [B, N, 1792], for `student(obs, encoded=...)`.  mask [B, N]
    uint8 / bool or None (every sphere counts); the features of a sphere that does not count are zeros and it adds nothing to the
    gradient.  The four conv tensors are packed by a differentiable torch.cat, so the packed gradient reaches the module's own
    parameters through cat's backward; `stacked` and `mask` get no gradient (an observation has none).  The workspace of the backward
    is kept per (device, stream, B, N).  The conv tensors must be float32 (the kernels read floats) and have te_sphere_encode's
    layout.  CUDA / ROCm tensors only: there is no CPU form of the kernels."""
    if not isinstance(student, FLIAStudent):
        raise TypeError("fused_conv_stack: student must be a FLIAStudent")
    conv = _conv_tensors(student)
    if any(p.dtype != torch.float32 for p in conv):
        raise ValueError(f"fused_conv_stack: the student's conv tensors must be float32, not {conv[0].dtype}: the kernels read floats")
    _conv_layout_words("fused_conv_stack", student)
    device = next(student.parameters()).device
    if device.type != "cuda" or stacked.device.type != "cuda":
        raise ValueError("fused_conv_stack runs the HIP kernels te_sphere_encode and te_sphere_encode_grad: the student and its "
                         "observation must live on a GPU")
    B, N = int(stacked.shape[0]), int(stacked.shape[1])
    _lib.require_f32("fused_conv_stack", "stacked_spheres", stacked, (B, N, *student.lidar_shape), device)
    if mask is not None:
        mask = _lib.require_bytes("fused_conv_stack", "validity_mask", mask, (B, N), device)
    params = torch.cat([p.reshape(-1) for p in conv])
    return _FusedConvStack.apply(params, stacked.detach(), mask)


class StudentTrainer:
    """The reference's supervised step (sl_pipeline.py:172-207): Adam, loss_mae_direction with w_mag = 1, w_dir = 100,
    w_raw_direction = 60, and clip_grad_norm_(1.0).  step() works on tensors that already are on the student's device (e.g. the armed
    rows of BatchedEnv.step_students) and makes no host read: the loss comes back as a tensor.  fit() is the reference's loop of such
    steps over an imitation.ImitationDataset, with its kill_high_correlation (noise on / replacement of last_action before the step).

    fused_encoder=True: the two conv blocks run through fused_conv_stack (te_sphere_encode forward, te_sphere_encode_grad backward;
    fp32 MFMA, the spheres the network does not look at skipped in both); Linear(1792, 512), the DeepSet, the trunk and the heads stay
    autograd.  The student must live on a GPU.  The switch is opt-in because the default must run wherever the module does.
    Measured on the MI355X (profiles/student_train.json): the encoder's forward + backward take 0.67 / 4.80 ms at
    1 024 / 8 192 rows of 6 valid spheres against 1.70 / 13.7 ms of autograd through the PyTorch formulation (2.5 - 2.9x; 2.9 - 4.1x with a
    rollout's masks), at 0.26 - 0.29 of the fp32 MFMA peak.  The whole step is 17.1 against 25.8 ms at 8 192 rows (1.5x; 1.7x with a
    rollout's masks); at 1 024 rows it is bound by the host's launches behind the encoder and not measurably faster (5.7 against 6.0 ms
    in the recorded run, 0.96 - 1.08x over three runs)."""
    W_MAG, W_DIR, W_RAW_DIRECTION = 1.0, 100.0, 60.0

    def __init__(self, student: FLIAStudent, lr: float = 1e-3, fused_encoder: bool = False):
        self.student = student
        self.fused_encoder = bool(fused_encoder)
        if self.fused_encoder and next(student.parameters()).device.type != "cuda":
            raise ValueError("StudentTrainer(fused_encoder=True) runs the HIP kernels te_sphere_encode and te_sphere_encode_grad: "
                             "the student must live on a GPU")
        self.optimizer = torch.optim.Adam(student.parameters(), lr=lr)
        self.noise_seed, self.batches_fitted = 0, 0     # fit(): the key and the running draw of te_dataset_gather's last_action noise
        self.last_modes: list = []                       # fit(): kill_high_correlation's branch of every batch of the last call

    def step(self, obs: Dict[str, torch.Tensor], teacher_action: torch.Tensor) -> torch.Tensor:
        self.student.train()
        encoded = None
        if self.fused_encoder:
            obs = dict(obs, stacked_spheres=obs["stacked_spheres"].contiguous(), validity_mask=obs["validity_mask"].contiguous())
            encoded = fused_conv_stack(self.student, obs["stacked_spheres"], obs["validity_mask"])
        loss = imitation_loss(self.student(obs, encoded), teacher_action, w_dir=self.W_DIR, w_mag=self.W_MAG, w_raw_direction=self.W_RAW_DIRECTION)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        nn.utils.clip_grad_norm_(self.student.parameters(), max_norm=1.0)
        self.optimizer.step()
        return loss.detach()

    def fit(self, dataset, epochs: int = 1, batch_size: int = 1024, rng: Optional[np.random.Generator] = None,
            kill_high_correlation: bool = True) -> torch.Tensor:
        """_train_ppo's loop (sl_pipeline.py:172-207) over an imitation.ImitationDataset on the student's device.  Per epoch one
        permutation of range(size) (torch.randperm on the device, PyTorch's device generator: torch.manual_seed fixes it) is stepped
        through in batches of batch_size, the last short one kept.  Per batch p = rng.random() (a numpy Generator, default
        default_rng(42)) picks kill_high_correlation's branch as the reference does: p < 0.2 replaces last_action by uniform noise,
        p < 0.6 keeps it, anything else adds N(0, 0.2) noise and clamps; the noise itself is drawn on the device by
        te_dataset_gather, keyed by (self.noise_seed, the ordinal of the batch among all this trainer has fitted), so rng is asked for
        exactly one number per batch.  kill_high_correlation=False keeps last_action and draws nothing from rng.  The permutation addresses the ring's slots; after a wrap they are not in age order,
        which a permutation does not care about.  Returns the per-batch losses [epochs * ceil(size / batch_size)] as one device
        tensor; the only host read is the dataset's size, once."""
        from .imitation import ImitationDataset, last_action_mode
        if not isinstance(dataset, ImitationDataset):
            raise ValueError("StudentTrainer.fit: dataset must be an imitation.ImitationDataset (a ring on a GPU), not "
                             f"{type(dataset).__name__}")
        device = next(self.student.parameters()).device
        if dataset.device != device:
            raise ValueError(f"StudentTrainer.fit: dataset lives on {dataset.device}, the student on {device}")
        if dataset.n_spheres != self.student.n_spheres:
            raise ValueError(f"StudentTrainer.fit: dataset has {dataset.n_spheres} spheres per row, the student takes {self.student.n_spheres}")
        epochs, batch_size = int(epochs), int(batch_size)
        if epochs < 1 or batch_size < 1:
            raise ValueError("StudentTrainer.fit: epochs and batch_size must be >= 1")
        size = dataset.size()
        if size < 1:
            raise ValueError("StudentTrainer.fit: dataset is empty")
        rng = np.random.default_rng(42) if rng is None else rng
        self.last_modes = []
        losses = []
        for _ in range(epochs):
            perm = torch.randperm(size, device=device)
            for at in range(0, size, batch_size):
                index = perm[at:at + batch_size]
                mode = last_action_mode(rng.random()) if kill_high_correlation else "keep"
                self.last_modes.append(mode)
                obs, teacher = dataset.batch(int(index.numel()), index=index, last_action_mode=mode, seed=self.noise_seed, draw=self.batches_fitted)
                losses.append(self.step(obs, teacher))
                self.batches_fitted += 1
        return torch.stack(losses)


class StudentDriver:
    """SB3-style `predict` over a FLIAStudent on the device: the network's output in eval mode, clamped to [-1, 1]^3 x [0, 1] as
    PolicyDriver clamps.  The student has no distribution: deterministic=False is a ValueError.

    fused_encoder=True: the sphere CNN's two conv blocks run as one te_sphere_encode launch (HIP, fp32 MFMA; the spheres the network
    does not look at are skipped), everything else through the module.  Inference only.  The four conv tensors are packed into one
    device buffer that keeps its address; refresh() repacks the module's current weights into it, in place: call it after every change
    of the module's conv weights (evaluate_policy does, once, before it starts).  Measured on the MI355X the launch takes 0.27 / 1.08 /
    8.5 ms at 2 048 / 8 192 / 65 536 rows of 6 valid spheres against 0.99 / 4.3 / 37.6 ms of the PyTorch formulation of the same two
    blocks, and less with a rollout's masks (profiles/student_encode.json): it was not slower at any size measured.
    At 65 536 rows the PyTorch formulation's one call also differed from its own result computed 8 192 rows at a time (by up to 1.09; its
    intermediates are past 2^31 bytes there), which the launch did not: fly batches of that size through the fused encoder.
    The switch is opt-in because the default must run wherever the module does (a CPU, autograd).

    encoder_precision="bf16" (with fused_encoder=True; the default is "fp32"): the launch is te_sphere_encode_bf16, the same two blocks
    with bf16 operands on the bf16 MFMA under the contract of include/threatengage.h: conv weights, cells and block1's output rounded to
    bf16 (round-to-nearest-even), fp32 accumulation from the fp32 bias, fp32 output in the same buffer, so everything behind the
    encoder is unchanged.  The driver owns a second buffer with the bf16 weights, which keeps its address too; refresh() repacks both.
    The features differ from the fp32 launch's by bf16 rounding (DESIGN.md section 7 has the measured gaps and timings,
    profiles/student_encode_bf16.json the run).  Opt-in because it changes the numbers."""
    accepts_torch = True
    PRECISIONS = ("fp32", "bf16")

    def __init__(self, student: FLIAStudent, fused_encoder: bool = False, encoder_precision: str = "fp32"):
        if not isinstance(student, FLIAStudent):
            raise TypeError("StudentDriver: student must be a FLIAStudent")
        if encoder_precision not in self.PRECISIONS:
            raise ValueError(f"StudentDriver: encoder_precision must be one of {self.PRECISIONS}, not {encoder_precision!r}")
        if encoder_precision == "bf16" and not fused_encoder:
            raise ValueError("StudentDriver: encoder_precision='bf16' is the HIP kernel te_sphere_encode_bf16 and needs fused_encoder=True; "
                             "the PyTorch formulation has no bf16 form")
        self.student = student
        self.fused_encoder = bool(fused_encoder)
        self.encoder_precision = encoder_precision
        self.low = None
        if self.fused_encoder:
            self.device = next(student.parameters()).device
            if self.device.type != "cuda":
                raise ValueError("StudentDriver(fused_encoder=True) runs the HIP kernel te_sphere_encode: the student must live on a GPU")
            self.params = torch.empty(_conv_layout_words("StudentDriver", student), dtype=torch.float32, device=self.device)
            self.weights_bf16 = None
            if self.encoder_precision == "bf16":
                words = C.c_size_t()
                _lib.call("te_sphere_bf16_words", student.lidar_shape[0], C.byref(words))
                self.weights_bf16 = torch.empty(int(words.value), dtype=torch.int16, device=self.device)   # bf16 bit patterns
            self._out = None
            self.refresh()

    @torch.no_grad()
    def refresh(self) -> None:
        if self.fused_encoder:
            torch.cat([p.detach().reshape(-1) for p in _conv_tensors(self.student)], out=self.params)
            if self.weights_bf16 is not None:
                _lib.call_on(self.device, "te_sphere_pack_bf16", self.params.data_ptr(), self.student.lidar_shape[0], self.weights_bf16.data_ptr())

    def encode(self, stacked: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        """te_sphere_encode (te_sphere_encode_bf16 with encoder_precision="bf16"): stacked [B, N, 3, 13, 26] f32, mask [B, N] uint8 /
        bool or None (every sphere counts) -> [B, N, 1792] f32; a buffer of this object, overwritten by the next call of the same
        batch size."""
        if not self.fused_encoder:
            raise ValueError("StudentDriver.encode: built with fused_encoder=False")
        B, N = int(stacked.shape[0]), int(stacked.shape[1])
        _lib.require_f32("StudentDriver.encode", "stacked_spheres", stacked, (B, N, *self.student.lidar_shape), self.device)
        if mask is not None:
            mask = _lib.require_bytes("StudentDriver.encode", "validity_mask", mask, (B, N), self.device)
        if self._out is None or self._out.shape[:2] != (B, N):
            self._out = torch.empty((B, N, SPHERE_FEATURES), dtype=torch.float32, device=self.device)
        _sphere_encode(self.params, self.weights_bf16, stacked, mask, self._out)
        return self._out

    @torch.no_grad()
    def predict(self, observation: Dict[str, torch.Tensor], state=None, episode_start=None, deterministic: bool = True):
        if not deterministic:
            raise ValueError("StudentDriver.predict: the student has no distribution to sample from: deterministic must be True")
        was_training = self.student.training
        self.student.eval()
        try:
            if self.fused_encoder:
                obs = dict(observation, stacked_spheres=observation["stacked_spheres"].contiguous(),
                           validity_mask=observation["validity_mask"].contiguous())
                a = self.student(obs, self.encode(obs["stacked_spheres"], obs["validity_mask"]))
            else:
                a = self.student(observation)
        finally:
            self.student.train(was_training)
        if self.low is None:
            self.low = torch.tensor([-1.0, -1.0, -1.0, 0.0], device=a.device)
        return torch.max(torch.min(a, torch.ones_like(a)), self.low), None
