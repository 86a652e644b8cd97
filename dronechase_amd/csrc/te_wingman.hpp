// te_wingman.hpp — the caller-driven pursuer (exp05's ally, Evaluation_Task's "nn" drivers): its observation, its drive and its info
// rows.  The C ABI on top of these kernels is te_env.hip's te_observe_wingman / te_observe_ally, te_set_wingman_actions /
// te_set_ally_actions, te_drive_wingman / te_drive_wingman_bf16 and te_wingman_info.
//
// The observation is Exp05_vFinal_Task.compute_lw_observation (exp05_vFinal_task.py:265-292) of pursuer `me`: the LIDAR cell and range
// of every other armed drone seen from the pursuer's IMU attitude, patched into a sphere of ones.  Same rules as the agent's sphere:
// closer wins in slot order, empty right after a reset.  It has two schedules, chosen per te_env by plan_kernels (te_env.hip):
//   observe_ally_kernel   one launch, one 256-thread workgroup per chunk of 64 envs: the last wave streams the chunk's tile while the
//                         others compute the features into LDS; after the barrier every wave patches the owned cells.
//   ally_view_kernel      two launches for full-size shards (48 us instead of 64 at 65 536 envs).  Single-wave workgroups: `n_fill`
//   + ally_patch_kernel   of them stream the background in the sub-step kernel's fill-wave shape while one wave per chunk (lane = env)
//                         computes cells / ranges / owners and leaves them as (cell | type << 16, r_hat) planes in a scratch buffer,
//                         and writes the per-env rows; then one thread per (env, drone) patches the owners into the finished background.
// Both are built from the same pieces below, each rule stated once: wingman_frame, wingman_feature, owns_cell, patch_cell, wingman_rows.
//
// Reference citations are file:line under the reference's src/ tree.
#pragma once

#include "te_logic.hpp"
#include "te_policy.hpp"
#include "te_policy_bf16.hpp"

namespace te {

constexpr uint32_t kNoCell = 0xFFFFFFFFu;   // a drone that leaves no feature (the observer itself, a disarmed drone); its r_hat is 1.0

// The observer's frame of pursuer `me`: world -> body rotation of its IMU attitude (the inverse quaternion) and its IMU position
struct WingFrame { M3 R; V3 own; };
TE_DEV WingFrame wingman_frame(const GView& v, int me) {
  const Q4 q = quat_of_euler(V3{v.gf(TE_D_OBS_EULER, me), v.gf(TE_D_OBS_EULER + 1, me), v.gf(TE_D_OBS_EULER + 2, me)});
  const float n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
  return WingFrame{rotation(Q4{-q.x / n2, -q.y / n2, -q.z / n2, q.w / n2}), obs_pos(v, me)};
}
// The feature drone j leaves in that frame: (cell, r_hat), or (kNoCell, 1.0)
TE_DEV void wingman_feature(const te_config& c, const GView& v, const WingFrame& f, int me, int j, uint32_t& cell, float& rhat) {
  cell = kNoCell; rhat = 1.0f;
  if (j != me && v.gi(TE_D_ARMED, j)) { int cj; lidar_cell(c, mul(f.R, sub(obs_pos(v, j), f.own)), cj, rhat); cell = (uint32_t)cj; }
}
// Does drone j own its cell?  s_cell / s_rhat: the features of lane l's env, [D][kEPB].  Owner of a cell = smallest range, the earlier
// slot on ties (strict '<' in slot order, lidar_math.py:262-311); a feature clipped to 1.0 never enters an empty cell.
TE_DEV bool owns_cell(const uint32_t* s_cell, const float* s_rhat, int l, int D, int j, uint32_t& cell, float& rhat) {
  cell = s_cell[j * kEPB + l];
  rhat = s_rhat[j * kEPB + l];
  if (cell == kNoCell || !(rhat < 1.0f)) return false;
  bool owner = true;
  for (int k = 0; k < D; ++k) {
    if (k == j || s_cell[k * kEPB + l] != cell) continue;
    const float rk = s_rhat[k * kEPB + l];
    if (rk < rhat || (rk == rhat && k < j)) owner = false;
  }
  return owner;
}
TE_DEV uint32_t feature_type(const te_config& c, int j) { return j < c.n_pursuers ? TE_TYPE_LOYALWINGMAN : TE_TYPE_LOITERINGMUNITION; }
// One owned cell into the sphere at `base`: range, type / 5, and 0.1 in the time plane when the sphere has one
TE_DEV void patch_cell(const te_config& c, float* __restrict__ base, uint32_t cell, float rhat, uint32_t type) {
  base[cell] = rhat;
  base[TE_LIDAR_CELLS + cell] = (float)type / 5.0f;
  if (c.lidar_channels != 2) base[2 * TE_LIDAR_CELLS + cell] = 0.1f;
}
// The per-env rows of pursuer `me` of env v.env: armed flag, the action it was last driven with, inertial row
TE_DEV void wingman_rows(const te_config& c, const GView& v, int me, int step, float* __restrict__ inertial, float* __restrict__ last_action,
                         uint8_t* __restrict__ active) {
  if (active) active[v.env] = v.gi(TE_D_ARMED, me) ? 1 : 0;
  if (last_action)
    reinterpret_cast<float4*>(last_action)[v.env] = make_float4(v.gf(TE_D_ALLY_ACTION, me), v.gf(TE_D_ALLY_ACTION + 1, me),
                                                                 v.gf(TE_D_ALLY_ACTION + 2, me), v.gf(TE_D_ALLY_ACTION + 3, me));
  if (inertial) inertial_obs_row(c, v, step, me, inertial + (size_t)v.env * TE_OBS_INERTIAL_WORDS);
}

__global__ __launch_bounds__(256) void observe_ally_kernel(Params p, int me, float* __restrict__ lidar, float* __restrict__ inertial,
                                                           float* __restrict__ last_action, uint8_t* __restrict__ active) {
  __shared__ uint32_t s_cell[kMaxD * kEPB];
  __shared__ float s_rhat[kMaxD * kEPB];
  const te_config& c = p.cfg;
  const int D = p.D;
  const int env0 = blockIdx.x * kEPB, nvalid = min(kEPB, p.N - env0);
  const int l = threadIdx.x & (kEPB - 1), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const bool valid = l < nvalid;
  const GView v{p.dstate, p.estate, D, p.Npad, env0 + l, c.n_pursuers};   // planes are padded to Npad: in bounds for every lane
  const int step = v.egi(TE_E_STEP);
  const bool sees = lidar && valid && step != 0;
  // wave roles: the last wave only streams the tile (a wave that has stores in flight waits for them before any later
  // load returns: in-order vmcnt), the others compute the features meanwhile
  const int nfeat = nw - 1;
  if (sees && w < nfeat) {
    const WingFrame f = wingman_frame(v, me);
    for (int j = w; j < D; j += nfeat) {
      uint32_t cell; float rhat;
      wingman_feature(c, v, f, me, j, cell, rhat);
      s_cell[j * kEPB + l] = cell; s_rhat[j * kEPB + l] = rhat;
    }
  }
  if (lidar && w == nfeat) {  // the chunk's tile: 64 * 1014 floats, 16-byte aligned; non-temporal like the sub-step kernel's background
    float* tile = lidar + (size_t)env0 * lidar_words(c);
    const int total = nvalid * lidar_words(c), quads = total >> 2;
    for (int qi = l; qi < quads; qi += kEPB) TE_FILL_STORE(reinterpret_cast<float4*>(tile) + qi);
    for (int f = (quads << 2) + l; f < total; f += kEPB) tile[f] = 1.0f;
  }
  if (w == 0 && valid) wingman_rows(c, v, me, step, inertial, last_action, active);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the ones must have landed before any patch
  __syncthreads();
  if (!sees) return;
  float* base = lidar + (size_t)(env0 + l) * lidar_words(c);
  for (int j = w; j < D; j += nw) {
    uint32_t cell; float rhat;
    if (owns_cell(s_cell, s_rhat, l, D, j, cell, rhat)) patch_cell(c, base, cell, rhat, feature_type(c, j));
  }
}

__global__ __launch_bounds__(64) void ally_view_kernel(Params p, int me, float* __restrict__ lidar, uint32_t quads, uint32_t n_fill,
                                                       float* __restrict__ inertial, float* __restrict__ last_action,
                                                       uint8_t* __restrict__ active, uint32_t* __restrict__ scratch) {
  __shared__ uint32_t s_cell[kMaxD * kEPB];
  __shared__ float s_rhat[kMaxD * kEPB];
  const int l = threadIdx.x;
  if (blockIdx.x < n_fill) {
    const uint32_t stride = n_fill * 64u;
    for (uint32_t q = blockIdx.x * 64u + (uint32_t)l; q < quads; q += stride) TE_FILL_STORE(reinterpret_cast<float4*>(lidar) + q);
    return;
  }
  const te_config& c = p.cfg;
  const int D = p.D;
  const int env = (int)(blockIdx.x - n_fill) * kEPB + l;
  const bool valid = env < p.N;
  const GView v{p.dstate, p.estate, D, p.Npad, env, c.n_pursuers};   // planes are padded to Npad: in bounds for every lane
  const int step = v.egi(TE_E_STEP);
  const bool sees = valid && step != 0;
  if (sees) {
    const WingFrame f = wingman_frame(v, me);
    for (int j = 0; j < D; ++j) {
      uint32_t cell; float rhat;
      wingman_feature(c, v, f, me, j, cell, rhat);
      s_cell[j * kEPB + l] = cell; s_rhat[j * kEPB + l] = rhat;
    }
  }
  if (valid) wingman_rows(c, v, me, step, inertial, last_action, active);
  // (each lane reads back only what it wrote: no barrier)
  for (int j = 0; j < D; ++j) {
    uint32_t out = kNoCell, cell; float rh = 1.0f, rhat;
    if (sees && owns_cell(s_cell, s_rhat, l, D, j, cell, rhat)) { out = cell | (feature_type(c, j) << 16); rh = rhat; }
    scratch[(size_t)(2 * j) * p.Npad + env] = out; scratch[(size_t)(2 * j + 1) * p.Npad + env] = __float_as_uint(rh);
  }
}
__global__ __launch_bounds__(256) void ally_patch_kernel(Params p, float* __restrict__ lidar, const uint32_t* __restrict__ scratch) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)p.D * p.Npad) return;
  const int j = (int)(i / p.Npad), env = (int)(i - (size_t)j * p.Npad);
  if (env >= p.N) return;
  const uint32_t w = scratch[(size_t)(2 * j) * p.Npad + env];
  if (w == kNoCell) return;
  patch_cell(p.cfg, lidar + (size_t)env * lidar_words(p.cfg), w & 0xFFFFu, __uint_as_float(scratch[(size_t)(2 * j + 1) * p.Npad + env]), w >> 16);
}

// exp05: pursuer.drive(action) of drive_lw_rl_agent (exp05_vFinal_task.py:255-260; quadcopter.py:379-413) for an armed pursuer
// `me` of env v: the velocity command, the set-point, and the action remembered as the pursuer's last action.
TE_DEV void drive_caller_pursuer(const GView& v, int me, float4 a) {
  float vx, vy, vz;
  command_to_velocity(a.x, a.y, a.z, a.w, vx, vy, vz);
  v.sf(TE_X_CMD + 0, me, vx); v.sf(TE_X_CMD + 1, me, vy); v.sf(TE_X_CMD + 2, me, vz);
  v.sf(TE_D_SETPOINT + 0, me, vx); v.sf(TE_D_SETPOINT + 1, me, vy); v.sf(TE_D_SETPOINT + 2, me, 0.0f); v.sf(TE_D_SETPOINT + 3, me, vz);
  v.sf(TE_D_ALLY_ACTION + 0, me, a.x); v.sf(TE_D_ALLY_ACTION + 1, me, a.y); v.sf(TE_D_ALLY_ACTION + 2, me, a.z); v.sf(TE_D_ALLY_ACTION + 3, me, a.w);
}

__global__ __launch_bounds__(256) void set_ally_actions_kernel(Params p, int me, const float* __restrict__ actions) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= p.N) return;
  const GView v{p.dstate, p.estate, p.D, p.Npad, env, p.cfg.n_pursuers};
  if (!v.gi(TE_D_ARMED, me)) return;
  drive_caller_pursuer(v, me, reinterpret_cast<const float4*>(actions)[env]);
}

// The tail of both drive kernels, for the thread that computed row `env`'s mean MU[4] (in LDS): mu[env] for every row when mu is
// non-null, then set_ally_actions_kernel's drive with the mean clamped to [-1, 1]^3 x [0, 1] where pursuer `me` is armed.
TE_DEV void drive_with_mean(const Params& p, int me, int env, const float* MU, float* __restrict__ mu) {
  if (mu) {
#pragma unroll
    for (int a = 0; a < 4; ++a) mu[(size_t)env * 4 + a] = MU[a];
  }
  const GView v{p.dstate, p.estate, p.D, p.Npad, env, p.cfg.n_pursuers};
  if (!v.gi(TE_D_ARMED, me)) return;
  drive_caller_pursuer(v, me, make_float4(fmaxf(fminf(MU[0], 1.f), -1.f), fmaxf(fminf(MU[1], 1.f), -1.f), fmaxf(fminf(MU[2], 1.f), -1.f),
                                          fmaxf(fminf(MU[3], 1.f), 0.f)));
}

// te_drive_wingman: the deterministic predict of the packed policy on pursuer `me`'s observation (te_observe_wingman's output,
// read as te_policy_act reads its rows), then set_ally_actions_kernel's drive with the clamped mean.  pol_forward is the one
// policy_act_kernel runs, so mu is bitwise te_policy_act's.  Every row is computed; rows of envs whose pursuer is dead keep
// their state (the reference does not call predict for them), mu is written for all rows.
template <int C, int S = POL_SHAPE_DEFAULT>
__global__ __launch_bounds__(kPolThreads) void policy_drive_kernel(PolicyParams P, PolicyIn in, Params p, int me, float* __restrict__ mu) {
  extern __shared__ __attribute__((aligned(16))) float pol_lds[];
  constexpr int M = pol_lds_plan(pol_shape(S, C)).M;
  const int tid = threadIdx.x, env = blockIdx.x * M + tid;
  pol_forward<C, S>(P, in, pol_lds, blockIdx.x * M, PolNoSave{});
  if (tid >= M || env >= in.n) return;
  drive_with_mean(p, me, env, pol_mu_lds<S>(pol_lds) + tid * 4, mu);   // read back by the thread that computed it
}

// te_drive_wingman_bf16: the same with te_policy_act_bf16's forward (te_policy_bf16.hpp).  pol_forward_bf16 is the one
// policy_act_bf16_kernel runs, on the same tile (pol_lds_plan_bf16: 32 rows of 256 threads for the default shape, 48 rows of 512
// threads for the wide ones), so mu is bitwise te_policy_act_bf16's; the tail is policy_drive_kernel's.
template <int C, int S = POL_SHAPE_DEFAULT>
__global__ __launch_bounds__(pol_lds_plan_bf16(pol_shape(S, C)).threads) void policy_drive_bf16_kernel(PolicyParams P, PolicyBf16 Wb, PolicyIn in,
                                                                                                      Params p, int me, float* __restrict__ mu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_lds_b[];
  constexpr PolLdsB lp = pol_lds_plan_bf16(pol_shape(S, C));
  constexpr int M = lp.M;
  const int tid = threadIdx.x, env = blockIdx.x * M + tid;
  pol_forward_bf16<C, S>(P, Wb, in, pol_lds_b, blockIdx.x * M, PolNoSaveB{});
  if (tid >= M || env >= in.n) return;
  drive_with_mean(p, me, env, reinterpret_cast<const float*>(pol_lds_b) + lp.mu + tid * 4, mu);   // read back by the thread that computed it
}

// Evaluation_Task.compute_info (evaluation_task.py:553-574): (lw_kills, lw_alive, lw_munitions, current_wave, step) per pursuer
__global__ __launch_bounds__(256) void wingman_info_kernel(Params p, int32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x, P = p.cfg.n_pursuers;
  if (i >= p.N * P) return;
  const int env = i / P, s = i - env * P;
  const GView v{p.dstate, p.estate, p.D, p.Npad, env, P};
  int32_t* row = out + (size_t)i * 5;
  row[0] = v.gi(TE_D_KILLS, s); row[1] = v.gi(TE_D_ARMED, s) ? 1 : 0; row[2] = v.gi(TE_D_MUNITION, s);
  row[3] = v.egi(TE_E_INFO_WAVE); row[4] = v.egi(TE_E_STEP);
}

}  // namespace te
