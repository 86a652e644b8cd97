// te_rollout.hpp — the PPO learner's advantage arithmetic (te_rollout_gae, te_adv_stats; include/threatengage.h).  Generic over the
// rollout's shape: nothing here knows the policy or the environments.
//
//   rollout_gae_kernel        GAE(lambda) over a [T][N] rollout, one thread per env walking t = T - 1 ... 0 (RolloutBuffer.finish of
//                             dronechase_amd/ppo.py, operation for operation, every operation rounded to fp32: contraction is off in the
//                             body, so no product is fused into the sum that follows it).  A wave reads 64 consecutive floats of a
//                             row; the loads of kGaeUnroll steps are issued before the carried chain consumes them.  No LDS, no atomics.
//   adv_stats_partial_kernel  256-thread workgroups, each owning the fixed slice [b kStatSlice, (b + 1) kStatSlice) of the n elements
//                             x[index[i]] (x[i] without an index): thread t takes elements t, t + 256, ... of the slice, sums d and d^2
//                             in fp64 with d = x - pivot (the first element: exact in fp64, and a constant input sums to exactly 0), a
//                             fixed tree over the 256 threads (opt_block_sum), one pair of fp64 partials per slice into the workspace.
//   adv_stats_final_kernel    one workgroup: thread t sums partials t, t + 256, ... in index order, the same tree, then
//                             mean = pivot + S1 / n and the unbiased std = sqrt((S2 - S1^2 / n) / (n - 1)) as two floats.
//
// No atomics: the partition depends on n only, every sum has a fixed order, so repeated calls are bitwise equal and an indexed call
// equals the call on the gathered elements.  The kernel boundary orders the partials between the two launches.
#pragma once

#include <cstddef>
#include <cstdint>

#include "te_policy_opt.hpp"             // opt_block_sum: the fixed tree over 256 threads

namespace te {

constexpr int kGaeThreads = 64;          // one wave per workgroup: 128 workgroups at 8 192 envs, spread over as many CUs
constexpr int kGaeUnroll = 8;            // steps whose loads are in flight together: 24 VGPRs of rewards, values and dones
constexpr int kStatThreads = 256;
constexpr int kStatSlice = 4096;         // elements per workgroup: 16 per thread; 2 048 workgroups for a 128 x 65 536 rollout
static_assert(kStatThreads == kOptThreads, "opt_block_sum reduces kOptThreads threads");
static_assert(kStatSlice % kStatThreads == 0, "a slice is whole rounds of the workgroup");

inline size_t stat_slices(int64_t n) { return ((size_t)n + kStatSlice - 1) / kStatSlice; }
inline size_t stat_workspace_bytes(int64_t n) { return stat_slices(n) * 2 * sizeof(double); }   // {sum d, sum d^2} per slice

struct GaeArgs {
  const float* r; const float* v; const float* d; const float* last_value;
  float* adv; float* ret;
  int n_steps, n_envs;
  float gamma, gamma_lambda;             // fl32(gamma), fl32(gamma * lambda) with the product formed in double on the host
};

__device__ inline void gae_step(float r, float v, float d, float gamma, float gamma_lambda, float& nxt, float& gae, float* adv, float* ret) {
#pragma clang fp contract(off)
  const float nt = 1.f - d;
  const float delta = (r + (gamma * nxt) * nt) - v;
  gae = delta + (gamma_lambda * nt) * gae;
  nxt = v;
  *adv = gae;
  *ret = gae + v;
}

__global__ __launch_bounds__(kGaeThreads) void rollout_gae_kernel(GaeArgs a) {
  const int e = (int)(blockIdx.x * kGaeThreads + threadIdx.x);
  if (e >= a.n_envs) return;             // the last wave is partial when N is not a multiple of 64
  const float* __restrict__ r = a.r; const float* __restrict__ v = a.v; const float* __restrict__ d = a.d;
  float* __restrict__ adv = a.adv; float* __restrict__ ret = a.ret;
  const size_t N = (size_t)a.n_envs;
  float nxt = a.last_value[e], gae = 0.f;
  int t = a.n_steps;
  for (int k = a.n_steps % kGaeUnroll; k > 0; --k) {      // the steps that do not fill a round, from the end of the rollout
    --t;
    const size_t i = (size_t)t * N + e;
    gae_step(r[i], v[i], d[i], a.gamma, a.gamma_lambda, nxt, gae, adv + i, ret + i);
  }
  for (; t > 0; t -= kGaeUnroll) {       // t is a multiple of kGaeUnroll here: rows t - 1 ... t - kGaeUnroll
    float rr[kGaeUnroll], vv[kGaeUnroll], dd[kGaeUnroll];
#pragma unroll
    for (int j = 0; j < kGaeUnroll; ++j) {
      const size_t i = (size_t)(t - 1 - j) * N + e;
      rr[j] = r[i]; vv[j] = v[i]; dd[j] = d[i];
    }
#pragma unroll
    for (int j = 0; j < kGaeUnroll; ++j) {
      const size_t i = (size_t)(t - 1 - j) * N + e;
      gae_step(rr[j], vv[j], dd[j], a.gamma, a.gamma_lambda, nxt, gae, adv + i, ret + i);
    }
  }
}

__device__ inline float stat_element(const float* x, const int64_t* index, int64_t i) { return x[index ? index[i] : i]; }

template <bool Indexed>
__global__ __launch_bounds__(kStatThreads) void adv_stats_partial_kernel(const float* __restrict__ x, const int64_t* __restrict__ index,
                                                                         int64_t n, double* __restrict__ partials) {
  __shared__ double wave_s1[kStatThreads / 64], wave_s2[kStatThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kStatSlice + threadIdx.x;
  const double pivot = (double)stat_element(x, Indexed ? index : nullptr, 0);
  float q[kStatSlice / kStatThreads];
#pragma unroll
  for (int j = 0; j < kStatSlice / kStatThreads; ++j) {   // all 16 loads (32 with an index) issued before the first sum
    const int64_t i = base + (int64_t)j * kStatThreads;
    q[j] = i < n ? stat_element(x, Indexed ? index : nullptr, i) : 0.f;
  }
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int j = 0; j < kStatSlice / kStatThreads; ++j) {
    const int64_t i = base + (int64_t)j * kStatThreads;
    const double dv = i < n ? (double)q[j] - pivot : 0.0;
    s1 += dv; s2 += dv * dv;
  }
  s1 = opt_block_sum(s1, wave_s1);
  s2 = opt_block_sum(s2, wave_s2);
  if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = s1; partials[2 * (size_t)blockIdx.x + 1] = s2; }
}

__global__ __launch_bounds__(kStatThreads) void adv_stats_final_kernel(const float* __restrict__ x, const int64_t* __restrict__ index,
                                                                       int64_t n, const double* __restrict__ partials, int64_t n_slices,
                                                                       float* __restrict__ out_mean_std) {
  __shared__ double wave_s1[kStatThreads / 64], wave_s2[kStatThreads / 64];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = threadIdx.x; i < n_slices; i += kStatThreads) { s1 += partials[2 * i]; s2 += partials[2 * i + 1]; }
  s1 = opt_block_sum(s1, wave_s1);
  s2 = opt_block_sum(s2, wave_s2);
  if (threadIdx.x == 0) {
    const double pivot = (double)stat_element(x, index, 0), cnt = (double)n;
    const double m2 = s2 - s1 * s1 / cnt;                 // the comparison's form lets a NaN through; n = 1: 0 / 0 = NaN, as torch.std
    out_mean_std[0] = (float)(pivot + s1 / cnt);
    out_mean_std[1] = (float)sqrt((m2 < 0.0 ? 0.0 : m2) / (cnt - 1.0));
  }
}

}  // namespace te
