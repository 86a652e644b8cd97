// te_policy_opt.hpp — the PPO learner's optimiser step (te_policy_adam_step, include/threatengage.h): clip_grad_norm_ and torch's
// non-fused Adam over ONE flat fp32 buffer of `words` parameters, in two launches.  Generic over the word count: nothing here knows
// the policy's layers (no pol_layer, no MFMA).
//
//   policy_gradnorm_kernel  256-thread workgroups, each owning the fixed slice [b kOptSlice, (b + 1) kOptSlice) of the gradient: thread t
//                           sums (grad_scale g)^2 over float4 t, t + 256, ... of the slice (and word 4 n4 + t of a tail shorter than
//                           a float4), the 256 sums are reduced by a fixed tree (xor butterfly per wave, the 4 waves in index order)
//                           and thread 0 stores the slice's partial.  Thread 0 of workgroup 0 also advances the step counter.
//   policy_adam_kernel      the same grid over the same slices.  Every workgroup re-sums ALL partials (thread t takes partials t,
//                           t + 256, ... in index order, in fp64, then the same fixed tree: every workgroup gets the same bits), forms
//                           the clip coefficient and applies Adam to its slice; thread 0 computes the two bias corrections of step t
//                           in fp64 and hands them over through LDS.  Workgroup 0 stores the norm and the coefficient for logging.
//
// No atomics at all: every sum has a fixed order, so a step depends on its inputs only.  The kernel boundary orders the partials and
// the step counter between the two launches.  Traffic of a step: g twice, p, m, v read and written = 28 bytes per word (6.6 MB for
// the policy's 235 049 words, L2-resident): the step is bound by its two launches.
//
// policy_adam_kernel<true> (te_policy_adam_step_bf16) is the same step with one addition: the thread that has just computed word w of a
// weight also stores its bf16 rounding (nearest-even, the `(__bf16)` conversion of the pack kernels) where te_policy_pack_bf16 and
// te_policy_pack_bf16_grad would put it, so the rounded copies are current when the step ends and no repack launch follows.  This header
// still knows no layer: the word ranges and the destinations' strides arrive as a table, OptRepack, which the host derives from the pack
// kernels' own plans.  Pad columns are not words of `params`: nobody writes them here, they keep the zeros of the first pack.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace te {

constexpr int kOptThreads = 256;
constexpr int kOptSlice = 4096;          // words per workgroup: 4 float4 per thread; 58 workgroups for the policy's 235 049 words
constexpr int kOptHeaderBytes = 64;      // word 0: step (i32); word 1: the last call's ||grad_scale g|| (f32); word 2: its clip coefficient (f32); rest zero
static_assert(kOptSlice % (4 * kOptThreads) == 0, "a slice is whole float4 rounds of the workgroup");

struct OptLayout {                       // byte offsets inside the state buffer (the public layout of include/threatengage.h)
  size_t m, v, partials, n_partials, bytes;
};

inline size_t opt_align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline OptLayout opt_layout(size_t words) {
  OptLayout o;
  o.n_partials = (words + kOptSlice - 1) / kOptSlice;
  o.m = kOptHeaderBytes;
  o.v = o.m + opt_align16(words * 4);
  o.partials = o.v + opt_align16(words * 4);
  o.bytes = o.partials + opt_align16(o.n_partials * 4);
  return o;
}

struct OptView {                         // the state's arrays as the kernels address them
  int* step; float* norm; float* coef;
  float* m; float* v; float* partials;
  size_t words;
  int n_partials;
};

inline OptView opt_view(void* state, size_t words) {
  const OptLayout o = opt_layout(words);
  char* b = static_cast<char*>(state);
  float* head = reinterpret_cast<float*>(b);
  return OptView{reinterpret_cast<int*>(b), head + 1, head + 2, reinterpret_cast<float*>(b + o.m), reinterpret_cast<float*>(b + o.v),
                 reinterpret_cast<float*>(b + o.partials), words, (int)o.n_partials};
}

struct AdamArgs {                        // the call's scalars, by value: a captured graph replays them as they were
  double lr, beta1, beta2;
  float b1, b2, one_minus_b1, one_minus_b2, eps, max_norm, scale;
};

// Where the bf16 roundings of the stepped words go.  Range r covers the words [src, end) of one weight [N][K], row-major; word
// src + n K + k goes to out[dst + n Kp + k] and, when the range has a transposed block (dst_t >= 0) and out_t is given, to
// out_t[dst_t + k Np + n].  Words outside every range (biases, mu, value, log_std) have no bf16 copy; an unused range is empty.
// A kernel argument by value: index `r` with compile-time constants only.
constexpr int kOptRepackRanges = 16;
struct OptRepack {
  struct { int src, end, K, Kp, dst, Np, dst_t; } r[kOptRepackRanges];
  __bf16 *out, *out_t;
};
struct OptNoRepack {};                   // policy_adam_kernel<false>'s: te_policy_adam_step

__device__ inline void opt_repack_word(const OptRepack& t, int w, float p) {
  int src = 0, K = 1, Kp = 0, dst = -1, Np = 0, dst_t = -1;
#pragma unroll
  for (int i = 0; i < kOptRepackRanges; ++i)
    if (w >= t.r[i].src && w < t.r[i].end) { src = t.r[i].src; K = t.r[i].K; Kp = t.r[i].Kp; dst = t.r[i].dst; Np = t.r[i].Np; dst_t = t.r[i].dst_t; }
  if (dst < 0) return;
  const int e = w - src, n = e / K, k = e - n * K;
  const __bf16 h = (__bf16)p;
  t.out[dst + n * Kp + k] = h;
  if (t.out_t && dst_t >= 0) t.out_t[dst_t + k * Np + n] = h;
}

template <typename T>
__device__ inline T opt_block_sum(T x, T* wave_sums) {   // a fixed tree over the 256 threads; every thread returns the total
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__device__ inline int opt_slice_words(size_t words, size_t base) {
  const size_t left = words - base;
  return left < (size_t)kOptSlice ? (int)left : kOptSlice;
}

__global__ __launch_bounds__(kOptThreads) void policy_gradnorm_kernel(OptView o, const float* __restrict__ grad, float scale) {
  __shared__ float wave_sums[kOptThreads / 64];
  const size_t base = (size_t)blockIdx.x * kOptSlice;
  const int n = opt_slice_words(o.words, base), n4 = n >> 2;
  const float* g = grad + base;          // 16-byte aligned: grad is, and a slice is a multiple of 4 words
  float acc = 0.f;
  for (int i = threadIdx.x; i < n4; i += kOptThreads) {
    const float4 q = reinterpret_cast<const float4*>(g)[i];
    const float x = scale * q.x, y = scale * q.y, z = scale * q.z, w = scale * q.w;
    acc = fmaf(x, x, acc); acc = fmaf(y, y, acc); acc = fmaf(z, z, acc); acc = fmaf(w, w, acc);
  }
  const int tail = (n4 << 2) + (int)threadIdx.x;
  if (tail < n) {
    const float x = scale * g[tail];
    acc = fmaf(x, x, acc);
  }
  const float total = opt_block_sum(acc, wave_sums);
  if (threadIdx.x == 0) {
    o.partials[blockIdx.x] = total;
    if (blockIdx.x == 0) *o.step += 1;
  }
}

__device__ inline double opt_pow(double b, int t) {      // b^t by squaring, fp64: at most 31 rounded products
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

__device__ inline void opt_adam(float g, float& p, float& m, float& v, const AdamArgs& a, float coef, float step_size, float bc2_sqrt) {
  const float gs = coef * (a.scale * g);
  m = fmaf(a.b1, m, a.one_minus_b1 * gs);
  v = fmaf(a.b2, v, a.one_minus_b2 * (gs * gs));
  p -= step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
}

template <bool REPACK>
__global__ __launch_bounds__(kOptThreads) void policy_adam_kernel(OptView o, float* __restrict__ params, const float* __restrict__ grad,
                                                                  AdamArgs a, std::conditional_t<REPACK, OptRepack, OptNoRepack> repack) {
  __shared__ double wave_sums[kOptThreads / 64];
  __shared__ float bias[2];              // lr / (1 - beta1^t), sqrt(1 - beta2^t)
  double part = 0.0;
  for (int i = threadIdx.x; i < o.n_partials; i += kOptThreads) part += (double)o.partials[i];
  if (threadIdx.x == 0) {                // fp64: 1 - 0.999f is already 4.7e-5 off 0.001
    const int t = *o.step;
    bias[0] = (float)(a.lr / (1.0 - opt_pow(a.beta1, t)));
    bias[1] = (float)sqrt(1.0 - opt_pow(a.beta2, t));
  }
  const float norm = (float)sqrt(opt_block_sum(part, wave_sums));   // its barrier also publishes bias[]
  // clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); the comparison's form lets a NaN norm through, as torch's clamp does
  const float c = a.max_norm / (norm + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;
  const float step_size = bias[0], bc2_sqrt = bias[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) { *o.norm = norm; *o.coef = coef; }

  const size_t base = (size_t)blockIdx.x * kOptSlice;
  const int n = opt_slice_words(o.words, base), n4 = n >> 2;
  const float* g = grad + base;
  float *p = params + base, *m = o.m + base, *v = o.v + base;
  for (int i = threadIdx.x; i < n4; i += kOptThreads) {
    const float4 gq = reinterpret_cast<const float4*>(g)[i];
    float4 pq = reinterpret_cast<float4*>(p)[i], mq = reinterpret_cast<float4*>(m)[i], vq = reinterpret_cast<float4*>(v)[i];
    opt_adam(gq.x, pq.x, mq.x, vq.x, a, coef, step_size, bc2_sqrt);
    opt_adam(gq.y, pq.y, mq.y, vq.y, a, coef, step_size, bc2_sqrt);
    opt_adam(gq.z, pq.z, mq.z, vq.z, a, coef, step_size, bc2_sqrt);
    opt_adam(gq.w, pq.w, mq.w, vq.w, a, coef, step_size, bc2_sqrt);
    reinterpret_cast<float4*>(p)[i] = pq; reinterpret_cast<float4*>(m)[i] = mq; reinterpret_cast<float4*>(v)[i] = vq;
    if constexpr (REPACK) {              // a float4 may straddle two rows or two layers (K = 15, K = 4): word by word
      const int w = (int)base + 4 * i;
      opt_repack_word(repack, w, pq.x); opt_repack_word(repack, w + 1, pq.y);
      opt_repack_word(repack, w + 2, pq.z); opt_repack_word(repack, w + 3, pq.w);
    }
  }
  const int tail = (n4 << 2) + (int)threadIdx.x;
  if (tail < n) {
    opt_adam(g[tail], p[tail], m[tail], v[tail], a, coef, step_size, bc2_sqrt);
    if constexpr (REPACK) opt_repack_word(repack, (int)base + tail, p[tail]);
  }
}

// te_policy_ppo_epoch's log, behind every minibatch's step: the gradient call's four statistics and the step's norm before clipping
// are added to the caller's running sums.  One thread, five fp32 adds in index order: the adds PPO.update() makes from Python.
__global__ void policy_epoch_sums_kernel(float* sums, const float* stats, const float* norm) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) sums[i] += stats[i];
  sums[4] += *norm;
}

}  // namespace te
