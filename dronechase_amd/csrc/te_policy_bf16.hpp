// te_policy_bf16.hpp — te_policy_act_bf16: the inference of te_policy.hpp with bf16 operands on v_mfma_f32_16x16x32_bf16, opt-in
// (PPOConfig.fused_forward_bf16, FusedPolicy(precision="bf16")).  The fp32 kernels of te_policy.hpp are untouched; this header reuses
// their description of the network (pol_shape, pol_layer, PolicyParams, PolicyIO) and adds a second, bf16 copy of the weights.
//
// Numerics contract (the one rule; include/threatengage.h states it too, tests/test_policy_bf16.py's CPU reference follows it):
//   * Weights are rounded ONCE to bf16, round-to-nearest-even (policy_pack_bf16_kernel); the fp32 packed buffer stays the master copy.
//   * The input of every weight layer is rounded to bf16, round-to-nearest-even, where it is stored for the MFMA: the LIDAR patch,
//     inertial_data, last_action, every hidden activation, the concat, the trunk, the head tiles, and the last hidden tile of each
//     head.  (On gfx950 `(__bf16)x` is v_cvt_pk_bf16_f32.)
//   * Products are accumulated in fp32 by the MFMA; the accumulator starts from the fp32 bias.  ReLU and tanhf run in fp32 on the
//     accumulator; the result is rounded when it is stored.
//   * mu and value stay on the vector ALU, one thread per row: fp32 weights and bias from the fp32 buffer, fmaf over the bf16 last
//     hidden tile in k order.
//   * log_std, the sample, logp and the clamp are policy_act_kernel's tail, in fp32.
//   * The sum order of an output is over k only (k-blocks of 32 in order; within a block the MFMA's own order): a row's outputs do
//     not depend on n, on the tile height, or on the row's place in the tile, and repeated calls are bitwise equal.
//
// Packed bf16 weights: ONE uint16 buffer; per MFMA layer (conv1 .. vf's last hidden layer, in the order of the fp32 buffer) the
// weight [N][Kp], Kp = roundup(K, 32), columns K .. Kp - 1 zero.  Every row is a multiple of 64 bytes, so with a 16-byte aligned
// buffer one B fragment (8 consecutive k of a weight row) is one aligned 16-byte load, also for K = 15 (inertial.0), K = 4 (action.0)
// and K = 48 (conv1 at C = 3).  Biases, mu, value and log_std are NOT in this buffer: they are read from the fp32 one.
//
// Tiles: activations live in LDS as bf16, row stride K + 8 elements.  K is a multiple of 16, so the stride is 4 (mod 8) dwords: the
// 16 rows of an A-fragment read (ds_read_b128) start in 16 different 16-byte slots of the 256-byte bank row.  A ds_read_b128 group is
// 12 lanes of one k-group and 4 of the next (one slot further), so one pair of rows per group still shares a slot: 2-way on 1 slot of
// 16, the same as the guide's row read of this operand; an XOR swizzle would remove it and is not done here.
//   default shape: 32 rows, 256 threads, 46.1 KB: three workgroups (12 waves) per CU.  Its bf16 weights are 0.47 MB, L2-resident
//                  whatever the tile, so a taller tile would save no traffic that matters, and at 64 rows (93 KB) only one workgroup
//                  of 4 waves would fit a CU, with nothing to hide a weight load's latency behind.  Hence 32.
//   F = 512 shapes: 48 rows, 512 threads (8 waves), 141.2 KB: Z + F + the 512-wide head tile at 64 rows would be 191 KB.  Every
//                  workgroup reads all 1.5 / 2.1 MB of bf16 weights for 48 rows, a sixth of the bytes per row of the fp32 kernel's
//                  16-row tile, and the CU holds two waves per SIMD.
//
// The forward itself is pol_forward_bf16<C, S, M>(..., save): the kernel below calls it with a hook that saves nothing, and
// te_policy_grad_bf16.hpp's tile kernel with one that writes every layer's input to its workspace and with a tile height of its own (the
// outputs of a row do not depend on it), so the gradient's forward is this one bit for bit.
#pragma once

namespace te {

typedef __bf16 pol_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pol_bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kPolBPad = 8;                    // bf16 elements (16 bytes) behind every LDS row
constexpr int kPolBZS = 448 + kPolBPad;        // LDS row strides in bf16 elements
constexpr int kPolBTS = 128 + kPolBPad;
constexpr int kPolBMfmaLayers = POL_L_MU;      // the layers of the bf16 buffer: every weight layer below mu and value

__host__ __device__ constexpr int pol_kp(int K) { return (K + 31) / 32 * 32; }

// Element offsets of every layer's weight [N][Kp] in the packed bf16 buffer.  A kernel argument by value, indexed with constants.
struct PolicyBf16 {
  const unsigned short* base;
  int at[kPolBMfmaLayers];
  int words;                                   // uint16 elements in all
};

inline PolicyBf16 policy_bf16_layout(PolShape S) {
  PolicyBf16 w{};
  int o = 0;
  for (int l = 0; l < kPolBMfmaLayers; ++l) {
    const PolLayer y = pol_layer(l, S);
    w.at[l] = o;
    o += y.N * pol_kp(y.K);
  }
  w.words = o;
  return w;
}

// fp32 packed buffer -> bf16 packed buffer in one launch: thread i writes element i of the bf16 buffer (a pad column: zero).
struct PolPackPlan {
  struct { int dst, src, K, Kp; } l[kPolBMfmaLayers];
  int end[kPolBMfmaLayers];                    // dst + N * Kp
  int total;
};

inline PolPackPlan policy_pack_plan(PolShape S) {
  const PolicyParams P = policy_layout(S);
  const PolicyBf16 W = policy_bf16_layout(S);
  PolPackPlan p{};
  for (int l = 0; l < kPolBMfmaLayers; ++l) {
    const PolLayer y = pol_layer(l, S);
    p.l[l] = {W.at[l], P.at[l].w, y.K, pol_kp(y.K)};
    p.end[l] = W.at[l] + y.N * pol_kp(y.K);
  }
  p.total = W.words;
  return p;
}

__global__ __launch_bounds__(256) void policy_pack_bf16_kernel(const float* __restrict__ params, PolPackPlan plan, __bf16* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= plan.total) return;
  int dst = 0, src = 0, K = 1, Kp = 1;
#pragma unroll
  for (int l = kPolBMfmaLayers - 1; l >= 0; --l)     // the layer that holds element i (an absent layer is empty: never chosen)
    if (i < plan.end[l]) { dst = plan.l[l].dst; src = plan.l[l].src; K = plan.l[l].K; Kp = plan.l[l].Kp; }
  const int e = i - dst, n = e / Kp, k = e - n * Kp;
  out[i] = k < K ? (__bf16)params[src + (size_t)n * K + k] : (__bf16)0.f;
}

// The LDS of policy_act_bf16_kernel for a shape.  Tile offsets and strides in bf16 elements from the start of the dynamic LDS; mu and
// val in floats from the start; bytes in all.  Z [M][kPolBZS] at 0, T1 and T2 [M][kPolBTS] behind it; the trunk F [M][fs] over T1 / T2
// (dead by then) and beyond; the heads' tiles B [M][bs] (hidden layer 1) at 0 and A [M][as] (hidden layers 0 and 2) behind B, both
// over the dead Z, when they fit it (default shape), else A behind F; MU [M][4] and VAL [M] in fp32 behind everything.
// tile_m: another tile height for the same map (te_policy_grad_bf16.hpp runs this forward at 32 rows for every shape); 0: the inference's.
struct PolLdsB { int M, threads, t1, t2, f, fs, a, as, b, bs, mu, val, bytes; };

__host__ __device__ constexpr int pol_max(int a, int b) { return a > b ? a : b; }

__host__ __device__ constexpr PolLdsB pol_lds_plan_bf16(PolShape S, int tile_m = 0) {
  const int h1 = S.n_hidden > 1 ? S.h[1] : 0, h2 = S.n_hidden > 2 ? S.h[2] : 0;
  const int fs = S.F + kPolBPad, as = pol_max(S.h[0], h2) + kPolBPad, bs = h1 + kPolBPad;
  const bool wide = S.F > 256;
  const int M = tile_m ? tile_m : (wide ? 48 : 32), threads = wide ? 512 : 256;
  const int t1 = M * kPolBZS, t2 = t1 + M * kPolBTS, f = t1;
  const int a = bs + as <= kPolBZS ? M * bs : f + M * fs;
  const int end = pol_max(pol_max(t2 + M * kPolBTS, f + M * fs), a + M * as);
  const int mu = (end + 7) / 8 * 4;            // 16-byte aligned, in floats
  return {M, threads, t1, t2, f, fs, a, as, 0, bs, mu, mu + 4 * M, (mu + 5 * M) * 4};
}

// A plan is sound when nothing lies over a live tile: F clear of Z (the trunk reads Z), B within the dead Z and clear of A and F,
// A clear of B and F (F stays live through both heads), MU / VAL behind every tile, every tile 16-byte aligned, all within the CU.
__host__ __device__ constexpr bool pol_lds_bf16_ok(PolShape S, int tile_m = 0) {
  const PolLdsB p = pol_lds_plan_bf16(S, tile_m);
  const int z_end = p.M * kPolBZS, f_end = p.f + p.M * p.fs, a_end = p.a + p.M * p.as, b_end = p.b + p.M * p.bs;
  return p.bytes <= kPolLdsLimit && p.M % 16 == 0 && p.M <= p.threads && p.threads % 64 == 0 && p.threads <= 1024 &&
         p.t1 >= z_end && p.t2 >= p.t1 + p.M * kPolBTS && p.f >= z_end && b_end <= z_end && b_end <= p.f &&
         (p.a >= b_end) && (a_end <= p.f || p.a >= f_end) &&
         p.mu * 2 >= pol_max(pol_max(p.t2 + p.M * kPolBTS, f_end), a_end) && p.val >= p.mu + 4 * p.M && p.bytes >= (p.val + p.M) * 4 &&
         p.fs % 8 == 0 && p.as % 8 == 0 && p.bs % 8 == 0 && p.a % 8 == 0 && p.f % 8 == 0 && p.mu % 4 == 0 &&
         (S.F <= 256 || p.M >= 32);
}
static_assert(pol_lds_bf16_ok(pol_shape(POL_SHAPE_DEFAULT, 3)) && pol_lds_plan_bf16(pol_shape(POL_SHAPE_DEFAULT, 3)).bytes * 3 <= kPolLdsLimit,
              "the default shape: three workgroups per CU");
static_assert(pol_lds_bf16_ok(pol_shape(POL_SHAPE_BO, 3)) && pol_lds_plan_bf16(pol_shape(POL_SHAPE_BO, 3)).M >= 32, "h[128, 256, 512] fits a CU at 32 rows or more");
static_assert(pol_lds_bf16_ok(pol_shape(POL_SHAPE_LEARN, 3)) && pol_lds_plan_bf16(pol_shape(POL_SHAPE_LEARN, 3)).M >= 32, "h[512, 128, 256] fits a CU at 32 rows or more");

// Y[16 MT, N] = X[16 MT, K] W^T + init on v_mfma_f32_16x16x32_bf16.  X: bf16 in LDS (row stride ldx elements, a multiple of 8;
// columns K .. Kp - 1 finite, the weights' pad columns are zero); W: [N][Kp] bf16 in global memory.  init(n) starts the accumulator
// of column n; epi(row, col, value) consumes one fp32 output element.  Lane l of a 16 x 16 tile (r = l & 15, h = l >> 4):
// A = X[r][k0 + 8 h + j], B = W[n0 + r][k0 + 8 h + j], j = 0..7: one 16-byte load each; C/D: column r, rows 4 h .. 4 h + 3 (pol_gemm's).
// Wave w of NW owns the 16-column slices w, w + NW, ... for all MT row tiles: one weight load feeds MT MFMAs.
// epi(m0, n, v) takes the four rows m0 .. m0 + 3 a lane holds of column n.  K2 > 0: a second operand pair, X2 [.][K2] and W2 [N][K2p],
// runs into the same accumulator behind the first (the trunk's gradient over both heads, te_policy_grad_bf16.hpp).
template <int K, int N, int MT, int NW, int K2 = 0, class Init, class Epi>
TE_DEV void pol_gemm_bf16(const __bf16* X, int ldx, const __bf16* __restrict__ W, Init init, Epi epi, const __bf16* X2 = nullptr, int ldx2 = 0,
                          const __bf16* __restrict__ W2 = nullptr) {
  static_assert(N % 16 == 0, "whole 16-column slices");
  constexpr int Kp = pol_kp(K), K2p = pol_kp(K2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
  for (int nt = wave; nt < N / 16; nt += NW) {
    const int n = nt * 16 + r;
    const float b0 = init(n);
    pol_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = pol_f32x4{b0, b0, b0, b0};
    const __bf16* wr = W + (size_t)n * Kp + 8 * h;
    const __bf16* xr = X + r * ldx + 8 * h;
#pragma unroll 8
    for (int k0 = 0; k0 < Kp; k0 += 32) {
      const pol_bf16x8 w = *reinterpret_cast<const pol_bf16x8*>(wr + k0);
      pol_bf16x8 a[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const pol_bf16x8*>(xr + 16 * t * ldx + k0);
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], w, acc[t], 0, 0, 0);
    }
    if constexpr (K2 > 0) {
      const __bf16* wr2 = W2 + (size_t)n * K2p + 8 * h;
      const __bf16* xr2 = X2 + r * ldx2 + 8 * h;
#pragma unroll 8
      for (int k0 = 0; k0 < K2p; k0 += 32) {
        const pol_bf16x8 w = *reinterpret_cast<const pol_bf16x8*>(wr2 + k0);
        pol_bf16x8 a[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const pol_bf16x8*>(xr2 + 16 * t * ldx2 + k0);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], w, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) epi(16 * t + 4 * h, n, acc[t]);
  }
}

// The forward of weight layer L of shape S on an M-row tile: Y = act(X W^T + b) with W from the bf16 buffer and b from the fp32 one; the
// fp32 result is rounded to bf16 and handed to store(m0, n, y): rows m0 .. m0 + 3 of column n.
template <int L, int C, int S, int ACT, int M, class Store>
TE_DEV void pol_linear_bf16(const PolicyParams& P, const PolicyBf16& Wb, const __bf16* X, int ldx, Store store) {
  constexpr PolLayer y = pol_layer(L, pol_shape(S, C));
  constexpr PolLdsB lp = pol_lds_plan_bf16(pol_shape(S, C), M);
  const float* __restrict__ bias = P.base + P.at[L].b;
  pol_gemm_bf16<y.K, y.N, lp.M / 16, lp.threads / 64>(
      X, ldx, reinterpret_cast<const __bf16*>(Wb.base) + Wb.at[L], [=](int n) { return bias[n]; },
      [=](int m0, int n, pol_f32x4 v) {
        pol_bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)(ACT == POL_RELU ? fmaxf(v[i], 0.f) : tanhf(v[i]));
        store(m0, n, o);
      });
}

// What pol_forward_bf16 hands to its `save` hook besides keeping it in LDS: every layer's input as the bf16 values the MFMA consumes
// (the buffers of te_policy.hpp's POL_SV_ list).  x4: rows m0 .. m0 + 3 of column col (conv position sub); x1: one element.
struct PolNoSaveB {
  TE_DEV void x4(int, int, int, int, pol_bf16x4) const {}
  TE_DEV void x1(int, int, int, int, __bf16) const {}
};

// rows m0 .. m0 + 3 of one column of an LDS tile with row stride ld
TE_DEV void pol_tile_put4(__bf16* p, int ld, pol_bf16x4 v) { p[0] = v[0]; p[ld] = v[1]; p[2 * ld] = v[2]; p[3 * ld] = v[3]; }

// One head: hidden layers L0, L0 + 1, L0 + 2 (those the shape has) with tanh, F -> A -> B -> A; returns the last one's output.
template <int L0, int C, int S, int M, class Save>
TE_DEV const __bf16* pol_head_bf16(const PolicyParams& P, const PolicyBf16& Wb, const __bf16* F, __bf16* A, __bf16* B, Save save) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolLdsB lp = pol_lds_plan_bf16(sh, M);
  constexpr int last = L0 == POL_L_PI0 ? POL_L_MU : POL_L_V;
  // next: the layer that reads this output, from its saved buffer
  auto to = [=](__bf16* Y, int ld, int next) {
    return [=](int m0, int n, pol_bf16x4 y) { pol_tile_put4(Y + m0 * ld + n, ld, y); save.x4(pol_layer(next, sh).x, m0, 0, n, y); };
  };
  pol_linear_bf16<L0, C, S, POL_TANH, M>(P, Wb, F, lp.fs, to(A, lp.as, sh.n_hidden > 1 ? L0 + 1 : last));
  __syncthreads();
  if constexpr (sh.n_hidden > 1) {
    pol_linear_bf16<L0 + 1, C, S, POL_TANH, M>(P, Wb, A, lp.as, to(B, lp.bs, sh.n_hidden > 2 ? L0 + 2 : last));
    __syncthreads();
  }
  if constexpr (sh.n_hidden > 2) {
    pol_linear_bf16<L0 + 2, C, S, POL_TANH, M>(P, Wb, B, lp.bs, to(A, lp.as, last));
    __syncthreads();
  }
  return sh.n_hidden == 2 ? B : A;
}

// The forward of the tile's M rows from row0 (rows >= in.n read zeros; row i is read at in.index[i], NULL: at i): mu and value of every
// row into MU [M][4] and VAL [M] of pol_lds_plan_bf16(S, M) (fp32); each layer's input also goes to save.  Thread tid < M computes row
// tid's mu and value and may read them back without a barrier.  te_policy_act_bf16 and te_policy_ppo_grad_bf16 both run this: their
// forwards are bitwise one.  M = 0: the inference's tile height.
template <int C, int S, int M = 0, class Save>
TE_DEV void pol_forward_bf16(const PolicyParams& P, const PolicyBf16& Wb, const PolicyIn& in, unsigned char* pol_lds_b, int row0, Save save) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolLdsB lp = pol_lds_plan_bf16(sh, M);
  static_assert(pol_lds_bf16_ok(sh, M), "the tile height fits the shape");
  constexpr int TM = lp.M, MT = TM / 16, NT = lp.threads, NW = NT / 64;
  __bf16* lds = reinterpret_cast<__bf16*>(pol_lds_b);
  __bf16* Z = lds;                             // [TM][kPolBZS]: lidar 0..191 | inertial 192..319 | last_action 320..447
  __bf16* T1 = lds + lp.t1;                    // [TM][kPolBTS]
  __bf16* T2 = lds + lp.t2;                    // [TM][kPolBTS]
  __bf16* F = lds + lp.f;                      // [TM][lp.fs] once T1 / T2 are dead
  __bf16* HA = lds + lp.a;                     // [TM][lp.as], [TM][lp.bs]
  __bf16* HB = lds + lp.b;
  float* MU = reinterpret_cast<float*>(pol_lds_b) + lp.mu;     // [TM][4]
  float* VAL = reinterpret_cast<float*>(pol_lds_b) + lp.val;   // [TM]
  const float* __restrict__ prm = P.base;
  const __bf16* __restrict__ wb = reinterpret_cast<const __bf16*>(Wb.base);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  auto src = [&](int row) -> size_t { return in.index ? (size_t)in.index[row] : (size_t)row; };

  // ---- LIDAR: conv1 + conv2, one conv2 output column (ow2) at a time.  conv1's k = c * 16 + kh * 4 + kw: k-block kb of 32 holds
  // channels 2 kb and 2 kb + 1, lane group h the patch rows kh = 2 (h & 1), + 1 of channel 2 kb + (h >> 1); a channel >= C is the
  // zero pad.  A work item is (conv1 position (oh, j), 16-channel slice nt): 8 per chunk, dealt over the waves.
  for (int ow2 = 0; ow2 < 3; ++ow2) {
    for (int item = wave; item < 8; item += NW) {
      const int pos = item & 3, nt = item >> 2, oh = pos >> 1, j = pos & 1, ow = 2 * ow2 + j, n = nt * 16 + r;
      constexpr int Kp = pol_kp(16 * C);
      const float b = prm[P.at[POL_L_C1].b + n];
      pol_f32x4 acc[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = pol_f32x4{b, b, b, b};
#pragma unroll
      for (int kb = 0; kb < Kp / 32; ++kb) {
        const int c = 2 * kb + (h >> 1), kh = 2 * (h & 1);
        const pol_bf16x8 w = *reinterpret_cast<const pol_bf16x8*>(wb + Wb.at[POL_L_C1] + n * Kp + kb * 32 + 8 * h);
        pol_bf16x8 a[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int row = row0 + 16 * t + r;
          float2 p0 = make_float2(0.f, 0.f), p1 = p0, p2 = p0, p3 = p0;
          if (c < C && row < in.n) {
            const float* s = in.lidar + (src(row) * C + c) * (13 * 26) + (4 * oh + kh) * 26 + 4 * ow;
            p0 = *reinterpret_cast<const float2*>(s);      p1 = *reinterpret_cast<const float2*>(s + 2);
            p2 = *reinterpret_cast<const float2*>(s + 26); p3 = *reinterpret_cast<const float2*>(s + 28);
          }
          a[t] = pol_bf16x8{(__bf16)p0.x, (__bf16)p0.y, (__bf16)p1.x, (__bf16)p1.y, (__bf16)p2.x, (__bf16)p2.y, (__bf16)p3.x, (__bf16)p3.y};
          if (nt == 0 && c < C) {      // the patch as the MFMA reads it: column kb * 32 + 8 h + e = c * 16 + kh * 4 + kw
#pragma unroll
            for (int e = 0; e < 8; ++e) save.x1(POL_SV_C1X, 16 * t + r, ow2 * 4 + oh * 2 + j, kb * 32 + 8 * h + e, a[t][e]);
          }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], w, acc[t], 0, 0, 0);
      }
      // conv1 output (row, co, oh, ow) -> conv2 patch of column ow2: T1[row][co * 4 + oh * 2 + j]
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        pol_bf16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)fmaxf(acc[t][i], 0.f);
        pol_tile_put4(T1 + (16 * t + 4 * h) * kPolBTS + n * 4 + oh * 2 + j, kPolBTS, o);
        save.x4(POL_SV_C2X, 16 * t + 4 * h, ow2, n * 4 + oh * 2 + j, o);
      }
    }
    __syncthreads();
    pol_linear_bf16<POL_L_C2, C, S, POL_RELU, M>(P, Wb, T1, kPolBTS, [=](int m0, int n, pol_bf16x4 y) {
      pol_tile_put4(Z + m0 * kPolBZS + n * 3 + ow2, kPolBZS, y);
      save.x4(POL_SV_FX, m0, 0, n * 3 + ow2, y);
    });
    __syncthreads();
  }

  // ---- inertial_data [15] and last_action [4], zero-padded to one k-block of 32, through 3 x (Linear(128) + ReLU) each
  for (int t = tid; t < TM * 32; t += NT) {
    const int m = t >> 5, k = t & 31, row = row0 + m;
    const __bf16 vi = (__bf16)((row < in.n && k < 15) ? in.inertial[src(row) * 15 + k] : 0.f);
    const __bf16 va = (__bf16)((row < in.n && k < 4) ? in.last_action[src(row) * 4 + k] : 0.f);
    T1[m * kPolBTS + k] = vi;
    T2[m * kPolBTS + k] = va;
    if (k < 15) save.x1(POL_SV_IN0X, m, 0, k, vi);
    if (k < 4) save.x1(POL_SV_AC0X, m, 0, k, va);
  }
  __syncthreads();
  // each chain ping-pongs between its own 128 columns of Z and its own tile (inertial: T1, last_action: T2); the two chains share
  // nothing, so layer i of both runs between one pair of barriers.  next: the layer that reads the output, from its saved buffer
  auto toZ = [=](int col0, int next) {
    const int sv = pol_layer(next, sh).x;
    return [=](int m0, int n, pol_bf16x4 y) { pol_tile_put4(Z + m0 * kPolBZS + col0 + n, kPolBZS, y); save.x4(sv, m0, 0, sv == POL_SV_FX ? col0 + n : n, y); };
  };
  auto toT = [=](__bf16* T, int next) {
    return [=](int m0, int n, pol_bf16x4 y) { pol_tile_put4(T + m0 * kPolBTS + n, kPolBTS, y); save.x4(pol_layer(next, sh).x, m0, 0, n, y); };
  };
  pol_linear_bf16<POL_L_IN0, C, S, POL_RELU, M>(P, Wb, T1, kPolBTS, toZ(192, POL_L_IN1));
  pol_linear_bf16<POL_L_AC0, C, S, POL_RELU, M>(P, Wb, T2, kPolBTS, toZ(320, POL_L_AC1));
  __syncthreads();
  pol_linear_bf16<POL_L_IN1, C, S, POL_RELU, M>(P, Wb, Z + 192, kPolBZS, toT(T1, POL_L_IN2));
  pol_linear_bf16<POL_L_AC1, C, S, POL_RELU, M>(P, Wb, Z + 320, kPolBZS, toT(T2, POL_L_AC2));
  __syncthreads();
  pol_linear_bf16<POL_L_IN2, C, S, POL_RELU, M>(P, Wb, T1, kPolBTS, toZ(192, POL_L_F));
  pol_linear_bf16<POL_L_AC2, C, S, POL_RELU, M>(P, Wb, T2, kPolBTS, toZ(320, POL_L_F));
  __syncthreads();

  // ---- trunk: concat [448] -> Linear(F) + ReLU
  pol_linear_bf16<POL_L_F, C, S, POL_RELU, M>(P, Wb, Z, kPolBZS, [=](int m0, int n, pol_bf16x4 y) {
    pol_tile_put4(F + m0 * lp.fs + n, lp.fs, y);
    save.x4(POL_SV_F, m0, 0, n, y);
  });
  __syncthreads();

  // ---- pi head, then mu; vf head, then value (one thread per row: the thread that wrote MU and VAL reads them back, no barrier)
  constexpr int KL = pol_layer(POL_L_MU, sh).K, ls = sh.n_hidden == 2 ? lp.bs : lp.as;
  const __bf16* PX = pol_head_bf16<POL_L_PI0, C, S, M>(P, Wb, F, HA, HB, save);
  static_assert(KL % 8 == 0, "the last hidden tile is read 8 elements at a time");
  if (tid < TM) {      // every sum runs over k in order; one 16-byte LDS read feeds 8 k of all four
    float s[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] = prm[P.at[POL_L_MU].b + a];
    for (int k0 = 0; k0 < KL; k0 += 8) {
      const pol_bf16x8 x = *reinterpret_cast<const pol_bf16x8*>(PX + tid * ls + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int a = 0; a < 4; ++a) s[a] = fmaf((float)x[j], prm[P.at[POL_L_MU].w + a * KL + k0 + j], s[a]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) MU[tid * 4 + a] = s[a];
  }
  __syncthreads();
  const __bf16* VX = pol_head_bf16<POL_L_VF0, C, S, M>(P, Wb, F, HA, HB, save);
  if (tid < TM) {
    float v = prm[P.at[POL_L_V].b];
    for (int k0 = 0; k0 < KL; k0 += 8) {
      const pol_bf16x8 x = *reinterpret_cast<const pol_bf16x8*>(VX + tid * ls + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v = fmaf((float)x[j], prm[P.at[POL_L_V].w + k0 + j], v);
    }
    VAL[tid] = v;
  }
}

template <int C, int S>
__global__ __launch_bounds__(pol_lds_plan_bf16(pol_shape(S, C)).threads) void policy_act_bf16_kernel(PolicyParams P, PolicyBf16 Wb, PolicyIO io) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_lds_b[];
  constexpr PolLdsB lp = pol_lds_plan_bf16(pol_shape(S, C));
  constexpr int M = lp.M;
  const PolicyIn in{io.lidar, io.inertial, io.last_action, nullptr, io.n};
  const int tid = threadIdx.x, row = blockIdx.x * M + tid;
  pol_forward_bf16<C, S>(P, Wb, in, pol_lds_b, blockIdx.x * M, PolNoSaveB{});
  // ---- policy_act_kernel's tail: the outputs of the row, read back by the thread that computed them
  const float* MU = reinterpret_cast<const float*>(pol_lds_b) + lp.mu;
  const float* VAL = reinterpret_cast<const float*>(pol_lds_b) + lp.val;
  const float* log_std = P.base + P.log_std;
  if (tid < M && row < io.n) {
    io.value[row] = VAL[tid];
    float lgp = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float mu = MU[tid * 4 + a];
      io.mu[(size_t)row * 4 + a] = mu;
      if (io.eps) {
        const float e = io.eps[(size_t)row * 4 + a], lsd = log_std[a];
        const float act = fmaf(expf(lsd), e, mu);
        lgp += -0.5f * e * e - lsd - 0.9189385332046727f;
        if (io.action) io.action[(size_t)row * 4 + a] = act;
        if (io.action_env) io.action_env[(size_t)row * 4 + a] = fmaxf(fminf(act, 1.f), a < 3 ? -1.f : 0.f);
      }
    }
    if (io.eps && io.logp) io.logp[row] = lgp;
  }
}

}  // namespace te
