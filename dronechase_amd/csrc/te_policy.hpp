// te_policy.hpp — inference of LidarInertialActionPolicy (dronechase_amd/ppo.py) in one launch: the forward pass, the
// Gaussian sample and its log-probability, and the action clamp te_step takes (te_policy_act, include/threatengage.h).
//
//   policy_act_kernel  one 256-thread workgroup (4 waves) per tile of kTileM = 32 rows.  Every layer is a GEMM on
//                      v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate): the tile's activations stay in LDS from layer to
//                      layer, the weights are read straight from the packed parameter buffer (0.94 MB: L2-resident and
//                      shared by every workgroup of the XCD).  A wave owns one 16-column slice of a layer's output at a
//                      time, for both 16-row halves of the tile: one 16-byte weight load feeds 8 MFMAs.  Barriers separate
//                      the layers.
//
// Layer by layer (C = LIDAR channels, 2 or 3):
//   conv1 (k4 s4) as a GEMM over non-overlapping 4x4 patches, [32 rows x 4 positions, 16 C] x [16 C, 32], computed
//     for one conv2 output column at a time (3 chunks): conv2 (k2 s2) reads rows 0-1 of conv1's 3 x 6 output only, so
//     conv1 needs 12 of its 18 positions and the LIDAR rows 8-12 and columns 24-25 are never read.  A lane reads a
//     patch row of 4 cells as two 8-byte loads (a LIDAR row is 104 bytes: 8-byte, not 16-byte aligned).  The output
//     lands in LDS already in conv2's patch order (ci * 4 + kh * 2 + kw).
//   conv2 as [32, 128] x [128, 64] per chunk, scattered into the flatten order (co * 3 + column) of the feature row.
//   inertial_data [15] and last_action [4], zero-padded to K = 16, through 3 x Linear(128) + ReLU each.
//   concat [448] -> Linear(256) + ReLU -> pi: 2 x Linear(64) + tanh, vf: 2 x Linear(64) + tanh.
//   mu = Linear(64, 4) and value = Linear(64, 1) on the vector ALU, one thread per row.
//
// Numerics: fp32 throughout.  A k-block of 16 is consumed as 4 MFMAs whose k index is strided by 4 (lane group h holds
// k0 + 4h .. k0 + 4h + 3 as one float4; MFMA s takes component s), so the sum order differs from PyTorch's; the
// accumulator starts from the bias.  The order is fixed per output element and does not depend on where the row sits in
// the tile, on the tile, or on N: a row's outputs are bitwise the same in any call.
#pragma once

namespace te {

constexpr int kPolTileM = 32;           // rows per workgroup (two 16-row MFMA tiles)
constexpr int kPolThreads = 256;        // 4 waves
constexpr int kPolZS = 448 + 4;         // LDS row strides in floats (+4: a 16-lane float4 column read spreads over the banks)
constexpr int kPolTS = 128 + 4;
constexpr int kPolFS = 256 + 4;
constexpr int kPolPS = 64 + 4;
constexpr int kPolZWords = kPolTileM * kPolZS;                     // concat features; later the heads' activations
constexpr int kPolUWords = 2 * kPolTileM * kPolTS;                 // two 128-wide ping-pong tiles; later the 256-wide trunk
static_assert(kPolTileM * kPolFS <= kPolUWords, "trunk tile fits the ping-pong region");
static_assert(2 * kPolTileM * kPolPS + kPolTileM * 4 <= kPolZWords, "head tiles fit the feature region");
constexpr int kPolLdsBytes = (kPolZWords + kPolUWords) * 4;

// What pol_forward hands to its `save` hook besides keeping it in LDS: every layer's input, i.e. what the weight gradient of that
// layer needs.  save(buf, m, sub, col, v): tile row m, sub-row sub (a conv position), column col.
enum {
  POL_SV_C1X = 0,   // conv1 patches: sub = conv1 position p = ow2 * 4 + oh * 2 + j (0..11), col = c * 16 + kh * 4 + kw
  POL_SV_C2X,       // conv2 patches (conv1 output after ReLU): sub = ow2 (0..2), col = ci * 4 + kh * 2 + kw
  POL_SV_IN0X, POL_SV_IN1X, POL_SV_IN2X,   // inputs of inertial.{0,2,4}: [15], [128], [128]
  POL_SV_AC0X, POL_SV_AC1X, POL_SV_AC2X,   // inputs of action.{0,2,4}: [4], [128], [128]
  POL_SV_FX,        // the concat [448] (conv2 output in flatten order co * 3 + ow2, inertial, last_action): input of final.0
  POL_SV_F,         // the trunk [256]: input of pi.0 and vf.0
  POL_SV_PI1X, POL_SV_MUX, POL_SV_VF1X, POL_SV_VX,   // [64] each: inputs of pi.2, mu, vf.2, value
  POL_SV_COUNT
};

// The 15 weight layers in the order of the packed parameter buffer, then the two bias-only pseudo-layers of the gradient's split-K
// reduction (te_policy_grad.hpp): d loss / d log_std [4] and the statistics [pg, vl, ent, clip_frac].
enum {
  POL_L_C1 = 0, POL_L_C2, POL_L_IN0, POL_L_IN1, POL_L_IN2, POL_L_AC0, POL_L_AC1, POL_L_AC2, POL_L_F,
  POL_L_PI0, POL_L_PI1, POL_L_VF0, POL_L_VF1, POL_L_MU, POL_L_V,
  POL_L_WEIGHTS, POL_L_LOGSTD = POL_L_WEIGHTS, POL_L_STATS, POL_L_COUNT
};

// The one description of the network: layer l computes N outputs from K inputs at each of its `pos` positions per sample (a conv's
// output positions; 1 for a Linear) and reads its input from saved buffer x.  The packed layout, the saved inputs' geometry, the
// gradient workspace and the split-K plan are all derived from this table.
struct PolLayer { int N, K, pos, x; };

__host__ __device__ constexpr PolLayer pol_layer(int l, int C) {
  const PolLayer t[POL_L_COUNT] = {
      {32, 16 * C, 12, POL_SV_C1X}, {64, 128, 3, POL_SV_C2X},
      {128, 15, 1, POL_SV_IN0X},    {128, 128, 1, POL_SV_IN1X}, {128, 128, 1, POL_SV_IN2X},
      {128, 4, 1, POL_SV_AC0X},     {128, 128, 1, POL_SV_AC1X}, {128, 128, 1, POL_SV_AC2X},
      {256, 448, 1, POL_SV_FX},
      {64, 256, 1, POL_SV_F},       {64, 64, 1, POL_SV_PI1X},
      {64, 256, 1, POL_SV_F},       {64, 64, 1, POL_SV_VF1X},
      {4, 64, 1, POL_SV_MUX},       {1, 64, 1, POL_SV_VX},
      {4, 0, 1, POL_SV_COUNT},      {4, 0, 1, POL_SV_COUNT}};   // log_std and the statistics: no input
  return t[l];
}
static_assert(pol_layer(POL_L_PI0, 3).K == pol_layer(POL_L_VF0, 3).K && pol_layer(POL_L_PI0, 3).pos == pol_layer(POL_L_VF0, 3).pos, "POL_SV_F feeds both");

// Float offsets of every tensor in the packed parameter buffer (the public layout of threatengage.h): per layer the weight
// [N][K], then the bias [N]; log_std last.  A kernel argument by value: index `at` with compile-time constants only, or it leaves the SGPRs.
struct PolicyParams {
  const float* base;
  struct { int w, b; } at[POL_L_WEIGHTS];
  int log_std, words;
};

inline PolicyParams policy_layout(int C) {
  PolicyParams p{};
  int o = 0;
  for (int l = 0; l < POL_L_WEIGHTS; ++l) {
    const PolLayer y = pol_layer(l, C);
    p.at[l].w = o; o += y.N * y.K;
    p.at[l].b = o; o += y.N;
  }
  p.log_std = o;
  p.words = o + pol_layer(POL_L_LOGSTD, C).N;
  return p;
}

struct PolicyIO {
  const float *lidar, *inertial, *last_action, *eps;
  float *mu, *value, *action, *logp, *action_env;
  int n;
};

// The rows a forward reads: row i of the tile set is read at index[i] (NULL: at i) of lidar / inertial / last_action.
struct PolicyIn {
  const float *lidar, *inertial, *last_action;
  const int64_t* index;
  int n;
};

typedef float pol_f32x4 __attribute__((ext_vector_type(4)));

enum { POL_RELU = 0, POL_TANH = 1 };

TE_DEV pol_f32x4 pol_mfma4(float4 a, float4 b, pol_f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// Y[32, N] = X[32, K] B + init, the GEMM every layer of the policy runs (forward and backward).  X in LDS (row stride ldx,
// columns K .. roundup(K, 16) zero); loadb(n, k) returns B[k .. k + 3][n] (k a multiple of 4, zero past K); init(n) starts the
// accumulator of column n; epi(row, col, value) consumes one output element.  Lane l of a 16 x 16 tile:
// A = X[l & 15][k0 + 4 (l >> 4) + s], B = B[k0 + 4 (l >> 4) + s][n0 + (l & 15)]; C/D: column l & 15, rows 4 (l >> 4) .. +3.
template <int K, int N, class LoadB, class Init, class Epi>
TE_DEV void pol_gemm(const float* X, int ldx, LoadB loadb, Init init, Epi epi) {
  static_assert(N % 16 == 0 && N / 16 >= kPolThreads / 64, "every wave owns at least one 16-column slice");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
  for (int nt = wave; nt < N / 16; nt += kPolThreads / 64) {
    const int n = nt * 16 + r;
    const float b0 = init(n);
    pol_f32x4 acc0 = {b0, b0, b0, b0}, acc1 = acc0;
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int k = k0 + 4 * h;
      const float4 w = loadb(n, k);
      const float4 a0 = *reinterpret_cast<const float4*>(X + r * ldx + k);
      const float4 a1 = *reinterpret_cast<const float4*>(X + (16 + r) * ldx + k);
      acc0 = pol_mfma4(a0, w, acc0);
      acc1 = pol_mfma4(a1, w, acc1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      epi(4 * h + i, n, acc0[i]);
      epi(16 + 4 * h + i, n, acc1[i]);
    }
  }
}

// Y[32, N] = act(X[32, K] W^T + b), W [N][K] row-major in global memory (the forward of a Linear layer): pol_gemm with
// B[k][n] = W[n][k], the accumulator starting from the bias.  store(row, col, value) writes one output element.
template <int K, int N, int ACT, class Store>
TE_DEV void pol_dense(const float* X, int ldx, const float* __restrict__ W, const float* __restrict__ bias, Store store) {
  pol_gemm<K, N>(
      X, ldx,
      [=](int n, int k) {
        const float* wr = W + (size_t)n * K;
        float4 w;
        if constexpr (K % 4 == 0) {
          w = k < K ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {  // K = 15: rows are not 16-byte aligned
          w.x = k + 0 < K ? wr[k + 0] : 0.f; w.y = k + 1 < K ? wr[k + 1] : 0.f;
          w.z = k + 2 < K ? wr[k + 2] : 0.f; w.w = k + 3 < K ? wr[k + 3] : 0.f;
        }
        return w;
      },
      [=](int n) { return bias[n]; },
      [=](int m, int n, float v) { store(m, n, ACT == POL_RELU ? fmaxf(v, 0.f) : tanhf(v)); });
}

// The forward of weight layer L on its packed weight and bias.
template <int L, int C, int ACT, class Store>
TE_DEV void pol_linear(const PolicyParams& P, const float* X, int ldx, Store store) {
  constexpr PolLayer y = pol_layer(L, C);
  pol_dense<y.K, y.N, ACT>(X, ldx, P.base + P.at[L].w, P.base + P.at[L].b, store);
}

struct PolNoSave {
  TE_DEV void operator()(int, int, int, int, float) const {}
};

// LDS of pol_forward once it returns: MU [32][4] and VAL [32] (rows of the tile), written by thread tid = row for tid < 32.
TE_DEV float* pol_mu_lds(float* lds) { return lds + 2 * kPolTileM * kPolPS; }
TE_DEV float* pol_val_lds(float* lds) { return lds + 2 * kPolTileM * kPolPS + kPolTileM * 4; }
static_assert(2 * kPolTileM * kPolPS + kPolTileM * 5 <= kPolZWords, "MU and VAL fit the feature region");

// The forward of the 32 rows from row0 (rows >= in.n read zeros): mu and value of every row into pol_mu_lds / pol_val_lds; each
// layer's input also goes to save().  Thread tid < 32 computes row tid's mu and value and may read them back without a barrier.
template <int C, class Save>
TE_DEV void pol_forward(const PolicyParams& P, const PolicyIn& in, float* pol_lds, int row0, Save save) {
  float* Z = pol_lds;                          // [32][kPolZS]: lidar 0..191 | inertial 192..319 | last_action 320..447
  float* T1 = pol_lds + kPolZWords;            // [32][kPolTS]
  float* T2 = T1 + kPolTileM * kPolTS;         // [32][kPolTS]
  float* F = T1;                               // [32][kPolFS] once T1 / T2 are dead
  float* P1 = Z;                               // [32][kPolPS] once Z is dead
  float* P2 = Z + kPolTileM * kPolPS;
  float* MU = pol_mu_lds(pol_lds);             // [32][4]
  float* VAL = pol_val_lds(pol_lds);           // [32]
  const float* __restrict__ prm = P.base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  auto src = [&](int row) -> size_t { return in.index ? (size_t)in.index[row] : (size_t)row; };
  // next: the layer that reads this output, from its saved buffer
  auto to = [=](float* Y, int ld, int next) { return [=](int m, int n, float v) { Y[m * ld + n] = v; save(pol_layer(next, C).x, m, 0, n, v); }; };

  // ---- LIDAR: conv1 + conv2, one conv2 output column (ow2) at a time
  {
    // wave w computes conv1 position (oh, j) = (w >> 1, w & 1) of the chunk for both row halves and all 32 channels
    const int oh = wave >> 1, j = wave & 1;
    for (int ow2 = 0; ow2 < 3; ++ow2) {
      const int ow = 2 * ow2 + j;
      pol_f32x4 acc[2][2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const float b = prm[P.at[POL_L_C1].b + nt * 16 + r];
        acc[0][nt] = pol_f32x4{b, b, b, b}; acc[1][nt] = acc[0][nt];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {      // k-block c: k = c * 16 + kh * 4 + kw, lane group h = kh
        float4 a[2], w[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int row = row0 + half * 16 + r;
          a[half] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (row < in.n) {
            const float* s = in.lidar + (src(row) * C + c) * (13 * 26) + (4 * oh + h) * 26 + 4 * ow;
            const float2 lo = *reinterpret_cast<const float2*>(s), hi = *reinterpret_cast<const float2*>(s + 2);
            a[half] = make_float4(lo.x, lo.y, hi.x, hi.y);
          }
          const int m = half * 16 + r, p = ow2 * 4 + oh * 2 + j, col = c * 16 + 4 * h;
          save(POL_SV_C1X, m, p, col + 0, a[half].x); save(POL_SV_C1X, m, p, col + 1, a[half].y);
          save(POL_SV_C1X, m, p, col + 2, a[half].z); save(POL_SV_C1X, m, p, col + 3, a[half].w);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) w[nt] = *reinterpret_cast<const float4*>(prm + P.at[POL_L_C1].w + (nt * 16 + r) * (16 * C) + c * 16 + 4 * h);
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[half][nt] = pol_mfma4(a[half], w[nt], acc[half][nt]);
      }
      // conv1 output (row, co, oh, ow) -> conv2 patch of column ow2: T1[row][co * 4 + oh * 2 + j]
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = half * 16 + 4 * h + i, col = (nt * 16 + r) * 4 + oh * 2 + j;
            const float v = fmaxf(acc[half][nt][i], 0.f);
            T1[m * kPolTS + col] = v;
            save(POL_SV_C2X, m, ow2, col, v);
          }
      __syncthreads();
      pol_linear<POL_L_C2, C, POL_RELU>(P, T1, kPolTS,
                                        [=](int m, int n, float v) { Z[m * kPolZS + n * 3 + ow2] = v; save(POL_SV_FX, m, 0, n * 3 + ow2, v); });
      __syncthreads();
    }
  }

  // ---- inertial_data and last_action: 3 x (Linear(128) + ReLU) each, into Z columns 192 and 320
  for (int t = tid; t < kPolTileM * 16; t += kPolThreads) {
    const int m = t >> 4, k = t & 15, row = row0 + m;
    const float vi = (row < in.n && k < 15) ? in.inertial[src(row) * 15 + k] : 0.f;
    const float va = (row < in.n && k < 4) ? in.last_action[src(row) * 4 + k] : 0.f;
    T1[m * kPolTS + k] = vi;
    T2[m * kPolTS + k] = va;
    if (k < 15) save(POL_SV_IN0X, m, 0, k, vi);
    if (k < 4) save(POL_SV_AC0X, m, 0, k, va);
  }
  __syncthreads();
  // each chain ping-pongs between its own 128 columns of Z and T1 (T2 holds last_action's input until its first layer)
  auto toZ = [=](int col0, int next) {
    const int sv = pol_layer(next, C).x;
    return [=](int m, int n, float v) { Z[m * kPolZS + col0 + n] = v; save(sv, m, 0, sv == POL_SV_FX ? col0 + n : n, v); };
  };
  pol_linear<POL_L_IN0, C, POL_RELU>(P, T1, kPolTS, toZ(192, POL_L_IN1));
  __syncthreads();
  pol_linear<POL_L_IN1, C, POL_RELU>(P, Z + 192, kPolZS, to(T1, kPolTS, POL_L_IN2));
  __syncthreads();
  pol_linear<POL_L_IN2, C, POL_RELU>(P, T1, kPolTS, toZ(192, POL_L_F));
  __syncthreads();
  pol_linear<POL_L_AC0, C, POL_RELU>(P, T2, kPolTS, toZ(320, POL_L_AC1));
  __syncthreads();
  pol_linear<POL_L_AC1, C, POL_RELU>(P, Z + 320, kPolZS, to(T1, kPolTS, POL_L_AC2));
  __syncthreads();
  pol_linear<POL_L_AC2, C, POL_RELU>(P, T1, kPolTS, toZ(320, POL_L_F));
  __syncthreads();

  // ---- trunk: concat [448] -> Linear(256) + ReLU
  pol_linear<POL_L_F, C, POL_RELU>(P, Z, kPolZS, to(F, kPolFS, POL_L_PI0));
  __syncthreads();

  // ---- pi head, then mu (one thread per row)
  pol_linear<POL_L_PI0, C, POL_TANH>(P, F, kPolFS, to(P1, kPolPS, POL_L_PI1));
  __syncthreads();
  pol_linear<POL_L_PI1, C, POL_TANH>(P, P1, kPolPS, to(P2, kPolPS, POL_L_MU));
  __syncthreads();
  if (tid < kPolTileM) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float s = prm[P.at[POL_L_MU].b + a];
      for (int k = 0; k < 64; ++k) s = fmaf(P2[tid * kPolPS + k], prm[P.at[POL_L_MU].w + a * 64 + k], s);
      MU[tid * 4 + a] = s;
    }
  }
  __syncthreads();
  // ---- vf head, then value (the thread that computed mu computes the value: no barrier needed)
  pol_linear<POL_L_VF0, C, POL_TANH>(P, F, kPolFS, to(P1, kPolPS, POL_L_VF1));
  __syncthreads();
  pol_linear<POL_L_VF1, C, POL_TANH>(P, P1, kPolPS, to(P2, kPolPS, POL_L_V));
  __syncthreads();
  if (tid < kPolTileM) {
    float v = prm[P.at[POL_L_V].b];
    for (int k = 0; k < 64; ++k) v = fmaf(P2[tid * kPolPS + k], prm[P.at[POL_L_V].w + k], v);
    VAL[tid] = v;
  }
}

template <int C>
__global__ __launch_bounds__(kPolThreads) void policy_act_kernel(PolicyParams P, PolicyIO io) {
  extern __shared__ __attribute__((aligned(16))) float pol_lds[];
  const PolicyIn in{io.lidar, io.inertial, io.last_action, nullptr, io.n};
  const int tid = threadIdx.x, row = blockIdx.x * kPolTileM + tid;
  pol_forward<C>(P, in, pol_lds, blockIdx.x * kPolTileM, PolNoSave{});
  // the outputs of the row, read back by the thread that computed them
  const float* MU = pol_mu_lds(pol_lds);
  const float* log_std = P.base + P.log_std;
  if (tid < kPolTileM && row < io.n) {
    io.value[row] = pol_val_lds(pol_lds)[tid];
    float lp = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float mu = MU[tid * 4 + a];
      io.mu[(size_t)row * 4 + a] = mu;
      if (io.eps) {
        const float e = io.eps[(size_t)row * 4 + a], ls = log_std[a];
        const float act = fmaf(expf(ls), e, mu);
        lp += -0.5f * e * e - ls - 0.9189385332046727f;
        if (io.action) io.action[(size_t)row * 4 + a] = act;
        if (io.action_env) io.action_env[(size_t)row * 4 + a] = fmaxf(fminf(act, 1.f), a < 3 ? -1.f : 0.f);
      }
    }
    if (io.eps && io.logp) io.logp[row] = lp;
  }
}

}  // namespace te
