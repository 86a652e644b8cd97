// te_policy.hpp — inference of LidarInertialActionPolicy (dronechase_amd/ppo.py) in one launch: the forward pass, the
// Gaussian sample and its log-probability, and the action clamp te_step takes (te_policy_act, include/threatengage.h).
//
//   policy_act_kernel  one 256-thread workgroup (4 waves) per tile of 32 rows (16 for the wide shapes, below).  Every layer is a
//                      GEMM on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate): the tile's activations stay in LDS from layer to
//                      layer, the weights are read straight from the packed parameter buffer (default shape, 0.94 MB: L2-resident
//                      and shared by every workgroup of the XCD; the wide shapes' 3.1 and 4.1 MB are most or more than all of an
//                      XCD's 4 MiB L2, and each workgroup reads all of them for 16 rows: expected to be bound by that traffic).  A wave owns one 16-column slice of a layer's output at a
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
//   concat [448] -> Linear(F) + ReLU -> pi: 1-3 x Linear(h[i]) + tanh, vf: the same widths.
//   mu = Linear(h[last], 4) and value = Linear(h[last], 1) on the vector ALU, one thread per row.
//
// The network's shape (F and the head widths) is one of the closed list pol_shape() serves, a template parameter next to C: every
// K and N of pol_gemm stays a compile-time constant.  The default shape (F = 256, heads 64, 64: 0.94 MB of weights) runs 32 rows
// per workgroup; the reference's trained shapes (F = 512, heads up to 512 wide: 3.1 and 4.1 MB) run 16, because their trunk tile
// and head tiles do not fit a CU's LDS at 32 rows (pol_lds_plan).  The sum order of an output is over k only, whatever the tile's
// height: a row's outputs do not depend on the tile height or on the row's place in the tile.
//
// Numerics: fp32 throughout.  A k-block of 16 is consumed as 4 MFMAs whose k index is strided by 4 (lane group h holds
// k0 + 4h .. k0 + 4h + 3 as one float4; MFMA s takes component s), so the sum order differs from PyTorch's; the
// accumulator starts from the bias.  The order is fixed per output element and does not depend on where the row sits in
// the tile, on the tile, or on N: a row's outputs are bitwise the same in any call.
#pragma once

namespace te {

constexpr int kPolTileM = 32;           // rows per workgroup of the default shape (two 16-row MFMA tiles)
constexpr int kPolThreads = 256;        // 4 waves
constexpr int kPolZS = 448 + 4;         // LDS row strides in floats (+4: a 16-lane float4 column read spreads over the banks)
constexpr int kPolTS = 128 + 4;
constexpr int kPolFS = 256 + 4;
constexpr int kPolPS = 64 + 4;
constexpr int kPolZWords = kPolTileM * kPolZS;                     // concat features; later the heads' activations
constexpr int kPolUWords = 2 * kPolTileM * kPolTS;                 // two 128-wide ping-pong tiles; later the 256-wide trunk
static_assert(kPolTileM * kPolFS <= kPolUWords, "trunk tile fits the ping-pong region");
static_assert(2 * kPolTileM * kPolPS + kPolTileM * 4 <= kPolZWords, "head tiles fit the feature region");
constexpr int kPolLdsBytes = (kPolZWords + kPolUWords) * 4;        // the default shape's
constexpr int kPolLdsLimit = 160 * 1024;                           // LDS of a gfx950 CU

// What pol_forward hands to its `save` hook besides keeping it in LDS: every layer's input, i.e. what the weight gradient of that
// layer needs.  save(buf, m, sub, col, v): tile row m, sub-row sub (a conv position), column col.
enum {
  POL_SV_C1X = 0,   // conv1 patches: sub = conv1 position p = ow2 * 4 + oh * 2 + j (0..11), col = c * 16 + kh * 4 + kw
  POL_SV_C2X,       // conv2 patches (conv1 output after ReLU): sub = ow2 (0..2), col = ci * 4 + kh * 2 + kw
  POL_SV_IN0X, POL_SV_IN1X, POL_SV_IN2X,   // inputs of inertial.{0,2,4}: [15], [128], [128]
  POL_SV_AC0X, POL_SV_AC1X, POL_SV_AC2X,   // inputs of action.{0,2,4}: [4], [128], [128]
  POL_SV_FX,        // the concat [448] (conv2 output in flatten order co * 3 + ow2, inertial, last_action): input of final.0
  POL_SV_F,         // the trunk [F]: input of pi.0 and vf.0
  POL_SV_PI1X, POL_SV_PI2X, POL_SV_MUX, POL_SV_VF1X, POL_SV_VF2X, POL_SV_VX,   // inputs of pi.2, pi.4, mu, vf.2, vf.4, value
  POL_SV_COUNT
};

// The weight layers in the order of the packed parameter buffer (a head has up to three; one a shape lacks has N = K = 0 and takes
// no words), then the two bias-only pseudo-layers of the gradient's split-K
// reduction (te_policy_grad.hpp): d loss / d log_std [4] and the statistics [pg, vl, ent, clip_frac].
enum {
  POL_L_C1 = 0, POL_L_C2, POL_L_IN0, POL_L_IN1, POL_L_IN2, POL_L_AC0, POL_L_AC1, POL_L_AC2, POL_L_F,
  POL_L_PI0, POL_L_PI1, POL_L_PI2, POL_L_VF0, POL_L_VF1, POL_L_VF2, POL_L_MU, POL_L_V,
  POL_L_WEIGHTS, POL_L_LOGSTD = POL_L_WEIGHTS, POL_L_STATS, POL_L_COUNT
};

// The one description of the network: layer l computes N outputs from K inputs at each of its `pos` positions per sample (a conv's
// output positions; 1 for a Linear) and reads its input from saved buffer x.  The packed layout, the saved inputs' geometry, the
// gradient workspace and the split-K plan are all derived from this table.
struct PolLayer { int N, K, pos, x; };

// A network shape: LIDAR channels, the trunk's width, and the widths of the pi and vf heads' hidden layers (the same for both).
struct PolShape { int C, F, n_hidden, h[3]; };

// The served shapes.  DEFAULT: SB3's defaults.  BO, LEARN: the networks the reference trains (its stage03 experiment apps continue
// from h[128, 256, 512] checkpoints; stage03/auxiliary/learn.py trains net_arch [512, 128, 256]), both with features_dim 512.
enum { POL_SHAPE_DEFAULT = 0, POL_SHAPE_BO, POL_SHAPE_LEARN, POL_SHAPE_COUNT };

__host__ __device__ constexpr PolShape pol_shape(int id, int C) {
  const PolShape t[POL_SHAPE_COUNT] = {{C, 256, 2, {64, 64, 0}}, {C, 512, 3, {128, 256, 512}}, {C, 512, 3, {512, 128, 256}}};
  return t[id];
}

__host__ __device__ constexpr PolLayer pol_layer(int l, PolShape s) {
  const int C = s.C, F = s.F, nh = s.n_hidden, h0 = s.h[0], h1 = nh > 1 ? s.h[1] : 0, h2 = nh > 2 ? s.h[2] : 0, last = s.h[nh - 1];
  const PolLayer t[POL_L_COUNT] = {
      {32, 16 * C, 12, POL_SV_C1X}, {64, 128, 3, POL_SV_C2X},
      {128, 15, 1, POL_SV_IN0X},    {128, 128, 1, POL_SV_IN1X}, {128, 128, 1, POL_SV_IN2X},
      {128, 4, 1, POL_SV_AC0X},     {128, 128, 1, POL_SV_AC1X}, {128, 128, 1, POL_SV_AC2X},
      {F, 448, 1, POL_SV_FX},
      {h0, F, 1, POL_SV_F},         {h1, h1 ? h0 : 0, 1, POL_SV_PI1X}, {h2, h2 ? h1 : 0, 1, POL_SV_PI2X},
      {h0, F, 1, POL_SV_F},         {h1, h1 ? h0 : 0, 1, POL_SV_VF1X}, {h2, h2 ? h1 : 0, 1, POL_SV_VF2X},
      {4, last, 1, POL_SV_MUX},     {1, last, 1, POL_SV_VX},
      {4, 0, 1, POL_SV_COUNT},      {4, 0, 1, POL_SV_COUNT}};   // log_std and the statistics: no input
  return t[l];
}
static_assert(pol_layer(POL_L_PI0, pol_shape(0, 3)).K == pol_layer(POL_L_VF0, pol_shape(0, 3)).K, "POL_SV_F feeds both");

// Float offsets of every tensor in the packed parameter buffer (the public layout of threatengage.h): per layer the weight
// [N][K], then the bias [N]; log_std last.  A kernel argument by value: index `at` with compile-time constants only, or it leaves the SGPRs.
struct PolicyParams {
  const float* base;
  struct { int w, b; } at[POL_L_WEIGHTS];
  int log_std, words;
};

inline PolicyParams policy_layout(PolShape S) {
  PolicyParams p{};
  int o = 0;
  for (int l = 0; l < POL_L_WEIGHTS; ++l) {
    const PolLayer y = pol_layer(l, S);
    p.at[l].w = o; o += y.N * y.K;
    p.at[l].b = o; o += y.N;
  }
  p.log_std = o;
  p.words = o + pol_layer(POL_L_LOGSTD, S).N;
  return p;
}

// The LDS of pol_forward for a shape, in floats from the start of the dynamic LDS.  M rows per workgroup.  The extractor's map is
// the same for every shape: Z [M][kPolZS] at 0, the ping-pong tiles T1, T2 [M][kPolTS] behind it.  Then the trunk F [M][fs], the
// heads' ping-pong tiles A [M][as] (hidden layers 0 and 2) and B [M][bs] (hidden layer 1), MU [M][4] and VAL [M].
//   default: F over T1 / T2, A, B, MU and VAL over Z (both dead by then): the map the kernel has always had, 91.6 KB.
//   F = 512: Z + F alone are 62 KB at 16 rows and F stays live through both heads; at 32 rows F, a 256-wide and a 512-wide head
//            tile would need 161.5 KB.  So 16 rows: F over T1 / T2 and beyond, B over Z, A, MU and VAL behind F: 95.3 KB.
struct PolLds { int M, f, fs, a, as, b, bs, mu, val, words; };

__host__ __device__ constexpr PolLds pol_lds_plan(PolShape S) {
  const int h1 = S.n_hidden > 1 ? S.h[1] : 0, h2 = S.n_hidden > 2 ? S.h[2] : 0;
  const int fs = S.F + 4, as = (S.h[0] > h2 ? S.h[0] : h2) + 4, bs = h1 + 4;
  if (S.F == 256 && as == kPolPS && bs == kPolPS)
    return {kPolTileM, kPolZWords, fs, 0, as, kPolTileM * kPolPS, bs, 2 * kPolTileM * kPolPS, 2 * kPolTileM * kPolPS + kPolTileM * 4,
            kPolZWords + kPolUWords};
  const int M = 16, z = M * kPolZS, a = z + M * fs, mu = a + M * as;
  return {M, z, fs, a, as, 0, bs, mu, mu + M * 4, mu + M * 5};
}

// A plan is sound when every tile lies where nothing live is: F clear of Z, B within the dead Z, A behind F, all within the CU.
__host__ __device__ constexpr bool pol_lds_ok(PolShape S) {
  const PolLds p = pol_lds_plan(S);
  const bool dflt = p.M == kPolTileM;
  return p.words * 4 <= kPolLdsLimit && p.words >= p.M * kPolZS + 2 * p.M * kPolTS && p.f >= p.M * kPolZS && p.f + p.M * p.fs <= p.words &&
         (dflt ? p.b + p.M * p.bs <= p.mu && p.val + p.M <= p.f
               : p.b + p.M * p.bs <= p.f && p.a >= p.f + p.M * p.fs && p.a + p.M * p.as <= p.mu && p.val + p.M <= p.words);
}
static_assert(pol_lds_ok(pol_shape(POL_SHAPE_DEFAULT, 3)) && pol_lds_plan(pol_shape(POL_SHAPE_DEFAULT, 3)).words * 4 == kPolLdsBytes,
              "the default shape keeps its LDS map");
static_assert(pol_lds_ok(pol_shape(POL_SHAPE_BO, 3)) && pol_lds_plan(pol_shape(POL_SHAPE_BO, 3)).words * 4 <= kPolLdsLimit, "h[128, 256, 512] fits a CU");
static_assert(pol_lds_ok(pol_shape(POL_SHAPE_LEARN, 3)) && pol_lds_plan(pol_shape(POL_SHAPE_LEARN, 3)).words * 4 <= kPolLdsLimit, "h[512, 128, 256] fits a CU");

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

// Y[16 MT, N] = X[16 MT, K] B + init, the GEMM every layer of the policy runs (forward and backward; MT = 2 unless the shape's
// tile is 16 rows).  X in LDS (row stride ldx,
// columns K .. roundup(K, 16) zero); loadb(n, k) returns B[k .. k + 3][n] (k a multiple of 4, zero past K); init(n) starts the
// accumulator of column n; epi(row, col, value) consumes one output element.  Lane l of a 16 x 16 tile:
// A = X[l & 15][k0 + 4 (l >> 4) + s], B = B[k0 + 4 (l >> 4) + s][n0 + (l & 15)]; C/D: column l & 15, rows 4 (l >> 4) .. +3.
template <int K, int N, int MT = 2, class LoadB, class Init, class Epi>
TE_DEV void pol_gemm(const float* X, int ldx, LoadB loadb, Init init, Epi epi) {
  static_assert(N % 16 == 0 && N / 16 >= kPolThreads / 64, "every wave owns at least one 16-column slice");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
  for (int nt = wave; nt < N / 16; nt += kPolThreads / 64) {
    const int n = nt * 16 + r;
    const float b0 = init(n);
    pol_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = pol_f32x4{b0, b0, b0, b0};
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int k = k0 + 4 * h;
      const float4 w = loadb(n, k);
      float4 a[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const float4*>(X + (16 * t + r) * ldx + k);
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = pol_mfma4(a[t], w, acc[t]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < MT; ++t) epi(16 * t + 4 * h + i, n, acc[t][i]);
  }
}

// Y[16 MT, N] = act(X[16 MT, K] W^T + b), W [N][K] row-major in global memory (the forward of a Linear layer): pol_gemm with
// B[k][n] = W[n][k], the accumulator starting from the bias.  store(row, col, value) writes one output element.
template <int K, int N, int ACT, int MT, class Store>
TE_DEV void pol_dense(const float* X, int ldx, const float* __restrict__ W, const float* __restrict__ bias, Store store) {
  pol_gemm<K, N, MT>(
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

// The forward of weight layer L of shape S on its packed weight and bias.
template <int L, int C, int S, int ACT, class Store>
TE_DEV void pol_linear(const PolicyParams& P, const float* X, int ldx, Store store) {
  constexpr PolLayer y = pol_layer(L, pol_shape(S, C));
  pol_dense<y.K, y.N, ACT, pol_lds_plan(pol_shape(S, C)).M / 16>(X, ldx, P.base + P.at[L].w, P.base + P.at[L].b, store);
}

struct PolNoSave {
  TE_DEV void operator()(int, int, int, int, float) const {}
};

// LDS of pol_forward once it returns: MU [M][4] and VAL [M] (rows of the tile), written by thread tid = row for tid < M.
template <int S = POL_SHAPE_DEFAULT>
TE_DEV float* pol_mu_lds(float* lds) { return lds + pol_lds_plan(pol_shape(S, 3)).mu; }
template <int S = POL_SHAPE_DEFAULT>
TE_DEV float* pol_val_lds(float* lds) { return lds + pol_lds_plan(pol_shape(S, 3)).val; }
static_assert(2 * kPolTileM * kPolPS + kPolTileM * 5 <= kPolZWords, "MU and VAL fit the feature region");

// One head of shape S: hidden layers L0, L0 + 1, L0 + 2 (those the shape has) with tanh, F -> A -> B -> A; returns the last one's output.
template <int L0, int C, int S, class To>
TE_DEV const float* pol_head(const PolicyParams& P, const float* F, float* A, float* B, To to) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolLds lp = pol_lds_plan(sh);
  constexpr int last = L0 == POL_L_PI0 ? POL_L_MU : POL_L_V;
  pol_linear<L0, C, S, POL_TANH>(P, F, lp.fs, to(A, lp.as, sh.n_hidden > 1 ? L0 + 1 : last));
  __syncthreads();
  if constexpr (sh.n_hidden > 1) {
    pol_linear<L0 + 1, C, S, POL_TANH>(P, A, lp.as, to(B, lp.bs, sh.n_hidden > 2 ? L0 + 2 : last));
    __syncthreads();
  }
  if constexpr (sh.n_hidden > 2) {
    pol_linear<L0 + 2, C, S, POL_TANH>(P, B, lp.bs, to(A, lp.as, last));
    __syncthreads();
  }
  return sh.n_hidden == 2 ? B : A;
}

// The forward of the tile's M rows from row0 (rows >= in.n read zeros): mu and value of every row into pol_mu_lds / pol_val_lds;
// each layer's input also goes to save().  Thread tid < M computes row tid's mu and value and may read them back without a barrier.
template <int C, int S = POL_SHAPE_DEFAULT, class Save>
TE_DEV void pol_forward(const PolicyParams& P, const PolicyIn& in, float* pol_lds, int row0, Save save) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolLds lp = pol_lds_plan(sh);
  constexpr int M = lp.M, MT = M / 16;
  float* Z = pol_lds;                          // [M][kPolZS]: lidar 0..191 | inertial 192..319 | last_action 320..447
  float* T1 = pol_lds + M * kPolZS;            // [M][kPolTS]
  float* T2 = T1 + M * kPolTS;                 // [M][kPolTS]
  float* F = pol_lds + lp.f;                   // [M][lp.fs] once T1 / T2 are dead
  float* HA = pol_lds + lp.a;                  // [M][lp.as], [M][lp.bs]: over Z once it is dead (the wide shapes' HA: behind F)
  float* HB = pol_lds + lp.b;
  float* MU = pol_lds + lp.mu;                 // [M][4]
  float* VAL = pol_lds + lp.val;               // [M]
  const float* __restrict__ prm = P.base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  auto src = [&](int row) -> size_t { return in.index ? (size_t)in.index[row] : (size_t)row; };
  // next: the layer that reads this output, from its saved buffer
  auto to = [=](float* Y, int ld, int next) { return [=](int m, int n, float v) { Y[m * ld + n] = v; save(pol_layer(next, sh).x, m, 0, n, v); }; };

  // ---- LIDAR: conv1 + conv2, one conv2 output column (ow2) at a time
  {
    // wave w computes conv1 position (oh, j) = (w >> 1, w & 1) of the chunk for every 16-row half and all 32 channels
    const int oh = wave >> 1, j = wave & 1;
    for (int ow2 = 0; ow2 < 3; ++ow2) {
      const int ow = 2 * ow2 + j;
      pol_f32x4 acc[MT][2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const float b = prm[P.at[POL_L_C1].b + nt * 16 + r];
#pragma unroll
        for (int half = 0; half < MT; ++half) acc[half][nt] = pol_f32x4{b, b, b, b};
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {      // k-block c: k = c * 16 + kh * 4 + kw, lane group h = kh
        float4 a[MT], w[2];
#pragma unroll
        for (int half = 0; half < MT; ++half) {
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
        for (int half = 0; half < MT; ++half)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[half][nt] = pol_mfma4(a[half], w[nt], acc[half][nt]);
      }
      // conv1 output (row, co, oh, ow) -> conv2 patch of column ow2: T1[row][co * 4 + oh * 2 + j]
#pragma unroll
      for (int half = 0; half < MT; ++half)
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
      pol_linear<POL_L_C2, C, S, POL_RELU>(P, T1, kPolTS,
                                        [=](int m, int n, float v) { Z[m * kPolZS + n * 3 + ow2] = v; save(POL_SV_FX, m, 0, n * 3 + ow2, v); });
      __syncthreads();
    }
  }

  // ---- inertial_data and last_action: 3 x (Linear(128) + ReLU) each, into Z columns 192 and 320
  for (int t = tid; t < M * 16; t += kPolThreads) {
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
    const int sv = pol_layer(next, sh).x;
    return [=](int m, int n, float v) { Z[m * kPolZS + col0 + n] = v; save(sv, m, 0, sv == POL_SV_FX ? col0 + n : n, v); };
  };
  pol_linear<POL_L_IN0, C, S, POL_RELU>(P, T1, kPolTS, toZ(192, POL_L_IN1));
  __syncthreads();
  pol_linear<POL_L_IN1, C, S, POL_RELU>(P, Z + 192, kPolZS, to(T1, kPolTS, POL_L_IN2));
  __syncthreads();
  pol_linear<POL_L_IN2, C, S, POL_RELU>(P, T1, kPolTS, toZ(192, POL_L_F));
  __syncthreads();
  pol_linear<POL_L_AC0, C, S, POL_RELU>(P, T2, kPolTS, toZ(320, POL_L_AC1));
  __syncthreads();
  pol_linear<POL_L_AC1, C, S, POL_RELU>(P, Z + 320, kPolZS, to(T1, kPolTS, POL_L_AC2));
  __syncthreads();
  pol_linear<POL_L_AC2, C, S, POL_RELU>(P, T1, kPolTS, toZ(320, POL_L_F));
  __syncthreads();

  // ---- trunk: concat [448] -> Linear(F) + ReLU
  pol_linear<POL_L_F, C, S, POL_RELU>(P, Z, kPolZS, to(F, lp.fs, POL_L_PI0));
  __syncthreads();

  // ---- pi head, then mu (one thread per row)
  constexpr int KL = pol_layer(POL_L_MU, sh).K, ls = sh.n_hidden == 2 ? lp.bs : lp.as;
  const float* PX = pol_head<POL_L_PI0, C, S>(P, F, HA, HB, to);
  if (tid < M) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float s = prm[P.at[POL_L_MU].b + a];
      for (int k = 0; k < KL; ++k) s = fmaf(PX[tid * ls + k], prm[P.at[POL_L_MU].w + a * KL + k], s);
      MU[tid * 4 + a] = s;
    }
  }
  __syncthreads();
  // ---- vf head, then value (the thread that computed mu computes the value: no barrier needed)
  const float* VX = pol_head<POL_L_VF0, C, S>(P, F, HA, HB, to);
  if (tid < M) {
    float v = prm[P.at[POL_L_V].b];
    for (int k = 0; k < KL; ++k) v = fmaf(VX[tid * ls + k], prm[P.at[POL_L_V].w + k], v);
    VAL[tid] = v;
  }
}

template <int C, int S = POL_SHAPE_DEFAULT>
__global__ __launch_bounds__(kPolThreads) void policy_act_kernel(PolicyParams P, PolicyIO io) {
  extern __shared__ __attribute__((aligned(16))) float pol_lds[];
  constexpr int M = pol_lds_plan(pol_shape(S, C)).M;
  const PolicyIn in{io.lidar, io.inertial, io.last_action, nullptr, io.n};
  const int tid = threadIdx.x, row = blockIdx.x * M + tid;
  pol_forward<C, S>(P, in, pol_lds, blockIdx.x * M, PolNoSave{});
  // the outputs of the row, read back by the thread that computed them
  const float* MU = pol_mu_lds<S>(pol_lds);
  const float* log_std = P.base + P.log_std;
  if (tid < M && row < io.n) {
    io.value[row] = pol_val_lds<S>(pol_lds)[tid];
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
