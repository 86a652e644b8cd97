// te_policy_grad.hpp — the gradient of PPO's loss for LidarInertialActionPolicy (dronechase_amd/ppo.py PPO.update) with respect to
// every parameter, in te_policy_act's packed layout (te_policy_ppo_grad, include/threatengage.h).  Three launches:
//
//   policy_grad_tile_kernel  one 256-thread workgroup per tile of M rows (the shape's tile of pol_lds_plan: 32 for the default, 16 for
//                            the wide shapes), the layer code of te_policy.hpp, for every served shape: the forward
//                            (pol_forward, every layer's input also stored to the workspace), the loss of each row, then the
//                            backward to every layer's pre-activation gradient dZ.  Each backward step is pol_gemm with
//                            B[k][n] = W[k][n] (dX = dZ W) on v_mfma_f32_16x16x4_f32; the activation derivative reads the
//                            layer's output back from the workspace (the tile's own rows, written earlier in the launch).  dZ
//                            goes to LDS for the next step and to the workspace.
//   policy_wgrad_kernel      split-K over the rows: dW = dZ^T X and db = sum dZ for every layer, as one [N][K + 1] GEMM whose
//                            column K is a column of ones in X.  A workgroup owns a 64 x 64 output tile and one slice of
//                            kGradSlice rows (a fixed constant: the sum order does not depend on the grid), stages 32 rows of
//                            dZ and X transposed in LDS per step, and writes fp32 partials; no atomics.
//   policy_grad_combine_kernel  one thread per output word: the partials summed slice by slice in order, times the layer's scale.
//
// The loss is PPO.update()'s (Schulman et al. 2017, SB3's form) for B rows; its gradient follows autograd's conventions:
// torch.min splits a tie evenly, clamp passes the gradient on the closed interval, ReLU has zero gradient at 0.  log_std and
// the four statistics [pg, vl, ent, clip_frac] are reduced as bias-only layers (K = 0) of the same split-K kernel.
// Every sum has a fixed order: for fixed inputs the gradient and the statistics are bitwise the same in every call.
#pragma once

namespace te {

constexpr int kGradSlice = 2048;      // rows (of a layer's reduction) per split-K slice
constexpr int kGradTile = 64;         // output tile of policy_wgrad_kernel: 64 x 64, four waves of 32 x 32
constexpr int kGradStep = 32;         // rows staged in LDS per step
constexpr int kGradLS = kGradStep + 4;
constexpr int kGradLayers = 19;       // 17 weight layers (two of them empty in the default shape), log_std, the statistics
static_assert(kGradLayers == POL_L_COUNT, "one split-K layer per row of pol_layer's table");

// One layer of the split-K reduction: partial[slice][N][K + 1] of dZ[R][N]^T [X[R][K] | 1].  Row counts R are multiples of 32.
struct GradLayer {
  const float* dz;
  const float* x;                      // NULL when K = 0
  float* part;
  float* w_out;                        // [N][K]
  float* b_out;                        // [N]
  float scale;
  int N, K, R, ntiles, ktiles, slices, wg0, word0;
};

struct GradPlan {
  GradLayer L[kGradLayers];
  int wgs, words;
};

// The workspace pointers of the tile kernel (dz[l]: layer POL_L_l's dZ [R][N]; the pseudo-layers' per-row terms) and the per-row inputs
// of the loss.  Like PolicyParams a kernel argument by value: index its arrays with compile-time constants only, or it leaves the SGPRs.
struct GradTileArgs {
  float* save[POL_SV_COUNT];
  int save_ld[POL_SV_COUNT], save_pos[POL_SV_COUNT];
  float* dz[POL_L_COUNT];
  const float *action, *old_logp, *adv, *ret, *adv_mean_std;
  float clip, vf_coef, ent_coef, inv_n;
};

struct PolWsSave {
  const GradTileArgs* g;
  int row0;
  TE_DEV void operator()(int buf, int m, int sub, int col, float v) const {
    g->save[buf][((size_t)(row0 + m) * g->save_pos[buf] + sub) * g->save_ld[buf] + col] = v;
  }
};

// B[k][n] = W[k][n] of a weight W [KO][NI] row-major (the backward of a Linear: dX[M][NI] = dZ[M][KO] W)
template <int NI>
TE_DEV auto pol_wT(const float* __restrict__ W) {
  return [=](int n, int k) {
    return make_float4(W[(size_t)k * NI + n], W[(size_t)(k + 1) * NI + n], W[(size_t)(k + 2) * NI + n], W[(size_t)(k + 3) * NI + n]);
  };
}

// The backward of weight layer L of shape S to its input: epi(m, k, dX[m][k]) of dX[M][K] = dZ[M][N] W.  (l: the layer whose weight
// is read, of L's shape; a constant once the caller's loop is unrolled.)
template <int L, int C, int S, class Epi>
TE_DEV void pol_linear_back(const PolicyParams& P, const float* dZ, int ld, Epi epi, int l = L) {
  constexpr PolLayer y = pol_layer(L, pol_shape(S, C));
  pol_gemm<y.N, y.K, pol_lds_plan(pol_shape(S, C)).M / 16>(dZ, ld, pol_wT<y.K>(P.base + P.at[l].w), [](int) { return 0.f; }, epi);
}

// The LDS of the tile kernel's backward for a shape, in floats from the start of the dynamic LDS (M rows, as the forward's).  When
// pol_forward returns only MU and VAL are live (every layer's output is in the workspace).  In the order of their use:
//   DMU [M][4], DV [M]   d loss / d mu and / d value, written by the loss while it reads MU and VAL; read by both heads
//   H[i] [M][hs[i]]      dZ of a head's hidden layer i (the last one first, down to 0; the pi head, then the vf head)
//   DF [M][fs]           the trunk's gradient: both heads' layer 0 add into it, so it is live through the whole vf head
//   DZ [M][kPolZS]       the concat's gradient, once the heads are dead; live to the end (the chains and conv2 read it)
//   T1, T2 [M][kPolTS]   the chains' and conv2's step tiles, once DF is dead
//   default: H[1], H[0], then DMU and DV behind VAL, all over the dead Z; DF, T1 and T2 in the ping-pong region: the map the kernel
//            has always had, inside the forward's 91 648 B.
//   F = 512: H[0] / H[2] share one tile as wide as max(h0, h2) + 4, H[1] is h1 + 4 wide, DF [16][516] behind them, DMU and DV
//            behind DF, all below the forward's MU: 20 752 words = 83 008 B of the forward's 95 296 B (BO; LEARN 18 704 words).
struct PolGradLds { int M, dmu, dv, hx[3], hs[3], df, fs, dz, t1, t2, words; };

__host__ __device__ constexpr PolGradLds pol_grad_lds_plan(PolShape S) {
  const PolLds f = pol_lds_plan(S);
  const int M = f.M;
  if (M == kPolTileM)
    return {M, f.val + M, f.val + 5 * M, {M * kPolPS, 0, 0}, {f.as, f.bs, f.as}, kPolZWords, f.fs, 0, kPolZWords, kPolZWords + M * kPolTS, f.words};
  const int hb = M * f.as, df = hb + M * f.bs, dmu = df + M * f.fs;
  return {M, dmu, dmu + 4 * M, {0, hb, 0}, {f.as, f.bs, f.as}, df, f.fs, 0, df, df + M * kPolTS, f.words};
}

// A backward plan is sound when every tile lies inside the launch's dynamic LDS (the forward's), DMU / DV are clear of the live MU /
// VAL, and no tile is placed over one that is live at the same time: the head tiles, DF, DMU and DV among themselves (a shape's
// hidden layers 0 and 2 share a tile: 2's dZ is dead when 0's is written); DZ clear of DF; T1 and T2 clear of DZ and each other.
__host__ __device__ constexpr bool pol_grad_lds_ok(PolShape S) {
  const PolLds f = pol_lds_plan(S);
  const PolGradLds p = pol_grad_lds_plan(S);
  const int M = p.M, nh = S.n_hidden;
  auto apart = [](int a, int an, int b, int bn) { return a + an <= b || b + bn <= a; };
  const int dn = 5 * M, mun = f.val + M - f.mu;       // DMU + DV and MU + VAL are each one run of words
  bool ok = p.words == f.words && p.dv == p.dmu + 4 * M && f.val == f.mu + 4 * M && p.dmu >= 0 && p.dmu + dn <= p.words &&
            apart(p.dmu, dn, f.mu, mun) && p.df >= 0 && p.df + M * p.fs <= p.words && apart(p.df, M * p.fs, p.dmu, dn) &&
            p.fs >= S.F + 4 && p.dz >= 0 && p.dz + M * kPolZS <= p.words && apart(p.dz, M * kPolZS, p.df, M * p.fs) &&
            p.t1 >= 0 && p.t2 + M * kPolTS <= p.words && apart(p.t1, M * kPolTS, p.t2, M * kPolTS) &&
            apart(p.t1, M * kPolTS, p.dz, M * kPolZS) && apart(p.t2, M * kPolTS, p.dz, M * kPolZS);
  for (int i = 0; i < nh; ++i) {
    ok = ok && p.hs[i] >= S.h[i] + 4 && p.hx[i] >= 0 && p.hx[i] + M * p.hs[i] <= p.words &&
         apart(p.hx[i], M * p.hs[i], p.dmu, dn) && apart(p.hx[i], M * p.hs[i], p.df, M * p.fs);
    if (i + 1 < nh) ok = ok && apart(p.hx[i], M * p.hs[i], p.hx[i + 1], M * p.hs[i + 1]);
  }
  return ok;
}
constexpr bool pol_grad_lds_is_todays(PolGradLds p) {   // the offsets policy_grad_tile_kernel had before it took a shape
  return p.M == 32 && p.hx[1] == 0 && p.hx[0] == 32 * 68 && p.hs[0] == 68 && p.hs[1] == 68 && p.dmu == 2 * 32 * 68 + 32 * 5 &&
         p.dv == p.dmu + 128 && p.dz == 0 && p.df == kPolZWords && p.fs == 260 && p.t1 == p.df && p.t2 == p.t1 + 32 * 132 &&
         p.words * 4 == kPolLdsBytes;
}
static_assert(pol_grad_lds_ok(pol_shape(POL_SHAPE_DEFAULT, 3)) && pol_grad_lds_is_todays(pol_grad_lds_plan(pol_shape(POL_SHAPE_DEFAULT, 3))),
              "the default shape's backward keeps its LDS map");
static_assert(pol_grad_lds_ok(pol_shape(POL_SHAPE_BO, 3)), "h[128, 256, 512]: the backward fits the forward's LDS");
static_assert(pol_grad_lds_ok(pol_shape(POL_SHAPE_LEARN, 3)), "h[512, 128, 256]: the backward fits the forward's LDS");

// The backward of one head of shape S (hidden layers L0 .. L0 + n_hidden - 1, output layer LAST with NO = 4 or 1 outputs) from
// D [M][NO] = d loss / d output: every hidden layer's dZ to its LDS tile and to the workspace, then to_trunk(m, n, dF[m][n]).
// at(sv, m, sub, col): the tile's rows of saved buffer sv.
template <int L0, int C, int S, class At, class Epi>
TE_DEV void pol_head_back(const PolicyParams& P, const GradTileArgs& g, float* lds, int row0, const float* D, At at, Epi to_trunk) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolGradLds gl = pol_grad_lds_plan(sh);
  constexpr int M = gl.M, nh = sh.n_hidden, LAST = L0 == POL_L_PI0 ? POL_L_MU : POL_L_V;
  constexpr PolLayer yo = pol_layer(LAST, sh);
  constexpr int KL = yo.K, NO = yo.N, il = nh - 1;
  const float* __restrict__ prm = P.base;
  const int tid = threadIdx.x;
  // the last hidden layer: dY = D W_out, d tanh = 1 - y^2
  for (int t = tid; t < M * KL; t += kPolThreads) {
    const int m = t / KL, k = t % KL;
    float d = 0.f;
    if constexpr (NO == 1) {
      d = D[m] * prm[P.at[LAST].w + k];
    } else {
#pragma unroll
      for (int a = 0; a < NO; ++a) d = fmaf(D[m * NO + a], prm[P.at[LAST].w + a * KL + k], d);
    }
    const float y = at(yo.x, m, 0, k), dz = d * (1.f - y * y);
    lds[gl.hx[il] + m * gl.hs[il] + k] = dz;
    g.dz[L0 + il][(size_t)(row0 + m) * KL + k] = dz;
  }
  __syncthreads();
  if constexpr (nh > 2) {
    constexpr PolLayer y2 = pol_layer(L0 + 2, sh);
    pol_linear_back<L0 + 2, C, S>(P, lds + gl.hx[2], gl.hs[2], [&](int m, int n, float v) {
      const float y = at(y2.x, m, 0, n), dz = v * (1.f - y * y);
      lds[gl.hx[1] + m * gl.hs[1] + n] = dz;
      g.dz[L0 + 1][(size_t)(row0 + m) * y2.K + n] = dz;
    });
    __syncthreads();
  }
  if constexpr (nh > 1) {
    constexpr PolLayer y1 = pol_layer(L0 + 1, sh);
    pol_linear_back<L0 + 1, C, S>(P, lds + gl.hx[1], gl.hs[1], [&](int m, int n, float v) {
      const float y = at(y1.x, m, 0, n), dz = v * (1.f - y * y);
      lds[gl.hx[0] + m * gl.hs[0] + n] = dz;
      g.dz[L0][(size_t)(row0 + m) * y1.K + n] = dz;
    });
    __syncthreads();
  }
  pol_linear_back<L0, C, S>(P, lds + gl.hx[0], gl.hs[0], to_trunk);
  __syncthreads();
}

template <int C, int S = POL_SHAPE_DEFAULT>
__global__ __launch_bounds__(kPolThreads) void policy_grad_tile_kernel(PolicyParams P, PolicyIn in, GradTileArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pol_lds[];
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolGradLds gl = pol_grad_lds_plan(sh);
  constexpr int M = gl.M, F = sh.F;
  const int tid = threadIdx.x, row0 = blockIdx.x * M;
  const float* __restrict__ prm = P.base;
  pol_forward<C, S>(P, in, pol_lds, row0, PolWsSave{&g, row0});

  // LDS of the backward (pol_grad_lds_plan): the forward's MU / VAL stay where pol_forward left them until the loss has read them
  float* DMU = pol_lds + gl.dmu;                   // [M][4]
  float* DV = pol_lds + gl.dv;                     // [M]
  float* DZ = pol_lds + gl.dz;                     // [M][kPolZS] gradient of the concat, once the heads are done
  float* DF = pol_lds + gl.df;                     // [M][gl.fs]
  float* T1 = pol_lds + gl.t1;                     // [M][kPolTS] x 2 once DF is dead
  float* T2 = pol_lds + gl.t2;
  auto at = [&](int sv, int m, int sub, int col) { return g.save[sv][((size_t)(row0 + m) * g.save_pos[sv] + sub) * g.save_ld[sv] + col]; };

  // ---- the loss of each row (thread tid = row: mu and value are its own)
  if (tid < M) {
    const int row = row0 + tid;
    const float* log_std = prm + P.log_std;
    float dmu[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f}, st[4] = {0.f, 0.f, 0.f, 0.f}, dv = 0.f;
    if (row < in.n) {
      const size_t s = in.index ? (size_t)in.index[row] : (size_t)row;
      const float v = pol_val_lds<S>(pol_lds)[tid];
      float logp = 0.f, ent = 0.f, d[4], var[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {   // torch.distributions.Normal(mu, exp(log_std)).log_prob(action).sum(-1), entropy().sum(-1)
        const float ls = log_std[a], sig = expf(ls);
        d[a] = g.action[s * 4 + a] - pol_mu_lds<S>(pol_lds)[tid * 4 + a];
        var[a] = sig * sig;
        logp += -(d[a] * d[a]) / (2.f * var[a]) - ls - 0.9189385332046727f;
        ent += 1.4189385332046727f + ls;
      }
      float A = g.adv[s];
      if (g.adv_mean_std) A = (A - g.adv_mean_std[0]) / (g.adv_mean_std[1] + 1e-8f);
      const float ratio = expf(logp - g.old_logp[s]), lo = 1.f - g.clip, hi = 1.f + g.clip;
      const float s1 = A * ratio, s2 = A * fminf(fmaxf(ratio, lo), hi);
      const float g1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f), g2 = s2 < s1 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
      // pg = -mean(min(s1, s2)): d pg / d ratio = -(g1 A + g2 A [lo <= ratio <= hi]) / B, d ratio / d logp = ratio
      const float dlogp = -g.inv_n * (g1 * A + g2 * A * (ratio >= lo && ratio <= hi ? 1.f : 0.f)) * ratio;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        dmu[a] = dlogp * d[a] / var[a];
        dls[a] = dlogp * (d[a] * d[a] / var[a] - 1.f) - g.ent_coef * g.inv_n;
      }
      const float e = v - g.ret[s];
      dv = g.vf_coef * 2.f * e * g.inv_n;
      st[0] = -fminf(s1, s2); st[1] = e * e; st[2] = ent; st[3] = fabsf(ratio - 1.f) > g.clip ? 1.f : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {     // padding rows (row >= n) get zeros: everything downstream of them is exactly 0
      DMU[tid * 4 + a] = dmu[a];
      g.dz[POL_L_MU][(size_t)row * 4 + a] = dmu[a];
      g.dz[POL_L_LOGSTD][(size_t)row * 4 + a] = dls[a];
      g.dz[POL_L_STATS][(size_t)row * 4 + a] = st[a];
    }
    DV[tid] = dv;
    g.dz[POL_L_V][row] = dv;
  }
  __syncthreads();

  // ---- heads: d tanh = 1 - y^2; the two heads' gradients of the trunk add up in DF, then ReLU's mask
  pol_head_back<POL_L_PI0, C, S>(P, g, pol_lds, row0, DMU, at, [&](int m, int n, float v) { DF[m * gl.fs + n] = v; });
  pol_head_back<POL_L_VF0, C, S>(P, g, pol_lds, row0, DV, at, [&](int m, int n, float v) {
    const float dz = at(POL_SV_F, m, 0, n) > 0.f ? DF[m * gl.fs + n] + v : 0.f;
    DF[m * gl.fs + n] = dz;
    g.dz[POL_L_F][(size_t)(row0 + m) * F + n] = dz;
  });

  // ---- trunk -> the concat: conv2 columns 0..191 (flatten order co * 3 + ow2), inertial 192..319, last_action 320..447
  pol_linear_back<POL_L_F, C, S>(P, DF, gl.fs, [&](int m, int n, float v) {
    const float dz = at(POL_SV_FX, m, 0, n) > 0.f ? v : 0.f;
    const size_t row = (size_t)(row0 + m);
    DZ[m * kPolZS + n] = dz;
    if (n < 192) g.dz[POL_L_C2][(row * 3 + n % 3) * 64 + n / 3] = dz;
    else if (n < 320) g.dz[POL_L_IN2][row * 128 + n - 192] = dz;
    else g.dz[POL_L_AC2][row * 128 + n - 320] = dz;
  });
  __syncthreads();

  // ---- the inertial and last_action MLPs: down to the first layer's dZ (their inputs need no gradient)
  constexpr auto layer = [](int l) { return pol_layer(l, pol_shape(S, C)); };
  constexpr auto same = [=](int a, int b) { return layer(a).N == layer(b).N && layer(a).K == layer(b).K; };
  static_assert(same(POL_L_IN1, POL_L_AC1) && same(POL_L_IN2, POL_L_AC2), "the two chains' hidden layers have one shape");
  static_assert(layer(POL_L_F).K == 448 && layer(POL_L_C2).N == 64 && layer(POL_L_IN2).N == 128 && layer(POL_L_C1).N == 32,
                "the extractor is the same for every shape");
#pragma unroll
  for (int chain = 0; chain < 2; ++chain) {   // unrolled: l0, and with it every index into P and g, is a compile-time constant
    const int l0 = chain ? POL_L_AC0 : POL_L_IN0;
    const int sv1 = layer(l0 + 1).x, sv2 = layer(l0 + 2).x;
    pol_linear_back<POL_L_IN2, C, S>(P, DZ + 192 + 128 * chain, kPolZS, [&](int m, int n, float v) {
      const float d = at(sv2, m, 0, n) > 0.f ? v : 0.f;
      T1[m * kPolTS + n] = d;
      g.dz[l0 + 1][(size_t)(row0 + m) * 128 + n] = d;
    }, l0 + 2);
    __syncthreads();
    pol_linear_back<POL_L_IN1, C, S>(P, T1, kPolTS, [&](int m, int n, float v) {
      g.dz[l0][(size_t)(row0 + m) * 128 + n] = at(sv1, m, 0, n) > 0.f ? v : 0.f;
    }, l0 + 1);
    __syncthreads();
  }

  // ---- conv2 -> conv1, one conv2 output column at a time: dZ of the 12 conv1 positions conv2 reads
  for (int ow2 = 0; ow2 < 3; ++ow2) {
    for (int t = tid; t < M * 64; t += kPolThreads) {
      const int m = t >> 6, co = t & 63;
      T2[m * kPolTS + co] = DZ[m * kPolZS + co * 3 + ow2];
    }
    __syncthreads();
    pol_linear_back<POL_L_C2, C, S>(P, T2, kPolTS, [&](int m, int n, float v) {
      // n = ci * 4 + kh * 2 + kw: conv1 channel ci at position p = ow2 * 4 + kh * 2 + kw
      const float d = at(POL_SV_C2X, m, ow2, n) > 0.f ? v : 0.f;
      g.dz[POL_L_C1][((size_t)(row0 + m) * 12 + ow2 * 4 + (n & 3)) * 32 + (n >> 2)] = d;
    });
    __syncthreads();
  }
}

// The split-K plan of shape S over Bp padded rows: layer l reduces dz[l] against x[l] (NULL where K = 0) into partials that take(bytes)
// hands out in layer order, and policy_grad_combine_kernel sums them into grad (at P's offsets) and stats.  Host only; both workspace
// layouts end in it.
template <class Take>
inline GradPlan policy_grad_plan(PolShape S, size_t Bp, const float* const (&dz)[kGradLayers], const float* const (&x)[kGradLayers], Take take,
                                 float* grad, float* stats, const PolicyParams& P, int n) {
  GradPlan g{};
  for (int l = 0; l < kGradLayers; ++l) {
    const PolLayer y = pol_layer(l, S);
    GradLayer& L = g.L[l];
    L.dz = dz[l];
    L.x = x[l];
    L.N = y.N; L.K = y.K; L.R = (int)(Bp * y.pos);
    L.ntiles = (y.N + kGradTile - 1) / kGradTile;
    L.ktiles = (y.K + 1 + kGradTile - 1) / kGradTile;
    L.slices = (L.R + kGradSlice - 1) / kGradSlice;
    L.wg0 = g.wgs; L.word0 = g.words;
    g.wgs += L.slices * L.ntiles * L.ktiles;
    g.words += y.N * (y.K + 1);
    L.part = static_cast<float*>(take((size_t)L.slices * y.N * (y.K + 1) * sizeof(float)));
    L.w_out = grad && l < POL_L_WEIGHTS ? grad + P.at[l].w : nullptr;
    L.b_out = l == POL_L_STATS ? stats : (grad ? grad + (l == POL_L_LOGSTD ? P.log_std : P.at[l].b) : nullptr);
    L.scale = l == POL_L_STATS ? 1.f / (float)n : 1.f;   // the statistics are means over the n rows
  }
  return g;
}

// The workspace of te_policy_ppo_grad for n rows (Bp = n rounded up to 32 for every shape: policy_wgrad_kernel stages 32 rows per step
// and reads every one of them, so the tile kernel runs Bp / M tiles and a 16-row shape's padding tiles write their rows like any
// padding row: zeros in dZ): every layer's input X [R][K] and pre-activation
// gradient dZ [R][N] row-major, R = Bp x the layer's positions, then the split-K partials, in the order of the take() calls.  Host
// only.  With ws == NULL only the size is computed; otherwise the tile kernel's pointers and the split-K plan are filled in.
inline size_t policy_grad_layout(PolShape S, int n, char* ws, const PolicyParams& P, float* grad, float* stats, GradTileArgs* ta, GradPlan* gp) {
  static_assert(kGradStep == kPolTileM && kGradSlice % kGradStep == 0, "Bp is a multiple of the split-K step, whatever the shape's tile");
  const size_t Bp = ((size_t)n + kGradStep - 1) / kGradStep * kGradStep;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* at = ws ? ws + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  GradTileArgs t{};
  for (int l = 0; l < POL_L_WEIGHTS; ++l) { const PolLayer y = pol_layer(l, S); t.save_pos[y.x] = y.pos; t.save_ld[y.x] = y.K; }
  for (int sv = 0; sv < POL_SV_COUNT; ++sv) t.save[sv] = static_cast<float*>(take(Bp * t.save_pos[sv] * t.save_ld[sv] * sizeof(float)));
  for (int l = 0; l < POL_L_COUNT; ++l) t.dz[l] = static_cast<float*>(take(Bp * pol_layer(l, S).pos * pol_layer(l, S).N * sizeof(float)));

  const float *dz[kGradLayers], *x[kGradLayers];
  for (int l = 0; l < kGradLayers; ++l) {
    dz[l] = t.dz[l];
    x[l] = l < POL_L_WEIGHTS ? t.save[pol_layer(l, S).x] : nullptr;
  }
  const GradPlan g = policy_grad_plan(S, Bp, dz, x, take, grad, stats, P, n);
  if (ta) *ta = t;
  if (gp) *gp = g;
  return off;
}

// The layer of work item `i` (workgroup or word): the table is indexed with compile-time indices only, so it stays in SGPRs.
template <class Key>
TE_DEV GradLayer grad_layer_of(const GradPlan& g, int i, Key key) {
  GradLayer L = g.L[0];
#pragma unroll
  for (int l = 1; l < kGradLayers; ++l)
    if (i >= key(g.L[l])) L = g.L[l];
  return L;
}

__global__ __launch_bounds__(256) void policy_wgrad_kernel(GradPlan g) {
  __shared__ __attribute__((aligned(16))) float sA[kGradTile * kGradLS], sB[kGradTile * kGradLS];
  const GradLayer L = grad_layer_of(g, (int)blockIdx.x, [](const GradLayer& l) { return l.wg0; });
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  const int local = (int)blockIdx.x - L.wg0, per_slice = L.ntiles * L.ktiles;
  const int slice = local / per_slice, nt = (local % per_slice) / L.ktiles, kt = local % L.ktiles;
  const int n0 = nt * kGradTile, c0 = kt * kGradTile, KC = L.K + 1;
  const int s0 = slice * kGradSlice, s1 = min(s0 + kGradSlice, L.R);
  const int wn = wave >> 1, wk = wave & 1;
  pol_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = pol_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = s0; r0 < s1; r0 += kGradStep) {
    // stage: thread (column cc, row quad q) loads 4 rows of one column of dZ and of [X | 1] (lanes read consecutive columns)
#pragma unroll
    for (int e = tid; e < kGradTile * (kGradStep / 4); e += 256) {
      const int cc = e & 63, q = e >> 6, n = n0 + cc, k = c0 + cc;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (n < L.N) {
        const float* p = L.dz + (size_t)(r0 + 4 * q) * L.N + n;
        a = make_float4(p[0], p[L.N], p[2 * L.N], p[3 * L.N]);
      }
      if (k < L.K) {
        const float* p = L.x + (size_t)(r0 + 4 * q) * L.K + k;
        b = make_float4(p[0], p[L.K], p[2 * L.K], p[3 * L.K]);
      } else if (k == L.K) {
        b = make_float4(1.f, 1.f, 1.f, 1.f);
      }
      *reinterpret_cast<float4*>(sA + cc * kGradLS + 4 * q) = a;
      *reinterpret_cast<float4*>(sB + cc * kGradLS + 4 * q) = b;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kGradStep; ks += 16) {
      float4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const float4*>(sA + (wn * 32 + i * 16 + r) * kGradLS + ks + 4 * h);
        b[i] = *reinterpret_cast<const float4*>(sB + (wk * 32 + i * 16 + r) * kGradLS + ks + 4 * h);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = pol_mfma4(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  // acc[i][j][v]: output row n (A's row) = n0 + wn * 32 + i * 16 + 4 h + v, column (B's column) = c0 + wk * 32 + j * 16 + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int n = n0 + wn * 32 + i * 16 + 4 * h + v, k = c0 + wk * 32 + j * 16 + r;
        if (n < L.N && k < KC) L.part[((size_t)slice * L.N + n) * KC + k] = acc[i][j][v];
      }
}

__global__ __launch_bounds__(256) void policy_grad_combine_kernel(GradPlan g) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  if (w >= g.words) return;
  const GradLayer L = grad_layer_of(g, w, [](const GradLayer& l) { return l.word0; });
  const int local = w - L.word0, KC = L.K + 1, n = local / KC, k = local % KC;
  const size_t stride = (size_t)L.N * KC;
  float s = 0.f;
  for (int sl = 0; sl < L.slices; ++sl) s += L.part[sl * stride + local];
  s *= L.scale;
  if (k < L.K) L.w_out[(size_t)n * L.K + k] = s;
  else L.b_out[n] = s;
}

}  // namespace te
