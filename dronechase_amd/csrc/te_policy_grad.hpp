// te_policy_grad.hpp — the gradient of PPO's loss for LidarInertialActionPolicy (dronechase_amd/ppo.py PPO.update) with respect to
// every parameter, in te_policy_act's packed layout (te_policy_ppo_grad, include/threatengage.h).  Three launches:
//
//   policy_grad_tile_kernel  one 256-thread workgroup per tile of kPolTileM = 32 rows, the layer code of te_policy.hpp: the forward
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
constexpr int kGradLayers = 17;       // 15 weight layers, log_std, the statistics

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

// The workspace pointers of the tile kernel and the per-row inputs of the loss.
struct GradTileArgs {
  float* save[POL_SV_COUNT];
  int save_ld[POL_SV_COUNT], save_pos[POL_SV_COUNT];
  float *dz_c1, *dz_c2, *dz_in[3], *dz_ac[3], *dz_f, *dz_pi[2], *dz_vf[2], *dz_mu, *dz_v, *dls, *st;
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

// B[k][n] = W[k][n] of a weight W [KO][NI] row-major (the backward of a Linear: dX[32][NI] = dZ[32][KO] W)
template <int NI>
TE_DEV auto pol_wT(const float* __restrict__ W) {
  return [=](int n, int k) {
    return make_float4(W[(size_t)k * NI + n], W[(size_t)(k + 1) * NI + n], W[(size_t)(k + 2) * NI + n], W[(size_t)(k + 3) * NI + n]);
  };
}

template <int C>
__global__ __launch_bounds__(kPolThreads) void policy_grad_tile_kernel(PolicyParams P, PolicyIn in, GradTileArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pol_lds[];
  const int tid = threadIdx.x, row0 = blockIdx.x * kPolTileM;
  const float* __restrict__ prm = P.base;
  pol_forward<C>(P, in, pol_lds, row0, PolWsSave{&g, row0});

  // LDS of the backward: the forward's MU / VAL stay where pol_forward left them until the loss has read them
  float* HA = pol_lds;                             // [32][kPolPS] head tiles
  float* HB = pol_lds + kPolTileM * kPolPS;
  float* DMU = pol_val_lds(pol_lds) + kPolTileM;   // [32][4], then DV [32]
  float* DV = DMU + kPolTileM * 4;
  float* DZ = pol_lds;                             // [32][kPolZS] gradient of the concat, once the heads are done
  float* DF = pol_lds + kPolZWords;                // [32][kPolFS]
  float* T1 = DF;                                  // [32][kPolTS] x 2 once DF is dead
  float* T2 = T1 + kPolTileM * kPolTS;
  static_assert(2 * kPolTileM * kPolPS + kPolTileM * 10 <= kPolZWords, "head tiles, MU, VAL, DMU and DV fit the feature region");
  auto at = [&](int sv, int m, int sub, int col) { return g.save[sv][((size_t)(row0 + m) * g.save_pos[sv] + sub) * g.save_ld[sv] + col]; };
  auto zero = [](int) { return 0.f; };

  // ---- the loss of each row (thread tid = row: mu and value are its own)
  if (tid < kPolTileM) {
    const int row = row0 + tid;
    const float* log_std = prm + P.log_std;
    float dmu[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f}, st[4] = {0.f, 0.f, 0.f, 0.f}, dv = 0.f;
    if (row < in.n) {
      const size_t s = in.index ? (size_t)in.index[row] : (size_t)row;
      const float v = pol_val_lds(pol_lds)[tid];
      float logp = 0.f, ent = 0.f, d[4], var[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {   // torch.distributions.Normal(mu, exp(log_std)).log_prob(action).sum(-1), entropy().sum(-1)
        const float ls = log_std[a], sig = expf(ls);
        d[a] = g.action[s * 4 + a] - pol_mu_lds(pol_lds)[tid * 4 + a];
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
      g.dz_mu[(size_t)row * 4 + a] = dmu[a];
      g.dls[(size_t)row * 4 + a] = dls[a];
      g.st[(size_t)row * 4 + a] = st[a];
    }
    DV[tid] = dv;
    g.dz_v[row] = dv;
  }
  __syncthreads();

  // ---- heads: d tanh = 1 - y^2; the two heads' gradients of the trunk add up in DF, then ReLU's mask
  for (int t = tid; t < kPolTileM * 64; t += kPolThreads) {
    const int m = t >> 6, k = t & 63;
    float d = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) d = fmaf(DMU[m * 4 + a], prm[P.muw + a * 64 + k], d);
    const float y = at(POL_SV_MUX, m, 0, k), dz = d * (1.f - y * y);
    HA[m * kPolPS + k] = dz;
    g.dz_pi[1][(size_t)(row0 + m) * 64 + k] = dz;
  }
  __syncthreads();
  pol_gemm<64, 64>(HA, kPolPS, pol_wT<64>(prm + P.pi_w[1]), zero, [&](int m, int n, float v) {
    const float y = at(POL_SV_PI1X, m, 0, n), dz = v * (1.f - y * y);
    HB[m * kPolPS + n] = dz;
    g.dz_pi[0][(size_t)(row0 + m) * 64 + n] = dz;
  });
  __syncthreads();
  pol_gemm<64, 256>(HB, kPolPS, pol_wT<256>(prm + P.pi_w[0]), zero, [&](int m, int n, float v) { DF[m * kPolFS + n] = v; });
  __syncthreads();
  for (int t = tid; t < kPolTileM * 64; t += kPolThreads) {
    const int m = t >> 6, k = t & 63;
    const float y = at(POL_SV_VX, m, 0, k), dz = DV[m] * prm[P.vw + k] * (1.f - y * y);
    HA[m * kPolPS + k] = dz;
    g.dz_vf[1][(size_t)(row0 + m) * 64 + k] = dz;
  }
  __syncthreads();
  pol_gemm<64, 64>(HA, kPolPS, pol_wT<64>(prm + P.vf_w[1]), zero, [&](int m, int n, float v) {
    const float y = at(POL_SV_VF1X, m, 0, n), dz = v * (1.f - y * y);
    HB[m * kPolPS + n] = dz;
    g.dz_vf[0][(size_t)(row0 + m) * 64 + n] = dz;
  });
  __syncthreads();
  pol_gemm<64, 256>(HB, kPolPS, pol_wT<256>(prm + P.vf_w[0]), zero, [&](int m, int n, float v) {
    const float dz = at(POL_SV_F, m, 0, n) > 0.f ? DF[m * kPolFS + n] + v : 0.f;
    DF[m * kPolFS + n] = dz;
    g.dz_f[(size_t)(row0 + m) * 256 + n] = dz;
  });
  __syncthreads();

  // ---- trunk -> the concat: conv2 columns 0..191 (flatten order co * 3 + ow2), inertial 192..319, last_action 320..447
  pol_gemm<256, 448>(DF, kPolFS, pol_wT<448>(prm + P.fw), zero, [&](int m, int n, float v) {
    const float dz = at(POL_SV_FX, m, 0, n) > 0.f ? v : 0.f;
    const size_t row = (size_t)(row0 + m);
    DZ[m * kPolZS + n] = dz;
    if (n < 192) g.dz_c2[(row * 3 + n % 3) * 64 + n / 3] = dz;
    else if (n < 320) g.dz_in[2][row * 128 + n - 192] = dz;
    else g.dz_ac[2][row * 128 + n - 320] = dz;
  });
  __syncthreads();

  // ---- the inertial and last_action MLPs: down to the first layer's dZ (their inputs need no gradient)
#pragma unroll
  for (int chain = 0; chain < 2; ++chain) {
    const int* w = chain ? P.ac_w : P.in_w;
    float* const* dz = chain ? g.dz_ac : g.dz_in;
    const int sv1 = chain ? POL_SV_AC1X : POL_SV_IN1X, sv2 = chain ? POL_SV_AC2X : POL_SV_IN2X;
    pol_gemm<128, 128>(DZ + 192 + 128 * chain, kPolZS, pol_wT<128>(prm + w[2]), zero, [&](int m, int n, float v) {
      const float d = at(sv2, m, 0, n) > 0.f ? v : 0.f;
      T1[m * kPolTS + n] = d;
      dz[1][(size_t)(row0 + m) * 128 + n] = d;
    });
    __syncthreads();
    pol_gemm<128, 128>(T1, kPolTS, pol_wT<128>(prm + w[1]), zero, [&](int m, int n, float v) {
      dz[0][(size_t)(row0 + m) * 128 + n] = at(sv1, m, 0, n) > 0.f ? v : 0.f;
    });
    __syncthreads();
  }

  // ---- conv2 -> conv1, one conv2 output column at a time: dZ of the 12 conv1 positions conv2 reads
  for (int ow2 = 0; ow2 < 3; ++ow2) {
    for (int t = tid; t < kPolTileM * 64; t += kPolThreads) {
      const int m = t >> 6, co = t & 63;
      T2[m * kPolTS + co] = DZ[m * kPolZS + co * 3 + ow2];
    }
    __syncthreads();
    pol_gemm<64, 128>(T2, kPolTS, pol_wT<128>(prm + P.c2w), zero, [&](int m, int n, float v) {
      // n = ci * 4 + kh * 2 + kw: conv1 channel ci at position p = ow2 * 4 + kh * 2 + kw
      const float d = at(POL_SV_C2X, m, ow2, n) > 0.f ? v : 0.f;
      g.dz_c1[((size_t)(row0 + m) * 12 + ow2 * 4 + (n & 3)) * 32 + (n >> 2)] = d;
    });
    __syncthreads();
  }
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
