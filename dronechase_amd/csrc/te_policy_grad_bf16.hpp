// te_policy_grad_bf16.hpp — te_policy_ppo_grad_bf16: the gradient of te_policy_grad.hpp with bf16 operands on v_mfma_f32_16x16x32_bf16,
// opt-in (PPOConfig.fused_update_bf16, FusedPolicy(grad_precision="bf16")).  The fp32 kernels are untouched.  Three launches again:
//
//   policy_grad_bf16_tile_kernel  one workgroup per tile of 32 rows: pol_forward_bf16 (te_policy_bf16.hpp: bitwise te_policy_act_bf16's
//                                 forward) with a save hook, the loss of each row (policy_grad_tile_kernel's, fp32), then the backward
//                                 to every layer's pre-activation gradient dZ.  Each backward step is pol_gemm_bf16 on the TRANSPOSED
//                                 bf16 weights (dX = dZ W: the B fragment of output column k is 8 consecutive n of W^T[k][.]).
//   policy_wgrad_bf16_kernel      split-K over the rows: dW = dZ^T [X | 1] per layer, bf16 operands, fp32 partials.  No LDS: the tile
//                                 kernel writes dZ and X TRANSPOSED (below), so a fragment is one 16-byte load of 8 consecutive rows.
//                                 log_std and the statistics are fp32 bias-only layers, summed in a fixed tree.
//   policy_grad_combine_kernel    te_policy_grad.hpp's, unchanged: the plan struct is the same.
//
// Numerics contract (include/threatengage.h states it too; tests/_policy_grad_bf16_ref.py is it as PyTorch autograd):
//   1. The forward is te_policy_act_bf16's, bit for bit (one function, pol_forward_bf16).
//   2. The workspace holds every layer's input as the bf16 values the MFMA consumed.  ReLU's mask is y > 0 and tanh' is 1 - y^2 (fp32)
//      on that stored bf16 output y.
//   3. The loss of a row and its derivatives are policy_grad_tile_kernel's, in fp32.
//   4. Every pre-activation gradient dZ is computed in fp32 from the MFMA accumulator and rounded ONCE to bf16 (nearest-even) where it
//      is stored; everything downstream (the next dX, dW, db, the VALU step from dmu / dv into the last hidden layer) reads the rounded
//      value.  dmu and dv count as dZ.  log_std's per-row gradient and the four statistics stay fp32.  The trunk's dZ is ONE
//      accumulator over both heads (dZ_pi0 W_pi0 + dZ_vf0 W_vf0), masked, then rounded.
//   5. dX = dZ W with the bf16 weights; the last hidden layer of a head: the fp32 mu / value weights on the vector ALU.
//   6. dW = dZ^T [X | 1], bf16 operands (the 1 is bf16 1.0), fp32 accumulation; slices of kGradSlice reduction rows, partials summed
//      slice by slice in order.  The gradient is the fp32 master weights': the weight rounding is straight-through.
//   7. Repeated calls are bitwise equal; `index` equals pre-gathered rows bitwise; rows past n contribute exactly 0 whatever the
//      workspace held (the tile kernel writes every one of the workspace's Bp = roundup(n, 32) rows before anything reads them).
//
// Workspace: per saved buffer sv the layer input X^T [K][pos * Bp] and per weight layer dZ^T [N][pos * Bp], bf16; the reduction row of
// (sample row, conv position sub) is sub * Bp + row, so the 4 rows a lane holds of one MFMA output column are 8 contiguous bytes.
// log_std's and the statistics' per-row terms: fp32 [Bp][4].  Then the fp32 split-K partials.  Half the fp32 call's bytes per row.
//
// Transposed weights: ONE uint16 buffer; per MFMA layer whose input needs a gradient (all but conv1, inertial.0 and action.0), in the
// order of the fp32 buffer, W^T [K][Np], Np = roundup(N, 32), columns N .. Np - 1 zero.
//
// Tile height: 32 rows for every shape (256 threads for the default shape, 512 for F = 512).  The backward holds four tiles at once
// while the trunk's gradient is formed (pi.0's dZ, vf.0's dZ, the head's other tile, and DF): at the inference's 48 rows that is
// 162.8 KB for h[512, 128, 256], more than a CU has; at 32 it is 108.5 KB (BO 92.2 KB), one workgroup of 8 waves per CU, and each
// workgroup reads the 2 x 1.5 / 2.1 MB of bf16 weights for 32 rows (the fp32 kernel: 3.1 / 4.1 MB for 16).  The default shape's
// backward fits the 46.6 KB of its forward + DZ, so three workgroups (12 waves) share a CU as in the inference.
#pragma once

namespace te {

constexpr int kPolGradBM = 32;                 // rows per workgroup, every shape

__host__ __device__ constexpr int pol_sv_pos(int sv) { return sv == POL_SV_C1X ? 12 : sv == POL_SV_C2X ? 3 : 1; }
__host__ __device__ constexpr bool pol_needs_dx(int l) { return l != POL_L_C1 && l != POL_L_IN0 && l != POL_L_AC0; }

// Element offsets of every layer's W^T [K][Np] in the transposed bf16 buffer (PolicyBf16: the same struct, another layout).
inline PolicyBf16 policy_bf16_t_layout(PolShape S) {
  PolicyBf16 w{};
  int o = 0;
  for (int l = 0; l < kPolBMfmaLayers; ++l) {
    const PolLayer y = pol_layer(l, S);
    w.at[l] = o;
    if (pol_needs_dx(l)) o += y.K * pol_kp(y.N);
  }
  w.words = o;
  return w;
}

struct PolPackTPlan {
  struct { int dst, src, N, K, Np; } l[kPolBMfmaLayers];
  int end[kPolBMfmaLayers];                    // dst + K * Np (a layer without a block: dst)
  int total;
};

inline PolPackTPlan policy_pack_t_plan(PolShape S) {
  const PolicyParams P = policy_layout(S);
  const PolicyBf16 W = policy_bf16_t_layout(S);
  PolPackTPlan p{};
  for (int l = 0; l < kPolBMfmaLayers; ++l) {
    const PolLayer y = pol_layer(l, S);
    p.l[l] = {W.at[l], P.at[l].w, y.N, y.K, pol_kp(y.N)};
    p.end[l] = W.at[l] + (pol_needs_dx(l) ? y.K * pol_kp(y.N) : 0);
  }
  p.total = W.words;
  return p;
}

// thread i writes element i of the transposed buffer: W^T[k][n] = bf16(W[n][k]), a pad column zero
__global__ __launch_bounds__(256) void policy_pack_bf16_t_kernel(const float* __restrict__ params, PolPackTPlan plan, __bf16* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= plan.total) return;
  int dst = 0, src = 0, N = 1, K = 1, Np = 1;
#pragma unroll
  for (int l = kPolBMfmaLayers - 1; l >= 0; --l)
    if (i < plan.end[l]) { dst = plan.l[l].dst; src = plan.l[l].src; N = plan.l[l].N; K = plan.l[l].K; Np = plan.l[l].Np; }
  const int e = i - dst, k = e / Np, n = e - k * Np;
  out[i] = n < N ? (__bf16)params[src + (size_t)n * K + k] : (__bf16)0.f;
}

// The workspace pointers of the tile kernel and the per-row inputs of the loss.  A kernel argument by value: index its arrays with
// compile-time constants only.
struct GradTileArgsB {
  __bf16* save[POL_SV_COUNT];                  // X^T [K][pos * Bp]
  __bf16* dz[POL_L_WEIGHTS];                   // dZ^T [N][pos * Bp]
  float *dls, *st;                             // [Bp][4]: d loss / d log_std per row, the statistics' per-row terms
  const float *action, *old_logp, *adv, *ret, *adv_mean_std;
  float clip, vf_coef, ent_coef, inv_n;
  int Bp;
};

// rows m0 .. m0 + 3 of column col (conv position sub) of a transposed workspace buffer with `pos` positions per row
TE_DEV __bf16* pol_ws_at(__bf16* base, int pos, int Bp, int row, int sub, int col) { return base + ((size_t)col * pos + sub) * Bp + row; }

struct PolWsSaveB {
  const GradTileArgsB* g;
  int row0;
  TE_DEV void x4(int buf, int m0, int sub, int col, pol_bf16x4 v) const {
    *reinterpret_cast<pol_bf16x4*>(pol_ws_at(g->save[buf], pol_sv_pos(buf), g->Bp, row0 + m0, sub, col)) = v;
  }
  TE_DEV void x1(int buf, int m, int sub, int col, __bf16 v) const { *pol_ws_at(g->save[buf], pol_sv_pos(buf), g->Bp, row0 + m, sub, col) = v; }
};

// The LDS of the tile kernel for a shape.  The forward runs in pol_lds_plan_bf16(S, 32)'s map; when it returns only MU and VAL are
// live.  The backward's tiles, offsets in bf16 elements, in the order of their use:
//   KEEP [M][ks]   dZ of pi's hidden layer 0, kept until the trunk's gradient reads it together with vf's
//   A [M][as]      dZ of a head's hidden layer 2, then of vf's layer 0;  B [M][bs]: of hidden layer 1
//   DF [M][fs]     the trunk's dZ, at 0, in a region max(fs, 2 (128 + 8)) wide
//   DZ [M][448+8]  the concat's dZ, over the dead head tiles
//   T1, T2 [M][128+8]  the chains' and conv2's step tiles, over the dead DF
// DMU [M][4] and DV [M] (fp32) lie behind the forward's map AND the backward's: the loss writes them while MU and VAL are live.
struct PolGradLdsB { int M, threads, df, fs, keep, ks, a, as, b, bs, dz, t1, t2, dmu, dv, bytes; };

__host__ __device__ constexpr PolGradLdsB pol_grad_lds_plan_bf16(PolShape S) {
  const PolLdsB f = pol_lds_plan_bf16(S, kPolGradBM);
  const int M = f.M, fs = S.F + kPolBPad, ks = S.h[0] + kPolBPad;
  const int dfw = pol_max(fs, 2 * kPolBTS);
  const int keep = M * dfw, a = keep + M * ks, b = a + M * f.as, heads_end = b + M * f.bs;
  const int dz = M * dfw, end = pol_max(heads_end, dz + M * kPolBZS);
  const int dmu = (pol_max(end * 2, f.bytes) + 15) / 16 * 4;   // in floats, 16-byte aligned
  return {M, f.threads, 0, fs, keep, ks, a, f.as, b, f.bs, dz, 0, M * kPolBTS, dmu, dmu + 4 * M, (dmu + 5 * M) * 4};
}

__host__ __device__ constexpr bool pol_grad_lds_bf16_ok(PolShape S) {
  const PolLdsB f = pol_lds_plan_bf16(S, kPolGradBM);
  const PolGradLdsB p = pol_grad_lds_plan_bf16(S);
  const int M = p.M, h1 = S.n_hidden > 1 ? S.h[1] : 0, h2 = S.n_hidden > 2 ? S.h[2] : 0;
  auto apart = [](int a, int an, int b, int bn) { return a + an <= b || b + bn <= a; };
  const int df_n = M * p.fs, keep_n = M * p.ks, a_n = M * p.as, b_n = M * p.bs, dz_n = M * kPolBZS, t_n = M * kPolBTS;
  return pol_lds_bf16_ok(S, kPolGradBM) && M == kPolGradBM && M % 16 == 0 && p.bytes <= kPolLdsLimit && S.n_hidden >= 2 &&
         p.fs >= S.F + 8 && p.ks >= S.h[0] + 8 && p.as >= pol_max(S.h[0], h2) + 8 && p.bs >= h1 + 8 &&
         p.fs % 8 == 0 && p.ks % 8 == 0 && p.as % 8 == 0 && p.bs % 8 == 0 && p.keep % 8 == 0 && p.a % 8 == 0 && p.b % 8 == 0 && p.dz % 8 == 0 &&
         p.t2 % 8 == 0 && p.dmu % 4 == 0 &&
         // the heads' tiles and DF are live together; DZ with DF; T1 / T2 with DZ
         apart(p.keep, keep_n, p.a, a_n) && apart(p.keep, keep_n, p.b, b_n) && apart(p.a, a_n, p.b, b_n) &&
         apart(p.df, df_n, p.keep, keep_n) && apart(p.df, df_n, p.a, a_n) && apart(p.df, df_n, p.b, b_n) && apart(p.df, df_n, p.dz, dz_n) &&
         apart(p.t1, t_n, p.t2, t_n) && apart(p.t1, t_n, p.dz, dz_n) && apart(p.t2, t_n, p.dz, dz_n) &&
         // DMU / DV behind every tile of both maps, clear of the forward's MU / VAL
         p.dmu * 4 >= f.bytes && p.dmu * 2 >= pol_max(pol_max(p.b + b_n, p.dz + dz_n), p.t2 + t_n) && p.dv == p.dmu + 4 * M &&
         p.bytes >= (p.dv + M) * 4;
}
static_assert(pol_grad_lds_bf16_ok(pol_shape(POL_SHAPE_DEFAULT, 3)) && pol_grad_lds_plan_bf16(pol_shape(POL_SHAPE_DEFAULT, 3)).bytes * 3 <= kPolLdsLimit,
              "the default shape: three workgroups per CU");
static_assert(pol_grad_lds_bf16_ok(pol_shape(POL_SHAPE_BO, 3)), "h[128, 256, 512]: forward and backward fit a CU at 32 rows");
static_assert(pol_grad_lds_bf16_ok(pol_shape(POL_SHAPE_LEARN, 3)), "h[512, 128, 256]: forward and backward fit a CU at 32 rows");

// the LDS tile (offset, stride) of the dZ of a head's hidden layer i
__host__ __device__ constexpr int pol_gb_tile(PolGradLdsB p, int i, bool pi) { return i == 1 ? p.b : (i == 0 && pi) ? p.keep : p.a; }
__host__ __device__ constexpr int pol_gb_ld(PolGradLdsB p, int i, bool pi) { return i == 1 ? p.bs : (i == 0 && pi) ? p.ks : p.as; }

// The backward of weight layer L of shape S to its input: epi(m0, k, dX[m0 .. m0 + 3][k]) of dX[M][K] = dZ[M][N] W, W^T from the
// transposed buffer (l: the layer whose weight is read, of L's shape).
template <int L, int C, int S, class Epi>
TE_DEV void pol_linear_back_bf16(const PolicyBf16& Wt, const __bf16* dZ, int ld, Epi epi, int l = L) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolLayer y = pol_layer(L, sh);
  constexpr PolGradLdsB gl = pol_grad_lds_plan_bf16(sh);
  static_assert(y.N % 32 == 0 && y.K % 16 == 0, "whole k-blocks of dZ, whole 16-column slices of dX");
  pol_gemm_bf16<y.N, y.K, gl.M / 16, gl.threads / 64>(dZ, ld, reinterpret_cast<const __bf16*>(Wt.base) + Wt.at[l], [](int) { return 0.f; }, epi);
}

// The backward of one head (hidden layers L0 .. L0 + n_hidden - 1, output layer mu or value) from D [M][NO] = d loss / d output
// (already rounded to bf16): every hidden layer's dZ to its LDS tile and to the workspace.  Layer 0's dZ stays in its tile (KEEP for
// pi, A for vf) for the trunk.  ld4(sv, m0, sub, col): rows m0 .. m0 + 3 of a saved buffer's column.
template <int L0, int C, int S, class Ld>
TE_DEV void pol_head_back_bf16(const PolicyParams& P, const PolicyBf16& Wt, const GradTileArgsB& g, __bf16* lds, int row0, const float* D, Ld ld4) {
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolGradLdsB gl = pol_grad_lds_plan_bf16(sh);
  constexpr bool pi = L0 == POL_L_PI0;
  constexpr int M = gl.M, NT = gl.threads, nh = sh.n_hidden, LAST = pi ? POL_L_MU : POL_L_V;
  constexpr PolLayer yo = pol_layer(LAST, sh);
  constexpr int KL = yo.K, NO = yo.N, il = nh - 1;
  const float* __restrict__ prm = P.base;
  const int tid = threadIdx.x;
  {  // the last hidden layer: dY = D W_out on the vector ALU, d tanh = 1 - y^2; a thread takes 4 rows of one column
    __bf16* H = lds + pol_gb_tile(gl, il, pi);
    constexpr int hs = pol_gb_ld(gl, il, pi);
    for (int t = tid; t < KL * (M / 4); t += NT) {
      const int k = t / (M / 4), m0 = (t % (M / 4)) * 4;
      float w[NO];
#pragma unroll
      for (int a = 0; a < NO; ++a) w[a] = prm[P.at[LAST].w + a * KL + k];
      const pol_bf16x4 y = ld4(yo.x, m0, 0, k);
      pol_bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float d = 0.f;
#pragma unroll
        for (int a = 0; a < NO; ++a) d = fmaf(D[(m0 + i) * NO + a], w[a], d);
        const float yy = (float)y[i];
        o[i] = (__bf16)(d * (1.f - yy * yy));
      }
      pol_tile_put4(H + m0 * hs + k, hs, o);
      *reinterpret_cast<pol_bf16x4*>(pol_ws_at(g.dz[L0 + il], 1, g.Bp, row0 + m0, 0, k)) = o;
    }
    __syncthreads();
  }
  if constexpr (nh > 2) {
    constexpr PolLayer y2 = pol_layer(L0 + 2, sh);
    pol_linear_back_bf16<L0 + 2, C, S>(Wt, lds + pol_gb_tile(gl, 2, pi), pol_gb_ld(gl, 2, pi), [&](int m0, int n, pol_f32x4 v) {
      const pol_bf16x4 y = ld4(y2.x, m0, 0, n);
      pol_bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float yy = (float)y[i]; o[i] = (__bf16)(v[i] * (1.f - yy * yy)); }
      pol_tile_put4(lds + pol_gb_tile(gl, 1, pi) + m0 * pol_gb_ld(gl, 1, pi) + n, pol_gb_ld(gl, 1, pi), o);
      *reinterpret_cast<pol_bf16x4*>(pol_ws_at(g.dz[L0 + 1], 1, g.Bp, row0 + m0, 0, n)) = o;
    });
    __syncthreads();
  }
  if constexpr (nh > 1) {
    constexpr PolLayer y1 = pol_layer(L0 + 1, sh);
    pol_linear_back_bf16<L0 + 1, C, S>(Wt, lds + pol_gb_tile(gl, 1, pi), pol_gb_ld(gl, 1, pi), [&](int m0, int n, pol_f32x4 v) {
      const pol_bf16x4 y = ld4(y1.x, m0, 0, n);
      pol_bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float yy = (float)y[i]; o[i] = (__bf16)(v[i] * (1.f - yy * yy)); }
      pol_tile_put4(lds + pol_gb_tile(gl, 0, pi) + m0 * pol_gb_ld(gl, 0, pi) + n, pol_gb_ld(gl, 0, pi), o);
      *reinterpret_cast<pol_bf16x4*>(pol_ws_at(g.dz[L0], 1, g.Bp, row0 + m0, 0, n)) = o;
    });
    __syncthreads();
  }
}

// ReLU's mask on the stored bf16 output, then the one rounding of dZ
TE_DEV pol_bf16x4 pol_relu_back4(pol_bf16x4 y, pol_f32x4 v) {
  pol_bf16x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (float)y[i] > 0.f ? (__bf16)v[i] : (__bf16)0.f;
  return o;
}

template <int C, int S>
__global__ __launch_bounds__(pol_grad_lds_plan_bf16(pol_shape(S, C)).threads) void policy_grad_bf16_tile_kernel(PolicyParams P, PolicyBf16 Wb, PolicyBf16 Wt,
                                                                                                            PolicyIn in, GradTileArgsB g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_lds_gb[];
  constexpr PolShape sh = pol_shape(S, C);
  constexpr PolGradLdsB gl = pol_grad_lds_plan_bf16(sh);
  constexpr PolLdsB fl = pol_lds_plan_bf16(sh, kPolGradBM);
  constexpr int M = gl.M, NT = gl.threads, MT = M / 16, NW = NT / 64, F = sh.F;
  const int tid = threadIdx.x, row0 = blockIdx.x * M;
  const float* __restrict__ prm = P.base;
  pol_forward_bf16<C, S, M>(P, Wb, in, pol_lds_gb, row0, PolWsSaveB{&g, row0});

  __bf16* lds = reinterpret_cast<__bf16*>(pol_lds_gb);
  float* ldf = reinterpret_cast<float*>(pol_lds_gb);
  float* DMU = ldf + gl.dmu;                       // [M][4]
  float* DV = ldf + gl.dv;                         // [M]
  __bf16* DF = lds + gl.df;                        // [M][gl.fs]
  __bf16* DZ = lds + gl.dz;                        // [M][kPolBZS]
  __bf16* T1 = lds + gl.t1;                        // [M][kPolBTS] x 2 once DF is dead
  __bf16* T2 = lds + gl.t2;
  const __bf16* __restrict__ wt = reinterpret_cast<const __bf16*>(Wt.base);
  auto ld4 = [&](int sv, int m0, int sub, int col) {
    return *reinterpret_cast<const pol_bf16x4*>(pol_ws_at(g.save[sv], pol_sv_pos(sv), g.Bp, row0 + m0, sub, col));
  };
  auto st4 = [&](int l, int pos, int m0, int sub, int col, pol_bf16x4 v) {
    *reinterpret_cast<pol_bf16x4*>(pol_ws_at(g.dz[l], pos, g.Bp, row0 + m0, sub, col)) = v;
  };

  // ---- the loss of each row (thread tid = row: mu and value are its own): policy_grad_tile_kernel's, then dmu and dv rounded
  if (tid < M) {
    const int row = row0 + tid;
    const float* log_std = prm + P.log_std;
    float dmu[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f}, st[4] = {0.f, 0.f, 0.f, 0.f}, dv = 0.f;
    if (row < in.n) {
      const size_t s = in.index ? (size_t)in.index[row] : (size_t)row;
      const float v = ldf[fl.val + tid];
      float logp = 0.f, ent = 0.f, d[4], var[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float ls = log_std[a], sig = expf(ls);
        d[a] = g.action[s * 4 + a] - ldf[fl.mu + tid * 4 + a];
        var[a] = sig * sig;
        logp += -(d[a] * d[a]) / (2.f * var[a]) - ls - 0.9189385332046727f;
        ent += 1.4189385332046727f + ls;
      }
      float A = g.adv[s];
      if (g.adv_mean_std) A = (A - g.adv_mean_std[0]) / (g.adv_mean_std[1] + 1e-8f);
      const float ratio = expf(logp - g.old_logp[s]), lo = 1.f - g.clip, hi = 1.f + g.clip;
      const float s1 = A * ratio, s2 = A * fminf(fmaxf(ratio, lo), hi);
      const float g1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f), g2 = s2 < s1 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
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
      const __bf16 q = (__bf16)dmu[a];
      DMU[tid * 4 + a] = (float)q;
      *pol_ws_at(g.dz[POL_L_MU], 1, g.Bp, row, 0, a) = q;
      g.dls[(size_t)row * 4 + a] = dls[a];
      g.st[(size_t)row * 4 + a] = st[a];
    }
    const __bf16 q = (__bf16)dv;
    DV[tid] = (float)q;
    *pol_ws_at(g.dz[POL_L_V], 1, g.Bp, row, 0, 0) = q;
  }
  __syncthreads();

  // ---- heads: d tanh = 1 - y^2; then the trunk's dZ in one accumulator over both heads' layer 0, ReLU's mask, one rounding
  pol_head_back_bf16<POL_L_PI0, C, S>(P, Wt, g, lds, row0, DMU, ld4);
  pol_head_back_bf16<POL_L_VF0, C, S>(P, Wt, g, lds, row0, DV, ld4);
  {
    constexpr int h0 = sh.h[0];
    static_assert(h0 % 32 == 0 && F % 16 == 0, "whole k-blocks of dZ, whole 16-column slices of dF");
    pol_gemm_bf16<h0, F, MT, NW, h0>(
        lds + gl.keep, gl.ks, wt + Wt.at[POL_L_PI0], [](int) { return 0.f; },
        [&](int m0, int n, pol_f32x4 v) {
          const pol_bf16x4 o = pol_relu_back4(ld4(POL_SV_F, m0, 0, n), v);
          pol_tile_put4(DF + m0 * gl.fs + n, gl.fs, o);
          st4(POL_L_F, 1, m0, 0, n, o);
        },
        lds + gl.a, gl.as, wt + Wt.at[POL_L_VF0]);
    __syncthreads();
  }

  // ---- trunk -> the concat: conv2 columns 0..191 (flatten order co * 3 + ow2), inertial 192..319, last_action 320..447
  pol_linear_back_bf16<POL_L_F, C, S>(Wt, DF, gl.fs, [&](int m0, int n, pol_f32x4 v) {
    const pol_bf16x4 o = pol_relu_back4(ld4(POL_SV_FX, m0, 0, n), v);
    pol_tile_put4(DZ + m0 * kPolBZS + n, kPolBZS, o);
    if (n < 192) st4(POL_L_C2, 3, m0, n % 3, n / 3, o);
    else if (n < 320) st4(POL_L_IN2, 1, m0, 0, n - 192, o);
    else st4(POL_L_AC2, 1, m0, 0, n - 320, o);
  });
  __syncthreads();

  // ---- the inertial and last_action MLPs, side by side (they share nothing): down to the first layer's dZ
  constexpr auto layer = [](int l) { return pol_layer(l, pol_shape(S, C)); };
  constexpr auto same = [=](int a, int b) { return layer(a).N == layer(b).N && layer(a).K == layer(b).K; };
  static_assert(same(POL_L_IN1, POL_L_AC1) && same(POL_L_IN2, POL_L_AC2), "the two chains' hidden layers have one shape");
  static_assert(layer(POL_L_F).K == 448 && layer(POL_L_C2).N == 64 && layer(POL_L_IN2).N == 128 && layer(POL_L_C1).N == 32,
                "the extractor is the same for every shape");
#pragma unroll
  for (int chain = 0; chain < 2; ++chain) {   // unrolled: l0, and with it every index into Wt and g, is a compile-time constant
    const int l0 = chain ? POL_L_AC0 : POL_L_IN0;
    const int sv2 = layer(l0 + 2).x;
    __bf16* T = chain ? T2 : T1;
    pol_linear_back_bf16<POL_L_IN2, C, S>(Wt, DZ + 192 + 128 * chain, kPolBZS, [&](int m0, int n, pol_f32x4 v) {
      const pol_bf16x4 o = pol_relu_back4(ld4(sv2, m0, 0, n), v);
      pol_tile_put4(T + m0 * kPolBTS + n, kPolBTS, o);
      st4(l0 + 1, 1, m0, 0, n, o);
    }, l0 + 2);
  }
  __syncthreads();
#pragma unroll
  for (int chain = 0; chain < 2; ++chain) {
    const int l0 = chain ? POL_L_AC0 : POL_L_IN0;
    const int sv1 = layer(l0 + 1).x;
    pol_linear_back_bf16<POL_L_IN1, C, S>(Wt, chain ? T2 : T1, kPolBTS, [&](int m0, int n, pol_f32x4 v) {
      st4(l0, 1, m0, 0, n, pol_relu_back4(ld4(sv1, m0, 0, n), v));
    }, l0 + 1);
  }
  __syncthreads();

  // ---- conv2 -> conv1, one conv2 output column at a time: dZ of the 12 conv1 positions conv2 reads
  for (int ow2 = 0; ow2 < 3; ++ow2) {
    for (int t = tid; t < M * 64; t += NT) {
      const int m = t >> 6, co = t & 63;
      T1[m * kPolBTS + co] = DZ[m * kPolBZS + co * 3 + ow2];
    }
    __syncthreads();
    pol_linear_back_bf16<POL_L_C2, C, S>(Wt, T1, kPolBTS, [&](int m0, int n, pol_f32x4 v) {
      // n = ci * 4 + kh * 2 + kw: conv1 channel ci at position p = ow2 * 4 + kh * 2 + kw
      st4(POL_L_C1, 12, m0, ow2 * 4 + (n & 3), n >> 2, pol_relu_back4(ld4(POL_SV_C2X, m0, ow2, n), v));
    });
    __syncthreads();
  }
}

// The workspace of te_policy_ppo_grad_bf16 for n rows, in the order of the take() calls (the header's top says what each holds).
// Host only.  With ws == NULL only the size is computed; otherwise the tile kernel's pointers and the split-K plan are filled in.  The
// plan is te_policy_grad.hpp's GradPlan: its dz / x pointers carry the bf16 transposed buffers (the fp32 per-row terms for log_std and
// the statistics), R is the buffers' row stride, and policy_grad_combine_kernel reads the partials as it always has.
inline size_t policy_grad_bf16_layout(PolShape S, int n, char* ws, const PolicyParams& P, float* grad, float* stats, GradTileArgsB* ta, GradPlan* gp) {
  static_assert(kGradSlice % 32 == 0 && kPolGradBM == 32, "Bp is a multiple of the tile and of the wgrad kernel's 32-row k-block");
  const size_t Bp = ((size_t)n + kPolGradBM - 1) / kPolGradBM * kPolGradBM;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* at = ws ? ws + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  GradTileArgsB t{};
  int save_ld[POL_SV_COUNT] = {};
  for (int l = 0; l < POL_L_WEIGHTS; ++l) save_ld[pol_layer(l, S).x] = pol_layer(l, S).K;
  for (int sv = 0; sv < POL_SV_COUNT; ++sv) t.save[sv] = reinterpret_cast<__bf16*>(take(Bp * pol_sv_pos(sv) * save_ld[sv] * 2));
  for (int l = 0; l < POL_L_WEIGHTS; ++l) t.dz[l] = reinterpret_cast<__bf16*>(take(Bp * pol_layer(l, S).pos * pol_layer(l, S).N * 2));
  t.dls = reinterpret_cast<float*>(take(Bp * 16));
  t.st = reinterpret_cast<float*>(take(Bp * 16));
  t.Bp = (int)Bp;

  const float *dz[kGradLayers], *x[kGradLayers];
  for (int l = 0; l < kGradLayers; ++l) {
    dz[l] = l < POL_L_WEIGHTS ? reinterpret_cast<const float*>(t.dz[l]) : (l == POL_L_LOGSTD ? t.dls : t.st);
    x[l] = l < POL_L_WEIGHTS ? reinterpret_cast<const float*>(t.save[pol_layer(l, S).x]) : nullptr;
  }
  const GradPlan g = policy_grad_plan(S, Bp, dz, x, take, grad, stats, P, n);
  if (ta) *ta = t;
  if (gp) *gp = g;
  return off;
}

// dW = dZ^T [X | 1] of one 64 x 64 output tile over one slice of kGradSlice reduction rows: four waves of 32 x 32, each 2 x 2 MFMA
// tiles.  A k-block is 32 reduction rows: lane (r, h) loads rows r0 + 8 h .. + 7 of column n0 + r of dZ^T (A) and of column c0 + r
// of X^T (B), 16 bytes each, straight from global memory.  Column K of [X | 1] is bf16 1.0; a column past N or past K is zero.
__global__ __launch_bounds__(256) void policy_wgrad_bf16_kernel(GradPlan g) {
  __shared__ float4 red[256];
  const GradLayer L = grad_layer_of(g, (int)blockIdx.x, [](const GradLayer& l) { return l.wg0; });
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4;
  const int local = (int)blockIdx.x - L.wg0, per_slice = L.ntiles * L.ktiles;
  const int slice = local / per_slice, nt = (local % per_slice) / L.ktiles, kt = local % L.ktiles;
  const int s0 = slice * kGradSlice, s1 = min(s0 + kGradSlice, L.R);
  if (L.K == 0) {   // log_std, the statistics: fp32 [R][4] per-row terms; a fixed order: strided per thread, then a tree
    const float4* rows = reinterpret_cast<const float4*>(L.dz);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = s0 + tid; i < s1; i += 256) { const float4 v = rows[i]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) { const float4 a = red[tid], b = red[tid + o]; red[tid] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
      __syncthreads();
    }
    if (tid == 0) { const float4 v = red[0]; float* p = L.part + (size_t)slice * 4; p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
    return;
  }
  const __bf16* dz = reinterpret_cast<const __bf16*>(L.dz);
  const __bf16* x = reinterpret_cast<const __bf16*>(L.x);
  const int n0 = nt * kGradTile + (wave >> 1) * 32, c0 = kt * kGradTile + (wave & 1) * 32, KC = L.K + 1;
  if (n0 >= L.N || c0 >= KC) return;            // the wave's 32 x 32 lies outside the layer
  const __bf16 one = (__bf16)1.f, zero = (__bf16)0.f;
  const __bf16* pa[2];
  const __bf16* pb[2];
  bool va[2], vb[2], ones[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = n0 + i * 16 + r, k = c0 + i * 16 + r;
    va[i] = n < L.N; vb[i] = k < L.K; ones[i] = k == L.K;
    pa[i] = dz + (size_t)min(n, L.N - 1) * L.R + 8 * h;
    pb[i] = x + (size_t)min(k, L.K - 1) * L.R + 8 * h;
  }
  pol_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = pol_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int r0 = s0; r0 < s1; r0 += 32) {
    pol_bf16x8 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i] = *reinterpret_cast<const pol_bf16x8*>(pa[i] + r0);
      b[i] = *reinterpret_cast<const pol_bf16x8*>(pb[i] + r0);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[i][e] = va[i] ? a[i][e] : zero;
        b[i][e] = vb[i] ? b[i][e] : (ones[i] ? one : zero);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
  // acc[i][j][v]: output row n (A's column of dZ^T) = n0 + i * 16 + 4 h + v, column (B's) = c0 + j * 16 + r
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int n = n0 + i * 16 + 4 * h + v, k = c0 + j * 16 + r;
        if (n < L.N && k < KC) L.part[((size_t)slice * L.N + n) * KC + k] = acc[i][j][v];
      }
}

}  // namespace te
