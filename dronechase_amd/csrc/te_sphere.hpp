// te_sphere.hpp — the two convolution blocks of the level5 student's sphere CNN (dronechase_amd/student.py, SphereCNN.block1 / block2)
// for every sphere of the stacked observation that the network looks at, in one launch (te_sphere_encode, include/threatengage.h), and
// the gradient of their four parameter tensors (te_sphere_encode_grad; the second half of this file).
//
//   sphere_encode_kernel  persistent 512-thread workgroups (8 waves), one per CU at most: a workgroup stages both layers' weights into
//                         LDS once, then takes spheres blockIdx.x, blockIdx.x + gridDim.x, ...  A sphere that does not count (its mask
//                         byte is 0, unless it is sphere 0 of a row whose mask is all zero) gets 1792 zeros and its input is never read.
//
// Per counting sphere [3][13][26]:
//   staging  the input into LDS as it is padded: circular by 2 in W, constant 1.0 by 2 in H -> IN [3][17][30].  The 1.0 rows are written
//            once per workgroup; no padded copy exists in global memory.
//   block1   conv 5x5 stride 2 + ReLU as a GEMM on v_mfma_f32_16x16x4_f32: M = the 91 output positions (7 x 13; six 16-row tiles),
//            N = 32 channels (two tiles), K = 75 = ci * 25 + kh * 5 + kw, zero-padded to 80.  The A operand is gathered from IN
//            (position's corner + the tap's offset, from a table in LDS).  The output lands in LDS padded for block2: circular by 1
//            in W, constant 1.0 by 1 in H -> P1 [32][9][15].
//   block2   conv 3x3 stride 2 + ReLU: M = 28 positions (4 x 7; two tiles), N = 64 (four tiles), K = 288 = ci * 9 + kh * 3 + kw; one
//            (M tile, N tile) per wave.  A lane's four results are four consecutive positions of one channel: one 16-byte store into
//            the flatten order (co, oh, ow).
//   The next counting sphere's input is loaded into registers before block2 and stored to LDS after it.
//
// LDS (sph_lds_plan): IN 6 KB, P1 17 KB, conv1 weights [32][80 + 4] 10.5 KB, conv2 weights [64][288 + 4] 73 KB, biases, the two
// offset tables: 108.2 KB, one workgroup per CU.  Weight rows are padded by 4 floats so that the 16 rows a 16-lane group reads start
// in 16 different 16-byte slots.
//
// Numerics: fp32 throughout, the accumulator starts from the bias.  A k-block of 16 is consumed as 4 MFMAs whose k index is strided by
// 4, as in te_policy.hpp's pol_gemm.  The sum order of an output element is over k only: it does not depend on the sphere's row, its
// slot, n_rows, the grid or the mask of any other sphere, so a sphere's features are bitwise the same wherever it is placed.
#pragma once

namespace te {

constexpr int kSphThreads = 512;                 // 8 waves
constexpr int kSphH = 13, kSphW = 26;            // a sphere's cells
constexpr int kSphC1 = 32, kSphC2 = 64;          // channels of block1 and block2
constexpr int kSphH1 = 7, kSphW1 = 13;           // block1's output
constexpr int kSphH2 = 4, kSphW2 = 7;            // block2's output
constexpr int kSphOut = kSphC2 * kSphH2 * kSphW2;   // 1792 features of a sphere
constexpr int kSphInH = kSphH + 4, kSphInW = kSphW + 4;       // IN rows and columns (padding 2)
constexpr int kSphP1H = kSphH1 + 2, kSphP1W = kSphW1 + 2;     // P1 rows and columns (padding 1)
constexpr int kSphK2 = kSphC1 * 9;               // 288
constexpr int kSphW2S = kSphK2 + 4;              // LDS row stride of conv2's weights
constexpr int kSphMaxSpheres = 8;

__host__ __device__ constexpr int sph_k1(int C) { return C * 25; }
__host__ __device__ constexpr int sph_k1p(int C) { return (sph_k1(C) + 15) / 16 * 16; }   // zero-padded: whole k-blocks of 16
__host__ __device__ constexpr int sph_w1s(int C) { return sph_k1p(C) + 4; }

// Float offsets of the four tensors in the parameter buffer (the public layout of threatengage.h): the reference's tensors, flattened.
struct SphParams { int w1, b1, w2, b2, words; };
__host__ __device__ constexpr SphParams sph_layout(int C) {
  const int w1 = 0, b1 = w1 + kSphC1 * sph_k1(C), w2 = b1 + kSphC1, b2 = w2 + kSphC2 * kSphK2;
  return {w1, b1, w2, b2, b2 + kSphC2};
}
static_assert(sph_layout(3).b1 % 4 == 0 && sph_layout(3).w2 % 4 == 0 && sph_layout(3).b2 % 4 == 0, "16-byte loads of every tensor");

// The LDS map in 4-byte words from the start of the dynamic LDS; every region starts on a 16-byte boundary.
struct SphLds { int in, p1, w1, w2, bias, off1, off2, words; };
__host__ __device__ constexpr SphLds sph_lds_plan(int C) {
  const int in = 0, p1 = in + (C * kSphInH * kSphInW + 3) / 4 * 4, w1 = p1 + kSphC1 * kSphP1H * kSphP1W, w2 = w1 + kSphC1 * sph_w1s(C),
            bias = w2 + kSphC2 * kSphW2S, off1 = bias + kSphC1 + kSphC2, off2 = off1 + sph_k1p(C);
  return {in, p1, w1, w2, bias, off1, off2, off2 + kSphK2};
}
static_assert(sph_lds_plan(3).words * 4 <= 160 * 1024, "fits the LDS of a gfx950 CU");
static_assert(sph_lds_plan(3).p1 % 4 == 0 && sph_lds_plan(3).w1 % 4 == 0 && sph_lds_plan(3).w2 % 4 == 0 && sph_lds_plan(3).off1 % 4 == 0 &&
              sph_lds_plan(3).off2 % 4 == 0, "float4 / int4 reads of the weights and the tables");

struct SphereIO {
  const float* params;
  const float* stacked;     // [n_rows][n_spheres][C][13][26]
  const uint8_t* mask;      // [n_rows][n_spheres] or NULL
  float* out;               // [n_rows][n_spheres][1792]
  int n_spheres, total;     // total = n_rows * n_spheres
};

typedef float sph_f32x4 __attribute__((ext_vector_type(4)));

TE_DEV sph_f32x4 sph_mfma4(float a0, float a1, float a2, float a3, float4 b, sph_f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b.w, acc, 0, 0, 0);
  return acc;
}

// One 16 x 16 output tile of a convolution as a GEMM over K (a multiple of 16): the lane's A row is the position whose window starts at
// X + corner; off[k] is tap k's offset from that corner, W + k the lane's weight row (column n of B).  Lane (r, h) = (lane & 15,
// lane >> 4) holds k0 + 4h .. k0 + 4h + 3 of a k-block; the result is column r, rows 4h .. 4h + 3.
template <int K>
TE_DEV sph_f32x4 sph_tile(const float* X, int corner, const int* off, const float* W, float bias, int h) {
  sph_f32x4 acc{bias, bias, bias, bias};
  const float* x = X + corner;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int k = k0 + 4 * h;
    const int4 o = *reinterpret_cast<const int4*>(off + k);
    const float4 w = *reinterpret_cast<const float4*>(W + k);
    acc = sph_mfma4(x[o.x], x[o.y], x[o.z], x[o.w], w, acc);
  }
  return acc;
}

// Does sphere i (row i / n_spheres, slot i % n_spheres) count?  mask NULL: every sphere does.
TE_DEV bool sph_counts(const uint8_t* __restrict__ mask, int n_spheres, int i) {
  if (!mask) return true;
  if (mask[i]) return true;
  const int s = i % n_spheres;
  if (s != 0) return false;
  int any = 0;
  for (int j = 1; j < n_spheres; ++j) any |= mask[i + j];
  return any == 0;
}

// The first counting sphere among i, i + stride, ... (or a value >= total); the ones passed over get their zeros.  Uniform over the workgroup.
TE_DEV int sph_next(const SphereIO& io, int i, int stride) {
  for (; i < io.total; i += stride) {
    if (sph_counts(io.mask, io.n_spheres, i)) return i;
    float4* o = reinterpret_cast<float4*>(io.out + (size_t)i * kSphOut);
    for (int t = threadIdx.x; t < kSphOut / 4; t += kSphThreads) o[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  return i;
}

// The per-workgroup setup, the staging of a sphere and block1 are functions because sphere_encode_grad_kernel (below) builds the same
// LDS image and recomputes block1 on it: one text, so Y1 in the backward is bitwise the forward's.
// Once per workgroup: both layers' weights, the biases, the tap offsets and the constant 1.0 rows of both padded tiles, into the LDS of
// sph_lds_plan(C) at `lds`.
template <int C>
TE_DEV void sph_setup(float* lds, const float* __restrict__ prm) {
  constexpr SphLds L = sph_lds_plan(C);
  constexpr SphParams P = sph_layout(C);
  constexpr int K1 = sph_k1(C), K1P = sph_k1p(C), W1S = sph_w1s(C);
  float* IN = lds + L.in;
  float* P1 = lds + L.p1;
  float* W1 = lds + L.w1;
  float* W2 = lds + L.w2;
  float* B = lds + L.bias;
  int* OFF1 = reinterpret_cast<int*>(lds + L.off1);
  int* OFF2 = reinterpret_cast<int*>(lds + L.off2);
  const int tid = threadIdx.x;
  for (int t = tid; t < kSphC1 * W1S; t += kSphThreads) {
    const int n = t / W1S, k = t % W1S;
    W1[t] = k < K1 ? prm[P.w1 + n * K1 + k] : 0.f;
  }
  for (int t = tid; t < kSphC2 * (kSphK2 / 4); t += kSphThreads) {
    const int n = t / (kSphK2 / 4), k = (t % (kSphK2 / 4)) * 4;
    *reinterpret_cast<float4*>(W2 + n * kSphW2S + k) = *reinterpret_cast<const float4*>(prm + P.w2 + n * kSphK2 + k);
  }
  for (int t = tid; t < kSphC1 + kSphC2; t += kSphThreads) B[t] = t < kSphC1 ? prm[P.b1 + t] : prm[P.b2 + t - kSphC1];
  for (int k = tid; k < K1P; k += kSphThreads)   // a padded tap reads the corner itself, against a zero weight
    OFF1[k] = k < K1 ? (k / 25) * (kSphInH * kSphInW) + (k % 25 / 5) * kSphInW + k % 5 : 0;
  for (int k = tid; k < kSphK2; k += kSphThreads) OFF2[k] = (k / 9) * (kSphP1H * kSphP1W) + (k % 9 / 3) * kSphP1W + k % 3;
  for (int t = tid; t < C * 4 * kSphInW; t += kSphThreads) {
    const int c = t / (4 * kSphInW), q = t % (4 * kSphInW) / kSphInW, col = t % kSphInW;
    IN[(c * kSphInH + (q < 2 ? q : kSphH + q)) * kSphInW + col] = 1.f;
  }
  for (int t = tid; t < kSphC1 * 2 * kSphP1W; t += kSphThreads) {
    const int c = t / (2 * kSphP1W), q = t % (2 * kSphP1W) / kSphP1W, col = t % kSphP1W;
    P1[(c * kSphP1H + (q ? kSphP1H - 1 : 0)) * kSphP1W + col] = 1.f;
  }
}

// IN's body: every cell below the 1.0 rows, the wrap included; a thread holds sph_cells_per_thread(C) of them between load and stage.
__host__ __device__ constexpr int sph_cells(int C) { return C * kSphH * kSphInW; }
__host__ __device__ constexpr int sph_cells_per_thread(int C) { return (sph_cells(C) + kSphThreads - 1) / kSphThreads; }

// body cell t of IN <- sphere i's cell, the column taken modulo the width: global memory -> registers ...
template <int C>
TE_DEV void sph_load(const float* __restrict__ stacked, int i, float (&cell)[sph_cells_per_thread(C)]) {
  const float* __restrict__ s = stacked + (size_t)i * (C * kSphH * kSphW);
#pragma unroll
  for (int j = 0; j < sph_cells_per_thread(C); ++j) {
    const int t = threadIdx.x + j * kSphThreads;
    if (t < sph_cells(C)) {
      const int row = t / kSphInW, col = t % kSphInW;      // row = c * 13 + y
      cell[j] = s[row * kSphW + (col + kSphW - 2) % kSphW];
    }
  }
}

// ... and registers -> LDS
template <int C>
TE_DEV void sph_stage(float* IN, const float (&cell)[sph_cells_per_thread(C)]) {
#pragma unroll
  for (int j = 0; j < sph_cells_per_thread(C); ++j) {
    const int t = threadIdx.x + j * kSphThreads;
    if (t < sph_cells(C)) {
      const int row = t / kSphInW, col = t % kSphInW, c = row / kSphH, y = row % kSphH;
      IN[(c * kSphInH + 2 + y) * kSphInW + col] = cell[j];
    }
  }
}

// block1 of the sphere staged in IN, into P1 (padded for block2, as the forward leaves it): 6 x 2 tiles over the 8 waves; rows 91 .. 95
// of the last tile compute position 90 again and are dropped.  The caller puts a barrier behind it.
template <int C>
TE_DEV void sph_block1(const float* IN, float* P1, const int* OFF1, const float* W1, const float* B) {
  constexpr int K1P = sph_k1p(C), W1S = sph_w1s(C);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
  for (int t = wave; t < 12; t += kSphThreads / 64) {
    const int mt = t >> 1, n = (t & 1) * 16 + r;
    const int m = min(mt * 16 + r, kSphH1 * kSphW1 - 1);
    const sph_f32x4 acc = sph_tile<K1P>(IN, (2 * (m / kSphW1)) * kSphInW + 2 * (m % kSphW1), OFF1, W1 + n * W1S, B[n], h);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int mo = mt * 16 + 4 * h + v;
      if (mo < kSphH1 * kSphW1) {
        const int oh = mo / kSphW1, ow = mo % kSphW1;
        float* row = P1 + (n * kSphP1H + 1 + oh) * kSphP1W;
        const float y = fmaxf(acc[v], 0.f);
        row[1 + ow] = y;
        if (ow == kSphW1 - 1) row[0] = y;                 // the circular padding of block2
        if (ow == 0) row[kSphP1W - 1] = y;
      }
    }
  }
}

template <int C>
__global__ __launch_bounds__(kSphThreads) void sphere_encode_kernel(SphereIO io) {
  extern __shared__ __attribute__((aligned(16))) float sph_lds[];
  constexpr SphLds L = sph_lds_plan(C);
  float* IN = sph_lds + L.in;
  float* P1 = sph_lds + L.p1;
  float* W1 = sph_lds + L.w1;
  float* W2 = sph_lds + L.w2;
  float* B = sph_lds + L.bias;
  int* OFF1 = reinterpret_cast<int*>(sph_lds + L.off1);
  int* OFF2 = reinterpret_cast<int*>(sph_lds + L.off2);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4, stride = gridDim.x;

  sph_setup<C>(sph_lds, io.params);
  float cell[sph_cells_per_thread(C)];
  int i = sph_next(io, blockIdx.x, stride);
  if (i < io.total) { sph_load<C>(io.stacked, i, cell); sph_stage<C>(IN, cell); }
  __syncthreads();
  while (i < io.total) {
    sph_block1<C>(IN, P1, OFF1, W1, B);
    __syncthreads();
    // ---- the next sphere of this workgroup: zeros for those that do not count, then the loads of the one that does
    const int next = sph_next(io, i + stride, stride);
    if (next < io.total) sph_load<C>(io.stacked, next, cell);
    // ---- block2: wave -> (M tile, N tile); rows 28 .. 31 compute position 27 again and are dropped
    {
      const int mt = wave >> 2, n = (wave & 3) * 16 + r;
      const int m = min(mt * 16 + r, kSphH2 * kSphW2 - 1);
      const sph_f32x4 acc = sph_tile<kSphK2>(P1, (2 * (m / kSphW2)) * kSphP1W + 2 * (m % kSphW2), OFF2, W2 + n * kSphW2S, B[kSphC1 + n], h);
      const int mo = mt * 16 + 4 * h;
      if (mo < kSphH2 * kSphW2)
        *reinterpret_cast<float4*>(io.out + (size_t)i * kSphOut + n * (kSphH2 * kSphW2) + mo) =
            make_float4(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    }
    if (next < io.total) sph_stage<C>(IN, cell);     // IN is dead since the barrier above
    __syncthreads();
    i = next;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// te_sphere_encode_grad: the gradient of the packed parameters (sph_layout) from the upstream gradient of te_sphere_encode's output.
//
//   sphere_encode_grad_kernel  the forward's grid and sphere order (persistent 512-thread workgroups, spheres blockIdx.x, + gridDim.x,
//                              ..., the same sph_counts rule).  A workgroup keeps its share of dW2, dW1, db2 and db1 in registers
//                              across all its spheres and writes it once, as partial gradient blockIdx.x of the workspace.
//   sphere_grad_reduce_kernel  grad[j] = the partials' element j summed in workgroup order.  grad is overwritten.
//
// Per counting sphere (G = its 1792 upstream values, out = what te_sphere_encode wrote for it):
//   block1   recomputed into P1 by sph_block1, the forward's own code on the forward's own LDS image: Y1 is bitwise the forward's
//            and never goes to global memory.
//   dZ2      = G * [out > 0] -> DZ [64][28, zero-padded to 32], row stride 36.
//   dW2      += im2col(P1)^T dZ2 as a GEMM: M = 288 taps (18 tiles) x N = 64 (4 tiles), K = 32 positions.  A wave owns one channel
//            tile and nine tap tiles (36 accumulator VGPRs); its B operand (dZ2) is read once per sphere.
//   columns  COL[pos][tap] = sum_m dZ2[m][pos] W2[m][tap]: M = 28 positions (2 tiles) x N = 288 (18 tiles), K = 64; 36 tiles over the
//            8 waves.  No barrier between this and dW2: both only read DZ.
//   dZ1      every cell of Y1 gathers its at most four contributions of COL in a fixed order (kh, then kw, ascending), adds the
//            column the circular padding copied it to (column 12 -> padded column 0, column 0 -> padded column 14), is masked
//            by [Y1 > 0] and is written over Y1 in P1.  The 1.0 rows of P1 take no gradient.  No float atomics.
//   dW1      += im2col(IN)^T dZ1: M = 75 taps padded to 80 (5 tiles) x N = 32 (2 tiles), K = 91 positions padded to 96 with zero
//            dZ1; ten tiles: one per wave, a second one for waves 0 and 1.
//   db2, db1 one thread per channel (wave 7; lanes 0 .. 31 of wave 6) sums the sphere's dZ2 / dZ1 in position order and adds the sum
//            to its running total.
//
// LDS (sph_grad_lds_plan): the forward's plan, then DZ 9 KB and COL [28][289] 31.6 KB: 148.8 KB of the CU's 160.  dZ1 lives in P1.
// Every sum has a fixed order that depends on the inputs, the grid (min(n_rows * n_spheres, CUs, kSphGradMaxGroups)) and nothing
// else: the same call on the same device gives the same bits.  A sphere that does not count is passed over: nothing of it is read.
constexpr int kSphDzS = 36;                      // LDS row stride of DZ: 28 positions, 4 zeros, 4 words that spread the rows over banks
constexpr int kSphColS = kSphK2 + 1;             // LDS row stride of COL (odd: the gather's rows start in different banks)
constexpr int kSphGradMaxGroups = 256;           // partial gradients in the workspace, at most (one per CU of an MI355X)

struct SphGradLds { int dz, col, words; };       // behind the forward's regions, which keep their offsets
__host__ __device__ constexpr SphGradLds sph_grad_lds_plan(int C) {
  const int dz = sph_lds_plan(C).words, col = dz + kSphC2 * kSphDzS;
  return {dz, col, col + (kSphH2 * kSphW2 * kSphColS + 3) / 4 * 4};
}
static_assert(sph_grad_lds_plan(3).words * 4 <= 160 * 1024, "fits the LDS of a gfx950 CU");
static_assert(sph_grad_lds_plan(3).dz % 4 == 0 && kSphDzS % 4 == 0, "float4 accesses of DZ");
static_assert(sph_layout(3).words % 4 == 0, "a partial gradient starts on a 16-byte boundary");

struct SphereGradIO {
  const float* params;
  const float* stacked;     // [n_rows][n_spheres][C][13][26]
  const uint8_t* mask;      // [n_rows][n_spheres] or NULL
  const float* out;         // [n_rows][n_spheres][1792], te_sphere_encode's
  const float* d_out;       // [n_rows][n_spheres][1792]
  float* partial;           // [gridDim.x][sph_layout(C).words]
  int n_spheres, total;
};

// The first counting sphere among i, i + stride, ... (or a value >= total).  Uniform over the workgroup.
TE_DEV int sph_next_counting(const uint8_t* __restrict__ mask, int n_spheres, int total, int i, int stride) {
  while (i < total && !sph_counts(mask, n_spheres, i)) i += stride;
  return i;
}

// dP1[n][y][x] from the column matrix (col = COL + n * 9): the windows (ph, pw) of block2 that cover the cell, tap (kh, kw) =
// (y - 2 ph, x - 2 pw), summed in the order kh, kw ascending.
TE_DEV float sph_dp1(const float* col, int y, int x) {
  float s = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ph = (y - kh) >> 1;
    if (((y - kh) & 1) || ph < 0 || ph >= kSphH2) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int pw = (x - kw) >> 1;
      if (((x - kw) & 1) || pw < 0 || pw >= kSphW2) continue;
      s += col[(ph * kSphW2 + pw) * kSphColS + kh * 3 + kw];
    }
  }
  return s;
}

// One 16 x 16 tile of dW1 += im2col(IN)^T dZ1 over the 96 (91) positions: rows = taps tt * 16 .. + 15, columns = channels.
TE_DEV sph_f32x4 sph_dw1_tile(const float* IN, const float* P1, const int* OFF1, int t, int r, int h, sph_f32x4 acc) {
  constexpr int kPos = kSphH1 * kSphW1;
  const float* x = IN + OFF1[(t >> 1) * 16 + r];
  const float* z = P1 + ((t & 1) * 16 + r) * (kSphP1H * kSphP1W);
#pragma unroll 2
  for (int k0 = 0; k0 < (kPos + 15) / 16 * 16; k0 += 16) {
    float a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = k0 + 4 * h + j, pc = min(p, kPos - 1), oh = pc / kSphW1, ow = pc % kSphW1;
      a[j] = x[2 * oh * kSphInW + 2 * ow];
      b[j] = p < kPos ? z[(1 + oh) * kSphP1W + 1 + ow] : 0.f;
    }
    acc = sph_mfma4(a[0], a[1], a[2], a[3], make_float4(b[0], b[1], b[2], b[3]), acc);
  }
  return acc;
}

template <int C>
__global__ __launch_bounds__(kSphThreads) void sphere_encode_grad_kernel(SphereGradIO io) {
  extern __shared__ __attribute__((aligned(16))) float sph_lds[];
  constexpr SphLds L = sph_lds_plan(C);
  constexpr SphGradLds G = sph_grad_lds_plan(C);
  constexpr SphParams P = sph_layout(C);
  constexpr int K1 = sph_k1(C), kPos1 = kSphH1 * kSphW1, kPos2 = kSphH2 * kSphW2;
  static_assert(sph_k1p(C) == 80 && kSphK2 == 288 && kSphC2 == 64 && kSphC1 == 32 && kPos2 <= 32, "the tile counts below");
  float* IN = sph_lds + L.in;
  float* P1 = sph_lds + L.p1;
  const float* W1 = sph_lds + L.w1;
  const float* W2 = sph_lds + L.w2;
  const float* B = sph_lds + L.bias;
  const int* OFF1 = reinterpret_cast<const int*>(sph_lds + L.off1);
  const int* OFF2 = reinterpret_cast<const int*>(sph_lds + L.off2);
  float* DZ = sph_lds + G.dz;
  float* COL = sph_lds + G.col;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4, stride = gridDim.x;

  sph_setup<C>(sph_lds, io.params);
  if (tid < kSphC2 * 4) DZ[(tid >> 2) * kSphDzS + kPos2 + (tid & 3)] = 0.f;    // positions 28 .. 31, once

  // dW2: channel tile nt2, tap tiles tt2, tt2 + 2, ..., tt2 + 16.  The lane's two k-blocks of positions and their window corners in P1;
  // a position past 27 reads position 27 against a zero dZ2.
  const int nt2 = wave & 3, tt2 = wave >> 2;
  int corner[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = min((j >> 2) * 16 + 4 * h + (j & 3), kPos2 - 1);
    corner[j] = 2 * (p / kSphW2) * kSphP1W + 2 * (p % kSphW2);
  }
  sph_f32x4 dw2[9], dw1[2];
#pragma unroll
  for (int j = 0; j < 9; ++j) dw2[j] = sph_f32x4{0.f, 0.f, 0.f, 0.f};
  dw1[0] = dw1[1] = sph_f32x4{0.f, 0.f, 0.f, 0.f};
  float db = 0.f;                                  // wave 7: db2[lane]; wave 6, lanes 0 .. 31: db1[lane]

  float cell[sph_cells_per_thread(C)];
  int i = sph_next_counting(io.mask, io.n_spheres, io.total, blockIdx.x, stride);
  if (i < io.total) { sph_load<C>(io.stacked, i, cell); sph_stage<C>(IN, cell); }
  __syncthreads();
  while (i < io.total) {
    // ---- dZ2 = G * [out > 0], four positions of one channel per thread; block1 again
    if (tid < kSphC2 * (kPos2 / 4)) {
      const int m = tid / (kPos2 / 4), q = tid % (kPos2 / 4) * 4;
      const size_t at = (size_t)i * kSphOut + m * kPos2 + q;
      const float4 g = *reinterpret_cast<const float4*>(io.d_out + at), o = *reinterpret_cast<const float4*>(io.out + at);
      *reinterpret_cast<float4*>(DZ + m * kSphDzS + q) =
          make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f);
    }
    sph_block1<C>(IN, P1, OFF1, W1, B);
    __syncthreads();
    const int next = sph_next_counting(io.mask, io.n_spheres, io.total, i + stride, stride);
    if (next < io.total) sph_load<C>(io.stacked, next, cell);
    // ---- dW2
    {
      const float* dz = DZ + (nt2 * 16 + r) * kSphDzS + 4 * h;
      const float4 b0 = *reinterpret_cast<const float4*>(dz), b1 = *reinterpret_cast<const float4*>(dz + 16);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const float* x = P1 + OFF2[(tt2 + 2 * j) * 16 + r];
        dw2[j] = sph_mfma4(x[corner[0]], x[corner[1]], x[corner[2]], x[corner[3]], b0, dw2[j]);
        dw2[j] = sph_mfma4(x[corner[4]], x[corner[5]], x[corner[6]], x[corner[7]], b1, dw2[j]);
      }
    }
    // ---- the column matrix: rows 28 .. 31 of the second position tile compute position 27 again and are dropped
    for (int t = wave; t < 36; t += kSphThreads / 64) {
      const int mt = t / 18, tap = t % 18 * 16 + r;
      const float* a = DZ + min(mt * 16 + r, kPos2 - 1);
      const float* w = W2 + tap;
      sph_f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k0 = 0; k0 < kSphC2; k0 += 16) {
        const float* am = a + (k0 + 4 * h) * kSphDzS;
        const float* wm = w + (k0 + 4 * h) * kSphW2S;
        acc = sph_mfma4(am[0], am[kSphDzS], am[2 * kSphDzS], am[3 * kSphDzS], make_float4(wm[0], wm[kSphW2S], wm[2 * kSphW2S], wm[3 * kSphW2S]), acc);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int po = mt * 16 + 4 * h + v;
        if (po < kPos2) COL[po * kSphColS + tap] = acc[v];
      }
    }
    if (wave == 7) {
      float s = 0.f;
      for (int p = 0; p < kPos2; ++p) s += DZ[lane * kSphDzS + p];
      db += s;
    }
    __syncthreads();
    // ---- dZ1 over Y1, in place
    for (int t = tid; t < kSphC1 * kPos1; t += kSphThreads) {
      const int n = t / kPos1, q = t % kPos1, oh = q / kSphW1, ow = q % kSphW1;
      const float* col = COL + n * 9;
      float d = sph_dp1(col, 1 + oh, 1 + ow);
      if (ow == kSphW1 - 1) d += sph_dp1(col, 1 + oh, 0);
      if (ow == 0) d += sph_dp1(col, 1 + oh, kSphP1W - 1);
      float* y = P1 + (n * kSphP1H + 1 + oh) * kSphP1W + 1 + ow;
      *y = *y > 0.f ? d : 0.f;
    }
    __syncthreads();
    // ---- dW1
    dw1[0] = sph_dw1_tile(IN, P1, OFF1, wave, r, h, dw1[0]);
    if (wave < 2) dw1[1] = sph_dw1_tile(IN, P1, OFF1, 8 + wave, r, h, dw1[1]);
    if (wave == 6 && lane < kSphC1) {
      float s = 0.f;
      for (int q = 0; q < kPos1; ++q) s += P1[(lane * kSphP1H + 1 + q / kSphW1) * kSphP1W + 1 + q % kSphW1];
      db += s;
    }
    __syncthreads();
    if (next < io.total) sph_stage<C>(IN, cell);
    __syncthreads();
    i = next;
  }

  // ---- this workgroup's partial gradient: every one of its words is written, by exactly one lane
  float* part = io.partial + (size_t)blockIdx.x * P.words;
#pragma unroll
  for (int j = 0; j < 9; ++j)      // rows 4h .. 4h + 3 of the tile are four consecutive taps of channel nt2 * 16 + r
    *reinterpret_cast<float4*>(part + P.w2 + (nt2 * 16 + r) * kSphK2 + (tt2 + 2 * j) * 16 + 4 * h) = make_float4(dw2[j][0], dw2[j][1], dw2[j][2], dw2[j][3]);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = s * 8 + wave;
    if (t < 10) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int tap = (t >> 1) * 16 + 4 * h + v;
        if (tap < K1) part[P.w1 + ((t & 1) * 16 + r) * K1 + tap] = dw1[s][v];
      }
    }
  }
  if (wave == 7) part[P.b2 + lane] = db;
  if (wave == 6 && lane < kSphC1) part[P.b1 + lane] = db;
}

__global__ __launch_bounds__(256) void sphere_grad_reduce_kernel(const float* __restrict__ partial, int groups, int words, float* __restrict__ grad) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= words) return;
  float s = partial[j];
  for (int g = 1; g < groups; ++g) s += partial[(size_t)g * words + j];
  grad[j] = s;
}

}  // namespace te
