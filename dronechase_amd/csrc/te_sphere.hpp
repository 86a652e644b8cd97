// te_sphere.hpp — the two convolution blocks of the level5 student's sphere CNN (dronechase_amd/student.py, SphereCNN.block1 / block2)
// for every sphere of the stacked observation that the network looks at, in one launch (te_sphere_encode, include/threatengage.h).
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

template <int C>
__global__ __launch_bounds__(kSphThreads) void sphere_encode_kernel(SphereIO io) {
  extern __shared__ __attribute__((aligned(16))) float sph_lds[];
  constexpr SphLds L = sph_lds_plan(C);
  constexpr SphParams P = sph_layout(C);
  constexpr int K1 = sph_k1(C), K1P = sph_k1p(C), W1S = sph_w1s(C);
  constexpr int kCells = C * kSphH * kSphInW;                        // IN's body: every cell below the 1.0 rows, the wrap included
  constexpr int kPerThread = (kCells + kSphThreads - 1) / kSphThreads;
  float* IN = sph_lds + L.in;
  float* P1 = sph_lds + L.p1;
  float* W1 = sph_lds + L.w1;
  float* W2 = sph_lds + L.w2;
  float* B = sph_lds + L.bias;
  int* OFF1 = reinterpret_cast<int*>(sph_lds + L.off1);
  int* OFF2 = reinterpret_cast<int*>(sph_lds + L.off2);
  const float* __restrict__ prm = io.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4, stride = gridDim.x;

  // ---- once per workgroup: weights, biases, tap offsets, the constant 1.0 rows of both padded tiles
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

  // body cell t of IN <- the sphere's cell, the column taken modulo the width
  float cell[kPerThread];
  auto load = [&](int i) {
    const float* __restrict__ s = io.stacked + (size_t)i * (C * kSphH * kSphW);
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int t = tid + j * kSphThreads;
      if (t < kCells) {
        const int row = t / kSphInW, col = t % kSphInW;      // row = c * 13 + y
        cell[j] = s[row * kSphW + (col + kSphW - 2) % kSphW];
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const int t = tid + j * kSphThreads;
      if (t < kCells) {
        const int row = t / kSphInW, col = t % kSphInW, c = row / kSphH, y = row % kSphH;
        IN[(c * kSphInH + 2 + y) * kSphInW + col] = cell[j];
      }
    }
  };

  int i = sph_next(io, blockIdx.x, stride);
  if (i < io.total) { load(i); stage(); }
  __syncthreads();
  while (i < io.total) {
    // ---- block1: 6 x 2 tiles over the 8 waves; rows 91 .. 95 of the last tile compute position 90 again and are dropped
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
    __syncthreads();
    // ---- the next sphere of this workgroup: zeros for those that do not count, then the loads of the one that does
    const int next = sph_next(io, i + stride, stride);
    if (next < io.total) load(next);
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
    if (next < io.total) stage();     // IN is dead since the barrier above
    __syncthreads();
    i = next;
  }
}

}  // namespace te
