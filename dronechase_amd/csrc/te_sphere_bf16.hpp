// te_sphere_bf16.hpp — te_sphere_encode_bf16: the forward of te_sphere.hpp (the level5 student's two convolution blocks, per sphere of
// the stacked observation) with bf16 operands on v_mfma_f32_16x16x32_bf16, opt-in (StudentDriver(..., encoder_precision="bf16")).
// The fp32 kernels of te_sphere.hpp are untouched; this header reuses their constants, SphereIO, sph_counts, sph_next and sph_load and
// adds a second, bf16 copy of the two conv weights.  Inference only: there is no bf16 backward.
//
// Numerics contract (the one rule; include/threatengage.h states it too, tests/_student_bf16_ref.py is its CPU form):
//   * Both conv weights are rounded ONCE to bf16, round-to-nearest-even (sphere_pack_bf16_kernel); the fp32 parameter buffer stays the
//     master copy, and both biases are read from it in fp32.
//   * A sphere's cells are rounded to bf16 (round-to-nearest-even; on gfx950 `(__bf16)x` is v_cvt_pk_bf16_f32) when they are staged into
//     LDS.  The padding constant 1.0 is exact in bf16.
//   * Products are accumulated in fp32 by the MFMA; the accumulator starts from the fp32 bias; ReLU runs in fp32.
//   * Block1's post-ReLU output is rounded to bf16 (round-to-nearest-even) when it is stored for block2.
//   * Block2's output is stored as fp32, in te_sphere_encode's buffer type and layout.
//   * The sum order of an output element is over k only: k-blocks of 32 in order, within a block the MFMA's own order.  A sphere's
//     features are therefore bitwise the same in any row, slot, batch, grid or mask of other spheres, and repeated calls are bitwise equal.
//   * A sphere that does not count (sph_counts: sphere 0 of an all-zero row counts) gets 1792 zeros and its input is never read.
//
// Packed bf16 weights (sph_bf16_layout; public, threatengage.h): ONE uint16 buffer, 16-byte aligned, two tensors [N][Kp] row-major:
//   w1 at element 0:     [32][128], k = (ci * 5 + kh) * 8 + kw: the kernel width padded from 5 to 8, so that the 8 k of a fragment are 8
//                        consecutive cells of one input row; columns with kw >= 5 and k >= 120 are zero.
//   w2 at element 4096:  [64][288], k = (kh * 3 + kw) * 32 + ci: one k-block of 32 is one tap, a fragment 8 consecutive channels.
//   22 528 elements (44 KB) in all; every row starts on a 64-byte boundary.
//
// sphere_encode_bf16_kernel: te_sphere.hpp's schedule — persistent 512-thread workgroups (8 waves) that take spheres blockIdx.x,
// blockIdx.x + gridDim.x, ..., the next counting sphere's cells prefetched into registers across both blocks; no tickets, no atomics.
//   weights  A wave's work is fixed: in block1 the channel tile wave & 1 (of 2) for position tiles wave >> 1 and, for waves 0 .. 3,
//            4 + (wave >> 1); in block2 the tile (positions wave >> 2, channels wave & 3).  Its weight fragments never change, so they
//            are loaded ONCE from the packed buffer into registers (4 + 9 fragments of 4 VGPRs = 52 VGPRs, plus 5 of bias) and never
//            go through LDS.  (The alternative, both packed tensors in LDS at 44 KB + padding, costs one more 16-byte LDS read per
//            MFMA and 46 KB; with them in registers the LDS holds only the two activation tiles.)
//   IN       [3][17][34] bf16, the sphere as it is padded (circular by 2 in W, 1.0 by 2 in H), plus 4 zero columns per row: a fragment
//            is the 8 cells from column 2 ow of one row (four aligned 4-byte reads: the start is 4-byte aligned only), it runs up to
//            column 31, and the cells past the tap's fifth meet zero weights, so they only have to be finite.  The row stride is 17
//            dwords: the 13 positions of an output row read consecutive dwords, the four input rows of a k-block are 17 apart.
//            k-rows 15 (k >= 120) read row 0 of the window against zero weights.
//   block1   D = W1 (A: 16 channels) x im2col (B: 16 positions): a lane's four results are four consecutive channels of one position:
//            one 8-byte store into P1, channels-last.  6 x 2 tiles, 4 MFMAs each.
//   P1       [9][15][40] bf16, block1's output padded for block2 (circular by 1 in W, 1.0 by 1 in H), 32 channels + 8 elements of
//            padding per cell (80 bytes = 5 slots of 16 bytes).  A block2 fragment is one 16-byte read.  Stride-2 positions are 10
//            slots apart and two output rows 150, both even: the 16 positions of a tile start in the 8 slots of one parity, two each,
//            and the k-group h adds h slots.  That 2-way conflict is what stride 2 leaves with whole slots per cell.
//   block2   D = im2col (A: 16 positions) x W2 (B: 16 channels), 9 MFMAs per wave: a lane's four results are four consecutive
//            positions of one channel: one 16-byte store into the flatten order (co, oh, ow).
// LDS: IN 3 468 B + P1 10 800 B = 14.3 KB, static.  The grid is min(spheres, 2 x CUs): two workgroups (4 waves per SIMD) share a CU,
// one in its MFMAs while the other stages or stores.
#pragma once

namespace te {

typedef __bf16 sph_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sph_bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sph_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSphBK1 = 128;                     // block1's padded K: 15 (ci, kh) rows of 8, and one zero row
constexpr int kSphBInS = 34;                     // IN's row stride in bf16 elements: 30 padded columns + 4 zeros
constexpr int kSphBInWords = 3 * kSphInH * kSphBInS;
constexpr int kSphBP1S = kSphC1 + 8;             // P1's cell stride in bf16 elements
constexpr int kSphBP1Words = kSphP1H * kSphP1W * kSphBP1S;
constexpr int kSphBGroupsPerCu = 2;

// Element offsets of the two tensors in the packed bf16 buffer
struct SphBf16 { int w1, w2, words; };
__host__ __device__ constexpr SphBf16 sph_bf16_layout() { return {0, kSphC1 * kSphBK1, kSphC1 * kSphBK1 + kSphC2 * kSphK2}; }
static_assert(sph_bf16_layout().w2 % 8 == 0 && kSphBK1 % 32 == 0 && kSphK2 % 32 == 0, "16-byte fragments, whole k-blocks");
static_assert(kSphBInS % 2 == 0 && 2 * (kSphW1 - 1) + 8 <= kSphBInS && kSphBInWords % 2 == 0, "a fragment of block1 stays in its row; 4-byte reads");
static_assert(kSphBP1S % 8 == 0, "16-byte fragments of block2");

// fp32 parameter buffer -> packed bf16 buffer: thread i writes element i (a pad column: zero)
__global__ __launch_bounds__(256) void sphere_pack_bf16_kernel(const float* __restrict__ params, __bf16* __restrict__ out) {
  constexpr SphParams P = sph_layout(3);
  constexpr SphBf16 W = sph_bf16_layout();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W.words) return;
  float v = 0.f;
  if (i < W.w2) {
    const int n = i / kSphBK1, k = i % kSphBK1, row = k / 8, kw = k % 8;     // row = ci * 5 + kh
    if (row < 15 && kw < 5) v = params[P.w1 + n * 75 + row * 5 + kw];
  } else {
    const int e = i - W.w2, n = e / kSphK2, k = e % kSphK2, tap = k / kSphC1, ci = k % kSphC1;
    v = params[P.w2 + n * kSphK2 + ci * 9 + tap];
  }
  out[i] = (__bf16)v;
}

// registers -> IN's body as bf16 (sph_load filled `cell`)
TE_DEV void sph_stage_bf16(__bf16* IN, const float (&cell)[sph_cells_per_thread(3)]) {
#pragma unroll
  for (int j = 0; j < sph_cells_per_thread(3); ++j) {
    const int t = threadIdx.x + j * kSphThreads;
    if (t < sph_cells(3)) {
      const int row = t / kSphInW, col = t % kSphInW, c = row / kSphH, y = row % kSphH;
      IN[(c * kSphInH + 2 + y) * kSphBInS + col] = (__bf16)cell[j];
    }
  }
}

template <int C>
__global__ __launch_bounds__(kSphThreads, kSphBGroupsPerCu * kSphThreads / 256) void sphere_encode_bf16_kernel(SphereIO io, const unsigned short* __restrict__ weights) {
  static_assert(C == 3, "the packed layout and IN are those of three channels");
  __shared__ __attribute__((aligned(16))) __bf16 IN[kSphBInWords];
  __shared__ __attribute__((aligned(16))) __bf16 P1[kSphBP1Words];
  constexpr SphParams P = sph_layout(C);
  constexpr SphBf16 WL = sph_bf16_layout();
  constexpr int kPos1 = kSphH1 * kSphW1, kPos2 = kSphH2 * kSphW2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4, stride = gridDim.x;

  // ---- once per workgroup: the 1.0 rows and the zero tails of both tiles (the bodies start as zeros) ...
  for (int t = tid; t < kSphBInWords; t += kSphThreads) {
    const int y = t / kSphBInS % kSphInH, col = t % kSphBInS;
    IN[t] = (__bf16)(col < kSphInW && (y < 2 || y >= kSphH + 2) ? 1.f : 0.f);
  }
  for (int t = tid; t < kSphBP1Words; t += kSphThreads) {
    const int y = t / (kSphP1W * kSphBP1S), c = t % kSphBP1S;
    P1[t] = (__bf16)(c < kSphC1 && (y == 0 || y == kSphP1H - 1) ? 1.f : 0.f);
  }
  // ---- ... and this wave's weight fragments and biases, into registers
  const __bf16* __restrict__ wb = reinterpret_cast<const __bf16*>(weights);
  const int nt1 = wave & 1, mt1 = wave >> 1, nt2 = wave & 3, mt2 = wave >> 2;
  sph_bf16x8 w1[kSphBK1 / 32], w2[kSphK2 / 32];
#pragma unroll
  for (int kb = 0; kb < kSphBK1 / 32; ++kb) w1[kb] = *reinterpret_cast<const sph_bf16x8*>(wb + WL.w1 + (nt1 * 16 + r) * kSphBK1 + kb * 32 + 8 * h);
#pragma unroll
  for (int kb = 0; kb < kSphK2 / 32; ++kb) w2[kb] = *reinterpret_cast<const sph_bf16x8*>(wb + WL.w2 + (nt2 * 16 + r) * kSphK2 + kb * 32 + 8 * h);
  const float4 b1 = *reinterpret_cast<const float4*>(io.params + P.b1 + nt1 * 16 + 4 * h);   // block1: rows 4h .. 4h + 3 are channels
  const float b2 = io.params[P.b2 + nt2 * 16 + r];                                           // block2: column r is a channel
  // block1's k-block kb, k-group h is row kb * 4 + h = ci * 5 + kh of the window; row 15 does not exist (zero weights): read row 0
  int row1[kSphBK1 / 32];
#pragma unroll
  for (int kb = 0; kb < kSphBK1 / 32; ++kb) {
    const int row = kb * 4 + h < 15 ? kb * 4 + h : 0;
    row1[kb] = ((row / 5) * kSphInH + row % 5) * (kSphBInS / 2);
  }
  // block2: the lane's position (rows 28 .. 31 compute position 27 again and are dropped) and its window's corner in P1
  const int m2 = min(mt2 * 16 + r, kPos2 - 1);
  const __bf16* a2 = P1 + ((2 * (m2 / kSphW2)) * kSphP1W + 2 * (m2 % kSphW2)) * kSphBP1S + 8 * h;

  float cell[sph_cells_per_thread(C)];
  int i = sph_next(io, blockIdx.x, stride);
  __syncthreads();                                   // the fills above, before the body is staged over them
  if (i < io.total) { sph_load<C>(io.stacked, i, cell); sph_stage_bf16(IN, cell); }
  __syncthreads();
  while (i < io.total) {
    // ---- the next sphere of this workgroup: zeros for those that do not count, then the loads of the one that does, in flight across
    // both blocks (the mask read and the loads are two global latencies in a row; behind block1 they were most of a sphere's time)
    const int next = sph_next(io, i + stride, stride);
    if (next < io.total) sph_load<C>(io.stacked, next, cell);
    // ---- block1: position tiles mt1 and, waves 0 .. 3, mt1 + 4; columns 91 .. 95 of the last tile compute position 90 again and are dropped
    for (int mt = mt1; mt < (kPos1 + 15) / 16; mt += 4) {
      const int m = min(mt * 16 + r, kPos1 - 1), oh = m / kSphW1, ow = m % kSphW1;
      const unsigned int* x = reinterpret_cast<const unsigned int*>(IN) + 2 * oh * (kSphBInS / 2) + ow;
      sph_f32x4 acc{b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int kb = 0; kb < kSphBK1 / 32; ++kb) {
        const unsigned int* q = x + row1[kb];
        const sph_u32x4 u{q[0], q[1], q[2], q[3]};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[kb], __builtin_bit_cast(sph_bf16x8, u), acc, 0, 0, 0);
      }
      if (mt * 16 + r < kPos1) {
        const sph_bf16x4 y{(__bf16)fmaxf(acc[0], 0.f), (__bf16)fmaxf(acc[1], 0.f), (__bf16)fmaxf(acc[2], 0.f), (__bf16)fmaxf(acc[3], 0.f)};
        __bf16* rowp = P1 + (1 + oh) * (kSphP1W * kSphBP1S) + nt1 * 16 + 4 * h;
        *reinterpret_cast<sph_bf16x4*>(rowp + (1 + ow) * kSphBP1S) = y;
        if (ow == kSphW1 - 1) *reinterpret_cast<sph_bf16x4*>(rowp) = y;                                  // the circular padding of block2
        if (ow == 0) *reinterpret_cast<sph_bf16x4*>(rowp + (kSphP1W - 1) * kSphBP1S) = y;
      }
    }
    __syncthreads();
    // ---- block2: k-block kb is tap (kh, kw) = (kb / 3, kb % 3), the fragment 8 channels of its cell
    {
      sph_f32x4 acc{b2, b2, b2, b2};
#pragma unroll
      for (int kb = 0; kb < kSphK2 / 32; ++kb)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const sph_bf16x8*>(a2 + ((kb / 3) * kSphP1W + kb % 3) * kSphBP1S), w2[kb], acc, 0, 0, 0);
      const int mo = mt2 * 16 + 4 * h;
      if (mo < kPos2)
        *reinterpret_cast<float4*>(io.out + (size_t)i * kSphOut + (nt2 * 16 + r) * kPos2 + mo) =
            make_float4(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    }
    if (next < io.total) sph_stage_bf16(IN, cell);   // IN is dead since the barrier above
    __syncthreads();
    i = next;
  }
}

}  // namespace te
