// te_dataset.hpp — the imitation dataset (te_dataset_*, include/threatengage.h): a ring of level5 student rows (stacked spheres, mask,
// inertial, last_action, teacher action) in caller-owned device memory, filled from te_step_students' outputs and sampled into batches
// without a host read.
//
//   dataset_scan_kernel    ONE workgroup of 16 waves.  Wave w owns the contiguous rows [w * seg, (w + 1) * seg), seg a multiple of 64.
//                          Pass 1: the wave walks its rows 64 at a time, keep = active != 0 && any mask byte != 0, and adds
//                          popcount(__ballot(keep)).  The 16 totals meet in LDS once (the kernel's only barrier), every wave sums
//                          the totals before its own, and pass 2 walks the same rows again: dst[row] = keep ? (total + base + rank)
//                          mod capacity : -1, rank = the kept lanes below this one.  Thread 0 stores total + count.  The order is that
//                          of the rows, whatever the timing: nothing waits on anything but the one barrier.
//   dataset_copy_kernel    one workgroup per source row; dst[row] < 0 leaves at once, before the row is touched.  Otherwise the row's
//                          spheres go over as float4 (6 spheres: 1 521 of them; float2 when n_spheres is odd and a row is 8 bytes
//                          off), the small fields on a few lanes next to them.
//   dataset_gather_kernel  one workgroup per output row: the slot from index[j] (clamped into the ring) or from Philox and the
//                          ring's size, the row's copy in the other direction, and kill_high_correlation's branch on last_action.
//
// A row is n_spheres * 4 056 + n_spheres + 92 bytes (24 434 at 6 spheres); byte offsets are size_t everywhere.
#pragma once

#include <cstddef>
#include <cstdint>

namespace te {

constexpr int kDsHeaderBytes = 64;       // word 0: total (i64), the rows ever appended; the rest is reserved and zero
constexpr int kDsScanWaves = 16, kDsScanThreads = kDsScanWaves * 64;
constexpr int kDsCopyThreads = 256;
constexpr int kDsSphereFloats = 3 * 13 * 26;
constexpr int kDsInertial = 15, kDsAction = 4;

inline size_t ds_align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline te_dataset_offsets dataset_offsets(const te_dataset_geom& g) {
  te_dataset_offsets o{};
  size_t at = kDsHeaderBytes;
  auto take = [&](size_t bytes) { size_t here = at; at = ds_align16(at + bytes); return here; };
  const size_t cap = (size_t)g.capacity, S = (size_t)g.n_spheres;
  o.header = 0;
  o.dst = take((size_t)g.max_append_rows * 4);
  o.stacked = take(cap * S * kDsSphereFloats * 4);
  o.mask = take(cap * S);
  o.inertial = take(cap * kDsInertial * 4);
  o.last_action = take(cap * kDsAction * 4);
  o.teacher = take(cap * kDsAction * 4);
  o.bytes = at;
  return o;
}

struct DatasetView {                     // the buffer's arrays as the kernels address them
  long long* total;
  int* dst;
  float* stacked; uint8_t* mask; float* inertial; float* last_action; float* teacher;
  int capacity, n_spheres;
};

inline DatasetView dataset_view(void* ds, const te_dataset_geom& g) {
  const te_dataset_offsets o = dataset_offsets(g);
  char* b = static_cast<char*>(ds);
  return DatasetView{reinterpret_cast<long long*>(b), reinterpret_cast<int*>(b + o.dst), reinterpret_cast<float*>(b + o.stacked),
                     reinterpret_cast<uint8_t*>(b + o.mask), reinterpret_cast<float*>(b + o.inertial), reinterpret_cast<float*>(b + o.last_action),
                     reinterpret_cast<float*>(b + o.teacher), g.capacity, g.n_spheres};
}

struct DatasetRows {                     // one side of a copy: the flat [n][...] arrays of te_step_students, or a batch
  const float* stacked; const uint8_t* mask; const float* inertial; const float* last_action; const float* teacher;
};

__device__ inline bool ds_keep(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ active, int n_spheres, long long row, int n_rows) {
  if (row >= (long long)n_rows) return false;
  if (active && active[row] == 0) return false;
  const uint8_t* m = mask + (size_t)row * (size_t)n_spheres;
  unsigned any = 0;
  for (int s = 0; s < n_spheres; ++s) any |= m[s];
  return any != 0;
}

__global__ __launch_bounds__(kDsScanThreads) void dataset_scan_kernel(DatasetView v, const uint8_t* __restrict__ mask,
                                                                      const uint8_t* __restrict__ active, int n_rows) {
  __shared__ int wave_total[kDsScanWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long total = *v.total;      // read by every thread before the barrier; thread 0 stores the new one after it
  const int blocks = (n_rows + 63) / 64;                               // blocks of 64 rows
  const long long seg = (long long)((blocks + kDsScanWaves - 1) / kDsScanWaves) * 64;
  const long long first = (long long)wave * seg;
  const long long last = first + seg < (long long)n_rows ? first + seg : (long long)n_rows;      // one past this wave's rows
  int count = 0;
  for (long long r = first; r < last; r += 64)
    count += __popcll(__ballot(ds_keep(mask, active, v.n_spheres, r + lane, n_rows)));
  if (lane == 0) wave_total[wave] = count;
  __syncthreads();
  long long base = 0, all = 0;
  for (int w = 0; w < kDsScanWaves; ++w) {
    const int c = wave_total[w];
    if (w < wave) base += c;
    all += c;
  }
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (long long r = first; r < last; r += 64) {
    const bool keep = ds_keep(mask, active, v.n_spheres, r + lane, n_rows);
    const unsigned long long kept = __ballot(keep);
    if (r + lane < (long long)n_rows)
      v.dst[r + lane] = keep ? (int)((unsigned long long)(total + base + __popcll(kept & below)) % (unsigned long long)v.capacity) : -1;
    base += __popcll(kept);
  }
  if (threadIdx.x == 0) *v.total = total + all;
}

// n floats from src to dst, both 16-byte aligned when n is a multiple of 4 and 8-byte aligned otherwise (n is even)
__device__ inline void ds_copy_floats(float* __restrict__ dst, const float* __restrict__ src, int n, bool wide) {
  if (wide) {
    const float4* s = reinterpret_cast<const float4*>(src);
    float4* d = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < n / 4; i += kDsCopyThreads) d[i] = s[i];
  } else {
    const float2* s = reinterpret_cast<const float2*>(src);
    float2* d = reinterpret_cast<float2*>(dst);
    for (int i = threadIdx.x; i < n / 2; i += kDsCopyThreads) d[i] = s[i];
  }
}

// the small fields of a row, each on lanes of its own: inertial on threads 0..14, last_action 64..67, teacher 128..131, mask 192..
__device__ inline void ds_copy_small(float* d_in, float* d_la, float* d_te, uint8_t* d_m, const float* s_in, const float* s_la,
                                     const float* s_te, const uint8_t* s_m, int n_spheres, bool copy_la) {
  const int t = threadIdx.x;
  if (t < kDsInertial) d_in[t] = s_in[t];
  else if (t >= 64 && t < 64 + kDsAction) { if (copy_la) d_la[t - 64] = s_la[t - 64]; }
  else if (t >= 128 && t < 128 + kDsAction) d_te[t - 128] = s_te[t - 128];
  else if (t >= 192 && t < 192 + n_spheres) d_m[t - 192] = s_m[t - 192];
}

__global__ __launch_bounds__(kDsCopyThreads) void dataset_copy_kernel(DatasetView v, DatasetRows in) {
  const size_t row = blockIdx.x;
  const int slot_i = v.dst[row];
  if (slot_i < 0) return;                // not kept: nothing of the row is read
  const size_t slot = (size_t)slot_i, S = (size_t)v.n_spheres, words = S * kDsSphereFloats;
  ds_copy_floats(v.stacked + slot * words, in.stacked + row * words, (int)words, (v.n_spheres & 1) == 0);
  ds_copy_small(v.inertial + slot * kDsInertial, v.last_action + slot * kDsAction, v.teacher + slot * kDsAction, v.mask + slot * S,
                in.inertial + row * kDsInertial, in.last_action + row * kDsAction, in.teacher + row * kDsAction, in.mask + row * S,
                v.n_spheres, true);
}

struct DatasetBatch {                    // te_dataset_gather's outputs and the draw
  float* stacked; uint8_t* mask; float* inertial; float* last_action; float* teacher; long long* out_index;
  const long long* index;
  uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
  int mode;
  float noise_std;
};

enum { DS_LA_KEEP = 0, DS_LA_RANDOM = 1, DS_LA_NOISE = 2 };

__device__ inline uint32_t ds_u24(uint32_t x) { return x >> 8; }

// kill_high_correlation on element k of a row's last_action: w = philox((j, draw, 2), seed)
__device__ inline float ds_last_action(float la, int k, const U4& w, int mode, float noise_std) {
  if (mode == DS_LA_RANDOM) {
    const uint32_t x = k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w;
    return __fsub_rn(__fmul_rn((float)ds_u24(x), 1.0f / 8388608.0f), 1.0f);
  }
  if (mode == DS_LA_NOISE) {             // Box-Muller: (w.x, w.y) give z0, z1; (w.z, w.w) give z2, z3
    const uint32_t a = k < 2 ? w.x : w.z, b = k < 2 ? w.y : w.w;
    const float u1 = __fmul_rn((float)(ds_u24(a) + 1u), 1.0f / 16777216.0f), u2 = __fmul_rn((float)ds_u24(b), 1.0f / 16777216.0f);
    const float r = sqrtf(__fmul_rn(-2.0f, logf(u1))), phi = __fmul_rn(6.28318530717958647692f, u2);
    const float z = __fmul_rn(r, (k & 1) ? sinf(phi) : cosf(phi));
    return fminf(fmaxf(__fadd_rn(la, __fmul_rn(noise_std, z)), -1.0f), 1.0f);
  }
  return la;
}

__global__ __launch_bounds__(kDsCopyThreads) void dataset_gather_kernel(DatasetView v, DatasetBatch b) {
  const size_t j = blockIdx.x;
  const int t = threadIdx.x;
  const size_t S = (size_t)v.n_spheres, words = S * kDsSphereFloats;
  const bool wide = (v.n_spheres & 1) == 0;
  long long slot_ll;
  if (b.index) {
    const long long i = b.index[j];
    slot_ll = i < 0 ? 0 : i >= (long long)v.capacity ? (long long)v.capacity - 1 : i;
  } else {
    const long long total = *v.total;
    const uint32_t size = (uint32_t)(total < (long long)v.capacity ? total : (long long)v.capacity);
    const U4 w = philox4x32_10((uint32_t)j, b.draw_lo, b.draw_hi, 1u, b.seed_lo, b.seed_hi);
    slot_ll = size ? (long long)__umulhi(w.x, size) : -1;
  }
  if (t == 0 && b.out_index) b.out_index[j] = slot_ll;
  if (slot_ll < 0) {                     // an empty ring: the row is zeros
    float* d = b.stacked + j * words;
    for (int i = t; i < (int)words; i += kDsCopyThreads) d[i] = 0.f;
    if (t < kDsInertial) b.inertial[j * kDsInertial + t] = 0.f;
    else if (t >= 64 && t < 64 + kDsAction) b.last_action[j * kDsAction + t - 64] = 0.f;
    else if (t >= 128 && t < 128 + kDsAction) b.teacher[j * kDsAction + t - 128] = 0.f;
    else if (t >= 192 && t < 192 + v.n_spheres) b.mask[j * S + t - 192] = 0;
    return;
  }
  const size_t slot = (size_t)slot_ll;
  ds_copy_floats(b.stacked + j * words, v.stacked + slot * words, (int)words, wide);
  ds_copy_small(b.inertial + j * kDsInertial, nullptr, b.teacher + j * kDsAction, b.mask + j * S, v.inertial + slot * kDsInertial, nullptr,
                v.teacher + slot * kDsAction, v.mask + slot * S, v.n_spheres, false);
  if (t >= 64 && t < 64 + kDsAction) {
    const int k = t - 64;
    float la = v.last_action[slot * kDsAction + k];
    if (b.mode != DS_LA_KEEP) {
      const U4 w = philox4x32_10((uint32_t)j, b.draw_lo, b.draw_hi, 2u, b.seed_lo, b.seed_hi);
      la = ds_last_action(la, k, w, b.mode, b.noise_std);
    }
    b.last_action[j * kDsAction + k] = la;
  }
}

}  // namespace te
