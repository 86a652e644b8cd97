// te_monitor.hpp — the episode monitor (te_monitor_*, include/threatengage.h): per-env episode return and length next to the
// step, the completed episodes of a window reduced on the device, and SB3 evaluate_policy's per-env record quotas.
//
//   monitor_step_kernel   one thread per env, 256-thread workgroups.  ret += reward (a plain fp32 add), len += 1; a wave whose
//                         __ballot(done) is empty stores the two words and leaves (the common case).  A wave with done lanes
//                         writes their records, reduces (count, len, info, ret, ret^2, min, max) over its lanes by an xor
//                         butterfly (a fixed tree: the sum's order depends on the lane index only) and lane 0 read-modify-writes
//                         the wave's OWN row of the buffer.  No float atomics; the only atomic is the integer `recorded`.
//   monitor_stats_kernel  one workgroup: thread t sums rows t, t + 256, ... in index order, the 256 partials are reduced by a
//                         fixed LDS tree, thread 0 writes te_monitor_summary; every thread then clears the rows it read.
//
// HBM traffic of a step: reward 4 + done 1 + ret 8 + len 8 = 21 bytes per env when nothing finishes, + info 16 = 37 on a done lane.
#pragma once

#include <cstddef>
#include <cstdint>

namespace te {

constexpr int kMonThreads = 256;
constexpr int kMonHeaderBytes = 64;      // word 0: recorded (i32); the rest is reserved and zero

struct MonitorRow {                      // one wave's window accumulators (72 bytes)
  long long count, sum_len, sum_info[4];
  double sum_ret, sum_ret2;
  float min_ret, max_ret;
};
static_assert(sizeof(MonitorRow) == 72, "MonitorRow is part of the buffer layout");
static_assert(sizeof(te_monitor_summary) == 80, "te_monitor_summary is part of the ABI");

inline size_t mon_align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline te_monitor_offsets monitor_offsets(int64_t N, int64_t R) {
  te_monitor_offsets o{};
  size_t at = kMonHeaderBytes;
  auto take = [&](size_t bytes) { size_t here = at; at = mon_align16(at + bytes); return here; };
  o.n_rows = (size_t)((N + 63) / 64);
  o.rows = take(o.n_rows * sizeof(MonitorRow));
  o.ret = take((size_t)N * 4); o.len = take((size_t)N * 4); o.episodes = take((size_t)N * 4);
  o.last_ret = take((size_t)N * 4); o.last_len = take((size_t)N * 4);
  o.rec_info = take((size_t)R * 16); o.rec_ret = take((size_t)R * 4); o.rec_len = take((size_t)R * 4);
  o.bytes = at;
  return o;
}

struct MonitorView {                     // the buffer's arrays as the kernels address them
  int* recorded;
  MonitorRow* rows;
  float* ret; int* len; int* episodes; float* last_ret; int* last_len;
  int4* rec_info; float* rec_ret; int* rec_len;
  int n_envs, n_records, n_rows;
};

inline MonitorView monitor_view(void* mon, int32_t N, int32_t R) {
  const te_monitor_offsets o = monitor_offsets(N, R);
  char* b = static_cast<char*>(mon);
  return MonitorView{reinterpret_cast<int*>(b), reinterpret_cast<MonitorRow*>(b + o.rows), reinterpret_cast<float*>(b + o.ret),
                     reinterpret_cast<int*>(b + o.len), reinterpret_cast<int*>(b + o.episodes), reinterpret_cast<float*>(b + o.last_ret),
                     reinterpret_cast<int*>(b + o.last_len), reinterpret_cast<int4*>(b + o.rec_info), reinterpret_cast<float*>(b + o.rec_ret),
                     reinterpret_cast<int*>(b + o.rec_len), N, R, (int)o.n_rows};
}

template <typename T>
__device__ inline T mon_wave_sum(T v) {  // xor butterfly over the 64 lanes: a fixed tree, every lane ends with the total
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ __launch_bounds__(kMonThreads) void monitor_step_kernel(MonitorView m, const float* __restrict__ reward,
                                                                   const uint8_t* __restrict__ done, const int4* __restrict__ info) {
  const int e = blockIdx.x * kMonThreads + threadIdx.x;
  const bool live = e < m.n_envs;
  float ret = 0.f;
  int len = 0;
  bool d = false;
  if (live) {
    ret = __fadd_rn(m.ret[e], reward[e]);
    len = m.len[e] + 1;
    d = done[e] != 0;
  }
  if (__ballot(d) == 0ull) {             // nothing finished in this wave
    if (live) { m.ret[e] = ret; m.len[e] = len; }
    return;
  }
  int4 row = make_int4(0, 0, 0, 0);
  if (d) {
    row = info[e];
    const int k = m.episodes[e];
    // evaluate_policy's quota of env e, (n_records + e) / N, and the exclusive prefix sum of the quotas before it
    const int q = m.n_records / m.n_envs, first_extra = m.n_envs - m.n_records % m.n_envs;
    const int quota = q + (e >= first_extra ? 1 : 0);
    if (k < quota) {
      const long long slot = (long long)e * q + (e > first_extra ? e - first_extra : 0) + k;
      m.rec_ret[slot] = ret; m.rec_len[slot] = len; m.rec_info[slot] = row;
      atomicAdd(m.recorded, 1);
    }
    m.episodes[e] = k + 1;
    m.last_ret[e] = ret; m.last_len[e] = len;
    m.ret[e] = 0.f; m.len[e] = 0;
  } else if (live) {
    m.ret[e] = ret; m.len[e] = len;
  }
  const double r = d ? (double)ret : 0.0;
  const long long count = mon_wave_sum<long long>(d ? 1 : 0);
  const long long sum_len = mon_wave_sum<long long>(d ? len : 0);
  const long long i0 = mon_wave_sum<long long>(row.x), i1 = mon_wave_sum<long long>(row.y);
  const long long i2 = mon_wave_sum<long long>(row.z), i3 = mon_wave_sum<long long>(row.w);
  const double sum_ret = mon_wave_sum<double>(r), sum_ret2 = mon_wave_sum<double>(r * r);
  float lo = d ? ret : INFINITY, hi = d ? ret : -INFINITY;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, s, 64));
    hi = fmaxf(hi, __shfl_xor(hi, s, 64));
  }
  if ((threadIdx.x & 63) == 0) {         // this wave's own row: no other wave touches it
    MonitorRow* w = m.rows + (e >> 6);
    const bool first = w->count == 0;
    w->count += count; w->sum_len += sum_len;
    w->sum_info[0] += i0; w->sum_info[1] += i1; w->sum_info[2] += i2; w->sum_info[3] += i3;
    w->sum_ret += sum_ret; w->sum_ret2 += sum_ret2;
    w->min_ret = first ? lo : fminf(w->min_ret, lo);
    w->max_ret = first ? hi : fmaxf(w->max_ret, hi);
  }
}

__global__ __launch_bounds__(kMonThreads) void monitor_stats_kernel(MonitorView m, te_monitor_summary* out, int reset_window) {
  __shared__ MonitorRow part[kMonThreads];
  const int t = threadIdx.x;
  MonitorRow a{};
  a.min_ret = INFINITY; a.max_ret = -INFINITY;
  for (int i = t; i < m.n_rows; i += kMonThreads) {
    const MonitorRow w = m.rows[i];
    if (w.count == 0) continue;
    a.count += w.count; a.sum_len += w.sum_len;
    for (int j = 0; j < 4; ++j) a.sum_info[j] += w.sum_info[j];
    a.sum_ret += w.sum_ret; a.sum_ret2 += w.sum_ret2;
    a.min_ret = fminf(a.min_ret, w.min_ret); a.max_ret = fmaxf(a.max_ret, w.max_ret);
  }
  part[t] = a;
  __syncthreads();
  for (int s = kMonThreads / 2; s >= 1; s >>= 1) {
    if (t < s) {
      MonitorRow& x = part[t];
      const MonitorRow& y = part[t + s];
      x.count += y.count; x.sum_len += y.sum_len;
      for (int j = 0; j < 4; ++j) x.sum_info[j] += y.sum_info[j];
      x.sum_ret += y.sum_ret; x.sum_ret2 += y.sum_ret2;
      x.min_ret = fminf(x.min_ret, y.min_ret); x.max_ret = fmaxf(x.max_ret, y.max_ret);
    }
    __syncthreads();
  }
  if (t == 0) {
    const MonitorRow& x = part[0];
    out->count = x.count; out->sum_len = x.sum_len;
    for (int j = 0; j < 4; ++j) out->sum_info[j] = x.sum_info[j];
    out->sum_ret = x.sum_ret; out->sum_ret2 = x.sum_ret2;
    out->min_ret = x.count ? x.min_ret : 0.f; out->max_ret = x.count ? x.max_ret : 0.f;
    out->recorded = *m.recorded; out->reserved = 0;
  }
  if (reset_window)
    for (int i = t; i < m.n_rows; i += kMonThreads) m.rows[i] = MonitorRow{};
}

}  // namespace te
