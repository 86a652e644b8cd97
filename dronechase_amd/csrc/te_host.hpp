// te_host.hpp — the host plumbing every C ABI entry shares (included by te_env.hip, the library's one translation unit): the
// thread-local error text, the HIP error check, the device guard, and for the entries that take no te_env
// (te_abi_stateless.hpp) one pointer check, one launch and one per-device cache.  Host only: no kernel lives here.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <mutex>
#include <string>

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return 1; }
#define TE_HIP(x)                                                                                      \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_));                  \
  } while (0)

struct DeviceGuard {
  int prev = -1; bool ok;
  explicit DeviceGuard(int dev) { ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess); if (prev == dev) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The required pointers of a call, checked in the order given: "who: null argument NAME", then "who: NAME must be A-byte aligned".
struct PtrArg { const char* name; const void* p; unsigned align; };
static int pointers_check(const std::string& who, std::initializer_list<PtrArg> ps) {
  for (const PtrArg& q : ps) {
    if (!q.p) return fail(who + ": null argument " + q.name);
    if ((uintptr_t)q.p & (q.align - 1)) return fail(who + ": " + q.name + " must be " + std::to_string(q.align) + "-byte aligned");
  }
  return 0;
}

// What the stateless entries ask a device once and keep, under one mutex (the errors are thread-local: callers on several threads are
// served).  Neither question is a stream operation, so a capturing stream allows both.
struct DeviceCache {
  std::mutex lock;
  std::map<const void*, uint64_t> opted;   // kernel -> one bit per device: its dynamic LDS above the default 64 KB is granted
  int cus[64] = {};                        // device -> its compute units; 0: not asked yet
};
static DeviceCache g_devices;

// dynamic LDS beyond the 64 KB a launch gets by default: opt in once per (function, device)
static int lds_opt_in(const void* fn, int lds_bytes) {
  int dev = 0;
  TE_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> hold(g_devices.lock);
  uint64_t& bits = g_devices.opted[fn];
  if (dev < 64 && !(bits >> dev & 1)) {
    TE_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    bits |= 1ull << dev;
  }
  return 0;
}

// the compute units of the current device, asked once per device: the sphere kernels run persistent workgroups, sized by the CU count
static int device_cu_count(const std::string& who, int* out) {
  int dev = 0;
  TE_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> hold(g_devices.lock);
  int n_cu = dev < 64 ? g_devices.cus[dev] : 0;
  if (!n_cu) {
    TE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    if (n_cu < 1) return fail(who + ": the device reports no compute units");
    if (dev < 64) g_devices.cus[dev] = n_cu;
  }
  *out = n_cu;
  return 0;
}

template <class T>
struct Formal { using type = T; };   // the arguments convert to the kernel's formals; they do not deduce them

// The one launch of every kernel that is no part of a te_env's plan: kernel(args...) on `groups` workgroups of `threads` with
// `lds_bytes` of dynamic LDS (0: none, and nothing to opt in to), on the caller's stream, and the launch's own error.
template <class... Args>
static int stateless_launch(void (*fn)(Args...), size_t groups, int threads, int lds_bytes, void* stream, const typename Formal<Args>::type&... args) {
  if (lds_bytes && lds_opt_in(reinterpret_cast<const void*>(fn), lds_bytes)) return 1;
  hipLaunchKernelGGL(fn, dim3((unsigned)groups), dim3(threads), (size_t)lds_bytes, (hipStream_t)stream, args...);
  TE_HIP(hipGetLastError());
  return 0;
}
