// Host-side helpers of the gfx950 canary sources and of the host-link, pace and LDS-path
// libraries, header-only (every .hip file still compiles on its own): the owners of device
// buffers and events, the sticky HIP status every entry point reports through, the launch with
// the largest dynamic LDS allocation, the timing sequence, and the prototypes of the functions
// one source calls in another that are not part of the C ABI.  The site text, the coverage walk
// and the launch plan come with canary_common.h from site.h.  This is the only place
// that frees a device buffer or destroys an event.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "canary_common.h"
#include "mfma_forms.h"

namespace canary {

#define CANARY_INTERNAL __attribute__((visibility("hidden")))  // cross-file, not exported

// The first HIP error wins.  stage() names what runs next ("reg_march: "); the error keeps the
// stage it happened in, and report() writes "<prefix><stage><hipGetErrorString>" once.
class Status {
 public:
  bool ok() const { return e_ == hipSuccess; }
  void stage(const char* what) {
    if (ok()) what_ = what;
  }
  // `what`, when given, names this one step instead of the current stage
  bool check(hipError_t e, const char* what = nullptr) {
    if (ok() && e != hipSuccess) {
      e_ = e;
      if (what) what_ = what;
    }
    return ok();
  }
  bool fail(const char* what) { return check(hipErrorLaunchFailure, what); }  // a launch nothing granted
  // 0, or -1 with the text in err
  int report(const char* prefix, char* err, int err_len) const {
    if (ok()) return 0;
    std::snprintf(err, err_len, "%s%s%s", prefix, what_, hipGetErrorString(e_));
    return -1;
  }

 private:
  hipError_t e_ = hipSuccess;
  const char* what_ = "";
};

// One step of a sequence: evaluated only while every earlier step succeeded (a macro, so the
// HIP call itself is skipped).  CANARY_HIP(st, call) or CANARY_HIP(st, call, "what: ").
#define CANARY_HIP(st, ...) ((st).ok() && (st).check(__VA_ARGS__))

// Owns one hipMalloc allocation.
template <typename T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; }  // move-only
  ~DeviceBuffer() {
    if (p_) (void)hipFree(p_);
  }
  hipError_t alloc(size_t bytes) {  // once per buffer
    bytes_ = bytes;
    return p_ ? hipErrorInvalidValue : hipMalloc(&p_, bytes);
  }
  hipError_t fill(int byte) { return hipMemset(p_, byte, bytes_); }
  hipError_t zero() { return fill(0); }
  hipError_t upload(const void* host) { return hipMemcpy(p_, host, bytes_, hipMemcpyHostToDevice); }
  hipError_t download(void* host) const { return hipMemcpy(host, p_, bytes_, hipMemcpyDeviceToHost); }
  T* get() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// Owns N events; everything is recorded on the null stream.
template <int N>
class Events {
 public:
  static constexpr int size = N;
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t create() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreate(&ev_[i]);
    return e;
  }
  hipError_t record(int i) const { return hipEventRecord(ev_[i], 0); }
  hipError_t synchronize(int i) const { return hipEventSynchronize(ev_[i]); }
  hipError_t elapsed_ms(int i, int j, float* ms) const { return hipEventElapsedTime(ms, ev_[i], ev_[j]); }

 private:
  hipEvent_t ev_[N] = {};
};

// The timing sequence of every check: record, launch(0), record, launch(1), ..., record,
// synchronize on the last event, hipGetLastError; ms[k] = device time of launch(k), which
// returns a hipError_t (an error ends the sequence) and may start several kernels.
template <typename Ev, int N, typename Launch>
bool time_stages(Status& st, const Ev& ev, float (&ms)[N], Launch&& launch) {
  static_assert(Ev::size > N, "one event more than stages");
  CANARY_HIP(st, ev.record(0));
  for (int k = 0; k < N; ++k) {
    if (st.ok()) st.check(launch(k));
    CANARY_HIP(st, ev.record(k + 1));
  }
  CANARY_HIP(st, ev.synchronize(N));
  CANARY_HIP(st, hipGetLastError());
  for (int k = 0; k < N; ++k) CANARY_HIP(st, ev.elapsed_ms(k, k + 1, &ms[k]));
  return st.ok();
}

// The verifier self-tests: `launch(st, prop, d_errors)` starts kernels that add to one zeroed
// device counter; returns the count once they finished, -1 on a HIP error.
template <typename Launch>
long long count_errors(int device, Launch&& launch) {
  Status st;
  hipDeviceProp_t prop;
  DeviceBuffer<unsigned long long> d_errors;
  unsigned long long h = 0;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  CANARY_HIP(st, d_errors.alloc(sizeof(h)));
  CANARY_HIP(st, d_errors.zero());
  if (st.ok()) launch(st, prop, d_errors.get());
  CANARY_HIP(st, hipGetLastError());
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, d_errors.download(&h));
  return st.ok() ? static_cast<long long>(h) : -1;
}

// ---- the MFMA rate launches (rate_chain<F>, mfma_forms.h): 8 blocks of 4 waves per CU ----
constexpr int kRateThreads = 256;
inline int rate_blocks(const hipDeviceProp_t& prop) { return prop.multiProcessorCount * 8; }
inline hipError_t alloc_rate_sink(DeviceBuffer<float>& sink, int blocks) {
  return sink.alloc(static_cast<size_t>(blocks) * kRateThreads * sizeof(float));
}

// Device ms of one launch of `kernel` with `iters` MFMA pairs per wave, after a warm-up of 16; 0 on a HIP error.
template <typename Ev, typename Kernel>
float time_rate_launch(Status& st, const Ev& ev, Kernel kernel, int blocks, int iters, float* sink) {
  float ms[1] = {0};
  if (!st.ok()) return 0;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRateThreads), 0, 0, 16, sink);  // warm-up
  time_stages(st, ev, ms, [&](int) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRateThreads), 0, 0, iters, sink);
    return hipSuccess;
  });
  return st.ok() ? ms[0] : 0;
}

// Dense TFLOP/s of such a launch of form F that took `ms` (0 when ms is): 2 * 32 * 32 * K flop per MFMA.
template <class F>
double rate_tflops(int iters, int blocks, float ms) {
  const double flops = 2.0 * 32 * 32 * F::kK * 2.0 /*chains*/ * iters * (blocks * (kRateThreads / kWave));
  return ms > 0 ? flops / (ms * 1e-3) / 1e12 : 0;
}

constexpr int kMaxLdsBytes = 160 * 1024;

// Stands in launch_with_max_lds's argument list for the granted allocation in 4-byte words.
struct granted_lds_words {};
template <typename T>
T lds_arg(T v, size_t) { return v; }
inline int lds_arg(granted_lds_words, size_t bytes) { return static_cast<int>(bytes / 4); }

// Launches `kernel` on the null stream with the largest dynamic LDS allocation the device
// grants (160 KB on gfx950, which keeps one workgroup per CU): maxSharedMemoryPerMultiProcessor
// capped at kMaxLdsBytes, else sharedMemPerBlock, rounded down to 1 KiB, two attempts.
// Returns the bytes granted, 0 on a HIP error.
template <typename Kernel, typename... Args>
size_t launch_with_max_lds(Kernel kernel, const hipDeviceProp_t& prop, dim3 grid, dim3 block, Args... args) {
  size_t bytes = prop.maxSharedMemoryPerMultiProcessor > 0 ? prop.maxSharedMemoryPerMultiProcessor : 0;
  if (bytes > static_cast<size_t>(kMaxLdsBytes)) bytes = kMaxLdsBytes;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (attempt == 1 || bytes == 0) bytes = prop.sharedMemPerBlock;
    bytes &= ~static_cast<size_t>(1023);
    if (bytes == 0) return 0;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(bytes));
    hipLaunchKernelGGL(kernel, grid, block, bytes, 0, lds_arg(args, bytes)...);
    if (hipGetLastError() == hipSuccess) return bytes;
  }
  return 0;
}

// hbm.hip: the warm-up write, then `passes` timed write + verify pairs over the n 16-byte
// words of buf; mismatches are added to *d_errors, the device ms to *t_write / *t_read.
CANARY_INTERNAL void hbm_passes(Status& st, const Events<3>& ev, const hipDeviceProp_t& prop, uint4* buf, uint64_t n,
                                int passes, unsigned long long* d_errors, float* t_write, float* t_read);

// sites.hip: "site check: 5 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)" for
// `errors` wrong results (unlocated ones included); returns its length.
CANARY_INTERNAL int sites_describe(const amdgpu_canary_sites_result& r, unsigned long long errors, char* buf, int len);

}  // namespace canary
