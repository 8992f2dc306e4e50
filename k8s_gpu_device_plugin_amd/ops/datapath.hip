// MI355X (gfx950 / CDNA4) health canary, part 2: the low-precision matrix datapaths
// and the LDS.
//
// canary.hip checks HBM and the bf16 MFMA path.  CDNA4's low-precision throughput runs
// on other instructions: the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (OCP fp8
// e4m3, bf8 e5m2 and fp4 e2m1 operands with one E8M0 scale per 32-element block; 2x and
// 4x the bf16 rate per clock, MI355X_MICROARCH.md "Matrix cores") and the non-scaled
// v_mfma_f32_32x32x16_fp8_fp8.  A pod that serves an fp8 or MXFP4 model computes on
// these, so a partition is advertised healthy only if they are exact too:
//
//   1. Exactness: one wave per block computes C[32x32] = A[32xK] * B[Kx32] from small
//      integers (exact in every format) with per-lane power-of-two block scales, then checks
//      every accumulator register against a scalar integer reference (form_check<F>).  Blocks
//      below `inject_blocks` perturb one operand: the fault injection that proves the verifier
//      sees a wrong result.
//   2. Rate: register-resident MFMA chains, 8 blocks of 4 waves per CU -> TFLOP/s (rate_chain<F>).
//   3. LDS march: every workgroup takes its CU's whole LDS (160 KB on gfx950), writes
//      an address-derived pattern, reads it back in reverse order (words written by
//      another wave, so addressing faults show) while writing the complement, then
//      reads the complement (both polarities of every bit).
//
// The forms, their operand and scale layout, form_check and rate_chain: mfma_forms.h.
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "canary_host.h"

namespace {

using namespace canary;

// One wave per block runs the exactness check of form F; blocks below `inject_blocks` perturb one operand.
template <class F>
__device__ __forceinline__ void exact_block(int ksteps, int vary_scale, int inject_blocks,
                                            unsigned long long* __restrict__ errors) {
  const int lane = threadIdx.x;
  uint32_t bad = form_check<F>(blockIdx.x, lane, ksteps, vary_scale, static_cast<int>(blockIdx.x) < inject_blocks);
  wave_sum(bad);
  if (lane == 0 && bad) atomicAdd(errors, static_cast<unsigned long long>(bad));
}

template <int FMT>
__global__ void __launch_bounds__(64) lowp_exact(int ksteps, int vary_scale, int inject_blocks,
                                                 unsigned long long* __restrict__ errors) {
  exact_block<FormScaled<FMT>>(ksteps, vary_scale, inject_blocks, errors);
}

__global__ void __launch_bounds__(64) fp8_exact(int ksteps, int inject_blocks, unsigned long long* __restrict__ errors) {
  exact_block<FormFp8Unscaled>(ksteps, 0, inject_blocks, errors);
}

template <int FMT>
constexpr auto lowp_rate = rate_chain<FormScaled<FMT>>;  // the kernel (mfma_forms.h)

// C[MxN] (fp32) = dequant(A)[MxK] * dequant(Bt)[NxK]^T with one E8M0 scale per 32 k:
// A, Bt hold one OCP code per byte (fp4 in the low nibble), sa [M][K/32], sb [N][K/32].
// One wave per 32x32 output tile; M, N % 32 == 0 and K % 64 == 0 (host-checked).
template <int FMT>
__global__ void __launch_bounds__(64) lowp_gemm(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt,
                                                const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb,
                                                float* __restrict__ C, int M, int N, int K) {
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int kblocks = K / 32;
  f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const uint8_t* ap = A + static_cast<size_t>(m0 + r) * K + k0;
    const uint8_t* bp = Bt + static_cast<size_t>(n0 + r) * K + k0;
    const auto at = [h](int j) { return kmap<FMT>(h, j); };
    const i32x8 a = raw_operand<FMT>(ap, at), b = raw_operand<FMT>(bp, at);
    const int ka = sa[static_cast<size_t>(m0 + r) * kblocks + k0 / 32 + h];
    const int kb = sb[static_cast<size_t>(n0 + r) * kblocks + k0 / 32 + h];
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 0, ka, 0, kb);
  }
  for (int reg = 0; reg < 16; ++reg) {
    const int row = cd_row32(reg, h);
    C[static_cast<size_t>(m0 + row) * N + n0 + (lane & 31)] = acc[reg];
  }
}

// One MFMA on raw fragments: lane l's operand element j is a[l * 32 + j] / b[l * 32 + j]
// (one code per byte), its scales sa[l] / sb[l]; C is written row-major with the 32x32
// C/D map.  For layout probes (scripts/probe_lowp_layout.py), not for the canary run.
template <int FMT>
__global__ void __launch_bounds__(64) lowp_raw(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                               const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb,
                                               float* __restrict__ C) {
  const int lane = threadIdx.x;
  const auto at = [](int j) { return j; };
  const i32x8 x = raw_operand<FMT>(a + lane * 32, at), y = raw_operand<FMT>(b + lane * 32, at);
  f32x16 acc = zero_f32x16();
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(x, y, acc, FMT, FMT, 0, sa[lane], 0, sb[lane]);
  for (int reg = 0; reg < 16; ++reg) {
    const int row = cd_row32(reg, lane >> 5);
    C[row * 32 + (lane & 31)] = acc[reg];
  }
}

__device__ __forceinline__ uint32_t lds_pat(uint32_t i, uint32_t seed) { return i * 0x9E3779B1u ^ seed; }

// March over `words` 4-byte LDS words (the whole dynamic allocation).  Block b < inject_blocks
// flips one bit between the write and the first read (verifier self-test: one mismatch each).
__global__ void __launch_bounds__(256) lds_march(int words, uint32_t seed, int inject_blocks,
                                                 unsigned long long* __restrict__ errors) {
  extern __shared__ uint32_t lds[];
  const uint32_t s = seed ^ mix32(blockIdx.x);
  const int t = threadIdx.x, nt = blockDim.x;
  for (int i = t; i < words; i += nt) lds[i] = lds_pat(i, s);
  __syncthreads();
  if (t == 0 && static_cast<int>(blockIdx.x) < inject_blocks) lds[words / 3] ^= 1u << (blockIdx.x & 31);
  __syncthreads();
  uint32_t bad = 0;
  for (int i = t; i < words; i += nt) {  // descending: thread t reads what thread nt-1-t wrote
    const int j = words - 1 - i;
    const uint32_t want = lds_pat(j, s);
    bad += lds[j] != want;
    lds[j] = ~want;
  }
  __syncthreads();
  for (int i = t; i < words; i += nt) bad += lds[i] != ~lds_pat(i, s);
  wave_sum(bad);
  // no __shared__ scratch: the dynamic allocation is the whole LDS
  if ((t & (kWave - 1)) == 0 && bad) atomicAdd(errors, static_cast<unsigned long long>(bad));
}

// Launches lds_march over 2 workgroups per CU with the largest LDS allocation the device
// grants (160 KB on gfx950); returns its size in bytes, 0 on a HIP error.
unsigned long long launch_lds_march(const hipDeviceProp_t& prop, int inject_blocks, unsigned long long* d_err) {
  return launch_with_max_lds(lds_march, prop, dim3(prop.multiProcessorCount * 2), dim3(256), granted_lds_words{},
                             0xC0FFEEu, inject_blocks, d_err);
}

// The instantiation of a block-scaled kernel for format code `fmt`; null for any other code.
template <typename K>
K by_format(int fmt, K fp8, K bf8, K fp4) {
  return fmt == kFp8 ? fp8 : fmt == kBf8 ? bf8 : fmt == kFp4 ? fp4 : nullptr;
}

// Dense TFLOP/s of the block-scaled form `fmt` from one timed launch; 0 on a HIP error or an unknown format.
double lowp_rate_tflops(Status& st, int fmt, int blocks, int iters, float* sink) {
  const auto kernel = by_format(fmt, lowp_rate<kFp8>, lowp_rate<kBf8>, lowp_rate<kFp4>);
  Events<2> ev;
  CANARY_HIP(st, ev.create());
  if (kernel == nullptr) return 0;
  static_assert(FormScaled<kFp8>::kK == FormScaled<kBf8>::kK && FormScaled<kFp8>::kK == FormScaled<kFp4>::kK);
  return rate_tflops<FormScaled<kFp8>>(iters, blocks, time_rate_launch(st, ev, kernel, blocks, iters, sink));
}

bool launch_lowp_exact(int fmt, int blocks, int ksteps, int vary, int inject, unsigned long long* d_err) {
  if (fmt == kFp8Unscaled)
    hipLaunchKernelGGL(fp8_exact, dim3(blocks), dim3(64), 0, 0, 4 * ksteps, inject, d_err);
  else if (const auto kernel = by_format(fmt, lowp_exact<kFp8>, lowp_exact<kBf8>, lowp_exact<kFp4>))
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, 0, ksteps, vary, inject, d_err);
  else
    return false;
  return hipGetLastError() == hipSuccess;
}

}  // namespace


extern "C" {

// Exactness of every low-precision MFMA form (2 blocks per CU each, K = 256, varied block
// scales), the LDS march, and the fp8 / fp4 rates (`iters` MFMA pairs per wave).
int amdgpu_canary_datapaths(int device, int iters, amdgpu_canary_datapath_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  Status st;
  hipDeviceProp_t prop;
  DeviceBuffer<unsigned long long> d_err;  // [0] lowp, [1] lds
  DeviceBuffer<float> sink;
  unsigned long long h_err[2] = {0, 0};
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  CANARY_HIP(st, d_err.alloc(sizeof(h_err)));
  CANARY_HIP(st, d_err.zero());
  CANARY_HIP(st, alloc_rate_sink(sink, rate_blocks(prop)));
  for (int fmt : {kFp8, kBf8, kFp4, kFp8Unscaled})
    if (st.ok() && !launch_lowp_exact(fmt, prop.multiProcessorCount * 2, 4, 1, 0, d_err.get())) st.fail("");
  if (st.ok()) {
    out->lds_bytes = launch_lds_march(prop, 0, d_err.get() + 1);
    if (out->lds_bytes == 0) st.fail("");
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, d_err.download(h_err));
  if (st.ok()) {
    out->lowp_errors = h_err[0];
    out->lds_errors = h_err[1];
    if (iters < 1) iters = 1;
    out->fp8_tflops = lowp_rate_tflops(st, kFp8, rate_blocks(prop), iters, sink.get());
    out->fp4_tflops = lowp_rate_tflops(st, kFp4, rate_blocks(prop), iters, sink.get());
  }
  return st.report("datapaths: ", err, err_len);
}

// Wrong accumulator registers of one low-precision form (fmt 0 fp8, 1 bf8, 4 fp4: block
// scaled, K = 64 * ksteps; 8: unscaled fp8, K = 64 * ksteps too) over 2 blocks per CU, of
// which `inject_blocks` compute with one perturbed operand.  -1 on a HIP error.
long long amdgpu_canary_lowp_check(int device, int fmt, int ksteps, int vary_scale, int inject_blocks) {
  if (ksteps < 1 || ksteps > 64 || inject_blocks < 0) return -1;
  return count_errors(device, [&](Status& st, const hipDeviceProp_t& prop, unsigned long long* d_err) {
    if (!launch_lowp_exact(fmt, prop.multiProcessorCount * 2, ksteps, vary_scale, inject_blocks, d_err)) st.fail("");
  });
}

// Dense TFLOP/s of the block-scaled form `fmt` (0 fp8, 1 bf8, 4 fp4); -1 on error.
int amdgpu_canary_lowp_rate(int device, int fmt, int iters, double* tflops) {
  *tflops = 0;
  if (iters < 1) return -1;
  Status st;
  hipDeviceProp_t prop;
  DeviceBuffer<float> sink;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  CANARY_HIP(st, alloc_rate_sink(sink, rate_blocks(prop)));
  if (!st.ok()) return -1;
  *tflops = lowp_rate_tflops(st, fmt, rate_blocks(prop), iters, sink.get());
  return *tflops > 0 ? 0 : -1;
}

// LDS march mismatches over 2 workgroups per CU (`inject_blocks` of them flip one bit);
// *bytes = LDS bytes per workgroup covered.  -1 on a HIP error.
long long amdgpu_canary_lds_check(int device, int inject_blocks, unsigned long long* bytes) {
  *bytes = 0;
  if (inject_blocks < 0) return -1;
  return count_errors(device, [&](Status& st, const hipDeviceProp_t& prop, unsigned long long* d_err) {
    *bytes = launch_lds_march(prop, inject_blocks, d_err);
    if (*bytes == 0) st.fail("");
  });
}

// Host wrapper for the numerics test (see lowp_gemm): all buffers in host memory.
int amdgpu_canary_lowp_gemm(int device, int fmt, const uint8_t* a_host, const uint8_t* bt_host, const uint8_t* sa_host,
                            const uint8_t* sb_host, float* c_host, int M, int N, int K, char* err, int err_len) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 64 || (fmt != kFp8 && fmt != kBf8 && fmt != kFp4)) {
    std::snprintf(err, err_len, "fmt %d shape (%d,%d,%d): need fmt 0/1/4, M,N %% 32 == 0, K %% 64 == 0", fmt, M, N, K);
    return -1;
  }
  Status st;
  DeviceBuffer<uint8_t> a, bt, sa, sb;
  DeviceBuffer<float> c;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, a.alloc(static_cast<size_t>(M) * K));
  CANARY_HIP(st, bt.alloc(static_cast<size_t>(N) * K));
  CANARY_HIP(st, sa.alloc(static_cast<size_t>(M) * (K / 32)));
  CANARY_HIP(st, sb.alloc(static_cast<size_t>(N) * (K / 32)));
  CANARY_HIP(st, c.alloc(static_cast<size_t>(M) * N * 4));
  CANARY_HIP(st, a.upload(a_host));
  CANARY_HIP(st, bt.upload(bt_host));
  CANARY_HIP(st, sa.upload(sa_host));
  CANARY_HIP(st, sb.upload(sb_host));
  if (st.ok()) {
    const auto kernel = by_format(fmt, lowp_gemm<kFp8>, lowp_gemm<kBf8>, lowp_gemm<kFp4>);
    hipLaunchKernelGGL(kernel, dim3(N / 32, M / 32), dim3(64), 0, 0, a.get(), bt.get(), sa.get(), sb.get(), c.get(), M, N,
                       K);
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, c.download(c_host));
  return st.report("", err, err_len);
}

// Raw-fragment probe (see lowp_raw): a, b [64][32] codes, sa, sb [64], c [32][32].
int amdgpu_canary_lowp_raw(int device, int fmt, const uint8_t* a_host, const uint8_t* b_host, const uint8_t* sa_host,
                           const uint8_t* sb_host, float* c_host) {
  if (fmt != kFp8 && fmt != kBf8 && fmt != kFp4) return -1;
  Status st;
  DeviceBuffer<uint8_t> buf;  // a, b, sa, sb back to back
  DeviceBuffer<float> c;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, buf.alloc(2 * 2048 + 2 * 64));
  CANARY_HIP(st, c.alloc(32 * 32 * 4));
  uint8_t *a = buf.get(), *b = a + 2048, *sa = a + 4096, *sb = a + 4160;
  CANARY_HIP(st, hipMemcpy(a, a_host, 2048, hipMemcpyHostToDevice));
  CANARY_HIP(st, hipMemcpy(b, b_host, 2048, hipMemcpyHostToDevice));
  CANARY_HIP(st, hipMemcpy(sa, sa_host, 64, hipMemcpyHostToDevice));
  CANARY_HIP(st, hipMemcpy(sb, sb_host, 64, hipMemcpyHostToDevice));
  if (st.ok()) {
    const auto kernel = by_format(fmt, lowp_raw<kFp8>, lowp_raw<kBf8>, lowp_raw<kFp4>);
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, 0, a, b, sa, sb, c.get());
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, c.download(c_host));
  return st.ok() ? 0 : -1;
}

}  // extern "C"
