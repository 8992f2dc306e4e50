// MI355X (gfx950 / CDNA4) partition health canary.
//
// The reference has no device-level health check at all: its health channel has no
// producer (plugin/plugin.go:181, SURVEY.md defect D9).  Before a partition is
// advertised (and after a GPU_POST_RESET) the plugin can run this canary on it, in a
// short-lived child process so the plugin daemon itself never holds a HIP context:
//
//   1. HBM pattern test  - every 16-byte word gets an address-derived pattern
//      (catches stuck bits and aliasing/addressing faults), written and read back
//      with 16 B/lane vector accesses, block-contiguous chunks, 16 blocks per CU,
//      non-temporal loads on the verify pass (shapes chosen by the on-hardware sweep
//      in hbm.hip: ~6.0 TB/s write, ~6.8 TB/s read+verify on MI355X); mismatches are
//      reduced per wave (64-lane shuffles) then per block in LDS, one atomic/block.
//      Write and read passes are timed separately -> achieved HBM GB/s (hbm.hip).
//   2. MFMA exactness    - v_mfma_f32_32x32x16_bf16 on small-integer operands
//      (exact in bf16 and fp32) checked lane-by-lane against a scalar reference
//      using the documented gfx950 fragment maps (form_check<FormBf16>, mfma_forms.h).
//   3. MFMA throughput   - register-resident 32x32x16 bf16 MFMA chains, 4 waves
//      per block (one per SIMD), 8 blocks per CU -> dense bf16 TFLOP/s (rate_chain<FormBf16>).
//   4. Matrix path       - LDS-staged MFMA GEMM on exact integer data, ABFT-checked (gemm.hip).
//   5. fp8 / bf8 / fp4 MFMA exactness and rate, LDS march (datapath.hip).
//   6. Site probe        - MFMA and vector-ALU exactness on every CU and SIMD, with the
//      place of each mismatch (sites.hip).
//   7. Fabric check      - a march through each XCD's L2, a cross-XCD exchange and the
//      global atomics, errors attributed per xcc and per (writer, reader) pair (fabric.hip).
//   8. CU memory check   - a march over each SIMD's vector register file (VGPRs and AGPRs)
//      and re-reads through each CU's vector L1, located per SIMD / CU (cumem.hip).  Not part
//      of amdgpu_canary_run: canary.py's run() calls amdgpu_canary_cu and merges its result.
//
// This file holds the two MFMA probes (2, 3) and amdgpu_canary_run, which runs checks 1-7 in
// that order.  The C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py) is declared in
// canary_common.h, the host-side helpers in canary_host.h, the MFMA forms in mfma_forms.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "canary_host.h"

namespace {

using namespace canary;

// One wave per block runs the bf16 form's exactness check, K = 16 * ksteps.  Blocks below `inject_blocks`
// perturb one A operand: the fault injection that proves the verifier sees a wrong matrix-core result.
__global__ void __launch_bounds__(64) mfma_exact(int ksteps, int inject_blocks,
                                                 unsigned long long* __restrict__ errors) {
  const int lane = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  uint32_t bad = form_check<FormBf16>(blk, lane, ksteps, 0, static_cast<int>(blk) < inject_blocks);
  wave_sum(bad);
  if (lane == 0 && bad) atomicAdd(errors, static_cast<unsigned long long>(bad));
}

constexpr auto mfma_rate = rate_chain<FormBf16>;  // the kernel (mfma_forms.h)

}  // namespace

extern "C" {

int amdgpu_canary_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

// hbm_bytes: size of the pattern buffer (rounded down to 16 B); passes: timed
// write+verify repetitions; mfma_iters: MFMA pairs per wave for the rate test.
// A HIP error of this function's own steps is reported as "<the call or kernel>: <HIP's text>".
int amdgpu_canary_run(int device, unsigned long long hbm_bytes, int passes, int mfma_iters,
                      amdgpu_canary_result* out) {
  std::memset(out, 0, sizeof(*out));
  out->device = device;
  Status st;
  hipDeviceProp_t prop;
  DeviceBuffer<uint4> buf;
  DeviceBuffer<unsigned long long> d_err;  // [0] hbm, [1] mfma
  DeviceBuffer<float> sink;
  Events<3> ev;
  const uint64_t n = hbm_bytes / sizeof(uint4);
  unsigned long long h_err[2] = {0, 0};
  float t_write = 0, t_read = 0, t_mfma = 0;
  if (passes < 1) passes = 1;
  CANARY_HIP(st, hipSetDevice(device), "hipSetDevice: ");
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties: ");
  if (st.ok()) {
    out->num_cus = prop.multiProcessorCount;
    std::snprintf(out->arch, sizeof(out->arch), "%s", prop.gcnArchName);
    out->hbm_bytes = n * sizeof(uint4);
  }
  CANARY_HIP(st, buf.alloc(n * sizeof(uint4) + 16), "hipMalloc: ");
  CANARY_HIP(st, d_err.alloc(sizeof(h_err)), "hipMalloc: ");
  CANARY_HIP(st, d_err.zero(), "hipMemset: ");
  CANARY_HIP(st, ev.create(), "hipEventCreate: ");
  // 1. HBM pattern test
  if (st.ok()) hbm_passes(st, ev, prop, buf.get(), n, passes, d_err.get(), &t_write, &t_read);
  // 2. MFMA exactness: 2 * #CUs single-wave blocks, K = 16 * 32
  if (st.ok()) {
    st.stage("mfma_exact: ");
    hipLaunchKernelGGL(mfma_exact, dim3(prop.multiProcessorCount * 2), dim3(64), 0, 0, 32, 0, d_err.get() + 1);
    st.check(hipGetLastError());
  }
  // 3. MFMA rate
  CANARY_HIP(st, alloc_rate_sink(sink, rate_blocks(prop)), "hipMalloc: ");
  st.stage("mfma_rate: ");
  t_mfma = time_rate_launch(st, ev, mfma_rate, rate_blocks(prop), mfma_iters, sink.get());
  CANARY_HIP(st, d_err.download(h_err), "hipMemcpy: ");
  if (st.report("", out->error, sizeof(out->error)) != 0) return -1;
  out->hbm_errors = h_err[0];
  out->mfma_errors = h_err[1];
  out->write_gbps = static_cast<double>(n) * sizeof(uint4) * passes / (t_write * 1e-3) / 1e9;
  out->read_gbps = static_cast<double>(n) * sizeof(uint4) * passes / (t_read * 1e-3) / 1e9;
  out->mfma_tflops = rate_tflops<FormBf16>(mfma_iters, rate_blocks(prop), t_mfma);
  out->elapsed_ms = t_write + t_read + t_mfma;
  // 4. matrix path: HBM -> L2 -> LDS DMA -> ds_read -> MFMA, exact and checksummed.  4096^3
  // (256 tiles of 256x256: one per CU) takes ~0.5 ms; hbm_bytes < 256 MiB (fault-injection
  // runs) uses 1024^3 on the 128x128 kernel.
  {
    const int g = hbm_bytes >= (256ull << 20) ? 4096 : 1024;
    if (amdgpu_canary_gemm_rate(device, g, g, g, 4, 0, 0, &out->gemm_tflops, &out->gemm_errors, out->error,
                                sizeof(out->error)) != 0)
      return -1;
  }
  // 5. low-precision datapaths (fp8 / bf8 / fp4 MFMA) and the LDS
  {
    amdgpu_canary_datapath_result dp;
    if (amdgpu_canary_datapaths(device, mfma_iters / 4 > 0 ? mfma_iters / 4 : 1, &dp, out->error,
                                sizeof(out->error)) != 0)
      return -1;
    out->fp8_tflops = dp.fp8_tflops;
    out->fp4_tflops = dp.fp4_tflops;
    out->lowp_errors = dp.lowp_errors;
    out->lds_errors = dp.lds_errors;
    out->lds_bytes = dp.lds_bytes;
  }
  // 6. where the matrix cores and the vector ALU compute: every CU and SIMD, mismatches located
  {
    amdgpu_canary_sites_result sr;
    if (amdgpu_canary_sites(device, 0, 4, -1, 0, nullptr, nullptr, 0, &sr, out->error, sizeof(out->error)) != 0)
      return -1;
    out->site_errors = sr.errors[0] + sr.errors[1] + sr.errors[2] + sr.unlocated_errors;
    out->cus_reached = sr.cus_reached;
    out->simds_reached = sr.simds_reached;
    out->cus_unreached = sr.cus_expected > sr.cus_reached ? sr.cus_expected - sr.cus_reached : 0;
    out->site_ms = sr.ms;
    out->n_bad_sites = sr.n_bad;
    std::memcpy(out->bad_sites, sr.bad_sites, sizeof(out->bad_sites));
    if (out->site_errors > 0) sites_describe(sr, out->site_errors, out->error, sizeof(out->error));
  }
  // 7. between a CU and HBM: each XCD's L2, the path from one XCD to another, the global atomics
  {
    amdgpu_canary_xcc_slot xt[kFabricXccs];
    amdgpu_canary_pair_slot pm[kFabricXccs * kFabricXccs];
    amdgpu_canary_fabric_result fr;
    char ferr[256] = "";
    if (amdgpu_canary_fabric(device, 0, 64, 2, -1, 0, 0, xt, pm, nullptr, 0, &fr, ferr, sizeof(ferr)) != 0) {
      std::snprintf(out->error, sizeof(out->error), "%s", ferr);
      return -1;
    }
    out->l2_errors = fr.l2_errors;
    out->xcd_errors = fr.xcd_errors;
    out->atomic_errors = fr.atomic_errors;
    out->l2_gbps = fr.march_ms > 0 ? static_cast<double>(fr.march_read_bytes) / (fr.march_ms * 1e-3) / 1e9 : 0.0;
    out->fabric_ms = fr.march_ms + fr.exchange_ms + fr.atomic_ms;
    out->xccs_reached = fr.xccs_reached;
    out->xcd_pairs_reached = fr.pairs_reached;
    out->xcd_pairs_unreached = fr.pairs_expected > fr.pairs_reached ? fr.pairs_expected - fr.pairs_reached : 0;
    if (out->error[0] == 0) amdgpu_canary_fabric_describe(&fr, xt, pm, out->error, sizeof(out->error));
  }
  // (8, the CU memory check, is merged in by canary.py's run())
  out->ok = (out->hbm_errors == 0 && out->mfma_errors == 0 && out->gemm_errors == 0 && out->lowp_errors == 0 &&
             out->lds_errors == 0 && out->site_errors == 0 && out->l2_errors == 0 && out->xcd_errors == 0 &&
             out->atomic_errors == 0)
                ? 1
                : 0;
  return out->error[0] ? -1 : 0;
}

// Fault-injection check of the MFMA verifier: `inject_blocks` of the 2 * #CUs exactness
// blocks compute with one perturbed operand.  Returns the mismatching accumulator
// registers found (0 expected without injection), -1 on a HIP error.
long long amdgpu_canary_mfma_detects(int device, int inject_blocks) {
  if (inject_blocks < 0) return -1;
  return count_errors(device, [&](Status&, const hipDeviceProp_t& prop, unsigned long long* d_err) {
    hipLaunchKernelGGL(mfma_exact, dim3(prop.multiProcessorCount * 2), dim3(64), 0, 0, 32, inject_blocks, d_err);
  });
}

}  // extern "C"
