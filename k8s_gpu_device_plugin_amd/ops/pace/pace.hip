// MI355X (gfx950 / CDNA4) health canary: the pace check.
//
// Every other check asks whether a partition computes and stores correctly, and three
// device-wide averages say how fast.  This one locates slowness the way the site probe
// locates wrong results: 4-wave workgroups (one wave per SIMD), one resident per CU through
// the largest dynamic LDS allocation, every wave reading its site (canary_common.h) first and
// last.  Each wave brackets its work with the two counters a wave can read,
//
//   * __builtin_amdgcn_s_memtime():     the shader clock, one tick per cycle the XCD ran;
//   * __builtin_amdgcn_s_memrealtime(): a constant-rate counter (hipDeviceAttributeWallClockRate),
//
// and lane 0 leaves one 32-byte record (pace_host.h) in its own slot, records[block * 4 + wave],
// with ordinary vector stores after the work.  No kernel reads the record buffer, and no
// stamp value feeds a computed result; the verdicts are the host's (pace_host.h).
//
//   * pace_mfma: `iters` iterations of four independent v_mfma_f32_32x32x16_bf16 accumulator
//     chains on the small integers of a_val / b_val, the operands fixed over the loop, so
//     every accumulator ends as iters x (A . B), which each lane then compares (a wrong MFMA
//     is still an error, located like the site probe's, and the loop cannot be shortened).
//     cycles / work is the cycles one SIMD needed per MFMA: 32 by the hardware's issue rate;
//     cycles / ticks is the clock the XCD ran.
//   * pace_fill, pace_mem: the fill writes hbm.hip's address-derived pattern under a seed of
//     its own; after the kernel boundary workgroup b streams slice b with 16-B non-temporal
//     loads, four in flight per lane, compares every word, and stamps around the whole read
//     (a barrier before the second stamp: the time is the workgroup's).  ticks per MiB is the
//     memory time of the XCD the workgroup ran on.
//
// Fault injection perturbs work counts and compared values, never an address.  No
// spin-waits, no inter-workgroup communication, every loop bounded by an argument.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/pace.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pace.h"

namespace {

using namespace canary;

constexpr int kThreads = kPaceWaves * kWave;
constexpr int kChains = 4;      // independent accumulator chains per wave
constexpr int kMemUnroll = 4;   // 16-B loads a lane keeps in flight
constexpr int kInjectLane = 3;
constexpr uint32_t kPaceSeed = 0x9ACEu;
// 2 workgroups per CU take turns on a CU, so a launch lasts two waves' loops: 0.5 ms at
// 32 cycles per MFMA and 2.4 GHz is 0.5e-3 * 2.4e9 / (2 * 4 * 32) = 4687 iterations, 4096 as
// a power of two.  Measured on an MI355X (docs/CANARY.md, "Pace", Measured) 4096 took 0.78 ms:
// the chip held 1.83-1.93 GHz in the loop, not 2.4 (0.56 ms for the two loops), and operand
// set-up, the closed-form compare and the launch itself add 0.22 ms that do not scale with
// iters.  0.5 ms less that leaves 0.28 ms of loop, which is 2048 iterations.
constexpr int kDefaultIters = 2048;

// hbm.hip's 16-B pattern under this stage's seed (unique per 16-B word of a <= 64 GiB buffer)
__device__ __forceinline__ u32x4 pace_pattern(uint64_t idx) {
  const uint32_t lo = static_cast<uint32_t>(idx), hi = static_cast<uint32_t>(idx >> 32);
  const uint32_t b = lo * 0x9E3779B1u ^ (hi + kPaceSeed) * 0x85EBCA77u;
  u32x4 v = {b, b ^ 0xA5A5A5A5u, ~b, b * 3u + 0x6A09E667u};
  return v;
}

__device__ __forceinline__ uint32_t wrong_words(const u32x4& got, const u32x4& want) {
  return (got[0] != want[0]) + (got[1] != want[1]) + (got[2] != want[2]) + (got[3] != want[3]);
}

// Lane 0 of a wave, after the work.
__device__ __forceinline__ void write_record(amdgpu_pace_record* __restrict__ rec, uint32_t site, uint32_t site_after,
                                             uint64_t cycles, uint64_t ticks, uint32_t work, uint32_t bad) {
  rec->site_first = site;
  rec->site_last = site_after;
  rec->cycles = cycles;
  rec->ticks = ticks;
  rec->work = work;
  rec->bad = bad;
}

#define PIN_V(x) asm volatile("" : "+v"(x))

// One wave per SIMD.  `iters` iterations of four MFMAs between the stamps, recorded as
// work = 4 * iters.  inject_kind 0: a wave that reads xcc inject_xcc runs inject_factor
// times as many (and checks against that true count); 1: so do the waves with global index
// < inject_waves; 2: lane 3 of those waves adds 1 to one operand element of the last MFMA.
// The host keeps iters * inject_factor below 2^16, so every accumulator stays below 2^24.
// The dynamic LDS allocation is not used: its size keeps one workgroup per CU.
__global__ void __launch_bounds__(kThreads) pace_mfma(int iters, int inject_kind, int inject_xcc, int inject_factor,
                                                      int inject_waves, uint32_t seed,
                                                      amdgpu_pace_record* __restrict__ records,
                                                      unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kPaceWaves + (threadIdx.x >> 6);  // < 2^14 (host-checked)
  const uint32_t key = gw | (seed << 14);
  const int r = lane & 31, h = lane >> 5;
  const bool first_waves = static_cast<int>(gw) < inject_waves;
  const bool slow = (inject_kind == kPaceInjectSlowXcc && static_cast<int>(site >> 10) == inject_xcc) ||
                    (inject_kind == kPaceInjectSlowWaves && first_waves);
  // the true count; the same in every lane of a wave, so the loop counter is scalar
  const int n = __builtin_amdgcn_readfirstlane(slow ? iters * inject_factor : iters);
  bf16x8 a[kChains], b[kChains];
#pragma unroll
  for (int c = 0; c < kChains; ++c) {
    const uint32_t blk = key | (static_cast<uint32_t>(c) << 16);
    for (int j = 0; j < 8; ++j) {  // lane l holds A[r][8h+j], B[8h+j][r]
      a[c][j] = bf16_of_int(a_val(blk, r, 8 * h + j));
      b[c][j] = bf16_of_int(b_val(blk, 8 * h + j, r));
    }
  }
  bf16x8 a_last = a[kChains - 1];
  if (inject_kind == kPaceInjectResult && first_waves && lane == kInjectLane)
    a_last[0] = bf16_of_int(a_val(key | (static_cast<uint32_t>(kChains - 1) << 16), r, 8 * h) + 1);
  f32x16 acc0 = zero_f32x16(), acc1 = zero_f32x16(), acc2 = zero_f32x16(), acc3 = zero_f32x16();
  PIN_V(a_last);  // the operands are ready before the first stamp
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  PIN_V(acc0);  // after the stamps: what depends on these values cannot start before them
  PIN_V(acc1);
  PIN_V(acc2);
  PIN_V(acc3);
  for (int i = 1; i < n; ++i) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[2], acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[3], b[3], acc3, 0, 0, 0);
  }
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc1, 0, 0, 0);
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[2], acc2, 0, 0, 0);
  acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_last, b[3], acc3, 0, 0, 0);
  PIN_V(acc0);  // the last results land before the second stamp
  PIN_V(acc1);
  PIN_V(acc2);
  PIN_V(acc3);
  // ... and one of them is read: the read waits for the last MFMA to finish, not only to issue
  int landed = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc3[15]));
  asm volatile("" : "+s"(landed));
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t site_after = site_id();
  // closed form: every accumulator is n x (A . B) over the 16 k of one MFMA
  const f32x16 acc[kChains] = {acc0, acc1, acc2, acc3};
  uint32_t bad = 0;
#pragma unroll
  for (int c = 0; c < kChains; ++c) {
    const uint32_t blk = key | (static_cast<uint32_t>(c) << 16);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = cd_row32(reg, h);
      int dot = 0;
#pragma unroll 1
      for (int k = 0; k < 16; ++k) dot += a_val(blk, row, k) * b_val(blk, k, r);
      bad += acc[c][reg] != static_cast<float>(n * dot);
    }
  }
  bad = wave_total(bad);
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  write_record(records + gw, site, site_after, c1 - c0, t1 - t0, static_cast<uint32_t>(kChains * iters), bad);
}

#undef PIN_V

// Grid-stride fill of n 16-B words.
__global__ void __launch_bounds__(256) pace_fill(u32x4* __restrict__ buf, uint64_t n) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += step) buf[i] = pace_pattern(i);
}

// Workgroup b streams slice b: slice_words 16-B words, a multiple of 256 (host-checked), in
// tiles of 256 * kMemUnroll and a tail of whole rows of 256.  A workgroup whose xcc is
// inject_xcc (-1: none) reads its slice inject_factor times and records one slice's bytes.
// buf is not __restrict__: a repeated read must load again.
__global__ void __launch_bounds__(kThreads) pace_mem(const u32x4* buf, int slice_words, int inject_xcc, int inject_factor,
                                                     amdgpu_pace_record* __restrict__ records,
                                                     unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kPaceWaves + (threadIdx.x >> 6);
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * static_cast<uint64_t>(slice_words);
  const int reps = static_cast<int>(site >> 10) == inject_xcc ? inject_factor : 1;
  constexpr int tile = 256 * kMemUnroll;
  uint32_t bad = 0;
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  asm volatile("" ::: "memory");
  for (int rep = 0; rep < reps; ++rep) {
    int w0 = 0;
    for (; w0 + tile <= slice_words; w0 += tile) {
      u32x4 v[kMemUnroll];
#pragma unroll
      for (int u = 0; u < kMemUnroll; ++u) v[u] = __builtin_nontemporal_load(buf + base + w0 + u * 256 + threadIdx.x);
#pragma unroll
      for (int u = 0; u < kMemUnroll; ++u) bad += wrong_words(v[u], pace_pattern(base + w0 + u * 256 + threadIdx.x));
    }
    for (int i = w0 + threadIdx.x; i < slice_words; i += 256)
      bad += wrong_words(__builtin_nontemporal_load(buf + base + i), pace_pattern(base + i));
    asm volatile("" ::: "memory");  // the next repetition loads again
  }
  bad = wave_total(bad);
  __syncthreads();  // every wave's part of the slice has arrived
  asm volatile("" ::: "memory");
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  write_record(records + gw, site, site_after, c1 - c0, t1 - t0, static_cast<uint32_t>(slice_words) * 16u, bad);
}

void bad_arguments(char* err, int err_len, int blocks, int iters, int slice_kb, double slow_ratio, int inject_kind,
                   int inject_xcc, int inject_factor, int inject_waves) {
  std::snprintf(err, err_len,
                "pace check: bad arguments (blocks %d in 0..%d, iters %d in 1..%d with the injected factor, slice_kb %d a "
                "multiple of 4 in 4..%d and at most 4 GiB in all, slow_ratio %g >= 1, inject %d/%d/%d/%d)",
                blocks, pace::kMaxBlocks, iters, pace::kMaxIters, slice_kb, pace::kMaxSliceKb, slow_ratio, inject_kind,
                inject_xcc, inject_factor, inject_waves);
}

}  // namespace

extern "C" {

int amdgpu_pace_sizeof(int which) {
  return which == 0   ? static_cast<int>(sizeof(amdgpu_pace_record))
         : which == 1 ? static_cast<int>(sizeof(amdgpu_pace_site_slot))
         : which == 2 ? static_cast<int>(sizeof(amdgpu_pace_xcc_slot))
         : which == 3 ? static_cast<int>(sizeof(amdgpu_pace_result))
                      : -1;
}

int amdgpu_pace_default_iters() { return kDefaultIters; }

int amdgpu_pace_reduce(const amdgpu_pace_record* mfma, int n_mfma, const amdgpu_pace_record* mem, int n_mem,
                       double tick_mhz, double clock_max_mhz, double slow_ratio, amdgpu_pace_site_slot* sites_out,
                       amdgpu_pace_xcc_slot* xccs_out, amdgpu_pace_result* result) {
  if (result == nullptr) return -1;
  std::memset(result, 0, sizeof(*result));
  std::vector<amdgpu_pace_site_slot> own_sites(sites_out ? 0 : kPaceSiteSlots);
  amdgpu_pace_xcc_slot own_xccs[kPaceXccs];
  return pace::reduce(mfma, n_mfma, mem, n_mem, tick_mhz, clock_max_mhz, slow_ratio,
                      sites_out ? sites_out : own_sites.data(), xccs_out ? xccs_out : own_xccs, result)
             ? 0
             : -1;
}

int amdgpu_pace_describe(const amdgpu_pace_result* r, const amdgpu_pace_xcc_slot* xccs, char* buf, int len) {
  return pace::describe(*r, xccs, buf, len);
}

int amdgpu_pace_note(const amdgpu_pace_result* r, const amdgpu_pace_xcc_slot* xccs, const amdgpu_pace_site_slot* sites,
                     char* buf, int len) {
  return pace::note(*r, xccs, sites, buf, len);
}

int amdgpu_pace_run(int device, int blocks, int iters, int slice_kb, double slow_ratio, int inject_kind, int inject_xcc,
                    int inject_factor, int inject_waves, amdgpu_pace_site_slot* sites_out,
                    amdgpu_pace_xcc_slot* xccs_out, unsigned int* wave_site_out, int wave_site_len,
                    amdgpu_pace_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  if (!pace::arguments_ok(blocks, iters, slice_kb, slow_ratio, inject_kind, inject_xcc, inject_factor, inject_waves,
                          wave_site_len, wave_site_out != nullptr)) {
    bad_arguments(err, err_len, blocks, iters, slice_kb, slow_ratio, inject_kind, inject_xcc, inject_factor, inject_waves);
    return -1;
  }
  std::vector<amdgpu_pace_site_slot> own_sites(sites_out ? 0 : kPaceSiteSlots);
  amdgpu_pace_site_slot* sites = sites_out ? sites_out : own_sites.data();
  amdgpu_pace_xcc_slot own_xccs[kPaceXccs];
  amdgpu_pace_xcc_slot* xccs = xccs_out ? xccs_out : own_xccs;
  Status st;
  hipDeviceProp_t prop;
  int wall_khz = 0, clock_khz = 0;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  CANARY_HIP(st, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, device), "wall clock rate: ");
  CANARY_HIP(st, hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, device), "clock rate: ");
  if (!st.ok()) return st.report("pace check: ", err, err_len);
  if (wall_khz <= 0) {
    std::snprintf(err, err_len, "pace check: the device reports no wall clock rate");
    return -1;
  }
  const double tick_mhz = wall_khz / 1000.0, clock_max_mhz = clock_khz > 0 ? clock_khz / 1000.0 : 0.0;
  const LaunchPlan plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
  const int grid = plan.grid, max_launches = plan.max_launches;
  const int mem_grid = launch_plan(blocks, prop.multiProcessorCount, 1).grid;
  const int slice_words = slice_kb * 64;  // a multiple of 256
  const uint64_t mem_words = static_cast<uint64_t>(mem_grid) * static_cast<uint64_t>(slice_words);
  if (mem_words * 16u > pace::kMaxMemBytes) {
    bad_arguments(err, err_len, blocks, iters, slice_kb, slow_ratio, inject_kind, inject_xcc, inject_factor, inject_waves);
    return -1;
  }
  const int slots = (grid > mem_grid ? grid : mem_grid) * kPaceWaves;
  out->cus_expected = prop.multiProcessorCount;
  out->iters = iters;
  out->slice_kb = slice_kb;
  out->blocks = grid;
  out->mem_blocks = mem_grid;

  DeviceBuffer<amdgpu_pace_record> d_records;
  DeviceBuffer<unsigned int> d_wave_site;
  DeviceBuffer<u32x4> d_buf;
  Events<3> ev;
  CANARY_HIP(st, d_records.alloc(sizeof(amdgpu_pace_record) * slots));
  CANARY_HIP(st, d_records.fill(0xFF));
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * 2 * wave_site_len));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, d_buf.alloc(mem_words * 16u));
  CANARY_HIP(st, ev.create());
  auto launch_failed = [&] {
    st.stage("launch: ");
    return hipErrorLaunchFailure;
  };
  // every kernel once over next to nothing, so no timed launch pays for loading its code
  st.stage("warm-up: ");
  if (st.ok()) {
    if (!launch_with_max_lds(pace_mfma, prop, dim3(1), dim3(kThreads), 1, -1, 0, 1, 0, 0u, d_records.get(),
                             static_cast<unsigned int*>(nullptr), 0))
      st.fail("warm-up launch: ");
    else if (!launch_with_max_lds(pace_mem, prop, dim3(1), dim3(kThreads), static_cast<const u32x4*>(d_buf.get()), 0, -1, 1,
                                  d_records.get(), static_cast<unsigned int*>(nullptr), 0))
      st.fail("warm-up launch: ");
    else
      hipLaunchKernelGGL(pace_fill, dim3(1), dim3(256), 0, 0, d_buf.get(), 0);
    CANARY_HIP(st, hipGetLastError());
    CANARY_HIP(st, hipDeviceSynchronize());
  }

  // stage 1: pace_mfma, topped up like the site probe
  std::vector<amdgpu_pace_record> h_mfma, h_mem(static_cast<size_t>(mem_grid) * kPaceWaves);
  h_mfma.reserve(static_cast<size_t>(max_launches) * grid * kPaceWaves);
  for (int l = 0; l < max_launches && st.ok(); ++l) {
    float ms[1] = {0};
    st.stage("pace_mfma: ");
    CANARY_HIP(st, d_records.fill(0xFF));
    time_stages(st, ev, ms, [&](int) {
      if (launch_with_max_lds(pace_mfma, prop, dim3(grid), dim3(kThreads), iters,
                              l == 0 || inject_kind == kPaceInjectSlowXcc ? inject_kind : -1, inject_xcc, inject_factor,
                              inject_waves, static_cast<uint32_t>(l), d_records.get(),
                              l == 0 ? d_wave_site.get() : nullptr, l == 0 ? wave_site_len : 0))
        return hipSuccess;
      return launch_failed();
    });
    const size_t have = h_mfma.size(), add = static_cast<size_t>(grid) * kPaceWaves;
    h_mfma.resize(have + add);
    CANARY_HIP(st, hipMemcpy(h_mfma.data() + have, d_records.get(), sizeof(amdgpu_pace_record) * add, hipMemcpyDeviceToHost));
    if (!st.ok()) break;
    out->mfma_ms += ms[0];
    out->launches = l + 1;
    amdgpu_pace_result cover = *out;
    if (!pace::reduce(h_mfma.data(), static_cast<int>(h_mfma.size()), nullptr, 0, tick_mhz, clock_max_mhz, slow_ratio,
                      sites, xccs, &cover)) {
      std::snprintf(err, err_len, "pace check: a record holds a site out of range");
      return -1;
    }
    if (covered(cover, out->cus_expected)) break;
  }

  // stage 2: the fill, then pace_mem
  if (st.ok()) {
    float ms[2] = {0, 0};
    st.stage("pace_mem: ");
    CANARY_HIP(st, d_records.fill(0xFF));
    const int fill_grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 8 : 8;
    time_stages(st, ev, ms, [&](int k) {
      if (k == 0) {
        hipLaunchKernelGGL(pace_fill, dim3(fill_grid), dim3(256), 0, 0, d_buf.get(), mem_words);
        return hipGetLastError();
      }
      if (launch_with_max_lds(pace_mem, prop, dim3(mem_grid), dim3(kThreads), static_cast<const u32x4*>(d_buf.get()),
                              slice_words, inject_kind == kPaceInjectSlowXcc ? inject_xcc : -1, inject_factor,
                              d_records.get(), wave_site_len > 0 ? d_wave_site.get() + wave_site_len : nullptr,
                              wave_site_len))
        return hipSuccess;
      return launch_failed();
    });
    CANARY_HIP(st, hipMemcpy(h_mem.data(), d_records.get(), sizeof(amdgpu_pace_record) * h_mem.size(), hipMemcpyDeviceToHost));
    out->fill_ms = ms[0];
    out->mem_ms = ms[1];
  }
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));
  if (!st.ok()) return st.report("pace check: ", err, err_len);
  if (!pace::reduce(h_mfma.data(), static_cast<int>(h_mfma.size()), h_mem.data(), static_cast<int>(h_mem.size()),
                    tick_mhz, clock_max_mhz, slow_ratio, sites, xccs, out)) {
    std::snprintf(err, err_len, "pace check: a record holds a site out of range");
    return -1;
  }
  return 0;
}

}  // extern "C"
