// MI355X (gfx950 / CDNA4) health canary, part 3: the site probe.
//
// The exactness kernels of canary.hip and datapath.hip are grids of single-wave blocks:
// nothing says that every CU takes one, a wave occupies one of a CU's four SIMDs (each
// with its own matrix core), and a mismatch is counted, never located.  site_probe runs
// the same kind of check as 4-wave workgroups that each take a CU's whole LDS, so one
// workgroup is resident per CU at a time, and every wave records where it ran:
//
//   * site_id(): (xcc, se, sh, cu, simd) from HW_REG_HW_ID bits 15:4 and HW_REG_XCC_ID
//     bits 3:0 (layout: hip/amd_detail/amd_device_functions.h above __smid()), packed into
//     14 bits (canary_common.h, site.h).  Read before and after the checks; a wave whose site
//     changed in between (context-switched to other hardware) is counted as moved and its
//     errors as unlocated.
//   * mfma: v_mfma_f32_32x32x16_bf16 on small integers: mfma_exact's form_check<FormBf16> (K = 16 * ksteps);
//   * lowp: v_mfma_scale_f32_32x32x64_f8f6f4 in fp8 with varied power-of-two block scales:
//     lowp_exact<fp8>'s form_check<FormScaled<kFp8>> of mfma_forms.h (K = 64 * ksteps);
//   * valu: a fixed per-lane chain of 32-bit multiply-add / shift / rotate, 64-bit add,
//     exact fp32 and fp64 FMA and a __shfl_xor butterfly, folded into one 32-bit digest
//     per lane and compared with digests the HOST computed with the same function: a
//     faulty SIMD cannot agree with itself.
//
// Lane 0 of each wave adds to table[site]; the host reads the table, counts the CUs and
// SIMDs reached and launches again (at most 3 more times) while some are missing.
// No spin-waits, no inter-workgroup communication, every loop bounded by a constant or an
// argument.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "canary_host.h"

namespace {

using namespace canary;

constexpr int kProbeWaves = 4;   // waves per workgroup: one per SIMD of a CU
constexpr int kValuRounds = 48;

// ---- valu chain: the same code on host and device ----------------------------------
struct valu_state {
  uint32_t x;
  uint64_t y;
};

__host__ __device__ inline uint32_t rotl32(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

__host__ __device__ inline valu_state valu_init(int lane) {
  return {0x6A09E667u + 0x9E3779B1u * static_cast<uint32_t>(lane), 0xBB67AE8584CAA73Bull + static_cast<uint64_t>(lane)};
}

// One round up to the cross-lane exchange.  fp32: 12-bit * 11-bit + 8-bit < 2^24; fp64:
// 24-bit * 24-bit + 20-bit < 2^53: every conversion, product and sum is exact.
__host__ __device__ inline void valu_round(valu_state& s, int lane, int round) {
  s.x = s.x * 0x85EBCA77u + static_cast<uint32_t>(lane * 64 + round);  // 32-bit multiply-add
  s.x = rotl32(s.x, 7) ^ (s.x >> 3) ^ (s.x << 5);                      // rotate, shifts
  s.y += (static_cast<uint64_t>(s.x) << 21) | static_cast<uint64_t>(round);  // 64-bit add
  const float f = __builtin_fmaf(static_cast<float>(s.x & 0xFFFu), static_cast<float>((s.x >> 12) & 0x7FFu),
                                 static_cast<float>(s.x >> 24));
  s.x ^= static_cast<uint32_t>(f);
  const double d = __builtin_fma(static_cast<double>(s.x & 0xFFFFFFu), static_cast<double>(s.y & 0xFFFFFFull),
                                 static_cast<double>((s.y >> 44) & 0xFFFFFull));
  s.y ^= static_cast<uint64_t>(d);
}

// fold in the x of lane ^ (1 << (round % 6))
__host__ __device__ inline void valu_fold(valu_state& s, uint32_t other) { s.x += rotl32(other, 13); }

__host__ __device__ inline uint32_t valu_digest(const valu_state& s) {
  return s.x ^ static_cast<uint32_t>(s.y) ^ static_cast<uint32_t>(s.y >> 32);
}

void valu_expected(uint32_t* digest) {  // the 64 lanes of one wave, shuffle emulated over an array
  valu_state s[kWave];
  for (int l = 0; l < kWave; ++l) s[l] = valu_init(l);
  for (int r = 0; r < kValuRounds; ++r) {
    uint32_t x[kWave];
    for (int l = 0; l < kWave; ++l) {
      valu_round(s[l], l, r);
      x[l] = s[l].x;
    }
    for (int l = 0; l < kWave; ++l) valu_fold(s[l], x[l ^ (1 << (r % 6))]);
  }
  for (int l = 0; l < kWave; ++l) digest[l] = valu_digest(s[l]);
}

// ---- the valu check: wrong results this lane sees (the MFMA checks: form_check, mfma_forms.h) ----
__device__ __forceinline__ uint32_t check_valu(int lane, const uint32_t* __restrict__ expect, bool inject) {
  valu_state s = valu_init(lane);
  if (inject && lane == 0) s.x ^= 1u;
  for (int r = 0; r < kValuRounds; ++r) {
    valu_round(s, lane, r);
    valu_fold(s, __shfl_xor(s.x, 1 << (r % 6), kWave));
  }
  return valu_digest(s) != expect[lane];
}

// counters[0] = waves that moved, counters[1] = their wrong results.  Waves with global
// index < inject_waves perturb one operand of check `inject_check` (verifier self-test).
// The dynamic LDS allocation is not used: its size keeps one workgroup per CU.
__global__ void __launch_bounds__(256) site_probe(int ksteps, int inject_check, int inject_waves, uint32_t seed,
                                                  const uint32_t* __restrict__ expect,
                                                  amdgpu_canary_site_slot* __restrict__ table,
                                                  unsigned int* __restrict__ counters,
                                                  unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kProbeWaves + (threadIdx.x >> 6);  // < 2^14 (host-checked)
  const uint32_t key = gw | (seed << 14);
  const bool inject = static_cast<int>(gw) < inject_waves;
  uint32_t bad[kSiteChecks];
  bad[0] = wave_total(form_check<FormBf16>(key, lane, ksteps, 0, inject && inject_check == 0));
  bad[1] = wave_total(form_check<FormScaled<kFp8>>(key, lane, ksteps, 1, inject && inject_check == 1));
  bad[2] = wave_total(check_valu(lane, expect, inject && inject_check == 2));
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  if (site_after == site) {
    amdgpu_canary_site_slot* slot = table + site;  // site < kSiteSlots by the mask in site_id()
    atomicAdd(&slot->waves, 1u);
    for (int c = 0; c < kSiteChecks; ++c)
      if (bad[c]) atomicAdd(&slot->bad[c], bad[c]);
  } else {
    atomicAdd(&counters[0], 1u);
    if (bad[0] + bad[1] + bad[2]) atomicAdd(&counters[1], bad[0] + bad[1] + bad[2]);
  }
}

// Fills the totals and the coverage counts of `r` from a host copy of the table.
void summarize(const amdgpu_canary_site_slot* t, amdgpu_canary_sites_result* r) {
  for (int c = 0; c < kSiteChecks; ++c) r->errors[c] = 0;
  r->waves = 0;
  for (int i = 0; i < kSiteSlots; ++i) {
    const amdgpu_canary_site_slot& s = t[i];
    if (s.waves == 0) continue;  // errors are only ever added together with a wave
    r->waves += s.waves;
    for (int c = 0; c < kSiteChecks; ++c) r->errors[c] += s.bad[c];
  }
  store_coverage(site_coverage([&](int i) { return t[i].waves != 0; },
                               [&](int i) { return t[i].waves != 0 && (t[i].bad[0] | t[i].bad[1] | t[i].bad[2]) != 0; }),
                 r);
}

}  // namespace

extern "C" {

// Runs the site probe on `device`.  blocks == 0: 2 workgroups per CU, then up to 3 more
// launches (new operands, same table) while fewer than multiProcessorCount CUs or 4 times
// as many SIMDs have been reached; blocks > 0: one launch of that many workgroups.
// table_out (kSiteSlots slots) and wave_site_out (the starting site of the first
// wave_site_len waves of the first launch) may be null.  0, or -1 with `err` set.
int amdgpu_canary_sites(int device, int blocks, int ksteps, int inject_check, int inject_waves,
                        amdgpu_canary_site_slot* table_out, unsigned int* wave_site_out, int wave_site_len,
                        amdgpu_canary_sites_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  if (blocks < 0 || blocks > kMaxBlocks || ksteps < 1 || ksteps > 64 || inject_check < -1 ||
      inject_check >= kSiteChecks || inject_waves < 0 || wave_site_len < 0 ||
      (wave_site_out == nullptr && wave_site_len != 0)) {
    std::snprintf(err, err_len, "site probe: bad arguments (blocks %d <= %d, ksteps %d in 1..64, inject %d/%d)", blocks,
                  kMaxBlocks, ksteps, inject_check, inject_waves);
    return -1;
  }
  std::vector<amdgpu_canary_site_slot> own_table(table_out ? 0 : kSiteSlots);
  amdgpu_canary_site_slot* table = table_out ? table_out : own_table.data();
  Status st;
  hipDeviceProp_t prop;
  uint32_t h_expect[kWave];
  unsigned int h_counters[2] = {0, 0};
  DeviceBuffer<uint32_t> d_expect;
  DeviceBuffer<amdgpu_canary_site_slot> d_table;
  DeviceBuffer<unsigned int> d_counters, d_wave_site;
  Events<2> ev;
  valu_expected(h_expect);
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  CANARY_HIP(st, d_expect.alloc(sizeof(h_expect)));
  CANARY_HIP(st, d_expect.upload(h_expect));
  CANARY_HIP(st, d_table.alloc(sizeof(amdgpu_canary_site_slot) * kSiteSlots));
  CANARY_HIP(st, d_table.zero());
  CANARY_HIP(st, d_counters.alloc(sizeof(h_counters)));
  CANARY_HIP(st, d_counters.zero());
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * wave_site_len));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, ev.create());
  if (st.ok()) {
    out->cus_expected = prop.multiProcessorCount;
    const LaunchPlan plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
    const int grid = plan.grid;
    for (int l = 0; l < plan.max_launches; ++l) {
      float ms[1] = {0};
      time_stages(st, ev, ms, [&](int) {
        if (launch_with_max_lds(site_probe, prop, dim3(grid), dim3(kProbeWaves * kWave), ksteps,
                                l == 0 ? inject_check : -1, l == 0 ? inject_waves : 0, static_cast<uint32_t>(l),
                                d_expect.get(), d_table.get(), d_counters.get(),
                                l == 0 ? d_wave_site.get() : nullptr, l == 0 ? wave_site_len : 0))
          return hipSuccess;
        st.stage("launch: ");
        return hipErrorLaunchFailure;
      });
      CANARY_HIP(st, d_table.download(table));
      if (!st.ok()) break;
      out->ms += ms[0];
      out->launches = l + 1;
      summarize(table, out);
      if (covered(*out, out->cus_expected)) break;
    }
  }
  CANARY_HIP(st, d_counters.download(h_counters));
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));
  out->moved = h_counters[0];
  out->unlocated_errors = h_counters[1];
  return st.report("site probe: ", err, err_len);
}

// "xcc3/se1/sh0/cu7/simd2" of a packed site
int amdgpu_canary_format_site(unsigned int site, char* buf, int len) { return format_site(site, true, buf, len); }

}  // extern "C"

int canary::sites_describe(const amdgpu_canary_sites_result& r, unsigned long long errors, char* buf, int len) {
  char where[64] = "an unknown site";  // every wrong wave moved while it ran
  if (r.n_bad > 0) format_site(r.bad_sites[0], true, where, sizeof(where));
  int n = std::snprintf(buf, len, "site check: %llu wrong results at %s", errors, where);
  if (r.n_bad > 1 && n > 0 && n < len)
    n += std::snprintf(buf + n, len - n, " (+%d more site%s)", r.n_bad - 1, r.n_bad > 2 ? "s" : "");
  return n;
}
