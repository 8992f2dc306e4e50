// MI355X (gfx950 / CDNA4) health canary, part 5: the two storage arrays next to the ALUs.
//
// Every other canary kernel keeps a few dozen registers per lane, and the L2 march reads
// with non-temporal loads precisely to bypass the CU's vector L1.  Two kernels, both grids
// of 4-wave workgroups (one wave per SIMD) that record their site as the site probe does:
//
//   * reg_march: each lane keeps kNV values pinned in VGPRs and kNA values pinned in AGPRs,
//     all live at once, so a wave is allocated its SIMD's whole 512-entry register file
//     (occupancy 1).  Per repetition: write value i as base ^ K(i) (base a per-thread word,
//     K(i) a distinct odd multiple, so a wrong register index or lane is caught, not only a
//     stuck bit), verify all in ascending order, write the complement (computed from base,
//     not from what was read), verify in descending order, take a new base.  The values are
//     pinned with EMPTY asm statements whose only content is the operand constraint ("+v":
//     a VGPR, "+a": an AGPR): volatile asm statements keep their order, so every write
//     barrier precedes every verify barrier and all values are live between them.  base
//     passes the same barrier at the start of each phase; otherwise the expected values are
//     loop-invariant, get hoisted, and the live set doubles.  Which physical entries the
//     values occupy is the compiler's choice; that none of them lives in scratch memory is
//     checked at build time (tests/test_canary_cu.py reads the resource-usage remarks).
//   * l1_fill / l1_march: l1_fill writes an address-derived 16-B pattern; the kernel
//     boundary makes it visible and leaves the L1s cold.  l1_march workgroup b (one resident
//     per CU: it takes the largest dynamic LDS allocation) reads slice b with plain 16-B
//     loads, which allocate in the L1 (wrong words of this pass came from L2 or HBM and are
//     counted apart as fill errors), then re-reads the same bytes l1_reps times with plain
//     loads, alternately reversed and forward and with the wave <-> chunk assignment rotated,
//     so a wave reads lines another wave brought in.  A barrier and a compiler memory
//     barrier between passes make the loads issue again.
//
// Lane 0 of each wave adds to table[site] with vector atomics.  No spin-waits, no
// inter-workgroup communication, every loop bounded by a constant or an argument.
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

constexpr int kCuWaves = 4;      // waves per workgroup: one per SIMD of a CU
// Values each lane keeps pinned: 480 of the 512 entries.  At -O3 this builds with no scratch
// and 13 accumulator entries to spare; the other VGPRs hold base, the counters and
// temporaries.  240 / 248 still builds without scratch but takes every entry, and pairs in
// between (232 / 248) spill, so the margin is kept.
constexpr int kNV = 240, kNA = 240;
constexpr int kInjectLane = 3, kInjectBit = 9, kInjectVgpr = 5, kInjectAgpr = 7;

// K(i): (2i + 1) * odd is injective mod 2^32.  VGPR value i takes K(i), AGPR value i K(256 + i).
constexpr uint32_t reg_key(int i) { return (2u * static_cast<uint32_t>(i) + 1u) * 0x9E3779B1u; }

// fabric.hip's 16-B pattern under a seed of its own (unique per 16-B word of a <= 4 GiB buffer)
__device__ __forceinline__ u32x4 cu_pattern(uint64_t idx) {
  const uint32_t lo = static_cast<uint32_t>(idx), hi = static_cast<uint32_t>(idx >> 32);
  const uint32_t b = lo * 0x9E3779B1u ^ (hi + 0xC0DEu) * 0x85EBCA77u;
  u32x4 v = {b, b ^ 0xA5A5A5A5u, ~b, b * 3u + 0x6A09E667u};
  return v;
}

#define PIN_V(x) asm volatile("" : "+v"(x))
#define PIN_A(x) asm volatile("" : "+a"(x))

// counters[0] = reg_march waves that moved, counters[1] = their wrong words.  Waves with
// global index < inject_waves flip bit 9 of VGPR value 5 (inject_kind 0) or AGPR value 7
// (inject_kind 1) in lane 3 after the first write of repetition 0 (verifier self-test).
__global__ void __launch_bounds__(256) reg_march(int reps, int inject_kind, int inject_waves, uint32_t seed,
                                                 amdgpu_canary_cu_slot* __restrict__ table,
                                                 unsigned int* __restrict__ counters,
                                                 unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kCuWaves + (threadIdx.x >> 6);  // < 2^14 (host-checked)
  const bool inject = static_cast<int>(gw) < inject_waves && lane == kInjectLane;
  uint32_t base = mix32((static_cast<uint64_t>(seed) << 32) | (static_cast<uint64_t>(gw) << 6) |
                        static_cast<uint64_t>(lane));
  uint32_t v[kNV], a[kNA];
  uint32_t bad_v = 0, bad_a = 0;
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    const uint32_t flip_v = (inject && r == 0 && inject_kind == 0) ? (1u << kInjectBit) : 0u;
    const uint32_t flip_a = (inject && r == 0 && inject_kind == 1) ? (1u << kInjectBit) : 0u;
    PIN_V(base);  // 1: write
#pragma unroll
    for (int i = 0; i < kNV; ++i) {
      v[i] = base ^ reg_key(i);
      PIN_V(v[i]);
    }
#pragma unroll
    for (int i = 0; i < kNA; ++i) {
      a[i] = base ^ reg_key(256 + i);
      PIN_A(a[i]);
    }
    v[kInjectVgpr] ^= flip_v;
    PIN_V(v[kInjectVgpr]);
    a[kInjectAgpr] ^= flip_a;
    PIN_A(a[kInjectAgpr]);
    PIN_V(base);  // 2: verify, ascending
#pragma unroll
    for (int i = 0; i < kNV; ++i) {
      PIN_V(v[i]);
      bad_v += v[i] != (base ^ reg_key(i));
    }
#pragma unroll
    for (int i = 0; i < kNA; ++i) {
      PIN_A(a[i]);
      bad_a += a[i] != (base ^ reg_key(256 + i));
    }
    PIN_V(base);  // 3: write the complement, from base
#pragma unroll
    for (int i = 0; i < kNV; ++i) {
      v[i] = ~(base ^ reg_key(i));
      PIN_V(v[i]);
    }
#pragma unroll
    for (int i = 0; i < kNA; ++i) {
      a[i] = ~(base ^ reg_key(256 + i));
      PIN_A(a[i]);
    }
    PIN_V(base);  // 4: verify, descending
#pragma unroll
    for (int i = kNA - 1; i >= 0; --i) {
      PIN_A(a[i]);
      bad_a += a[i] != ~(base ^ reg_key(256 + i));
    }
#pragma unroll
    for (int i = kNV - 1; i >= 0; --i) {
      PIN_V(v[i]);
      bad_v += v[i] != ~(base ^ reg_key(i));
    }
    base = base * 0x85EBCA77u + 0x6A09E667u;  // 5
  }
  bad_v = wave_total(bad_v);
  bad_a = wave_total(bad_a);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  if (site_after == site) {
    amdgpu_canary_cu_slot* slot = table + site;  // site < kSiteSlots by the mask in site_id()
    atomicAdd(&slot->waves, 1u);
    if (bad_v) atomicAdd(&slot->bad_vgpr, bad_v);
    if (bad_a) atomicAdd(&slot->bad_agpr, bad_a);
  } else {
    atomicAdd(&counters[0], 1u);
    if (bad_v + bad_a) atomicAdd(&counters[1], bad_v + bad_a);
  }
}

#undef PIN_V
#undef PIN_A

// Workgroup b writes slice b (slice_words 16-B words) of buf.
__global__ void __launch_bounds__(256) l1_fill(u32x4* __restrict__ buf, int slice_words) {
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * slice_words;
  for (int i = threadIdx.x; i < slice_words; i += 256) buf[base + i] = cu_pattern(base + i);
}

__device__ __forceinline__ uint32_t wrong_words(const u32x4& got, const u32x4& want) {
  return (got[0] != want[0]) + (got[1] != want[1]) + (got[2] != want[2]) + (got[3] != want[3]);
}

// slice_words is a multiple of 256 (host-checked): the slice is slice_words / 64 chunks of
// 1 KiB, one wave-load each; in pass p wave w takes the chunks congruent to (w + p) mod 4,
// odd passes mirrored.  counters[2] = waves that moved, [3] = their wrong re-read words,
// [4] = wrong words of pass 1.  cu_waves[site >> 2] counts the located waves of each CU.
// The first inject_wgs workgroups flip bit 9 of the first word that lane 3 of wave 0 loaded
// in pass 2, in its register.  The dynamic LDS allocation is not used: its size keeps one
// workgroup per CU.
__global__ void __launch_bounds__(256) l1_march(const u32x4* buf, int slice_words, int l1_reps, int inject_wgs,
                                                amdgpu_canary_cu_slot* __restrict__ table,
                                                unsigned int* __restrict__ cu_waves,
                                                unsigned int* __restrict__ counters,
                                                unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kCuWaves + wave;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * slice_words;
  const int chunks = slice_words >> 6;
  const bool inject = static_cast<int>(blockIdx.x) < inject_wgs && threadIdx.x == kInjectLane;
  uint32_t bad_fill = 0, bad = 0;
  for (int p = 0; p <= l1_reps; ++p) {
    const int first = (wave + p) & 3;
    for (int c = first; c < chunks; c += kCuWaves) {
      int i = c * kWave + lane;        // < slice_words
      if (p & 1) i = slice_words - 1 - i;
      u32x4 got = buf[base + i];
      if (inject && p == 1 && c == first) got[0] ^= 1u << kInjectBit;
      const uint32_t n = wrong_words(got, cu_pattern(base + i));
      if (p == 0) bad_fill += n;
      else bad += n;
    }
    __syncthreads();  // every line of the slice has been brought in before anyone re-reads
    asm volatile("" ::: "memory");
  }
  bad = wave_total(bad);
  bad_fill = wave_total(bad_fill);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  if (bad_fill) atomicAdd(&counters[4], bad_fill);
  if (site_after == site) {
    atomicAdd(&cu_waves[site >> 2], 1u);
    if (bad) atomicAdd(&table[site].bad_l1, bad);
  } else {
    atomicAdd(&counters[2], 1u);
    if (bad) atomicAdd(&counters[3], bad);
  }
}

// Fills the located totals and the coverage counts of `r` from host copies of the tables.
void summarize(const amdgpu_canary_cu_slot* t, const unsigned int* cu_waves, amdgpu_canary_cu_result* r) {
  r->vgpr_errors = r->agpr_errors = r->l1_errors = r->waves = 0;
  r->l1_cus_reached = 0;
  for (int i = 0; i < kSiteSlots; ++i) {
    const amdgpu_canary_cu_slot& s = t[i];
    r->waves += s.waves;
    r->vgpr_errors += s.bad_vgpr;
    r->agpr_errors += s.bad_agpr;
    r->l1_errors += s.bad_l1;  // l1_march may add these at a site no reg_march wave stayed on: bad without a wave
  }
  for (int cu = 0; cu < kSiteSlots / 4; ++cu) r->l1_cus_reached += cu_waves[cu] > 0;
  store_coverage(site_coverage([&](int i) { return t[i].waves != 0; },
                               [&](int i) { return (t[i].bad_vgpr | t[i].bad_agpr | t[i].bad_l1) != 0; }),
                 r);
}

}  // namespace

extern "C" {

void amdgpu_canary_cu_regs(int* nv, int* na) {
  if (nv) *nv = kNV;
  if (na) *na = kNA;
}

int amdgpu_canary_cu_sizeof(int which) {
  return which == 0 ? static_cast<int>(sizeof(amdgpu_canary_cu_slot))
         : which == 1 ? static_cast<int>(sizeof(amdgpu_canary_cu_result))
                      : -1;
}

// The place of the first failing check (register, then l1) as the canary's error text;
// returns its length, 0 when neither failed.  Host only.
int amdgpu_canary_cu_describe(const amdgpu_canary_cu_result* r, const amdgpu_canary_cu_slot* table, char* buf,
                              int len) {
  const unsigned long long reg = r->vgpr_errors + r->agpr_errors + r->unlocated_errors;
  if (reg > 0) {
    int sites = 0, first = -1;
    for (int s = 0; s < kSiteSlots; ++s) {
      if ((table[s].bad_vgpr | table[s].bad_agpr) == 0) continue;
      if (first < 0) first = s;
      ++sites;
    }
    if (first < 0)  // every wave that saw one moved while it marched
      return std::snprintf(buf, len, "register check: %llu wrong words at an unknown site", reg);
    char where[48];
    format_site(static_cast<unsigned int>(first), true, where, sizeof(where));
    int n = std::snprintf(buf, len, "register check: %llu wrong words at %s (%s", reg, where,
                          r->vgpr_errors && r->agpr_errors ? "vgpr+agpr" : r->agpr_errors ? "agpr" : "vgpr");
    if (sites > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, "; +%d more site%s", sites - 1, sites > 2 ? "s" : "");
    if (n > 0 && n < len) n += std::snprintf(buf + n, len - n, ")");
    return n;
  }
  if (r->l1_errors > 0) {
    int cus = 0, first = -1;
    for (int cu = 0; cu < kSiteSlots / 4; ++cu) {
      if ((table[cu * 4].bad_l1 | table[cu * 4 + 1].bad_l1 | table[cu * 4 + 2].bad_l1 | table[cu * 4 + 3].bad_l1) == 0)
        continue;
      if (first < 0) first = cu;
      ++cus;
    }
    if (first < 0) return std::snprintf(buf, len, "l1 check: %llu wrong words at an unknown cu", r->l1_errors);
    char where[48];
    format_site(static_cast<unsigned int>(first) << 2, false, where, sizeof(where));
    int n = std::snprintf(buf, len, "l1 check: %llu wrong words at %s", r->l1_errors, where);
    if (cus > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more cu%s)", cus - 1, cus > 2 ? "s" : "");
    return n;
  }
  return 0;
}

// Runs both marches on `device`.  blocks == 0: 2 workgroups per CU, then up to 3 more
// launches of each kernel (new register operands, same tables) while the register march has
// reached fewer than multiProcessorCount CUs or 4 times as many SIMDs, or the L1 march fewer
// CUs; blocks > 0: one launch of that many workgroups.  inject_kind -1 none, 0 vgpr, 1 agpr
// (the first inject_waves waves), 2 l1 (the first inject_waves workgroups), first launch
// only.  table_out (kSiteSlots slots) and wave_site_out (2 * wave_site_len entries, see
// canary_common.h) may be null.  0, or -1 with `err` set.
int amdgpu_canary_cu(int device, int blocks, int reps, int l1_kb, int l1_reps, int inject_kind, int inject_waves,
                     amdgpu_canary_cu_slot* table_out, unsigned int* wave_site_out, int wave_site_len,
                     amdgpu_canary_cu_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  out->regs_vgpr = kNV;
  out->regs_agpr = kNA;
  if (blocks < 0 || blocks > kMaxBlocks || reps < 1 || reps > 64 || l1_kb < 4 || l1_kb > 32 || l1_kb % 4 != 0 ||
      l1_reps < 1 || l1_reps > 64 || inject_kind < -1 || inject_kind >= kCuInjectKinds || inject_waves < 0 ||
      wave_site_len < 0 || (wave_site_out == nullptr && wave_site_len != 0)) {
    std::snprintf(err, err_len,
                  "cu check: bad arguments (blocks %d in 0..%d, reps %d in 1..64, l1_kb %d a multiple of 4 in 4..32, "
                  "l1_reps %d in 1..64, inject %d/%d)",
                  blocks, kMaxBlocks, reps, l1_kb, l1_reps, inject_kind, inject_waves);
    return -1;
  }
  std::vector<amdgpu_canary_cu_slot> own_table(table_out ? 0 : kSiteSlots);
  amdgpu_canary_cu_slot* table = table_out ? table_out : own_table.data();
  std::vector<unsigned int> cu_waves(kSiteSlots / 4, 0);
  Status st;
  hipDeviceProp_t prop;
  unsigned int h_counters[5] = {0, 0, 0, 0, 0};
  DeviceBuffer<amdgpu_canary_cu_slot> d_table;
  DeviceBuffer<unsigned int> d_cu_waves, d_counters, d_wave_site;
  DeviceBuffer<u32x4> d_buf;
  Events<3> ev;
  const int slice_words = l1_kb * 64;  // 16-B words; a multiple of 256
  LaunchPlan plan = {0, 0};
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (st.ok()) plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
  const int grid = plan.grid;
  CANARY_HIP(st, d_buf.alloc(static_cast<size_t>(grid) * slice_words * sizeof(u32x4)));
  CANARY_HIP(st, d_table.alloc(sizeof(amdgpu_canary_cu_slot) * kSiteSlots));
  CANARY_HIP(st, d_table.zero());
  CANARY_HIP(st, d_cu_waves.alloc(sizeof(unsigned int) * cu_waves.size()));
  CANARY_HIP(st, d_cu_waves.zero());
  CANARY_HIP(st, d_counters.alloc(sizeof(h_counters)));
  CANARY_HIP(st, d_counters.zero());
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * 2 * static_cast<size_t>(wave_site_len)));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, ev.create());
  if (st.ok()) {
    out->cus_expected = prop.multiProcessorCount;
    for (int l = 0; l < plan.max_launches; ++l) {
      float ms[2] = {0, 0};  // reg_march; l1_fill and l1_march
      const int inj = l == 0 ? inject_kind : -1;
      time_stages(st, ev, ms, [&](int k) {
        if (k == 0) {
          st.stage("reg_march: ");
          hipLaunchKernelGGL(reg_march, dim3(grid), dim3(kCuWaves * kWave), 0, 0, reps, inj,
                             inj == 0 || inj == 1 ? inject_waves : 0, static_cast<uint32_t>(l), d_table.get(),
                             d_counters.get(), l == 0 ? d_wave_site.get() : nullptr, l == 0 ? wave_site_len : 0);
          return hipGetLastError();
        }
        if (l == 0) {  // the pattern does not change: one fill serves every launch
          st.stage("l1_fill: ");
          hipLaunchKernelGGL(l1_fill, dim3(grid), dim3(kCuWaves * kWave), 0, 0, d_buf.get(), slice_words);
          const hipError_t e = hipGetLastError();
          if (e != hipSuccess) return e;
        }
        if (launch_with_max_lds(l1_march, prop, dim3(grid), dim3(kCuWaves * kWave), d_buf.get(), slice_words, l1_reps,
                                inj == 2 ? inject_waves : 0, d_table.get(), d_cu_waves.get(), d_counters.get(),
                                l == 0 && d_wave_site.get() ? d_wave_site.get() + wave_site_len : nullptr,
                                l == 0 ? wave_site_len : 0))
          return hipSuccess;
        st.stage("l1_march launch: ");
        return hipErrorLaunchFailure;
      });
      st.stage("");
      CANARY_HIP(st, d_table.download(table));
      CANARY_HIP(st, d_cu_waves.download(cu_waves.data()));
      if (!st.ok()) break;
      out->reg_ms += ms[0];
      out->l1_ms += ms[1];
      out->launches = l + 1;
      summarize(table, cu_waves.data(), out);
      if (covered(*out, out->cus_expected) && out->l1_cus_reached >= out->cus_expected) break;
    }
  }
  CANARY_HIP(st, d_counters.download(h_counters));
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));
  out->moved = h_counters[0];
  out->unlocated_errors = h_counters[1];
  out->l1_moved = h_counters[2];
  out->l1_errors += h_counters[3];
  out->l1_fill_errors = h_counters[4];
  return st.report("cu check: ", err, err_len);
}

}  // extern "C"
