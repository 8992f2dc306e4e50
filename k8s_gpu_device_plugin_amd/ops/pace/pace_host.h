// The pace check's host side, shared by pace.hip and tests/native/pace_selftest.cpp: the
// record every wave leaves, the tables and the result the reduction fills, the reduction
// itself (located records -> per-site and per-XCD medians -> ratios, slow sites, slow XCDs)
// and the error and note texts.  The packed site, its text and the coverage walk are
// ../site.h's.  No HIP include: a plain C++17 compiler compiles it.
//
// Only differences within one wave are ever used (cycles and ticks are each the difference
// of two reads of one counter by one wave); nothing assumes that the counters of two XCDs agree.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../site.h"

extern "C" {

constexpr int kPaceXccs = 16;            // HW_REG_XCC_ID is 4 bits wide
constexpr int kPaceSiteSlots = kSiteSlots;  // packed sites (site.h)
constexpr int kPaceWaves = 4;            // waves per workgroup: records[block * 4 + wave]
constexpr unsigned int kPaceUnwritten = kSiteUnwritten;  // site_first of a slot no wave wrote

struct amdgpu_pace_record {  // what one wave leaves; 32 bytes
  unsigned int site_first;   // site_id() before the work
  unsigned int site_last;    // ... and after it
  unsigned long long cycles;  // difference of the shader-clock counter around the work
  unsigned long long ticks;   // difference of the constant-rate counter around the work
  unsigned int work;         // pace_mfma: MFMAs issued; pace_mem: bytes the workgroup read
  unsigned int bad;          // wrong result words the wave saw
};

struct amdgpu_pace_site_slot {  // one per packed site, MFMA stage
  double cycles_per_mfma;       // median over the site's located records of cycles / work (0: none timed)
  double clock_mhz;             // median of cycles / ticks * tick_mhz
  unsigned int waves;           // located records
  unsigned int bad;             // their wrong words
};

struct amdgpu_pace_xcc_slot {  // one per xcc
  double clock_mhz;            // median over the xcc's located MFMA records (0: none)
  double cycles_per_mfma;      // median of its sites' values
  double us_per_mib;           // median over its located memory workgroups (wave 0's record)
  unsigned int waves;          // located MFMA records
  unsigned int blocks;         // located memory workgroups
  unsigned long long bad_mfma;  // wrong accumulator words of its located waves
  unsigned long long bad_mem;   // wrong 32-bit words its located waves read
};

struct amdgpu_pace_result {
  unsigned long long mfma_errors;       // located wrong words of the MFMA stage
  unsigned long long mem_errors;        // located wrong words of the memory stage
  unsigned long long unlocated_errors;  // wrong words of waves (either stage) whose site changed
  unsigned long long pace_errors;       // the three together: what fails the check
  unsigned long long waves;             // located MFMA records
  unsigned long long moved;             // MFMA records whose site changed: timings dropped
  unsigned long long mem_waves;         // located memory records
  unsigned long long mem_moved;
  double tick_mhz;                      // rate of the constant counter
  double clock_max_mhz;                 // the part's maximum shader clock
  double slow_ratio;
  double clock_mhz_min;                 // over XCDs (0: no XCD timed)
  double clock_mhz_max;
  double clock_mhz_median;
  double clock_fraction;                // clock_mhz_min / clock_max_mhz
  double xcd_pace_ratio;                // slowest XCD clock / median over XCDs; 1 when balanced
  double xcd_mem_ratio;                 // median us_per_mib over XCDs / the largest; 1 when balanced
  double cycles_per_mfma_min;           // over sites
  double cycles_per_mfma_median;
  double cycles_per_mfma_max;
  double us_per_mib_median;             // over XCDs
  double us_per_mib_max;
  double mfma_ms;                       // device time of the pace_mfma launches
  double fill_ms;                       // device time of pace_fill
  double mem_ms;                        // device time of pace_mem
  int launches;                         // pace_mfma launches
  int cus_reached;                      // distinct (xcc, se, sh, cu) with a located MFMA record
  int simds_reached;                    // distinct sites with one
  int cus_expected;                     // multiProcessorCount (0 from the bare reduction)
  int mem_cus_reached;                  // distinct CUs with a located memory record
  int xccs_reached;                     // XCDs with a timed MFMA record
  int mem_xccs_reached;                 // XCDs with a timed memory workgroup
  int pace_xcc;                         // the XCD with the lowest clock (-1: fewer than two XCDs)
  int mem_xcc;                          // the XCD with the largest us_per_mib (-1: fewer than two)
  int n_bad;                            // sites with a wrong MFMA result
  unsigned int bad_sites[16];           // the first 16 of them, packed
  int n_slow;                           // sites above slow_ratio x the median cycles per MFMA
  unsigned int slow_sites[16];          // the first 16 of them, packed
  unsigned int slow_xccs_clock;         // bit x: xcc x ran below the median clock / slow_ratio
  unsigned int slow_xccs_cycles;        // bit x: its cycles per MFMA exceed the median x slow_ratio
  unsigned int slow_xccs_mem;           // bit x: its us_per_mib exceeds the median x slow_ratio
  int iters;                            // as run (0 from the bare reduction)
  int slice_kb;
  int blocks;                           // grid of one pace_mfma launch
  int mem_blocks;                       // grid of pace_mem
};

}  // extern "C"

namespace pace {

using canary::format_site;
using canary::located;
using canary::plural;
using canary::records_valid;

constexpr double kMiB = 1048576.0;

// Median of v (reordered): the middle element, or the mean of the two middle ones; 0 if empty.
inline double median(std::vector<double>& v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2;
}

inline bool timed(const amdgpu_pace_record& r) { return r.ticks > 0 && r.cycles > 0 && r.work > 0; }

// The reduction.  mfma / mem: n_mfma / n_mem records in launch order (records[block * 4 + wave]
// within a launch; unwritten slots are skipped); either may be empty.  sites (kPaceSiteSlots)
// and xccs (kPaceXccs) are filled; out keeps cus_expected, the ms, launches, iters, slice_kb,
// blocks and mem_blocks the caller set and gets everything else.  false: a bad argument.
inline bool reduce(const amdgpu_pace_record* mfma, int n_mfma, const amdgpu_pace_record* mem, int n_mem,
                   double tick_mhz, double clock_max_mhz, double slow_ratio, amdgpu_pace_site_slot* sites,
                   amdgpu_pace_xcc_slot* xccs, amdgpu_pace_result* out) {
  if (n_mfma < 0 || n_mem < 0 || (n_mfma > 0 && mfma == nullptr) || (n_mem > 0 && mem == nullptr) ||
      !(tick_mhz > 0) || !(clock_max_mhz >= 0) || !(slow_ratio >= 1) || sites == nullptr || xccs == nullptr ||
      out == nullptr || n_mem % kPaceWaves != 0 || !records_valid(mfma, n_mfma) || !records_valid(mem, n_mem))
    return false;
  std::memset(sites, 0, sizeof(*sites) * kPaceSiteSlots);
  std::memset(xccs, 0, sizeof(*xccs) * kPaceXccs);
  amdgpu_pace_result r = *out;
  r.mfma_errors = r.mem_errors = r.unlocated_errors = r.pace_errors = 0;
  r.waves = r.moved = r.mem_waves = r.mem_moved = 0;
  r.tick_mhz = tick_mhz;
  r.clock_max_mhz = clock_max_mhz;
  r.slow_ratio = slow_ratio;
  r.clock_mhz_min = r.clock_mhz_max = r.clock_mhz_median = r.clock_fraction = 0;
  r.cycles_per_mfma_min = r.cycles_per_mfma_median = r.cycles_per_mfma_max = 0;
  r.us_per_mib_median = r.us_per_mib_max = 0;
  r.xcd_pace_ratio = r.xcd_mem_ratio = 1.0;
  r.cus_reached = r.simds_reached = r.mem_cus_reached = r.xccs_reached = r.mem_xccs_reached = 0;
  r.pace_xcc = r.mem_xcc = -1;
  r.n_bad = r.n_slow = 0;
  std::memset(r.bad_sites, 0, sizeof(r.bad_sites));
  std::memset(r.slow_sites, 0, sizeof(r.slow_sites));
  r.slow_xccs_clock = r.slow_xccs_cycles = r.slow_xccs_mem = 0;

  // ---- MFMA stage: located records by site ----
  std::vector<int> order;  // indices of the located, timed records, grouped by site below
  order.reserve(n_mfma);
  for (int i = 0; i < n_mfma; ++i) {
    const amdgpu_pace_record& rec = mfma[i];
    if (rec.site_first == kPaceUnwritten) continue;
    if (!located(rec)) {
      ++r.moved;
      r.unlocated_errors += rec.bad;
      continue;
    }
    ++r.waves;
    r.mfma_errors += rec.bad;
    sites[rec.site_first].waves += 1;
    sites[rec.site_first].bad += rec.bad;
    xccs[rec.site_first >> 10].waves += 1;
    xccs[rec.site_first >> 10].bad_mfma += rec.bad;
    if (timed(rec)) order.push_back(i);
  }
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return mfma[a].site_first < mfma[b].site_first; });
  std::vector<double> v, w;
  std::vector<double> xcc_clock[kPaceXccs], xcc_cpm[kPaceXccs], all_cpm;
  for (size_t i = 0; i < order.size();) {
    const unsigned int site = mfma[order[i]].site_first;
    v.clear();
    w.clear();
    for (; i < order.size() && mfma[order[i]].site_first == site; ++i) {
      const amdgpu_pace_record& rec = mfma[order[i]];
      v.push_back(static_cast<double>(rec.cycles) / static_cast<double>(rec.work));
      const double mhz = static_cast<double>(rec.cycles) / static_cast<double>(rec.ticks) * tick_mhz;
      w.push_back(mhz);
      xcc_clock[site >> 10].push_back(mhz);
    }
    sites[site].cycles_per_mfma = median(v);
    sites[site].clock_mhz = median(w);
    xcc_cpm[site >> 10].push_back(sites[site].cycles_per_mfma);
    all_cpm.push_back(sites[site].cycles_per_mfma);
  }
  canary::store_coverage(canary::site_coverage([&](int s) { return sites[s].waves != 0; },
                                               [&](int s) { return sites[s].waves != 0 && sites[s].bad != 0; }),
                         &r);
  // slow sites: above slow_ratio x the median over sites
  if (!all_cpm.empty()) {
    r.cycles_per_mfma_median = median(all_cpm);  // sorts
    r.cycles_per_mfma_min = all_cpm.front();
    r.cycles_per_mfma_max = all_cpm.back();
    const double limit = slow_ratio * r.cycles_per_mfma_median;
    for (int s = 0; s < kPaceSiteSlots; ++s) {
      if (!(sites[s].cycles_per_mfma > limit)) continue;
      if (r.n_slow < 16) r.slow_sites[r.n_slow] = static_cast<unsigned int>(s);
      ++r.n_slow;
    }
  }
  // per XCD, then across XCDs
  std::vector<double> clocks, cpms;
  for (int x = 0; x < kPaceXccs; ++x) {
    if (xcc_clock[x].empty()) continue;
    xccs[x].clock_mhz = median(xcc_clock[x]);
    xccs[x].cycles_per_mfma = median(xcc_cpm[x]);
    clocks.push_back(xccs[x].clock_mhz);
    cpms.push_back(xccs[x].cycles_per_mfma);
    ++r.xccs_reached;
  }
  if (!clocks.empty()) {
    r.clock_mhz_median = median(clocks);  // sorts
    r.clock_mhz_min = clocks.front();
    r.clock_mhz_max = clocks.back();
    r.clock_fraction = clock_max_mhz > 0 ? r.clock_mhz_min / clock_max_mhz : 0.0;
  }
  if (r.xccs_reached > 1) {
    const double cpm_median = median(cpms);
    r.xcd_pace_ratio = r.clock_mhz_min / r.clock_mhz_median;
    for (int x = 0; x < kPaceXccs; ++x) {
      if (xcc_clock[x].empty()) continue;
      if (r.pace_xcc < 0 || xccs[x].clock_mhz < xccs[r.pace_xcc].clock_mhz) r.pace_xcc = x;
      if (xccs[x].clock_mhz < r.clock_mhz_median / slow_ratio) r.slow_xccs_clock |= 1u << x;
      if (xccs[x].cycles_per_mfma > cpm_median * slow_ratio) r.slow_xccs_cycles |= 1u << x;
    }
  }

  // ---- memory stage: bad of every located wave, time of wave 0 of each located workgroup ----
  std::vector<double> xcc_us[kPaceXccs];
  std::vector<unsigned char> cu_seen(kPaceSiteSlots / 4, 0);
  for (int i = 0; i < n_mem; ++i) {
    const amdgpu_pace_record& rec = mem[i];
    if (rec.site_first == kPaceUnwritten) continue;
    if (!located(rec)) {
      ++r.mem_moved;
      r.unlocated_errors += rec.bad;
      continue;
    }
    ++r.mem_waves;
    r.mem_errors += rec.bad;
    const int x = static_cast<int>(rec.site_first >> 10);
    xccs[x].bad_mem += rec.bad;
    if (!cu_seen[rec.site_first >> 2]) {
      cu_seen[rec.site_first >> 2] = 1;
      ++r.mem_cus_reached;
    }
    if (i % kPaceWaves != 0) continue;
    xccs[x].blocks += 1;
    if (timed(rec))
      xcc_us[x].push_back(static_cast<double>(rec.ticks) / tick_mhz / (static_cast<double>(rec.work) / kMiB));
  }
  std::vector<double> us;
  for (int x = 0; x < kPaceXccs; ++x) {
    if (xcc_us[x].empty()) continue;
    xccs[x].us_per_mib = median(xcc_us[x]);
    us.push_back(xccs[x].us_per_mib);
    ++r.mem_xccs_reached;
  }
  if (!us.empty()) {
    r.us_per_mib_median = median(us);  // sorts
    r.us_per_mib_max = us.back();
  }
  if (r.mem_xccs_reached > 1) {
    r.xcd_mem_ratio = r.us_per_mib_median / r.us_per_mib_max;
    for (int x = 0; x < kPaceXccs; ++x) {
      if (xcc_us[x].empty()) continue;
      if (r.mem_xcc < 0 || xccs[x].us_per_mib > xccs[r.mem_xcc].us_per_mib) r.mem_xcc = x;
      if (xccs[x].us_per_mib > r.us_per_mib_median * slow_ratio) r.slow_xccs_mem |= 1u << x;
    }
  }
  r.pace_errors = r.mfma_errors + r.mem_errors + r.unlocated_errors;
  *out = r;
  return true;
}

// The text of the first failing stage, in the house style:
//   "pace check: 3 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
//   "pace check: 2 wrong words read on xcc5 (+1 more xcc)"
//   "pace check: 4 wrong results at an unknown site"   (every wrong wave moved while it ran)
// Returns its length, 0 (and an empty text) if nothing failed.
inline int describe(const amdgpu_pace_result& r, const amdgpu_pace_xcc_slot* xccs, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  if (r.mfma_errors > 0 && r.n_bad > 0) {
    char where[64];
    format_site(r.bad_sites[0], true, where, sizeof(where));
    int n = std::snprintf(buf, len, "pace check: %llu wrong result%s at %s", r.mfma_errors, plural(r.mfma_errors), where);
    if (r.n_bad > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more site%s)", r.n_bad - 1, r.n_bad > 2 ? "s" : "");
    return n;
  }
  if (r.mem_errors > 0) {
    int first = -1, bad_xccs = 0;
    for (int x = 0; x < kPaceXccs; ++x) {
      if (xccs[x].bad_mem == 0) continue;
      if (first < 0) first = x;
      ++bad_xccs;
    }
    int n = std::snprintf(buf, len, "pace check: %llu wrong word%s read on xcc%d", r.mem_errors, plural(r.mem_errors), first);
    if (bad_xccs > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more xcc%s)", bad_xccs - 1, bad_xccs > 2 ? "s" : "");
    return n;
  }
  if (r.unlocated_errors > 0)
    return std::snprintf(buf, len, "pace check: %llu wrong result%s at an unknown site", r.unlocated_errors,
                         plural(r.unlocated_errors));
  return 0;
}

// What was slow, if anything: the slowest clock first, then memory time, then cycles.
//   "pace: xcc5 ran 1210 MHz beside a median of 2105 (ratio 0.57)"
//   "pace: xcc5 took 85.2 us per MiB beside a median of 41.0 (ratio 0.48)"
//   "pace: xcc5 took 128.3 cycles per MFMA beside a median of 32.1 over XCDs"
//   "pace: xcc3/se1/sh0/cu7/simd2 took 64.2 cycles per MFMA beside a median of 32.1 (+2 more sites)"
// Returns its length, 0 (and an empty text) if nothing was slow.
inline int note(const amdgpu_pace_result& r, const amdgpu_pace_xcc_slot* xccs, const amdgpu_pace_site_slot* sites,
                char* buf, int len) {
  if (len > 0) buf[0] = 0;
  if (r.slow_xccs_clock != 0 && r.pace_xcc >= 0)
    return std::snprintf(buf, len, "pace: xcc%d ran %.0f MHz beside a median of %.0f (ratio %.2f)", r.pace_xcc,
                         xccs[r.pace_xcc].clock_mhz, r.clock_mhz_median, r.xcd_pace_ratio);
  if (r.slow_xccs_mem != 0 && r.mem_xcc >= 0)
    return std::snprintf(buf, len, "pace: xcc%d took %.1f us per MiB beside a median of %.1f (ratio %.2f)", r.mem_xcc,
                         xccs[r.mem_xcc].us_per_mib, r.us_per_mib_median, r.xcd_mem_ratio);
  if (r.slow_xccs_cycles != 0) {
    int worst = -1;
    std::vector<double> cpms;
    for (int x = 0; x < kPaceXccs; ++x) {
      if (xccs[x].clock_mhz > 0) cpms.push_back(xccs[x].cycles_per_mfma);
      if ((r.slow_xccs_cycles >> x & 1u) && (worst < 0 || xccs[x].cycles_per_mfma > xccs[worst].cycles_per_mfma)) worst = x;
    }
    return std::snprintf(buf, len, "pace: xcc%d took %.1f cycles per MFMA beside a median of %.1f over XCDs", worst,
                         xccs[worst].cycles_per_mfma, median(cpms));
  }
  if (r.n_slow > 0) {
    char where[64];
    format_site(r.slow_sites[0], true, where, sizeof(where));
    int n = std::snprintf(buf, len, "pace: %s took %.1f cycles per MFMA beside a median of %.1f", where,
                          sites[r.slow_sites[0]].cycles_per_mfma, r.cycles_per_mfma_median);
    if (r.n_slow > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more site%s)", r.n_slow - 1, r.n_slow > 2 ? "s" : "");
    return n;
  }
  return 0;
}

// pace_mfma's accumulators hold iters x (A . B) with |A . B| <= 16 * 4 * 4: exact in fp32 below 2^24.
constexpr int kMaxIters = (1 << 24) / 256 - 1;  // 65535: the true iteration count, injection included
constexpr int kMaxInjectFactor = 16;
using canary::kMaxBlocks;
constexpr int kMaxSliceKb = 16384;
constexpr unsigned long long kMaxMemBytes = 4ull << 30;  // slices together

// The argument rule of amdgpu_pace_run, checked before any HIP call.
inline bool arguments_ok(int blocks, int iters, int slice_kb, double slow_ratio, int inject_kind, int inject_xcc,
                         int inject_factor, int inject_waves, int wave_site_len, bool have_wave_site) {
  if (blocks < 0 || blocks > kMaxBlocks || iters < 1 || iters > kMaxIters) return false;
  if (slice_kb < 4 || slice_kb > kMaxSliceKb || slice_kb % 4 != 0) return false;
  // blocks == 0: the grid is the CU count, checked against kMaxMemBytes once that is known
  if (static_cast<unsigned long long>(blocks) * static_cast<unsigned long long>(slice_kb) * 1024ull > kMaxMemBytes) return false;
  if (!(slow_ratio >= 1) || !(slow_ratio <= 1e6)) return false;
  if (inject_kind < -1 || inject_kind > 2) return false;
  if (inject_xcc < 0 || inject_xcc >= kPaceXccs || inject_waves < 0) return false;
  if (inject_factor < 1 || inject_factor > kMaxInjectFactor) return false;
  if (inject_kind >= 0 && inject_kind <= 1 && static_cast<long long>(iters) * inject_factor > kMaxIters) return false;
  if (wave_site_len < 0 || (!have_wave_site && wave_site_len != 0)) return false;
  return true;
}

}  // namespace pace
