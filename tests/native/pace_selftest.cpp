// Stand-alone self-test of the pace check's host side (ops/pace/pace_host.h): no HIP, no
// Python.  tests/test_pace_model.py compiles it with g++ -fsanitize=address,undefined and
// runs it directly; it exits 0 and prints "ok", or prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pace_host.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

constexpr double kTick = 100.0, kClockMax = 2400.0;

unsigned int site(unsigned xcc, unsigned cu = 0, unsigned simd = 0, unsigned se = 0) {
  return xcc << 10 | se << 7 | cu << 2 | simd;
}

amdgpu_pace_record rec(unsigned int s, unsigned long long cycles, unsigned long long ticks, unsigned int work,
                       unsigned int bad = 0, unsigned int last = kPaceUnwritten) {
  return amdgpu_pace_record{s, last == kPaceUnwritten ? s : last, cycles, ticks, work, bad};
}

struct Reduced {
  std::vector<amdgpu_pace_site_slot> sites = std::vector<amdgpu_pace_site_slot>(kPaceSiteSlots);
  amdgpu_pace_xcc_slot xccs[kPaceXccs];
  amdgpu_pace_result r;
  bool ok;
  std::string error, note;
};

Reduced run(const std::vector<amdgpu_pace_record>& mfma, const std::vector<amdgpu_pace_record>& mem, double slow_ratio = 1.5) {
  Reduced out;
  std::memset(&out.r, 0, sizeof(out.r));
  out.ok = pace::reduce(mfma.empty() ? nullptr : mfma.data(), static_cast<int>(mfma.size()),
                        mem.empty() ? nullptr : mem.data(), static_cast<int>(mem.size()), kTick, kClockMax, slow_ratio,
                        out.sites.data(), out.xccs, &out.r);
  if (!out.ok) return out;
  char buf[256];
  pace::describe(out.r, out.xccs, buf, sizeof(buf));
  out.error = buf;
  pace::note(out.r, out.xccs, out.sites.data(), buf, sizeof(buf));
  out.note = buf;
  // a text cut short stays terminated and inside its buffer
  char tiny[8];
  pace::describe(out.r, out.xccs, tiny, sizeof(tiny));
  CHECK(std::strlen(tiny) < sizeof(tiny));
  pace::note(out.r, out.xccs, out.sites.data(), tiny, sizeof(tiny));
  CHECK(std::strlen(tiny) < sizeof(tiny));
  return out;
}

// 8 XCDs x 2 CUs x 4 SIMDs, 4096 MFMAs at 32 cycles on 2100 MHz; one 1 MiB workgroup per CU at 40 us
void table(std::vector<amdgpu_pace_record>& mfma, std::vector<amdgpu_pace_record>& mem, int xccs = 8) {
  for (int x = 0; x < xccs; ++x)
    for (unsigned cu = 0; cu < 2; ++cu)
      for (unsigned simd = 0; simd < 4; ++simd) {
        mfma.push_back(rec(site(x, cu, simd), 32ull * 4096, 32ull * 4096 / 21, 4096));
        mem.push_back(rec(site(x, cu, simd), 84000, 4000 + simd, 1u << 20));
      }
}

void balanced() {
  std::vector<amdgpu_pace_record> mfma, mem;
  table(mfma, mem);
  const Reduced o = run(mfma, mem);
  CHECK(o.ok && o.r.xcd_pace_ratio == 1.0 && o.r.xcd_mem_ratio == 1.0);
  CHECK(o.r.n_slow == 0 && o.r.slow_xccs_clock == 0 && o.r.slow_xccs_cycles == 0 && o.r.slow_xccs_mem == 0);
  CHECK(o.r.waves == 64 && o.r.moved == 0 && o.r.cus_reached == 16 && o.r.simds_reached == 64 && o.r.xccs_reached == 8);
  CHECK(o.r.mem_waves == 64 && o.r.mem_cus_reached == 16 && o.r.mem_xccs_reached == 8 && o.xccs[3].blocks == 2);
  CHECK(o.r.cycles_per_mfma_min == 32.0 && o.r.cycles_per_mfma_max == 32.0 && o.xccs[7].us_per_mib == 40.0);
  CHECK(o.r.pace_errors == 0 && o.error.empty() && o.note.empty());
}

void half_clock_and_texts() {
  std::vector<amdgpu_pace_record> mfma, mem;
  table(mfma, mem);
  for (auto& m : mfma)
    if (m.site_first >> 10 == 5) m.ticks *= 2;
  Reduced o = run(mfma, mem);
  CHECK(o.ok && o.r.pace_xcc == 5 && o.r.slow_xccs_clock == 1u << 5 && o.r.n_slow == 0);
  CHECK(o.r.xcd_pace_ratio > 0.4999 && o.r.xcd_pace_ratio < 0.5001);
  CHECK(o.note.rfind("pace: xcc5 ran ", 0) == 0 && o.note.find("(ratio 0.50)") != std::string::npos);
  // wrong results: located, at two sites
  mfma[0].bad = 3;
  mfma[9].bad = 1;
  o = run(mfma, mem);
  CHECK(o.r.mfma_errors == 4 && o.r.n_bad == 2 && o.r.pace_errors == 4);
  CHECK(o.error == "pace check: 4 wrong results at xcc0/se0/sh0/cu0/simd0 (+1 more site)");
  mfma[0].bad = mfma[9].bad = 0;
  mem[21].bad = 2;  // wave 1 of a workgroup on xcc2
  o = run(mfma, mem);
  CHECK(o.r.mem_errors == 2 && o.error == "pace check: 2 wrong words read on xcc2");
}

void moved_and_unwritten() {
  std::vector<amdgpu_pace_record> mfma, mem;
  table(mfma, mem);
  mfma.push_back(rec(site(1, 1, 1), 1u << 30, 7, 4096, 5, site(1, 1, 2)));
  mfma.push_back(amdgpu_pace_record{kPaceUnwritten, kPaceUnwritten, ~0ull, ~0ull, kPaceUnwritten, kPaceUnwritten});
  mem[4].site_last ^= 4u;  // wave 0 of the second workgroup moved
  mem[4].bad = 1;
  const Reduced o = run(mfma, mem);
  CHECK(o.ok && o.r.moved == 1 && o.r.mem_moved == 1 && o.r.unlocated_errors == 6 && o.r.mfma_errors == 0);
  CHECK(o.r.waves == 64 && o.r.n_slow == 0 && o.xccs[0].blocks == 1);
  CHECK(o.error == "pace check: 6 wrong results at an unknown site");
}

void seventeen_slow_sites() {
  std::vector<amdgpu_pace_record> mfma, mem;
  for (unsigned cu = 0; cu < 16; ++cu)
    for (unsigned simd = 0; simd < 4; ++simd)
      mfma.push_back(rec(site(0, cu, simd), (cu * 4 + simd < 17 ? 80ull : 32ull) * 1024, 1600, 1024));
  const Reduced o = run(mfma, mem);
  CHECK(o.ok && o.r.n_slow == 17 && o.r.slow_sites[15] == 15 && o.r.xccs_reached == 1 && o.r.pace_xcc == -1);
  CHECK(o.r.xcd_pace_ratio == 1.0 && o.r.slow_xccs_clock == 0 && o.r.slow_xccs_cycles == 0);
  CHECK(o.note.find("(+16 more sites)") != std::string::npos);
}

void boundaries_and_medians() {
  std::vector<amdgpu_pace_record> mfma, mem;
  table(mfma, mem);
  mfma[1].cycles = 48ull * 4096;       // exactly 1.5 x the median: not slow
  mfma[2].cycles = 48ull * 4096 + 64;  // above it
  const Reduced o = run(mfma, mem);
  CHECK(o.r.n_slow == 1 && o.r.slow_sites[0] == mfma[2].site_first);
  std::vector<double> v = {3, 1, 2};
  CHECK(pace::median(v) == 2);
  v = {4, 1, 3, 2};
  CHECK(pace::median(v) == 2.5);
  v.clear();
  CHECK(pace::median(v) == 0);
}

void refusals() {
  std::vector<amdgpu_pace_record> mfma, mem, none;
  table(mfma, mem);
  Reduced o;
  std::memset(&o.r, 0, sizeof(o.r));
  CHECK(!pace::reduce(mfma.data(), 64, nullptr, 0, 0.0, kClockMax, 1.5, o.sites.data(), o.xccs, &o.r));
  CHECK(!pace::reduce(mfma.data(), 64, nullptr, 0, kTick, kClockMax, 0.5, o.sites.data(), o.xccs, &o.r));
  CHECK(!pace::reduce(mfma.data(), 64, mem.data(), 3, kTick, kClockMax, 1.5, o.sites.data(), o.xccs, &o.r));
  CHECK(!pace::reduce(nullptr, 1, nullptr, 0, kTick, kClockMax, 1.5, o.sites.data(), o.xccs, &o.r));
  mfma[3].site_last = kPaceSiteSlots;
  CHECK(!pace::reduce(mfma.data(), 64, nullptr, 0, kTick, kClockMax, 1.5, o.sites.data(), o.xccs, &o.r));
  CHECK(run(none, none).ok);
  // the argument rule of the run: iters and the injected factor stay below 2^16 together
  CHECK(pace::arguments_ok(0, 4096, 1024, 1.5, -1, 0, 4, 0, 0, false));
  CHECK(pace::arguments_ok(16, 256, 64, 2.0, 0, 7, 4, 0, 64, true));
  CHECK(!pace::arguments_ok(0, 65536, 1024, 1.5, -1, 0, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(0, 16384, 1024, 1.5, 0, 0, 4, 0, 0, false));
  CHECK(pace::arguments_ok(0, 16383, 1024, 1.5, 0, 0, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(0, 0, 1024, 1.5, -1, 0, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(0, 256, 6, 1.5, -1, 0, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(4096, 256, 16384, 1.5, -1, 0, 4, 0, 0, false));  // 64 GiB of slices
  CHECK(!pace::arguments_ok(0, 256, 1024, 1.5, 3, 0, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(0, 256, 1024, 1.5, 0, 16, 4, 0, 0, false));
  CHECK(!pace::arguments_ok(0, 256, 1024, 1.5, -1, 0, 4, 0, 8, false));
}

}  // namespace

int main() {
  balanced();
  half_clock_and_texts();
  moved_and_unwritten();
  seventeen_slow_sites();
  boundaries_and_medians();
  refusals();
  static_assert(sizeof(amdgpu_pace_record) == 32, "record");
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
