// Stand-alone self-test of the site vocabulary (ops/site.h): no HIP, no Python.
// tests/test_canary_site.py compiles it with g++ -fsanitize=address,undefined and runs it
// directly; it exits 0 and prints "ok", or prints what failed and exits 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "site.h"

namespace {

using namespace canary;

int failures = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

struct Table {
  std::vector<unsigned char> waves = std::vector<unsigned char>(kSiteSlots, 0), bad = std::vector<unsigned char>(kSiteSlots, 0);
  // cumem.hip's rule: a bad site counts with or without a wave
  SiteCoverage any_bad() const {
    return site_coverage([&](int s) { return waves[s] != 0; }, [&](int s) { return bad[s] != 0; });
  }
  // sites.hip's and pace_host.h's rule: only a reached site can be bad
  SiteCoverage reached_bad() const {
    return site_coverage([&](int s) { return waves[s] != 0; }, [&](int s) { return waves[s] != 0 && bad[s] != 0; });
  }
};

unsigned int site(unsigned xcc, unsigned se, unsigned sh, unsigned cu, unsigned simd) {
  return xcc << 10 | se << 7 | sh << 6 | cu << 2 | simd;
}

void coverage() {
  Table t;
  SiteCoverage c = t.any_bad();
  CHECK(c.cus_reached == 0 && c.simds_reached == 0 && c.n_bad == 0);
  for (unsigned int b : c.bad_sites) CHECK(b == 0);
  CHECK(covered(c, 0) && !covered(c, 1));

  t.waves[site(3, 1, 0, 7, 2)] = 1;  // one site
  c = t.any_bad();
  CHECK(c.cus_reached == 1 && c.simds_reached == 1 && c.n_bad == 0);
  CHECK(!covered(c, 1));  // one CU, but one of its four SIMDs

  for (unsigned simd = 0; simd < 4; ++simd) t.waves[site(3, 1, 0, 7, simd)] = 1;  // all four SIMDs of that CU
  c = t.any_bad();
  CHECK(c.cus_reached == 1 && c.simds_reached == 4);
  CHECK(covered(c, 1) && !covered(c, 2));

  Table two;  // two CUs, one SIMD each
  two.waves[site(0, 0, 0, 1, 3)] = 1;
  two.waves[site(0, 0, 1, 1, 0)] = 1;
  c = two.any_bad();
  CHECK(c.cus_reached == 2 && c.simds_reached == 2 && !covered(c, 2));

  // a bad site with no wave: the callables decide
  two.bad[site(5, 2, 0, 9, 1)] = 1;
  c = two.any_bad();
  CHECK(c.cus_reached == 2 && c.simds_reached == 2 && c.n_bad == 1 && c.bad_sites[0] == site(5, 2, 0, 9, 1));
  c = two.reached_bad();
  CHECK(c.cus_reached == 2 && c.simds_reached == 2 && c.n_bad == 0 && c.bad_sites[0] == 0);
  two.bad[site(0, 0, 1, 1, 0)] = 1;  // and one that a wave reached: both rules name it first
  CHECK(two.any_bad().n_bad == 2 && two.any_bad().bad_sites[0] == site(0, 0, 1, 1, 0));
  CHECK(two.reached_bad().n_bad == 1 && two.reached_bad().bad_sites[0] == site(0, 0, 1, 1, 0));

  // 17 bad sites, set in descending order: all counted, the lowest 16 listed ascending
  Table many;
  for (int i = 16; i >= 0; --i) {
    many.waves[37 * i + 5] = 1;
    many.bad[37 * i + 5] = 1;
  }
  c = many.reached_bad();
  CHECK(c.n_bad == 17 && c.simds_reached == 17);
  for (int i = 0; i < 16; ++i) CHECK(c.bad_sites[i] == static_cast<unsigned int>(37 * i + 5));

  Table last;  // the last slot
  last.waves[kSiteSlots - 1] = 1;
  last.bad[kSiteSlots - 1] = 1;
  c = last.reached_bad();
  CHECK(c.cus_reached == 1 && c.simds_reached == 1 && c.n_bad == 1 && c.bad_sites[0] == static_cast<unsigned int>(kSiteSlots - 1));

  struct Result {
    int cus_reached = -1, simds_reached = -1, n_bad = -1;
    unsigned int bad_sites[16];
  } r;
  std::memset(r.bad_sites, 0xFF, sizeof(r.bad_sites));
  store_coverage(c, &r);
  CHECK(r.cus_reached == 1 && r.simds_reached == 1 && r.n_bad == 1 && r.bad_sites[0] == c.bad_sites[0] && r.bad_sites[15] == 0);
  CHECK(!covered(r, 1));
}

void plans() {
  for (int per_cu = 1; per_cu <= 2; ++per_cu) {
    for (bool top_up : {false, true}) {
      // automatic: per_cu workgroups per CU, at least 1, at most kMaxBlocks; 4 launches only when topped up
      const int launches = top_up ? 4 : 1;
      LaunchPlan p = launch_plan(0, 0, per_cu, top_up);  // a device that reports no CU
      CHECK(p.grid == 1 && p.max_launches == launches);
      p = launch_plan(0, 256, per_cu, top_up);
      CHECK(p.grid == per_cu * 256 && p.max_launches == launches);
      p = launch_plan(0, 4096, per_cu, top_up);  // the cap
      CHECK(p.grid == kMaxBlocks && p.max_launches == launches);
      // a grid the caller names: one launch of it, whatever the device
      for (int cus : {0, 256, 4096}) {
        p = launch_plan(1, cus, per_cu, top_up);
        CHECK(p.grid == 1 && p.max_launches == 1);
        p = launch_plan(kMaxBlocks, cus, per_cu, top_up);
        CHECK(p.grid == kMaxBlocks && p.max_launches == 1);
      }
    }
  }
  CHECK(launch_plan(0, 256, 1).max_launches == 1);  // no top-up unless asked for
  CHECK(kMaxBlocks * 4 == kSiteSlots);              // the index of a wave of 4-wave workgroups fits a site table
}

struct Rec {
  unsigned int site_first, site_last;
};

void records() {
  const Rec good[] = {{0, 0}, {site(15, 7, 1, 15, 3), site(15, 7, 1, 15, 3)}, {5, 9}};
  CHECK(records_valid(good, 3) && records_valid(good, 0) && records_valid(static_cast<const Rec*>(nullptr), 0));
  CHECK(located(good[0]) && located(good[1]) && !located(good[2]));
  const Rec unwritten[] = {{kSiteUnwritten, kSiteUnwritten}, {kSiteUnwritten, 77777}, {1, 1}};  // skipped, whatever follows
  CHECK(records_valid(unwritten, 3));
  const Rec at_end[] = {{1, 1}, {static_cast<unsigned int>(kSiteSlots), static_cast<unsigned int>(kSiteSlots)}};
  CHECK(!records_valid(at_end, 2) && records_valid(at_end, 1));
  const Rec last_out[] = {{static_cast<unsigned int>(kSiteSlots - 1), static_cast<unsigned int>(kSiteSlots)}};
  CHECK(!records_valid(last_out, 1));
  const Rec last_unwritten[] = {{3, kSiteUnwritten}};  // only site_first marks an unwritten record
  CHECK(!records_valid(last_unwritten, 1));
}

void texts() {
  char buf[64];
  CHECK(format_site(site(3, 1, 0, 7, 2), true, buf, sizeof(buf)) == 22 && std::strcmp(buf, "xcc3/se1/sh0/cu7/simd2") == 0);
  CHECK(format_site(site(3, 1, 0, 7, 2), false, buf, sizeof(buf)) == 16 && std::strcmp(buf, "xcc3/se1/sh0/cu7") == 0);
  format_site(kSiteSlots - 1, true, buf, sizeof(buf));
  CHECK(std::strcmp(buf, "xcc15/se7/sh1/cu15/simd3") == 0);
  format_site(0, true, buf, sizeof(buf));
  CHECK(std::strcmp(buf, "xcc0/se0/sh0/cu0/simd0") == 0);
  char tiny[8];  // a text cut short stays terminated and inside its buffer
  format_site(kSiteSlots - 1, true, tiny, sizeof(tiny));
  CHECK(std::strlen(tiny) < sizeof(tiny));
  CHECK(std::strcmp(plural(0), "s") == 0 && std::strcmp(plural(1), "") == 0 && std::strcmp(plural(2), "s") == 0);
}

}  // namespace

int main() {
  coverage();
  plans();
  records();
  texts();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
