// The site vocabulary of the located checks, host only, shared by canary_common.h and
// canary_host.h (so by every canary source and by the host-link check), pace/pace_host.h,
// ldspath/ldspath_host.h and tests/native/site_selftest.cpp: the packed site and its text, the
// rule for a wave's record, the coverage walk over a table of sites, and the launch plan.
// No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <cstdio>

// A site is (xcc, se, sh, cu, simd) packed into 14 bits:
//   simd 1:0 | cu 5:2 | sh 6 | se 9:7 | xcc 13:10
constexpr int kSiteSlots = 1 << 14;
constexpr unsigned int kSiteUnwritten = 0xFFFFFFFFu;  // site_first of a record no wave wrote

namespace canary {

constexpr int kMaxBlocks = 4096;  // grid cap of the located checks: the index of a wave of 4-wave workgroups < 2^14

// "xcc3/se1/sh0/cu7/simd2" of a packed site, "xcc3/se1/sh0/cu7" without simd
inline int format_site(unsigned int site, bool simd, char* buf, int len) {
  int n = std::snprintf(buf, len, "xcc%u/se%u/sh%u/cu%u", (site >> 10) & 0xFu, (site >> 7) & 7u, (site >> 6) & 1u,
                        (site >> 2) & 0xFu);
  if (simd && n > 0 && n < len) n += std::snprintf(buf + n, len - n, "/simd%u", site & 3u);
  return n;
}

inline const char* plural(unsigned long long n) { return n == 1 ? "" : "s"; }

// A wave's record holds site_id() before its work and after it: located if it stayed.
template <class Rec>
bool located(const Rec& r) {
  return r.site_first == r.site_last;
}

// Every written record's sites lie below kSiteSlots.
template <class Rec>
bool records_valid(const Rec* r, int n) {
  for (int i = 0; i < n; ++i) {
    if (r[i].site_first == kSiteUnwritten) continue;
    if (r[i].site_first >= static_cast<unsigned int>(kSiteSlots) || r[i].site_last >= static_cast<unsigned int>(kSiteSlots))
      return false;
  }
  return true;
}

struct SiteCoverage {
  int cus_reached;    // distinct (xcc, se, sh, cu) with a reached site
  int simds_reached;  // reached sites
  int n_bad;          // bad sites
  unsigned int bad_sites[16];  // the first 16 of them, packed, ascending
};

// One walk over the kSiteSlots sites, CU by CU: reached(site) and bad(site) are the caller's
// predicates (whether a bad site must also be reached is the caller's to say).
template <class Reached, class Bad>
SiteCoverage site_coverage(Reached reached, Bad bad) {
  SiteCoverage c = {};
  for (int cu = 0; cu < kSiteSlots / 4; ++cu) {
    bool any = false;
    for (int simd = 0; simd < 4; ++simd) {
      const int site = cu * 4 + simd;
      if (reached(site)) {
        any = true;
        ++c.simds_reached;
      }
      if (bad(site)) {
        if (c.n_bad < 16) c.bad_sites[c.n_bad] = static_cast<unsigned int>(site);
        ++c.n_bad;
      }
    }
    c.cus_reached += any;
  }
  return c;
}

// Copies a coverage into a result struct with the same four fields.
template <class Result>
void store_coverage(const SiteCoverage& c, Result* r) {
  r->cus_reached = c.cus_reached;
  r->simds_reached = c.simds_reached;
  r->n_bad = c.n_bad;
  for (int i = 0; i < 16; ++i) r->bad_sites[i] = c.bad_sites[i];
}

// Every CU and every SIMD of it has been reached (c: a SiteCoverage or a result carrying its counts).
template <class Coverage>
bool covered(const Coverage& c, int cus_expected) {
  return c.cus_reached >= cus_expected && c.simds_reached >= 4 * cus_expected;
}

struct LaunchPlan {
  int grid;          // workgroups of one launch
  int max_launches;  // 4 when the caller tops up until covered(), else 1
};

// blocks == 0: per_cu workgroups per CU, at most kMaxBlocks and at least 1, topped up when
// asked to; blocks > 0: one launch of that many (the callers refuse more than kMaxBlocks).
inline LaunchPlan launch_plan(int blocks, int cus, int per_cu, bool top_up = false) {
  const bool automatic = blocks == 0;
  int grid = automatic ? per_cu * cus : blocks;
  if (grid > kMaxBlocks) grid = kMaxBlocks;
  if (grid < 1) grid = 1;
  return {grid, automatic && top_up ? 4 : 1};
}

}  // namespace canary
