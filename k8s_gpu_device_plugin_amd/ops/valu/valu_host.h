// The vector-ALU check's host side, written once: the record every wave of valu_sweep leaves, the
// result, the expected tables, the reduction of the records with the consensus rule, and the
// error texts.  The packed site, its text and the coverage walk are ../site.h's; the ops are
// valu_ops.h's.  No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../site.h"
#include "valu_ops.h"

extern "C" {

constexpr int kValuMaxOps = 128;                       // room for ops in a result
constexpr int kValuGroupOps = valu::kMaxGroupOps;      // room for a group's ops in a record
constexpr int kValuGroups = 8;                         // room for groups in a result
constexpr int kValuWaves = 4;                          // waves per workgroup: records[block * 4 + wave]
constexpr unsigned int kValuNone = kSiteUnwritten;     // site_first of a slot no wave wrote; first_op: nothing wrong

struct amdgpu_valu_record {  // what one wave of one valu_sweep launch leaves; 272 bytes
  unsigned int site_first;   // site_id() before the work
  unsigned int site_last;    // ... and after it
  unsigned int first_op;     // first exact op of the group (its index in the table) with a wrong lane, all-ones: none
  unsigned int first_lane;   // ... and its lowest wrong lane
  unsigned int bad[kValuGroupOps];     // wrong lanes per op of the group (exact ops)
  unsigned int digest[kValuGroupOps];  // the wave's digest per op of the group (judged for consensus ops)
};

struct amdgpu_valu_result {
  unsigned long long errors[kValuMaxOps];       // located wrong results per op
  unsigned long long group_errors[kValuGroups]; // ... per group
  unsigned long long unlocated_errors;          // those of waves whose site changed
  unsigned long long valu_errors;               // what fails the check: all of the above
  unsigned long long waves;                     // located records, over all groups
  unsigned long long moved;                     // records whose site changed
  double group_ms[kValuGroups];                 // device time of the group's kernel over all launches
  double ms;                                    // their sum
  int launches;
  int cus_reached;     // distinct (xcc, se, sh, cu) with a located record of every selected group
  int simds_reached;   // distinct sites with one
  int cus_expected;    // multiProcessorCount (0 from the bare reduction)
  int n_bad;           // sites with a located wrong result
  unsigned int bad_sites[16];               // the first 16 of them, packed
  int op_n_bad[kValuMaxOps];                // sites with a located wrong result of that op
  unsigned int op_first_site[kValuMaxOps];  // the lowest of them
  unsigned int op_first_lane[kValuMaxOps];  // first_lane of the first bad record there (all-ones for a consensus op)
  unsigned char selected[kValuMaxOps];      // 1: the op was selected
  unsigned char unjudged[kValuMaxOps];      // 1: a selected consensus op without a majority to judge it by
  int blocks;          // grid of one launch; rounds as run (0 from the bare reduction)
  int rounds;
};

}  // extern "C"

namespace valu {

using canary::format_site;
using canary::kMaxBlocks;
using canary::located;
using canary::plural;
using canary::records_valid;

static_assert(kNumOps <= kValuMaxOps && kNumGroups <= kValuGroups, "a result has room for the table");

inline unsigned int group_mask(const unsigned char* selected) {
  unsigned int m = 0;
  for (int op = 0; op < kNumOps; ++op)
    if (selected[op]) m |= 1u << kOps[op].group;
  return m;
}

// recs: the records of every launch, in any order (unwritten slots are skipped); record i is of
// group group_of[i], which must hold a selected op.  An exact op counts the record's bad[];
// a consensus op is judged by the digest most located records of its group agree on: a record
// that differs has one wrong result, and with fewer than three located records, or a largest
// group of half of them or fewer, the op is unjudged.  A site is reached once every selected
// group has a located record there.  out keeps group_ms, ms, launches, cus_expected, blocks and
// rounds the caller set and gets everything else.  false: a bad argument.
inline bool reduce(const amdgpu_valu_record* recs, const int* group_of, int n, const unsigned char* selected,
                   amdgpu_valu_result* out) {
  if (out == nullptr || selected == nullptr || n < 0 || (n > 0 && (recs == nullptr || group_of == nullptr)) ||
      !records_valid(recs, n))
    return false;
  const unsigned int groups = group_mask(selected);
  if (groups == 0) return false;
  for (int i = 0; i < n; ++i)
    if (group_of[i] < 0 || group_of[i] >= kNumGroups || !((groups >> group_of[i]) & 1u)) return false;
  amdgpu_valu_result r;
  std::memset(&r, 0, sizeof(r));
  std::memcpy(r.group_ms, out->group_ms, sizeof(r.group_ms));
  r.ms = out->ms;
  r.launches = out->launches;
  r.cus_expected = out->cus_expected;
  r.blocks = out->blocks;
  r.rounds = out->rounds;
  for (int op = 0; op < kNumOps; ++op) r.selected[op] = selected[op] ? 1 : 0;
  for (int op = 0; op < kValuMaxOps; ++op) r.op_first_site[op] = r.op_first_lane[op] = kValuNone;
  std::vector<unsigned int> reached(kSiteSlots, 0), site_bad(kSiteSlots, 0);
  std::vector<unsigned char> op_bad(static_cast<size_t>(kNumOps) * kSiteSlots, 0);
  auto wrong = [&](int op, const amdgpu_valu_record& rec, unsigned long long count, unsigned int lane) {
    r.errors[op] += count;
    site_bad[rec.site_first] += 1;
    unsigned char& seen = op_bad[static_cast<size_t>(op) * kSiteSlots + rec.site_first];
    if (seen) return;
    seen = 1;
    ++r.op_n_bad[op];
    if (rec.site_first < r.op_first_site[op]) {  // the lowest bad site is named, with its first bad record's lane
      r.op_first_site[op] = rec.site_first;
      r.op_first_lane[op] = lane;
    }
  };
  // the majority digest of each selected consensus op over the located records of its group
  std::vector<unsigned int> majority(kNumOps, 0);
  for (int op = 0; op < kNumOps; ++op) {
    if (!r.selected[op] || kOps[op].cls != kConsensus) continue;
    const int g = kOps[op].group, slot = op - group_first(g);
    std::vector<unsigned int> d;
    for (int i = 0; i < n; ++i)
      if (group_of[i] == g && recs[i].site_first != kValuNone && located(recs[i])) d.push_back(recs[i].digest[slot]);
    std::sort(d.begin(), d.end());
    size_t best = 0;
    for (size_t i = 0, j = 0; i < d.size(); i = j) {
      while (j < d.size() && d[j] == d[i]) ++j;
      if (j - i > best) {
        best = j - i;
        majority[op] = d[i];
      }
    }
    r.unjudged[op] = d.size() < 3 || 2 * best <= d.size();
  }
  for (int i = 0; i < n; ++i) {
    const amdgpu_valu_record& rec = recs[i];
    if (rec.site_first == kValuNone) continue;
    const int g = group_of[i], first = group_first(g), count = group_count(g);
    if (!located(rec)) {
      ++r.moved;
      for (int s = 0; s < count; ++s)
        if (r.selected[first + s] && kOps[first + s].cls == kExact) r.unlocated_errors += rec.bad[s];
      continue;
    }
    ++r.waves;
    reached[rec.site_first] |= 1u << g;
    for (int s = 0; s < count; ++s) {
      const int op = first + s;
      if (!r.selected[op]) continue;
      if (kOps[op].cls == kExact) {
        if (rec.bad[s]) wrong(op, rec, rec.bad[s], rec.first_op == static_cast<unsigned int>(op) ? rec.first_lane : kValuNone);
      } else if (!r.unjudged[op] && rec.digest[s] != majority[op]) {
        wrong(op, rec, 1, kValuNone);
      }
    }
  }
  r.valu_errors = r.unlocated_errors;
  for (int op = 0; op < kNumOps; ++op) {
    r.valu_errors += r.errors[op];
    r.group_errors[kOps[op].group] += r.errors[op];
  }
  canary::store_coverage(canary::site_coverage([&](int site) { return reached[site] == groups; },
                                               [&](int site) { return site_bad[site] != 0; }),
                         &r);
  *out = r;
  return true;
}

// The text of op `which`, or of the first failing op (which < 0):
//   "vector ALU check: 5 wrong results in cvt_scalef32_pk_fp4_f32 at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
//   "vector ALU check: 4 wrong results at an unknown site"   (every wrong wave moved while it ran)
// Returns its length, 0 (and an empty text) if nothing failed.
inline int describe(const amdgpu_valu_result& r, int which, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  for (int op = 0; op < kNumOps; ++op) {
    if ((which >= 0 && which != op) || r.errors[op] == 0 || r.op_n_bad[op] == 0) continue;
    char where[64];
    format_site(r.op_first_site[op], true, where, sizeof(where));
    int n = std::snprintf(buf, len, "vector ALU check: %llu wrong result%s in %s at %s", r.errors[op], plural(r.errors[op]),
                          kOps[op].name, where);
    const int others = r.op_n_bad[op] - 1;
    if (others > 0 && n > 0 && n < len) n += std::snprintf(buf + n, len - n, " (+%d more site%s)", others, others > 1 ? "s" : "");
    return n;
  }
  if (which < 0 && r.unlocated_errors > 0)
    return std::snprintf(buf, len, "vector ALU check: %llu wrong result%s at an unknown site", r.unlocated_errors,
                         plural(r.unlocated_errors));
  return 0;
}

// The argument rule of amdgpu_valu_run, checked before any HIP call.
inline bool arguments_ok(int blocks, int rounds, const unsigned char* selected, int inject_op, int inject_waves, int wave_site_len,
                         bool have_wave_site) {
  if (blocks < 0 || blocks > kMaxBlocks || rounds < 1 || rounds > kMaxRounds) return false;
  if (selected == nullptr || group_mask(selected) == 0) return false;
  if (inject_waves < 0 || inject_op < -1 || inject_op >= kNumOps) return false;
  if (inject_op >= 0 && !selected[inject_op]) return false;
  if (wave_site_len < 0 || (!have_wave_site && wave_site_len != 0)) return false;
  return true;
}

}  // namespace valu
