// The matrix-forms check's host side, written once: the record every wave of form_sweep leaves,
// the result, the reduction of the records and the error texts.  The packed site, its text and
// the coverage walk are ../site.h's; the forms are matforms_forms.h's.  No HIP include: a plain
// C++17 compiler compiles it (tests/native/matforms_selftest.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../site.h"
#include "matforms_forms.h"

extern "C" {

constexpr int kMatFormsMax = matforms::kMaxForms;  // room for forms in a record and a result
constexpr int kMatFormsWaves = 4;                  // waves per workgroup: records[block * 4 + wave]
constexpr unsigned int kMatFormsNone = kSiteUnwritten;  // site_first of a slot no wave wrote; first_form: nothing wrong

struct amdgpu_matforms_record {  // what one wave of one form_sweep launch leaves; 80 bytes
  unsigned int site_first;       // site_id() before the work
  unsigned int site_last;        // ... and after it
  unsigned int first_form;       // form of the first wrong accumulator, all-ones: none
  unsigned int first_reg;        // ... and its register
  unsigned int bad[kMatFormsMax];  // wrong accumulators per form (a launch fills its own forms)
};

struct amdgpu_matforms_result {
  unsigned long long errors[kMatFormsMax];      // located wrong accumulators per form
  unsigned long long unlocated_errors;          // those of waves whose site changed
  unsigned long long matforms_errors;           // what fails the check: all of the above
  unsigned long long waves;                     // located records, over all forms
  unsigned long long moved;                     // records whose site changed
  unsigned long long form_waves[kMatFormsMax];  // located records per form
  double tflops[kMatFormsMax];                  // dense TFLOP/s (i8: TOP/s) per form, 0 unless rates were asked for
  double form_ms[kMatFormsMax];                 // device time of the form's check over all launches
  double ms;                                    // their sum
  int launches;
  int cus_reached;     // distinct (xcc, se, sh, cu) with a located record of every selected form
  int simds_reached;   // distinct sites with one
  int cus_expected;    // multiProcessorCount (0 from the bare reduction)
  int n_bad;           // sites with a located wrong accumulator
  unsigned int bad_sites[16];  // the first 16 of them, packed
  int form_n_bad[kMatFormsMax];  // sites with a located wrong accumulator of that form
  unsigned int form_first_site[kMatFormsMax];  // the lowest of them
  unsigned int form_first_reg[kMatFormsMax];   // first_reg of the first bad record there
  unsigned int forms;  // bit f: form f was selected
  int blocks;          // grid of one launch; ksteps, vary_scale as run (0 from the bare reduction)
  int ksteps;
  int vary_scale;
};

}  // extern "C"

namespace matforms {

using canary::format_site;
using canary::kMaxBlocks;
using canary::located;
using canary::plural;
using canary::records_valid;

constexpr unsigned int kAllForms = (1u << kNumForms) - 1u;

// recs: the records of every launch, in any order (unwritten slots are skipped); record i
// belongs to form form_of[i], which must be one of the selected `forms` (bit f: form f), and
// only its bad[form_of[i]] counts.  A site is reached once every selected form has a located
// record there.  out keeps tflops, form_ms, ms, launches, cus_expected, blocks, ksteps and
// vary_scale the caller set and gets everything else.  false: a bad argument.
inline bool reduce(const amdgpu_matforms_record* recs, const int* form_of, int n, unsigned int forms,
                   amdgpu_matforms_result* out) {
  if (out == nullptr || n < 0 || (n > 0 && (recs == nullptr || form_of == nullptr)) || !records_valid(recs, n)) return false;
  if (forms == 0 || (forms & ~kAllForms)) return false;
  for (int i = 0; i < n; ++i)
    if (form_of[i] < 0 || form_of[i] >= kNumForms || !((forms >> form_of[i]) & 1u)) return false;
  amdgpu_matforms_result r;
  std::memset(&r, 0, sizeof(r));
  std::memcpy(r.tflops, out->tflops, sizeof(r.tflops));
  std::memcpy(r.form_ms, out->form_ms, sizeof(r.form_ms));
  r.ms = out->ms;
  r.launches = out->launches;
  r.cus_expected = out->cus_expected;
  r.blocks = out->blocks;
  r.ksteps = out->ksteps;
  r.vary_scale = out->vary_scale;
  r.forms = forms;
  std::vector<unsigned int> reached(kSiteSlots, 0), site_bad(kSiteSlots, 0);
  std::vector<unsigned char> form_bad(static_cast<size_t>(kNumForms) * kSiteSlots, 0);
  for (int f = 0; f < kMatFormsMax; ++f) r.form_first_site[f] = r.form_first_reg[f] = kMatFormsNone;
  for (int i = 0; i < n; ++i) {
    const amdgpu_matforms_record& rec = recs[i];
    if (rec.site_first == kMatFormsNone) continue;
    const int f = form_of[i];
    const unsigned long long total = rec.bad[f];
    if (!located(rec)) {
      ++r.moved;
      r.unlocated_errors += total;
      continue;
    }
    ++r.waves;
    ++r.form_waves[f];
    reached[rec.site_first] |= 1u << f;
    r.errors[f] += total;
    if (total == 0) continue;
    site_bad[rec.site_first] += 1;
    unsigned char& seen = form_bad[static_cast<size_t>(f) * kSiteSlots + rec.site_first];
    if (!seen) {
      seen = 1;
      ++r.form_n_bad[f];
      if (rec.site_first < r.form_first_site[f]) {  // the lowest bad site is named, with its first bad record's register
        r.form_first_site[f] = rec.site_first;
        r.form_first_reg[f] = rec.first_reg;
      }
    }
  }
  r.matforms_errors = r.unlocated_errors;
  for (int f = 0; f < kNumForms; ++f) r.matforms_errors += r.errors[f];
  canary::store_coverage(canary::site_coverage([&](int site) { return reached[site] == forms; },
                                               [&](int site) { return site_bad[site] != 0; }),
                         &r);
  *out = r;
  return true;
}

// The text of form `which`, or of the first failing form (which < 0):
//   "matrix form check: 5 wrong results in i8 32x32x32 at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
//   "matrix form check: 4 wrong results at an unknown site"   (every wrong wave moved while it ran)
// Returns its length, 0 (and an empty text) if nothing failed.
inline int describe(const amdgpu_matforms_result& r, int which, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  for (int f = 0; f < kNumForms; ++f) {
    if ((which >= 0 && which != f) || r.errors[f] == 0 || r.form_n_bad[f] == 0) continue;
    char where[64];
    format_site(r.form_first_site[f], true, where, sizeof(where));
    int n = std::snprintf(buf, len, "matrix form check: %llu wrong result%s in %s at %s", r.errors[f], plural(r.errors[f]),
                          kForms[f].text, where);
    const int others = r.form_n_bad[f] - 1;
    if (others > 0 && n > 0 && n < len) n += std::snprintf(buf + n, len - n, " (+%d more site%s)", others, others > 1 ? "s" : "");
    return n;
  }
  if (which < 0 && r.unlocated_errors > 0)
    return std::snprintf(buf, len, "matrix form check: %llu wrong result%s at an unknown site", r.unlocated_errors,
                         plural(r.unlocated_errors));
  return 0;
}

// The argument rule of amdgpu_matforms_run, checked before any HIP call.
inline bool arguments_ok(int blocks, int ksteps, int vary_scale, unsigned int forms, int inject_form, int inject_waves,
                         int wave_site_len, bool have_wave_site) {
  if (blocks < 0 || blocks > kMaxBlocks || ksteps < 1 || ksteps > kMaxKsteps || vary_scale < 0 || vary_scale > 1) return false;
  if (forms == 0 || (forms & ~kAllForms)) return false;
  if (inject_waves < 0 || inject_form < -1 || inject_form >= kNumForms) return false;
  if (inject_form >= 0 && !((forms >> inject_form) & 1u)) return false;
  if (wave_site_len < 0 || (!have_wave_site && wave_site_len != 0)) return false;
  return true;
}

}  // namespace matforms
