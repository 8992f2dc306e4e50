// What the host and the device of the attention-path check must agree on, written once: the
// shape rules, the three data sets, the closed form of what a healthy kernel gives for the two
// exact ones, the float64 reference of the third, the result and its texts.  The hash and the
// small integers are ../mfma_forms.h's.  No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../mfma_forms.h"

extern "C" {

constexpr int kAttnSets = 3;  // 0 uniform, 1 routed, 2 hashed

struct amdgpu_attn_result {                    // 168 bytes
  unsigned long long o_errors[kAttnSets];      // wrong elements of O per set (the exact sets: bit mismatches)
  unsigned long long lse_errors[kAttnSets];    // lse values outside the bound
  unsigned long long first_bad[kAttnSets];     // (head * Sq + row) * 128 + d of the first wrong element, ~0: none
  unsigned long long first_bad_lse[kAttnSets]; // head * Sq + row of the first wrong lse, ~0: none
  double ms[kAttnSets];                        // device time of the `iters` timed launches of each set
  double tflops;                               // 4 H Sq Sk 128 flop per launch over all sets (causal: visible tiles only)
  double max_err;                              // hashed set: the largest |o - ref| seen in the checked rows
  double max_lse_err;                          // ... and the largest |lse - ref| there
  int heads, seq_q, seq_k, causal;
  int iters, rows;
};

}  // extern "C"

namespace attn {

constexpr int kD = 128;        // head dimension
constexpr int kBlockQ = 128;   // queries of a workgroup
constexpr int kBlockK = 64;    // keys of a tile
constexpr int kMaxSeq = 65536; // 4 * 65536 < 2^24: the integer sums of the exact sets stay exact in fp32
constexpr int kMaxBlocks = 1 << 20;  // workgroups of one launch
constexpr int kUniform = 0, kRouted = 1, kHashed = 2;
constexpr int kMaxRows = 64;   // checked rows per head of the hashed set

inline const char* set_name(int set) { return set == kUniform ? "uniform" : set == kRouted ? "routed" : set == kHashed ? "hashed" : "?"; }

// Sq a positive multiple of 128, Sk a positive multiple of 64, Sk >= Sq when causal.
FORMS_HD bool shape_ok(int H, int Sq, int Sk, int causal) {
  return H > 0 && Sq > 0 && Sk > 0 && Sq % kBlockQ == 0 && Sk % kBlockK == 0 && Sq <= kMaxSeq && Sk <= kMaxSeq &&
         (!causal || Sk >= Sq) && static_cast<long long>(H) * (Sq / kBlockQ) <= kMaxBlocks;
}
inline int shape_text(int H, int Sq, int Sk, int causal, char* buf, int len) {
  return std::snprintf(buf, len,
                       "attention path: shape (%d,%d,%d) does not fit (Sq %% %d, Sk %% %d, both at most %d%s)", H, Sq, Sk,
                       kBlockQ, kBlockK, kMaxSeq, causal ? ", Sk >= Sq when causal" : "");
}

// Key j is visible to query i.
FORMS_HD bool visible(int i, int j, int Sq, int Sk, int causal) { return !causal || j <= i + (Sk - Sq); }
FORMS_HD int n_visible(int i, int Sq, int Sk, int causal) { return causal ? i + (Sk - Sq) + 1 : Sk; }

// Key tiles a workgroup's query block q0 .. q0 + 127 walks: the rate counts these.
FORMS_HD int tiles_of_block(int q0, int Sq, int Sk, int causal) {
  return causal ? (q0 + kBlockQ + (Sk - Sq)) / kBlockK : Sk / kBlockK;
}

// ---- the data ----
FORMS_HD uint16_t bf16_bits(float f) {  // exact for every value used here
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return static_cast<uint16_t>(u >> 16);
}
FORMS_HD uint64_t data_key(int which, int set, int head, int row, int d) {
  return (static_cast<uint64_t>(which + 1) << 58) ^ (static_cast<uint64_t>(set) << 54) ^ (static_cast<uint64_t>(head) << 32) ^
         (static_cast<uint64_t>(row) << 8) ^ static_cast<uint64_t>(d);
}
// a multiple of 1/4 in [-2, 2]
FORMS_HD float quarter(uint64_t key) { return (static_cast<int>(canary::mix32(key) % 17u) - 8) * 0.25f; }

// routed: key j points at dimension pi(j) & 127.  Within a block of 128 keys pi is a permutation
// (5 is odd), rotated by 3 per block, so query i's matching key of block b is match_key(i, b).
FORMS_HD int pi(int j) { return 5 * j + 3 * (j >> 7); }
FORMS_HD int match_key(int i, int b) {  // 5 * 77 = 385 = 3 * 128 + 1
  return 128 * b + static_cast<int>((77u * static_cast<uint32_t>((i & 127) - 3 * b)) & 127u);
}

FORMS_HD float q_val(int set, int head, int i, int d) {
  return set == kUniform ? 0.f : set == kRouted ? (d == (i & 127) ? 64.f : 0.f) : quarter(data_key(0, set, head, i, d));
}
FORMS_HD float k_val(int set, int head, int j, int d) {
  return set == kRouted ? (d == (pi(j) & 127) ? 64.f : 0.f) : quarter(data_key(1, set, head, j, d));
}
FORMS_HD int v_val(int set, int head, int j, int d) { return canary::small_int(data_key(2, set, head, j, d)); }  // in [-4, 4]

// ---- the exact sets: T_i, the visible keys of highest score ----
// uniform: every visible key (all scores are 0).  routed: the visible matching keys, one per
// block of 128 keys at most, score 64 * 64; every visible key if none matches.
struct Top {
  int count;      // |T_i|
  int matching;   // 1: T_i is the matching keys (raw score 4096), 0: every visible key (raw score 0)
};
FORMS_HD Top top_of(int set, int i, int Sq, int Sk, int causal) {
  int n = 0;
  if (set == kRouted)
    for (int b = 0; 128 * b < Sk; ++b) {
      const int j = match_key(i, b);
      n += j < Sk && visible(i, j, Sq, Sk, causal);
    }
  return n ? Top{n, 1} : Top{n_visible(i, Sq, Sk, causal), 0};
}
// The sum over T_i of V[j][d]: an integer of magnitude below 2^24.
FORMS_HD int top_sum(int set, int head, int i, int d, Top t, int Sq, int Sk, int causal) {
  int s = 0;
  if (t.matching) {
    for (int b = 0; 128 * b < Sk; ++b) {
      const int j = match_key(i, b);
      if (j < Sk && visible(i, j, Sq, Sk, causal)) s += v_val(set, head, j, d);
    }
  } else {
    for (int j = 0; j < t.count; ++j) s += v_val(set, head, j, d);  // the visible keys are 0 .. count - 1
  }
  return s;
}
// What a healthy kernel writes: one IEEE division of two exact floats.
FORMS_HD float expected_o(int sum, Top t) { return static_cast<float>(sum) / static_cast<float>(t.count); }
inline double expected_lse(Top t) { return std::log(static_cast<double>(t.count)) + (t.matching ? 4096.0 / std::sqrt(128.0) : 0.0); }

// ---- the bounds (derived: P rounded to bf16 is 2^-9 relative per term, once more for the row sum) ----
constexpr double kOBound = 1.0 / 64;  // 2^-8 * max|V| = 2^-8 * 4
FORMS_HD bool lse_within(double got, double ref) {
  const double e = got - ref, a = ref < 0 ? -ref : ref;
  return (e < 0 ? -e : e) <= 1.0 / 256 + a / 1048576;  // 2^-8 + 2^-20 |ref|; false for a NaN
}

// ---- the hashed set's checked rows: the corners of the first and last query block, then hashed ones ----
inline int checked_row(int n, int head, int Sq) {
  const int corners[4] = {0, kBlockQ - 1, Sq - kBlockQ, Sq - 1};
  return n < 4 ? corners[n] : static_cast<int>(canary::mix32(0xA77Eull << 40 ^ static_cast<uint64_t>(head) << 16 ^ n) % static_cast<uint32_t>(Sq));
}
// float64 softmax attention of one row of set `set`: o[128] and the natural-log lse.
inline void reference_row(int set, int head, int i, int Sq, int Sk, int causal, double* o, double* lse) {
  const int n = n_visible(i, Sq, Sk, causal);
  double q[kD], m = -INFINITY, l = 0;
  for (int d = 0; d < kD; ++d) q[d] = q_val(set, head, i, d), o[d] = 0;
  double* s = new double[n];
  for (int j = 0; j < n; ++j) {
    double dot = 0;
    for (int d = 0; d < kD; ++d) dot += q[d] * k_val(set, head, j, d);
    s[j] = dot / std::sqrt(128.0);
    m = s[j] > m ? s[j] : m;
  }
  for (int j = 0; j < n; ++j) {
    const double p = std::exp(s[j] - m);
    l += p;
    for (int d = 0; d < kD; ++d) o[d] += p * v_val(set, head, j, d);
  }
  for (int d = 0; d < kD; ++d) o[d] /= l;
  *lse = m + std::log(l);
  delete[] s;
}

// ---- the texts ----
// "attention path: 3 wrong elements in routed (first at head 2, row 17, d 5; causal, 8x1024x1024)",
// "attention path: 2 wrong lse values in hashed (first at head 0, row 3; 8x1024x1024)"; 0 and an
// empty text if every set was right.
inline int describe(const amdgpu_attn_result& r, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  const char* mask = r.causal ? "causal, " : "";
  for (int s = 0; s < kAttnSets; ++s) {
    if (r.o_errors[s]) {
      const unsigned long long at = r.first_bad[s], row = at / kD;
      return std::snprintf(buf, len, "attention path: %llu wrong element%s in %s (first at head %llu, row %llu, d %llu; %s%dx%dx%d)",
                           r.o_errors[s], r.o_errors[s] == 1 ? "" : "s", set_name(s), row / r.seq_q, row % r.seq_q, at % kD,
                           mask, r.heads, r.seq_q, r.seq_k);
    }
    if (r.lse_errors[s]) {
      const unsigned long long row = r.first_bad_lse[s];
      return std::snprintf(buf, len, "attention path: %llu wrong lse value%s in %s (first at head %llu, row %llu; %s%dx%dx%d)",
                           r.lse_errors[s], r.lse_errors[s] == 1 ? "" : "s", set_name(s), row / r.seq_q, row % r.seq_q, mask,
                           r.heads, r.seq_q, r.seq_k);
    }
  }
  return 0;
}

}  // namespace attn
