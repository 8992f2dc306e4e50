// What the host and the device of the decode-attention check must agree on, written once: the
// shape rules and the refusals, the partition rule, the block table and the sequence lengths of
// the check, the three data sets, the closed form of what a healthy kernel gives for the two
// exact ones, the float64 reference of the third, the result and its texts.  The hash and the
// small integers are ../mfma_forms.h's.  No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../mfma_forms.h"

extern "C" {

constexpr int kDecodeSets = 3;  // 0 uniform, 1 routed, 2 hashed

struct amdgpu_decode_result {                    // 168 bytes
  unsigned long long o_errors[kDecodeSets];      // wrong elements of o per set (the exact sets: bit mismatches)
  unsigned long long lse_errors[kDecodeSets];    // lse values outside the bound
  unsigned long long first_bad[kDecodeSets];     // (seq * Hq + head) * 128 + d of the first wrong element, ~0: none
  unsigned long long first_bad_lse[kDecodeSets]; // seq * Hq + head of the first wrong lse, ~0: none
  double ms[kDecodeSets];                        // device time of the `iters` timed launch pairs of each set
  double kv_gbps;                                // bytes of K and V of all visible pages per pair over that time
  double max_err;                                // hashed set: the largest |o - ref|
  double max_lse_err;                            // ... and the largest |lse - ref|
  int batch, q_heads, kv_heads, seq;
  int splits, iters;
};

}  // extern "C"

namespace decode {

constexpr int kD = 128;          // head dimension
constexpr int kPage = 16;        // keys of a page
constexpr int kTile = 128;       // keys of a tile: 4 waves of 32, 8 pages
constexpr int kPageBytes = kPage * kD * 2;  // one page of one KV head: 4 KiB
constexpr int kMaxSeq = 65536;   // 4 * 65536 < 2^24: the integer sums of the exact sets stay exact in fp32
constexpr int kMaxSplits = 64;
constexpr int kMaxBatch = 65536, kMaxHeads = 1024;
constexpr int kUniform = 0, kRouted = 1, kHashed = 2;

inline const char* set_name(int set) { return set == kUniform ? "uniform" : set == kRouted ? "routed" : set == kHashed ? "hashed" : "?"; }

// ---- the shape rules ----
FORMS_HD bool group_ok(int Hq, int Hkv) {
  if (Hq <= 0 || Hkv <= 0 || Hq > kMaxHeads || Hq % Hkv) return false;
  const int g = Hq / Hkv;
  return g == 1 || g == 2 || g == 4 || g == 8 || g == 16;
}
FORMS_HD bool shape_ok(int B, int Hq, int Hkv, int P, int max_pages) {
  return B > 0 && B <= kMaxBatch && group_ok(Hq, Hkv) && P > 0 && max_pages > 0 && max_pages <= kMaxSeq / kPage;
}
FORMS_HD int pages_of(int len) { return (len + kPage - 1) / kPage; }
FORMS_HD int tiles_of(int len) { return (len + kTile - 1) / kTile; }
// A partition is a whole number of tiles: partition s of `splits` walks tiles s * n .. s * n + n - 1.
FORMS_HD int tiles_per_split(int len, int splits) { return (tiles_of(len) + splits - 1) / splits; }

// The host's verdict on a call, before any HIP call: 0, or -1 with the text in `err`.
inline int refuse(int B, int Hq, int Hkv, int P, int max_pages, int splits, const int* table, const int* lens, char* err,
                  int err_len) {
  if (!shape_ok(B, Hq, Hkv, P, max_pages)) {
    std::snprintf(err, err_len,
                  "decode path: shape (%d,%d/%d,%d pages,%d per sequence) does not fit (positive, Hq = G Hkv with G in 1, 2, 4, "
                  "8, 16, at most %d keys)", B, Hq, Hkv, P, max_pages, kMaxSeq);
    return -1;
  }
  if (splits < 0 || splits > kMaxSplits) {
    std::snprintf(err, err_len, "decode path: splits %d does not fit (0 .. %d)", splits, kMaxSplits);
    return -1;
  }
  for (int b = 0; b < B; ++b) {
    if (lens[b] < 1 || lens[b] > kMaxSeq || lens[b] > kPage * max_pages) {
      std::snprintf(err, err_len, "decode path: seq_lens[%d] = %d does not fit (1 .. %d, the table's %d pages)", b, lens[b],
                    kMaxSeq < kPage * max_pages ? kMaxSeq : kPage * max_pages, max_pages);
      return -1;
    }
    for (int t = 0; t < pages_of(lens[b]); ++t) {
      const int e = table[static_cast<size_t>(b) * max_pages + t];
      if (e < 0 || e >= P) {
        std::snprintf(err, err_len, "decode path: block_table[%d][%d] = %d does not fit (pages 0 .. %d)", b, t, e, P - 1);
        return -1;
      }
    }
  }
  return 0;
}

// splits = 0: the smallest value that gives `want` workgroups, at most 64 and the longest sequence's tiles.
inline int choose_splits(int B, int Hkv, int longest, int want) {
  const long long wgs = static_cast<long long>(B) * Hkv;
  int s = static_cast<int>((want + wgs - 1) / wgs);
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > tiles_of(longest)) s = tiles_of(longest);
  return s < 1 ? 1 : s;
}

// ---- the check's sequences and its block table ----
FORMS_HD int check_len(int b, int seq) {  // hashed in [seq / 2, seq]; the first is seq, the second odd
  const int lo = seq / 2 > 1 ? seq / 2 : 1;
  int len = lo + static_cast<int>(canary::mix32(0xDEC0ull << 40 ^ static_cast<uint64_t>(b)) % static_cast<uint32_t>(seq - lo + 1));
  if (b == 0) len = seq;
  if (b == 1 && !(len & 1)) len += len < seq ? 1 : -1;
  return len < 1 ? 1 : len;
}
inline int gcd(long long a, long long b) { return b ? gcd(b, a % b) : static_cast<int>(a); }
// Logical page n (sequence b, entry t: n = b * max_pages + t) sits at physical page
// (mult * n + add) mod P: a permutation of the P pages for a multiplier coprime to P, and not the identity.
struct Perm {
  long long P, mult, add;
  int at(long long n) const { return static_cast<int>((mult * n + add) % P); }
};
inline Perm check_perm(int P) {
  long long mult = canary::mix32(0x7AB1Eull << 40 ^ static_cast<uint64_t>(P)) % static_cast<uint32_t>(P);
  while (gcd(mult, P) != 1 || (P > 2 && mult == 1)) mult = mult + 1 < P ? mult + 1 : 1;
  return Perm{P, mult, canary::mix32(0xADDull << 40 ^ static_cast<uint64_t>(P)) % static_cast<uint32_t>(P)};
}
// table [B][max_pages] (-1 past a sequence's last page) and lens [B] of the check at `seq` keys: P = B * max_pages pages.
inline void check_table(int B, int seq, int* table, int* lens) {
  const int max_pages = pages_of(seq);
  const Perm perm = check_perm(B * max_pages);
  for (int b = 0; b < B; ++b) {
    lens[b] = check_len(b, seq);
    for (int t = 0; t < max_pages; ++t)
      table[static_cast<size_t>(b) * max_pages + t] = t < pages_of(lens[b]) ? perm.at(static_cast<long long>(b) * max_pages + t) : -1;
  }
}

// ---- the data: functions of (set, sequence, head, key, d) ----
FORMS_HD uint16_t bf16_bits(float f) {  // exact for every value used here
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return static_cast<uint16_t>(u >> 16);
}
FORMS_HD uint64_t data_key(int which, int set, int b, int head, int key, int d) {
  return (static_cast<uint64_t>(which + 1) << 58) ^ (static_cast<uint64_t>(set) << 54) ^ (static_cast<uint64_t>(b) << 34) ^
         (static_cast<uint64_t>(head) << 24) ^ (static_cast<uint64_t>(key) << 7) ^ static_cast<uint64_t>(d);
}
// a multiple of 1/4 in [-2, 2]
FORMS_HD float quarter(uint64_t key) { return (static_cast<int>(canary::mix32(key) % 17u) - 8) * 0.25f; }

// routed: key j points at dimension pi(j) & 127.  Within a block of 128 keys pi is a permutation
// (5 is odd), rotated by 3 per block, so the key of block blk that matches dimension i is match_key(i, blk).
FORMS_HD int pi(int j) { return 5 * j + 3 * (j >> 7); }
FORMS_HD int match_key(int i, int blk) {  // 5 * 77 = 385 = 3 * 128 + 1
  return 128 * blk + static_cast<int>((77u * static_cast<uint32_t>((i & 127) - 3 * blk)) & 127u);
}
FORMS_HD int routed_dim(int b, int hq) { return (hq + 5 * b) & 127; }

FORMS_HD float q_val(int set, int b, int hq, int d) {
  return set == kUniform ? 0.f : set == kRouted ? (d == routed_dim(b, hq) ? 64.f : 0.f) : quarter(data_key(0, set, b, hq, 0, d));
}
FORMS_HD float k_val(int set, int b, int kvh, int j, int d) {
  return set == kRouted ? (d == (pi(j) & 127) ? 64.f : 0.f) : quarter(data_key(1, set, b, kvh, j, d));
}
FORMS_HD int v_val(int set, int b, int kvh, int j, int d) { return canary::small_int(data_key(2, set, b, kvh, j, d)); }  // in [-4, 4]

// ---- the exact sets: T, the visible keys of highest score ----
// uniform: every visible key (all scores are 0).  routed: the visible matching keys, one per
// block of 128 keys at most, score 64 * 64; every visible key if none matches.
struct Top {
  int count;      // |T|
  int matching;   // 1: T is the matching keys (raw score 4096), 0: every visible key (raw score 0)
};
FORMS_HD Top top_of(int set, int b, int hq, int len) {
  int n = 0;
  if (set == kRouted)
    for (int blk = 0; 128 * blk < len; ++blk) n += match_key(routed_dim(b, hq), blk) < len;
  return n ? Top{n, 1} : Top{len, 0};
}
// The sum over T of V[j][d]: an integer of magnitude below 2^24.
FORMS_HD int top_sum(int set, int b, int hq, int kvh, int d, Top t, int len) {
  int s = 0;
  if (t.matching) {
    for (int blk = 0; 128 * blk < len; ++blk) {
      const int j = match_key(routed_dim(b, hq), blk);
      if (j < len) s += v_val(set, b, kvh, j, d);
    }
  } else {
    for (int j = 0; j < len; ++j) s += v_val(set, b, kvh, j, d);
  }
  return s;
}
// What a healthy kernel writes: one IEEE division of two exact floats.
FORMS_HD float expected_o(int sum, Top t) { return static_cast<float>(sum) / static_cast<float>(t.count); }
FORMS_HD double expected_lse(Top t) {
  return std::log(static_cast<double>(t.count)) + (t.matching ? 4096.0 / 11.313708498984761 /* sqrt(128) */ : 0.0);
}

// ---- the bounds (derived: P rounded to bf16 is 2^-9 relative per term, once more for the sum, a few 2^-24 per merge) ----
constexpr double kOBound = (1.0 / 256 + 1.0 / 1048576) * 4;  // (2^-8 + 2^-20) max|V|
FORMS_HD bool lse_within(double got, double ref) {
  const double e = got - ref, a = ref < 0 ? -ref : ref;
  return (e < 0 ? -e : e) <= 1.0 / 256 + a / 1048576;  // 2^-8 + 2^-20 |ref|; false for a NaN
}

// float64 softmax attention of the G query heads of KV head kvh of sequence b over its first `len`
// keys: o [G][128] and the natural-log lse [G].  K and V are generated once per key for all G heads.
inline void reference_group(int set, int b, int kvh, int G, int len, double* o, double* lse) {
  double q[16][kD], m[16], l[16], k[kD], v[kD];
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY, l[g] = 0;
    for (int d = 0; d < kD; ++d) q[g][d] = q_val(set, b, kvh * G + g, d), o[g * kD + d] = 0;
  }
  for (int j = 0; j < len; ++j) {
    for (int d = 0; d < kD; ++d) k[d] = k_val(set, b, kvh, j, d), v[d] = v_val(set, b, kvh, j, d);
    for (int g = 0; g < G; ++g) {
      double dot = 0;
      for (int d = 0; d < kD; ++d) dot += q[g][d] * k[d];
      const double s = dot / std::sqrt(128.0);
      if (s > m[g]) {  // the running maximum moves: rescale what was summed
        const double a = std::exp(m[g] - s);
        l[g] *= a;
        for (int d = 0; d < kD; ++d) o[g * kD + d] *= a;
        m[g] = s;
      }
      const double p = std::exp(s - m[g]);
      l[g] += p;
      for (int d = 0; d < kD; ++d) o[g * kD + d] += p * v[d];
    }
  }
  for (int g = 0; g < G; ++g) {
    for (int d = 0; d < kD; ++d) o[g * kD + d] /= l[g];
    lse[g] = m[g] + std::log(l[g]);
  }
}

// ---- the texts ----
// "decode path: 1 wrong element in routed (first at seq 2, head 5, d 17; 8x32/4x4096, 7 splits)",
// "decode path: 2 wrong lse values in hashed (first at seq 0, head 3; 8x32/4x4096, 7 splits)"; 0 and
// an empty text if every set was right.
inline int describe(const amdgpu_decode_result& r, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  for (int s = 0; s < kDecodeSets; ++s) {
    if (r.o_errors[s]) {
      const unsigned long long at = r.first_bad[s], row = at / kD;
      return std::snprintf(buf, len, "decode path: %llu wrong element%s in %s (first at seq %llu, head %llu, d %llu; %dx%d/%dx%d, %d splits)",
                           r.o_errors[s], r.o_errors[s] == 1 ? "" : "s", set_name(s), row / r.q_heads, row % r.q_heads, at % kD,
                           r.batch, r.q_heads, r.kv_heads, r.seq, r.splits);
    }
    if (r.lse_errors[s]) {
      const unsigned long long row = r.first_bad_lse[s];
      return std::snprintf(buf, len, "decode path: %llu wrong lse value%s in %s (first at seq %llu, head %llu; %dx%d/%dx%d, %d splits)",
                           r.lse_errors[s], r.lse_errors[s] == 1 ? "" : "s", set_name(s), row / r.q_heads, row % r.q_heads,
                           r.batch, r.q_heads, r.kv_heads, r.seq, r.splits);
    }
  }
  return 0;
}

}  // namespace decode
