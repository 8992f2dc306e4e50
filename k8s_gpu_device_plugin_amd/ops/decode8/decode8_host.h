// What the host and the device of the fp8 decode-attention check must agree on, written once: the
// e4m3 codes, the per-KV-head scales, the refusals, the three data sets as codes, the closed form of
// what a healthy kernel gives for the two exact ones, the float64 reference of the third, the
// bounds, the result and its texts.  Everything that does not depend on the element type (the shape
// and partition rules, the check's lengths and block table, the routed permutation, T and its sum,
// the lse bound) is ../decode/decode_host.h's.  No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <cstring>

#include "../decode/decode_host.h"

extern "C" {

struct amdgpu_decode8_result {                   // 168 bytes, the fields of amdgpu_decode_result
  unsigned long long o_errors[kDecodeSets];      // wrong elements of o per set (the exact sets: bit mismatches)
  unsigned long long lse_errors[kDecodeSets];    // lse values outside the bound
  unsigned long long first_bad[kDecodeSets];     // (seq * Hq + head) * 128 + d of the first wrong element, ~0: none
  unsigned long long first_bad_lse[kDecodeSets]; // seq * Hq + head of the first wrong lse, ~0: none
  double ms[kDecodeSets];                        // device time of the `iters` timed launch pairs of each set
  double kv_gbps;                                // bytes of K and V of all visible pages per pair over that time
  double max_err;                                // hashed set: the largest |o - ref| / v_scale
  double max_lse_err;                            // ... and the largest |lse - ref|
  int batch, q_heads, kv_heads, seq;
  int splits, iters;
};

}  // extern "C"

namespace decode8 {

using decode::kD;
using decode::kHashed;
using decode::kMaxSeq;
using decode::kMaxSplits;
using decode::kPage;
using decode::kRouted;
using decode::kTile;
using decode::kUniform;
using decode::group_ok;
using decode::lse_within;
using decode::pages_of;
using decode::shape_ok;
using decode::tiles_per_split;
using decode::Top;

constexpr int kPageBytes = kPage * kD;  // one page of one KV head: 2 KiB
constexpr uint8_t kPoison = 0xFF;       // an e4m3 NaN: what the check's caches hold wherever no visible key lies

// ---- OCP e4m3 (the gfx950 fp8): bias 7, largest value 448, 0x7F / 0xFF are NaN, no infinity ----
FORMS_HD float fp8_value(uint8_t code) {
  const int e = (code >> 3) & 15, m = code & 7;
  if (e == 15 && m == 7) return NAN;
  float x = e ? (8 + m) * 0.125f : m * 0.125f;           // 1.m, or 0.m of a subnormal
  for (int i = e ? e : 1; i < 7; ++i) x *= 0.5f;          // 2^(e - 7), subnormals 2^-6
  for (int i = 7; i < e; ++i) x *= 2.f;
  return code & 0x80 ? -x : x;
}
// The code of n / 4 for n in [-8, 8], and of +-64 (n = +-256): the K values of the three sets.  Zero is 0x00.
FORMS_HD uint8_t quarter_code(int n) {
  const int a = n < 0 ? -n : n;
  const int c = a == 0 ? 0x00 : a == 1 ? 0x28 : a == 2 ? 0x30 : a == 3 ? 0x34 : a < 8 ? 0x38 + 2 * (a - 4) : a == 8 ? 0x40 : 0x68;
  return static_cast<uint8_t>(n < 0 ? c | 0x80 : c);
}

// ---- the scales, per KV head ----
// exact sets: powers of two that differ per head; hashed: a multiple of 2^-10 in (1/2, 2), never a power of two
FORMS_HD float k_scale_of(int set, int kvh) {
  if (set != kHashed) return kvh & 1 ? 0.5f : 1.f;
  uint32_t n = 1 + canary::mix32(0x5CA1Eull << 40 ^ static_cast<uint64_t>(kvh)) % 1535u;
  if (n == 512) ++n;
  return 0.5f + n * (1.f / 1024);
}
FORMS_HD float v_scale_of(int set, int kvh) {
  if (set != kHashed) return kvh % 3 == 0 ? 0.25f : kvh % 3 == 1 ? 1.f : 2.f;
  uint32_t n = 1 + canary::mix32(0x5CA1Full << 40 ^ static_cast<uint64_t>(kvh)) % 1535u;
  if (n == 512) ++n;
  return 0.5f + n * (1.f / 1024);
}
FORMS_HD bool scale_ok(float s) { return s > 0.f && s <= 3.4028234663852886e38f; }  // finite and positive; false for a NaN

// ---- the data as codes: decode's values (Q as bf16 there and here), K and V as e4m3 ----
using decode::q_val;
FORMS_HD uint8_t k_code(int set, int b, int kvh, int j, int d) { return quarter_code(static_cast<int>(decode::k_val(set, b, kvh, j, d) * 4.f)); }
FORMS_HD uint8_t v_code(int set, int b, int kvh, int j, int d) {
  return static_cast<uint8_t>(canary::lowp_code<canary::kFp8>(decode::v_val(set, b, kvh, j, d)));
}

// ---- the exact sets ----
// What a healthy pair writes: one IEEE division of two exact floats and one exact scaling by a power of two.
FORMS_HD float expected_o(int sum, Top t, float v_scale) { return static_cast<float>(sum) / static_cast<float>(t.count) * v_scale; }
FORMS_HD double expected_lse(Top t, float k_scale) {
  return std::log(static_cast<double>(t.count)) + (t.matching ? k_scale * 4096.0 / 11.313708498984761 /* sqrt(128) */ : 0.0);
}

// ---- the bounds (derived) ----
// decode's derivation carries over, because e4m3 -> bf16 is exact: P rounded to bf16 is 2^-9 relative
// per term, once more for the sum: 2^-8.  The small term is re-derived for the folded factor.  The
// largest score of the hashed set is |q k| <= 128 * 2 * 2 = 512 times k_scale < 2: X = 1024 log2(e) /
// sqrt(128) = 130.6 in the base-2 domain.  x = fl(s fl(k_scale c)) with c a rounded constant carries
// 3 * 2^-24 X, m (one of the x) the same, x - m one rounding of at most 2 X: 8 X 2^-24 < 2^-14 on the
// exponent, ln2 of that relative on p, twice that on a quotient of sums of p: below 9e-5.  The
// merges, the division and the epilogue's multiply add a few 2^-24 more: eps = 2^-13 covers all.
// lse = ln2 (m + log2 l), with l from the unrounded p, moves by a few 2^-24 |ref|: decode's lse_within holds.
constexpr double kOBoundPerVScale = (1.0 / 256 + 1.0 / 8192) * 4;  // (2^-8 + 2^-13) max|V|, times v_scale

// float64 softmax attention of the G query heads of KV head kvh of sequence b over its first `len`
// keys of the dequantised cache: o [G][128] and the natural-log lse [G].
inline void reference_group(int set, int b, int kvh, int G, int len, double* o, double* lse) {
  const double ks = k_scale_of(set, kvh), vs = v_scale_of(set, kvh);
  double q[16][kD], m[16], l[16], k[kD], v[kD];
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY, l[g] = 0;
    for (int d = 0; d < kD; ++d) q[g][d] = q_val(set, b, kvh * G + g, d), o[g * kD + d] = 0;
  }
  for (int j = 0; j < len; ++j) {
    for (int d = 0; d < kD; ++d) k[d] = ks * fp8_value(k_code(set, b, kvh, j, d)), v[d] = vs * fp8_value(v_code(set, b, kvh, j, d));
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

// ---- the refusals: decode's, in its wording, and the scales ----
inline int refuse(int B, int Hq, int Hkv, int P, int max_pages, int splits, const int* table, const int* lens, const float* k_scale,
                  const float* v_scale, char* err, int err_len) {
  char text[256];
  if (decode::refuse(B, Hq, Hkv, P, max_pages, splits, table, lens, text, sizeof(text)) != 0) {
    std::snprintf(err, err_len, "decode8 path:%s", text + std::strlen("decode path:"));
    return -1;
  }
  for (int which = 0; which < 2; ++which)
    for (int h = 0; h < Hkv; ++h) {
      const float s = (which ? v_scale : k_scale)[h];
      if (!scale_ok(s)) {
        std::snprintf(err, err_len, "decode8 path: %s_scale[%d] = %g does not fit (finite, > 0)", which ? "v" : "k", h, static_cast<double>(s));
        return -1;
      }
    }
  return 0;
}

// ---- the texts ----
// "decode8 path: 1 wrong element in routed (first at seq 2, head 5, d 17; 8x32/4x4096, 7 splits)",
// "decode8 path: 2 wrong lse values in hashed (first at seq 0, head 3; 8x32/4x4096, 7 splits)"; 0 and
// an empty text if every set was right.
inline int describe(const amdgpu_decode8_result& r, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  for (int s = 0; s < kDecodeSets; ++s) {
    if (r.o_errors[s]) {
      const unsigned long long at = r.first_bad[s], row = at / kD;
      return std::snprintf(buf, len, "decode8 path: %llu wrong element%s in %s (first at seq %llu, head %llu, d %llu; %dx%d/%dx%d, %d splits)",
                           r.o_errors[s], r.o_errors[s] == 1 ? "" : "s", decode::set_name(s), row / r.q_heads, row % r.q_heads, at % kD,
                           r.batch, r.q_heads, r.kv_heads, r.seq, r.splits);
    }
    if (r.lse_errors[s]) {
      const unsigned long long row = r.first_bad_lse[s];
      return std::snprintf(buf, len, "decode8 path: %llu wrong lse value%s in %s (first at seq %llu, head %llu; %dx%d/%dx%d, %d splits)",
                           r.lse_errors[s], r.lse_errors[s] == 1 ? "" : "s", decode::set_name(s), row / r.q_heads, row % r.q_heads,
                           r.batch, r.q_heads, r.kv_heads, r.seq, r.splits);
    }
  }
  return 0;
}

}  // namespace decode8
