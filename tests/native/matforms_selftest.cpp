// Stand-alone self-test of the matrix-forms check's host side (ops/matforms/matforms_forms.h,
// ops/matforms/matforms_host.h): no HIP, no Python, no GPU.  tests/test_matforms_selftest.py
// compiles it with g++ -fsanitize=address,undefined and runs it directly; it exits 0 and prints
// "ok", or prints what failed and exits 1.
//
// For every form of the table it emulates the MFMA from the operands alone: every lane's
// operand words are built by the code the kernels run (form_operands), decoded back to integers
// by decoders written here from the formats' definitions, placed into A[M][K] and B[K][M] by
// k_of_a / k_of_b, scaled by the byte of the lane that holds each k-block, multiplied in int64
// and read through cd_row.  What each lane reads must be the reference the kernels compare with
// (form_ref), for ksteps 1, 3 and 8, scales fixed and varied.  Then the reduction of
// matforms_host.h on hand-built records: located and moved waves, coverage, the error text, and
// 17 bad sites of which 16 are listed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "matforms/matforms_host.h"

namespace {

using namespace matforms;

int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// ---- decoders, from the formats' definitions (not from the Enc* of the header) ---------------
// sign, ebits, mbits minifloat without infinities or NaNs in the range used
double minifloat(uint64_t code, int ebits, int mbits, int bias) {
  const int sign = (code >> (ebits + mbits)) & 1;
  const int e = (code >> mbits) & ((1u << ebits) - 1);
  const int m = code & ((1u << mbits) - 1);
  const double v = e ? std::ldexp(1.0 + m / static_cast<double>(1 << mbits), e - bias) : std::ldexp(m / static_cast<double>(1 << mbits), 1 - bias);
  return sign ? -v : v;
}
double decode(EncF16*, uint64_t c) { return minifloat(c, 5, 10, 15); }
double decode(EncBf16*, uint64_t c) { return minifloat(c, 8, 7, 127); }
double decode(EncI8*, uint64_t c) { return static_cast<double>(static_cast<int8_t>(static_cast<uint8_t>(c))); }
double decode(EncF32*, uint64_t c) {
  const uint32_t u = static_cast<uint32_t>(c);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
double decode(EncF64*, uint64_t c) {
  double d;
  std::memcpy(&d, &c, 8);
  return d;
}
double decode(EncLowp<kFp8>*, uint64_t c) { return minifloat(c, 4, 3, 7); }
double decode(EncLowp<kBf8>*, uint64_t c) { return minifloat(c, 5, 2, 15); }
double decode(EncLowp<kFp6>*, uint64_t c) { return minifloat(c, 2, 3, 1); }
double decode(EncLowp<kBf6>*, uint64_t c) { return minifloat(c, 3, 2, 3); }
double decode(EncLowp<kFp4>*, uint64_t c) { return minifloat(c, 2, 1, 1); }

// element j, `bits` wide at bit j * bits of the operand's words
uint64_t element(const uint32_t* w, int words, int j, int bits) {
  uint64_t all[5] = {0, 0, 0, 0, 0};  // the operand as 64-bit pieces, one spare
  for (int i = 0; i < words; ++i) all[i / 2] |= static_cast<uint64_t>(w[i]) << (32 * (i % 2));
  const int p = j * bits, i = p / 64, sh = p % 64;
  uint64_t v = all[i] >> sh;
  if (sh + bits > 64) v |= all[i + 1] << (64 - sh);
  return bits == 64 ? v : v & ((1ull << bits) - 1);
}

template <class Enc>
int64_t integer_of(uint64_t code) {
  const double v = decode(static_cast<Enc*>(nullptr), code);
  CHECK(v == std::floor(v));
  return static_cast<int64_t>(v);
}

// C[M][M] of one wave, emulated from the operands
template <class F>
std::vector<int64_t> emulate(uint32_t key, int ksteps, int vary, bool inject) {
  constexpr int M = F::kM, K = F::kK, blocks = F::kScaled ? K / 32 : 1;
  std::vector<int64_t> C(M * M, 0);
  for (int s = 0; s < ksteps; ++s) {
    std::vector<int64_t> A(M * K, 1 << 30), B(K * M, 1 << 30);
    std::vector<int> SA(M * blocks, 0), SB(M * blocks, 0);
    for (int lane = 0; lane < 64; ++lane) {
      const int r = lane % M, g = lane / M;
      typename F::operand_a a;
      typename F::operand_b b;
      int sa, sb;
      form_operands<F>(key, lane, s, vary, inject, a, b, sa, sb);
      for (int j = 0; j < F::kElems; ++j) {
        const int ka = F::k_of_a(g, j), kb = F::k_of_b(g, j);
        CHECK(ka >= 0 && ka < K && kb >= 0 && kb < K);
        CHECK(A[r * K + ka] == (1 << 30) && B[kb * M + r] == (1 << 30));  // each (row, k) held once
        A[r * K + ka] = integer_of<typename F::EA>(element(a.w, F::kWordsA, j, F::EA::kBits));
        B[kb * M + r] = integer_of<typename F::EB>(element(b.w, F::kWordsB, j, F::EB::kBits));
        CHECK(std::llabs(A[r * K + ka]) <= F::kR && std::llabs(B[kb * M + r]) <= F::kR);
      }
      if (F::kScaled) {  // the lane's byte: k-block g of its row of A and of its column of B
        CHECK(g < blocks && (sa == 127 || (vary && sa == 128)) && (sb == 127 || (vary && sb == 128)));
        SA[r * blocks + g] = sa - 127;
        SB[r * blocks + g] = sb - 127;
      } else {
        CHECK(sa == 127 && sb == 127);
      }
    }
    for (int row = 0; row < M; ++row)
      for (int col = 0; col < M; ++col)
        for (int k = 0; k < K; ++k) {
          const int blk = F::kScaled ? k / 32 : 0;
          C[row * M + col] += A[row * K + k] * B[k * M + col] * (1ll << (SA[row * blocks + blk] + SB[col * blocks + blk]));
        }
  }
  return C;
}

template <class F>
void test_form() {
  constexpr int M = F::kM;
  static_assert(F::kK == F::kElems * 64 / M && F::kAcc * 64 == M * M, "every element of A, B and C is held once");
  static_assert(F::kWordsA <= kOperandWords && F::kWordsB <= kOperandWords, "a raw operand has room");
  static_assert((F::kAccKind == kAccF64 ? 2 : 1) * F::kAcc <= kAccWords, "raw accumulators have room");
  for (int ksteps : {1, 3, 8})
    for (int vary = 0; vary < 2; ++vary)
      for (uint32_t key : {0u, 9u, (2u << 14) | 1234u}) {
        const std::vector<int64_t> C = emulate<F>(key, ksteps, vary, false);
        std::vector<int> seen(M * M, 0);
        int64_t largest = 0;
        for (int lane = 0; lane < 64; ++lane)
          for (int reg = 0; reg < F::kAcc; ++reg) {
            const int row = F::cd_row(reg, lane / M), col = lane % M;
            CHECK(row >= 0 && row < M);
            ++seen[row * M + col];
            const int64_t ref = form_ref<F>(key, row, col, ksteps, vary);
            CHECK(C[row * M + col] == ref);
            largest = std::llabs(ref) > largest ? std::llabs(ref) : largest;
          }
        for (int v : seen) CHECK(v == 1);
        // exact in the accumulator type, whatever the order of the sums
        CHECK(largest < (F::kAccKind == kAccF32 ? 1ll << 24 : F::kAccKind == kAccI32 ? 1ll << 31 : 1ll << 53));
        if (ksteps == 3) {  // the injection: exactly the predicted elements, all in row 0
          const std::vector<int64_t> D = emulate<F>(key, ksteps, vary, true);
          int changed = 0;
          for (int i = 0; i < M * M; ++i) {
            changed += C[i] != D[i];
            CHECK(i < M || C[i] == D[i]);
          }
          CHECK(changed == inject_expected<F>(key));
        }
      }
  CHECK(F::perturbed(F::kR) == F::kR - 1 && F::perturbed(-F::kR) == -F::kR + 1 && F::perturbed(0) == 1);
}

amdgpu_matforms_record record(unsigned int first, unsigned int last, int form, unsigned int bad, unsigned int reg = 0) {
  amdgpu_matforms_record r;
  std::memset(&r, 0, sizeof(r));
  r.site_first = first;
  r.site_last = last;
  r.first_form = bad ? static_cast<unsigned int>(form) : kMatFormsNone;
  r.first_reg = bad ? reg : kMatFormsNone;
  r.bad[form] = bad;
  return r;
}

unsigned int site(unsigned int xcc, unsigned int se, unsigned int cu, unsigned int simd) {
  return xcc << 10 | se << 7 | cu << 2 | simd;
}

void test_reduce() {
  int i8 = -1, f64 = -1;
  for (int f = 0; f < kNumForms; ++f) {
    if (std::string(kForms[f].name) == "i8_32") i8 = f;
    if (std::string(kForms[f].name) == "f64_16") f64 = f;
    for (int g = 0; g < f; ++g) CHECK(std::string(kForms[f].name) != kForms[g].name && kForms[f].key_offset != kForms[g].key_offset);
  }
  CHECK(i8 >= 0 && f64 >= 0);
  if (i8 < 0 || f64 < 0) return;
  const unsigned int forms = 1u << i8 | 1u << f64;
  char text[256];
  amdgpu_matforms_result r;

  {  // healthy: two CUs, one of them with all four SIMDs reached by both forms, one by i8 alone
    std::vector<amdgpu_matforms_record> recs;
    std::vector<int> of;
    for (unsigned int simd = 0; simd < 4; ++simd)
      for (int f : {i8, f64}) {
        recs.push_back(record(site(1, 0, 2, simd), site(1, 0, 2, simd), f, 0));
        of.push_back(f);
      }
    recs.push_back(record(site(2, 1, 5, 0), site(2, 1, 5, 0), i8, 0));
    of.push_back(i8);
    recs.push_back(record(kMatFormsNone, kMatFormsNone, i8, 7));  // a slot no wave wrote
    of.push_back(i8);
    std::memset(&r, 0, sizeof(r));
    r.cus_expected = 2;
    r.ms = 1.5;
    CHECK(reduce(recs.data(), of.data(), static_cast<int>(recs.size()), forms, &r));
    CHECK(r.matforms_errors == 0 && r.waves == 9 && r.moved == 0 && r.form_waves[i8] == 5 && r.form_waves[f64] == 4);
    CHECK(r.cus_reached == 1 && r.simds_reached == 4 && r.n_bad == 0 && r.cus_expected == 2 && r.ms == 1.5 && r.forms == forms);
    CHECK(!canary::covered(r, r.cus_expected) && canary::covered(r, 1));
    CHECK(describe(r, -1, text, sizeof(text)) == 0 && text[0] == 0);
  }
  {  // located and moved: the moved wave's errors are unlocated and still fail the check
    const amdgpu_matforms_record recs[] = {
        record(site(3, 1, 7, 2), site(3, 1, 7, 2), i8, 3, 5), record(site(3, 1, 7, 2), site(3, 1, 7, 2), i8, 2, 9),
        record(site(4, 0, 1, 1), site(4, 0, 1, 1), i8, 0), record(site(5, 0, 0, 0), site(5, 0, 0, 1), f64, 4, 1),
        record(site(6, 0, 0, 3), site(6, 0, 0, 3), i8, 1, 2)};
    const int of[] = {i8, i8, i8, f64, i8};
    std::memset(&r, 0, sizeof(r));
    CHECK(reduce(recs, of, 5, forms, &r));
    CHECK(r.errors[i8] == 6 && r.errors[f64] == 0 && r.unlocated_errors == 4 && r.matforms_errors == 10);
    CHECK(r.waves == 4 && r.moved == 1 && r.n_bad == 2 && r.bad_sites[0] == site(3, 1, 7, 2) && r.bad_sites[1] == site(6, 0, 0, 3));
    CHECK(r.form_n_bad[i8] == 2 && r.form_first_site[i8] == site(3, 1, 7, 2) && r.form_first_reg[i8] == 5);
    describe(r, -1, text, sizeof(text));
    CHECK(std::string(text) == "matrix form check: 6 wrong results in i8 32x32x32 at xcc3/se1/sh0/cu7/simd2 (+1 more site)");
    CHECK(describe(r, f64, text, sizeof(text)) == 0);
    const amdgpu_matforms_record one[] = {record(site(5, 0, 0, 0), site(5, 0, 0, 1), f64, 1)};
    std::memset(&r, 0, sizeof(r));
    CHECK(reduce(one, of + 3, 1, forms, &r));
    describe(r, -1, text, sizeof(text));
    CHECK(std::string(text) == "matrix form check: 1 wrong result at an unknown site" && r.n_bad == 0 && r.matforms_errors == 1);
  }
  {  // 17 bad sites: 16 listed, all counted
    std::vector<amdgpu_matforms_record> recs;
    std::vector<int> of;
    for (unsigned int i = 0; i < 17; ++i) {
      recs.push_back(record(site(i % 8, i / 8, i, i % 4), site(i % 8, i / 8, i, i % 4), f64, 1));
      of.push_back(f64);
    }
    std::memset(&r, 0, sizeof(r));
    CHECK(reduce(recs.data(), of.data(), 17, forms, &r));
    CHECK(r.n_bad == 17 && r.form_n_bad[f64] == 17 && r.errors[f64] == 17);
    for (int i = 1; i < 16; ++i) CHECK(r.bad_sites[i] > r.bad_sites[i - 1]);
    describe(r, -1, text, sizeof(text));
    CHECK(std::string(text).find("17 wrong results in f64 16x16x4 at xcc0/se0/sh0/cu0/simd0 (+16 more sites)") != std::string::npos);
    char tiny[8];  // a short buffer is not overrun
    describe(r, -1, tiny, sizeof(tiny));
    CHECK(std::strlen(tiny) == 7);
  }
  {  // refused: a site out of range, a form outside the selection, no forms
    const amdgpu_matforms_record bad_site[] = {record(1u << 14, 1u << 14, i8, 0)};
    const int of[] = {i8};
    std::memset(&r, 0, sizeof(r));
    CHECK(!reduce(bad_site, of, 1, forms, &r));
    const amdgpu_matforms_record fine[] = {record(1, 1, i8, 0)};
    CHECK(!reduce(fine, of, 1, 1u << f64, &r) && !reduce(fine, of, 1, 0, &r) && !reduce(fine, of, 1, 1u << kNumForms, &r));
    CHECK(reduce(nullptr, nullptr, 0, forms, &r) && r.waves == 0);
  }
  CHECK(arguments_ok(0, 4, 1, kAllForms, -1, 0, 0, false) && arguments_ok(8, 8, 0, forms, i8, 3, 32, true));
  CHECK(!arguments_ok(-1, 4, 1, kAllForms, -1, 0, 0, false) && !arguments_ok(4097, 4, 1, kAllForms, -1, 0, 0, false));
  CHECK(!arguments_ok(0, 0, 1, kAllForms, -1, 0, 0, false) && !arguments_ok(0, 9, 1, kAllForms, -1, 0, 0, false));
  CHECK(!arguments_ok(0, 4, 2, kAllForms, -1, 0, 0, false) && !arguments_ok(0, 4, 1, 0, -1, 0, 0, false));
  CHECK(!arguments_ok(0, 4, 1, forms, kNumForms, 1, 0, false) && !arguments_ok(0, 4, 1, 1u << f64, i8, 1, 0, false));
  CHECK(!arguments_ok(0, 4, 1, kAllForms, -1, -1, 0, false) && !arguments_ok(0, 4, 1, kAllForms, -1, 0, 4, false));
}

}  // namespace

int main() {
  int forms = 0;
  for (int f = 0; f < kMaxForms; ++f)
    forms += with_form(f, [](auto form) { test_form<decltype(form)>(); });
  CHECK(forms == kNumForms && !with_form(-1, [](auto) {}));
  test_reduce();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("%d forms\nok\n", forms);
  return 0;
}
