// The LDS-path check's host side (ops/ldspath/ldspath_host.h) as a program of its own, for
// AddressSanitizer and UBSan: the tables, the maps, the expected atomic tables, the reduction
// and the texts, with nothing from HIP and nothing loaded into Python.  Prints "ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ldspath_host.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

unsigned int site(unsigned xcc, unsigned se, unsigned sh, unsigned cu, unsigned simd) {
  return xcc << 10 | se << 7 | sh << 6 | cu << 2 | simd;
}

amdgpu_ldspath_record rec(unsigned int s0, unsigned int s1, unsigned int sub, unsigned int at, unsigned int bad) {
  amdgpu_ldspath_record r;
  std::memset(&r, 0, sizeof(r));
  r.site_first = s0;
  r.site_last = s1;
  r.first_sub = bad ? sub : kLdsUnwritten;
  r.first_at = at;
  if (bad) r.bad[sub] = bad;
  return r;
}

std::string text(const amdgpu_ldspath_result& r, int which) {
  char buf[256];
  const int n = ldspath::describe(r, which, buf, sizeof(buf));
  CHECK(n == static_cast<int>(std::strlen(buf)));
  return buf;
}

void lane_tables() {
  using namespace ldspath;
  for (int k = 0; k < kNumLaneOps; ++k) {
    const LaneOp& op = kLaneOps[k];
    bool seen[64] = {};
    for (int o = 0; o < lane_outputs(op); ++o) {
      for (int l = 0; l < 64; ++l) {
        const int c = src_code(op, o, l);
        CHECK(c >= 0 && c <= kSrcZero);
        if (o == 0 && c < 64) seen[c] = true;
      }
    }
    if (lane_op_bijective(op)) CHECK(std::all_of(seen, seen + 64, [](bool b) { return b; }));
    if (op.kind == kOpPermute) CHECK((op.a * op.c) % 64 == 1);
    CHECK(kLaneOpNames[k] != nullptr && kLaneOpNames[k][0] != 0);
  }
  CHECK(lane_expected(7, 3, kSrcZero, 0) == 0u);
  CHECK(lane_expected(7, 3, 5, 2) == lane_value(7, 3, 5, 2, 0) && lane_expected(7, 3, 64 + 5, 2) == lane_value(7, 3, 5, 2, 1));
}

void transposed_read() {
  using namespace ldspath;
  for (int r = 0; r < tr_rounds(kMaxRounds); ++r) {
    for (int l = 0; l < 64; ++l) {
      const int a = tr_addr(l, r);
      CHECK(a >= 0 && a % 8 == 0 && a + 8 <= kTrImageBytes);
      for (int q = 0; q < 4; ++q) CHECK(tr_source(l, q, r) >= 0 && tr_source(l, q, r) < kTrElems);
    }
  }
  std::vector<unsigned char> seen(kTrElems, 0);
  for (int i = 0; i < kTrElems; ++i) seen[tr_pat(i, 0x1D5A)] = 1;  // a bijection: the multiplier is odd
  CHECK(std::all_of(seen.begin(), seen.end(), [](unsigned char b) { return b == 1; }));
}

void atomics() {
  using namespace ldspath;
  std::vector<uint32_t> t(kAtomWords);
  CHECK(!atomic_expected(-1, 1, t.data()) && !atomic_expected(kAtomForms, 1, t.data()) && !atomic_expected(0, 0, t.data()) &&
        !atomic_expected(0, kMaxSteps + 1, t.data()) && !atomic_expected(0, 1, nullptr));
  for (int f = 0; f < kAtomForms; ++f) CHECK(atomic_expected(f, kMaxSteps, t.data()));
  CHECK(atomic_expected(kAtomTicket, 3, t.data()) && t[0] == 3 && t[255] == 3 && t[256] == 768 && t[257] == 0);
  for (int th = 0; th < kThreads; ++th) {
    for (int s = 0; s < 4; ++s) {
      CHECK(static_cast<uint32_t>(atomic_operand(kAtomAnd, th, s, false)) & kInjectBit);
      CHECK(!(static_cast<uint32_t>(atomic_operand(kAtomOr, th, s, false)) & kInjectBit));
      const int64_t f = static_cast<int64_t>(atomic_operand(kAtomF32Add, th, s, false));
      CHECK(f >= -4 && f <= 4);
      CHECK(atomic_index(kAtomU64Add, th, s) < 256 && atomic_index(kAtomCas, th, s) < kAtomWords);
      for (int form = 0; form < kAtomForms; ++form)
        CHECK(atomic_operand(form, th, s, true) != atomic_operand(form, th, s, false));
    }
  }
}

void reduction() {
  const unsigned int a = site(3, 1, 0, 7, 2), b = site(4, 0, 1, 2, 1), a3 = site(3, 1, 0, 7, 3);
  const int none[kLdsStages] = {0, 0, 0, 0};
  const amdgpu_ldspath_record* const nothing[kLdsStages] = {nullptr, nullptr, nullptr, nullptr};
  amdgpu_ldspath_result r;
  std::memset(&r, 0, sizeof(r));
  CHECK(ldspath::reduce(nothing, none, &r) && r.ldspath_errors == 0 && r.waves == 0 && text(r, -1).empty());
  CHECK(!ldspath::reduce(nothing, none, nullptr));

  std::vector<amdgpu_ldspath_record> w = {rec(a, a, 3, 0x1a40, 3), rec(a3, a3, 0, 0, 0), rec(b, b, 0, 0x10, 1),
                                          rec(kLdsUnwritten, kLdsUnwritten, 0, 0, 0), rec(b, a, 1, 4, 5)};
  std::vector<amdgpu_ldspath_record> at = {rec(site(1, 0, 0, 3, 0), site(1, 0, 0, 3, 0), ldspath::kAtomU64Add, 41, 2)};
  std::vector<amdgpu_ldspath_record> ln = {rec(a, a, 20, 0, 4), rec(b, b, 20, 1, 1)};
  std::vector<amdgpu_ldspath_record> tr = {rec(a, a, 0, 2, 2)};
  const amdgpu_ldspath_record* const recs[kLdsStages] = {w.data(), at.data(), ln.data(), tr.data()};
  const int n[kLdsStages] = {5, 1, 2, 1};
  std::memset(&r, 0, sizeof(r));
  r.cus_expected = 256;
  CHECK(ldspath::reduce(recs, n, &r));
  CHECK(r.cus_expected == 256 && r.waves == 3 && r.moved == 1 && r.unlocated_errors == 5);
  CHECK(r.lds_errors == 4 && r.plain_errors == 1 && r.subword_errors == 3 && r.dma_errors == 0);
  CHECK(r.lds_atomic_errors == 2 && r.lane_errors == 5 && r.tr_errors == 2 && r.ldspath_errors == 4 + 2 + 5 + 2 + 5);
  CHECK(r.cus_reached == 2 && r.simds_reached == 3 && r.n_bad == 3 && r.bad_sites[0] == site(1, 0, 0, 3, 0));
  CHECK(text(r, 0) == "lds check: 4 wrong words at xcc3/se1/sh0/cu7 (pass 4, 8-bit store; first at offset 0x1a40; +1 more CU)");
  CHECK(text(r, 1) == "lds atomic check: 2 wrong elements in u64 add at xcc1/se0/sh0/cu3 (first at 41)");
  CHECK(text(r, 2) == "lane check: 5 wrong words in dpp row_ror:3 at xcc3/se1/sh0/cu7/simd2 (+1 more site)");
  CHECK(text(r, 3) == "lds transpose check: 2 wrong elements at xcc3/se1/sh0/cu7/simd2");
  CHECK(text(r, -1) == text(r, 0));

  // dma alone fails the check; beside a plain error it is reported and not added
  std::vector<amdgpu_ldspath_record> d = {rec(a, a, 4, 0x40, 1)};
  const amdgpu_ldspath_record* const only_dma[kLdsStages] = {d.data(), nullptr, nullptr, nullptr};
  const int one[kLdsStages] = {1, 0, 0, 0};
  std::memset(&r, 0, sizeof(r));
  CHECK(ldspath::reduce(only_dma, one, &r) && r.dma_errors == 1 && r.lds_errors == 0 && r.ldspath_errors == 1);
  CHECK(text(r, -1) == "lds dma check: 1 wrong word at xcc3/se1/sh0/cu7 (pass 5, dma fill; first at offset 0x40)");
  const std::vector<amdgpu_ldspath_record> d2 = {d[0], rec(b, b, 0, 8, 2)};
  const amdgpu_ldspath_record* const dma_and_plain[kLdsStages] = {d2.data(), nullptr, nullptr, nullptr};
  const int two[kLdsStages] = {2, 0, 0, 0};
  std::memset(&r, 0, sizeof(r));
  CHECK(ldspath::reduce(dma_and_plain, two, &r) && r.dma_errors == 1 && r.lds_errors == 2 && r.ldspath_errors == 2);

  // every wrong wave moved
  std::vector<amdgpu_ldspath_record> m = {rec(a, b, 0, 0, 4)};
  const amdgpu_ldspath_record* const moved[kLdsStages] = {nullptr, nullptr, m.data(), nullptr};
  const int lane_one[kLdsStages] = {0, 0, 1, 0};
  std::memset(&r, 0, sizeof(r));
  CHECK(ldspath::reduce(moved, lane_one, &r) && r.ldspath_errors == 4 && r.lane_errors == 0 && r.stage_moved[2] == 1);
  CHECK(text(r, -1) == "ldspath check: 4 wrong words at an unknown site" && text(r, 2).empty());

  // a site out of range is refused
  m[0] = rec(kLdsSiteSlots, kLdsSiteSlots, 0, 0, 1);
  CHECK(!ldspath::reduce(moved, lane_one, &r));
  const int negative[kLdsStages] = {0, -1, 0, 0};
  CHECK(!ldspath::reduce(nothing, negative, &r));

  // a buffer too small for the text is not overrun
  char tiny[8];
  std::memset(&r, 0, sizeof(r));
  CHECK(ldspath::reduce(recs, n, &r));
  ldspath::describe(r, 0, tiny, sizeof(tiny));
  CHECK(std::strlen(tiny) == sizeof(tiny) - 1);
}

void arguments() {
  using ldspath::arguments_ok;
  CHECK(arguments_ok(0, 1, 1, 1, -1, 0, 0, 0, false) && arguments_ok(4096, 64, 64, 64, 5, 3, 0, 16, true));
  CHECK(!arguments_ok(-1, 1, 1, 1, -1, 0, 0, 0, false) && !arguments_ok(4097, 1, 1, 1, -1, 0, 0, 0, false));
  CHECK(!arguments_ok(0, 0, 1, 1, -1, 0, 0, 0, false) && !arguments_ok(0, 1, 65, 1, -1, 0, 0, 0, false));
  CHECK(!arguments_ok(0, 1, 1, 0, -1, 0, 0, 0, false) && !arguments_ok(0, 1, 1, 1, 6, 0, 0, 0, false));
  CHECK(!arguments_ok(0, 1, 1, 1, 3, 1, ldspath::kAtomForms, 0, false) && !arguments_ok(0, 1, 1, 1, 4, 1, ldspath::kNumLaneOps, 0, false));
  CHECK(!arguments_ok(0, 1, 1, 1, -1, -1, 0, 0, false) && !arguments_ok(0, 1, 1, 1, -1, 0, 0, 4, false));
}

}  // namespace

int main() {
  lane_tables();
  transposed_read();
  atomics();
  reduction();
  arguments();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
