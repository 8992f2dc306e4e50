// Stand-alone self-test of the host-link check's host model (ops/hostlink/hostlink_host.h):
// no HIP, no Python.  tests/test_hostlink_model.py compiles it with
// g++ -fsanitize=address,undefined and runs it directly; it exits 0 and prints "ok", or
// prints what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostlink_host.h"

namespace {

using namespace hostlink;

int failures = 0;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

constexpr uint64_t kTile = 1024;  // a tile of the bulk kernels at UNROLL 4: 256 threads x 4 words

void fill_and_verify(uint64_t n) {
  std::vector<Word16> buf(n);
  fill(buf.data(), n, kSeedRead);
  long long first = 0;
  CHECK(verify(buf.data(), n, kSeedRead, &first) == 0 && first == -1);
  CHECK(verify(buf.data(), n, kSeedWrite, &first) > 0 && first == 0);  // another seed: the first word differs
  // one bit in the first word, one in the last, two 32-bit words of one 16-B word
  buf[0].c[0] ^= 1u;
  CHECK(verify(buf.data(), n, kSeedRead, &first) == 1 && first == 0);
  buf[0].c[0] ^= 1u;
  buf[n - 1].c[3] ^= 0x80000000u;
  CHECK(verify(buf.data(), n, kSeedRead, &first) == 1 && first == static_cast<long long>((n - 1) * 16 + 12));
  buf[n - 1].c[1] ^= 4u;
  uint64_t calls = 0, seen_bad = 0;
  CHECK(verify_each(buf.data(), n, kSeedRead, 0, &first, [&](uint64_t i, uint32_t bad) {
          ++calls;
          seen_bad += bad;
          CHECK(i == n - 1);
        }) == 2);
  CHECK(calls == 1 && seen_bad == 2 && first == static_cast<long long>((n - 1) * 16 + 4));
}

void injected_words(uint64_t n, uint64_t count) {
  std::vector<Word16> buf(n);
  fill(buf.data(), n, kSeedH2D);
  uint64_t last = 0;
  for (uint64_t f = 0; f < count; ++f) {
    const uint64_t w = inject_word(n, count, f);
    CHECK(w < n && (f == 0 || w > last));
    last = w;
    buf[w].c[kInjectComp] ^= 1u << kInjectBit;
  }
  long long first = -1;
  CHECK(verify(buf.data(), n, kSeedH2D, &first) == count);
  CHECK(first == static_cast<long long>(inject_word(n, count, 0) * 16 + 4 * kInjectComp));
}

void pattern_is_unique_across_2_32() {
  // indices that differ only above bit 32 differ through the high half
  const uint64_t base = (1ull << 32) - 2;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) CHECK(pattern(base + i, 7).c[0] != pattern(base + j, 7).c[0]);
  CHECK(pattern(5, 7).c[0] != pattern(5 + (1ull << 32), 7).c[0]);
  const Word16 w = pattern(12345, 99);
  CHECK(w.c[1] == (w.c[0] ^ 0xA5A5A5A5u) && w.c[2] == ~w.c[0] && w.c[3] == w.c[0] * 3u + 0x6A09E667u);
}

void atomic_tables(int blocks, int host_adds) {
  const uint32_t waves = static_cast<uint32_t>(blocks) * kThreads / kLanes;
  for (int op = 0; op < kLinkOps; ++op) {
    std::vector<unsigned char> t(table_bytes(op)), init(table_bytes(op));
    atomic_expected(op, blocks, host_adds, t.data());
    int first = 0;
    CHECK(atomic_compare(op, blocks, host_adds, t.data(), &first) == 0 && first == -1);
    atomic_initial(op, init.data());
    CHECK(atomic_compare(op, blocks, host_adds, init.data(), &first) > 0 && first >= 0);  // nothing ran
    t[0] ^= 1;  // element 0 of every table is in use
    CHECK(atomic_compare(op, blocks, host_adds, t.data(), &first) >= 1 && first >= 0);
  }
  // totals: every thread adds once, every wave takes one ticket and increments one CAS word
  std::vector<unsigned char> t(table_bytes(kU64Add));
  atomic_expected(kU64Add, blocks, host_adds, t.data());
  uint64_t sum = 0, want = 0;
  for (int e = 0; e < kAddElems; ++e) sum += reinterpret_cast<uint64_t*>(t.data())[e] - atomic_init(kU64Add, e);
  for (uint32_t g = 0; g < waves * kLanes; ++g) want += atomic_operand(kU64Add, g, 0, false);
  for (int i = 0; i < host_adds; ++i) want += host_add_operand(i);
  CHECK(sum == want);
  t.assign(table_bytes(kTicket), 0);
  atomic_expected(kTicket, blocks, host_adds, t.data());
  CHECK(reinterpret_cast<uint32_t*>(t.data())[0] == waves);
  // swap in reverse wave order is accepted too, a duplicated token is not
  t.assign(table_bytes(kSwap), 0);
  atomic_initial(kSwap, t.data());
  uint64_t* s = reinterpret_cast<uint64_t*>(t.data());
  for (uint32_t w = waves; w-- > 0;) {
    uint64_t& slot = s[atomic_row_hash(kSwap, w, 0) & (kSwapSlots - 1)];
    s[kSwapSlots + w] = slot;
    slot = atomic_operand(kSwap, w * kLanes, 0, false);
  }
  int first = 0;
  CHECK(atomic_compare(kSwap, blocks, host_adds, t.data(), &first) == 0);
  const uint64_t kept = s[kSwapSlots];
  s[kSwapSlots] = atomic_operand(kSwap, 0, 0, false);  // wave 0 got its own token back: whatever it held is lost
  CHECK(atomic_compare(kSwap, blocks, host_adds, t.data(), &first) == 1);
  s[kSwapSlots] = kept;
  if (waves < static_cast<uint32_t>(kMaxWaves)) {
    s[kSwapSlots + waves] = 1;  // an entry no wave owns
    CHECK(atomic_compare(kSwap, blocks, host_adds, t.data(), &first) == 1 && first == static_cast<int>(waves));
  }
}

}  // namespace

int main() {
  for (uint64_t n : {uint64_t{1}, kTile / 2, kTile / 2 + 1, kTile, kTile + 1}) fill_and_verify(n);
  injected_words(1, 1);
  injected_words(kTile + 1, 3);
  injected_words(65536, 3);
  pattern_is_unique_across_2_32();
  for (int blocks : {1, 13, 64})
    for (int host_adds : {0, 1024}) atomic_tables(blocks, host_adds);
  static_assert(table_offset(kLinkOps) == kTablesBytes && kTablesBytes % 256 == 0, "table layout");
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
