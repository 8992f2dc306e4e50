// The host-link check's model, shared by the kernels (hostlink.hip), the host code that
// drives them, and tests/native/hostlink_selftest.cpp: the 16-byte pattern, the host-side
// fill and verifier, and the (operation, thread, step) -> (element, operand) map of the
// system-scope atomics with the tables a healthy run leaves behind.  No HIP dependency beyond
// the __host__ __device__ qualifiers, so a plain C++17 compiler compiles it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../mfma_forms.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HOSTLINK_HD __host__ __device__
#else
#define HOSTLINK_HD
#endif

namespace hostlink {

// One unit of data: four 32-bit words.
struct alignas(16) Word16 {
  uint32_t c[4];
};

// The HBM sweep's pattern (ops/hbm.hip): lo * odd constant is a bijection mod 2^32, so no two
// 16-B words within any 2^32 consecutive indices share a pattern, and every bit of every
// word takes both values across a buffer.
HOSTLINK_HD inline Word16 pattern(uint64_t idx, uint32_t seed) {
  const uint32_t lo = static_cast<uint32_t>(idx), hi = static_cast<uint32_t>(idx >> 32);
  const uint32_t b = lo * 0x9E3779B1u ^ (hi + seed) * 0x85EBCA77u;
  return Word16{{b, b ^ 0xA5A5A5A5u, ~b, b * 3u + 0x6A09E667u}};
}

// The seeds of the four bulk stages (repetition r adds r).
constexpr uint32_t kSeedRead = 0x48520000u, kSeedWrite = 0x48570000u, kSeedH2D = 0x48320000u, kSeedD2H = 0x44320000u;

// The injected flip: bit 9 of 32-bit word 1 of a 16-B word (byte offset 16 * word + 4).
constexpr int kInjectComp = 1, kInjectBit = 9;

// Word f of the `count` spread-out words the host corrupts in a buffer of n (count <= n):
// distinct and ascending, so the first wrong offset is that of f = 0.
HOSTLINK_HD inline uint64_t inject_word(uint64_t n, uint64_t count, uint64_t f) {
  const uint64_t stride = n / count;
  return f * stride + stride / 2;
}

inline void fill(Word16* buf, uint64_t n, uint32_t seed, uint64_t idx0 = 0) {
  for (uint64_t i = 0; i < n; ++i) buf[i] = pattern(idx0 + i, seed);
}

// Compares buf[0..n) with pattern(idx0 + i, seed); on_bad(i, wrong 32-bit words of word i)
// for every 16-B word that differs, in ascending order.  Returns the wrong 32-bit words and
// sets *first_offset to the byte offset of the first of them (-1: none).
template <typename OnBad>
inline uint64_t verify_each(const Word16* buf, uint64_t n, uint32_t seed, uint64_t idx0, long long* first_offset,
                            OnBad&& on_bad) {
  uint64_t wrong = 0;
  *first_offset = -1;
  for (uint64_t i = 0; i < n; ++i) {
    const Word16 want = pattern(idx0 + i, seed);
    const Word16 got = buf[i];
    if (((got.c[0] ^ want.c[0]) | (got.c[1] ^ want.c[1]) | (got.c[2] ^ want.c[2]) | (got.c[3] ^ want.c[3])) == 0) continue;
    uint32_t bad = 0;
    for (int c = 0; c < 4; ++c) {
      if (buf[i].c[c] == want.c[c]) continue;
      if (*first_offset < 0) *first_offset = static_cast<long long>(i * 16 + 4 * c);
      ++bad;
    }
    wrong += bad;
    on_bad(i, bad);
  }
  return wrong;
}

inline uint64_t verify(const Word16* buf, uint64_t n, uint32_t seed, long long* first_offset) {
  return verify_each(buf, n, seed, 0, first_offset, [](uint64_t, uint32_t) {});
}

// ---- system-scope atomics: FetchAdd, Swap and CAS, the three AtomicOps PCIe defines ------
enum { kU32Add, kU64Add, kTicket, kCasInc, kSwap, kLinkOps };

constexpr int kThreads = 256, kLanes = 64;
constexpr int kAtomicMaxBlocks = 64;  // the grid the check starts with
constexpr int kMaxWaves = kAtomicMaxBlocks * kThreads / kLanes;
constexpr int kAddElems = 1024;       // elements of either add table: 16 rows of 64
constexpr int kCasWords = 64;
constexpr int kSwapSlots = 64;
constexpr int kCasRetries = 1 << 12;  // a word takes at most kMaxWaves increments in all
constexpr int kMaxHostAdds = 1 << 20;

HOSTLINK_HD constexpr int table_bytes(int op) {
  return op == kU32Add ? kAddElems * 4
         : op == kU64Add ? kAddElems * 8
         : op == kTicket ? (1 + kMaxWaves) * 4        // the ticket word, then seen[]
         : op == kCasInc ? kCasWords * 8
                         : (kSwapSlots + kMaxWaves) * 8;  // the slots, then what each wave got back
}
HOSTLINK_HD constexpr int table_offset(int op) {  // tables back to back, each a multiple of 256 B
  int off = 0;
  for (int o = 0; o < op; ++o) off += (table_bytes(o) + 255) & ~255;
  return off;
}
constexpr int kTablesBytes = table_offset(kLinkOps);
constexpr int kCappedOffset = kTablesBytes;  // one more u32: CAS loops that ran out of retries
constexpr int kTablesAlloc = kTablesBytes + 256;

using canary::fmix64;  // ../mfma_forms.h

// As in ops/fabric.hip: wave `wave` (global index) hits one row of 64 consecutive elements,
// lane l taking element 64 * row + l.  The CAS loop and the swap take word hash & 63.
HOSTLINK_HD inline uint32_t atomic_row_hash(int op, uint32_t wave, int step) {
  return static_cast<uint32_t>(fmix64((static_cast<uint64_t>(op + 1) << 56) ^ (1ull << 55) ^
                                      (static_cast<uint64_t>(wave) << 8) ^ static_cast<uint64_t>(step)));
}
HOSTLINK_HD inline uint32_t atomic_elem(int op, uint32_t gid, int step) {
  return (atomic_row_hash(op, gid >> 6, step) & (kAddElems / 64 - 1)) * 64u + (gid & 63u);
}

// The operand of thread `gid` at `step`; `inject` perturbs it so the result must change.
// swap: the wave's token, non-zero and different from every slot's initial value.
HOSTLINK_HD inline uint64_t atomic_operand(int op, uint32_t gid, int step, bool inject) {
  const uint64_t h =
      fmix64((static_cast<uint64_t>(op + 1) << 56) ^ (static_cast<uint64_t>(gid) << 8) ^ static_cast<uint64_t>(step));
  const uint64_t inj = inject ? 1u : 0u;
  switch (op) {
    case kU32Add: return static_cast<uint32_t>(h) + inj;
    case kU64Add: return h + inj;
    case kCasInc: return 1u + (h & 7u) + inj;
    case kSwap: return (0x70C5ull << 48) | (inj << 40) | ((gid >> 6) + 1u);
    default: return 1u + inj;  // kTicket: what the wave adds to seen[its ticket]
  }
}
HOSTLINK_HD inline uint64_t atomic_init(int op, uint32_t elem) {
  switch (op) {
    case kU32Add: case kU64Add: return elem;
    case kSwap: return elem < static_cast<uint32_t>(kSwapSlots) ? (0x1717ull << 48) | elem : 0;
    default: return 0;
  }
}

// The calling host thread's own adds to the u64 add table while the kernel runs.
inline uint32_t host_add_elem(int i) {
  return static_cast<uint32_t>(fmix64((0xC0ull << 56) ^ static_cast<uint64_t>(i))) & (kAddElems - 1);
}
inline uint64_t host_add_operand(int i) { return fmix64((0xC1ull << 56) ^ static_cast<uint64_t>(i)); }

inline void atomic_initial(int op, unsigned char* t) {
  std::memset(t, 0, table_bytes(op));
  if (op == kU32Add)
    for (uint32_t e = 0; e < static_cast<uint32_t>(kAddElems); ++e)
      reinterpret_cast<uint32_t*>(t)[e] = static_cast<uint32_t>(atomic_init(op, e));
  if (op == kU64Add)
    for (uint32_t e = 0; e < static_cast<uint32_t>(kAddElems); ++e) reinterpret_cast<uint64_t*>(t)[e] = atomic_init(op, e);
  if (op == kSwap)
    for (uint32_t e = 0; e < static_cast<uint32_t>(kSwapSlots); ++e) reinterpret_cast<uint64_t*>(t)[e] = atomic_init(op, e);
}

// The table of `op` after a healthy grid of `blocks` workgroups and `host_adds` host adds.
// swap depends on the order: this is the table the waves leave when they run in index
// order, one of the outcomes atomic_compare accepts.
inline void atomic_expected(int op, int blocks, int host_adds, unsigned char* t) {
  atomic_initial(op, t);
  const uint32_t threads = static_cast<uint32_t>(blocks) * kThreads, waves = threads / kLanes;
  uint32_t* t32 = reinterpret_cast<uint32_t*>(t);
  uint64_t* t64 = reinterpret_cast<uint64_t*>(t);
  switch (op) {
    case kU32Add:
      for (uint32_t g = 0; g < threads; ++g) t32[atomic_elem(op, g, 0)] += static_cast<uint32_t>(atomic_operand(op, g, 0, false));
      break;
    case kU64Add:
      for (uint32_t g = 0; g < threads; ++g) t64[atomic_elem(op, g, 0)] += atomic_operand(op, g, 0, false);
      for (int i = 0; i < host_adds; ++i) t64[host_add_elem(i)] += host_add_operand(i);
      break;
    case kTicket:
      t32[0] = waves;
      for (uint32_t w = 0; w < waves; ++w) t32[1 + w] = 1;
      break;
    case kCasInc:
      for (uint32_t w = 0; w < waves; ++w)
        t64[atomic_row_hash(op, w, 0) & (kCasWords - 1)] += atomic_operand(op, w * kLanes, 0, false);
      break;
    default:
      for (uint32_t w = 0; w < waves; ++w) {
        uint64_t& slot = t64[atomic_row_hash(op, w, 0) & (kSwapSlots - 1)];
        t64[kSwapSlots + w] = slot;
        slot = atomic_operand(op, w * kLanes, 0, false);
      }
  }
}

// Wrong elements of `got` for operation `op`; *first = the lowest of them (-1: none).
// Every form but swap is compared element by element with atomic_expected.  swap: what the
// waves got back together with what the slots hold at the end must be the tokens and the
// slots' initial values, each exactly once, in any order; every expected value that is
// missing counts (*first: its wave, or kMaxWaves + slot for an initial value), and so does
// every entry past the last wave that is not 0.
inline uint64_t atomic_compare(int op, int blocks, int host_adds, const unsigned char* got, int* first) {
  uint64_t bad = 0;
  *first = -1;
  std::vector<unsigned char> want(table_bytes(op));
  atomic_expected(op, blocks, host_adds, want.data());
  if (op != kSwap) {
    const int width = (op == kU64Add || op == kCasInc) ? 8 : 4, n = table_bytes(op) / width;
    for (int e = 0; e < n; ++e) {
      if (std::memcmp(got + e * width, want.data() + e * width, width) == 0) continue;
      if (bad == 0) *first = e;
      ++bad;
    }
    return bad;
  }
  const uint32_t waves = static_cast<uint32_t>(blocks) * kThreads / kLanes;
  std::vector<uint64_t> g(kSwapSlots + waves);
  std::memcpy(g.data(), got, g.size() * 8);
  std::sort(g.begin(), g.end());
  for (uint32_t k = 0; k < kSwapSlots + waves; ++k) {  // tokens first, then the initial values
    const uint64_t v = k < waves ? atomic_operand(op, k * kLanes, 0, false) : atomic_init(op, k - waves);
    const auto range = std::equal_range(g.begin(), g.end(), v);
    if (range.second - range.first == 1) continue;  // absent, or held twice: then another is absent too
    if (range.first == range.second) {
      if (bad == 0) *first = k < waves ? static_cast<int>(k) : kMaxWaves + static_cast<int>(k - waves);
      ++bad;
    }
  }
  for (uint32_t w = waves; w < static_cast<uint32_t>(kMaxWaves); ++w) {
    uint64_t v;
    std::memcpy(&v, got + (kSwapSlots + w) * 8, 8);
    if (v == 0) continue;
    if (bad == 0) *first = static_cast<int>(w);
    ++bad;
  }
  return bad;
}

}  // namespace hostlink
