// MI355X (gfx950 / CDNA4) health canary, part 4: what lies between a CU and HBM.
//
// The HBM sweep streams hundreds of MiB through the per-XCD L2s, so no line is read back
// while it is L2-resident, data that one XCD wrote and another read is never attributed,
// and no other check issues a global atomic.  Three launches of 256-thread workgroups:
//
//   * l2_march: workgroup b owns slice b (slice_kb KiB) of one buffer.  It writes an
//     address-derived pattern with plain stores (they keep the line in the XCD's L2), waits
//     (s_waitcnt vmcnt(0), barrier), reads the slice `reps` times in reverse order with 16-B
//     non-temporal loads (they bypass L1 and are served by L2; reversed, so a wave reads
//     words other waves wrote), writes the complement and reads it forward.  The slice is
//     left holding the complement.  Lane 0 reads HW_REG_XCC_ID first and last and adds
//     {blocks, bytes, bad words} to table[xcc]; a workgroup whose xcc changed is counted as
//     moved and its errors as unlocated.
//   * xcd_exchange: a second launch, so the hand-off is a kernel boundary.  The host groups
//     the slices by the xcc that wrote them; reader workgroup r checks, for every writer
//     xcc w, slice list_w[r % len(list_w)] against the complement and adds {reads, bad
//     words} to matrix[w][its xcc].  The grid is at least as long as every list, so every
//     slice is read.
//   * atomic_exact: every global atomic form on operands that make the result independent
//     of order, into tables the HOST predicts with the same operand functions
//     (atomic_elem / atomic_operand below).
//
// No workgroup waits for another, every loop is bounded by an argument or a constant.
// Errors are counted in 32-bit words (march, exchange) and table elements (atomics).
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "canary_host.h"

namespace {

using namespace canary;

constexpr int kThreads = 256;
constexpr int kInjectKinds = 3;  // 0 l2, 1 xcd, 2 atomic
// the injected flip: bit 9 of 32-bit word 1 of 16-B word 37 (byte offset 0x254) of a slice
constexpr int kInjectWord = 37, kInjectBit = 9;

// The 16-B pattern of canary.hip's HBM test under a seed of its own: lo * odd constant is a
// bijection mod 2^32, so no two 16-B words of the buffer (<= 4 GiB) share a pattern; with
// the complement pass every bit of every word takes both values.
__device__ __forceinline__ u32x4 fabric_pattern(uint64_t idx) {
  const uint32_t lo = static_cast<uint32_t>(idx), hi = static_cast<uint32_t>(idx >> 32);
  const uint32_t b = lo * 0x9E3779B1u ^ (hi + 0x5EEDu) * 0x85EBCA77u;
  u32x4 v = {b, b ^ 0xA5A5A5A5u, ~b, b * 3u + 0x6A09E667u};
  return v;
}

__device__ __forceinline__ uint32_t xcc_id() { return __builtin_amdgcn_s_getreg(getreg_imm(kHwRegXccId, 0, 4)) & 0xFu; }

// Compares one loaded 16-B word; keeps the lowest byte offset of a wrong 32-bit word.
__device__ __forceinline__ void check16(const u32x4& v, const u32x4& want, uint32_t word, uint32_t& bad, uint32_t& first) {
  for (int c = 0; c < 4; ++c) {
    if (v[c] != want[c]) {
      ++bad;
      const uint32_t off = word * 16u + 4u * c;
      first = off < first ? off : first;
    }
  }
}

// counters: [0] moved march workgroups, [1] their wrong words, [2] moved exchange
// workgroups, [3] their wrong words.  first_bad: min over (slice << 32 | byte offset).
__global__ void __launch_bounds__(kThreads) l2_march(u32x4* __restrict__ buf, int slice_words, int reps, int inject_kind,
                                                    int inject_blocks, amdgpu_canary_xcc_slot* __restrict__ table,
                                                    unsigned int* __restrict__ slice_xcc,
                                                    unsigned long long* __restrict__ first_bad,
                                                    unsigned long long* __restrict__ counters) {
  __shared__ unsigned int s_bad, s_first;
  const uint32_t xcc = xcc_id();
  const int tid = threadIdx.x;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * slice_words;
  u32x4* s = buf + base;
  const bool inject = static_cast<int>(blockIdx.x) < inject_blocks;  // uniform over the workgroup
  if (tid == 0) {
    s_bad = 0;
    s_first = 0xFFFFFFFFu;
  }
  for (int i = tid; i < slice_words; i += kThreads) s[i] = fabric_pattern(base + i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (inject && inject_kind == 0) {  // a thread of the last wave flips a bit the first wave stored
    if (tid == kThreads - 1)
      reinterpret_cast<uint32_t*>(s + kInjectWord)[1] = fabric_pattern(base + kInjectWord)[1] ^ (1u << kInjectBit);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  uint32_t bad = 0, first = 0xFFFFFFFFu;
  for (int r = 0; r < reps; ++r) {
#pragma unroll 4
    for (int i = tid; i < slice_words; i += kThreads) {
      const int j = slice_words - 1 - i;
      check16(__builtin_nontemporal_load(s + j), fabric_pattern(base + j), j, bad, first);
    }
    __syncthreads();  // every read of this pass is done before the next pass or the next write
  }
  for (int i = tid; i < slice_words; i += kThreads) s[i] = ~fabric_pattern(base + i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll 4
  for (int i = tid; i < slice_words; i += kThreads)
    check16(__builtin_nontemporal_load(s + i), ~fabric_pattern(base + i), i, bad, first);
  if (inject && inject_kind == 1) {  // after the last compare: only the exchange sees it
    __syncthreads();
    if (tid == kThreads - 1)
      reinterpret_cast<uint32_t*>(s + kInjectWord)[1] = ~fabric_pattern(base + kInjectWord)[1] ^ (1u << kInjectBit);
  }
  if (bad) {
    atomicAdd(&s_bad, bad);
    atomicMin(&s_first, first);
  }
  __syncthreads();
  if (tid != 0) return;
  const uint32_t xcc_after = xcc_id();
  slice_xcc[blockIdx.x] = xcc;
  if (xcc_after == xcc) {
    amdgpu_canary_xcc_slot* slot = table + xcc;  // xcc < kFabricXccs by the mask in xcc_id()
    atomicAdd(&slot->blocks, 1ull);
    atomicAdd(&slot->bytes, static_cast<unsigned long long>(slice_words) * 16ull);
    if (s_bad) atomicAdd(&slot->bad, static_cast<unsigned long long>(s_bad));
  } else {
    atomicAdd(&counters[0], 1ull);
    if (s_bad) atomicAdd(&counters[1], static_cast<unsigned long long>(s_bad));
  }
  if (s_bad) atomicMin(first_bad, (static_cast<unsigned long long>(blockIdx.x) << 32) | s_first);
}

// lists: the slices grouped by writer xcc, list w at lists[list_off[w] .. list_off[w + 1]).
__global__ void __launch_bounds__(kThreads) xcd_exchange(const u32x4* __restrict__ buf, int slice_words, int slices,
                                                        const int* __restrict__ lists, const int* __restrict__ list_off,
                                                        amdgpu_canary_pair_slot* __restrict__ matrix,
                                                        unsigned long long* __restrict__ counters) {
  __shared__ unsigned int s_bad[kFabricXccs];
  const uint32_t xcc = xcc_id();
  const int tid = threadIdx.x;
  if (tid < kFabricXccs) s_bad[tid] = 0;
  __syncthreads();
  for (int w = 0; w < kFabricXccs; ++w) {
    const int len = list_off[w + 1] - list_off[w];
    if (len <= 0) continue;
    const int slice = lists[list_off[w] + static_cast<int>(blockIdx.x % static_cast<unsigned int>(len))];
    if (slice < 0 || slice >= slices) continue;  // host-built; never read outside the buffer
    const uint64_t base = static_cast<uint64_t>(slice) * slice_words;
    uint32_t bad = 0, first = 0;
#pragma unroll 4
    for (int i = tid; i < slice_words; i += kThreads)
      check16(__builtin_nontemporal_load(buf + base + i), ~fabric_pattern(base + i), i, bad, first);
    if (bad) atomicAdd(&s_bad[w], bad);
  }
  __syncthreads();
  if (tid != 0) return;
  const uint32_t xcc_after = xcc_id();
  unsigned long long moved_bad = 0;
  for (int w = 0; w < kFabricXccs; ++w) {
    if (list_off[w + 1] - list_off[w] <= 0) continue;
    if (xcc_after == xcc) {
      amdgpu_canary_pair_slot* cell = matrix + w * kFabricXccs + xcc;
      atomicAdd(&cell->reads, 1ull);
      if (s_bad[w]) atomicAdd(&cell->bad, static_cast<unsigned long long>(s_bad[w]));
    } else {
      moved_bad += s_bad[w];
    }
  }
  if (xcc_after != xcc) {
    atomicAdd(&counters[2], 1ull);
    if (moved_bad) atomicAdd(&counters[3], moved_bad);
  }
}

// ---- atomics: the (operation, thread, step) -> (element, operand) map, host and device ----
enum {
  kU32Add, kU64Add, kI32Min, kU32Max, kU64Max, kAnd, kOr, kXor, kF32Add, kF64Add, kPkBf16, kPkF16, kCasInc, kTicket
};
static_assert(kTicket + 1 == kAtomicOps, "operation list and kAtomicOps disagree");
const char* const kOpNames[kAtomicOps] = {"u32 add", "u64 add", "i32 min", "u32 max", "u64 max", "and", "or", "xor",
                                          "f32 add", "f64 add", "pk_add_bf16", "pk_add_f16", "cas inc", "ticket"};

constexpr int kSteps = 8;            // J: operations per thread and form
constexpr int kCasWords = 64;
constexpr int kCasRetries = 1 << 14;  // a word takes at most 4096 * 4 * kSteps increments in all
constexpr int kMaxWaves = kMaxBlocks * kThreads / kWave;
constexpr uint32_t kDenseWaves = 512;  // waves that add to the packed forms at every step

__host__ __device__ constexpr int table_bytes(int op) {
  return op == kCasInc ? kCasWords * 4
         : op == kTicket ? (1 + kMaxWaves) * 4  // the ticket word, then seen[]
         : (op == kU64Add || op == kU64Max || op == kF64Add) ? kAtomicElems * 8
                                                           : kAtomicElems * 4;
}
__host__ __device__ constexpr int table_offset(int op) {  // tables back to back, each a multiple of 256 B
  int off = 0;
  for (int o = 0; o < op; ++o) off += (table_bytes(o) + 255) & ~255;
  return off;
}
constexpr int kTablesBytes = table_offset(kAtomicOps);
constexpr int kCappedOffset = kTablesBytes;  // one more word: CAS loops that ran out of retries

// The row of 64 consecutive elements that wave `wave` (global index) hits at `step`, lane l
// taking element 64 * row + l: one wave-instruction covers 256 (or 512) contiguous bytes.
// The CAS loop takes word hash & 63 of the same hash.
__host__ __device__ inline uint32_t atomic_row_hash(int op, uint32_t wave, int step) {
  return static_cast<uint32_t>(fmix64((static_cast<uint64_t>(op + 1) << 56) ^ (1ull << 55) ^
                                      (static_cast<uint64_t>(wave) << 8) ^ static_cast<uint64_t>(step)));
}
__host__ __device__ inline uint32_t atomic_elem(int op, uint32_t gid, int step) {
  return (atomic_row_hash(op, gid >> 6, step) & 31u) * 64u + (gid & 63u);
}

// bits of `elem` that the and / or operands may touch: never bit (elem & 31), which only an
// injected operand clears / sets
__host__ __device__ inline uint32_t bit_sel(uint32_t elem) {
  return static_cast<uint32_t>(fmix64(0xB175ull << 40 ^ elem)) & ~(1u << (elem & 31u));
}

__host__ __device__ inline uint32_t bf16_bits(int v) {  // exact for |v| <= 256
  const float f = static_cast<float>(v);
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u >> 16;
}
__host__ __device__ inline uint32_t f16_bits(int v) {  // exact for 0 <= v <= 2048
  if (v <= 0) return 0;
  int e = 0;
  while ((v >> (e + 1)) != 0) ++e;
  const uint32_t mant = e <= 10 ? static_cast<uint32_t>(v) << (10 - e) : static_cast<uint32_t>(v) >> (e - 10);
  return (static_cast<uint32_t>(e + 15) << 10) | (mant & 0x3FFu);
}

// The operand of thread `gid` (global index) at `step`, to element `elem`; `inject` perturbs
// it so that the element's result must change.  Integer forms: raw bits.  f32 / f64 add: a
// small signed integer (two's complement), sums stay far below 2^24 / 2^53.  Packed forms:
// two non-negative integers (low | high << 16); waves below kDenseWaves add at every step,
// the others rarely, so an element's total stays <= 256 (bf16) and <= 2048 (f16) for every
// grid up to kMaxBlocks and every partial sum in any order is representable.
__host__ __device__ inline uint64_t atomic_operand(int op, uint32_t gid, int step, uint32_t elem, bool inject) {
  const uint64_t h =
      fmix64((static_cast<uint64_t>(op + 1) << 56) ^ (static_cast<uint64_t>(gid) << 8) ^ static_cast<uint64_t>(step));
  const uint32_t h32 = static_cast<uint32_t>(h);
  const bool dense = (gid >> 6) < kDenseWaves;
  const uint32_t inj = inject ? 1u : 0u;
  switch (op) {
    case kU32Add: return h32 + inj;
    case kU64Add: return h + inj;
    case kI32Min: return inject ? 0x80000000u : h32;
    case kU32Max: return inject ? 0xFFFFFFFFu : h32;
    case kU64Max: return inject ? ~0ull : h;
    case kAnd: return inject ? ~(1u << (elem & 31u)) : ~((1u << (h32 & 31u)) & bit_sel(elem));
    case kOr: return inject ? (1u << (elem & 31u)) : ((1u << (h32 & 31u)) & bit_sel(elem));
    case kXor: return h32 ^ inj;
    case kF32Add: return static_cast<uint64_t>(static_cast<int64_t>(h32 & 15u) - 8 + inj);
    case kF64Add: return static_cast<uint64_t>(static_cast<int64_t>(h32 & 0xFFFFFu) - (1 << 19) + inj);
    case kPkBf16: {
      const uint32_t lo = dense ? (h32 & 1u) : ((h32 & 63u) == 0u), hi = dense ? ((h32 >> 8) & 1u) : (((h32 >> 8) & 63u) == 0u);
      return (lo + inj) | (hi << 16);
    }
    case kPkF16: {
      const uint32_t a = h32, b = h32 >> 8;
      const uint32_t lo = dense ? (a & 7u) : ((a & 15u) == 0u ? ((a >> 4) & 7u) : 0u);
      const uint32_t hi = dense ? (b & 7u) : ((b & 15u) == 0u ? ((b >> 4) & 7u) : 0u);
      return (lo + inj) | (hi << 16);
    }
    case kCasInc: return 1u + (h32 & 7u) + inj;
    default: return 1u + inj;  // kTicket: what the wave adds to seen[its ticket]
  }
}

// initial value of element `elem`: untouched elements must still hold it afterwards
__host__ __device__ inline uint64_t atomic_init(int op, uint32_t elem) {
  switch (op) {
    case kU32Add: case kU64Add: case kU32Max: case kU64Max: return elem;
    case kI32Min: return 0x7FFFFFFFu - elem;
    case kAnd: return 0xFFFFFFFFu;
    case kXor: return elem * 0x9E3779B1u;
    case kPkBf16: return bf16_bits(1) | (bf16_bits(2) << 16);
    case kPkF16: return f16_bits(1) | (f16_bits(2) << 16);
    default: return 0;  // or, f32 add, f64 add (+0.0), cas inc, ticket
  }
}

template <int OP>
__device__ __forceinline__ void atomic_form(unsigned char* __restrict__ tables, uint32_t gid, bool inject) {
  unsigned char* t = tables + table_offset(OP);
  for (int step = 0; step < kSteps; ++step) {
    const uint32_t e = atomic_elem(OP, gid, step);  // < kAtomicElems
    const uint64_t v = atomic_operand(OP, gid, step, e, inject && step == 0);
    if (OP == kU32Add) atomicAdd(reinterpret_cast<unsigned int*>(t) + e, static_cast<unsigned int>(v));
    if (OP == kU64Add) atomicAdd(reinterpret_cast<unsigned long long*>(t) + e, static_cast<unsigned long long>(v));
    if (OP == kI32Min) atomicMin(reinterpret_cast<int*>(t) + e, static_cast<int>(static_cast<uint32_t>(v)));
    if (OP == kU32Max) atomicMax(reinterpret_cast<unsigned int*>(t) + e, static_cast<unsigned int>(v));
    if (OP == kU64Max) atomicMax(reinterpret_cast<unsigned long long*>(t) + e, static_cast<unsigned long long>(v));
    if (OP == kAnd) atomicAnd(reinterpret_cast<unsigned int*>(t) + e, static_cast<unsigned int>(v));
    if (OP == kOr) atomicOr(reinterpret_cast<unsigned int*>(t) + e, static_cast<unsigned int>(v));
    if (OP == kXor) atomicXor(reinterpret_cast<unsigned int*>(t) + e, static_cast<unsigned int>(v));
    if (OP == kF32Add) unsafeAtomicAdd(reinterpret_cast<float*>(t) + e, static_cast<float>(static_cast<int64_t>(v)));
    if (OP == kF64Add) unsafeAtomicAdd(reinterpret_cast<double*>(t) + e, static_cast<double>(static_cast<int64_t>(v)));
    if (OP == kPkBf16) {
      const uint32_t bits = bf16_bits(static_cast<int>(v & 0xFFFFu)) | (bf16_bits(static_cast<int>(v >> 16)) << 16);
      __hip_bfloat162 x;
      __builtin_memcpy(static_cast<void*>(&x), &bits, 4);
      unsafeAtomicAdd(reinterpret_cast<__hip_bfloat162*>(t) + e, x);
    }
    if (OP == kPkF16) {
      const uint32_t bits = f16_bits(static_cast<int>(v & 0xFFFFu)) | (f16_bits(static_cast<int>(v >> 16)) << 16);
      __half2 x;
      __builtin_memcpy(static_cast<void*>(&x), &bits, 4);
      unsafeAtomicAdd(reinterpret_cast<__half2*>(t) + e, x);
    }
  }
}

// Workgroups below inject_blocks perturb, in thread 0 at step 0, the operand of inject_op.
__global__ void __launch_bounds__(kThreads) atomic_exact(unsigned char* __restrict__ tables, int inject_op,
                                                        int inject_blocks) {
  const uint32_t gid = blockIdx.x * kThreads + threadIdx.x;  // < 2^20 (host-checked grid)
  const bool inject = static_cast<int>(blockIdx.x) < inject_blocks && threadIdx.x == 0;
  atomic_form<kU32Add>(tables, gid, inject && inject_op == kU32Add);
  atomic_form<kU64Add>(tables, gid, inject && inject_op == kU64Add);
  atomic_form<kI32Min>(tables, gid, inject && inject_op == kI32Min);
  atomic_form<kU32Max>(tables, gid, inject && inject_op == kU32Max);
  atomic_form<kU64Max>(tables, gid, inject && inject_op == kU64Max);
  atomic_form<kAnd>(tables, gid, inject && inject_op == kAnd);
  atomic_form<kOr>(tables, gid, inject && inject_op == kOr);
  atomic_form<kXor>(tables, gid, inject && inject_op == kXor);
  atomic_form<kF32Add>(tables, gid, inject && inject_op == kF32Add);
  atomic_form<kF64Add>(tables, gid, inject && inject_op == kF64Add);
  atomic_form<kPkBf16>(tables, gid, inject && inject_op == kPkBf16);
  atomic_form<kPkF16>(tables, gid, inject && inject_op == kPkF16);
  if ((threadIdx.x & (kWave - 1)) != 0) return;
  // lane 0 of each wave: a CAS-increment loop with capped retries ...
  const uint32_t wave = gid >> 6, waves = gridDim.x * (kThreads / kWave);
  unsigned int* cas = reinterpret_cast<unsigned int*>(tables + table_offset(kCasInc));
  for (int step = 0; step < kSteps; ++step) {
    unsigned int* p = cas + (atomic_row_hash(kCasInc, wave, step) & (kCasWords - 1));
    const unsigned int amount = static_cast<unsigned int>(
        atomic_operand(kCasInc, gid, step, 0, inject && inject_op == kCasInc && step == 0));
    unsigned int old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool done = false;
    for (int tries = 0; tries < kCasRetries && !done; ++tries) {
      const unsigned int seen = atomicCAS(p, old, old + amount);
      done = seen == old;
      old = seen;
    }
    if (!done) atomicAdd(reinterpret_cast<unsigned int*>(tables + kCappedOffset), 1u);
  }
  // ... and one ticket, whose returned value picks the word it then marks
  unsigned int* ticket = reinterpret_cast<unsigned int*>(tables + table_offset(kTicket));
  const unsigned int mine = atomicAdd(ticket, 1u);
  if (mine < waves && mine < static_cast<unsigned int>(kMaxWaves))
    atomicAdd(ticket + 1 + mine,
              static_cast<unsigned int>(atomic_operand(kTicket, gid, 0, 0, inject && inject_op == kTicket)));
}

// ---- host model of the atomics ---------------------------------------------------------
void atomic_initial(int op, unsigned char* t) {
  if (op == kCasInc || op == kTicket) {
    std::memset(t, 0, table_bytes(op));
    return;
  }
  const bool wide = table_bytes(op) == kAtomicElems * 8;
  for (uint32_t e = 0; e < static_cast<uint32_t>(kAtomicElems); ++e) {
    const uint64_t v = atomic_init(op, e);
    if (wide) reinterpret_cast<uint64_t*>(t)[e] = v;
    else reinterpret_cast<uint32_t*>(t)[e] = static_cast<uint32_t>(v);
  }
}

// The table of `op` after a healthy grid of `blocks` workgroups: the device's loops, in
// thread order.  The packed forms are summed as integers and converted once.
void atomic_expected(int op, int blocks, unsigned char* t) {
  atomic_initial(op, t);
  const uint32_t threads = static_cast<uint32_t>(blocks) * kThreads, waves = threads / kWave;
  uint32_t* t32 = reinterpret_cast<uint32_t*>(t);
  uint64_t* t64 = reinterpret_cast<uint64_t*>(t);
  if (op == kTicket) {
    t32[0] = waves;
    for (uint32_t w = 0; w < waves; ++w) t32[1 + w] = 1;
    return;
  }
  if (op == kCasInc) {
    for (uint32_t w = 0; w < waves; ++w)
      for (int step = 0; step < kSteps; ++step)
        t32[atomic_row_hash(op, w, step) & (kCasWords - 1)] +=
            static_cast<uint32_t>(atomic_operand(op, w * kWave, step, 0, false));
    return;
  }
  std::vector<int64_t> sums;  // f32 / f64: the integer sum; packed: low and high totals
  if (op == kF32Add || op == kF64Add) sums.assign(kAtomicElems, 0);
  if (op == kPkBf16 || op == kPkF16) sums.assign(2 * kAtomicElems, 0);
  for (uint32_t w = 0; w < waves; ++w) {
    for (int step = 0; step < kSteps; ++step) {
      const uint32_t row = (atomic_row_hash(op, w, step) & 31u) * 64u;
      for (uint32_t lane = 0; lane < static_cast<uint32_t>(kWave); ++lane) {
        const uint32_t e = row + lane;
        const uint64_t v = atomic_operand(op, w * kWave + lane, step, e, false);
        const uint32_t v32 = static_cast<uint32_t>(v);
        switch (op) {
          case kU32Add: t32[e] += v32; break;
          case kU64Add: t64[e] += v; break;
          case kI32Min:
            if (static_cast<int32_t>(v32) < static_cast<int32_t>(t32[e])) t32[e] = v32;
            break;
          case kU32Max: t32[e] = v32 > t32[e] ? v32 : t32[e]; break;
          case kU64Max: t64[e] = v > t64[e] ? v : t64[e]; break;
          case kAnd: t32[e] &= v32; break;
          case kOr: t32[e] |= v32; break;
          case kXor: t32[e] ^= v32; break;
          case kF32Add: case kF64Add: sums[e] += static_cast<int64_t>(v); break;
          default:  // packed
            sums[2 * e] += v32 & 0xFFFFu;
            sums[2 * e + 1] += v32 >> 16;
        }
      }
    }
  }
  for (uint32_t e = 0; e < static_cast<uint32_t>(kAtomicElems); ++e) {
    if (op == kF32Add) reinterpret_cast<float*>(t)[e] = static_cast<float>(sums[e]);
    if (op == kF64Add) reinterpret_cast<double*>(t)[e] = static_cast<double>(sums[e]);
    if (op == kPkBf16)
      t32[e] = bf16_bits(static_cast<int>(sums[2 * e]) + 1) | (bf16_bits(static_cast<int>(sums[2 * e + 1]) + 2) << 16);
    if (op == kPkF16)
      t32[e] = f16_bits(static_cast<int>(sums[2 * e]) + 1) | (f16_bits(static_cast<int>(sums[2 * e + 1]) + 2) << 16);
  }
}

// wrong elements of `op` (raw bits compared); *first = the lowest wrong element
unsigned long long atomic_compare(int op, const unsigned char* got, const unsigned char* want, int* first) {
  const int width = table_bytes(op) == kAtomicElems * 8 ? 8 : 4, n = table_bytes(op) / width;
  unsigned long long bad = 0;
  for (int e = 0; e < n; ++e) {
    if (std::memcmp(got + e * width, want + e * width, width) != 0) {
      if (bad == 0) *first = e;
      ++bad;
    }
  }
  return bad;
}

}  // namespace

extern "C" {

const char* amdgpu_canary_atomic_op_name(int op) { return op >= 0 && op < kAtomicOps ? kOpNames[op] : "?"; }

// The place of the first failing check (l2, then xcd, then atomic) as the canary's error
// text; returns its length, 0 when every count is 0.
int amdgpu_canary_fabric_describe(const amdgpu_canary_fabric_result* r, const amdgpu_canary_xcc_slot* xcc_table,
                                  const amdgpu_canary_pair_slot* pair_matrix, char* buf, int len) {
  if (r->l2_errors > 0) {
    int bad_xccs = 0;
    for (int x = 0; x < kFabricXccs; ++x) bad_xccs += xcc_table[x].bad > 0;
    if (r->first_bad_xcc < 0)
      return std::snprintf(buf, len, "l2 check: %llu wrong words on an unknown xcc (slice %d, offset 0x%x)",
                           r->l2_errors, r->first_bad_slice, r->first_bad_offset);
    int n = std::snprintf(buf, len, "l2 check: %llu wrong words on xcc%d (slice %d, offset 0x%x)", r->l2_errors,
                          r->first_bad_xcc, r->first_bad_slice, r->first_bad_offset);
    if (bad_xccs > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more xcc%s)", bad_xccs - 1, bad_xccs > 2 ? "s" : "");
    return n;
  }
  if (r->xcd_errors > 0) {
    int bad_pairs = 0, first = -1;
    for (int c = 0; c < kFabricXccs * kFabricXccs; ++c) {
      if (pair_matrix[c].bad == 0) continue;
      if (first < 0) first = c;
      ++bad_pairs;
    }
    if (first < 0)  // every reader that saw one moved while it read
      return std::snprintf(buf, len, "xcd check: %llu wrong words read on an unknown xcc", r->xcd_errors);
    int n = std::snprintf(buf, len, "xcd check: %llu wrong words written on xcc%d, read on xcc%d", r->xcd_errors,
                          first / kFabricXccs, first % kFabricXccs);
    if (bad_pairs > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more pair%s)", bad_pairs - 1, bad_pairs > 2 ? "s" : "");
    return n;
  }
  if (r->atomic_errors > 0)
    return std::snprintf(buf, len, "atomic check: %llu wrong elements in %s (first at %d)", r->atomic_errors,
                         amdgpu_canary_atomic_op_name(r->first_bad_op), r->first_bad_elem);
  return 0;
}

// Host only: the expected table of operation `op` after a grid of `blocks` workgroups, as
// the device lays it out (cas inc: 64 words; ticket: the ticket word, then seen[16384]).
// Returns the bytes written, or -1 on a bad argument or a short buffer.
int amdgpu_canary_atomic_expected(int op, int blocks, void* out, int out_bytes) {
  if (op < 0 || op >= kAtomicOps || blocks < 1 || blocks > kMaxBlocks || out == nullptr || out_bytes < table_bytes(op))
    return -1;
  atomic_expected(op, blocks, static_cast<unsigned char*>(out));
  return table_bytes(op);
}

// Runs the three checks on `device` with a grid of `blocks` workgroups (0: one per CU).
// inject_kind -1 none, 0 l2, 1 xcd, 2 atomic (operation inject_op), in the first
// inject_blocks workgroups.  xcc_table_out (kFabricXccs slots), pair_matrix_out
// (kFabricXccs^2 cells, [writer][reader]) and slice_xcc_out (the xcc each of the first
// slice_xcc_len slices was written on) may be null.  0, or -1 with `err` set.
int amdgpu_canary_fabric(int device, int blocks, int slice_kb, int reps, int inject_kind, int inject_op,
                         int inject_blocks, amdgpu_canary_xcc_slot* xcc_table_out,
                         amdgpu_canary_pair_slot* pair_matrix_out, unsigned int* slice_xcc_out, int slice_xcc_len,
                         amdgpu_canary_fabric_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  out->first_bad_slice = out->first_bad_xcc = out->first_bad_op = out->first_bad_elem = -1;
  if (blocks < 0 || blocks > kMaxBlocks || slice_kb < 4 || slice_kb > 1024 || slice_kb % 4 != 0 || reps < 1 ||
      reps > 16 || inject_kind < -1 || inject_kind >= kInjectKinds || inject_op < 0 || inject_op >= kAtomicOps ||
      inject_blocks < 0 || slice_xcc_len < 0 || (slice_xcc_out == nullptr && slice_xcc_len != 0)) {
    std::snprintf(err, err_len,
                  "fabric check: bad arguments (blocks %d in 0..%d, slice_kb %d a multiple of 4 in 4..1024, reps %d in "
                  "1..16, inject %d/%d/%d)",
                  blocks, kMaxBlocks, slice_kb, reps, inject_kind, inject_op, inject_blocks);
    return -1;
  }
  Status st;
  hipDeviceProp_t prop;
  DeviceBuffer<u32x4> d_buf;
  DeviceBuffer<unsigned char> d_state, d_tables;
  DeviceBuffer<int> d_lists;
  Events<3> ev;
  // device state of the march and the exchange, one allocation
  constexpr size_t kTableOff = 0, kMatrixOff = kTableOff + sizeof(amdgpu_canary_xcc_slot) * kFabricXccs,
                   kCountersOff = kMatrixOff + sizeof(amdgpu_canary_pair_slot) * kFabricXccs * kFabricXccs,
                   kFirstOff = kCountersOff + 4 * sizeof(unsigned long long),
                   kSliceXccOff = kFirstOff + sizeof(unsigned long long);
  std::vector<unsigned char> h_state, h_tables(kTablesBytes + 256, 0), h_got, want;
  std::vector<int> h_lists;
  int grid = 0, slice_words = slice_kb * 64;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (st.ok()) {
    grid = launch_plan(blocks, prop.multiProcessorCount, 1).grid;
    out->blocks = grid;
    out->slice_kb = slice_kb;
    h_state.assign(kSliceXccOff + sizeof(unsigned int) * grid, 0);
    std::memset(h_state.data() + kFirstOff, 0xFF, sizeof(unsigned long long));  // no wrong word yet
    std::memset(h_state.data() + kSliceXccOff, 0xFF, sizeof(unsigned int) * grid);
    for (int op = 0; op < kAtomicOps; ++op) atomic_initial(op, h_tables.data() + table_offset(op));
  }
  CANARY_HIP(st, d_buf.alloc(static_cast<size_t>(grid) * slice_words * sizeof(u32x4)));
  CANARY_HIP(st, d_state.alloc(h_state.size()));
  CANARY_HIP(st, d_state.upload(h_state.data()));
  CANARY_HIP(st, d_tables.alloc(h_tables.size()));
  CANARY_HIP(st, d_tables.upload(h_tables.data()));
  CANARY_HIP(st, d_lists.alloc(sizeof(int) * (grid + kFabricXccs + 1)));
  CANARY_HIP(st, ev.create());
  if (st.ok()) {
    auto* d_table = reinterpret_cast<amdgpu_canary_xcc_slot*>(d_state.get() + kTableOff);
    auto* d_matrix = reinterpret_cast<amdgpu_canary_pair_slot*>(d_state.get() + kMatrixOff);
    auto* d_counters = reinterpret_cast<unsigned long long*>(d_state.get() + kCountersOff);
    auto* d_first = reinterpret_cast<unsigned long long*>(d_state.get() + kFirstOff);
    auto* d_slice_xcc = reinterpret_cast<unsigned int*>(d_state.get() + kSliceXccOff);
    // the atomics and the march, back to back
    float ms[2] = {0, 0};
    time_stages(st, ev, ms, [&](int k) {
      if (k == 0) {
        st.stage("atomic_exact: ");
        hipLaunchKernelGGL(atomic_exact, dim3(grid), dim3(kThreads), 0, 0, d_tables.get(), inject_op,
                           inject_kind == 2 ? inject_blocks : 0);
      } else {
        st.stage("l2_march: ");
        hipLaunchKernelGGL(l2_march, dim3(grid), dim3(kThreads), 0, 0, d_buf.get(), slice_words, reps, inject_kind,
                           inject_kind == 0 || inject_kind == 1 ? inject_blocks : 0, d_table, d_slice_xcc, d_first,
                           d_counters);
      }
      return hipGetLastError();
    });
    st.stage("");
    out->atomic_ms = ms[0];
    out->march_ms = ms[1];
    // the slices of each writer xcc, in slice order
    CANARY_HIP(st, hipMemcpy(h_state.data() + kSliceXccOff, d_slice_xcc, sizeof(unsigned int) * grid,
                             hipMemcpyDeviceToHost));
    if (st.ok()) {
      const unsigned int* sx = reinterpret_cast<const unsigned int*>(h_state.data() + kSliceXccOff);
      h_lists.assign(kFabricXccs + 1, 0);  // list_off[17], then the lists
      for (int w = 0; w < kFabricXccs; ++w) {
        h_lists[w] = static_cast<int>(h_lists.size()) - (kFabricXccs + 1);
        for (int s = 0; s < grid; ++s)
          if (sx[s] == static_cast<unsigned int>(w)) h_lists.push_back(s);
      }
      h_lists[kFabricXccs] = static_cast<int>(h_lists.size()) - (kFabricXccs + 1);  // <= grid
      st.check(hipMemcpy(d_lists.get(), h_lists.data(), sizeof(int) * h_lists.size(), hipMemcpyHostToDevice));
    }
    float exchange_ms[1] = {0};
    time_stages(st, ev, exchange_ms, [&](int) {
      st.stage("xcd_exchange: ");
      hipLaunchKernelGGL(xcd_exchange, dim3(grid), dim3(kThreads), 0, 0, d_buf.get(), slice_words, grid,
                         d_lists.get() + kFabricXccs + 1, d_lists.get(), d_matrix, d_counters);
      return hipGetLastError();
    });
    st.stage("");
    out->exchange_ms = exchange_ms[0];
  }
  CANARY_HIP(st, d_state.download(h_state.data()));
  if (st.ok()) h_got.resize(h_tables.size());
  CANARY_HIP(st, d_tables.download(h_got.data()));
  if (st.ok()) {
    const auto* table = reinterpret_cast<const amdgpu_canary_xcc_slot*>(h_state.data() + kTableOff);
    const auto* matrix = reinterpret_cast<const amdgpu_canary_pair_slot*>(h_state.data() + kMatrixOff);
    const auto* counters = reinterpret_cast<const unsigned long long*>(h_state.data() + kCountersOff);
    const auto* sx = reinterpret_cast<const unsigned int*>(h_state.data() + kSliceXccOff);
    unsigned long long first = 0;
    std::memcpy(&first, h_state.data() + kFirstOff, sizeof(first));
    for (int x = 0; x < kFabricXccs; ++x) {
      out->xccs_reached += table[x].blocks > 0;
      out->l2_errors += table[x].bad;
    }
    out->unlocated_errors = counters[1];
    out->l2_errors += counters[1];
    out->moved = counters[0] + counters[2];
    for (int c = 0; c < kFabricXccs * kFabricXccs; ++c) {
      out->pairs_reached += matrix[c].reads > 0;
      out->xcd_errors += matrix[c].bad;
    }
    out->xcd_errors += counters[3];
    out->pairs_expected = out->xccs_reached * out->xccs_reached;
    out->march_read_bytes = static_cast<unsigned long long>(grid) * slice_words * 16ull * (reps + 1);
    if (first != ~0ull) {
      out->first_bad_slice = static_cast<int>(first >> 32);
      out->first_bad_offset = static_cast<unsigned int>(first);
      if (out->first_bad_slice < grid && sx[out->first_bad_slice] < static_cast<unsigned int>(kFabricXccs))
        out->first_bad_xcc = static_cast<int>(sx[out->first_bad_slice]);
    }
    want.resize(table_bytes(kTicket));
    for (int op = 0; op < kAtomicOps; ++op) {
      int first_elem = -1;
      atomic_expected(op, grid, want.data());
      out->atomic_bad[op] = atomic_compare(op, h_got.data() + table_offset(op), want.data(), &first_elem);
      if (op == kCasInc) {  // loops that ran out of retries
        unsigned int capped = 0;
        std::memcpy(&capped, h_got.data() + kCappedOffset, sizeof(capped));
        if (capped && out->atomic_bad[op] == 0) first_elem = 0;
        out->atomic_bad[op] += capped;
      }
      if (out->atomic_bad[op] && out->first_bad_op < 0) {
        out->first_bad_op = op;
        out->first_bad_elem = first_elem;
      }
      out->atomic_errors += out->atomic_bad[op];
    }
    if (xcc_table_out) std::memcpy(xcc_table_out, table, sizeof(amdgpu_canary_xcc_slot) * kFabricXccs);
    if (pair_matrix_out)
      std::memcpy(pair_matrix_out, matrix, sizeof(amdgpu_canary_pair_slot) * kFabricXccs * kFabricXccs);
    if (slice_xcc_len > 0)
      std::memcpy(slice_xcc_out, sx, sizeof(unsigned int) * (slice_xcc_len < grid ? slice_xcc_len : grid));
  }
  return st.report("fabric check: ", err, err_len);
}

}  // extern "C"
