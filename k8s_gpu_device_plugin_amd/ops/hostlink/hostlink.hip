// MI355X (gfx950 / CDNA4) health canary: the link between the GPU and the host.
//
// Every other check stays on the package.  This one moves a payload over PCIe in both
// directions, by both paths a container uses, and issues the atomics ROCm itself relies on,
// over pinned, coherent host memory (hipHostMallocCoherent | hipHostMallocMapped):
//
//   * host_read: the host fills the buffer with an address-derived pattern (unique per 16-B
//     word), 256-thread workgroups read it in tile-stride order with 16-B non-temporal
//     loads, UNROLL independent ones in flight per lane, and compare.  Each workgroup reads
//     HW_REG_XCC_ID first and last; its bytes and wrong 32-bit words go to table[xcc], a
//     workgroup whose xcc changed is counted as moved and its errors as unlocated.
//   * host_write: tile_fill stores another pattern in the same traversal and records the
//     xcc of each workgroup; the HOST verifies.  The writer of word i is workgroup
//     (i / tile) % grid, so its xcc locates a wrong word.
//   * copy_h2d: the host refills, hipMemcpyAsync pinned -> device (the copy-engine path of
//     hipMemcpy), dev_verify compares on the device.
//   * copy_d2h: tile_fill writes the device buffer, hipMemcpyAsync device -> pinned, the
//     host verifies.
//   * host_atomic: system-scope FetchAdd, Swap and CAS in 32 and 64 bits (the three
//     AtomicOps PCIe defines) on a small pinned table, while the calling host thread adds
//     to the same words; the host predicts the tables (hostlink_host.h).
//
// No workgroup waits for another and the GPU never waits for the host: every hand-off is a
// kernel boundary or a synchronize, every loop is bounded by an argument or a constant.
// Fault injection perturbs values that are then compared, never an address.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/hostlink.py).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hostlink.h"

namespace {

using namespace canary;
using hostlink::HostBuffer;
using hostlink::Word16;
using hostlink::kLinkOps;
using hostlink::kThreads;

constexpr int kInjectKinds = 5;  // 0 read, 1 write, 2 h2d, 3 d2h, 4 atomic
// Measured on an MI355X (docs/CANARY.md, "Host link", Measured): one workgroup per CU with
// UNROLL 2, the smallest configuration tried, read fastest (55.6-56.6 GB/s; UNROLL 4 and 8 and
// larger grids 51-54) and wrote within run-to-run spread of the best; 64 workgroups of atomics
// took 3.4 ms beside 5.0 ms for the four bulk stages at 64 MiB, so that grid was kept.
constexpr int kDefaultUnroll = 2;
constexpr int kDefaultAtomicBlocks = hostlink::kAtomicMaxBlocks;
constexpr int kKernelStartWaitMs = 5;        // the host's bounded wait for host_atomic's first add
constexpr size_t kWarmCopyBytes = 1u << 20;  // untimed copy in each direction before the timed ones

__device__ __forceinline__ uint32_t xcc_id() { return __builtin_amdgcn_s_getreg(getreg_imm(kHwRegXccId, 0, 4)) & 0xFu; }

__device__ __forceinline__ u32x4 pattern4(uint64_t idx, uint32_t seed) {
  const Word16 w = hostlink::pattern(idx, seed);
  u32x4 v = {w.c[0], w.c[1], w.c[2], w.c[3]};
  return v;
}

// Compares one loaded 16-B word; keeps the lowest byte offset of a wrong 32-bit word.
__device__ __forceinline__ void check16(const u32x4& v, const u32x4& want, uint64_t word, uint32_t& bad, uint64_t& first) {
  for (int c = 0; c < 4; ++c) {
    if (v[c] != want[c]) {
      ++bad;
      const uint64_t off = word * 16u + 4u * c;
      first = off < first ? off : first;
    }
  }
}

// The lowest wrong byte offset of the workgroup to *first_bad: one 64-bit atomicMin per
// workgroup that saw one.  Every thread calls it.
__device__ __forceinline__ void block_min_first(uint32_t bad, uint64_t first, unsigned long long* __restrict__ first_bad) {
  __shared__ unsigned long long s_first;
  if (threadIdx.x == 0) s_first = ~0ull;
  __syncthreads();
  if (bad) atomicMin(&s_first, static_cast<unsigned long long>(first));
  __syncthreads();
  if (threadIdx.x == 0 && s_first != ~0ull) atomicMin(first_bad, s_first);
}

// counters: [0] moved workgroups, [1] their wrong words.  Tile-stride like tile_verify in
// ops/hbm.hip: workgroup b reads tiles b, b + G, ... of 256 * UNROLL words; the words past
// the last whole tile are a scalar tail.  `buf` is host memory.
template <int UNROLL>
__global__ void __launch_bounds__(kThreads) host_read(const u32x4* __restrict__ buf, uint64_t n, uint32_t seed,
                                                     amdgpu_hostlink_xcc_slot* __restrict__ table,
                                                     unsigned int* __restrict__ block_xcc,
                                                     unsigned long long* __restrict__ first_bad,
                                                     unsigned long long* __restrict__ counters) {
  const uint32_t xcc = xcc_id();
  constexpr uint64_t tile = 256ull * UNROLL;
  uint32_t bad = 0;
  uint64_t first = ~0ull, words = 0;
  for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += static_cast<uint64_t>(gridDim.x) * tile) {
    if (t0 + tile <= n) {
      u32x4 v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = __builtin_nontemporal_load(buf + t0 + u * 256ull + threadIdx.x);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const uint64_t i = t0 + u * 256ull + threadIdx.x;
        check16(v[u], pattern4(i, seed), i, bad, first);
      }
      words += tile;
    } else {
      for (uint64_t i = t0 + threadIdx.x; i < n; i += 256) check16(__builtin_nontemporal_load(buf + i), pattern4(i, seed), i, bad, first);
      words += n - t0;
    }
  }
  block_min_first(bad, first, first_bad);
  const uint32_t xcc_after = xcc_id();
  const bool located = xcc_after == xcc;  // uniform over the workgroup
  block_add_errors(bad, located ? &table[xcc].read_bad : &counters[1]);  // xcc < kHostlinkXccs by the mask
  if (threadIdx.x != 0 || words == 0) return;  // an idle workgroup adds nothing
  block_xcc[blockIdx.x] = xcc;
  if (located) {
    atomicAdd(&table[xcc].read_blocks, 1ull);
    atomicAdd(&table[xcc].read_bytes, static_cast<unsigned long long>(words) * 16ull);
  } else {
    atomicAdd(&counters[0], 1ull);
  }
}

// Stores pattern(i, seed) with 16-B non-temporal stores in the same traversal, into host
// memory (host_write) or device memory (copy_d2h).  The first inject_blocks workgroups flip
// one bit of the first word they store.
template <int UNROLL>
__global__ void __launch_bounds__(kThreads) tile_fill(u32x4* __restrict__ buf, uint64_t n, uint32_t seed, int inject_blocks,
                                                     unsigned int* __restrict__ block_xcc) {
  const uint32_t xcc = xcc_id();
  constexpr uint64_t tile = 256ull * UNROLL;
  const uint64_t flip = static_cast<int>(blockIdx.x) < inject_blocks ? blockIdx.x * tile : ~0ull;
  for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += static_cast<uint64_t>(gridDim.x) * tile) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint64_t i = t0 + u * 256ull + threadIdx.x;
      if (i < n) {
        u32x4 v = pattern4(i, seed);
        if (i == flip) v[hostlink::kInjectComp] ^= 1u << hostlink::kInjectBit;
        __builtin_nontemporal_store(v, buf + i);
      }
    }
  }
  if (threadIdx.x == 0 && block_xcc != nullptr && blockIdx.x * tile < n) block_xcc[blockIdx.x] = xcc;
}

// Plain grid-stride verify of the device buffer after the host-to-device copy.
__global__ void __launch_bounds__(kThreads) dev_verify(const u32x4* __restrict__ buf, uint64_t n, uint32_t seed,
                                                      unsigned long long* __restrict__ errors,
                                                      unsigned long long* __restrict__ first_bad) {
  uint32_t bad = 0;
  uint64_t first = ~0ull;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += step)
    check16(buf[i], pattern4(i, seed), i, bad, first);
  block_min_first(bad, first, first_bad);
  block_add_errors(bad, errors);
}

template <typename T>
__device__ __forceinline__ T sys_add(T* p, T v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One operation per thread and add form; lane 0 of each wave then takes a ticket, runs one
// CAS-increment loop and makes one exchange.  `tables` is host memory.  Thread 0 of
// workgroup 0 perturbs its operand of inject_op (-1: none).
__global__ void __launch_bounds__(kThreads) host_atomic(unsigned char* __restrict__ tables, int inject_op) {
  using namespace hostlink;
  const uint32_t gid = blockIdx.x * kThreads + threadIdx.x;  // < 2^14 (host-checked grid)
  const bool inject = gid == 0;
  sys_add(reinterpret_cast<uint32_t*>(tables + table_offset(kU32Add)) + atomic_elem(kU32Add, gid, 0),
          static_cast<uint32_t>(atomic_operand(kU32Add, gid, 0, inject && inject_op == kU32Add)));
  sys_add(reinterpret_cast<uint64_t*>(tables + table_offset(kU64Add)) + atomic_elem(kU64Add, gid, 0),
          atomic_operand(kU64Add, gid, 0, inject && inject_op == kU64Add));
  if ((threadIdx.x & (kLanes - 1)) != 0) return;
  const uint32_t wave = gid >> 6, waves = gridDim.x * (kThreads / kLanes);
  // a ticket, whose returned value picks the word the wave then marks
  uint32_t* ticket = reinterpret_cast<uint32_t*>(tables + table_offset(kTicket));
  const uint32_t mine = sys_add(ticket, 1u);
  if (mine < waves && mine < static_cast<uint32_t>(kMaxWaves))
    sys_add(ticket + 1 + mine, static_cast<uint32_t>(atomic_operand(kTicket, gid, 0, inject && inject_op == kTicket)));
  // a CAS-increment loop with capped retries
  uint64_t* p = reinterpret_cast<uint64_t*>(tables + table_offset(kCasInc)) + (atomic_row_hash(kCasInc, wave, 0) & (kCasWords - 1));
  const uint64_t amount = atomic_operand(kCasInc, gid, 0, inject && inject_op == kCasInc);
  uint64_t old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  bool done = false;
  for (int tries = 0; tries < kCasRetries && !done; ++tries) {
    uint64_t seen = old;
    done = __hip_atomic_compare_exchange_strong(p, &seen, old + amount, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_SYSTEM);
    old = seen;
  }
  if (!done) sys_add(reinterpret_cast<uint32_t*>(tables + kCappedOffset), 1u);
  // an exchange of the wave's token into one of 64 slots; what came back is stored
  uint64_t* slots = reinterpret_cast<uint64_t*>(tables + table_offset(kSwap));
  const uint64_t back = __hip_atomic_exchange(slots + (atomic_row_hash(kSwap, wave, 0) & (kSwapSlots - 1)),
                                              atomic_operand(kSwap, gid, 0, inject && inject_op == kSwap), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_SYSTEM);
  if (wave < static_cast<uint32_t>(kMaxWaves)) slots[kSwapSlots + wave] = back;
}

const char* const kOpNames[kLinkOps] = {"u32 add", "u64 add", "ticket", "cas inc", "swap"};

// The kernels of one UNROLL.
struct Variant {
  int unroll;
  void (*read)(const u32x4*, uint64_t, uint32_t, amdgpu_hostlink_xcc_slot*, unsigned int*, unsigned long long*,
               unsigned long long*);
  void (*fill)(u32x4*, uint64_t, uint32_t, int, unsigned int*);
};
constexpr Variant kVariants[] = {{2, host_read<2>, tile_fill<2>}, {4, host_read<4>, tile_fill<4>}, {8, host_read<8>, tile_fill<8>}};

const Variant* variant_of(int unroll) {
  for (const Variant& v : kVariants)
    if (v.unroll == (unroll == 0 ? kDefaultUnroll : unroll)) return &v;
  return nullptr;
}

class CpuTimer {  // adds the time it lived to *ms
 public:
  explicit CpuTimer(double* ms) : ms_(ms), t0_(std::chrono::steady_clock::now()) {}
  ~CpuTimer() { *ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count(); }

 private:
  double* ms_;
  std::chrono::steady_clock::time_point t0_;
};

void flip_words(Word16* buf, uint64_t n, int count) {
  for (int f = 0; f < count; ++f) buf[hostlink::inject_word(n, count, f)].c[hostlink::kInjectComp] ^= 1u << hostlink::kInjectBit;
}

}  // namespace

extern "C" {

const char* amdgpu_hostlink_atomic_op_name(int op) { return op >= 0 && op < kLinkOps ? kOpNames[op] : "?"; }

int amdgpu_hostlink_sizeof(int which) {
  return which == 0 ? static_cast<int>(sizeof(amdgpu_hostlink_xcc_slot))
         : which == 1 ? static_cast<int>(sizeof(amdgpu_hostlink_result))
                      : -1;
}

int amdgpu_hostlink_tile_words(int unroll) {
  const Variant* v = variant_of(unroll);
  return v ? 256 * v->unroll : -1;
}

int amdgpu_hostlink_pattern(unsigned long long idx0, unsigned long long n, unsigned int seed, void* out) {
  if (out == nullptr) return -1;
  Word16* w = static_cast<Word16*>(out);
  for (uint64_t i = 0; i < n; ++i) {  // `out` need not be 16-B aligned
    const Word16 v = hostlink::pattern(idx0 + i, seed);
    std::memcpy(reinterpret_cast<unsigned char*>(w) + i * 16, &v, 16);
  }
  return 0;
}

// `buf` must be 4-byte aligned.
int amdgpu_hostlink_verify(const void* buf, unsigned long long n, unsigned int seed, unsigned long long* wrong_words,
                           long long* first_offset) {
  if (buf == nullptr || wrong_words == nullptr || first_offset == nullptr) return -1;
  *wrong_words = hostlink::verify(static_cast<const Word16*>(buf), n, seed, first_offset);
  return 0;
}

// The table of `op` after `blocks` workgroups (1..64) and `host_adds` host adds, as the device
// lays it out.  Returns the bytes written, or -1 on a bad argument or a short buffer.
int amdgpu_hostlink_atomic_expected(int op, int blocks, int host_adds, void* out, int out_bytes) {
  if (op < 0 || op >= kLinkOps || blocks < 1 || blocks > hostlink::kAtomicMaxBlocks || host_adds < 0 ||
      host_adds > hostlink::kMaxHostAdds || out == nullptr || out_bytes < hostlink::table_bytes(op))
    return -1;
  hostlink::atomic_expected(op, blocks, host_adds, static_cast<unsigned char*>(out));
  return hostlink::table_bytes(op);
}

// The acceptance rule of `op` on a caller-supplied table: wrong elements, -1 on a bad argument.
long long amdgpu_hostlink_atomic_compare(int op, int blocks, int host_adds, const void* got, int got_bytes, int* first) {
  if (op < 0 || op >= kLinkOps || blocks < 1 || blocks > hostlink::kAtomicMaxBlocks || host_adds < 0 ||
      host_adds > hostlink::kMaxHostAdds || got == nullptr || first == nullptr || got_bytes < hostlink::table_bytes(op))
    return -1;
  return static_cast<long long>(hostlink::atomic_compare(op, blocks, host_adds, static_cast<const unsigned char*>(got), first));
}

int amdgpu_hostlink_describe(const amdgpu_hostlink_result* r, const amdgpu_hostlink_xcc_slot* xcc_table, char* buf,
                             int len) {
  for (int s = 0; s < 2; ++s) {
    const unsigned long long errors = s == 0 ? r->read_errors : r->write_errors;
    if (errors == 0) continue;
    const char* stage = s == 0 ? "read" : "write";
    const char* verb = s == 0 ? "read" : "written";
    int bad_xccs = 0;
    for (int x = 0; x < kHostlinkXccs; ++x) bad_xccs += (s == 0 ? xcc_table[x].read_bad : xcc_table[x].write_bad) > 0;
    if (r->first_bad_xcc[s] < 0)
      return std::snprintf(buf, len, "host %s check: %llu wrong word%s %s on an unknown xcc (first at offset 0x%llx)", stage,
                           errors, plural(errors), verb, static_cast<unsigned long long>(r->first_bad_offset[s]));
    int n = std::snprintf(buf, len, "host %s check: %llu wrong word%s %s on xcc%d (first at offset 0x%llx)", stage, errors,
                          plural(errors), verb, r->first_bad_xcc[s], static_cast<unsigned long long>(r->first_bad_offset[s]));
    if (bad_xccs > 1 && n > 0 && n < len)
      n += std::snprintf(buf + n, len - n, " (+%d more xcc%s)", bad_xccs - 1, bad_xccs > 2 ? "s" : "");
    return n;
  }
  for (int s = 2; s < 4; ++s) {
    const unsigned long long errors = s == 2 ? r->h2d_errors : r->d2h_errors;
    if (errors == 0) continue;
    return std::snprintf(buf, len, "host copy check: %llu wrong word%s after the %s copy (first at offset 0x%llx)", errors,
                         plural(errors), s == 2 ? "host-to-device" : "device-to-host",
                         static_cast<unsigned long long>(r->first_bad_offset[s]));
  }
  if (r->atomic_errors > 0)
    return std::snprintf(buf, len, "host atomic check: %llu wrong element%s in %s (first at %d)", r->atomic_errors,
                         plural(r->atomic_errors), amdgpu_hostlink_atomic_op_name(r->first_bad_op), r->first_bad_elem);
  return 0;
}

int amdgpu_hostlink_run(int device, unsigned long long bytes, int blocks, int reps, int inject_kind, int inject_op,
                        int inject_n, int host_adds, int unroll, int atomic_blocks,
                        amdgpu_hostlink_xcc_slot* xcc_table_out, unsigned int* block_xcc_out, int block_xcc_len,
                        amdgpu_hostlink_result* out, char* err, int err_len) {
  using namespace hostlink;
  std::memset(out, 0, sizeof(*out));
  for (long long& f : out->first_bad_offset) f = -1;
  out->first_bad_op = out->first_bad_elem = out->first_bad_xcc[0] = out->first_bad_xcc[1] = -1;
  const Variant* var = variant_of(unroll);
  const uint64_t n = bytes / 16;
  if (bytes == 0 || bytes % 16 != 0 || bytes > (64ull << 30) || blocks < 0 || blocks > kMaxBlocks || reps < 1 || reps > 16 ||
      inject_kind < -1 || inject_kind >= kInjectKinds || inject_op < 0 || inject_op >= kLinkOps || inject_n < 0 ||
      (inject_kind >= 0 && inject_kind < 4 && static_cast<uint64_t>(inject_n) > n) || host_adds < 0 ||
      host_adds > kMaxHostAdds || var == nullptr || atomic_blocks < 0 || atomic_blocks > kAtomicMaxBlocks ||
      block_xcc_len < 0 || (block_xcc_out == nullptr && block_xcc_len != 0)) {
    std::snprintf(err, err_len,
                  "host link check: bad arguments (bytes %llu a positive multiple of 16, blocks %d in 0..%d, reps %d in "
                  "1..16, inject %d/%d/%d, host_adds %d, unroll %d in 2, 4, 8, atomic_blocks %d in 0..%d)",
                  bytes, blocks, kMaxBlocks, reps, inject_kind, inject_op, inject_n, host_adds, unroll, atomic_blocks,
                  kAtomicMaxBlocks);
    return -1;
  }
  Status st;
  hipDeviceProp_t prop;
  HostBuffer<Word16> h_buf;
  HostBuffer<unsigned char> h_tables;
  DeviceBuffer<u32x4> d_buf;
  DeviceBuffer<unsigned char> d_state;
  Events<2> ev;
  // device state of the bulk stages, one allocation
  constexpr size_t kTableOff = 0, kCountersOff = kTableOff + sizeof(amdgpu_hostlink_xcc_slot) * kHostlinkXccs,
                   kFirstOff = kCountersOff + 2 * sizeof(unsigned long long),  // read, h2d
                   kCopyErrOff = kFirstOff + 2 * sizeof(unsigned long long),
                   kBlockXccOff = kCopyErrOff + sizeof(unsigned long long);  // host_read's, then host_write's
  std::vector<unsigned char> h_state;
  int grid = 0;
  const int agrid = atomic_blocks > 0 ? atomic_blocks : kDefaultAtomicBlocks;
  const uint64_t tile = 256ull * var->unroll;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (st.ok()) {
    grid = launch_plan(blocks, prop.multiProcessorCount, 1).grid;
    out->blocks = grid;
    out->atomic_blocks = agrid;
    out->reps = reps;
    out->bytes = bytes;
    out->host_adds = host_adds;
    h_state.assign(kBlockXccOff + 2 * sizeof(unsigned int) * grid, 0);
    std::memset(h_state.data() + kFirstOff, 0xFF, 2 * sizeof(unsigned long long));  // no wrong word yet
    std::memset(h_state.data() + kBlockXccOff, 0xFF, 2 * sizeof(unsigned int) * grid);
  }
  CANARY_HIP(st, h_buf.alloc(bytes), "hipHostMalloc of the pinned buffer: ");
  CANARY_HIP(st, h_tables.alloc(kTablesAlloc), "hipHostMalloc of the atomic tables: ");
  CANARY_HIP(st, d_buf.alloc(bytes));
  CANARY_HIP(st, d_state.alloc(h_state.size()));
  CANARY_HIP(st, d_state.upload(h_state.data()));
  CANARY_HIP(st, ev.create());
  if (!st.ok()) return st.report("host link check: ", err, err_len);

  auto* d_table = reinterpret_cast<amdgpu_hostlink_xcc_slot*>(d_state.get() + kTableOff);
  auto* d_counters = reinterpret_cast<unsigned long long*>(d_state.get() + kCountersOff);
  auto* d_first = reinterpret_cast<unsigned long long*>(d_state.get() + kFirstOff);
  auto* d_copy_err = reinterpret_cast<unsigned long long*>(d_state.get() + kCopyErrOff);
  auto* d_block_xcc = reinterpret_cast<unsigned int*>(d_state.get() + kBlockXccOff);
  const u32x4* pinned_ro = reinterpret_cast<const u32x4*>(h_buf.device());
  u32x4* pinned = reinterpret_cast<u32x4*>(h_buf.device());
  const int vgrid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 4 : 4;  // dev_verify: HBM-side, not a link rate

  // every kernel once over no words, so no timed launch pays for loading its code
  st.stage("warm-up: ");
  if (st.ok()) {
    hipLaunchKernelGGL(var->read, dim3(1), dim3(kThreads), 0, 0, pinned_ro, 0, 0u, d_table, d_block_xcc, d_first, d_counters);
    hipLaunchKernelGGL(var->fill, dim3(1), dim3(kThreads), 0, 0, pinned, 0, 0u, 0, static_cast<unsigned int*>(nullptr));
    hipLaunchKernelGGL(dev_verify, dim3(1), dim3(kThreads), 0, 0, d_buf.get(), 0, 0u, d_copy_err, d_first + 1);
    st.check(hipGetLastError());
  }
  // ... and one short copy in each direction: the first copy of a process sets the copy path up
  const size_t warm = bytes < kWarmCopyBytes ? static_cast<size_t>(bytes) : kWarmCopyBytes;
  CANARY_HIP(st, hipMemcpyAsync(d_buf.get(), h_buf.host(), warm, hipMemcpyHostToDevice, 0));
  CANARY_HIP(st, hipMemcpyAsync(h_buf.host(), d_buf.get(), warm, hipMemcpyDeviceToHost, 0));
  CANARY_HIP(st, hipDeviceSynchronize());

  std::vector<unsigned long long> write_bad(grid, 0);
  float ms[1] = {0};
  for (int r = 0; r < reps && st.ok(); ++r) {
    // stage 1: the GPU reads host memory
    {
      CpuTimer t(&out->host_cpu_ms);
      fill(h_buf.host(), n, kSeedRead + r);
      if (inject_kind == 0 && r == 0) flip_words(h_buf.host(), n, inject_n);
    }
    time_stages(st, ev, ms, [&](int) {
      st.stage("host_read: ");
      hipLaunchKernelGGL(var->read, dim3(grid), dim3(kThreads), 0, 0, pinned_ro, n, kSeedRead + r, d_table, d_block_xcc,
                         d_first, d_counters);
      return hipGetLastError();
    });
    out->stage_ms[0] += ms[0];
    // stage 2: the GPU writes host memory, the host verifies
    time_stages(st, ev, ms, [&](int) {
      st.stage("host_write: ");
      hipLaunchKernelGGL(var->fill, dim3(grid), dim3(kThreads), 0, 0, pinned, n, kSeedWrite + r,
                         inject_kind == 1 && r == 0 ? inject_n : 0, d_block_xcc + grid);
      return hipGetLastError();
    });
    out->stage_ms[1] += ms[0];
    if (st.ok()) {
      CpuTimer t(&out->host_cpu_ms);
      long long first = -1;
      out->write_errors += verify_each(h_buf.host(), n, kSeedWrite + r, 0, &first, [&](uint64_t i, uint32_t bad) {
        write_bad[(i / tile) % grid] += bad;
      });
      if (out->first_bad_offset[1] < 0) out->first_bad_offset[1] = first;
    }
    // stage 3: the copy engine reads host memory, the device verifies
    {
      CpuTimer t(&out->host_cpu_ms);
      fill(h_buf.host(), n, kSeedH2D + r);
      if (inject_kind == 2 && r == 0) flip_words(h_buf.host(), n, inject_n);
    }
    time_stages(st, ev, ms, [&](int) {
      st.stage("copy_h2d: ");
      return hipMemcpyAsync(d_buf.get(), h_buf.host(), bytes, hipMemcpyHostToDevice, 0);
    });
    out->stage_ms[2] += ms[0];
    st.stage("dev_verify: ");
    if (st.ok()) {
      hipLaunchKernelGGL(dev_verify, dim3(vgrid), dim3(kThreads), 0, 0, d_buf.get(), n, kSeedH2D + r, d_copy_err, d_first + 1);
      st.check(hipGetLastError());
    }
    // stage 4: the device fills its buffer, the copy engine writes host memory, the host verifies
    st.stage("tile_fill: ");
    if (st.ok()) {
      hipLaunchKernelGGL(var->fill, dim3(grid), dim3(kThreads), 0, 0, d_buf.get(), n, kSeedD2H + r,
                         inject_kind == 3 && r == 0 ? inject_n : 0, static_cast<unsigned int*>(nullptr));
      st.check(hipGetLastError());
    }
    time_stages(st, ev, ms, [&](int) {
      st.stage("copy_d2h: ");
      return hipMemcpyAsync(h_buf.host(), d_buf.get(), bytes, hipMemcpyDeviceToHost, 0);
    });
    out->stage_ms[3] += ms[0];
    if (st.ok()) {
      CpuTimer t(&out->host_cpu_ms);
      long long first = -1;
      out->d2h_errors += verify(h_buf.host(), n, kSeedD2H + r, &first);
      if (out->first_bad_offset[3] < 0) out->first_bad_offset[3] = first;
    }
  }

  // stage 5: system-scope atomics, with the host adding to the same table meanwhile
  if (st.ok()) {
    std::memset(h_tables.host(), 0, kTablesAlloc);
    for (int op = 0; op < kLinkOps; ++op) atomic_initial(op, h_tables.host() + table_offset(op));
    uint64_t* t64 = reinterpret_cast<uint64_t*>(h_tables.host() + table_offset(kU64Add));
    // the counter the host watches: the sum of the first row of the u32 add table, which the
    // kernel's waves add to from start to end and the host never does
    const uint32_t* t32 = reinterpret_cast<const uint32_t*>(h_tables.host() + table_offset(kU32Add));
    auto progress = [t32] {
      uint32_t sum = 0;
      for (int e = 0; e < kLanes; ++e) sum += __atomic_load_n(&t32[e], __ATOMIC_RELAXED);
      return sum;
    };
    const uint32_t idle = progress();
    time_stages(st, ev, ms, [&](int) {
      st.stage("host_atomic: ");
      hipLaunchKernelGGL(host_atomic, dim3(agrid), dim3(kThreads), 0, 0, h_tables.device(), inject_kind == 4 ? inject_op : -1);
      const hipError_t e = hipGetLastError();
      // the adds should land while the kernel runs: wait, for a bounded time, for its first add there
      const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(kKernelStartWaitMs);
      while (e == hipSuccess && host_adds > 0 && progress() == idle && std::chrono::steady_clock::now() < deadline) {
      }
      const uint32_t before = progress();
      for (int i = 0; i < host_adds; ++i) __atomic_fetch_add(&t64[host_add_elem(i)], host_add_operand(i), __ATOMIC_RELAXED);
      out->atomic_overlap = host_adds > 0 && progress() != before;
      return e;
    });
    out->atomic_ms = ms[0];
  }
  st.stage("");
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, d_state.download(h_state.data()));
  if (st.ok()) {
    auto* table = reinterpret_cast<amdgpu_hostlink_xcc_slot*>(h_state.data() + kTableOff);
    const auto* counters = reinterpret_cast<const unsigned long long*>(h_state.data() + kCountersOff);
    const auto* bx = reinterpret_cast<const unsigned int*>(h_state.data() + kBlockXccOff);
    unsigned long long first[2], copy_err = 0;
    std::memcpy(first, h_state.data() + kFirstOff, sizeof(first));
    std::memcpy(&copy_err, h_state.data() + kCopyErrOff, sizeof(copy_err));
    // what the host found in each writer's words goes to the writer's xcc
    // (a workgroup that recorded none had no work and wrote nothing)
    for (int b = 0; b < grid; ++b) {
      const unsigned int x = bx[grid + b];
      if (x >= static_cast<unsigned int>(kHostlinkXccs)) continue;
      table[x].write_blocks += 1;
      table[x].write_bad += write_bad[b];
    }
    for (int x = 0; x < kHostlinkXccs; ++x) {
      out->xccs_reached += table[x].read_blocks > 0;
      out->read_errors += table[x].read_bad;
    }
    out->unlocated_errors = counters[1];
    out->read_errors += counters[1];
    out->moved = counters[0];
    out->h2d_errors = copy_err;
    if (first[0] != ~0ull) out->first_bad_offset[0] = static_cast<long long>(first[0]);
    if (first[1] != ~0ull) out->first_bad_offset[2] = static_cast<long long>(first[1]);
    for (int s = 0; s < 2; ++s) {  // the workgroup that read / wrote the first wrong word, and its xcc
      const long long off = out->first_bad_offset[s];
      if (off < 0) continue;
      const unsigned int x = bx[s * grid + static_cast<int>((static_cast<uint64_t>(off) / 16 / tile) % grid)];
      if (x < static_cast<unsigned int>(kHostlinkXccs)) out->first_bad_xcc[s] = static_cast<int>(x);
    }
    for (int op = 0; op < kLinkOps; ++op) {
      int first_elem = -1;
      out->atomic_bad[op] = atomic_compare(op, agrid, host_adds, h_tables.host() + table_offset(op), &first_elem);
      if (op == kCasInc) {  // loops that ran out of retries
        unsigned int capped = 0;
        std::memcpy(&capped, h_tables.host() + kCappedOffset, sizeof(capped));
        if (capped && out->atomic_bad[op] == 0) first_elem = 0;
        out->atomic_bad[op] += capped;
      }
      if (out->atomic_bad[op] && out->first_bad_op < 0) {
        out->first_bad_op = op;
        out->first_bad_elem = first_elem;
      }
      out->atomic_errors += out->atomic_bad[op];
    }
    if (xcc_table_out) std::memcpy(xcc_table_out, table, sizeof(amdgpu_hostlink_xcc_slot) * kHostlinkXccs);
    for (int s = 0; s < 2 && block_xcc_len > 0; ++s) {
      std::memset(block_xcc_out + s * block_xcc_len, 0xFF, sizeof(unsigned int) * block_xcc_len);
      std::memcpy(block_xcc_out + s * block_xcc_len, bx + s * grid,
                  sizeof(unsigned int) * (block_xcc_len < grid ? block_xcc_len : grid));
    }
  }
  return st.report("host link check: ", err, err_len);
}

}  // extern "C"
