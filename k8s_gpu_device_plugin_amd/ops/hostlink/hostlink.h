// C ABI of the host-link check (ops/hostlink/libamdgpu_hostlink.so), mirrored with ctypes in
// ops/hostlink.py, and the owner of pinned host memory.  The library is built apart from
// libamdgpu_canary.so and shares its header-only helpers (../canary_common.h, ../canary_host.h,
// ../site.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "hostlink_host.h"

namespace hostlink {

// Owns one pinned, coherent, mapped host allocation; the only place that frees one.
template <typename T>
class HostBuffer {
 public:
  HostBuffer() = default;
  HostBuffer(const HostBuffer&) = delete;
  HostBuffer& operator=(const HostBuffer&) = delete;
  ~HostBuffer() {
    if (p_) (void)hipHostFree(p_);
  }
  hipError_t alloc(size_t bytes) {  // once per buffer
    if (p_) return hipErrorInvalidValue;
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, p, 0);
    d_ = static_cast<T*>(d);
    return e;
  }
  T* host() const { return p_; }
  T* device() const { return d_; }  // what a kernel is given

 private:
  T* p_ = nullptr;
  T* d_ = nullptr;
};

}  // namespace hostlink

extern "C" {

constexpr int kHostlinkXccs = 16;  // HW_REG_XCC_ID is 4 bits wide
constexpr int kHostlinkStages = 4;  // 0 host_read, 1 host_write, 2 copy_h2d, 3 copy_d2h (then 4: host_atomic)

struct amdgpu_hostlink_xcc_slot {  // one per xcc
  unsigned long long read_blocks;   // host_read workgroups with work that ran on it from first to last
  unsigned long long read_bytes;    // bytes they read over the link
  unsigned long long read_bad;      // wrong 32-bit words they read
  unsigned long long write_blocks;  // host_write workgroups with work that started on it
  unsigned long long write_bad;     // wrong 32-bit words the host found in what they wrote
};

struct amdgpu_hostlink_result {
  unsigned long long read_errors;       // wrong 32-bit words, unlocated ones included
  unsigned long long write_errors;
  unsigned long long h2d_errors;
  unsigned long long d2h_errors;
  unsigned long long atomic_errors;     // wrong table elements over the five forms
  unsigned long long atomic_bad[hostlink::kLinkOps];
  unsigned long long unlocated_errors;  // read errors of workgroups whose xcc changed while they ran
  unsigned long long moved;             // those workgroups
  long long first_bad_offset[kHostlinkStages];  // byte offset of the first wrong 32-bit word (-1: none)
  unsigned long long bytes;
  int first_bad_op;                     // first wrong atomic element: operation (-1: none)
  int first_bad_elem;
  int first_bad_xcc[2];                 // xcc that read / wrote the first wrong word (-1: none or unknown)
  int xccs_reached;                     // xccs with a located host_read workgroup
  int blocks;                           // the grid of the bulk kernels
  int atomic_blocks;                    // the grid of host_atomic
  int reps;
  int atomic_overlap;                   // 1: the host saw the kernel's u32 adds move between its first and last add
  int host_adds;
  double stage_ms[kHostlinkStages];     // device time of each bulk stage, all repetitions
  double atomic_ms;
  double host_cpu_ms;                   // the host's fills and verifies
};

// Runs the five stages on `device` over `bytes` (a positive multiple of 16) of pinned host
// memory.  blocks: grid of the bulk kernels (0: one workgroup per CU); unroll: 16-B accesses
// a lane keeps in flight (0: the default; 2, 4 or 8); atomic_blocks: grid of the atomics
// (0: the default).  inject_kind -1 none, 0 read, 1 write, 2 h2d, 3 d2h (inject_n words or
// workgroups), 4 atomic (one operand of operation inject_op).  xcc_table_out (kHostlinkXccs
// slots) and block_xcc_out (2 * block_xcc_len entries: the xcc of the first block_xcc_len
// workgroups of host_read, then of host_write; all-ones where a workgroup had no work) may
// be null.  0, or -1 with `err` set.
int amdgpu_hostlink_run(int device, unsigned long long bytes, int blocks, int reps, int inject_kind, int inject_op,
                        int inject_n, int host_adds, int unroll, int atomic_blocks,
                        amdgpu_hostlink_xcc_slot* xcc_table_out, unsigned int* block_xcc_out, int block_xcc_len,
                        amdgpu_hostlink_result* result, char* err, int err_len);
// "host read check: 3 wrong words read on xcc5 (first at offset 0x1a40)" of the first failing stage; 0 if none failed
int amdgpu_hostlink_describe(const amdgpu_hostlink_result* r, const amdgpu_hostlink_xcc_slot* xcc_table, char* buf,
                             int len);
int amdgpu_hostlink_sizeof(int which);  // 0: amdgpu_hostlink_xcc_slot, 1: amdgpu_hostlink_result
int amdgpu_hostlink_tile_words(int unroll);  // 16-B words of one tile at `unroll` (0: the default); -1: no such kernel
// host only
int amdgpu_hostlink_pattern(unsigned long long idx0, unsigned long long n, unsigned int seed, void* out);
int amdgpu_hostlink_verify(const void* buf, unsigned long long n, unsigned int seed, unsigned long long* wrong_words,
                           long long* first_offset);
int amdgpu_hostlink_atomic_expected(int op, int blocks, int host_adds, void* out, int out_bytes);
long long amdgpu_hostlink_atomic_compare(int op, int blocks, int host_adds, const void* got, int got_bytes, int* first);
const char* amdgpu_hostlink_atomic_op_name(int op);  // "u64 add"

}  // extern "C"

static_assert(sizeof(amdgpu_hostlink_xcc_slot) == 40, "hostlink.XccSlot");
static_assert(sizeof(amdgpu_hostlink_result) == 224, "hostlink.HostLinkResult");
