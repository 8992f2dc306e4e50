// Shared by every gfx950 canary source (canary.hip, hbm.hip, gemm.hip, datapath.hip,
// sites.hip, fabric.hip, cumem.hip) and, through canary_host.h, by the libraries of the
// host-link, pace and LDS-path checks.  Device side: the s_getreg immediates, site_id(), the
// wave and block error reductions.  And the C ABI, declared here once: every result struct that
// canary.py mirrors with ctypes, with its size pinned, and the prototype of every exported entry
// point that another source calls.  The host-side helpers are in canary_host.h, the packed site
// and kMaxBlocks in site.h, the operand hash, MFMA vector types, lane maps and forms in mfma_forms.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "site.h"

namespace canary {

constexpr int kWave = 64;

// s_getreg_b32 immediate: register id 5:0, bit offset 10:6, size - 1 15:11
constexpr int kHwRegHwId = 4, kHwRegXccId = 20;
constexpr int getreg_imm(int reg, int offset, int size) { return ((size - 1) << 11) | (offset << 6) | reg; }

using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

// Sum over the wave; lane 0 holds it.  One loop, two spellings: which one a kernel calls changes
// the registers the compiler allocates and how it unrolls the kernel's other loops (mfma_exact:
// 32 VGPRs in place, 48 by value).  In place: mfma_exact, lowp_exact, fp8_exact (datapath.hip's
// exact_block), lds_march; by value: all others.  Compare the kernel-resource-usage remarks before
// changing a call site (tests/test_canary_forms.py pins canary.hip's, datapath.hip's and sites.hip's).
__device__ __forceinline__ void wave_sum(uint32_t& v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
}
__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
  wave_sum(v);
  return v;
}

// Block total of `bad`, then one atomic per block that saw any.  Every thread of a block of
// at most 256 calls it.
__device__ __forceinline__ void block_add_errors(uint32_t bad, unsigned long long* __restrict__ errors) {
  bad = wave_total(bad);
  __shared__ uint32_t wave_bad[256 / kWave];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) wave_bad[wid] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < static_cast<int>(blockDim.x / kWave); ++w) t += wave_bad[w];
    if (t) atomicAdd(errors, static_cast<unsigned long long>(t));
  }
}

}  // namespace canary

// ---- site probe (sites.hip): where on the chip each exactness check ran ----------------
// A site is (xcc, se, sh, cu, simd) packed into 14 bits (site.h: kSiteSlots of them).

namespace canary {

// HW_ID 15:4 = simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13 (3 bits: 14:13 on gfx942/950,
// bit 15 reads 0 there).  cu, sh and se are contiguous, so they move as one 8-bit field.
__device__ __forceinline__ uint32_t site_id() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(getreg_imm(kHwRegHwId, 4, 12));
  const uint32_t xcc = __builtin_amdgcn_s_getreg(getreg_imm(kHwRegXccId, 0, 4));
  return ((hw & 3u) | (((hw >> 4) & 0xFFu) << 2) | ((xcc & 0xFu) << 10)) & (kSiteSlots - 1);
}

}  // namespace canary

extern "C" {

// ---- the whole run (canary.hip) and the entry points it calls in hbm.hip, gemm.hip, datapath.hip ----
struct amdgpu_canary_result {
  int ok;
  int device;
  unsigned long long hbm_bytes;
  unsigned long long hbm_errors;
  unsigned long long mfma_errors;
  double write_gbps;
  double read_gbps;
  double mfma_tflops;
  double elapsed_ms;
  int num_cus;
  char arch[64];
  char error[256];
  double gemm_tflops;                   // LDS-staged MFMA GEMM (matrix path) rate
  unsigned long long gemm_errors;       // ABFT row/column checksum mismatches
  double fp8_tflops;                    // block-scaled fp8 MFMA rate (datapath.hip)
  double fp4_tflops;                    // block-scaled fp4 MFMA rate
  unsigned long long lowp_errors;       // fp8 / bf8 / fp4 MFMA exactness mismatches
  unsigned long long lds_errors;        // LDS march mismatches
  unsigned long long lds_bytes;         // LDS bytes per workgroup the march covered
  unsigned long long site_errors;       // site probe (sites.hip): wrong mfma + lowp + valu results + unlocated
  int cus_reached;                      // CUs the site probe ran on
  int simds_reached;                    // (CU, SIMD) sites it ran on
  int cus_unreached;                    // num_cus - cus_reached: reported, does not fail the run
  double site_ms;                       // device time of the site probe's launches
  int n_bad_sites;                      // sites with a wrong result
  unsigned int bad_sites[16];           // the first 16 of them, packed (below)
  unsigned long long l2_errors;         // fabric check (fabric.hip): wrong words of the L2 march, unlocated included
  unsigned long long xcd_errors;        // wrong words of the cross-XCD exchange
  unsigned long long atomic_errors;     // wrong elements of the global-atomic tables
  double l2_gbps;                       // bytes the march read back / its device time (a lower bound)
  double fabric_ms;                     // device time of the fabric check's three launches
  int xccs_reached;                     // XCDs the march ran on
  int xcd_pairs_reached;                // (writer, reader) XCD pairs the exchange covered
  int xcd_pairs_unreached;              // xccs_reached^2 - pairs reached: reported, does not fail the run
};

struct amdgpu_canary_datapath_result {  // datapath.hip; no ctypes mirror
  double fp8_tflops;                // block-scaled fp8 (e4m3) MFMA, dense
  double fp4_tflops;                // block-scaled fp4 (e2m1) MFMA, dense
  unsigned long long lowp_errors;   // wrong accumulators over fp8 / bf8 / fp4 / unscaled fp8
  unsigned long long lds_errors;    // LDS march mismatches
  unsigned long long lds_bytes;     // LDS bytes per workgroup the march covered
};

int amdgpu_canary_datapaths(int device, int iters, amdgpu_canary_datapath_result* out, char* err, int err_len);
int amdgpu_canary_gemm_rate(int device, int M, int N, int K, int iters, int flags, int kernel, double* tflops,
                            unsigned long long* errors, char* err, int err_len);
// flags of amdgpu_canary_gemm_rate
constexpr int kGemmInject = 1, kGemmRandomData = 2, kGemmSkipVerifiedLaunch = 4;
// the ABFT verdict on a caller-supplied C (any positive M, N; 0 < K <= 65536): wrong rows, wrong columns
int amdgpu_canary_abft(int device, const unsigned short* a_host, const unsigned short* bt_host, const float* c_host,
                       int M, int N, int K, unsigned long long* row_errors, unsigned long long* col_errors, char* err,
                       int err_len);
// host only: the grid of GEMM kernel id `kernel` at M x N (0: refused) and each workgroup's tile origin
int amdgpu_canary_gemm_tile_map(int kernel, int M, int N, int* m0_out, int* n0_out, int len);

constexpr int kSiteChecks = 3;  // 0 mfma, 1 lowp, 2 valu

struct amdgpu_canary_site_slot {  // one per packed site
  unsigned int waves;             // waves that ran all three checks here
  unsigned int bad[kSiteChecks];  // wrong results they found, per check
};

struct amdgpu_canary_sites_result {
  unsigned long long errors[kSiteChecks];  // located wrong results per check
  unsigned long long unlocated_errors;     // wrong results of waves that changed site while checking
  unsigned long long waves;                // located waves
  unsigned long long moved;                // waves that changed site while checking
  int launches;
  int cus_reached;    // distinct (xcc, se, sh, cu) with a located wave
  int simds_reached;  // distinct sites with a located wave
  int cus_expected;   // multiProcessorCount
  int n_bad;          // sites with a wrong result
  unsigned int bad_sites[16];  // the first 16 of them, packed
  double ms;          // device time over all launches
};

int amdgpu_canary_sites(int device, int blocks, int ksteps, int inject_check, int inject_waves,
                        amdgpu_canary_site_slot* table_out, unsigned int* wave_site_out, int wave_site_len,
                        amdgpu_canary_sites_result* result, char* err, int err_len);
int amdgpu_canary_format_site(unsigned int site, char* buf, int len);  // "xcc3/se1/sh0/cu7/simd2"

// ---- fabric check (fabric.hip): per-XCD L2 march, cross-XCD exchange, global atomics ----
constexpr int kFabricXccs = 16;    // HW_REG_XCC_ID is 4 bits wide
constexpr int kAtomicOps = 14;     // order of canary.ATOMIC_OPS
constexpr int kAtomicElems = 2048; // elements of one operation's table

struct amdgpu_canary_xcc_slot {  // one per xcc: what the L2 march did there
  unsigned long long blocks;     // workgroups (= slices) that ran on it from first to last
  unsigned long long bytes;      // bytes of their slices
  unsigned long long bad;        // wrong 32-bit words they read back
};

struct amdgpu_canary_pair_slot {  // matrix[writer xcc][reader xcc] of the exchange
  unsigned long long reads;       // slices read
  unsigned long long bad;         // wrong 32-bit words in them
};

struct amdgpu_canary_fabric_result {
  unsigned long long l2_errors;         // wrong words of the march, unlocated ones included
  unsigned long long unlocated_errors;  // those of workgroups whose xcc changed while they ran
  unsigned long long xcd_errors;        // wrong words of the exchange
  unsigned long long atomic_errors;     // wrong table elements over all operations
  unsigned long long moved;             // workgroups (of either launch) whose xcc changed
  unsigned long long atomic_bad[kAtomicOps];
  unsigned long long march_read_bytes;  // bytes the march's read passes loaded
  int blocks;                           // the grid of all three launches
  int slice_kb;
  int xccs_reached;                     // xccs with a located march workgroup
  int pairs_reached;                    // non-empty cells of the pair matrix
  int pairs_expected;                   // xccs_reached squared
  int first_bad_slice;                  // first wrong word of the march: slice (-1: none),
  unsigned int first_bad_offset;        //   byte offset in it,
  int first_bad_xcc;                    //   and the xcc its workgroup started on
  int first_bad_op;                     // first wrong atomic element: operation (-1: none)
  int first_bad_elem;
  double march_ms;                      // device time of each launch
  double exchange_ms;
  double atomic_ms;
};

int amdgpu_canary_fabric(int device, int blocks, int slice_kb, int reps, int inject_kind, int inject_op,
                         int inject_blocks, amdgpu_canary_xcc_slot* xcc_table_out,
                         amdgpu_canary_pair_slot* pair_matrix_out, unsigned int* slice_xcc_out, int slice_xcc_len,
                         amdgpu_canary_fabric_result* result, char* err, int err_len);
int amdgpu_canary_atomic_expected(int op, int blocks, void* out, int out_bytes);
const char* amdgpu_canary_atomic_op_name(int op);  // "u64 add"
// "l2 check: 3 wrong words on xcc5 (slice 17, offset 0x1a40)" of the first failing check; 0 if none failed
int amdgpu_canary_fabric_describe(const amdgpu_canary_fabric_result* r, const amdgpu_canary_xcc_slot* xcc_table,
                                  const amdgpu_canary_pair_slot* pair_matrix, char* buf, int len);

// ---- CU memory check (cumem.hip): vector register file march, per-CU L1 march -----------
constexpr int kCuInjectKinds = 3;  // 0 vgpr, 1 agpr, 2 l1

struct amdgpu_canary_cu_slot {  // one per packed site
  unsigned int waves;           // reg_march waves that ran here from first to last
  unsigned int bad_vgpr;        // wrong words they read back from values pinned in VGPRs
  unsigned int bad_agpr;        //   ... and in AGPRs
  unsigned int bad_l1;          // wrong words l1_march waves here saw in a re-read pass
};

struct amdgpu_canary_cu_result {
  unsigned long long vgpr_errors;       // located wrong words of the register march
  unsigned long long agpr_errors;
  unsigned long long l1_errors;         // wrong words of the re-read passes, unlocated ones included
  unsigned long long l1_fill_errors;    // wrong words of pass 1 (from L2 / HBM: not an L1 verdict)
  unsigned long long unlocated_errors;  // wrong register words of waves that changed site while marching
  unsigned long long moved;             // reg_march waves that changed site
  unsigned long long waves;             // located reg_march waves
  unsigned long long l1_moved;          // l1_march waves that changed site (their errors stay in l1_errors)
  int launches;
  int cus_reached;     // distinct (xcc, se, sh, cu) with a located reg_march wave
  int simds_reached;   // distinct sites with one
  int cus_expected;    // multiProcessorCount
  int l1_cus_reached;  // distinct (xcc, se, sh, cu) whose L1 a located l1_march wave re-read
  int regs_vgpr;       // NV: values each lane keeps pinned in VGPRs
  int regs_agpr;       // NA: ... in AGPRs
  int n_bad;           // sites with a wrong word of any kind
  unsigned int bad_sites[16];  // the first 16 of them, packed
  double reg_ms;       // device time of the reg_march launches
  double l1_ms;        // device time of l1_fill and the l1_march launches
};

// wave_site_out, when not null, holds 2 * wave_site_len entries: the starting site of the
// first wave_site_len waves of the first reg_march launch, then those of the first l1_march.
int amdgpu_canary_cu(int device, int blocks, int reps, int l1_kb, int l1_reps, int inject_kind, int inject_waves,
                     amdgpu_canary_cu_slot* table_out, unsigned int* wave_site_out, int wave_site_len,
                     amdgpu_canary_cu_result* result, char* err, int err_len);
void amdgpu_canary_cu_regs(int* nv, int* na);
int amdgpu_canary_cu_sizeof(int which);  // 0: amdgpu_canary_cu_slot, 1: amdgpu_canary_cu_result
// "register check: 3 wrong words at xcc3/se1/sh0/cu7/simd2 (agpr; +1 more site)", else
// "l1 check: 2 wrong words at xcc3/se1/sh0/cu7"; 0 if neither failed.  `table`: kSiteSlots slots.
int amdgpu_canary_cu_describe(const amdgpu_canary_cu_result* r, const amdgpu_canary_cu_slot* table, char* buf,
                              int len);

}  // extern "C"

// The sizes canary.py's ctypes mirrors have (tests/test_canary_abi.py pins the same numbers).
static_assert(sizeof(amdgpu_canary_result) == 608, "canary.CanaryResult");
static_assert(sizeof(amdgpu_canary_datapath_result) == 40, "no mirror: five 8-byte fields");
static_assert(sizeof(amdgpu_canary_site_slot) == 16, "canary.SiteSlot");
static_assert(sizeof(amdgpu_canary_sites_result) == 144, "canary.SitesResult");
static_assert(sizeof(amdgpu_canary_xcc_slot) == 24, "canary.XccSlot");
static_assert(sizeof(amdgpu_canary_pair_slot) == 16, "canary.PairSlot");
static_assert(sizeof(amdgpu_canary_fabric_result) == 224, "canary.FabricResult");
static_assert(sizeof(amdgpu_canary_cu_slot) == 16, "canary.CuSlot");
static_assert(sizeof(amdgpu_canary_cu_result) == 176, "canary.CuResult");
