// MI355X (gfx950 / CDNA4) health canary: the bf16 matrix path.
//
// Three GEMMs on v_mfma_f32_*_bf16 (a plain one-wave-per-tile kernel for the numerics test,
// the LDS-staged 128x128 kernel, and the 256x256 ping-pong kernel with its measured
// variants, kernel ids 1-11 in kGemmVariants), the operand fills, and the ABFT row / column
// checksums that verify a whole product of exact integer data.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "canary_host.h"

namespace {

using namespace canary;

// Plain MFMA GEMM used by the numerics test: C[MxN] (fp32) = A[MxK] * B[KxN] (bf16,
// row-major).  One wave per 32x32 output tile, K stepped 16 at a time through
// v_mfma_f32_32x32x16_bf16 with the gfx950 operand maps: lane l (r = l&31, h = l>>5)
// feeds A[r][k0+8h+j] and B[k0+8h+j][r]; accumulator reg i of lane l is
// C[cd_row32(i, h)][l&31].  M, N multiples of 32, K multiple of 16 (host-checked).
__global__ void __launch_bounds__(64) mfma_gemm(const short* __restrict__ A, const short* __restrict__ B,
                                                float* __restrict__ C, int M, int N, int K) {
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int tm = blockIdx.y * 32, tn = blockIdx.x * 32;
  if (tm + 32 > M || tn + 32 > N) return;  // host checks shapes; never touch memory past them
  f32x16 acc = zero_f32x16();
  for (int k0 = 0; k0 < K; k0 += 16) {
    bf16x8 a, b;
    for (int j = 0; j < 8; ++j) {
      a[j] = A[static_cast<size_t>(tm + r) * K + k0 + 8 * h + j];
      b[j] = B[static_cast<size_t>(k0 + 8 * h + j) * N + tn + r];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  for (int i = 0; i < 16; ++i) {
    const int row = tm + cd_row32(i, h);
    C[static_cast<size_t>(row) * N + tn + r] = acc[i];
  }
}

// ---- LDS-staged MFMA GEMM: the matrix path a real workload takes --------------------
// C[MxN] (fp32) = A[MxK] * B, A row-major bf16, B given transposed (Bt[NxK] row-major,
// so both operands are K-contiguous).  A 128x128 block tile, BK = 64, 4 waves as 2x2,
// each wave 64x64 = 2x2 v_mfma_f32_32x32x16_bf16 tiles (64 accumulator registers).
// Operands stream HBM -> LDS with global_load_lds (16 B per lane, no VGPR round trip),
// double-buffered so tile t+1 lands while tile t is multiplied; fragments come out of
// LDS with one ds_read_b128 per operand per k-step.  Blocks are remapped XCD-aware so
// the tiles that share A rows share an XCD's L2.  Integer-valued operands make every
// result exact, so an ABFT row/column checksum (below) verifies the whole path - HBM,
// L2, the LDS DMA, LDS reads and the matrix cores - not just the MFMA unit.
constexpr int kTileM = 128, kTileN = 128, kTileK = 64;
constexpr int kTileBytes = kTileM * kTileK * 2;  // one operand tile, 16 KiB
typedef __attribute__((address_space(3))) void* lds_void_ptr;

// The index maps below are host + device: the kernels pass blockIdx.x and gridDim.x, and
// amdgpu_canary_gemm_tile_map walks the same arithmetic on the host (tests/test_canary_gemm.py
// checks that every grid is a permutation of its tile set).
__host__ __device__ __forceinline__ int xcd_remap(int orig, int nwg) {  // bijective for any nwg
  const int xcd = orig % 8, q = nwg / 8, r = nwg % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// Output tile of workgroup `block` of `nblocks` in gemm_lds: XCD-aware remap, then row-major tiles.
__host__ __device__ __forceinline__ void tile_origin128(int block, int nblocks, int M, int N, int* m0, int* n0) {
  const int nbn = N / kTileN;
  const int wg = xcd_remap(block, nblocks);
  *m0 = (wg / nbn) * kTileM;
  *n0 = (wg % nbn) * kTileN;
}

// An operand tile in LDS is [rows][64] bf16: 128 B rows of eight 16 B chunks.  The 16 lanes of
// one ds_read_b128 cycle (rows r..r+15, same k chunk) would hit 2 of the 16 bank slots of a
// 256 B bank row (8-way conflict), so the image is swizzled: logical chunk `chunk` of row `row`
// sits at this physical chunk.  Row parity picks the 128 B half of the bank row and
// (row >> 1) & 7 the slot in it, so 16 consecutive rows cover all 16 slots (conflict-free, for
// the 16x16x32 lane groups too; `chunk ^ (row & 7)` measured 2-way, SQ_LDS_BANK_CONFLICT).
__device__ __forceinline__ int swizzled_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// The 8 k values of logical chunk `chunk` of row `row` of tile image S: one ds_read_b128.
__device__ __forceinline__ bf16x8 frag(const short* S, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(S + row * kTileK + (swizzled_chunk(row, chunk) << 3));
}

// Piece p of an operand tile: rows 8p .. 8p+7 (1 KiB) of the tile whose first row is r0 and
// first k is k0, from HBM straight into the image at `base`.  Lane l lands at physical chunk
// l & 7 of row l >> 3 (the glds destination must stay lane-linear), so the swizzle is applied
// on its global source address.
__device__ __forceinline__ void glds_piece(const short* src, int r0, int K, int k0, char* base, int p, int lane) {
  const int row = p * 8 + (lane >> 3), kc = swizzled_chunk(row, lane & 7) * 8;
  __builtin_amdgcn_global_load_lds(src + static_cast<size_t>(r0 + row) * K + k0 + kc, (lds_void_ptr)(base + p * 1024),
                                   16, 0, 0);
}

__global__ void __launch_bounds__(256) gemm_lds(const short* __restrict__ A, const short* __restrict__ Bt,
                                               float* __restrict__ C, int M, int N, int K) {
  // one __shared__ array for everything (a second object can de-pipeline glds waits)
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * kTileBytes];  // [buf][A|B][128][64] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int m0, n0;
  tile_origin128(blockIdx.x, gridDim.x, M, N, &m0, &n0);
  if (m0 + kTileM > M || n0 + kTileN > N) return;  // host checks shapes
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  // Wave w issues pieces 4w .. 4w+3 of A and of B.  This is glds_piece written out, here and in
  // gemm256: with the call in this loop the compiler allocates both kernels' registers differently.
  auto stage = [&](int t, int buf) {
    const int k0 = t * kTileK;
    char* base = smem + buf * 2 * kTileBytes;
    for (int i = 0; i < 4; ++i) {
      const int row = (wave * 4 + i) * 8 + (lane >> 3), kc = ((lane & 7) ^ ((row >> 1) & 7)) * 8;
      __builtin_amdgcn_global_load_lds(A + static_cast<size_t>(m0 + row) * K + k0 + kc,
                                       (lds_void_ptr)(base + (wave * 4 + i) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bt + static_cast<size_t>(n0 + row) * K + k0 + kc,
                                       (lds_void_ptr)(base + kTileBytes + (wave * 4 + i) * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = zero_f32x16();

  const int T = K / kTileK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    if (t + 1 < T) stage(t + 1, cur ^ 1);
    const short* As = reinterpret_cast<const short*>(smem + cur * 2 * kTileBytes);
    const short* Bs = As + kTileM * kTileK;
#pragma unroll
    for (int kk = 0; kk < kTileK / 16; ++kk) {
      const int chunk = 2 * kk + h;  // logical 16 B chunk of this lane's 8 k values
      bf16x8 a[2], b[2];
      for (int i = 0; i < 2; ++i) a[i] = frag(As, wr * 64 + i * 32 + r, chunk);
      for (int j = 0; j < 2; ++j) b[j] = frag(Bs, wc * 64 + j * 32 + r, chunk);
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 has landed
    __syncthreads();                                   // ... and nobody still reads tile t's buffer
  }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j)
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;  // cd_row32, in this order of sums
        C[static_cast<size_t>(row) * N + n0 + wc * 64 + j * 32 + r] = acc[i][j][e];
      }
}

// ---- 256x256-tile GEMM, two wave groups in ping-pong: the fast matrix path ------------
// Same contract as gemm_lds (A [MxK], Bt [NxK] bf16, fp32 C), M, N % 256 == 0, K % 64 == 0.
// 8 waves = 2 groups (wr) x 4 (wc); a wave owns 128x64 of C as 2 halves x 4x4 tiles of
// v_mfma_f32_16x16x32_bf16 (128 accumulator registers).  Per K-tile (BK = 64) a wave runs
// four sections, each closed by a raw s_barrier:
//   L0: ds_read A half 0 + all of B (16 x b128)   M0: 32 MFMA into half 0
//   L1: ds_read A half 1 (8 x b128)               M1: 32 MFMA into half 1
// Group 1 executes one extra barrier first, so it runs one barrier interval behind group
// 0.  Waves w and w+4 share a SIMD, hence on every SIMD one wave is in an MFMA section
// while its partner reads LDS: the MFMA pipe does not wait for fragment loads.
// Operands stream in with global_load_lds into 2 LDS buffers (2 x 64 KiB, 1 block/CU).
// Interval i (between barriers i and i+1) holds group 0's section i and group 1's
// section i-1.  Tile t lives in buffer t&1 and is read in intervals 4t..4t+3; tile t+2
// is issued by both groups in interval 4t+4 (right after the barrier that ends the last
// read of tile t) and each wave retires its own copies with s_waitcnt vmcnt(0) before
// barrier 4t+8, which precedes the first read of tile t+2.  The DMA therefore stays in
// flight across three barriers (__syncthreads would drain it at each: vmcnt(0)).
// Write-after-read is covered by every reading section ending in lgkmcnt(0) before its
// barrier.  The LDS image is gemm_lds's (swizzled_chunk).  Tiles are rastered in groups of 4
// tile rows, so one XCD's consecutive workgroups share 4 A panels and a run of B panels in
// their L2.
constexpr int kBT = 256, kBK = kTileK;  // the same 128 B LDS rows, so frag and glds_piece serve here too
constexpr int kBOp = kBT * kBK * 2;     // one operand tile, 32 KiB
constexpr int kBStage = 2 * kBOp;       // A + B of one K-tile, 64 KiB
constexpr int kGroupM256 = 4;           // tile rows per raster group
using f32x4 = __attribute__((ext_vector_type(4))) float;

// Output tile of workgroup `block` of `nblocks`: XCD-aware bijective remap, then tiles rastered
// in groups of `group` tile rows so one XCD's consecutive workgroups share A and B panels in L2.
__host__ __device__ __forceinline__ void tile_origin256(int block, int nblocks, int M, int N, int group, int* m0,
                                                        int* n0) {
  const int nbm = M / kBT, nbn = N / kBT;
  const int wg = xcd_remap(block, nblocks);
  const int per_group = group * nbn, first_m = (wg / per_group) * group;
  const int gm = nbm - first_m < group ? nbm - first_m : group;
  *m0 = (first_m + (wg % per_group) % gm) * kBT;
  *n0 = ((wg % per_group) / gm) * kBT;
}

__device__ __forceinline__ void section_end() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this section's LDS reads are done
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);  // nothing crosses a section boundary
}

// The parts gemm256 and gemm256s share.  Their L sections (the frag loops) stay written out in
// both kernels, and so does gemm256's M0: as calls they change the kernels' register allocation.
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[2][4][4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// An M section: 32 MFMA into one half's 4x4 tiles, under raised wave priority when kPrio.
template <bool kPrio>
__device__ __forceinline__ void mfma_section(f32x4 (&acc)[4][4], const bf16x8 (&a)[4][2], const bf16x8 (&b)[4][2]) {
  if constexpr (kPrio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
  if constexpr (kPrio) __builtin_amdgcn_s_setprio(0);
}

__global__ void __launch_bounds__(512) gemm256(const short* __restrict__ A, const short* __restrict__ Bt,
                                              float* __restrict__ C, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kBStage];  // the only LDS object
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int m0, n0;
  tile_origin256(blockIdx.x, gridDim.x, M, N, kGroupM256, &m0, &n0);
  if (m0 + kBT > M || n0 + kBT > N) return;  // host checks shapes (block-uniform exit)
  const int wr = wave >> 2, wc = wave & 3;
  const bool g1 = wr == 1;
  const int r16 = lane & 15, q = lane >> 4;

  auto stage = [&](int t) {  // pieces 4w .. 4w+3 of A and of B per wave, written out as in gemm_lds
    const int k0 = t * kBK;
    char* base = smem + (t & 1) * kBStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (wave * 4 + i) * 8 + (lane >> 3), kc = ((lane & 7) ^ ((row >> 1) & 7)) * 8;
      __builtin_amdgcn_global_load_lds(A + static_cast<size_t>(m0 + row) * K + k0 + kc,
                                       (lds_void_ptr)(base + (wave * 4 + i) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bt + static_cast<size_t>(n0 + row) * K + k0 + kc,
                                       (lds_void_ptr)(base + kBOp + (wave * 4 + i) * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[2][4][4];
  zero_acc(acc);
  bf16x8 a[4][2], b[4][2];

  const int T = K / kBK;
  stage(0);
  if (T > 1) {
    stage(1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile 0 landed; tile 1 may fly on
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  section_end();
  if (g1) section_end();  // the one-interval stagger

  for (int t = 0; t < T; ++t) {
    const short* As = reinterpret_cast<const short*>(smem + (t & 1) * kBStage);
    const short* Bs = As + kBT * kBK;
    // L0
    if (!g1 && t >= 1 && t + 1 < T) stage(t + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j][s] = frag(Bs, wc * 64 + j * 16 + r16, 4 * s + q);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i][s] = frag(As, wr * 128 + i * 16 + r16, 4 * s + q);
    section_end();
    // M0: mfma_section<true>(acc[0], a, b), written out
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[0][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][s], b[j][s], acc[0][i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    section_end();
    // L1
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i][s] = frag(As, wr * 128 + 64 + i * 16 + r16, 4 * s + q);
    if (g1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 (issued in interval 4t)
    section_end();
    // M1
    if (g1 && t + 2 < T) stage(t + 2);
    mfma_section<true>(acc[1], a, b);
    if (!g1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 (issued in interval 4t)
    section_end();
  }
  if (!g1) section_end();  // both groups pass the same number of barriers

#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = m0 + wr * 128 + h * 64 + i * 16 + q * 4 + e;
          C[static_cast<size_t>(row) * N + n0 + wc * 64 + j * 16 + r16] = acc[h][i][j][e];
        }
}

// ---- gemm256 with region-wise staging: the DMA issued from LDS-read sections ----------
// gemm256 issues all eight 1 KiB pieces of a wave in one section, and a piece costs
// ~60-185 issue cycles (MI355X_MICROARCH.md, LDS-DMA piece row), so that section runs
// about twice as long as the others.  Here a tile's regions are refilled as soon as they
// are free: B and the A rows every wave reads in L0 ("A-h0": rows 0-63 and 128-191) are
// last read in interval 4t+1, so their refill for tile t+2 (6 pieces per wave) is issued
// in L(t,1); the A-h1 rows are last read in interval 4t+3, so theirs (2 pieces) is issued
// in L(t+1,0).  All DMA sits in L sections (which are shorter than the partner wave's
// MFMA section), and a tile is retired with vmcnt(6) before barrier 4t+8: the next
// tile's six younger pieces stay in flight.  Measured (4096^3 / 8192^3, integer data):
// 1254-1264 / 1308-1314 TFLOP/s vs gemm256's 1069-1084 / 1078-1090.
// kBEarly of a wave's 4 B pieces of tile t+2 go with its A-h0 pieces in L(t,1), the rest
// with the A-h1 pieces in L(t+1,0): the split balances DMA issue between the two L
// sections (L0 also carries twice L1's ds_reads).
// kG1Early: group 1 issues each refill from the MFMA section one interval earlier (the
// first interval its region is free) instead of from its next LDS-read section.
// kScalarWave: the wave index goes through readfirstlane, so everything derived from it
// (LDS piece addresses -> M0, group branches) is scalar instead of per-lane.
// kGroupM: tile rows per raster group; kPrio: raise wave priority around MFMA sections.
template <int kBEarly, bool kG1Early = false, bool kScalarWave = true, int kGroupM = kGroupM256, bool kPrio = true>
__global__ void __launch_bounds__(512) gemm256s(const short* __restrict__ A, const short* __restrict__ Bt,
                                               float* __restrict__ C, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kBStage];  // the only LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = kScalarWave ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  int m0, n0;
  tile_origin256(blockIdx.x, gridDim.x, M, N, kGroupM, &m0, &n0);
  if (m0 + kBT > M || n0 + kBT > N) return;  // host checks shapes (block-uniform exit)
  const int wr = wave >> 2, wc = wave & 3;
  const bool g1 = wr == 1;
  const int r16 = lane & 15, q = lane >> 4;

  // A-h0 pieces are 0-7 and 16-23, A-h1 pieces 8-15 and 24-31; wave w owns list entries 2w, 2w+1
  auto a_piece = [](int k, int half) { return (k < 8 ? k : k + 8) + 8 * half; };
  auto stage_b_ah0 = [&](int t) {  // kBEarly B + 2 A-h0 pieces
    char* base = smem + (t & 1) * kBStage;
#pragma unroll
    for (int i = 0; i < kBEarly; ++i) glds_piece(Bt, n0, K, t * kBK, base + kBOp, wave * 4 + i, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) glds_piece(A, m0, K, t * kBK, base, a_piece(wave * 2 + i, 0), lane);
  };
  auto stage_ah1 = [&](int t) {  // 4 - kBEarly B + 2 A-h1 pieces
    char* base = smem + (t & 1) * kBStage;
#pragma unroll
    for (int i = kBEarly; i < 4; ++i) glds_piece(Bt, n0, K, t * kBK, base + kBOp, wave * 4 + i, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) glds_piece(A, m0, K, t * kBK, base, a_piece(wave * 2 + i, 1), lane);
  };
  auto retire = [&](int t) {  // tile t+1 landed; tile t+2's 2 + kBEarly pieces may fly on
    if (t + 2 >= K / kBK)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + kBEarly) : "memory");
  };

  f32x4 acc[2][4][4];
  zero_acc(acc);
  bf16x8 a[4][2], b[4][2];

  const int T = K / kBK;
  stage_b_ah0(0);
  stage_ah1(0);
  if (T > 1) {
    stage_b_ah0(1);
    stage_ah1(1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile 0 landed; tile 1 may fly on
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  section_end();
  if (g1) section_end();  // the one-interval stagger

  for (int t = 0; t < T; ++t) {
    const short* As = reinterpret_cast<const short*>(smem + (t & 1) * kBStage);
    const short* Bs = As + kBT * kBK;
    // L0
    if ((!kG1Early || !g1) && t >= 1 && t + 1 < T) stage_ah1(t + 1);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j][s2] = frag(Bs, wc * 64 + j * 16 + r16, 4 * s2 + q);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i][s2] = frag(As, wr * 128 + i * 16 + r16, 4 * s2 + q);
    section_end();
    // M0
    if (kG1Early && g1 && t + 2 < T) stage_b_ah0(t + 2);
    mfma_section<kPrio>(acc[0], a, b);
    section_end();
    // L1
    if ((!kG1Early || !g1) && t + 2 < T) stage_b_ah0(t + 2);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i][s2] = frag(As, wr * 128 + 64 + i * 16 + r16, 4 * s2 + q);
    if (g1) retire(t);
    section_end();
    // M1
    if (kG1Early && g1 && t + 2 < T) stage_ah1(t + 2);
    mfma_section<kPrio>(acc[1], a, b);
    if (!g1) retire(t);
    section_end();
  }
  if (!g1) section_end();  // both groups pass the same number of barriers

  // Epilogue through LDS: after the last barrier no wave reads a staging buffer and no DMA
  // is in flight, so each wave turns its 64x64 fp32 half-outputs into whole rows in a
  // 16 KiB region of its own (8 x 16 KiB = the whole 128 KiB; 256 B rows: a ds_write_b32
  // is 2-way, which costs nothing on that instruction, and the b128 read-back is
  // conflict-free) and stores them with dwordx4: 16 row-contiguous stores of 4 rows x
  // 256 B per half instead of 64 column-scattered dword stores.
  static_assert(8 * 64 * 64 * 4 <= 2 * kBStage, "epilogue regions fit the staging LDS");
  float* region = reinterpret_cast<float*>(smem + wave * (64 * 64 * 4));
  constexpr int kLd = 64;  // floats per row
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) region[(i * 16 + q * 4 + e) * kLd + j * 16 + r16] = acc[h][i][j][e];
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int row = p * 4 + (lane >> 4), c4 = (lane & 15) * 4;
      const float4 v = *reinterpret_cast<const float4*>(region + row * kLd + c4);
      *reinterpret_cast<float4*>(C + static_cast<size_t>(m0 + wr * 128 + h * 64 + row) * N + n0 + wc * 64 + c4) = v;
    }
  }
}

// Integer operands in [-4, 4] (exact in bf16): element (i, k) of operand `which`.
__global__ void __launch_bounds__(256) gemm_fill(short* __restrict__ X, int rows, int K, uint32_t which) {
  const size_t n = static_cast<size_t>(rows) * K;
  for (size_t e = blockIdx.x * 256ull + threadIdx.x; e < n; e += static_cast<size_t>(gridDim.x) * 256)
    X[e] = bf16_of_int(small_int((static_cast<uint64_t>(which) << 56) ^ e));
}

// Uniform random bf16 in [-1, 1) (rate measurement on data with full mantissas: the
// clock the chip holds under MFMA load depends on operand bit activity).
__global__ void __launch_bounds__(256) gemm_fill_random(short* __restrict__ X, int rows, int K, uint32_t which) {
  const size_t n = static_cast<size_t>(rows) * K;
  for (size_t e = blockIdx.x * 256ull + threadIdx.x; e < n; e += static_cast<size_t>(gridDim.x) * 256) {
    const float f = static_cast<float>(mix32((static_cast<uint64_t>(which) << 56) ^ e) >> 8) * (2.0f / 16777216.0f) - 1.0f;
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    X[e] = static_cast<short>(u >> 16);
  }
}

__device__ __forceinline__ int bf16_to_int(short v) {
  const uint32_t u = static_cast<uint32_t>(static_cast<uint16_t>(v)) << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return static_cast<int>(f);
}

// colsum[k] += sum over a 64-row slab of X[row][k]: threads over k (coalesced), blocks
// over (k range, row slab) so the whole chip takes part; out must be zeroed.  Two's-
// complement wrap-around makes the unsigned atomic add a signed one.
constexpr int kSlab = 64;
__global__ void __launch_bounds__(256) gemm_colsum(const short* __restrict__ X, int rows, int K,
                                                   long long* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int r0 = blockIdx.y * kSlab, r1 = r0 + kSlab < rows ? r0 + kSlab : rows;
  long long s = 0;
  for (int i = r0; i < r1; ++i) s += bf16_to_int(X[static_cast<size_t>(i) * K + k]);
  atomicAdd(reinterpret_cast<unsigned long long*>(out + k), static_cast<unsigned long long>(s));
}

// An element of a healthy product is an integer of magnitude <= 2^24 and never -0: the
// accumulators start at +0, and under round-to-nearest +0 + -0 and a + -a both give +0.
// Decided on the bit pattern, so NaN, Inf and denormals need no floating-point compare and a
// fraction below the units place cannot hide behind the cast to an integer.
__device__ __forceinline__ bool abft_healthy(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  const uint32_t mag = u & 0x7fffffffu;
  if (mag == 0) return u == 0;                        // +0, not -0
  if (mag < 0x3f800000u || mag > 0x4b800000u) return false;  // 0 < |v| < 1; |v| > 2^24, Inf, NaN
  const int frac_bits = 150 - static_cast<int>(mag >> 23);  // mantissa bits below the units place
  return frac_bits <= 0 || (mag & ((1u << frac_bits) - 1u)) == 0;
}

// ABFT: for row i, sum_n C[i][n] must equal sum_k A[i][k] * (sum_n Bt[n][k]); for column
// n, sum_m C[m][n] must equal sum_k (sum_m A[m][k]) * Bt[n][k].  One block per row /
// column, int64 reductions (C holds exact integers).  mode 0 = rows, 1 = columns; a row or
// column is wrong when its checksum is off or it holds an element that is not healthy
// (those stay out of the sum), and adds 1 to errors[mode].
__global__ void __launch_bounds__(256) gemm_abft(const short* __restrict__ X, const float* __restrict__ C,
                                                 const long long* __restrict__ other_sum, int M, int N, int K,
                                                 int mode, unsigned long long* __restrict__ errors) {
  __shared__ long long red[3][256];
  const int idx = blockIdx.x, tid = threadIdx.x;
  long long expect = 0, got = 0, bad = 0;
  for (int k = tid; k < K; k += 256) expect += static_cast<long long>(bf16_to_int(X[static_cast<size_t>(idx) * K + k])) * other_sum[k];
  const int n_el = mode == 0 ? N : M;
  for (int e = tid; e < n_el; e += 256) {
    const float v = mode == 0 ? C[static_cast<size_t>(idx) * N + e] : C[static_cast<size_t>(e) * N + idx];
    if (abft_healthy(v))
      got += static_cast<long long>(v);
    else
      ++bad;
  }
  red[0][tid] = expect;
  red[1][tid] = got;
  red[2][tid] = bad;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0 && (red[0][0] != red[1][0] || red[2][0] != 0)) atomicAdd(errors + mode, 1ull);
}

// What a GEMM kernel id means: the edge of its square output tiles (one workgroup each), the tile
// rows per raster group (0: gemm_lds rasters row-major), its block size and the kernel.
using gemm_fn = void (*)(const short*, const short*, float*, int, int, int);
struct GemmVariant {
  int tile, group, threads;
  gemm_fn kernel;
};
template <int kBEarly, bool kG1Early = false, bool kScalarWave = true, int kGroupM = kGroupM256, bool kPrio = true>
constexpr GemmVariant staged = {kBT, kGroupM, 512, gemm256s<kBEarly, kG1Early, kScalarWave, kGroupM, kPrio>};

constexpr GemmVariant kGemmVariants[] = {
    {},                                  // 0 is no kernel: pick_gemm's own choice
    {kTileM, 0, 256, gemm_lds},          // 1 128x128 tiles
    {kBT, kGroupM256, 512, gemm256},     // 2 256x256 tiles, wave-group ping-pong, whole-tile DMA
    staged<4>,                           // 3 region-wise DMA from the LDS-read sections
    staged<2>,                           // 4 ... 2 of a wave's 4 B pieces early
    staged<0>,                           // 5 ... none
    staged<3>,                           // 6 ... 3
    staged<4, true>,                     // 7 group 1 refills from its MFMA sections
    staged<4, false, false>,             // 8 per-lane wave index
    staged<4, false, true, 2>,           // 9 raster groups of 2 tile rows
    staged<4, false, true, 8>,           // 10 ... of 8
    staged<4, false, true, 4, false>,    // 11 no wave priority around MFMA sections
};
constexpr int kGemmVariantCount = sizeof(kGemmVariants) / sizeof(kGemmVariants[0]);

// GEMM kernel choice: `kernel` itself if it is an id of kGemmVariants whose tiles divide the
// shape; for 0, gemm256s (3) when the shape divides into 256x256 tiles and gives at least 256
// of them (one per CU), else gemm_lds (1).  Returns 0 for a shape the kernel cannot take.
int pick_gemm(int M, int N, int K, int kernel) {
  if (M <= 0 || N <= 0 || K <= 0 || K % kTileK || kernel < 0 || kernel >= kGemmVariantCount) return 0;
  const auto fits = [&](int id) { return M % kGemmVariants[id].tile == 0 && N % kGemmVariants[id].tile == 0; };
  if (kernel != 0) return fits(kernel) ? kernel : 0;
  if (fits(3) && (M / kBT) * (N / kBT) >= 256) return 3;
  return fits(1) ? 1 : 0;
}

void launch_gemm(int kind, const short* a, const short* b, float* c, int M, int N, int K) {
  const GemmVariant& v = kGemmVariants[kind];
  hipLaunchKernelGGL(v.kernel, dim3((M / v.tile) * (N / v.tile)), dim3(v.threads), 0, 0, a, b, c, M, N, K);
}

// The numerics tests' path: operands from host memory, `launch(a, b, c)` on them, C back to the host.
template <typename Launch>
int gemm_on_host_data(int device, const unsigned short* a_host, size_t a_bytes, const unsigned short* b_host,
                      size_t b_bytes, float* c_host, size_t c_bytes, char* err, int err_len, Launch&& launch) {
  Status st;
  DeviceBuffer<short> a, b;
  DeviceBuffer<float> c;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, a.alloc(a_bytes));
  CANARY_HIP(st, b.alloc(b_bytes));
  CANARY_HIP(st, c.alloc(c_bytes));
  CANARY_HIP(st, a.upload(a_host));
  CANARY_HIP(st, b.upload(b_host));
  if (st.ok()) {
    launch(a.get(), b.get(), c.get());
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, c.download(c_host));
  return st.report("", err, err_len);
}

// Owns the device side of one ABFT-verified product: A [MxK], Bt [NxK], C [MxN], the K column
// sums of A and of Bt, and the two counters (wrong rows, wrong columns).
class AbftProduct {
 public:
  DeviceBuffer<short> a, b;
  DeviceBuffer<float> c;

  // selects the device; the counters start at zero
  void alloc(Status& st, int device, int M, int N, int K) {
    CANARY_HIP(st, hipSetDevice(device));
    CANARY_HIP(st, a.alloc(static_cast<size_t>(M) * K * 2));
    CANARY_HIP(st, b.alloc(static_cast<size_t>(N) * K * 2));
    CANARY_HIP(st, c.alloc(static_cast<size_t>(M) * N * 4));
    CANARY_HIP(st, asum_.alloc(static_cast<size_t>(K) * 8));
    CANARY_HIP(st, bsum_.alloc(static_cast<size_t>(K) * 8));
    CANARY_HIP(st, counts_.alloc(2 * sizeof(unsigned long long)));
    CANARY_HIP(st, counts_.zero());
  }
  // The checksum sequence: the column sums of A and of Bt, then the row and the column verdicts
  // on C, added to the counters.  Shape-generic: any positive M, N, K.
  void verify(Status& st, int M, int N, int K) {
    CANARY_HIP(st, asum_.zero());
    CANARY_HIP(st, bsum_.zero());
    if (!st.ok()) return;
    const int kb = (K + 255) / 256;
    hipLaunchKernelGGL(gemm_colsum, dim3(kb, (M + kSlab - 1) / kSlab), dim3(256), 0, 0, a.get(), M, K, asum_.get());
    hipLaunchKernelGGL(gemm_colsum, dim3(kb, (N + kSlab - 1) / kSlab), dim3(256), 0, 0, b.get(), N, K, bsum_.get());
    hipLaunchKernelGGL(gemm_abft, dim3(M), dim3(256), 0, 0, a.get(), c.get(), bsum_.get(), M, N, K, 0, counts_.get());
    hipLaunchKernelGGL(gemm_abft, dim3(N), dim3(256), 0, 0, b.get(), c.get(), asum_.get(), M, N, K, 1, counts_.get());
    st.check(hipGetLastError());
  }
  // waits for the device; counts = {wrong rows, wrong columns}
  void finish(Status& st, unsigned long long (&counts)[2]) {
    CANARY_HIP(st, hipDeviceSynchronize());
    CANARY_HIP(st, counts_.download(counts));
  }

 private:
  DeviceBuffer<long long> asum_, bsum_;
  DeviceBuffer<unsigned long long> counts_;
};

}  // namespace

extern "C" {

// Tile origin of every workgroup of kernel id `kernel` at shape M x N, on the host (no GPU
// needed): returns the grid size and fills the first min(len, grid) entries of m0_out / n0_out
// with the kernel's own index arithmetic; 0 if pick_gemm refuses the shape or the id.
int amdgpu_canary_gemm_tile_map(int kernel, int M, int N, int* m0_out, int* n0_out, int len) {
  const int kind = pick_gemm(M, N, kTileK, kernel);
  if (kind == 0) return 0;
  const GemmVariant& v = kGemmVariants[kind];
  const int grid = (M / v.tile) * (N / v.tile);
  for (int b = 0; b < grid && b < len; ++b) {
    if (v.tile == kTileM)
      tile_origin128(b, grid, M, N, &m0_out[b], &n0_out[b]);
    else
      tile_origin256(b, grid, M, N, v.group, &m0_out[b], &n0_out[b]);
  }
  return grid;
}

// The ABFT verdict on a caller-supplied C: uploads A [MxK], Bt [NxK] (bf16 bit patterns) and
// C [MxN], runs the checksum sequence and returns the wrong rows and the wrong columns.
int amdgpu_canary_abft(int device, const unsigned short* a_host, const unsigned short* bt_host, const float* c_host,
                       int M, int N, int K, unsigned long long* row_errors, unsigned long long* col_errors, char* err,
                       int err_len) {
  *row_errors = 0;
  *col_errors = 0;
  if (M <= 0 || N <= 0 || K <= 0 || K > 65536) {
    std::snprintf(err, err_len, "abft shape (%d,%d,%d) must be positive with K <= 65536", M, N, K);
    return -1;
  }
  Status st;
  AbftProduct p;
  unsigned long long counts[2] = {0, 0};
  p.alloc(st, device, M, N, K);
  CANARY_HIP(st, p.a.upload(a_host));
  CANARY_HIP(st, p.b.upload(bt_host));
  CANARY_HIP(st, p.c.upload(c_host));
  p.verify(st, M, N, K);
  p.finish(st, counts);
  *row_errors = counts[0];
  *col_errors = counts[1];
  return st.report("", err, err_len);
}

// Host wrapper for the numerics test: inputs/outputs in host memory.
int amdgpu_canary_mfma_gemm(int device, const unsigned short* a_host, const unsigned short* b_host, float* c_host,
                            int M, int N, int K, char* err, int err_len) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 32 || N % 32 || K % 16) {
    std::snprintf(err, err_len, "shape (%d,%d,%d) must be M,N %% 32 == 0 and K %% 16 == 0", M, N, K);
    return -1;
  }
  return gemm_on_host_data(device, a_host, static_cast<size_t>(M) * K * 2, b_host, static_cast<size_t>(K) * N * 2,
                           c_host, static_cast<size_t>(M) * N * 4, err, err_len,
                           [&](const short* a, const short* b, float* c) {
                             hipLaunchKernelGGL(mfma_gemm, dim3(N / 32, M / 32), dim3(64), 0, 0, a, b, c, M, N, K);
                           });
}

// LDS-staged GEMM on host data (numerics test): A [MxK], Bt [NxK] bf16 row-major.
int amdgpu_canary_gemm(int device, const unsigned short* a_host, const unsigned short* bt_host, float* c_host, int M,
                       int N, int K, int kernel, char* err, int err_len) {
  const int kind = pick_gemm(M, N, K, kernel);
  if (kind == 0) {
    std::snprintf(err, err_len, "shape (%d,%d,%d) does not fit kernel %d (M,N %% 128 or 256, K %% 64)", M, N, K,
                  kernel);
    return -1;
  }
  return gemm_on_host_data(device, a_host, static_cast<size_t>(M) * K * 2, bt_host, static_cast<size_t>(N) * K * 2,
                           c_host, static_cast<size_t>(M) * N * 4, err, err_len,
                           [&](const short* a, const short* b, float* c) { launch_gemm(kind, a, b, c, M, N, K); });
}

// Matrix-path canary: device-generated integer operands, `iters` timed GEMMs, then C is
// poisoned (every byte 0xFF: NaN) and one more, untimed GEMM writes the product that the ABFT
// row + column checksums verify, so a tile a launch leaves unwritten cannot hide behind an
// earlier launch's data.  *tflops = dense bf16 rate achieved, *errors = wrong rows + wrong
// columns (0 on a healthy partition).
// flags bit 0 corrupts one element of C before the check (verifier self-test); bit 1
// fills the operands with random bf16 in [-1, 1) instead and skips the (then inexact)
// checksums: the rate on full-mantissa data, comparable with a BLAS benchmark; bit 2 skips
// the launch after the poison, so every row and every column must be reported (M + N).
int amdgpu_canary_gemm_rate(int device, int M, int N, int K, int iters, int flags, int kernel, double* tflops,
                            unsigned long long* errors, char* err, int err_len) {
  const bool inject = flags & kGemmInject, random_data = flags & kGemmRandomData,
             skip_verified_launch = flags & kGemmSkipVerifiedLaunch;
  *tflops = 0;
  *errors = 0;
  const int kind = pick_gemm(M, N, K, kernel);
  if (kind == 0 || K > 65536 || iters < 1) {
    std::snprintf(err, err_len,
                  "shape (%d,%d,%d) x %d iters does not fit kernel %d (M,N %% 128 or 256, K %% 64, K <= 65536, "
                  "iters >= 1)",
                  M, N, K, iters, kernel);
    return -1;
  }
  Status st;
  AbftProduct p;
  Events<2> ev;
  float ms[1] = {0};
  unsigned long long counts[2] = {0, 0};
  p.alloc(st, device, M, N, K);
  CANARY_HIP(st, ev.create());
  const auto launch = [&] { launch_gemm(kind, p.a.get(), p.b.get(), p.c.get(), M, N, K); };
  if (st.ok()) {
    const auto fill = random_data ? gemm_fill_random : gemm_fill;
    hipLaunchKernelGGL(fill, dim3(2048), dim3(256), 0, 0, p.a.get(), M, K, 1u);
    hipLaunchKernelGGL(fill, dim3(2048), dim3(256), 0, 0, p.b.get(), N, K, 2u);
    launch();  // warm-up
    st.check(hipGetLastError());
  }
  time_stages(st, ev, ms, [&](int) {
    for (int i = 0; i < iters; ++i) launch();
    return hipSuccess;
  });
  if (!random_data) {
    CANARY_HIP(st, p.c.fill(0xFF));  // the poison: what is verified below was written after it
    if (st.ok() && !skip_verified_launch) {
      launch();
      st.check(hipGetLastError());
    }
  }
  if (inject) {
    const float junk = 12345.0f;
    CANARY_HIP(st, hipMemcpy(p.c.get() + static_cast<size_t>(M / 2) * N + N / 3, &junk, 4, hipMemcpyHostToDevice));
  }
  if (!random_data) p.verify(st, M, N, K);
  p.finish(st, counts);
  *errors = counts[0] + counts[1];
  if (st.ok() && ms[0] > 0) *tflops = 2.0 * M * N * K * iters / (ms[0] * 1e-3) / 1e12;
  return st.report("", err, err_len);
}

}  // extern "C"
