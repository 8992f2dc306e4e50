// MI355X (gfx950 / CDNA4) health canary: the LDS-path check.
//
// The data path beside the ALUs of every CU: the LDS at every access width, its atomic units,
// the LDS-DMA fill, the transposed read, and the lane-crossing networks (the LDS crossbar behind
// ds_bpermute / ds_permute / ds_swizzle, the DPP row and bank network, v_permlane*_swap, the
// lane <-> scalar moves).  The shape is the site probe's and the pace check's: 4-wave
// workgroups (one wave per SIMD), one resident per CU through the largest dynamic LDS
// allocation, every wave reading its site (canary_common.h) first and last, and lane 0 of
// every wave leaving one record (ldspath_host.h) in its own slot, records[block * 4 + wave],
// with ordinary vector stores.  No kernel reads a record, no workgroup waits for another,
// every loop is bounded by an argument or a constant, and fault injection perturbs a value
// that is then compared, never an address.  The verdicts are the host's (ldspath_host.h).
//
//   * lds_widths: the march of ldspath_host.h's kWidthPasses over the whole allocation;
//   * lds_atomic: ten atomic forms on a table in LDS against the table the host predicts;
//   * lane_xchg:  every op of kLaneOps against its lane map, and the dump of the map itself;
//   * lds_tr:     ds_read_b64_tr_b16 over a 128 KiB image of distinct 16-bit elements.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/ldspath.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "ldspath.h"

namespace {

using namespace canary;
namespace lp = ldspath;

constexpr int kThreads = lp::kThreads;
constexpr int kTableWords = lp::kAtomForms * lp::kAtomWords;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using i16x4 = __attribute__((ext_vector_type(4))) short;
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef __attribute__((address_space(3))) i16x4* lds_i16x4_ptr;

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Minimum over the wave, in every lane.
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v = umin(v, __shfl_xor(v, off, kWave));
  return v;
}

__device__ __forceinline__ void write_head(amdgpu_ldspath_record* __restrict__ rec, uint32_t site, uint32_t site_after,
                                           uint32_t first_sub, uint32_t first_at) {
  rec->site_first = site;
  rec->site_last = site_after;
  rec->first_sub = first_sub;
  rec->first_at = first_at;
}

// The buffer the LDS-DMA pass reads: `words` words, the same for every workgroup.
__global__ void __launch_bounds__(256) dma_fill(uint32_t* __restrict__ buf, int words, uint32_t seed) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) buf[i] = lp::dma_pat(i, seed);
}

// count wrong words into pass `pass`, and keep the lowest (pass, byte offset) of one; no branch
#define NOTE(pass, offset, wrong)                                                                              \
  do {                                                                                                         \
    const uint32_t wrong_ = (wrong);                                                                           \
    bad[pass] += wrong_;                                                                                       \
    first = umin(first, wrong_ ? (static_cast<uint32_t>(pass) << 18) | static_cast<uint32_t>(offset) : kLdsUnwritten); \
  } while (0)

// Stage 1.  `words`: the granted allocation in 32-bit words, a multiple of 256.  Passes are
// numbered as in kWidthPasses (0-based here); the conflict pass runs second, on pass 0's data.
// Injection: lane 0 of the first inject_waves waves flips bit 9 of the first word it is about
// to read itself (kind 0: pass 0, and flips it back before the conflict loads; 1: pass 3; 2:
// after the DMA fill), in repetition 0.
__global__ void __launch_bounds__(kThreads) lds_widths(int words, int reps, uint32_t seed, int inject_kind, int inject_waves,
                                                       const uint32_t* __restrict__ dma_src,
                                                       amdgpu_ldspath_record* __restrict__ records,
                                                       unsigned int* __restrict__ wave_site, int wave_site_len) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t site = site_id();
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const uint32_t gw = blockIdx.x * kLdsWaves + wv;
  const bool inj = lane == 0 && static_cast<int>(gw) < inject_waves;
  u32x4* const l4 = reinterpret_cast<u32x4*>(lds);
  u32x2* const l2 = reinterpret_cast<u32x2*>(lds);
  unsigned short* const l16 = reinterpret_cast<unsigned short*>(lds);
  unsigned char* const l8 = reinterpret_cast<unsigned char*>(lds);
  const int nvec = words / 4, npair = words / 2;
  uint32_t bad[lp::kNumWidthPasses] = {0, 0, 0, 0, 0, 0};
  uint32_t first = kLdsUnwritten;
  // A zero the compiler takes for a per-lane value.  Added to the seed it keeps the patterns
  // in vector registers (in scalar ones the kernel spills SGPRs), and the loops below are not
  // unrolled for the same reason; tests/test_ldspath_abi.py reads the spill counts from the build.
  int vz = 0;
  asm volatile("" : "+v"(vz));
#pragma unroll 1
  for (int rep = 0; rep < reps; ++rep) {
    const uint32_t s = lp::block_seed(seed, blockIdx.x, rep) + vz, s2 = s ^ 0x5A5A5A5Au, s3 = s ^ 0xC3C3C3C3u;
    const bool inj_now = inj && rep == 0;
    // pass 0: 128-bit stores, 32-bit loads in descending order (a wave reads words other waves wrote)
#pragma unroll 1
    for (int v = t; v < nvec; v += kThreads) {
      const uint32_t i = 4u * v;
      const u32x4 x = {lp::lds_pat(i, s), lp::lds_pat(i + 1, s), lp::lds_pat(i + 2, s), lp::lds_pat(i + 3, s)};
      l4[v] = x;
    }
    __syncthreads();
    if (inj_now && inject_kind == kLdsInjectLds) lds[words - 1 - t] ^= lp::kInjectBit;
#pragma unroll 1
    for (int i = words - 1 - t; i >= 0; i -= kThreads) NOTE(0, 4 * i, lds[i] != lp::lds_pat(i, s));
    if (inj_now && inject_kind == kLdsInjectLds) lds[words - 1 - t] ^= lp::kInjectBit;
    __syncthreads();
    // pass 5: conflict and broadcast loads of the same data; (chunk, bank) pairs are dealt to the waves
    {
      const int chunks = (words + 4095) / 4096, chunks32 = (words + 2047) / 2048;
#pragma unroll 1
      for (int k = wv; k < chunks * 64; k += kLdsWaves) {  // 32-bit, lane stride 64 dwords: one bank
        const int w = (k >> 6) * 4096 + 64 * lane + (k & 63);
        if (w < words) NOTE(5, 4 * w, lds[w] != lp::lds_pat(w, s));
      }
#pragma unroll 1
      for (int k = wv; k < chunks32 * 32; k += kLdsWaves) {  // 32-bit, lane stride 32: one bank of the 32-bank modulus
        const int w = (k >> 5) * 2048 + 32 * lane + (k & 31);
        if (w < words) NOTE(5, 4 * w, lds[w] != lp::lds_pat(w, s));
      }
#pragma unroll 1
      for (int k = wv; k < chunks * 32; k += kLdsWaves) {  // 64-bit, lane stride 64 dwords
        const int w = (k >> 5) * 4096 + 64 * lane + 2 * (k & 31);
        if (w < words) {
          const u32x2 g = l2[w >> 1];
          NOTE(5, 4 * w, (g[0] != lp::lds_pat(w, s)) + (g[1] != lp::lds_pat(w + 1, s)));
        }
      }
#pragma unroll 1
      for (int k = wv; k < chunks * 16; k += kLdsWaves) {  // 128-bit, lane stride 64 dwords
        const int w = (k >> 4) * 4096 + 64 * lane + 4 * (k & 15);
        if (w < words) {
          const u32x4 g = l4[w >> 2];
          NOTE(5, 4 * w, (g[0] != lp::lds_pat(w, s)) + (g[1] != lp::lds_pat(w + 1, s)) + (g[2] != lp::lds_pat(w + 2, s)) +
                             (g[3] != lp::lds_pat(w + 3, s)));
        }
      }
#pragma unroll 1
      for (int j = 0; j < 256; ++j) {
        // hashed in vector registers (vz is 0, but not to the compiler): the same address in every lane
        const uint32_t h0 = lp::mix32((static_cast<uint64_t>(s) << 16) ^ static_cast<uint64_t>(j * 8 + wv + vz));
        const uint32_t h1 = lp::mix32((static_cast<uint64_t>(s) << 16) ^ static_cast<uint64_t>(j * 8 + wv + 4 + vz));
        const int w0 = h0 % static_cast<uint32_t>(words), w1 = h1 % static_cast<uint32_t>(words);
        NOTE(5, 4 * w0, lds[w0] != lp::lds_pat(w0, s));  // all 64 lanes on one address
        const int w = (lane & 1) ? w1 : w0;              // two addresses alternating by lane parity
        NOTE(5, 4 * w, lds[w] != lp::lds_pat(w, s));
      }
    }
    __syncthreads();
    // pass 1: 32-bit stores of the complement, 128-bit loads
#pragma unroll 1
    for (int i = t; i < words; i += kThreads) lds[i] = ~lp::lds_pat(i, s);
    __syncthreads();
#pragma unroll 1
    for (int v = t; v < nvec; v += kThreads) {
      const u32x4 g = l4[v];
      const uint32_t i = 4u * v;
      const int j = g[0] != ~lp::lds_pat(i, s) ? 0 : g[1] != ~lp::lds_pat(i + 1, s) ? 1 : g[2] != ~lp::lds_pat(i + 2, s) ? 2 : 3;
      NOTE(1, 4 * (i + j), (g[0] != ~lp::lds_pat(i, s)) + (g[1] != ~lp::lds_pat(i + 1, s)) + (g[2] != ~lp::lds_pat(i + 2, s)) +
                               (g[3] != ~lp::lds_pat(i + 3, s)));
    }
    __syncthreads();
    // pass 2: 64-bit stores, then every halfword and every byte on its own (sub-dword extraction)
#pragma unroll 1
    for (int p = t; p < npair; p += kThreads) {
      const u32x2 x = {lp::lds_pat(2 * p, s2), lp::lds_pat(2 * p + 1, s2)};
      l2[p] = x;
    }
    __syncthreads();
#pragma unroll 1
    for (int h = t; h < 2 * words; h += kThreads)
      NOTE(2, 2 * h, l16[h] != ((lp::lds_pat(h >> 1, s2) >> (16 * (h & 1))) & 0xFFFFu));
#pragma unroll 1
    for (int b = t; b < 4 * words; b += kThreads) NOTE(2, b, l8[b] != ((lp::lds_pat(b >> 2, s2) >> (8 * (b & 3))) & 0xFFu));
    __syncthreads();
    // pass 3: bytes into the lower half, halfwords into the upper half (the byte enables), 64-bit loads
#pragma unroll 1
    for (int b = t; b < 2 * words; b += kThreads) l8[b] = static_cast<unsigned char>(lp::lds_pat(b >> 2, s3) >> (8 * (b & 3)));
#pragma unroll 1
    for (int h = words + t; h < 2 * words; h += kThreads)
      l16[h] = static_cast<unsigned short>(lp::lds_pat(h >> 1, s3) >> (16 * (h & 1)));
    __syncthreads();
    if (inj_now && inject_kind == kLdsInjectSubword) lds[2 * t] ^= lp::kInjectBit;
#pragma unroll 1
    for (int p = t; p < npair; p += kThreads) {
      const u32x2 g = l2[p];
      const bool lo = g[0] != lp::lds_pat(2 * p, s3);
      NOTE(3, 4 * (2 * p + (lo ? 0 : 1)), lo + (g[1] != lp::lds_pat(2 * p + 1, s3)));
    }
    __syncthreads();
    // pass 4: LDS-DMA fill, lane-linear: 4 bytes per lane into the lower part, 16 into the upper
    {
      const int words_a = (words / 512) * 256, words_b = words - words_a;  // both multiples of 256 words
#pragma unroll 1
      for (int c = wv; c < words_a / 64; c += kLdsWaves)
        __builtin_amdgcn_global_load_lds(dma_src + c * 64 + lane, (lds_void_ptr)(lds + c * 64), 4, 0, 0);
#pragma unroll 1
      for (int c = wv; c < words_b / 256; c += kLdsWaves)
        __builtin_amdgcn_global_load_lds(dma_src + words_a + c * 256 + lane * 4, (lds_void_ptr)(lds + words_a + c * 256), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (inj_now && inject_kind == kLdsInjectDma) lds[4 * t] ^= lp::kInjectBit;
#pragma unroll 1
      for (int v = t; v < nvec; v += kThreads) {
        const u32x4 g = l4[v];
        const uint32_t i = 4u * v;
        const int j = g[0] != lp::dma_pat(i, seed) ? 0 : g[1] != lp::dma_pat(i + 1, seed) ? 1 : g[2] != lp::dma_pat(i + 2, seed) ? 2 : 3;
        NOTE(4, 4 * (i + j), (g[0] != lp::dma_pat(i, seed)) + (g[1] != lp::dma_pat(i + 1, seed)) +
                                 (g[2] != lp::dma_pat(i + 2, seed)) + (g[3] != lp::dma_pat(i + 3, seed)));
      }
    }
    __syncthreads();  // the next repetition overwrites what was just read
  }
  first = wave_min(first);
#pragma unroll
  for (int k = 0; k < lp::kNumWidthPasses; ++k) bad[k] = wave_total(bad[k]);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  amdgpu_ldspath_record* rec = records + gw;
  write_head(rec, site, site_after, first == kLdsUnwritten ? kLdsUnwritten : first >> 18, first & 0x3FFFFu);
#pragma unroll
  for (int k = 0; k < lp::kNumWidthPasses; ++k) rec->bad[k] = bad[k];
}

#undef NOTE

// Stage 2.  The table sits at the start of the allocation (`words` >= kTableWords, else the
// kernel does nothing); `expected` is the host's.  Thread kInjectLane of the first
// inject_blocks workgroups perturbs its operand of form inject_op in step 0.
__global__ void __launch_bounds__(kThreads) lds_atomic(int words, int steps, int inject_blocks, int inject_op,
                                                       const uint32_t* __restrict__ expected,
                                                       amdgpu_ldspath_record* __restrict__ records,
                                                       unsigned int* __restrict__ wave_site, int wave_site_len) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  if (words < kTableWords) return;
  const uint32_t site = site_id();
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const uint32_t gw = blockIdx.x * kLdsWaves + wv;
  for (int w = t; w < kTableWords; w += kThreads) lds[w] = lp::atomic_init(w / lp::kAtomWords, w % lp::kAtomWords);
  __syncthreads();
  const bool inj = static_cast<int>(blockIdx.x) < inject_blocks && t == lp::kInjectLane;
  int zero = 0;
  asm volatile("" : "+v"(zero));  // an address the compiler cannot prove uniform: one returning add per lane
  uint32_t lost = 0, spun = 0;
#pragma unroll 1
  for (int s = 0; s < steps; ++s) {
#define OPERAND(form) lp::atomic_operand(form, t, s, inj && s == 0 && inject_op == form)
#define ELEMENT(form) (lds + form * lp::kAtomWords + lp::atomic_index(form, t, s))
    atomicAdd(ELEMENT(lp::kAtomU32Add), static_cast<uint32_t>(OPERAND(lp::kAtomU32Add)));
    atomicAdd(reinterpret_cast<unsigned long long*>(lds + lp::kAtomU64Add * lp::kAtomWords) + lp::atomic_index(lp::kAtomU64Add, t, s),
              static_cast<unsigned long long>(OPERAND(lp::kAtomU64Add)));
    atomicMin(reinterpret_cast<int*>(ELEMENT(lp::kAtomI32Min)), static_cast<int>(OPERAND(lp::kAtomI32Min)));
    atomicMax(ELEMENT(lp::kAtomU32Max), static_cast<uint32_t>(OPERAND(lp::kAtomU32Max)));
    atomicAnd(ELEMENT(lp::kAtomAnd), static_cast<uint32_t>(OPERAND(lp::kAtomAnd)));
    atomicOr(ELEMENT(lp::kAtomOr), static_cast<uint32_t>(OPERAND(lp::kAtomOr)));
    atomicXor(ELEMENT(lp::kAtomXor), static_cast<uint32_t>(OPERAND(lp::kAtomXor)));
    atomicAdd(reinterpret_cast<float*>(ELEMENT(lp::kAtomF32Add)),
              static_cast<float>(static_cast<int>(static_cast<int64_t>(OPERAND(lp::kAtomF32Add)))));
    {  // every thread takes a ticket (a returning add) and marks it seen
      uint32_t* const region = lds + lp::kAtomTicket * lp::kAtomWords;
      const uint32_t ticket = atomicAdd(region + 256 + zero, 1u);
      lost += ticket >= static_cast<uint32_t>(kThreads * steps);
      atomicAdd(region + (ticket & 255u), static_cast<uint32_t>(OPERAND(lp::kAtomTicket)));
    }
    {  // compare-and-swap increment: a loop that runs out of tries is an error, not a spin
      uint32_t* const p = ELEMENT(lp::kAtomCas);
      const uint32_t v = static_cast<uint32_t>(OPERAND(lp::kAtomCas));
      uint32_t old = *p;
      int tries = 0;
#pragma unroll 1
      for (; tries < lp::kCasTries; ++tries) {
        const uint32_t prev = atomicCAS(p, old, old + v);
        if (prev == old) break;
        old = prev;
      }
      spun += tries == lp::kCasTries;
    }
#undef OPERAND
#undef ELEMENT
  }
  __syncthreads();
  // thread t compares words 2t and 2t + 1 of every form's region, untouched elements included
  uint32_t bad[lp::kAtomForms];
  uint32_t first = kLdsUnwritten;
#pragma unroll
  for (int f = 0; f < lp::kAtomForms; ++f) {
    const u32x2 got = reinterpret_cast<const u32x2*>(lds + f * lp::kAtomWords)[t];
    const u32x2 want = reinterpret_cast<const u32x2*>(expected + f * lp::kAtomWords)[t];
    const bool w0 = got[0] != want[0], w1 = got[1] != want[1];
    uint32_t wrong, elem;
    if (f == lp::kAtomU64Add) {
      wrong = w0 || w1;
      elem = t;
    } else {
      wrong = w0 + w1;
      elem = 2 * t + (w0 ? 0 : 1);
    }
    if (f == lp::kAtomTicket && lost) wrong += lost, elem = 256;
    if (f == lp::kAtomCas && spun) wrong += spun;
    bad[f] = wrong;
    if (wrong) first = umin(first, (static_cast<uint32_t>(f) << 16) | elem);
  }
  first = wave_min(first);
#pragma unroll
  for (int f = 0; f < lp::kAtomForms; ++f) bad[f] = wave_total(bad[f]);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  amdgpu_ldspath_record* rec = records + gw;
  write_head(rec, site, site_after, first == kLdsUnwritten ? kLdsUnwritten : first >> 16, first & 0xFFFFu);
#pragma unroll
  for (int f = 0; f < lp::kAtomForms; ++f) rec->bad[f] = bad[f];
}

// Op K of kLaneOps on x and the second value y; o1 only for the two swaps.
template <int K>
__device__ __forceinline__ void lane_apply(int lane, uint32_t x, uint32_t y, uint32_t& o0, uint32_t& o1) {
  constexpr lp::LaneOp op = lp::kLaneOps[K];
  o1 = 0;
  if constexpr (op.kind == lp::kOpBpermute) {
    o0 = __builtin_amdgcn_ds_bpermute(4 * lp::src_code(op, 0, lane), x);
  } else if constexpr (op.kind == lp::kOpPermute) {
    o0 = __builtin_amdgcn_ds_permute(4 * ((lane * op.a + op.b) & 63), x);
  } else if constexpr (op.kind == lp::kOpSwizzleBits) {
    o0 = __builtin_amdgcn_ds_swizzle(x, op.a | (op.b << 5) | (op.c << 10));
  } else if constexpr (op.kind == lp::kOpSwizzleQuad) {
    o0 = __builtin_amdgcn_ds_swizzle(x, 0x8000 | op.a);
  } else if constexpr (op.kind == lp::kOpDpp) {
    o0 = __builtin_amdgcn_update_dpp(y, x, op.a, op.b, op.c, op.d != 0);
  } else if constexpr (op.kind == lp::kOpSwap32) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    o0 = r[0];
    o1 = r[1];
  } else if constexpr (op.kind == lp::kOpSwap16) {
    const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    o0 = r[0];
    o1 = r[1];
  } else if constexpr (op.kind == lp::kOpReadlane) {
    o0 = __builtin_amdgcn_readlane(x, op.a);
  } else if constexpr (op.kind == lp::kOpReadfirstlane) {
    o0 = __builtin_amdgcn_readfirstlane(x);
  } else {
    // no builtin for it; the lane select is an inline constant, the s_nop covers the SGPR the readlane wrote
    const uint32_t v = __builtin_amdgcn_readlane(x, op.a);
    o0 = y;
    asm volatile("s_nop 4\n\tv_writelane_b32 %0, %1, %2" : "+v"(o0) : "s"(v), "n"(op.b));
  }
}

// `rounds` rounds of op K.  Every branch around lane_apply is uniform: EXEC stays full.
template <int K>
__device__ __forceinline__ void lane_rounds(uint32_t seed, uint32_t gw, int lane, int rounds, bool inject,
                                            unsigned int* __restrict__ dump, uint32_t& first,
                                            amdgpu_ldspath_record* __restrict__ rec) {
  constexpr lp::LaneOp op = lp::kLaneOps[K];
  constexpr bool two = lp::lane_outputs(op) == 2;
  const int c0 = lp::src_code(op, 0, lane), c1 = two ? lp::src_code(op, 1, lane) : 0;
  uint32_t bad = 0;
  for (int r = 0; r < rounds; ++r) {
    const uint32_t x = dump ? static_cast<uint32_t>(lane) : lp::lane_value(seed, gw, lane, r, 0);
    const uint32_t y = dump ? static_cast<uint32_t>(64 + lane) : lp::lane_value(seed, gw, lane, r, 1);
    uint32_t o0, o1;
    lane_apply<K>(lane, x, y, o0, o1);
    if (inject && r == 0 && lane == lp::kInjectLane) o0 += 1;
    if (dump) {
      dump[(K * 2) * 64 + lane] = o0;
      dump[(K * 2 + 1) * 64 + lane] = two ? o1 : kLdsUnwritten;
    }
    const uint32_t wrong = (o0 != lp::lane_expected(seed, gw, c0, r)) + (two && o1 != lp::lane_expected(seed, gw, c1, r));
    if (wrong) {
      bad += wrong;
      first = umin(first, (static_cast<uint32_t>(K) << 16) | static_cast<uint32_t>(r));
    }
  }
  bad = wave_total(bad);
  if (lane == 0) rec->bad[K] = bad;
}

template <int... K>
__device__ __forceinline__ void lane_all(std::integer_sequence<int, K...>, uint32_t seed, uint32_t gw, int lane, int rounds,
                                         int inject_op, unsigned int* __restrict__ dump, uint32_t& first,
                                         amdgpu_ldspath_record* __restrict__ rec) {
  (lane_rounds<K>(seed, gw, lane, rounds, inject_op == K, dump, first, rec), ...);
}

// Stage 3.  inject_op >= 0: lane 3 of the first inject_waves waves adds 1 to what it received
// in that op, round 0.  dump != nullptr (one wave): x = lane, the second value = 64 + lane, and
// what every lane received is written out; the counts of such a launch mean nothing.
// The dynamic LDS allocation is not used: its size keeps one workgroup per CU.
__global__ void __launch_bounds__(kThreads) lane_xchg(int rounds, uint32_t seed, int inject_op, int inject_waves,
                                                      unsigned int* __restrict__ dump,
                                                      amdgpu_ldspath_record* __restrict__ records,
                                                      unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kLdsWaves + (threadIdx.x >> 6);
  amdgpu_ldspath_record* rec = records + gw;
  uint32_t first = kLdsUnwritten;
  lane_all(std::make_integer_sequence<int, lp::kNumLaneOps>{}, seed, gw, lane, rounds,
           static_cast<int>(gw) < inject_waves ? inject_op : -1, dump, first, rec);
  first = wave_min(first);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  write_head(rec, site, site_after, first == kLdsUnwritten ? kLdsUnwritten : first >> 16, first & 0xFFFFu);
}

// Stage 4.  The image is the first kTrImageBytes of the allocation (`words` must cover it,
// else the kernel does nothing).  No divergent path leads to the read: EXEC is all ones.
// Lane 3 of the first inject_waves waves adds 1 to element 2 of its first read.
__global__ void __launch_bounds__(kThreads) lds_tr(int words, int rounds, uint32_t seed, int inject_waves,
                                                   amdgpu_ldspath_record* __restrict__ records,
                                                   unsigned int* __restrict__ wave_site, int wave_site_len) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  if (words < lp::kTrImageBytes / 4) return;
  const uint32_t site = site_id();
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const uint32_t gw = blockIdx.x * kLdsWaves + (t >> 6);
  for (int w = t; w < lp::kTrElems / 2; w += kThreads) lds[w] = lp::tr_pat(2 * w, seed) | (lp::tr_pat(2 * w + 1, seed) << 16);
  __syncthreads();
  const bool inj = static_cast<int>(gw) < inject_waves && lane == lp::kInjectLane;
  uint32_t bad = 0, first = kLdsUnwritten;
  for (int r = 0; r < rounds; ++r) {
    const int addr = lp::tr_addr(lane, r);
    i16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(lds_void_ptr)(reinterpret_cast<char*>(lds) + addr));
    if (inj && r == 0) got[2] = static_cast<short>(got[2] + 1);
    uint32_t wrong = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) wrong += static_cast<uint32_t>(static_cast<unsigned short>(got[q])) != lp::tr_pat(lp::tr_source(lane, q, r), seed);
    if (wrong) {
      bad += wrong;
      first = umin(first, static_cast<uint32_t>(r));
    }
  }
  first = wave_min(first);
  bad = wave_total(bad);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  write_head(records + gw, site, site_after, first == kLdsUnwritten ? kLdsUnwritten : 0u, first);
  records[gw].bad[0] = bad;
}

void bad_arguments(char* err, int err_len, int blocks, int reps, int steps, int rounds, int inject_kind, int inject_waves,
                   int inject_op) {
  std::snprintf(err, err_len,
                "ldspath check: bad arguments (blocks %d in 0..%d, reps %d in 1..%d, steps %d in 1..%d, rounds %d in 1..%d, "
                "inject %d/%d/%d with an op below %d or a form below %d)",
                blocks, lp::kMaxBlocks, reps, lp::kMaxReps, steps, lp::kMaxSteps, rounds, lp::kMaxRounds, inject_kind,
                inject_waves, inject_op, lp::kNumLaneOps, lp::kAtomForms);
}

int copy_name(const char* name, char* buf, int len) {
  return buf != nullptr && len > 0 ? std::snprintf(buf, len, "%s", name) : static_cast<int>(std::strlen(name));
}

}  // namespace

extern "C" {

int amdgpu_ldspath_sizeof(int which) {
  return which == 0 ? static_cast<int>(sizeof(amdgpu_ldspath_record)) : which == 1 ? static_cast<int>(sizeof(amdgpu_ldspath_result)) : -1;
}

int amdgpu_ldspath_ops(int table, int index, char* buf, int len) {
  static const char* const kinds[] = {"plain", "subword", "dma", "conflict"};
  const int count = table == 0 ? lp::kNumLaneOps : table == 1 ? lp::kAtomForms : table == 2 || table == 3 ? lp::kNumWidthPasses : -1;
  if (count < 0 || index >= count) return -1;
  if (index < 0) return count;
  return copy_name(table == 0   ? lp::kLaneOpNames[index]
                   : table == 1 ? lp::kAtomNames[index]
                   : table == 2 ? lp::kWidthPasses[index].name
                                : kinds[lp::kWidthPasses[index].kind],
                   buf, len);
}

int amdgpu_ldspath_lane_map(int op, int* out) {
  if (op < 0 || op >= lp::kNumLaneOps || out == nullptr) return -1;
  const int outputs = lp::lane_outputs(lp::kLaneOps[op]);
  for (int o = 0; o < 2; ++o)
    for (int l = 0; l < 64; ++l) out[o * 64 + l] = o < outputs ? lp::src_code(lp::kLaneOps[op], o, l) : -1;
  return outputs;
}

int amdgpu_ldspath_tr_map(int round, int* addr_out, int* source_out) {
  if (round < 0 || round >= lp::tr_rounds(lp::kMaxRounds) || addr_out == nullptr || source_out == nullptr) return -1;
  for (int l = 0; l < 64; ++l) {
    addr_out[l] = lp::tr_addr(l, round);
    for (int q = 0; q < 4; ++q) source_out[l * 4 + q] = lp::tr_source(l, q, round);
  }
  return 0;
}

int amdgpu_ldspath_atomic_expected(int form, int steps, unsigned int* out, int out_words) {
  if (out_words < lp::kAtomWords) return -1;
  return lp::atomic_expected(form, steps, out) ? 0 : -1;
}

int amdgpu_ldspath_reduce(const amdgpu_ldspath_record* widths, int n_widths, const amdgpu_ldspath_record* atomic,
                          int n_atomic, const amdgpu_ldspath_record* lane, int n_lane, const amdgpu_ldspath_record* tr,
                          int n_tr, amdgpu_ldspath_result* result) {
  if (result == nullptr) return -1;
  std::memset(result, 0, sizeof(*result));
  const amdgpu_ldspath_record* const recs[kLdsStages] = {widths, atomic, lane, tr};
  const int n[kLdsStages] = {n_widths, n_atomic, n_lane, n_tr};
  return lp::reduce(recs, n, result) ? 0 : -1;
}

int amdgpu_ldspath_describe(const amdgpu_ldspath_result* r, int which, char* buf, int len) {
  return lp::describe(*r, which, buf, len);
}

int amdgpu_ldspath_lane_sources(int device, unsigned int* out, int out_len, char* err, int err_len) {
  constexpr int n = lp::kNumLaneOps * 128;
  if (out == nullptr || out_len < n) {
    std::snprintf(err, err_len, "ldspath check: bad arguments (lane_sources needs room for %d values)", n);
    return -1;
  }
  Status st;
  DeviceBuffer<unsigned int> d_dump;
  DeviceBuffer<amdgpu_ldspath_record> d_record;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, d_dump.alloc(sizeof(unsigned int) * n));
  CANARY_HIP(st, d_dump.fill(0xFF));
  CANARY_HIP(st, d_record.alloc(sizeof(amdgpu_ldspath_record)));
  st.stage("lane_xchg (dump): ");
  if (st.ok()) {  // one wave
    hipLaunchKernelGGL(lane_xchg, dim3(1), dim3(kWave), 0, 0, 1, 0u, -1, 0, d_dump.get(), d_record.get(),
                       static_cast<unsigned int*>(nullptr), 0);
    CANARY_HIP(st, hipGetLastError());
    CANARY_HIP(st, hipDeviceSynchronize());
  }
  CANARY_HIP(st, d_dump.download(out));
  return st.report("ldspath check: ", err, err_len);
}

int amdgpu_ldspath_run(int device, int blocks, int reps, int steps, int rounds, int inject_kind, int inject_waves,
                       int inject_op, unsigned int* wave_site_out, int wave_site_len, amdgpu_ldspath_result* out, char* err,
                       int err_len) {
  std::memset(out, 0, sizeof(*out));
  if (!lp::arguments_ok(blocks, reps, steps, rounds, inject_kind, inject_waves, inject_op, wave_site_len,
                        wave_site_out != nullptr)) {
    bad_arguments(err, err_len, blocks, reps, steps, rounds, inject_kind, inject_waves, inject_op);
    return -1;
  }
  Status st;
  hipDeviceProp_t prop;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (!st.ok()) return st.report("ldspath check: ", err, err_len);
  const LaunchPlan plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
  const int grid = plan.grid, max_launches = plan.max_launches;
  const size_t slots = static_cast<size_t>(grid) * kLdsWaves;
  out->cus_expected = prop.multiProcessorCount;
  out->blocks = grid;
  out->reps = reps;
  out->steps = steps;
  out->rounds = rounds;

  std::vector<uint32_t> h_expected(kTableWords);
  for (int f = 0; f < lp::kAtomForms; ++f) lp::atomic_expected(f, steps, h_expected.data() + f * lp::kAtomWords);
  DeviceBuffer<amdgpu_ldspath_record> d_records;  // the four stages' slots, one after another
  DeviceBuffer<unsigned int> d_wave_site;
  DeviceBuffer<uint32_t> d_dma, d_expected;
  Events<kLdsStages + 1> ev;
  CANARY_HIP(st, d_records.alloc(sizeof(amdgpu_ldspath_record) * slots * kLdsStages));
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * kLdsStages * wave_site_len));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, d_dma.alloc(kMaxLdsBytes));
  CANARY_HIP(st, d_expected.alloc(sizeof(uint32_t) * kTableWords));
  CANARY_HIP(st, d_expected.upload(h_expected.data()));
  CANARY_HIP(st, ev.create());

  std::vector<amdgpu_ldspath_record> h[kLdsStages];
  size_t granted = 0;
  for (int l = 0; l < max_launches && st.ok(); ++l) {
    const uint32_t seed = 0x1D5Au + static_cast<uint32_t>(l);
    const int kind = l == 0 ? inject_kind : -1;
    const int waves = l == 0 ? inject_waves : 0;
    unsigned int* ws[kLdsStages];
    for (int s = 0; s < kLdsStages; ++s) ws[s] = l == 0 && wave_site_len > 0 ? d_wave_site.get() + s * wave_site_len : nullptr;
    const int ws_len = l == 0 ? wave_site_len : 0;
    float ms[kLdsStages] = {0, 0, 0, 0};
    st.stage("dma_fill: ");
    CANARY_HIP(st, d_records.fill(0xFF));
    if (st.ok()) {  // an earlier launch than the one that reads it
      hipLaunchKernelGGL(dma_fill, dim3(16), dim3(256), 0, 0, d_dma.get(), kMaxLdsBytes / 4, seed);
      CANARY_HIP(st, hipGetLastError());
    }
    st.stage("launch: ");
    time_stages(st, ev, ms, [&](int k) {
      size_t got = 0;
      amdgpu_ldspath_record* rec = d_records.get() + slots * k;
      if (k == 0)
        got = launch_with_max_lds(lds_widths, prop, dim3(grid), dim3(kThreads), granted_lds_words{}, reps, seed, kind, waves,
                                  static_cast<const uint32_t*>(d_dma.get()), rec, ws[0], ws_len);
      else if (k == 1)
        got = launch_with_max_lds(lds_atomic, prop, dim3(grid), dim3(kThreads), granted_lds_words{}, steps,
                                  kind == kLdsInjectAtomic ? waves : 0, inject_op, static_cast<const uint32_t*>(d_expected.get()),
                                  rec, ws[1], ws_len);
      else if (k == 2)
        got = launch_with_max_lds(lane_xchg, prop, dim3(grid), dim3(kThreads), rounds, seed, kind == kLdsInjectLane ? inject_op : -1,
                                  kind == kLdsInjectLane ? waves : 0, static_cast<unsigned int*>(nullptr), rec, ws[2], ws_len);
      else
        got = launch_with_max_lds(lds_tr, prop, dim3(grid), dim3(kThreads), granted_lds_words{}, lp::tr_rounds(rounds), seed,
                                  kind == kLdsInjectTr ? waves : 0, rec, ws[3], ws_len);
      if (got == 0) return hipErrorLaunchFailure;
      granted = got;
      return hipSuccess;
    });
    for (int s = 0; s < kLdsStages && st.ok(); ++s) {
      const size_t have = h[s].size();
      h[s].resize(have + slots);
      CANARY_HIP(st, hipMemcpy(h[s].data() + have, d_records.get() + slots * s, sizeof(amdgpu_ldspath_record) * slots,
                               hipMemcpyDeviceToHost));
      out->stage_ms[s] += ms[s];
    }
    if (!st.ok()) break;
    if (granted < static_cast<size_t>(lp::kTrImageBytes)) {
      std::snprintf(err, err_len, "ldspath check: the device grants %zu bytes of LDS, the transposed-read image needs %d",
                    granted, lp::kTrImageBytes);
      return -1;
    }
    out->launches = l + 1;
    out->lds_bytes = granted;
    const amdgpu_ldspath_record* const recs[kLdsStages] = {h[0].data(), h[1].data(), h[2].data(), h[3].data()};
    const int n[kLdsStages] = {static_cast<int>(h[0].size()), static_cast<int>(h[1].size()), static_cast<int>(h[2].size()),
                               static_cast<int>(h[3].size())};
    if (!lp::reduce(recs, n, out)) {
      std::snprintf(err, err_len, "ldspath check: a record holds a site out of range");
      return -1;
    }
    if (covered(*out, out->cus_expected)) break;
  }
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));
  return st.report("ldspath check: ", err, err_len);
}

}  // extern "C"
