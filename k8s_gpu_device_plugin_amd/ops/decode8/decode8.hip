// MI355X (gfx950 / CDNA4) health canary: the fp8 decode-attention path (paged e4m3 KV cache, GQA, split-KV).
//
// o[B][Hq][128] (fp32) = softmax(q k^T / sqrt(128)) v over the first seq_lens[b] keys of sequence b
// and lse[B][Hq], where key j of KV head h is k_scale[h] * fp8(k_cache[...]) and likewise V: what
// ops/decode runs on a bf16 cache, on the cache inference containers actually keep.  The MFMA lane
// maps, the bf16 pack of P, the v_permlane32_swap reductions, the base-2 online softmax and the two
// merges are decode_split's; everything between HBM and the MFMA operands is new.
//
// kv8_split: one workgroup of 4 waves per (sequence, KV head, partition).
//   * Work split: decode_split's.  In every 128-key tile wave w owns keys 32 w .. 32 w + 31 (pages
//     2 w and 2 w + 1, 2 KiB each) from the DMA to the accumulators; its loop ends at its own last
//     visible tile.
//   * LDS: KV8_STAGES x 32 KiB, one __shared__ object.  A wave's stage is a K image and a V image
//     of [32 rows][128 B]; one global_load_lds_dwordx4 of the wave moves 8 rows, so a page is 2
//     pieces of K and 2 of V.  Source of row j: cache + ((table[b][page] * Hkv + kvh) * 16 + j) * 128.
//     Logical 16 B chunk c of row r sits at physical chunk c ^ swizzle(r), applied on the global
//     source address (swizzle() below says why it is not r & 7).  Table entries are fetched a tile
//     ahead; a page at or past ceil(len / 16) is neither looked up nor staged.  Producer and consumer
//     are the same wave: s_waitcnt vmcnt(n) with n the loads of the later tiles in flight, no barrier.
//   * Scores: S^T[32 keys][32 q] = K Q^T, 8 v_mfma_f32_32x32x16_bf16.  Lane (r, h) reads logical chunk
//     2 s' + h of K row r with one ds_read_b128: 16 codes, d = 16 (2 s' + h) .. + 15, decoded to bf16
//     in registers (exact); the first 8 are the A operand of step 2 s', the next 8 of step 2 s' + 1.
//     Q is loaded once from global memory in that permutation of d.  Scaled in fp32 by
//     k_scale[kvh] * log2(e) / sqrt(128), one factor per workgroup.
//   * Second product: O^T[128 d][32 q] += V^T P^T, 2 key steps x 4 d-blocks.  One ds_read_b64_tr_b8
//     per (step, d-block) supplies keys 16 t + 4 h + 8 (j >> 2) + (j & 3) of column 32 db + r: in a
//     16-lane group lane 2 q + p supplies the address of row q, bytes 8 p .. 8 p + 7, and lane i
//     receives byte i of rows 0 .. 7 (measured; docs/CANARY.md).  On a ragged tile the bytes of keys
//     >= len are zeroed before decoding: the rest of a last page is whatever the cache holds.
//   * Merge: decode_split's, through the wave's own slice and one barrier, to the workspace.
// kv8_combine: decode_combine's algorithm, then (acc / l) * v_scale[kvh].
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/decode8.py): decode8.h.
#include "decode8.h"

#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

namespace {

using namespace canary;
using namespace decode8;

typedef __attribute__((address_space(3))) void* lds_void_ptr;
using i32x2 = __attribute__((ext_vector_type(2))) int;
typedef __attribute__((address_space(3))) i32x2* lds_i32x2_ptr;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int kRowBytes = kD;               // 128 B: a row of K or V
constexpr int kImage = 32 * kRowBytes;      // a wave's 32 keys of K or of V: 4 KiB
constexpr int kStage = 2 * kImage;          // K + V of one tile
// Stages of a wave's slice.  2 is the draft: 16 KiB per wave, 64 KiB per workgroup, two workgroups
// per CU, tile t + 1 in flight while tile t is computed.  4 is the alternative it is measured
// against (docs/CANARY.md, "The fp8 decode-attention path / Measured"): 128 KiB, one workgroup per
// CU, three tiles in flight; -DKV8_STAGES=4 builds it.
#ifndef KV8_STAGES
#define KV8_STAGES 2
#endif
constexpr int kStages = KV8_STAGES;
static_assert(kStages == 2 || kStages == 4, "two or four stages");
constexpr int kSlice = kStages * kStage;    // a wave's stages
constexpr int kStateMl = 16 * kD * 4;       // a wave's merge state in its slice: acc [16][128], then (m, l) [16]
constexpr float kScaleLog2e = 0.12751743074602467f;  // log2(e) / sqrt(128)
constexpr float kLn2 = 0.6931471805599453f;

// The chunk swizzle of a [32][128 B] image.  A row is 32 banks of the 64, so rows of one parity
// start in the same bank and a 16 B chunk falls into one of 16 bank groups: (row & 1, physical chunk).
//   * K: ds_read_b128, 16 lanes a pass: rows 16 n .. 16 n + 15, one logical chunk.  Conflict-free
//     when the 8 rows of one parity get 8 different physical chunks.
//   * V: ds_read_b64_tr_b8, 32 lanes a pass: of rows 16 t + 4 h + {0..3, 8..11} both halves of the
//     logical chunks 2 db and 2 db + 1.  Conflict-free when, among the 4 rows of one parity, the
//     pairs {c, c ^ 1} ^ swizzle are disjoint: swizzle >> 1 must differ.
// Row bits (r3, r1) vary among those 4 rows and r2 is fixed, so swizzle = (r3, r1, r2) meets both; the
// first candidate, r & 7, gives rows 0 and 8 the same chunk in both patterns.  -DKV8_SWIZZLE=0 builds that one.
#ifndef KV8_SWIZZLE
#define KV8_SWIZZLE 1
#endif
__device__ __forceinline__ int swizzle(int row) {
  return KV8_SWIZZLE ? ((row >> 1) & 4) | (row & 2) | ((row >> 2) & 1) : row & 7;
}

// max / sum of x with the value lane l ^ 32 holds: one v_permlane32_swap, no LDS.  Each result of
// the swap is copied to a scalar first (ops/attn/attn.hip says why).
__device__ __forceinline__ float with_other_half(float x, bool sum) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  const float a = __builtin_bit_cast(float, r0), b = __builtin_bit_cast(float, r1);
  return sum ? a + b : fmaxf(a, b);
}

// two fp32 -> one dword of two bf16, round to nearest even: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}

// Two dwords of 4 e4m3 codes each -> 8 bf16, exact: v_cvt_scalef32_pk_bf16_fp8 at a scale of exactly
// 1.0 (never a caller's scale), one instruction per pair of codes.
__device__ __forceinline__ bf16x8 to_bf16x8(unsigned w0, unsigned w1) {
  const u32x4 x = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true))};
  return __builtin_bit_cast(bf16x8, x);
}

// 2^(m_w - m), and exactly 0 for a state that saw no key (m_w = -inf, also when m is)
__device__ __forceinline__ float merge_weight(float m_w, float m) {
  return m_w == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_w - m);
}

// s_waitcnt vmcnt(n) for the wave-uniform n a tile loop can ask for: whole pages of 4 loads
__device__ __forceinline__ void wait_loads(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
  }
}

__global__ void __launch_bounds__(256) kv8_split(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kc,
                                                 const uint8_t* __restrict__ Vc, const float* __restrict__ k_scale,
                                                 const int* __restrict__ table, const int* __restrict__ lens,
                                                 float* __restrict__ ws_acc, float* __restrict__ ws_ml, int B, int Hq, int Hkv,
                                                 int max_pages, int splits) {
#pragma clang fp contract(off)  // s * factor - m as two roundings: m is one of the s * factor
  __shared__ __attribute__((aligned(16))) char smem[4 * kSlice];  // the only LDS object: [wave][stage][K|V][32][128 B]
  static_assert(kStateMl + 16 * 8 <= kSlice, "a wave's merge state fits its slice");

  // host checks the call; never touch memory for one this kernel was not built for
  if (B <= 0 || !group_ok(Hq, Hkv) || max_pages <= 0 || splits < 1 || splits > kMaxSplits ||
      static_cast<long long>(gridDim.x) != static_cast<long long>(B) * Hkv * splits) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5, G = Hq / Hkv;
  const int wg = blockIdx.x, part = wg % splits, kvh = (wg / splits) % Hkv, b = wg / splits / Hkv;
  const int len = lens[b];
  if (len < 1 || len > kMaxSeq || len > kPage * max_pages) return;  // the whole workgroup, ahead of the barrier
  const int npages = pages_of(len), per = tiles_per_split(len, splits), t0 = part * per;
  // wave w sees a key of tile t when 128 t + 32 w < len: its loop is t0 .. t_end - 1, empty for an empty partition
  const int mine = len - 32 * wave, t_mine = mine > 0 ? (mine + kTile - 1) / kTile : 0;
  const int t_end = t0 + per < t_mine ? t0 + per : t_mine;
  const float factor = k_scale[kvh] * kScaleLog2e;  // the dequantisation of K, folded into the score factor

  const int* pages = table + static_cast<size_t>(b) * max_pages;
  char* slice = smem + wave * kSlice;

  // the wave's two table entries of tile t; a page past the sequence's last is not looked up
  auto lookup = [&](int t, int (&e)[2]) {
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      const int pg = 8 * t + 2 * wave + ph;
      e[ph] = pg < npages ? pages[pg] : -1;
    }
  };
  // the wave's pages of tile t that exist: 2, or 1 on its last tile, 0 past it
  auto staged_pages = [&](int t) {
    const int n = npages - (8 * t + 2 * wave);
    return t >= t_end || n <= 0 ? 0 : n < 2 ? n : 2;
  };
  // ... and its 32 keys of K and of V into stage `buf`: 2 pieces (8 rows, 1 KiB) of each per page
  auto stage = [&](int t, int buf, const int (&e)[2]) {
    char* base = slice + buf * kStage;
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      if (ph >= staged_pages(t)) continue;  // wave-uniform
      const size_t page = (static_cast<size_t>(e[ph]) * Hkv + kvh) * kPageBytes;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 16 * ph + 8 * i + (lane >> 3), cb = ((lane & 7) ^ swizzle(row)) << 4;
        const size_t src = page + (row & 15) * kRowBytes + cb;
        __builtin_amdgcn_global_load_lds(Kc + src, (lds_void_ptr)(base + (2 * ph + i) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(Vc + src, (lds_void_ptr)(base + kImage + (2 * ph + i) * 1024), 16, 0, 0);
      }
    }
  };
  int ent[2] = {-1, -1};
  if (t0 < t_end) {
    lookup(t0, ent);
#pragma unroll
    for (int i = 0; i < kStages - 1; ++i) {  // stage() skips a tile past the wave's last
      stage(t0 + i, i, ent);
      lookup(t0 + i + 1, ent);
    }
  }

  // Query row r < G of this KV head as the B operand of every score MFMA.  Step 2 s' + u of lane half
  // h multiplies d = 16 (2 s' + h) + 8 u .. + 7, the order in which the lane decodes its K chunk.
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (r < G) {
    const bf16x8* qp = reinterpret_cast<const bf16x8*>(Q + (static_cast<size_t>(b) * Hq + kvh * G + r) * kD);
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = qp[4 * (s >> 1) + 2 * h + (s & 1)];
  }

  // The lane's transposed-read address within a 16-key step of a V image, per d-block db: lane
  // 2 q + p of 16-lane group g names row 4 (g >> 1) + 8 (q >> 2) + (q & 3), bytes 32 db + 16 (g & 1) + 8 p .. + 7.
  int vaddr[4];
  {
    const int g = lane >> 4, q = (lane >> 1) & 7, p = lane & 1;
    const int row = 4 * (g >> 1) + 8 * (q >> 2) + (q & 3);  // swizzle(row + 16 t) is the row's own
#pragma unroll
    for (int db = 0; db < 4; ++db) vaddr[db] = row * kRowBytes + (((2 * db + (g & 1)) ^ swizzle(row)) << 4) + 8 * p;
  }

  f32x16 acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[db][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int t = t0; t < t_end; ++t) {
    const int cur = (t - t0) & (kStages - 1), k0 = t * kTile + 32 * wave;  // the wave's first key of the tile: visible
    int later = 0;  // loads of the tiles in flight behind tile t
#pragma unroll
    for (int i = 1; i < kStages - 1; ++i) later += 4 * staged_pages(t + i);
    wait_loads(later);  // tile t has landed
    stage(t + kStages - 1, (cur + kStages - 1) & (kStages - 1), ent);  // tile t - 1's stage is free: this wave read it
    lookup(t + kStages, ent);
    const char* Ks = slice + cur * kStage;
    const char* Vs = Ks + kImage;
    const bool ragged = k0 + 32 > len;
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int sp = 0; sp < 4; ++sp) {
      const u32x4 c = *reinterpret_cast<const u32x4*>(Ks + r * kRowBytes + (((2 * sp + h) ^ swizzle(r)) << 4));
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(to_bf16x8(c[0], c[1]), qf[2 * sp], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(to_bf16x8(c[2], c[3]), qf[2 * sp + 1], s, 0, 0, 0);
    }
    float mt = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float x = s[e] * factor;
      if (ragged && k0 + cd_row32(e, h) >= len) x = -INFINITY;
      s[e] = x;
      mt = fmaxf(mt, x);
    }
    const float m_new = fmaxf(m, with_other_half(mt, false));  // finite: key k0 is visible
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    float lt = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s[e] = __builtin_amdgcn_exp2f(s[e] - m_new);
      lt += s[e];
    }
    l = l * alpha + with_other_half(lt, true);
    m = m_new;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[db][e] *= alpha;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {  // 16 keys per step
      const int e0 = 8 * t2;
      const u32x4 packed = {pack_bf16(s[e0 + 0], s[e0 + 1]), pack_bf16(s[e0 + 2], s[e0 + 3]),
                            pack_bf16(s[e0 + 4], s[e0 + 5]), pack_bf16(s[e0 + 6], s[e0 + 7])};
      const bf16x8 pf = __builtin_bit_cast(bf16x8, packed);
      const char* Vt = Vs + t2 * 16 * kRowBytes;
      // byte j of the fragment is key k0 + 16 t2 + 4 h + 8 (j >> 2) + (j & 3): on a ragged tile keep the visible ones
      unsigned keep[2] = {~0u, ~0u};
      if (ragged) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int vis = len - (k0 + 16 * t2 + 4 * h + 8 * u);
          keep[u] = vis >= 4 ? ~0u : vis <= 0 ? 0u : (1u << (8 * vis)) - 1u;
        }
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2_ptr)(lds_void_ptr)(Vt + vaddr[db]));
        const bf16x8 vf = to_bf16x8(static_cast<unsigned>(v[0]) & keep[0], static_cast<unsigned>(v[1]) & keep[1]);
        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, acc[db], 0, 0, 0);
      }
    }
  }

  // The wave's state of its G rows into its own slice (its stages are free: every tile it staged was
  // waited for and read), one barrier, then every thread merges the 4 states of (row, d) pairs.
  if (r < G) {
    float* st_acc = reinterpret_cast<float*>(slice) + r * kD;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int eg = 0; eg < 4; ++eg)  // d = 32 db + cd_row32(4 eg .. + 3, h)
        *reinterpret_cast<f32x4*>(st_acc + 32 * db + 8 * eg + 4 * h) =
            f32x4{acc[db][4 * eg], acc[db][4 * eg + 1], acc[db][4 * eg + 2], acc[db][4 * eg + 3]};
    if (h == 0) *reinterpret_cast<f32x2*>(slice + kStateMl + r * 8) = f32x2{m, l};
  }
  __syncthreads();
  const int d = tid & (kD - 1);
  for (int g = tid >> 7; g < G; g += 2) {
    float mw[4], mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mw[w] = reinterpret_cast<const float*>(smem + w * kSlice + kStateMl)[2 * g];
      mx = fmaxf(mx, mw[w]);
    }
    float lsum = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wt = merge_weight(mw[w], mx);
      lsum += reinterpret_cast<const float*>(smem + w * kSlice + kStateMl)[2 * g + 1] * wt;
      a += reinterpret_cast<const float*>(smem + w * kSlice)[g * kD + d] * wt;
    }
    const size_t at = (static_cast<size_t>(b) * Hq + kvh * G + g) * splits + part;
    ws_acc[at * kD + d] = a;
    if (d == 0) *reinterpret_cast<f32x2*>(ws_ml + 2 * at) = f32x2{mx, lsum};
  }
}

// One wave per (sequence, query head): lane i holds d = 2 i, 2 i + 1.  decode_combine's merge, then
// the dequantisation of V: one multiply after the correctly rounded division.
__global__ void __launch_bounds__(256) kv8_combine(const float* __restrict__ ws_acc, const float* __restrict__ ws_ml,
                                                   const float* __restrict__ v_scale, float* __restrict__ O,
                                                   float* __restrict__ L, int rows, int Hq, int Hkv, int splits) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows || splits < 1 || splits > kMaxSplits || !group_ok(Hq, Hkv)) return;
  const float* ml = ws_ml + static_cast<size_t>(row) * splits * 2;
  const float* part = ws_acc + static_cast<size_t>(row) * splits * kD + 2 * lane;
  const float vs = v_scale[(row % Hq) / (Hq / Hkv)];
  float m = -INFINITY;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, ml[2 * s]);
  float l = 0.f;
  f32x2 a = {0.f, 0.f};
  for (int s = 0; s < splits; ++s) {
    if (ml[2 * s] == -INFINITY) continue;  // an empty partition
    const float wt = __builtin_amdgcn_exp2f(ml[2 * s] - m);
    const f32x2 v = *reinterpret_cast<const f32x2*>(part + static_cast<size_t>(s) * kD);
    l += ml[2 * s + 1] * wt;
    a[0] += v[0] * wt;
    a[1] += v[1] * wt;
  }
  *reinterpret_cast<f32x2*>(O + static_cast<size_t>(row) * kD + 2 * lane) = f32x2{a[0] / l * vs, a[1] / l * vs};
  if (lane == 0) L[row] = kLn2 * (m + log2f(l));
}

// ---- the check's data and its verifier --------------------------------------------------------
// The visible keys of every sequence through the block table; the caches were poisoned before.
__global__ void __launch_bounds__(256) kv8_fill(uint16_t* __restrict__ Q, uint8_t* __restrict__ Kc, uint8_t* __restrict__ Vc,
                                                float* __restrict__ k_scale, float* __restrict__ v_scale,
                                                const int* __restrict__ table, const int* __restrict__ lens, int set, int B,
                                                int Hq, int Hkv, int max_pages, int seq) {
  const size_t nq = static_cast<size_t>(B) * Hq * kD, nk = static_cast<size_t>(B) * Hkv * seq * kD;
  const size_t first = blockIdx.x * 256ull + threadIdx.x, step = static_cast<size_t>(gridDim.x) * 256;
  for (size_t e = first; e < static_cast<size_t>(Hkv); e += step)
    k_scale[e] = k_scale_of(set, static_cast<int>(e)), v_scale[e] = v_scale_of(set, static_cast<int>(e));
  for (size_t e = first; e < nq; e += step) {
    const int d = e % kD, hq = (e / kD) % Hq, b = e / kD / Hq;
    Q[e] = decode::bf16_bits(q_val(set, b, hq, d));
  }
  for (size_t e = first; e < nk; e += step) {
    const int d = e % kD, j = (e / kD) % seq, kvh = (e / kD / seq) % Hkv, b = e / kD / seq / Hkv;
    if (j >= lens[b]) continue;
    const int page = table[static_cast<size_t>(b) * max_pages + j / kPage];
    const size_t at = ((static_cast<size_t>(page) * Hkv + kvh) * kPage + j % kPage) * kD + d;
    Kc[at] = k_code(set, b, kvh, j, d);
    Vc[at] = v_code(set, b, kvh, j, d);
  }
}

// counts[0] wrong elements of o, [1] wrong lse values, [2] / [3] the smallest index of each.
// One block per (sequence, head) of an exact set, one thread per d: the bits of o against the closed
// form, so a NaN, an Inf and a -0 for a +0 all count.
__global__ void __launch_bounds__(kD) kv8_verify(const float* __restrict__ O, const float* __restrict__ L,
                                                 const int* __restrict__ lens, int set, int Hq, int Hkv,
                                                 unsigned long long* __restrict__ counts) {
  const int b = blockIdx.x / Hq, hq = blockIdx.x % Hq, kvh = hq / (Hq / Hkv), d = threadIdx.x, len = lens[b];
  const Top top = decode::top_of(set, b, hq, len);
  const float want = expected_o(decode::top_sum(set, b, hq, kvh, d, top, len), top, v_scale_of(set, kvh));
  const size_t at = static_cast<size_t>(blockIdx.x) * kD + d;
  const bool bad = __builtin_bit_cast(uint32_t, O[at]) != __builtin_bit_cast(uint32_t, want);
  if (bad) atomicMin(counts + 2, static_cast<unsigned long long>(at));
  block_add_errors(bad, counts);
  if (d == 0 && !lse_within(L[blockIdx.x], expected_lse(top, k_scale_of(set, kvh)))) {
    atomicAdd(counts + 1, 1ull);
    atomicMin(counts + 3, static_cast<unsigned long long>(blockIdx.x));
  }
}

// The device side of one decode attention: the operands, the workspace of the partial states, o and lse.
struct Decode8Buffers {
  DeviceBuffer<uint16_t> q;
  DeviceBuffer<uint8_t> k, v;
  DeviceBuffer<int> table, lens;
  DeviceBuffer<float> k_scale, v_scale, ws_acc, ws_ml, o, lse;
  int B = 0, Hq = 0, Hkv = 0, max_pages = 0, splits = 0;
  void alloc(Status& st, int device, int B_, int Hq_, int Hkv_, int P, int max_pages_, int splits_) {
    B = B_, Hq = Hq_, Hkv = Hkv_, max_pages = max_pages_, splits = splits_;
    const size_t rows = static_cast<size_t>(B) * Hq, cache = static_cast<size_t>(P) * Hkv * kPageBytes;
    CANARY_HIP(st, hipSetDevice(device));
    CANARY_HIP(st, q.alloc(rows * kD * 2));
    CANARY_HIP(st, k.alloc(cache));
    CANARY_HIP(st, v.alloc(cache));
    CANARY_HIP(st, k_scale.alloc(static_cast<size_t>(Hkv) * 4));
    CANARY_HIP(st, v_scale.alloc(static_cast<size_t>(Hkv) * 4));
    CANARY_HIP(st, table.alloc(static_cast<size_t>(B) * max_pages * 4));
    CANARY_HIP(st, lens.alloc(static_cast<size_t>(B) * 4));
    CANARY_HIP(st, ws_acc.alloc(rows * splits * kD * 4));
    CANARY_HIP(st, ws_ml.alloc(rows * splits * 2 * 4));
    CANARY_HIP(st, o.alloc(rows * kD * 4));
    CANARY_HIP(st, lse.alloc(rows * 4));
  }
  void launch() const {  // the pair
    hipLaunchKernelGGL(kv8_split, dim3(B * Hkv * splits), dim3(256), 0, 0, q.get(), k.get(), v.get(), k_scale.get(), table.get(),
                       lens.get(), ws_acc.get(), ws_ml.get(), B, Hq, Hkv, max_pages, splits);
    hipLaunchKernelGGL(kv8_combine, dim3((B * Hq + 3) / 4), dim3(256), 0, 0, ws_acc.get(), ws_ml.get(), v_scale.get(), o.get(),
                       lse.get(), B * Hq, Hq, Hkv, splits);
  }
};

// splits = 0: decode's rule, at least four workgroups per CU of the device
int resolve_splits(Status& st, int device, int splits, int B, int Hkv, int longest) {
  if (splits) return splits;
  hipDeviceProp_t prop;
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  return st.ok() ? decode::choose_splits(B, Hkv, longest, 4 * prop.multiProcessorCount) : 1;
}

// The hashed set's verdict on downloaded o and lse: every (sequence, head) against float64, the
// (sequence, KV head) groups shared among up to 16 host threads.
void judge_hashed(const std::vector<float>& o, const std::vector<float>& lse, const std::vector<int>& lens, int B, int Hq, int Hkv,
                  amdgpu_decode8_result* res) {
  const int G = Hq / Hkv, groups = B * Hkv;
  std::vector<double> ref_o(static_cast<size_t>(B) * Hq * kD), ref_lse(static_cast<size_t>(B) * Hq);
  unsigned n = std::thread::hardware_concurrency();
  n = n < 1 ? 1 : n > 16 ? 16 : n;
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < n; ++w)
    pool.emplace_back([&, w] {
      for (int grp = static_cast<int>(w); grp < groups; grp += static_cast<int>(n)) {
        const int b = grp / Hkv, kvh = grp % Hkv;
        const size_t row = static_cast<size_t>(b) * Hq + kvh * G;
        reference_group(kHashed, b, kvh, G, lens[b], &ref_o[row * kD], &ref_lse[row]);
      }
    });
  for (std::thread& t : pool) t.join();
  for (unsigned long long row = 0; row < static_cast<unsigned long long>(B) * Hq; ++row) {
    const double vs = v_scale_of(kHashed, static_cast<int>(row % Hq) / G);
    for (int d = 0; d < kD; ++d) {
      const double e = std::fabs(static_cast<double>(o[row * kD + d]) - ref_o[row * kD + d]) / vs;
      if (!(e <= res->max_err)) res->max_err = e;  // a NaN sticks
      if (!(e <= kOBoundPerVScale) && res->o_errors[kHashed]++ == 0) res->first_bad[kHashed] = row * kD + d;
    }
    const double e = std::fabs(static_cast<double>(lse[row]) - ref_lse[row]);
    if (!(e <= res->max_lse_err)) res->max_lse_err = e;
    if (!lse_within(lse[row], ref_lse[row]) && res->lse_errors[kHashed]++ == 0) res->first_bad_lse[kHashed] = row;
  }
}

// a shape the check's own data is defined for
bool data_shape_ok(int B, int Hq, int Hkv, int seq) { return seq >= 1 && seq <= kMaxSeq && shape_ok(B, Hq, Hkv, 1, pages_of(seq)); }

}  // namespace

extern "C" {

int amdgpu_decode8_sizeof(int which) { return which == 0 ? static_cast<int>(sizeof(amdgpu_decode8_result)) : -1; }

int amdgpu_decode8_describe(const amdgpu_decode8_result* r, char* buf, int len) { return describe(*r, buf, len); }

int amdgpu_decode8_operands(int set, int B, int Hq, int Hkv, int seq, unsigned short* q, unsigned char* k_cache,
                            unsigned char* v_cache, float* k_scale, float* v_scale, int* block_table, int* seq_lens) {
  if (set < 0 || set >= kDecodeSets || !data_shape_ok(B, Hq, Hkv, seq)) return -1;
  const int max_pages = pages_of(seq);
  decode::check_table(B, seq, block_table, seq_lens);
  for (size_t e = 0; e < static_cast<size_t>(B) * max_pages * Hkv * kPage * kD; ++e) k_cache[e] = v_cache[e] = kPoison;
  for (int kvh = 0; kvh < Hkv; ++kvh) k_scale[kvh] = k_scale_of(set, kvh), v_scale[kvh] = v_scale_of(set, kvh);
  for (int b = 0; b < B; ++b) {
    for (int hq = 0; hq < Hq; ++hq)
      for (int d = 0; d < kD; ++d) q[(static_cast<size_t>(b) * Hq + hq) * kD + d] = decode::bf16_bits(q_val(set, b, hq, d));
    for (int kvh = 0; kvh < Hkv; ++kvh)
      for (int j = 0; j < seq_lens[b]; ++j) {
        const int page = block_table[static_cast<size_t>(b) * max_pages + j / kPage];
        const size_t at = ((static_cast<size_t>(page) * Hkv + kvh) * kPage + j % kPage) * kD;
        for (int d = 0; d < kD; ++d) k_cache[at + d] = k_code(set, b, kvh, j, d), v_cache[at + d] = v_code(set, b, kvh, j, d);
      }
  }
  return 0;
}

int amdgpu_decode8_expected(int set, int B, int Hq, int Hkv, int seq, float* o, double* lse) {
  if ((set != kUniform && set != kRouted) || !data_shape_ok(B, Hq, Hkv, seq)) return -1;
  for (int b = 0; b < B; ++b)
    for (int hq = 0; hq < Hq; ++hq) {
      const int len = decode::check_len(b, seq), kvh = hq / (Hq / Hkv);
      const Top top = decode::top_of(set, b, hq, len);
      for (int d = 0; d < kD; ++d)
        o[(static_cast<size_t>(b) * Hq + hq) * kD + d] =
            expected_o(decode::top_sum(set, b, hq, kvh, d, top, len), top, v_scale_of(set, kvh));
      lse[static_cast<size_t>(b) * Hq + hq] = expected_lse(top, k_scale_of(set, kvh));
    }
  return 0;
}

int amdgpu_decode8_run(int device, const unsigned short* q, const unsigned char* k_cache, const unsigned char* v_cache,
                       const float* k_scale, const float* v_scale, const int* block_table, const int* seq_lens, float* o,
                       float* lse, int B, int Hq, int Hkv, int P, int max_pages, int splits, char* err, int err_len) {
  if (refuse(B, Hq, Hkv, P, max_pages, splits, block_table, seq_lens, k_scale, v_scale, err, err_len) != 0) return -1;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = seq_lens[b] > longest ? seq_lens[b] : longest;
  Status st;
  Decode8Buffers buf;
  CANARY_HIP(st, hipSetDevice(device));
  splits = resolve_splits(st, device, splits, B, Hkv, longest);
  buf.alloc(st, device, B, Hq, Hkv, P, max_pages, splits);
  CANARY_HIP(st, buf.q.upload(q));
  CANARY_HIP(st, buf.k.upload(k_cache));
  CANARY_HIP(st, buf.v.upload(v_cache));
  CANARY_HIP(st, buf.k_scale.upload(k_scale));
  CANARY_HIP(st, buf.v_scale.upload(v_scale));
  CANARY_HIP(st, buf.table.upload(block_table));
  CANARY_HIP(st, buf.lens.upload(seq_lens));
  if (st.ok()) {
    buf.launch();
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, buf.o.download(o));
  CANARY_HIP(st, buf.lse.download(lse));
  return st.report("decode8 path: ", err, err_len);
}

int amdgpu_decode8_check(int device, int B, int Hq, int Hkv, int seq, int splits, int iters, int flags,
                         amdgpu_decode8_result* result, char* err, int err_len) {
  *result = amdgpu_decode8_result();
  if (B == 0) B = kDecode8DefaultBatch;
  if (Hq == 0) Hq = Hkv ? Hkv : kDecode8DefaultQHeads;
  if (Hkv == 0) Hkv = Hq % kDecode8DefaultKvHeads == 0 && Hq / kDecode8DefaultKvHeads <= 16 ? kDecode8DefaultKvHeads : Hq;
  if (seq == 0) seq = kDecode8DefaultSeq;
  if (seq < 1 || seq > kMaxSeq || iters < 1) {
    std::snprintf(err, err_len, "decode8 path: seq %d, iters %d does not fit (seq 1 .. %d, iters at least 1)", seq, iters, kMaxSeq);
    return -1;
  }
  const int max_pages = pages_of(seq);
  const long long P = static_cast<long long>(B > 0 ? B : 0) * max_pages;
  std::vector<int> table, lens;
  std::vector<float> ones(Hkv > 0 && Hkv <= decode::kMaxHeads ? Hkv : 1, 1.f);  // the check's scales are its own
  if (P > 0 && P < (1ll << 28) && shape_ok(B, Hq, Hkv, static_cast<int>(P), max_pages)) {
    table.resize(static_cast<size_t>(P)), lens.resize(B);
    decode::check_table(B, seq, table.data(), lens.data());
  }
  if (refuse(B, Hq, Hkv, static_cast<int>(P < (1ll << 28) ? P : 0), max_pages, splits, table.data(), lens.data(), ones.data(),
             ones.data(), err, err_len) != 0)
    return -1;
  Status st;
  Decode8Buffers buf;
  DeviceBuffer<unsigned long long> d_counts;
  Events<2> ev;
  CANARY_HIP(st, hipSetDevice(device));
  splits = resolve_splits(st, device, splits, B, Hkv, seq);
  result->batch = B, result->q_heads = Hq, result->kv_heads = Hkv, result->seq = seq;
  result->splits = splits, result->iters = iters;
  buf.alloc(st, device, B, Hq, Hkv, static_cast<int>(P), max_pages, splits);
  CANARY_HIP(st, d_counts.alloc(4 * sizeof(unsigned long long)));
  CANARY_HIP(st, ev.create());
  CANARY_HIP(st, buf.table.upload(table.data()));
  CANARY_HIP(st, buf.lens.upload(lens.data()));
  CANARY_HIP(st, buf.k.fill(kPoison));  // NaN wherever no visible key lies: the rest of a last page, unused pages
  CANARY_HIP(st, buf.v.fill(kPoison));
  const size_t rows = static_cast<size_t>(B) * Hq;
  double total_ms = 0, kv_bytes = 0;
  for (int b = 0; b < B; ++b) kv_bytes += 2.0 * pages_of(lens[b]) * Hkv * kPageBytes;
  for (int set = 0; set < kDecodeSets; ++set) {
    unsigned long long counts[4] = {0, 0, ~0ull, ~0ull};
    float ms[1] = {0};
    CANARY_HIP(st, d_counts.upload(counts));
    if (st.ok()) {
      hipLaunchKernelGGL(kv8_fill, dim3(2048), dim3(256), 0, 0, buf.q.get(), buf.k.get(), buf.v.get(), buf.k_scale.get(),
                         buf.v_scale.get(), buf.table.get(), buf.lens.get(), set, B, Hq, Hkv, max_pages, seq);
      buf.launch();  // warm-up
      st.check(hipGetLastError());
    }
    time_stages(st, ev, ms, [&](int) {
      for (int i = 0; i < iters; ++i) buf.launch();
      return hipSuccess;
    });
    CANARY_HIP(st, buf.o.fill(0xFF));  // the poison: what is verified below was written after it
    CANARY_HIP(st, buf.lse.fill(0xFF));
    if (st.ok() && !(flags & kDecode8SkipVerifiedLaunch)) {
      buf.launch();
      st.check(hipGetLastError());
    }
    if (flags & kDecode8Inject) {
      const float junk = 12345.0f;
      CANARY_HIP(st, hipMemcpy(buf.o.get() + (static_cast<size_t>(B / 2) * Hq + Hq - 1) * kD + 5, &junk, 4, hipMemcpyHostToDevice));
    }
    if (set != kHashed) {
      if (st.ok()) {
        hipLaunchKernelGGL(kv8_verify, dim3(B * Hq), dim3(kD), 0, 0, buf.o.get(), buf.lse.get(), buf.lens.get(), set, Hq, Hkv,
                           d_counts.get());
        st.check(hipGetLastError());
      }
      CANARY_HIP(st, hipDeviceSynchronize());
      CANARY_HIP(st, d_counts.download(counts));
      result->o_errors[set] = counts[0], result->lse_errors[set] = counts[1];
      result->first_bad[set] = counts[2], result->first_bad_lse[set] = counts[3];
    } else {
      std::vector<float> o(rows * kD), lse(rows);
      CANARY_HIP(st, hipDeviceSynchronize());
      CANARY_HIP(st, buf.o.download(o.data()));
      CANARY_HIP(st, buf.lse.download(lse.data()));
      result->first_bad[set] = result->first_bad_lse[set] = ~0ull;
      if (st.ok()) judge_hashed(o, lse, lens, B, Hq, Hkv, result);
    }
    result->ms[set] = ms[0];
    total_ms += ms[0];
  }
  if (st.ok() && total_ms > 0) result->kv_gbps = kv_bytes * iters * kDecodeSets / (total_ms * 1e-3) / 1e9;
  return st.report("decode8 path: ", err, err_len);
}

}  // extern "C"
