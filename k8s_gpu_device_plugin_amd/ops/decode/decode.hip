// MI355X (gfx950 / CDNA4) health canary: the decode-attention path (paged KV cache, GQA, split-KV).
//
// o[B][Hq][128] (fp32) = softmax(q k^T / sqrt(128)) v over the first seq_lens[b] keys of sequence b
// and lse[B][Hq]: one query token per sequence, G = Hq / Hkv query heads sharing one KV head, K and
// V scattered over pages of 16 keys behind a block table, the key range split over workgroups and
// merged afterwards.  What an inference container spends its time in and no other check runs: page
// ids fetched from memory and turned into the source addresses of the LDS DMA, KV streamed through
// LDS with no reuse, a ragged tail masked in the middle of a page, and partial softmax states merged
// twice, through LDS and through HBM, empty ones included.
//
// decode_split: one workgroup of 4 waves per (sequence, KV head, partition).
//   * Work split: a partition is tiles_per_split 128-key tiles.  In every tile wave w owns keys
//     32 w .. 32 w + 31 (pages 2 w and 2 w + 1) from the DMA to the accumulators; it never touches
//     another wave's keys, and its loop ends at its own last visible tile.
//   * LDS: 128 KiB, one __shared__ object, one workgroup per CU.  Wave w's slice is 32 KiB: two
//     stages of a K image and a V image of [32][256 B].  Logical 16 B chunk c of row r sits at
//     physical chunk c ^ ((r >> 1) & 7) (the bf16 kernels' swizzle), applied on the global source
//     address.  A page is 4 pieces of 1 KiB of K and 4 of V (global_load_lds, 16 B per lane) whose
//     source is cache + ((table[b][page] * Hkv + kvh) * 16 + row) * 256; the two table entries of
//     the next tile are loaded a tile ahead.  Pages at or past ceil(len / 16) are neither looked up
//     nor staged.  Producer and consumer are the same wave: s_waitcnt vmcnt(0), no barrier in the loop.
//   * Scores: S^T[32 keys][32 queries] = K Q^T, 8 v_mfma_f32_32x32x16_bf16.  A is K (row r, chunk
//     2 s + h), B is Q^T: query row r < G from global memory, zero for r >= G.  Scaled in fp32 by
//     log2(e) / sqrt(128); keys >= len become -inf (only on a wave's ragged tile).
//   * Softmax, base 2, per wave, as attn_fwd: in-register max and sum of the lane's 16 scores and one
//     v_permlane32_swap each; alpha = 2^(m_old - m_new); p by v_exp_f32; l from the unrounded p.  A
//     wave computes a tile only if its first key is visible, so m_new is finite: no (-inf) - (-inf).
//   * Second product: O^T[128 d][32 queries] += V^T P^T, 2 key steps x 4 d-blocks, P packed by
//     v_cvt_pk_bf16_f32, V read by ds_read_b64_tr_b16 (attn_fwd's map), 64 accumulators per lane.
//     On a ragged tile the V elements of keys >= len are zeroed: the rest of a last page is
//     whatever the cache holds, and 0 x NaN is NaN.
//   * Merge: each wave writes (m, l, acc) of its G rows into its own slice, one barrier, then the 4
//     states are merged (m = max, weights 2^(m_w - m), 0 for an empty wave) by all 256 threads over
//     (row, d) and stored unnormalised to the workspace [B][Hq][splits].
// decode_combine: one wave per (sequence, query head), two d per lane: merges the `splits` states by
// the same rule, skipping empty ones, divides by l (correctly rounded) and writes o and lse.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/decode.py): decode.h.
#include "decode.h"

#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

namespace {

using namespace canary;
using namespace decode;

typedef __attribute__((address_space(3))) void* lds_void_ptr;
using i16x4 = __attribute__((ext_vector_type(4))) short;
typedef __attribute__((address_space(3))) i16x4* lds_i16x4_ptr;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int kRowBytes = kD * 2;           // 256 B: a row of K or V
constexpr int kImage = 32 * kRowBytes;      // a wave's 32 keys of K or of V: 8 KiB
constexpr int kStage = 2 * kImage;          // K + V of one tile
// Stages of a wave's slice.  2 is the design: 32 KiB per wave, one workgroup per CU, tile t + 1 in
// flight while tile t is computed.  1 is the alternative it was measured against (docs/CANARY.md, "The
// decode-attention path / Measured"): 16 KiB per wave, two workgroups per CU, the next tile issued
// after the compute; -DDECODE_STAGES=1 builds it.
#ifndef DECODE_STAGES
#define DECODE_STAGES 2
#endif
constexpr int kStages = DECODE_STAGES;
static_assert(kStages == 1 || kStages == 2, "one or two stages");
constexpr int kSlice = kStages * kStage;    // a wave's stages: 32 KiB
constexpr int kStateMl = 16 * kD * 4;       // a wave's merge state in its slice: acc [16][128], then (m, l) [16]
constexpr float kScaleLog2e = 0.12751743074602467f;  // log2(e) / sqrt(128)
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ int swizzled_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// Logical 16 B chunk `chunk` of row `row` of an image as a bf16 operand: one ds_read_b128.
__device__ __forceinline__ bf16x8 frag16(const char* S, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(S + row * kRowBytes + (swizzled_chunk(row, chunk) << 4));
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

// 2^(m_w - m), and exactly 0 for a state that saw no key (m_w = -inf, also when m is)
__device__ __forceinline__ float merge_weight(float m_w, float m) {
  return m_w == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_w - m);
}

__global__ void __launch_bounds__(256) decode_split(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kc,
                                                    const uint16_t* __restrict__ Vc, const int* __restrict__ table,
                                                    const int* __restrict__ lens, float* __restrict__ ws_acc,
                                                    float* __restrict__ ws_ml, int B, int Hq, int Hkv, int max_pages, int splits) {
#pragma clang fp contract(off)  // s * scale - m as two roundings: m is one of the s * scale
  __shared__ __attribute__((aligned(16))) char smem[4 * kSlice];  // the only LDS object: [wave][stage][K|V][32][256 B]
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

  const char* Kb = reinterpret_cast<const char*>(Kc);
  const char* Vb = reinterpret_cast<const char*>(Vc);
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
  // ... and its 32 keys of K and of V into stage `buf`: 4 pieces (4 rows, 1 KiB) of each per page
  auto stage = [&](int t, int buf, const int (&e)[2]) {
    char* base = slice + buf * kStage;
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      if (8 * t + 2 * wave + ph >= npages) continue;  // wave-uniform
      const size_t page = (static_cast<size_t>(e[ph]) * Hkv + kvh) * kPageBytes;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * ph + 4 * i + (lane >> 4), cb = swizzled_chunk(row, lane & 15) << 4;
        const size_t src = page + (row & 15) * kRowBytes + cb;
        __builtin_amdgcn_global_load_lds(Kb + src, (lds_void_ptr)(base + (4 * ph + i) * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(Vb + src, (lds_void_ptr)(base + kImage + (4 * ph + i) * 1024), 16, 0, 0);
      }
    }
  };
  int ent[2];
  if (t0 < t_end) {
    lookup(t0, ent);
    stage(t0, 0, ent);
    lookup(t0 + 1, ent);
  }

  // Query row r < G of this KV head as the B operand of every score MFMA: chunk 2 s + h for d-step s.
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (r < G) {
    const bf16x8* qp = reinterpret_cast<const bf16x8*>(Q + (static_cast<size_t>(b) * Hq + kvh * G + r) * kD);
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = qp[2 * s + h];
  }

  // The lane's two transposed-read addresses within a 16-key step of a V image, per d-block db and
  // half u: it names row 8 u + 4 (g >> 1) + q, columns 32 db + 16 (g & 1) + 4 p .. + 3 (8 B).
  int vaddr[2][4];
  {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const int row = 8 * u + 4 * (g >> 1) + q, col = 32 * db + 16 * (g & 1) + 4 * p;
        // (row + 16 t) >> 1 & 7 does not depend on the step t, so the swizzle is the row's own
        vaddr[u][db] = row * kRowBytes + (swizzled_chunk(row, col >> 3) << 4) + (col & 7) * 2;
      }
  }

  f32x16 acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[db][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int t = t0; t < t_end; ++t) {
    const int cur = (t - t0) & (kStages - 1), k0 = t * kTile + 32 * wave;  // the wave's first key of the tile: visible
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // tile t has landed
    if (kStages == 2 && t + 1 < t_end) {                       // tile t - 1's stage is free: this wave read it
      stage(t + 1, cur ^ 1, ent);
      lookup(t + 2, ent);
    }
    const char* Ks = slice + cur * kStage;
    const char* Vs = Ks + kImage;
    const bool ragged = k0 + 32 > len;
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
    for (int st = 0; st < 8; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag16(Ks, r, 2 * st + h), qf[st], s, 0, 0, 0);
    float mt = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float x = s[e] * kScaleLog2e;
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
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(lds_void_ptr)(Vt + vaddr[0][db]));
        const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(lds_void_ptr)(Vt + vaddr[1][db]));
        bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        if (ragged) {  // element j is key 16 t2 + 4 h + 8 (j >> 2) + (j & 3) of the wave's 32
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (k0 + 16 * t2 + 4 * h + 8 * (j >> 2) + (j & 3) >= len) vf[j] = 0;
        }
        acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, acc[db], 0, 0, 0);
      }
    }
    if (kStages == 1 && t + 1 < t_end) {  // the only stage is free now
      stage(t + 1, 0, ent);
      lookup(t + 2, ent);
    }
  }

  // The wave's state of its G rows into its own slice (its stages are free: the last tile was waited
  // for and read), one barrier, then every thread merges the 4 states of (row, d) pairs.
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

// One wave per (sequence, query head): lane i holds d = 2 i, 2 i + 1.
__global__ void __launch_bounds__(256) decode_combine(const float* __restrict__ ws_acc, const float* __restrict__ ws_ml,
                                                      float* __restrict__ O, float* __restrict__ L, int rows, int splits) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows || splits < 1 || splits > kMaxSplits) return;
  const float* ml = ws_ml + static_cast<size_t>(row) * splits * 2;
  const float* part = ws_acc + static_cast<size_t>(row) * splits * kD + 2 * lane;
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
  *reinterpret_cast<f32x2*>(O + static_cast<size_t>(row) * kD + 2 * lane) = f32x2{a[0] / l, a[1] / l};
  if (lane == 0) L[row] = kLn2 * (m + log2f(l));
}

// ---- the check's data and its verifier --------------------------------------------------------
// The visible keys of every sequence through the block table; the caches were poisoned before.
__global__ void __launch_bounds__(256) decode_fill(uint16_t* __restrict__ Q, uint16_t* __restrict__ Kc, uint16_t* __restrict__ Vc,
                                                   const int* __restrict__ table, const int* __restrict__ lens, int set, int B,
                                                   int Hq, int Hkv, int max_pages, int seq) {
  const size_t nq = static_cast<size_t>(B) * Hq * kD, nk = static_cast<size_t>(B) * Hkv * seq * kD;
  const size_t first = blockIdx.x * 256ull + threadIdx.x, step = static_cast<size_t>(gridDim.x) * 256;
  for (size_t e = first; e < nq; e += step) {
    const int d = e % kD, hq = (e / kD) % Hq, b = e / kD / Hq;
    Q[e] = bf16_bits(q_val(set, b, hq, d));
  }
  for (size_t e = first; e < nk; e += step) {
    const int d = e % kD, j = (e / kD) % seq, kvh = (e / kD / seq) % Hkv, b = e / kD / seq / Hkv;
    if (j >= lens[b]) continue;
    const int page = table[static_cast<size_t>(b) * max_pages + j / kPage];
    const size_t at = ((static_cast<size_t>(page) * Hkv + kvh) * kPage + j % kPage) * kD + d;
    Kc[at] = bf16_bits(k_val(set, b, kvh, j, d));
    Vc[at] = bf16_bits(static_cast<float>(v_val(set, b, kvh, j, d)));
  }
}

// counts[0] wrong elements of o, [1] wrong lse values, [2] / [3] the smallest index of each.
// One block per (sequence, head) of an exact set, one thread per d: the bits of o against one IEEE
// division of the closed form, so a NaN, an Inf and a -0 for a +0 all count.
__global__ void __launch_bounds__(kD) decode_verify(const float* __restrict__ O, const float* __restrict__ L,
                                                    const int* __restrict__ lens, int set, int Hq, int Hkv,
                                                    unsigned long long* __restrict__ counts) {
  const int b = blockIdx.x / Hq, hq = blockIdx.x % Hq, d = threadIdx.x, len = lens[b];
  const Top top = top_of(set, b, hq, len);
  const float want = expected_o(top_sum(set, b, hq, hq / (Hq / Hkv), d, top, len), top);
  const size_t at = static_cast<size_t>(blockIdx.x) * kD + d;
  const bool bad = __builtin_bit_cast(uint32_t, O[at]) != __builtin_bit_cast(uint32_t, want);
  if (bad) atomicMin(counts + 2, static_cast<unsigned long long>(at));
  block_add_errors(bad, counts);
  if (d == 0 && !lse_within(L[blockIdx.x], expected_lse(top))) {
    atomicAdd(counts + 1, 1ull);
    atomicMin(counts + 3, static_cast<unsigned long long>(blockIdx.x));
  }
}

// The device side of one decode attention: the operands, the workspace of the partial states, o and lse.
struct DecodeBuffers {
  DeviceBuffer<uint16_t> q, k, v;
  DeviceBuffer<int> table, lens;
  DeviceBuffer<float> ws_acc, ws_ml, o, lse;
  int B = 0, Hq = 0, Hkv = 0, max_pages = 0, splits = 0;
  void alloc(Status& st, int device, int B_, int Hq_, int Hkv_, int P, int max_pages_, int splits_) {
    B = B_, Hq = Hq_, Hkv = Hkv_, max_pages = max_pages_, splits = splits_;
    const size_t rows = static_cast<size_t>(B) * Hq, cache = static_cast<size_t>(P) * Hkv * kPageBytes;
    CANARY_HIP(st, hipSetDevice(device));
    CANARY_HIP(st, q.alloc(rows * kD * 2));
    CANARY_HIP(st, k.alloc(cache));
    CANARY_HIP(st, v.alloc(cache));
    CANARY_HIP(st, table.alloc(static_cast<size_t>(B) * max_pages * 4));
    CANARY_HIP(st, lens.alloc(static_cast<size_t>(B) * 4));
    CANARY_HIP(st, ws_acc.alloc(rows * splits * kD * 4));
    CANARY_HIP(st, ws_ml.alloc(rows * splits * 2 * 4));
    CANARY_HIP(st, o.alloc(rows * kD * 4));
    CANARY_HIP(st, lse.alloc(rows * 4));
  }
  void launch() const {  // the pair
    hipLaunchKernelGGL(decode_split, dim3(B * Hkv * splits), dim3(256), 0, 0, q.get(), k.get(), v.get(), table.get(), lens.get(),
                       ws_acc.get(), ws_ml.get(), B, Hq, Hkv, max_pages, splits);
    hipLaunchKernelGGL(decode_combine, dim3((B * Hq + 3) / 4), dim3(256), 0, 0, ws_acc.get(), ws_ml.get(), o.get(), lse.get(),
                       B * Hq, splits);
  }
};

// splits = 0: at least four workgroups per CU of the device (two per CU measured 5 % slower: with one
// resident workgroup per CU and lengths between seq / 2 and seq, more and shorter workgroups even out the tail)
int resolve_splits(Status& st, int device, int splits, int B, int Hkv, int longest) {
  if (splits) return splits;
  hipDeviceProp_t prop;
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  return st.ok() ? choose_splits(B, Hkv, longest, 4 * prop.multiProcessorCount) : 1;
}

// The hashed set's verdict on downloaded o and lse: every (sequence, head) against float64, the
// (sequence, KV head) groups shared among up to 16 host threads.
void judge_hashed(const std::vector<float>& o, const std::vector<float>& lse, const std::vector<int>& lens, int B, int Hq, int Hkv,
                  amdgpu_decode_result* res) {
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
    for (int d = 0; d < kD; ++d) {
      const double e = std::fabs(static_cast<double>(o[row * kD + d]) - ref_o[row * kD + d]);
      if (!(e <= res->max_err)) res->max_err = e;  // a NaN sticks
      if (!(e <= kOBound) && res->o_errors[kHashed]++ == 0) res->first_bad[kHashed] = row * kD + d;
    }
    const double e = std::fabs(static_cast<double>(lse[row]) - ref_lse[row]);
    if (!(e <= res->max_lse_err)) res->max_lse_err = e;
    if (!lse_within(lse[row], ref_lse[row]) && res->lse_errors[kHashed]++ == 0) res->first_bad_lse[kHashed] = row;
  }
}

}  // namespace

extern "C" {

int amdgpu_decode_sizeof(int which) { return which == 0 ? static_cast<int>(sizeof(amdgpu_decode_result)) : -1; }

int amdgpu_decode_describe(const amdgpu_decode_result* r, char* buf, int len) { return describe(*r, buf, len); }

int amdgpu_decode_operands(int set, int B, int Hq, int Hkv, int seq, unsigned short* q, unsigned short* k_cache,
                           unsigned short* v_cache, int* block_table, int* seq_lens) {
  if (set < 0 || set >= kDecodeSets || seq < 1 || seq > kMaxSeq || !shape_ok(B, Hq, Hkv, 1, pages_of(seq))) return -1;
  const int max_pages = pages_of(seq);
  check_table(B, seq, block_table, seq_lens);
  for (size_t e = 0; e < static_cast<size_t>(B) * max_pages * Hkv * kPage * kD; ++e) k_cache[e] = v_cache[e] = 0xFFFF;
  for (int b = 0; b < B; ++b) {
    for (int hq = 0; hq < Hq; ++hq)
      for (int d = 0; d < kD; ++d) q[(static_cast<size_t>(b) * Hq + hq) * kD + d] = bf16_bits(q_val(set, b, hq, d));
    for (int kvh = 0; kvh < Hkv; ++kvh)
      for (int j = 0; j < seq_lens[b]; ++j) {
        const int page = block_table[static_cast<size_t>(b) * max_pages + j / kPage];
        const size_t at = ((static_cast<size_t>(page) * Hkv + kvh) * kPage + j % kPage) * kD;
        for (int d = 0; d < kD; ++d) {
          k_cache[at + d] = bf16_bits(k_val(set, b, kvh, j, d));
          v_cache[at + d] = bf16_bits(static_cast<float>(v_val(set, b, kvh, j, d)));
        }
      }
  }
  return 0;
}

int amdgpu_decode_expected(int set, int B, int Hq, int Hkv, int seq, float* o, double* lse) {
  if ((set != kUniform && set != kRouted) || seq < 1 || seq > kMaxSeq || !shape_ok(B, Hq, Hkv, 1, pages_of(seq))) return -1;
  for (int b = 0; b < B; ++b)
    for (int hq = 0; hq < Hq; ++hq) {
      const int len = check_len(b, seq);
      const Top top = top_of(set, b, hq, len);
      for (int d = 0; d < kD; ++d)
        o[(static_cast<size_t>(b) * Hq + hq) * kD + d] = expected_o(top_sum(set, b, hq, hq / (Hq / Hkv), d, top, len), top);
      lse[static_cast<size_t>(b) * Hq + hq] = expected_lse(top);
    }
  return 0;
}

int amdgpu_decode_run(int device, const unsigned short* q, const unsigned short* k_cache, const unsigned short* v_cache,
                      const int* block_table, const int* seq_lens, float* o, float* lse, int B, int Hq, int Hkv, int P,
                      int max_pages, int splits, char* err, int err_len) {
  if (refuse(B, Hq, Hkv, P, max_pages, splits, block_table, seq_lens, err, err_len) != 0) return -1;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = seq_lens[b] > longest ? seq_lens[b] : longest;
  Status st;
  DecodeBuffers buf;
  CANARY_HIP(st, hipSetDevice(device));
  splits = resolve_splits(st, device, splits, B, Hkv, longest);
  buf.alloc(st, device, B, Hq, Hkv, P, max_pages, splits);
  CANARY_HIP(st, buf.q.upload(q));
  CANARY_HIP(st, buf.k.upload(k_cache));
  CANARY_HIP(st, buf.v.upload(v_cache));
  CANARY_HIP(st, buf.table.upload(block_table));
  CANARY_HIP(st, buf.lens.upload(seq_lens));
  if (st.ok()) {
    buf.launch();
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, buf.o.download(o));
  CANARY_HIP(st, buf.lse.download(lse));
  return st.report("decode path: ", err, err_len);
}

int amdgpu_decode_check(int device, int B, int Hq, int Hkv, int seq, int splits, int iters, int flags,
                        amdgpu_decode_result* result, char* err, int err_len) {
  *result = amdgpu_decode_result();
  if (B == 0) B = kDecodeDefaultBatch;
  if (Hq == 0) Hq = Hkv ? Hkv : kDecodeDefaultQHeads;
  if (Hkv == 0) Hkv = Hq % kDecodeDefaultKvHeads == 0 && Hq / kDecodeDefaultKvHeads <= 16 ? kDecodeDefaultKvHeads : Hq;
  if (seq == 0) seq = kDecodeDefaultSeq;
  if (seq < 1 || seq > kMaxSeq || iters < 1) {
    std::snprintf(err, err_len, "decode path: seq %d, iters %d does not fit (seq 1 .. %d, iters at least 1)", seq, iters, kMaxSeq);
    return -1;
  }
  const int max_pages = pages_of(seq);
  const long long P = static_cast<long long>(B > 0 ? B : 0) * max_pages;
  std::vector<int> table, lens;
  if (P > 0 && P < (1ll << 28) && shape_ok(B, Hq, Hkv, static_cast<int>(P), max_pages)) {
    table.resize(static_cast<size_t>(P)), lens.resize(B);
    check_table(B, seq, table.data(), lens.data());
  }
  if (refuse(B, Hq, Hkv, static_cast<int>(P < (1ll << 28) ? P : 0), max_pages, splits, table.data(), lens.data(), err, err_len) != 0)
    return -1;
  Status st;
  DecodeBuffers buf;
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
  CANARY_HIP(st, buf.k.fill(0xFF));  // NaN wherever no visible key lies: the rest of a last page, unused pages
  CANARY_HIP(st, buf.v.fill(0xFF));
  const size_t rows = static_cast<size_t>(B) * Hq;
  double total_ms = 0, kv_bytes = 0;
  for (int b = 0; b < B; ++b) kv_bytes += 2.0 * pages_of(lens[b]) * Hkv * kPageBytes;
  for (int set = 0; set < kDecodeSets; ++set) {
    unsigned long long counts[4] = {0, 0, ~0ull, ~0ull};
    float ms[1] = {0};
    CANARY_HIP(st, d_counts.upload(counts));
    if (st.ok()) {
      hipLaunchKernelGGL(decode_fill, dim3(2048), dim3(256), 0, 0, buf.q.get(), buf.k.get(), buf.v.get(), buf.table.get(),
                         buf.lens.get(), set, B, Hq, Hkv, max_pages, seq);
      buf.launch();  // warm-up
      st.check(hipGetLastError());
    }
    time_stages(st, ev, ms, [&](int) {
      for (int i = 0; i < iters; ++i) buf.launch();
      return hipSuccess;
    });
    CANARY_HIP(st, buf.o.fill(0xFF));  // the poison: what is verified below was written after it
    CANARY_HIP(st, buf.lse.fill(0xFF));
    if (st.ok() && !(flags & kDecodeSkipVerifiedLaunch)) {
      buf.launch();
      st.check(hipGetLastError());
    }
    if (flags & kDecodeInject) {
      const float junk = 12345.0f;
      CANARY_HIP(st, hipMemcpy(buf.o.get() + (static_cast<size_t>(B / 2) * Hq + Hq - 1) * kD + 5, &junk, 4, hipMemcpyHostToDevice));
    }
    if (set != kHashed) {
      if (st.ok()) {
        hipLaunchKernelGGL(decode_verify, dim3(B * Hq), dim3(kD), 0, 0, buf.o.get(), buf.lse.get(), buf.lens.get(), set, Hq, Hkv,
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
  return st.report("decode path: ", err, err_len);
}

}  // extern "C"
