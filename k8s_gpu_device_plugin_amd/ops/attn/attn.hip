// MI355X (gfx950 / CDNA4) health canary: the attention path (fused bf16 flash attention, forward).
//
// O[H][Sq][128] (fp32) = softmax(Q K^T / sqrt(128)) V and lse[H][Sq], bf16 in, fp32 accumulation.
// The path every fused attention kernel takes and no other check runs: two chained MFMAs with the
// C/D registers of the first feeding an operand of the second, a row maximum and a row sum across
// lanes, v_exp_f32 on the critical path, an fp32 -> bf16 pack between the MFMAs, a running rescale
// of the accumulators, and V read from LDS across its rows.
//
// attn_fwd, both products transposed so that a lane owns one query from the scores to the store:
//   * Work split: one workgroup of 4 waves takes 128 queries of one head, a wave 32 of them.  K and
//     V stream through in tiles of 64 keys.  Workgroups are remapped with the bijective xcd_remap,
//     heads outermost, so the query blocks that share one head's K and V share an XCD's L2; within
//     a head the last query block comes first (under a causal mask it has the most tiles).
//   * LDS: a K tile and a V tile are [64][256 B] images, two buffers of each: 64 KiB, one
//     __shared__ object, two workgroups per CU.  Logical 16 B chunk c of row r sits at physical
//     chunk c ^ ((r >> 1) & 7) (swizzled_chunk, as in ops/gemm.hip; it permutes the low three bits
//     of the 16 chunks of a row), applied on the global source address because the DMA destination
//     must stay lane-linear.  A wave issues 4 pieces (4 rows, 1 KiB) of K and 4 of V per tile with
//     __builtin_amdgcn_global_load_lds, 16 B per lane; tile t+1 lands while tile t is computed;
//     s_waitcnt vmcnt(0) and a barrier close each tile.
//   * Scores: S^T[keys][queries] = K Q^T on v_mfma_f32_32x32x16_bf16.  A is K: lane l (r = l & 31,
//     h = l >> 5) reads row 32 kb + r, logical chunk 2 s + h for d-step s, one ds_read_b128.  B is
//     Q^T: the lane's query row, chunk 2 s + h, loaded once from global memory into 32 VGPRs.  Q
//     is not pre-scaled (log2(e) / sqrt(128) times 64 is not a bf16); the scores are scaled in
//     fp32.  In C/D (cd_row32) the lane then holds query r and keys (e & 3) + 8 (e >> 2) + 4 h of
//     each 32-key block: 32 of the tile's 64 scores, the other 32 in lane l ^ 32.
//   * Softmax, base 2: row maximum and row sum are an in-register reduction and one
//     v_permlane32_swap.  alpha = 2^(m_old - m_new) is one scalar per lane; p = 2^(s - m_new) by
//     v_exp_f32; l = l alpha + sum p (the unrounded p).
//   * Second product: O^T[d][queries] += V^T P^T.  B is P^T: for step t (16 keys) the lane's
//     accumulators 8 (t & 1) .. + 7 of block t >> 1, packed to bf16 by v_cvt_pk_bf16_f32, so
//     element j of the operand is key 16 t + 4 h + 8 (j >> 2) + (j & 3).  A must hold the same keys
//     of column 32 db + r of V: two ds_read_b64_tr_b16, one per j >> 2.  In a 16-lane group g the
//     lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3 of the group's block and
//     lane i receives column i of rows 0 .. 3 (the map ops/ldspath measures: tr_source): here
//     row q is key 16 t + 8 (j >> 2) + 4 (g >> 1) + q and the block's columns are
//     32 db + 16 (g & 1) .. + 15, which is the lane's own h = g >> 1 and r = 16 (g & 1) + i.  The
//     key order fits, so no other read pattern is needed.  4 x 16 accumulators per lane.
//   * Masking: on tiles that cross the diagonal of the wave's 32 queries the hidden scores become
//     -inf; a wave skips tiles wholly above its diagonal (it still stages and meets the barrier),
//     and the workgroup's loop ends at its last visible tile.  Key 0 is visible to every query, so
//     m is finite after the first tile and no (-inf) - (-inf) arises.
//   * Epilogue: acc / l by the correctly rounded fp32 division, 4 consecutive d per 16 B store,
//     lse = ln2 (m + log2 l).
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/attn.py): attn.h.
#include "attn.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {

using namespace canary;
using namespace attn;

typedef __attribute__((address_space(3))) void* lds_void_ptr;
using i16x4 = __attribute__((ext_vector_type(4))) short;
typedef __attribute__((address_space(3))) i16x4* lds_i16x4_ptr;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int kRowBytes = kD * 2;             // 256 B: a row of K or V
constexpr int kImage = kBlockK * kRowBytes;   // one tile image: 16 KiB
constexpr int kStage = 2 * kImage;            // K + V of one tile
constexpr float kScaleLog2e = 0.12751743074602467f;  // log2(e) / sqrt(128)
constexpr float kLn2 = 0.6931471805599453f;

// gemm.hip's, which keeps them in an anonymous namespace
__host__ __device__ __forceinline__ int xcd_remap(int orig, int nwg) {  // bijective for any nwg
  const int xcd = orig % 8, q = nwg / 8, r = nwg % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}
__device__ __forceinline__ int swizzled_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// Logical 16 B chunk `chunk` of row `row` of a tile image as a bf16 operand: one ds_read_b128.
__device__ __forceinline__ bf16x8 frag16(const char* S, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(S + row * kRowBytes + (swizzled_chunk(row, chunk) << 4));
}

// max / sum of x with the value lane l ^ 32 holds: one v_permlane32_swap, no LDS.
__device__ __forceinline__ float with_other_half(float x, bool sum) {
  // The swap exchanges the upper half of its first register with the lower half of its second:
  // given x twice, the two results hold the own and the other lane's x, in either order.  Each
  // result is copied to a scalar first: __builtin_bit_cast applied to r[1] itself reads r[0].
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

__global__ void __launch_bounds__(256) attn_fwd(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K,
                                                const uint16_t* __restrict__ V, float* __restrict__ O,
                                                float* __restrict__ L, int H, int Sq, int Sk, int causal) {
#pragma clang fp contract(off)  // s * scale - m as two roundings: m is one of the s * scale
  __shared__ __attribute__((aligned(16))) char smem[2 * kStage];  // the only LDS object: [buf][K|V][64][256 B]

  // host checks shapes; never touch memory for one this kernel was not built for
  if (!shape_ok(H, Sq, Sk, causal) || static_cast<long long>(gridDim.x) != static_cast<long long>(H) * (Sq / kBlockQ)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nqb = Sq / kBlockQ, wg = xcd_remap(blockIdx.x, gridDim.x);
  const int head = wg / nqb, q0 = (nqb - 1 - wg % nqb) * kBlockQ, qw = q0 + 32 * wave;
  const int off = Sk - Sq, T = tiles_of_block(q0, Sq, Sk, causal);
  const char* Kh = reinterpret_cast<const char*>(K + static_cast<size_t>(head) * Sk * kD);
  const char* Vh = reinterpret_cast<const char*>(V + static_cast<size_t>(head) * Sk * kD);

  // Wave w issues pieces 4w .. 4w+3 (4 rows each) of K and of V.
  auto stage = [&](int t, int buf) {
    char* base = smem + buf * kStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = wave * 4 + i, row = piece * 4 + (lane >> 4), cb = swizzled_chunk(row, lane & 15) << 4;
      const size_t src = static_cast<size_t>(t * kBlockK + row) * kRowBytes + cb;
      __builtin_amdgcn_global_load_lds(Kh + src, (lds_void_ptr)(base + piece * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Vh + src, (lds_void_ptr)(base + kImage + piece * 1024), 16, 0, 0);
    }
  };
  stage(0, 0);

  // The lane's query row as the B operand of every score MFMA: chunk 2 s + h for d-step s.
  bf16x8 qf[8];
  {
    const bf16x8* qp = reinterpret_cast<const bf16x8*>(Q + (static_cast<size_t>(head) * Sq + qw + r) * kD);
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

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, k0 = t * kBlockK;
    if (t + 1 < T) stage(t + 1, cur ^ 1);
    if (!causal || k0 <= qw + 31 + off) {  // else the tile is wholly above this wave's diagonal
      const char* Ks = smem + cur * kStage;
      const char* Vs = Ks + kImage;
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
#pragma unroll
        for (int st = 0; st < 8; ++st)
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag16(Ks, 32 * kb + r, 2 * st + h), qf[st], s[kb], 0, 0, 0);
      }
      const bool diagonal = causal && k0 + kBlockK - 1 > qw + off;
      float mt = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float x = s[kb][e] * kScaleLog2e;
          if (diagonal && k0 + 32 * kb + cd_row32(e, h) > qw + r + off) x = -INFINITY;
          s[kb][e] = x;
          mt = fmaxf(mt, x);
        }
      const float m_new = fmaxf(m, with_other_half(mt, false));
      const float alpha = __builtin_amdgcn_exp2f(m - m_new);
      float lt = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          s[kb][e] = __builtin_amdgcn_exp2f(s[kb][e] - m_new);
          lt += s[kb][e];
        }
      l = l * alpha + with_other_half(lt, true);
      m = m_new;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[db][e] *= alpha;
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {  // 16 keys per step
        const f32x16& pt = s[t4 >> 1];
        const int e0 = 8 * (t4 & 1);
        const u32x4 packed = {pack_bf16(pt[e0 + 0], pt[e0 + 1]), pack_bf16(pt[e0 + 2], pt[e0 + 3]),
                              pack_bf16(pt[e0 + 4], pt[e0 + 5]), pack_bf16(pt[e0 + 6], pt[e0 + 7])};
        const bf16x8 pf = __builtin_bit_cast(bf16x8, packed);
        const char* Vt = Vs + t4 * 16 * kRowBytes;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(lds_void_ptr)(Vt + vaddr[0][db]));
          const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(lds_void_ptr)(Vt + vaddr[1][db]));
          const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, acc[db], 0, 0, 0);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 has landed
    __syncthreads();                                   // ... and nobody still reads tile t's buffer
  }

  float* out = O + (static_cast<size_t>(head) * Sq + qw + r) * kD;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int eg = 0; eg < 4; ++eg) {
      const f32x4 v = {acc[db][4 * eg] / l, acc[db][4 * eg + 1] / l, acc[db][4 * eg + 2] / l, acc[db][4 * eg + 3] / l};
      *reinterpret_cast<f32x4*>(out + 32 * db + 8 * eg + 4 * h) = v;  // d = 32 db + cd_row32(4 eg .. + 3, h)
    }
  if (h == 0) L[static_cast<size_t>(head) * Sq + qw + r] = kLn2 * (m + log2f(l));
}

// ---- the check's data and its verifier --------------------------------------------------------
__global__ void __launch_bounds__(256) attn_fill(uint16_t* __restrict__ Q, uint16_t* __restrict__ K, uint16_t* __restrict__ V,
                                                 int set, int H, int Sq, int Sk) {
  const size_t nq = static_cast<size_t>(H) * Sq * kD, nk = static_cast<size_t>(H) * Sk * kD;
  const size_t first = blockIdx.x * 256ull + threadIdx.x, step = static_cast<size_t>(gridDim.x) * 256;
  for (size_t e = first; e < nq; e += step) {
    const int d = e % kD, i = (e / kD) % Sq, head = e / kD / Sq;
    Q[e] = bf16_bits(q_val(set, head, i, d));
  }
  for (size_t e = first; e < nk; e += step) {
    const int d = e % kD, j = (e / kD) % Sk, head = e / kD / Sk;
    K[e] = bf16_bits(k_val(set, head, j, d));
    V[e] = bf16_bits(static_cast<float>(v_val(set, head, j, d)));
  }
}

// counts[0] wrong elements of O, [1] wrong lse values, [2] / [3] the smallest index of each.
// One block per (head, row) of an exact set, one thread per d: the bits of O against one IEEE
// division of the closed form, so a NaN, an Inf and a -0 for a +0 all count.
__global__ void __launch_bounds__(kD) attn_verify(const float* __restrict__ O, const float* __restrict__ L, int set, int H,
                                                  int Sq, int Sk, int causal, unsigned long long* __restrict__ counts) {
  const int head = blockIdx.x / Sq, i = blockIdx.x % Sq, d = threadIdx.x;
  const Top top = top_of(set, i, Sq, Sk, causal);
  const float want = expected_o(top_sum(set, head, i, d, top, Sq, Sk, causal), top);
  const size_t at = static_cast<size_t>(blockIdx.x) * kD + d;
  const bool bad = __builtin_bit_cast(uint32_t, O[at]) != __builtin_bit_cast(uint32_t, want);
  if (bad) atomicMin(counts + 2, static_cast<unsigned long long>(at));
  block_add_errors(bad, counts);
  if (d == 0) {
    const double ref = log(static_cast<double>(top.count)) + (top.matching ? 4096.0 / sqrt(128.0) : 0.0);
    if (!lse_within(L[blockIdx.x], ref)) {
      atomicAdd(counts + 1, 1ull);
      atomicMin(counts + 3, static_cast<unsigned long long>(blockIdx.x));
    }
  }
}

void launch_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, float* o, float* lse, int H, int Sq, int Sk, int causal) {
  hipLaunchKernelGGL(attn_fwd, dim3(H * (Sq / kBlockQ)), dim3(256), 0, 0, q, k, v, o, lse, H, Sq, Sk, causal);
}

// The device side of one attention: Q, K, V, O, lse.
struct AttnBuffers {
  DeviceBuffer<uint16_t> q, k, v;
  DeviceBuffer<float> o, lse;
  void alloc(Status& st, int device, int H, int Sq, int Sk) {
    CANARY_HIP(st, hipSetDevice(device));
    CANARY_HIP(st, q.alloc(static_cast<size_t>(H) * Sq * kD * 2));
    CANARY_HIP(st, k.alloc(static_cast<size_t>(H) * Sk * kD * 2));
    CANARY_HIP(st, v.alloc(static_cast<size_t>(H) * Sk * kD * 2));
    CANARY_HIP(st, o.alloc(static_cast<size_t>(H) * Sq * kD * 4));
    CANARY_HIP(st, lse.alloc(static_cast<size_t>(H) * Sq * 4));
  }
  void launch(int H, int Sq, int Sk, int causal) const { launch_fwd(q.get(), k.get(), v.get(), o.get(), lse.get(), H, Sq, Sk, causal); }
};

// The hashed set's verdict on downloaded O and lse: `rows` distinct rows per head against float64.
void judge_hashed(const std::vector<float>& o, const std::vector<float>& lse, int H, int Sq, int Sk, int causal, int rows,
                  amdgpu_attn_result* res) {
  double ref[kD], ref_lse;
  for (int head = 0; head < H; ++head) {
    int picked[kMaxRows], n = 0;
    for (int c = 0; n < rows && c < 8 * kMaxRows; ++c) {
      const int i = checked_row(c, head, Sq);
      bool seen = false;
      for (int k = 0; k < n; ++k) seen = seen || picked[k] == i;
      if (seen) continue;
      picked[n++] = i;
      reference_row(kHashed, head, i, Sq, Sk, causal, ref, &ref_lse);
      const unsigned long long row = static_cast<unsigned long long>(head) * Sq + i;
      for (int d = 0; d < kD; ++d) {
        const double e = std::fabs(static_cast<double>(o[row * kD + d]) - ref[d]);
        if (!(e <= res->max_err)) res->max_err = e;  // a NaN sticks
        if (!(e <= kOBound)) {
          if (res->o_errors[kHashed]++ == 0 || row * kD + d < res->first_bad[kHashed]) res->first_bad[kHashed] = row * kD + d;
        }
      }
      const double e = std::fabs(static_cast<double>(lse[row]) - ref_lse);
      if (!(e <= res->max_lse_err)) res->max_lse_err = e;
      if (!lse_within(lse[row], ref_lse)) {
        if (res->lse_errors[kHashed]++ == 0 || row < res->first_bad_lse[kHashed]) res->first_bad_lse[kHashed] = row;
      }
    }
  }
}

}  // namespace

extern "C" {

int amdgpu_attn_sizeof(int which) { return which == 0 ? static_cast<int>(sizeof(amdgpu_attn_result)) : -1; }

int amdgpu_attn_describe(const amdgpu_attn_result* r, char* buf, int len) { return describe(*r, buf, len); }

int amdgpu_attn_operands(int set, int H, int Sq, int Sk, unsigned short* q, unsigned short* k, unsigned short* v) {
  if (set < 0 || set >= kAttnSets || H <= 0 || Sq <= 0 || Sk <= 0) return -1;
  for (int head = 0; head < H; ++head) {
    for (int i = 0; i < Sq; ++i)
      for (int d = 0; d < kD; ++d) q[(static_cast<size_t>(head) * Sq + i) * kD + d] = bf16_bits(q_val(set, head, i, d));
    for (int j = 0; j < Sk; ++j)
      for (int d = 0; d < kD; ++d) {
        k[(static_cast<size_t>(head) * Sk + j) * kD + d] = bf16_bits(k_val(set, head, j, d));
        v[(static_cast<size_t>(head) * Sk + j) * kD + d] = bf16_bits(static_cast<float>(v_val(set, head, j, d)));
      }
  }
  return 0;
}

int amdgpu_attn_expected(int set, int H, int Sq, int Sk, int causal, float* o, double* lse) {
  if ((set != kUniform && set != kRouted) || H <= 0 || Sq <= 0 || Sk <= 0 || (causal && Sk < Sq)) return -1;
  for (int head = 0; head < H; ++head)
    for (int i = 0; i < Sq; ++i) {
      const Top top = top_of(set, i, Sq, Sk, causal);
      for (int d = 0; d < kD; ++d)
        o[(static_cast<size_t>(head) * Sq + i) * kD + d] = expected_o(top_sum(set, head, i, d, top, Sq, Sk, causal), top);
      lse[static_cast<size_t>(head) * Sq + i] = expected_lse(top);
    }
  return 0;
}

int amdgpu_attn_run(int device, const unsigned short* q, const unsigned short* k, const unsigned short* v, float* o,
                    float* lse, int H, int Sq, int Sk, int causal, char* err, int err_len) {
  if (!shape_ok(H, Sq, Sk, causal)) {
    shape_text(H, Sq, Sk, causal, err, err_len);
    return -1;
  }
  Status st;
  AttnBuffers b;
  b.alloc(st, device, H, Sq, Sk);
  CANARY_HIP(st, b.q.upload(q));
  CANARY_HIP(st, b.k.upload(k));
  CANARY_HIP(st, b.v.upload(v));
  if (st.ok()) {
    b.launch(H, Sq, Sk, causal);
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, b.o.download(o));
  CANARY_HIP(st, b.lse.download(lse));
  return st.report("attention path: ", err, err_len);
}

int amdgpu_attn_check(int device, int H, int Sq, int Sk, int causal, int iters, int rows, int flags,
                      amdgpu_attn_result* result, char* err, int err_len) {
  *result = amdgpu_attn_result();
  if (H == 0) H = kAttnDefaultHeads;
  if (Sq == 0) Sq = Sk ? Sk : kAttnDefaultSeq;
  if (Sk == 0) Sk = Sq;
  causal = causal != 0;
  if (!shape_ok(H, Sq, Sk, causal)) {
    shape_text(H, Sq, Sk, causal, err, err_len);
    return -1;
  }
  if (iters < 1 || rows < 4 || rows > kMaxRows) {
    std::snprintf(err, err_len, "attention path: iters %d must be at least 1 and rows %d within 4..%d", iters, rows, kMaxRows);
    return -1;
  }
  result->heads = H, result->seq_q = Sq, result->seq_k = Sk, result->causal = causal;
  result->iters = iters, result->rows = rows;
  Status st;
  AttnBuffers b;
  DeviceBuffer<unsigned long long> d_counts;
  Events<2> ev;
  b.alloc(st, device, H, Sq, Sk);
  CANARY_HIP(st, d_counts.alloc(4 * sizeof(unsigned long long)));
  CANARY_HIP(st, ev.create());
  const size_t n_o = static_cast<size_t>(H) * Sq * kD, n_lse = static_cast<size_t>(H) * Sq;
  double total_ms = 0;
  for (int set = 0; set < kAttnSets; ++set) {
    unsigned long long counts[4] = {0, 0, ~0ull, ~0ull};
    float ms[1] = {0};
    CANARY_HIP(st, d_counts.upload(counts));
    if (st.ok()) {
      hipLaunchKernelGGL(attn_fill, dim3(2048), dim3(256), 0, 0, b.q.get(), b.k.get(), b.v.get(), set, H, Sq, Sk);
      b.launch(H, Sq, Sk, causal);  // warm-up
      st.check(hipGetLastError());
    }
    time_stages(st, ev, ms, [&](int) {
      for (int i = 0; i < iters; ++i) b.launch(H, Sq, Sk, causal);
      return hipSuccess;
    });
    CANARY_HIP(st, b.o.fill(0xFF));  // the poison: what is verified below was written after it
    CANARY_HIP(st, b.lse.fill(0xFF));
    if (st.ok() && !(flags & kAttnSkipVerifiedLaunch)) {
      b.launch(H, Sq, Sk, causal);
      st.check(hipGetLastError());
    }
    if (flags & kAttnInject) {  // a row the hashed set always checks
      const float junk = 12345.0f;
      CANARY_HIP(st, hipMemcpy(b.o.get() + (static_cast<size_t>(H / 2) * Sq + Sq - 1) * kD + 5, &junk, 4, hipMemcpyHostToDevice));
    }
    if (set != kHashed) {
      if (st.ok()) {
        hipLaunchKernelGGL(attn_verify, dim3(H * Sq), dim3(kD), 0, 0, b.o.get(), b.lse.get(), set, H, Sq, Sk, causal,
                           d_counts.get());
        st.check(hipGetLastError());
      }
      CANARY_HIP(st, hipDeviceSynchronize());
      CANARY_HIP(st, d_counts.download(counts));
      result->o_errors[set] = counts[0], result->lse_errors[set] = counts[1];
      result->first_bad[set] = counts[2], result->first_bad_lse[set] = counts[3];
    } else {
      std::vector<float> o(n_o), lse(n_lse);
      CANARY_HIP(st, hipDeviceSynchronize());
      CANARY_HIP(st, b.o.download(o.data()));
      CANARY_HIP(st, b.lse.download(lse.data()));
      result->first_bad[set] = result->first_bad_lse[set] = ~0ull;
      if (st.ok()) judge_hashed(o, lse, H, Sq, Sk, causal, rows, result);
    }
    result->ms[set] = ms[0];
    total_ms += ms[0];
  }
  double tiles = 0;  // (workgroup, key tile) pairs a launch walks
  for (int q0 = 0; q0 < Sq; q0 += kBlockQ) tiles += tiles_of_block(q0, Sq, Sk, causal);
  if (st.ok() && total_ms > 0)
    result->tflops = 4.0 * H * tiles * kBlockQ * kBlockK * kD * iters * kAttnSets / (total_ms * 1e-3) / 1e12;
  return st.report("attention path: ", err, err_len);
}

}  // extern "C"
