// The MFMA forms of the gfx950 canary, each written once: the exact small-integer operands, the
// lane maps, the three forms, and the exactness check, rate chain and raw-code loader that
// canary.hip, datapath.hip and sites.hip share.  No HIP include: all but the MFMA builtins is
// FORMS_HD, so a plain C++17 compiler runs the same code (tests/native/forms_selftest.cpp).
//
// Operand layout; lane l is r = l & 31, h = l >> 5, and holds elements of row r of A and of
// column r of B (the same map for both); C/D does not depend on the operand type (cd_row32):
//   * 32x32x16 (bf16, unscaled fp8): element j (0..7) is k = 8 h + j (cdna_hip_programming.md §3).
//   * scaled 32x32x64, measured with raw fragments (scripts/probe_lowp_layout.py, profiles/r2/
//     lowp_layout_probe.json): byte j of the 8-dword operand for fp8/bf8, nibble j of the low 4
//     dwords for fp4; the lane's scale operand (byte 0, op_sel 0) is the E8M0 exponent of k-block
//     h of that row.  fp4: element j is k = 32 h + j.  fp8/bf8: k = 32 (j >> 4) + 16 h + (j & 15),
//     two K=32 halves, so block h spans elements 16h..16h+15 of BOTH lane halves.
//     tests/test_gpu_datapath.py checks this map against a PyTorch fp32 GEMM on random codes.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define FORMS_HD __host__ __device__ __forceinline__
#else
#define FORMS_HD inline
#endif

namespace canary {

FORMS_HD uint64_t fmix64(uint64_t x) {  // the hash of every canary pattern
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
FORMS_HD uint32_t mix32(uint64_t x) { return static_cast<uint32_t>(fmix64(x)); }

// small integer in [-4, 4] from a hash: exactly representable in bf16, fp8 (e4m3 and
// e5m2) and fp4 (e2m1), so MFMA results on such operands are exact in fp32
FORMS_HD int small_int(uint64_t key) { return static_cast<int>(mix32(key) % 9u) - 4; }

// A[row][k] and B[k][col] of exactness block `blk`
FORMS_HD int a_val(uint32_t blk, int row, int k) {
  return small_int((static_cast<uint64_t>(blk) << 40) ^ (static_cast<uint64_t>(row) << 20) ^ static_cast<uint64_t>(k));
}
FORMS_HD int b_val(uint32_t blk, int k, int col) {
  return small_int(0x5555ull ^ (static_cast<uint64_t>(blk) << 40) ^ (static_cast<uint64_t>(k) << 20) ^
                   static_cast<uint64_t>(col) ^ (1ull << 62));
}

// C/D map of the 32x32 forms: accumulator register `reg` (0-15) of a lane in half h is the
// element of this row in column lane & 31.
FORMS_HD int cd_row32(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

FORMS_HD short bf16_of_int(int v) {
  const float f = static_cast<float>(v);
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return static_cast<short>(u >> 16);  // exact for small integers
}

constexpr int kFp8 = 0, kBf8 = 1, kFp4 = 4;  // cbsz / blgp format codes
constexpr int kFp8Unscaled = 8;             // host-side id of v_mfma_f32_32x32x16_fp8_fp8

// OCP code of a small integer v in [-4, 4] (every one is exact in all three formats).
template <int FMT>
FORMS_HD uint32_t lowp_code(int v) {
  const uint32_t m = static_cast<uint32_t>(v < 0 ? -v : v);
  uint32_t c;
  if (FMT == kFp8) c = m == 0 ? 0u : m == 1 ? 0x38u : m == 2 ? 0x40u : m == 3 ? 0x44u : 0x48u;       // e4m3fn
  else if (FMT == kBf8) c = m == 0 ? 0u : m == 1 ? 0x3Cu : m == 2 ? 0x40u : m == 3 ? 0x42u : 0x44u;  // e5m2
  else c = m == 0 ? 0u : m == 1 ? 0x2u : m == 2 ? 0x4u : m == 3 ? 0x5u : 0x6u;                       // e2m1
  if (v < 0) c |= FMT == kFp4 ? 0x8u : 0x80u;
  return c;
}

template <int FMT>
constexpr int kBits = FMT == kFp4 ? 4 : 8;

// k (within one 64-deep step) of element j of a lane in half h of the scaled form
template <int FMT>
FORMS_HD int kmap(int h, int j) {
  return FMT == kFp4 ? 32 * h + j : 32 * (j >> 4) + 16 * h + (j & 15);
}

// E8M0 block scale of (row or column `rc`, k-block `kb`, operand `which`) when varied:
// 2^0 or 2^1, so every product stays an exact small integer in fp32.
FORMS_HD int scale_exp(int vary, int rc, int kb, int which) {
  return vary ? static_cast<int>(mix32((static_cast<uint64_t>(which) << 48) ^ (static_cast<uint64_t>(rc) << 24) ^
                                       static_cast<uint64_t>(kb)) & 1u)
              : 0;
}

// The register vectors of the MFMA builtins; to a plain C++ compiler, arrays of the same shape.
#ifdef __HIPCC__
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using i32x8 = __attribute__((ext_vector_type(8))) int;
#else
template <class T, int N>
struct host_vec {
  T v[N];
  T& operator[](int i) { return v[i]; }
};
using bf16x8 = host_vec<short, 8>;
using i32x8 = host_vec<int, 8>;
#endif

// element j (0..31) of a lane's operand of the scaled form
template <int FMT>
FORMS_HD void put(i32x8& x, int j, uint32_t code) {
  constexpr int b = kBits<FMT>;
  x[(j * b) >> 5] |= static_cast<int>(code << ((j * b) & 31));
}

// ---- the forms -----------------------------------------------------------------------------
// A form says: kK, the k of one MFMA; kElems, a lane's operand elements; kKeyOffset, which keeps
// its data apart from another form's; k_of(h, j), the k (in a step) of element j in half h; set(),
// which stores integer v as element j of a zeroed operand; perturbed(), what a fault injection
// puts in place of av; scale(), the E8M0 byte of the lane's scale operand (row or column r, step
// s, half h: k-block 2 s + h of kBlockK k; kBlockK 1: no scales); ref_shift(), the A plus B scale
// exponent of block kb of C[row][col]; mfma(), the instruction.  kUnrollOperands and kBlockK 1
// keep the parent's register counts (profiles/mfma_forms/README.md lists each spelling tried).
struct Form32x32x16 {  // what the two unscaled forms share
  static constexpr int kK = 16, kElems = 8, kBlockK = 1;
  FORMS_HD static int k_of(int h, int j) { return 8 * h + j; }
  FORMS_HD static int scale(int, int, int, int, int) { return 127; }  // 2^0, and not an operand
  FORMS_HD static int ref_shift(int, int, int, int) { return 0; }
  FORMS_HD static int perturbed(int av) { return av == 4 ? 3 : av + 1; }  // stays within [-4, 4]
};

struct FormBf16 : Form32x32x16 {  // v_mfma_f32_32x32x16_bf16
  static constexpr uint32_t kKeyOffset = 0;
  static constexpr bool kUnrollOperands = false;
  using operand = bf16x8;
  FORMS_HD static void set(operand& x, int j, int v) { x[j] = bf16_of_int(v); }
  FORMS_HD static int perturbed(int av) { return av + 1; }  // 5 is exact in bf16
#ifdef __HIPCC__
  __device__ __forceinline__ static f32x16 mfma(operand a, operand b, f32x16 acc, int, int) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
#endif
};

struct FormFp8Unscaled : Form32x32x16 {  // v_mfma_f32_32x32x16_fp8_fp8: byte j of a 2-dword operand
  static constexpr uint32_t kKeyOffset = 0x77u << 20;
  static constexpr bool kUnrollOperands = true;
  using operand = uint64_t;
  FORMS_HD static void set(operand& x, int j, int v) { x |= static_cast<uint64_t>(lowp_code<kFp8>(v)) << (8 * j); }
#ifdef __HIPCC__
  __device__ __forceinline__ static f32x16 mfma(operand a, operand b, f32x16 acc, int, int) {
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(static_cast<long>(a), static_cast<long>(b), acc, 0, 0, 0);
  }
#endif
};

template <int FMT>
struct FormScaled {  // v_mfma_scale_f32_32x32x64_f8f6f4 with both operands in format FMT
  static constexpr int kK = 64, kElems = 32, kBlockK = 32;
  static constexpr uint32_t kKeyOffset = static_cast<uint32_t>(FMT + 1) << 20;  // distinct data per format
  static constexpr bool kUnrollOperands = true;
  using operand = i32x8;
  FORMS_HD static int k_of(int h, int j) { return kmap<FMT>(h, j); }
  FORMS_HD static void set(operand& x, int j, int v) { put<FMT>(x, j, lowp_code<FMT>(v)); }
  FORMS_HD static int perturbed(int av) { return av == 4 ? 3 : av + 1; }
  FORMS_HD static int scale(int vary, int r, int s, int h, int which) {
    return 127 + scale_exp(vary, r, 2 * s + h, which);
  }
  FORMS_HD static int ref_shift(int vary, int row, int col, int kb) {
    return scale_exp(vary, row, kb, 0) + scale_exp(vary, col, kb, 1);
  }
#ifdef __HIPCC__
  __device__ __forceinline__ static f32x16 mfma(operand a, operand b, f32x16 acc, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 0, sa, 0, sb);
  }
#endif
};

// Two pieces of the check as text: in functions of their own lowp_exact and fp8_exact take two
// more VGPRs.  form_element and form_ref are the same text as functions, for the self-test.
// Element j of A and B of a lane for step s; `inject` perturbs lane 0, step 0, element 0 of A.
#define CANARY_FORM_ELEMENT(F, a, b, blk, lane, r, h, s, j, inject)               \
  {                                                                               \
    const int k = F::kK * (s) + F::k_of(h, j);                                    \
    int av = a_val(blk, r, k);                                                    \
    if ((s) == 0 && (j) == 0 && (lane) == 0 && (inject)) av = F::perturbed(av);  \
    F::set(a, j, av);                                                             \
    F::set(b, j, b_val(blk, k, r));                                               \
  }
// ref += C[row][col] of exactness block `blk` over K = F::kK * ksteps
#define CANARY_FORM_REF(F, ref, blk, row, col, ksteps, vary_scale)                                  \
  for (int kb = 0; kb < F::kK / F::kBlockK * (ksteps); ++kb) {                                      \
    int part = 0;                                                                                   \
    for (int j = 0; j < F::kBlockK; ++j)                                                            \
      part += a_val(blk, row, F::kBlockK * kb + j) * b_val(blk, F::kBlockK * kb + j, col);          \
    ref += part * (1 << F::ref_shift(vary_scale, row, col, kb)); /* part may be negative */         \
  }
template <class F>
FORMS_HD void form_element(typename F::operand& a, typename F::operand& b, uint32_t blk, int lane, int s, int j,
                           bool inject) {
  const int r = lane & 31, h = lane >> 5;
  CANARY_FORM_ELEMENT(F, a, b, blk, lane, r, h, s, j, inject)
}
template <class F>
FORMS_HD int form_ref(uint32_t blk, int row, int col, int ksteps, int vary_scale) {
  int ref = 0;
  CANARY_FORM_REF(F, ref, blk, row, col, ksteps, vary_scale)
  return ref;
}

#ifdef __HIPCC__

// A zeroed accumulator.  rate_chain and lowp_gemm (datapath.hip) spell the loop out instead: with
// the call rate_chain's fp4 instance takes 77 VGPRs for 70 and lowp_gemm is scheduled differently.
__device__ __forceinline__ f32x16 zero_f32x16() {
  f32x16 v;
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  return v;
}

// The exactness check of form F: one wave computes C[32x32] = A[32xK] * B[Kx32], K = F::kK * ksteps,
// one MFMA per step; returns how many of this lane's 16 accumulators differ from the integer reference.
template <class F>
__device__ __forceinline__ uint32_t form_check(uint32_t key, int lane, int ksteps, int vary_scale, bool inject) {
  const int r = lane & 31, h = lane >> 5;
  const uint32_t blk = key + F::kKeyOffset;
  f32x16 acc = zero_f32x16();
  for (int s = 0; s < ksteps; ++s) {
    typename F::operand a, b;
    a = b = typename F::operand();
    if constexpr (F::kUnrollOperands) {
#pragma unroll
      for (int j = 0; j < F::kElems; ++j) CANARY_FORM_ELEMENT(F, a, b, blk, lane, r, h, s, j, inject)
    } else {
      for (int j = 0; j < F::kElems; ++j) CANARY_FORM_ELEMENT(F, a, b, blk, lane, r, h, s, j, inject)
    }
    acc = F::mfma(a, b, acc, F::scale(vary_scale, r, s, h, 0), F::scale(vary_scale, r, s, h, 1));
  }
  uint32_t bad = 0;
  const int col = lane & 31;
  for (int reg = 0; reg < 16; ++reg) {
    const int row = cd_row32(reg, h);
    int ref = 0;
    CANARY_FORM_REF(F, ref, blk, row, col, ksteps, vary_scale)
    bad += acc[reg] != static_cast<float>(ref);
  }
  return bad;
}

// The rate chain of form F: register-resident operands, two independent accumulator chains per wave.
// A kernel template: as a function the rate kernels call, the scaled forms take 99 VGPRs for 68.
template <class F>
__global__ void __launch_bounds__(256) rate_chain(int iters, float* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  typename F::operand a, b;
  a = b = typename F::operand();
#pragma unroll
  for (int j = 0; j < F::kElems; ++j) {
    F::set(a, j, ((lane + j) % 5) - 2);
    F::set(b, j, ((lane * 3 + j) % 7) - 3);
  }
  f32x16 acc0, acc1;
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
  for (int it = 0; it < iters; ++it) {
    acc0 = F::mfma(a, b, acc0, 127, 127);
    acc1 = F::mfma(b, a, acc1, 127, 127);
  }
  float s = 0.f;
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i];
  if (s == 1234.5f) sink[blockIdx.x * blockDim.x + threadIdx.x] = s;  // keeps the chains live
}

// A lane's operand of the scaled form from raw codes, one per byte (fp4: low nibble): element j is p[at(j)].
template <int FMT, class At>
__device__ __forceinline__ i32x8 raw_operand(const uint8_t* __restrict__ p, At at) {
  i32x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 32; ++j) put<FMT>(x, j, p[at(j)] & ((1u << kBits<FMT>) - 1));
  return x;
}

#endif  // __HIPCC__

#undef CANARY_FORM_ELEMENT
#undef CANARY_FORM_REF

}  // namespace canary
