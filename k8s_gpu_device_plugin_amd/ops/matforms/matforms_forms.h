// The other matrix forms of gfx950, each written once: f16, i8, f32, f64, fp6, the mixed MX
// formats and the 16x16 shapes, beside the three forms of ../mfma_forms.h.  One description per
// form feeds the exactness check, the integer reference, the rate chain, the raw single-wave
// MFMA and the table the host reads (kForms).  No HIP include: all but the MFMA builtins is
// FORMS_HD, so a plain C++17 compiler runs the same code (tests/native/matforms_selftest.cpp).
//
// Lane l of a form with M rows is r = l % M, g = l / M (64 / M groups) and holds kElems elements
// of row r of A and of column r of B; K = kElems * 64 / M.  Two operand maps occur:
//   * kMapLinear: element j is k = kElems g + j (cdna_hip_programming.md §3 for bf16 16x16x32,
//     f32 32x32x2 / 16x16x4 and f64 16x16x4; ../mfma_forms.h for fp4);
//   * kMapHalves: k = (K / 2) (j >> 4) + 16 g + (j & 15), the 8-bit operands of the scaled
//     instruction (two K / 2 halves; ../mfma_forms.h for 32x32x64).
// C/D: the guide's shape maps, and f64's own (row = g + 4 reg).  The lane's scale byte (byte 0,
// op_sel 0) is the E8M0 exponent of k-block g (32 k) of its row or column.  Every map that is
// not the guide's was read from the hardware with one-hot operands (matforms.operand_map,
// profiles/matforms/map_<form>.json) and tests/test_gpu_matforms.py compares each again.
#pragma once
#include <cstdint>

#include "../mfma_forms.h"

#ifdef __HIPCC__
#define MATFORMS_UNROLL _Pragma("unroll")
#else
#define MATFORMS_UNROLL
#endif

namespace matforms {

using canary::fmix64;
using canary::kBf8;
using canary::kFp4;
using canary::kFp8;
using canary::lowp_code;
using canary::mix32;
using canary::scale_exp;
constexpr int kFp6 = 2, kBf6 = 3;  // cbsz / blgp format codes beside kFp8, kBf8, kFp4

constexpr int kMaxKsteps = 8;
constexpr int kOperandWords = 8;   // a lane's raw operand, as amdgpu_matforms_raw takes it
constexpr int kAccWords = 16;      // a lane's raw accumulators, as it returns them
constexpr int kAccF32 = 0, kAccI32 = 1, kAccF64 = 2;
constexpr int kMapLinear = 0, kMapHalves = 1;

// integer in [-R, R] from a hash
FORMS_HD int small_int(uint64_t key, int R) {
  return static_cast<int>(mix32(key) % static_cast<uint32_t>(2 * R + 1)) - R;
}

template <int N>
struct Words {
  uint32_t w[N];
};

// `bits` bits of code as element j of a zeroed operand
template <int BITS>
FORMS_HD void put_bits(uint32_t* w, int j, uint64_t code) {
  const int p = j * BITS, i = p >> 5, sh = p & 31;
  w[i] |= static_cast<uint32_t>(code << sh);
  if (sh + BITS > 32) w[i + 1] |= static_cast<uint32_t>(code >> (32 - sh));
}

// ---- the number formats: the code of an integer v that the format holds exactly --------------
FORMS_HD uint32_t f32_bits(int v) {
  const float f = static_cast<float>(v);
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
struct EncF16 {  // |v| <= 2048
  static constexpr int kBits = 16;
  FORMS_HD static uint64_t code(int v) {
    const uint32_t u = f32_bits(v), e = (u >> 23) & 0xFFu;
    if (e == 0) return 0;  // v == 0
    return ((u >> 16) & 0x8000u) | ((e - 112u) << 10) | ((u >> 13) & 0x3FFu);
  }
};
struct EncBf16 {  // |v| <= 256
  static constexpr int kBits = 16;
  FORMS_HD static uint64_t code(int v) { return f32_bits(v) >> 16; }
};
struct EncI8 {
  static constexpr int kBits = 8;
  FORMS_HD static uint64_t code(int v) { return static_cast<uint32_t>(v) & 0xFFu; }
};
struct EncF32 {
  static constexpr int kBits = 32;
  FORMS_HD static uint64_t code(int v) { return f32_bits(v); }
};
struct EncF64 {
  static constexpr int kBits = 64;
  FORMS_HD static uint64_t code(int v) {
    const double d = static_cast<double>(v);
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    return u;
  }
};
template <int FMT>
struct EncLowp {  // fp8 e4m3, bf8 e5m2, fp6 e2m3, bf6 e3m2, fp4 e2m1; |v| <= 4
  static constexpr int kBits = FMT == kFp4 ? 4 : (FMT == kFp6 || FMT == kBf6) ? 6 : 8;
  FORMS_HD static uint64_t code(int v) {
    if (FMT == kFp8 || FMT == kBf8 || FMT == kFp4) return lowp_code<FMT>(v);
    const uint32_t m = static_cast<uint32_t>(v < 0 ? -v : v);
    const uint32_t c = FMT == kFp6 ? (m == 0 ? 0u : m == 1 ? 0x08u : m == 2 ? 0x10u : m == 3 ? 0x14u : 0x18u)   // e2m3
                                   : (m == 0 ? 0u : m == 1 ? 0x0Cu : m == 2 ? 0x10u : m == 3 ? 0x12u : 0x14u);  // e3m2
    return c | (v < 0 ? 0x20u : 0u);
  }
};

FORMS_HD int k_of_map(int map, int K, int elems, int g, int j) {
  return map == kMapLinear ? elems * g + j : (K / 2) * (j >> 4) + 16 * g + (j & 15);
}

// The register vectors of the builtins (f32x16, bf16x8, i32x8: ../mfma_forms.h).
#ifdef __HIPCC__
using canary::bf16x8;
using canary::f32x16;
using canary::i32x8;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
using f64x4 = __attribute__((ext_vector_type(4))) double;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
template <int KIND, int N>
struct acc_type;
template <> struct acc_type<kAccF32, 16> { using type = f32x16; using elem = float; };
template <> struct acc_type<kAccF32, 4> { using type = f32x4; using elem = float; };
template <> struct acc_type<kAccI32, 16> { using type = i32x16; using elem = int; };
template <> struct acc_type<kAccI32, 4> { using type = i32x4; using elem = int; };
template <> struct acc_type<kAccF64, 4> { using type = f64x4; using elem = double; };

template <class V, int N>
__device__ __forceinline__ V vec_of(const Words<N>& x) {  // the operand's words as the builtin's vector
  struct alignas(alignof(V)) Raw { uint32_t w[sizeof(V) / 4]; } raw;
#pragma unroll
  for (int i = 0; i < static_cast<int>(sizeof(V) / 4); ++i) raw.w[i] = i < N ? x.w[i] : 0u;
  return __builtin_bit_cast(V, raw);
}
#endif

// ---- the forms -----------------------------------------------------------------------------
// A form says: kName and kInstruction (the mnemonic the assembly must hold); kM; kElems, a
// lane's elements per operand; the two encodings EA and EB; the two operand maps; kR, values in
// [-kR, kR]; the accumulator kind and count; kScaled, whether the lane carries E8M0 scales of
// 32-k blocks; kKeyOffset, which keeps its data apart from another form's; mfma().
template <class EA_, class EB_, int M, int ELEMS, int MAP_A, int MAP_B, int R, int ACC, bool SCALED, uint32_t KEY>
struct FormBase {
  using EA = EA_;
  using EB = EB_;
  static constexpr int kM = M, kGroups = 64 / M, kElems = ELEMS, kK = ELEMS * (64 / M), kR = R;
  static constexpr int kMapA = MAP_A, kMapB = MAP_B;
  static constexpr int kAccKind = ACC, kAcc = M == 32 ? 16 : 4;
  static constexpr bool kScaled = SCALED;
  static constexpr int kBlockK = SCALED ? 32 : 1;
  static constexpr uint32_t kKeyOffset = KEY << 20;
  static constexpr int kWordsA = (ELEMS * EA::kBits + 31) / 32, kWordsB = (ELEMS * EB::kBits + 31) / 32;
  using operand_a = Words<kWordsA>;
  using operand_b = Words<kWordsB>;
  FORMS_HD static int k_of_a(int g, int j) { return k_of_map(MAP_A, kK, ELEMS, g, j); }
  FORMS_HD static int k_of_b(int g, int j) { return k_of_map(MAP_B, kK, ELEMS, g, j); }
  FORMS_HD static void set_a(operand_a& x, int j, int v) { put_bits<EA::kBits>(x.w, j, EA::code(v)); }
  FORMS_HD static void set_b(operand_b& x, int j, int v) { put_bits<EB::kBits>(x.w, j, EB::code(v)); }
  // C/D: accumulator `reg` of a lane in group g is this row of column lane % kM
  FORMS_HD static int cd_row(int reg, int g) {
    return M == 32 ? canary::cd_row32(reg, g) : ACC == kAccF64 ? g + 4 * reg : 4 * g + reg;
  }
  FORMS_HD static int perturbed(int av) { return av == R ? R - 1 : av + 1; }  // stays within [-R, R]
  // the E8M0 byte of the lane's scale operand: row or column r, step s, k-block g of the step
  FORMS_HD static int scale(int vary, int r, int s, int g, int which) {
    return SCALED ? 127 + scale_exp(vary, r, kGroups * s + g, which) : 127;
  }
  FORMS_HD static int ref_shift(int vary, int row, int col, int kb) {
    return SCALED ? scale_exp(vary, row, kb, 0) + scale_exp(vary, col, kb, 1) : 0;
  }
#ifdef __HIPCC__
  using acc_t = typename acc_type<ACC, (M == 32 ? 16 : 4)>::type;
  using acc_elem = typename acc_type<ACC, (M == 32 ? 16 : 4)>::elem;
#endif
};

#ifdef __HIPCC__
#define MATFORMS_MFMA(...)                                                                                      \
  __device__ __forceinline__ static acc_t mfma(const operand_a& a, const operand_b& b, acc_t acc, int sa, int sb) { \
    return __VA_ARGS__;                                                                                         \
  }
#else
#define MATFORMS_MFMA(...)
#endif

struct FormF16_32 : FormBase<EncF16, EncF16, 32, 8, kMapLinear, kMapLinear, 128, kAccF32, false, 0x101> {
  static constexpr const char *kName = "f16_32", *kText = "f16 32x32x16", *kInstruction = "v_mfma_f32_32x32x16_f16";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_32x32x16_f16(vec_of<f16x8>(a), vec_of<f16x8>(b), acc, 0, 0, 0))
};
struct FormF16_16 : FormBase<EncF16, EncF16, 16, 8, kMapLinear, kMapLinear, 128, kAccF32, false, 0x102> {
  static constexpr const char *kName = "f16_16", *kText = "f16 16x16x32", *kInstruction = "v_mfma_f32_16x16x32_f16";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_16x16x32_f16(vec_of<f16x8>(a), vec_of<f16x8>(b), acc, 0, 0, 0))
};
struct FormBf16_16 : FormBase<EncBf16, EncBf16, 16, 8, kMapLinear, kMapLinear, 128, kAccF32, false, 0x103> {
  static constexpr const char *kName = "bf16_16", *kText = "bf16 16x16x32", *kInstruction = "v_mfma_f32_16x16x32_bf16";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_16x16x32_bf16(vec_of<bf16x8>(a), vec_of<bf16x8>(b), acc, 0, 0, 0))
};
struct FormI8_32 : FormBase<EncI8, EncI8, 32, 16, kMapLinear, kMapLinear, 127, kAccI32, false, 0x104> {
  static constexpr const char *kName = "i8_32", *kText = "i8 32x32x32", *kInstruction = "v_mfma_i32_32x32x32_i8";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_i32_32x32x32_i8(vec_of<i32x4>(a), vec_of<i32x4>(b), acc, 0, 0, 0))
};
struct FormI8_16 : FormBase<EncI8, EncI8, 16, 16, kMapLinear, kMapLinear, 127, kAccI32, false, 0x105> {
  static constexpr const char *kName = "i8_16", *kText = "i8 16x16x64", *kInstruction = "v_mfma_i32_16x16x64_i8";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_i32_16x16x64_i8(vec_of<i32x4>(a), vec_of<i32x4>(b), acc, 0, 0, 0))
};
struct FormF32_32 : FormBase<EncF32, EncF32, 32, 1, kMapLinear, kMapLinear, 512, kAccF32, false, 0x106> {
  static constexpr const char *kName = "f32_32", *kText = "f32 32x32x2", *kInstruction = "v_mfma_f32_32x32x2_f32";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_32x32x2f32(vec_of<float>(a), vec_of<float>(b), acc, 0, 0, 0))
};
struct FormF32_16 : FormBase<EncF32, EncF32, 16, 1, kMapLinear, kMapLinear, 512, kAccF32, false, 0x107> {
  static constexpr const char *kName = "f32_16", *kText = "f32 16x16x4", *kInstruction = "v_mfma_f32_16x16x4_f32";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_16x16x4f32(vec_of<float>(a), vec_of<float>(b), acc, 0, 0, 0))
};
struct FormF64_16 : FormBase<EncF64, EncF64, 16, 1, kMapLinear, kMapLinear, 1 << 20, kAccF64, false, 0x108> {
  static constexpr const char *kName = "f64_16", *kText = "f64 16x16x4", *kInstruction = "v_mfma_f64_16x16x4_f64";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f64_16x16x4f64(vec_of<double>(a), vec_of<double>(b), acc, 0, 0, 0))
};
struct FormFp8_16 : FormBase<EncLowp<kFp8>, EncLowp<kFp8>, 16, 8, kMapLinear, kMapLinear, 4, kAccF32, false, 0x109> {
  static constexpr const char *kName = "fp8_16", *kText = "fp8 16x16x32", *kInstruction = "v_mfma_f32_16x16x32_fp8_fp8";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(vec_of<long>(a), vec_of<long>(b), acc, 0, 0, 0))
};
struct FormBf8Fp8_32 : FormBase<EncLowp<kBf8>, EncLowp<kFp8>, 32, 8, kMapLinear, kMapLinear, 4, kAccF32, false, 0x10A> {
  static constexpr const char *kName = "bf8fp8_32", *kText = "bf8 x fp8 32x32x16", *kInstruction = "v_mfma_f32_32x32x16_bf8_fp8";
  MATFORMS_MFMA(__builtin_amdgcn_mfma_f32_32x32x16_bf8_fp8(vec_of<long>(a), vec_of<long>(b), acc, 0, 0, 0))
};
template <int FA, int FB, int M, uint32_t KEY>
using FormMx = FormBase<EncLowp<FA>, EncLowp<FB>, M, 32, (FA == kFp8 || FA == kBf8) ? kMapHalves : kMapLinear,
                        (FB == kFp8 || FB == kBf8) ? kMapHalves : kMapLinear, 4, kAccF32, true, KEY>;
#define MATFORMS_MX32(FA, FB) \
  MATFORMS_MFMA(__builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vec_of<i32x8>(a), vec_of<i32x8>(b), acc, FA, FB, 0, sa, 0, sb))
#define MATFORMS_MX16(FA, FB) \
  MATFORMS_MFMA(__builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vec_of<i32x8>(a), vec_of<i32x8>(b), acc, FA, FB, 0, sa, 0, sb))
struct FormMxFp6_32 : FormMx<kFp6, kFp6, 32, 0x10B> {
  static constexpr const char *kName = "mxfp6_32", *kText = "mx-fp6 32x32x64", *kInstruction = "v_mfma_scale_f32_32x32x64_f8f6f4";
  MATFORMS_MX32(kFp6, kFp6)
};
struct FormMxBf6_32 : FormMx<kBf6, kBf6, 32, 0x10C> {
  static constexpr const char *kName = "mxbf6_32", *kText = "mx-bf6 32x32x64", *kInstruction = "v_mfma_scale_f32_32x32x64_f8f6f4";
  MATFORMS_MX32(kBf6, kBf6)
};
struct FormMxFp8Fp4_32 : FormMx<kFp8, kFp4, 32, 0x10D> {
  static constexpr const char *kName = "mxfp8fp4_32", *kText = "mx-fp8 x mx-fp4 32x32x64",
                              *kInstruction = "v_mfma_scale_f32_32x32x64_f8f6f4";
  MATFORMS_MX32(kFp8, kFp4)
};
struct FormMxFp8_16 : FormMx<kFp8, kFp8, 16, 0x10E> {
  static constexpr const char *kName = "mxfp8_16", *kText = "mx-fp8 16x16x128", *kInstruction = "v_mfma_scale_f32_16x16x128_f8f6f4";
  MATFORMS_MX16(kFp8, kFp8)
};
struct FormMxFp4_16 : FormMx<kFp4, kFp4, 16, 0x10F> {
  static constexpr const char *kName = "mxfp4_16", *kText = "mx-fp4 16x16x128", *kInstruction = "v_mfma_scale_f32_16x16x128_f8f6f4";
  MATFORMS_MX16(kFp4, kFp4)
};
#undef MATFORMS_MX32
#undef MATFORMS_MX16
#undef MATFORMS_MFMA

// The table: X(index, form), in the order of matforms.FORMS.  A form whose map is not
// established on the hardware has no row here.
#define MATFORMS_FORMS(X)                                                                                    \
  X(0, FormF16_32) X(1, FormF16_16) X(2, FormBf16_16) X(3, FormI8_32) X(4, FormI8_16) X(5, FormF32_32)        \
  X(6, FormF32_16) X(7, FormF64_16) X(8, FormFp8_16) X(9, FormBf8Fp8_32) X(10, FormMxFp6_32) X(11, FormMxBf6_32) \
  X(12, FormMxFp8Fp4_32) X(13, FormMxFp8_16) X(14, FormMxFp4_16)

struct FormInfo {
  const char* name;         // "i8_32"
  const char* text;         // "i8 32x32x32", as the error text names it
  const char* instruction;  // the mnemonic
  int m, k, elems, r, acc_kind, acc, scaled, bits_a, bits_b, map_a, map_b;
  uint32_t key_offset;
};
template <class F>
constexpr FormInfo info_of() {
  return {F::kName, F::kText, F::kInstruction, F::kM, F::kK, F::kElems, F::kR, F::kAccKind, F::kAcc, F::kScaled ? 1 : 0,
          F::EA::kBits, F::EB::kBits, F::kMapA, F::kMapB, F::kKeyOffset};
}
#define X(i, F) info_of<F>(),
constexpr FormInfo kForms[] = {MATFORMS_FORMS(X)};
#undef X
constexpr int kNumForms = sizeof(kForms) / sizeof(kForms[0]);
constexpr int kMaxForms = 16;  // a record's and a result's room
static_assert(kNumForms <= kMaxForms, "a record counts every form");

// fn(F{}) for form `form` of the table; false: no such form
template <class Fn>
inline bool with_form(int form, Fn&& fn) {
  switch (form) {
#define X(i, F) \
  case i: fn(F{}); return true;
    MATFORMS_FORMS(X)
#undef X
    default: return false;
  }
}

// ---- the data and the reference ----------------------------------------------------------------
// A[row][k] and B[k][col] of exactness block `blk` (the key scheme of ../mfma_forms.h)
template <class F>
FORMS_HD int a_val(uint32_t blk, int row, int k) {
  return small_int((static_cast<uint64_t>(blk) << 40) ^ (static_cast<uint64_t>(row) << 20) ^ static_cast<uint64_t>(k), F::kR);
}
template <class F>
FORMS_HD int b_val(uint32_t blk, int k, int col) {
  return small_int(0x5555ull ^ (static_cast<uint64_t>(blk) << 40) ^ (static_cast<uint64_t>(k) << 20) ^
                       static_cast<uint64_t>(col) ^ (1ull << 62),
                   F::kR);
}

// A lane's operands and scale bytes of step s; `inject` perturbs lane 0, step 0, element 0 of A.
template <class F>
FORMS_HD void form_operands(uint32_t key, int lane, int s, int vary_scale, bool inject, typename F::operand_a& a,
                            typename F::operand_b& b, int& sa, int& sb) {
  const int r = lane % F::kM, g = lane / F::kM;
  const uint32_t blk = key + F::kKeyOffset;
  a = typename F::operand_a();
  b = typename F::operand_b();
  MATFORMS_UNROLL
  for (int j = 0; j < F::kElems; ++j) {
    int av = a_val<F>(blk, r, F::kK * s + F::k_of_a(g, j));
    if (s == 0 && j == 0 && lane == 0 && inject) av = F::perturbed(av);
    F::set_a(a, j, av);
    F::set_b(b, j, b_val<F>(blk, F::kK * s + F::k_of_b(g, j), r));
  }
  sa = F::scale(vary_scale, r, s, g, 0);
  sb = F::scale(vary_scale, r, s, g, 1);
}

// C[row][col] of exactness block key + kKeyOffset over K = kK * ksteps, an exact integer
template <class F>
FORMS_HD int64_t form_ref(uint32_t key, int row, int col, int ksteps, int vary_scale) {
  const uint32_t blk = key + F::kKeyOffset;
  int64_t ref = 0;
  for (int kb = 0; kb < F::kK / F::kBlockK * ksteps; ++kb) {
    int64_t part = 0;
    for (int j = 0; j < F::kBlockK; ++j)
      part += static_cast<int64_t>(a_val<F>(blk, row, F::kBlockK * kb + j)) * b_val<F>(blk, F::kBlockK * kb + j, col);
    ref += part * (1 << F::ref_shift(vary_scale, row, col, kb));  // part may be negative
  }
  return ref;
}

// Accumulators a wave with the injection gets wrong: A[0][k of lane 0's element 0] moved by one, so
// every column whose B element at that k is not zero (a scale of 2^0 or 2^1 leaves none at zero).
template <class F>
FORMS_HD int inject_expected(uint32_t key) {
  const uint32_t blk = key + F::kKeyOffset;
  int n = 0;
  for (int col = 0; col < F::kM; ++col) n += b_val<F>(blk, F::k_of_a(0, 0), col) != 0;
  return n;
}

#ifdef __HIPCC__

// The exactness check of form F: one wave computes C[M x M] = A[M x K] * B[K x M], K = kK * ksteps,
// one MFMA per step; returns how many of this lane's accumulators differ from the integer reference
// and lowers first_reg to the first of them.
template <class F>
__device__ __forceinline__ uint32_t form_check(uint32_t key, int lane, int ksteps, int vary_scale, bool inject,
                                               uint32_t& first_reg) {
  const int g = lane / F::kM, col = lane % F::kM;
  typename F::acc_t acc;
#pragma unroll
  for (int i = 0; i < F::kAcc; ++i) acc[i] = 0;
  for (int s = 0; s < ksteps; ++s) {
    typename F::operand_a a;
    typename F::operand_b b;
    int sa, sb;
    form_operands<F>(key, lane, s, vary_scale, inject, a, b, sa, sb);
    acc = F::mfma(a, b, acc, sa, sb);
  }
  uint32_t bad = 0;
#pragma unroll
  for (int reg = F::kAcc - 1; reg >= 0; --reg) {
    const int64_t ref = form_ref<F>(key, F::cd_row(reg, g), col, ksteps, vary_scale);
    const bool wrong = acc[reg] != static_cast<typename F::acc_elem>(ref);
    bad += wrong;
    if (wrong) first_reg = static_cast<uint32_t>(reg);
  }
  return bad;
}

#endif  // __HIPCC__

}  // namespace matforms
