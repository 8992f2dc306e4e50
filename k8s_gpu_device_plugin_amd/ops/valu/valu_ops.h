// The vector-ALU ops of the gfx950 canary's stand-alone VALU check, each written once: the table
// the kernel dispatch, the host entry points and Python read (kOps), the operand generator, and
// for every op of class exact a host reference in plain integer, float or double arithmetic.
// No HIP include: the device side (valu.hip) supplies only the builtin behind each op, so a plain
// C++17 compiler compiles this file.
//
// An op takes up to three 64-bit operand words (a, b, c; what they hold is the op's operand
// kinds) and leaves up to kMaxResults 32-bit result words.  Operands depend on (seed, op, round,
// lane) only, so one table of 64 lane digests per op describes a whole launch.
#pragma once
#include <cmath>
#include <cstdint>

#include "../mfma_forms.h"

namespace valu {

using canary::fmix64;

constexpr int kLanes = 64;
constexpr int kMaxRounds = 16;
constexpr int kMaxResults = 32;   // result words of one op
constexpr int kMaxGroupOps = 32;  // room for a group's ops in a record
constexpr int kInjectLane = 3;

enum Group { kGroupInt, kGroupBit, kGroupF32, kGroupF64, kGroupF16, kGroupCvt, kGroupApprox, kNumGroups };
constexpr const char* kGroupNames[kNumGroups] = {"int", "bit", "f32", "f64", "f16", "cvt", "approx"};
enum Class { kExact, kConsensus };

// What an operand word holds (the generator's rule for it).
enum Kind {
  kNone,
  kU32,      // 32 hashed bits
  kU64,      // 64 hashed bits
  kPermSel,  // four v_perm selector bytes: 0..7, 12 (0x00) or 13 (0xff)
  kSmallInt, // integer in [-8, 8]
  kF32,      // normal f32, exponent in [-12, 12]
  kF32Pos,   // ... positive
  kF32Big,   // normal f32 with |x| >= 1, exponent in [0, 12]
  kF32Zero,  // kF32, or a zero of either sign one time in four
  kF32Int,   // integer in [-64, 64] as f32
  kF32Exp,   // normal f32, exponent in [-12, 5]: the argument of exp2
  kF32Sin,   // normal f32, exponent in [-8, -3]: |x| < 1/4 revolution
  kF32Cos,   // normal f32, exponent in [-8, -4]: |x| < 1/8 revolution
  kF32x2,    // two kF32
  kF64,      // normal f64, exponent in [-60, 60]
  kF64Pos,   // ... positive
  kF16N,     // one normal f16 (any normal exponent) in the low half
  kF16x2,    // two f16 in [1, 16) of either sign with 6 mantissa bits
  kF16x2Int, // two integers in [-8, 8] as f16
  kBf16x2Int,// ... as bf16
  kFp8Word,  // four e4m3 codes; a launch's 64 lanes hold all 256, NaN codes replaced
  kBf8Word,  // four e5m2 codes likewise, infinity and NaN codes replaced
  kFp4Word,  // eight e2m1 codes; the 64 lanes hold every byte
  kScale,    // 2^s as f32, s in [-2, 2]
  kEncFp8,   // an encoder input for e4m3 as f32 (enc_input below), times the op's scale
  kEncBf8,   // ... for e5m2
  kEncFp4,   // ... for e2m1
  kF16Small, // one normal f16 with |x| < 8 in the low half
  kF16Mid,   // one normal f16, 2^-10 <= |x| < 2^11, in the low half
  kF16Pos,   // ... positive
  kFp6Codes, // a six-bit offset: element j of the 32 is code (offset + j) & 63, and the 64 lanes start at every offset
  kEncSeed,  // 64 hashed bits, the seed of the 32 encoder inputs of a 2xpk16 conversion (expand below)
  kF64Big,   // normal f64 with 1 <= |x| < 2^21
  kNumKinds
};
constexpr const char* kKindNames[kNumKinds] = {
    "none", "u32", "u64", "perm_sel", "small_int", "f32", "f32_pos", "f32_big", "f32_zero", "f32_int", "f32_exp", "f32_sin", "f32_cos",
    "f32x2", "f64", "f64_pos", "f16", "f16x2", "f16x2_int", "bf16x2_int", "fp8_word", "bf8_word", "fp4_word", "scale", "enc_fp8",
    "enc_bf8", "enc_fp4", "f16_small", "f16_mid", "f16_pos", "fp6_codes", "enc_seed", "f64_big"};
enum RKind { kRBits, kRF32, kRF64, kRF16x2 };  // what the result words hold

enum Op : int {
  // int
  kMulLoU32, kMulHiU32, kMulHiI32, kMadU64U32, kMadI64I32, kAdd3U32, kLshlB64, kPkAddU16, kPkMulLoU16, kSdot4, kUdot4,
  kSadU8, kLerpU8, kLshlAddU32, kAshrI64, kMinI32, kMaxU32, kMed3I32, kMed3U32, kPkMadU16, kPkMinI16, kPkMaxU16, kPkLshlB16,
  kSdot8, kUdot8, kSdot2, kMsadU8,
  // bit
  kPermB32, kAlignBit, kAlignByte, kBfeU32, kBfeI32, kBfrev, kBcnt, kFfbh, kBitop96, kBitopE8, kBitopCA, kBitop6B,
  kAshrPkI8, kMbcnt, kFfbl,
  // f32
  kAddF32, kMulF32, kFmaF32, kPkFmaF32, kDivF32, kSqrtF32, kMed3F32, kLdexpF32, kFrexpMantF32, kFrexpExpF32, kFractF32,
  kRndneF32, kFloorF32, kCvtI32F32, kCvtF32I32, kCvtF32Ubyte, kClassF32, kPkMulF32, kPkAddF32, kMinF32, kMaxF32, kCeilF32,
  kTruncF32, kCvtU32F32, kCvtF32U32,
  // f64
  kAddF64, kFmaF64, kDivF64, kSqrtF64, kCvtF32F64, kMulF64, kCvtF64F32, kCvtI32F64, kCvtF64I32,
  // f16
  kPkFmaF16, kPkAddF16, kFdot2, kFdot2Bf16, kCvtPkrtz, kCvtF32F16, kCvtPkBf16F32, kPkMulF16, kCvtF16F32,
  // cvt
  kCvtF32Fp8, kCvtF32Bf8, kCvtPkF32Fp8, kScalePkF32Fp8, kScalePkF32Bf8, kScalePkF32Fp4, kCvtPkFp8F32, kCvtPkBf8F32,
  kScalePkFp8F32, kScalePkBf8F32, kScalePkFp4F32, kCvtPkF32Bf8, kScalePk32F32Fp6, kScalePk32F32Bf6, kScale2xPk16Fp6, kScale2xPk16Bf6,
  // approx
  kExp2, kLog2, kRcp, kRsq, kSqrtRaw, kSin, kCos, kRcpF64, kRsqF64, kPrng, kCvtSrFp8, kExpF16, kLogF16, kRcpF16, kScaleSrPkFp4,
  kNumOps
};

struct OpInfo {
  const char* name;
  const char* mnemonic;  // an instruction the op's kernel must hold
  int group;
  int cls;
  int kind[3];
  int results;
  int rkind;
};

constexpr OpInfo kOps[] = {
    {"mul_lo_u32", "v_mul_lo_u32", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"mul_hi_u32", "v_mul_hi_u32", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"mul_hi_i32", "v_mul_hi_i32", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"mad_u64_u32", "v_mad_u64_u32", kGroupInt, kExact, {kU32, kU32, kU64}, 2, kRBits},
    {"mad_i64_i32", "v_mad_i64_i32", kGroupInt, kExact, {kU32, kU32, kU64}, 2, kRBits},
    {"add3_u32", "v_add3_u32", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"lshl_b64", "v_lshlrev_b64", kGroupInt, kExact, {kU64, kU32, kNone}, 2, kRBits},
    {"pk_add_u16", "v_pk_add_u16", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"pk_mul_lo_u16", "v_pk_mul_lo_u16", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"sdot4", "v_dot4c_i32_i8", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"udot4", "v_dot4_u32_u8", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"sad_u8", "v_sad_u8", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"lerp_u8", "v_lerp_u8", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"lshl_add_u32", "v_lshl_add_u32", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"ashr_i64", "v_ashrrev_i64", kGroupInt, kExact, {kU64, kU32, kNone}, 2, kRBits},
    {"min_i32", "v_min_i32", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"max_u32", "v_max_u32", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"med3_i32", "v_med3_i32", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"med3_u32", "v_med3_u32", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"pk_mad_u16", "v_pk_mad_u16", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"pk_min_i16", "v_pk_min_i16", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"pk_max_u16", "v_pk_max_u16", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"pk_lshlrev_b16", "v_pk_lshlrev_b16", kGroupInt, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"sdot8", "v_dot8c_i32_i4", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"udot8", "v_dot8_u32_u4", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"sdot2", "v_dot2c_i32_i16", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"msad_u8", "v_msad_u8", kGroupInt, kExact, {kU32, kU32, kU32}, 1, kRBits},

    {"perm_b32", "v_perm_b32", kGroupBit, kExact, {kU32, kU32, kPermSel}, 1, kRBits},
    {"alignbit", "v_alignbit_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"alignbyte", "v_alignbyte_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bfe_u32", "v_bfe_u32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bfe_i32", "v_bfe_i32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bfrev", "v_bfrev_b32", kGroupBit, kExact, {kU32, kNone, kNone}, 1, kRBits},
    {"bcnt", "v_bcnt_u32_b32", kGroupBit, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"ffbh", "v_ffbh_u32", kGroupBit, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"bitop3_96", "v_bitop3_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bitop3_e8", "v_bitop3_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bitop3_ca", "v_bitop3_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"bitop3_6b", "v_bitop3_b32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"ashr_pk_i8_i32", "v_ashr_pk_i8_i32", kGroupBit, kExact, {kU32, kU32, kU32}, 1, kRBits},
    {"mbcnt", "v_mbcnt_hi_u32_b32", kGroupBit, kExact, {kU32, kU32, kNone}, 1, kRBits},
    {"ffbl", "v_ffbl_b32", kGroupBit, kExact, {kU32, kU32, kNone}, 1, kRBits},

    {"add_f32", "v_add_f32", kGroupF32, kExact, {kF32, kF32, kNone}, 1, kRF32},
    {"mul_f32", "v_mul_f32", kGroupF32, kExact, {kF32, kF32, kNone}, 1, kRF32},
    {"fma_f32", "v_fma_f32", kGroupF32, kExact, {kF32, kF32, kF32}, 1, kRF32},
    {"pk_fma_f32", "v_pk_fma_f32", kGroupF32, kExact, {kF32x2, kF32x2, kF32x2}, 2, kRF32},
    {"div_f32", "v_div_fixup_f32", kGroupF32, kExact, {kF32, kF32, kNone}, 1, kRF32},
    {"sqrt_f32", "v_sqrt_f32", kGroupF32, kExact, {kF32Pos, kNone, kNone}, 1, kRF32},
    {"med3_f32", "v_med3_f32", kGroupF32, kExact, {kF32, kF32, kF32}, 1, kRF32},
    {"ldexp_f32", "v_ldexp_f32", kGroupF32, kExact, {kF32, kSmallInt, kNone}, 1, kRF32},
    {"frexp_mant_f32", "v_frexp_mant_f32", kGroupF32, kExact, {kF32, kNone, kNone}, 1, kRF32},
    {"frexp_exp_f32", "v_frexp_exp_i32_f32", kGroupF32, kExact, {kF32, kNone, kNone}, 1, kRBits},
    {"fract_f32", "v_fract_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRF32},
    {"rndne_f32", "v_rndne_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRF32},
    {"floor_f32", "v_floor_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRF32},
    {"cvt_i32_f32", "v_cvt_i32_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRBits},
    {"cvt_f32_i32", "v_cvt_f32_i32", kGroupF32, kExact, {kU32, kNone, kNone}, 1, kRF32},
    {"cvt_f32_ubyte", "v_cvt_f32_ubyte3", kGroupF32, kExact, {kU32, kNone, kNone}, 4, kRF32},
    {"class_f32", "v_cmp_class_f32", kGroupF32, kExact, {kF32Zero, kU32, kNone}, 1, kRBits},
    {"pk_mul_f32", "v_pk_mul_f32", kGroupF32, kExact, {kF32x2, kF32x2, kNone}, 2, kRF32},
    {"pk_add_f32", "v_pk_add_f32", kGroupF32, kExact, {kF32x2, kF32x2, kNone}, 2, kRF32},
    {"min_f32", "v_min_f32", kGroupF32, kExact, {kF32, kF32, kNone}, 1, kRF32},
    {"max_f32", "v_max_f32", kGroupF32, kExact, {kF32, kF32, kNone}, 1, kRF32},
    {"ceil_f32", "v_ceil_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRF32},
    {"trunc_f32", "v_trunc_f32", kGroupF32, kExact, {kF32Big, kNone, kNone}, 1, kRF32},
    {"cvt_u32_f32", "v_cvt_u32_f32", kGroupF32, kExact, {kF32Pos, kNone, kNone}, 1, kRBits},
    {"cvt_f32_u32", "v_cvt_f32_u32", kGroupF32, kExact, {kU32, kNone, kNone}, 1, kRF32},

    {"add_f64", "v_add_f64", kGroupF64, kExact, {kF64, kF64, kNone}, 2, kRF64},
    {"fma_f64", "v_fma_f64", kGroupF64, kExact, {kF64, kF64, kF64}, 2, kRF64},
    {"div_f64", "v_div_fixup_f64", kGroupF64, kExact, {kF64, kF64, kNone}, 2, kRF64},
    {"sqrt_f64", "v_rsq_f64", kGroupF64, kExact, {kF64Pos, kNone, kNone}, 2, kRF64},
    {"cvt_f32_f64", "v_cvt_f32_f64", kGroupF64, kExact, {kF64, kNone, kNone}, 1, kRF32},
    {"mul_f64", "v_mul_f64", kGroupF64, kExact, {kF64, kF64, kNone}, 2, kRF64},
    {"cvt_f64_f32", "v_cvt_f64_f32", kGroupF64, kExact, {kF32, kNone, kNone}, 2, kRF64},
    {"cvt_i32_f64", "v_cvt_i32_f64", kGroupF64, kExact, {kF64Big, kNone, kNone}, 1, kRBits},
    {"cvt_f64_i32", "v_cvt_f64_i32", kGroupF64, kExact, {kU32, kNone, kNone}, 2, kRF64},

    {"pk_fma_f16", "v_pk_fma_f16", kGroupF16, kExact, {kF16x2, kF16x2, kF16x2}, 1, kRF16x2},
    {"pk_add_f16", "v_pk_add_f16", kGroupF16, kExact, {kF16x2, kF16x2, kNone}, 1, kRF16x2},
    {"fdot2", "v_dot2c_f32_f16", kGroupF16, kExact, {kF16x2Int, kF16x2Int, kF32Int}, 1, kRF32},
    {"fdot2_f32_bf16", "v_dot2c_f32_bf16", kGroupF16, kExact, {kBf16x2Int, kBf16x2Int, kF32Int}, 1, kRF32},
    {"cvt_pkrtz", "v_cvt_pkrtz_f16_f32", kGroupF16, kExact, {kF32, kF32, kNone}, 1, kRF16x2},
    {"cvt_f32_f16", "v_cvt_f32_f16", kGroupF16, kExact, {kF16N, kNone, kNone}, 1, kRF32},
    {"cvt_pk_bf16_f32", "v_cvt_pk_bf16_f32", kGroupF16, kExact, {kF32, kF32, kNone}, 1, kRBits},
    {"pk_mul_f16", "v_pk_mul_f16", kGroupF16, kExact, {kF16x2, kF16x2, kNone}, 1, kRF16x2},
    {"cvt_f16_f32", "v_cvt_f16_f32", kGroupF16, kExact, {kF32, kNone, kNone}, 1, kRF16x2},

    {"cvt_f32_fp8", "v_cvt_f32_fp8", kGroupCvt, kExact, {kFp8Word, kNone, kNone}, 4, kRF32},
    {"cvt_f32_bf8", "v_cvt_f32_bf8", kGroupCvt, kExact, {kBf8Word, kNone, kNone}, 4, kRF32},
    {"cvt_pk_f32_fp8", "v_cvt_pk_f32_fp8", kGroupCvt, kExact, {kFp8Word, kNone, kNone}, 4, kRF32},
    {"cvt_scalef32_pk_f32_fp8", "v_cvt_scalef32_pk_f32_fp8", kGroupCvt, kExact, {kFp8Word, kNone, kScale}, 4, kRF32},
    {"cvt_scalef32_pk_f32_bf8", "v_cvt_scalef32_pk_f32_bf8", kGroupCvt, kExact, {kBf8Word, kNone, kScale}, 4, kRF32},
    {"cvt_scalef32_pk_f32_fp4", "v_cvt_scalef32_pk_f32_fp4", kGroupCvt, kExact, {kFp4Word, kNone, kScale}, 8, kRF32},
    {"cvt_pk_fp8_f32", "v_cvt_pk_fp8_f32", kGroupCvt, kExact, {kEncFp8, kEncFp8, kNone}, 1, kRBits},
    {"cvt_pk_bf8_f32", "v_cvt_pk_bf8_f32", kGroupCvt, kExact, {kEncBf8, kEncBf8, kNone}, 1, kRBits},
    {"cvt_scalef32_pk_fp8_f32", "v_cvt_scalef32_pk_fp8_f32", kGroupCvt, kExact, {kEncFp8, kEncFp8, kScale}, 1, kRBits},
    {"cvt_scalef32_pk_bf8_f32", "v_cvt_scalef32_pk_bf8_f32", kGroupCvt, kExact, {kEncBf8, kEncBf8, kScale}, 1, kRBits},
    {"cvt_scalef32_pk_fp4_f32", "v_cvt_scalef32_pk_fp4_f32", kGroupCvt, kExact, {kEncFp4, kEncFp4, kScale}, 1, kRBits},
    {"cvt_pk_f32_bf8", "v_cvt_pk_f32_bf8", kGroupCvt, kExact, {kBf8Word, kNone, kNone}, 4, kRF32},
    {"cvt_scalef32_pk32_f32_fp6", "v_cvt_scalef32_pk32_f32_fp6", kGroupCvt, kExact, {kFp6Codes, kNone, kScale}, 32, kRF32},
    {"cvt_scalef32_pk32_f32_bf6", "v_cvt_scalef32_pk32_f32_bf6", kGroupCvt, kExact, {kFp6Codes, kNone, kScale}, 32, kRF32},
    {"cvt_scalef32_2xpk16_fp6_f32", "v_cvt_scalef32_2xpk16_fp6_f32", kGroupCvt, kExact, {kEncSeed, kNone, kScale}, 6, kRBits},
    {"cvt_scalef32_2xpk16_bf6_f32", "v_cvt_scalef32_2xpk16_bf6_f32", kGroupCvt, kExact, {kEncSeed, kNone, kScale}, 6, kRBits},

    {"exp2_f32", "v_exp_f32", kGroupApprox, kConsensus, {kF32Exp, kNone, kNone}, 1, kRF32},
    {"log2_f32", "v_log_f32", kGroupApprox, kConsensus, {kF32Pos, kNone, kNone}, 1, kRF32},
    {"rcp_f32", "v_rcp_f32", kGroupApprox, kConsensus, {kF32, kNone, kNone}, 1, kRF32},
    {"rsq_f32", "v_rsq_f32", kGroupApprox, kConsensus, {kF32Pos, kNone, kNone}, 1, kRF32},
    {"sqrt_raw_f32", "v_sqrt_f32", kGroupApprox, kConsensus, {kF32Pos, kNone, kNone}, 1, kRF32},
    {"sin_f32", "v_sin_f32", kGroupApprox, kConsensus, {kF32Sin, kNone, kNone}, 1, kRF32},
    {"cos_f32", "v_cos_f32", kGroupApprox, kConsensus, {kF32Cos, kNone, kNone}, 1, kRF32},
    {"rcp_f64", "v_rcp_f64", kGroupApprox, kConsensus, {kF64, kNone, kNone}, 2, kRF64},
    {"rsq_f64", "v_rsq_f64", kGroupApprox, kConsensus, {kF64Pos, kNone, kNone}, 2, kRF64},
    {"prng_b32", "v_prng_b32", kGroupApprox, kConsensus, {kU32, kNone, kNone}, 1, kRBits},
    {"cvt_sr_fp8_f32", "v_cvt_sr_fp8_f32", kGroupApprox, kConsensus, {kEncFp8, kU32, kNone}, 1, kRBits},
    {"exp2_f16", "v_exp_f16", kGroupApprox, kConsensus, {kF16Small, kNone, kNone}, 1, kRBits},
    {"log2_f16", "v_log_f16", kGroupApprox, kConsensus, {kF16Pos, kNone, kNone}, 1, kRBits},
    {"rcp_f16", "v_rcp_f16", kGroupApprox, kConsensus, {kF16Mid, kNone, kNone}, 1, kRBits},
    {"cvt_scalef32_sr_pk_fp4_f32", "v_cvt_scalef32_sr_pk_fp4_f32", kGroupApprox, kConsensus, {kEncFp4, kEncFp4, kScale}, 1, kRBits},
};
static_assert(sizeof(kOps) / sizeof(kOps[0]) == kNumOps, "one row per Op");

// A group's ops are contiguous in the table.
constexpr int group_first(int g) {
  for (int i = 0; i < kNumOps; ++i)
    if (kOps[i].group == g) return i;
  return kNumOps;
}
constexpr int group_count(int g) {
  int n = 0;
  for (int i = 0; i < kNumOps; ++i) n += kOps[i].group == g;
  return n;
}
constexpr bool groups_fit() {
  for (int g = 0; g < kNumGroups; ++g) {
    if (group_count(g) < 1 || group_count(g) > kMaxGroupOps) return false;
    for (int i = 0; i < group_count(g); ++i)
      if (kOps[group_first(g) + i].group != g) return false;
  }
  return true;
}
static_assert(groups_fit(), "every group is one run of at most kMaxGroupOps rows");

// ---- bits and formats --------------------------------------------------------------------------
FORMS_HD uint32_t bits_of(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
FORMS_HD float f32_of(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
FORMS_HD uint64_t bits_of(double f) {
  uint64_t u;
  __builtin_memcpy(&u, &f, 8);
  return u;
}
FORMS_HD double f64_of(uint64_t u) {
  double f;
  __builtin_memcpy(&f, &u, 8);
  return f;
}
FORMS_HD float pow2f(int k) { return f32_of(static_cast<uint32_t>(127 + k) << 23); }  // k in the normal range
FORMS_HD uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

// A small binary format: e exponent bits, m mantissa bits, its bias, and how many of its
// magnitude codes (from 0 up) are finite.
struct Fmt {
  int e, m, bias, finite;
};
constexpr Fmt kE4M3 = {4, 3, 7, 127}, kE5M2 = {5, 2, 15, 124}, kE2M1 = {2, 1, 1, 8}, kHalf = {5, 10, 15, 31744};
constexpr Fmt kE2M3 = {2, 3, 1, 32}, kE3M2 = {3, 2, 3, 32};  // fp6, bf6

// The value of magnitude code `code` (no sign bit), exact in f32.
FORMS_HD float lowp_value(Fmt f, uint32_t code) {
  const uint32_t e = code >> f.m, m = code & ((1u << f.m) - 1u);
  if (e == 0) return static_cast<float>(m) * pow2f(1 - f.bias - f.m);
  return f32_of(((e - f.bias + 127u) << 23) | (m << (23 - f.m)));
}
FORMS_HD float lowp_decode(Fmt f, uint32_t code) {
  const float v = lowp_value(f, code & ((1u << (f.e + f.m)) - 1u));
  return (code >> (f.e + f.m)) & 1u ? -v : v;
}

// ---- the operand generator -----------------------------------------------------------------------
FORMS_HD uint64_t op_hash(uint32_t seed, int op, int round, int lane, int which) {
  return fmix64((static_cast<uint64_t>(seed) << 32) ^ (static_cast<uint64_t>(op) << 24) ^ (static_cast<uint64_t>(round) << 16) ^
                (static_cast<uint64_t>(lane) << 8) ^ static_cast<uint64_t>(which) ^ 0x9E3779B97F4A7C15ull);
}
FORMS_HD uint32_t f32_in(uint64_t h, int emin, int emax, bool positive) {
  const uint32_t e = 127u + emin + static_cast<uint32_t>((h >> 32) & 0xFFFFu) % static_cast<uint32_t>(emax - emin + 1);
  return (positive ? 0u : static_cast<uint32_t>(h >> 63) << 31) | (e << 23) | (static_cast<uint32_t>(h) & 0x7FFFFFu);
}
FORMS_HD uint64_t f64_in(uint64_t h, uint64_t h2, bool positive) {
  const uint64_t e = 1023u - 60u + (h2 & 0xFFFFu) % 121u;
  return (positive ? 0ull : (h2 >> 63) << 63) | (e << 52) | (h & 0xFFFFFFFFFFFFFull);
}
FORMS_HD int small_int(uint32_t h, int r) { return static_cast<int>(h % static_cast<uint32_t>(2 * r + 1)) - r; }
FORMS_HD uint32_t f16_of_small_int(int v) {  // |v| <= 2048
  const uint32_t u = bits_of(static_cast<float>(v));
  return v == 0 ? 0u : ((u >> 16) & 0x8000u) | ((((u >> 23) & 0xFFu) - 112u) << 10) | ((u >> 13) & 0x3FFu);
}
FORMS_HD int scale_exp_of(uint64_t h) { return static_cast<int>(h % 5u) - 2; }

// An encoder's input for format f: a representable value, the midpoint of two neighbours (the
// tie), a value just above or below that midpoint, or zero; of either sign; times 2^scale_exp.
// Every step is exact in f32.
FORMS_HD uint32_t enc_input(Fmt f, uint64_t h, int scale_exp) {
  const int variant = static_cast<int>((h >> 40) & 7u);
  const bool mid = variant >= 2 && variant <= 5;
  const uint32_t i = static_cast<uint32_t>(h & 0xFFFFFFu) % static_cast<uint32_t>(mid ? f.finite - 1 : f.finite);
  float v = lowp_value(f, i);
  if (mid) v = 0.5f * (v + lowp_value(f, i + 1));
  if (variant == 4) v = v + v * pow2f(-18);
  if (variant == 5) v = v - v * pow2f(-18);
  if (variant == 7) v = 0.f;
  v = v * pow2f(scale_exp);
  return bits_of(v) | (static_cast<uint32_t>(h >> 63) << 31);
}

// Four codes per lane so that the 64 lanes of a round hold every byte value once; a code the
// format reads as NaN or infinity is replaced by a finite one.
FORMS_HD uint32_t code_word(int kind, uint32_t seed, int round, int lane) {
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j) {
    uint32_t b = (static_cast<uint32_t>(lane) * 4u + j + static_cast<uint32_t>(round) * 67u + seed * 13u) & 0xFFu;
    if (kind == kFp8Word && (b & 0x7Fu) == 0x7Fu) b ^= 1u;
    if (kind == kBf8Word && (b & 0x7Cu) == 0x7Cu) b ^= 4u;
    w |= b << (8 * j);
  }
  return w;
}

// Operand `which` (0 a, 1 b, 2 c) of op `op` in round `round` of lane `lane`.
FORMS_HD uint64_t operand(uint32_t seed, int op, int round, int lane, int which) {
  const int kind = kOps[op].kind[which];
  const uint64_t h = op_hash(seed, op, round, lane, which);
  const uint32_t lo = static_cast<uint32_t>(h), hi = static_cast<uint32_t>(h >> 32);
  switch (kind) {
    case kU32: return lo;
    case kU64: return h;
    case kPermSel: {
      uint32_t s = 0;
      for (int j = 0; j < 4; ++j) {
        const uint32_t n = (lo >> (4 * j)) & 0xFu;
        s |= (n < 8 ? n : 12u + (n & 1u)) << (8 * j);
      }
      return s;
    }
    case kSmallInt: return static_cast<uint32_t>(small_int(lo, 8));
    case kF32: return f32_in(h, -12, 12, false);
    case kF32Pos: return f32_in(h, -12, 12, true);
    case kF32Big: return f32_in(h, 0, 12, false);
    case kF32Zero: return (hi >> 16 & 3u) == 0 ? (hi >> 31) << 31 : f32_in(h, -12, 12, false);
    case kF32Int: return bits_of(static_cast<float>(small_int(lo, 64)));
    case kF32Exp: return f32_in(h, -12, 5, false);
    case kF32Sin: return f32_in(h, -8, -3, false);
    case kF32Cos: return f32_in(h, -8, -4, false);
    case kF32x2: return f32_in(h, -12, 12, false) | static_cast<uint64_t>(f32_in(fmix64(h), -12, 12, false)) << 32;
    case kF64: return f64_in(h, fmix64(h), false);
    case kF64Pos: return f64_in(h, fmix64(h), true);
    case kF64Big: return ((h >> 63) << 63) | ((1023ull + (fmix64(h) & 0xFFFFu) % 21u) << 52) | (h & 0xFFFFFFFFFFFFFull);
    case kF16N: return (lo & 0x83FFu) | ((1u + (hi & 0xFFFFu) % 30u) << 10);
    case kF16Small: return (lo & 0x83FFu) | ((7u + (hi & 0xFFFFu) % 11u) << 10);
    case kF16Mid: return (lo & 0x83FFu) | ((5u + (hi & 0xFFFFu) % 21u) << 10);
    case kF16Pos: return (lo & 0x03FFu) | ((5u + (hi & 0xFFFFu) % 21u) << 10);
    case kFp6Codes: return (static_cast<uint32_t>(lane) + static_cast<uint32_t>(round) * 29u + seed * 13u) & 63u;
    case kEncSeed: return h;
    case kF16x2: {
      uint32_t w = 0;
      for (int j = 0; j < 2; ++j) {
        const uint32_t x = lo >> (16 * j);
        w |= ((x & 0x8000u) | ((15u + ((x >> 10) & 3u)) << 10) | (x & 0x3F0u)) << (16 * j);
      }
      return w;
    }
    case kF16x2Int: return f16_of_small_int(small_int(lo, 8)) | f16_of_small_int(small_int(hi, 8)) << 16;
    case kBf16x2Int:
      return (bits_of(static_cast<float>(small_int(lo, 8))) >> 16) | (bits_of(static_cast<float>(small_int(hi, 8))) & 0xFFFF0000u);
    case kFp8Word:
    case kBf8Word:
    case kFp4Word: return code_word(kind, seed, round, lane);
    case kScale: return bits_of(pow2f(scale_exp_of(h)));
    case kEncFp8:
    case kEncBf8:
    case kEncFp4: {
      const int s = kOps[op].kind[2] == kScale ? scale_exp_of(op_hash(seed, op, round, lane, 2)) : 0;
      return enc_input(kind == kEncFp8 ? kE4M3 : kind == kEncBf8 ? kE5M2 : kE2M1, h, s);
    }
    default: return 0;
  }
}

// The 32 elements of a wide conversion's operand, from its operand word a and its scale c: the
// six-bit codes of a pk32 decoder, the f32 encoder inputs of a 2xpk16 encoder.
constexpr int kWide = 32;
FORMS_HD bool is_wide(int op) { return kOps[op].kind[0] == kFp6Codes || kOps[op].kind[0] == kEncSeed; }
FORMS_HD Fmt wide_fmt(int op) { return op == kScalePk32F32Fp6 || op == kScale2xPk16Fp6 ? kE2M3 : kE3M2; }
FORMS_HD uint32_t expand(int op, uint64_t a, uint64_t c, int j) {
  if (kOps[op].kind[0] == kFp6Codes) return (static_cast<uint32_t>(a) + static_cast<uint32_t>(j)) & 63u;
  return enc_input(wide_fmt(op), fmix64(a + static_cast<uint64_t>(j)),
                   static_cast<int>((static_cast<uint32_t>(c) >> 23) & 0xFFu) - 127);
}
// six-bit element j of six packed words
FORMS_HD void put6(uint32_t* w, int j, uint32_t code) {
  const int p = j * 6, i = p >> 5, sh = p & 31;
  w[i] |= code << sh;
  if (sh + 6 > 32) w[i + 1] |= code >> (32 - sh);
}

// The fold of an op's result words into a lane's digest, and of the lanes' digests into a wave's.
FORMS_HD uint32_t fold(uint32_t digest, uint32_t word) { return rotl32(digest, 5) ^ (word * 0x9E3779B1u); }
FORMS_HD uint32_t lane_weight(int lane) { return 2u * static_cast<uint32_t>(lane) + 1u; }  // wave digest: sum of digest * weight

// The canonical forms of arguments both sides derive from a raw operand.
FORMS_HD uint32_t bfe_width(uint32_t off, uint32_t c) { return 1u + c % (32u - off > 31u ? 31u : 32u - off); }  // off + width <= 32
FORMS_HD uint32_t lanes_below(uint32_t mask, int lane, int half) {  // bits of `mask` below the lane within its half of the wave
  const int n = lane - 32 * half;
  return n <= 0 ? 0u : n >= 32 ? mask : mask & ((1u << n) - 1u);
}

// ---- the host references: plain integer, float and double arithmetic -------------------------------
inline bool f32_ok(uint32_t u) { return (u << 1) == 0 || (((u >> 23) & 0xFFu) != 0 && ((u >> 23) & 0xFFu) != 0xFFu); }
inline bool f64_ok(uint64_t u) { return (u << 1) == 0 || (((u >> 52) & 0x7FFu) != 0 && ((u >> 52) & 0x7FFu) != 0x7FFu); }
inline bool f16_ok(uint32_t u) { return (u & 0x7FFFu) == 0 || (((u >> 10) & 0x1Fu) != 0 && ((u >> 10) & 0x1Fu) != 0x1Fu); }

// The code of format f nearest to x, ties to the even code (|x| within the format's finite range).
inline uint32_t lowp_encode(Fmt f, double x) {
  const uint32_t sign = std::signbit(x) ? 1u << (f.e + f.m) : 0u;
  const double ax = std::fabs(x);
  if (ax == 0) return sign;
  int e;
  std::frexp(ax, &e);  // ax = m 2^e, m in [0.5, 1)
  const int E = e - 1 < 1 - f.bias ? 1 - f.bias : e - 1;
  const double r = std::nearbyint(std::ldexp(ax, f.m - E));  // round to nearest even
  return sign | ((static_cast<uint32_t>(E + f.bias - 1) << f.m) + static_cast<uint32_t>(r));
}
inline double half_value(uint32_t h) { return static_cast<double>(lowp_decode(kHalf, h & 0xFFFFu)); }
inline uint32_t bf16_rne(uint32_t u) { return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16; }
inline int32_t s4(uint32_t x) { return static_cast<int32_t>((x & 0xFu) ^ 8u) - 8; }
inline uint32_t sat_i8(int32_t v) { return static_cast<uint32_t>(v < -128 ? -128 : v > 127 ? 127 : v) & 0xFFu; }
inline uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c, uint32_t table) {
  uint32_t d = 0;
  for (int i = 0; i < 32; ++i) d |= ((table >> ((((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u))) & 1u) << i;
  return d;
}
inline uint32_t perm_b32(uint32_t a, uint32_t b, uint32_t sel) {
  const uint64_t both = (static_cast<uint64_t>(a) << 32) | b;
  uint32_t d = 0;
  for (int j = 0; j < 4; ++j) {
    const uint32_t s = (sel >> (8 * j)) & 0xFFu;
    d |= (s < 8 ? static_cast<uint32_t>(both >> (8 * s)) & 0xFFu : s == 12 ? 0u : 0xFFu) << (8 * j);
  }
  return d;
}
inline float median(float a, float b, float c) {
  const float lo = a < b ? a : b, hi = a < b ? b : a;
  return c < lo ? lo : c > hi ? hi : c;
}
inline void put_f64(double v, uint32_t* r) {
  const uint64_t u = bits_of(v);
  r[0] = static_cast<uint32_t>(u);
  r[1] = static_cast<uint32_t>(u >> 32);
}
inline void put_u64(uint64_t u, uint32_t* r) {
  r[0] = static_cast<uint32_t>(u);
  r[1] = static_cast<uint32_t>(u >> 32);
}

// The result words of exact op `op` on operands a, b, c in lane `lane`; false: not an exact op.
inline bool reference(int op, uint64_t a64, uint64_t b64, uint64_t c64, int lane, uint32_t* r) {
  const uint32_t a = static_cast<uint32_t>(a64), b = static_cast<uint32_t>(b64), c = static_cast<uint32_t>(c64);
  const int32_t ai = static_cast<int32_t>(a), bi = static_cast<int32_t>(b);
  const float af = f32_of(a), bf = f32_of(b), cf = f32_of(c);
  const double ad = f64_of(a64), bd = f64_of(b64), cd = f64_of(c64);
  const float scale = cf;  // of the scaled conversions
  switch (op) {
    case kMulLoU32: r[0] = a * b; break;
    case kMulHiU32: r[0] = static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32); break;
    case kMulHiI32: r[0] = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(ai) * bi) >> 32); break;
    case kMadU64U32: put_u64(static_cast<uint64_t>(a) * b + c64, r); break;
    case kMadI64I32: put_u64(static_cast<uint64_t>(static_cast<int64_t>(ai) * bi) + c64, r); break;
    case kAdd3U32: r[0] = a + b + c; break;
    case kLshlB64: put_u64(a64 << (b & 63u), r); break;
    case kPkAddU16: r[0] = ((a + b) & 0xFFFFu) | (((a >> 16) + (b >> 16)) << 16); break;
    case kPkMulLoU16: r[0] = (((a & 0xFFFFu) * (b & 0xFFFFu)) & 0xFFFFu) | (((a >> 16) * (b >> 16)) << 16); break;
    case kSdot4:
    case kUdot4: {
      uint32_t s = c;
      for (int j = 0; j < 4; ++j) {
        const uint32_t x = (a >> (8 * j)) & 0xFFu, y = (b >> (8 * j)) & 0xFFu;
        s += op == kUdot4 ? x * y : static_cast<uint32_t>(static_cast<int8_t>(x) * static_cast<int8_t>(y));
      }
      r[0] = s;
      break;
    }
    case kSadU8: {
      uint32_t s = c;
      for (int j = 0; j < 4; ++j) {
        const int x = (a >> (8 * j)) & 0xFF, y = (b >> (8 * j)) & 0xFF;
        s += static_cast<uint32_t>(x > y ? x - y : y - x);
      }
      r[0] = s;
      break;
    }
    case kLerpU8: {
      r[0] = 0;
      for (int j = 0; j < 4; ++j)
        r[0] |= ((((a >> (8 * j)) & 0xFFu) + ((b >> (8 * j)) & 0xFFu) + ((c >> (8 * j)) & 1u)) >> 1) << (8 * j);
      break;
    }
    case kLshlAddU32: r[0] = (a << (b & 3u)) + c; break;
    case kAshrI64: put_u64(static_cast<uint64_t>(static_cast<int64_t>(a64) >> (b & 63u)), r); break;
    case kMinI32: r[0] = static_cast<uint32_t>(ai < bi ? ai : bi); break;
    case kMaxU32: r[0] = a > b ? a : b; break;
    case kMed3I32: {
      const int32_t ci = static_cast<int32_t>(c), lo = ai < bi ? ai : bi, hi = ai < bi ? bi : ai;
      r[0] = static_cast<uint32_t>(ci < lo ? lo : ci > hi ? hi : ci);
      break;
    }
    case kMed3U32: {
      const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
      r[0] = c < lo ? lo : c > hi ? hi : c;
      break;
    }
    case kPkMadU16: r[0] = (((a & 0xFFFFu) * (b & 0xFFFFu) + (c & 0xFFFFu)) & 0xFFFFu) | (((a >> 16) * (b >> 16) + (c >> 16)) << 16); break;
    case kPkMinI16:
    case kPkMaxU16:
    case kPkLshlB16:
      r[0] = 0;
      for (int j = 0; j < 2; ++j) {
        const uint32_t x = (a >> (16 * j)) & 0xFFFFu, y = (b >> (16 * j)) & 0xFFFFu;
        const uint32_t v = op == kPkMinI16 ? (static_cast<int16_t>(x) < static_cast<int16_t>(y) ? x : y)
                           : op == kPkMaxU16 ? (x > y ? x : y) : (x << (y & 15u)) & 0xFFFFu;
        r[0] |= v << (16 * j);
      }
      break;
    case kSdot8:
    case kUdot8: {
      uint32_t s = c;
      for (int j = 0; j < 8; ++j) {
        const uint32_t x = (a >> (4 * j)) & 0xFu, y = (b >> (4 * j)) & 0xFu;
        s += op == kUdot8 ? x * y : static_cast<uint32_t>(s4(x) * s4(y));
      }
      r[0] = s;
      break;
    }
    case kSdot2: r[0] = c + static_cast<uint32_t>(static_cast<int16_t>(a) * static_cast<int16_t>(b)) +
                        static_cast<uint32_t>(static_cast<int16_t>(a >> 16) * static_cast<int16_t>(b >> 16)); break;
    case kMsadU8: {  // bytes whose reference byte (b) is zero are skipped
      uint32_t s = c;
      for (int j = 0; j < 4; ++j) {
        const int x = (a >> (8 * j)) & 0xFF, y = (b >> (8 * j)) & 0xFF;
        if (y != 0) s += static_cast<uint32_t>(x > y ? x - y : y - x);
      }
      r[0] = s;
      break;
    }
    case kFfbl: {
      const uint32_t x = (a << (b & 31u)) | 0x80000000u;
      r[0] = 0;
      while (!((x >> r[0]) & 1u)) ++r[0];
      break;
    }
    case kPermB32: r[0] = perm_b32(a, b, c); break;
    case kAlignBit: r[0] = static_cast<uint32_t>(((static_cast<uint64_t>(a) << 32) | b) >> (c & 31u)); break;
    case kAlignByte: r[0] = static_cast<uint32_t>(((static_cast<uint64_t>(a) << 32) | b) >> (8 * (c & 3u))); break;
    case kBfeU32: r[0] = (a >> (b & 31u)) & ((1u << bfe_width(b & 31u, c)) - 1u); break;
    case kBfeI32: {
      const uint32_t w = bfe_width(b & 31u, c), v = (a >> (b & 31u)) & ((1u << w) - 1u);
      r[0] = (v >> (w - 1)) & 1u ? v | ~((1u << w) - 1u) : v;
      break;
    }
    case kBfrev: {
      r[0] = 0;
      for (int i = 0; i < 32; ++i) r[0] |= ((a >> i) & 1u) << (31 - i);
      break;
    }
    case kBcnt: {
      r[0] = b;
      for (int i = 0; i < 32; ++i) r[0] += (a >> i) & 1u;
      break;
    }
    case kFfbh: {
      const uint32_t x = (a >> (b & 31u)) | 1u;
      r[0] = 0;
      while (!((x << r[0]) & 0x80000000u)) ++r[0];
      break;
    }
    case kBitop96: r[0] = bitop3(a, b, c, 0x96); break;
    case kBitopE8: r[0] = bitop3(a, b, c, 0xE8); break;
    case kBitopCA: r[0] = bitop3(a, b, c, 0xCA); break;
    case kBitop6B: r[0] = bitop3(a, b, c, 0x6B); break;
    case kAshrPkI8: r[0] = sat_i8(ai >> (c & 31u)) | (sat_i8(bi >> (c & 31u)) << 8); break;
    case kMbcnt: {
      uint32_t n = 0;
      for (int half = 0; half < 2; ++half) {
        const uint32_t m = lanes_below(half ? b : a, lane, half);
        for (int i = 0; i < 32; ++i) n += (m >> i) & 1u;
      }
      r[0] = n;
      break;
    }
    case kAddF32: r[0] = bits_of(af + bf); break;
    case kMulF32: r[0] = bits_of(af * bf); break;
    case kFmaF32: r[0] = bits_of(std::fma(af, bf, cf)); break;
    case kPkFmaF32:
      r[0] = bits_of(std::fma(af, bf, cf));
      r[1] = bits_of(std::fma(f32_of(a64 >> 32), f32_of(b64 >> 32), f32_of(c64 >> 32)));
      break;
    case kDivF32: r[0] = bits_of(af / bf); break;
    case kSqrtF32: r[0] = bits_of(std::sqrt(af)); break;
    case kMed3F32: r[0] = bits_of(median(af, bf, cf)); break;
    case kLdexpF32: r[0] = bits_of(std::ldexp(af, bi)); break;
    case kFrexpMantF32: {
      int e;
      r[0] = bits_of(std::frexp(af, &e));
      break;
    }
    case kFrexpExpF32: {
      int e;
      std::frexp(af, &e);
      r[0] = static_cast<uint32_t>(e);
      break;
    }
    case kFractF32: r[0] = bits_of(af - std::floor(af)); break;  // exact for |x| >= 1
    case kRndneF32: r[0] = bits_of(std::nearbyint(af)); break;
    case kFloorF32: r[0] = bits_of(std::floor(af)); break;
    case kCvtI32F32: r[0] = static_cast<uint32_t>(static_cast<int32_t>(af)); break;
    case kCvtF32I32: r[0] = bits_of(static_cast<float>(ai)); break;
    case kCvtF32Ubyte:
      for (int j = 0; j < 4; ++j) r[j] = bits_of(static_cast<float>((a >> (8 * j)) & 0xFFu));
      break;
    case kClassF32: {  // the mask's bit of the value's class: 3 -normal, 5 -0, 6 +0, 8 +normal
      const bool neg = a >> 31, zero = (a << 1) == 0;
      r[0] = (b >> (zero ? (neg ? 5 : 6) : (neg ? 3 : 8))) & 1u;
      break;
    }
    case kPkMulF32:
      r[0] = bits_of(af * bf);
      r[1] = bits_of(f32_of(a64 >> 32) * f32_of(b64 >> 32));
      break;
    case kPkAddF32:
      r[0] = bits_of(af + bf);
      r[1] = bits_of(f32_of(a64 >> 32) + f32_of(b64 >> 32));
      break;
    case kMinF32: r[0] = bits_of(af < bf ? af : bf); break;
    case kMaxF32: r[0] = bits_of(af > bf ? af : bf); break;
    case kCeilF32: r[0] = bits_of(std::ceil(af)); break;
    case kTruncF32: r[0] = bits_of(std::trunc(af)); break;
    case kCvtU32F32: r[0] = static_cast<uint32_t>(af); break;
    case kCvtF32U32: r[0] = bits_of(static_cast<float>(a)); break;
    case kMulF64: put_f64(ad * bd, r); break;
    case kCvtF64F32: put_f64(static_cast<double>(af), r); break;
    case kCvtI32F64: r[0] = static_cast<uint32_t>(static_cast<int32_t>(ad)); break;
    case kCvtF64I32: put_f64(static_cast<double>(ai), r); break;
    case kAddF64: put_f64(ad + bd, r); break;
    case kFmaF64: put_f64(std::fma(ad, bd, cd), r); break;
    case kDivF64: put_f64(ad / bd, r); break;
    case kSqrtF64: put_f64(std::sqrt(ad), r); break;
    case kCvtF32F64: r[0] = bits_of(static_cast<float>(ad)); break;
    case kPkFmaF16:
    case kPkMulF16:
    case kPkAddF16:
      r[0] = 0;
      for (int j = 0; j < 2; ++j) {  // exact in double, then one rounding
        const double x = half_value(a >> (16 * j)), y = half_value(b >> (16 * j)), z = half_value(c >> (16 * j));
        r[0] |= lowp_encode(kHalf, op == kPkFmaF16 ? x * y + z : op == kPkMulF16 ? x * y : x + y) << (16 * j);
      }
      break;
    case kFdot2: r[0] = bits_of(static_cast<float>(half_value(a) * half_value(b) + half_value(a >> 16) * half_value(b >> 16) + cf)); break;
    case kFdot2Bf16:
      r[0] = bits_of(f32_of(a << 16) * f32_of(b << 16) + f32_of(a & 0xFFFF0000u) * f32_of(b & 0xFFFF0000u) + cf);  // small integers
      break;
    case kCvtPkrtz: {
      r[0] = 0;
      for (int j = 0; j < 2; ++j) {
        const uint32_t u = j ? b : a;
        r[0] |= (((u >> 16) & 0x8000u) | ((((u >> 23) & 0xFFu) - 112u) << 10) | ((u >> 13) & 0x3FFu)) << (16 * j);  // truncation
      }
      break;
    }
    case kCvtF16F32: r[0] = lowp_encode(kHalf, af); break;
    case kCvtF32F16: r[0] = bits_of(lowp_decode(kHalf, a & 0xFFFFu)); break;
    case kCvtPkBf16F32: r[0] = bf16_rne(a) | (bf16_rne(b) << 16); break;
    case kCvtF32Fp8:
    case kCvtF32Bf8:
      for (int j = 0; j < 4; ++j) r[j] = bits_of(lowp_decode(op == kCvtF32Fp8 ? kE4M3 : kE5M2, (a >> (8 * j)) & 0xFFu));
      break;
    case kCvtPkF32Bf8:
      for (int j = 0; j < 4; ++j) r[j] = bits_of(lowp_decode(kE5M2, (a >> (8 * j)) & 0xFFu));
      break;
    case kScalePk32F32Fp6:
    case kScalePk32F32Bf6:
      for (int j = 0; j < kWide; ++j) r[j] = bits_of(lowp_decode(wide_fmt(op), expand(op, a64, c64, j)) * scale);
      break;
    case kScale2xPk16Fp6:
    case kScale2xPk16Bf6:
      for (int j = 0; j < 6; ++j) r[j] = 0;
      for (int j = 0; j < kWide; ++j)  // the two sources interleave: code j is of element j / 2 of source j % 2
        put6(r, j, lowp_encode(wide_fmt(op), f32_of(expand(op, a64, c64, (j >> 1) + 16 * (j & 1))) / scale));
      break;
    case kCvtPkF32Fp8:
      for (int j = 0; j < 4; ++j) r[j] = bits_of(lowp_decode(kE4M3, (a >> (8 * j)) & 0xFFu));
      break;
    case kScalePkF32Fp8:
    case kScalePkF32Bf8:
      for (int j = 0; j < 4; ++j) r[j] = bits_of(lowp_decode(op == kScalePkF32Fp8 ? kE4M3 : kE5M2, (a >> (8 * j)) & 0xFFu) * scale);
      break;
    case kScalePkF32Fp4:
      for (int j = 0; j < 8; ++j) r[j] = bits_of(lowp_decode(kE2M1, (a >> (4 * j)) & 0xFu) * scale);
      break;
    case kCvtPkFp8F32: r[0] = lowp_encode(kE4M3, af) | (lowp_encode(kE4M3, bf) << 8); break;
    case kCvtPkBf8F32: r[0] = lowp_encode(kE5M2, af) | (lowp_encode(kE5M2, bf) << 8); break;
    case kScalePkFp8F32: r[0] = lowp_encode(kE4M3, af / scale) | (lowp_encode(kE4M3, bf / scale) << 8); break;
    case kScalePkBf8F32: r[0] = lowp_encode(kE5M2, af / scale) | (lowp_encode(kE5M2, bf / scale) << 8); break;
    case kScalePkFp4F32: r[0] = lowp_encode(kE2M1, af / scale) | (lowp_encode(kE2M1, bf / scale) << 4); break;
    default: return false;
  }
  return true;
}

// Every floating operand word of `kind` is a normal number or a zero.
inline bool operand_ok(int kind, uint64_t v) {
  const uint32_t lo = static_cast<uint32_t>(v), hi = static_cast<uint32_t>(v >> 32);
  switch (kind) {
    case kF32: case kF32Pos: case kF32Big: case kF32Zero: case kF32Int: case kF32Exp: case kF32Sin: case kF32Cos: case kScale:
    case kEncFp8: case kEncBf8: case kEncFp4: return f32_ok(lo);
    case kF32x2: return f32_ok(lo) && f32_ok(hi);
    case kF64: case kF64Pos: case kF64Big: return f64_ok(v);
    case kF16N: case kF16Small: case kF16Mid: case kF16Pos: return f16_ok(lo) && (lo & 0x7FFFu) != 0;
    case kF16x2: case kF16x2Int: return f16_ok(lo) && f16_ok(lo >> 16);
    case kBf16x2Int: return f32_ok(lo << 16) && f32_ok(lo & 0xFFFF0000u);
    default: return true;
  }
}
inline bool result_ok(int rkind, int results, const uint32_t* r) {
  for (int i = 0; i < results; ++i) {
    if (rkind == kRF32 && !f32_ok(r[i])) return false;
    if (rkind == kRF16x2 && !(f16_ok(r[i]) && f16_ok(r[i] >> 16))) return false;
    if (rkind == kRF64 && (i & 1) && !f64_ok((static_cast<uint64_t>(r[i]) << 32) | r[i - 1])) return false;
  }
  return true;
}

// The 64 lane digests of exact op `op` over `rounds` rounds: 0; -1: not an exact op or bad
// rounds; -2: a generated case left the range the references are specified for.
inline int expected_digests(int op, uint32_t seed, int rounds, uint32_t* digest) {
  if (op < 0 || op >= kNumOps || kOps[op].cls != kExact || rounds < 1 || rounds > kMaxRounds) return -1;
  for (int lane = 0; lane < kLanes; ++lane) {
    uint32_t d = 0;
    for (int round = 0; round < rounds; ++round) {
      uint64_t v[3];
      for (int w = 0; w < 3; ++w) {
        v[w] = operand(seed, op, round, lane, w);
        if (!operand_ok(kOps[op].kind[w], v[w])) return -2;
      }
      uint32_t r[kMaxResults] = {};
      reference(op, v[0], v[1], v[2], lane, r);
      if (!result_ok(kOps[op].rkind, kOps[op].results, r)) return -2;
      for (int i = 0; i < kOps[op].results; ++i) d = fold(d, r[i]);
    }
    digest[lane] = d;
  }
  return 0;
}
}  // namespace valu
