// MI355X (gfx950 / CDNA4) health canary: the vector-ALU check.
//
// The vector ALU on the instructions no other kernel of the canary issues (valu_ops.h):
// transcendentals, the division and square-root chains, packed and dot-product math, byte and
// bit operations, and the fp8 / bf8 / fp4 conversions of gfx950.  The shape is the site probe's:
// 4-wave workgroups (one wave per SIMD), one resident per CU through the largest dynamic LDS
// allocation, every wave reading its site (canary_common.h) first and last, and lane 0 of every
// wave leaving one record (valu_host.h) in its own slot, records[block * 4 + wave], with ordinary
// vector stores.  No kernel reads a record, no workgroup waits for another, every loop is bounded
// by an argument or a constant, and fault injection perturbs a value that is then compared,
// never an address.  The verdicts are the host's (valu_host.h).
//
//   * valu_sweep<G>: every selected op of group G, `rounds` rounds each, one kernel per group (so
//     none spills).  The workgroup copies the launch's expected lane digests of the group
//     (ops x 64 words) from global memory into LDS once, with 16-byte loads; the op loop compares
//     against LDS.  Operands and results pass an empty asm statement, so no op is folded away,
//     merged with another or computed at compile time;
//   * valu_raw: one op on the caller's operand words, every lane's raw result words out.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/valu.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "valu.h"

namespace {

using namespace canary;
namespace vu = valu;

constexpr int kThreads = kValuWaves * kWave;
constexpr int kExpectWords = vu::kMaxGroupOps * vu::kLanes;  // a group's expected table, as allocated

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
typedef short short2_t __attribute__((ext_vector_type(2)));
typedef unsigned int uint6_t __attribute__((ext_vector_type(6)));
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef float float32_t __attribute__((ext_vector_type(32)));

// the 32 six-bit codes of a pk32 decoder's operand, packed
template <int OP>
__device__ __forceinline__ uint6_t wide_codes(uint64_t a, uint64_t c) {
  uint32_t w[6] = {};
#pragma unroll
  for (int j = 0; j < vu::kWide; ++j) vu::put6(w, j, vu::expand(OP, a, c, j));
  uint6_t v = {w[0], w[1], w[2], w[3], w[4], w[5]};
  asm volatile("" : "+v"(v));
  return v;
}
// half `which` of the 32 inputs of a 2xpk16 encoder
template <int OP>
__device__ __forceinline__ float16_t wide_inputs(uint64_t a, uint64_t c, int which) {
  struct {
    float f[16];
  } in;
#pragma unroll
  for (int j = 0; j < 16; ++j) in.f[j] = vu::f32_of(vu::expand(OP, a, c, 16 * which + j));
  float16_t v = __builtin_bit_cast(float16_t, in);
  asm volatile("" : "+v"(v));
  return v;
}
template <int N>
struct Words {
  uint32_t w[N];
};
__device__ __forceinline__ void put(float32_t v, uint32_t* r) {
  const Words<32> raw = __builtin_bit_cast(Words<32>, v);
#pragma unroll
  for (int j = 0; j < 32; ++j) r[j] = raw.w[j];
}
__device__ __forceinline__ void put(uint6_t v, uint32_t* r) {
  // a six-element vector is padded to eight
  const Words<sizeof(uint6_t) / 4> raw = __builtin_bit_cast(Words<sizeof(uint6_t) / 4>, v);
#pragma unroll
  for (int j = 0; j < 6; ++j) r[j] = raw.w[j];
}

template <class To, class From>
__device__ __forceinline__ To as(From v) {
  return __builtin_bit_cast(To, v);
}
__device__ __forceinline__ void put(float2_t v, uint32_t* r) {
  r[0] = as<uint32_t>(v.x);
  r[1] = as<uint32_t>(v.y);
}
__device__ __forceinline__ void put(uint64_t v, uint32_t* r) {
  r[0] = static_cast<uint32_t>(v);
  r[1] = static_cast<uint32_t>(v >> 32);
}

// The instruction behind op OP: operands a, b, c (valu_ops.h says what each holds), result words r.
template <int OP>
__device__ __forceinline__ void dev_op(uint64_t a64, uint64_t b64, uint64_t c64, uint32_t* r) {
  const uint32_t a = static_cast<uint32_t>(a64), b = static_cast<uint32_t>(b64), c = static_cast<uint32_t>(c64);
  const int32_t ai = static_cast<int32_t>(a), bi = static_cast<int32_t>(b);
  const float af = as<float>(a), bf = as<float>(b), cf = as<float>(c);
  const double ad = as<double>(a64), bd = as<double>(b64), cd = as<double>(c64);
  switch (OP) {
    case vu::kMulLoU32: r[0] = a * b; break;
    case vu::kMulHiU32: r[0] = __umulhi(a, b); break;
    case vu::kMulHiI32: r[0] = static_cast<uint32_t>(__mulhi(ai, bi)); break;
    case vu::kMadU64U32: put(static_cast<uint64_t>(a) * b + c64, r); break;
    case vu::kMadI64I32: put(static_cast<uint64_t>(static_cast<int64_t>(ai) * bi + static_cast<int64_t>(c64)), r); break;
    case vu::kAdd3U32: r[0] = a + b + c; break;
    case vu::kLshlB64: put(a64 << (b & 63u), r); break;
    case vu::kPkAddU16: r[0] = as<uint32_t>(as<ushort2_t>(a) + as<ushort2_t>(b)); break;
    case vu::kPkMulLoU16: r[0] = as<uint32_t>(as<ushort2_t>(a) * as<ushort2_t>(b)); break;
    case vu::kSdot4: r[0] = static_cast<uint32_t>(__builtin_amdgcn_sdot4(ai, bi, static_cast<int>(c), false)); break;
    case vu::kUdot4: r[0] = __builtin_amdgcn_udot4(a, b, c, false); break;
    case vu::kSadU8: r[0] = __builtin_amdgcn_sad_u8(a, b, c); break;
    case vu::kLerpU8: r[0] = __builtin_amdgcn_lerp(a, b, c); break;
    case vu::kLshlAddU32: r[0] = (a << (b & 3u)) + c; break;
    case vu::kAshrI64: put(static_cast<uint64_t>(static_cast<int64_t>(a64) >> (b & 63u)), r); break;
    case vu::kMinI32: r[0] = static_cast<uint32_t>(min(ai, bi)); break;
    case vu::kMaxU32: r[0] = max(a, b); break;
    case vu::kMed3I32: r[0] = static_cast<uint32_t>(max(min(ai, bi), min(max(ai, bi), static_cast<int32_t>(c)))); break;
    case vu::kMed3U32: r[0] = max(min(a, b), min(max(a, b), c)); break;
    case vu::kPkMadU16: r[0] = as<uint32_t>(as<ushort2_t>(a) * as<ushort2_t>(b) + as<ushort2_t>(c)); break;
    case vu::kPkMinI16: r[0] = as<uint32_t>(__builtin_elementwise_min(as<short2_t>(a), as<short2_t>(b))); break;
    case vu::kPkMaxU16: r[0] = as<uint32_t>(__builtin_elementwise_max(as<ushort2_t>(a), as<ushort2_t>(b))); break;
    case vu::kPkLshlB16: {
      const ushort2_t fifteen = {15, 15};
      r[0] = as<uint32_t>(as<ushort2_t>(a) << (as<ushort2_t>(b) & fifteen));
      break;
    }
    case vu::kSdot8: r[0] = static_cast<uint32_t>(__builtin_amdgcn_sdot8(ai, bi, static_cast<int>(c), false)); break;
    case vu::kUdot8: r[0] = __builtin_amdgcn_udot8(a, b, c, false); break;
    case vu::kSdot2: r[0] = static_cast<uint32_t>(__builtin_amdgcn_sdot2(as<short2_t>(a), as<short2_t>(b), static_cast<int>(c), false)); break;
    case vu::kMsadU8: r[0] = __builtin_amdgcn_msad_u8(a, b, c); break;
    case vu::kFfbl: r[0] = static_cast<uint32_t>(__builtin_ctz((a << (b & 31u)) | 0x80000000u)); break;
    case vu::kPermB32: r[0] = __builtin_amdgcn_perm(a, b, c); break;
    case vu::kAlignBit: r[0] = __builtin_amdgcn_alignbit(a, b, c); break;
    case vu::kAlignByte: r[0] = __builtin_amdgcn_alignbyte(a, b, c); break;
    case vu::kBfeU32: r[0] = __builtin_amdgcn_ubfe(a, b & 31u, vu::bfe_width(b & 31u, c)); break;
    case vu::kBfeI32: r[0] = static_cast<uint32_t>(__builtin_amdgcn_sbfe(ai, b & 31u, vu::bfe_width(b & 31u, c))); break;
    case vu::kBfrev: r[0] = __builtin_bitreverse32(a); break;
    case vu::kBcnt: r[0] = __builtin_popcount(a) + b; break;
    case vu::kFfbh: r[0] = static_cast<uint32_t>(__builtin_clz((a >> (b & 31u)) | 1u)); break;
    case vu::kBitop96: r[0] = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); break;
    case vu::kBitopE8: r[0] = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); break;
    case vu::kBitopCA: r[0] = __builtin_amdgcn_bitop3_b32(a, b, c, 0xCA); break;
    case vu::kBitop6B: r[0] = __builtin_amdgcn_bitop3_b32(a, b, c, 0x6B); break;
    case vu::kAshrPkI8: r[0] = __builtin_amdgcn_ashr_pk_i8_i32(a, b, c); break;
    case vu::kMbcnt: r[0] = __builtin_amdgcn_mbcnt_hi(b, __builtin_amdgcn_mbcnt_lo(a, 0u)); break;
    case vu::kAddF32: r[0] = as<uint32_t>(af + bf); break;
    case vu::kMulF32: r[0] = as<uint32_t>(af * bf); break;
    case vu::kFmaF32: r[0] = as<uint32_t>(__builtin_fmaf(af, bf, cf)); break;
    case vu::kPkFmaF32: put(__builtin_elementwise_fma(as<float2_t>(a64), as<float2_t>(b64), as<float2_t>(c64)), r); break;
    case vu::kDivF32: r[0] = as<uint32_t>(af / bf); break;       // correctly rounded: div_scale, div_fmas, div_fixup
    case vu::kSqrtF32: r[0] = as<uint32_t>(__builtin_sqrtf(af)); break;  // correctly rounded
    case vu::kMed3F32: r[0] = as<uint32_t>(__builtin_amdgcn_fmed3f(af, bf, cf)); break;
    case vu::kLdexpF32: r[0] = as<uint32_t>(__builtin_amdgcn_ldexpf(af, bi)); break;
    case vu::kFrexpMantF32: r[0] = as<uint32_t>(__builtin_amdgcn_frexp_mantf(af)); break;
    case vu::kFrexpExpF32: r[0] = static_cast<uint32_t>(__builtin_amdgcn_frexp_expf(af)); break;
    case vu::kFractF32: r[0] = as<uint32_t>(__builtin_amdgcn_fractf(af)); break;
    case vu::kRndneF32: r[0] = as<uint32_t>(__builtin_rintf(af)); break;
    case vu::kFloorF32: r[0] = as<uint32_t>(__builtin_floorf(af)); break;
    case vu::kCvtI32F32: r[0] = static_cast<uint32_t>(static_cast<int32_t>(af)); break;
    case vu::kCvtF32I32: r[0] = as<uint32_t>(static_cast<float>(ai)); break;
    case vu::kCvtF32Ubyte:
      r[0] = as<uint32_t>(static_cast<float>(a & 0xFFu));
      r[1] = as<uint32_t>(static_cast<float>((a >> 8) & 0xFFu));
      r[2] = as<uint32_t>(static_cast<float>((a >> 16) & 0xFFu));
      r[3] = as<uint32_t>(static_cast<float>(a >> 24));
      break;
    case vu::kClassF32: r[0] = __builtin_amdgcn_class(af, bi) ? 1u : 0u; break;
    case vu::kPkMulF32: put(as<float2_t>(a64) * as<float2_t>(b64), r); break;
    case vu::kPkAddF32: put(as<float2_t>(a64) + as<float2_t>(b64), r); break;
    case vu::kMinF32: r[0] = as<uint32_t>(__builtin_fminf(af, bf)); break;
    case vu::kMaxF32: r[0] = as<uint32_t>(__builtin_fmaxf(af, bf)); break;
    case vu::kCeilF32: r[0] = as<uint32_t>(__builtin_ceilf(af)); break;
    case vu::kTruncF32: r[0] = as<uint32_t>(__builtin_truncf(af)); break;
    case vu::kCvtU32F32: r[0] = static_cast<uint32_t>(af); break;
    case vu::kCvtF32U32: r[0] = as<uint32_t>(static_cast<float>(a)); break;
    case vu::kMulF64: put(as<uint64_t>(ad * bd), r); break;
    case vu::kCvtF64F32: put(as<uint64_t>(static_cast<double>(af)), r); break;
    case vu::kCvtI32F64: r[0] = static_cast<uint32_t>(static_cast<int32_t>(ad)); break;
    case vu::kCvtF64I32: put(as<uint64_t>(static_cast<double>(ai)), r); break;
    case vu::kAddF64: put(as<uint64_t>(ad + bd), r); break;
    case vu::kFmaF64: put(as<uint64_t>(__builtin_fma(ad, bd, cd)), r); break;
    case vu::kDivF64: put(as<uint64_t>(ad / bd), r); break;
    case vu::kSqrtF64: put(as<uint64_t>(__builtin_sqrt(ad)), r); break;
    case vu::kCvtF32F64: r[0] = as<uint32_t>(static_cast<float>(ad)); break;
    case vu::kPkFmaF16: r[0] = as<uint32_t>(__builtin_elementwise_fma(as<half2_t>(a), as<half2_t>(b), as<half2_t>(c))); break;
    case vu::kPkMulF16: r[0] = as<uint32_t>(as<half2_t>(a) * as<half2_t>(b)); break;
    case vu::kCvtF16F32: r[0] = as<unsigned short>(static_cast<_Float16>(af)); break;
    case vu::kPkAddF16: r[0] = as<uint32_t>(as<half2_t>(a) + as<half2_t>(b)); break;
    case vu::kFdot2: r[0] = as<uint32_t>(__builtin_amdgcn_fdot2(as<half2_t>(a), as<half2_t>(b), cf, false)); break;
    case vu::kFdot2Bf16: r[0] = as<uint32_t>(__builtin_amdgcn_fdot2_f32_bf16(as<bf16x2_t>(a), as<bf16x2_t>(b), cf, false)); break;
    case vu::kCvtPkrtz: r[0] = as<uint32_t>(__builtin_amdgcn_cvt_pkrtz(af, bf)); break;
    case vu::kCvtF32F16: r[0] = as<uint32_t>(static_cast<float>(as<_Float16>(static_cast<unsigned short>(a)))); break;
    case vu::kCvtPkBf16F32: {
      float2_t v = {af, bf};
      r[0] = as<uint32_t>(__builtin_convertvector(v, bf16x2_t));
      break;
    }
    case vu::kCvtF32Fp8:
      r[0] = as<uint32_t>(__builtin_amdgcn_cvt_f32_fp8(ai, 0));
      r[1] = as<uint32_t>(__builtin_amdgcn_cvt_f32_fp8(ai, 1));
      r[2] = as<uint32_t>(__builtin_amdgcn_cvt_f32_fp8(ai, 2));
      r[3] = as<uint32_t>(__builtin_amdgcn_cvt_f32_fp8(ai, 3));
      break;
    case vu::kCvtF32Bf8:
      r[0] = as<uint32_t>(__builtin_amdgcn_cvt_f32_bf8(ai, 0));
      r[1] = as<uint32_t>(__builtin_amdgcn_cvt_f32_bf8(ai, 1));
      r[2] = as<uint32_t>(__builtin_amdgcn_cvt_f32_bf8(ai, 2));
      r[3] = as<uint32_t>(__builtin_amdgcn_cvt_f32_bf8(ai, 3));
      break;
    case vu::kCvtPkF32Fp8:
      put(__builtin_amdgcn_cvt_pk_f32_fp8(ai, false), r);
      put(__builtin_amdgcn_cvt_pk_f32_fp8(ai, true), r + 2);
      break;
    case vu::kScalePkF32Fp8:
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp8(a, cf, false), r);
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp8(a, cf, true), r + 2);
      break;
    case vu::kScalePkF32Bf8:
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_bf8(a, cf, false), r);
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_bf8(a, cf, true), r + 2);
      break;
    case vu::kScalePkF32Fp4:
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, cf, 0), r);
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, cf, 1), r + 2);
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, cf, 2), r + 4);
      put(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, cf, 3), r + 6);
      break;
    case vu::kCvtPkFp8F32: r[0] = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(af, bf, 0, false)); break;
    case vu::kCvtPkBf8F32: r[0] = static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_bf8_f32(af, bf, 0, false)); break;
    case vu::kScalePkFp8F32: {
      short2_t old = {0, 0};
      r[0] = as<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_fp8_f32(old, af, bf, cf, false));
      break;
    }
    case vu::kScalePkBf8F32: {
      short2_t old = {0, 0};
      r[0] = as<uint32_t>(__builtin_amdgcn_cvt_scalef32_pk_bf8_f32(old, af, bf, cf, false));
      break;
    }
    case vu::kScalePkFp4F32: r[0] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, af, bf, cf, 0); break;
    case vu::kCvtPkF32Bf8:
      put(__builtin_amdgcn_cvt_pk_f32_bf8(ai, false), r);
      put(__builtin_amdgcn_cvt_pk_f32_bf8(ai, true), r + 2);
      break;
    case vu::kScalePk32F32Fp6: put(__builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(wide_codes<OP>(a64, c64), cf), r); break;
    case vu::kScalePk32F32Bf6: put(__builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(wide_codes<OP>(a64, c64), cf), r); break;
    case vu::kScale2xPk16Fp6:
      put(__builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(wide_inputs<OP>(a64, c64, 0), wide_inputs<OP>(a64, c64, 1), cf), r);
      break;
    case vu::kScale2xPk16Bf6:
      put(__builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(wide_inputs<OP>(a64, c64, 0), wide_inputs<OP>(a64, c64, 1), cf), r);
      break;
    case vu::kExpF16: r[0] = as<unsigned short>(__builtin_elementwise_exp2(as<_Float16>(static_cast<unsigned short>(a)))); break;
    case vu::kLogF16: r[0] = as<unsigned short>(__builtin_elementwise_log2(as<_Float16>(static_cast<unsigned short>(a)))); break;
    case vu::kRcpF16: r[0] = as<unsigned short>(__builtin_amdgcn_rcph(as<_Float16>(static_cast<unsigned short>(a)))); break;
    case vu::kScaleSrPkFp4: {
      const float2_t v = {af, bf};
      r[0] = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, v, a * 0x9E3779B1u ^ b, cf, 0);
      break;
    }
    case vu::kExp2: r[0] = as<uint32_t>(__builtin_amdgcn_exp2f(af)); break;
    case vu::kLog2: r[0] = as<uint32_t>(__builtin_amdgcn_logf(af)); break;
    case vu::kRcp: r[0] = as<uint32_t>(__builtin_amdgcn_rcpf(af)); break;
    case vu::kRsq: r[0] = as<uint32_t>(__builtin_amdgcn_rsqf(af)); break;
    case vu::kSqrtRaw: r[0] = as<uint32_t>(__builtin_amdgcn_sqrtf(af)); break;
    case vu::kSin: r[0] = as<uint32_t>(__builtin_amdgcn_sinf(af)); break;
    case vu::kCos: r[0] = as<uint32_t>(__builtin_amdgcn_cosf(af)); break;
    case vu::kRcpF64: put(as<uint64_t>(__builtin_amdgcn_rcp(ad)), r); break;
    case vu::kRsqF64: put(as<uint64_t>(__builtin_amdgcn_rsq(ad)), r); break;
    case vu::kPrng: r[0] = __builtin_amdgcn_prng_b32(a); break;
    case vu::kCvtSrFp8: r[0] = static_cast<uint32_t>(__builtin_amdgcn_cvt_sr_fp8_f32(af, bi, 0, 0)); break;
    default: break;
  }
}

// One op on operands the compiler cannot see through, its result words made opaque too.
template <int OP>
__device__ __forceinline__ void opaque_op(uint64_t a, uint64_t b, uint64_t c, uint32_t* r) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
  dev_op<OP>(a, b, c, r);
#pragma unroll
  for (int i = 0; i < vu::kOps[OP].results; ++i) asm volatile("" : "+v"(r[i]));
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, kWave);
    v = o < v ? o : v;
  }
  return v;
}

struct SweepArgs {
  int rounds;
  uint32_t seed;
  uint32_t mask;  // bit s: op s of the group is selected
  int inject_op;  // table index, or -1
};

// Op OP (slot `OP - group_first` of its group): the lane's digest over the rounds, compared with
// the table in LDS (exact ops); lane 0 leaves the wave's count of wrong lanes and its digest.
template <int OP>
__device__ __forceinline__ void sweep_op(const SweepArgs& args, int lane, bool inject, const uint32_t* expect,
                                         amdgpu_valu_record* rec, uint32_t& first_op, uint32_t& first_lane) {
  constexpr int slot = OP - vu::group_first(vu::kOps[OP].group);
  uint32_t bad = 0, wave_digest = 0;
  if ((args.mask >> slot) & 1u) {  // uniform
    uint32_t digest = 0;
    for (int round = 0; round < args.rounds; ++round) {
      uint32_t r[vu::kMaxResults];
      opaque_op<OP>(vu::kOps[OP].kind[0] != vu::kNone ? vu::operand(args.seed, OP, round, lane, 0) : 0,
                    vu::kOps[OP].kind[1] != vu::kNone ? vu::operand(args.seed, OP, round, lane, 1) : 0,
                    vu::kOps[OP].kind[2] != vu::kNone ? vu::operand(args.seed, OP, round, lane, 2) : 0, r);
      if (inject && args.inject_op == OP && round == 0 && lane == vu::kInjectLane) r[0] += 1u;
#pragma unroll
      for (int i = 0; i < vu::kOps[OP].results; ++i) digest = vu::fold(digest, r[i]);
    }
    const uint32_t wrong = vu::kOps[OP].cls == vu::kExact && digest != expect[slot * vu::kLanes + lane];
    bad = wave_total(wrong);
    wave_digest = wave_total(digest * vu::lane_weight(lane));
    const uint32_t lowest = wave_min(wrong ? static_cast<uint32_t>(lane) : kValuNone);
    if (first_op == kValuNone && lowest != kValuNone) {
      first_op = OP;
      first_lane = lowest;
    }
  }
  if (lane == 0) {
    rec->bad[slot] = bad;
    rec->digest[slot] = wave_digest;
  }
}

template <int G, int... S>
__device__ __forceinline__ void sweep_ops(std::integer_sequence<int, S...>, const SweepArgs& args, int lane, bool inject,
                                          const uint32_t* expect, amdgpu_valu_record* rec, uint32_t& first_op,
                                          uint32_t& first_lane) {
  (sweep_op<vu::group_first(G) + S>(args, lane, inject, expect, rec, first_op, first_lane), ...);
}

// Waves with global index < inject_waves perturb the first result word of args.inject_op.  Of
// the dynamic LDS allocation (its size keeps one workgroup per CU) the first kExpectWords words
// hold the expected table.
template <int G>
__global__ void __launch_bounds__(kThreads) valu_sweep(SweepArgs args, int inject_waves, const u32x4* __restrict__ expect,
                                                       amdgpu_valu_record* __restrict__ records,
                                                       unsigned int* __restrict__ wave_site, int wave_site_len) {
  extern __shared__ u32x4 lds_expect[];
  constexpr int count = vu::group_count(G);
  const uint32_t site = site_id();
  for (int i = threadIdx.x; i < count * vu::kLanes / 4; i += kThreads) lds_expect[i] = expect[i];  // < kExpectWords / 4
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kValuWaves + (threadIdx.x >> 6);  // < 2^14 (host-checked)
  amdgpu_valu_record* rec = records + gw;
  uint32_t first_op = kValuNone, first_lane = kValuNone;
  sweep_ops<G>(std::make_integer_sequence<int, count>{}, args, lane, static_cast<int>(gw) < inject_waves,
               reinterpret_cast<const uint32_t*>(lds_expect), rec, first_op, first_lane);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
#pragma unroll
  for (int s = count; s < kValuGroupOps; ++s) rec->bad[s] = rec->digest[s] = 0;
  rec->site_first = site;
  rec->site_last = site_after;
  rec->first_op = first_op;
  rec->first_lane = first_lane;
}

template <int OP>
__device__ __forceinline__ void raw_one(int op, uint64_t a, uint64_t b, uint64_t c, uint32_t* __restrict__ out) {
  if (op != OP) return;  // uniform
  uint32_t r[vu::kMaxResults];
  opaque_op<OP>(a, b, c, r);
#pragma unroll
  for (int i = 0; i < vu::kOps[OP].results; ++i) out[i] = r[i];  // the rest stays zero
}
template <int... OP>
__device__ __forceinline__ void raw_any(std::integer_sequence<int, OP...>, int op, uint64_t a, uint64_t b, uint64_t c,
                                        uint32_t* __restrict__ out) {
  (raw_one<OP>(op, a, b, c, out), ...);
}

// Op `op` once per lane on the caller's operands; waves at or past n_waves do nothing.
__global__ void __launch_bounds__(kThreads) valu_raw(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                     const uint64_t* __restrict__ c, uint32_t* __restrict__ out, int n_waves) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kValuWaves + (threadIdx.x >> 6);
  if (static_cast<int>(gw) >= n_waves) return;  // the whole wave
  const size_t idx = static_cast<size_t>(gw) * kWave + lane;
  raw_any(std::make_integer_sequence<int, vu::kNumOps>{}, op, a[idx], b[idx], c[idx], out + idx * vu::kMaxResults);
}

template <class Fn>
bool with_group(int g, Fn&& fn) {
  switch (g) {
    case vu::kGroupInt: fn(std::integral_constant<int, vu::kGroupInt>{}); return true;
    case vu::kGroupBit: fn(std::integral_constant<int, vu::kGroupBit>{}); return true;
    case vu::kGroupF32: fn(std::integral_constant<int, vu::kGroupF32>{}); return true;
    case vu::kGroupF64: fn(std::integral_constant<int, vu::kGroupF64>{}); return true;
    case vu::kGroupF16: fn(std::integral_constant<int, vu::kGroupF16>{}); return true;
    case vu::kGroupCvt: fn(std::integral_constant<int, vu::kGroupCvt>{}); return true;
    case vu::kGroupApprox: fn(std::integral_constant<int, vu::kGroupApprox>{}); return true;
    default: return false;
  }
}

}  // namespace

extern "C" {

int amdgpu_valu_sizeof(int which) {
  const int v[9] = {static_cast<int>(sizeof(amdgpu_valu_record)), static_cast<int>(sizeof(amdgpu_valu_result)), kValuWaves,
                    kValuMaxOps, kValuGroupOps, kValuGroups, vu::kMaxRounds, vu::kMaxResults, vu::kInjectLane};
  return which >= 0 && which < 9 ? v[which] : -1;
}

int amdgpu_valu_kind(int kind, char* buf, int len) {
  if (kind < 0 || kind >= vu::kNumKinds) return -1;
  return buf != nullptr && len > 0 ? std::snprintf(buf, len, "%s", vu::kKindNames[kind]) : static_cast<int>(std::strlen(vu::kKindNames[kind]));
}

int amdgpu_valu_expand(int op, unsigned long long a, unsigned long long c, unsigned int* out) {
  if (op < 0 || op >= vu::kNumOps || !vu::is_wide(op) || out == nullptr) return -1;
  for (int j = 0; j < vu::kWide; ++j) out[j] = vu::expand(op, a, c, j);
  return 0;
}

int amdgpu_valu_ops(int index, int what, char* buf, int len) {
  if (index < 0) return vu::kNumOps;
  if (index >= vu::kNumOps || what < 0 || what > 2) return -1;
  const vu::OpInfo& o = vu::kOps[index];
  const char* text = what == 0 ? o.name : what == 1 ? o.mnemonic : vu::kGroupNames[o.group];
  return buf != nullptr && len > 0 ? std::snprintf(buf, len, "%s", text) : static_cast<int>(std::strlen(text));
}

int amdgpu_valu_op_ints(int index, int* out) {
  if (index < 0 || index >= vu::kNumOps || out == nullptr) return -1;
  const vu::OpInfo& o = vu::kOps[index];
  const int v[7] = {o.group, o.cls, o.kind[0], o.kind[1], o.kind[2], o.results, o.rkind};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return 0;
}

int amdgpu_valu_operands(int op, unsigned int seed, int rounds, unsigned long long* a, unsigned long long* b,
                         unsigned long long* c) {
  if (op < 0 || op >= vu::kNumOps || rounds < 1 || rounds > vu::kMaxRounds || !a || !b || !c) return -1;
  unsigned long long* out[3] = {a, b, c};
  for (int r = 0; r < rounds; ++r)
    for (int lane = 0; lane < kWave; ++lane)
      for (int w = 0; w < 3; ++w) out[w][r * kWave + lane] = vu::kOps[op].kind[w] != vu::kNone ? vu::operand(seed, op, r, lane, w) : 0;
  return 0;
}

int amdgpu_valu_expected(int op, unsigned int seed, int rounds, unsigned int* digest) {
  return digest == nullptr ? -1 : vu::expected_digests(op, seed, rounds, digest);
}

int amdgpu_valu_reduce(const amdgpu_valu_record* recs, const int* group_of, int n, const unsigned char* selected,
                       amdgpu_valu_result* result) {
  if (result == nullptr) return -1;
  std::memset(result, 0, sizeof(*result));
  return vu::reduce(recs, group_of, n, selected, result) ? 0 : -1;
}

int amdgpu_valu_describe(const amdgpu_valu_result* r, int which, char* buf, int len) { return vu::describe(*r, which, buf, len); }

int amdgpu_valu_raw(int device, int op, const unsigned long long* a, const unsigned long long* b, const unsigned long long* c,
                    unsigned int* out, int n_waves, char* err, int err_len) {
  if (err == nullptr || err_len <= 0) return -1;
  if (op < 0 || op >= vu::kNumOps || !a || !b || !c || !out || n_waves < 1 || n_waves > (1 << 20)) {
    std::snprintf(err, err_len, "vector ALU check: bad arguments (raw: op %d below %d, waves %d in 1..%d)", op, vu::kNumOps,
                  n_waves, 1 << 20);
    return -1;
  }
  const size_t lanes = static_cast<size_t>(n_waves) * kWave;
  Status st;
  DeviceBuffer<uint64_t> d_a, d_b, d_c;
  DeviceBuffer<uint32_t> d_out;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, d_a.alloc(lanes * 8));
  CANARY_HIP(st, d_b.alloc(lanes * 8));
  CANARY_HIP(st, d_c.alloc(lanes * 8));
  CANARY_HIP(st, d_out.alloc(lanes * vu::kMaxResults * 4));
  CANARY_HIP(st, d_a.upload(a));
  CANARY_HIP(st, d_b.upload(b));
  CANARY_HIP(st, d_c.upload(c));
  CANARY_HIP(st, d_out.zero());
  st.stage("valu_raw: ");
  if (st.ok()) {
    hipLaunchKernelGGL(valu_raw, dim3((n_waves + kValuWaves - 1) / kValuWaves), dim3(kThreads), 0, 0, op, d_a.get(), d_b.get(),
                       d_c.get(), d_out.get(), n_waves);
    CANARY_HIP(st, hipGetLastError());
    CANARY_HIP(st, hipDeviceSynchronize());
  }
  CANARY_HIP(st, d_out.download(out));
  return st.report("vector ALU check: ", err, err_len);
}

int amdgpu_valu_run(int device, int blocks, int rounds, unsigned int seed, const unsigned char* selected, int inject_op,
                    int inject_waves, unsigned int* wave_site_out, int wave_site_len, amdgpu_valu_result* out, char* err,
                    int err_len) {
  if (out == nullptr || err == nullptr || err_len <= 0) return -1;
  std::memset(out, 0, sizeof(*out));
  if (!vu::arguments_ok(blocks, rounds, selected, inject_op, inject_waves, wave_site_len, wave_site_out != nullptr)) {
    std::snprintf(err, err_len,
                  "vector ALU check: bad arguments (blocks %d in 0..%d, rounds %d in 1..%d, at least one of the %d ops selected, "
                  "inject %d/%d with a selected op)",
                  blocks, vu::kMaxBlocks, rounds, vu::kMaxRounds, vu::kNumOps, inject_op, inject_waves);
    return -1;
  }
  const unsigned int groups = vu::group_mask(selected);
  // the launches' expected tables (the operands do not depend on the launch): group g at g * kExpectWords
  std::vector<uint32_t> expect(static_cast<size_t>(vu::kNumGroups) * kExpectWords, 0);
  uint32_t masks[vu::kNumGroups] = {};
  for (int op = 0; op < vu::kNumOps; ++op) {
    if (!selected[op]) continue;
    const int g = vu::kOps[op].group, slot = op - vu::group_first(g);
    masks[g] |= 1u << slot;
    if (vu::kOps[op].cls == vu::kExact && vu::expected_digests(op, seed, rounds, &expect[g * kExpectWords + slot * vu::kLanes]) != 0) {
      std::snprintf(err, err_len, "vector ALU check: a generated case of %s is not a normal number or a zero", vu::kOps[op].name);
      return -1;
    }
  }
  Status st;
  hipDeviceProp_t prop;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (!st.ok()) return st.report("vector ALU check: ", err, err_len);
  const LaunchPlan plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
  const int grid = plan.grid;
  const size_t slots = static_cast<size_t>(grid) * kValuWaves;
  out->cus_expected = prop.multiProcessorCount;
  out->blocks = grid;
  out->rounds = rounds;

  DeviceBuffer<amdgpu_valu_record> d_records;  // the groups' slots, one group after another
  DeviceBuffer<uint32_t> d_expect;
  DeviceBuffer<unsigned int> d_wave_site;
  Events<vu::kNumGroups + 1> ev;
  CANARY_HIP(st, d_records.alloc(sizeof(amdgpu_valu_record) * slots * vu::kNumGroups));
  CANARY_HIP(st, d_expect.alloc(expect.size() * 4));
  CANARY_HIP(st, d_expect.upload(expect.data()));
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * vu::kNumGroups * wave_site_len));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, ev.create());

  std::vector<amdgpu_valu_record> h;
  std::vector<int> group_of;
  for (int l = 0; l < plan.max_launches && st.ok(); ++l) {
    float ms[vu::kNumGroups] = {};
    CANARY_HIP(st, d_records.fill(0xFF));
    st.stage("valu_sweep: ");
    time_stages(st, ev, ms, [&](int g) {
      if (!((groups >> g) & 1u)) return hipSuccess;
      size_t got = 0;
      with_group(g, [&](auto group) {
        constexpr int G = decltype(group)::value;
        const SweepArgs args = {rounds, seed, masks[G], l == 0 ? inject_op : -1};
        got = launch_with_max_lds(valu_sweep<G>, prop, dim3(grid), dim3(kThreads), args, l == 0 ? inject_waves : 0,
                                  reinterpret_cast<const u32x4*>(d_expect.get() + G * kExpectWords), d_records.get() + slots * G,
                                  l == 0 && wave_site_len > 0 ? d_wave_site.get() + static_cast<size_t>(G) * wave_site_len : nullptr,
                                  l == 0 ? wave_site_len : 0);
      });
      return got ? hipSuccess : hipErrorLaunchFailure;
    });
    for (int g = 0; g < vu::kNumGroups && st.ok(); ++g) {
      if (!((groups >> g) & 1u)) continue;
      const size_t have = h.size();
      h.resize(have + slots);
      group_of.resize(have + slots, g);
      CANARY_HIP(st, hipMemcpy(h.data() + have, d_records.get() + slots * g, sizeof(amdgpu_valu_record) * slots,
                               hipMemcpyDeviceToHost));
      out->group_ms[g] += ms[g];
      out->ms += ms[g];
    }
    if (!st.ok()) break;
    out->launches = l + 1;
    if (!vu::reduce(h.data(), group_of.data(), static_cast<int>(h.size()), selected, out)) {
      std::snprintf(err, err_len, "vector ALU check: a record holds a site out of range");
      return -1;
    }
    if (covered(*out, out->cus_expected)) break;
  }
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));
  return st.report("vector ALU check: ", err, err_len);
}

}  // extern "C"
