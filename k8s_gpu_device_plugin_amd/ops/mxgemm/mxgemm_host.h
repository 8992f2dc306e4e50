// What the host and the device of the block-scaled matrix-path check must agree on, written once:
// the packing of an operand row, the integer data and its E8M0 scales, the shape rules, the result
// and its text.  The operand hash, the OCP codes of small integers and the format ids are
// ../mfma_forms.h's.  No HIP include: a plain C++17 compiler compiles it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../mfma_forms.h"

extern "C" {

struct amdgpu_mxgemm_result {    // 56 bytes
  unsigned long long row_errors; // rows of the verified product whose checksum is off or that hold an unhealthy element
  unsigned long long col_errors; // ... and columns
  double ms;                     // device time of the `iters` timed launches
  double tflops;                 // dense rate over them: 2 M N K flop per launch
  int fmt;                       // the project's format id: 0 fp8, 1 bf8, 4 fp4
  int kernel;                    // the kernel id that ran (never 0)
  int m, n, k;
  int iters;
};

}  // extern "C"

namespace mxgemm {

using canary::kBf8;
using canary::kFp4;
using canary::kFp8;

constexpr int kRowBytes = 128;  // K bytes of one operand tile row in LDS, whatever the format
constexpr int kMaxK = 65536;    // K * 16 * 4 <= 2^22: every element of a healthy product is an integer below 2^24
constexpr int kScaleBlock = 32; // k per E8M0 byte

FORMS_HD constexpr bool format_ok(int fmt) { return fmt == kFp8 || fmt == kBf8 || fmt == kFp4; }
FORMS_HD constexpr int bits(int fmt) { return fmt == kFp4 ? 4 : 8; }
FORMS_HD constexpr int tile_k(int fmt) { return kRowBytes * 8 / bits(fmt); }  // BK: 128 (fp8, bf8), 256 (fp4)
FORMS_HD size_t row_bytes(int fmt, int K) { return static_cast<size_t>(K) * bits(fmt) / 8; }
inline const char* format_name(int fmt) { return fmt == kFp8 ? "fp8" : fmt == kBf8 ? "bf8" : fmt == kFp4 ? "fp4" : "?"; }

// ---- the packing: element k of a row is `bits` wide at bit shift_of(k) of byte byte_of(k) ----
// One code per byte for the 8-bit formats; fp4 two per byte, the even k in the low nibble.
FORMS_HD size_t byte_of(int fmt, int k) { return fmt == kFp4 ? static_cast<size_t>(k) >> 1 : static_cast<size_t>(k); }
FORMS_HD int shift_of(int fmt, int k) { return fmt == kFp4 ? 4 * (k & 1) : 0; }
FORMS_HD uint32_t code_at(int fmt, const uint8_t* row, int k) {
  return (row[byte_of(fmt, k)] >> shift_of(fmt, k)) & ((1u << bits(fmt)) - 1u);
}

// ---- the integer data: operand `which` (0: A, 1: Bt) ----
FORMS_HD int value(int which, int row, int k, int K) {  // in [-4, 4]
  return canary::small_int((static_cast<uint64_t>(which + 1) << 56) ^ (static_cast<uint64_t>(row) * K + k));
}
FORMS_HD int scale_byte(int vary, int which, int row, int kblock) {  // 127 or 128: 2^0 or 2^1
  return 127 + canary::scale_exp(vary, row, kblock, which);
}
FORMS_HD uint32_t code_of(int fmt, int v) {
  return fmt == kFp8 ? canary::lowp_code<kFp8>(v) : fmt == kBf8 ? canary::lowp_code<kBf8>(v) : canary::lowp_code<kFp4>(v);
}
// The integer a code of code_of stands for; any other code gives 99, which no checksum survives.
FORMS_HD int int_of_code(int fmt, uint32_t code) {
  const uint32_t sign = fmt == kFp4 ? 0x8u : 0x80u;
  for (int m = 0; m <= 4; ++m)
    if ((code & ~sign) == code_of(fmt, m)) return (code & sign) ? -m : m;
  return 99;
}
// The byte at `byte` of a packed row of the data: one code, or two for fp4.
FORMS_HD uint8_t packed_byte(int fmt, int which, int row, size_t byte, int K) {
  if (fmt != kFp4) return static_cast<uint8_t>(code_of(fmt, value(which, row, static_cast<int>(byte), K)));
  const int k = static_cast<int>(byte) * 2;
  return static_cast<uint8_t>(code_of(fmt, value(which, row, k, K)) | (code_of(fmt, value(which, row, k + 1, K)) << 4));
}
// What an element and its scale byte are worth in the checksums: v * 2^(scale - 127), scale in 127 .. 158.
FORMS_HD long long scaled(int v, int scale) {
  return scale >= 127 && scale < 127 + 32 ? static_cast<long long>(v) * (1ll << (scale - 127)) : 0;
}

// ---- the shape rules ----
// M, N multiples of the kernel's tile edge, K a multiple of BK, K <= 65536.
inline bool shape_ok(int fmt, int tile, int M, int N, int K) {
  return format_ok(fmt) && tile > 0 && M > 0 && N > 0 && K > 0 && M % tile == 0 && N % tile == 0 && K % tile_k(fmt) == 0 &&
         K <= kMaxK;
}
inline int shape_text(int fmt, int kernel, int M, int N, int K, char* buf, int len) {
  if (!format_ok(fmt)) return std::snprintf(buf, len, "mx matrix path: no format %d (0 fp8, 1 bf8, 4 fp4)", fmt);
  return std::snprintf(buf, len,
                       "mx matrix path: shape (%d,%d,%d) does not fit %s kernel %d (M,N %% 128 or 256, K %% %d, K <= %d)", M, N,
                       K, format_name(fmt), kernel, tile_k(fmt), kMaxK);
}

// "mx matrix path: 1 wrong row and 1 wrong column in fp4 (kernel 2, 4096x4096x4096)"; 0 and an
// empty text if the product was right.
inline int describe(const amdgpu_mxgemm_result& r, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  if (r.row_errors == 0 && r.col_errors == 0) return 0;
  return std::snprintf(buf, len, "mx matrix path: %llu wrong row%s and %llu wrong column%s in %s (kernel %d, %dx%dx%d)",
                       r.row_errors, r.row_errors == 1 ? "" : "s", r.col_errors, r.col_errors == 1 ? "" : "s",
                       format_name(r.fmt), r.kernel, r.m, r.n, r.k);
}

}  // namespace mxgemm
