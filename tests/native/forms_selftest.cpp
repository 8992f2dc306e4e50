// Stand-alone self-test of the MFMA forms (ops/mfma_forms.h): no HIP, no Python, no GPU.
// tests/test_canary_forms.py compiles it with g++ -fsanitize=address,undefined and runs it
// directly; it exits 0 and prints "ok", or prints what failed and exits 1.
//
// For each of the five forms it emulates the MFMA from the operands alone: every lane's
// operands are built by the code the kernels run (form_element), decoded back to integers by
// decoders written here from the formats' definitions, and placed into A[32][K] and B[K][32]
// where the instruction takes them from, with the block scale of the lane that supplies each
// k-block.  Those layouts are written a second time here (hw_k, hw_kblock), so a later change
// of the header's maps shows; an error both copies shared from the start would not, and only
// the GPU test against a PyTorch GEMM (tests/test_gpu_datapath.py) ties the map to the hardware.
// The product is read through cd_row32.  What each lane reads must be the reference the kernels
// compare with (form_ref): a wrong map and a wrong reference that agree with each other do not pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mfma_forms.h"

namespace {

using namespace canary;

int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// the key offsets are data keys: exactly these
static_assert(FormBf16::kKeyOffset == 0, "bf16");
static_assert(FormFp8Unscaled::kKeyOffset == 0x77u << 20, "unscaled fp8");
static_assert(FormScaled<kFp8>::kKeyOffset == 1u << 20 && FormScaled<kBf8>::kKeyOffset == 2u << 20 &&
                  FormScaled<kFp4>::kKeyOffset == 5u << 20,
              "scaled: (FMT + 1) << 20");
static_assert(FormBf16::kK == 16 && FormFp8Unscaled::kK == 16 && FormScaled<kFp4>::kK == 64, "k per MFMA");

// ---- decoders, from the formats' definitions (not from lowp_code / bf16_of_int) -------------
// An OCP minifloat with `ebits` exponent and `mbits` mantissa bits, no infinities or NaNs in the
// range used; the result times 4 (every value here is a multiple of 0.25) as an integer.
int minifloat_x4(uint32_t code, int ebits, int mbits, int bias) {
  const int sign = (code >> (ebits + mbits)) & 1;
  const int e = (code >> mbits) & ((1 << ebits) - 1);
  const int m = code & ((1 << mbits) - 1);
  // value = (e ? 2^mbits + m : m) * 2^((e ? e : 1) - bias - mbits)
  const int mant = e ? (1 << mbits) + m : m;
  const int exp2 = (e ? e : 1) - bias - mbits + 2;  // + 2: times 4
  int v = exp2 >= 0 ? mant << exp2 : (mant % (1 << -exp2) == 0 ? mant >> -exp2 : -100000);
  return sign ? -v : v;
}

template <int FMT>
int decode_lowp(uint32_t code) {
  const int x4 = FMT == kFp8   ? minifloat_x4(code, 4, 3, 7)
                 : FMT == kBf8 ? minifloat_x4(code, 5, 2, 15)
                               : minifloat_x4(code, 2, 1, 1);
  CHECK(x4 % 4 == 0);
  return x4 / 4;
}

int decode_bf16(short s) {
  const uint32_t u = static_cast<uint32_t>(static_cast<uint16_t>(s)) << 16;
  float f;
  std::memcpy(&f, &u, 4);
  CHECK(f == static_cast<float>(static_cast<int>(f)));
  return static_cast<int>(f);
}

// Element j of an operand, as the hardware takes it: bf16 j, byte j, or nibble j of the low dwords.
int element(const bf16x8& x, int j, FormBf16*) { return decode_bf16(x.v[j]); }
int element(const uint64_t& x, int j, FormFp8Unscaled*) { return decode_lowp<kFp8>((x >> (8 * j)) & 0xFFu); }
template <int FMT>
int element(const i32x8& x, int j, FormScaled<FMT>*) {
  const int bits = FMT == kFp4 ? 4 : 8;
  return decode_lowp<FMT>((static_cast<uint32_t>(x.v[(j * bits) / 32]) >> ((j * bits) % 32)) & ((1u << bits) - 1));
}

void codes() {
  for (int v = -4; v <= 4; ++v) {
    CHECK(decode_lowp<kFp8>(lowp_code<kFp8>(v)) == v);
    CHECK(decode_lowp<kBf8>(lowp_code<kBf8>(v)) == v);
    CHECK(decode_lowp<kFp4>(lowp_code<kFp4>(v)) == v);
    CHECK(lowp_code<kFp8>(v) < 256 && lowp_code<kBf8>(v) < 256 && lowp_code<kFp4>(v) < 16);
    CHECK(decode_bf16(bf16_of_int(v)) == v && decode_bf16(bf16_of_int(v + 1)) == v + 1);
  }
  for (uint32_t key = 0; key < 4096; ++key) {
    const int v = small_int(0x9E3779B97F4A7C15ull * key);
    CHECK(v >= -4 && v <= 4);
  }
  // the C/D map reads every element of the 32x32 tile exactly once
  int seen[32][32] = {};
  for (int lane = 0; lane < 64; ++lane)
    for (int reg = 0; reg < 16; ++reg) ++seen[cd_row32(reg, lane >> 5)][lane & 31];
  for (auto& row : seen)
    for (int n : row) CHECK(n == 1);
}

template <class F>
constexpr bool scaled = F::kBlockK > 1;

// Where the instruction takes element j of a lane in half h from: k within the step.
int hw_k(int h, int j, FormBf16*) { return h * 8 + j; }
int hw_k(int h, int j, FormFp8Unscaled*) { return h * 8 + j; }
template <int FMT>
int hw_k(int h, int j, FormScaled<FMT>*) {
  if (FMT == kFp4) return h * 32 + j;        // the lane's 32 nibbles are one k-block
  return (j / 16) * 32 + h * 16 + j % 16;    // bytes: two K = 32 halves, each split 16 / 16 over the lane halves
}
// The k-block (of 32) of the whole K whose scale a lane in half h supplies in step s.
int hw_kblock(int s, int h) { return 2 * s + h; }

// The wrong registers over the wave.
template <class F>
int emulate(uint32_t key, int ksteps, int vary, bool inject, bool* all_in_row0) {
  const uint32_t blk = key + F::kKeyOffset;
  const int K = F::kK * ksteps, blocks = scaled<F> ? K / F::kBlockK : 1, block_k = scaled<F> ? F::kBlockK : K;
  std::vector<int> A(32 * K, 0), B(K * 32, 0), heldA(32 * K, 0), heldB(K * 32, 0);
  std::vector<int> ea(32 * blocks, 0), eb(32 * blocks, 0), owned(32 * blocks, 0);
  for (int s = 0; s < ksteps; ++s) {
    for (int lane = 0; lane < 64; ++lane) {
      const int r = lane & 31, h = lane >> 5;
      typename F::operand a = typename F::operand(), b = typename F::operand();
      for (int j = 0; j < F::kElems; ++j) form_element<F>(a, b, blk, lane, s, j, inject);
      for (int j = 0; j < F::kElems; ++j) {
        const int k = F::kK * s + hw_k(h, j, static_cast<F*>(nullptr));
        CHECK(F::k_of(h, j) == hw_k(h, j, static_cast<F*>(nullptr)));
        A[r * K + k] = element(a, j, static_cast<F*>(nullptr));
        B[k * 32 + r] = element(b, j, static_cast<F*>(nullptr));
        ++heldA[r * K + k];
        ++heldB[k * 32 + r];
      }
      if (scaled<F>) {  // the lane's scale operand is that of one k-block of its row / column
        const int kb = hw_kblock(s, h);
        ea[r * blocks + kb] = F::scale(vary, r, s, h, 0) - 127;
        eb[r * blocks + kb] = F::scale(vary, r, s, h, 1) - 127;
        ++owned[r * blocks + kb];
        const int e0 = ea[r * blocks + kb], e1 = eb[r * blocks + kb];
        CHECK(e0 >= 0 && e0 <= 1 && e1 >= 0 && e1 <= 1);
        if (!vary) CHECK(e0 == 0 && e1 == 0);
      } else {
        CHECK(F::scale(vary, r, s, h, 0) == 127 && F::scale(vary, r, s, h, 1) == 127);
      }
    }
  }
  // every k of every row (column) is held by exactly one (half, element), every block scale by one lane
  for (int n : heldA) CHECK(n == 1);
  for (int n : heldB) CHECK(n == 1);
  if (scaled<F>)
    for (int n : owned) CHECK(n == 1);
  int wrong = 0;
  *all_in_row0 = true;
  for (int lane = 0; lane < 64; ++lane) {
    for (int reg = 0; reg < 16; ++reg) {
      const int row = cd_row32(reg, lane >> 5), col = lane & 31;
      long long c = 0;
      for (int kb = 0; kb < blocks; ++kb) {
        long long part = 0;
        for (int k = kb * block_k; k < (kb + 1) * block_k; ++k) part += A[row * K + k] * B[k * 32 + col];
        c += part * (1ll << (ea[row * blocks + kb] + eb[col * blocks + kb]));
      }
      if (c != form_ref<F>(blk, row, col, ksteps, vary)) {
        ++wrong;
        if (row != 0) *all_in_row0 = false;
      }
      CHECK(c > -(1 << 24) && c < (1 << 24));  // exact in fp32
    }
  }
  return wrong;
}

template <class F>
void form(const char* name) {
  const int before = failures;
  bool varied_anything = false;
  for (uint32_t key : {0u, 5u, (3u << 14) | 77u}) {  // block indices, and a site probe's key
    for (int ksteps : {1, 2}) {
      for (int vary : {0, 1}) {
        bool row0 = true;
        CHECK(emulate<F>(key, ksteps, vary, false, &row0) == 0);
        const int wrong = emulate<F>(key, ksteps, vary, true, &row0);
        CHECK(wrong >= 1 && wrong <= 32 && row0);
        if (vary)
          for (int rc = 0; rc < 32; ++rc)
            varied_anything |= F::scale(1, rc, 0, 0, 0) != 127 || F::scale(1, rc, 0, 1, 1) != 127;
      }
    }
  }
  CHECK(varied_anything == scaled<F>);  // "varied" scales that never vary would check nothing
  if (failures != before) std::printf("form %s failed\n", name);
}

}  // namespace

int main() {
  codes();
  form<FormBf16>("bf16");
  form<FormFp8Unscaled>("fp8 unscaled");
  form<FormScaled<kFp8>>("fp8");
  form<FormScaled<kBf8>>("bf8");
  form<FormScaled<kFp4>>("fp4");
  if (failures) {
    std::printf("%d failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
