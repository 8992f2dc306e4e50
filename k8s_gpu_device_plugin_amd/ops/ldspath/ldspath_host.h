// The LDS-path check's shared side: everything ldspath.hip's kernels and the host must agree
// on, written once.  The patterns, the width-pass table, the lane-op table with its lane map,
// the transposed-read address map, the atomics' operand functions and expected tables, the
// record every wave leaves, the result, the reduction of the records and the texts; the packed
// site, its text and the coverage walk are ../site.h's.  No HIP
// include: a plain C++17 compiler compiles it (tests/native/ldspath_selftest.cpp), and under
// hipcc the functions marked LDSPATH_HD are compiled for the device too, so both sides run the
// same code.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mfma_forms.h"
#include "../site.h"

#ifdef __HIPCC__
#define LDSPATH_HD __host__ __device__ inline
#else
#define LDSPATH_HD inline
#endif

extern "C" {

constexpr int kLdsSiteSlots = kSiteSlots;  // packed sites (site.h)
constexpr int kLdsWaves = 4;            // waves per workgroup: records[block * 4 + wave]
constexpr int kLdsStages = 4;           // 0 lds_widths, 1 lds_atomic, 2 lane_xchg, 3 lds_tr
constexpr int kLdsSubs = 48;            // sub-checks a record counts: passes, forms, ops, or 1
constexpr unsigned int kLdsUnwritten = kSiteUnwritten;  // site_first of a slot no wave wrote; first_sub: nothing wrong

struct amdgpu_ldspath_record {  // what one wave leaves per stage; 208 bytes
  unsigned int site_first;      // site_id() before the work
  unsigned int site_last;       // ... and after it
  unsigned int first_sub;       // sub-check of the first wrong word (pass, form, op; 0 for lds_tr), all-ones: none
  unsigned int first_at;        // lds_widths: byte offset; lds_atomic: element; lane_xchg, lds_tr: round
  unsigned int bad[kLdsSubs];   // wrong words per sub-check
};

struct amdgpu_ldspath_result {
  unsigned long long lds_errors;         // located wrong words of lds_widths: plain + subword + conflict
  unsigned long long plain_errors;
  unsigned long long subword_errors;
  unsigned long long conflict_errors;
  unsigned long long dma_errors;         // located wrong words of the LDS-DMA pass (may be L2's or HBM's)
  unsigned long long lds_atomic_errors;  // located wrong table elements
  unsigned long long lane_errors;        // located wrong words of lane_xchg
  unsigned long long tr_errors;          // located wrong 16-bit elements of lds_tr
  unsigned long long unlocated_errors;   // wrong words (any stage) of waves whose site changed
  unsigned long long ldspath_errors;     // what fails the check: all of the above, dma only while lds_errors is 0
  unsigned long long waves;              // located lds_widths records
  unsigned long long moved;              // lds_widths records whose site changed
  unsigned long long stage_waves[kLdsStages];  // located records per stage
  unsigned long long stage_moved[kLdsStages];
  unsigned long long lds_bytes;          // bytes of the allocation the march covered (0 from the bare reduction)
  unsigned long long sub_bad[kLdsStages][kLdsSubs];  // located wrong words per stage and sub-check
  double stage_ms[kLdsStages];           // device time per stage over all launches
  int launches;
  int cus_reached;                       // distinct (xcc, se, sh, cu) with a located lds_widths record
  int simds_reached;                     // distinct sites with one
  int cus_expected;                      // multiProcessorCount (0 from the bare reduction)
  int n_bad;                             // sites with a located wrong word of any stage
  unsigned int bad_sites[16];            // the first 16 of them, packed
  int stage_n_bad[kLdsStages];           // CUs (stages 0, 1) or sites (2, 3) with a located wrong word
  unsigned int stage_first_site[kLdsStages];  // the lowest of them (stages 0, 1: the reading wave's site)
  unsigned int stage_first_sub[kLdsStages];   // first_sub / first_at of the first bad record at that CU or site
  unsigned int stage_first_at[kLdsStages];
  int blocks;                            // grid of one launch; reps, steps, rounds as run (0 from the bare reduction)
  int reps;
  int steps;
  int rounds;
};

}  // extern "C"

namespace ldspath {

using canary::format_site;
using canary::kMaxBlocks;
using canary::located;
using canary::plural;
using canary::records_valid;

constexpr int kMaxReps = 64, kMaxSteps = 64, kMaxRounds = 64;
constexpr int kThreads = 256;
constexpr uint32_t kInjectBit = 1u << 9;
constexpr int kInjectLane = 3;
constexpr int kInjectKinds = 6;  // 0 lds, 1 subword, 2 dma, 3 atomic, 4 lane, 5 tr

using canary::mix32;  // the hash of mfma_forms.h

// ---- stage 1: lds_widths -------------------------------------------------------------------
// Word i of the region under seed s (s already folds in the launch seed, the block and the rep).
LDSPATH_HD uint32_t lds_pat(uint32_t i, uint32_t s) { return i * 0x9E3779B1u ^ s; }
LDSPATH_HD uint32_t block_seed(uint32_t seed, uint32_t block, uint32_t rep) {
  return mix32((static_cast<uint64_t>(seed) << 32) ^ (static_cast<uint64_t>(rep) << 20) ^ block);
}
// Word i of the global buffer the LDS-DMA pass reads (the same for every workgroup).
LDSPATH_HD uint32_t dma_pat(uint32_t i, uint32_t seed) { return (i * 0x85EBCA77u + 0x6A09E667u) ^ (seed * 0x9E3779B1u); }

constexpr int kKindPlain = 0, kKindSubword = 1, kKindDma = 2, kKindConflict = 3;
struct WidthPass {
  const char* name;   // as the error text names it
  const char* store;  // how the data got there
  const char* load;   // how it is read back
  const char* map;    // lane -> address
  int kind;
};
// In the order of the docs; the kernel runs pass 6 right after pass 1, on the data pass 1 left.
constexpr WidthPass kWidthPasses[] = {
    {"128-bit store", "ds_write_b128", "ds_read_b32", "store lane-linear, load descending", kKindPlain},
    {"128-bit load", "ds_write_b32 of the complement", "ds_read_b128", "lane-linear", kKindPlain},
    {"sub-dword load", "ds_write_b64", "ds_read_u16, then ds_read_u8", "lane-linear", kKindSubword},
    {"8-bit store", "ds_write_b8 (lower half), ds_write_b16 (upper half)", "ds_read_b64", "lane-linear", kKindSubword},
    {"dma fill", "global_load_lds_dword (lower half), global_load_lds_dwordx4 (upper half)", "ds_read_b128",
     "lane-linear", kKindDma},
    {"conflict load", "pass 1's", "ds_read_b32 / b64 / b128",
     "lane stride 64 dwords (b32 also 32), one address, two addresses by lane parity", kKindConflict},
};
constexpr int kNumWidthPasses = sizeof(kWidthPasses) / sizeof(kWidthPasses[0]);

// ---- stage 2: lds_atomic -------------------------------------------------------------------
// One table of kAtomForms regions of kAtomWords 32-bit words.  32-bit forms: 512 elements; the
// u64 form: 256; ticket: seen[0..255] then the counter at 256, the rest untouched.
constexpr int kAtomForms = 10;
constexpr int kAtomWords = 512;
constexpr int kAtomU32Add = 0, kAtomU64Add = 1, kAtomI32Min = 2, kAtomU32Max = 3, kAtomAnd = 4, kAtomOr = 5,
              kAtomXor = 6, kAtomF32Add = 7, kAtomTicket = 8, kAtomCas = 9;
constexpr const char* kAtomNames[kAtomForms] = {"u32 add", "u64 add", "i32 min", "u32 max", "and",
                                                "or",      "xor",     "f32 add", "ticket",  "cas increment"};
constexpr int kCasTries = 1024;  // more than the 256 threads that could ever collide on one element

LDSPATH_HD uint32_t atomic_hash(int form, int thread, int step, int what) {
  return mix32((static_cast<uint64_t>(form) << 48) ^ (static_cast<uint64_t>(what) << 40) ^
               (static_cast<uint64_t>(step) << 16) ^ static_cast<uint64_t>(thread));
}
// Element a thread hits in a step: below 512 (32-bit forms) or 256 (u64); the ticket form has no index.
LDSPATH_HD int atomic_index(int form, int thread, int step) {
  return static_cast<int>(atomic_hash(form, thread, step, 0) % (form == kAtomU64Add ? 256u : 512u));
}
// The operand, by thread, step and form only; `inject` perturbs it so that the element it goes
// to must end up wrong: every reduction is order-independent, f32 operands are small integers,
// and no and/or mask touches kInjectBit unless injected.
LDSPATH_HD uint64_t atomic_operand(int form, int thread, int step, bool inject) {
  const uint32_t h = atomic_hash(form, thread, step, 1), h2 = atomic_hash(form, thread, step, 2);
  switch (form) {
    case kAtomU32Add: return h + (inject ? kInjectBit : 0u);
    case kAtomU64Add: return ((static_cast<uint64_t>(h2) << 32) | h) + (inject ? kInjectBit : 0u);
    case kAtomI32Min: return inject ? 0x80000000u : (h & 0x7FFFFFFFu) - 0x40000000u;  // as int: [-2^30, 2^30)
    case kAtomU32Max: return inject ? 0xFFFFFFFFu : h >> 1;
    case kAtomAnd: return inject ? ~kInjectBit : (h | h2 | kInjectBit);
    case kAtomOr: return inject ? kInjectBit : (h & h2 & ~kInjectBit);
    case kAtomXor: return h ^ (inject ? kInjectBit : 0u);
    case kAtomF32Add: return static_cast<uint64_t>(static_cast<int64_t>(static_cast<int>(h % 9u) - 4 + (inject ? 1 : 0)));
    case kAtomTicket: return inject ? 2u : 1u;  // what the thread adds to seen[ticket & 255]
    default: return (h & 0xFFu) + 1u + (inject ? 1u : 0u);  // cas increment
  }
}
// What word w of a form's region holds before the atomics.
LDSPATH_HD uint32_t atomic_init(int form, int w) {
  switch (form) {
    case kAtomI32Min: return 0x7FFFFFFFu;
    case kAtomAnd: return 0xFFFFFFFFu;
    case kAtomU32Max:
    case kAtomOr:
    case kAtomF32Add:
    case kAtomTicket: return 0u;
    default: return mix32(0xA70Bull ^ (static_cast<uint64_t>(form) << 32) ^ static_cast<uint64_t>(w));
  }
}

// The table (kAtomWords words) form `form` must hold after kThreads threads ran `steps` steps.
inline bool atomic_expected(int form, int steps, uint32_t* out) {
  if (form < 0 || form >= kAtomForms || steps < 1 || steps > kMaxSteps || out == nullptr) return false;
  for (int w = 0; w < kAtomWords; ++w) out[w] = atomic_init(form, w);
  std::vector<int> fsum(form == kAtomF32Add ? kAtomWords : 0, 0);
  for (int s = 0; s < steps; ++s) {
    for (int t = 0; t < kThreads; ++t) {
      const uint64_t v = atomic_operand(form, t, s, false);
      const int e = atomic_index(form, t, s);
      const uint32_t v32 = static_cast<uint32_t>(v);
      switch (form) {
        case kAtomU32Add:
        case kAtomCas: out[e] += v32; break;
        case kAtomU64Add: {
          const uint64_t sum = ((static_cast<uint64_t>(out[2 * e + 1]) << 32) | out[2 * e]) + v;
          out[2 * e] = static_cast<uint32_t>(sum);
          out[2 * e + 1] = static_cast<uint32_t>(sum >> 32);
          break;
        }
        case kAtomI32Min:
          if (static_cast<int32_t>(v32) < static_cast<int32_t>(out[e])) out[e] = v32;
          break;
        case kAtomU32Max:
          if (v32 > out[e]) out[e] = v32;
          break;
        case kAtomAnd: out[e] &= v32; break;
        case kAtomOr: out[e] |= v32; break;
        case kAtomXor: out[e] ^= v32; break;
        case kAtomF32Add: fsum[e] += static_cast<int>(static_cast<int64_t>(v)); break;
        default: break;  // ticket: below
      }
    }
  }
  if (form == kAtomF32Add) {
    for (int w = 0; w < kAtomWords; ++w) {
      const float f = static_cast<float>(fsum[w]);  // exact: |sum| <= 256 * 64 * 4 < 2^24
      std::memcpy(&out[w], &f, 4);
    }
  }
  if (form == kAtomTicket) {
    for (int w = 0; w < 256; ++w) out[w] = static_cast<uint32_t>(steps);  // every ticket & 255 taken `steps` times
    out[256] = static_cast<uint32_t>(kThreads * steps);
  }
  return true;
}

// ---- stage 3: lane_xchg ----------------------------------------------------------------------
// What a lane receives is a source code: 0..63 the x of that lane, 64..127 the second value
// (DPP's and writelane's `old`, the swaps' src operand) of lane code - 64, kSrcZero a zero.
constexpr int kSrcZero = 128;
constexpr int kOpBpermute = 0, kOpPermute = 1, kOpSwizzleBits = 2, kOpSwizzleQuad = 3, kOpDpp = 4, kOpSwap32 = 5,
              kOpSwap16 = 6, kOpReadlane = 7, kOpReadfirstlane = 8, kOpWritelane = 9;
struct LaneOp {
  int kind;
  int a, b, c, d;  // by kind, see src_code
};
constexpr int quad(int p0, int p1, int p2, int p3) { return p0 | p1 << 2 | p2 << 4 | p3 << 6; }
constexpr int kDppRowShl = 0x100, kDppRowShr = 0x110, kDppRowRor = 0x120, kDppWaveShl = 0x130, kDppWaveRol = 0x134,
              kDppWaveShr = 0x138, kDppWaveRor = 0x13C, kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141,
              kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;
constexpr LaneOp kLaneOps[] = {
    {kOpBpermute, 0, 0x2B, 0, 0},      // hashed, many-to-one
    {kOpBpermute, 1, 17, 0, 0},        // rotation by 17
    {kOpPermute, 5, 3, 13, 0},         // lane l sends to 5 l + 3; 13 = 5^-1 mod 64
    {kOpPermute, 27, 40, 19, 0},       // 27 l + 40; 19 = 27^-1
    {kOpPermute, 63, 63, 63, 0},       // 63 l + 63 = 63 - l: reversal
    {kOpSwizzleBits, 0x1F, 0, 1, 0},   // swap neighbours
    {kOpSwizzleBits, 0x1F, 0, 0x1F, 0},  // reversal within 32 lanes
    {kOpSwizzleBits, 0, 5, 0, 0},      // broadcast lane 5 of each half
    {kOpSwizzleBits, 0x1C, 2, 0x11, 0},  // and, or and xor together
    {kOpSwizzleQuad, quad(1, 0, 3, 2), 0, 0, 0},
    {kOpSwizzleQuad, quad(2, 2, 0, 3), 0, 0, 0},
    {kOpDpp, quad(3, 2, 1, 0), 0xF, 0xF, 0},
    {kOpDpp, quad(1, 3, 0, 2), 0xF, 0xF, 0},
    {kOpDpp, quad(2, 2, 2, 2), 0xF, 0xF, 0},  // broadcast within quads
    {kOpDpp, kDppRowShl + 1, 0xF, 0xF, 0},
    {kOpDpp, kDppRowShl + 7, 0xF, 0xF, 0},
    {kOpDpp, kDppRowShr + 1, 0xF, 0xF, 0},
    {kOpDpp, kDppRowShr + 12, 0xF, 0xF, 0},
    {kOpDpp, kDppRowShr + 3, 0xF, 0xF, 1},    // bound_ctrl: lanes without a source read 0
    {kOpDpp, kDppRowRor + 1, 0xF, 0xF, 0},
    {kOpDpp, kDppRowRor + 3, 0xF, 0xF, 0},
    {kOpDpp, kDppRowRor + 11, 0xF, 0xF, 0},
    {kOpDpp, kDppRowMirror, 0xF, 0xF, 0},
    {kOpDpp, kDppRowHalfMirror, 0xF, 0xF, 0},
    {kOpDpp, kDppWaveShl, 0xF, 0xF, 0},
    {kOpDpp, kDppWaveRol, 0xF, 0xF, 0},
    {kOpDpp, kDppWaveShr, 0xF, 0xF, 0},
    {kOpDpp, kDppWaveRor, 0xF, 0xF, 0},
    {kOpDpp, kDppRowBcast15, 0xA, 0xF, 0},    // the scan idiom: rows 1 and 3 only
    {kOpDpp, kDppRowBcast31, 0xC, 0xF, 0},    // rows 2 and 3 only
    {kOpDpp, kDppRowMirror, 0x6, 0xF, 0},     // partial row_mask
    {kOpDpp, kDppRowRor + 5, 0xF, 0x9, 0},    // partial bank_mask
    {kOpSwap32, 0, 0, 0, 0},
    {kOpSwap16, 0, 0, 0, 0},
    {kOpReadlane, 37, 0, 0, 0},
    {kOpReadlane, 6, 0, 0, 0},
    {kOpReadfirstlane, 0, 0, 0, 0},
    {kOpWritelane, 52, 9, 0, 0},   // x of lane 52 into lane 9 of the second value
    {kOpWritelane, 11, 60, 0, 0},
};
constexpr int kNumLaneOps = sizeof(kLaneOps) / sizeof(kLaneOps[0]);
static_assert(kNumLaneOps <= kLdsSubs, "a record counts every op");
constexpr const char* kLaneOpNames[kNumLaneOps] = {
    "ds_bpermute hash", "ds_bpermute rot:17", "ds_permute 5l+3", "ds_permute 27l+40", "ds_permute reverse",
    "ds_swizzle swap:1", "ds_swizzle reverse:32", "ds_swizzle broadcast:5", "ds_swizzle bitmask:0x1c,2,0x11",
    "ds_swizzle quad_perm:[1,0,3,2]", "ds_swizzle quad_perm:[2,2,0,3]", "dpp quad_perm:[3,2,1,0]",
    "dpp quad_perm:[1,3,0,2]", "dpp quad_perm:[2,2,2,2]", "dpp row_shl:1", "dpp row_shl:7", "dpp row_shr:1",
    "dpp row_shr:12", "dpp row_shr:3 bound_ctrl", "dpp row_ror:1", "dpp row_ror:3", "dpp row_ror:11", "dpp row_mirror",
    "dpp row_half_mirror", "dpp wave_shl:1", "dpp wave_rol:1", "dpp wave_shr:1", "dpp wave_ror:1",
    "dpp row_bcast:15 row_mask:0xa", "dpp row_bcast:31 row_mask:0xc", "dpp row_mirror row_mask:0x6",
    "dpp row_ror:5 bank_mask:0x9", "v_permlane32_swap", "v_permlane16_swap", "v_readlane 37", "v_readlane 6",
    "v_readfirstlane", "v_writelane 52->9", "v_writelane 11->60"};

constexpr int lane_outputs(const LaneOp& op) { return op.kind == kOpSwap32 || op.kind == kOpSwap16 ? 2 : 1; }
// every lane receives from a distinct lane (of x alone)
constexpr bool lane_op_bijective(const LaneOp& op) {
  return op.kind == kOpPermute || (op.kind == kOpBpermute && op.a == 1) ||
         (op.kind == kOpSwizzleBits && op.a == 0x1F && op.b == 0) ||
         (op.kind == kOpSwizzleQuad && op.a == quad(1, 0, 3, 2)) ||
         (op.kind == kOpDpp && op.b == 0xF && op.c == 0xF &&
          (op.a == quad(3, 2, 1, 0) || op.a == quad(1, 3, 0, 2) || (op.a > kDppRowRor && op.a < kDppWaveShl) ||
           op.a == kDppWaveRol || op.a == kDppWaveRor || op.a == kDppRowMirror || op.a == kDppRowHalfMirror));
}

// The lane a DPP control reads for lane l, -1 where it has none.
LDSPATH_HD int dpp_source(int ctrl, int l) {
  const int row = l & ~15, i = l & 15;
  if (ctrl < 0x100) return (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);
  if (ctrl > kDppRowShl && ctrl < kDppRowShr) return i + (ctrl - kDppRowShl) < 16 ? l + (ctrl - kDppRowShl) : -1;
  if (ctrl > kDppRowShr && ctrl < kDppRowRor) return i - (ctrl - kDppRowShr) >= 0 ? l - (ctrl - kDppRowShr) : -1;
  if (ctrl > kDppRowRor && ctrl < kDppWaveShl) return row | ((i - (ctrl - kDppRowRor)) & 15);
  if (ctrl == kDppWaveShl) return l + 1 < 64 ? l + 1 : -1;
  if (ctrl == kDppWaveRol) return (l + 1) & 63;
  if (ctrl == kDppWaveShr) return l >= 1 ? l - 1 : -1;
  if (ctrl == kDppWaveRor) return (l - 1) & 63;
  if (ctrl == kDppRowMirror) return row | (15 - i);
  if (ctrl == kDppRowHalfMirror) return (l & ~7) | (7 - (l & 7));
  if (ctrl == kDppRowBcast15) return l >= 16 ? row - 1 : -1;
  if (ctrl == kDppRowBcast31) return l >= 32 ? 31 : -1;
  return -1;
}

// The source code of output `out` (0; 1 for the swaps' second value) of lane l.
LDSPATH_HD int src_code(const LaneOp& op, int out, int l) {
  switch (op.kind) {
    case kOpBpermute: return op.a == 0 ? static_cast<int>(((l * 0x9E5u + static_cast<unsigned>(op.b)) >> 3) & 63u) : (l + op.b) & 63;
    case kOpPermute: return ((l - op.b) * op.c) & 63;  // the lane d with a d + b = l (mod 64)
    case kOpSwizzleBits: return (l & 32) | ((((l & 31) & op.a) | op.b) ^ op.c);
    case kOpSwizzleQuad: return (l & ~3) | ((op.a >> (2 * (l & 3))) & 3);
    case kOpDpp: {
      if (!((op.b >> (l >> 4)) & 1) || !((op.c >> ((l >> 2) & 3)) & 1)) return 64 + l;  // masked: keeps old
      const int s = dpp_source(op.a, l);
      return s >= 0 ? s : op.d ? kSrcZero : 64 + l;
    }
    case kOpSwap32:  // lanes 32-63 of the first operand change places with lanes 0-31 of the second
      return out == 0 ? (l < 32 ? l : 64 + (l - 32)) : (l < 32 ? l + 32 : 64 + l);
    case kOpSwap16:  // odd rows of the first operand change places with even rows of the second
      return out == 0 ? ((l & 16) ? 64 + (l - 16) : l) : ((l & 16) ? 64 + l : l + 16);
    case kOpReadlane: return op.a;
    case kOpReadfirstlane: return 0;
    default: return l == op.b ? op.a : 64 + l;  // writelane
  }
}

// x (which 0) and the second value (which 1) of lane l of wave w in round r.
LDSPATH_HD uint32_t lane_value(uint32_t seed, uint32_t w, int l, int r, int which) {
  return mix32((static_cast<uint64_t>(seed) << 32) ^ (static_cast<uint64_t>(w) << 16) ^
               (static_cast<uint64_t>(which) << 14) ^ (static_cast<uint64_t>(r) << 6) ^ static_cast<uint64_t>(l));
}
LDSPATH_HD uint32_t lane_expected(uint32_t seed, uint32_t w, int code, int r) {
  return code == kSrcZero ? 0u : lane_value(seed, w, code & 63, r, code >> 6);
}

// ---- stage 4: lds_tr ----------------------------------------------------------------------
constexpr int kTrImageBytes = 128 * 1024;
constexpr int kTrElems = kTrImageBytes / 2;
constexpr int kTrFixedRounds = 6;  // four row strides and the two dual-use images; hashed rounds follow
LDSPATH_HD uint32_t tr_pat(uint32_t i, uint32_t seed) { return (i * 0x9E37u + seed) & 0xFFFFu; }
constexpr int tr_rounds(int rounds) { return kTrFixedRounds + rounds; }

// Byte offset of 16-byte chunk ch of row `row` in the two dual-use images of a [rows][128 x 16-bit] tile.
LDSPATH_HD int tr_off_a(int row, int ch) {
  return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}
LDSPATH_HD int tr_off_b(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// The 8-byte-aligned byte address lane l supplies in round r: lane 4q + p of a 16-lane group
// names row q, columns 4p .. 4p + 3 of that group's block.
LDSPATH_HD int tr_addr(int l, int r) {
  const int g = l >> 4, q = (l >> 2) & 3, p = l & 3;
  if (r < 4) {
    const int stride = r == 0 ? 32 : r == 1 ? 64 : r == 2 ? 256 : 264;
    return 4096 * r + g * 4 * stride + q * stride + 8 * p;
  }
  if (r == 4) return 32768 + tr_off_a(4 * g + q + 8, 2 * g + 4 + (p >> 1)) + 8 * (p & 1);
  if (r == 5) return 65536 + tr_off_b(4 * g + q + 4, 2 * g + 6 + (p >> 1)) + 8 * (p & 1);
  return static_cast<int>(mix32((static_cast<uint64_t>(r) << 8) ^ static_cast<uint64_t>(l) ^ 0x7A0000ull) % (kTrImageBytes / 8)) * 8;
}
// The 16-bit element (index into the image) lane l receives in element q of round r.
LDSPATH_HD int tr_source(int l, int q, int r) {
  const int i = l & 15;
  return (tr_addr((l & ~15) + 4 * q + (i >> 2), r) >> 1) + (i & 3);
}

// ---- records -> result ---------------------------------------------------------------------
inline int stage_subs(int stage) {
  return stage == 0 ? kNumWidthPasses : stage == 1 ? kAtomForms : stage == 2 ? kNumLaneOps : 1;
}

// recs[s] / n[s]: stage s's records in launch order (unwritten slots are skipped); any may be
// empty.  out keeps lds_bytes, stage_ms, launches, cus_expected, blocks, reps, steps and rounds
// the caller set and gets everything else.  false: a bad argument.
inline bool reduce(const amdgpu_ldspath_record* const recs[kLdsStages], const int n[kLdsStages], amdgpu_ldspath_result* out) {
  if (out == nullptr) return false;
  for (int s = 0; s < kLdsStages; ++s)
    if (n[s] < 0 || (n[s] > 0 && recs[s] == nullptr) || !records_valid(recs[s], n[s])) return false;
  amdgpu_ldspath_result r;
  std::memset(&r, 0, sizeof(r));
  r.lds_bytes = out->lds_bytes;
  std::memcpy(r.stage_ms, out->stage_ms, sizeof(r.stage_ms));
  r.launches = out->launches;
  r.cus_expected = out->cus_expected;
  r.blocks = out->blocks;
  r.reps = out->reps;
  r.steps = out->steps;
  r.rounds = out->rounds;
  std::vector<unsigned char> reached(kLdsSiteSlots, 0);
  std::vector<unsigned int> site_bad(kLdsSiteSlots, 0);
  for (int s = 0; s < kLdsStages; ++s) {
    const bool by_cu = s < 2;  // an LDS fault belongs to a CU; a lane fault to a SIMD
    std::vector<unsigned int> where_bad(kLdsSiteSlots, 0);  // by_cu: index site | 3
    r.stage_first_site[s] = r.stage_first_sub[s] = r.stage_first_at[s] = kLdsUnwritten;
    const int subs = stage_subs(s);
    unsigned int best = kLdsUnwritten;
    for (int i = 0; i < n[s]; ++i) {
      const amdgpu_ldspath_record& rec = recs[s][i];
      if (rec.site_first == kLdsUnwritten) continue;
      unsigned long long total = 0;
      for (int k = 0; k < subs; ++k) total += rec.bad[k];
      if (!located(rec)) {
        ++r.stage_moved[s];
        r.unlocated_errors += total;
        continue;
      }
      ++r.stage_waves[s];
      if (s == 0) reached[rec.site_first] = 1;
      for (int k = 0; k < subs; ++k) r.sub_bad[s][k] += rec.bad[k];
      if (total == 0) continue;
      site_bad[rec.site_first] += 1;
      const unsigned int key = by_cu ? (rec.site_first | 3u) : rec.site_first;
      // the lowest bad CU (or site) is named, with the detail of its first bad record
      if (where_bad[key]++ == 0 && key < best) {
        best = key;
        r.stage_first_site[s] = rec.site_first;
        r.stage_first_sub[s] = rec.first_sub;
        r.stage_first_at[s] = rec.first_at;
      }
    }
    for (int k = 0; k < kLdsSiteSlots; ++k) r.stage_n_bad[s] += where_bad[k] != 0;
  }
  for (int k = 0; k < kNumWidthPasses; ++k) {
    const unsigned long long b = r.sub_bad[0][k];
    switch (kWidthPasses[k].kind) {
      case kKindPlain: r.plain_errors += b; break;
      case kKindSubword: r.subword_errors += b; break;
      case kKindDma: r.dma_errors += b; break;
      default: r.conflict_errors += b; break;
    }
  }
  r.lds_errors = r.plain_errors + r.subword_errors + r.conflict_errors;
  for (int k = 0; k < kAtomForms; ++k) r.lds_atomic_errors += r.sub_bad[1][k];
  for (int k = 0; k < kNumLaneOps; ++k) r.lane_errors += r.sub_bad[2][k];
  r.tr_errors = r.sub_bad[3][0];
  r.waves = r.stage_waves[0];
  r.moved = r.stage_moved[0];
  // wrong DMA words may be L2's or HBM's; beside wrong plain-store words they are the LDS's again and are not added
  r.ldspath_errors = r.lds_errors + (r.lds_errors == 0 ? r.dma_errors : 0) + r.lds_atomic_errors + r.lane_errors +
                     r.tr_errors + r.unlocated_errors;
  canary::store_coverage(canary::site_coverage([&](int site) { return reached[site] != 0; },
                                               [&](int site) { return site_bad[site] != 0; }),
                         &r);
  *out = r;
  return true;
}

// "+1 more CU" / "+2 more sites", empty when there are no others
inline void more_text(char* buf, int len, int others, const char* unit) {
  if (len > 0) buf[0] = 0;
  if (others > 0) std::snprintf(buf, len, "+%d more %s%s", others, unit, others > 1 ? "s" : "");
}

// The text of stage `which` (0..3), or of the first failing stage (which < 0):
//   "lds check: 3 wrong words at xcc3/se1/sh0/cu7 (pass 4, 8-bit store; first at offset 0x1a40; +1 more CU)"
//   "lds dma check: 1 wrong word at xcc3/se1/sh0/cu7 (pass 5, dma fill; first at offset 0x40)"
//   "lds atomic check: 2 wrong elements in u64 add at xcc1/se0/sh0/cu3 (first at 41)"
//   "lane check: 4 wrong words in dpp row_ror:3 at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
//   "lds transpose check: 2 wrong elements at xcc3/se1/sh0/cu7/simd2 (+1 more site)"
//   "ldspath check: 4 wrong words at an unknown site"     (every wrong wave moved while it ran)
// Returns its length, 0 (and an empty text) if that stage did not fail.
inline int describe(const amdgpu_ldspath_result& r, int which, char* buf, int len) {
  if (len > 0) buf[0] = 0;
  char where[64], others[48];
  if ((which < 0 || which == 0) && (r.lds_errors > 0 || r.dma_errors > 0) && r.stage_n_bad[0] > 0) {
    const unsigned long long count = r.lds_errors > 0 ? r.lds_errors : r.dma_errors;
    format_site(r.stage_first_site[0], false, where, sizeof(where));
    more_text(others, sizeof(others), r.stage_n_bad[0] - 1, "CU");
    const unsigned int pass = r.stage_first_sub[0] < static_cast<unsigned int>(kNumWidthPasses) ? r.stage_first_sub[0] : 0;
    return std::snprintf(buf, len, "%s: %llu wrong word%s at %s (pass %u, %s; first at offset 0x%x%s%s)",
                         r.lds_errors > 0 ? "lds check" : "lds dma check", count, plural(count), where, pass + 1,
                         kWidthPasses[pass].name, r.stage_first_at[0], others[0] ? "; " : "", others);
  }
  if ((which < 0 || which == 1) && r.lds_atomic_errors > 0 && r.stage_n_bad[1] > 0) {
    format_site(r.stage_first_site[1], false, where, sizeof(where));
    more_text(others, sizeof(others), r.stage_n_bad[1] - 1, "CU");
    const unsigned int form = r.stage_first_sub[1] < static_cast<unsigned int>(kAtomForms) ? r.stage_first_sub[1] : 0;
    return std::snprintf(buf, len, "lds atomic check: %llu wrong element%s in %s at %s (first at %u%s%s)",
                         r.lds_atomic_errors, plural(r.lds_atomic_errors), kAtomNames[form], where, r.stage_first_at[1],
                         others[0] ? "; " : "", others);
  }
  if ((which < 0 || which == 2) && r.lane_errors > 0 && r.stage_n_bad[2] > 0) {
    format_site(r.stage_first_site[2], true, where, sizeof(where));
    more_text(others, sizeof(others), r.stage_n_bad[2] - 1, "site");
    const unsigned int op = r.stage_first_sub[2] < static_cast<unsigned int>(kNumLaneOps) ? r.stage_first_sub[2] : 0;
    return std::snprintf(buf, len, "lane check: %llu wrong word%s in %s at %s%s%s%s", r.lane_errors, plural(r.lane_errors),
                         kLaneOpNames[op], where, others[0] ? " (" : "", others, others[0] ? ")" : "");
  }
  if ((which < 0 || which == 3) && r.tr_errors > 0 && r.stage_n_bad[3] > 0) {
    format_site(r.stage_first_site[3], true, where, sizeof(where));
    more_text(others, sizeof(others), r.stage_n_bad[3] - 1, "site");
    return std::snprintf(buf, len, "lds transpose check: %llu wrong element%s at %s%s%s%s", r.tr_errors, plural(r.tr_errors),
                         where, others[0] ? " (" : "", others, others[0] ? ")" : "");
  }
  if (which < 0 && r.unlocated_errors > 0)
    return std::snprintf(buf, len, "ldspath check: %llu wrong word%s at an unknown site", r.unlocated_errors,
                         plural(r.unlocated_errors));
  return 0;
}

// The argument rule of amdgpu_ldspath_run, checked before any HIP call.
inline bool arguments_ok(int blocks, int reps, int steps, int rounds, int inject_kind, int inject_waves, int inject_op,
                         int wave_site_len, bool have_wave_site) {
  if (blocks < 0 || blocks > kMaxBlocks || reps < 1 || reps > kMaxReps || steps < 1 || steps > kMaxSteps) return false;
  if (rounds < 1 || rounds > kMaxRounds || inject_kind < -1 || inject_kind >= kInjectKinds || inject_waves < 0) return false;
  if (inject_op < 0 || (inject_kind == 3 && inject_op >= kAtomForms) || (inject_kind == 4 && inject_op >= kNumLaneOps)) return false;
  if (wave_site_len < 0 || (!have_wave_site && wave_site_len != 0)) return false;
  return true;
}

}  // namespace ldspath
