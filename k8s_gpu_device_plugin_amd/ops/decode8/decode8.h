// C ABI of the fp8 decode-attention check (ops/decode8/libamdgpu_decode8.so), mirrored with ctypes in
// ops/decode8.py.  The library is built apart from libamdgpu_canary.so and libamdgpu_decode.so and
// shares their header-only helpers (../canary_host.h, ../decode/decode_host.h through decode8_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "decode8_host.h"

extern "C" {

// o[B][Hq][128] (fp32) = softmax(q k^T / sqrt(128)) v over the first seq_lens[b] keys of sequence b,
// and lse[B][Hq], on host data through kv8_split and kv8_combine.  q [B][Hq][128]: bf16 bit patterns.
// k_cache and v_cache [P][Hkv][16][128]: OCP e4m3 codes, one byte each; key j of KV head h is
// k_scale[h] * fp8(k_cache[...]), likewise V.  k_scale, v_scale [Hkv]: finite and positive.
// block_table, seq_lens, Hq / Hkv and splits are amdgpu_decode_run's.  0, or -1 with `err` set (a
// bad shape, length, table entry, splits or scale is refused before any HIP call).
int amdgpu_decode8_run(int device, const unsigned short* q, const unsigned char* k_cache, const unsigned char* v_cache,
                       const float* k_scale, const float* v_scale, const int* block_table, const int* seq_lens, float* o,
                       float* lse, int B, int Hq, int Hkv, int P, int max_pages, int splits, char* err, int err_len);
// The check: amdgpu_decode_check's sequence per data set (uniform, routed, hashed) on caches poisoned
// with 0xFF (an e4m3 NaN) and filled on the device through the check's permuted block table.  Bit
// equality with the closed form for the first two, the derived bounds against a float64 host
// reference over the dequantised values for the third.  flags as below.  0, or -1 with `err` set.
int amdgpu_decode8_check(int device, int B, int Hq, int Hkv, int seq, int splits, int iters, int flags,
                         amdgpu_decode8_result* result, char* err, int err_len);
constexpr int kDecode8Inject = 1, kDecode8SkipVerifiedLaunch = 2;
// decode's default workload; with one byte per element 1 GiB of K and V
constexpr int kDecode8DefaultBatch = 64, kDecode8DefaultQHeads = 32, kDecode8DefaultKvHeads = 8, kDecode8DefaultSeq = 8192;
// host only: the failing text of a result into buf (returns its length); 0 if it did not fail
int amdgpu_decode8_describe(const amdgpu_decode8_result* r, char* buf, int len);
// host only: the check's own data of set `set` as the check lays it out: q [B][Hq][128] (bf16 bits),
// the caches [B * ceil(seq / 16)][Hkv][16][128] (codes; 0xFF where no visible key lies), the scales
// [Hkv], the table [B][ceil(seq / 16)] (-1 past a sequence's last page) and the lengths [B].  0, or -1.
int amdgpu_decode8_operands(int set, int B, int Hq, int Hkv, int seq, unsigned short* q, unsigned char* k_cache,
                            unsigned char* v_cache, float* k_scale, float* v_scale, int* block_table, int* seq_lens);
// host only: what a healthy pair gives for an exact set (0 uniform, 1 routed): o [B][Hq][128]
// bit for bit, lse [B][Hq] in float64.  0, or -1 (the hashed set has no closed form).
int amdgpu_decode8_expected(int set, int B, int Hq, int Hkv, int seq, float* o, double* lse);
// 0: sizeof(amdgpu_decode8_result); -1 otherwise
int amdgpu_decode8_sizeof(int which);

}  // extern "C"

static_assert(sizeof(amdgpu_decode8_result) == 168, "decode8.Decode8Result");
