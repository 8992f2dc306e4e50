// C ABI of the decode-attention check (ops/decode/libamdgpu_decode.so), mirrored with ctypes in
// ops/decode.py.  The library is built apart from libamdgpu_canary.so and shares its header-only
// helpers (../canary_host.h); shape rules, data, closed forms and the result are in decode_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "decode_host.h"

extern "C" {

// o[B][Hq][128] (fp32) = softmax(q k^T / sqrt(128)) v over the first seq_lens[b] keys of sequence b,
// and lse[B][Hq], the natural-log sum of exponentials of the scaled scores, on host data through
// decode_split and decode_combine.  q [B][Hq][128], k_cache and v_cache [P][Hkv][16][128]: bf16 bit
// patterns.  block_table [B][max_pages]: entry t is the physical page of keys 16 t .. 16 t + 15 of
// the sequence (entries past its last page are not read).  Query head hq reads KV head hq / (Hq / Hkv).
// splits: partitions of each sequence's key range, 0: the library chooses.  0, or -1 with `err` set
// (a bad shape, length, table entry or splits is refused before any HIP call).
int amdgpu_decode_run(int device, const unsigned short* q, const unsigned short* k_cache, const unsigned short* v_cache,
                      const int* block_table, const int* seq_lens, float* o, float* lse, int B, int Hq, int Hkv, int P,
                      int max_pages, int splits, char* err, int err_len);
// The check.  Per data set (uniform, routed, hashed): the caches filled on the device through the
// check's permuted block table, one warm-up launch pair, `iters` timed ones, o and lse poisoned with
// 0xFF bytes, one untimed pair, and the verdict on that output: bit equality with the closed form
// for the first two, the derived bounds against a float64 host reference of every (sequence, head)
// for the third.  B, Hq, Hkv, seq of 0: the default workload.  flags: kDecodeInject writes one junk
// element of o after each verified pair (1 error per set), kDecodeSkipVerifiedLaunch leaves the
// poison in place.  0, or -1 with `err` set.
int amdgpu_decode_check(int device, int B, int Hq, int Hkv, int seq, int splits, int iters, int flags,
                        amdgpu_decode_result* result, char* err, int err_len);
constexpr int kDecodeInject = 1, kDecodeSkipVerifiedLaunch = 2;
// 2 GiB of K and V; on the 256 CUs of an MI355X the library chooses 2 splits: 1024 workgroups, four per CU
constexpr int kDecodeDefaultBatch = 64, kDecodeDefaultQHeads = 32, kDecodeDefaultKvHeads = 8, kDecodeDefaultSeq = 8192;
// host only: the failing text of a result into buf (returns its length); 0 if it did not fail
int amdgpu_decode_describe(const amdgpu_decode_result* r, char* buf, int len);
// host only: the check's own data of set `set` as the check lays it out: q [B][Hq][128], the caches
// [B * ceil(seq / 16)][Hkv][16][128] (bf16 bit patterns; 0xFFFF where no visible key lies), the
// table [B][ceil(seq / 16)] (-1 past a sequence's last page) and the lengths [B].  0, or -1.
int amdgpu_decode_operands(int set, int B, int Hq, int Hkv, int seq, unsigned short* q, unsigned short* k_cache,
                           unsigned short* v_cache, int* block_table, int* seq_lens);
// host only: what a healthy pair gives for an exact set (0 uniform, 1 routed): o [B][Hq][128]
// bit for bit, lse [B][Hq] in float64.  0, or -1 (the hashed set has no closed form).
int amdgpu_decode_expected(int set, int B, int Hq, int Hkv, int seq, float* o, double* lse);
// 0: sizeof(amdgpu_decode_result); -1 otherwise
int amdgpu_decode_sizeof(int which);

}  // extern "C"

static_assert(sizeof(amdgpu_decode_result) == 168, "decode.DecodeResult");
