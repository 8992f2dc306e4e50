// C ABI of the attention-path check (ops/attn/libamdgpu_attn.so), mirrored with ctypes in
// ops/attn.py.  The library is built apart from libamdgpu_canary.so and shares its header-only
// helpers (../canary_host.h); shape rules, data, closed forms and the result are in attn_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "attn_host.h"

extern "C" {

// o[H][Sq][128] (fp32) = softmax(q k^T / sqrt(128)) v and lse[H][Sq], its natural-log sum of
// exponentials, on host data through attn_fwd.  q [H][Sq][128], k and v [H][Sk][128]: bf16 bit
// patterns.  causal: key j is visible to query i when j <= i + (Sk - Sq).  0, or -1 with `err`
// set (a refused shape is refused before any HIP call).
int amdgpu_attn_run(int device, const unsigned short* q, const unsigned short* k, const unsigned short* v, float* o,
                    float* lse, int H, int Sq, int Sk, int causal, char* err, int err_len);
// The check.  Per data set (uniform, routed, hashed): device-generated operands, one warm-up launch,
// `iters` timed ones, O and lse poisoned with 0xFF bytes, one untimed launch, and the verdict on
// that output: bit equality with the closed form for the first two, the derived bounds against a
// float64 host reference of `rows` rows per head for the third.  H, Sq, Sk of 0: the default
// workload.  flags: kAttnInject writes one junk element of O after each verified launch (1 error
// per set), kAttnSkipVerifiedLaunch leaves the poison in place.  0, or -1 with `err` set.
int amdgpu_attn_check(int device, int H, int Sq, int Sk, int causal, int iters, int rows, int flags,
                      amdgpu_attn_result* result, char* err, int err_len);
constexpr int kAttnInject = 1, kAttnSkipVerifiedLaunch = 2;
constexpr int kAttnDefaultHeads = 32, kAttnDefaultSeq = 4096;  // 1024 workgroups: 4 per CU of an MI355X
// host only: the failing text of a result into buf (returns its length); 0 if it did not fail
int amdgpu_attn_describe(const amdgpu_attn_result* r, char* buf, int len);
// host only: the check's own data of set `set` as bf16 bit patterns, q [H][Sq][128], k and v [H][Sk][128].  0, or -1.
int amdgpu_attn_operands(int set, int H, int Sq, int Sk, unsigned short* q, unsigned short* k, unsigned short* v);
// host only: what a healthy kernel gives for an exact set (0 uniform, 1 routed): o [H][Sq][128]
// bit for bit, lse [H][Sq] in float64.  0, or -1 (the hashed set has no closed form).
int amdgpu_attn_expected(int set, int H, int Sq, int Sk, int causal, float* o, double* lse);
// 0: sizeof(amdgpu_attn_result); -1 otherwise
int amdgpu_attn_sizeof(int which);

}  // extern "C"

static_assert(sizeof(amdgpu_attn_result) == 168, "attn.AttnResult");
