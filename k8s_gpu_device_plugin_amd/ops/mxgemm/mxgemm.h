// C ABI of the block-scaled matrix-path check (ops/mxgemm/libamdgpu_mxgemm.so), mirrored with
// ctypes in ops/mxgemm.py.  The library is built apart from libamdgpu_canary.so and shares its
// header-only helpers (../canary_host.h); packing, data, shape rules and the result are in
// mxgemm_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "mxgemm_host.h"

extern "C" {

// C[MxN] (fp32) = dequant(A)[MxK] * dequant(Bt)[NxK]^T on host data through mx_gemm.  a / bt: packed
// rows (one OCP code per byte, fp4 two per byte with the even k in the low nibble), sa [M][K/32],
// sb [N][K/32] E8M0 bytes.  kernel: an id of the table, 0 for the library's choice.  0, or -1 with
// `err` set (a refused shape is refused before any HIP call).
int amdgpu_mxgemm_run(int device, int fmt, int kernel, const unsigned char* a, const unsigned char* bt,
                      const unsigned char* sa, const unsigned char* sb, float* c, int M, int N, int K, char* err,
                      int err_len);
// The check: device-generated integer operands and scales, one warm-up launch, `iters` timed ones,
// C poisoned with 0xFF bytes, one untimed launch, and the ABFT verdict on that product.
// flags: kMxInject writes one junk element after the verified launch (2 errors expected),
// kMxSkipVerifiedLaunch leaves the poison in place (M + N expected).  0, or -1 with `err` set.
int amdgpu_mxgemm_check(int device, int fmt, int kernel, int M, int N, int K, int iters, int vary_scale, int flags,
                        amdgpu_mxgemm_result* result, char* err, int err_len);
constexpr int kMxInject = 1, kMxSkipVerifiedLaunch = 2;
// host only: the failing text of a result into buf (returns its length); 0 if it did not fail
int amdgpu_mxgemm_describe(const amdgpu_mxgemm_result* r, char* buf, int len);
// host only: the table.  id < 0: the number of ids (0 included); else out3 = tile edge, threads,
// LDS bytes of kernel `id` (zeros for id 0).  -1: no such id.
int amdgpu_mxgemm_kernels(int id, int* out3);
// host only: the id that runs for `kernel` at this shape (kernel 0: the library's choice); 0: refused
int amdgpu_mxgemm_pick(int fmt, int kernel, int M, int N, int K);
// host only: the check's own data of operand `which` (0: A, 1: Bt): codes [rows][K] one per byte,
// scales [rows][K/32], values [rows][K] int64 (the integers the codes stand for).  0, or -1.
int amdgpu_mxgemm_operand(int fmt, int which, int rows, int K, int vary_scale, unsigned char* codes,
                          unsigned char* scales, long long* values);
// 0: sizeof(amdgpu_mxgemm_result); -1 otherwise
int amdgpu_mxgemm_sizeof(int which);

}  // extern "C"

static_assert(sizeof(amdgpu_mxgemm_result) == 56, "mxgemm.MxGemmResult");
