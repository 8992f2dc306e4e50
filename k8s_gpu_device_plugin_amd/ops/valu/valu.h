// C ABI of the vector-ALU check (ops/valu/libamdgpu_valu.so), mirrored with ctypes in
// ops/valu.py.  The library is built apart from libamdgpu_canary.so and shares its header-only
// helpers (../canary_common.h, ../canary_host.h, ../site.h); the ops are in valu_ops.h, the
// structs and the reduction in valu_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "valu_host.h"

extern "C" {

// Runs valu_sweep of every group that holds a selected op (selected[op] != 0, kNumOps entries) on
// `device` and reduces the records.  blocks == 0: 2 workgroups per CU plus up to 3 more launches
// while a CU or SIMD has no located record of some selected group; blocks > 0: one launch of that
// many workgroups.  rounds: 1..16 per op.  inject_op >= 0: lane 3 of the first inject_waves waves
// of the first launch adds 1 to the first result word of that op in round 0.  wave_site_out
// (group g: wave_site_out[g * wave_site_len + wave], the starting site of the first
// wave_site_len waves of the first launch; all-ones where none ran) may be null.
// 0, or -1 with `err` set.
int amdgpu_valu_run(int device, int blocks, int rounds, unsigned int seed, const unsigned char* selected, int inject_op,
                    int inject_waves, unsigned int* wave_site_out, int wave_site_len, amdgpu_valu_result* result, char* err,
                    int err_len);
// host only: the reduction on caller-supplied records; group_of[i] is the group record i belongs to.
int amdgpu_valu_reduce(const amdgpu_valu_record* recs, const int* group_of, int n, const unsigned char* selected,
                       amdgpu_valu_result* result);
// One op on caller-supplied operands, n_waves waves: lane l of wave w reads a / b / c[w * 64 + l]
// and leaves its result words in out[(w * 64 + l) * 32 ..] (zero past the op's results).
int amdgpu_valu_raw(int device, int op, const unsigned long long* a, const unsigned long long* b, const unsigned long long* c,
                    unsigned int* out, int n_waves, char* err, int err_len);
// host only: the operands of round r, lane l at a / b / c[r * 64 + l].  0, or -1.
int amdgpu_valu_operands(int op, unsigned int seed, int rounds, unsigned long long* a, unsigned long long* b,
                         unsigned long long* c);
// host only: the 64 lane digests of an exact op.  0; -1: bad arguments; -2: a generated case is not normal or zero.
int amdgpu_valu_expected(int op, unsigned int seed, int rounds, unsigned int* digest);
// the table: index < 0: the count; what 0 name, 1 mnemonic, 2 group name into buf (returns the length); -1: no such entry
int amdgpu_valu_ops(int index, int what, char* buf, int len);
// group, class (0 exact, 1 consensus), the three operand kinds, result words, result kind
int amdgpu_valu_op_ints(int index, int* out7);
// the text of op `which` (< 0: the first failing); 0 if it did not fail
int amdgpu_valu_describe(const amdgpu_valu_result* r, int which, char* buf, int len);
// host only: the 32 elements of a wide conversion's operand (six-bit codes of a pk32 decoder, f32 encoder inputs of
// a 2xpk16 encoder) from its operand words a and c.  0, or -1: not a wide op.
int amdgpu_valu_expand(int op, unsigned long long a, unsigned long long c, unsigned int* out32);
// the name of operand kind `kind` into buf (returns the length); -1: no such kind
int amdgpu_valu_kind(int kind, char* buf, int len);
// 0: record, 1: result; the constants ops/valu.py repeats: 2 waves per workgroup, 3 ops a result has room for,
// 4 ops a record has room for, 5 groups a result has room for, 6 the most rounds, 7 result words of a lane, 8 the injected lane
int amdgpu_valu_sizeof(int which);

}  // extern "C"

static_assert(sizeof(amdgpu_valu_record) == 272, "valu.Record");
static_assert(sizeof(amdgpu_valu_result) == 3080, "valu.ValuResult");
