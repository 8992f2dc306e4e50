// C ABI of the LDS-path check (ops/ldspath/libamdgpu_ldspath.so), mirrored with ctypes in
// ops/ldspath.py.  The library is built apart from libamdgpu_canary.so and shares its
// header-only helpers (../canary_common.h, ../canary_host.h, ../site.h); the tables, the
// structs and the reduction are in ldspath_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "ldspath_host.h"

extern "C" {

// inject_kind of amdgpu_ldspath_run
constexpr int kLdsInjectLds = 0, kLdsInjectSubword = 1, kLdsInjectDma = 2, kLdsInjectAtomic = 3, kLdsInjectLane = 4,
              kLdsInjectTr = 5;

// Runs the four stages on `device` and reduces their records.  blocks == 0: 2 workgroups per
// CU plus up to 3 more launches (of all four stages) while a CU or SIMD has no located
// lds_widths record; blocks > 0: one launch of that many workgroups.  reps: repetitions of the
// width-pass table; steps: atomic operations per thread and form; rounds: rounds per lane op,
// and hashed rounds of the transposed read after its 6 fixed ones (each 1..64).  inject_kind -1
// none, else the first inject_waves waves (atomic: workgroups) of the first launch perturb one
// compared value: 0 lds, 1 subword, 2 dma, 3 atomic (form inject_op), 4 lane (op inject_op), 5 tr.
// wave_site_out (4 * wave_site_len entries: per stage, the starting site of the first
// wave_site_len waves of the first launch; all-ones where none ran) may be null.
// 0, or -1 with `err` set.
int amdgpu_ldspath_run(int device, int blocks, int reps, int steps, int rounds, int inject_kind, int inject_waves,
                       int inject_op, unsigned int* wave_site_out, int wave_site_len, amdgpu_ldspath_result* result,
                       char* err, int err_len);
// host only: the reduction on caller-supplied records of the four stages (any may be empty).
// 0, or -1 on a bad argument (a site out of range).
int amdgpu_ldspath_reduce(const amdgpu_ldspath_record* widths, int n_widths, const amdgpu_ldspath_record* atomic,
                          int n_atomic, const amdgpu_ldspath_record* lane, int n_lane, const amdgpu_ldspath_record* tr,
                          int n_tr, amdgpu_ldspath_result* result);
// One wave with x = lane and the second value = 64 + lane: out[(op * 2 + output) * 64 + lane] is
// what each lane received (output 1 only for the two swaps).  out_len >= ops * 128.
int amdgpu_ldspath_lane_sources(int device, unsigned int* out, int out_len, char* err, int err_len);
// host only: the table's source codes of op k, out[output * 64 + lane] (128 entries): 0..63 x of
// that lane, 64..127 the second value of lane code - 64, 128 zero.  Returns the outputs (1 or 2), -1: no such op.
int amdgpu_ldspath_lane_map(int op, int* out);
// host only: round r of the transposed read.  addr_out[lane] (64): the byte address each lane
// supplies; source_out[lane * 4 + q] (256): the 16-bit element index it receives.  0, or -1.
int amdgpu_ldspath_tr_map(int round, int* addr_out, int* source_out);
// host only: the 512 words form `form` holds after `steps` steps of 256 threads.  0, or -1.
int amdgpu_ldspath_atomic_expected(int form, int steps, unsigned int* out, int out_words);
// the text of stage `which` (0 widths, 1 atomic, 2 lane, 3 transpose; < 0: the first failing); 0 if it did not fail
int amdgpu_ldspath_describe(const amdgpu_ldspath_result* r, int which, char* buf, int len);
int amdgpu_ldspath_sizeof(int which);  // 0: record, 1: result
// table 0 lane ops, 1 atomic forms, 2 width passes, 3 the kind of each width pass.  index < 0:
// the count; else the name is written to buf and its length returned; -1: no such entry.
int amdgpu_ldspath_ops(int table, int index, char* buf, int len);

}  // extern "C"

static_assert(sizeof(amdgpu_ldspath_record) == 208, "ldspath.Record");
static_assert(sizeof(amdgpu_ldspath_result) == 1904, "ldspath.LdsPathResult");
