// C ABI of the matrix-forms check (ops/matforms/libamdgpu_matforms.so), mirrored with ctypes in
// ops/matforms.py.  The library is built apart from libamdgpu_canary.so and shares its
// header-only helpers (../canary_common.h, ../canary_host.h, ../site.h); the forms are in
// matforms_forms.h, the structs and the reduction in matforms_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "matforms_host.h"

extern "C" {

// Runs form_sweep of every form in the bit set `forms` on `device` and reduces the records.
// blocks == 0: 2 workgroups per CU plus up to 3 more launches (of every selected form) while a
// CU or SIMD has no located record of some form; blocks > 0: one launch of that many
// workgroups.  ksteps: MFMAs per check (1..8); vary_scale: the E8M0 scales of the scaled forms
// vary (2^0 / 2^1) or stay 2^0.  inject_form >= 0: lane 0 of the first inject_waves waves of the
// first launch perturbs element 0 of A in step 0 of that form.  rate_iters > 0: the rate chain
// of every selected form runs too, that many MFMAs per chain, and result->tflops is filled.
// wave_site_out (form f: wave_site_out[f * wave_site_len + wave], the starting site of the
// first wave_site_len waves of the first launch; all-ones where none ran) may be null.
// 0, or -1 with `err` set.
int amdgpu_matforms_run(int device, int blocks, int ksteps, int vary_scale, unsigned int forms, int inject_form,
                        int inject_waves, int rate_iters, unsigned int* wave_site_out, int wave_site_len,
                        amdgpu_matforms_result* result, char* err, int err_len);
// host only: the reduction on caller-supplied records; form_of[i] is the form record i belongs to.
int amdgpu_matforms_reduce(const amdgpu_matforms_record* recs, const int* form_of, int n, unsigned int forms,
                           amdgpu_matforms_result* result);
// n_waves single-wave MFMAs of form `form` on raw operand registers, zero accumulators in: wave w,
// lane l reads a_words / b_words[(w * 64 + l) * 8 ..] and the scale bytes scale_a / scale_b[w * 64 + l]
// (unscaled forms ignore them) and leaves its raw accumulators in out[(w * 64 + l) * 16 ..].
int amdgpu_matforms_raw(int device, int form, const unsigned int* a_words, const unsigned int* b_words,
                        const unsigned int* scale_a, const unsigned int* scale_b, unsigned int* out, int n_waves, char* err,
                        int err_len);
// host only: what a wave with key `key` feeds the MFMAs: step s, lane l at [(s * 64 + l) * 8 ..]
// of a_words / b_words and [s * 64 + l] of scale_a / scale_b.  0, or -1.
int amdgpu_matforms_operands(int form, unsigned int key, int ksteps, int vary_scale, int inject, unsigned int* a_words,
                             unsigned int* b_words, unsigned int* scale_a, unsigned int* scale_b);
// host only: the reference C[row * M + col] of that wave.  0, or -1.
int amdgpu_matforms_expected(int form, unsigned int key, int ksteps, int vary_scale, long long* out);
// host only: accumulators wave `wave` of the first launch gets wrong under the injection; -1: no such form
int amdgpu_matforms_inject_expected(int form, int wave);
// host only: the table's map.  a_k / b_k[lane * elems + j]: the k (in a step) of element j;
// cd_row[lane * acc + reg]: the row of accumulator reg; scale_block[lane]: the k-block (32 k) the
// lane's scale byte belongs to, -1 for an unscaled form.  Rows and columns are lane % M.  0, or -1.
int amdgpu_matforms_map(int form, int* a_k, int* b_k, int* cd_row, int* scale_block);
// the table: index < 0: the count; what 0 name, 1 text, 2 instruction into buf (returns the length);
// -1: no such entry
int amdgpu_matforms_forms(int index, int what, char* buf, int len);
// m, k, elems, r, acc_kind (0 f32, 1 i32, 2 f64), acc, scaled, bits_a, bits_b, map_a, map_b, key_offset
int amdgpu_matforms_form_ints(int index, unsigned int* out12);
// host only: the code of integer `value` (|value| <= r) in the format of operand `which` (0 A, 1 B);
// returns the element's bits, -1: no such form or value
int amdgpu_matforms_encode(int form, int which, int value, unsigned long long* code);
// the text of form `which` (< 0: the first failing); 0 if it did not fail
int amdgpu_matforms_describe(const amdgpu_matforms_result* r, int which, char* buf, int len);
int amdgpu_matforms_sizeof(int which);  // 0: record, 1: result

}  // extern "C"

static_assert(sizeof(amdgpu_matforms_record) == 80, "matforms.Record");
static_assert(sizeof(amdgpu_matforms_result) == 848, "matforms.MatFormsResult");
