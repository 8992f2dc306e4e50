// C ABI of the pace check (ops/pace/libamdgpu_pace.so), mirrored with ctypes in ops/pace.py.
// The library is built apart from libamdgpu_canary.so and shares its header-only helpers
// (../canary_common.h, ../canary_host.h, ../site.h); the structs and the reduction are
// in pace_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../canary_host.h"
#include "pace_host.h"

extern "C" {

// inject_kind of amdgpu_pace_run
constexpr int kPaceInjectSlowXcc = 0, kPaceInjectSlowWaves = 1, kPaceInjectResult = 2;

// Runs both stages on `device` and reduces their records.  blocks == 0: pace_mfma as 2
// workgroups per CU plus up to 3 more launches while a CU or SIMD has no located record, and
// pace_mem as one workgroup per CU; blocks > 0: one launch of that many workgroups each.
// iters: iterations of four MFMAs per wave (1..65535, the injected factor included);
// slice_kb: KiB each pace_mem workgroup streams (a multiple of 4).  inject_kind -1 none,
// 0 slow_xcc (every wave on inject_xcc does inject_factor times the work it records),
// 1 slow_waves (the first inject_waves waves of the first pace_mfma launch do), 2 result (lane
// 3 of the first inject_waves waves perturbs one operand of the last MFMA).
// sites_out (kPaceSiteSlots), xccs_out (kPaceXccs), wave_site_out (2 * wave_site_len entries:
// the starting site of the first wave_site_len waves of the first pace_mfma launch, then of
// pace_mem; all-ones where none ran) may be null.  0, or -1 with `err` set.
int amdgpu_pace_run(int device, int blocks, int iters, int slice_kb, double slow_ratio, int inject_kind, int inject_xcc,
                    int inject_factor, int inject_waves, amdgpu_pace_site_slot* sites_out,
                    amdgpu_pace_xcc_slot* xccs_out, unsigned int* wave_site_out, int wave_site_len,
                    amdgpu_pace_result* result, char* err, int err_len);
// host only: the reduction on caller-supplied records (mfma: n_mfma, mem: n_mem = 4 per
// workgroup; either may be empty).  0, or -1 on a bad argument.
int amdgpu_pace_reduce(const amdgpu_pace_record* mfma, int n_mfma, const amdgpu_pace_record* mem, int n_mem,
                       double tick_mhz, double clock_max_mhz, double slow_ratio, amdgpu_pace_site_slot* sites_out,
                       amdgpu_pace_xcc_slot* xccs_out, amdgpu_pace_result* result);
// "pace check: 3 wrong results at xcc3/se1/sh0/cu7/simd2 (+1 more site)"; 0 if nothing failed
int amdgpu_pace_describe(const amdgpu_pace_result* r, const amdgpu_pace_xcc_slot* xccs, char* buf, int len);
// "pace: xcc5 ran 1210 MHz beside a median of 2105 (ratio 0.57)"; 0 if nothing was slow
int amdgpu_pace_note(const amdgpu_pace_result* r, const amdgpu_pace_xcc_slot* xccs, const amdgpu_pace_site_slot* sites,
                     char* buf, int len);
int amdgpu_pace_sizeof(int which);  // 0: record, 1: site slot, 2: xcc slot, 3: result
int amdgpu_pace_default_iters();

}  // extern "C"

static_assert(sizeof(amdgpu_pace_record) == 32, "pace.Record");
static_assert(sizeof(amdgpu_pace_site_slot) == 24, "pace.SiteSlot");
static_assert(sizeof(amdgpu_pace_xcc_slot) == 48, "pace.XccSlot");
static_assert(sizeof(amdgpu_pace_result) == 400, "pace.PaceResult");
