// MI355X (gfx950 / CDNA4) health canary: the matrix-forms check.
//
// The matrix cores on the instruction forms the canary's own three do not touch: f16, i8, f32,
// f64, fp6, the mixed MX formats and the 16x16 shapes (matforms_forms.h).  The shape is the site
// probe's: 4-wave workgroups (one wave per SIMD), one resident per CU through the largest
// dynamic LDS allocation, every wave reading its site (canary_common.h) first and last, and
// lane 0 of every wave leaving one record (matforms_host.h) in its own slot,
// records[block * 4 + wave], with ordinary vector stores.  No kernel reads a record, no
// workgroup waits for another, every loop is bounded by an argument or a constant, and fault
// injection perturbs a value that is then compared, never an address.  The verdicts are the
// host's (matforms_host.h).
//
//   * form_sweep<F>: the exactness check of form F, one kernel per form (so none spills);
//   * raw_mfma<F>:   single-wave MFMAs on the caller's raw operand registers (the map probe);
//   * form_rate<F>: register-resident operands, independent accumulator chains (reported only).
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/matforms.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "matforms.h"

namespace {

using namespace canary;
namespace mf = matforms;

constexpr int kThreads = kMatFormsWaves * kWave;

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, kWave);
    v = o < v ? o : v;
  }
  return v;
}

// Waves with global index < inject_waves perturb element 0 of A of lane 0 in step 0.
// The dynamic LDS allocation is not used: its size keeps one workgroup per CU.
template <class F>
__global__ void __launch_bounds__(kThreads) form_sweep(int form, int ksteps, int vary_scale, int inject_waves, uint32_t seed,
                                                       amdgpu_matforms_record* __restrict__ records,
                                                       unsigned int* __restrict__ wave_site, int wave_site_len) {
  const uint32_t site = site_id();
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kMatFormsWaves + (threadIdx.x >> 6);  // < 2^14 (host-checked)
  const uint32_t key = gw | (seed << 14);
  uint32_t first_reg = kMatFormsNone;
  const uint32_t bad = wave_total(mf::form_check<F>(key, lane, ksteps, vary_scale, static_cast<int>(gw) < inject_waves, first_reg));
  first_reg = wave_min(first_reg);
  const uint32_t site_after = site_id();
  if (lane != 0) return;
  if (wave_site != nullptr && static_cast<int>(gw) < wave_site_len) wave_site[gw] = site;
  amdgpu_matforms_record* rec = records + gw;
  rec->site_first = site;
  rec->site_last = site_after;
  rec->first_form = bad ? static_cast<uint32_t>(form) : kMatFormsNone;
  rec->first_reg = first_reg;
#pragma unroll
  for (int f = 0; f < kMatFormsMax; ++f) rec->bad[f] = f == form ? bad : 0u;
}

// One MFMA of form F per wave on raw registers; waves at or past n_waves do nothing.
template <class F>
__global__ void __launch_bounds__(kThreads) raw_mfma(const uint32_t* __restrict__ a_words, const uint32_t* __restrict__ b_words,
                                                     const uint32_t* __restrict__ scale_a, const uint32_t* __restrict__ scale_b,
                                                     uint32_t* __restrict__ out, int n_waves) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t gw = blockIdx.x * kMatFormsWaves + (threadIdx.x >> 6);
  if (static_cast<int>(gw) >= n_waves) return;  // the whole wave
  const size_t idx = static_cast<size_t>(gw) * kWave + lane;
  typename F::operand_a a;
  typename F::operand_b b;
#pragma unroll
  for (int i = 0; i < F::kWordsA; ++i) a.w[i] = a_words[idx * mf::kOperandWords + i];
#pragma unroll
  for (int i = 0; i < F::kWordsB; ++i) b.w[i] = b_words[idx * mf::kOperandWords + i];
  typename F::acc_t acc;
#pragma unroll
  for (int i = 0; i < F::kAcc; ++i) acc[i] = 0;
  acc = F::mfma(a, b, acc, static_cast<int>(scale_a[idx]), static_cast<int>(scale_b[idx]));
  constexpr int words = sizeof(typename F::acc_t) / 4;
  struct Raw {
    uint32_t w[words];
  };
  const Raw raw = __builtin_bit_cast(Raw, acc);
#pragma unroll
  for (int i = 0; i < mf::kAccWords; ++i) out[idx * mf::kAccWords + i] = i < words ? raw.w[i] : 0u;
}

// The rate chain of form F: register-resident operands, kChains independent accumulator chains
// per wave (the 16x16 forms issue faster than their result returns: four; the 32x32 forms: two).
template <class F>
constexpr int kChains = F::kAcc == 16 ? 2 : 4;
template <class F>
__global__ void __launch_bounds__(kRateThreads) form_rate(int iters, float* __restrict__ sink) {
  const int lane = threadIdx.x & (kWave - 1);
  typename F::operand_a a = {};
  typename F::operand_b b = {};
#pragma unroll
  for (int j = 0; j < F::kElems; ++j) {
    F::set_a(a, j, ((lane + j) % 5) - 2);
    F::set_b(b, j, ((lane * 3 + j) % 7) - 3);
  }
  typename F::acc_t acc[kChains<F>];
#pragma unroll
  for (int c = 0; c < kChains<F>; ++c)
#pragma unroll
    for (int i = 0; i < F::kAcc; ++i) acc[c][i] = 0;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < kChains<F>; ++c) acc[c] = F::mfma(a, b, acc[c], 127, 127);
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kChains<F>; ++c)
#pragma unroll
    for (int i = 0; i < F::kAcc; ++i) s += static_cast<float>(acc[c][i]);
  if (s == 1234.5f) sink[blockIdx.x * blockDim.x + threadIdx.x] = s;  // keeps the chains live
}

void bad_arguments(char* err, int err_len, int blocks, int ksteps, int vary_scale, unsigned int forms, int inject_form,
                   int inject_waves) {
  std::snprintf(err, err_len,
                "matrix form check: bad arguments (blocks %d in 0..%d, ksteps %d in 1..%d, vary_scale %d in 0..1, forms 0x%x "
                "within 0x%x and not empty, inject %d/%d with a selected form below %d)",
                blocks, mf::kMaxBlocks, ksteps, mf::kMaxKsteps, vary_scale, forms, mf::kAllForms, inject_form, inject_waves,
                mf::kNumForms);
}

}  // namespace

extern "C" {

int amdgpu_matforms_sizeof(int which) {
  return which == 0 ? static_cast<int>(sizeof(amdgpu_matforms_record)) : which == 1 ? static_cast<int>(sizeof(amdgpu_matforms_result)) : -1;
}

int amdgpu_matforms_forms(int index, int what, char* buf, int len) {
  if (index < 0) return mf::kNumForms;
  if (index >= mf::kNumForms || what < 0 || what > 2) return -1;
  const mf::FormInfo& f = mf::kForms[index];
  const char* text = what == 0 ? f.name : what == 1 ? f.text : f.instruction;
  return buf != nullptr && len > 0 ? std::snprintf(buf, len, "%s", text) : static_cast<int>(std::strlen(text));
}

int amdgpu_matforms_form_ints(int index, unsigned int* out) {
  if (index < 0 || index >= mf::kNumForms || out == nullptr) return -1;
  const mf::FormInfo& f = mf::kForms[index];
  const int v[11] = {f.m, f.k, f.elems, f.r, f.acc_kind, f.acc, f.scaled, f.bits_a, f.bits_b, f.map_a, f.map_b};
  for (int i = 0; i < 11; ++i) out[i] = static_cast<unsigned int>(v[i]);
  out[11] = f.key_offset;
  return 0;
}

int amdgpu_matforms_encode(int form, int which, int value, unsigned long long* code) {
  int bits = -1;
  if (code == nullptr || which < 0 || which > 1) return -1;
  mf::with_form(form, [&](auto f) {
    using F = decltype(f);
    if (value < -F::kR || value > F::kR) return;
    *code = which == 0 ? F::EA::code(value) : F::EB::code(value);
    bits = which == 0 ? F::EA::kBits : F::EB::kBits;
  });
  return bits;
}

int amdgpu_matforms_operands(int form, unsigned int key, int ksteps, int vary_scale, int inject, unsigned int* a_words,
                             unsigned int* b_words, unsigned int* scale_a, unsigned int* scale_b) {
  if (ksteps < 1 || ksteps > mf::kMaxKsteps || !a_words || !b_words || !scale_a || !scale_b) return -1;
  const bool known = mf::with_form(form, [&](auto f) {
    using F = decltype(f);
    for (int s = 0; s < ksteps; ++s)
      for (int lane = 0; lane < kWave; ++lane) {
        typename F::operand_a a;
        typename F::operand_b b;
        int sa, sb;
        mf::form_operands<F>(key, lane, s, vary_scale, inject != 0, a, b, sa, sb);
        const size_t idx = static_cast<size_t>(s) * kWave + lane;
        for (int i = 0; i < mf::kOperandWords; ++i) {
          a_words[idx * mf::kOperandWords + i] = i < F::kWordsA ? a.w[i] : 0u;
          b_words[idx * mf::kOperandWords + i] = i < F::kWordsB ? b.w[i] : 0u;
        }
        scale_a[idx] = static_cast<unsigned int>(sa);
        scale_b[idx] = static_cast<unsigned int>(sb);
      }
  });
  return known ? 0 : -1;
}

int amdgpu_matforms_expected(int form, unsigned int key, int ksteps, int vary_scale, long long* out) {
  if (ksteps < 1 || ksteps > mf::kMaxKsteps || out == nullptr) return -1;
  const bool known = mf::with_form(form, [&](auto f) {
    using F = decltype(f);
    for (int row = 0; row < F::kM; ++row)
      for (int col = 0; col < F::kM; ++col) out[row * F::kM + col] = mf::form_ref<F>(key, row, col, ksteps, vary_scale);
  });
  return known ? 0 : -1;
}

int amdgpu_matforms_inject_expected(int form, int wave) {
  int n = -1;
  if (wave < 0) return -1;
  mf::with_form(form, [&](auto f) { n = mf::inject_expected<decltype(f)>(static_cast<uint32_t>(wave)); });
  return n;
}

int amdgpu_matforms_map(int form, int* a_k, int* b_k, int* cd_row, int* scale_block) {
  if (!a_k || !b_k || !cd_row || !scale_block) return -1;
  const bool known = mf::with_form(form, [&](auto f) {
    using F = decltype(f);
    for (int lane = 0; lane < kWave; ++lane) {
      const int g = lane / F::kM;
      for (int j = 0; j < F::kElems; ++j) {
        a_k[lane * F::kElems + j] = F::k_of_a(g, j);
        b_k[lane * F::kElems + j] = F::k_of_b(g, j);
      }
      for (int reg = 0; reg < F::kAcc; ++reg) cd_row[lane * F::kAcc + reg] = F::cd_row(reg, g);
      scale_block[lane] = F::kScaled ? g : -1;
    }
  });
  return known ? 0 : -1;
}

int amdgpu_matforms_reduce(const amdgpu_matforms_record* recs, const int* form_of, int n, unsigned int forms,
                           amdgpu_matforms_result* result) {
  if (result == nullptr) return -1;
  std::memset(result, 0, sizeof(*result));
  return mf::reduce(recs, form_of, n, forms, result) ? 0 : -1;
}

int amdgpu_matforms_describe(const amdgpu_matforms_result* r, int which, char* buf, int len) {
  return mf::describe(*r, which, buf, len);
}

int amdgpu_matforms_raw(int device, int form, const unsigned int* a_words, const unsigned int* b_words,
                        const unsigned int* scale_a, const unsigned int* scale_b, unsigned int* out, int n_waves, char* err,
                        int err_len) {
  if (form < 0 || form >= mf::kNumForms || !a_words || !b_words || !scale_a || !scale_b || !out || n_waves < 1 ||
      n_waves > (1 << 20)) {
    std::snprintf(err, err_len, "matrix form check: bad arguments (raw: form %d below %d, waves %d in 1..%d)", form,
                  mf::kNumForms, n_waves, 1 << 20);
    return -1;
  }
  const size_t lanes = static_cast<size_t>(n_waves) * kWave;
  Status st;
  DeviceBuffer<uint32_t> d_a, d_b, d_sa, d_sb, d_out;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, d_a.alloc(lanes * mf::kOperandWords * 4));
  CANARY_HIP(st, d_b.alloc(lanes * mf::kOperandWords * 4));
  CANARY_HIP(st, d_sa.alloc(lanes * 4));
  CANARY_HIP(st, d_sb.alloc(lanes * 4));
  CANARY_HIP(st, d_out.alloc(lanes * mf::kAccWords * 4));
  CANARY_HIP(st, d_a.upload(a_words));
  CANARY_HIP(st, d_b.upload(b_words));
  CANARY_HIP(st, d_sa.upload(scale_a));
  CANARY_HIP(st, d_sb.upload(scale_b));
  CANARY_HIP(st, d_out.zero());
  st.stage("raw_mfma: ");
  if (st.ok()) {
    const int grid = (n_waves + kMatFormsWaves - 1) / kMatFormsWaves;
    mf::with_form(form, [&](auto f) {
      hipLaunchKernelGGL(raw_mfma<decltype(f)>, dim3(grid), dim3(kThreads), 0, 0, d_a.get(), d_b.get(), d_sa.get(), d_sb.get(),
                         d_out.get(), n_waves);
    });
    CANARY_HIP(st, hipGetLastError());
    CANARY_HIP(st, hipDeviceSynchronize());
  }
  CANARY_HIP(st, d_out.download(out));
  return st.report("matrix form check: ", err, err_len);
}

int amdgpu_matforms_run(int device, int blocks, int ksteps, int vary_scale, unsigned int forms, int inject_form,
                        int inject_waves, int rate_iters, unsigned int* wave_site_out, int wave_site_len,
                        amdgpu_matforms_result* out, char* err, int err_len) {
  std::memset(out, 0, sizeof(*out));
  if (!mf::arguments_ok(blocks, ksteps, vary_scale, forms, inject_form, inject_waves, wave_site_len, wave_site_out != nullptr) ||
      rate_iters < 0 || rate_iters > (1 << 20)) {
    bad_arguments(err, err_len, blocks, ksteps, vary_scale, forms, inject_form, inject_waves);
    return -1;
  }
  Status st;
  hipDeviceProp_t prop;
  CANARY_HIP(st, hipSetDevice(device));
  CANARY_HIP(st, hipGetDeviceProperties(&prop, device));
  if (!st.ok()) return st.report("matrix form check: ", err, err_len);
  const LaunchPlan plan = launch_plan(blocks, prop.multiProcessorCount, 2, true);
  const int grid = plan.grid;
  const size_t slots = static_cast<size_t>(grid) * kMatFormsWaves;
  out->cus_expected = prop.multiProcessorCount;
  out->blocks = grid;
  out->ksteps = ksteps;
  out->vary_scale = vary_scale;

  DeviceBuffer<amdgpu_matforms_record> d_records;  // the forms' slots, one form after another
  DeviceBuffer<unsigned int> d_wave_site;
  Events<mf::kNumForms + 1> ev;
  CANARY_HIP(st, d_records.alloc(sizeof(amdgpu_matforms_record) * slots * mf::kNumForms));
  if (wave_site_len > 0) {
    CANARY_HIP(st, d_wave_site.alloc(sizeof(unsigned int) * mf::kNumForms * wave_site_len));
    CANARY_HIP(st, d_wave_site.fill(0xFF));
  }
  CANARY_HIP(st, ev.create());

  std::vector<amdgpu_matforms_record> h;
  std::vector<int> form_of;
  for (int l = 0; l < plan.max_launches && st.ok(); ++l) {
    float ms[mf::kNumForms] = {};
    CANARY_HIP(st, d_records.fill(0xFF));
    st.stage("form_sweep: ");
    time_stages(st, ev, ms, [&](int k) {
      if (!((forms >> k) & 1u)) return hipSuccess;
      size_t got = 0;
      mf::with_form(k, [&](auto f) {
        got = launch_with_max_lds(form_sweep<decltype(f)>, prop, dim3(grid), dim3(kThreads), k, ksteps, vary_scale,
                                  l == 0 && k == inject_form ? inject_waves : 0, static_cast<uint32_t>(l),
                                  d_records.get() + slots * k,
                                  l == 0 && wave_site_len > 0 ? d_wave_site.get() + static_cast<size_t>(k) * wave_site_len : nullptr,
                                  l == 0 ? wave_site_len : 0);
      });
      return got ? hipSuccess : hipErrorLaunchFailure;
    });
    for (int k = 0; k < mf::kNumForms && st.ok(); ++k) {
      if (!((forms >> k) & 1u)) continue;
      const size_t have = h.size();
      h.resize(have + slots);
      form_of.resize(have + slots, k);
      CANARY_HIP(st, hipMemcpy(h.data() + have, d_records.get() + slots * k, sizeof(amdgpu_matforms_record) * slots,
                               hipMemcpyDeviceToHost));
      out->form_ms[k] += ms[k];
      out->ms += ms[k];
    }
    if (!st.ok()) break;
    out->launches = l + 1;
    if (!mf::reduce(h.data(), form_of.data(), static_cast<int>(h.size()), forms, out)) {
      std::snprintf(err, err_len, "matrix form check: a record holds a site out of range");
      return -1;
    }
    if (covered(*out, out->cus_expected)) break;
  }
  if (wave_site_len > 0) CANARY_HIP(st, d_wave_site.download(wave_site_out));

  if (rate_iters > 0 && st.ok()) {
    const int rblocks = rate_blocks(prop);
    DeviceBuffer<float> d_sink;
    Events<2> rev;
    CANARY_HIP(st, alloc_rate_sink(d_sink, rblocks));
    CANARY_HIP(st, rev.create());
    st.stage("form_rate: ");
    for (int k = 0; k < mf::kNumForms && st.ok(); ++k) {
      if (!((forms >> k) & 1u)) continue;
      mf::with_form(k, [&](auto f) {
        using F = decltype(f);
        const float ms = time_rate_launch(st, rev, form_rate<F>, rblocks, rate_iters, d_sink.get());
        const double flops = 2.0 * F::kM * F::kM * F::kK * kChains<F> * rate_iters * (static_cast<double>(rblocks) * (kRateThreads / kWave));
        out->tflops[k] = ms > 0 ? flops / (ms * 1e-3) / 1e12 : 0;
      });
    }
  }
  return st.report("matrix form check: ", err, err_len);
}

}  // extern "C"
