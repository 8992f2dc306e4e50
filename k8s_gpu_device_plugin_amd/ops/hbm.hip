// MI355X (gfx950 / CDNA4) health canary: the HBM pattern test.
//
// Every 16-byte word gets an address-derived pattern, written and read back with 16 B/lane
// vector accesses; mismatches are reduced per wave, then per block, one atomic per block
// (block_add_errors, canary_common.h).  The kernels are templates over the access shape: the
// canary runs the shape that the on-hardware sweep picked (hbm_write / hbm_verify below),
// amdgpu_canary_hbm_sweep times all 13 of them.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/canary.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canary_host.h"

namespace {

using namespace canary;

// Address-derived 16-byte pattern, ~5 integer ops per word so the verify pass stays
// HBM-bound: lo * odd constant is a bijection mod 2^32, so no two words of a <=64 GiB
// buffer share a pattern (aliasing / addressing faults are caught), and every data bit
// takes both values across the buffer (stuck-at faults are caught).
__device__ __forceinline__ uint4 pattern(uint64_t idx, uint32_t seed) {
  const uint32_t lo = static_cast<uint32_t>(idx), hi = static_cast<uint32_t>(idx >> 32);
  const uint32_t b = lo * 0x9E3779B1u ^ (hi + seed) * 0x85EBCA77u;
  return make_uint4(b, b ^ 0xA5A5A5A5u, ~b, b * 3u + 0x6A09E667u);
}

__device__ __forceinline__ uint32_t diff(const uint4& a, const uint4& b) {
  return (a.x != b.x) + (a.y != b.y) + (a.z != b.z) + (a.w != b.w);
}

// ---- HBM access-shape sweep (used to pick the canary's streaming shape on gfx950) ----
// UNROLL independent 16 B accesses in flight per lane; NT = non-temporal (streaming)
// loads/stores; CHUNKED = each block streams one contiguous chunk instead of a
// grid-stride walk.
__device__ __forceinline__ uint4 nt_load(const uint4* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store(const uint4& v, uint4* p) {
  const u32x4 x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(p));
}

template <int UNROLL, bool NT, bool CHUNKED>
__global__ void __launch_bounds__(256) sweep_write(uint4* __restrict__ buf, uint64_t n, uint32_t seed) {
  uint64_t begin, end, step;
  if (CHUNKED) {
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    begin = blockIdx.x * per + threadIdx.x;
    end = min<uint64_t>(n, (blockIdx.x + 1) * per);
    step = blockDim.x;
  } else {
    begin = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    end = n;
    step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  }
  uint64_t i = begin;
  for (; i + (UNROLL - 1) * step < end; i += UNROLL * step) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint4 v = pattern(i + u * step, seed);
      if (NT) nt_store(v, buf + i + u * step);
      else buf[i + u * step] = v;
    }
  }
  for (; i < end; i += step) buf[i] = pattern(i, seed);
}

template <int UNROLL, bool NT, bool CHUNKED>
__global__ void __launch_bounds__(256) sweep_verify(const uint4* __restrict__ buf, uint64_t n, uint32_t seed,
                                                    unsigned long long* __restrict__ errors) {
  uint64_t begin, end, step;
  if (CHUNKED) {
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    begin = blockIdx.x * per + threadIdx.x;
    end = min<uint64_t>(n, (blockIdx.x + 1) * per);
    step = blockDim.x;
  } else {
    begin = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    end = n;
    step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  }
  uint32_t bad = 0;
  uint64_t i = begin;
  for (; i + (UNROLL - 1) * step < end; i += UNROLL * step) {
    uint4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) v[u] = NT ? nt_load(buf + i + u * step) : buf[i + u * step];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) bad += diff(v[u], pattern(i + u * step, seed));
  }
  for (; i < end; i += step) bad += diff(buf[i], pattern(i, seed));
  block_add_errors(bad, errors);
}

// Tile-stride: block b streams tiles b, b + G, b + 2G, ... of 256 * UNROLL contiguous
// 16 B elements, so every wave reads whole contiguous runs (like CHUNKED) while the grid
// sweeps the buffer front to back together (like grid-stride): no per-block tail.
template <int UNROLL, bool NT>
__global__ void __launch_bounds__(256) tile_write(uint4* __restrict__ buf, uint64_t n, uint32_t seed) {
  const uint64_t tile = 256ull * UNROLL;
  for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += static_cast<uint64_t>(gridDim.x) * tile) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint64_t i = t0 + u * 256ull + threadIdx.x;
      if (i < n) {
        const uint4 v = pattern(i, seed);
        if (NT) nt_store(v, buf + i);
        else buf[i] = v;
      }
    }
  }
}

template <int UNROLL, bool NT>
__global__ void __launch_bounds__(256) tile_verify(const uint4* __restrict__ buf, uint64_t n, uint32_t seed,
                                                   unsigned long long* __restrict__ errors) {
  const uint64_t tile = 256ull * UNROLL;
  uint32_t bad = 0;
  for (uint64_t t0 = blockIdx.x * tile; t0 < n; t0 += static_cast<uint64_t>(gridDim.x) * tile) {
    if (t0 + tile <= n) {
      uint4 v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const uint64_t i = t0 + u * 256ull + threadIdx.x;
        v[u] = NT ? nt_load(buf + i) : buf[i];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) bad += diff(v[u], pattern(t0 + u * 256ull + threadIdx.x, seed));
    } else {
      for (uint64_t i = t0 + threadIdx.x; i < n; i += 256) bad += diff(buf[i], pattern(i, seed));
    }
  }
  block_add_errors(bad, errors);
}

// Shapes picked from the on-hardware sweep (profiles/hbm_sweep_gpu.json, 4 GiB buffer):
// writes: block-contiguous chunks, plain stores (~6.0 TB/s); verify: block-contiguous
// chunks, non-temporal loads (~6.8 TB/s), both at 16 blocks of 256 threads per CU.
// Re-swept at the canary's 1 GiB (profiles/r2/hbm_sweep_session4.json): behind plain
// stores the verify measures ~5.9 TB/s, since it also pays for the write-back of the lines
// the write phase left dirty in the caches; behind non-temporal stores it reads at 6.7 TB/s
// but the write drops to 5.6.  The write+verify pair takes the same time either way.
// Tile-stride (no per-block tail) was no faster than block-contiguous chunks.
constexpr int kBlocksPerCu = 16;
#define hbm_write sweep_write<4, false, true>
#define hbm_verify sweep_verify<4, true, true>

// One write launch and one verify launch of a shape, each timed: adds their ms to *t_write / *t_read.
template <auto Write, auto Verify>
void timed_pair(Status& st, const Events<3>& ev, uint4* buf, uint64_t n, int blocks, uint32_t seed,
                unsigned long long* d_errors, float* t_write, float* t_read) {
  float ms[2] = {0, 0};
  time_stages(st, ev, ms, [&](int k) {
    if (k == 0) hipLaunchKernelGGL(Write, dim3(blocks), dim3(256), 0, 0, buf, n, seed);
    else hipLaunchKernelGGL(Verify, dim3(blocks), dim3(256), 0, 0, buf, n, seed, d_errors);
    return hipSuccess;
  });
  *t_write += ms[0];
  *t_read += ms[1];
}

using pair_fn = decltype(&timed_pair<hbm_write, hbm_verify>);
template <int U, bool NT, bool CH>
constexpr pair_fn sweep_pair = timed_pair<sweep_write<U, NT, CH>, sweep_verify<U, NT, CH>>;
template <int U, bool NT>
constexpr pair_fn tile_pair = timed_pair<tile_write<U, false>, tile_verify<U, NT>>;  // NT: the verify only

// amdgpu_canary_hbm_sweep's variants, by index
constexpr pair_fn kSweepVariants[] = {
    sweep_pair<4, false, false>,   // 0 U4 grid-stride
    sweep_pair<8, false, false>,   // 1 U8 grid-stride
    sweep_pair<4, true, false>,    // 2 U4 NT
    sweep_pair<8, true, false>,    // 3 U8 NT
    sweep_pair<4, false, true>,    // 4 U4 chunked
    sweep_pair<8, false, true>,    // 5 U8 chunked
    sweep_pair<4, true, true>,     // 6 U4 NT chunked
    sweep_pair<16, false, false>,  // 7 U16 grid-stride
    sweep_pair<8, true, true>,     // 8 U8 NT chunked
    sweep_pair<2, true, true>,     // 9 U2 NT chunked
    tile_pair<4, true>,            // 10 U4 tile-stride (NT verify)
    tile_pair<8, true>,            // 11 U8 tile-stride (NT verify)
    tile_pair<8, false>,           // 12 U8 tile-stride
};

}  // namespace

void canary::hbm_passes(Status& st, const Events<3>& ev, const hipDeviceProp_t& prop, uint4* buf, uint64_t n,
                        int passes, unsigned long long* d_errors, float* t_write, float* t_read) {
  const int blocks = prop.multiProcessorCount * kBlocksPerCu;  // >> #CUs
  // warm-up (first-touch page mapping) outside the timed region
  st.stage("hbm_write: ");
  if (st.ok()) {
    hipLaunchKernelGGL(hbm_write, dim3(blocks), dim3(256), 0, 0, buf, n, 0x1234u);
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  st.stage("hbm_write + hbm_verify: ");
  for (int p = 0; p < passes; ++p)
    timed_pair<hbm_write, hbm_verify>(st, ev, buf, n, blocks, 0xA5A5u + p, d_errors, t_write, t_read);
  st.stage("");
}

extern "C" {

// Fault-injection self-check of the HBM verifier: writes the pattern, corrupts
// `flips` 4-byte words at spread-out offsets behind the kernel's back (hipMemcpy), and
// returns how many mismatching words the verify kernel reports (expected == flips).
long long amdgpu_canary_detects_corruption(int device, unsigned long long hbm_bytes, int flips) {
  const uint64_t n = hbm_bytes / sizeof(uint4);
  if (n == 0 || flips < 0) return -1;
  DeviceBuffer<uint4> buf;
  return count_errors(device, [&](Status& st, const hipDeviceProp_t& prop, unsigned long long* d_err) {
    const int blocks = prop.multiProcessorCount * kBlocksPerCu;
    if (!CANARY_HIP(st, buf.alloc(n * sizeof(uint4)))) return;
    hipLaunchKernelGGL(hbm_write, dim3(blocks), dim3(256), 0, 0, buf.get(), n, 77u);
    st.check(hipDeviceSynchronize());
    for (int f = 0; f < flips; ++f) {
      const uint64_t word = (static_cast<uint64_t>(f) * 2654435761ull) % n;
      const uint32_t junk = 0xDEADBEEFu ^ static_cast<uint32_t>(f);
      char* where = reinterpret_cast<char*>(buf.get() + word) + 4 * (f & 3);
      CANARY_HIP(st, hipMemcpy(where, &junk, 4, hipMemcpyHostToDevice));
    }
    if (st.ok()) hipLaunchKernelGGL(hbm_verify, dim3(blocks), dim3(256), 0, 0, buf.get(), n, 77u, d_err);
  });
}

// Write and read+verify rates of one access shape (kSweepVariants[variant]) over `bytes`,
// averaged over `reps` repetitions after a warm-up one.  blocks_per_cu scales the grid.
// -1: no such device, -2: no memory, -3: a HIP error while it ran.
int amdgpu_canary_hbm_sweep(int device, unsigned long long bytes, int variant, int blocks_per_cu, int reps,
                            double* write_gbps, double* read_gbps, unsigned long long* errors) {
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return -1;
  const uint64_t n = bytes / sizeof(uint4);
  DeviceBuffer<uint4> buf;
  DeviceBuffer<unsigned long long> err;
  if (buf.alloc(n * sizeof(uint4)) != hipSuccess || err.alloc(8) != hipSuccess || err.zero() != hipSuccess) return -2;
  const int blocks = prop.multiProcessorCount * (blocks_per_cu > 0 ? blocks_per_cu : 8);
  Status st;
  Events<3> ev;
  float tw = 0, tr = 0;
  CANARY_HIP(st, ev.create());
  if (variant >= 0 && variant < static_cast<int>(sizeof(kSweepVariants) / sizeof(kSweepVariants[0]))) {
    for (int r = 0; r < reps + 1; ++r) {  // first repetition is warm-up
      float w = 0, v = 0;
      kSweepVariants[variant](st, ev, buf.get(), n, blocks, 9u + r, err.get(), &w, &v);
      if (r) {  // the mean over the timed repetitions
        tw += w / reps;
        tr += v / reps;
      }
    }
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  (void)err.download(errors);
  *write_gbps = tw > 0 ? n * 16.0 / (tw * 1e-3) / 1e9 : 0;
  *read_gbps = tr > 0 ? n * 16.0 / (tr * 1e-3) / 1e9 : 0;
  return st.ok() ? 0 : -3;
}

}  // extern "C"
