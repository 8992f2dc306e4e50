// MI355X (gfx950 / CDNA4) health canary: the block-scaled (MX-fp8 / bf8 / fp4) matrix path.
//
// C[MxN] (fp32) = dequant(A)[MxK] * dequant(Bt)[NxK]^T on v_mfma_scale_f32_32x32x64_f8f6f4, both
// operands K-contiguous and packed (one OCP code per byte; fp4 two per byte, the even k in the low
// nibble), one E8M0 scale byte per 32 k: sa [M][K/32], sb [N][K/32].  The path an MX inference
// kernel takes: packed rows HBM -> L2 -> LDS DMA -> swizzled ds_read_b128 -> scaled MFMA -> store
// of C, with the scale bytes fetched per K-tile.  Integer data makes every element exact, so the
// ABFT row / column checksums below verify the whole product without a tolerance.
//
// mx_gemm<FMT, TILE>, one template for both kernel ids:
//   * A K-tile is 128 B of every operand row, whatever the format: BK = 128 (fp8, bf8) or 256
//     (fp4).  The LDS image of an operand tile is [TILE][128 B], the geometry of the bf16 kernels
//     (ops/gemm.hip), with their swizzle: logical 16 B chunk c of row r sits at physical chunk
//     c ^ ((r >> 1) & 7), applied on the global source address because the DMA destination must
//     stay lane-linear.  Two buffers of A + B: 64 KiB (TILE 128), 128 KiB (TILE 256), one
//     __shared__ object.
//   * Movement: __builtin_amdgcn_global_load_lds, 16 B per lane; a wave issues 4 pieces (8 rows,
//     1 KiB) of A and 4 of B per K-tile.  Tile t+1 lands while tile t is multiplied;
//     s_waitcnt vmcnt(0) and a barrier close each K-tile.
//   * Fragments: lane l is r = l & 31, h = l >> 5.  Step s (64 k) of a K-tile reads, per owned
//     row, logical chunk 2s + h (fp4: the low four dwords of the operand, the high four zero) or
//     chunks 4s + h and 4s + 2 + h (fp8 / bf8: elements 0..15 and 16..31), whole ds_read_b128.
//   * Scales: straight into registers, not through LDS.  The bytes of one row for one K-tile are
//     contiguous and aligned in sa / sb (4 for the 8-bit formats, 8 for fp4), so each lane loads
//     one dword (or a dword pair) per owned row per K-tile and takes byte 2s + h with a shift:
//     byte 0 of the scale operand, op_sel 0.  The loads for tile t+1 are issued with its DMA, a
//     whole K-tile of MFMAs ahead of their use, and are retired by the same vmcnt(0).  Staging
//     them in LDS would need room beside the images (the 64 / 128 KiB are full), a second DMA
//     shape for 4-byte rows and one more LDS read per MFMA; the registers cost 2 x (MI + 2) x
//     (1 or 2) VGPRs, at most 24 of the 256 a wave has here.
//   * Work split: TILE 128 is 4 waves as 2x2, a wave 64x64 = 2x2 MFMA tiles (64 accumulators), two
//     workgroups per CU; TILE 256 is 8 waves as 2x4, a wave 128x64 = 4x2 tiles (128
//     accumulators), one workgroup per CU, plain double buffering.  Workgroups are remapped with
//     the bijective xcd_remap and tiles run row-major, so tiles that share A rows share an XCD's L2.
//
// C ABI for ctypes (k8s_gpu_device_plugin_amd/ops/mxgemm.py): mxgemm.h.
#include "mxgemm.h"

#include <cstdint>
#include <cstdio>

namespace {

using namespace canary;
using namespace mxgemm;

typedef __attribute__((address_space(3))) void* lds_void_ptr;

// gemm.hip's, which keeps them in an anonymous namespace
__host__ __device__ __forceinline__ int xcd_remap(int orig, int nwg) {  // bijective for any nwg
  const int xcd = orig % 8, q = nwg / 8, r = nwg % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}
__device__ __forceinline__ int swizzled_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// Logical 16 B chunk `chunk` of row `row` of an operand image: one ds_read_b128.
__device__ __forceinline__ u32x4 frag16(const char* S, int row, int chunk) {
  return *reinterpret_cast<const u32x4*>(S + row * kRowBytes + (swizzled_chunk(row, chunk) << 4));
}

// A lane's operand of step s from row `row` of image S.
template <int FMT>
__device__ __forceinline__ i32x8 operand(const char* S, int row, int s, int h) {
  if constexpr (FMT == kFp4) {
    const u32x4 lo = frag16(S, row, 2 * s + h);
    return i32x8{static_cast<int>(lo[0]), static_cast<int>(lo[1]), static_cast<int>(lo[2]), static_cast<int>(lo[3]), 0, 0, 0, 0};
  } else {
    const u32x4 lo = frag16(S, row, 4 * s + h), hi = frag16(S, row, 4 * s + 2 + h);
    return i32x8{static_cast<int>(lo[0]), static_cast<int>(lo[1]), static_cast<int>(lo[2]), static_cast<int>(lo[3]),
                 static_cast<int>(hi[0]), static_cast<int>(hi[1]), static_cast<int>(hi[2]), static_cast<int>(hi[3])};
  }
}

template <int FMT, int TILE>
__global__ void __launch_bounds__(2 * TILE) mx_gemm(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt,
                                                    const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sb,
                                                    float* __restrict__ C, int M, int N, int K) {
  constexpr int kBK = tile_k(FMT);           // k of a K-tile
  constexpr int kSteps = kBK / 64;           // MFMA steps per K-tile: 2 (fp8, bf8), 4 (fp4)
  constexpr int kWords = kBK / kScaleBlock / 4;  // dwords of scale bytes per row per K-tile: 1, 2
  constexpr int kOp = TILE * kRowBytes;      // one operand image
  constexpr int kStage = 2 * kOp;            // A + B of one K-tile
  constexpr int kAcross = TILE / 64;         // waves across N; 2 wave rows of TILE / 2
  constexpr int kMI = TILE / 64, kNJ = 2;    // a wave's MFMA tiles: kMI x 2
  __shared__ __attribute__((aligned(16))) char smem[2 * kStage];  // the only LDS object: [buf][A|B][TILE][128 B]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = xcd_remap(blockIdx.x, gridDim.x), nbn = N / TILE;
  const int m0 = (wg / nbn) * TILE, n0 = (wg % nbn) * TILE;
  if (m0 + TILE > M || n0 + TILE > N || K % kBK) return;  // host checks shapes; never touch memory past them
  const int wr = wave / kAcross, wc = wave % kAcross;
  const int r = lane & 31, h = lane >> 5;
  const size_t row_b = row_bytes(FMT, K);
  const int kblocks = K / kScaleBlock;

  // Wave w issues pieces 4w .. 4w+3 of A and of B (TILE / 8 pieces each, 2 TILE / 64 waves).
  auto stage = [&](int t, int buf) {
    char* base = smem + buf * kStage;
    const size_t k_b = static_cast<size_t>(t) * kRowBytes;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = wave * 4 + i, row = piece * 8 + (lane >> 3), cb = swizzled_chunk(row, lane & 7) << 4;
      __builtin_amdgcn_global_load_lds(A + static_cast<size_t>(m0 + row) * row_b + k_b + cb,
                                       (lds_void_ptr)(base + piece * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(Bt + static_cast<size_t>(n0 + row) * row_b + k_b + cb,
                                       (lds_void_ptr)(base + kOp + piece * 1024), 16, 0, 0);
    }
  };
  // The scale bytes of K-tile t of the lane's kMI rows of A and 2 columns of B.
  const uint8_t* sa_row = sa + static_cast<size_t>(m0 + wr * (TILE / 2) + r) * kblocks;
  const uint8_t* sb_row = sb + static_cast<size_t>(n0 + wc * 64 + r) * kblocks;
  uint32_t next_a[kMI][kWords], next_b[kNJ][kWords], cur_a[kMI][kWords], cur_b[kNJ][kWords];
  auto fetch_scales = [&](int t) {
    const size_t at = static_cast<size_t>(t) * (kBK / kScaleBlock);
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
#pragma unroll
      for (int i = 0; i < kMI; ++i)
        next_a[i][w] = *reinterpret_cast<const uint32_t*>(sa_row + static_cast<size_t>(i) * 32 * kblocks + at + 4 * w);
#pragma unroll
      for (int j = 0; j < kNJ; ++j)
        next_b[j][w] = *reinterpret_cast<const uint32_t*>(sb_row + static_cast<size_t>(j) * 32 * kblocks + at + 4 * w);
    }
  };

  f32x16 acc[kMI][kNJ];
#pragma unroll
  for (int i = 0; i < kMI; ++i)
#pragma unroll
    for (int j = 0; j < kNJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int T = K / kBK;
  stage(0, 0);
  fetch_scales(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
#pragma unroll
    for (int w = 0; w < kWords; ++w) {
#pragma unroll
      for (int i = 0; i < kMI; ++i) cur_a[i][w] = next_a[i][w];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) cur_b[j][w] = next_b[j][w];
    }
    if (t + 1 < T) {
      stage(t + 1, cur ^ 1);
      fetch_scales(t + 1);
    }
    const char* As = smem + cur * kStage;
    const char* Bs = As + kOp;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      // byte 2s + h of the tile's scale bytes: dword (2s + h) >> 2 = s >> 1, bit 8 ((2s + h) & 3) = 16 (s & 1) + 8 h
      const int word = s >> 1, shift = 16 * (s & 1) + 8 * h;
      i32x8 a[kMI], b[kNJ];
      int ka[kMI], kb[kNJ];
#pragma unroll
      for (int i = 0; i < kMI; ++i) {
        a[i] = operand<FMT>(As, wr * (TILE / 2) + i * 32 + r, s, h);
        ka[i] = static_cast<int>((cur_a[i][word] >> shift) & 0xffu);
      }
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        b[j] = operand<FMT>(Bs, wc * 64 + j * 32 + r, s, h);
        kb[j] = static_cast<int>((cur_b[j][word] >> shift) & 0xffu);
      }
#pragma unroll
      for (int i = 0; i < kMI; ++i)
#pragma unroll
        for (int j = 0; j < kNJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], FMT, FMT, 0, ka[i], 0, kb[j]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t+1 and its scale bytes have landed
    __syncthreads();                                   // ... and nobody still reads tile t's buffer
  }
#pragma unroll
  for (int i = 0; i < kMI; ++i)
#pragma unroll
    for (int j = 0; j < kNJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wr * (TILE / 2) + i * 32 + cd_row32(e, h);
        C[static_cast<size_t>(row) * N + n0 + wc * 64 + j * 32 + r] = acc[i][j][e];
      }
}

// ---- the check's data and its verifier --------------------------------------------------------
// Packed codes of integers in [-4, 4] and their scale bytes, from mxgemm_host.h's functions.
__global__ void __launch_bounds__(256) mx_fill(uint8_t* __restrict__ X, uint8_t* __restrict__ sc, int fmt, int which,
                                               int rows, int K, int vary) {
  const size_t row_b = row_bytes(fmt, K), n = static_cast<size_t>(rows) * row_b;
  const size_t kblocks = K / kScaleBlock, ns = static_cast<size_t>(rows) * kblocks;
  const size_t first = blockIdx.x * 256ull + threadIdx.x, step = static_cast<size_t>(gridDim.x) * 256;
  for (size_t e = first; e < n; e += step) X[e] = packed_byte(fmt, which, static_cast<int>(e / row_b), e % row_b, K);
  for (size_t e = first; e < ns; e += step)
    sc[e] = static_cast<uint8_t>(scale_byte(vary, which, static_cast<int>(e / kblocks), static_cast<int>(e % kblocks)));
}

// What element k of row `row` of a packed operand is worth: its integer times 2^(scale - 127).
__device__ __forceinline__ long long scaled_at(const uint8_t* __restrict__ X, const uint8_t* __restrict__ sc, int fmt,
                                               int row, int k, int K) {
  const int v = int_of_code(fmt, code_at(fmt, X + static_cast<size_t>(row) * row_bytes(fmt, K), k));
  return scaled(v, sc[static_cast<size_t>(row) * (K / kScaleBlock) + k / kScaleBlock]);
}

// colsum[k] += the scaled sum over a 64-row slab of X[row][k], as gemm.hip's gemm_colsum; out must be zeroed.
constexpr int kSlab = 64;
__global__ void __launch_bounds__(256) mx_colsum(const uint8_t* __restrict__ X, const uint8_t* __restrict__ sc, int fmt,
                                                 int rows, int K, long long* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int r0 = blockIdx.y * kSlab, r1 = r0 + kSlab < rows ? r0 + kSlab : rows;
  long long s = 0;
  for (int i = r0; i < r1; ++i) s += scaled_at(X, sc, fmt, i, k, K);
  atomicAdd(reinterpret_cast<unsigned long long*>(out + k), static_cast<unsigned long long>(s));
}

// gemm.hip's rule: an integer of magnitude <= 2^24, no NaN / Inf, no -0, decided on the bit pattern.
__device__ __forceinline__ bool abft_healthy(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  const uint32_t mag = u & 0x7fffffffu;
  if (mag == 0) return u == 0;
  if (mag < 0x3f800000u || mag > 0x4b800000u) return false;
  const int frac_bits = 150 - static_cast<int>(mag >> 23);
  return frac_bits <= 0 || (mag & ((1u << frac_bits) - 1u)) == 0;
}

// ABFT as gemm.hip's gemm_abft, on scaled values: one block per row (mode 0) or column (mode 1).
__global__ void __launch_bounds__(256) mx_abft(const uint8_t* __restrict__ X, const uint8_t* __restrict__ sc,
                                               const float* __restrict__ C, const long long* __restrict__ other_sum,
                                               int fmt, int M, int N, int K, int mode,
                                               unsigned long long* __restrict__ errors) {
  __shared__ long long red[3][256];
  const int idx = blockIdx.x, tid = threadIdx.x;
  long long expect = 0, got = 0, bad = 0;
  for (int k = tid; k < K; k += 256) expect += scaled_at(X, sc, fmt, idx, k, K) * other_sum[k];
  const int n_el = mode == 0 ? N : M;
  for (int e = tid; e < n_el; e += 256) {
    const float v = mode == 0 ? C[static_cast<size_t>(idx) * N + e] : C[static_cast<size_t>(e) * N + idx];
    if (abft_healthy(v))
      got += static_cast<long long>(v);
    else
      ++bad;
  }
  red[0][tid] = expect;
  red[1][tid] = got;
  red[2][tid] = bad;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0 && (red[0][0] != red[1][0] || red[2][0] != 0)) atomicAdd(errors + mode, 1ull);
}

// ---- the table: what a kernel id means ----------------------------------------------------------
using mx_fn = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, float*, int, int, int);
struct MxVariant {
  int tile, threads, lds_bytes;
  mx_fn fp8, bf8, fp4;
};
template <int TILE>
constexpr MxVariant tiled = {TILE, 2 * TILE, 4 * TILE * kRowBytes, mx_gemm<kFp8, TILE>, mx_gemm<kBf8, TILE>, mx_gemm<kFp4, TILE>};
constexpr MxVariant kMxVariants[] = {
    {},          // 0 is no kernel: pick_mx's own choice
    tiled<128>,  // 1 128x128 tiles, 4 waves, two workgroups per CU
    tiled<256>,  // 2 256x256 tiles, 8 waves, one workgroup per CU
};
constexpr int kMxVariantCount = sizeof(kMxVariants) / sizeof(kMxVariants[0]);
constexpr int kCus = 256;  // of an MI355X: the choice below wants a 256-tile for each

// `kernel` itself if its tiles divide the shape; for 0, id 2 when the shape divides into at least one
// 256-tile per CU, else id 1.  0 for a shape the kernel cannot take.
int pick_mx(int fmt, int kernel, int M, int N, int K) {
  if (kernel < 0 || kernel >= kMxVariantCount) return 0;
  const auto fits = [&](int id) { return shape_ok(fmt, kMxVariants[id].tile, M, N, K); };
  if (kernel != 0) return fits(kernel) ? kernel : 0;
  if (fits(2) && (M / 256) * (N / 256) >= kCus) return 2;
  return fits(1) ? 1 : 0;
}

void launch_mx(int fmt, int id, const uint8_t* a, const uint8_t* bt, const uint8_t* sa, const uint8_t* sb, float* c, int M,
               int N, int K) {
  const MxVariant& v = kMxVariants[id];
  const mx_fn kernel = fmt == kFp8 ? v.fp8 : fmt == kBf8 ? v.bf8 : v.fp4;
  hipLaunchKernelGGL(kernel, dim3((M / v.tile) * (N / v.tile)), dim3(v.threads), 0, 0, a, bt, sa, sb, c, M, N, K);
}

// The device side of one product: packed A and Bt, their scale bytes, C.
struct MxProduct {
  DeviceBuffer<uint8_t> a, b, sa, sb;
  DeviceBuffer<float> c;
  void alloc(Status& st, int device, int fmt, int M, int N, int K) {
    CANARY_HIP(st, hipSetDevice(device));
    CANARY_HIP(st, a.alloc(M * row_bytes(fmt, K)));
    CANARY_HIP(st, b.alloc(N * row_bytes(fmt, K)));
    CANARY_HIP(st, sa.alloc(static_cast<size_t>(M) * (K / kScaleBlock)));
    CANARY_HIP(st, sb.alloc(static_cast<size_t>(N) * (K / kScaleBlock)));
    CANARY_HIP(st, c.alloc(static_cast<size_t>(M) * N * 4));
  }
  void launch(int fmt, int id, int M, int N, int K) const {
    launch_mx(fmt, id, a.get(), b.get(), sa.get(), sb.get(), c.get(), M, N, K);
  }
};

}  // namespace

extern "C" {

int amdgpu_mxgemm_sizeof(int which) { return which == 0 ? static_cast<int>(sizeof(amdgpu_mxgemm_result)) : -1; }

int amdgpu_mxgemm_describe(const amdgpu_mxgemm_result* r, char* buf, int len) { return describe(*r, buf, len); }

int amdgpu_mxgemm_kernels(int id, int* out3) {
  if (id < 0) return kMxVariantCount;
  if (id >= kMxVariantCount || out3 == nullptr) return -1;
  out3[0] = kMxVariants[id].tile;
  out3[1] = kMxVariants[id].threads;
  out3[2] = kMxVariants[id].lds_bytes;
  return 0;
}

int amdgpu_mxgemm_pick(int fmt, int kernel, int M, int N, int K) { return pick_mx(fmt, kernel, M, N, K); }

int amdgpu_mxgemm_operand(int fmt, int which, int rows, int K, int vary_scale, unsigned char* codes, unsigned char* scales,
                          long long* values) {
  if (!format_ok(fmt) || which < 0 || which > 1 || rows <= 0 || K <= 0 || K % kScaleBlock) return -1;
  for (int row = 0; row < rows; ++row) {
    for (int k = 0; k < K; ++k) {
      const int v = value(which, row, k, K);
      if (codes) codes[static_cast<size_t>(row) * K + k] = static_cast<unsigned char>(code_of(fmt, v));
      if (values) values[static_cast<size_t>(row) * K + k] = v;
    }
    for (int kb = 0; scales && kb < K / kScaleBlock; ++kb)
      scales[static_cast<size_t>(row) * (K / kScaleBlock) + kb] = static_cast<unsigned char>(scale_byte(vary_scale, which, row, kb));
  }
  return 0;
}

int amdgpu_mxgemm_run(int device, int fmt, int kernel, const unsigned char* a, const unsigned char* bt,
                      const unsigned char* sa, const unsigned char* sb, float* c, int M, int N, int K, char* err,
                      int err_len) {
  const int id = pick_mx(fmt, kernel, M, N, K);
  if (id == 0) {
    shape_text(fmt, kernel, M, N, K, err, err_len);
    return -1;
  }
  Status st;
  MxProduct p;
  p.alloc(st, device, fmt, M, N, K);
  CANARY_HIP(st, p.a.upload(a));
  CANARY_HIP(st, p.b.upload(bt));
  CANARY_HIP(st, p.sa.upload(sa));
  CANARY_HIP(st, p.sb.upload(sb));
  if (st.ok()) {
    p.launch(fmt, id, M, N, K);
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, p.c.download(c));
  return st.report("mx matrix path: ", err, err_len);
}

int amdgpu_mxgemm_check(int device, int fmt, int kernel, int M, int N, int K, int iters, int vary_scale, int flags,
                        amdgpu_mxgemm_result* result, char* err, int err_len) {
  *result = amdgpu_mxgemm_result();
  const int id = pick_mx(fmt, kernel, M, N, K);
  if (id == 0 || iters < 1) {
    if (id == 0)
      shape_text(fmt, kernel, M, N, K, err, err_len);
    else
      std::snprintf(err, err_len, "mx matrix path: iters %d must be at least 1", iters);
    return -1;
  }
  Status st;
  MxProduct p;
  DeviceBuffer<long long> asum, bsum;
  DeviceBuffer<unsigned long long> d_counts;
  Events<2> ev;
  float ms[1] = {0};
  unsigned long long counts[2] = {0, 0};
  p.alloc(st, device, fmt, M, N, K);
  CANARY_HIP(st, asum.alloc(static_cast<size_t>(K) * 8));
  CANARY_HIP(st, bsum.alloc(static_cast<size_t>(K) * 8));
  CANARY_HIP(st, d_counts.alloc(sizeof(counts)));
  CANARY_HIP(st, asum.zero());
  CANARY_HIP(st, bsum.zero());
  CANARY_HIP(st, d_counts.zero());
  CANARY_HIP(st, ev.create());
  if (st.ok()) {
    hipLaunchKernelGGL(mx_fill, dim3(2048), dim3(256), 0, 0, p.a.get(), p.sa.get(), fmt, 0, M, K, vary_scale);
    hipLaunchKernelGGL(mx_fill, dim3(2048), dim3(256), 0, 0, p.b.get(), p.sb.get(), fmt, 1, N, K, vary_scale);
    p.launch(fmt, id, M, N, K);  // warm-up
    st.check(hipGetLastError());
  }
  time_stages(st, ev, ms, [&](int) {
    for (int i = 0; i < iters; ++i) p.launch(fmt, id, M, N, K);
    return hipSuccess;
  });
  CANARY_HIP(st, p.c.fill(0xFF));  // the poison: what is verified below was written after it
  if (st.ok() && !(flags & kMxSkipVerifiedLaunch)) {
    p.launch(fmt, id, M, N, K);
    st.check(hipGetLastError());
  }
  if (flags & kMxInject) {
    const float junk = 12345.0f;
    CANARY_HIP(st, hipMemcpy(p.c.get() + static_cast<size_t>(M / 2) * N + N / 3, &junk, 4, hipMemcpyHostToDevice));
  }
  if (st.ok()) {
    const int kb = (K + 255) / 256;
    hipLaunchKernelGGL(mx_colsum, dim3(kb, (M + kSlab - 1) / kSlab), dim3(256), 0, 0, p.a.get(), p.sa.get(), fmt, M, K, asum.get());
    hipLaunchKernelGGL(mx_colsum, dim3(kb, (N + kSlab - 1) / kSlab), dim3(256), 0, 0, p.b.get(), p.sb.get(), fmt, N, K, bsum.get());
    hipLaunchKernelGGL(mx_abft, dim3(M), dim3(256), 0, 0, p.a.get(), p.sa.get(), p.c.get(), bsum.get(), fmt, M, N, K, 0,
                       d_counts.get());
    hipLaunchKernelGGL(mx_abft, dim3(N), dim3(256), 0, 0, p.b.get(), p.sb.get(), p.c.get(), asum.get(), fmt, M, N, K, 1,
                       d_counts.get());
    st.check(hipGetLastError());
  }
  CANARY_HIP(st, hipDeviceSynchronize());
  CANARY_HIP(st, d_counts.download(counts));
  result->row_errors = counts[0];
  result->col_errors = counts[1];
  result->fmt = fmt;
  result->kernel = id;
  result->m = M;
  result->n = N;
  result->k = K;
  result->iters = iters;
  result->ms = ms[0];
  if (st.ok() && ms[0] > 0) result->tflops = 2.0 * M * N * K * iters / (ms[0] * 1e-3) / 1e12;
  return st.report("mx matrix path: ", err, err_len);
}

}  // extern "C"
