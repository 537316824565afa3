// Shared plumbing for libdasac_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "chip.hpp"
#include "dasac_hip.h"

namespace dasac {

int fail(int code, const char* fmt, ...);   // records dasac_last_error(), returns code

// CUs this process leaves to kernels that run BESIDE its own (RCCL's all-reduce kernels under the overlapped data-parallel
// wrapper): 0 by default, a multiple of 8 (whole CUs per XCD); dasac_set_reserved_cus / DASAC_SK_RESERVE_CUS.  Sizes the
// persistent stream-K grid and the grid cap of the streaming kernels.
int reserved_cus();

inline hipStream_t as_stream(dasac_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

#define DASAC_REQUIRE(cond, ...)                                        \
  do {                                                                  \
    if (!(cond)) return ::dasac::fail(DASAC_EINVAL, __VA_ARGS__);       \
  } while (0)

#define DASAC_CHECK_LAUNCH(what)                                                          \
  do {                                                                                    \
    hipError_t e_ = hipGetLastError();                                                    \
    if (e_ != hipSuccess) return ::dasac::fail(DASAC_ELAUNCH, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

#define DASAC_HIP(call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return ::dasac::fail(DASAC_ELAUNCH, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// vectors aligned to their ELEMENT: the planes of a [B,C,H,W] tensor with an odd H*W (769 x 769) sit at every 4-byte phase, and
// global memory takes such a load or store at full width
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef long long i64x2u __attribute__((ext_vector_type(2), aligned(8)));

// a quad of one fp32 plane: nx = 1..4 pixels from p on, the slots past nx read as 0
__device__ __forceinline__ f32x4u load_quad(const float* __restrict__ p, int nx) {
  if (nx == 4) return *reinterpret_cast<const f32x4u*>(p);
  f32x4u v = f32x4u{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 3; ++e)
    if (e < nx) v[e] = p[e];
  return v;
}

// grid for a grid-stride streaming kernel: enough blocks to fill 256 CUs several times over
inline int stream_grid(int64_t work_items, int block, int max_blocks = 0) {
  if (max_blocks <= 0) max_blocks = (kNumCu - reserved_cus()) * 16;
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return static_cast<int>(g);
}

// ---- n / d for 0 <= n < 2^31 and a launch-constant d >= 1: one v_mul_hi_u32 + one shift instead of the ~30-instruction
// runtime division (the streaming kernels are issue-bound on exactly such index math: tools/isa_count.py).
// l = ceil(log2 d), mul = ceil(2^(31+l) / d) < 2^32, n / d = (n * mul) >> (31 + l)  (exact: 2^(31+l) <= mul*d <= 2^(31+l) + 2^l);
// d = 1 is flagged by mul = 0.
struct FastDiv {
  unsigned mul, shift;
};
inline FastDiv fast_div(int d) {
  if (d <= 1) return FastDiv{0u, 0u};
  int l = 1;
  while ((1ll << l) < d) ++l;
  const unsigned long long p = 1ull << (31 + l);
  return FastDiv{(unsigned)((p + (unsigned)d - 1) / (unsigned)d), (unsigned)(l - 1)};
}
__device__ __forceinline__ int fdiv(int n, FastDiv f) { return f.mul ? (int)(__umulhi((unsigned)n, f.mul) >> f.shift) : n; }

// ---- wave / block reductions (64-wide) ------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// The fixed-order sum over a 256-thread block: wave butterflies, lane 0 of each wave to LDS, (r0 + r1) + (r2 + r3).  Run-to-run
// determinism and every "bit for bit" test of the reductions rest on this order.  The sum is valid in EVERY thread after the call
// (a caller that uses it in thread 0 only leaves the LDS reads to that thread).  One call per kernel: the slots are not guarded
// against a second one.  The (s, q) pair form of the train-mode BatchNorm kernels and the one-column-per-thread form with max and
// min columns (tensor_stats_chunks, activation_stats_planes) keep the same order written out: on a shared helper each of them
// compiled to another instruction stream (profiles/pointwise_split.md).
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double r[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return (r[0] + r[1]) + (r[2] + r[3]);
}

}  // namespace dasac
