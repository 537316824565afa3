// What the head's kernel files share (upsample.hip, cross_entropy.hip, warp.hip): the block size and class limit of the streaming
// kernels, the scalar-base + lane-offset addressing, the quad helpers, and the one launch cross_entropy.hip borrows from upsample.hip.
#pragma once
#include "bilinear.hpp"
#include "common.hpp"

#include <type_traits>

namespace dasac {

constexpr int kMaxC = 32;   // classes held in registers
constexpr int kHB = 256;

// scalar base + 32-bit per-lane byte offset: the form the global_load / global_store saddr encoding takes without any VALU
__device__ __forceinline__ float ld_off(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ float* at_off(float* base, unsigned byte_off) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off);
}

// a quad of one fp32 plane out: nx = 1..4 pixels from o on (a dwordx4 store, or the last 1..3 pixels of a row or plane one by one)
__device__ __forceinline__ void store_quad(float* o, f32x4u v, int nx) {
  if (nx == 4) {
    *reinterpret_cast<f32x4u*>(o) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (e < nx) o[e] = v[e];
  }
}

// the class count a launcher compiles in: 19 (Cityscapes), or kMaxC for the generic (runtime-C) instantiation.  f(integral_constant)
template <class F>
inline void dispatch_classes(int C, F f) {
  if (C == 19) f(std::integral_constant<int, 19>{}); else f(std::integral_constant<int, kMaxC>{});
}

// grid.x per image of a kernel that walks `items` items of each of B images in blocks of kHB: enough for 16 blocks per CU in all
inline int blocks_per_image(int64_t items, int B) { return stream_grid(items, kHB, (kNumCu * 16 + B - 1) / B); }

// upsample.hip's vertical transpose pass d[plane][i][j] = gscale * sum_y wy(y->i) * tmp[plane][y][j] over `planes` planes (the
// library is not relocatable device code: a kernel is launched from the file that defines it).  DASAC_OK or the launch error.
int launch_upsample_bwd_y(const float* tmp, int64_t planes, int H, int h, int w, const float* gscale, float* d, hipStream_t s);

}  // namespace dasac
