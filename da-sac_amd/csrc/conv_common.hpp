// What the convolution files share (conv_gemm.hip, conv_wgrad.hip, conv_pack.hip, winograd.hip): vector types, tile constants,
// the geometry both GEMM kernels take, buffer-descriptor loads, the split-bf16 operand helpers and the host's geometry checks.
// The integer rules -- padding, tiles, schedules, splits, the block maps -- are conv_plan.hpp's.
#pragma once
#include "common.hpp"
#include "conv_plan.hpp"

namespace dasac {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;      // 4 waves
constexpr int kInvalid = 1 << 20;  // dh of a padded table row: never in bounds

struct GemmGeom {
  // gathered tensor X [Nb, Cx, H, W]
  int H, W, CxHW;                // CxHW = Cx*H*W (image stride)
  // pixel grid of the GEMM's N dimension: Nb x OH x OW, gather coordinate = o*stride + d
  int OH, OW, stride;
  int Npix;                      // Nb*OH*OW
  int n_tile0;                   // first pixel tile of this launch (a conv may be issued as several launches over pixel ranges)
  int M, Mpad, Kpad;
  // output tensor [Nb, M, OutH, OutW]; element (oh*ostride, ow*ostride)
  int OutH, OutW, ostride;
  unsigned x_bytes, w_bytes, z_bytes, out_bytes;  // buffer-descriptor extents (gathered tensor, packed weights, dZ, output): < 4 GiB
};

// Buffer addressing.  Every global read of the GEMM loops goes through a raw buffer descriptor:
//   address = base + voffset (VGPR) + soffset (SGPR);  reads past num_records return 0.
// That turns the zero padding of the convolution into an ADDRESS decision (out-of-image taps get the
// poison offset 2^31 >= num_records) and moves the per-row part of the address (channel plane, K-step
// of the weights) into the scalar operand -- the vector ALU, which shares issue bandwidth with the
// matrix pipe (measured: ~6 matrix-pipe cycles lost per VALU instruction), stays almost idle.
// Offsets are UNSIGNED 32-bit byte offsets: a tensor may be up to 4 GiB - 4 KiB (round 5; rounds 1-4 kept them below 2^31 and
// used 2^31 as the poison).  The poison is the largest offset: always >= num_records, whatever scalar offset is added (the
// hardware compares the per-lane offset with num_records - soffset), and never combined with an instruction immediate.
constexpr unsigned kPoison = 0xFFFFFFFFu;
constexpr int kRsrcFlags = 0x00020000;   // raw buffer, 32-bit data format (gfx9 family word 3)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, kRsrcFlags);
}
__device__ __forceinline__ float buf_f32(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// agent-scope (sc1) 16-byte accesses for data handed from one workgroup to another inside a launch: an sc1 store is
// written through to memory, an sc1 load does not hit a stale line of this XCD's L2 / this CU's L1 -- the per-XCD L2s
// are not coherent with each other (MI355X_MICROARCH.md, inter-workgroup visibility).  With both sides sc1 the hand-off
// needs no buffer_wbl2 / buffer_inv fences (1.7-6.5 us each), only the flag's own release/acquire ordering.
constexpr int kAuxSc1 = 16;
__device__ __forceinline__ f32x4 buf_f32x4_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, kAuxSc1);
  return f32x4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
}
__device__ __forceinline__ f32x4 buf_f32x4(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  return f32x4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
}

// Split-bf16 ("bf16x3") operands: x = head + tail with head = bf16(x) (round to nearest even) and
// tail = bf16(x - head); eight consecutive k values of one row / pixel make one 16-byte MFMA operand.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16x8 as_bf16x8(f32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {          // v_cvt_pk_bf16_f32, a in the low half
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ __forceinline__ void split_bf16(f32x4 v0, f32x4 v1, f32x4& heads, f32x4& tails) {
  const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned h = pack_bf16(v[2 * p], v[2 * p + 1]);
    const float t0 = v[2 * p] - __uint_as_float(h << 16), t1 = v[2 * p + 1] - __uint_as_float(h & 0xffff0000u);   // exact
    heads[p] = __uint_as_float(h);
    tails[p] = __uint_as_float(pack_bf16(t0, t1));
  }
}

// ---- host: geometry of a launch, checked once ----
inline int fill_geom(GemmGeom& g, int Nb, int Cx, int H, int W, int OH, int OW, int stride, int M, int Mpad, int Kpad,
                     int OutH, int OutW, int ostride) {
  DASAC_REQUIRE(Nb > 0 && Cx > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && stride > 0 && M > 0, "conv: bad geometry");
  DASAC_REQUIRE((int64_t)Nb * Cx * H * W < (1ll << 30) && (int64_t)Nb * M * OutH * OutW < (1ll << 30) &&
                    (int64_t)Nb * OH * OW < (1ll << 30),
                "conv: tensor exceeds 2^30 elements (32-bit byte offsets)");
  DASAC_REQUIRE(Kpad % 16 == 0 && Mpad % 32 == 0 && Mpad >= M, "conv: bad padding Kpad=%d Mpad=%d", Kpad, Mpad);
  g.H = H; g.W = W; g.CxHW = Cx * H * W; g.OH = OH; g.OW = OW; g.stride = stride; g.Npix = Nb * OH * OW; g.n_tile0 = 0;
  g.M = M; g.Mpad = Mpad; g.Kpad = Kpad; g.OutH = OutH; g.OutW = OutW; g.ostride = ostride;
  DASAC_REQUIRE((int64_t)Nb * Cx * H * W * 4 <= kMaxTensorBytes && (int64_t)Nb * M * OH * OW * 4 <= kMaxTensorBytes,
                "conv: tensor exceeds the 4 GiB buffer-descriptor window");
  DASAC_REQUIRE((int64_t)Nb * M * OutH * OutW * 4 <= kMaxTensorBytes, "conv: output exceeds the 4 GiB buffer-descriptor window");
  // (row / plane offsets inside ONE image travel as signed scalar offsets)
  DASAC_REQUIRE((int64_t)Cx * H * W * 4 < (1ll << 31) && (int64_t)M * OutH * OutW * 4 < (1ll << 31) && (int64_t)M * OH * OW * 4 < (1ll << 31),
                "conv: one image of a tensor exceeds 2 GiB");
  g.x_bytes = (unsigned)((int64_t)Nb * Cx * H * W * 4);
  g.z_bytes = (unsigned)((int64_t)Nb * M * OH * OW * 4);
  g.out_bytes = (unsigned)((int64_t)Nb * M * OutH * OutW * 4);
  g.w_bytes = 0;
  return DASAC_OK;
}

}  // namespace dasac
