// Test-time augmentation for inference (infer_val.py:160-163 is single-scale; evaluation and pseudo-label statistics are
// usually taken over a few scales, plain and mirrored, with the class probabilities averaged): two kernels.
//
//   image_pyramid   the scaled (and mirrored) copies of a normalised image that the backbone runs on: bilinear,
//                   align_corners=True, [B,Cin,H,W] -> [B or 2B,Cin,Hs,Ws]; the mirrored half is written by the thread that
//                   computed the plain value, so one launch is one read of the source and the halves agree bit for bit.
//   infer_fuse      infer_labels of head.hip over S <= 8 low-resolution logit tensors at once: per output pixel and source the
//                   bilinear taps (at the mirrored column for a source that saw the mirrored image: interpolate(x).flip(-1)),
//                   the max-subtracted softmax, then mean or max over the sources, argmax (first maximum wins), LUT.  Writes
//                   1 byte per pixel (+ 4 for the confidence, + 4 C for the fused probabilities); none of the S upsampled
//                   [B,C,H,W] tensors, their flips, softmaxes or running sum ever exists.
//
// Tap arithmetic: ATen's align_corners=True weights, tap_ac / ac_scale of head.hip restated (as visualise.hip does), with the
// operations in the same order -- a single unflipped source gives infer_labels' bits.  image_pyramid takes the same taps from
// integers instead (pyr_tap): the fp32 product scale * dst is off by up to ~2e-6 pixels at an inexact scale (37 -> 46 rows is
// 0.8), which times the pixel-to-pixel difference of an image is a few 1e-6 of its range -- more than a pointwise kernel may
// differ from float64.  The logits that infer_fuse reads are smooth by comparison and are held to infer_labels' bits.
//
// Shape of infer_fuse: one pixel per thread, v[CT] (this source) and acc[CT] (fused) in registers.  Four pixels per thread, as
// in upsample_softmax, buys that kernel dwordx4 stores of its 76 B per pixel and shared taps at the fixed 8x factor; here the
// mandatory output is ONE byte per pixel, the sources have S different factors (a scale-0.5 source is upsampled 16x, the
// full-size one 8x: no common narrow-quad case), and 4 x (19 + 19) live class values would leave two waves per SIMD for a
// kernel whose time is gathers from L2 and expf, i.e. latency that wants waves (head.hip's round-4 note measured the same
// trade going the same way at two pixels per thread).  The source loop is a runtime loop over a by-value argument struct
// (wave-uniform scalar loads), not unrolled: S x 19 taps in flight would cost the registers that the occupancy needs.
#include "common.hpp"

#include <climits>

namespace dasac {

constexpr int kInfB = 256;
constexpr int kInfMaxC = 32;   // classes held in registers (kMaxC of head.hip)

struct InfTap {
  int i0, i1;
  float w0, w1;
};
__device__ __forceinline__ InfTap inf_tap(int dst, float scale, int n_in) {
  const float src = scale * (float)dst;
  int i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  InfTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  t.w1 = src - (float)i0;
  t.w0 = 1.f - t.w1;
  return t;
}
static float inf_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }

// src = dst * (n_in - 1) / (n_out - 1) exactly: i0 the quotient, w1 the remainder over the divisor (one rounding).  den =
// max(n_out - 1, 1), div = fast_div(den); dst * (n_in - 1) < 2^31 is the entry's check.  Unit scale: remainder 0, weights (1, 0).
__device__ __forceinline__ InfTap pyr_tap(int dst, int n_in, int den, FastDiv div) {
  const int num = dst * (n_in - 1);
  int i0 = fdiv(num, div);
  const int r = num - i0 * den;
  if (i0 > n_in - 1) i0 = n_in - 1;                  // n_out = 1 only: dst = 0, nothing to clamp otherwise
  InfTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  t.w1 = (float)r / (float)den;
  t.w0 = 1.f - t.w1;
  return t;
}

// One output pixel of the plain copy per thread and step; blockIdx.y = (b, channel) plane, so the plane bases are scalars.
// The mirrored copy of batch row b is row B + b: `planes` planes further on.
__global__ __launch_bounds__(kInfB) void image_pyramid(const float* __restrict__ x, int H, int W, int Hs, int Ws, int den_h, int den_w,
                                                       FastDiv div_h, FastDiv div_w, FastDiv div_ws, int planes, int with_flip, float* __restrict__ out) {
  const int plane = blockIdx.y, n_out = Hs * Ws;
  const float* pl = x + (size_t)plane * H * W;
  float* o = out + (size_t)plane * n_out;
  float* om = o + (size_t)planes * n_out;
  for (int p = blockIdx.x * kInfB + threadIdx.x; p < n_out; p += gridDim.x * kInfB) {
    const int oy = fdiv(p, div_ws), ox = p - oy * Ws;
    const InfTap ty = pyr_tap(oy, H, den_h, div_h), tx = pyr_tap(ox, W, den_w, div_w);
    const int r0 = ty.i0 * W, r1 = ty.i1 * W;
    const float top = tx.w0 * pl[r0 + tx.i0] + tx.w1 * pl[r0 + tx.i1];
    const float bot = tx.w0 * pl[r1 + tx.i0] + tx.w1 * pl[r1 + tx.i1];
    const float val = ty.w0 * top + ty.w1 * bot;      // unit scale: weights (1, 0), val = the source pixel
    o[p] = val;
    if (with_flip) om[oy * Ws + (Ws - 1 - ox)] = val;
  }
}

struct InferSources {                                // by value
  const float* x[DASAC_INFER_MAX_SOURCES];           // [B,C,h,w] each
  int h[DASAC_INFER_MAX_SOURCES], w[DASAC_INFER_MAX_SOURCES];
  float sh[DASAC_INFER_MAX_SOURCES], sw[DASAC_INFER_MAX_SOURCES];
  unsigned flip;                                     // bit s: source s saw the mirrored image
  int n;
};

// CT = compile-time class count (19), kInfMaxC = the generic runtime-C instantiation; MODE = DASAC_INFER_MEAN / _MAX.
template <int CT, int MODE>
__global__ __launch_bounds__(kInfB) void infer_fuse(const InferSources src, int Crt, int H, int W, FastDiv div_w,
                                                    const uint8_t* __restrict__ lut, uint8_t* __restrict__ labels,
                                                    float* __restrict__ conf, float* __restrict__ probs, int blocks_per_image) {
  const int C = CT < kInfMaxC ? CT : Crt;
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
  const int HW = H * W;
  for (int p = chunk * kInfB + threadIdx.x; p < HW; p += blocks_per_image * kInfB) {
    const int oy = fdiv(p, div_w), ox = p - oy * W;
    float acc[CT];                                   // probabilities are >= 0: 0 starts the sum and the maximum alike
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.f;
    for (int s = 0; s < src.n; ++s) {
      const int h = src.h[s], w = src.w[s], hw = h * w;
      const float* xb = src.x[s] + (size_t)b * C * hw;
      const int sx = ((src.flip >> s) & 1u) ? W - 1 - ox : ox;
      const InfTap ty = inf_tap(oy, src.sh[s], h), tx = inf_tap(sx, src.sw[s], w);
      const int o00 = ty.i0 * w + tx.i0, o01 = ty.i0 * w + tx.i1, o10 = ty.i1 * w + tx.i0, o11 = ty.i1 * w + tx.i1;
      float v[CT];
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < C) {
          const float* pl = xb + (size_t)c * hw;
          const float top = tx.w0 * pl[o00] + tx.w1 * pl[o01];
          const float bot = tx.w0 * pl[o10] + tx.w1 * pl[o11];
          v[c] = ty.w0 * top + ty.w1 * bot;
          mx = fmaxf(mx, v[c]);
        }
      }
      float den = 0.f;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          v[c] = expf(v[c] - mx);
          den += v[c];
        }
      const float inv = 1.f / den;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          const float pr = v[c] * inv;
          acc[c] = MODE == DASAC_INFER_MEAN ? acc[c] + pr : fmaxf(acc[c], pr);
        }
    }
    const float norm = 1.f / (float)src.n;           // one source: exactly 1
    int best = 0;
    float bp = -1.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        if (MODE == DASAC_INFER_MEAN) acc[c] *= norm;
        if (acc[c] > bp) {                           // strict: the first maximum wins
          bp = acc[c];
          best = c;
        }
      }
    labels[(size_t)b * HW + p] = lut ? lut[best] : (uint8_t)best;
    if (conf) conf[(size_t)b * HW + p] = bp;
    if (probs) {
      float* pb = probs + (size_t)b * C * HW + p;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) pb[(size_t)c * HW] = acc[c];
    }
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_image_pyramid(const float* image, int B, int Cin, int H, int W, int Hs, int Ws, int with_flip, float* out,
                                   dasac_stream_t stream) {
  DASAC_REQUIRE(image && out, "image_pyramid: null pointer");
  DASAC_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0, "image_pyramid: bad shape");
  DASAC_REQUIRE((int64_t)B * Cin < 65536 && (int64_t)H * W < (1ll << 30) && (int64_t)Hs * Ws < (1ll << 30), "image_pyramid: too large");
  DASAC_REQUIRE((int64_t)Hs * H < (1ll << 31) && (int64_t)Ws * W < (1ll << 31), "image_pyramid: too large");
  const int planes = B * Cin, den_h = Hs > 1 ? Hs - 1 : 1, den_w = Ws > 1 ? Ws - 1 : 1;
  const int grid = stream_grid((int64_t)Hs * Ws, kInfB, (kNumCu * 16 + planes - 1) / planes);
  hipLaunchKernelGGL(image_pyramid, dim3(grid, planes), dim3(kInfB), 0, as_stream(stream), image, H, W, Hs, Ws, den_h, den_w,
                     fast_div(den_h), fast_div(den_w), fast_div(Ws), planes, with_flip ? 1 : 0, out);
  DASAC_CHECK_LAUNCH("image_pyramid");
  return DASAC_OK;
}

extern "C" int dasac_infer_fuse(const dasac_infer_source* sources, int n_sources, int B, int C, int H, int W, int mode,
                                const uint8_t* lut, uint8_t* labels, float* conf, float* probs, dasac_stream_t stream) {
  DASAC_REQUIRE(sources && labels, "infer_fuse: null pointer");
  DASAC_REQUIRE(n_sources >= 1 && n_sources <= DASAC_INFER_MAX_SOURCES, "infer_fuse: %d sources (1..%d)", n_sources,
                DASAC_INFER_MAX_SOURCES);
  DASAC_REQUIRE(mode == DASAC_INFER_MEAN || mode == DASAC_INFER_MAX, "infer_fuse: unknown mode %d", mode);
  DASAC_REQUIRE(B > 0 && C > 0 && C <= kInfMaxC && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30), "infer_fuse: bad shape");
  InferSources a = {};
  a.n = n_sources;
  for (int s = 0; s < n_sources; ++s) {
    const dasac_infer_source& q = sources[s];
    DASAC_REQUIRE(q.logits && q.h > 0 && q.w > 0 && (int64_t)q.h * q.w < (1ll << 30), "infer_fuse: bad source %d", s);
    a.x[s] = q.logits;
    a.h[s] = q.h;
    a.w[s] = q.w;
    a.sh[s] = inf_scale(q.h, H);
    a.sw[s] = inf_scale(q.w, W);
    if (q.flip) a.flip |= 1u << s;
  }
  const int per = stream_grid((int64_t)H * W, kInfB, (kNumCu * 16 + B - 1) / B);
  hipStream_t st = as_stream(stream);
#define DASAC_FUSE(CT, MODE) \
  hipLaunchKernelGGL((infer_fuse<CT, MODE>), dim3(per * B), dim3(kInfB), 0, st, a, C, H, W, fast_div(W), lut, labels, conf, probs, per)
  if (C == 19) {
    if (mode == DASAC_INFER_MEAN) DASAC_FUSE(19, DASAC_INFER_MEAN); else DASAC_FUSE(19, DASAC_INFER_MAX);
  } else {
    if (mode == DASAC_INFER_MEAN) DASAC_FUSE(kInfMaxC, DASAC_INFER_MEAN); else DASAC_FUSE(kInfMaxC, DASAC_INFER_MAX);
  }
#undef DASAC_FUSE
  DASAC_CHECK_LAUNCH("infer_fuse");
  return DASAC_OK;
}
