// Test-time augmentation for inference (infer_val.py:160-163 is single-scale; evaluation and pseudo-label statistics are
// usually taken over a few scales, plain and mirrored, with the class probabilities averaged): two kernels.
//
//   image_pyramid   the scaled (and mirrored) copies of a normalised image that the backbone runs on: bilinear,
//                   align_corners=True, [B,Cin,H,W] -> [B or 2B,Cin,Hs,Ws]; the mirrored half is written by the thread that
//                   computed the plain value, so one launch is one read of the source and the halves agree bit for bit.
//   infer_fuse      the label-map kernel (infer_val.py:160-163 + the writer's argmax / trainId->labelId LUT, :60-65) over
//                   S <= 8 low-resolution logit tensors at once: per output pixel and source the bilinear taps (at the mirrored
//                   column for a source that saw the mirrored image: interpolate(x).flip(-1)), the max-subtracted softmax, then
//                   mean or max over the sources, argmax (first maximum wins), LUT.  Writes 1 byte per pixel (+ 4 for the
//                   confidence, + 4 C for the fused probabilities); none of the S upsampled [B,C,H,W] tensors, their flips,
//                   softmaxes or running sum ever exists.  dasac_infer_labels is this kernel over one unflipped source.
//
// Tap arithmetic: ATen's align_corners=True weights, tap_ac / ac_scale of bilinear.hpp.  image_pyramid takes the same taps from
// integers instead (pyr_tap): the fp32 product scale * dst is off by up to ~2e-6 pixels at an inexact scale (37 -> 46 rows is
// 0.8), which times the pixel-to-pixel difference of an image is a few 1e-6 of its range -- more than a pointwise kernel may
// differ from float64.  The logits that infer_fuse reads are smooth by comparison.
//
// Shape of infer_fuse: one pixel per thread, v[CT] (this source) and acc[CT] (fused) in registers.  Four pixels per thread, as
// in upsample_softmax, buys that kernel dwordx4 stores of its 76 B per pixel and shared taps at the fixed 8x factor; here the
// mandatory output is ONE byte per pixel, the sources have S different factors (a scale-0.5 source is upsampled 16x, the
// full-size one 8x: no common narrow-quad case), and 4 x (19 + 19) live class values would leave two waves per SIMD for a
// kernel whose time is gathers from L2 and expf, i.e. latency that wants waves (upsample.hip's round-4 note measured the same
// trade going the same way at two pixels per thread).  The source loop is a runtime loop over a by-value argument struct
// (wave-uniform scalar loads), not unrolled: S x 19 taps in flight would cost the registers that the occupancy needs.
#include "bilinear.hpp"
#include "common.hpp"

#include <climits>

namespace dasac {

constexpr int kInfB = 256;
constexpr int kInfMaxC = 32;   // classes held in registers

// src = dst * (n_in - 1) / (n_out - 1) exactly: i0 the quotient, w1 the remainder over the divisor (one rounding).  den =
// max(n_out - 1, 1), div = fast_div(den); dst * (n_in - 1) < 2^31 is the entry's check.  Unit scale: remainder 0, weights (1, 0).
__device__ __forceinline__ Tap pyr_tap(int dst, int n_in, int den, FastDiv div) {
  const int num = dst * (n_in - 1);
  int i0 = fdiv(num, div);
  const int r = num - i0 * den;
  if (i0 > n_in - 1) i0 = n_in - 1;                  // n_out = 1 only: dst = 0, nothing to clamp otherwise
  Tap t;
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
    const TapPix q = tap_pix(pyr_tap(oy, H, den_h, div_h), pyr_tap(ox, W, den_w, div_w), W);
    const float val = tap_mix(q, pl[q.o00], pl[q.o01], pl[q.o10], pl[q.o11]);   // unit scale: weights (1, 0), the source pixel
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

// The softmax over the classes of source s's bilinear taps at output pixel (oy, ox) of image b, as v[c] * (the value returned):
// v[0..C) = exp(tap mix - their maximum), returned 1 / their sum.
template <int CT>
__device__ __forceinline__ float source_probs(const InferSources& src, int s, int b, int C, int oy, int ox, int W, float (&v)[CT]) {
  const int h = src.h[s], w = src.w[s], hw = h * w;
  const float* xb = src.x[s] + (size_t)b * C * hw;
  const int sx = ((src.flip >> s) & 1u) ? W - 1 - ox : ox;
  const TapPix q = tap_pix(tap_ac(oy, src.sh[s], h), tap_ac(sx, src.sw[s], w), w);
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      const float* pl = xb + (size_t)c * hw;
      v[c] = tap_mix(q, pl[q.o00], pl[q.o01], pl[q.o10], pl[q.o11]);
      mx = fmaxf(mx, v[c]);
    }
  float den = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      v[c] = expf(v[c] - mx);
      den += v[c];
    }
  return 1.f / den;
}

// CT = compile-time class count (19), kInfMaxC = the generic runtime-C instantiation; MODE = DASAC_INFER_MEAN / _MAX.
// SINGLE (dasac_infer_labels): source 0 alone is the fused result -- no acc[] beside v[], no source loop, no `probs`; the bits
// are those of the mean over one source (0 + p = p and p * 1 = p exactly).  The fused value is a local of the argmax loop and
// `probs` is stored from there: written back into acc[] under the runtime-C predicate it costs the generic instantiation a wave
// per SIMD (143 instead of 124 VGPRs).
template <int CT, int MODE, bool SINGLE>
__global__ __launch_bounds__(kInfB) void infer_fuse(const InferSources src, int Crt, int H, int W, FastDiv div_w,
                                                    const uint8_t* __restrict__ lut, uint8_t* __restrict__ labels,
                                                    float* __restrict__ conf, float* __restrict__ probs, int blocks_per_image) {
  const int C = CT < kInfMaxC ? CT : Crt;
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
  const int HW = H * W;
  for (int p = chunk * kInfB + threadIdx.x; p < HW; p += blocks_per_image * kInfB) {
    const int oy = fdiv(p, div_w), ox = p - oy * W;
    float acc[CT], scale;                            // the fused value of class c is acc[c] * scale
    if (SINGLE) {
      scale = source_probs<CT>(src, 0, b, C, oy, ox, W, acc);
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = 0.f;     // probabilities are >= 0: 0 starts the sum and the maximum alike
      for (int s = 0; s < src.n; ++s) {
        float v[CT];
        const float inv = source_probs<CT>(src, s, b, C, oy, ox, W, v);
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) {
            const float pr = v[c] * inv;
            acc[c] = MODE == DASAC_INFER_MEAN ? acc[c] + pr : fmaxf(acc[c], pr);
          }
      }
      scale = 1.f / (float)src.n;                    // one source: exactly 1
    }
    float* pb = (!SINGLE && probs) ? probs + (size_t)b * C * HW + p : nullptr;
    int best = 0;
    float bp = -1.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        const float f = (SINGLE || MODE == DASAC_INFER_MEAN) ? acc[c] * scale : acc[c];
        if (f > bp) {                                // strict: the first maximum wins, as torch.argmax / numpy.argmax
          bp = f;
          best = c;
        }
        if (pb) pb[(size_t)c * HW] = f;
      }
    labels[(size_t)b * HW + p] = lut ? lut[best] : (uint8_t)best;
    if (conf) conf[(size_t)b * HW + p] = bp;
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

// One launch of the label-map kernel; `single`: a.n == 1, unflipped, mean, no probs (dasac_infer_labels).
static void launch_infer_fuse(const InferSources& a, bool single, int B, int C, int H, int W, int mode, const uint8_t* lut,
                              uint8_t* labels, float* conf, float* probs, dasac_stream_t stream) {
  const int per = stream_grid((int64_t)H * W, kInfB, (kNumCu * 16 + B - 1) / B);
  hipStream_t st = as_stream(stream);
#define DASAC_FUSE(CT, MODE, SINGLE)                                                                                          \
  hipLaunchKernelGGL((infer_fuse<CT, MODE, SINGLE>), dim3(per * B), dim3(kInfB), 0, st, a, C, H, W, fast_div(W), lut, labels, \
                     conf, probs, per)
  if (single) {
    if (C == 19) DASAC_FUSE(19, DASAC_INFER_MEAN, true); else DASAC_FUSE(kInfMaxC, DASAC_INFER_MEAN, true);
  } else if (C == 19) {
    if (mode == DASAC_INFER_MEAN) DASAC_FUSE(19, DASAC_INFER_MEAN, false); else DASAC_FUSE(19, DASAC_INFER_MAX, false);
  } else {
    if (mode == DASAC_INFER_MEAN) DASAC_FUSE(kInfMaxC, DASAC_INFER_MEAN, false); else DASAC_FUSE(kInfMaxC, DASAC_INFER_MAX, false);
  }
#undef DASAC_FUSE
}

extern "C" int dasac_infer_labels(const float* logits, int B, int C, int h, int w, int H, int W, const uint8_t* lut,
                                  uint8_t* labels, float* conf, dasac_stream_t stream) {
  DASAC_REQUIRE(logits && labels, "infer_labels: null pointer");
  DASAC_REQUIRE(B > 0 && C > 0 && C <= kInfMaxC && h > 0 && w > 0 && H > 0 && W > 0, "infer_labels: bad shape");
  DASAC_REQUIRE((int64_t)H * W < (1ll << 30) && (int64_t)h * w < (1ll << 30), "infer_labels: plane too large");
  InferSources a = {};
  a.n = 1;
  a.x[0] = logits;
  a.h[0] = h;
  a.w[0] = w;
  a.sh[0] = ac_scale(h, H);
  a.sw[0] = ac_scale(w, W);
  launch_infer_fuse(a, true, B, C, H, W, DASAC_INFER_MEAN, lut, labels, conf, nullptr, stream);
  DASAC_CHECK_LAUNCH("infer_labels");
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
    a.sh[s] = ac_scale(q.h, H);
    a.sw[s] = ac_scale(q.w, W);
    if (q.flip) a.flip |= 1u << s;
  }
  launch_infer_fuse(a, false, B, C, H, W, mode, lut, labels, conf, probs, stream);
  DASAC_CHECK_LAUNCH("infer_fuse");
  return DASAC_OK;
}
