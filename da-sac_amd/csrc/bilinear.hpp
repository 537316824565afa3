// Bilinear taps, align_corners=True: ATen's upsample_bilinear2d weights (UpSample.h: scale = (in - 1) / (out - 1), 0 for an output
// extent of 1; src = scale * dst, i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1), w1 = src - i0).  Both tap indices stay inside
// the plane whatever the scale is (dst >= 0, scale >= 0): shrinking, enlarging, extent 1.  The library builds with
// -ffp-contract=off, and every kernel that resamples is held to bits that rest on the order of the operations below.
// Compiles for the host alone too (tools/ce_bwd_plan_check.cpp walks upsample_index.hpp, which needs tap_ac and ac_scale).
#pragma once
#if defined(__HIPCC__) || defined(__HIP__)      // __HIP__: the compiler's own, set before any HIP header is
#include <hip/hip_runtime.h>
#define DASAC_BIL_HD __host__ __device__ __forceinline__
#else
#define DASAC_BIL_HD inline
#endif

namespace dasac {

struct Tap {
  int i0, i1;
  float w0, w1;
};
DASAC_BIL_HD Tap tap_ac(int dst, float scale, int n_in) {
  const float src = scale * (float)dst;
  int i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  Tap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  t.w1 = src - (float)i0;
  t.w0 = 1.f - t.w1;
  return t;
}
DASAC_BIL_HD float ac_scale(int n_in, int n_out) {
  return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
}

struct TapPix {                                        // the four taps of one output pixel inside an h x w plane
  int o00, o01, o10, o11;
  float wx0, wx1, wy0, wy1;
};
DASAC_BIL_HD TapPix tap_pix(const Tap& ty, const Tap& tx, int w) {
  TapPix p;
  p.o00 = ty.i0 * w + tx.i0;
  p.o01 = ty.i0 * w + tx.i1;
  p.o10 = ty.i1 * w + tx.i0;
  p.o11 = ty.i1 * w + tx.i1;
  p.wx0 = tx.w0, p.wx1 = tx.w1, p.wy0 = ty.w0, p.wy1 = ty.w1;
  return p;
}
DASAC_BIL_HD float tap_mix(const TapPix& p, float v00, float v01, float v10, float v11) {
  const float top = p.wx0 * v00 + p.wx1 * v01;
  const float bot = p.wx0 * v10 + p.wx1 * v11;
  return p.wy0 * top + p.wy1 * bot;
}

}  // namespace dasac
