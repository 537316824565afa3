// Index arithmetic of the transposed bilinear upsampling (upsample.hip: upsample_bwd_x / _y) and of the cross-entropy backward
// fused with it (cross_entropy.hip: ce_bwd_rows, ce_bwd_rows_wave): which high-resolution positions feed a low-resolution one and
// with what weight, where a segment's gradients sit in LDS, and the two launch plans.  Plain functions, compiled for the host AND
// the device: the kernels and the launcher call exactly what the stand-alone host check (tools/ce_bwd_plan_check.cpp) walks, so
// the promises the kernels rely on -- a wave segment spans at most 256 pixels, a column has at most SPAN taps, every LDS index
// lies inside [0, pitch) -- are checked for every (w, W) the walk covers, not only at the GPU tests' shapes.
#pragma once
#include "bilinear.hpp"

#if defined(__HIPCC__)
#define DASAC_UPS_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define DASAC_UPS_HD inline
#endif

namespace dasac {

// ---- transpose of the bilinear upsampling, separable and gather-based (deterministic) ---------
// pass X: tmp[plane][y][j] = sum_x wx(x->j) * g[plane][y][x]          (reads the big gradient once)
// pass Y: d[plane][i][j]   = gscale * sum_y wy(y->i) * tmp[plane][y][j]
DASAC_UPS_HD float weight_to(int dst, float scale, int n_in, int target) {
  const Tap t = tap_ac(dst, scale, n_in);
  float wgt = 0.f;
  if (t.i0 == target) wgt += t.w0;
  if (t.i1 == target) wgt += t.w1;   // i0 == i1 at the border: both weights land on the same source
  return wgt;
}
DASAC_UPS_HD void src_range(int target, float scale, int n_out, int& lo, int& hi) {
  // high-res positions whose taps can touch `target`:  target-1 < scale*dst < target+1
  if (scale <= 0.f) {
    lo = 0;
    hi = n_out - 1;
    return;
  }
  lo = (int)floorf((float)(target - 1) / scale) - 1;
  hi = (int)ceilf((float)(target + 1) / scale) + 1;
  if (lo < 0) lo = 0;
  if (hi > n_out - 1) hi = n_out - 1;
}

// ---- the fused cross-entropy backward: a block keeps the gradients of one SEGMENT of low-resolution columns in LDS ------------
// LDS index x + x/8 spreads the stride-8 phase-2 reads over all banks
DASAC_UPS_HD int ce_lds_index(int x) { return x + (x >> 3); }

// the taps of column j in ce_bwd_rows_wave: src_range is generous by two positions on either side; the zero weights at both ends
// are dropped
DASAC_UPS_HD void ce_taps(int j, float sw, int W, int w, int& lo, int& hi) {
  src_range(j, sw, W, lo, hi);
  while (lo < hi && weight_to(lo, sw, w, j) == 0.f) ++lo;
  while (hi > lo && weight_to(hi, sw, w, j) == 0.f) --hi;
}

// the x range [xs, xe] the taps of the columns j0 .. j1 - 1 touch; xs is rounded down to a multiple of 4, so that quads start on
// the same grid for every segment
DASAC_UPS_HD void segment_range(int j0, int j1, float sw, int W, int& xs, int& xe) {
  int dummy;
  src_range(j0, sw, W, xs, dummy);
  src_range(j1 - 1, sw, W, dummy, xe);
  xs &= ~3;
}

// the widest segment of `cols` columns each (the last may be shorter), in whole quads
inline int segment_span(int cols, int w, int W, float sw) {
  int span = 0;
  for (int sg = 0; sg * cols < w; ++sg) {
    const int j1 = (sg + 1) * cols < w ? (sg + 1) * cols : w;
    int xs, xe;
    segment_range(sg * cols, j1, sw, W, xs, xe);
    const int quads = (xe | 3) + 1 - xs;
    if (quads > span) span = quads;
  }
  return span;
}

// ce_bwd_rows: one 128-thread block per (high-res row, segment).  The x range of a segment (+ the taps' reach on both sides) bounds
// the LDS row; ~300 pixels (about 24 KB for 19 classes) lets six blocks share a CU.
struct CeRowsPlan {
  int seg_cols, n_seg;   // columns per segment, segments per row
  int span, pitch;       // widest segment in pixels (whole quads), floats per class row in LDS
};
inline CeRowsPlan ce_rows_plan(int w, int W, float sw) {
  CeRowsPlan p;
  p.seg_cols = w;
  if (sw > 0.f) p.seg_cols = (int)(300.f * sw) - 2;
  p.seg_cols = p.seg_cols < 4 ? 4 : (p.seg_cols > w ? w : p.seg_cols);
  p.n_seg = (w + p.seg_cols - 1) / p.seg_cols;
  p.span = segment_span(p.seg_cols, w, W, sw);
  p.pitch = ce_lds_index(p.span - 1) + 2;
  return p;
}

// ce_bwd_rows_wave<19, SPAN>: one wave per (image, chunk of `rows` high-res rows, segment).  A segment is at most 256 pixels (one
// quad per lane in phase 1) and at most 64 columns (one per lane in phase 2); SPAN = 16 where taps <= 16, else 24.  `ok` is false
// where the kernel's conditions do not hold (the launcher then runs ce_bwd_rows); the other fields are set either way.
constexpr int kCeWaveLanes = 64, kCeWaveClasses = 19;
constexpr int kCeWaveMaxSpan = 256, kCeWaveMaxTaps = 24, kCeWaveMaxLds = 60 * 1024;
struct CeWavePlan {
  bool ok;
  int cols, n_seg;       // columns per segment (balanced), segments per row
  int span, pitch;       // as in CeRowsPlan
  int taps;              // most taps of any column (ce_taps)
  int rows, n_chunks;    // high-res rows per block, blocks per image and segment
};
inline CeWavePlan ce_wave_plan(int B, int H, int w, int W, float sw, int usable_cus) {
  CeWavePlan p;
  int cols_max = (int)(250.f * sw) - 1;   // a segment: <= 256 pixels for phase 1, <= 64 columns for phase 2
  if (cols_max > kCeWaveLanes) cols_max = kCeWaveLanes;
  cols_max = cols_max < 1 ? 1 : (cols_max > w ? w : cols_max);
  p.cols = (w + (w + cols_max - 1) / cols_max - 1) / ((w + cols_max - 1) / cols_max);   // balanced segments
  p.n_seg = (w + p.cols - 1) / p.cols;
  p.span = segment_span(p.cols, w, W, sw);
  p.taps = 0;
  for (int j = 0; j < w; ++j) {
    int lo, hi;
    ce_taps(j, sw, W, w, lo, hi);
    if (hi - lo + 1 > p.taps) p.taps = hi - lo + 1;
  }
  // rows per block: ONE round of blocks that nearly fills the chip (two 224-register waves per SIMD = 8 blocks per CU); all
  // blocks do the same work, so a second, partly filled round would cost a whole round's time
  const int slots = usable_cus * 8;
  const int per_row = B * p.n_seg > 1 ? B * p.n_seg : 1;
  const int chunks_max = slots / per_row > 1 ? slots / per_row : 1;
  p.rows = (H + chunks_max - 1) / chunks_max;
  if (p.rows < 4) p.rows = 4;
  p.n_chunks = (H + p.rows - 1) / p.rows;
  p.pitch = ce_lds_index(p.span - 1) + 2;
  p.ok = sw > 0.f && W >= 4 && p.span <= kCeWaveMaxSpan && p.taps <= kCeWaveMaxTaps &&
         (long long)B * p.n_chunks * p.n_seg < (1ll << 31) &&
         (long long)kCeWaveClasses * p.pitch * (long long)sizeof(float) <= kCeWaveMaxLds;
  return p;
}

}  // namespace dasac
