// Index arithmetic of the Winograd F(2x2,3x3) and F(4x4,3x3) paths for dilated 3x3 convolutions (winograd.hip): phase sizes, the
// numbering of tiles, patch and tensor offsets.  Plain integer functions, compiled for the host AND the device: the kernels call exactly what
// the stand-alone host check (tools/winograd_index_check.cpp) walks, so an offset the check has seen in range is the offset the
// kernel forms.
//
// A 3x3 convolution of dilation d, padding d, stride 1 splits into d*d independent undilated 3x3 convolutions ("phases"): output
// (y, x) with y % d == py, x % d == px only reads input pixels of the same residues.  Along one axis of extent n = q*d + r, phase
// p holds q + 1 samples for p < r and q otherwise; its samples are cut into F(2,3) tiles of two outputs, t = 0 .. ceil(samples/2)-1.
// Tile (p, t) produces the outputs o0 = p + 2*d*t and o0 + d (the second one may lie past the map) from the four inputs
// o0 - d, o0, o0 + d, o0 + 2d (any of them may lie outside: zero padding).
//
// Tiles of an axis are numbered g = t*d + p while every phase still has a tile t ("full" part), then the r leftover tiles t = b of
// the longer phases.  Consecutive g therefore means consecutive pixels: a wave whose lanes run along g reads and writes runs of d
// adjacent floats, and the four taps of a patch row fill each other's gaps.
//
// Everything above is F(2,3) per axis.  The functions that depend on the outputs per tile take them as a template parameter TM
// (2 by default: F(2x2,3x3); 4: F(4x4,3x3) -- forward, data gradient and weight gradient have both forms): a phase of q samples has
// ceil(q / TM) tiles, tile (p, t) produces the outputs o0 + e*d, e = 0 .. TM-1, o0 = p + TM*d*t, from the TM + 2 inputs
// o0 + (k - 1)*d, and the longer phases have a leftover tile when q % TM == 0.  The structs are the same for both, so a kernel of
// either form takes a Geom by value.  What else depends on TM stands under "the two forms" below.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DASAC_HD __host__ __device__ __forceinline__
#else
#define DASAC_HD inline
#endif

namespace dasac {
namespace wino {

// n / d for 0 <= n < 2^31 by multiply and shift (the scheme of dasac::fast_div in common.hpp, usable on both sides)
struct Div {
  unsigned mul, shift;
  int d;
};
DASAC_HD Div make_div(int d) {
  Div f{0u, 0u, d < 1 ? 1 : d};
  if (d <= 1) return f;
  int l = 1;
  while ((1ll << l) < d) ++l;
  const unsigned long long p = 1ull << (31 + l);
  f.mul = (unsigned)((p + (unsigned)d - 1) / (unsigned)d);
  f.shift = (unsigned)(l - 1);
  return f;
}
DASAC_HD int div(int n, Div f) {
  return f.mul ? (int)((unsigned)(((unsigned long long)(unsigned)n * f.mul) >> 32) >> f.shift) : n;
}

// ---- the two forms: everything beyond the tile arithmetic that depends on TM ------------------------------------------------------
// points of a tile = entries of the batched point GEMMs: (TM + 2)^2 = 16 or 36
template <int TM>
constexpr int kPoints = (TM + 2) * (TM + 2);
// F(4x4) pads the tile axis T of the transformed tensors to a multiple of 4 (the batched point contraction needs one, and 4x4 tiles
// rarely give one); the padding tiles are zero at every point.  F(2x2) takes the tile count as it is.
template <int TM>
constexpr bool kPaddedT = TM == 4;
template <int TM>
DASAC_HD int64_t padded_tiles(int64_t tiles) { return kPaddedT<TM> ? (tiles + 3) / 4 * 4 : tiles; }

struct Axis {
  int n, d;      // extent, dilation
  int q, r;      // n = q*d + r
  int b;         // tiles of a phase with q samples: ceil(q / TM)
  int full;      // tiles numbered t*d + p (t < b); 0 when q == 0
  int tiles;     // full + the leftover tiles (t == b) of the r longer phases, which exist when q % TM == 0
  Div by_d;
};
template <int TM = 2>
DASAC_HD Axis make_axis(int n, int d) {
  static_assert(TM == 2 || TM == 4, "outputs per tile and axis: 2 or 4 (coord_to_tile shifts by log2)");
  Axis a;
  a.n = n;
  a.d = d;
  a.q = n / d;
  a.r = n - a.q * d;
  a.b = (a.q + TM - 1) / TM;
  a.full = a.b * d;
  a.tiles = a.full + ((a.q & (TM - 1)) == 0 ? a.r : 0);
  a.by_d = make_div(d);
  return a;
}
DASAC_HD int phase_samples(const Axis& a, int p) { return a.q + (p < a.r ? 1 : 0); }
// tile number -> (phase, tile of the phase)
DASAC_HD void tile_decode(const Axis& a, int g, int& p, int& t) {
  if (g < a.full) {
    t = div(g, a.by_d);
    p = g - t * a.d;
  } else {
    t = a.b;
    p = g - a.full;
  }
}
DASAC_HD int tile_encode(const Axis& a, int p, int t) { return t < a.b ? t * a.d + p : a.full + p; }
// first output coordinate of a tile; the patch's inputs are first_out + (k - 1)*d, k = 0..TM+1, its outputs first_out + e*d, e = 0..TM-1
template <int TM = 2>
DASAC_HD int first_out(const Axis& a, int p, int t) { return p + TM * a.d * t; }
// output coordinate -> (tile number, e = which of the tile's TM outputs): the phase's sample index i splits into (i / TM, i % TM)
template <int TM = 2>
DASAC_HD void coord_to_tile(const Axis& a, int o, int& g, int& e) {
  const int i = div(o, a.by_d), p = o - i * a.d;
  e = i & (TM - 1);
  g = tile_encode(a, p, i >> (TM == 4 ? 2 : 1));
}

struct Geom {
  Axis ay, ax;
  int N, H, W, HW;
  int tiles_img;          // ay.tiles * ax.tiles
  int T;                  // the pixel axis of the point GEMMs: padded_tiles(N * tiles_img); tiles N * tiles_img .. T-1 are padding
  Div by_tiles_img, by_tx, by_hw, by_w;
};
template <int TM = 2>
DASAC_HD Geom make_geom(int N, int H, int W, int d) {
  Geom g;
  g.ay = make_axis<TM>(H, d);
  g.ax = make_axis<TM>(W, d);
  g.N = N;
  g.H = H;
  g.W = W;
  g.HW = H * W;
  g.tiles_img = g.ay.tiles * g.ax.tiles;
  g.T = (int)padded_tiles<TM>(N * g.tiles_img);
  g.by_tiles_img = make_div(g.tiles_img);
  g.by_tx = make_div(g.ax.tiles);
  g.by_hw = make_div(g.HW);
  g.by_w = make_div(W);
  return g;
}
// tile -> (image, first output row, first output column); not for the padding tiles of TM == 4 (real_tile)
template <int TM = 2>
DASAC_HD void tile_origin(const Geom& g, int tile, int& n, int& y0, int& x0) {
  n = div(tile, g.by_tiles_img);
  const int rem = tile - n * g.tiles_img;
  const int gy = div(rem, g.by_tx), gx = rem - gy * g.ax.tiles;
  int p, t;
  tile_decode(g.ay, gy, p, t);
  y0 = first_out<TM>(g.ay, p, t);
  tile_decode(g.ax, gx, p, t);
  x0 = first_out<TM>(g.ax, p, t);
}
DASAC_HD bool real_tile(const Geom& g, int tile) { return tile < g.N * g.tiles_img; }
// flattened output pixel (n, y, x) -> its tile and position (ey, ex) inside the tile's TM x TM outputs; `rem` = y*W + x
template <int TM = 2>
DASAC_HD void pixel_tile(const Geom& g, int pix, int& n, int& rem, int& tile, int& ey, int& ex) {
  n = div(pix, g.by_hw);
  rem = pix - n * g.HW;
  const int y = div(rem, g.by_w), x = rem - y * g.W;
  int gy, gx;
  coord_to_tile<TM>(g.ay, y, gy, ey);
  coord_to_tile<TM>(g.ax, x, gx, ex);
  tile = (n * g.ay.tiles + gy) * g.ax.tiles + gx;
}

constexpr unsigned kOutside = 0xFFFFFFFFu;   // byte offset of a tap outside the image: past any buffer extent, reads as zero

// byte offset into x [N, C, H, W] of tap (ky, kx), 0 .. TM+1 each, of the patch whose first output is (y0, x0); kOutside for the zero padding
DASAC_HD unsigned patch_offset(const Geom& g, int C, int n, int c, int y0, int x0, int ky, int kx) {
  const int y = y0 + (ky - 1) * g.ay.d, x = x0 + (kx - 1) * g.ax.d;
  if ((unsigned)y >= (unsigned)g.H || (unsigned)x >= (unsigned)g.W) return kOutside;
  return (unsigned)((n * C + c) * g.HW + y * g.W + x) * 4u;
}
// byte offset into a transformed tensor [points][C][T] (V, dM, or the point GEMMs' output), pt < kPoints<TM>
DASAC_HD unsigned point_offset(const Geom& g, int C, int pt, int c, int tile) { return (unsigned)((pt * C + c) * g.T + tile) * 4u; }
// byte offset into an NCHW activation of M channels
DASAC_HD unsigned out_offset(const Geom& g, int M, int n, int m, int rem) { return (unsigned)((n * M + m) * g.HW + rem) * 4u; }
// byte offset into the ReLU bit masks [M][w32] of the word that holds flattened pixel `pix` of channel m
DASAC_HD unsigned out_bits_offset(int m, int w32, int pix) { return (unsigned)(m * w32 + (pix >> 5)) * 4u; }
// largest tensor the 32-bit byte offsets reach (kMaxTensorBytes of conv_common.hpp)
constexpr int64_t kMaxBytes = (1ll << 32) - 4096;

}  // namespace wino
}  // namespace dasac
