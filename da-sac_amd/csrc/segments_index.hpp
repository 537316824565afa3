// Index arithmetic of the connected-component kernels (segments.hip): the tile <-> image index maps, the border pixels the merge
// kernel visits with the neighbours it unites them with, and the size-bin rule.  Plain integer functions, compiled for the host AND
// the device: the kernels call exactly what the stand-alone host check (tools/segments_index_check.cpp) prints, so a neighbour the
// check has seen inside the image and inside its row is the neighbour the kernel reads.
//
// An image is cut into tiles of kSegTileH x kSegTileW pixels, x fastest.  A pixel's index is y * W + x; inside a tile its local
// index is ly * kSegTileW + lx.  Both orders are row-major, so the smallest local index of a set of tile pixels is also its
// smallest image index: a tile's local roots are canonical for the tile.
//
// Border items of an image, numbered 0 .. seg_border_items - 1: first the pixels of the FIRST ROW of every tile row but the top one
// (tiles_y - 1 rows of W pixels: "horizontal seam" items), then the pixels of the FIRST COLUMN of every tile column but the left one
// (tiles_x - 1 columns of H pixels: "vertical seam" items).  A horizontal-seam pixel (y, x) is united with (y-1, x) and, under
// connectivity 8, with (y-1, x-1) and (y-1, x+1); a vertical-seam pixel with (y, x-1) and, under connectivity 8, (y-1, x-1) and
// (y+1, x-1) -- always inside the image, never across a row end.  Every pair of adjacent pixels that lie in different tiles is
// reached from one of its two pixels: a pair across a tile-row seam from its lower pixel, a pair across a tile-column seam from its
// right pixel (a corner pair from both).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DASAC_SEG_HD __host__ __device__ __forceinline__
#else
#define DASAC_SEG_HD inline
#endif

namespace dasac {
namespace seg {

constexpr int kTileH = 32, kTileW = 64;                // ops.SEGMENT_TILE restates it (tests/test_segments_cpu.py compares)
constexpr int kTilePixels = kTileH * kTileW;
constexpr int kBins = 24;                              // DASAC_SEGMENT_BINS

DASAC_SEG_HD int tiles(int n, int tile) { return (n + tile - 1) / tile; }

// image index of the tile pixel `local` of the tile whose first pixel is (y0, x0)
DASAC_SEG_HD int local_to_image(int y0, int x0, int local, int W) { return (y0 + local / kTileW) * W + x0 + local % kTileW; }

// bin of a segment of `size` >= 1 pixels: min(floor(log2(size)), kBins - 1)
DASAC_SEG_HD int bin_of(int size) {
  int b = 0;
  while (b < kBins - 1 && (size >> (b + 1)) != 0) ++b;
  return b;
}

DASAC_SEG_HD int64_t border_items(int H, int W) {
  return (int64_t)(tiles(H, kTileH) - 1) * W + (int64_t)(tiles(W, kTileW) - 1) * H;
}

// pixel (y, x) of border item `item`; true for a vertical-seam item
DASAC_SEG_HD bool border_pixel(int64_t item, int H, int W, int& y, int& x) {
  const int64_t horizontal = (int64_t)(tiles(H, kTileH) - 1) * W;
  const bool vertical = item >= horizontal;
  const int64_t rest = vertical ? item - horizontal : item;
  const int run = vertical ? H : W;                    // one division for both kinds, y and x by selects
  const int seam = (int)(rest / run), along = (int)(rest - (int64_t)seam * run);
  y = vertical ? along : (seam + 1) * kTileH;
  x = vertical ? (seam + 1) * kTileW : along;
  return vertical;
}

// image indices of the pixels a border pixel is united with (when they hold its class); returns how many, at most 3
DASAC_SEG_HD int border_neighbours(int y, int x, bool vertical, int H, int W, int connectivity, int (&out)[3]) {
  // horizontal seam: y >= kTileH, row y - 1 exists; vertical seam: x >= kTileW, column x - 1 exists
  const int straight = vertical ? y * W + x - 1 : (y - 1) * W + x;
  const bool has_before = connectivity == 8 && (vertical ? y > 0 : x > 0);
  const bool has_after = connectivity == 8 && (vertical ? y + 1 < H : x + 1 < W);
  const int before = has_before ? (y - 1) * W + x - 1 : straight;               // the diagonal towards smaller y / x
  const int after = !has_after ? straight : vertical ? (y + 1) * W + x - 1 : (y - 1) * W + x + 1;   // ... towards larger y / x
  out[0] = straight;                                   // fixed slots (no indexed store: the array stays in registers on the device);
  out[1] = has_before ? before : after;                // slots at and past the returned count are not to be read
  out[2] = after;
  return 1 + (has_before ? 1 : 0) + (has_after ? 1 : 0);
}

}  // namespace seg
}  // namespace dasac
