// Stand-alone host check of csrc/segments_index.hpp (tests/test_segments_index_host.py builds it with AddressSanitizer and UBSan and
// reads its output): for image sizes around the tile edges and both connectivities it prints every border item the merge kernel
// visits with the neighbours it would unite the pixel with, one line each
//   P <H> <W> <connectivity> <item> <y> <x> <vertical> <n> <neighbour indices...>
// after marking pixel and neighbours in an array of exactly H * W bytes (an index outside the image is a sanitizer error), and the
// tile constants, the bin rule at the sizes that matter and the local <-> image index map:
//   T <tile_h> <tile_w> <bins>
//   B <size> <bin>
//   L <H> <W> <tiles_y> <tiles_x> <pixels covered exactly once: 1 / 0>
#include <cstdio>
#include <vector>

#include "segments_index.hpp"

using namespace dasac;

int main() {
  std::printf("T %d %d %d\n", seg::kTileH, seg::kTileW, seg::kBins);
  const int sizes[] = {1, 2, 3, 4, 7, 8, (1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 1 << 30, 0x7fffffff};
  for (int s : sizes) std::printf("B %d %d\n", s, seg::bin_of(s));
  for (int k = 0; k < 31; ++k) std::printf("B %d %d\n", 1 << k, seg::bin_of(1 << k));

  const int TH = seg::kTileH, TW = seg::kTileW;
  const int shapes[][2] = {{1, 1},           {1, 7},           {7, 1},       {TH - 1, TW - 1},       {TH, TW},     {TH + 1, TW + 1},
                           {2 * TH, 2 * TW}, {2 * TH + 3, 2 * TW + 5}, {TH + 1, 3}, {3, TW + 1},     {3 * TH + 1, 1}, {1, 3 * TW + 1}};
  for (const auto& shape : shapes) {
    const int H = shape[0], W = shape[1];
    const int tiles_y = seg::tiles(H, TH), tiles_x = seg::tiles(W, TW);
    // every pixel of the image is the pixel of exactly one (tile, local index)
    std::vector<unsigned char> seen((size_t)H * W, 0);
    bool once = true;
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx)
        for (int local = 0; local < seg::kTilePixels; ++local) {
          const int y = ty * TH + local / TW, x = tx * TW + local % TW;
          if (y < H && x < W) {
            const int at = seg::local_to_image(ty * TH, tx * TW, local, W);
            once = once && at == y * W + x && seen[(size_t)at]++ == 0;
          }
        }
    for (unsigned char v : seen) once = once && v == 1;
    std::printf("L %d %d %d %d %d\n", H, W, tiles_y, tiles_x, once ? 1 : 0);

    for (int connectivity : {4, 8}) {
      std::vector<unsigned char> touched((size_t)H * W, 0);
      const int64_t items = seg::border_items(H, W);
      for (int64_t item = 0; item < items; ++item) {
        int y, x, nb[3];
        const bool vertical = seg::border_pixel(item, H, W, y, x);
        const int n = seg::border_neighbours(y, x, vertical, H, W, connectivity, nb);
        touched[(size_t)y * W + x] = 1;
        std::printf("P %d %d %d %lld %d %d %d %d", H, W, connectivity, (long long)item, y, x, vertical ? 1 : 0, n);
        for (int k = 0; k < n; ++k) {
          touched[(size_t)nb[k]] = 1;
          std::printf(" %d", nb[k]);
        }
        std::printf("\n");
      }
    }
  }
  std::printf("segments index check: done\n");
  return 0;
}
