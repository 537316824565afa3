// How a quad-streaming count kernel splits an image over blocks (plain C++: tools/count_split_check.cpp runs it on the host).
#pragma once
#include <cstdint>

namespace dasac {

struct QuadSplit {
  int64_t blocks_per_image, quads_per_block;           // block (b, j) takes quads [j * per, (j + 1) * per) of image b
};

// Blocks per image: at least `min_quads_per_thread` quads per thread until the grid of B images holds `blocks_per_cu` blocks per
// usable CU, and with `max_block_quads` > 0 never fewer than keep a block at or below that many quads (its u32 bins exact).
inline QuadSplit quad_split(int64_t n_quads, int B, int usable_cus, int blocks_per_cu, int min_quads_per_thread, int block,
                            int64_t max_block_quads = 0) {
  const int64_t chunk = (int64_t)min_quads_per_thread * block;
  int64_t bpi = (n_quads + chunk - 1) / chunk;
  const int64_t fill = ((int64_t)usable_cus * blocks_per_cu + B - 1) / B;
  if (bpi > fill) bpi = fill;
  if (max_block_quads > 0) {
    const int64_t need = (n_quads + max_block_quads - 1) / max_block_quads;
    if (bpi < need) bpi = need;
  }
  return QuadSplit{bpi, (n_quads + bpi - 1) / bpi};
}

}  // namespace dasac
