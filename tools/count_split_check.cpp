// Stand-alone host check of csrc/count_split.hpp (tests/test_count_split_host.py builds and runs it): prints the split of every
// (H*W, B, usable CUs) the test lists, with the constants of dasac_mask_counts / dasac_confusion_counts (a block holds at most 2^29
// quads), of dasac_boundary_counts (no such limit) and with a limit of 7 quads, which no kernel uses but which makes the limit decide
// the split at every size.  One row each:  limit HW B cus blocks_per_image quads_per_block
#include <cstdio>

#include "count_split.hpp"

int main() {
  const long long hw[] = {1, 3, 63, 4096, 769ll * 769, 1024ll * 2048, (1ll << 33) + 5};
  const int batch[] = {1, 3, 8}, cus[] = {256, 248};
  const long long limits[] = {1ll << 29, 0, 7};
  for (long long limit : limits)
    for (long long HW : hw)
      for (int B : batch)
        for (int cu : cus) {
          const dasac::QuadSplit s = dasac::quad_split((HW + 3) >> 2, B, cu, 8, 4, 256, limit);
          std::printf("%lld %lld %d %d %lld %lld\n", limit, HW, B, cu, (long long)s.blocks_per_image, (long long)s.quads_per_block);
        }
  return 0;
}
