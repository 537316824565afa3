// Stand-alone host check of the conv GEMM's and the weight gradient's launch plans and block maps (csrc/conv_plan.hpp;
// tests/test_conv_plan_host.py builds it, feeds it and compares every line with tests/gemm_schedule_ref.py).  Reads one request per
// line from stdin and answers each with one line (a walk asked to print: plus one line per block):
//   gemm M K Npix pix_begin pix_end schedule workspace reserved full_chip
//        -> gemm kind grid m_tiles n_tiles lead_n tail_tiles split wants_streamk uses_workspace workspace_bytes
//   wgrad M K Cx Npix        -> wgrad Mpad Kpad bm bnk m_tiles k_tiles splits per grid psum_offset workspace_bytes
//   batched batch M C T      -> batched splits per grid psum_offset workspace_bytes            (walked too when splits > 0)
//   walk M K Npix 1 reserved  (one block per tile, whole tensor) -> walk kind grid m_tiles n_tiles KT busy bad
//   wwalk M K Cx Npix print  -> wwalk grid m_tiles k_tiles splits per busy bad                 [w bid m_tile k_tile split p_begin p_end]*
// (busy: the blocks with work) and ends with "conv plan check: S shapes, P plans walked, B blocks walked, X bad".  A walk runs the
// map functions the kernels call for every block of the grid and counts what breaks a promise:
//   * one block per tile: a block whose range is not one whole tile, a tile reached by no block or by two;
//   * weight gradient: a pixel range off the 32-pixel steps, ranges that overlap or leave gaps in [0, Npix), a (tile, split) reached
//     by no block or by two, a slab or Psum row outside the stated workspace.
// (The stream-K and tail maps are written inside conv_gemm: gemm_schedule_ref.py is their check, test_gemm_schedule_cpu.py.)
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "conv_plan.hpp"

using namespace dasac;

static long long g_bad = 0, g_shapes = 0, g_plans = 0, g_blocks = 0;
static const char* g_line = "";
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (g_bad++ < 20) std::printf("FAILED %s (line %d) at: %s\n", #cond, __LINE__, g_line); \
    }                                                                                \
  } while (0)

// every block of a one-block-per-tile GEMM launch, as conv_gemm<..., SK = 0, ...> maps it
static void walk_gemm(const GemmPlan& p) {
  const long long bad0 = g_bad;
  const int KT = p.k_steps;
  const long long total = (long long)p.m_tiles * p.n_tiles * KT;
  CHECK(p.kind == kGemmTiles && total < (1ll << 31) && p.grid > 0 && p.workspace_bytes == 0);
  std::vector<int> seen((size_t)p.m_tiles * p.n_tiles, 0);
  long long busy = 0;
  for (int bid = 0; bid < p.grid; ++bid) {
    const GemmWork w = gemm_tile_work(bid, p.m_tiles, p.n_tiles, KT);
    if (!w.has_work) continue;
    ++busy;
    const bool whole = w.it >= 0 && w.it % KT == 0 && w.it_end == w.it + KT && w.it_end <= total;      // one whole tile, nothing deposited
    CHECK(whole);
    if (whole) ++seen[w.it / KT];
  }
  for (int v : seen) CHECK(v == 1);                                       // every (tile, K-step) once
  ++g_plans;
  g_blocks += p.grid;
  std::printf("walk %d %d %d %d %d %lld %lld\n", p.kind, p.grid, p.m_tiles, p.n_tiles, KT, busy, g_bad - bad0);
}

// every block of a weight-gradient launch: `entries` batch entries of m_tiles x k_tiles tiles (1: conv_wgrad)
static void walk_wgrad(int m_tiles, int k_tiles, int splits, int per, int grid, int Npix, size_t rows, size_t cols, int bm, int bnk,
                       size_t slab, size_t entries, size_t psum_offset, size_t psum_rows, size_t workspace_bytes, bool print) {
  CHECK(splits >= 1 && per > 0 && per % kWgPix == 0 && (long long)splits * per >= Npix && grid % kNumXcd == 0);
  std::vector<int> seen((size_t)m_tiles * k_tiles * splits, 0);
  std::vector<std::pair<int, int>> range(splits, std::make_pair(-1, -1));
  for (int bid = 0; bid < grid; ++bid) {
    const int n_blocks = m_tiles * k_tiles * splits;
    const int lb = wgrad_list_index(bid, n_blocks);
    if (lb >= n_blocks) {
      if (print) std::printf("w %d -1 -1 -1 -1 -1\n", bid);
      continue;
    }
    const WgradTile w = wgrad_tile(lb, m_tiles, k_tiles);
    const PixelRange px = wgrad_pixels(w.split, per, Npix);
    if (print) std::printf("w %d %d %d %d %d %d\n", bid, w.m_tile, w.k_tile, w.split, px.begin, px.end);
    const bool inside = w.m_tile >= 0 && w.m_tile < m_tiles && w.k_tile >= 0 && w.k_tile < k_tiles && w.split >= 0 && w.split < splits;
    CHECK(inside);
    if (!inside) continue;
    ++seen[((size_t)w.split * k_tiles + w.k_tile) * m_tiles + w.m_tile];
    CHECK(px.begin % kWgPix == 0 && px.begin >= 0 && px.end <= Npix);
    CHECK(range[w.split].first < 0 || range[w.split] == std::make_pair(px.begin, px.end));
    range[w.split] = std::make_pair(px.begin, px.end);
    // the last element of the tile's slab rows, and of its Psum rows, inside the stated workspace
    const size_t last = ((size_t)w.split * entries + (entries - 1)) * slab + ((size_t)w.m_tile * bm + bm - 1) * cols + (size_t)w.k_tile * bnk + bnk - 1;
    CHECK((size_t)w.m_tile * bm + bm <= rows && (size_t)w.k_tile * bnk + bnk <= cols && last < psum_offset);
    CHECK((psum_offset + (size_t)w.split * psum_rows + (size_t)w.m_tile * bm + bm) * sizeof(float) <= workspace_bytes);
  }
  for (int v : seen) CHECK(v == 1);
  int at = 0;
  bool ended = false;
  for (const auto& r : range) {                                        // the splits tile [0, Npix); only trailing ones are empty
    CHECK(r.first >= 0);
    if (r.second > r.first) {
      CHECK(!ended && r.first == at);
      at = r.second;
    } else {
      ended = true;
    }
  }
  CHECK(at == Npix);
  ++g_plans;
  g_blocks += grid;
}

int main() {
  char line[256], cmd[16];
  while (std::fgets(line, sizeof line, stdin)) {
    g_line = line;
    long long a[9] = {0};
    const int n = std::sscanf(line, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld", cmd, a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8);
    if (n < 1) continue;
    const long long bad0 = g_bad;
    if (!std::strcmp(cmd, "gemm") && n == 10) {
      const GemmPlan p = gemm_plan((int)a[0], (int)a[1], a[2], a[3], a[4], (int)a[5], a[6] != 0, (int)a[7], a[8] != 0);
      std::printf("gemm %d %d %d %d %d %d %d %d %d %zu\n", p.kind, p.grid, p.m_tiles, p.n_tiles, p.lead_n, p.tail_tiles, p.split,
                  (int)p.wants_streamk, (int)p.uses_workspace, p.workspace_bytes);
      ++g_shapes;
    } else if (!std::strcmp(cmd, "wgrad") && n == 5) {
      const WgradPlan p = wgrad_plan((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
      std::printf("wgrad %d %d %d %d %d %d %d %d %d %zu %zu\n", p.Mpad, p.Kpad, p.bm, p.bnk, p.m_tiles, p.k_tiles, p.splits, p.per, p.grid,
                  p.psum_offset, p.workspace_bytes);
      ++g_shapes;
    } else if (!std::strcmp(cmd, "batched") && n == 5) {
      const int batch = (int)a[0], M = (int)a[1], C = (int)a[2], T = (int)a[3];
      const WgradBatchedPlan p = wgrad_batched_plan(batch, M, C, T);
      if (p.splits > 0)
        walk_wgrad(p.m_tiles, p.k_tiles, p.splits, p.per, p.grid, T, M, C, 128, 128, (size_t)M * C, batch, p.psum_offset, M, p.workspace_bytes, false);
      std::printf("batched %d %d %d %zu %zu\n", p.splits, p.per, p.grid, p.psum_offset, p.workspace_bytes);
      ++g_shapes;
    } else if (!std::strcmp(cmd, "walk") && n == 6) {
      walk_gemm(gemm_plan((int)a[0], (int)a[1], a[2], 0, a[2], 1, true, (int)a[4], true));
    } else if (!std::strcmp(cmd, "wwalk") && n == 6) {
      const WgradPlan p = wgrad_plan((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
      std::printf("wwalk %d %d %d %d %d", p.grid, p.m_tiles, p.k_tiles, p.splits, p.per);
      if (a[4]) std::printf(" -\n");
      walk_wgrad(p.m_tiles, p.k_tiles, p.splits, p.per, p.grid, (int)a[3], p.Mpad, p.Kpad, p.bm, p.bnk, p.slab, 1, p.psum_offset, p.Mpad,
                 p.workspace_bytes, a[4] != 0);
      if (!a[4]) std::printf(" %d %lld\n", p.m_tiles * p.k_tiles * p.splits, g_bad - bad0);
    } else {
      std::printf("FAILED to read: %s", line);
      ++g_bad;
    }
  }
  std::printf("conv plan check: %lld shapes, %lld plans walked, %lld blocks walked, %lld bad\n", g_shapes, g_plans, g_blocks, g_bad);
  return g_bad ? 1 : 0;
}
