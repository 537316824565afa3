// Stand-alone host check of the two launch plans of dasac_ce_loss_bwd_low (csrc/upsample_index.hpp; tests/test_ce_bwd_plan_host.py
// builds and runs it).  For every (w, W) with w in 1..130 and W in w..13*w, and for the shapes listed in main(), it walks what
// ce_bwd_rows and ce_bwd_rows_wave do with a plan and counts what breaks a promise the kernels rely on:
//   * every low-resolution column lies in exactly one segment, and no segment is empty;
//   * a column's tap range [lo, hi] (src_range in the block kernel, ce_taps in the wave kernel) lies inside its segment's [xs, xe];
//   * every LDS index of phase 1 (the pixels a block writes) and of phase 2 (the pixels a column reads) is below the pitch, and
//     phase 2 reads only what phase 1 wrote -- on a real array of C * pitch floats, so an index out of range is the sanitiser's find;
//   * wave plan, where ok: span <= 256 (one quad per lane), cols <= 64, a column's taps <= SPAN (16 where taps <= 16, else 24),
//     the hanging quad of a row rotates by at most 3 and loads inside the row, rows * n_chunks covers H with no empty chunk,
//     19 * pitch floats <= 60 KiB.
// One line per listed shape:  B H w W cus | seg_cols n_seg span pitch | ok cols n_seg span pitch taps rows n_chunks
#include <cstdio>
#include <vector>

#include "upsample_index.hpp"

using namespace dasac;

static long long bad = 0;
#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      if (bad++ < 20) std::printf("FAILED %s (w=%d W=%d, line %d)\n", #cond, w, W, __LINE__); \
    }                                                                                  \
  } while (0)

// The index arithmetic is the same for every class row: the first and the last class are walked (the last ends the array).
static const int kClasses[2] = {0, kCeWaveClasses - 1};

// phases 1 and 2 of one segment on `lds` ([C][pitch]); wave = the one-wave kernel's spelling of both
static void walk_segment(std::vector<float>& lds, int C, int pitch, int j0, int j1, int w, int W, float sw, bool wave, int span_taps) {
  int xs, xe;
  segment_range(j0, j1, sw, W, xs, xe);
  CHECK(j1 > j0 && xs >= 0 && xe <= W - 1 && xs <= xe);
  if (wave) {
    CHECK(xe - xs < 4 * kCeWaveLanes);
    for (int lane = 0; lane < kCeWaveLanes; ++lane) {
      const int ox = xs + lane * 4;
      if (ox > xe) continue;
      const int rot = ox + 4 - W > 0 ? ox + 4 - W : 0, ox_ld = ox - rot;
      CHECK(rot <= 3 && ox_ld >= 0 && ox_ld + 3 <= W - 1);
      const int at = ce_lds_index(ox - xs);
      CHECK(at >= 0 && at + 3 < pitch && at + 3 == ce_lds_index(ox - xs + 3));      // a quad's four slots are consecutive
      for (int c : kClasses)
        for (int e = 0; e < 4; ++e) lds[(size_t)c * pitch + at + e] = 1.f;
    }
  } else {
    for (int ox = xs; ox <= xe; ox += 4) {
      const int nx = W - ox < 4 ? W - ox : 4;
      for (int e = 0; e < nx; ++e) {
        const int at = ce_lds_index(ox + e - xs);
        CHECK(at >= 0 && at < pitch);
        for (int c : kClasses) lds[(size_t)c * pitch + at] = 1.f;
      }
    }
  }
  for (int j = j0; j < j1; ++j) {
    int lo, hi;
    if (wave) ce_taps(j, sw, W, w, lo, hi); else src_range(j, sw, W, lo, hi);
    CHECK(xs <= lo && lo <= hi && hi <= xe);
    if (wave) CHECK(hi - lo + 1 <= span_taps);
    // the wave kernel forms span_taps indices (the slots behind the last tap repeat it); the block kernel reads lo .. hi
    const int n = wave ? span_taps : hi - lo + 1;
    for (int i = 0; i < n; ++i) {
      const int at = ce_lds_index((lo + i < hi ? lo + i : hi) - xs);
      CHECK(at >= 0 && at < pitch);
      for (int c : kClasses) CHECK(lds[(size_t)c * pitch + at] == 1.f);
    }
  }
}

static void walk_plans(int B, int H, int w, int W, int cus, bool print) {
  const int C = kCeWaveClasses;
  const float sw = ac_scale(w, W);
  const CeRowsPlan rp = ce_rows_plan(w, W, sw);
  CHECK(rp.seg_cols >= 1 && rp.n_seg >= 1 && (rp.n_seg - 1) * rp.seg_cols < w && rp.n_seg * rp.seg_cols >= w && rp.pitch > 0);
  {
    std::vector<float> lds((size_t)C * rp.pitch);
    for (int sg = 0; sg < rp.n_seg; ++sg) {
      for (float& v : lds) v = 0.f;
      walk_segment(lds, C, rp.pitch, sg * rp.seg_cols, (sg + 1) * rp.seg_cols < w ? (sg + 1) * rp.seg_cols : w, w, W, sw, false, 0);
    }
  }
  const CeWavePlan wp = ce_wave_plan(B, H, w, W, sw, cus);
  if (wp.ok) {
    const int span_taps = wp.taps <= 16 ? 16 : 24;
    CHECK(wp.span <= 256 && wp.taps >= 1 && wp.taps <= 24 && wp.cols >= 1 && wp.cols <= kCeWaveLanes);
    CHECK((wp.n_seg - 1) * wp.cols < w && wp.n_seg * wp.cols >= w);
    CHECK(wp.rows >= 1 && (long long)wp.rows * wp.n_chunks >= H && H > (long long)wp.rows * (wp.n_chunks - 1));
    CHECK((long long)C * wp.pitch * 4 <= 60 * 1024);
    std::vector<float> lds((size_t)C * wp.pitch);
    for (int sg = 0; sg < wp.n_seg; ++sg) {
      for (float& v : lds) v = 0.f;
      walk_segment(lds, C, wp.pitch, sg * wp.cols, (sg + 1) * wp.cols < w ? (sg + 1) * wp.cols : w, w, W, sw, true, span_taps);
    }
  }
  if (print)
    std::printf("%d %d %d %d %d | %d %d %d %d | %d %d %d %d %d %d %d %d\n", B, H, w, W, cus, rp.seg_cols, rp.n_seg, rp.span, rp.pitch,
                (int)wp.ok, wp.cols, wp.n_seg, wp.span, wp.pitch, wp.taps, wp.rows, wp.n_chunks);
}

int main() {
  // (B, H, w, W) of LOW_CASES in tests/test_gpu_head_fp64.py
  const int low[][4] = {{2, 65, 13, 97}, {3, 33, 7, 49}, {1, 8, 6, 12},  {2, 38, 6, 46}, {2, 50, 9, 71}, {1, 33, 33, 35}, {2, 10, 4, 3},
                        {2, 40, 30, 60}, {1, 65, 5, 65}, {1, 65, 9, 65}, {1, 38, 6, 46}, {2, 20, 2, 49}, {2, 17, 5, 33}};
  for (const auto& s : low) walk_plans(s[0], s[1], s[2], s[3], 256, true);
  // the workload (97 -> 769), the next crop size (129 -> 1025) and the reference's 512 x 1024 crop
  const int big[][3] = {{769, 97, 769}, {1025, 129, 1025}, {512, 129, 1024}};
  const int batch[] = {1, 8, 16}, cus[] = {256, 248};
  for (const auto& s : big)
    for (int B : batch)
      for (int cu : cus) walk_plans(B, s[0], s[1], s[2], cu, true);
  long long pairs = 0;
  for (int w = 1; w <= 130; ++w)
    for (int W = w; W <= 13 * w; ++W, ++pairs) walk_plans(8, W, w, W, 256, false);
  std::printf("ce bwd plan check: %lld (w, W) pairs, %lld bad\n", pairs, bad);
  return bad ? 1 : 0;
}
