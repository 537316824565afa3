// Stand-alone host check of csrc/winograd_index.hpp: walks every offset the input and the output transform of winograd.hip form
// (and, with four outputs per tile, the input, the grad and the output transform of the F(4x4,3x3) paths: check_shape4)
// for a list of shapes and requires each to lie inside its tensor, the tile numbering to be a bijection, and every output pixel
// to belong to exactly one (tile, ey, ex).  Small shapes also touch heap arrays of the tensors' exact sizes at those offsets, so a
// build with -fsanitize=address,undefined reports any access the arithmetic check itself would have missed.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ida-sac_amd/csrc tools/winograd_index_check.cpp -o wino_check && ./wino_check
//
// Host code only: never loaded into Python, never run on the GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "winograd_index.hpp"

using namespace dasac::wino;

static long long g_bad = 0;
#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      if (g_bad++ < 10) {                          \
        std::printf("FAIL %s: ", #cond);           \
        std::printf(__VA_ARGS__);                  \
        std::printf("\n");                         \
      }                                            \
    }                                              \
  } while (0)

static void check_div(int d, int limit) {
  const Div f = make_div(d);
  const int probes[] = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, limit - 1, limit, limit / d * d, limit / d * d - 1};
  for (int n : probes)
    if (n >= 0) EXPECT(div(n, f) == n / d, "d=%d n=%d got %d", d, n, div(n, f));
}

static void check_shape(int N, int C, int M, int H, int W, int d, bool say = true) {
  const Geom g = make_geom(N, H, W, d);
  const long long x_bytes = 4ll * N * C * H * W, v_bytes = 4ll * 16 * C * g.T, y_bytes = 4ll * 16 * M * g.T, out_bytes = 4ll * N * M * H * W;
  const int npix = N * H * W, w32 = (npix + 31) / 32;
  EXPECT(x_bytes <= kMaxBytes && v_bytes <= kMaxBytes && y_bytes <= kMaxBytes && out_bytes <= kMaxBytes, "tensor too large");
  // phase sizes against their definition
  for (const Axis* a : {&g.ay, &g.ax}) {
    int tiles = 0, samples = 0;
    for (int p = 0; p < a->d; ++p) {
      int cnt = 0;
      for (int o = p; o < a->n; o += a->d) ++cnt;
      EXPECT(phase_samples(*a, p) == cnt, "phase %d of n=%d d=%d: %d != %d", p, a->n, a->d, phase_samples(*a, p), cnt);
      tiles += (cnt + 1) / 2;
      samples += cnt;
    }
    EXPECT(tiles == a->tiles && samples == a->n, "n=%d d=%d: %d tiles, expected %d", a->n, a->d, a->tiles, tiles);
    std::vector<int> seen(a->tiles, 0);
    for (int p = 0; p < a->d; ++p)
      for (int t = 0; t < (phase_samples(*a, p) + 1) / 2; ++t) {
        const int gi = tile_encode(*a, p, t);
        EXPECT(gi >= 0 && gi < a->tiles, "tile number %d of %d", gi, a->tiles);
        if (gi < 0 || gi >= a->tiles) continue;
        ++seen[gi];
        int p2, t2;
        tile_decode(*a, gi, p2, t2);
        EXPECT(p2 == p && t2 == t, "decode(encode(%d,%d)) = (%d,%d)", p, t, p2, t2);
      }
    for (int gi = 0; gi < a->tiles; ++gi) EXPECT(seen[gi] == 1, "tile %d of axis n=%d d=%d named %d times", gi, a->n, a->d, seen[gi]);
    check_div(a->d, a->n);
  }
  check_div(g.tiles_img, g.T);
  check_div(g.ax.tiles, g.tiles_img);
  check_div(g.HW, npix);
  check_div(W, g.HW);

  // small shapes: real arrays of the exact sizes, touched at every offset (what the sanitizers watch)
  const bool touch = x_bytes + v_bytes + y_bytes + out_bytes < (96ll << 20);
  std::vector<unsigned char> X, V, Y, O;
  std::vector<unsigned> bits;
  if (touch) {
    X.assign(x_bytes, 0);
    V.assign(v_bytes, 0);
    Y.assign(y_bytes, 0);
    O.assign(out_bytes, 0);
    bits.assign((size_t)M * w32, 0u);
  }
  // channels walked: all of them when the arrays are touched, else the first and the last (offsets are monotonic in c)
  std::vector<int> cs, ms;
  for (int c = 0; c < C; ++c)
    if (touch || c == 0 || c == C - 1) cs.push_back(c);
  for (int m = 0; m < M; ++m)
    if (touch || m == 0 || m == M - 1) ms.push_back(m);

  // ---- input transform: every (c, tile): 16 gathered taps, 16 stores
  std::vector<int> reads((size_t)N * H * W, 0);
  for (int c : cs)
    for (int tile = 0; tile < g.T; ++tile) {
      int n, y0, x0;
      tile_origin(g, tile, n, y0, x0);
      EXPECT(n >= 0 && n < N && y0 >= 0 && y0 < H && x0 >= 0 && x0 < W, "tile %d -> image %d origin (%d,%d)", tile, n, y0, x0);
      for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) {
          const unsigned off = patch_offset(g, C, n, c, y0, x0, ky, kx);
          const int y = y0 + (ky - 1) * d, x = x0 + (kx - 1) * d;
          const bool inside = y >= 0 && y < H && x >= 0 && x < W;
          EXPECT(inside == (off != kOutside), "tile %d tap (%d,%d): inside %d offset %u", tile, ky, kx, (int)inside, off);
          if (off == kOutside) continue;
          EXPECT((long long)off + 4 <= x_bytes && off % 4 == 0, "x offset %u of %lld", off, x_bytes);
          EXPECT(off == 4u * (unsigned)(((n * C + c) * H + y) * W + x), "x offset %u is not (%d,%d,%d,%d)", off, n, c, y, x);
          if (touch && (long long)off + 4 <= x_bytes) ++X[off];
          if (c == cs[0]) ++reads[(size_t)(n * H + y) * W + x];
        }
      for (int pt = 0; pt < 16; ++pt) {
        const unsigned off = point_offset(g, C, pt, c, tile);
        EXPECT((long long)off + 4 <= v_bytes && off % 4 == 0, "v offset %u of %lld", off, v_bytes);
        if (touch && (long long)off + 4 <= v_bytes) {
          EXPECT(V[off] == 0, "v offset %u written twice", off);
          V[off] = 1;
        }
      }
    }
  // every input pixel belongs to the 4x4 patches of exactly 2 x 2 tiles, fewer only next to the far edges
  for (size_t i = 0; i < reads.size(); ++i) EXPECT(reads[i] >= 1 && reads[i] <= 4, "pixel %zu read %d times", i, reads[i]);
  if (touch)
    for (long long i = 0; i < v_bytes; i += 4) EXPECT(V[i] == 1, "v offset %lld never written", i);

  // ---- output transform: every (m, pixel): 9 loads, one store, one bit
  std::vector<int> tile_hits(g.T, 0);
  for (int m : ms)
    for (int pix = 0; pix < npix; ++pix) {
      int n, rem, tile, ey, ex;
      pixel_tile(g, pix, n, rem, tile, ey, ex);
      EXPECT(n == pix / (H * W) && rem == pix % (H * W), "pixel %d -> image %d rem %d", pix, n, rem);
      EXPECT(tile >= 0 && tile < g.T && (ey | ex) >= 0 && ey <= 1 && ex <= 1, "pixel %d -> tile %d (%d,%d)", pix, tile, ey, ex);
      if (tile < 0 || tile >= g.T) continue;
      int n2, y0, x0;
      tile_origin(g, tile, n2, y0, x0);
      EXPECT(n2 == n && y0 + ey * d == rem / W && x0 + ex * d == rem % W, "pixel %d is not output (%d,%d) of tile %d", pix, ey, ex, tile);
      if (m == ms[0]) ++tile_hits[tile];
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) {
          const int pt = (ey + j) * 4 + ex + k;
          EXPECT(pt >= 0 && pt < 16, "point %d", pt);
          const unsigned off = point_offset(g, M, pt, m, tile);
          EXPECT((long long)off + 4 <= y_bytes && off % 4 == 0, "y offset %u of %lld", off, y_bytes);
          if (touch && (long long)off + 4 <= y_bytes) ++Y[off];
        }
      const unsigned off = out_offset(g, M, n, m, rem);
      EXPECT((long long)off + 4 <= out_bytes && off == 4u * (unsigned)((n * M + m) * H * W + rem), "out offset %u of %lld", off, out_bytes);
      if (touch && (long long)off + 4 <= out_bytes) {
        EXPECT(O[off] == 0, "out offset %u written twice", off);
        O[off] = 1;
      }
      const long long word = (long long)m * w32 + (pix >> 5);
      EXPECT(word < (long long)M * w32, "bit word %lld of %lld", word, (long long)M * w32);
      if (touch && word < (long long)M * w32) bits[word] |= 1u << (pix & 31);
    }
  for (int t = 0; t < g.T; ++t) EXPECT(tile_hits[t] >= 1 && tile_hits[t] <= 4, "tile %d holds %d output pixels", t, tile_hits[t]);
  if (touch)
    for (long long i = 0; i < out_bytes; i += 4) EXPECT(O[i] == 1, "out offset %lld never written", i);
  if (say)
    std::printf("N=%d C=%d M=%d %dx%d d=%d: %d x %d tiles per image, T=%d%s\n", N, C, M, H, W, d, g.ay.tiles, g.ax.tiles, g.T,
                touch ? " (arrays touched)" : "");
}

// ---- F(4x4,3x3): input_transform<F4> and grad_transform<F4> of winograd.hip, tensors [36][C][T] with T padded to a multiple of 4 -------
static void check_shape4(int N, int C, int M, int H, int W, int d, bool say = true) {
  const Geom g = make_geom<4>(N, H, W, d);
  const int real = N * g.tiles_img;
  const long long x_bytes = 4ll * N * C * H * W, v_bytes = 4ll * 36 * C * g.T, dz_bytes = 4ll * N * M * H * W, m_bytes = 4ll * 36 * M * g.T;
  EXPECT(x_bytes <= kMaxBytes && v_bytes <= kMaxBytes && dz_bytes <= kMaxBytes && m_bytes <= kMaxBytes, "tensor too large");
  EXPECT(g.T % 4 == 0 && g.T >= real && g.T < real + 4, "T=%d for %d tiles", g.T, real);
  for (const Axis* a : {&g.ay, &g.ax}) {
    int tiles = 0;
    for (int p = 0; p < a->d; ++p) {
      int cnt = 0;
      for (int o = p; o < a->n; o += a->d) ++cnt;
      EXPECT(phase_samples(*a, p) == cnt, "m=4 phase %d of n=%d d=%d: %d != %d", p, a->n, a->d, phase_samples(*a, p), cnt);
      tiles += (cnt + 3) / 4;
    }
    EXPECT(tiles == a->tiles, "m=4 n=%d d=%d: %d tiles, expected %d", a->n, a->d, a->tiles, tiles);
    std::vector<int> seen(a->tiles, 0);
    for (int p = 0; p < a->d; ++p)
      for (int t = 0; t < (phase_samples(*a, p) + 3) / 4; ++t) {
        const int gi = tile_encode(*a, p, t);
        EXPECT(gi >= 0 && gi < a->tiles, "m=4 tile number %d of %d", gi, a->tiles);
        if (gi < 0 || gi >= a->tiles) continue;
        ++seen[gi];
        int p2, t2;
        tile_decode(*a, gi, p2, t2);
        EXPECT(p2 == p && t2 == t, "m=4 decode(encode(%d,%d)) = (%d,%d)", p, t, p2, t2);
      }
    for (int gi = 0; gi < a->tiles; ++gi) EXPECT(seen[gi] == 1, "m=4 tile %d of axis n=%d d=%d named %d times", gi, a->n, a->d, seen[gi]);
    // every coordinate is output e of exactly the tile coord_to_tile names
    for (int o = 0; o < a->n; ++o) {
      int gi, e, p, t;
      coord_to_tile<4>(*a, o, gi, e);
      EXPECT(gi >= 0 && gi < a->tiles && e >= 0 && e < 4, "m=4 coordinate %d -> tile %d output %d", o, gi, e);
      if (gi < 0 || gi >= a->tiles) continue;
      tile_decode(*a, gi, p, t);
      EXPECT(first_out<4>(*a, p, t) + e * a->d == o, "m=4 coordinate %d is not output %d of tile %d", o, e, gi);
    }
  }
  check_div(g.tiles_img, g.T);
  check_div(g.ax.tiles, g.tiles_img);

  const bool touch = x_bytes + v_bytes + dz_bytes + m_bytes < (96ll << 20);
  std::vector<unsigned char> X, V, Z, Mt;
  if (touch) {
    X.assign(x_bytes, 0);
    V.assign(v_bytes, 0);
    Z.assign(dz_bytes, 0);
    Mt.assign(m_bytes, 0);
  }
  std::vector<int> cs, ms;
  for (int c = 0; c < C; ++c)
    if (touch || c == 0 || c == C - 1) cs.push_back(c);
  for (int m = 0; m < M; ++m)
    if (touch || m == 0 || m == M - 1) ms.push_back(m);

  // the 36 stores of a (channel, tile), padding tiles included: both kernels write every tile below T
  auto stores = [&](int Cn, int c, int tile, std::vector<unsigned char>& arr, long long bytes, const char* what) {
    for (int pt = 0; pt < 36; ++pt) {
      const unsigned off = point_offset(g, Cn, pt, c, tile);
      EXPECT((long long)off + 4 <= bytes && off % 4 == 0, "m=4 %s offset %u of %lld", what, off, bytes);
      EXPECT(off == 4u * (unsigned)((pt * Cn + c) * g.T + tile), "m=4 %s offset %u is not (%d,%d,%d)", what, off, pt, c, tile);
      if (touch && (long long)off + 4 <= bytes) {
        EXPECT(arr[off] == 0, "m=4 %s offset %u written twice", what, off);
        arr[off] = 1;
      }
    }
  };
  // ---- input_transform<F4>: 36 gathered taps of the 6x6 patch
  std::vector<int> reads((size_t)N * H * W, 0);
  for (int c : cs)
    for (int tile = 0; tile < g.T; ++tile) {
      stores(C, c, tile, V, v_bytes, "v");
      EXPECT(real_tile(g, tile) == (tile < real), "m=4 tile %d real", tile);
      if (!real_tile(g, tile)) continue;
      int n, y0, x0;
      tile_origin<4>(g, tile, n, y0, x0);
      EXPECT(n >= 0 && n < N && y0 >= 0 && y0 < H && x0 >= 0 && x0 < W, "m=4 tile %d -> image %d origin (%d,%d)", tile, n, y0, x0);
      for (int ky = 0; ky < 6; ++ky)
        for (int kx = 0; kx < 6; ++kx) {
          const unsigned off = patch_offset(g, C, n, c, y0, x0, ky, kx);
          const int y = y0 + (ky - 1) * d, x = x0 + (kx - 1) * d;
          const bool inside = y >= 0 && y < H && x >= 0 && x < W;
          EXPECT(inside == (off != kOutside), "m=4 tile %d tap (%d,%d): inside %d offset %u", tile, ky, kx, (int)inside, off);
          if (off == kOutside) continue;
          EXPECT((long long)off + 4 <= x_bytes && off == 4u * (unsigned)(((n * C + c) * H + y) * W + x), "m=4 x offset %u of %lld", off, x_bytes);
          if (touch && (long long)off + 4 <= x_bytes) ++X[off];
          if (c == cs[0]) ++reads[(size_t)(n * H + y) * W + x];
        }
    }
  // an input pixel lies in the 6-wide patches (4 apart) of one or two tiles per axis
  for (size_t i = 0; i < reads.size(); ++i) EXPECT(reads[i] >= 1 && reads[i] <= 4, "m=4 pixel %zu read %d times", i, reads[i]);
  // ---- grad_transform<F4>: the 4x4 output pixels, taps (ey + 1, ex + 1); every pixel of dz exactly once
  std::vector<int> owned((size_t)N * H * W, 0);
  for (int m : ms)
    for (int tile = 0; tile < g.T; ++tile) {
      stores(M, m, tile, Mt, m_bytes, "dm");
      if (!real_tile(g, tile)) continue;
      int n, y0, x0;
      tile_origin<4>(g, tile, n, y0, x0);
      for (int ey = 0; ey < 4; ++ey)
        for (int ex = 0; ex < 4; ++ex) {
          const unsigned off = patch_offset(g, M, n, m, y0, x0, ey + 1, ex + 1);
          const int y = y0 + ey * d, x = x0 + ex * d;
          const bool inside = y < H && x < W;
          EXPECT(inside == (off != kOutside), "m=4 tile %d output (%d,%d): inside %d offset %u", tile, ey, ex, (int)inside, off);
          if (off == kOutside) continue;
          EXPECT((long long)off + 4 <= dz_bytes && off == 4u * (unsigned)(((n * M + m) * H + y) * W + x), "m=4 dz offset %u of %lld", off, dz_bytes);
          if (touch && (long long)off + 4 <= dz_bytes) ++Z[off];
          if (m == ms[0]) ++owned[(size_t)(n * H + y) * W + x];
        }
    }
  for (size_t i = 0; i < owned.size(); ++i) EXPECT(owned[i] == 1, "m=4 pixel %zu belongs to %d tiles", i, owned[i]);
  // ---- output_transform4 (forward / data gradient): per (m, real tile) 36 loads of y [36][M][T], and per in-image output one store
  // and one load of its word of the masks [M][w32] (relu_bits_pack forms the same word offsets from the pixel index); every element
  // of out and every pixel's bit exactly once, the padding tiles nothing
  {
    const int npix = N * H * W, w32 = (npix + 31) / 32;
    const long long y_bytes = m_bytes, out_bytes = dz_bytes, bits_bytes = 4ll * M * w32;
    std::vector<unsigned char> Y, O;
    std::vector<unsigned> bits;
    if (touch) {
      Y.assign(y_bytes, 0);
      O.assign(out_bytes, 0);
      bits.assign((size_t)M * w32, 0u);
    }
    for (int m : ms)
      for (int tile = 0; tile < g.T; ++tile) {
        if (!real_tile(g, tile)) continue;
        int n, y0, x0;
        tile_origin<4>(g, tile, n, y0, x0);
        for (int pt = 0; pt < 36; ++pt) {
          const unsigned off = point_offset(g, M, pt, m, tile);
          EXPECT((long long)off + 4 <= y_bytes && off % 4 == 0, "m=4 y offset %u of %lld", off, y_bytes);
          if (touch && (long long)off + 4 <= y_bytes) ++Y[off];
        }
        for (int ey = 0; ey < 4; ++ey)
          for (int ex = 0; ex < 4; ++ex) {
            const int y = y0 + ey * d, x = x0 + ex * d;
            if (!(y < H && x < W)) continue;                 // the kernel's `in`: an overhanging output stores nothing
            const int rem = y * W + x, pix = n * H * W + rem;
            const unsigned off = out_offset(g, M, n, m, rem);
            EXPECT((long long)off + 4 <= out_bytes && off == 4u * (unsigned)((n * M + m) * H * W + rem), "m=4 out offset %u of %lld", off, out_bytes);
            if (touch && (long long)off + 4 <= out_bytes) {
              EXPECT(O[off] == 0, "m=4 out offset %u written twice", off);
              O[off] = 1;
            }
            const unsigned boff = out_bits_offset(m, w32, pix);
            EXPECT((long long)boff + 4 <= bits_bytes && boff == 4u * (unsigned)(m * w32 + pix / 32), "m=4 bit word offset %u of %lld", boff, bits_bytes);
            if (touch && (long long)boff + 4 <= bits_bytes) {
              EXPECT(!(bits[boff / 4] >> (pix & 31) & 1u), "m=4 bit of pixel %d named twice", pix);
              bits[boff / 4] += 1u << (pix & 31);
            }
          }
      }
    if (touch) {
      for (long long i = 0; i < out_bytes; i += 4) EXPECT(O[i] == 1, "m=4 out offset %lld never written", i);
      for (int m = 0; m < M; ++m)
        for (int p = 0; p < w32 * 32; ++p)
          EXPECT((bits[(size_t)m * w32 + p / 32] >> (p & 31) & 1u) == (p < npix ? 1u : 0u), "m=4 bit %d of channel %d", p, m);
    }
  }
  if (touch) {
    for (long long i = 0; i < v_bytes; i += 4) EXPECT(V[i] == 1, "m=4 v offset %lld never written", i);
    for (long long i = 0; i < m_bytes; i += 4) EXPECT(Mt[i] == 1, "m=4 dm offset %lld never written", i);
  }
  if (say)
    std::printf("m=4 N=%d C=%d M=%d %dx%d d=%d: %d x %d tiles per image, T=%d (%d padding)%s\n", N, C, M, H, W, d, g.ay.tiles, g.ax.tiles,
                g.T, g.T - real, touch ? " (arrays touched)" : "");
}

int main() {
  // the shapes of tests/test_gpu_winograd.py, forward (C = Cin, M = Cout) and data gradient (swapped), and the layer4 conv2 of the step
  const int shapes[][6] = {{2, 32, 128, 9, 7, 4}, {1, 32, 128, 11, 13, 2}, {2, 16, 128, 10, 10, 1}, {1, 16, 128, 97, 97, 4},
                           {8, 512, 512, 97, 97, 4}};
  for (const auto& s : shapes) {
    check_shape(s[0], s[1], s[2], s[3], s[4], s[5]);
    if (s[1] != s[2]) check_shape(s[0], s[2], s[1], s[3], s[4], s[5]);
  }
  // a sweep of small maps and dilations: empty phases, one-tile phases, every parity of q
  for (int d = 1; d <= 5; ++d)
    for (int h = 1; h <= 12; ++h)
      for (int w = 1; w <= 12; w += 3) check_shape(1, 2, 3, h, w, d, false);
  const Geom big = make_geom(8, 97, 97, 4);
  if (big.ay.tiles != 49 || big.ax.tiles != 49 || big.T != 19208) {
    std::printf("FAIL: 8 x 97 x 97, d = 4 must give 49 x 49 tiles per image, 19208 in all\n");
    ++g_bad;
  }
  // F(4x4,3x3) weight gradient: the shapes of tests/test_gpu_winograd4_wgrad.py, the two layers of the step at 8 crops and at one, and
  // a sweep over dilations 1, 2, 4 and extents with every residue of q modulo 4, phases shorter than one tile included
  const long long bad2 = g_bad;
  const int shapes4[][6] = {{3, 128, 128, 8, 8, 1}, {2, 128, 128, 9, 11, 1}, {1, 128, 256, 17, 19, 2}, {1, 256, 128, 33, 35, 4},
                            {1, 128, 128, 5, 7, 2}, {1, 256, 256, 17, 17, 2}, {2, 512, 512, 33, 33, 4}, {8, 256, 256, 97, 97, 2},
                            {8, 512, 512, 97, 97, 4}, {1, 512, 512, 97, 97, 4},
                            // tests/test_gpu_winograd4_conv.py, forward and data gradient (channel counts swapped)
                            {1, 16, 128, 9, 8, 1}, {1, 128, 16, 9, 8, 1}, {1, 32, 128, 17, 19, 1}, {1, 128, 32, 17, 19, 1},
                            {3, 48, 256, 21, 23, 2}, {3, 256, 48, 21, 23, 2}, {2, 64, 128, 33, 35, 4}, {2, 128, 64, 33, 35, 4}};
  for (const auto& s : shapes4) check_shape4(s[0], s[1], s[2], s[3], s[4], s[5]);
  const int extents[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 15, 16, 17, 19, 20, 21, 32, 33, 35, 97};
  for (int d : {1, 2, 4})
    for (int h : extents)
      for (int w : {5, 8, 17, 33, 97}) check_shape4(h % 2 + 1, 2, 3, h, w, d, false);
  const Geom big4 = make_geom<4>(8, 97, 97, 2), one4 = make_geom<4>(1, 97, 97, 4), pad4 = make_geom<4>(1, 17, 17, 2);
  if (big4.ay.tiles != 25 || big4.T != 5000 || one4.tiles_img != 625 || one4.T != 628 || pad4.tiles_img != 25 || pad4.T != 28) {
    std::printf("FAIL: 97 x 97 at dilation 2 or 4 must give 25 x 25 four-output tiles per image, one crop 628 with padding\n");
    ++g_bad;
  }
  std::printf("winograd index check, m = 4: %lld bad\n", g_bad - bad2);
  std::printf("winograd index check: %lld bad\n", g_bad);
  return g_bad ? 1 : 0;
}
