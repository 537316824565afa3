// Where in the image the errors are (dasac_boundary_counts): per mask layer the validation counts of dasac_mask_counts split by the
// Chebyshev distance of the pixel to the nearest class contour -- trimap / boundary-band IoU, its complement the interior IoU, and
// Boundary IoU (Cheng et al., 2021) all follow from one exact integer table per layer, int64 [R+1][5][C].  A diagnostic the
// reference does not have; include/dasac_hip.h has the full definitions.
//
// A map is one label per pixel; a value inside [0, C) is a class, every other value is "no class" and transparent: never a
// contour, never a cause of one.  d_L(p) of a class pixel p is the smallest max(|dy|, |dx|) to a pixel of the same image that
// holds a DIFFERENT class; slot = d - 1 for 1 <= d <= R, R otherwise.  Rows tp / fp / fn (dasac_mask_counts' rule) go to the slot
// of the pixel in the ground truth, row `pred` to its slot in the predicted map, row `both` (prediction == ground truth) to the
// larger of the two.
//
// Two kernels on the stream, the first of the file's kind that is not a pure streaming pass:
//   boundary_prepare   streaming (the shape of validation.hip: four consecutive pixels per thread, every class plane ONE dwordx4
//                      load declared 4-byte aligned, the last 1..3 pixels of an image element by element): the scores are read ONCE
//                      and arg-maxed (first maximum wins) into u8 maps in the caller's workspace, int64 label maps and the ground truth
//                      are narrowed to u8 beside them (ground truth: class or 0x7f, bit 7 = equals ignore_index).  Every image
//                      starts at a multiple of 4 bytes there, so a thread stores its four codes as one dword.
//   boundary_stencil   one block per 32 x 64 tile of one image.  Per map: the tile plus an R-wide halo of the u8 map goes to LDS
//                      (pixels outside the image as "no class": the border is no contour and images do not see each other; no
//                      load leaves a tensor), then two separable passes.  ROW pass, per staged pixel (y', x): the class k1 of the
//                      nearest class pixel of its row, its distance d1, and the distance d2 of the nearest pixel of the row that
//                      holds a class other than k1 -- at most 2R + 2 byte reads, one packed dword out.  COLUMN pass, per tile pixel
//                      of class c: d = min over |dy| <= R of max(|dy|, c != k1 ? d1 : d2) at (y + dy, x), rows by ascending |dy|
//                      and no further than the best d so far: 2R + 1 dword reads at most, where a ring scan takes (2R + 1)^2.
//                      The ground truth goes first and its slots stay in registers for all layers; a u8 label map of the caller
//                      is staged from where it is.
//
// Counting: integer adds only -- u32 LDS adds into ONE layer's [R+1][5][C] histogram per block (at most three per pixel; a wave
// whose 64 lanes hold one key, the rule in an interior, adds once for all), then one u64 global add per non-zero bin per block
// and layer.  Exact, and the same bits on every run whatever order the tiles arrive in.
//
// Cost (profiles/boundary_counts.md): the first kernel moves mask_counts' bytes at mask_counts' rate; the stencil is bound by
// instruction issue, not by memory -- the byte-wise row scan and the column scan of a tile, per map -- and grows with R.
//
// LDS: dynamic, sized by R and C: histogram + row table (32 + 2R) x 64 dwords + staged bytes (32 + 2R) x (64 + 2R): 19 KB at
// R = 8, C = 19; 43 KB at the limits R = 16, C = 64.  Registers: eight pixels per thread (ground-truth code and slot each); C = 19
// is compiled into the arg-max.  No scratch, <= 128 VGPRs.
#include "count_split.hpp"
#include "count_stream.hpp"

namespace dasac {

constexpr int kBdBlock = kCountBlock;
constexpr int kBdWaves = kBdBlock / kWave;
constexpr int kBdScores = kCountScores, kBdMaps = kCountMaps, kBdLayers = kBdScores + kBdMaps;
constexpr int kBdMaxRadius = DASAC_BOUNDARY_MAX_RADIUS;
constexpr int kBdMaxC = 64;
constexpr int kBdRowsOut = 5;                          // tp, fp, fn, pred, both
constexpr int kBdTileW = kWave, kBdTileH = 32;         // a wave is one row of the tile
constexpr int kBdOwn = kBdTileH / kBdWaves;            // pixels per thread: rows wave, wave + 4, ...
constexpr int kBdNone = 0x7f;                          // "no class" in a u8 map of the workspace
constexpr int kBdIgnored = 0x80;                       // ground-truth code: the pixel equals ignore_index
constexpr int kBdStage = 8;                            // byte loads a thread keeps in flight while it stages a tile
constexpr int kBdBlocksPerCu = 8;

struct BdMapSet {                                      // by value; [0] = ground-truth codes, [1 + l] = layer l
  const uint8_t* p[1 + kBdLayers];
  int64_t image_stride[1 + kBdLayers];                 // bytes from one image to the next
};

// arg-max (first maximum wins, strict >) over the C planes at nx pixels from `lp` on, as four code bytes.  Not argmax_quad: a running
// maximum at every C -- with its 19 quads held at once beside the maps' codes this kernel takes 149 VGPRs instead of 95
template <int CT>
__device__ __forceinline__ unsigned bd_argmax4(const float* __restrict__ lp, int C, int64_t HW, int nx) {
  f32x4u best = load_quad(lp, nx);
  int arg[4] = {0, 0, 0, 0};
  if constexpr (CT > 0) {
#pragma unroll
    for (int c = 1; c < CT; ++c) {
      const f32x4u v = load_quad(lp + (int64_t)c * HW, nx);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e]) {
          best[e] = v[e];
          arg[e] = c;
        }
    }
  } else {
    for (int c = 1; c < C; ++c) {
      const f32x4u v = load_quad(lp + (int64_t)c * HW, nx);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e]) {
          best[e] = v[e];
          arg[e] = c;
        }
    }
  }
  unsigned code = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) code |= (unsigned)(e < nx ? arg[e] : kBdNone) << (8 * e);
  return code;
}

// grid: B * blocks_per_image blocks; block (b, j) takes quads [j * per, (j + 1) * per) of image b (quad = 4 consecutive pixels).
// ws: maps of `map_stride` bytes (0 the ground truth, 1 + l score layer l, 1 + ns + l int64 map l), images `HWp` (a multiple of 4) bytes
// apart: a quad is one aligned dword, also the last of an image
template <int CT>
__global__ __launch_bounds__(kBdBlock) void boundary_prepare(const CountLayers src, int ns, int nm, const int64_t* __restrict__ gt,
                                                             int Crt, int64_t HW, int64_t HWp, int64_t map_stride,
                                                             int blocks_per_image, int64_t per, int64_t ignore_index,
                                                             uint8_t* __restrict__ ws) {
  const int C = CT > 0 ? CT : Crt;
  const int64_t b = blockIdx.x / (unsigned)blocks_per_image;
  const int j = (int)(blockIdx.x - b * blocks_per_image);
  const int64_t n_quads = (HW + 3) >> 2;
  const int64_t q0 = j * per;
  int64_t q1 = q0 + per;
  if (q1 > n_quads) q1 = n_quads;

  for (int64_t q = q0 + threadIdx.x; q < q1; q += kBdBlock) {
    const int64_t r = q << 2;
    const int nx = HW - r >= 4 ? 4 : (int)(HW - r);    // 1..4: r < HW because q < ceil(HW / 4)
    uint8_t* out = ws + b * HWp + r;                   // r + 4 <= HWp
    int64_t g[4];
    load_quad(gt + b * HW + r, nx, -1, g);             // past nx: no class
    unsigned code = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned cls = (g[e] >= 0 && g[e] < C) ? (unsigned)g[e] : (unsigned)kBdNone;
      const unsigned ign = (e < nx && g[e] == ignore_index) ? (unsigned)kBdIgnored : 0u;
      code |= (cls | ign) << (8 * e);
    }
    *reinterpret_cast<unsigned*>(out) = code;
#pragma unroll
    for (int l = 0; l < kBdScores; ++l)
      if (l < ns)
        *reinterpret_cast<unsigned*>(out + (1 + l) * map_stride) = bd_argmax4<CT>(src.s[l] + b * C * HW + r, C, HW, nx);
#pragma unroll
    for (int l = 0; l < kBdMaps; ++l)
      if (l < nm) {
        load_quad(static_cast<const int64_t*>(src.m[l]) + b * HW + r, nx, -1, g);
        code = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) code |= ((g[e] >= 0 && g[e] < C) ? (unsigned)g[e] : (unsigned)kBdNone) << (8 * e);
        *reinterpret_cast<unsigned*>(out + (1 + ns + l) * map_stride) = code;
      }
  }
}

// one key per lane into the block's histogram; a negative key adds nothing.  A wave is one row of the tile: in an interior all its
// lanes hold ONE key, which one lane adds for all (64 adds at one address would take 64 LDS cycles); next to a contour the keys
// differ from lane to lane and every lane adds its own -- cheaper there than one round of the match loop of count_add4 per key
__device__ __forceinline__ void bd_add(unsigned int* __restrict__ h, int key) {
  if (key >= 0) {
    const int lead = __builtin_amdgcn_readfirstlane(key);
    const unsigned long long same = __ballot(key == lead), active = __ballot(true);
    if (same == active) {
      if ((int)(threadIdx.x & (kWave - 1)) == __ffsll((long long)same) - 1) atomicAdd(&h[lead], (unsigned)__popcll(same));
    } else {
      atomicAdd(&h[key], 1u);
    }
  }
}

// slot of the tile pixel (y, x) of class `cls` from the row table (entries k1 | d1 << 8 | d2 << 16, row y of the tile at y + R)
__device__ __forceinline__ int bd_slot(const unsigned int* __restrict__ tab, int y, int x, int cls, int R) {
  if (cls == kBdNone) return R;
  const unsigned int* col = tab + (y + R) * kBdTileW + x;
  int d = R + 1;
  for (int a = 0; a <= R && a < d; ++a) {              // rows further than the best distance so far can not improve it
    unsigned e = col[-a * kBdTileW];
    int rd = (int)(e & 0xffu) != cls ? (int)((e >> 8) & 0xffu) : (int)((e >> 16) & 0xffu);
    rd = rd > a ? rd : a;
    d = rd < d ? rd : d;
    if (a) {
      e = col[a * kBdTileW];
      rd = (int)(e & 0xffu) != cls ? (int)((e >> 8) & 0xffu) : (int)((e >> 16) & 0xffu);
      rd = rd > a ? rd : a;
      d = rd < d ? rd : d;
    }
  }
  return d <= R ? d - 1 : R;
}

// grid: B * tiles_y * tiles_x blocks, x fastest.  dynamic LDS: bd_lds_bytes(R, C)
__global__ __launch_bounds__(kBdBlock) void boundary_stencil(const BdMapSet maps, int n_layers, int C, int H, int W, int R,
                                                             int tiles_x, int tiles_y, FastDiv div_pitch,
                                                             unsigned long long* __restrict__ table) {
  extern __shared__ unsigned int s_bd[];
  const int n_bins = (R + 1) * kBdRowsOut * C;
  const int rows = kBdTileH + 2 * R, pitch = kBdTileW + 2 * R;     // staged rows, staged bytes per row
  unsigned int* hist = s_bd;
  unsigned int* tab = hist + n_bins;                               // [rows][kBdTileW]
  uint8_t* raw = reinterpret_cast<uint8_t*>(tab + rows * kBdTileW);  // [rows][pitch]
  for (int i = threadIdx.x; i < n_bins; i += kBdBlock) hist[i] = 0;

  unsigned t = blockIdx.x;
  const int tx = (int)(t % (unsigned)tiles_x);
  t /= (unsigned)tiles_x;
  const int ty = (int)(t % (unsigned)tiles_y);
  const int64_t b = t / (unsigned)tiles_y;
  const int x0 = tx * kBdTileW, y0 = ty * kBdTileH;
  const int lane = (int)(threadIdx.x & (kWave - 1)), wave = (int)(threadIdx.x >> 6);
  const bool in_x = x0 + lane < W;

  int g_code[kBdOwn], g_slot[kBdOwn];                  // the ground truth of this thread's pixels, for all layers

  for (int m = 0; m <= n_layers; ++m) {
    // stage the tile and its halo; outside the image: no class
    const uint8_t* img = maps.p[m] + b * maps.image_stride[m];
    for (int i0 = threadIdx.x; i0 < rows * pitch; i0 += kBdStage * kBdBlock) {
      int v[kBdStage];                                 // kBdStage loads in flight per thread, then their LDS stores
#pragma unroll
      for (int k = 0; k < kBdStage; ++k) {
        const int i = i0 + k * kBdBlock;
        const int yy = fdiv(i, div_pitch), xx = i - yy * pitch;
        const int gy = y0 - R + yy, gx = x0 - R + xx;
        v[k] = kBdNone;
        if (i < rows * pitch && gy >= 0 && gy < H && gx >= 0 && gx < W) v[k] = img[(int64_t)gy * W + gx];
      }
#pragma unroll
      for (int k = 0; k < kBdStage; ++k) {
        const int i = i0 + k * kBdBlock;
        if (m > 0) v[k] = v[k] < C ? v[k] : kBdNone;   // a caller's u8 map: 255 and anything out of range
        if (i < rows * pitch) raw[i] = (uint8_t)v[k];
      }
    }
    __syncthreads();

    // row pass: a wave takes one staged row at a time
    for (int i = threadIdx.x; i < rows * kBdTileW; i += kBdBlock) {
      const int yy = i >> 6;
      const int gy = y0 - R + yy;
      int k1 = kBdNone, d1 = R + 1, d2 = R + 1;
      if (gy >= 0 && gy < H) {                         // the same for the whole wave
        const uint8_t* c = raw + yy * pitch + R + lane;
        for (int dx = 0; dx <= R && d2 > R; ++dx) {
          const int left = c[-dx] & kBdNone, right = c[dx] & kBdNone;
          if (left != kBdNone) {
            if (k1 == kBdNone) {
              k1 = left;
              d1 = dx;
            } else if (left != k1) {
              d2 = dx;
            }
          }
          if (right != kBdNone) {
            if (k1 == kBdNone) {
              k1 = right;
              d1 = dx;
            } else if (right != k1 && d2 > R) {
              d2 = dx;
            }
          }
        }
      }
      tab[i] = (unsigned)k1 | ((unsigned)d1 << 8) | ((unsigned)d2 << 16);
    }
    __syncthreads();

    // column pass and counting: this thread's pixels (wave + 4 i, lane)
    if (m == 0) {
#pragma unroll
      for (int i = 0; i < kBdOwn; ++i) {
        const int y = wave + kBdWaves * i;
        const int code = raw[(y + R) * pitch + R + lane];
        const bool inside = in_x && y0 + y < H;
        g_code[i] = inside ? code : kBdIgnored | kBdNone;          // outside the image: counts nothing
        g_slot[i] = bd_slot(tab, y, lane, code & kBdNone, R);
      }
    } else {
#pragma unroll
      for (int i = 0; i < kBdOwn; ++i) {
        const int y = wave + kBdWaves * i;
        const int a = raw[(y + R) * pitch + R + lane];
        const int sa = bd_slot(tab, y, lane, a, R);
        const int gc = g_code[i] & kBdNone, sg = g_slot[i];
        const bool counted = !(g_code[i] & kBdIgnored);
        const bool hit = a == gc && a != kBdNone;
        const int base_g = sg * kBdRowsOut * C, base_a = sa * kBdRowsOut * C;
        // a pixel adds at most three times: tp[g] or fp[a]; both[a] (a hit) or fn[g] (a miss); pred[a]
        bd_add(hist, !counted ? -1 : hit ? base_g + gc : a != kBdNone ? base_g + C + a : -1);
        bd_add(hist, !counted ? -1 : hit ? (sg > sa ? base_g : base_a) + 4 * C + a : gc != kBdNone ? base_g + 2 * C + gc : -1);
        bd_add(hist, (!counted || a == kBdNone) ? -1 : base_a + 3 * C + a);
      }
    }
    __syncthreads();                                   // raw and tab are free again; the layer's histogram is complete
    if (m > 0) {
      unsigned long long* out = table + (int64_t)(m - 1) * n_bins;
      for (int i = threadIdx.x; i < n_bins; i += kBdBlock) {
        const unsigned v = hist[i];
        if (v) {
          atomicAdd(&out[i], (unsigned long long)v);
          hist[i] = 0;                                 // two barriers before the next layer counts
        }
      }
    }
  }
}

inline size_t bd_lds_bytes(int R, int C) {
  const size_t rows = kBdTileH + 2 * R, pitch = kBdTileW + 2 * R;
  return ((size_t)(R + 1) * kBdRowsOut * C + rows * kBdTileW) * sizeof(unsigned int) + align_up(rows * pitch, 4);
}

// bytes of one u8 map of the workspace, and from one image to the next in it
inline int64_t bd_image_bytes(int H, int W) { return ((int64_t)H * W + 3) / 4 * 4; }
inline int64_t bd_map_bytes(int B, int H, int W) { return (B * bd_image_bytes(H, W) + 15) / 16 * 16; }

}  // namespace dasac

// one map per non-NULL slot and one for the ground truth: an upper bound -- a uint8 label map is staged from where it is and takes
// no map (the call itself checks ws_bytes against the maps it writes), so the caller need not know the slots' types to size it
extern "C" size_t dasac_boundary_counts_workspace(int layers, int B, int H, int W) {
  using namespace dasac;
  if (layers < 0 || layers > kBdLayers || B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)(layers + 1) * (size_t)bd_map_bytes(B, H, W);
}

extern "C" int dasac_boundary_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                                     const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C,
                                     int H, int W, int R, int ignore_index, int64_t* table, void* workspace, size_t ws_bytes,
                                     dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(gt && table && workspace, "boundary_counts: null gt, table or workspace");
  DASAC_REQUIRE(B > 0 && H > 0 && W > 0, "boundary_counts: B, H and W must be positive");
  DASAC_REQUIRE(C >= 1 && C <= kBdMaxC, "boundary_counts: C must be in 1..%d", kBdMaxC);
  DASAC_REQUIRE(R >= 1 && R <= kBdMaxRadius, "boundary_counts: R must be in 1..%d", kBdMaxRadius);
  CountLayers src;
  BdMapSet maps = {};
  const int64_t HW = (int64_t)H * W, HWp = bd_image_bytes(H, W), map_stride = bd_map_bytes(B, H, W);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int ns, nm;
  const bool aligned = gather_count_layers(scores0, scores1, scores2, scores3, labels0, labels1, labels_u8_mask, src, ns, nm) &&
                       ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(table)) & 7u) == 0 &&
                       (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0;
  int n_maps = 0, n_ws = 0, n64 = 0;
  auto add_map = [&](const uint8_t* p, int64_t image_stride) {
    maps.p[n_maps] = p;
    maps.image_stride[n_maps++] = image_stride;
  };
  add_map(ws + n_ws++ * map_stride, HWp);              // workspace map 0 is the ground truth, 1 + l score layer l
  for (int l = 0; l < ns; ++l) add_map(ws + n_ws++ * map_stride, HWp);
  for (int l = 0; l < nm; ++l)
    if (src.u8[l]) {                                   // staged from where it is, any address
      add_map(static_cast<const uint8_t*>(src.m[l]), HW);
    } else {                                           // boundary_prepare sees the int64 maps alone: map n64 to workspace map 1 + ns + n64
      src.m[n64++] = src.m[l];
      add_map(ws + n_ws++ * map_stride, HWp);
    }
  nm = n64;
  const int n_layers = n_maps - 1;
  DASAC_REQUIRE(n_layers > 0, "boundary_counts: no layer");
  DASAC_REQUIRE(aligned, "boundary_counts: fp32 / int64 tensors must be aligned to their element size, the workspace to 16 bytes");
  DASAC_REQUIRE(ws_bytes >= (size_t)n_ws * (size_t)map_stride, "boundary_counts: workspace too small (%zu < %zu)", ws_bytes,
                (size_t)n_ws * (size_t)map_stride);
  const int tiles_x = (W + kBdTileW - 1) / kBdTileW, tiles_y = (H + kBdTileH - 1) / kBdTileH;
  DASAC_REQUIRE((int64_t)tiles_x * tiles_y * B <= 0x7fffffffll, "boundary_counts: B * H * W too large for one launch");
  // the streaming pass keeps no u32 bins: no limit on a block's quads
  const QuadSplit split = quad_split((HW + 3) >> 2, B, kNumCu - reserved_cus(), kBdBlocksPerCu, 4, kBdBlock);
  const int64_t bpi = split.blocks_per_image, per = split.quads_per_block;
  DASAC_REQUIRE(bpi * B <= 0x7fffffffll, "boundary_counts: B * H * W too large for one launch");
  hipStream_t s = as_stream(stream);
  if (C == 19) {
    hipLaunchKernelGGL((boundary_prepare<19>), dim3((unsigned)(bpi * B)), dim3(kBdBlock), 0, s, src, ns, nm, gt, C, HW, HWp,
                       map_stride, (int)bpi, per, (int64_t)ignore_index, ws);
  } else {
    hipLaunchKernelGGL((boundary_prepare<0>), dim3((unsigned)(bpi * B)), dim3(kBdBlock), 0, s, src, ns, nm, gt, C, HW, HWp,
                       map_stride, (int)bpi, per, (int64_t)ignore_index, ws);
  }
  DASAC_CHECK_LAUNCH("boundary_prepare");
  hipLaunchKernelGGL(boundary_stencil, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(kBdBlock), bd_lds_bytes(R, C), s, maps, n_layers, C,
                     H, W, R, tiles_x, tiles_y, fast_div(kBdTileW + 2 * R), reinterpret_cast<unsigned long long*>(table));
  DASAC_CHECK_LAUNCH("boundary_stencil");
  return DASAC_OK;
}
