// On which OBJECTS the errors are: connected-component labelling of a label map on the device (dasac_label_segments), the exact
// size-stratified segment tables built on it (dasac_segment_counts) and the removal of specks below a size (dasac_segment_filter).
// A diagnostic the reference does not have; include/dasac_hip.h has the full definitions.
//
// A map is one label per pixel; a value inside [0, C) is a class, every other value (255, -1, out of range) is "no class".  Two
// pixels of one image are adjacent under connectivity 4 when they share an edge, under connectivity 8 when they share an edge or a
// corner.  A segment is a maximal set of pixels of one class connected through adjacent pixels of that class; no-class pixels belong
// to no segment; the images of a batch do not see each other, and a run that ends at the right edge of row y is not adjacent to one
// that starts at the left edge of row y + 1.  A segment's root is the smallest y * W + x among its pixels, its size its pixel count,
// its bin min(floor(log2(size)), DASAC_SEGMENT_BINS - 1).
//
// Union-find with the ONE invariant parent[p] <= p, kept at all times: a set's root is then its smallest index -- canonical by
// construction, whatever order the unions arrive in -- and every chase descends along strictly decreasing indices, so it is bounded.
// A union links the larger root below the smaller one with an atomic min and goes on with the value that min RETURNED: each retry
// holds a strictly smaller pair.  No loop waits for another workgroup: no spin, no flag, no grid barrier; a phase that needs another
// phase's results is another launch.  Per map, a fixed number of launches:
//   seg_local      one block per 32 x 64 tile: the tile's class bytes go to LDS (int64 narrowed, uint8 byte by byte from any address;
//                  outside the image: no class), parents are LOCAL indices in LDS; every pixel is united with its left and upper
//                  neighbours (under connectivity 8 with the two upper diagonals when the pixel above holds another class -- when it
//                  holds the same, it links them already); then every pixel writes the IMAGE index of its local root.
//   seg_merge      border pixels only (segments_index.hpp lists them): unions across the tile seams on the image-wide parents.
//                  Other workgroups write those concurrently, so parents are READ with relaxed agent-scope atomic loads (a plain
//                  load may be served stale from the CU's L1) and WRITTEN with agent-scope atomic mins; the only decision that ends
//                  a union by linking rests on what the atomic min returned, and "both ends reached one root" is true of any two
//                  chains of links ever observed, fresh or stale: a stale read costs steps, never a wrong union.  Chases halve
//                  their path (an atomic min of the grandparent: still <=, still the same set).
//   seg_resolve    after the kernel boundary plain loads are fine: every pixel chases to its root and writes it in place of its
//                  parent (other chasers meet either value, both lead down to the root), and adds 1 to the int32 counter at the
//                  root -- one add per wave and DISTINCT root among its lanes.  For a layer of dasac_segment_counts the same pass
//                  adds the per-segment n and m counters of both sides at their roots.
//   seg_tabulate   (dasac_segment_counts) the root pixels of both sides bin their segment and add its four rows to a per-block u32
//                  LDS histogram (a block stays inside one image, whose segments' pixels sum to H * W < 2^32), then one u64 global
//                  add per non-zero cell.
//   seg_broadcast / seg_filter_apply   every pixel reads the count at its root.
// dasac_segment_counts first arg-maxes the score layers (first maximum wins) into u8 maps and narrows the ground truth to a code
// byte (class or 0x7f, bit 7 = equals ignore_index) in the workspace: seg_prepare, the quad-streaming shape of count_stream.hpp.
//
// Integer adds only; no floating-point atomics.  No load or store leaves a tensor or the workspace: uint8 maps are read and written
// byte by byte, int64 / int32 tensors element by element.  LDS: 10 KB static in seg_local; dynamic 768 * C bytes in seg_tabulate
// (48 KB at C = 64).  No scratch, <= 128 VGPRs.
#include "count_split.hpp"
#include "count_stream.hpp"
#include "segments_index.hpp"

namespace dasac {

static_assert(seg::kBins == DASAC_SEGMENT_BINS, "segments_index.hpp and dasac_hip.h disagree on the bins");

constexpr int kSegBlock = kCountBlock;
constexpr int kSegOwn = seg::kTilePixels / kSegBlock;  // tile pixels per thread
constexpr int kSegNone = 0xff;                         // "no class" among the staged class bytes
constexpr int kSegCodeNone = 0x7f, kSegCodeIgnored = 0x80;   // ground-truth code byte of the workspace
constexpr int kSegRows = 4;                            // segments, pixels, matched pixels, matched segments
constexpr int kSegMaxC = 255, kSegCountMaxC = 64;
constexpr int kSegBlocksPerCu = 8;
enum { kSegI64 = 0, kSegU8 = 1, kSegGtCode = 2 };

struct SegSrc {                                        // by value: where a map's labels are read from
  const void* p;
  int64_t image_stride;                                // elements from one image to the next
  int kind;
};

// class of pixel i of image b: [0, C) or kSegNone
__device__ __forceinline__ int seg_class(const SegSrc& s, int64_t b, int64_t i, int C) {
  if (s.kind == kSegI64) {
    const int64_t v = static_cast<const int64_t*>(s.p)[b * s.image_stride + i];
    return (v >= 0 && v < C) ? (int)v : kSegNone;
  }
  int v = static_cast<const uint8_t*>(s.p)[b * s.image_stride + i];
  if (s.kind == kSegGtCode && (v & kSegCodeIgnored)) v = kSegNone;   // an ignored pixel is no class in the ground-truth map
  return v < C ? v : kSegNone;                         // kSegCodeNone >= C: C <= 64 where codes are read
}

#define DASAC_SEG_LOAD(ptr, scope) __hip_atomic_load(ptr, __ATOMIC_RELAXED, scope)

// Root of x while other threads unite (SCOPE: workgroup for LDS parents, agent for the image-wide ones).  Descends while the parent
// is a smaller, valid index: bounded by x whatever it reads.  HALVE: x's parent becomes its grandparent (x is no root: a parent
// below it was read, and parents only ever decrease)
template <int SCOPE, bool HALVE>
__device__ __forceinline__ int seg_find(int* par, int x) {
  int p = DASAC_SEG_LOAD(par + x, SCOPE);
  while ((unsigned)p < (unsigned)x) {
    const int gp = DASAC_SEG_LOAD(par + p, SCOPE);
    if (HALVE && (unsigned)gp < (unsigned)p) __hip_atomic_fetch_min(par + x, gp, __ATOMIC_RELAXED, SCOPE);
    x = p;
    p = gp;
  }
  return x;
}

// Unites the sets of a and b.  Every trip either ends or goes on with a pair whose larger member is strictly smaller: the min at the
// larger root a returned either a itself (a WAS a root at that moment and now hangs below b: done) or a smaller parent another
// thread gave it meanwhile, with which the union goes on (whichever of the two links the min did not keep is made again there)
template <int SCOPE, bool HALVE>
__device__ __forceinline__ void seg_union(int* par, int a, int b) {
  for (;;) {
    a = seg_find<SCOPE, HALVE>(par, a);
    b = seg_find<SCOPE, HALVE>(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old >= a) return;                              // == a: linked.  (> a never happens: parent[a] <= a)
    a = old;
  }
}

// grid: B * tiles_y * tiles_x blocks, x fastest.  Writes parent[b][y][x] for every pixel of the image (-1: no class) and zeroes the
// pixel's entry of the counter maps z0..z2 (NULL: none)
__global__ __launch_bounds__(kSegBlock) void seg_local(const SegSrc src, int C, int H, int W, int conn8, int tiles_x, int tiles_y,
                                                       int* __restrict__ parent, int* __restrict__ z0, int* __restrict__ z1,
                                                       int* __restrict__ z2) {
  __shared__ int s_par[seg::kTilePixels];
  __shared__ uint8_t s_cls[seg::kTilePixels];
  unsigned t = blockIdx.x;
  const int tx = (int)(t % (unsigned)tiles_x);
  t /= (unsigned)tiles_x;
  const int ty = (int)(t % (unsigned)tiles_y);
  const int64_t b = t / (unsigned)tiles_y;
  const int x0 = tx * seg::kTileW, y0 = ty * seg::kTileH;
  const int64_t HW = (int64_t)H * W;

#pragma unroll
  for (int k = 0; k < kSegOwn; ++k) {
    const int li = threadIdx.x + k * kSegBlock;
    const int gy = y0 + li / seg::kTileW, gx = x0 + li % seg::kTileW;
    s_cls[li] = (uint8_t)((gy < H && gx < W) ? seg_class(src, b, (int64_t)gy * W + gx, C) : kSegNone);
    s_par[li] = li;
  }
  __syncthreads();
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  for (int k = 0; k < kSegOwn; ++k) {
    const int li = threadIdx.x + k * kSegBlock;
    const int ly = li / seg::kTileW, lx = li % seg::kTileW;
    const int c = s_cls[li];
    if (c == kSegNone) continue;
    if (lx > 0 && s_cls[li - 1] == c) seg_union<WG, false>(s_par, li, li - 1);
    if (ly > 0) {
      if (s_cls[li - seg::kTileW] == c) {
        seg_union<WG, false>(s_par, li, li - seg::kTileW);
      } else if (conn8) {
        if (lx > 0 && s_cls[li - seg::kTileW - 1] == c) seg_union<WG, false>(s_par, li, li - seg::kTileW - 1);
        if (lx + 1 < seg::kTileW && s_cls[li - seg::kTileW + 1] == c) seg_union<WG, false>(s_par, li, li - seg::kTileW + 1);
      }
    }
  }
  __syncthreads();                                     // all unions done: the finds below only read
  for (int k = 0; k < kSegOwn; ++k) {
    const int li = threadIdx.x + k * kSegBlock;
    const int gy = y0 + li / seg::kTileW, gx = x0 + li % seg::kTileW;
    if (gy < H && gx < W) {
      const int64_t at = b * HW + (int64_t)gy * W + gx;
      parent[at] = s_cls[li] == kSegNone ? -1 : seg::local_to_image(y0, x0, seg_find<WG, false>(s_par, li), W);
      if (z0) z0[at] = 0;
      if (z1) z1[at] = 0;
      if (z2) z2[at] = 0;
    }
  }
}

// grid-stride over the B * items border items
__global__ __launch_bounds__(kSegBlock) void seg_merge(const SegSrc src, int C, int H, int W, int connectivity, int64_t items,
                                                       int64_t total, int* parent) {
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  const int64_t HW = (int64_t)H * W;
  for (int64_t t = (int64_t)blockIdx.x * kSegBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kSegBlock) {
    const int64_t b = t / items;
    int y, x, nb[3];
    const bool vertical = seg::border_pixel(t - b * items, H, W, y, x);
    const int at = y * W + x;
    const int c = seg_class(src, b, at, C);
    if (c == kSegNone) continue;
    const int n = seg::border_neighbours(y, x, vertical, H, W, connectivity, nb);
#pragma unroll
    for (int k = 0; k < 3; ++k)                        // unrolled: nb stays in registers
      if (k < n && seg_class(src, b, nb[k], C) == c) seg_union<AG, true>(parent + b * HW, at, nb[k]);
  }
}

// after a kernel boundary: plain loads.  Bounded like seg_find
__device__ __forceinline__ int seg_chase(const int* par, int x) {
  int p = par[x];
  while ((unsigned)p < (unsigned)x) {
    x = p;
    p = par[x];
  }
  return x;
}

// All 64 lanes of the wave call together: for each k < K adds the number of lanes with pred[k] to cnt[k][root] (root < 0: nothing).
// One trip per DISTINCT root among the wave's lanes, each trip one add per counter by one lane for all lanes that hold the root:
// inside a region that is one trip, and a large segment with specks in it costs its root one add per wave and counter, not one
// per pixel (64 lanes adding to one address serialise; a million of them is what an image-wide segment would make)
template <int K>
__device__ __forceinline__ void seg_add(int* const (&cnt)[K], int root, const bool (&pred)[K]) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  unsigned long long todo = __ballot(root >= 0);
  while (todo) {                                       // wave-uniform: every trip clears at least the leading lane's bit
    const int first = __ffsll((long long)todo) - 1;
    const int lead = __builtin_amdgcn_readlane(root, first);
    const bool mine = root == lead;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned long long m = __ballot(mine && pred[k]);
      if (m != 0 && lane == first && cnt[k]) atomicAdd(&cnt[k][lead], (int)__popcll(m));
    }
    todo &= ~__ballot(mine);
  }
}

struct SegLayerArgs {                                  // what seg_resolve<true> counts beside the layer's segment sizes
  SegSrc layer;
  const uint8_t* gt_code;                              // images gt_stride bytes apart
  int64_t gt_stride;
  const int* gt_root;                                  // the ground truth's resolved roots
  int *gt_m, *n, *m;                                   // counters at the ground-truth root / at the layer's root
  int C;
};

// grid: B * bpi blocks; block (b, j) strides over image b.  parent -> roots in place; size (NULL: not counted) += 1 at the root
template <bool LAYER>
__global__ __launch_bounds__(kSegBlock) void seg_resolve(int* parent, int* __restrict__ size, int64_t HW, int bpi,
                                                         const SegLayerArgs a) {
  const int64_t b = blockIdx.x / (unsigned)bpi;
  const int j = (int)(blockIdx.x - b * bpi);
  int* par = parent + b * HW;
  for (int64_t i0 = (int64_t)j * kSegBlock; i0 < HW; i0 += (int64_t)bpi * kSegBlock) {    // the same trips for the whole block
    const int64_t i = i0 + threadIdx.x;
    int root = -1;
    if (i < HW && par[i] >= 0) {
      root = seg_chase(par, (int)i);
      par[i] = root;
    }
    if constexpr (LAYER) {
      int gt_root = -1;
      bool counted = false, hit = false;
      if (i < HW) {
        const int code = a.gt_code[b * a.gt_stride + i];
        counted = !(code & kSegCodeIgnored);
        hit = counted && root >= 0 && seg_class(a.layer, b, i, a.C) == (code & kSegCodeNone);   // a class: the layer's pixel holds one
        gt_root = a.gt_root[b * HW + i];
      }
      int* const at_root[3] = {size + b * HW, a.n + b * HW, a.m + b * HW};
      seg_add(at_root, root, {true, counted, hit});
      int* const at_gt_root[1] = {a.gt_m + b * HW};
      seg_add(at_gt_root, gt_root, {hit});
    } else {
      int* const at_root[1] = {size ? size + b * HW : nullptr};
      if (size) seg_add(at_root, root, {true});
    }
  }
}

// size[p] = size[root of p] for every pixel that is no root (roots hold their count already, no-class pixels their 0)
__global__ __launch_bounds__(kSegBlock) void seg_broadcast(const int* __restrict__ segment, int* size, int64_t HW, int bpi) {
  const int64_t b = blockIdx.x / (unsigned)bpi;
  const int j = (int)(blockIdx.x - b * bpi);
  for (int64_t i = (int64_t)j * kSegBlock + threadIdx.x; i < HW; i += (int64_t)bpi * kSegBlock) {
    const int r = segment[b * HW + i];
    if (r >= 0 && r != i) size[b * HW + i] = size[b * HW + r];       // only roots are read, only other pixels written
  }
}

// out = labels, but `fill` where the pixel's segment is smaller than min_size (min_size <= 1: a copy; roots and size are not read)
template <typename T>
__global__ __launch_bounds__(kSegBlock) void seg_filter_apply(const T* __restrict__ labels, const int* __restrict__ root,
                                                              const int* __restrict__ size, int64_t HW, int bpi, int min_size, T fill,
                                                              T* __restrict__ out) {
  const int64_t b = blockIdx.x / (unsigned)bpi;
  const int j = (int)(blockIdx.x - b * bpi);
  for (int64_t i = (int64_t)j * kSegBlock + threadIdx.x; i < HW; i += (int64_t)bpi * kSegBlock) {
    T v = labels[b * HW + i];
    if (min_size > 1) {
      const int r = root[b * HW + i];
      if (r >= 0 && size[b * HW + r] < min_size) v = fill;
    }
    out[b * HW + i] = v;
  }
}

// grid: B * bpi blocks; block (b, j) takes quads of image b.  ws: map 0 the ground-truth codes, map 1 + l score layer l, `map_stride`
// bytes apart, images HWp (a multiple of 4) bytes apart: a quad is one aligned dword, also the last of an image
__global__ __launch_bounds__(kSegBlock) void seg_prepare(const CountLayers src, int ns, const int64_t* __restrict__ gt, int C, int64_t HW,
                                                         int64_t HWp, int64_t map_stride, int bpi, int64_t ignore_index,
                                                         uint8_t* __restrict__ ws) {
  const int64_t b = blockIdx.x / (unsigned)bpi;
  const int j = (int)(blockIdx.x - b * bpi);
  const int64_t n_quads = (HW + 3) >> 2;
  for (int64_t q = (int64_t)j * kSegBlock + threadIdx.x; q < n_quads; q += (int64_t)bpi * kSegBlock) {
    const int64_t r = q << 2;
    const int nx = HW - r >= 4 ? 4 : (int)(HW - r);
    uint8_t* out = ws + b * HWp + r;                   // r + 4 <= HWp
    int64_t g[4];
    load_quad(gt + b * HW + r, nx, -1, g);
    unsigned code = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned cls = (g[e] >= 0 && g[e] < C) ? (unsigned)g[e] : (unsigned)kSegCodeNone;
      const unsigned ign = (e < nx && g[e] == ignore_index) ? (unsigned)kSegCodeIgnored : 0u;
      code |= (cls | ign) << (8 * e);
    }
    *reinterpret_cast<unsigned*>(out) = code;
    for (int l = 0; l < ns; ++l) {
      int p[4];
      argmax_quad<0>(src.s[l] + b * C * HW, C, HW, r, nx, p);
      code = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) code |= (unsigned)(e < nx ? p[e] : kSegCodeNone) << (8 * e);
      *reinterpret_cast<unsigned*>(out + (1 + l) * map_stride) = code;
    }
  }
}

struct SegSide {                                       // resolved roots and the counters at them
  const int* root;
  const int *size, *n, *m;
};

// grid: B * bpi blocks.  dynamic LDS: 2 * kBins * kSegRows * C u32.  Side 0 = the ground truth's segments (n unused: every pixel of
// one is counted; its m is zeroed again for the next layer), side 1 = the layer's
__global__ __launch_bounds__(kSegBlock) void seg_tabulate(const SegSide gt, int* __restrict__ gt_m, const uint8_t* __restrict__ gt_code,
                                                          int64_t gt_stride, const SegSide layer, const SegSrc layer_src, int C,
                                                          int64_t HW, int bpi, unsigned long long* __restrict__ table) {
  extern __shared__ unsigned int s_seg[];
  const int n_bins = 2 * seg::kBins * kSegRows * C;
  for (int i = threadIdx.x; i < n_bins; i += kSegBlock) s_seg[i] = 0;
  __syncthreads();
  const int64_t b = blockIdx.x / (unsigned)bpi;
  const int j = (int)(blockIdx.x - b * bpi);
  for (int64_t i = (int64_t)j * kSegBlock + threadIdx.x; i < HW; i += (int64_t)bpi * kSegBlock) {
    const int64_t at = b * HW + i;
    if (gt.root[at] == i) {
      const int c = gt_code[b * gt_stride + i] & kSegCodeNone, s = gt.size[at], m = gt_m[at];
      gt_m[at] = 0;
      unsigned int* cell = s_seg + (0 * seg::kBins + seg::bin_of(s)) * kSegRows * C + c;
      atomicAdd(cell, 1u);
      atomicAdd(cell + C, (unsigned)s);
      if (m) atomicAdd(cell + 2 * C, (unsigned)m);
      if (2 * (int64_t)m > s) atomicAdd(cell + 3 * C, 1u);
    }
    if (layer.root[at] == i) {
      const int n = layer.n[at], m = layer.m[at];
      if (n > 0) {
        const int c = seg_class(layer_src, b, i, C);
        unsigned int* cell = s_seg + (1 * seg::kBins + seg::bin_of(layer.size[at])) * kSegRows * C + c;
        atomicAdd(cell, 1u);
        atomicAdd(cell + C, (unsigned)n);
        if (m) atomicAdd(cell + 2 * C, (unsigned)m);
        if (2 * (int64_t)m > n) atomicAdd(cell + 3 * C, 1u);
      }
    }
  }
  __syncthreads();
  flush_bins(s_seg, 1, 0, n_bins, table);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline int64_t seg_int_map_bytes(int B, int H, int W) { return ((int64_t)B * H * W * 4 + 15) / 16 * 16; }
inline int64_t seg_image_bytes(int H, int W) { return ((int64_t)H * W + 3) / 4 * 4; }
inline int64_t seg_u8_map_bytes(int B, int H, int W) { return (B * seg_image_bytes(H, W) + 15) / 16 * 16; }

// blocks per image of the pixel-streaming kernels: four pixels per thread until the grid fills the chip
inline int seg_blocks_per_image(int64_t HW, int B) {
  return (int)quad_split(HW, B, kNumCu - reserved_cus(), kSegBlocksPerCu, 4, kSegBlock).blocks_per_image;
}

inline bool seg_shape_ok(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffll) return false;
  const int64_t tiles = (int64_t)seg::tiles(H, seg::kTileH) * seg::tiles(W, seg::kTileW) * B;
  return tiles <= 0x7fffffffll && (int64_t)seg_blocks_per_image((int64_t)H * W, B) * B <= 0x7fffffffll;
}

// seg_local + seg_merge: image-wide parents of one map, its counter maps zeroed
static int seg_components(const SegSrc& src, int B, int C, int H, int W, int connectivity, int* parent, int* z0, int* z1, int* z2,
                          hipStream_t s) {
  const int tiles_x = seg::tiles(W, seg::kTileW), tiles_y = seg::tiles(H, seg::kTileH);
  hipLaunchKernelGGL(seg_local, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(kSegBlock), 0, s, src, C, H, W, connectivity == 8 ? 1 : 0,
                     tiles_x, tiles_y, parent, z0, z1, z2);
  DASAC_CHECK_LAUNCH("seg_local");
  const int64_t items = seg::border_items(H, W);
  if (items > 0) {
    hipLaunchKernelGGL(seg_merge, dim3((unsigned)stream_grid(items * B, kSegBlock)), dim3(kSegBlock), 0, s, src, C, H, W, connectivity,
                       items, items * B, parent);
    DASAC_CHECK_LAUNCH("seg_merge");
  }
  return DASAC_OK;
}

#define DASAC_SEG_TRY(call)          \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != DASAC_OK) return rc_; \
  } while (0)

}  // namespace dasac

extern "C" size_t dasac_label_segments_workspace(int B, int H, int W) {
  (void)B, (void)H, (void)W;                           // the parents are built in `segment`, the counts in `size`
  return 0;
}

extern "C" int dasac_label_segments(const void* labels, int labels_u8, int B, int C, int H, int W, int connectivity, int32_t* segment,
                                    int32_t* size, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  using namespace dasac;
  (void)workspace, (void)ws_bytes;
  DASAC_REQUIRE(labels && segment, "label_segments: null labels or segment");
  DASAC_REQUIRE(seg_shape_ok(B, H, W), "label_segments: B, H and W must be positive, H * W at most 2^31 - 1");
  DASAC_REQUIRE(C >= 1 && C <= kSegMaxC, "label_segments: C must be in 1..%d", kSegMaxC);
  DASAC_REQUIRE(connectivity == 4 || connectivity == 8, "label_segments: connectivity must be 4 or 8 (got %d)", connectivity);
  DASAC_REQUIRE((labels_u8 || (reinterpret_cast<uintptr_t>(labels) & 7u) == 0) &&
                    ((reinterpret_cast<uintptr_t>(segment) | reinterpret_cast<uintptr_t>(size)) & 3u) == 0,
                "label_segments: int64 / int32 tensors must be aligned to their element size");
  const int64_t HW = (int64_t)H * W;
  const SegSrc src{labels, HW, labels_u8 ? kSegU8 : kSegI64};
  hipStream_t s = as_stream(stream);
  DASAC_SEG_TRY(seg_components(src, B, C, H, W, connectivity, segment, size, nullptr, nullptr, s));
  const int bpi = seg_blocks_per_image(HW, B);
  hipLaunchKernelGGL((seg_resolve<false>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, segment, size, HW, bpi, SegLayerArgs{});
  DASAC_CHECK_LAUNCH("seg_resolve");
  if (size) {
    hipLaunchKernelGGL(seg_broadcast, dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, segment, size, HW, bpi);
    DASAC_CHECK_LAUNCH("seg_broadcast");
  }
  return DASAC_OK;
}

// roots and sizes, one int32 map each
extern "C" size_t dasac_segment_filter_workspace(int B, int H, int W) {
  using namespace dasac;
  if (!seg_shape_ok(B, H, W)) return 0;
  return 2 * (size_t)seg_int_map_bytes(B, H, W);
}

extern "C" int dasac_segment_filter(const void* labels, int labels_u8, int B, int C, int H, int W, int connectivity, int min_size,
                                    int fill, void* out, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(labels && out && workspace, "segment_filter: null labels, out or workspace");
  DASAC_REQUIRE(seg_shape_ok(B, H, W), "segment_filter: B, H and W must be positive, H * W at most 2^31 - 1");
  DASAC_REQUIRE(C >= 1 && C <= kSegMaxC, "segment_filter: C must be in 1..%d", kSegMaxC);
  DASAC_REQUIRE(connectivity == 4 || connectivity == 8, "segment_filter: connectivity must be 4 or 8 (got %d)", connectivity);
  DASAC_REQUIRE(!labels_u8 || (fill >= 0 && fill <= 255), "segment_filter: fill %d does not fit a uint8 map", fill);
  const int64_t HW = (int64_t)H * W;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(labels), oo = reinterpret_cast<uintptr_t>(out);
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)HW * (labels_u8 ? 1u : 8u);
  DASAC_REQUIRE(oo + bytes <= lo || lo + bytes <= oo, "segment_filter: out may not alias labels");
  DASAC_REQUIRE((labels_u8 || ((lo | oo) & 7u) == 0) && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0,
                "segment_filter: int64 tensors must be aligned to their element size, the workspace to 16 bytes");
  const size_t need = dasac_segment_filter_workspace(B, H, W);
  DASAC_REQUIRE(ws_bytes >= need, "segment_filter: workspace too small (%zu < %zu)", ws_bytes, need);
  int* root = static_cast<int*>(workspace);
  int* size = reinterpret_cast<int*>(static_cast<uint8_t*>(workspace) + seg_int_map_bytes(B, H, W));
  hipStream_t s = as_stream(stream);
  const int bpi = seg_blocks_per_image(HW, B);
  if (min_size > 1) {
    const SegSrc src{labels, HW, labels_u8 ? kSegU8 : kSegI64};
    DASAC_SEG_TRY(seg_components(src, B, C, H, W, connectivity, root, size, nullptr, nullptr, s));
    hipLaunchKernelGGL((seg_resolve<false>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, root, size, HW, bpi, SegLayerArgs{});
    DASAC_CHECK_LAUNCH("seg_resolve");
  }
  if (labels_u8) {
    hipLaunchKernelGGL((seg_filter_apply<uint8_t>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, static_cast<const uint8_t*>(labels),
                       root, size, HW, bpi, min_size, (uint8_t)fill, static_cast<uint8_t*>(out));
  } else {
    hipLaunchKernelGGL((seg_filter_apply<int64_t>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, static_cast<const int64_t*>(labels),
                       root, size, HW, bpi, min_size, (int64_t)fill, static_cast<int64_t*>(out));
  }
  DASAC_CHECK_LAUNCH("seg_filter_apply");
  return DASAC_OK;
}

// one uint8 map per non-NULL slot and one for the ground truth (an upper bound: only score layers are arg-maxed into one, label maps
// are read where they are), then seven int32 maps: the ground truth's roots, sizes and m, the layer's roots, sizes, n and m
extern "C" size_t dasac_segment_counts_workspace(int layers, int B, int H, int W) {
  using namespace dasac;
  if (layers < 0 || layers > kCountScores + kCountMaps || !seg_shape_ok(B, H, W)) return 0;
  return (size_t)(layers + 1) * (size_t)seg_u8_map_bytes(B, H, W) + 7 * (size_t)seg_int_map_bytes(B, H, W);
}

extern "C" int dasac_segment_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                                    const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C,
                                    int H, int W, int connectivity, int ignore_index, int64_t* table, void* workspace, size_t ws_bytes,
                                    dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(gt && table && workspace, "segment_counts: null gt, table or workspace");
  DASAC_REQUIRE(seg_shape_ok(B, H, W), "segment_counts: B, H and W must be positive, H * W at most 2^31 - 1");
  DASAC_REQUIRE(C >= 1 && C <= kSegCountMaxC, "segment_counts: C must be in 1..%d", kSegCountMaxC);
  DASAC_REQUIRE(connectivity == 4 || connectivity == 8, "segment_counts: connectivity must be 4 or 8 (got %d)", connectivity);
  CountLayers src;
  int ns, nm;
  const bool aligned = gather_count_layers(scores0, scores1, scores2, scores3, labels0, labels1, labels_u8_mask, src, ns, nm) &&
                       ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(table)) & 7u) == 0 &&
                       (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0;
  const int n_layers = ns + nm;
  DASAC_REQUIRE(n_layers > 0, "segment_counts: no layer");
  DASAC_REQUIRE(aligned, "segment_counts: fp32 / int64 tensors must be aligned to their element size, the workspace to 16 bytes");
  const size_t need = dasac_segment_counts_workspace(n_layers, B, H, W);
  DASAC_REQUIRE(ws_bytes >= need, "segment_counts: workspace too small (%zu < %zu)", ws_bytes, need);
  const int64_t HW = (int64_t)H * W, HWp = seg_image_bytes(H, W), map_stride = seg_u8_map_bytes(B, H, W);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int* maps[7];                                        // gt roots, sizes, m; layer roots, sizes, n, m
  for (int k = 0; k < 7; ++k) maps[k] = reinterpret_cast<int*>(ws + (n_layers + 1) * map_stride + k * seg_int_map_bytes(B, H, W));
  hipStream_t s = as_stream(stream);
  const int bpi = seg_blocks_per_image(HW, B);
  const int bpi_quads = seg_blocks_per_image((HW + 3) >> 2, B);

  hipLaunchKernelGGL(seg_prepare, dim3((unsigned)(bpi_quads * B)), dim3(kSegBlock), 0, s, src, ns, gt, C, HW, HWp, map_stride, bpi_quads,
                     (int64_t)ignore_index, ws);
  DASAC_CHECK_LAUNCH("seg_prepare");
  const SegSrc gt_src{ws, HWp, kSegGtCode};
  DASAC_SEG_TRY(seg_components(gt_src, B, C, H, W, connectivity, maps[0], maps[1], maps[2], nullptr, s));
  hipLaunchKernelGGL((seg_resolve<false>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, maps[0], maps[1], HW, bpi, SegLayerArgs{});
  DASAC_CHECK_LAUNCH("seg_resolve");
  const int n_bins = 2 * seg::kBins * kSegRows * C;
  for (int l = 0; l < n_layers; ++l) {
    const SegSrc layer = l < ns ? SegSrc{ws + (1 + l) * map_stride, HWp, kSegU8}
                                : SegSrc{src.m[l - ns], HW, src.u8[l - ns] ? kSegU8 : kSegI64};
    DASAC_SEG_TRY(seg_components(layer, B, C, H, W, connectivity, maps[3], maps[4], maps[5], maps[6], s));
    const SegLayerArgs args{layer, ws, HWp, maps[0], maps[2], maps[5], maps[6], C};
    hipLaunchKernelGGL((seg_resolve<true>), dim3((unsigned)(bpi * B)), dim3(kSegBlock), 0, s, maps[3], maps[4], HW, bpi, args);
    DASAC_CHECK_LAUNCH("seg_resolve");
    hipLaunchKernelGGL(seg_tabulate, dim3((unsigned)(bpi * B)), dim3(kSegBlock), (size_t)n_bins * sizeof(unsigned), s,
                       SegSide{maps[0], maps[1], nullptr, nullptr}, maps[2], ws, HWp, SegSide{maps[3], maps[4], maps[5], maps[6]}, layer, C,
                       HW, bpi, reinterpret_cast<unsigned long long*>(table) + (int64_t)l * n_bins);
    DASAC_CHECK_LAUNCH("seg_tabulate");
  }
  return DASAC_OK;
}
