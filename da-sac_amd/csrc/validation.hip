// Validation counts for several mask layers at once (the whole of it):
//   train.py:386-399 keeps one `Jaccard` per mask layer -- `logits_up`, `teacher_init`, `teacher_refined` through
//   `torch.argmax(., 1)` (:367-368,394-395) and the label map `teacher_labels` as it is (:396-397) -- and
//   utils/metrics.py:18-39 `Jaccard.add_sample` loops over the classes with three `.item()` syncs each.  Here ONE launch per
//   batch reads the ground truth once and accumulates the (tp, fp, fn) pixel counts of every layer: counts[L][3][C].
//
// Per pixel with ground truth g and prediction p (metrics.py:28-39):
//   g == ignore_index        skipped (the reference overwrites p with ignore_index there: neither side is a class);
//   p == g                   tp[g]   (only a g inside [0, C) is a bin);
//   otherwise                fp[p] if 0 <= p < C, fn[g] if 0 <= g < C
// so a label-map pixel of 255 over a labelled ground truth is a false negative only, and g == -1 a false positive only
// (what dasac_iou_counts does and g14 pins).  The arg-max takes the FIRST maximum (strict >), like torch.argmax and
// dasac_iou_counts.
//
// Counting: integer adds only -- u32 LDS adds into a histogram per wave, one u64 global add per non-zero bin per block.
// Exact, and the same bits on every run whatever order the adds arrive in.  The reference accumulates in float32, which stops
// being exact past 2^24 pixels per class; the project keeps exact int64 counts and a float32 summary (driver.summarise_iou,
// g14), here too.
//
// Streaming shape, loaders and key merging: count_stream.hpp (a quad of four pixels per thread, one dwordx4 per class plane, the
// last 1..3 pixels of an image element by element; count_add4 merges equal keys before LDS).  A quad whose four pixels are all
// ignored skips its score loads.
//
// Registers: C = 19 is compiled in (19 x 4 values in flight per layer, layers one after the other): <= 128 VGPRs, four waves
// per SIMD; the runtime-C path keeps a running maximum.
//
// Second half of the file: dasac_confusion_counts, the same pass with the joint key (ground truth x prediction, and arg-max
// class x confidence bin x hit) -- a diagnostic the reference does not have; the marginal counts above follow from its tables.
#include <atomic>

#include "count_split.hpp"
#include "count_stream.hpp"

namespace dasac {

constexpr int kMcBlock = kCountBlock;                  // 4 waves, each with its own [layers][3][64] u32 histogram
constexpr int kMcWaves = kMcBlock / kWave;
constexpr int kMcScores = kCountScores, kMcMaps = kCountMaps, kMcLayers = kMcScores + kMcMaps;
constexpr int kMcBins = 3 * 64;                        // key = kind * 64 + class, kind 0 tp / 1 fp / 2 fn
constexpr int kMcBlocksPerCu = 8;
constexpr int64_t kMcMaxBlockQuads = 1ll << 29;        // a block's u32 bins can not overflow: at most 2^31 pixels per block

// keys of one layer's four predictions: pc = predicted class or -1 when it is no class, eq = (p == g) on the full values
__device__ __forceinline__ void mc_count(unsigned int* __restrict__ h, const int (&pc)[4], const bool (&eq)[4], const int (&gc)[4],
                                         const bool (&skip)[4]) {
  int k1[4], k2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k1[e] = skip[e] ? -1 : eq[e] ? gc[e] : (pc[e] | 64);                  // a class is < 64: | adds the kind, and -1 stays -1
    k2[e] = (skip[e] || eq[e]) ? -1 : (gc[e] | 128);
  }
  count_add4(h, k1);
  count_add4(h, k2);
}

// the launch's split of an image's quads over blocks (count_split.hpp), or the error when the grid does not fit one launch
static int mc_split(const char* what, int64_t HW, int B, QuadSplit& split) {
  split = quad_split((HW + 3) >> 2, B, kNumCu - reserved_cus(), kMcBlocksPerCu, 4, kMcBlock, kMcMaxBlockQuads);
  DASAC_REQUIRE(split.blocks_per_image * B <= 0x7fffffffll, "%s: B * HW too large for one launch", what);
  return DASAC_OK;
}

// grid: B * blocks_per_image blocks; block (b, j) takes quads [j * per, (j + 1) * per) of image b (quad = 4 consecutive pixels)
template <int CT>
__global__ __launch_bounds__(kMcBlock) void mask_counts(const CountLayers layers, int ns, int nm, const int64_t* __restrict__ gt,
                                                        int Crt, int64_t HW, int blocks_per_image, int64_t per,
                                                        int64_t ignore_index, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int s[kMcWaves][kMcLayers * kMcBins];
  for (int i = threadIdx.x; i < kMcWaves * kMcLayers * kMcBins; i += kMcBlock) (&s[0][0])[i] = 0;
  __syncthreads();

  const int C = CT > 0 ? CT : Crt;
  const int64_t b = blockIdx.x / (unsigned)blocks_per_image;
  const int j = (int)(blockIdx.x - b * blocks_per_image);
  const int64_t n_quads = (HW + 3) >> 2;
  const int64_t q0 = j * per;
  int64_t q1 = q0 + per;
  if (q1 > n_quads) q1 = n_quads;
  const int64_t* gt_b = gt + b * HW;
  unsigned int* hw = s[threadIdx.x >> 6];

  for (int64_t q = q0 + threadIdx.x; q < q1; q += kMcBlock) {
    const int64_t r = q << 2;
    const int nx = HW - r >= 4 ? 4 : (int)(HW - r);    // 1..4: r < HW because q < ceil(HW / 4)
    int64_t g[4];
    load_quad(gt_b + r, nx, ignore_index, g);
    bool skip[4];
    int gc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      skip[e] = g[e] == ignore_index;                  // utils/metrics.py:28-30: only ignore_index pixels are dropped
      gc[e] = (g[e] >= 0 && g[e] < C) ? (int)g[e] : -1;
    }
    if (skip[0] && skip[1] && skip[2] && skip[3]) continue;
#pragma unroll
    for (int l = 0; l < kMcScores; ++l)
      if (l < ns) {
        int pc[4];
        argmax_quad<CT>(layers.s[l] + b * C * HW, C, HW, r, nx, pc);
        bool eq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) eq[e] = g[e] == pc[e];
        mc_count(hw + l * kMcBins, pc, eq, gc, skip);
      }
#pragma unroll
    for (int l = 0; l < kMcMaps; ++l)
      if (l < nm) {
        int64_t p[4];
        load_quad(static_cast<const int64_t*>(layers.m[l]) + b * HW + r, nx, ignore_index, p);
        int pc[4];
        bool eq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pc[e] = (p[e] >= 0 && p[e] < C) ? (int)p[e] : -1;
          eq[e] = p[e] == g[e];
        }
        mc_count(hw + (ns + l) * kMcBins, pc, eq, gc, skip);
      }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < (ns + nm) * kMcBins; i += kMcBlock) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kMcWaves; ++w) sum += s[w][i];
    const int l = i / kMcBins, k = i - l * kMcBins;
    if (sum && (k & 63) < C) atomicAdd(&counts[(l * 3 + (k >> 6)) * C + (k & 63)], sum);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Joint tables of the same pass (dasac_confusion_counts): confusion[L][C+1][C+1] (row = ground truth, column = prediction, index C
// = "no class") and, for the score layers, reliability[Ls][C][n_bins][2] (arg-max class, bin of the winning confidence, miss / hit).
//
// The loads are those of mask_counts; the key is wider: row * (C + 1) + col, so 255 is a bin and "adds nothing" is a negative key.
// LDS is one dynamic array sized by the launch: `copies` (one per wave, or one per block when four would not fit 64 KiB) tables of
// [L][(C+1)^2] u32, then ONE [Ls][C][n_bins][2] u32 table per block -- the confidence bins of neighbouring pixels differ, so those
// keys are not merged and each pixel adds once.  C = 19, 3 + 1 layers, 10 bins: 25.6 + 4.5 KB, four blocks per CU beside 128 VGPRs.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kCfMaxBins = 32;
constexpr size_t kCfLdsMax = 160 * 1024;               // what one workgroup may take
constexpr size_t kCfLdsPlain = 64 * 1024;              // above this a kernel's dynamic-LDS limit has to be raised

// grid and block as mask_counts; dynamic LDS: (copies * (ns + nm) * (C+1)^2 + (REL ? ns * C * n_bins * 2 : 0)) * 4 bytes
template <int CT, bool REL>
__global__ __launch_bounds__(kMcBlock) void confusion_counts(const CountLayers layers, int ns, int nm,
                                                             const int64_t* __restrict__ gt, int Crt, int64_t HW, int blocks_per_image,
                                                             int64_t per, int64_t ignore_index, int copies, int n_bins, int softmax_mask,
                                                             unsigned long long* __restrict__ confusion,
                                                             unsigned long long* __restrict__ reliability) {
  extern __shared__ unsigned int s_cf[];
  const int C = CT > 0 ? CT : Crt;
  const int side = C + 1, bins = side * side;
  const int n_conf = (ns + nm) * bins;                 // one copy
  const int n_rel = REL ? ns * C * n_bins * 2 : 0;
  for (int i = threadIdx.x; i < copies * n_conf + n_rel; i += kMcBlock) s_cf[i] = 0;
  __syncthreads();

  const int64_t b = blockIdx.x / (unsigned)blocks_per_image;
  const int j = (int)(blockIdx.x - b * blocks_per_image);
  const int64_t n_quads = (HW + 3) >> 2;
  const int64_t q0 = j * per;
  int64_t q1 = q0 + per;
  if (q1 > n_quads) q1 = n_quads;
  const int64_t* gt_b = gt + b * HW;
  unsigned int* hw = s_cf + (copies > 1 ? (int)(threadIdx.x >> 6) * n_conf : 0);
  unsigned int* hr = s_cf + copies * n_conf;
  const float fbins = (float)n_bins;

  for (int64_t q = q0 + threadIdx.x; q < q1; q += kMcBlock) {
    const int64_t r = q << 2;
    const int nx = HW - r >= 4 ? 4 : (int)(HW - r);    // 1..4: r < HW because q < ceil(HW / 4)
    int64_t g[4];
    load_quad(gt_b + r, nx, ignore_index, g);
    bool skip[4];
    int row[4];                                        // the row's first bin
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      skip[e] = g[e] == ignore_index;                  // first: a gt of 255 is skipped when ignore_index is 255, a bin otherwise
      row[e] = ((g[e] >= 0 && g[e] < C) ? (int)g[e] : C) * side;
    }
    if (skip[0] && skip[1] && skip[2] && skip[3]) continue;
#pragma unroll
    for (int l = 0; l < kMcScores; ++l)
      if (l < ns) {
        int pc[4], k[4];
        if constexpr (REL) {
          float conf[4];
          argmax_quad<CT, true>(layers.s[l] + b * C * HW, C, HW, r, nx, (softmax_mask >> l) & 1, pc, conf);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (!skip[e]) {
              const float t = conf[e] * fbins;         // one fp32 multiply; NaN and <= 0 to bin 0, >= 1 to the last bin
              const int bin = !(conf[e] > 0.f) ? 0 : (t >= fbins ? n_bins - 1 : (int)t);
              atomicAdd(&hr[((l * C + pc[e]) * n_bins + bin) * 2 + (row[e] == pc[e] * side ? 1 : 0)], 1u);
            }
        } else {
          argmax_quad<CT>(layers.s[l] + b * C * HW, C, HW, r, nx, pc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = skip[e] ? -1 : row[e] + pc[e];
        count_add4(hw + l * bins, k);
      }
#pragma unroll
    for (int l = 0; l < kMcMaps; ++l)
      if (l < nm) {
        int64_t p[4];
        if (layers.u8[l]) {
          load_quad(static_cast<const uint8_t*>(layers.m[l]) + b * HW + r, nx, ignore_index, p);
        } else {
          load_quad(static_cast<const int64_t*>(layers.m[l]) + b * HW + r, nx, ignore_index, p);
        }
        int k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = skip[e] ? -1 : row[e] + ((p[e] >= 0 && p[e] < C) ? (int)p[e] : C);
        count_add4(hw + (ns + l) * bins, k);
      }
  }

  __syncthreads();
  flush_bins(s_cf, copies, n_conf, n_conf, confusion);
  if constexpr (REL) flush_bins(hr, 1, 0, n_rel, reliability);
}

inline size_t cf_lds_bytes(int copies, int layers, int scores, int C, int n_bins) {
  return ((size_t)copies * layers * (C + 1) * (C + 1) + (size_t)scores * C * n_bins * 2) * sizeof(unsigned int);
}

// one launch over `ns` score layers and `nm` label maps (either may be 0) into tables that start at these layers
static int cf_launch(const CountLayers& layers, int ns, int nm, const int64_t* gt, int B, int C, int64_t HW, int ignore_index,
                     int64_t* confusion, int64_t* reliability, int n_bins, int softmax_mask, hipStream_t stream) {
  const int rel_bins = reliability && ns > 0 ? n_bins : 0;
  const bool rel = rel_bins > 0;
  const int copies = cf_lds_bytes(kMcWaves, ns + nm, ns, C, rel_bins) <= kCfLdsPlain ? kMcWaves : 1;
  const size_t lds = cf_lds_bytes(copies, ns + nm, ns, C, rel_bins);
  DASAC_REQUIRE(lds <= kCfLdsMax, "confusion_counts: the tables do not fit LDS");
  if (lds > kCfLdsPlain) {                               // raise the kernels' dynamic-LDS limit once per device, not per launch
    static std::atomic<unsigned long long> raised{0};    // (only the runtime-C kernels get here: C = 19 stays below 64 KiB)
    int dev = 0;
    DASAC_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
      DASAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(confusion_counts<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)kCfLdsMax));
      DASAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(confusion_counts<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)kCfLdsMax));
      raised.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  QuadSplit split;
  if (int rc = mc_split("confusion_counts", HW, B, split)) return rc;
  const dim3 grid((unsigned)(split.blocks_per_image * B)), block(kMcBlock);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(confusion);
  unsigned long long* out_rel = reinterpret_cast<unsigned long long*>(reliability);
#define DASAC_CF_LAUNCH(CT, REL)                                                                                                  \
  hipLaunchKernelGGL((confusion_counts<CT, REL>), grid, block, lds, stream, layers, ns, nm, gt, C, HW, (int)split.blocks_per_image,   \
                     split.quads_per_block, (int64_t)ignore_index, copies, rel_bins, softmax_mask, out, out_rel)
  if (C == 19) {
    if (rel) DASAC_CF_LAUNCH(19, true); else DASAC_CF_LAUNCH(19, false);
  } else {
    if (rel) DASAC_CF_LAUNCH(0, true); else DASAC_CF_LAUNCH(0, false);
  }
#undef DASAC_CF_LAUNCH
  DASAC_CHECK_LAUNCH("confusion_counts");
  return DASAC_OK;
}

}  // namespace dasac

extern "C" int dasac_confusion_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                                      const void* labels0, const void* labels1, int labels_u8_mask, const int64_t* gt, int B, int C,
                                      int64_t HW, int ignore_index, int64_t* confusion, int64_t* reliability, int n_bins,
                                      int softmax_mask, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(gt && confusion, "confusion_counts: null gt or confusion");
  DASAC_REQUIRE(B > 0 && C > 0 && HW > 0, "confusion_counts: B, C and HW must be positive");
  DASAC_REQUIRE(C <= 64, "confusion_counts: at most 64 classes");
  DASAC_REQUIRE(!reliability || (n_bins >= 1 && n_bins <= kCfMaxBins), "confusion_counts: n_bins must be in 1..32");
  CountLayers layers;
  int ns, nm;
  const bool aligned = gather_count_layers(scores0, scores1, scores2, scores3, labels0, labels1, labels_u8_mask, layers, ns, nm) &&
                       ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(confusion) |
                         reinterpret_cast<uintptr_t>(reliability)) & 7u) == 0;
  DASAC_REQUIRE(ns + nm > 0, "confusion_counts: no layer");
  DASAC_REQUIRE(aligned, "confusion_counts: fp32 / int64 tensors must be aligned to their element size");
  hipStream_t s = as_stream(stream);
  const int rel_bins = reliability && ns > 0 ? n_bins : 0;
  if (cf_lds_bytes(1, ns + nm, ns, C, rel_bins) <= kCfLdsMax || ns == 0 || nm == 0)
    return cf_launch(layers, ns, nm, gt, B, C, HW, ignore_index, confusion, reliability, n_bins, softmax_mask, s);
  // close to 64 classes with every slot used and many bins the tables of all layers exceed one workgroup's LDS: the score layers
  // (with their reliability tables) and the label maps go in two launches
  int rc = cf_launch(layers, ns, 0, gt, B, C, HW, ignore_index, confusion, reliability, n_bins, softmax_mask, s);
  if (rc != DASAC_OK) return rc;
  CountLayers maps = {};
  for (int i = 0; i < nm; ++i) {
    maps.m[i] = layers.m[i];
    maps.u8[i] = layers.u8[i];
  }
  return cf_launch(maps, 0, nm, gt, B, C, HW, ignore_index, confusion + (int64_t)ns * (C + 1) * (C + 1), nullptr, 0, 0, s);
}

extern "C" int dasac_mask_counts(const float* scores0, const float* scores1, const float* scores2, const float* scores3,
                                 const int64_t* labels0, const int64_t* labels1, const int64_t* gt, int B, int C, int64_t HW,
                                 int ignore_index, int64_t* counts, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(gt && counts, "mask_counts: null gt or counts");
  DASAC_REQUIRE(B > 0 && C > 0 && HW > 0, "mask_counts: B, C and HW must be positive");
  DASAC_REQUIRE(C <= 64, "mask_counts: at most 64 classes");
  CountLayers layers;
  int ns, nm;
  const bool aligned = gather_count_layers(scores0, scores1, scores2, scores3, labels0, labels1, 0, layers, ns, nm) &&
                       ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(counts)) & 7u) == 0;
  DASAC_REQUIRE(ns + nm > 0, "mask_counts: no layer");
  DASAC_REQUIRE(aligned, "mask_counts: fp32 / int64 tensors must be aligned to their element size");
  QuadSplit split;
  if (int rc = mc_split("mask_counts", HW, B, split)) return rc;
  const dim3 grid((unsigned)(split.blocks_per_image * B)), block(kMcBlock);
  const int bpi = (int)split.blocks_per_image;
  const int64_t per = split.quads_per_block;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  if (C == 19) {
    hipLaunchKernelGGL((mask_counts<19>), grid, block, 0, as_stream(stream), layers, ns, nm, gt, C, HW, bpi, per,
                       (int64_t)ignore_index, out);
  } else {
    hipLaunchKernelGGL((mask_counts<0>), grid, block, 0, as_stream(stream), layers, ns, nm, gt, C, HW, bpi, per,
                       (int64_t)ignore_index, out);
  }
  DASAC_CHECK_LAUNCH("mask_counts");
  return DASAC_OK;
}
