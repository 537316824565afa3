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
// Streaming shape: lanes along pixels, four consecutive pixels per thread, every class plane ONE dwordx4 load.  The
// planes of a [B,C,H,W] tensor with an odd H*W (769 x 769) sit at every 4-byte phase, so the loads are declared 4-byte aligned
// (`aligned(4)` vector types, as in head.hip: global memory takes them at full width) -- no head to peel; the ground truth and
// the label maps are two 8-byte-aligned 16-byte loads.  The last 1..3 pixels of an image are read element by element: no load
// touches an element outside its own image, so none leaves a buffer.  A quad whose four pixels are all ignored skips its
// score loads.
//
// Segmentation maps are a few large regions, the worst input of a one-atomic-per-pixel histogram.  Keys are merged before
// LDS as in label_hist (sampling.hip): a thread whose four keys are equal joins a wave-wide match -- per distinct key ONE lane
// adds 4 x (lanes holding it) -- every other thread adds once per run of equal keys.
//
// Registers: C = 19 is compiled in (19 x 4 values in flight per layer, layers one after the other): <= 128 VGPRs, four waves
// per SIMD; the runtime-C path keeps a running maximum.
//
// Second half of the file: dasac_confusion_counts, the same pass with the joint key (ground truth x prediction, and arg-max
// class x confidence bin x hit) -- a diagnostic the reference does not have; the marginal counts above follow from its tables.
#include <atomic>

#include "common.hpp"

namespace dasac {

constexpr int kMcBlock = 256;                          // 4 waves, each with its own [layers][3][64] u32 histogram
constexpr int kMcWaves = kMcBlock / kWave;
constexpr int kMcScores = 4, kMcMaps = 2, kMcLayers = kMcScores + kMcMaps;
constexpr int kMcBins = 3 * 64;                        // key = kind * 64 + class, kind 0 tp / 1 fp / 2 fn
constexpr int kMcNone = 255;                           // "adds nothing"
constexpr int kMcBlocksPerCu = 8;
constexpr int64_t kMcMaxBlockQuads = 1ll << 29;        // a block's u32 bins can not overflow: at most 2^31 pixels per block

typedef float mc_f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef long long mc_i64x2u __attribute__((ext_vector_type(2), aligned(8)));

struct MaskLayers {                                    // by value: no device-side table
  const float* s[kMcScores];                           // [B,C,HW] fp32, the first `ns` set
  const int64_t* m[kMcMaps];                           // [B,HW] int64, the first `nm` set
};

// one thread's four keys of one kind into the wave's histogram of one layer
__device__ __forceinline__ void mc_add4(unsigned int* __restrict__ h, const int (&k)[4]) {
  if (k[1] == k[0] && k[2] == k[0] && k[3] == k[0]) {
    if (k[0] != kMcNone) {
      // wave-wide match over the lanes that hold one key each: one add per distinct key
      const int lane = (int)(threadIdx.x & (kWave - 1));
      bool pending = true;
      while (pending) {
        const int lead = __builtin_amdgcn_readfirstlane(k[0]);
        const unsigned long long same = __ballot(k[0] == lead);
        if (k[0] == lead) {
          if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[lead], 4u * (unsigned)__popcll(same));
          pending = false;
        }
      }
    }
  } else {
    int cur = k[0];
    unsigned run = 1;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
      if (k[e] == cur) {
        ++run;
      } else {
        if (cur != kMcNone) atomicAdd(&h[cur], run);
        cur = k[e];
        run = 1;
      }
    }
    if (cur != kMcNone) atomicAdd(&h[cur], run);
  }
}

// keys of one layer's four predictions: pc = predicted class or -1 when it is no class, eq = (p == g) on the full values
__device__ __forceinline__ void mc_count(unsigned int* __restrict__ h, const int (&pc)[4], const bool (&eq)[4], const int (&gc)[4],
                                         const bool (&skip)[4]) {
  int k1[4], k2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k1[e] = skip[e] ? kMcNone : eq[e] ? (gc[e] >= 0 ? gc[e] : kMcNone) : (pc[e] >= 0 ? 64 + pc[e] : kMcNone);
    k2[e] = (skip[e] || eq[e] || gc[e] < 0) ? kMcNone : 128 + gc[e];
  }
  mc_add4(h, k1);
  mc_add4(h, k2);
}

// arg-max over the C planes of one score tensor at pixels r .. r+nx-1 of one image (`img` = the image's first plane)
template <int CT>
__device__ __forceinline__ void mc_argmax(const float* __restrict__ img, int C, int64_t HW, int64_t r, int nx, int (&p)[4]) {
  const float* lp = img + r;
  if constexpr (CT > 0) {
    mc_f32x4u v[CT];
    if (nx == 4) {
#pragma unroll
      for (int c = 0; c < CT; ++c) v[c] = *reinterpret_cast<const mc_f32x4u*>(lp + (int64_t)c * HW);
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        v[c] = mc_f32x4u{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (e < nx) v[c][e] = lp[(int64_t)c * HW + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float best = v[0][e];
      int k = 0;
#pragma unroll
      for (int c = 1; c < CT; ++c)
        if (v[c][e] > best) {
          best = v[c][e];
          k = c;
        }
      p[e] = k;
    }
  } else {
    float best[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      best[e] = e < nx ? lp[e] : 0.f;
      p[e] = 0;
    }
    for (int c = 1; c < C; ++c) {
      const float* cp = lp + (int64_t)c * HW;
      mc_f32x4u v = mc_f32x4u{0.f, 0.f, 0.f, 0.f};
      if (nx == 4) {
        v = *reinterpret_cast<const mc_f32x4u*>(cp);
      } else {
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (e < nx) v[e] = cp[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e]) {
          best[e] = v[e];
          p[e] = c;
        }
    }
  }
}

// four int64 labels at pixels r .. r+nx-1; the slots past nx read as `fill`
__device__ __forceinline__ void mc_load_labels(const int64_t* __restrict__ src, int nx, int64_t fill, int64_t (&g)[4]) {
  if (nx == 4) {
    const mc_i64x2u a = *reinterpret_cast<const mc_i64x2u*>(src), b = *reinterpret_cast<const mc_i64x2u*>(src + 2);
    g[0] = a[0];
    g[1] = a[1];
    g[2] = b[0];
    g[3] = b[1];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = fill;
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (e < nx) g[e] = src[e];
  }
}

// grid: B * blocks_per_image blocks; block (b, j) takes quads [j * per, (j + 1) * per) of image b (quad = 4 consecutive pixels)
template <int CT>
__global__ __launch_bounds__(kMcBlock) void mask_counts(const MaskLayers layers, int ns, int nm, const int64_t* __restrict__ gt,
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
    mc_load_labels(gt_b + r, nx, ignore_index, g);
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
        mc_argmax<CT>(layers.s[l] + b * C * HW, C, HW, r, nx, pc);
        bool eq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) eq[e] = g[e] == pc[e];
        mc_count(hw + l * kMcBins, pc, eq, gc, skip);
      }
#pragma unroll
    for (int l = 0; l < kMcMaps; ++l)
      if (l < nm) {
        int64_t p[4];
        mc_load_labels(layers.m[l] + b * HW + r, nx, ignore_index, p);
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

struct ConfusionLayers {                               // by value: no device-side table
  const float* s[kMcScores];                           // [B,C,HW] fp32, the first `ns` set
  const void* m[kMcMaps];                              // [B,HW] int64 or uint8, the first `nm` set
  int u8[kMcMaps];                                     // map l holds uint8
};

// one thread's four keys into one table; a negative key adds nothing (mc_add4 with the sentinel out of the key space)
__device__ __forceinline__ void cf_add4(unsigned int* __restrict__ h, const int (&k)[4]) {
  if (k[1] == k[0] && k[2] == k[0] && k[3] == k[0]) {
    if (k[0] >= 0) {
      const int lane = (int)(threadIdx.x & (kWave - 1));
      bool pending = true;
      while (pending) {
        const int lead = __builtin_amdgcn_readfirstlane(k[0]);
        const unsigned long long same = __ballot(k[0] == lead);
        if (k[0] == lead) {
          if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[lead], 4u * (unsigned)__popcll(same));
          pending = false;
        }
      }
    }
  } else {
    int cur = k[0];
    unsigned run = 1;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
      if (k[e] == cur) {
        ++run;
      } else {
        if (cur >= 0) atomicAdd(&h[cur], run);
        cur = k[e];
        run = 1;
      }
    }
    if (cur >= 0) atomicAdd(&h[cur], run);
  }
}

// mc_argmax that also returns the winning confidence: the winning score itself, or with `softmax` 1 / sum_c expf(x_c - max_c x)
// (classes in order, fp32).  The runtime-C path reads the planes a second time for that sum.
template <int CT>
__device__ __forceinline__ void cf_argmax_conf(const float* __restrict__ img, int C, int64_t HW, int64_t r, int nx, bool softmax,
                                               int (&p)[4], float (&conf)[4]) {
  const float* lp = img + r;
  if constexpr (CT > 0) {
    mc_f32x4u v[CT];
    if (nx == 4) {
#pragma unroll
      for (int c = 0; c < CT; ++c) v[c] = *reinterpret_cast<const mc_f32x4u*>(lp + (int64_t)c * HW);
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        v[c] = mc_f32x4u{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (e < nx) v[c][e] = lp[(int64_t)c * HW + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float best = v[0][e];
      int k = 0;
#pragma unroll
      for (int c = 1; c < CT; ++c)
        if (v[c][e] > best) {
          best = v[c][e];
          k = c;
        }
      p[e] = k;
      conf[e] = best;
    }
    if (softmax) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c) sum += expf(v[c][e] - conf[e]);
        conf[e] = 1.0f / sum;
      }
    }
  } else {
    mc_argmax<0>(img, C, HW, r, nx, p);
    float best[4], sum[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      best[e] = e < nx ? lp[(int64_t)p[e] * HW + e] : 0.f;
      sum[e] = 0.f;
    }
    if (softmax) {
      for (int c = 0; c < C; ++c) {
        const float* cp = lp + (int64_t)c * HW;
        mc_f32x4u v = mc_f32x4u{0.f, 0.f, 0.f, 0.f};
        if (nx == 4) {
          v = *reinterpret_cast<const mc_f32x4u*>(cp);
        } else {
#pragma unroll
          for (int e = 0; e < 3; ++e)
            if (e < nx) v[e] = cp[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] += expf(v[e] - best[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) conf[e] = softmax ? 1.0f / sum[e] : best[e];
  }
}

// four uint8 labels at pixels r .. r+nx-1 (any address: byte loads); the slots past nx read as `fill`
__device__ __forceinline__ void cf_load_labels_u8(const uint8_t* __restrict__ src, int nx, int64_t fill, int64_t (&g)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = e < nx ? (int64_t)src[e] : fill;
}

// grid and block as mask_counts; dynamic LDS: (copies * (ns + nm) * (C+1)^2 + (REL ? ns * C * n_bins * 2 : 0)) * 4 bytes
template <int CT, bool REL>
__global__ __launch_bounds__(kMcBlock) void confusion_counts(const ConfusionLayers layers, int ns, int nm,
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
    mc_load_labels(gt_b + r, nx, ignore_index, g);
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
          cf_argmax_conf<CT>(layers.s[l] + b * C * HW, C, HW, r, nx, (softmax_mask >> l) & 1, pc, conf);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (!skip[e]) {
              const float t = conf[e] * fbins;         // one fp32 multiply; NaN and <= 0 to bin 0, >= 1 to the last bin
              const int bin = !(conf[e] > 0.f) ? 0 : (t >= fbins ? n_bins - 1 : (int)t);
              atomicAdd(&hr[((l * C + pc[e]) * n_bins + bin) * 2 + (row[e] == pc[e] * side ? 1 : 0)], 1u);
            }
        } else {
          mc_argmax<CT>(layers.s[l] + b * C * HW, C, HW, r, nx, pc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = skip[e] ? -1 : row[e] + pc[e];
        cf_add4(hw + l * bins, k);
      }
#pragma unroll
    for (int l = 0; l < kMcMaps; ++l)
      if (l < nm) {
        int64_t p[4];
        if (layers.u8[l]) {
          cf_load_labels_u8(static_cast<const uint8_t*>(layers.m[l]) + b * HW + r, nx, ignore_index, p);
        } else {
          mc_load_labels(static_cast<const int64_t*>(layers.m[l]) + b * HW + r, nx, ignore_index, p);
        }
        int k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = skip[e] ? -1 : row[e] + ((p[e] >= 0 && p[e] < C) ? (int)p[e] : C);
        cf_add4(hw + (ns + l) * bins, k);
      }
  }

  __syncthreads();
  for (int i = threadIdx.x; i < n_conf; i += kMcBlock) {
    unsigned long long sum = 0;
    for (int w = 0; w < copies; ++w) sum += s_cf[w * n_conf + i];
    if (sum) atomicAdd(&confusion[i], sum);
  }
  if constexpr (REL) {
    for (int i = threadIdx.x; i < n_rel; i += kMcBlock)
      if (hr[i]) atomicAdd(&reliability[i], (unsigned long long)hr[i]);
  }
}

inline size_t cf_lds_bytes(int copies, int layers, int scores, int C, int n_bins) {
  return ((size_t)copies * layers * (C + 1) * (C + 1) + (size_t)scores * C * n_bins * 2) * sizeof(unsigned int);
}

// one launch over `ns` score layers and `nm` label maps (either may be 0) into tables that start at these layers
static int cf_launch(const ConfusionLayers& layers, int ns, int nm, const int64_t* gt, int B, int C, int64_t HW, int ignore_index,
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
  // blocks per image as in dasac_mask_counts
  const int64_t n_quads = (HW + 3) >> 2;
  int64_t bpi = (n_quads + 4 * kMcBlock - 1) / (4 * kMcBlock);
  const int64_t fill = ((int64_t)(kNumCu - reserved_cus()) * kMcBlocksPerCu + B - 1) / B;
  if (bpi > fill) bpi = fill;
  const int64_t need = (n_quads + kMcMaxBlockQuads - 1) / kMcMaxBlockQuads;
  if (bpi < need) bpi = need;
  DASAC_REQUIRE(bpi * B <= 0x7fffffffll, "confusion_counts: B * HW too large for one launch");
  const int64_t per = (n_quads + bpi - 1) / bpi;
  const dim3 grid((unsigned)(bpi * B)), block(kMcBlock);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(confusion);
  unsigned long long* out_rel = reinterpret_cast<unsigned long long*>(reliability);
#define DASAC_CF_LAUNCH(CT, REL)                                                                                                  \
  hipLaunchKernelGGL((confusion_counts<CT, REL>), grid, block, lds, stream, layers, ns, nm, gt, C, HW, (int)bpi, per,            \
                     (int64_t)ignore_index, copies, rel_bins, softmax_mask, out, out_rel)
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
  ConfusionLayers layers = {};
  int ns = 0, nm = 0;
  const float* sc[kMcScores] = {scores0, scores1, scores2, scores3};
  const void* mp[kMcMaps] = {labels0, labels1};
  for (int i = 0; i < kMcScores; ++i)
    if (sc[i]) layers.s[ns++] = sc[i];
  for (int i = 0; i < kMcMaps; ++i)
    if (mp[i]) {
      layers.u8[nm] = (labels_u8_mask >> i) & 1;
      layers.m[nm++] = mp[i];
    }
  DASAC_REQUIRE(ns + nm > 0, "confusion_counts: no layer");
  bool aligned = (reinterpret_cast<uintptr_t>(gt) & 7u) == 0 && (reinterpret_cast<uintptr_t>(confusion) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(reliability) & 7u) == 0;
  for (int i = 0; i < ns; ++i) aligned = aligned && (reinterpret_cast<uintptr_t>(layers.s[i]) & 3u) == 0;
  for (int i = 0; i < nm; ++i) aligned = aligned && (layers.u8[i] || (reinterpret_cast<uintptr_t>(layers.m[i]) & 7u) == 0);
  DASAC_REQUIRE(aligned, "confusion_counts: fp32 / int64 tensors must be aligned to their element size");
  hipStream_t s = as_stream(stream);
  const int rel_bins = reliability && ns > 0 ? n_bins : 0;
  if (cf_lds_bytes(1, ns + nm, ns, C, rel_bins) <= kCfLdsMax || ns == 0 || nm == 0)
    return cf_launch(layers, ns, nm, gt, B, C, HW, ignore_index, confusion, reliability, n_bins, softmax_mask, s);
  // close to 64 classes with every slot used and many bins the tables of all layers exceed one workgroup's LDS: the score layers
  // (with their reliability tables) and the label maps go in two launches
  int rc = cf_launch(layers, ns, 0, gt, B, C, HW, ignore_index, confusion, reliability, n_bins, softmax_mask, s);
  if (rc != DASAC_OK) return rc;
  ConfusionLayers maps = {};
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
  MaskLayers layers = {};
  int ns = 0, nm = 0;
  const float* sc[kMcScores] = {scores0, scores1, scores2, scores3};
  const int64_t* mp[kMcMaps] = {labels0, labels1};
  for (int i = 0; i < kMcScores; ++i)
    if (sc[i]) layers.s[ns++] = sc[i];
  for (int i = 0; i < kMcMaps; ++i)
    if (mp[i]) layers.m[nm++] = mp[i];
  DASAC_REQUIRE(ns + nm > 0, "mask_counts: no layer");
  bool aligned = (reinterpret_cast<uintptr_t>(gt) & 7u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7u) == 0;
  for (int i = 0; i < ns; ++i) aligned = aligned && (reinterpret_cast<uintptr_t>(layers.s[i]) & 3u) == 0;
  for (int i = 0; i < nm; ++i) aligned = aligned && (reinterpret_cast<uintptr_t>(layers.m[i]) & 7u) == 0;
  DASAC_REQUIRE(aligned, "mask_counts: fp32 / int64 tensors must be aligned to their element size");
  // blocks per image: at least four quads per thread until the grid holds kMcBlocksPerCu blocks per CU, and never fewer than
  // keeps a block's pixel count at or below 2^31 (u32 bins)
  const int64_t n_quads = (HW + 3) >> 2;
  int64_t bpi = (n_quads + 4 * kMcBlock - 1) / (4 * kMcBlock);
  const int64_t fill = ((int64_t)(kNumCu - reserved_cus()) * kMcBlocksPerCu + B - 1) / B;
  if (bpi > fill) bpi = fill;
  const int64_t need = (n_quads + kMcMaxBlockQuads - 1) / kMcMaxBlockQuads;
  if (bpi < need) bpi = need;
  DASAC_REQUIRE(bpi * B <= 0x7fffffffll, "mask_counts: B * HW too large for one launch");
  const int64_t per = (n_quads + bpi - 1) / bpi;
  const dim3 grid((unsigned)(bpi * B)), block(kMcBlock);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  if (C == 19) {
    hipLaunchKernelGGL((mask_counts<19>), grid, block, 0, as_stream(stream), layers, ns, nm, gt, C, HW, (int)bpi, per,
                       (int64_t)ignore_index, out);
  } else {
    hipLaunchKernelGGL((mask_counts<0>), grid, block, 0, as_stream(stream), layers, ns, nm, gt, C, HW, (int)bpi, per,
                       (int64_t)ignore_index, out);
  }
  DASAC_CHECK_LAUNCH("mask_counts");
  return DASAC_OK;
}
