// What the exact integer count kernels share (validation.hip, boundary.hip, consistency.hip; label_hist in
// sampling.hip is the same design with 16 bytes per lane and keeps its own copy).
//
// Streaming shape: lanes along pixels, a QUAD of four consecutive pixels per thread, every plane ONE dwordx4 load
// declared 4-byte aligned (f32x4u: no head to peel), int64 labels two 8-byte-aligned 16-byte loads.  The last 1..3 pixels of an
// image are read element by element: no load touches an element outside its own plane, so none leaves a buffer.
//
// Counting: u32 LDS adds into a histogram per wave, one u64 global add per non-zero bin per block -- exact, and the same bits on
// every run whatever order the adds arrive in.  Segmentation maps are a few large regions, the worst input of a one-atomic-per-pixel
// histogram (64 lanes adding to one address serialise), so keys are merged before LDS: a thread whose keys are all equal joins a
// wave-wide match -- per distinct key ONE lane adds for all lanes holding it -- every other thread adds once per run of equal keys.
#pragma once
#include "common.hpp"

namespace dasac {

constexpr int kCountBlock = 256;                       // threads per block of every count kernel: 4 waves
constexpr int kCountScores = 4, kCountMaps = 2;        // layer slots of the validation count calls

struct CountLayers {                                   // by value: no device-side table
  const float* s[kCountScores];                        // [B,C,HW] fp32, the first `ns` set
  const void* m[kCountMaps];                           // [B,HW] int64 or uint8, the first `nm` set
  int u8[kCountMaps];                                  // map l holds uint8
};

// gathers the non-NULL slots in order; false when a tensor is not aligned to its element size
inline bool gather_count_layers(const float* s0, const float* s1, const float* s2, const float* s3, const void* m0, const void* m1,
                                int u8_mask, CountLayers& layers, int& ns, int& nm) {
  const float* sc[kCountScores] = {s0, s1, s2, s3};
  const void* mp[kCountMaps] = {m0, m1};
  layers = CountLayers{};
  ns = nm = 0;
  bool aligned = true;
  for (int i = 0; i < kCountScores; ++i)
    if (sc[i]) {
      aligned = aligned && (reinterpret_cast<uintptr_t>(sc[i]) & 3u) == 0;
      layers.s[ns++] = sc[i];
    }
  for (int i = 0; i < kCountMaps; ++i)
    if (mp[i]) {
      layers.u8[nm] = (u8_mask >> i) & 1;
      aligned = aligned && (layers.u8[nm] || (reinterpret_cast<uintptr_t>(mp[i]) & 7u) == 0);
      layers.m[nm++] = mp[i];
    }
  return aligned;
}

// All calling lanes are active together and hold one key each: the number of lanes that hold this lane's key, and `leader` on the
// one lane that adds for them
__device__ __forceinline__ unsigned wave_match(int key, bool& leader) {
  const int lane = (int)(threadIdx.x & (kWave - 1));
  for (;;) {                                           // one trip per distinct key of the wave: the lanes holding it leave together
    const int lead = __builtin_amdgcn_readfirstlane(key);
    const unsigned long long same = __ballot(key == lead);
    if (key == lead) {
      leader = lane == __ffsll((long long)same) - 1;
      return (unsigned)__popcll(same);
    }
  }
}

// one thread's four keys into one table, one add per run of equal keys; a negative key adds nothing
__device__ __forceinline__ void count_runs4(unsigned int* __restrict__ h, const int (&k)[4]) {
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

// ... merged: four equal keys join the wave-wide match, anything else goes run by run
__device__ __forceinline__ void count_add4(unsigned int* __restrict__ h, const int (&k)[4]) {
  if (k[1] == k[0] && k[2] == k[0] && k[3] == k[0]) {
    if (k[0] >= 0) {
      bool leader;
      const unsigned n = wave_match(k[0], leader);
      if (leader) atomicAdd(&h[k[0]], 4u * n);
    }
  } else {
    count_runs4(h, k);
  }
}

// sums the `copies` u32 tables (`stride` apart) of a block: one u64 global add per non-zero bin.  (A block is kCountBlock threads:
// the mask on the thread index costs nothing and tells the compiler that i starts below the stride.)
__device__ __forceinline__ void flush_bins(const unsigned int* __restrict__ s, int copies, int stride, int n,
                                           unsigned long long* __restrict__ out) {
  for (int i = threadIdx.x & (kCountBlock - 1); i < n; i += kCountBlock) {
    unsigned long long sum = 0;
    for (int w = 0; w < copies; ++w) sum += s[w * stride + i];
    if (sum) atomicAdd(&out[i], sum);
  }
}

// (load_quad of an fp32 plane: common.hpp)
// four int64 labels; the slots past nx read as `fill`
__device__ __forceinline__ void load_quad(const int64_t* __restrict__ src, int nx, int64_t fill, int64_t (&g)[4]) {
  if (nx == 4) {
    const i64x2u a = *reinterpret_cast<const i64x2u*>(src), b = *reinterpret_cast<const i64x2u*>(src + 2);
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

// four uint8 labels (any address: byte loads); the slots past nx read as `fill`
__device__ __forceinline__ void load_quad(const uint8_t* __restrict__ src, int nx, int64_t fill, int64_t (&g)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = e < nx ? (int64_t)src[e] : fill;
}

// arg-max (the FIRST maximum: strict >, like torch.argmax) over the C planes of one score tensor at pixels r .. r+nx-1 of one image
// (`img` = the image's first plane).  CT > 0: the class count compiled in, all CT quads in flight; CT == 0: a running maximum over
// `C` planes.  CONF also returns the winning confidence: the winning score itself, or with `softmax` 1 / sum_c expf(x_c - max_c x)
// (classes in order, fp32) -- the runtime-C path reads the planes a second time for that sum.
template <int CT, bool CONF>
__device__ __forceinline__ void argmax_quad(const float* __restrict__ img, int C, int64_t HW, int64_t r, int nx, bool softmax,
                                            int (&p)[4], float (&conf)[4]) {
  const float* lp = img + r;
  if constexpr (CT > 0) {
    f32x4u v[CT];
    if (nx == 4) {                                     // ONE branch around all CT loads, not one per plane
#pragma unroll
      for (int c = 0; c < CT; ++c) v[c] = load_quad(lp + (int64_t)c * HW, 4);
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) v[c] = load_quad(lp + (int64_t)c * HW, nx);
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
    if (CONF && softmax) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c) sum += expf(v[c][e] - conf[e]);
        conf[e] = 1.0f / sum;
      }
    }
  } else {
    float best[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      best[e] = e < nx ? lp[e] : 0.f;
      p[e] = 0;
    }
    for (int c = 1; c < C; ++c) {
      const f32x4u v = load_quad(lp + (int64_t)c * HW, nx);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v[e] > best[e]) {
          best[e] = v[e];
          p[e] = c;
        }
    }
    if constexpr (CONF) {
      float sum[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        best[e] = e < nx ? lp[(int64_t)p[e] * HW + e] : 0.f;
        sum[e] = 0.f;
      }
      if (softmax) {
        for (int c = 0; c < C; ++c) {
          const f32x4u v = load_quad(lp + (int64_t)c * HW, nx);
#pragma unroll
          for (int e = 0; e < 4; ++e) sum[e] += expf(v[e] - best[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) conf[e] = softmax ? 1.0f / sum[e] : best[e];
    }
  }
}

template <int CT>
__device__ __forceinline__ void argmax_quad(const float* __restrict__ img, int C, int64_t HW, int64_t r, int nx, int (&p)[4]) {
  float conf[4];
  argmax_quad<CT, false>(img, C, HW, r, nx, false, p, conf);
}

}  // namespace dasac
