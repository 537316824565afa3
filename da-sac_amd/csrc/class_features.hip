// Class-conditional feature tables (dasac_label_nodes, dasac_class_feature_stats): exact fp64 moments of an fp32 activation
// [N,Cf,HW] per CLASS and channel, the class of a position read from a label map at the feature map's own resolution -- a
// diagnostic the reference does not have.  include/dasac_hip.h has the definitions.
//
// label_nodes: one thread per node.  The node's pixel, then its (2r+1)^2 window clipped to the image, leaving at the first pixel that
// differs; 1 byte written per node.  A label map is read a handful of times per call, a feature tensor Cf times: this kernel does not
// matter next to the one below.
//
// Stage 1 (class_feature_planes<CT>): one 256-thread block per (sample, group of G channels).  Lanes run along positions: element i
// of a plane belongs to thread (i / 4) % 256, which takes its quads in ascending order and the four elements of a quad in ascending
// order, whatever the address -- every full quad of x is ONE dwordx4 load declared 4-byte aligned, its four node bytes one load
// declared 1-byte aligned, and the last 1..3 elements of a plane and their nodes are read one by one (activations.hip's rule: no
// load leaves its plane, none leaves `nodes`, one code path at every placement).  The accumulators, sum and sum of squares per
// class, are registers with COMPILE-TIME class indices: the loop over classes is fully unrolled and selects with `node == c`; a
// runtime-indexed accumulator array would live in scratch.  CT = 19 holds all classes at once; the generic instantiation holds 16
// and makes ceil(C / 16) passes over the plane (32 classes x 2 doubles are 128 VGPRs on their own).  The block first ORs the
// sample's node bytes into a mask of the classes PRESENT (one pass over HW bytes per G channels), kept in a scalar register: the
// unrolled loop skips an absent class with a scalar branch per quad, and so do the butterflies.  A crop holds a handful of
// classes, and a skipped class leaves the same bits as an accumulated one: exactly 0.
// The node bytes are re-read from L1 / L2 for every channel (HW bytes beside 4 HW bytes of x), not staged in LDS: a Cityscapes
// frame's 33 KB would cost the occupancy that hides the loads' latency.
// Per (wave, channel, present class) ONE butterfly at the end of the plane; the four waves meet in LDS in a fixed order; one partial
// row [C][2] per (sample, channel) goes to the workspace.  The block of channel group 0 also counts its sample's nodes per class:
// u32 LDS adds, one u64 global add per present class (integers: exact in any order, the count kernels' precedent).
//
// Stage 2 (class_feature_finish): one lane per (channel, class) adds the samples' partial rows in ascending order and then adds the
// result to `sums`.  No floating-point atomics, every combination in a fixed order: the same values give the same bits wherever x
// and nodes lie.  x is widened to double and squared in double (exact: 48 significant bits); there is no finite filter.
//
// Registers: two quads of x in flight (8 VGPRs), 2 CT accumulators (76 VGPRs at CT = 19); no scratch, <= 128 VGPRs (4 waves per
// SIMD) for every kernel of this file.
#include "common.hpp"

namespace dasac {

constexpr int kCfBlock = 256;
constexpr int kCfMaxC = 32;                      // classes of a table
constexpr int kCfPassC = 16;                     // classes per pass of the generic instantiation
constexpr int kCfMaxGroup = 8;                   // channels per block
constexpr int kCfMaxRadius = 8;
constexpr int64_t kCfMaxPlane = 1ll << 30;

typedef const char __attribute__((address_space(1)))* cf_gptr;
typedef unsigned cf_u32u __attribute__((aligned(1)));
__device__ __forceinline__ f32x4u cf_load4(cf_gptr plane, unsigned i) {
  return *reinterpret_cast<const f32x4u __attribute__((address_space(1)))*>(plane + i * 4u);
}
__device__ __forceinline__ float cf_load1(cf_gptr plane, unsigned i) {
  return *reinterpret_cast<const float __attribute__((address_space(1)))*>(plane + i * 4u);
}
__device__ __forceinline__ unsigned cf_nodes4(cf_gptr nodes, unsigned i) {      // nodes i .. i+3, node i in the low byte
  return *reinterpret_cast<const cf_u32u __attribute__((address_space(1)))*>(nodes + i);
}
__device__ __forceinline__ unsigned cf_node1(cf_gptr nodes, unsigned i) {
  return *reinterpret_cast<const unsigned char __attribute__((address_space(1)))*>(nodes + i);
}

template <typename T>
__global__ __launch_bounds__(kCfBlock) void label_nodes(const T* __restrict__ labels, int N, int H, int W, int h, int w, int C,
                                                        int radius, uint8_t* __restrict__ nodes) {
  const int64_t total = (int64_t)N * h * w;
  for (int64_t t = (int64_t)blockIdx.x * kCfBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kCfBlock) {
    const int j = (int)(t % w), i = (int)((t / w) % h);
    const int64_t n = t / ((int64_t)w * h);
    // where align_corners=True puts the node, halves rounded up
    const int Y = h > 1 ? (int)((2ll * i * (H - 1) + (h - 1)) / (2ll * (h - 1))) : 0;
    const int X = w > 1 ? (int)((2ll * j * (W - 1) + (w - 1)) / (2ll * (w - 1))) : 0;
    const T* img = labels + n * (int64_t)H * W;
    const T v = img[(int64_t)Y * W + X];
    bool pure = (int64_t)v >= 0 && (int64_t)v < C;
    const int y0 = max(Y - radius, 0), y1 = min(Y + radius, H - 1), x0 = max(X - radius, 0), x1 = min(X + radius, W - 1);
    for (int y = y0; y <= y1 && pure; ++y)
      for (int x = x0; x <= x1; ++x)
        if (img[(int64_t)y * W + x] != v) {
          pure = false;
          break;
        }
    nodes[t] = pure ? (uint8_t)v : (uint8_t)255;
  }
}

template <int CT>
struct CfAcc {
  double s[CT], q[CT];
};

// one element into the accumulators of the classes c0 .. c0+CT-1 that are present; `rel` = node - c0 (anything else: no class here)
template <int CT>
__device__ __forceinline__ void cf_take(CfAcc<CT>& a, unsigned present, float v, int rel) {
  const double d = (double)v;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if ((present >> c) & 1u) {      // scalar
      const double t = rel == c ? d : 0.0;
      a.s[c] += t;
      a.q[c] = fma(t, t, a.q[c]);      // t * t is exact in double: acc + t^2 in one instruction
    }
}

// one quad: the class test is one scalar branch per four elements
template <int CT>
__device__ __forceinline__ void cf_take4(CfAcc<CT>& a, unsigned present, f32x4u v, unsigned lab, int c0, int C) {
  double d[4];
  int rel[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int l = (int)((lab >> (8 * e)) & 255u);
    d[e] = (double)v[e];
    rel[e] = l < C ? l - c0 : -1;
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if ((present >> c) & 1u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // ascending element order per accumulator
        const double t = rel[e] == c ? d[e] : 0.0;
        a.s[c] += t;
        a.q[c] = fma(t, t, a.q[c]);
      }
    }
}

// grid (ceil(Cf / G), N).  CT == 19: C == 19, one pass; CT == kCfPassC: any C <= 32, ceil(C / 16) passes.
template <int CT>
__global__ __launch_bounds__(kCfBlock, 4) void class_feature_planes(const float* __restrict__ x, const uint8_t* __restrict__ nodes_all, int Cf,
                                                                 int HW, int C, int G, double* __restrict__ partial,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ double red[kCfBlock / kWave][2 * CT];
  __shared__ unsigned hist[kCfMaxC];
  __shared__ unsigned wave_mask[kCfBlock / kWave];
  const int n = blockIdx.y, f0 = blockIdx.x * G, f1 = min(f0 + G, Cf);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const cf_gptr nodes = (cf_gptr)(uintptr_t)(nodes_all + (size_t)n * HW);
  const int quads = HW >> 2;
  const bool count = f0 == 0;      // block-uniform

  // ---- the classes present in this sample (and, in the block of channel group 0, their node counts)
  if (tid < kCfMaxC) hist[tid] = 0;
  __syncthreads();
  unsigned mine = 0;
  {
    int q = tid;
    for (; q < quads; q += kCfBlock) {
      const unsigned lab = cf_nodes4(nodes, 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned l = (lab >> (8 * e)) & 255u;
        if (l < (unsigned)C) {
          mine |= 1u << l;
          if (count) atomicAdd(&hist[l], 1u);
        }
      }
    }
    if (q == quads)
      for (int i = 4 * quads; i < HW; ++i) {
        const unsigned l = cf_node1(nodes, i);
        if (l < (unsigned)C) {
          mine |= 1u << l;
          if (count) atomicAdd(&hist[l], 1u);
        }
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine |= __shfl_xor(mine, o, 64);
  if (lane == 0) wave_mask[wv] = mine;
  __syncthreads();
  const unsigned present_all = __builtin_amdgcn_readfirstlane(wave_mask[0] | wave_mask[1] | wave_mask[2] | wave_mask[3]);
  if (count && tid < C && hist[tid]) atomicAdd(&counts[tid], (unsigned long long)hist[tid]);

  for (int f = f0; f < f1; ++f) {
    const size_t plane = (size_t)n * Cf + f;
    const cf_gptr xp = (cf_gptr)(uintptr_t)(x + plane * HW);
    double* out = partial + plane * (size_t)C * 2;
    for (int c0 = 0; c0 < C; c0 += CT) {
      const unsigned present = (present_all >> c0) & (CT < 32 ? (1u << CT) - 1u : ~0u);
      CfAcc<CT> a;
#pragma unroll
      for (int c = 0; c < CT; ++c) a.s[c] = a.q[c] = 0.0;
      if (present) {      // a sample without a class of this pass: the plane is not read
        int q = tid;
        for (; q + kCfBlock < quads; q += 2 * kCfBlock) {      // two quads in flight
          const f32x4u v[2] = {cf_load4(xp, 4 * q), cf_load4(xp, 4 * (q + kCfBlock))};
          const unsigned lab[2] = {cf_nodes4(nodes, 4 * q), cf_nodes4(nodes, 4 * (q + kCfBlock))};
          cf_take4<CT>(a, present, v[0], lab[0], c0, C);
          cf_take4<CT>(a, present, v[1], lab[1], c0, C);
        }
        for (; q < quads; q += kCfBlock) cf_take4<CT>(a, present, cf_load4(xp, 4 * q), cf_nodes4(nodes, 4 * q), c0, C);
        if (q == quads)      // the thread whose next quad is the plane's partial one: its last 1..3 elements, one by one
          for (int i = 4 * quads; i < HW; ++i) {
            const int l = (int)cf_node1(nodes, i);
            cf_take<CT>(a, present, cf_load1(xp, i), l < C ? l - c0 : -1);
          }
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        double s = 0.0, sq = 0.0;
        if ((present >> c) & 1u) {
          s = wave_sum(a.s[c]);
          sq = wave_sum(a.q[c]);
        }
        if (lane == 0) {
          red[wv][2 * c] = s;
          red[wv][2 * c + 1] = sq;
        }
      }
      __syncthreads();
      if (tid < 2 * CT && c0 + (tid >> 1) < C)      // one cell per thread, the four waves in a fixed order
        out[2 * c0 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
      __syncthreads();
    }
  }
}

// one lane per (channel f, class c), f-major as the partial rows lie
__global__ __launch_bounds__(kCfBlock) void class_feature_finish(const double* __restrict__ partial, int N, int Cf, int C,
                                                                 double* __restrict__ sums) {
  const int64_t t = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
  if (t >= (int64_t)Cf * C) return;
  const int f = (int)(t / C), c = (int)(t - (int64_t)f * C);
  double s = 0.0, sq = 0.0;
  for (int n = 0; n < N; ++n) {      // samples in ascending order
    const double* r = partial + (((size_t)n * Cf + f) * C + c) * 2;
    s += r[0];
    sq += r[1];
  }
  double* o = sums + ((size_t)c * Cf + f) * 2;
  o[0] += s;
  o[1] += sq;
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_label_nodes(const void* labels, int labels_u8, int N, int H, int W, int h, int w, int C, int radius,
                                 uint8_t* nodes, dasac_stream_t stream) {
  DASAC_REQUIRE(labels && nodes, "label_nodes: null pointer");
  DASAC_REQUIRE(N > 0 && H > 0 && W > 0 && h > 0 && w > 0, "label_nodes: bad shape");
  DASAC_REQUIRE(C >= 1 && C <= 255, "label_nodes: 1..255 classes (got %d)", C);
  DASAC_REQUIRE(radius >= 0 && radius <= kCfMaxRadius, "label_nodes: radius 0..%d (got %d)", kCfMaxRadius, radius);
  DASAC_REQUIRE((int64_t)H * W < (1ll << 31) && (int64_t)N * h * w < (1ll << 31), "label_nodes: too large");
  DASAC_REQUIRE(labels_u8 || (reinterpret_cast<uintptr_t>(labels) & 7u) == 0, "label_nodes: misaligned int64 labels");
  const int grid = stream_grid((int64_t)N * h * w, kCfBlock);
  hipStream_t s = as_stream(stream);
  if (labels_u8)
    hipLaunchKernelGGL(label_nodes<uint8_t>, dim3(grid), dim3(kCfBlock), 0, s, reinterpret_cast<const uint8_t*>(labels), N, H, W, h, w, C,
                       radius, nodes);
  else
    hipLaunchKernelGGL(label_nodes<int64_t>, dim3(grid), dim3(kCfBlock), 0, s, reinterpret_cast<const int64_t*>(labels), N, H, W, h, w, C,
                       radius, nodes);
  DASAC_CHECK_LAUNCH("label_nodes");
  return DASAC_OK;
}

extern "C" size_t dasac_class_feature_stats_workspace(int N, int Cf, int C) {
  return (N > 0 && Cf > 0 && C > 0) ? (size_t)N * Cf * C * 2 * sizeof(double) : 0;
}

extern "C" int dasac_class_feature_stats(const float* x, const uint8_t* nodes, int N, int Cf, int HW, int C, double* sums,
                                         int64_t* counts, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(x && nodes && sums && counts && workspace, "class_feature_stats: null pointer");
  DASAC_REQUIRE(C >= 1 && C <= kCfMaxC, "class_feature_stats: 1..%d classes (got %d)", kCfMaxC, C);
  DASAC_REQUIRE(N >= 1 && N <= 65535 && Cf >= 1, "class_feature_stats: 1..65535 samples and Cf >= 1 channels (got N=%d, Cf=%d)", N, Cf);
  DASAC_REQUIRE(HW >= 1 && HW < kCfMaxPlane, "class_feature_stats: 1 <= HW < 2^30 (got %d)", HW);
  DASAC_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0 &&
                    ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
                "class_feature_stats: misaligned x / sums / counts / workspace");
  DASAC_REQUIRE(ws_bytes >= dasac_class_feature_stats_workspace(N, Cf, C), "class_feature_stats: workspace too small");
  // channels per block: enough blocks to fill the chip several times over, the present-class pass shared by up to 8 channels
  int G = (int)(((int64_t)N * Cf) / (8 * kNumCu));
  G = G < 1 ? 1 : (G > kCfMaxGroup ? kCfMaxGroup : G);
  const dim3 grid((unsigned)((Cf + G - 1) / G), (unsigned)N);
  hipStream_t s = as_stream(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (C == 19)
    hipLaunchKernelGGL(class_feature_planes<19>, grid, dim3(kCfBlock), 0, s, x, nodes, Cf, HW, C, G, partial, cnt);
  else
    hipLaunchKernelGGL(class_feature_planes<kCfPassC>, grid, dim3(kCfBlock), 0, s, x, nodes, Cf, HW, C, G, partial, cnt);
  DASAC_CHECK_LAUNCH("class_feature_planes");
  const int64_t cells = (int64_t)Cf * C;
  hipLaunchKernelGGL(class_feature_finish, dim3((unsigned)((cells + kCfBlock - 1) / kCfBlock)), dim3(kCfBlock), 0, s, partial, N, Cf, C, sums);
  DASAC_CHECK_LAUNCH("class_feature_finish");
  return DASAC_OK;
}
