// Per-layer activation health / domain-gap table (dasac_activation_stats): one streaming pass over the fp32 NCHW activations a
// forward pass of the engine already holds, reduced per CHANNEL and per SAMPLE SEGMENT -- a diagnostic the reference does not
// have.  include/dasac_hip.h has the table's definition; columns of a row (fp64; counts and indices are exact integers < 2^53):
//   0 sum   sum x over FINITE x (each widened to double)     3 nonfinite        number of Inf / NaN
//   1 sumsq sum x^2 over finite x (squared in double)        4 first_nonfinite  1 + flat NCHW index in its tensor of the first, or 0
//   2 maxabs max |x| over finite x, 0 if none                5 zeros            number of x == 0 (either sign)
//
// Stage 1 (activation_stats_planes): one 256-thread block per (tensor, sample, channel) plane, found by binary search over the
// descriptors' plane0; one partial row per plane in the workspace.  Stage 2 (activation_stats_finish): one wave per output
// (segment, row); lane l adds samples b0 + l, b0 + l + 64, ... of the segment in ascending order and the lanes meet in the usual
// butterfly.  No atomics, every combination in a fixed order.
//
// Placement independence: a plane of H*W floats starts wherever (n*C + c)*H*W lands -- at 97 x 97 or 769 x 769 on every 4-byte
// phase -- and activations are fresh allocations on every forward.  Element i of a plane belongs to thread (i / 4) % 256, which
// takes its quads in ascending order and the four elements of a quad in ascending order, whatever the address: every full quad is
// ONE dwordx4 load declared 4-byte aligned (the hardware takes it at any dword phase), and the last 1..3 elements of a plane are
// read one by one, so no load touches an element outside its own plane and there is one code path, not an aligned and a
// misaligned one.  x^2 is exact in double (48 significant bits), so fma(d, d, acc) is acc + d*d in one instruction.
//
// Registers: four quads in flight per thread (16 VGPRs), seven accumulators; no scratch, <= 64 VGPRs (8 waves per SIMD).
#include <climits>

#include "common.hpp"

namespace dasac {

constexpr int kActCols = 6;
constexpr int kActBlock = 256;
constexpr int kActMaxSegments = 8;
constexpr int kActMaxTensors = 1 << 16;
constexpr int64_t kActMaxPlane = 1ll << 30;      // floats per plane: 32-bit byte offsets inside a plane
constexpr double kActNone = 0x1p62;      // "no non-finite entry": above every index

struct ActTensor {      // one 32-byte row of `tensors`
  const float* x;
  int64_t HW;
  int32_t C, row0;
  int64_t plane0;
};
static_assert(sizeof(ActTensor) == 32, "dasac_activation_stats: 32-byte descriptor rows");

// activations are global memory; a pointer read from a descriptor row is a generic one to the compiler (flat loads) unless told.
// A plane is addressed as "scalar plane base + 32-bit byte offset": planes of up to 2^30 floats, no 64-bit address per load.
typedef const char __attribute__((address_space(1)))* act_gptr;
__device__ __forceinline__ f32x4u act_load4(act_gptr plane, unsigned i) {
  return *reinterpret_cast<const f32x4u __attribute__((address_space(1)))*>(plane + i * 4u);
}
__device__ __forceinline__ float act_load1(act_gptr plane, unsigned i) {
  return *reinterpret_cast<const float __attribute__((address_space(1)))*>(plane + i * 4u);
}

struct ActAcc {
  double sum = 0, sumsq = 0;
  float maxabs = 0.f;
  int nonfinite = 0, zeros = 0;
  int first = INT_MAX;      // index inside the plane
};

__device__ __forceinline__ void act_take(ActAcc& a, float v, int i) {
  const bool fin = isfinite(v);
  const double d = fin ? (double)v : 0.0;
  a.sum += d;
  a.sumsq = fma(d, d, a.sumsq);
  a.maxabs = fmaxf(a.maxabs, fin ? fabsf(v) : 0.f);
  a.zeros += v == 0.f;
  a.nonfinite += !fin;
  if (!fin) a.first = i < a.first ? i : a.first;
}

__device__ __forceinline__ void act_take4(ActAcc& a, f32x4u v, int i) {
#pragma unroll
  for (int e = 0; e < 4; ++e) act_take(a, v[e], i + e);
}

// the last row whose `key` (plane0 or row0) is <= v; rows are in ascending key order and row 0 has key 0
template <typename Key>
__device__ __forceinline__ int act_find(const ActTensor* __restrict__ tensors, int n_tensors, int64_t v, Key key) {
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key(tensors[mid]) <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kActBlock) void activation_stats_planes(const ActTensor* __restrict__ tensors, int n_tensors, int N,
                                                                     double* __restrict__ partial) {
  const int64_t plane = blockIdx.x;
  const ActTensor T = tensors[act_find(tensors, n_tensors, plane, [](const ActTensor& t) { return t.plane0; })];
  const int64_t local = plane - T.plane0;      // n*C + c
  const int64_t HW = T.HW;
  ActAcc a;
  if (local < (int64_t)N * T.C && HW > 0 && HW <= kActMaxPlane) {      // (a table that does not add up to the grid: zeros, never a read outside a tensor)
    const act_gptr x = (act_gptr)(uintptr_t)(T.x + local * HW);
    const int n = (int)HW, quads = n >> 2;
    int q = threadIdx.x;
    for (; q + 3 * kActBlock < quads; q += 4 * kActBlock) {      // four quads in flight
      f32x4u v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = act_load4(x, 4 * (q + u * kActBlock));
#pragma unroll
      for (int u = 0; u < 4; ++u) act_take4(a, v[u], 4 * (q + u * kActBlock));
    }
    for (; q < quads; q += kActBlock) act_take4(a, act_load4(x, 4 * q), 4 * q);
    if (q == quads)      // the thread whose next quad is the plane's partial one: its last 1..3 elements, one by one
      for (int i = 4 * quads; i < n; ++i) act_take(a, act_load1(x, i), i);
  }
  __shared__ double red[kActBlock / kWave][kActCols];
  const double s = wave_sum(a.sum), sq = wave_sum(a.sumsq), mx = wave_max((double)a.maxabs);
  const double nf = wave_sum((double)a.nonfinite), zr = wave_sum((double)a.zeros);
  const double fi = wave_min(a.first == INT_MAX ? kActNone : (double)a.first);
  if ((threadIdx.x & 63) == 0) {
    double* r = red[threadIdx.x >> 6];
    r[0] = s, r[1] = sq, r[2] = mx, r[3] = nf, r[4] = fi, r[5] = zr;
  }
  __syncthreads();
  if (threadIdx.x < kActCols) {      // one column per thread, the four waves in a fixed order
    const int c = threadIdx.x;
    const double w0 = red[0][c], w1 = red[1][c], w2 = red[2][c], w3 = red[3][c];
    double v;
    if (c == 2) v = fmax(fmax(w0, w1), fmax(w2, w3));
    else if (c == 4) {
      v = fmin(fmin(w0, w1), fmin(w2, w3));
      v = v < kActNone ? v + 1.0 : 0.0;      // 1 + index inside the plane; the finish adds the plane's start
    } else v = (w0 + w1) + (w2 + w3);
    partial[plane * kActCols + c] = v;
  }
}

// grid (R, n_segments), one wave each.  seg_bounds is device memory the host never saw: clamped to 0..N, so a bad table gives a
// wrong row, never a read outside the workspace.
__global__ __launch_bounds__(kWave) void activation_stats_finish(const ActTensor* __restrict__ tensors, int n_tensors, int N, int R,
                                                                 const int32_t* __restrict__ seg_bounds,
                                                                 const double* __restrict__ partial, double* __restrict__ table) {
  const int row = blockIdx.x, seg = blockIdx.y;
  const ActTensor T = tensors[act_find(tensors, n_tensors, row, [](const ActTensor& t) { return (int64_t)t.row0; })];
  const int c = row - T.row0;
  const int b0 = min(max(seg_bounds[seg], 0), N), b1 = min(max(seg_bounds[seg + 1], 0), N);
  double s = 0, sq = 0, mx = 0, nf = 0, zr = 0, first = kActNone;
  if (c < T.C) {
    for (int n = b0 + threadIdx.x; n < b1; n += kWave) {
      const int64_t local = (int64_t)n * T.C + c;
      const double* r = partial + (T.plane0 + local) * kActCols;
      s += r[0], sq += r[1], nf += r[3], zr += r[5];
      mx = fmax(mx, r[2]);
      if (r[4] > 0) first = fmin(first, (double)(local * T.HW) + r[4]);
    }
  }
  s = wave_sum(s), sq = wave_sum(sq), nf = wave_sum(nf), zr = wave_sum(zr);
  mx = wave_max(mx), first = wave_min(first);
  if (threadIdx.x == 0) {
    double* out = table + ((size_t)seg * R + row) * kActCols;
    out[0] = s, out[1] = sq, out[2] = mx, out[3] = nf, out[4] = first < kActNone ? first : 0.0, out[5] = zr;
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" size_t dasac_activation_stats_workspace(int64_t n_planes) {
  return n_planes > 0 ? (size_t)n_planes * kActCols * sizeof(double) : 0;
}

extern "C" int dasac_activation_stats(const void* tensors, int n_tensors, int N, int R, const int32_t* seg_bounds, int n_segments,
                                      void* workspace, size_t workspace_bytes, double* table, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && seg_bounds && workspace && table, "activation_stats: null pointer");
  DASAC_REQUIRE(n_tensors >= 1 && n_tensors <= kActMaxTensors, "activation_stats: 1..%d tensors (got %d)", kActMaxTensors, n_tensors);
  DASAC_REQUIRE(N >= 1 && R >= n_tensors, "activation_stats: N >= 1 samples and R >= n_tensors channel rows (got N=%d, R=%d)", N, R);
  DASAC_REQUIRE(n_segments >= 1 && n_segments <= kActMaxSegments && n_segments <= N,
                "activation_stats: 1..%d non-empty segments of N=%d samples (got %d)", kActMaxSegments, N, n_segments);
  const int64_t n_planes = (int64_t)N * R;
  DASAC_REQUIRE(n_planes < (1ll << 31), "activation_stats: N*R = %lld planes exceed one grid", (long long)n_planes);
  DASAC_REQUIRE((((uintptr_t)tensors | (uintptr_t)workspace | (uintptr_t)table) & 7) == 0 && ((uintptr_t)seg_bounds & 3) == 0,
                "activation_stats: misaligned descriptors / workspace / table / seg_bounds");
  DASAC_REQUIRE(workspace_bytes >= dasac_activation_stats_workspace(n_planes), "activation_stats: workspace too small");
  hipStream_t s = as_stream(stream);
  const ActTensor* rows = reinterpret_cast<const ActTensor*>(tensors);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(activation_stats_planes, dim3((unsigned)n_planes), dim3(kActBlock), 0, s, rows, n_tensors, N, partial);
  DASAC_CHECK_LAUNCH("activation_stats_planes");
  hipLaunchKernelGGL(activation_stats_finish, dim3(R, n_segments), dim3(kWave), 0, s, rows, n_tensors, N, R, seg_bounds, partial, table);
  DASAC_CHECK_LAUNCH("activation_stats_finish");
  return DASAC_OK;
}
