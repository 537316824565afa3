// Winograd for the wide dilated 3x3 convolutions (conv2 of layer3 and layer4 of the ResNet-101 backbone: 256 -> 256 at dilation 2,
// 512 -> 512 at dilation 4, 97x97 maps; models/deeplabv2.py:65-66), UNFUSED: streaming transform kernels around the existing GEMMs.
// ONE kernel family in TWO forms, F(2x2,3x3) (struct F2: 16 points per 2x2-output tile) and F(4x4,3x3) (struct F4: 36 points per
// 4x4-output tile); a form is its five 1-D rows and its tile size, everything else is written once.  With P points and N = TM + 2:
//
//   filter transform   U[pt] = G g G^T per (cout, cin), frozen-BN scale folded in, written as the packed operand of a 1x1 conv
//   input transform    V[pt][c][tile] = (B^T d B)[pt] of the N x N patch (stride = dilation) of every tile
//   P point GEMMs      Y[pt][m][tile] = sum_c U[pt][m][c] * V[pt][c][tile]          (dasac_conv_gemm, 1x1, H = 1, W = tiles)
//   output transform   out[n][m][y][x] = epi((A^T Y A)[ey][ex]) -- shift, ReLU, ReLU bits recorded or consumed
//
// and the weight gradient as the exact adjoint, dW = G^T [sum over tiles (A dY A^T) (.) (B^T d B)] G:
//
//   grad transform     dM[pt][m][tile] = (A dY A^T)[pt] of every tile's TM x TM output pixels
//   P contractions     S[split][pt][m][c] = sum over the split's tiles of dM[pt][m][t] * V[pt][c][t]   (dasac_conv_wgrad_batched, ONE launch)
//   finish             dW[m][c] = scale[m] * G^T (sum_split S) G, the frozen BN's dot rows and sum of dz
//
// F(2x2) spends 2.25 x fewer multiplies than the direct contraction, F(4x4) 1.71 x fewer again with transformed tensors of 0.59
// times the size, at 2 - 4 x the direct kernel's error against float64: the weight gradient runs as F(4x4) wherever it measured
// faster, the forward and the data gradient per measured route (ops.WINOGRAD4_ROUTES; profiles/EXPERIMENTS.md).  The price of either
// is two passes over [P][C][tiles] tensors.  No new matrix kernel.  Only the output transform is two kernels (see there).
// Index arithmetic lives in winograd_index.hpp and is walked on the host by tools/winograd_index_check.cpp.  Every global access
// goes through a buffer descriptor of the tensor's exact extent with the whole offset in the per-lane operand (the scalar
// offset is not range checked by the hardware): an offset past the extent reads zero / stores nothing.
// The library is built without contraction and without fast-math, and tests/test_gpu_winograd_bits.py pins every result bit: the
// rows below ARE the summation order, parentheses included.
#include "conv_common.hpp"
#include "winograd_index.hpp"

namespace dasac {
namespace wino {

constexpr int kBlock = 256;

// (make_rsrc: conv_common.hpp)
__device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, unsigned voff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}
__device__ __forceinline__ void st(__amdgpu_buffer_rsrc_t r, unsigned voff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, 0, 0);
}

// ---- the two forms -----------------------------------------------------------------------------------------------------------
// TM outputs per tile and axis, N = TM + 2 points per axis, P = N * N points; kPaddedT: Geom::T is rounded up and the padding tiles
// are written as zeros.  The 1-D rows: bt = B^T (N -> N), a = A (TM -> N), g = G (3 -> N), gt = G^T (N -> 3), at = A^T (N -> TM).
//
// F(2x2,3x3), evaluation points 0, 1, -1, inf:
//   B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]   A = [[1,0],[1,1],[1,-1],[0,-1]]   G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
// (no `at`: its output transform, one thread per pixel, applies the signs of A^T per lane)
struct F2 {
  static constexpr int TM = 2, N = TM + 2, P = kPoints<TM>;
  static constexpr bool kPaddedT = wino::kPaddedT<TM>;
  static __device__ __forceinline__ void bt(const float (&d)[4], float (&o)[4]) {
    o[0] = d[0] - d[2];
    o[1] = d[1] + d[2];
    o[2] = d[2] - d[1];
    o[3] = d[1] - d[3];
  }
  static __device__ __forceinline__ void a(const float (&y)[2], float (&o)[4]) {
    o[0] = y[0];
    o[1] = y[0] + y[1];
    o[2] = y[0] - y[1];
    o[3] = -y[1];
  }
  static __device__ __forceinline__ void g(const float (&w)[3], float (&o)[4]) {
    o[0] = w[0];
    o[1] = 0.5f * ((w[0] + w[2]) + w[1]);
    o[2] = 0.5f * ((w[0] + w[2]) - w[1]);
    o[3] = w[2];
  }
  static __device__ __forceinline__ void gt(const float (&p)[4], float (&o)[3]) {
    o[0] = p[0] + 0.5f * (p[1] + p[2]);
    o[1] = 0.5f * (p[1] - p[2]);
    o[2] = 0.5f * (p[1] + p[2]) + p[3];
  }
};

// F(4x4,3x3), evaluation points 0, 1, -1, 2, -1/2, inf, chosen for the weight gradient's error against float64
// (profiles/EXPERIMENTS.md); B^T scaled to integers and G carrying the inverse factors:
//   B^T = [[2,3,-4,-3,2,0],[0,2,5,1,-2,0],[0,2,1,-5,2,0],[0,-1,-2,1,2,0],[0,-2,1,2,-1,0],[0,2,3,-4,-3,2]]
//   A   = [[1,0,0,0],[1,1,1,1],[1,-1,1,-1],[1,2,4,8],[1,-1/2,1/4,-1/8],[0,0,0,1]]
//   G   = [[1/2,0,0],[1/6,1/6,1/6],[1/6,-1/6,1/6],[1/30,1/15,2/15],[16/15,-8/15,4/15],[0,0,1/2]]
// (tests/winograd4_ref.py holds them as fractions and checks the identities in float64)
struct F4 {
  static constexpr int TM = 4, N = TM + 2, P = kPoints<TM>;
  static constexpr bool kPaddedT = wino::kPaddedT<TM>;
  static constexpr float k6 = 1.f / 6.f, k15 = 1.f / 15.f, k30 = 1.f / 30.f;
  static __device__ __forceinline__ void bt(const float (&d)[6], float (&o)[6]) {
    o[0] = (2.f * (d[0] + d[4]) + 3.f * (d[1] - d[3])) - 4.f * d[2];
    o[1] = (2.f * (d[1] - d[4]) + 5.f * d[2]) + d[3];
    o[2] = (2.f * (d[1] + d[4]) + d[2]) - 5.f * d[3];
    o[3] = (d[3] - d[1]) + 2.f * (d[4] - d[2]);
    o[4] = 2.f * (d[3] - d[1]) + (d[2] - d[4]);
    o[5] = (2.f * (d[1] + d[5]) + 3.f * (d[2] - d[4])) - 4.f * d[3];
  }
  static __device__ __forceinline__ void a(const float (&y)[4], float (&o)[6]) {
    o[0] = y[0];
    o[1] = (y[0] + y[2]) + (y[1] + y[3]);
    o[2] = (y[0] + y[2]) - (y[1] + y[3]);
    o[3] = (y[0] + 4.f * y[2]) + (2.f * y[1] + 8.f * y[3]);
    o[4] = (y[0] + 0.25f * y[2]) - (0.5f * y[1] + 0.125f * y[3]);
    o[5] = y[3];
  }
  static __device__ __forceinline__ void g(const float (&w)[3], float (&o)[6]) {
    o[0] = 0.5f * w[0];
    o[1] = k6 * ((w[0] + w[2]) + w[1]);
    o[2] = k6 * ((w[0] + w[2]) - w[1]);
    o[3] = (k30 * w[0] + k15 * w[1]) + (2.f * k15) * w[2];
    o[4] = ((16.f * k15) * w[0] - (8.f * k15) * w[1]) + (4.f * k15) * w[2];
    o[5] = 0.5f * w[2];
  }
  static __device__ __forceinline__ void gt(const float (&p)[6], float (&o)[3]) {
    o[0] = (0.5f * p[0] + k6 * (p[1] + p[2])) + (k30 * p[3] + (16.f * k15) * p[4]);
    o[1] = k6 * (p[1] - p[2]) + (k15 * p[3] - (8.f * k15) * p[4]);
    o[2] = (k6 * (p[1] + p[2]) + 0.5f * p[5]) + ((2.f * k15) * p[3] + (4.f * k15) * p[4]);
  }
  static __device__ __forceinline__ void at(const float (&y)[6], float (&o)[4]) {
    o[0] = (y[0] + (y[1] + y[2])) + (y[3] + y[4]);
    o[1] = (y[1] - y[2]) + (2.f * y[3] - 0.5f * y[4]);
    o[2] = (y[1] + y[2]) + (4.f * y[3] + 0.25f * y[4]);
    o[3] = ((y[1] - y[2]) + y[5]) + (8.f * y[3] - 0.125f * y[4]);
  }
};

// The shared kernels load their patch a row at a time (the taps of a row are neighbours in memory; issuing them column by column
// measured 8 % slower on the F(2x2) input transform) and make both passes column first: the rows of a form on every column of the
// patch, then on every row of the result.

// ---- filter transform ------------------------------------------------------------------------------------------------------
// One thread per element (k, m) of the packed [Kpad/4][Mpad][4] matrix; it writes all P points (K and M padding as zeros).
// mode 0 (forward): m = cout, k = cin, g = w[m][k] * scale[m].   mode 1 (data gradient): m = cin, k = cout,
// g = rot180(w[k][m]) * scale[k].   U = G g G^T.
template <class F>
__global__ __launch_bounds__(kBlock) void filter_transform(const float* __restrict__ Wt, const float* __restrict__ scale,
                                                            float* __restrict__ U, int Cout, int Cin, int Mpad, int Kpad, int mode,
                                                            unsigned w_bytes, unsigned u_bytes) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;      // == offset inside one point's packed matrix
  const int per_point = Kpad * Mpad;
  if (idx >= per_point) return;
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(Wt, w_bytes), ru = make_rsrc(U, u_bytes);
  const int row4 = Mpad * 4;
  const int kq = idx / row4, rem = idx - kq * row4;
  const int m = rem >> 2, k = kq * 4 + (rem & 3);
  const int M = mode == 0 ? Cout : Cin, K = mode == 0 ? Cin : Cout;
  const bool real = m < M && k < K;
  const int co = mode == 0 ? m : k, ci = mode == 0 ? k : m;
  const float s = (real && scale) ? ld(make_rsrc(scale, (unsigned)Cout * 4u), (unsigned)co * 4u) : 1.f;
  float w[3][3];                                           // the filter, loaded a row at a time
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tap = mode == 0 ? a * 3 + b : (2 - a) * 3 + (2 - b);
      w[a][b] = ld(rw, real ? (unsigned)((co * Cin + ci) * 9 + tap) * 4u : kOutside) * s;
    }
  float t[F::N][3];                                        // G g
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    float g[3], o[F::N];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = w[a][b];
    F::g(g, o);
#pragma unroll
    for (int a = 0; a < F::N; ++a) t[a][b] = o[a];
  }
#pragma unroll
  for (int a = 0; a < F::N; ++a) {
    float u[F::N];
    F::g(t[a], u);
#pragma unroll
    for (int b = 0; b < F::N; ++b) st(ru, (unsigned)((a * F::N + b) * per_point + idx) * 4u, u[b]);
  }
}

// (channel, tile) of a thread of the per-tile kernels, grid (ceil(T / 256), channels): lanes along tiles.  False: nothing left to
// do -- past T, or a padding tile, whose P points at `r` this writes as zeros.
template <class F>
__device__ __forceinline__ bool tile_thread(const Geom& g, __amdgpu_buffer_rsrc_t r, int channels, int& c, int& tile) {
  tile = blockIdx.x * kBlock + threadIdx.x;
  c = blockIdx.y;
  if (tile >= g.T) return false;
  if constexpr (F::kPaddedT)
    if (!real_tile(g, tile)) {
#pragma unroll
      for (int pt = 0; pt < F::P; ++pt) st(r, point_offset(g, channels, pt, c, tile), 0.f);
      return false;
    }
  return true;
}

// ---- input transform -------------------------------------------------------------------------------------------------------
// grid (ceil(T / 256), C): one thread per (channel, tile), lanes along tiles.  V = B^T d B of the N x N patch (taps `dilation`
// apart), P stores.
template <class F>
__global__ __launch_bounds__(kBlock) void input_transform(const float* __restrict__ X, float* __restrict__ V, Geom g, int C,
                                                           unsigned x_bytes, unsigned v_bytes) {
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(X, x_bytes), rv = make_rsrc(V, v_bytes);
  int c, tile;
  if (!tile_thread<F>(g, rv, C, c, tile)) return;
  int n, y0, x0;
  tile_origin<F::TM>(g, tile, n, y0, x0);
  float p[F::N][F::N];                                     // the patch, loaded a row at a time: the taps of a row share cache lines
#pragma unroll
  for (int ky = 0; ky < F::N; ++ky)
#pragma unroll
    for (int kx = 0; kx < F::N; ++kx) p[ky][kx] = ld(rx, patch_offset(g, C, n, c, y0, x0, ky, kx));
  float t[F::N][F::N];                                     // B^T d
#pragma unroll
  for (int kx = 0; kx < F::N; ++kx) {
    float d[F::N], o[F::N];
#pragma unroll
    for (int ky = 0; ky < F::N; ++ky) d[ky] = p[ky][kx];
    F::bt(d, o);
#pragma unroll
    for (int a = 0; a < F::N; ++a) t[a][kx] = o[a];
  }
#pragma unroll
  for (int a = 0; a < F::N; ++a) {
    float v[F::N];
    F::bt(t[a], v);
#pragma unroll
    for (int b = 0; b < F::N; ++b) st(rv, point_offset(g, C, a * F::N + b, c, tile), v[b]);
  }
}

// ---- weight gradient: transform of dY ----------------------------------------------------------------------------------------
// The adjoint of the output transform.  grid (ceil(T / 256), M): one thread per (channel, tile), lanes along tiles, tiles numbered as
// input_transform numbers them.  dM = A dY A^T of the tile's TM x TM output pixels; output (ey, ex) is tap (ey + 1, ex + 1) of the
// tile's patch, so a pixel of a tile that hangs over the map edge takes patch_offset's zero.
template <class F>
__global__ __launch_bounds__(kBlock) void grad_transform(const float* __restrict__ dY, float* __restrict__ dM, Geom g, int M,
                                                          unsigned y_bytes, unsigned m_bytes) {
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(dY, y_bytes), rm = make_rsrc(dM, m_bytes);
  int m, tile;
  if (!tile_thread<F>(g, rm, M, m, tile)) return;
  int n, y0, x0;
  tile_origin<F::TM>(g, tile, n, y0, x0);
  float p[F::TM][F::TM];                                   // the tile's pixels, loaded a row at a time
#pragma unroll
  for (int ey = 0; ey < F::TM; ++ey)
#pragma unroll
    for (int ex = 0; ex < F::TM; ++ex) p[ey][ex] = ld(ry, patch_offset(g, M, n, m, y0, x0, ey + 1, ex + 1));
  float t[F::N][F::TM];                                    // A dY
#pragma unroll
  for (int ex = 0; ex < F::TM; ++ex) {
    float d[F::TM], o[F::N];
#pragma unroll
    for (int ey = 0; ey < F::TM; ++ey) d[ey] = p[ey][ex];
    F::a(d, o);
#pragma unroll
    for (int a = 0; a < F::N; ++a) t[a][ex] = o[a];
  }
#pragma unroll
  for (int a = 0; a < F::N; ++a) {
    float v[F::N];
    F::a(t[a], v);
#pragma unroll
    for (int b = 0; b < F::N; ++b) st(rm, point_offset(g, M, a * F::N + b, m, tile), v[b]);
  }
}

// ---- weight gradient: finish -------------------------------------------------------------------------------------------------
// S [splits][P][M][C] (the batched point contraction's slabs), Ssum [splits][M] (channel sums of point (1,1) of dM, whose row of A
// is all ones = sum of dz) -> dW[co][ci][3][3] = scale[co] * (G^T (sum_s S[s]) G), dot[blockIdx.x][co] = this block's part of
// sum W * (unscaled gradient), sum_dz[co] = sum_s Ssum[s][co]: dot and sum_dz exactly as dasac_conv_wgrad_finish leaves them.
// grid (C / 64, M), 256 threads = 64 input channels x 4 split lanes; a thread adds the splits s = lane, lane + 4, ... of its
// channel's P points, the four lanes meet in LDS in a fixed order, and the block writes its 64 x 9 gradients as one contiguous run
// of dW.
template <class F>
__global__ __launch_bounds__(kBlock) void wgrad_finish(const float* __restrict__ S, const float* __restrict__ Ssum, int splits, int M,
                                                        int C, const float* __restrict__ Wt, const float* __restrict__ scale,
                                                        float* __restrict__ dW, float* __restrict__ dot, float* __restrict__ sum_dz,
                                                        unsigned s_bytes, unsigned w_bytes) {
  const int co = blockIdx.y, ci0 = blockIdx.x * 64;
  const int tx = threadIdx.x, c = tx & 63, q = tx >> 6;
  const __amdgpu_buffer_rsrc_t rp = make_rsrc(S, s_bytes), rw = make_rsrc(Wt, w_bytes), rd = make_rsrc(dW, w_bytes);
  if (sum_dz && blockIdx.x == 0 && q == 0) {                 // one wave: the splits' channel sums in parallel
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(Ssum, (unsigned)(splits * M) * 4u);
    float sv = 0.f;
    for (int s = c; s < splits; s += 64) sv += ld(rs, (unsigned)(s * M + co) * 4u);
    sv = wave_sum(sv);
    if (c == 0) st(make_rsrc(sum_dz, (unsigned)M * 4u), (unsigned)co * 4u, sv);
  }
  __shared__ float red[4][F::P][64];
  __shared__ float grad[64 * 9];
  float acc[F::P];
#pragma unroll
  for (int pt = 0; pt < F::P; ++pt) acc[pt] = 0.f;
  const unsigned point = (unsigned)(M * C), slab = (unsigned)F::P * point;
  const unsigned e0 = (unsigned)(co * C + ci0 + c);
  for (int s = q; s < splits; s += 4)
#pragma unroll
    for (int pt = 0; pt < F::P; ++pt) acc[pt] += ld(rp, ((unsigned)s * slab + (unsigned)pt * point + e0) * 4u);
#pragma unroll
  for (int pt = 0; pt < F::P; ++pt) red[q][pt][c] = acc[pt];
  __syncthreads();
  if (q == 0) {
    float r[3][F::N];                                      // G^T (sum of the splits)
#pragma unroll
    for (int b = 0; b < F::N; ++b) {
      float p[F::N], o[3];
#pragma unroll
      for (int a = 0; a < F::N; ++a)
        p[a] = (red[0][a * F::N + b][c] + red[1][a * F::N + b][c]) + (red[2][a * F::N + b][c] + red[3][a * F::N + b][c]);
      F::gt(p, o);
#pragma unroll
      for (int a = 0; a < 3; ++a) r[a][b] = o[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float o[3];
      F::gt(r[a], o);
#pragma unroll
      for (int b = 0; b < 3; ++b) grad[c * 9 + a * 3 + b] = o[b];
    }
  }
  __syncthreads();
  const float sc = scale ? ld(make_rsrc(scale, (unsigned)M * 4u), (unsigned)co * 4u) : 1.f;
  float part = 0.f;
  for (int e = tx; e < 64 * 9; e += kBlock) {
    const unsigned off = ((unsigned)(co * C + ci0) * 9u + (unsigned)e) * 4u;
    if (dot) part += grad[e] * ld(rw, off);
    st(rd, off, grad[e] * sc);
  }
  if (dot) {
    __shared__ float redd[4];
    part = wave_sum(part);
    if (c == 0) redd[q] = part;
    __syncthreads();
    if (tx == 0) st(make_rsrc(dot, (unsigned)((C / 64) * M) * 4u), (unsigned)(blockIdx.x * M + co) * 4u, (redd[0] + redd[1]) + (redd[2] + redd[3]));
  }
}

// ---- output transform ------------------------------------------------------------------------------------------------------
// The one transform that is a kernel per form.  F(2x2) runs one thread per OUTPUT element and takes the recorded ReLU bits from a
// wave ballot; F(4x4) would load up to 36 points for one output that way, runs one thread per TILE, and records the bits in a second
// pass (relu_bits_pack).  Both end in record_bits.

// bits[m][pix >> 5] bit (pix & 31) = `positive` of the thread of flattened pixel pix = n*HW + rem, lanes along pixels (the layout of
// conv_gemm.hip's Epilogue): a wave ballot is two mask words, stored by lanes 0 and 32; a word whose 32 pixels all lie past the last
// pixel does not exist, the bits past the last pixel of the last word are zeros (`positive` is false there).
__device__ __forceinline__ void record_bits(unsigned* obits, unsigned bits_bytes, int m, int w32, int pix, bool positive) {
  const unsigned long long ballot = __builtin_amdgcn_ballot_w64(positive);
  const int lane = threadIdx.x & 63, wcol = pix >> 5;
  if ((lane & 31) == 0 && wcol < w32)
    __builtin_amdgcn_raw_buffer_store_b32((unsigned)(lane ? ballot >> 32 : ballot), make_rsrc(obits, bits_bytes), out_bits_offset(m, w32, pix), 0, 0);
}

// F(2x2).  grid (ceil(N*H*W / 256), M): one thread per output element, lanes along the flattened (n, y, x) pixel index -- the pixel
// axis of the ReLU bit masks.  Output (ey, ex) of a tile is sum_j sum_k sy_j sx_k Y[ey + j][ex + k], signs (+,+,+) for e = 0 and
// (+,-,-) for e = 1 (A^T = [[1,1,1,0],[0,1,-1,-1]]): nine loads; the four outputs of a tile re-read its values from cache.
// BITS: 0 none, 1 record (v > 0 after the ReLU), 2 mask (v = bit ? v : 0).
template <int BITS>
__global__ __launch_bounds__(kBlock) void output_transform(const float* __restrict__ Y, float* __restrict__ Out, Geom g, int M,
                                                            const float* __restrict__ shift, int relu,
                                                            const unsigned* __restrict__ mbits, unsigned* __restrict__ obits,
                                                            int w32, unsigned y_bytes, unsigned out_bytes, unsigned bits_bytes) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  const int m = blockIdx.y;
  const bool live = pix < g.N * g.HW;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(Y, y_bytes), ro = make_rsrc(Out, out_bytes);
  int n = 0, rem = 0, tile = 0, ey = 0, ex = 0;
  if (live) pixel_tile(g, pix, n, rem, tile, ey, ex);
  float v[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[j][k] = ld(ry, live ? point_offset(g, M, (ey + j) * 4 + ex + k, m, tile) : kOutside);
  const float sy = ey ? -1.f : 1.f, sx = ex ? -1.f : 1.f;
  float row[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) row[j] = (v[j][0] + sx * v[j][1]) + sx * v[j][2];
  float o = (row[0] + sy * row[1]) + sy * row[2];
  if (shift) o = o + ld(make_rsrc(shift, (unsigned)M * 4u), (unsigned)m * 4u);
  if (relu) o = fmaxf(o, 0.f);
  if constexpr (BITS == 2) {
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(mbits, bits_bytes);
    const unsigned word = __builtin_amdgcn_raw_buffer_load_b32(rb, live ? out_bits_offset(m, w32, pix) : kOutside, 0, 0);
    o = (word >> (pix & 31)) & 1u ? o : 0.f;
  }
  st(ro, live ? out_offset(g, M, n, m, rem) : kOutside, o);
  if constexpr (BITS == 1) record_bits(obits, bits_bytes, m, w32, pix, live && o > 0.f);
}

// F(4x4): out = epi(A^T Y A) over Y [36][M][T].  grid (ceil(T / 256), M): one thread per (channel, tile), lanes along tiles, the
// mapping of input_transform and grad_transform -- 36 loads for 16 outputs (2.25 per output; one thread per output element would
// load up to 36 for one), each load a run of 64 consecutive tiles of one point.  Consecutive tile numbers are consecutive phases, so
// a store instruction writes runs of `d` adjacent floats and the four stores of an output row fill each other's gaps: the mirror of
// what grad_transform reads.  Padding tiles and overhanging outputs store nothing.
// MASK: the elements whose bit in `mbits` is clear become zero.  The price of the mapping is that a wave no longer holds 64
// consecutive pixels, so the RECORDED ReLU bits cannot be a ballot here: relu_bits_pack below reads the stored output back.  (Adding
// the bits into zeroed words with buffer atomics, one per run of outputs that share a word, was built and measured: 0.40 ms for the
// layer4 launch against 0.12 ms without bits -- the atomics are per lane at the L2; the second pass costs 0.07 ms.)
template <bool MASK>
__global__ __launch_bounds__(kBlock) void output_transform4(const float* __restrict__ Y, float* __restrict__ Out, Geom g, int M,
                                                             const float* __restrict__ shift, int relu,
                                                             const unsigned* __restrict__ mbits, int w32, unsigned y_bytes,
                                                             unsigned out_bytes, unsigned bits_bytes) {
  using F = F4;
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (!real_tile(g, tile)) return;
  const int m = blockIdx.y;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(Y, y_bytes), ro = make_rsrc(Out, out_bytes);
  int n, y0, x0;
  tile_origin<F::TM>(g, tile, n, y0, x0);
  float t[F::TM][F::N];                                    // A^T Y, a column of the points at a time
#pragma unroll
  for (int b = 0; b < F::N; ++b) {
    float v[F::N], o[F::TM];
#pragma unroll
    for (int a = 0; a < F::N; ++a) v[a] = ld(ry, point_offset(g, M, a * F::N + b, m, tile));
    F::at(v, o);
#pragma unroll
    for (int e = 0; e < F::TM; ++e) t[e][b] = o[e];
  }
  const float sh = shift ? ld(make_rsrc(shift, (unsigned)M * 4u), (unsigned)m * 4u) : 0.f;
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(mbits, MASK ? bits_bytes : 0u);
#pragma unroll
  for (int ey = 0; ey < F::TM; ++ey) {
    float o[F::TM];
    F::at(t[ey], o);
    const int y = y0 + ey * g.ay.d;
#pragma unroll
    for (int ex = 0; ex < F::TM; ++ex) {
      const int x = x0 + ex * g.ax.d;
      const bool in = y < g.H && x < g.W;
      const int rem = y * g.W + x, pix = n * g.HW + rem;
      float v = o[ex];
      if (shift) v = v + sh;
      if (relu) v = fmaxf(v, 0.f);
      if constexpr (MASK) {
        const unsigned word = __builtin_amdgcn_raw_buffer_load_b32(rb, in ? out_bits_offset(m, w32, pix) : kOutside, 0, 0);
        v = (word >> (pix & 31)) & 1u ? v : 0.f;
      }
      st(ro, in ? out_offset(g, M, n, m, rem) : kOutside, v);
    }
  }
}

// The ReLU pattern of a stored activation.  grid (ceil(N*H*W / 256), M): one thread per element, lanes along pixels; every word is
// written.
__global__ __launch_bounds__(kBlock) void relu_bits_pack(const float* __restrict__ Out, unsigned* __restrict__ obits, Geom g, int M,
                                                          int w32, unsigned out_bytes, unsigned bits_bytes) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  const int m = blockIdx.y;
  const bool live = pix < g.N * g.HW;
  const int n = live ? div(pix, g.by_hw) : 0;
  const float v = ld(make_rsrc(Out, out_bytes), live ? out_offset(g, M, n, m, pix - n * g.HW) : kOutside);
  record_bits(obits, bits_bytes, m, w32, pix, live && v > 0.f);
}

}  // namespace wino
}  // namespace dasac

using namespace dasac;
using dasac::wino::F2;
using dasac::wino::F4;
using dasac::wino::Geom;

// ---- entry points: one body per pair, the form as a template parameter, `who` = the exported name without its prefix ------------
// Geometry of an activation of C channels and of its transformed tensor [P][C][T]
template <class F>
static int wino_geom(Geom& g, const char* who, int Nb, int C, int H, int W, int dilation) {
  DASAC_REQUIRE(Nb > 0 && C > 0 && H > 0 && W > 0 && dilation > 0, "%s: bad geometry", who);
  DASAC_REQUIRE((int64_t)Nb * H * W < (1ll << 30), "%s: more than 2^30 pixels", who);
  g = wino::make_geom<F::TM>(Nb, H, W, dilation);
  DASAC_REQUIRE(F::P * (int64_t)C * g.T * 4 <= wino::kMaxBytes && (int64_t)C * Nb * H * W * 4 <= wino::kMaxBytes,
                "%s: a tensor exceeds the 4 GiB buffer-descriptor window", who);
  DASAC_REQUIRE(C <= 65535, "%s: more than 65535 channels", who);
  return DASAC_OK;
}

template <class F>
static int tiles_impl(int Nb, int H, int W, int dilation) {
  if (Nb <= 0 || H <= 0 || W <= 0 || dilation <= 0) return 0;
  const int64_t t = (int64_t)Nb * wino::make_axis<F::TM>(H, dilation).tiles * wino::make_axis<F::TM>(W, dilation).tiles;
  return t < (1ll << 30) ? (int)wino::padded_tiles<F::TM>(t) : 0;
}

template <class F>
static int filter_impl(const char* who, const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                       dasac_stream_t stream) {
  DASAC_REQUIRE(w && u, "%s: null pointer", who);
  DASAC_REQUIRE(Cout > 0 && Cin > 0, "%s: bad channel counts", who);
  const int M = transposed ? Cin : Cout, K = transposed ? Cout : Cin;
  const int Mpad = dasac_conv_mpad(M), Kpad = dasac_conv_kpad(K);
  const int64_t per_point = (int64_t)Kpad * Mpad;
  DASAC_REQUIRE(F::P * per_point * 4 <= wino::kMaxBytes && (int64_t)Cout * Cin * 9 * 4 <= wino::kMaxBytes,
                "%s: operand exceeds the 4 GiB buffer-descriptor window", who);
  hipLaunchKernelGGL(wino::filter_transform<F>, dim3((unsigned)((per_point + wino::kBlock - 1) / wino::kBlock)), dim3(wino::kBlock), 0,
                     as_stream(stream), w, scale, u, Cout, Cin, Mpad, Kpad, transposed ? 1 : 0, (unsigned)((int64_t)Cout * Cin * 9 * 4),
                     (unsigned)(F::P * per_point * 4));
  DASAC_CHECK_LAUNCH(who);
  return DASAC_OK;
}

// the two per-tile transforms of an activation: x -> V (input_transform) and dz -> dM (grad_transform)
template <class F>
static int transform_impl(const char* who, void (*kernel)(const float*, float*, Geom, int, unsigned, unsigned), const float* x, int Nb,
                          int C, int H, int W, int dilation, float* v, size_t v_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(x && v, "%s: null pointer", who);
  Geom g;
  const int rc = wino_geom<F>(g, who, Nb, C, H, W, dilation);
  if (rc) return rc;
  const size_t need = (size_t)F::P * C * g.T * 4;
  if (v_bytes < need) return fail(DASAC_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, v_bytes, need);
  hipLaunchKernelGGL(kernel, dim3((g.T + wino::kBlock - 1) / wino::kBlock, C), dim3(wino::kBlock), 0, as_stream(stream), x, v, g, C,
                     (unsigned)((int64_t)Nb * C * H * W * 4), (unsigned)need);
  DASAC_CHECK_LAUNCH(who);
  return DASAC_OK;
}

template <class F>
static int output_impl(const char* who, const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                       int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out, dasac_stream_t stream) {
  DASAC_REQUIRE(y && out, "%s: null pointer", who);
  DASAC_REQUIRE(!(mask_bits && relu_bits_out), "%s: record the ReLU pattern OR mask with one", who);
  DASAC_REQUIRE(!relu_bits_out || relu, "%s: relu_bits_out records the pattern of a ReLU epilogue", who);
  Geom g;
  const int rc = wino_geom<F>(g, who, Nb, M, H, W, dilation);
  if (rc) return rc;
  const size_t need = (size_t)F::P * M * g.T * 4;
  if (y_bytes < need) return fail(DASAC_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, y_bytes, need);
  const int npix = Nb * H * W, w32 = (npix + 31) / 32;
  DASAC_REQUIRE((int64_t)M * w32 * 4 < (1ll << 31), "%s: bit mask exceeds 2 GiB", who);
  const unsigned bits_bytes = (unsigned)((int64_t)M * w32 * 4), out_bytes = (unsigned)((int64_t)Nb * M * H * W * 4);
  const dim3 per_pixel((npix + wino::kBlock - 1) / wino::kBlock, M), per_tile((g.T + wino::kBlock - 1) / wino::kBlock, M), block(wino::kBlock);
  hipStream_t s = as_stream(stream);
  if constexpr (F::TM == 2) {
    if (relu_bits_out)
      hipLaunchKernelGGL(wino::output_transform<1>, per_pixel, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                         (unsigned)need, out_bytes, bits_bytes);
    else if (mask_bits)
      hipLaunchKernelGGL(wino::output_transform<2>, per_pixel, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                         (unsigned)need, out_bytes, bits_bytes);
    else
      hipLaunchKernelGGL(wino::output_transform<0>, per_pixel, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                         (unsigned)need, out_bytes, bits_bytes);
  } else {
    if (mask_bits)
      hipLaunchKernelGGL(wino::output_transform4<true>, per_tile, block, 0, s, y, out, g, M, shift, relu, mask_bits, w32, (unsigned)need,
                         out_bytes, bits_bytes);
    else
      hipLaunchKernelGGL(wino::output_transform4<false>, per_tile, block, 0, s, y, out, g, M, shift, relu, mask_bits, w32, (unsigned)need,
                         out_bytes, bits_bytes);
    if (relu_bits_out) {
      DASAC_CHECK_LAUNCH(who);
      hipLaunchKernelGGL(wino::relu_bits_pack, per_pixel, block, 0, s, out, relu_bits_out, g, M, w32, out_bytes, bits_bytes);
    }
  }
  DASAC_CHECK_LAUNCH(who);
  return DASAC_OK;
}

template <class F>
static int wgrad_finish_impl(const char* who, const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w,
                             const float* scale, float* dw, float* dot, float* sum_dz, dasac_stream_t stream) {
  DASAC_REQUIRE(workspace && w && dw, "%s: null pointer", who);
  DASAC_REQUIRE(M > 0 && M <= 65535 && C > 0 && C % 64 == 0, "%s: needs 1..65535 output channels and a multiple of 64 input channels", who);
  const int splits = dasac_conv_wgrad_batched_splits(F::P, M, C, T);
  DASAC_REQUIRE(splits > 0, "%s: the batched weight-gradient launch does not take this shape", who);
  const size_t need = dasac_conv_wgrad_batched_workspace(F::P, M, C, T);
  if (ws_bytes < need) return fail(DASAC_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
  const int64_t s_elems = (int64_t)splits * F::P * M * C;
  DASAC_REQUIRE(s_elems * 4 <= wino::kMaxBytes && (int64_t)M * C * 9 * 4 <= wino::kMaxBytes,
                "%s: a tensor exceeds the 4 GiB buffer-descriptor window", who);
  const float* S = reinterpret_cast<const float*>(workspace);
  hipLaunchKernelGGL(wino::wgrad_finish<F>, dim3(C / 64, M), dim3(wino::kBlock), 0, as_stream(stream), S, S + s_elems, splits, M, C, w, scale,
                     dw, dot, sum_dz, (unsigned)(s_elems * 4), (unsigned)((int64_t)M * C * 9 * 4));
  DASAC_CHECK_LAUNCH(who);
  return DASAC_OK;
}

extern "C" int dasac_winograd_tiles(int Nb, int H, int W, int dilation) { return tiles_impl<F2>(Nb, H, W, dilation); }
extern "C" int dasac_winograd4_tiles(int Nb, int H, int W, int dilation) { return tiles_impl<F4>(Nb, H, W, dilation); }

extern "C" int dasac_winograd_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                                     dasac_stream_t stream) {
  return filter_impl<F2>("winograd_filter", w, scale, Cout, Cin, transposed, u, stream);
}
extern "C" int dasac_winograd4_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                                      dasac_stream_t stream) {
  return filter_impl<F4>("winograd4_filter", w, scale, Cout, Cin, transposed, u, stream);
}

extern "C" int dasac_winograd_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                                    dasac_stream_t stream) {
  return transform_impl<F2>("winograd_input", wino::input_transform<F2>, x, Nb, C, H, W, dilation, v, v_bytes, stream);
}
extern "C" int dasac_winograd4_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                                     dasac_stream_t stream) {
  return transform_impl<F4>("winograd4_input", wino::input_transform<F4>, x, Nb, C, H, W, dilation, v, v_bytes, stream);
}

extern "C" int dasac_winograd_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                                         dasac_stream_t stream) {
  return transform_impl<F2>("winograd_grad_input", wino::grad_transform<F2>, dz, Nb, M, H, W, dilation, dm, dm_bytes, stream);
}
extern "C" int dasac_winograd4_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                                          dasac_stream_t stream) {
  return transform_impl<F4>("winograd4_grad_input", wino::grad_transform<F4>, dz, Nb, M, H, W, dilation, dm, dm_bytes, stream);
}

extern "C" int dasac_winograd_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                                     int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out,
                                     dasac_stream_t stream) {
  return output_impl<F2>("winograd_output", y, y_bytes, Nb, M, H, W, dilation, shift, relu, mask_bits, relu_bits_out, out, stream);
}
extern "C" int dasac_winograd4_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                                      int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out,
                                      dasac_stream_t stream) {
  return output_impl<F4>("winograd4_output", y, y_bytes, Nb, M, H, W, dilation, shift, relu, mask_bits, relu_bits_out, out, stream);
}

extern "C" int dasac_winograd_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w,
                                           const float* scale, float* dw, float* dot, float* sum_dz, dasac_stream_t stream) {
  return wgrad_finish_impl<F2>("winograd_wgrad_finish", workspace, ws_bytes, M, C, T, w, scale, dw, dot, sum_dz, stream);
}
extern "C" int dasac_winograd4_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w,
                                            const float* scale, float* dw, float* dot, float* sum_dz, dasac_stream_t stream) {
  return wgrad_finish_impl<F4>("winograd4_wgrad_finish", workspace, ws_bytes, M, C, T, w, scale, dw, dot, sum_dz, stream);
}
