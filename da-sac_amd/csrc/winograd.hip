// Winograd F(2x2,3x3) for the wide dilated 3x3 convolutions (layer4 of the ResNet-101 backbone: 512 -> 512, dilation 4, 97x97
// maps; models/deeplabv2.py:65-66), UNFUSED: three streaming kernels around sixteen calls of the existing dasac_conv_gemm.
//
//   filter transform   U[pt] = G g G^T per (cout, cin), frozen-BN scale folded in, written as the packed operand of a 1x1 conv
//   input transform    V[pt][c][tile] = (B^T d B)[pt] of the 4x4 patch (stride = dilation) of every tile
//   16 point GEMMs     Y[pt][m][tile] = sum_c U[pt][m][c] * V[pt][c][tile]          (dasac_conv_gemm, 1x1, H = 1, W = tiles)
//   output transform   out[n][m][y][x] = epi((A^T Y A)[ey][ex]) -- shift, ReLU, ReLU bits recorded or consumed
//
// and the weight gradient as the exact adjoint, dW = G^T [sum over tiles (A dY A^T) (.) (B^T d B)] G:
//
//   grad transform     dM[pt][m][tile] = (A dY A^T)[pt] of every tile's 2x2 output pixels
//   16 contractions    P[split][pt][m][c] = sum over the split's tiles of dM[pt][m][t] * V[pt][c][t]   (dasac_conv_wgrad_batched, ONE launch)
//   finish             dW[m][c] = scale[m] * G^T (sum_split P) G, the frozen BN's dot rows and sum of dz
//
// 2.25 x fewer multiplies than the direct contraction; the price is two passes over [16][C][tiles] tensors.  No new matrix kernel.
// All three GEMMs also have an F(4x4,3x3) form (36 points per 4x4-output tile, 1.71 x fewer multiplies again; second half of the
// file): the weight gradient wherever it measured faster, the forward and the data gradient per measured route (ops.WINOGRAD4_ROUTES).
// Index arithmetic lives in winograd_index.hpp and is walked on the host by tools/winograd_index_check.cpp.  Every global access
// goes through a buffer descriptor of the tensor's exact extent with the whole offset in the per-lane operand (the scalar
// offset is not range checked by the hardware): an offset past the extent reads zero / stores nothing.
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

// ---- filter transform ------------------------------------------------------------------------------------------------------
// One thread per element (k, m) of the packed [Kpad/4][Mpad][4] matrix; it writes all 16 points (K and M padding as zeros).
// mode 0 (forward): m = cout, k = cin, g = w[m][k] * scale[m].   mode 1 (data gradient): m = cin, k = cout,
// g = rot180(w[k][m]) * scale[k].   U = G g G^T with G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]].
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
  float g[3][3];
  const bool real = m < M && k < K;
  const int co = mode == 0 ? m : k, ci = mode == 0 ? k : m;
  const float s = (real && scale) ? ld(make_rsrc(scale, (unsigned)Cout * 4u), (unsigned)co * 4u) : 1.f;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tap = mode == 0 ? a * 3 + b : (2 - a) * 3 + (2 - b);
      const unsigned off = real ? (unsigned)((co * Cin + ci) * 9 + tap) * 4u : kOutside;
      g[a][b] = ld(rw, off) * s;
    }
  float t[4][3];                                           // G g
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = 0.5f * ((g[0][b] + g[2][b]) + g[1][b]);
    t[2][b] = 0.5f * ((g[0][b] + g[2][b]) - g[1][b]);
    t[3][b] = g[2][b];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float u[4] = {t[a][0], 0.5f * ((t[a][0] + t[a][2]) + t[a][1]), 0.5f * ((t[a][0] + t[a][2]) - t[a][1]), t[a][2]};
#pragma unroll
    for (int b = 0; b < 4; ++b) st(ru, (unsigned)((a * 4 + b) * per_point + idx) * 4u, u[b]);
  }
}

// ---- input transform -------------------------------------------------------------------------------------------------------
// grid (ceil(T / 256), C): one thread per (channel, tile), lanes along tiles.  V = B^T d B, B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]].
__global__ __launch_bounds__(kBlock) void input_transform(const float* __restrict__ X, float* __restrict__ V, Geom g, int C,
                                                           unsigned x_bytes, unsigned v_bytes) {
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (tile >= g.T) return;
  const int c = blockIdx.y;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(X, x_bytes), rv = make_rsrc(V, v_bytes);
  int n, y0, x0;
  tile_origin(g, tile, n, y0, x0);
  float d[4][4];
#pragma unroll
  for (int ky = 0; ky < 4; ++ky)
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) d[ky][kx] = ld(rx, patch_offset(g, C, n, c, y0, x0, ky, kx));
  float t[4][4];                                           // B^T d
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) {
    t[0][kx] = d[0][kx] - d[2][kx];
    t[1][kx] = d[1][kx] + d[2][kx];
    t[2][kx] = d[2][kx] - d[1][kx];
    t[3][kx] = d[1][kx] - d[3][kx];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float v[4] = {t[a][0] - t[a][2], t[a][1] + t[a][2], t[a][2] - t[a][1], t[a][1] - t[a][3]};
#pragma unroll
    for (int b = 0; b < 4; ++b) st(rv, point_offset(g, C, a * 4 + b, c, tile), v[b]);
  }
}

// ---- output transform ------------------------------------------------------------------------------------------------------
// grid (ceil(N*H*W / 256), M): one thread per OUTPUT element, lanes along the flattened (n, y, x) pixel index -- the pixel axis of
// the ReLU bit masks (conv_gemm.hip Epilogue: bits[m][pix >> 5] bit pix & 31), so a wave ballot is two mask words, as in the
// direct epilogue.  Output (ey, ex) of a tile is sum_j sum_k sy_j sx_k Y[ey + j][ex + k], signs (+,+,+) for e = 0 and (+,-,-)
// for e = 1 (A^T = [[1,1,1,0],[0,1,-1,-1]]): nine loads; the four outputs of a tile re-read its values from cache.
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
    const unsigned word = __builtin_amdgcn_raw_buffer_load_b32(rb, live ? (unsigned)(m * w32 + (pix >> 5)) * 4u : kOutside, 0, 0);
    o = (word >> (pix & 31)) & 1u ? o : 0.f;
  }
  st(ro, live ? out_offset(g, M, n, m, rem) : kOutside, o);
  if constexpr (BITS == 1) {
    const unsigned long long ballot = __builtin_amdgcn_ballot_w64(live && o > 0.f);
    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(obits, bits_bytes);
    // lanes 0 and 32 store the wave's two words; a word whose 32 pixels all lie past the last pixel does not exist
    const int wcol = pix >> 5;
    if ((lane & 31) == 0 && wcol < w32)
      __builtin_amdgcn_raw_buffer_store_b32((unsigned)(lane ? ballot >> 32 : ballot), rb, (unsigned)(m * w32 + wcol) * 4u, 0, 0);
  }
}

// ---- weight gradient: transform of dY ----------------------------------------------------------------------------------------
// The adjoint of the output transform.  grid (ceil(T / 256), M): one thread per (channel, tile), lanes along tiles, tiles numbered as
// input_transform numbers them.  dM = A dY A^T of the tile's 2x2 output pixels, A = [[1,0],[1,1],[1,-1],[0,-1]]; output (ey, ex)
// is tap (ey + 1, ex + 1) of the tile's patch, so a pixel of a tile that hangs over the map edge takes patch_offset's zero.
__global__ __launch_bounds__(kBlock) void grad_transform(const float* __restrict__ dY, float* __restrict__ dM, Geom g, int M,
                                                          unsigned y_bytes, unsigned m_bytes) {
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (tile >= g.T) return;
  const int m = blockIdx.y;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(dY, y_bytes), rm = make_rsrc(dM, m_bytes);
  int n, y0, x0;
  tile_origin(g, tile, n, y0, x0);
  float d[2][2];
#pragma unroll
  for (int ey = 0; ey < 2; ++ey)
#pragma unroll
    for (int ex = 0; ex < 2; ++ex) d[ey][ex] = ld(ry, patch_offset(g, M, n, m, y0, x0, ey + 1, ex + 1));
  float t[4][2];                                           // A dY
#pragma unroll
  for (int ex = 0; ex < 2; ++ex) {
    t[0][ex] = d[0][ex];
    t[1][ex] = d[0][ex] + d[1][ex];
    t[2][ex] = d[0][ex] - d[1][ex];
    t[3][ex] = -d[1][ex];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float v[4] = {t[a][0], t[a][0] + t[a][1], t[a][0] - t[a][1], -t[a][1]};
#pragma unroll
    for (int b = 0; b < 4; ++b) st(rm, point_offset(g, M, a * 4 + b, m, tile), v[b]);
  }
}

// ---- weight gradient: finish -------------------------------------------------------------------------------------------------
// P [splits][16][M][C] (the batched point contraction's slabs), Psum [splits][M] (channel sums of point (1,1) of dM = sum of dz)
// -> dW[co][ci][3][3] = scale[co] * (G^T (sum_s P[s]) G), dot[blockIdx.x][co] = this block's part of sum W * (unscaled gradient),
// sum_dz[co] = sum_s Psum[s][co]: dot and sum_dz exactly as dasac_conv_wgrad_finish leaves them.  grid (C / 64, M), 256 threads =
// 64 input channels x 4 split lanes; a thread adds the splits s = lane, lane + 4, ... of its channel's 16 points, the four lanes
// meet in LDS in a fixed order, and the block writes its 64 x 9 gradients as one contiguous run of dW.
__global__ __launch_bounds__(kBlock) void wgrad_finish(const float* __restrict__ P, const float* __restrict__ Psum, int splits, int M,
                                                        int C, const float* __restrict__ Wt, const float* __restrict__ scale,
                                                        float* __restrict__ dW, float* __restrict__ dot, float* __restrict__ sum_dz,
                                                        unsigned p_bytes, unsigned w_bytes) {
  const int co = blockIdx.y, ci0 = blockIdx.x * 64;
  const int tx = threadIdx.x, c = tx & 63, q = tx >> 6;
  const __amdgpu_buffer_rsrc_t rp = make_rsrc(P, p_bytes), rw = make_rsrc(Wt, w_bytes), rd = make_rsrc(dW, w_bytes);
  if (sum_dz && blockIdx.x == 0 && q == 0) {                 // one wave: the splits' channel sums in parallel
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(Psum, (unsigned)(splits * M) * 4u);
    float sv = 0.f;
    for (int s = c; s < splits; s += 64) sv += ld(rs, (unsigned)(s * M + co) * 4u);
    sv = wave_sum(sv);
    if (c == 0) st(make_rsrc(sum_dz, (unsigned)M * 4u), (unsigned)co * 4u, sv);
  }
  __shared__ float red[4][16][64];
  __shared__ float grad[64 * 9];
  float acc[16];
#pragma unroll
  for (int pt = 0; pt < 16; ++pt) acc[pt] = 0.f;
  const unsigned point = (unsigned)(M * C), slab = 16u * point;
  const unsigned e0 = (unsigned)(co * C + ci0 + c);
  for (int s = q; s < splits; s += 4)
#pragma unroll
    for (int pt = 0; pt < 16; ++pt) acc[pt] += ld(rp, ((unsigned)s * slab + (unsigned)pt * point + e0) * 4u);
#pragma unroll
  for (int pt = 0; pt < 16; ++pt) red[q][pt][c] = acc[pt];
  __syncthreads();
  if (q == 0) {
    float p[4][4];
#pragma unroll
    for (int pt = 0; pt < 16; ++pt) p[pt >> 2][pt & 3] = (red[0][pt][c] + red[1][pt][c]) + (red[2][pt][c] + red[3][pt][c]);
    float r[3][4];                                         // G^T P
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      r[0][b] = p[0][b] + 0.5f * (p[1][b] + p[2][b]);
      r[1][b] = 0.5f * (p[1][b] - p[2][b]);
      r[2][b] = 0.5f * (p[1][b] + p[2][b]) + p[3][b];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      grad[c * 9 + a * 3 + 0] = r[a][0] + 0.5f * (r[a][1] + r[a][2]);
      grad[c * 9 + a * 3 + 1] = 0.5f * (r[a][1] - r[a][2]);
      grad[c * 9 + a * 3 + 2] = 0.5f * (r[a][1] + r[a][2]) + r[a][3];
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

// ---- weight gradient as F(4x4,3x3) -------------------------------------------------------------------------------------------
// The same adjoint with four outputs per tile and axis: 36 point products per 4x4 output tile where F(2x2) spends 4 x 16, and
// transformed tensors [36][C][T] of 0.59 times the size.  Evaluation points 0, 1, -1, 2, -1/2, inf, chosen for the weight gradient's
// error against float64 (profiles/EXPERIMENTS.md); the three matrices, B^T scaled to integers and G carrying the inverse factors:
//   B^T = [[2,3,-4,-3,2,0],[0,2,5,1,-2,0],[0,2,1,-5,2,0],[0,-1,-2,1,2,0],[0,-2,1,2,-1,0],[0,2,3,-4,-3,2]]
//   A   = [[1,0,0,0],[1,1,1,1],[1,-1,1,-1],[1,2,4,8],[1,-1/2,1/4,-1/8],[0,0,0,1]]
//   G   = [[1/2,0,0],[1/6,1/6,1/6],[1/6,-1/6,1/6],[1/30,1/15,2/15],[16/15,-8/15,4/15],[0,0,1/2]]
// (tests/winograd4_ref.py holds them as fractions and checks the identities in float64).  The kernels are the twins of the F(2x2)
// ones above -- one thread per (channel, tile), lanes along tiles, exact-extent descriptors -- and additionally write the padding
// tiles (Geom::T is rounded up to a multiple of 4) as zeros at all 36 points.  The forward and the data gradient have the same form
// (filter_transform4 / input_transform4 / 36 point GEMMs / output_transform4, further down): at 2 - 4 x the direct kernel's error
// against float64, they run where ops.winograd4_routed's table says the end-to-end bounds were measured to hold
// (profiles/EXPERIMENTS.md).
__device__ __forceinline__ void bt6(float d0, float d1, float d2, float d3, float d4, float d5, float (&o)[6]) {
  o[0] = (2.f * (d0 + d4) + 3.f * (d1 - d3)) - 4.f * d2;
  o[1] = (2.f * (d1 - d4) + 5.f * d2) + d3;
  o[2] = (2.f * (d1 + d4) + d2) - 5.f * d3;
  o[3] = (d3 - d1) + 2.f * (d4 - d2);
  o[4] = 2.f * (d3 - d1) + (d2 - d4);
  o[5] = (2.f * (d1 + d5) + 3.f * (d2 - d4)) - 4.f * d3;
}
__device__ __forceinline__ void a6(float y0, float y1, float y2, float y3, float (&o)[6]) {
  o[0] = y0;
  o[1] = (y0 + y2) + (y1 + y3);
  o[2] = (y0 + y2) - (y1 + y3);
  o[3] = (y0 + 4.f * y2) + (2.f * y1 + 8.f * y3);
  o[4] = (y0 + 0.25f * y2) - (0.5f * y1 + 0.125f * y3);
  o[5] = y3;
}
__device__ __forceinline__ void gt3(float p0, float p1, float p2, float p3, float p4, float p5, float (&o)[3]) {
  constexpr float k6 = 1.f / 6.f, k15 = 1.f / 15.f, k30 = 1.f / 30.f;
  o[0] = (0.5f * p0 + k6 * (p1 + p2)) + (k30 * p3 + (16.f * k15) * p4);
  o[1] = k6 * (p1 - p2) + (k15 * p3 - (8.f * k15) * p4);
  o[2] = (k6 * (p1 + p2) + 0.5f * p5) + ((2.f * k15) * p3 + (4.f * k15) * p4);
}

// grid (ceil(T / 256), C).  V = B^T d B of the 6x6 patch (taps `dilation` apart), 36 stores.
__global__ __launch_bounds__(kBlock) void input_transform4(const float* __restrict__ X, float* __restrict__ V, Geom g, int C,
                                                            unsigned x_bytes, unsigned v_bytes) {
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (tile >= g.T) return;
  const int c = blockIdx.y;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(X, x_bytes), rv = make_rsrc(V, v_bytes);
  if (!real_tile(g, tile)) {
#pragma unroll
    for (int pt = 0; pt < 36; ++pt) st(rv, point_offset(g, C, pt, c, tile), 0.f);
    return;
  }
  int n, y0, x0;
  tile_origin<4>(g, tile, n, y0, x0);
  float t[6][6];                                           // B^T d, a column of the patch at a time
#pragma unroll
  for (int kx = 0; kx < 6; ++kx) {
    float d[6], o[6];
#pragma unroll
    for (int ky = 0; ky < 6; ++ky) d[ky] = ld(rx, patch_offset(g, C, n, c, y0, x0, ky, kx));
    bt6(d[0], d[1], d[2], d[3], d[4], d[5], o);
#pragma unroll
    for (int a = 0; a < 6; ++a) t[a][kx] = o[a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float v[6];
    bt6(t[a][0], t[a][1], t[a][2], t[a][3], t[a][4], t[a][5], v);
#pragma unroll
    for (int b = 0; b < 6; ++b) st(rv, point_offset(g, C, a * 6 + b, c, tile), v[b]);
  }
}

// grid (ceil(T / 256), M).  dM = A dY A^T of the tile's 4x4 output pixels; output (ey, ex) is tap (ey + 1, ex + 1) of the tile's
// patch, so the overhang of a tile past the map edge takes patch_offset's zero.
__global__ __launch_bounds__(kBlock) void grad_transform4(const float* __restrict__ dY, float* __restrict__ dM, Geom g, int M,
                                                           unsigned y_bytes, unsigned m_bytes) {
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (tile >= g.T) return;
  const int m = blockIdx.y;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(dY, y_bytes), rm = make_rsrc(dM, m_bytes);
  if (!real_tile(g, tile)) {
#pragma unroll
    for (int pt = 0; pt < 36; ++pt) st(rm, point_offset(g, M, pt, m, tile), 0.f);
    return;
  }
  int n, y0, x0;
  tile_origin<4>(g, tile, n, y0, x0);
  float t[6][4];                                           // A dY
#pragma unroll
  for (int ex = 0; ex < 4; ++ex) {
    float d[4], o[6];
#pragma unroll
    for (int ey = 0; ey < 4; ++ey) d[ey] = ld(ry, patch_offset(g, M, n, m, y0, x0, ey + 1, ex + 1));
    a6(d[0], d[1], d[2], d[3], o);
#pragma unroll
    for (int a = 0; a < 6; ++a) t[a][ex] = o[a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float v[6];
    a6(t[a][0], t[a][1], t[a][2], t[a][3], v);
#pragma unroll
    for (int b = 0; b < 6; ++b) st(rm, point_offset(g, M, a * 6 + b, m, tile), v[b]);
  }
}

// P [splits][36][M][C], Psum [splits][M] (channel sums of point (1,1) of dM, whose row of A is all ones = sum of dz) -> dW, dot and
// sum_dz as wgrad_finish leaves them.  Same grid, thread roles and summation order; 36 points, G^T (.) G from 6x6 to 3x3.
__global__ __launch_bounds__(kBlock) void wgrad_finish4(const float* __restrict__ P, const float* __restrict__ Psum, int splits, int M,
                                                         int C, const float* __restrict__ Wt, const float* __restrict__ scale,
                                                         float* __restrict__ dW, float* __restrict__ dot, float* __restrict__ sum_dz,
                                                         unsigned p_bytes, unsigned w_bytes) {
  const int co = blockIdx.y, ci0 = blockIdx.x * 64;
  const int tx = threadIdx.x, c = tx & 63, q = tx >> 6;
  const __amdgpu_buffer_rsrc_t rp = make_rsrc(P, p_bytes), rw = make_rsrc(Wt, w_bytes), rd = make_rsrc(dW, w_bytes);
  if (sum_dz && blockIdx.x == 0 && q == 0) {                 // one wave: the splits' channel sums in parallel
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(Psum, (unsigned)(splits * M) * 4u);
    float sv = 0.f;
    for (int s = c; s < splits; s += 64) sv += ld(rs, (unsigned)(s * M + co) * 4u);
    sv = wave_sum(sv);
    if (c == 0) st(make_rsrc(sum_dz, (unsigned)M * 4u), (unsigned)co * 4u, sv);
  }
  __shared__ float red[4][36][64];
  __shared__ float grad[64 * 9];
  float acc[36];
#pragma unroll
  for (int pt = 0; pt < 36; ++pt) acc[pt] = 0.f;
  const unsigned point = (unsigned)(M * C), slab = 36u * point;
  const unsigned e0 = (unsigned)(co * C + ci0 + c);
  for (int s = q; s < splits; s += 4)
#pragma unroll
    for (int pt = 0; pt < 36; ++pt) acc[pt] += ld(rp, ((unsigned)s * slab + (unsigned)pt * point + e0) * 4u);
#pragma unroll
  for (int pt = 0; pt < 36; ++pt) red[q][pt][c] = acc[pt];
  __syncthreads();
  if (q == 0) {
    float r[3][6];                                         // G^T P, a column of the points at a time
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      float p[6], o[3];
#pragma unroll
      for (int a = 0; a < 6; ++a) p[a] = (red[0][a * 6 + b][c] + red[1][a * 6 + b][c]) + (red[2][a * 6 + b][c] + red[3][a * 6 + b][c]);
      gt3(p[0], p[1], p[2], p[3], p[4], p[5], o);
#pragma unroll
      for (int a = 0; a < 3; ++a) r[a][b] = o[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float o[3];
      gt3(r[a][0], r[a][1], r[a][2], r[a][3], r[a][4], r[a][5], o);
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

// ---- forward and data gradient as F(4x4,3x3) --------------------------------------------------------------------------------
// G g along one axis: three taps -> six points
__device__ __forceinline__ void g6(float g0, float g1, float g2, float (&o)[6]) {
  constexpr float k6 = 1.f / 6.f, k15 = 1.f / 15.f, k30 = 1.f / 30.f;
  o[0] = 0.5f * g0;
  o[1] = k6 * ((g0 + g2) + g1);
  o[2] = k6 * ((g0 + g2) - g1);
  o[3] = (k30 * g0 + k15 * g1) + (2.f * k15) * g2;
  o[4] = ((16.f * k15) * g0 - (8.f * k15) * g1) + (4.f * k15) * g2;
  o[5] = 0.5f * g2;
}
// A^T y along one axis: six points -> four outputs
__device__ __forceinline__ void at4(float y0, float y1, float y2, float y3, float y4, float y5, float (&o)[4]) {
  o[0] = (y0 + (y1 + y2)) + (y3 + y4);
  o[1] = (y1 - y2) + (2.f * y3 - 0.5f * y4);
  o[2] = (y1 + y2) + (4.f * y3 + 0.25f * y4);
  o[3] = ((y1 - y2) + y5) + (8.f * y3 - 0.125f * y4);
}

// The twin of filter_transform: one thread per element (k, m) of the packed [Kpad/4][Mpad][4] matrix, 36 points, U = G g G^T.
__global__ __launch_bounds__(kBlock) void filter_transform4(const float* __restrict__ Wt, const float* __restrict__ scale,
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
  float t[6][3];                                           // G g, a column of the filter at a time
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    float g[3], o[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int tap = mode == 0 ? a * 3 + b : (2 - a) * 3 + (2 - b);
      g[a] = ld(rw, real ? (unsigned)((co * Cin + ci) * 9 + tap) * 4u : kOutside) * s;
    }
    g6(g[0], g[1], g[2], o);
#pragma unroll
    for (int a = 0; a < 6; ++a) t[a][b] = o[a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float u[6];
    g6(t[a][0], t[a][1], t[a][2], u);
#pragma unroll
    for (int b = 0; b < 6; ++b) st(ru, (unsigned)((a * 6 + b) * per_point + idx) * 4u, u[b]);
  }
}

// out = epi(A^T Y A) over Y [36][M][T].  grid (ceil(T / 256), M): one thread per (channel, tile), lanes along tiles, the mapping of
// input_transform4 and grad_transform4 -- 36 loads for 16 outputs (2.25 per output; one thread per output element would load up to
// 36 for one), each load a run of 64 consecutive tiles of one point.  Consecutive tile numbers are consecutive phases, so a store
// instruction writes runs of `d` adjacent floats and the four stores of an output row fill each other's gaps: the mirror of what
// grad_transform4 reads.  Padding tiles and overhanging outputs store nothing.
// MASK: the elements whose bit in `mbits` is clear become zero.  The price of the mapping is that a wave no longer holds 64
// consecutive pixels, so the RECORDED ReLU bits cannot be a ballot here: relu_bits_pack below reads the stored output back.  (Adding
// the bits into zeroed words with buffer atomics, one per run of outputs that share a word, was built and measured: 0.40 ms for the
// layer4 launch against 0.12 ms without bits -- the atomics are per lane at the L2; the second pass costs 0.07 ms.)
template <bool MASK>
__global__ __launch_bounds__(kBlock) void output_transform4(const float* __restrict__ Y, float* __restrict__ Out, Geom g, int M,
                                                             const float* __restrict__ shift, int relu,
                                                             const unsigned* __restrict__ mbits, int w32, unsigned y_bytes,
                                                             unsigned out_bytes, unsigned bits_bytes) {
  const int tile = blockIdx.x * kBlock + threadIdx.x;
  if (!real_tile(g, tile)) return;
  const int m = blockIdx.y;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(Y, y_bytes), ro = make_rsrc(Out, out_bytes);
  int n, y0, x0;
  tile_origin<4>(g, tile, n, y0, x0);
  float t[4][6];                                           // A^T Y, a column of the points at a time
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    float v[6], o[4];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = ld(ry, point_offset(g, M, a * 6 + b, m, tile));
    at4(v[0], v[1], v[2], v[3], v[4], v[5], o);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e][b] = o[e];
  }
  const float sh = shift ? ld(make_rsrc(shift, (unsigned)M * 4u), (unsigned)m * 4u) : 0.f;
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(mbits, MASK ? bits_bytes : 0u);
#pragma unroll
  for (int ey = 0; ey < 4; ++ey) {
    float o[4];
    at4(t[ey][0], t[ey][1], t[ey][2], t[ey][3], t[ey][4], t[ey][5], o);
    const int y = y0 + ey * g.ay.d;
#pragma unroll
    for (int ex = 0; ex < 4; ++ex) {
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

// bits[m][pix >> 5] bit (pix & 31) = out[n][m][rem] > 0 over the flattened pixel index pix = n*HW + rem: the ReLU pattern of a stored
// activation in the layout of the direct epilogue.  grid (ceil(N*H*W / 256), M): one thread per element, lanes along pixels, a wave
// ballot is two words (the tail of output_transform<1>); every word is written, the bits past the last pixel as zeros.
__global__ __launch_bounds__(kBlock) void relu_bits_pack(const float* __restrict__ Out, unsigned* __restrict__ obits, Geom g, int M,
                                                          int w32, unsigned out_bytes, unsigned bits_bytes) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  const int m = blockIdx.y;
  const bool live = pix < g.N * g.HW;
  const int n = live ? div(pix, g.by_hw) : 0;
  const float v = ld(make_rsrc(Out, out_bytes), live ? out_offset(g, M, n, m, pix - n * g.HW) : kOutside);
  const unsigned long long ballot = __builtin_amdgcn_ballot_w64(live && v > 0.f);
  const int lane = threadIdx.x & 63, wcol = pix >> 5;
  if ((lane & 31) == 0 && wcol < w32)
    __builtin_amdgcn_raw_buffer_store_b32((unsigned)(lane ? ballot >> 32 : ballot), make_rsrc(obits, bits_bytes), out_bits_offset(m, w32, pix), 0, 0);
}

}  // namespace wino
}  // namespace dasac

using namespace dasac;
using dasac::wino::Geom;

static int wino_geom(Geom& g, const char* who, int Nb, int C, int M, int H, int W, int dilation) {
  DASAC_REQUIRE(Nb > 0 && C > 0 && M > 0 && H > 0 && W > 0 && dilation > 0, "%s: bad geometry", who);
  DASAC_REQUIRE((int64_t)Nb * H * W < (1ll << 30), "%s: more than 2^30 pixels", who);
  g = wino::make_geom(Nb, H, W, dilation);
  const int64_t cmax = C > M ? C : M;
  DASAC_REQUIRE(16 * cmax * (int64_t)g.T * 4 <= wino::kMaxBytes && cmax * (int64_t)Nb * H * W * 4 <= wino::kMaxBytes,
                "%s: a tensor exceeds the 4 GiB buffer-descriptor window", who);
  return DASAC_OK;
}

extern "C" int dasac_winograd_tiles(int Nb, int H, int W, int dilation) {
  if (Nb <= 0 || H <= 0 || W <= 0 || dilation <= 0) return 0;
  const int64_t t = (int64_t)Nb * wino::make_axis(H, dilation).tiles * wino::make_axis(W, dilation).tiles;
  return t < (1ll << 30) ? (int)t : 0;
}

extern "C" int dasac_winograd_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                                     dasac_stream_t stream) {
  DASAC_REQUIRE(w && u, "winograd_filter: null pointer");
  DASAC_REQUIRE(Cout > 0 && Cin > 0, "winograd_filter: bad channel counts");
  const int M = transposed ? Cin : Cout, K = transposed ? Cout : Cin;
  const int Mpad = dasac_conv_mpad(M), Kpad = dasac_conv_kpad(K);
  const int64_t per_point = (int64_t)Kpad * Mpad;
  DASAC_REQUIRE(16 * per_point * 4 <= wino::kMaxBytes && (int64_t)Cout * Cin * 9 * 4 <= wino::kMaxBytes,
                "winograd_filter: operand exceeds the 4 GiB buffer-descriptor window");
  hipLaunchKernelGGL(wino::filter_transform, dim3((unsigned)((per_point + wino::kBlock - 1) / wino::kBlock)), dim3(wino::kBlock), 0,
                     as_stream(stream), w, scale, u, Cout, Cin, Mpad, Kpad, transposed ? 1 : 0, (unsigned)((int64_t)Cout * Cin * 9 * 4),
                     (unsigned)(16 * per_point * 4));
  DASAC_CHECK_LAUNCH("winograd filter_transform");
  return DASAC_OK;
}

extern "C" int dasac_winograd_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                                    dasac_stream_t stream) {
  DASAC_REQUIRE(x && v, "winograd_input: null pointer");
  Geom g;
  const int rc = wino_geom(g, "winograd_input", Nb, C, C, H, W, dilation);
  if (rc) return rc;
  DASAC_REQUIRE(C <= 65535, "winograd_input: more than 65535 channels");
  const size_t need = (size_t)16 * C * g.T * 4;
  if (v_bytes < need) return fail(DASAC_EWORKSPACE, "winograd_input: workspace too small (%zu < %zu)", v_bytes, need);
  hipLaunchKernelGGL(wino::input_transform, dim3((g.T + wino::kBlock - 1) / wino::kBlock, C), dim3(wino::kBlock), 0, as_stream(stream), x,
                     v, g, C, (unsigned)((int64_t)Nb * C * H * W * 4), (unsigned)need);
  DASAC_CHECK_LAUNCH("winograd input_transform");
  return DASAC_OK;
}

extern "C" int dasac_winograd_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                                     int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out,
                                     dasac_stream_t stream) {
  DASAC_REQUIRE(y && out, "winograd_output: null pointer");
  DASAC_REQUIRE(!(mask_bits && relu_bits_out), "winograd_output: record the ReLU pattern OR mask with one");
  DASAC_REQUIRE(!relu_bits_out || relu, "winograd_output: relu_bits_out records the pattern of a ReLU epilogue");
  Geom g;
  const int rc = wino_geom(g, "winograd_output", Nb, M, M, H, W, dilation);
  if (rc) return rc;
  DASAC_REQUIRE(M <= 65535, "winograd_output: more than 65535 channels");
  const size_t need = (size_t)16 * M * g.T * 4;
  if (y_bytes < need) return fail(DASAC_EWORKSPACE, "winograd_output: workspace too small (%zu < %zu)", y_bytes, need);
  const int npix = Nb * H * W, w32 = (npix + 31) / 32;
  DASAC_REQUIRE((int64_t)M * w32 * 4 < (1ll << 31), "winograd_output: bit mask exceeds 2 GiB");
  const unsigned bits_bytes = (unsigned)((int64_t)M * w32 * 4), out_bytes = (unsigned)((int64_t)Nb * M * H * W * 4);
  const dim3 grid((npix + wino::kBlock - 1) / wino::kBlock, M), block(wino::kBlock);
  hipStream_t s = as_stream(stream);
  if (relu_bits_out)
    hipLaunchKernelGGL(wino::output_transform<1>, grid, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                       (unsigned)need, out_bytes, bits_bytes);
  else if (mask_bits)
    hipLaunchKernelGGL(wino::output_transform<2>, grid, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                       (unsigned)need, out_bytes, bits_bytes);
  else
    hipLaunchKernelGGL(wino::output_transform<0>, grid, block, 0, s, y, out, g, M, shift, relu, mask_bits, relu_bits_out, w32,
                       (unsigned)need, out_bytes, bits_bytes);
  DASAC_CHECK_LAUNCH("winograd output_transform");
  return DASAC_OK;
}

extern "C" int dasac_winograd_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                                         dasac_stream_t stream) {
  DASAC_REQUIRE(dz && dm, "winograd_grad_input: null pointer");
  Geom g;
  const int rc = wino_geom(g, "winograd_grad_input", Nb, M, M, H, W, dilation);
  if (rc) return rc;
  DASAC_REQUIRE(M <= 65535, "winograd_grad_input: more than 65535 channels");
  const size_t need = (size_t)16 * M * g.T * 4;
  if (dm_bytes < need) return fail(DASAC_EWORKSPACE, "winograd_grad_input: workspace too small (%zu < %zu)", dm_bytes, need);
  hipLaunchKernelGGL(wino::grad_transform, dim3((g.T + wino::kBlock - 1) / wino::kBlock, M), dim3(wino::kBlock), 0, as_stream(stream), dz,
                     dm, g, M, (unsigned)((int64_t)Nb * M * H * W * 4), (unsigned)need);
  DASAC_CHECK_LAUNCH("winograd grad_transform");
  return DASAC_OK;
}

extern "C" int dasac_winograd_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w,
                                           const float* scale, float* dw, float* dot, float* sum_dz, dasac_stream_t stream) {
  DASAC_REQUIRE(workspace && w && dw, "winograd_wgrad_finish: null pointer");
  DASAC_REQUIRE(M > 0 && M <= 65535 && C > 0 && C % 64 == 0, "winograd_wgrad_finish: needs 1..65535 output channels and a multiple of 64 input channels");
  const int splits = dasac_conv_wgrad_batched_splits(16, M, C, T);
  DASAC_REQUIRE(splits > 0, "winograd_wgrad_finish: the batched weight-gradient launch does not take this shape");
  const size_t need = dasac_conv_wgrad_batched_workspace(16, M, C, T);
  if (ws_bytes < need) return fail(DASAC_EWORKSPACE, "winograd_wgrad_finish: workspace too small (%zu < %zu)", ws_bytes, need);
  const int64_t p_elems = (int64_t)splits * 16 * M * C;
  DASAC_REQUIRE(p_elems * 4 <= wino::kMaxBytes && (int64_t)M * C * 9 * 4 <= wino::kMaxBytes,
                "winograd_wgrad_finish: a tensor exceeds the 4 GiB buffer-descriptor window");
  const float* P = reinterpret_cast<const float*>(workspace);
  hipLaunchKernelGGL(wino::wgrad_finish, dim3(C / 64, M), dim3(wino::kBlock), 0, as_stream(stream), P, P + p_elems, splits, M, C, w, scale,
                     dw, dot, sum_dz, (unsigned)(p_elems * 4), (unsigned)((int64_t)M * C * 9 * 4));
  DASAC_CHECK_LAUNCH("winograd wgrad_finish");
  return DASAC_OK;
}

// ---- F(4x4,3x3) weight gradient: entry points -------------------------------------------------------------------------------
static int wino_geom4(Geom& g, const char* who, int Nb, int C, int H, int W, int dilation) {
  DASAC_REQUIRE(Nb > 0 && C > 0 && C <= 65535 && H > 0 && W > 0 && dilation > 0, "%s: bad geometry", who);
  DASAC_REQUIRE((int64_t)Nb * H * W < (1ll << 30), "%s: more than 2^30 pixels", who);
  g = wino::make_geom<4>(Nb, H, W, dilation);
  DASAC_REQUIRE(36 * (int64_t)C * g.T * 4 <= wino::kMaxBytes && (int64_t)C * Nb * H * W * 4 <= wino::kMaxBytes,
                "%s: a tensor exceeds the 4 GiB buffer-descriptor window", who);
  return DASAC_OK;
}

extern "C" int dasac_winograd4_tiles(int Nb, int H, int W, int dilation) {
  if (Nb <= 0 || H <= 0 || W <= 0 || dilation <= 0) return 0;
  const int64_t t = (int64_t)Nb * wino::make_axis<4>(H, dilation).tiles * wino::make_axis<4>(W, dilation).tiles;
  return t < (1ll << 30) ? (int)((t + 3) / 4 * 4) : 0;
}

extern "C" int dasac_winograd4_input(const float* x, int Nb, int C, int H, int W, int dilation, float* v, size_t v_bytes,
                                     dasac_stream_t stream) {
  DASAC_REQUIRE(x && v, "winograd4_input: null pointer");
  Geom g;
  const int rc = wino_geom4(g, "winograd4_input", Nb, C, H, W, dilation);
  if (rc) return rc;
  const size_t need = (size_t)36 * C * g.T * 4;
  if (v_bytes < need) return fail(DASAC_EWORKSPACE, "winograd4_input: workspace too small (%zu < %zu)", v_bytes, need);
  hipLaunchKernelGGL(wino::input_transform4, dim3((g.T + wino::kBlock - 1) / wino::kBlock, C), dim3(wino::kBlock), 0, as_stream(stream), x,
                     v, g, C, (unsigned)((int64_t)Nb * C * H * W * 4), (unsigned)need);
  DASAC_CHECK_LAUNCH("winograd input_transform4");
  return DASAC_OK;
}

extern "C" int dasac_winograd4_grad_input(const float* dz, int Nb, int M, int H, int W, int dilation, float* dm, size_t dm_bytes,
                                          dasac_stream_t stream) {
  DASAC_REQUIRE(dz && dm, "winograd4_grad_input: null pointer");
  Geom g;
  const int rc = wino_geom4(g, "winograd4_grad_input", Nb, M, H, W, dilation);
  if (rc) return rc;
  const size_t need = (size_t)36 * M * g.T * 4;
  if (dm_bytes < need) return fail(DASAC_EWORKSPACE, "winograd4_grad_input: workspace too small (%zu < %zu)", dm_bytes, need);
  hipLaunchKernelGGL(wino::grad_transform4, dim3((g.T + wino::kBlock - 1) / wino::kBlock, M), dim3(wino::kBlock), 0, as_stream(stream), dz,
                     dm, g, M, (unsigned)((int64_t)Nb * M * H * W * 4), (unsigned)need);
  DASAC_CHECK_LAUNCH("winograd grad_transform4");
  return DASAC_OK;
}

extern "C" int dasac_winograd4_wgrad_finish(const void* workspace, size_t ws_bytes, int M, int C, int T, const float* w,
                                            const float* scale, float* dw, float* dot, float* sum_dz, dasac_stream_t stream) {
  DASAC_REQUIRE(workspace && w && dw, "winograd4_wgrad_finish: null pointer");
  DASAC_REQUIRE(M > 0 && M <= 65535 && C > 0 && C % 64 == 0, "winograd4_wgrad_finish: needs 1..65535 output channels and a multiple of 64 input channels");
  const int splits = dasac_conv_wgrad_batched_splits(36, M, C, T);
  DASAC_REQUIRE(splits > 0, "winograd4_wgrad_finish: the batched weight-gradient launch does not take this shape");
  const size_t need = dasac_conv_wgrad_batched_workspace(36, M, C, T);
  if (ws_bytes < need) return fail(DASAC_EWORKSPACE, "winograd4_wgrad_finish: workspace too small (%zu < %zu)", ws_bytes, need);
  const int64_t p_elems = (int64_t)splits * 36 * M * C;
  DASAC_REQUIRE(p_elems * 4 <= wino::kMaxBytes && (int64_t)M * C * 9 * 4 <= wino::kMaxBytes,
                "winograd4_wgrad_finish: a tensor exceeds the 4 GiB buffer-descriptor window");
  const float* P = reinterpret_cast<const float*>(workspace);
  hipLaunchKernelGGL(wino::wgrad_finish4, dim3(C / 64, M), dim3(wino::kBlock), 0, as_stream(stream), P, P + p_elems, splits, M, C, w, scale,
                     dw, dot, sum_dz, (unsigned)(p_elems * 4), (unsigned)((int64_t)M * C * 9 * 4));
  DASAC_CHECK_LAUNCH("winograd wgrad_finish4");
  return DASAC_OK;
}

// ---- F(4x4,3x3) forward and data gradient: entry points ------------------------------------------------------------------------
extern "C" int dasac_winograd4_filter(const float* w, const float* scale, int Cout, int Cin, int transposed, float* u,
                                      dasac_stream_t stream) {
  DASAC_REQUIRE(w && u, "winograd4_filter: null pointer");
  DASAC_REQUIRE(Cout > 0 && Cin > 0, "winograd4_filter: bad channel counts");
  const int M = transposed ? Cin : Cout, K = transposed ? Cout : Cin;
  const int Mpad = dasac_conv_mpad(M), Kpad = dasac_conv_kpad(K);
  const int64_t per_point = (int64_t)Kpad * Mpad;
  DASAC_REQUIRE(36 * per_point * 4 <= wino::kMaxBytes && (int64_t)Cout * Cin * 9 * 4 <= wino::kMaxBytes,
                "winograd4_filter: operand exceeds the 4 GiB buffer-descriptor window");
  hipLaunchKernelGGL(wino::filter_transform4, dim3((unsigned)((per_point + wino::kBlock - 1) / wino::kBlock)), dim3(wino::kBlock), 0,
                     as_stream(stream), w, scale, u, Cout, Cin, Mpad, Kpad, transposed ? 1 : 0, (unsigned)((int64_t)Cout * Cin * 9 * 4),
                     (unsigned)(36 * per_point * 4));
  DASAC_CHECK_LAUNCH("winograd filter_transform4");
  return DASAC_OK;
}

extern "C" int dasac_winograd4_output(const float* y, size_t y_bytes, int Nb, int M, int H, int W, int dilation, const float* shift,
                                      int relu, const uint32_t* mask_bits, uint32_t* relu_bits_out, float* out,
                                      dasac_stream_t stream) {
  DASAC_REQUIRE(y && out, "winograd4_output: null pointer");
  DASAC_REQUIRE(!(mask_bits && relu_bits_out), "winograd4_output: record the ReLU pattern OR mask with one");
  DASAC_REQUIRE(!relu_bits_out || relu, "winograd4_output: relu_bits_out records the pattern of a ReLU epilogue");
  Geom g;
  const int rc = wino_geom4(g, "winograd4_output", Nb, M, H, W, dilation);
  if (rc) return rc;
  const size_t need = (size_t)36 * M * g.T * 4;
  if (y_bytes < need) return fail(DASAC_EWORKSPACE, "winograd4_output: workspace too small (%zu < %zu)", y_bytes, need);
  const int npix = Nb * H * W, w32 = (npix + 31) / 32;
  DASAC_REQUIRE((int64_t)M * w32 * 4 < (1ll << 31), "winograd4_output: bit mask exceeds 2 GiB");
  const unsigned bits_bytes = (unsigned)((int64_t)M * w32 * 4), out_bytes = (unsigned)((int64_t)Nb * M * H * W * 4);
  const dim3 grid((g.T + wino::kBlock - 1) / wino::kBlock, M), block(wino::kBlock);
  hipStream_t s = as_stream(stream);
  if (mask_bits)
    hipLaunchKernelGGL(wino::output_transform4<true>, grid, block, 0, s, y, out, g, M, shift, relu, mask_bits, w32, (unsigned)need, out_bytes,
                       bits_bytes);
  else
    hipLaunchKernelGGL(wino::output_transform4<false>, grid, block, 0, s, y, out, g, M, shift, relu, mask_bits, w32, (unsigned)need, out_bytes,
                       bits_bytes);
  if (relu_bits_out) {
    DASAC_CHECK_LAUNCH("winograd output_transform4");
    hipLaunchKernelGGL(wino::relu_bits_pack, dim3((npix + wino::kBlock - 1) / wino::kBlock, M), block, 0, s, out, relu_bits_out, g, M, w32,
                       out_bytes, bits_bytes);
  }
  DASAC_CHECK_LAUNCH("winograd output_transform4");
  return DASAC_OK;
}
