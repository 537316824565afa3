// The SAC head on MI355X, view fusion: affine warps of the T teacher views into the reference frame, their pooling, and the
// warp back.  HBM-bound (gather-bound) streaming passes over [B,C,H,W] fp32 planes (C = 19): lanes run along pixels, the class
// dimension is a register loop.
//
//   warp_pool          models/sac.py:289-305 + 238-269 / 218-236          affine warp of T views -> fused pooling
//   warp_back          models/sac.py:309-311
//   warp_affine        models/sac.py:295-296 (diagnostic frame warp)
#include "head_common.hpp"

namespace dasac {

// ---- affine warps: affine_grid + grid_sample(bilinear, zeros, align_corners=False) -------------
struct Sample {
  int o00, o01, o10, o11;     // flat offsets (clamped)
  float w00, w01, w10, w11;   // weights, 0 when the corner is out of bounds
};
__device__ __forceinline__ Sample make_sample_ex(const float* __restrict__ th, int oy, int ox, int H, int W, int& cx0o, int& cx1o,
                                                 int& cy0o, int& cy1o) {
  const float xb = (2.f * (float)ox + 1.f) / (float)W - 1.f;
  const float yb = (2.f * (float)oy + 1.f) / (float)H - 1.f;
  const float gx = th[0] * xb + th[1] * yb + th[2];
  const float gy = th[3] * xb + th[4] * yb + th[5];
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float wx1 = ix - x0f, wx0 = (x0f + 1.f) - ix;
  const float wy1 = iy - y0f, wy0 = (y0f + 1.f) - iy;
  // keep the integer conversion safe for wild thetas
  const float xc = fminf(fmaxf(x0f, -2.f), (float)W + 1.f), yc = fminf(fmaxf(y0f, -2.f), (float)H + 1.f);
  const int x0 = (int)xc, y0 = (int)yc, x1 = x0 + 1, y1 = y0 + 1;
  const bool far = (xc != x0f) || (yc != y0f);
  const bool vx0 = !far && x0 >= 0 && x0 < W, vx1 = !far && x1 >= 0 && x1 < W;
  const bool vy0 = !far && y0 >= 0 && y0 < H, vy1 = !far && y1 >= 0 && y1 < H;
  const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
  const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
  Sample s;
  s.o00 = cy0 * W + cx0; s.o01 = cy0 * W + cx1; s.o10 = cy1 * W + cx0; s.o11 = cy1 * W + cx1;
  s.w00 = (vx0 && vy0) ? wx0 * wy0 : 0.f;
  s.w01 = (vx1 && vy0) ? wx1 * wy0 : 0.f;
  s.w10 = (vx0 && vy1) ? wx0 * wy1 : 0.f;
  s.w11 = (vx1 && vy1) ? wx1 * wy1 : 0.f;
  cx0o = cx0; cx1o = cx1; cy0o = cy0; cy1o = cy1;
  return s;
}
__device__ __forceinline__ Sample make_sample(const float* __restrict__ th, int oy, int ox, int H, int W) {
  int a, b, c, d;
  return make_sample_ex(th, oy, ox, H, W, a, b, c, d);
}
// The same sample with its four taps as TWO 8-byte gathers (round 5: the warp kernels are bound by the number of gather / store
// instructions their CU's address unit processes -- 130 us of gathers + 91 us of stores = warp_back's 220 -- not by bytes).  The
// two taps of a source row sit in columns {pb, pb + 1}, pb = min(cx0, W - 2): one dwordx2 at (row, pb) holds both, and a select
// per tap puts each into place (clamped columns included: cx0, cx1 are always pb or pb + 1).  W >= 2.
struct SampleP {
  unsigned a_top, a_bot;      // byte offsets of the two pairs
  bool hi0, hi1;              // tap column == pb + 1
  float w00, w01, w10, w11;
};
__device__ __forceinline__ SampleP make_sample_pair(const float* __restrict__ th, int oy, int ox, int H, int W) {
  int cx0, cx1, cy0, cy1;
  const Sample s = make_sample_ex(th, oy, ox, H, W, cx0, cx1, cy0, cy1);
  const int pb = min(cx0, W - 2);
  SampleP p;
  p.a_top = (unsigned)(cy0 * W + pb) * 4u;
  p.a_bot = (unsigned)(cy1 * W + pb) * 4u;
  p.hi0 = cx0 != pb;
  p.hi1 = cx1 != pb;
  p.w00 = s.w00; p.w01 = s.w01; p.w10 = s.w10; p.w11 = s.w11;
  return p;
}
__device__ __forceinline__ f32x2u ld_pair(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const f32x2u*>(reinterpret_cast<const char*>(base) + byte_off);
}
// pl[o00]*w00 + pl[o01]*w01 + pl[o10]*w10 + pl[o11]*w11 from the two pairs, same order as take()
__device__ __forceinline__ float blend_pairs(const f32x2u t, const f32x2u b, const SampleP& p) {
  const float v00 = p.hi0 ? t[1] : t[0], v01 = p.hi1 ? t[1] : t[0];
  const float v10 = p.hi0 ? b[1] : b[0], v11 = p.hi1 ? b[1] : b[0];
  return v00 * p.w00 + v01 * p.w01 + v10 * p.w10 + v11 * p.w11;
}
__device__ __forceinline__ float take(const float* __restrict__ pl, const Sample& s) {
  return pl[s.o00] * s.w00 + pl[s.o01] * s.w01 + pl[s.o10] * s.w10 + pl[s.o11] * s.w11;
}

// (Round 4, measured and rejected: walking the output in 64 x 4 pixel tiles -- a wave per row segment, four adjacent rows per block,
// so that vertically adjacent outputs share their source row inside a block -- to cut the over-fetch the counters show for these
// kernels (`warp_back` moves 2.4x, `warp_pool` 1.4x its algorithmic bytes: profiles/r4_head_kernel_pmc.md).  `warp_pool` went
// 294 -> 755 us, `warp_back` 220 -> 245 us: the linear pixel order keeps every wave's 19 x T class-plane streams sequential in
// DRAM, the tile order breaks each of them into 256-byte pieces three rows apart.  The linear order stays.)
// generic warp of a [B,C,H,W] tensor (frames_aligned diagnostic)
__global__ __launch_bounds__(kHB) void warp_affine(const float* __restrict__ x, const float* __restrict__ theta, int C,
                                                   int H, int W, float* __restrict__ out, int blocks_per_image) {
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
  const int HW = H * W;
  const float* th = theta + b * 6;
  for (int p = chunk * kHB + threadIdx.x; p < HW; p += blocks_per_image * kHB) {
    const Sample s = make_sample(th, p / W, p % W, H, W);
    for (int c = 0; c < C; ++c) {
      const size_t pb = ((size_t)b * C + c) * HW;
      out[pb + p] = take(x + pb, s);
    }
  }
}

// views -> reference frame -> pooled.  One thread per (group, pixel):
//   a_t   = sample(probs[n*T+t], theta[n*T+t])                     (teacher_aligned, optional output)
//   cov_t = coverage(theta_inv[n*T+t]) at this pixel               (sac.py:299-301, quirk 4)
//   avg (mode 0):  S = sum_t a_t*cov_t ; Z = sum_c S ; mask = Z > tol ; S /= max(Z, 1e-3)
//   minentropy (mode 1): S = a_t*cov_t of the view with the lowest entropy (first minimum)
__global__ __launch_bounds__(kHB) void warp_pool(const float* __restrict__ probs, const float* __restrict__ theta,
                                                 const float* __restrict__ theta_inv, int T, int C, int H, int W,
                                                 int mode, float tol, float* __restrict__ aligned,
                                                 float* __restrict__ pooled, float* __restrict__ mask,
                                                 int blocks_per_group) {
  const int n = blockIdx.x / blocks_per_group, chunk = blockIdx.x % blocks_per_group;
  const int HW = H * W;
  for (int p = chunk * kHB + threadIdx.x; p < HW; p += blocks_per_group * kHB) {
    const int oy = p / W, ox = p - oy * W;
    float S[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) S[c] = 0.f;
    float best_ent = INFINITY, zsum = 0.f;
    for (int t = 0; t < T; ++t) {
      const int b = n * T + t;
      float v[kMaxC];
      float vs = 0.f;
      if (theta) {
        const Sample s = make_sample(theta + b * 6, oy, ox, H, W);
        const Sample si = make_sample(theta_inv + b * 6, oy, ox, H, W);
        const float cov = si.w00 + si.w01 + si.w10 + si.w11;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < C) {
            const size_t pb = ((size_t)b * C + c) * HW;
            const float a = take(probs + pb, s);
            if (aligned) aligned[pb + p] = a;
            v[c] = a * cov;
            vs += v[c];
          }
      } else {   // views already aligned and coverage-weighted by the caller (SAC._avg_pool / _minentropy_pool on their own)
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < C) {
            v[c] = probs[((size_t)b * C + c) * HW + p];
            vs += v[c];
          }
      }
      if (mode == 0) {
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < C) S[c] += v[c];
      } else {
        // sac.py:189-196 entropy with eps = 1e-5; empty pixels get 1/eps
        float ent = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < C) ent -= v[c] * logf((v[c] + 1e-5f) / (1.f + 1e-5f));
        if (vs < 0.1f) ent = 1.f / 1e-5f;
        zsum += vs;
        if (ent < best_ent) {
          best_ent = ent;
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c < C) S[c] = v[c];
        }
      }
    }
    float m;
    if (mode == 0) {
      float Z = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) Z += S[c];
      m = Z > tol ? 1.f : 0.f;
      const float den = fmaxf(Z, 1e-3f);
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) S[c] = S[c] / den;
    } else {
      m = zsum > tol ? 1.f : 0.f;
    }
    mask[(size_t)n * HW + p] = m;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) pooled[((size_t)n * C + c) * HW + p] = S[c];
  }
}

// The default configuration (avg pooling of TT <= 4 warped views, CT classes known at compile time) with the memory-level
// parallelism the generic kernel above lacks: that one walks the views one after the other and, the class count being a
// runtime value, gets four dependent-looking gathers in flight at a time -- 1.5 TB/s of algorithmic bytes, latency-bound.
// Here the T sample descriptors of a pixel are built first, then every class issues its 4*T taps as ONE batch (16 independent
// loads for T = 4; the unrolled class loop lets the compiler run several classes ahead).  Same arithmetic in the same order
// (per class S = ((a0*cov0 + a1*cov1) + a2*cov2) + a3*cov3 accumulated from 0 in view order, then Z, mask, S / max(Z, 1e-3)):
// bit-identical to the generic kernel, which stays for min-entropy pooling, pre-aligned views, T > 4 and other class counts.
// Round 5: every plane base is a scalar (group pointer + compile-time (view, class) offset) and the pixel a 32-bit lane offset --
// no 64-bit per-lane address arithmetic in front of the 16 gathers and 4 stores of a class: 2054 instead of 2672 VALU instructions
// per pixel, 325 -> 235 us at 2 x 4 x 19 x 769^2 (same box, tools/head_exp.py).  DASAC_WP_ROWS vertically adjacent pixels per
// thread (the row below shares a source row: fewer L2 fills, as in warp_back): 2 rows need 256 VGPRs and run 566 us -- one row.
constexpr int kWpRows = 1;
__device__ __forceinline__ float take_off(const float* __restrict__ pl, const Sample& s) {
  return ld_off(pl, (unsigned)s.o00 * 4u) * s.w00 + ld_off(pl, (unsigned)s.o01 * 4u) * s.w01 + ld_off(pl, (unsigned)s.o10 * 4u) * s.w10 +
         ld_off(pl, (unsigned)s.o11 * 4u) * s.w11;
}
template <int CT, int TT, int R>
__device__ __forceinline__ void warp_pool_rows(const float* __restrict__ probs_n, const float* __restrict__ theta_n,
                                               const float* __restrict__ theta_inv_n, int H, int W, int HW, float tol,
                                               float* __restrict__ aligned_n, float* __restrict__ pooled_n,
                                               float* __restrict__ mask_n, int oy, int ox) {
  Sample s[R][TT];                              // (8-byte pair gathers as in warp_back: 280 against 225 us here -- four dword gathers stay)
  float cov[R][TT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      s[r][t] = make_sample(theta_n + t * 6, oy + r, ox, H, W);
      const Sample si = make_sample(theta_inv_n + t * 6, oy + r, ox, H, W);
      cov[r][t] = si.w00 + si.w01 + si.w10 + si.w11;
    }
  const unsigned o0 = (unsigned)(oy * W + ox) * 4u, pitch = (unsigned)W * 4u;
  float S[R][CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    float a[R][TT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int t = 0; t < TT; ++t) a[r][t] = take_off(probs_n + (size_t)(t * CT + c) * HW, s[r][t]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (aligned_n) *at_off(aligned_n + (size_t)(t * CT + c) * HW, o0 + (unsigned)r * pitch) = a[r][t];
        acc += a[r][t] * cov[r][t];
      }
      S[r][c] = acc;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float Z = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) Z += S[r][c];
    const float den = fmaxf(Z, 1e-3f);
    *at_off(mask_n, o0 + (unsigned)r * pitch) = Z > tol ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) *at_off(pooled_n + (size_t)c * HW, o0 + (unsigned)r * pitch) = S[r][c] / den;
  }
}
template <int CT, int TT>
__global__ __launch_bounds__(kHB) void warp_pool_avg(const float* __restrict__ probs, const float* __restrict__ theta,
                                                     const float* __restrict__ theta_inv, int H, int W, float tol,
                                                     float* __restrict__ aligned, float* __restrict__ pooled,
                                                     float* __restrict__ mask, int blocks_per_group, int items, FastDiv div_w) {
  const int n = blockIdx.x / blocks_per_group, chunk = blockIdx.x % blocks_per_group;
  const int HW = H * W;
  const float* probs_n = probs + (size_t)n * TT * CT * HW;
  float* aligned_n = aligned ? aligned + (size_t)n * TT * CT * HW : nullptr;
  float* pooled_n = pooled + (size_t)n * CT * HW;
  float* mask_n = mask + (size_t)n * HW;
  const float* th = theta + n * TT * 6;
  const float* thi = theta_inv + n * TT * 6;
  for (int it = chunk * kHB + threadIdx.x; it < items; it += blocks_per_group * kHB) {
    const int rr = fdiv(it, div_w), ox = it - rr * W;
    const int oy = kWpRows * rr;
    if (oy + kWpRows <= H) {
      warp_pool_rows<CT, TT, kWpRows>(probs_n, th, thi, H, W, HW, tol, aligned_n, pooled_n, mask_n, oy, ox);
    } else {
      for (int y = oy; y < H; ++y) warp_pool_rows<CT, TT, 1>(probs_n, th, thi, H, W, HW, tol, aligned_n, pooled_n, mask_n, y, ox);
    }
  }
}

// refined[b] = sample(pooled[g(b)], theta_inv[b]) * sample(mask[g(b)], theta_inv[b]),  g(b) = group_of[b]
// (round 4, measured: a compile-time class count with all 4 x 19 taps of a pixel in flight makes this kernel SLOWER -- 327 vs
// 213 us at 8 x 19 x 769^2: the registers of 76 gathers in flight cost more occupancy than the batching wins; the class loop stays)
// Round 5: a thread owns kWbRows vertically adjacent pixels.  The counters showed 2.4x the algorithmic bytes entering L2: the
// row below re-reads the lower source row of the row above, and in the linear pixel order that neighbour is another block on
// another XCD (its own L2).  With the rows in one thread a shared source row is fetched once per group of rows, and sixteen
// taps are in flight instead of four.  The block still walks the plane of row groups linearly, so the store streams stay
// sequential in DRAM; per pixel the same make_sample / take arithmetic: identical bits.  Class planes are scalar
// bases + 32-bit per-lane byte offsets.  Same-box A/B of two rows against the one-row kernel (tools/head_exp.py, three pairs):
// 204 / 215 / 205 us against 214 / 232 / 215 at 8 x 19 x 769^2.  L2 fills per launch (FETCH_SIZE x 2): 687 MB with one row, 568
// with two, 503 with four (kWbRows) against 360 MB for one pass per view; kernel time 217 / 208 / 202 us.  Knock-outs: without
// its stores 130 us, without its gathers 91 us, without both 32 us -- 130 + 91 = the kernel: loads and stores do not overlap,
// what adds up is the number of gather / store instructions the CU's address unit works through.  Hence (late in the round) the
// four taps as two 8-byte pair gathers (SampleP) and the next class's gathers issued in front of this class's stores: 219 -> 192
// us, same box.  (The same pairs in warp_pool_avg: 225 -> 281 us -- kept there as four dword gathers.)
// (Measured and rejected on the way: four horizontally adjacent pixels per thread with dwordx4 stores 364 us -- gathers whose
// lanes sit 16 bytes apart; an XCD-aware chunk order (XCD x walks the x-th eighth of every pass, so that vertical neighbours
// share an L2) 224 against 208 us here and 445 against 311 us for warp_pool: what these kernels need is the linear pixel
// order's sequential DRAM streams, not fewer L2 fills.)
constexpr int kWbRows = 4;       // vertically adjacent output pixels per thread
// R rows of one output column: R sample descriptors, then the classes NC at a time with all NC * R * 4 taps issued before the
// first is used (R, NC compile-time: as run-time predicates the compiler sinks the lower rows' taps under their test and waits
// for four loads at a time).
template <int R>
__device__ __forceinline__ void warp_back_rows(const float* __restrict__ pooled_n, const float* __restrict__ mask_n,
                                               const float* __restrict__ th, float* __restrict__ refined_b, int C, int H, int W,
                                               int HW, int oy, int ox) {
  SampleP s[R];
  float mv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s[r] = make_sample_pair(th, oy + r, ox, H, W);
    mv[r] = blend_pairs(ld_pair(mask_n, s[r].a_top), ld_pair(mask_n, s[r].a_bot), s[r]);
  }
  const unsigned o0 = (unsigned)(oy * W + ox) * 4u, pitch = (unsigned)W * 4u;
  // One class = R * 2 pair gathers and R stores.  vmcnt retires a wave's loads and stores in issue order, so a class whose
  // gathers are issued AFTER the previous class's stores waits for those stores to drain: two register sets, the next class's
  // gathers go out before this class's stores (208 against 221 us, same box).
  auto load = [&](f32x2u (&t)[R][2], int c) {
    const float* pl = pooled_n + (size_t)c * HW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      t[r][0] = ld_pair(pl, s[r].a_top);
      t[r][1] = ld_pair(pl, s[r].a_bot);
    }
  };
  auto store = [&](const f32x2u (&t)[R][2], int c) {
    float* out = refined_b + (size_t)c * HW;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float a = blend_pairs(t[r][0], t[r][1], s[r]);
      *at_off(out, o0 + (unsigned)r * pitch) = a * mv[r];
    }
  };
  f32x2u ta[R][2], tb[R][2];
  load(ta, 0);
  int c = 0;
  for (; c + 2 <= C; c += 2) {
    load(tb, c + 1);
    __builtin_amdgcn_sched_barrier(0);          // the gathers of class c + 1 stay in front of the stores of class c
    store(ta, c);
    if (c + 2 < C) load(ta, c + 2);
    __builtin_amdgcn_sched_barrier(0);
    store(tb, c + 1);
  }
  if (c < C) store(ta, c);
}
__global__ __launch_bounds__(kHB) void warp_back(const float* __restrict__ pooled, const float* __restrict__ mask,
                                                 const float* __restrict__ theta_inv, int group_div, int C, int H, int W,
                                                 float* __restrict__ refined, int blocks_per_image, int items, FastDiv div_w) {
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
  const int n = b / group_div;
  const int HW = H * W;
  const float* pooled_n = pooled + (size_t)n * C * HW;
  const float* mask_n = mask + (size_t)n * HW;
  float* refined_b = refined + (size_t)b * C * HW;
  for (int it = chunk * kHB + threadIdx.x; it < items; it += blocks_per_image * kHB) {
    const int r = fdiv(it, div_w), ox = it - r * W;
    const int oy = kWbRows * r;
    if (oy + kWbRows <= H) {
      warp_back_rows<kWbRows>(pooled_n, mask_n, theta_inv + b * 6, refined_b, C, H, W, HW, oy, ox);
    } else {                                    // the last rows of a height that is no multiple of kWbRows
      for (int y = oy; y < H; ++y) warp_back_rows<1>(pooled_n, mask_n, theta_inv + b * 6, refined_b, C, H, W, HW, y, ox);
    }
  }
}

// W == 1: no pair of columns exists for the 8-byte gathers above -- four scalar taps per sample (make_sample / take, the same
// products in the same order), one thread per output pixel.  Any size grid_sample accepts is accepted here too.
__global__ __launch_bounds__(kHB) void warp_back_scalar(const float* __restrict__ pooled, const float* __restrict__ mask,
                                                        const float* __restrict__ theta_inv, int group_div, int C, int H, int W,
                                                        float* __restrict__ refined, int blocks_per_image) {
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x % blocks_per_image;
  const int n = b / group_div;
  const int HW = H * W;
  const float* pooled_n = pooled + (size_t)n * C * HW;
  float* refined_b = refined + (size_t)b * C * HW;
  for (int p = chunk * kHB + threadIdx.x; p < HW; p += blocks_per_image * kHB) {
    const Sample s = make_sample(theta_inv + b * 6, p / W, p % W, H, W);
    const float mv = take(mask + (size_t)n * HW, s);
    for (int c = 0; c < C; ++c) refined_b[(size_t)c * HW + p] = take(pooled_n + (size_t)c * HW, s) * mv;
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_warp_affine(const float* x, const float* theta, int B, int C, int H, int W, float* out,
                                 dasac_stream_t stream) {
  DASAC_REQUIRE(x && theta && out && B > 0 && C > 0 && H > 0 && W > 0, "warp_affine: bad arguments");
  const int per = blocks_per_image((int64_t)H * W, B);
  hipLaunchKernelGGL(warp_affine, dim3(per * B), dim3(kHB), 0, as_stream(stream), x, theta, C, H, W, out, per);
  DASAC_CHECK_LAUNCH("warp_affine");
  return DASAC_OK;
}

extern "C" int dasac_warp_pool(const float* probs, const float* theta, const float* theta_inv, int N, int T, int C, int H,
                               int W, int mode, float tolerance, float* aligned, float* pooled, float* mask,
                               dasac_stream_t stream) {
  DASAC_REQUIRE(probs && pooled && mask && ((theta && theta_inv) || (!theta && !theta_inv && !aligned)), "warp_pool: null pointer");
  DASAC_REQUIRE(N > 0 && T > 0 && C > 0 && C <= kMaxC && (mode == 0 || mode == 1), "warp_pool: bad arguments");
  DASAC_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 30), "warp_pool: bad shape");
  const int per = blocks_per_image((int64_t)H * W, N);
  hipStream_t s = as_stream(stream);
  const int items_r = (H + kWpRows - 1) / kWpRows * W;
  const int per_r = blocks_per_image(items_r, N);
#define DASAC_WPA(TT) hipLaunchKernelGGL((warp_pool_avg<19, TT>), dim3(per_r * N), dim3(kHB), 0, s, probs, theta, theta_inv, H, W, tolerance, aligned, pooled, mask, per_r, items_r, fast_div(W))
  if (mode == 0 && theta && C == 19 && T == 4) DASAC_WPA(4);
  else if (mode == 0 && theta && C == 19 && T == 2) DASAC_WPA(2);
  else if (mode == 0 && theta && C == 19 && T == 1) DASAC_WPA(1);
  else
    hipLaunchKernelGGL(warp_pool, dim3(per * N), dim3(kHB), 0, s, probs, theta, theta_inv, T, C, H, W, mode, tolerance, aligned, pooled,
                       mask, per);
#undef DASAC_WPA
  DASAC_CHECK_LAUNCH("warp_pool");
  return DASAC_OK;
}

extern "C" int dasac_warp_back(const float* pooled, const float* mask, const float* theta_inv, int B, int views_per_group,
                               int C, int H, int W, float* refined, dasac_stream_t stream) {
  DASAC_REQUIRE(pooled && mask && theta_inv && refined && B > 0 && views_per_group > 0, "warp_back: bad arguments");
  DASAC_REQUIRE(C > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30), "warp_back: bad shape");
  hipStream_t s = as_stream(stream);
  if (W < 2) {          // the pair gathers need two columns: scalar taps for one-column maps
    const int per = blocks_per_image((int64_t)H * W, B);
    hipLaunchKernelGGL(warp_back_scalar, dim3(per * B), dim3(kHB), 0, s, pooled, mask, theta_inv, views_per_group, C, H, W, refined, per);
  } else {
    const int items = (H + kWbRows - 1) / kWbRows * W;      // groups of kWbRows rows
    const int per = blocks_per_image(items, B);
    hipLaunchKernelGGL(warp_back, dim3(per * B), dim3(kHB), 0, s, pooled, mask, theta_inv, views_per_group, C, H, W, refined, per, items,
                       fast_div(W));
  }
  DASAC_CHECK_LAUNCH("warp_back");
  return DASAC_OK;
}
