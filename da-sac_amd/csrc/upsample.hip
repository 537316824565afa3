// The SAC head on MI355X, bilinear half: the stride-8 logits to full resolution and back.  Like every head kernel these are
// HBM-bound streaming passes over [B,C,H,W] fp32 planes (C = 19): lanes run along pixels (coalesced NCHW plane reads), the class
// dimension is a register loop.
//
//   upsample_softmax   models/deeplabv2.py:217, models/sac.py:275-282   bilinear(ac=True) [+softmax, prior sums, pad mask]
//   upsample_bwd_x/y   transpose of the above (separable gather, deterministic)
// The bilinear taps (tap_ac / ac_scale) are bilinear.hpp's, the transpose's tap ranges upsample_index.hpp's; the inference label
// map (dasac_infer_labels) is in inference.hip.
#include "head_common.hpp"
#include "upsample_index.hpp"

#include <algorithm>

namespace dasac {

constexpr float kQ32 = 4294967296.f;     // fixed-point scale of the order-independent (integer) class sums

// Four consecutive high-res pixels of one row per thread, loop over classes.  Optional outputs:
//   up    [B,C,H,W]  upsampled logits
//   probs [B,C,H,W]  softmax(up) * (ignore ? 0 : 1)
//   csum  [C] class sums of the UNMASKED softmax (running class prior, sac.py:108), accumulated in Q32 fixed point
//         (order-independent => run-to-run bit-identical); the launcher converts the slots to double afterwards
// CT = compile-time class count (19 for Cityscapes) so the per-pixel class vectors stay in registers.
// HBM-bound: 76 B written per pixel and output.  Four pixels per thread make every store a (4-byte aligned) dwordx4 and
// let the pixels share their low-resolution taps: at the 8x factor of the backbone the four x positions touch at most
// three low-res columns, so a class costs 6 L1/L2 loads per 4 pixels instead of 16.

template <int CT, bool SOFTMAX, bool NARROW>
__global__ __launch_bounds__(kHB, (SOFTMAX && NARROW) ? 4 : 1) void upsample_softmax(const float* __restrict__ x, int Crt, int h, int w, int H, int W,
                                                        float sh, float sw, const uint8_t* __restrict__ ignore,
                                                        float* __restrict__ up, float* __restrict__ probs,
                                                        unsigned long long* __restrict__ csum, int items, FastDiv div_wq) {
  const int C = CT < kMaxC ? CT : Crt;          // CT == kMaxC is the generic (runtime-C) instantiation
  const int HW = H * W, hw = h * w, Wq = (W + 3) >> 2;
  const int b = blockIdx.y;                     // one image per block row: every plane base below is a scalar
  __shared__ unsigned long long s_sum[kMaxC];
  if (csum) {
    if (threadIdx.x < kMaxC) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
  }
  float acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0.f;
  // Round 5 (the kernel is issue-bound: ~4000 VALU instructions per 4 pixels in the probs path, tools/isa_count.py): the image
  // is the block row, so the class planes are scalar bases + ONE 32-bit per-lane byte offset shared by all classes (no 64-bit
  // per-lane address arithmetic per load / store); row / quad index by FastDiv; one select per tap instead of two.
  for (int it = blockIdx.x * kHB + threadIdx.x; it < items; it += gridDim.x * kHB) {
    const int oy = fdiv(it, div_wq), q = it - oy * Wq;
    const int ox = q * 4, nx = min(4, W - ox);
    const float* xb = x + (size_t)b * C * hw;
    const Tap ty = tap_ac(oy, sh, h);
    Tap tx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) tx[e] = tap_ac(min(ox + e, W - 1), sw, w);
    const int c_lo = tx[0].i0;
    // the usual case: the 4 pixels start in low-res column c_lo or c_lo + 1, so their taps are (t0,t1) or (t1,t2) -- t1, t2 read
    // at clamped columns, which is exactly where tap_ac puts i1 on the last column
    // (NARROW: the launcher has checked every quad of a row -- the up-factor-8 case; the kernel then carries no second path:
    // 131 instead of 207 VGPRs in the probs instantiation, three waves per SIMD instead of two)
    const bool narrow = NARROW || tx[3].i0 - c_lo <= 1;
    const int r0 = ty.i0 * w, r1 = ty.i1 * w;
    const int k1 = min(c_lo + 1, w - 1), k2 = min(c_lo + 2, w - 1);
    const unsigned a00 = (unsigned)(r0 + c_lo) * 4u, a01 = (unsigned)(r0 + k1) * 4u, a02 = (unsigned)(r0 + k2) * 4u;
    const unsigned a10 = (unsigned)(r1 + c_lo) * 4u, a11 = (unsigned)(r1 + k1) * 4u, a12 = (unsigned)(r1 + k2) * 4u;
    bool hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) hi[e] = tx[e].i0 != c_lo;
    float v[4][SOFTMAX ? CT : 1];                 // SOFTMAX: all classes of the 4 pixels stay in registers
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const size_t obase = (size_t)b * C * HW;      // scalar
    const unsigned ooff = (unsigned)(oy * W + ox) * 4u;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c < C) {
        const float* pl = xb + (size_t)c * hw;
        float val[4];
        if (narrow) {
          const float t0 = ld_off(pl, a00), t1 = ld_off(pl, a01), t2 = ld_off(pl, a02);
          const float b0 = ld_off(pl, a10), b1 = ld_off(pl, a11), b2 = ld_off(pl, a12);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float ta = hi[e] ? t1 : t0, tb = hi[e] ? t2 : t1;
            const float ba = hi[e] ? b1 : b0, bb = hi[e] ? b2 : b1;
            const float top = tx[e].w0 * ta + tx[e].w1 * tb;
            const float bot = tx[e].w0 * ba + tx[e].w1 * bb;
            val[e] = ty.w0 * top + ty.w1 * bot;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float top = tx[e].w0 * pl[r0 + tx[e].i0] + tx[e].w1 * pl[r0 + tx[e].i1];
            const float bot = tx[e].w0 * pl[r1 + tx[e].i0] + tx[e].w1 * pl[r1 + tx[e].i1];
            val[e] = ty.w0 * top + ty.w1 * bot;
          }
        }
        if (SOFTMAX) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e][c] = val[e];
            mx[e] = fmaxf(mx[e], val[e]);
          }
        } else {                                     // logits only: stream the class plane out, nothing kept
          store_quad(at_off(up + obase + (size_t)c * HW, ooff), f32x4u{val[0], val[1], val[2], val[3]}, nx);
        }
      }
    }
    if (SOFTMAX && up) {
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {                                   // (written out, like the probs tail below: on store_quad the softmax
          float* o = at_off(up + obase + (size_t)c * HW, ooff);   // instantiations lose their stream and <kMaxC> its timing row,
          if (nx == 4) {                               // profiles/head_split.md)
            *reinterpret_cast<f32x4u*>(o) = f32x4u{v[0][c], v[1][c], v[2][c], v[3][c]};
          } else {
#pragma unroll
            for (int e = 0; e < 3; ++e)
              if (e < nx) o[e] = v[e][c];
          }
        }
    }
    if (SOFTMAX && (probs || csum)) {
      float inv[4];
      bool ign[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) {
            v[e][c] = expf(v[e][c] - mx[e]);
            den += v[e][c];
          }
        inv[e] = 1.f / den;
        ign[e] = ignore && e < nx && ignore[(size_t)b * HW + (size_t)(oy * W + ox + e)];
      }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
          float pr[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            pr[e] = v[e][c] * inv[e];
            if (e < nx) acc[c] += pr[e];
            if (ign[e]) pr[e] = 0.f;
          }
          if (probs) {
            float* o = at_off(probs + obase + (size_t)c * HW, ooff);
            if (nx == 4) {
              *reinterpret_cast<f32x4u*>(o) = f32x4u{pr[0], pr[1], pr[2], pr[3]};
            } else {
#pragma unroll
              for (int e = 0; e < 3; ++e)
                if (e < nx) o[e] = pr[e];
            }
          }
        }
    }
  }
  if (csum) {
    // per-thread partials -> wave sums (shuffles, fixed order) -> Q32 fixed point: integer adds commute, so the LDS atomic per
    // wave and class and the global one per block and class give the SAME bits whatever order the waves / blocks arrive in
    // (a wave's sum of probabilities is < 2^13, the total < B*HW < 2^31: no overflow; 2^-33 rounding per wave partial).
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        const float ws = wave_sum(acc[c]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum[c], __float2ull_rn(ws * kQ32));
      }
    __syncthreads();
    if (threadIdx.x < C) atomicAdd(&csum[threadIdx.x], s_sum[threadIdx.x]);
  }
}

// (Round 4, measured and rejected: a two-pixels-per-thread variant of the probs path -- 152 instead of 225 VGPRs, three instead of two
// waves per SIMD, 8-byte stores -- runs 238 us against this kernel's 214 at 8 x 19 x 769^2, 297 us when forced to four waves per SIMD
// with 92 bytes of scratch: sharing the low-resolution taps among four pixels and the dwordx4 stores outweigh the occupancy.)
// class sums: Q32 fixed point -> double, in place (the caller's buffer holds 8-byte slots either way)
__global__ void q32_to_double(unsigned long long* __restrict__ q, int C) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const unsigned long long v = q[c];
  reinterpret_cast<double*>(q)[c] = (double)v * (1.0 / 4294967296.0);
}

// ---- transpose of the bilinear upsampling, separable and gather-based (deterministic) ---------
// pass X: tmp[plane][y][j] = sum_x wx(x->j) * g[plane][y][x]          (reads the big gradient once)
// pass Y: d[plane][i][j]   = gscale * sum_y wy(y->i) * tmp[plane][y][j]
__global__ __launch_bounds__(kHB) void upsample_bwd_x(const float* __restrict__ g, int H, int W, int w, float sw,
                                                      float* __restrict__ tmp, int64_t total) {
  // total = planes*H*w; thread -> (plane, y, j), j fastest
  for (int64_t i = (int64_t)blockIdx.x * kHB + threadIdx.x; i < total; i += (int64_t)gridDim.x * kHB) {
    const int j = (int)(i % w);
    const int64_t row = i / w;   // plane*H + y
    int lo, hi;
    src_range(j, sw, W, lo, hi);
    const float* gr = g + row * W;
    float s = 0.f;
    for (int x = lo; x <= hi; ++x) s += weight_to(x, sw, w, j) * gr[x];
    tmp[i] = s;
  }
}

__global__ __launch_bounds__(kHB) void upsample_bwd_y(const float* __restrict__ tmp, int H, int h, int w, float sh,
                                                      const float* __restrict__ gscale, float* __restrict__ d,
                                                      int64_t total) {
  const float gs = gscale ? gscale[0] : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * kHB + threadIdx.x; i < total; i += (int64_t)gridDim.x * kHB) {
    const int j = (int)(i % w);
    const int64_t r = i / w;
    const int ii = (int)(r % h);
    const int64_t plane = r / h;
    int lo, hi;
    src_range(ii, sh, H, lo, hi);
    const float* tp = tmp + plane * H * w + j;
    float s = 0.f;
    for (int y = lo; y <= hi; ++y) s += weight_to(y, sh, h, ii) * tp[(size_t)y * w];
    d[i] = s * gs;
  }
}

int launch_upsample_bwd_y(const float* tmp, int64_t planes, int H, int h, int w, const float* gscale, float* d, hipStream_t s) {
  const int64_t t2 = planes * h * w;
  hipLaunchKernelGGL(upsample_bwd_y, dim3(stream_grid(t2, kHB)), dim3(kHB), 0, s, tmp, H, h, w, ac_scale(h, H), gscale, d, t2);
  DASAC_CHECK_LAUNCH("upsample_bwd_y");
  return DASAC_OK;
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_upsample_softmax(const float* logits, int B, int C, int h, int w, int H, int W,
                                      const uint8_t* ignore, float* up, float* probs, double* class_sums,
                                      dasac_stream_t stream) {
  DASAC_REQUIRE(logits && (up || probs || class_sums), "upsample_softmax: null pointer");
  DASAC_REQUIRE(B > 0 && C > 0 && C <= kMaxC && h > 0 && w > 0 && H > 0 && W > 0, "upsample_softmax: bad shape");
  hipStream_t s = as_stream(stream);
  if (class_sums) DASAC_HIP(hipMemsetAsync(class_sums, 0, C * sizeof(double), s));
  DASAC_REQUIRE(B < 65536 && (int64_t)H * W < (1ll << 30) && (int64_t)h * w < (1ll << 30), "upsample_softmax: plane too large");
  const int Wq = (W + 3) / 4, items = H * Wq;    // per image: grid.y is the image
  const bool softmax = probs || class_sums;
  // softmax path: a few items per thread so that the class-sum reduction at the end is amortised
  const int total = stream_grid((int64_t)B * items, kHB, softmax ? kNumCu * 4 : kNumCu * 16);
  const int grid = std::max(1, std::min((items + kHB - 1) / kHB, (total + B - 1) / B));
  const float sw = ac_scale(w, W);
  bool narrow = true;                            // tap_ac's column arithmetic, on the host (one fp32 multiply: same bits)
  for (int ox = 0; ox < W && narrow; ox += 4) {
    auto col = [&](int dst) { return std::min((int)(sw * (float)dst), w - 1); };
    narrow = col(std::min(ox + 3, W - 1)) - col(ox) <= 1;
  }
#define DASAC_UPS(CT, SM, NW)                                                                                                  \
  hipLaunchKernelGGL((upsample_softmax<CT, SM, NW>), dim3(grid, B), dim3(kHB), 0, s, logits, C, h, w, H, W, ac_scale(h, H), \
                     sw, ignore, up, probs, reinterpret_cast<unsigned long long*>(class_sums), items, fast_div(Wq))
  if (C == 19 && narrow) {
    if (softmax) DASAC_UPS(19, true, true); else DASAC_UPS(19, false, true);
  } else if (C == 19) {
    if (softmax) DASAC_UPS(19, true, false); else DASAC_UPS(19, false, false);
  } else {
    if (softmax) DASAC_UPS(kMaxC, true, false); else DASAC_UPS(kMaxC, false, false);
  }
#undef DASAC_UPS
  DASAC_CHECK_LAUNCH("upsample_softmax");
  if (class_sums) {
    hipLaunchKernelGGL(q32_to_double, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned long long*>(class_sums), C);
    DASAC_CHECK_LAUNCH("q32_to_double");
  }
  return DASAC_OK;
}

extern "C" size_t dasac_upsample_bwd_workspace(int planes, int H, int w) { return (size_t)planes * H * w * sizeof(float); }

extern "C" int dasac_upsample_bwd(const float* grad_up, int planes, int h, int w, int H, int W, const float* gscale,
                                  float* grad_low, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(grad_up && grad_low && workspace, "upsample_bwd: null pointer");
  if (ws_bytes < dasac_upsample_bwd_workspace(planes, H, w)) return fail(DASAC_EWORKSPACE, "upsample_bwd: workspace too small");
  hipStream_t s = as_stream(stream);
  float* tmp = reinterpret_cast<float*>(workspace);
  const int64_t t1 = (int64_t)planes * H * w;
  hipLaunchKernelGGL(upsample_bwd_x, dim3(stream_grid(t1, kHB)), dim3(kHB), 0, s, grad_up, H, W, w, ac_scale(w, W), tmp, t1);
  DASAC_CHECK_LAUNCH("upsample_bwd_x");
  return launch_upsample_bwd_y(tmp, planes, H, h, w, gscale, grad_low, s);
}
