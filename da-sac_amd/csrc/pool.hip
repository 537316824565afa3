// Max pooling, forward and backward.
#include "common.hpp"

namespace dasac {

// ---- max pooling (deeplabv2.py:126 3x3/2 pad 1 ceil_mode; torchvision VGG 2x2/2) -------------------
// forward also records the argmax position inside the window (kh*k + kw), first maximum wins.
// KT / ST: compile-time window and stride (0 = take the runtime values): the 3x3/2 stem pool and the 2x2/2, 3x3/1 VGG pools
// get unrolled windows and no integer division by a runtime value; all index math is 32-bit (total < 2^31, checked by the host).
// argmax byte: bits 0-6 = position inside the window (kh*k + kw), bit 7 = (pooled value > 0) for windows up to 11 x 11 -- the
// backward pass with the producer's ReLU folded in (`relu_mask`) then needs no read of the pooled tensor (a third of its bytes)
constexpr int kPoolSignMaxK = 11;

template <int KT, int ST>
__global__ __launch_bounds__(256) void maxpool_fwd(const float* __restrict__ x, int H, int W, int OH, int OW, int k_rt, int s_rt,
                                                   int pad, float* __restrict__ y, uint8_t* __restrict__ arg, int total) {
  const int k = KT ? KT : k_rt, s = ST ? ST : s_rt;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int ow = i % OW, r = i / OW;
    const int oh = r % OH, plane = r / OH;
    const float* xp = x + (size_t)plane * H * W;
    const int ih0 = oh * s - pad, iw0 = ow * s - pad;
    float best = -INFINITY;
    int code = 0;
#pragma unroll
    for (int a = 0; a < (KT ? KT : 15); ++a) {
      if (!KT && a >= k) break;
      const int ih = ih0 + a;
      const bool rowok = (unsigned)ih < (unsigned)H;
#pragma unroll
      for (int b = 0; b < (KT ? KT : 15); ++b) {
        if (!KT && b >= k) break;
        const int iw = iw0 + b;
        if (rowok && (unsigned)iw < (unsigned)W) {
          const float v = xp[ih * W + iw];
          if (v > best || v != v) {
            best = v;
            code = a * k + b;
          }
        }
      }
    }
    y[i] = best;
    arg[i] = (uint8_t)(code | ((k <= kPoolSignMaxK && best > 0.f) ? 0x80 : 0));
  }
}

// The 3x3 / stride-2 stem pool (deeplabv2.py:126) and the 2x2 / 2 VGG pools with FOUR horizontally adjacent outputs per thread:
// the 3*ST + KT input columns under them are read once per window row as two dwordx4 + (KT + 3*ST - 8) scalars (9 load
// instructions per 4 outputs for 3x3/2 where the one-output kernel issues 36 dword loads), y leaves as one dwordx4.  Same scan
// order per output (rows outer, columns inner, first maximum wins, NaN propagates): identical y and argmax codes.
template <int KT, int ST>
__global__ __launch_bounds__(256) void maxpool_fwd_quad(const float* __restrict__ x, int H, int W, int OH, int OW, int pad,
                                                        float* __restrict__ y, uint8_t* __restrict__ arg, int items) {
  constexpr int NCOL = 3 * ST + KT;
  static_assert(NCOL >= 8 && NCOL <= 12, "maxpool_fwd_quad: two dwordx4 loads + up to four scalars per window row");
  const int OWq = (OW + 3) >> 2;
  for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
    const int q = it % OWq, r = it / OWq;
    const int oh = r % OH, plane = r / OH;
    const int ow0 = q * 4, nx = min(4, OW - ow0);
    const float* xp = x + (size_t)plane * H * W;
    const int ih0 = oh * ST - pad, iw0 = ow0 * ST - pad;
    const bool inner = iw0 >= 0 && iw0 + NCOL <= W;
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int code[4] = {0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < KT; ++a) {
      const int ih = ih0 + a;
      if ((unsigned)ih >= (unsigned)H) continue;
      const float* row = xp + ih * W + iw0;
      float v[NCOL];
      if (inner) {
        const f32x4u v0 = *reinterpret_cast<const f32x4u*>(row), v1 = *reinterpret_cast<const f32x4u*>(row + 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[c] = v0[c];
          v[4 + c] = v1[c];
        }
#pragma unroll
        for (int c = 8; c < NCOL; ++c) v[c] = row[c];
      } else {
#pragma unroll
        for (int c = 0; c < NCOL; ++c) v[c] = (unsigned)(iw0 + c) < (unsigned)W ? row[c] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < KT; ++b) {
          const int c = e * ST + b;
          const float val = v[c];
          if ((inner || (unsigned)(iw0 + c) < (unsigned)W) && (val > best[e] || val != val)) {
            best[e] = val;
            code[e] = a * KT + b;
          }
        }
    }
    const size_t o = ((size_t)plane * OH + oh) * OW + ow0;
    if (nx == 4) {
      *reinterpret_cast<f32x4u*>(y + o) = f32x4u{best[0], best[1], best[2], best[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < nx) y[o + e] = best[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nx) arg[o + e] = (uint8_t)(code[e] | (best[e] > 0.f ? 0x80 : 0));
  }
}

// dx[ih,iw] = sum over windows o containing (ih,iw) with argmax(o) == this position of dy(o)
// relu_mask: additionally require y(o) > 0 -- the pooled tensor is ReLU output, so this is exactly
// the ReLU backward of the producer folded in (no need to keep the un-pooled activation).
// Four consecutive input pixels of one row per thread: the (at most 2 x 3 for the 3x3/2 stem pool) windows that can
// have picked any of them are read ONCE (argmax code, pooled value, gradient) and each routes its gradient to the
// pixel its code names -- a scatter inside the thread's registers, no atomics; one dwordx4 store.  32-bit index math.
template <int KT, int ST>
__global__ __launch_bounds__(256) void maxpool_bwd(const float* __restrict__ dy, const float* __restrict__ y,
                                                   const uint8_t* __restrict__ arg, int H, int W, int OH, int OW, int k_rt,
                                                   int s_rt, int pad, int relu_mask, float* __restrict__ dx, int items) {
  const int k = KT ? KT : k_rt, s = ST ? ST : s_rt;
  const int Wq = (W + 3) >> 2;
  for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
    const int q = it % Wq, row = it / Wq;            // row = plane*H + ih
    const int ih = row % H, plane = row / H;
    const int iw0 = q * 4, nx = min(4, W - iw0);
    // windows: oh*s - pad <= ih <= oh*s - pad + k - 1, same for the columns iw0 .. iw0+3
    int oh_lo = (ih + pad - k + 1 + s - 1) / s, oh_hi = min((ih + pad) / s, OH - 1);
    int ow_lo = (iw0 + pad - k + 1 + s - 1) / s, ow_hi = min((iw0 + nx - 1 + pad) / s, OW - 1);
    if (ih + pad - k + 1 < 0) oh_lo = 0;
    if (iw0 + pad - k + 1 < 0) ow_lo = 0;
    const size_t ob = (size_t)plane * OH * OW;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KT > 0 && ST > 0) {
      // compile-time window / stride: at most NR x NC windows can have picked one of the four pixels.  ALL their argmax
      // codes, pooled values and gradients are loaded first (clamped addresses, one batch in flight), then routed -- the
      // runtime-bounded loop below serialises three dependent loads per window.
      constexpr int NR = (KT + ST - 1) / ST, NC = (3 + KT + ST - 1) / ST;
      int code[NR][NC];
      float yv[NR][NC], dv[NR][NC];
#pragma unroll
      for (int a = 0; a < NR; ++a)
#pragma unroll
        for (int b = 0; b < NC; ++b) {
          const size_t o = ob + (size_t)min(oh_lo + a, OH - 1) * OW + min(ow_lo + b, OW - 1);
          const int ab = arg[o];
          code[a][b] = ab & 0x7f;
          dv[a][b] = dy[o];
          yv[a][b] = !relu_mask ? 1.f : (KT <= kPoolSignMaxK ? (float)(ab >> 7) : y[o]);    // bit 7: pooled value > 0
        }
#pragma unroll
      for (int a = 0; a < NR; ++a)
#pragma unroll
        for (int b = 0; b < NC; ++b) {
          const int oh = oh_lo + a, ow = ow_lo + b;
          const int r = oh * s - pad + code[a][b] / k, c = ow * s - pad + code[a][b] % k - iw0;
          if (oh <= oh_hi && ow <= ow_hi && r == ih && (unsigned)c < 4u && yv[a][b] > 0.f) {
            const float d = dv[a][b];
            g[0] += c == 0 ? d : 0.f;
            g[1] += c == 1 ? d : 0.f;
            g[2] += c == 2 ? d : 0.f;
            g[3] += c == 3 ? d : 0.f;
          }
        }
    } else {
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const size_t o = ob + (size_t)oh * OW + ow;
        const int ab = arg[o];
        const int code = k <= kPoolSignMaxK ? (ab & 0x7f) : ab;
        const int r = oh * s - pad + code / k, c = ow * s - pad + code % k - iw0;
        if (r == ih && (unsigned)c < 4u && (!relu_mask || (k <= kPoolSignMaxK ? (ab >> 7) != 0 : y[o] > 0.f))) {
          const float d = dy[o];
          g[0] += c == 0 ? d : 0.f;
          g[1] += c == 1 ? d : 0.f;
          g[2] += c == 2 ? d : 0.f;
          g[3] += c == 3 ? d : 0.f;
        }
      }
    }
    float* out = dx + (size_t)row * W + iw0;
    if (nx == 4) {
      *reinterpret_cast<f32x4u*>(out) = f32x4u{g[0], g[1], g[2], g[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < nx) out[e] = g[e];
    }
  }
}

// The stem pool (3x3, stride 2, padding 1: deeplabv2.py:126) with a 2 x 4 input block per thread -- rows 2p, 2p+1, columns
// 4q .. 4q+3.  Round 5: the kernel above is ISSUE-bound, not byte-bound (tools/isa_count.py: 306 VALU + 122 SALU instructions per
// 16 bytes stored = 330 of its 400 us at 16 x 64 x 385^2); this one spends ~1/4 of that per pixel:
//   * window oh covers input rows 2oh-1 .. 2oh+1, so the block's rows meet window rows p and p+1 only and its columns meet window
//     columns 2q .. 2q+2: SIX windows per eight pixels (the one-row kernel reads six per four), each read once;
//   * which (window, argmax code) pairs can name which pixel is known at compile time: row 2p <- (p, a=1); row 2p+1 <- (p, a=2),
//     (p+1, a=0); column 4q <- (2q, b=1); 4q+1 <- (2q, b=2), (2q+1, b=0); 4q+2 <- (2q+1, b=1); 4q+3 <- (2q+1, b=2), (2q+2, b=0)
//     -- 18 compare/select/add triples instead of a computed scatter over every pixel of the thread;
//   * the two index divisions are multiplications (FastDiv).
// Every pixel adds its candidate windows in the order the kernel above does (window rows ascending, columns ascending, from
// +0), a window that does not exist or whose pooled value is not positive (ReLU bit) contributes +0: identical bits.
__global__ __launch_bounds__(256) void maxpool_bwd_3s2p1(const float* __restrict__ dy, const uint8_t* __restrict__ arg, int H, int W,
                                                         int OH, int OW, int relu_mask, float* __restrict__ dx, int items, int Hp,
                                                         int Wq, FastDiv div_wq, FastDiv div_hp) {
  for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
    const int rowp = fdiv(it, div_wq), q = it - rowp * Wq;       // rowp = plane * Hp + p
    const int plane = fdiv(rowp, div_hp), p = rowp - plane * Hp;
    const int ih = 2 * p, iw0 = 4 * q, ow0 = 2 * q;
    const size_t ob = (size_t)plane * OH * OW;
    float d[2][3];
    int code[2][3];
    const bool wide = ow0 + 2 < OW;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const bool rok = p + a < OH;
      const size_t o = ob + (size_t)min(p + a, OH - 1) * OW + ow0;
      float v[3];
      int ab[3];
      if (wide) {
        const f32x2u v01 = *reinterpret_cast<const f32x2u*>(dy + o);
        v[0] = v01[0];
        v[1] = v01[1];
        v[2] = dy[o + 2];
#pragma unroll
        for (int b = 0; b < 3; ++b) ab[b] = arg[o + b];
      } else {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const size_t ob_ = o + min(b, OW - 1 - ow0);
          v[b] = dy[ob_];
          ab[b] = arg[ob_];
        }
      }
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const bool ok = rok && ow0 + b < OW && (!relu_mask || (ab[b] & 0x80));
        d[a][b] = ok ? v[b] : 0.f;
        code[a][b] = ab[b] & 0x7f;
      }
    }
    auto pick = [&](int a, int ka, int b, int kb) { return code[a][b] == ka * 3 + kb ? d[a][b] : 0.f; };
    float g0[4], g1[4];
    // row 2p: window row p with a = 1
    g0[0] = 0.f + pick(0, 1, 0, 1);
    g0[1] = (0.f + pick(0, 1, 0, 2)) + pick(0, 1, 1, 0);
    g0[2] = 0.f + pick(0, 1, 1, 1);
    g0[3] = (0.f + pick(0, 1, 1, 2)) + pick(0, 1, 2, 0);
    // row 2p+1: window row p with a = 2, then window row p+1 with a = 0
    g1[0] = (0.f + pick(0, 2, 0, 1)) + pick(1, 0, 0, 1);
    g1[1] = (((0.f + pick(0, 2, 0, 2)) + pick(0, 2, 1, 0)) + pick(1, 0, 0, 2)) + pick(1, 0, 1, 0);
    g1[2] = (0.f + pick(0, 2, 1, 1)) + pick(1, 0, 1, 1);
    g1[3] = (((0.f + pick(0, 2, 1, 2)) + pick(0, 2, 2, 0)) + pick(1, 0, 1, 2)) + pick(1, 0, 2, 0);
    float* out = dx + ((size_t)plane * H + ih) * W + iw0;
    const bool two = ih + 1 < H;
    if (iw0 + 4 <= W) {
      *reinterpret_cast<f32x4u*>(out) = f32x4u{g0[0], g0[1], g0[2], g0[3]};
      if (two) *reinterpret_cast<f32x4u*>(out + W) = f32x4u{g1[0], g1[1], g1[2], g1[3]};
    } else {
      const int nx = W - iw0;
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (e < nx) {
          out[e] = g0[e];
          if (two) out[W + e] = g1[e];
        }
    }
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_maxpool_fwd(const float* x, int planes, int H, int W, int OH, int OW, int k, int s, int pad, float* y,
                                 uint8_t* argmax, dasac_stream_t stream) {
  DASAC_REQUIRE(x && y && argmax && planes > 0 && k > 0 && k <= 15 && s > 0, "maxpool_fwd: bad arguments");
  const int64_t total = (int64_t)planes * OH * OW;
  DASAC_REQUIRE(total < (1ll << 31), "maxpool_fwd: tensor too large");
  const dim3 grid(stream_grid(total, 256));
  hipStream_t st = as_stream(stream);
  const int items4 = planes * OH * ((OW + 3) / 4);
  const dim3 grid4(stream_grid(items4, 256));
  if (k == 3 && s == 2) hipLaunchKernelGGL((maxpool_fwd_quad<3, 2>), grid4, dim3(256), 0, st, x, H, W, OH, OW, pad, y, argmax, items4);
  else if (k == 2 && s == 2) hipLaunchKernelGGL((maxpool_fwd_quad<2, 2>), grid4, dim3(256), 0, st, x, H, W, OH, OW, pad, y, argmax, items4);
  else if (k == 3 && s == 1) hipLaunchKernelGGL((maxpool_fwd<3, 1>), grid, dim3(256), 0, st, x, H, W, OH, OW, k, s, pad, y, argmax, (int)total);
  else hipLaunchKernelGGL((maxpool_fwd<0, 0>), grid, dim3(256), 0, st, x, H, W, OH, OW, k, s, pad, y, argmax, (int)total);
  DASAC_CHECK_LAUNCH("maxpool_fwd");
  return DASAC_OK;
}

extern "C" int dasac_maxpool_bwd(const float* dy, const float* y, const uint8_t* argmax, int planes, int H, int W, int OH,
                                 int OW, int k, int s, int pad, int relu_mask, float* dx, dasac_stream_t stream) {
  DASAC_REQUIRE(dy && y && argmax && dx && planes > 0, "maxpool_bwd: bad arguments");
  const int64_t items = (int64_t)planes * H * ((W + 3) / 4);
  DASAC_REQUIRE(items < (1ll << 31) && k >= 1 && s >= 1, "maxpool_bwd: tensor too large");
  const dim3 grid(stream_grid(items, 256));
  hipStream_t st = as_stream(stream);
  const int Hp = (H + 1) / 2, Wq = (W + 3) / 4;
  if (k == 3 && s == 2 && pad == 1 && OH >= 1 && OW >= 1) {
    const int items2 = planes * Hp * Wq;
    hipLaunchKernelGGL(maxpool_bwd_3s2p1, dim3(stream_grid(items2, 256)), dim3(256), 0, st, dy, argmax, H, W, OH, OW, relu_mask, dx,
                       items2, Hp, Wq, fast_div(Wq), fast_div(Hp));
  } else if (k == 3 && s == 2) hipLaunchKernelGGL((maxpool_bwd<3, 2>), grid, dim3(256), 0, st, dy, y, argmax, H, W, OH, OW, k, s, pad, relu_mask, dx, (int)items);
  else if (k == 2 && s == 2) hipLaunchKernelGGL((maxpool_bwd<2, 2>), grid, dim3(256), 0, st, dy, y, argmax, H, W, OH, OW, k, s, pad, relu_mask, dx, (int)items);
  else if (k == 3 && s == 1) hipLaunchKernelGGL((maxpool_bwd<3, 1>), grid, dim3(256), 0, st, dy, y, argmax, H, W, OH, OW, k, s, pad, relu_mask, dx, (int)items);
  else hipLaunchKernelGGL((maxpool_bwd<0, 0>), grid, dim3(256), 0, st, dy, y, argmax, H, W, OH, OW, k, s, pad, relu_mask, dx, (int)items);
  DASAC_CHECK_LAUNCH("maxpool_bwd");
  return DASAC_OK;
}
