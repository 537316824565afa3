// Small HBM-bound helpers around the conv GEMMs: frozen-BN folding and parameter gradients,
// max-pooling, per-channel reductions, the momentum-teacher multi-tensor update, Dropout2d scaling.
#include "common.hpp"

namespace dasac {

// ---- frozen BatchNorm (eval mode; models/__init__.py:29 + models/basenet.py:97-100) -------------
// ATen eval batch_norm: invstd = 1/sqrt(var+eps); alpha = gamma*invstd; beta' = beta - mean*alpha
__global__ void bn_fold(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                        const float* __restrict__ var, const float* __restrict__ conv_bias, float eps, int C,
                        float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float is = 1.f / sqrtf(var[c] + eps);
  const float a = gamma[c] * is;
  const float m = conv_bias ? mean[c] - conv_bias[c] : mean[c];   // BN(conv + b) = a*conv + (beta - (mean-b)*a)
  scale[c] = a;
  shift[c] = beta[c] - m * a;
  if (invstd) invstd[c] = is;
}

// every frozen BN of a network in one launch: chunk (j, c) = 256 channels of job j
__global__ __launch_bounds__(256) void bn_fold_multi(const dasac_fold_job* __restrict__ jobs, const int2* __restrict__ chunks) {
  const int2 ch = chunks[blockIdx.x];
  const dasac_fold_job jb = jobs[ch.x];
  const int c = ch.y * 256 + threadIdx.x;
  if (c >= jb.C) return;
  const float is = 1.f / sqrtf(jb.var[c] + jb.eps);
  const float a = jb.gamma[c] * is;
  const float m = jb.conv_bias ? jb.mean[c] - jb.conv_bias[c] : jb.mean[c];
  jb.scale[c] = a;
  jb.shift[c] = jb.beta[c] - m * a;
  jb.invstd[c] = is;
}

// dgamma = invstd*(dot + (b - mean)*sum_dz), dbeta = sum_dz, dbias_conv = scale*sum_dz
// dot: [dot_rows][C] partial rows of dasac_conv_wgrad_finish, added here in row order (deterministic)
__global__ void bn_param_grads(const float* __restrict__ dot, int dot_rows, const float* __restrict__ sum_dz,
                               const float* __restrict__ mean,
                               const float* __restrict__ invstd, const float* __restrict__ scale,
                               const float* __restrict__ conv_bias, int C, float* __restrict__ dgamma,
                               float* __restrict__ dbeta, float* __restrict__ dbias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = sum_dz[c];
  const float b = conv_bias ? conv_bias[c] : 0.f;
  if (dgamma) {
    float d = 0.f;
    for (int r = 0; r < dot_rows; ++r) d += dot[(size_t)r * C + c];
    dgamma[c] = invstd[c] * (d + (b - mean[c]) * s);
  }
  if (dbeta) dbeta[c] = s;
  if (dbias) dbias[c] = (scale ? scale[c] : 1.f) * s;
}

// out[c] = sum_{n,p} x[n,c,p]; one block per channel
__global__ __launch_bounds__(256) void channel_sums(const float* __restrict__ x, int N, int C, int HW, float* __restrict__ out) {
  const int c = blockIdx.x;
  double s = 0;
  for (int n = 0; n < N; ++n) {
    const float* p = x + ((size_t)n * C + c) * HW;
    float part = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) part += p[i];
    s += part;
  }
  __shared__ double red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (float)(red[0] + red[1] + red[2] + red[3]);
}

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

// ---- momentum teacher (models/sac.py:83-102) as one multi-tensor launch --------------------------
// chunk table: for chunk i, tensor id + chunk index.  sq_chunk[i] = sum (slow-fast)^2 over the chunk (pre-update);
// if update: slow = slow*m + fast*(1-m).
struct TensorPair {
  const float* fast;
  float* slow;
  int64_t n;
};
constexpr int kEmaChunk = 256 * 16;

__global__ __launch_bounds__(256) void ema_chunks(const TensorPair* __restrict__ pairs, const int2* __restrict__ chunks,
                                                  float momentum, float one_minus, int update, double* __restrict__ sq_chunk) {
  const int2 ch = chunks[blockIdx.x];
  const TensorPair tp = pairs[ch.x];
  const int64_t base = (int64_t)ch.y * kEmaChunk;
  double acc = 0;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < tp.n) {
      const float f = tp.fast[i], sl = tp.slow[i];
      const float d = sl - f;
      acc += (double)d * (double)d;
      if (update) {
        float v = sl * momentum;
        v = v + f * one_minus;
        tp.slow[i] = v;
      }
    }
  }
  __shared__ double red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) sq_chunk[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);      // one partial per chunk: no atomics
}

// sq[t] = sum of tensor t's chunk partials, in a fixed order (one wave per tensor; `chunks` is sorted by tensor id)
__global__ __launch_bounds__(64) void ema_tensor_sums(const int2* __restrict__ chunks, int n_chunks, const double* __restrict__ sq_chunk,
                                                      double* __restrict__ sq) {
  const int t = blockIdx.x;
  int lo = 0, hi = n_chunks;                       // first chunk whose tensor id is >= t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunks[mid].x < t) lo = mid + 1; else hi = mid;
  }
  double s = 0;
  for (int i = lo + threadIdx.x; i < n_chunks && chunks[i].x == t; i += 64) s += sq_chunk[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) sq[t] = s;
}

__global__ void ema_finish(const double* __restrict__ sq, int n, float* __restrict__ out) {
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 64) s += sqrt(sq[i]);
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = (float)s;
}

// ---- torch.optim.SGD(momentum, dampening 0, nesterov or not) over every parameter in one launch ---------
// (base_trainer.py:63-66 builds it over the four groups of basenet.py:73-95; per-group lr / weight decay)
//   d = g (+ g2) + wd*p ;  buf = first ? d : momentum*buf + d ;  p = p - lr*buf        (same op order as ATen)
// NESTEROV (OPT_NESTEROV, base_trainer.py:64): p = p - lr*(d + momentum*buf) -- torch/optim/sgd.py:462-473,
// `_foreach_add_(grads, bufs, alpha=momentum)` then `_foreach_add_(params, grads, alpha=-lr)`, each `x + alpha*y` one fma.
// g2 (optional): a second gradient of the same parameter -- the source-pass gradient the driver set aside while the target
// pass ran (train.py accumulates both into .grad: one `add_` launch per parameter, 320 per step; here the sum happens in
// the update itself, g2 + g in AccumulateGrad's operand order, so the result is bit-identical).
struct SgdTensor {
  float* p;
  const float* g;
  const float* g2;
  float* buf;
  int64_t n;
  int64_t group;
};
struct SgdGroups {
  float lr[8], wd[8];
};

// a*b + c as ATen's foreach kernels compute it: they are built with fp contraction, so every `x + alpha*y` of theirs is ONE fma
// (tools/aten_contraction_probe.py: 2^20 elements per op, no element differs from the fma form; profiles/fused_optim.md).
// This file is built with contraction off: the plain-momentum kernel keeps the two roundings it has always had.
template <bool FMA>
__device__ __forceinline__ float mul_add(float a, float b, float c) {
  return FMA ? __fmaf_rn(a, b, c) : a * b + c;
}

// ---- global gradient-norm clipping / non-finite step skipping: the device control block -----------------
// Written by grad_norm_finish (below the update kernels), read by the CTL forms of sgd_chunks / adam_chunks.  The update
// needs ONE global fact before any parameter may be written -- the L2 norm of g2 + g over ALL parameters -- and takes it from
// here, so the host never sees it (no synchronisation).  flags: kCtlClip multiplies the summed gradient by `coef` (one fp32
// multiply, before weight decay: what clip_grad_norm_ does to .grad); kCtlSkip makes every block return without a write while
// `skip` is set.
struct GradCtl {
  float total;          // ||g2 + g||_2 over every tensor of the table, before clipping
  float coef;           // min(max_norm / (total + 1e-6), 1), NaN kept as torch.clamp keeps it; 1 when only measuring
  int32_t skip;         // total is not finite
  int32_t reserved;
};
static_assert(sizeof(GradCtl) == 16, "GradCtl is the 16-byte control block of include/dasac_hip.h");
constexpr int kCtlClip = 1, kCtlSkip = 2;

// CTL = false is the kernel as it has always been (`ctl` / `flags` unused).  CTL = true: `first` may be -1, then bit 32 of each
// row's `group` says whether THAT tensor takes its first step -- one table and one norm for the whole step.  A skipped first step
// still writes buf = -0: the host has allocated the buffer and will call the next step a later one, whose momentum*(-0) + d is
// d for every d (a +0 would turn d = -0 into +0), i.e. exactly the first-step rule.
template <bool NESTEROV, bool CTL>
__global__ __launch_bounds__(256) void sgd_chunks(const SgdTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                  SgdGroups hp, float momentum, int first, const GradCtl* __restrict__ ctl, int flags) {
  const int2 ch = chunks[blockIdx.x];
  const SgdTensor t = tensors[ch.x];
  const int64_t group = CTL ? (t.group & 7) : t.group;
  const float lr = hp.lr[group], wd = hp.wd[group];
  const int64_t base = (int64_t)ch.y * kEmaChunk;
  bool clip = false;
  float coef = 1.f;
  if (CTL) {
    if (first < 0) first = (int)((t.group >> 32) & 1);
    if ((flags & kCtlSkip) && ctl->skip) {
      if (first) {
#pragma unroll 4
        for (int j = 0; j < 16; ++j) {
          const int64_t i = base + j * 256 + threadIdx.x;
          if (i < t.n) t.buf[i] = -0.f;
        }
      }
      return;
    }
    clip = (flags & kCtlClip) != 0;
    coef = ctl->coef;
  }
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < t.n) {
      const float p = t.p[i];
      float d = t.g[i];
      if (t.g2) d = t.g2[i] + d;
      if (CTL) {
        if (clip) d = d * coef;
      }
      if (wd != 0.f) d = mul_add<NESTEROV>(wd, p, d);
      float b = d;
      if (!first) {
        b = t.buf[i] * momentum;
        b = b + d;
      }
      t.buf[i] = b;
      if (NESTEROV) b = mul_add<true>(momentum, b, d);      // sgd.py:462-465, grad.add(buf, alpha=momentum)
      t.p[i] = mul_add<NESTEROV>(-lr, b, p);
    }
  }
}

// ---- torch.optim.Adam (L2 weight decay in the gradient, no amsgrad / maximize) over every parameter in one launch ---------
// (base_trainer.py:57-61: Adam(groups, lr, betas=(BETA1, 0.999), weight_decay); core/config.py:135-140 ships BETA1 = 0.5).
// Operation order of torch/optim/adam.py, _multi_tensor_adam, the non-capturable, non-amsgrad path (torch 2.10):
//   :698-700  g = g + wd*p                      _foreach_add(grads, params, alpha=weight_decay), only if wd != 0
//   :705-707  m = lerp(m, g, 1 - beta1)         _foreach_lerp_; ATen/native/Lerp.h:32-34 picks the formula by |w| < 0.5:
//                                               m + w*(g - m)   or   g - (g - m)*(1 - w)    (BETA1 = 0.5 takes the second)
//   :709      v = v*beta2                       _foreach_mul_
//   :722-724  v = v + (1 - beta2)*(g*g)         _foreach_addcmul_: a + value*(b*c)
//   :772-781  step_size = lr/(1 - beta1^step), bc2_sqrt = (1 - beta2^step)^0.5: python doubles, per tensor (HOST side)
//   :791-794  den = sqrt(v); den = den/bc2_sqrt; den = den + eps
//   :795-800  p = p + (-step_size)*(m/den)      _foreach_addcdiv_: a + value*(b/c)
// with every scalar rounded to fp32 once (the foreach functors' opmath type) and every `a + s*x` above one fma, as ATen's
// kernels contract it (mul_add<true>; the separate _foreach_mul_ / sqrt / div / add passes round on their own).  This file is
// compiled without fast-math: `/` and sqrtf are the correctly rounded ones.  g2 as for sgd_chunks.
struct AdamTensor {
  float* p;
  const float* g;
  const float* g2;
  float* m;
  float* v;
  int64_t n;
  int32_t group;
  int32_t reserved;
  float step_size;
  float bc2_sqrt;
};
static_assert(sizeof(AdamTensor) == 64, "AdamTensor is 8 x 8 bytes (dasac_hip/optim.py builds it as int64 rows)");
struct AdamGroups {
  float wd[8];
};
struct AdamScalars {
  float w1, one_minus_w1, beta2, w2, eps;      // w1 = 1 - beta1, w2 = 1 - beta2 (rounded from the double difference)
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float wd, float neg_step, float bc2_sqrt,
                                             const AdamScalars& s, bool small_w) {
  if (wd != 0.f) g = mul_add<true>(wd, p, g);
  const float diff = g - m;
  m = small_w ? mul_add<true>(s.w1, diff, m) : mul_add<true>(-diff, s.one_minus_w1, g);
  v = v * s.beta2;
  v = mul_add<true>(s.w2, g * g, v);
  float den = sqrtf(v);
  den = den / bc2_sqrt;
  den = den + s.eps;
  p = mul_add<true>(neg_step, m / den, p);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));      // 16-byte aligned: one global_load/store_dwordx4
// CTL = false is the kernel as it has always been (`ctl` / `flags` unused); CTL = true: GradCtl above.
template <bool CTL>
__global__ __launch_bounds__(256) void adam_chunks(const AdamTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                   AdamGroups hp, AdamScalars s, const GradCtl* __restrict__ ctl, int flags) {
  const int2 ch = chunks[blockIdx.x];
  const AdamTensor t = tensors[ch.x];
  const float wd = hp.wd[t.group & 7], neg_step = -t.step_size, bc2_sqrt = t.bc2_sqrt;
  const bool small_w = fabsf(s.w1) < 0.5f;
  const int64_t base = (int64_t)ch.y * kEmaChunk;
  bool clip = false;
  float coef = 1.f;
  if (CTL) {
    if ((flags & kCtlSkip) && ctl->skip) return;      // p, m and v stay as they are
    clip = (flags & kCtlClip) != 0;
    coef = ctl->coef;
  }
  // 16-byte accesses where the whole chunk lies inside the tensor and every pointer allows them (a gradient inside a
  // flat reduction buffer may sit at any 4-byte offset); `base` is a multiple of 4096 elements, so alignment is the pointers'
  const uintptr_t bits = (uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.g2 | (uintptr_t)t.m | (uintptr_t)t.v;
  if ((bits & 15) == 0 && base + kEmaChunk <= t.n) {
#pragma unroll 2
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + (j * 256 + threadIdx.x) * 4;
      f32x4 p = *reinterpret_cast<const f32x4*>(t.p + i), g = *reinterpret_cast<const f32x4*>(t.g + i);
      f32x4 m = *reinterpret_cast<const f32x4*>(t.m + i), v = *reinterpret_cast<const f32x4*>(t.v + i);
      if (t.g2) {
        const f32x4 g2 = *reinterpret_cast<const f32x4*>(t.g2 + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = g2[e] + g[e];
      }
      if (CTL) {
        if (clip) {
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = g[e] * coef;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_element(pe, g[e], me, ve, wd, neg_step, bc2_sqrt, s, small_w);
        p[e] = pe, m[e] = me, v[e] = ve;
      }
      *reinterpret_cast<f32x4*>(t.m + i) = m;
      *reinterpret_cast<f32x4*>(t.v + i) = v;
      *reinterpret_cast<f32x4*>(t.p + i) = p;
    }
    return;
  }
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < t.n) {
      float p = t.p[i], g = t.g[i], m = t.m[i], v = t.v[i];
      if (t.g2) g = t.g2[i] + g;
      if (CTL) {
        if (clip) g = g * coef;
      }
      adam_element(p, g, m, v, wd, neg_step, bc2_sqrt, s, small_w);
      t.m[i] = m;
      t.v[i] = v;
      t.p[i] = p;
    }
  }
}

// ---- ||g2 + g||_2 over every tensor of an optimiser table, and the control block the CTL update kernels read ---------
// One double partial per (tensor, chunk) of the update kernels' own tables (rows of `row_bytes`: g at byte 8, g2 at 16, n at
// `n_off`), no atomics; grad_norm_finish adds the partials in a fixed order: the same inputs give the same bits.  d = g2 + g is
// the fp32 sum the update applies (AccumulateGrad's operand order); d*d is exact in double.  Thread t owns elements
// (j*256 + t)*4 + e of the chunk on BOTH paths -- one dwordx4 load per j where the chunk is whole and both pointers are
// 16-byte aligned, four guarded scalar loads otherwise -- and adds them in the same order, so the norm does not depend on
// where a gradient happens to lie (a view into a flat reduction buffer may sit at any 4-byte offset).
__global__ __launch_bounds__(256) void grad_sq_chunks(const char* __restrict__ rows, int row_bytes, int n_off,
                                                      const int2* __restrict__ chunks, double* __restrict__ sq_chunk) {
  const int2 ch = chunks[blockIdx.x];
  const char* row = rows + (size_t)ch.x * row_bytes;
  const float* g = *reinterpret_cast<const float* const*>(row + 8);
  const float* g2 = *reinterpret_cast<const float* const*>(row + 16);
  const int64_t n = *reinterpret_cast<const int64_t*>(row + n_off);
  const int64_t base = (int64_t)ch.y * kEmaChunk;
  double acc = 0;
  if ((((uintptr_t)g | (uintptr_t)g2) & 15) == 0 && base + kEmaChunk <= n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + (j * 256 + threadIdx.x) * 4;
      f32x4 d = *reinterpret_cast<const f32x4*>(g + i);
      if (g2) {
        const f32x4 d2 = *reinterpret_cast<const f32x4*>(g2 + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = d2[e] + d[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)d[e] * (double)d[e];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = base + (j * 256 + threadIdx.x) * 4 + e;
        if (i < n) {
          float d = g[i];
          if (g2) d = g2[i] + d;
          acc += (double)d * (double)d;
        }
      }
    }
  }
  __shared__ double red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) sq_chunk[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);      // one partial per chunk: no atomics
}

// total, coef and the skip flag from the chunk partials; in fp32 from the square root on, as torch.nn.utils.clip_grad_norm_
// computes them.  A NaN norm gives a NaN coef (torch.clamp keeps NaN; fminf would not).  One block, fixed summation order.
__global__ __launch_bounds__(256) void grad_norm_finish(const double* __restrict__ sq_chunk, int n_chunks, float max_norm,
                                                        GradCtl* __restrict__ ctl, int64_t* __restrict__ skipped) {
  double s = 0;
  for (int i = threadIdx.x; i < n_chunks; i += 256) s += sq_chunk[i];
  __shared__ double red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
    float coef = 1.f;
    if (max_norm > 0.f) {
      const float c = max_norm / (total + 1e-6f);
      coef = c > 1.f ? 1.f : c;
    }
    const int skip = isfinite(total) ? 0 : 1;
    ctl->total = total;
    ctl->coef = coef;
    ctl->skip = skip;
    ctl->reserved = 0;
    if (skipped) *skipped += skip;
  }
}

// ---- per-tensor gradient health table: one more multi-tensor pass over the update's own table ---------
// Columns of a row (fp64; counts and indices are exact integers below 2^53), d = g2 + g as in grad_sq_chunks:
//   0 g_sumsq            sum d^2 over FINITE d              4 g_zeros   number of d == 0 (either sign)
//   1 g_maxabs           max |d| over finite d, 0 if none   5 p_sumsq   sum p^2 plainly (Inf / NaN show)
//   2 g_nonfinite        number of d that are Inf or NaN    6 p_maxabs  max |p| over finite p
//   3 g_first_nonfinite  1 + flat index of the first, or 0  7 s_sumsq   sum state^2 plainly, 0 without a state
constexpr int kStatCols = 8;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// elements i .. i+3 of a tensor of n: one dwordx4 load where `vec` (whole chunk, 16-byte aligned pointer), four guarded scalar
// loads otherwise (0 beyond the end)
__device__ __forceinline__ f32x4 chunk_load4(const float* __restrict__ x, int64_t i, int64_t n, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = i + e < n ? x[i + e] : 0.f;
  return v;
}

// One partial row per (tensor, chunk), no atomics.  Rows as grad_sq_chunks reads them, plus p at byte 0 and the state pointer
// (momentum_buffer / exp_avg) at byte 24; either may be null: zeros in its columns.  first_bit (the SGD table): bit 32 of `group`
// (the 8 bytes after n) marks a tensor that takes its first step -- its momentum buffer is uninitialised memory and is NOT read.
// Thread t owns elements (j*256 + t)*4 + e on the vector and on the scalar path, each input takes the path its own pointer
// allows, and the per-thread sums run in the same order on both: the table does not depend on where a tensor lies.
__global__ __launch_bounds__(256) void tensor_stats_chunks(const char* __restrict__ rows, int row_bytes, int n_off, int first_bit,
                                                           const int2* __restrict__ chunks, double* __restrict__ partial) {
  const int2 ch = chunks[blockIdx.x];
  const char* row = rows + (size_t)ch.x * row_bytes;
  const float* p = *reinterpret_cast<const float* const*>(row);
  const float* g = *reinterpret_cast<const float* const*>(row + 8);
  const float* g2 = *reinterpret_cast<const float* const*>(row + 16);
  const float* st = *reinterpret_cast<const float* const*>(row + 24);
  const int64_t n = *reinterpret_cast<const int64_t*>(row + n_off);
  if (first_bit && ((*reinterpret_cast<const int64_t*>(row + n_off + 8) >> 32) & 1)) st = nullptr;
  const int64_t base = (int64_t)ch.y * kEmaChunk;
  const bool whole = base + kEmaChunk <= n;
  const bool vec_g = whole && (((uintptr_t)g | (uintptr_t)g2) & 15) == 0;
  const bool vec_p = whole && ((uintptr_t)p & 15) == 0, vec_s = whole && ((uintptr_t)st & 15) == 0;
  double g_sq = 0, p_sq = 0, s_sq = 0;
  float g_max = 0.f, p_max = 0.f;
  int nonfinite = 0, zeros = 0, first = kEmaChunk;      // first: offset inside the chunk, kEmaChunk = none
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int off = (j * 256 + threadIdx.x) * 4;
    const int64_t i = base + off;
    f32x4 d = chunk_load4(g, i, n, vec_g);
    if (g2) {
      const f32x4 d2 = chunk_load4(g2, i, n, vec_g);
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = d2[e] + d[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (whole || i + e < n) {
        if (isfinite(d[e])) {
          g_sq += (double)d[e] * (double)d[e];
          g_max = fmaxf(g_max, fabsf(d[e]));
          zeros += d[e] == 0.f;
        } else {
          ++nonfinite;
          first = min(first, off + e);
        }
      }
    }
    if (p) {      // elements beyond the end load as 0: nothing to guard
      const f32x4 v = chunk_load4(p, i, n, vec_p);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p_sq += (double)v[e] * (double)v[e];
        if (isfinite(v[e])) p_max = fmaxf(p_max, fabsf(v[e]));
      }
    }
    if (st) {
      const f32x4 v = chunk_load4(st, i, n, vec_s);
#pragma unroll
      for (int e = 0; e < 4; ++e) s_sq += (double)v[e] * (double)v[e];
    }
  }
  __shared__ double red[4][kStatCols];
  g_sq = wave_sum(g_sq), p_sq = wave_sum(p_sq), s_sq = wave_sum(s_sq);
  const double nf = wave_sum((double)nonfinite), zr = wave_sum((double)zeros);
  g_max = wave_max(g_max), p_max = wave_max(p_max);
  const double fi = wave_min((double)first);
  if ((threadIdx.x & 63) == 0) {
    double* r = red[threadIdx.x >> 6];
    r[0] = g_sq, r[1] = g_max, r[2] = nf, r[3] = fi, r[4] = zr, r[5] = p_sq, r[6] = p_max, r[7] = s_sq;
  }
  __syncthreads();
  if (threadIdx.x < kStatCols) {      // one column per thread, the four waves in a fixed order
    const int c = threadIdx.x;
    const double a = red[0][c], b = red[1][c], e = red[2][c], f = red[3][c];
    double v;
    if (c == 1 || c == 6) v = fmax(fmax(a, b), fmax(e, f));
    else if (c == 3) {
      v = fmin(fmin(a, b), fmin(e, f));
      v = v < (double)kEmaChunk ? (double)base + v + 1.0 : 0.0;
    } else v = (a + b) + (e + f);
    partial[(size_t)blockIdx.x * kStatCols + c] = v;
  }
}

// One block (one wave) per OUTPUT row.  row_of[r] = the row's tensor in this step's table, or -1: eight zeros.  `chunks` is
// ordered by tensor, so a tensor's partials are one contiguous run (binary search over chunks[].x); lane l combines chunks
// l, l + 64, ... of the run in ascending order and the lanes meet in the usual butterfly: a fixed order, the same bits every run.
// ctl non-null and ctl->skip set: the row also goes to `captured`, and block 0 notes *skipped -- which grad_norm_finish has just
// incremented on the same stream -- in captured_at.
__global__ __launch_bounds__(64) void tensor_stats_finish(const int2* __restrict__ chunks, int n_chunks, int n_tensors,
                                                          const int32_t* __restrict__ row_of, const double* __restrict__ partial,
                                                          double* __restrict__ table, const GradCtl* __restrict__ ctl,
                                                          double* __restrict__ captured, int64_t* __restrict__ captured_at,
                                                          const int64_t* __restrict__ skipped) {
  const int t = row_of[blockIdx.x];
  double sum[5] = {0, 0, 0, 0, 0}, g_max = 0, p_max = 0, first = 0x1p62;      // sums: columns 0, 2, 4, 5, 7
  if (t >= 0 && t < n_tensors) {
    int lo = 0, hi = n_chunks;                       // first chunk whose tensor id is >= t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (chunks[mid].x < t) lo = mid + 1; else hi = mid;
    }
    for (int i = lo + threadIdx.x; i < n_chunks && chunks[i].x == t; i += 64) {
      const double* r = partial + (size_t)i * kStatCols;
      sum[0] += r[0], sum[1] += r[2], sum[2] += r[4], sum[3] += r[5], sum[4] += r[7];
      g_max = fmax(g_max, r[1]), p_max = fmax(p_max, r[6]);
      if (r[3] > 0) first = fmin(first, r[3]);
    }
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) sum[c] = wave_sum(sum[c]);
  g_max = wave_max(g_max), p_max = wave_max(p_max), first = wave_min(first);
  if (threadIdx.x == 0) {
    const double out[kStatCols] = {sum[0], g_max, sum[1], first < 0x1p62 ? first : 0.0, sum[2], sum[3], p_max, sum[4]};
    const bool capture = ctl && ctl->skip;
#pragma unroll
    for (int c = 0; c < kStatCols; ++c) {
      table[(size_t)blockIdx.x * kStatCols + c] = out[c];
      if (capture) captured[(size_t)blockIdx.x * kStatCols + c] = out[c];
    }
    if (capture && blockIdx.x == 0) *captured_at = *skipped;
  }
}

// y[n,c,:] = x[n,c,:] * m[n,c]   (Dropout2d with an explicit keep/(1-p) mask, fcn.py:52,56)
__global__ __launch_bounds__(256) void scale_planes(const float* __restrict__ x, const float* __restrict__ m, int HW,
                                                    float* __restrict__ y, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    y[i] = x[i] * m[i / HW];
}

// out = a + b (gradient joins); c = a*alpha elementwise helpers
__global__ __launch_bounds__(256) void add2(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                            int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = a[i] + b[i];
}

__global__ __launch_bounds__(256) void relu_mask(const float* __restrict__ dy, const float* __restrict__ y,
                                                 float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                             const float* conv_bias, float eps, int C, float* scale, float* shift, float* invstd,
                             dasac_stream_t stream) {
  DASAC_REQUIRE(gamma && beta && mean && var && scale && shift && C > 0, "bn_fold: bad arguments");
  hipLaunchKernelGGL(bn_fold, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), gamma, beta, mean, var, conv_bias, eps, C,
                     scale, shift, invstd);
  DASAC_CHECK_LAUNCH("bn_fold");
  return DASAC_OK;
}

extern "C" int dasac_bn_fold_multi(const dasac_fold_job* jobs, const int32_t* chunks, int n_chunks, dasac_stream_t stream) {
  DASAC_REQUIRE(jobs && chunks && n_chunks > 0, "bn_fold_multi: bad arguments");
  DASAC_REQUIRE((((uintptr_t)jobs | (uintptr_t)chunks) & 7) == 0, "bn_fold_multi: misaligned job table / chunk list");
  hipLaunchKernelGGL(bn_fold_multi, dim3(n_chunks), dim3(256), 0, as_stream(stream), jobs, reinterpret_cast<const int2*>(chunks));
  DASAC_CHECK_LAUNCH("bn_fold_multi");
  return DASAC_OK;
}

extern "C" int dasac_bn_param_grads(const float* dot, int dot_rows, const float* sum_dz, const float* mean, const float* invstd,
                                    const float* scale, const float* conv_bias, int C, float* dgamma, float* dbeta,
                                    float* dbias, dasac_stream_t stream) {
  DASAC_REQUIRE(sum_dz && C > 0 && (!dgamma || (dot && dot_rows > 0 && mean && invstd)), "bn_param_grads: bad arguments");
  hipLaunchKernelGGL(bn_param_grads, dim3((C + 63) / 64), dim3(64), 0, as_stream(stream), dot, dot_rows, sum_dz, mean, invstd, scale,
                     conv_bias, C, dgamma, dbeta, dbias);
  DASAC_CHECK_LAUNCH("bn_param_grads");
  return DASAC_OK;
}

extern "C" int dasac_channel_sums(const float* x, int N, int C, int64_t HW, float* out, dasac_stream_t stream) {
  DASAC_REQUIRE(x && out && N > 0 && C > 0 && HW > 0 && HW < (1ll << 31), "channel_sums: bad arguments");
  hipLaunchKernelGGL(channel_sums, dim3(C), dim3(256), 0, as_stream(stream), x, N, C, (int)HW, out);
  DASAC_CHECK_LAUNCH("channel_sums");
  return DASAC_OK;
}

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

extern "C" int dasac_ema_chunk_elems(void) { return kEmaChunk; }

// pairs: device array of {fast*, slow*, int64 n} (24 bytes each); chunks: device array of int32 pairs
// (tensor id, chunk index within the tensor), SORTED by tensor id; sq: device [n_tensors + n_chunks] doubles (scratch: per-tensor
// sums, then one partial per chunk -- summed in a fixed order, so teacher_diff is bit-identical from run to run); out: device [1].
extern "C" int dasac_ema_update(const void* pairs, int n_tensors, const int32_t* chunks, int n_chunks, double momentum,
                                int update, double* sq, float* out, dasac_stream_t stream) {
  DASAC_REQUIRE(pairs && chunks && sq && out && n_tensors > 0 && n_chunks > 0, "ema_update: bad arguments");
  DASAC_REQUIRE((((uintptr_t)pairs | (uintptr_t)chunks | (uintptr_t)sq) & 7) == 0, "ema_update: misaligned pair table / chunk list / sq");
  hipStream_t s = as_stream(stream);
  double* sq_chunk = sq + n_tensors;
  // sac.py:95 multiplies by the python double (1. - momentum) cast to fp32: the difference is taken from the DOUBLE momentum
  // (1 - fl32(0.99) is 0.0099999905, fl32(1 - 0.99) is 0.01), so the momentum arrives as a double and both factors round once
  const float one_minus = (float)(1.0 - momentum);
  hipLaunchKernelGGL(ema_chunks, dim3(n_chunks), dim3(256), 0, s, reinterpret_cast<const TensorPair*>(pairs),
                     reinterpret_cast<const int2*>(chunks), (float)momentum, one_minus, update, sq_chunk);
  DASAC_CHECK_LAUNCH("ema_chunks");
  hipLaunchKernelGGL(ema_tensor_sums, dim3(n_tensors), dim3(64), 0, s, reinterpret_cast<const int2*>(chunks), n_chunks, sq_chunk, sq);
  DASAC_CHECK_LAUNCH("ema_tensor_sums");
  hipLaunchKernelGGL(ema_finish, dim3(1), dim3(64), 0, s, sq, n_tensors, out);
  DASAC_CHECK_LAUNCH("ema_finish");
  return DASAC_OK;
}

// the 64-bit row tables and the int2 chunk lists of the multi-tensor kernels: 8-byte aligned (include/dasac_hip.h)
static bool rows_aligned(const void* tensors, const void* chunks) { return (((uintptr_t)tensors | (uintptr_t)chunks) & 7) == 0; }

static SgdGroups sgd_groups(const float* group_lr, const float* group_wd, int n_groups) {
  SgdGroups hp;
  for (int i = 0; i < 8; ++i) {
    hp.lr[i] = i < n_groups ? group_lr[i] : 0.f;
    hp.wd[i] = i < n_groups ? group_wd[i] : 0.f;
  }
  return hp;
}

template <bool NESTEROV, bool CTL>
static int launch_sgd(const void* tensors, const int32_t* chunks, int n_chunks, const SgdGroups& hp, float momentum, int first,
                      const void* ctl, int flags, dasac_stream_t stream) {
  hipLaunchKernelGGL((sgd_chunks<NESTEROV, CTL>), dim3(n_chunks), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const SgdTensor*>(tensors), reinterpret_cast<const int2*>(chunks), hp, momentum, first,
                     reinterpret_cast<const GradCtl*>(ctl), flags);
  DASAC_CHECK_LAUNCH("sgd_chunks");
  return DASAC_OK;
}

extern "C" int dasac_sgd_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_lr,
                              const float* group_wd, int n_groups, float momentum, int first, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_lr && group_wd && n_tensors > 0 && n_chunks > 0, "sgd_step: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "sgd_step: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "sgd_step: 1..8 parameter groups");
  return launch_sgd<false, false>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, nullptr, 0, stream);
}

extern "C" int dasac_sgd_nesterov_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                       const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                                       dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_lr && group_wd && n_tensors > 0 && n_chunks > 0, "sgd_nesterov_step: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "sgd_nesterov_step: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "sgd_nesterov_step: 1..8 parameter groups");
  DASAC_REQUIRE(momentum > 0.f, "sgd_nesterov_step: Nesterov momentum requires a momentum");
  return launch_sgd<true, false>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, nullptr, 0, stream);
}

static bool ctl_args_ok(const void* ctl, int apply_coef, int honour_skip) {
  return ctl && ((uintptr_t)ctl & 15) == 0 && (apply_coef == 0 || apply_coef == 1) && (honour_skip == 0 || honour_skip == 1);
}

extern "C" int dasac_sgd_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_lr,
                                  const float* group_wd, int n_groups, float momentum, int first, const void* ctl, int apply_coef,
                                  int honour_skip, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_lr && group_wd && n_tensors > 0 && n_chunks > 0, "sgd_step_ctl: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "sgd_step_ctl: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "sgd_step_ctl: 1..8 parameter groups");
  DASAC_REQUIRE(first >= -1 && first <= 1, "sgd_step_ctl: first is 0, 1 or -1 (per row)");
  DASAC_REQUIRE(ctl_args_ok(ctl, apply_coef, honour_skip), "sgd_step_ctl: a 16-byte aligned control block and 0/1 flags");
  return launch_sgd<false, true>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, ctl,
                                 apply_coef * kCtlClip + honour_skip * kCtlSkip, stream);
}

extern "C" int dasac_sgd_nesterov_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                           const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                                           const void* ctl, int apply_coef, int honour_skip, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_lr && group_wd && n_tensors > 0 && n_chunks > 0, "sgd_nesterov_step_ctl: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "sgd_nesterov_step_ctl: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "sgd_nesterov_step_ctl: 1..8 parameter groups");
  DASAC_REQUIRE(momentum > 0.f, "sgd_nesterov_step_ctl: Nesterov momentum requires a momentum");
  DASAC_REQUIRE(first >= -1 && first <= 1, "sgd_nesterov_step_ctl: first is 0, 1 or -1 (per row)");
  DASAC_REQUIRE(ctl_args_ok(ctl, apply_coef, honour_skip), "sgd_nesterov_step_ctl: a 16-byte aligned control block and 0/1 flags");
  return launch_sgd<true, true>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, ctl,
                                apply_coef * kCtlClip + honour_skip * kCtlSkip, stream);
}

template <bool CTL>
static int launch_adam(const void* tensors, const int32_t* chunks, int n_chunks, const float* group_wd, int n_groups, double beta1,
                       double beta2, double eps, const void* ctl, int flags, dasac_stream_t stream) {
  AdamGroups hp;
  for (int i = 0; i < 8; ++i) hp.wd[i] = i < n_groups ? group_wd[i] : 0.f;
  // adam.py:706,720 form 1 - beta in python doubles; the foreach functors then round each scalar to fp32 once
  AdamScalars s;
  s.w1 = (float)(1.0 - beta1);
  s.one_minus_w1 = 1.f - s.w1;                  // Lerp.h:34, opmath_t(1) - weight
  s.beta2 = (float)beta2;
  s.w2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  hipLaunchKernelGGL(adam_chunks<CTL>, dim3(n_chunks), dim3(256), 0, as_stream(stream), reinterpret_cast<const AdamTensor*>(tensors),
                     reinterpret_cast<const int2*>(chunks), hp, s, reinterpret_cast<const GradCtl*>(ctl), flags);
  DASAC_CHECK_LAUNCH("adam_chunks");
  return DASAC_OK;
}

extern "C" int dasac_adam_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_wd,
                               int n_groups, double beta1, double beta2, double eps, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_wd && n_tensors > 0 && n_chunks > 0, "adam_step: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "adam_step: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "adam_step: 1..8 parameter groups");
  DASAC_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "adam_step: betas in [0, 1), eps >= 0");
  return launch_adam<false>(tensors, chunks, n_chunks, group_wd, n_groups, beta1, beta2, eps, nullptr, 0, stream);
}

extern "C" int dasac_adam_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_wd,
                                   int n_groups, double beta1, double beta2, double eps, const void* ctl, int apply_coef,
                                   int honour_skip, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && group_wd && n_tensors > 0 && n_chunks > 0, "adam_step_ctl: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "adam_step_ctl: misaligned row table / chunk list");
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "adam_step_ctl: 1..8 parameter groups");
  DASAC_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "adam_step_ctl: betas in [0, 1), eps >= 0");
  DASAC_REQUIRE(ctl_args_ok(ctl, apply_coef, honour_skip), "adam_step_ctl: a 16-byte aligned control block and 0/1 flags");
  return launch_adam<true>(tensors, chunks, n_chunks, group_wd, n_groups, beta1, beta2, eps, ctl,
                           apply_coef * kCtlClip + honour_skip * kCtlSkip, stream);
}

extern "C" size_t dasac_grad_norm_workspace(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(double) : 0; }

extern "C" int dasac_grad_norm(const void* tensors, int row_bytes, int n_tensors, const int32_t* chunks, int n_chunks, float max_norm,
                               void* workspace, size_t workspace_bytes, void* ctl, int64_t* skipped, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && workspace && ctl && n_tensors > 0 && n_chunks > 0, "grad_norm: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "grad_norm: misaligned row table / chunk list");
  DASAC_REQUIRE(row_bytes == (int)sizeof(SgdTensor) || row_bytes == (int)sizeof(AdamTensor),
                "grad_norm: row_bytes names the table, 48 (dasac_sgd_step) or 64 (dasac_adam_step)");
  DASAC_REQUIRE(workspace_bytes >= dasac_grad_norm_workspace(n_chunks) && ((uintptr_t)workspace & 7) == 0, "grad_norm: workspace too small");
  DASAC_REQUIRE(((uintptr_t)ctl & 15) == 0 && ((uintptr_t)skipped & 7) == 0, "grad_norm: misaligned control block / counter");
  DASAC_REQUIRE(max_norm == max_norm && max_norm <= 3.4028234664e38f, "grad_norm: max_norm is a finite number (<= 0: measure only)");
  hipStream_t s = as_stream(stream);
  const int n_off = row_bytes == (int)sizeof(SgdTensor) ? (int)offsetof(SgdTensor, n) : (int)offsetof(AdamTensor, n);
  static_assert(offsetof(SgdTensor, g) == 8 && offsetof(SgdTensor, g2) == 16 && offsetof(AdamTensor, g) == 8 && offsetof(AdamTensor, g2) == 16,
                "grad_sq_chunks reads g and g2 at bytes 8 and 16 of either row");
  double* sq_chunk = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(grad_sq_chunks, dim3(n_chunks), dim3(256), 0, s, reinterpret_cast<const char*>(tensors), row_bytes, n_off,
                     reinterpret_cast<const int2*>(chunks), sq_chunk);
  DASAC_CHECK_LAUNCH("grad_sq_chunks");
  hipLaunchKernelGGL(grad_norm_finish, dim3(1), dim3(256), 0, s, sq_chunk, n_chunks, max_norm, reinterpret_cast<GradCtl*>(ctl), skipped);
  DASAC_CHECK_LAUNCH("grad_norm_finish");
  return DASAC_OK;
}

extern "C" size_t dasac_tensor_stats_workspace(int n_chunks) {
  return n_chunks > 0 ? (size_t)n_chunks * kStatCols * sizeof(double) : 0;
}

extern "C" int dasac_tensor_stats(const void* tensors, int row_bytes, int n_tensors, const int32_t* chunks, int n_chunks,
                                  const int32_t* row_of, int n_rows, void* workspace, size_t workspace_bytes, double* table,
                                  const void* ctl, double* captured, int64_t* captured_at, const int64_t* skipped,
                                  dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && row_of && workspace && table && n_tensors > 0 && n_chunks > 0 && n_rows > 0,
                "tensor_stats: bad arguments");
  DASAC_REQUIRE(row_bytes == (int)sizeof(SgdTensor) || row_bytes == (int)sizeof(AdamTensor),
                "tensor_stats: row_bytes names the table, 48 (dasac_sgd_step) or 64 (dasac_adam_step)");
  DASAC_REQUIRE(((uintptr_t)tensors & 7) == 0 && ((uintptr_t)chunks & 7) == 0 && ((uintptr_t)row_of & 3) == 0 &&
                    ((uintptr_t)table & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                "tensor_stats: misaligned table / chunks / row_of / workspace");
  DASAC_REQUIRE(workspace_bytes >= dasac_tensor_stats_workspace(n_chunks), "tensor_stats: workspace too small");
  const int given = (ctl != nullptr) + (captured != nullptr) + (captured_at != nullptr) + (skipped != nullptr);
  DASAC_REQUIRE(given == 0 || given == 4, "tensor_stats: ctl, captured, captured_at and skipped are all null or all given");
  DASAC_REQUIRE(((uintptr_t)ctl & 15) == 0 && ((uintptr_t)captured & 7) == 0 && ((uintptr_t)captured_at & 7) == 0 &&
                    ((uintptr_t)skipped & 7) == 0,
                "tensor_stats: misaligned control block / captured table / counters");
  hipStream_t s = as_stream(stream);
  const bool sgd = row_bytes == (int)sizeof(SgdTensor);
  const int n_off = sgd ? (int)offsetof(SgdTensor, n) : (int)offsetof(AdamTensor, n);
  static_assert(offsetof(SgdTensor, p) == 0 && offsetof(AdamTensor, p) == 0 && offsetof(SgdTensor, buf) == 24 && offsetof(AdamTensor, m) == 24 &&
                    offsetof(SgdTensor, group) == offsetof(SgdTensor, n) + 8 && offsetof(AdamTensor, group) == offsetof(AdamTensor, n) + 8,
                "tensor_stats_chunks reads p at byte 0, the state pointer at 24 and `group` right after n in either row");
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(tensor_stats_chunks, dim3(n_chunks), dim3(256), 0, s, reinterpret_cast<const char*>(tensors), row_bytes, n_off,
                     sgd ? 1 : 0, reinterpret_cast<const int2*>(chunks), partial);
  DASAC_CHECK_LAUNCH("tensor_stats_chunks");
  hipLaunchKernelGGL(tensor_stats_finish, dim3(n_rows), dim3(64), 0, s, reinterpret_cast<const int2*>(chunks), n_chunks, n_tensors, row_of,
                     partial, table, reinterpret_cast<const GradCtl*>(ctl), captured, captured_at, skipped);
  DASAC_CHECK_LAUNCH("tensor_stats_finish");
  return DASAC_OK;
}

extern "C" int dasac_scale_planes(const float* x, const float* plane_scale, int64_t planes, int64_t HW, float* y,
                                  dasac_stream_t stream) {
  DASAC_REQUIRE(x && plane_scale && y && planes > 0 && HW > 0, "scale_planes: bad arguments");
  const int64_t total = planes * HW;
  hipLaunchKernelGGL(scale_planes, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(stream), x, plane_scale, (int)HW, y, total);
  DASAC_CHECK_LAUNCH("scale_planes");
  return DASAC_OK;
}

extern "C" int dasac_add(const float* a, const float* b, float* out, int64_t n, dasac_stream_t stream) {
  DASAC_REQUIRE(a && b && out && n > 0, "add: bad arguments");
  hipLaunchKernelGGL(add2, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), a, b, out, n);
  DASAC_CHECK_LAUNCH("add");
  return DASAC_OK;
}

extern "C" int dasac_relu_mask(const float* dy, const float* y, float* out, int64_t n, dasac_stream_t stream) {
  DASAC_REQUIRE(dy && y && out && n > 0, "relu_mask: bad arguments");
  hipLaunchKernelGGL(relu_mask, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), dy, y, out, n);
  DASAC_CHECK_LAUNCH("relu_mask");
  return DASAC_OK;
}

// ------------------------------------------------------------------------------------------------
// Train-mode BatchNorm (baseline / AdaBN mode: models/__init__.py:29 leaves BN un-frozen, every
// nn.SyncBatchNorm of deeplabv2.py:15 / fcn.py:8 normalises with batch statistics; train.py:281-289
// re-estimates the running statistics on target crops).  Cross-rank statistics (SyncBN) are summed by
// the caller with one RCCL all-reduce of the raw (sum, sum of squares) / (sum dy, sum dy*xhat) vectors.
// ------------------------------------------------------------------------------------------------
namespace dasac {

constexpr int kBnChunk = 256 * 16;

// Two-stage, atomic-free (deterministic) per-channel reductions: stage 1 writes one (s, q) pair of doubles per (plane, chunk),
// stage 2 (bn_sums_finish, one wave per channel) adds the N*chunks pairs of a channel in a fixed order.
// partial[(plane*chunks + chunk)*2 + {0,1}] = sum z, sum z^2 of the chunk        (grid = (chunks, N*C planes))
__global__ __launch_bounds__(256) void bn_stats(const float* __restrict__ z, int C, int HW, double* __restrict__ partial) {
  const int plane = blockIdx.y;
  const float* p = z + (size_t)plane * HW;
  double s = 0, q = 0;
  const int hi = min(HW, (int)(blockIdx.x + 1) * kBnChunk);
  for (int i = blockIdx.x * kBnChunk + threadIdx.x * 4; i < hi; i += 256 * 4) {      // 16-byte loads (4-byte aligned planes)
    if (i + 4 <= hi) {
      const f32x4u v4 = *reinterpret_cast<const f32x4u*>(p + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double v = v4[e];
        s += v;
        q += v * v;
      }
    } else {
      for (int e = i; e < hi; ++e) {
        const double v = p[e];
        s += v;
        q += v * v;
      }
    }
  }
  __shared__ double rs[4], rq[4];
  s = wave_sum(s);
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)plane * gridDim.x + blockIdx.x) * 2;
    o[0] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
    o[1] = (rq[0] + rq[1]) + (rq[2] + rq[3]);
  }
}

// sums[c] = sum over (n, chunk) of the s-partials, sums[C + c] = of the q-partials; grid C, one wave each
__global__ __launch_bounds__(64) void bn_sums_finish(const double* __restrict__ partial, int N, int C, int chunks,
                                                     double* __restrict__ sums, float* __restrict__ out0,
                                                     float* __restrict__ out1) {
  const int c = blockIdx.x;
  double s = 0, q = 0;
  for (int j = threadIdx.x; j < N * chunks; j += 64) {
    const int n = j / chunks, k = j - n * chunks;
    const double* o = partial + ((size_t)(n * C + c) * chunks + k) * 2;
    s += o[0];
    q += o[1];
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if (threadIdx.x == 0) {
    sums[c] = s;
    sums[C + c] = q;
    if (out0) out0[c] = (float)s;       // backward: d beta = sum dy, d gamma = sum dy*xhat of THIS rank (no extra launch)
    if (out1) out1[c] = (float)q;
  }
}

// per-tile channel statistics left by dasac_conv_gemm_stats -> sums[c], sums[C + c] (doubles): a thread per channel adds the
// tiles in ascending order (coalesced across the channels of a block; fixed order = deterministic)
__global__ __launch_bounds__(64) void bn_tile_stats_reduce(const float* __restrict__ ts, int n_tiles, int C, int Mpad,
                                                           double* __restrict__ sums) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double s = 0, q = 0;
#pragma unroll 4
  for (int i = 0; i < n_tiles; ++i) {
    s += (double)ts[(size_t)(2 * i) * Mpad + c];
    q += (double)ts[(size_t)(2 * i + 1) * Mpad + c];
  }
  sums[c] = s;
  sums[C + c] = q;
}

// batch mean / biased var -> scale, shift, mean, invstd; running stats: momentum update with the unbiased var
// `sums` null: the sums come from `tile_stats` (dasac_conv_gemm_stats), added here in tile order -- one launch per BN layer
__global__ void bn_train_finalize(const double* __restrict__ sums, const float* __restrict__ tile_stats, int n_tiles, int Mpad,
                                  double count_host, const double* __restrict__ count_dev,
                                  const float* __restrict__ gamma,
                                  const float* __restrict__ beta, float* __restrict__ running_mean,
                                  float* __restrict__ running_var, int64_t* __restrict__ num_batches_tracked, float momentum,
                                  float eps, int C,
                                  float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_out,
                                  float* __restrict__ invstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && num_batches_tracked) num_batches_tracked[0] += 1;      // nn.BatchNorm bookkeeping, no extra launch
  if (c >= C) return;
  const double count = count_dev ? count_dev[0] : count_host;   // SyncBN: the all-reduced count stays on the device
  double s1, s2;
  if (sums) {
    s1 = sums[c];
    s2 = sums[C + c];
  } else {
    s1 = s2 = 0;
#pragma unroll 4
    for (int i = 0; i < n_tiles; ++i) {
      s1 += (double)tile_stats[(size_t)(2 * i) * Mpad + c];
      s2 += (double)tile_stats[(size_t)(2 * i + 1) * Mpad + c];
    }
  }
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0) var = 0;
  const float meanf = (float)m, varf = (float)var;
  const float is = 1.f / sqrtf(varf + eps);
  const float a = gamma[c] * is;
  scale[c] = a;
  shift[c] = beta[c] - meanf * a;
  mean_out[c] = meanf;
  invstd_out[c] = is;
  if (running_mean) {
    const float unbiased = count > 1 ? (float)(var * count / (count - 1)) : varf;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// y = relu?(z*scale[c] + shift[c] (+res))
__global__ __launch_bounds__(256) void bn_apply(const float* __restrict__ z, const float* __restrict__ scale,
                                                const float* __restrict__ shift, const float* __restrict__ res, int relu,
                                                int C, int HW, float* __restrict__ y, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i / HW) % C);
    float v = z[i] * scale[c] + shift[c];
    if (res) v += res[i];
    if (relu) v = fmaxf(v, 0.f);
    y[i] = v;
  }
}

// One rank (no all-reduce between statistics and normalisation): finalize + apply in ONE launch.  A block owns a 16K-element chunk
// of one (n, c) plane; it first adds its channel's tile statistics (dasac_conv_gemm_stats) -- 256 threads stride over the tiles,
// wave butterflies, the four wave sums added in a fixed order: every block of a channel gets the same bits -- derives scale /
// shift exactly as bn_train_finalize does, normalises its chunk with 16-byte accesses; the block of (n = 0, chunk 0) also writes
// mean / invstd (for the backward pass) and moves the running statistics.  Saves a 5 us launch per BN layer and pass.
constexpr int kBnBig = 256 * 64;
__global__ __launch_bounds__(256) void bn_apply_tiles(const float* __restrict__ z, const float* __restrict__ ts, int n_tiles, int Mpad,
                                                      double count, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ running_mean, float* __restrict__ running_var,
                                                      int64_t* __restrict__ num_batches_tracked, float momentum, float eps,
                                                      const float* __restrict__ res, int relu, int C, int HW,
                                                      float* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ invstd_out) {
  const int plane = blockIdx.y, c = plane % C, n = plane / C;
  double s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < n_tiles; i += 256) {
    s1 += (double)ts[(size_t)(2 * i) * Mpad + c];
    s2 += (double)ts[(size_t)(2 * i + 1) * Mpad + c];
  }
  __shared__ double r1[4], r2[4];
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) {
    r1[threadIdx.x >> 6] = s1;
    r2[threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  s1 = (r1[0] + r1[1]) + (r1[2] + r1[3]);
  s2 = (r2[0] + r2[1]) + (r2[2] + r2[3]);
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0) var = 0;
  const float meanf = (float)m, varf = (float)var;
  const float is = 1.f / sqrtf(varf + eps);
  const float a = gamma[c] * is;
  const float sh = beta[c] - meanf * a;
  if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    mean_out[c] = meanf;
    invstd_out[c] = is;
    if (running_mean) {
      const float unbiased = count > 1 ? (float)(var * count / (count - 1)) : varf;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
    if (c == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
  }
  const size_t pb = (size_t)plane * HW;
  const int lo = blockIdx.x * kBnBig, hi = min(HW, lo + kBnBig);
  for (int i = lo + threadIdx.x * 4; i < hi; i += 256 * 4) {
    if (i + 4 <= hi) {
      f32x4u v = *reinterpret_cast<const f32x4u*>(z + pb + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] * a + sh;
      if (res) {
        const f32x4u rv = *reinterpret_cast<const f32x4u*>(res + pb + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += rv[e];
      }
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      *reinterpret_cast<f32x4u*>(y + pb + i) = v;
    } else {
      for (int e = i; e < hi; ++e) {
        float v = z[pb + e] * a + sh;
        if (res) v += res[pb + e];
        if (relu) v = fmaxf(v, 0.f);
        y[pb + e] = v;
      }
    }
  }
}

// The backward twin: a block adds its channel's (plane, chunk) partial pairs of bn_bwd_reduce itself (N * chunks of them, fixed
// order, the same in every block), forms dz for a 16K-element chunk of one plane, and the block of (n = 0, chunk 0) writes
// d gamma / d beta -- no separate finish / parameter launches on one rank.
__global__ __launch_bounds__(256) void bn_bwd_apply_partials(const float* __restrict__ dy, const float* __restrict__ z,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const double* __restrict__ partial,
                                                             int N, int chunks_r, double count, int C, int HW,
                                                             float* __restrict__ dz, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  const int plane = blockIdx.y, c = plane % C, n = plane / C;
  // the channel's N * chunks partial pairs: strided over the block (independent loads) and folded by a fixed tree -- the same
  // order in every block and every run; round 4 had every thread walk all of them serially (75-300 dependent loads per block)
  __shared__ double red_s[256], red_q[256];
  double s = 0, q = 0;
  for (int j = threadIdx.x; j < N * chunks_r; j += 256) {
    const int nn = j / chunks_r, k = j - nn * chunks_r;
    const double* o = partial + ((size_t)(nn * C + c) * chunks_r + k) * 2;
    s += o[0];
    q += o[1];
  }
  red_s[threadIdx.x] = s;
  red_q[threadIdx.x] = q;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red_s[threadIdx.x] += red_s[threadIdx.x + o];
      red_q[threadIdx.x] += red_q[threadIdx.x + o];
    }
    __syncthreads();
  }
  s = red_s[0];
  q = red_q[0];
  if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
  }
  const float is = invstd[c], mu = mean[c];
  const float a = (float)(s / count), b = (float)(q / count), gi = gamma[c] * is;
  const size_t pb = (size_t)plane * HW;
  const int lo = blockIdx.x * kBnBig, hi = min(HW, lo + kBnBig);
  for (int i = lo + threadIdx.x * 4; i < hi; i += 256 * 4) {
    if (i + 4 <= hi) {
      const f32x4u d = *reinterpret_cast<const f32x4u*>(dy + pb + i), zz = *reinterpret_cast<const f32x4u*>(z + pb + i);
      f32x4u o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (zz[e] - mu) * is;
        o[e] = gi * (d[e] - a - xh * b);
      }
      *reinterpret_cast<f32x4u*>(dz + pb + i) = o;
    } else {
      for (int e = i; e < hi; ++e) {
        const float xh = (z[pb + e] - mu) * is;
        dz[pb + e] = gi * (dy[pb + e] - a - xh * b);
      }
    }
  }
}

// partial pairs (as bn_stats) of sum dy, sum dy * xhat,  xhat = (z - mean)*invstd
__global__ __launch_bounds__(256) void bn_bwd_reduce(const float* __restrict__ dy, const float* __restrict__ z,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd, int C,
                                                     int HW, double* __restrict__ partial) {
  const int plane = blockIdx.y, c = plane % C;
  const float* pd = dy + (size_t)plane * HW;
  const float* pz = z + (size_t)plane * HW;
  const float m = mean[c], is = invstd[c];
  double s = 0, q = 0;
  const int hi = min(HW, (int)(blockIdx.x + 1) * kBnChunk);
  for (int i = blockIdx.x * kBnChunk + threadIdx.x * 4; i < hi; i += 256 * 4) {      // 16-byte loads (4-byte aligned planes)
    if (i + 4 <= hi) {
      const f32x4u d4 = *reinterpret_cast<const f32x4u*>(pd + i), z4 = *reinterpret_cast<const f32x4u*>(pz + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s += d4[e];
        q += (double)d4[e] * (double)((z4[e] - m) * is);
      }
    } else {
      for (int e = i; e < hi; ++e) {
        const float d = pd[e];
        s += d;
        q += (double)d * (double)((pz[e] - m) * is);
      }
    }
  }
  __shared__ double rs[4], rq[4];
  s = wave_sum(s);
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)plane * gridDim.x + blockIdx.x) * 2;
    o[0] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
    o[1] = (rq[0] + rq[1]) + (rq[2] + rq[3]);
  }
}

// dz = gamma*invstd * (dy - sum_dy/n - xhat * sum_dy_xhat/n);  dgamma = sum_dy_xhat, dbeta = sum_dy
__global__ __launch_bounds__(256) void bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ z,
                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma, const double* __restrict__ sums,
                                                    double count_host, const double* __restrict__ count_dev, int C, int HW,
                                                    float* __restrict__ dz, int64_t total) {
  const double count = count_dev ? count_dev[0] : count_host;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i / HW) % C);
    const float is = invstd[c];
    const float xh = (z[i] - mean[c]) * is;
    const float a = (float)(sums[c] / count), b = (float)(sums[C + c] / count);
    dz[i] = gamma[c] * is * (dy[i] - a - xh * b);
  }
}

__global__ void bn_bwd_params(const double* __restrict__ sums, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (dbeta) dbeta[c] = (float)sums[c];
  if (dgamma) dgamma[c] = (float)sums[C + c];
}

}  // namespace dasac

extern "C" size_t dasac_bn_stats_workspace(int N, int C, int64_t HW) {
  return (size_t)N * C * (size_t)((HW + kBnChunk - 1) / kBnChunk) * 2 * sizeof(double);
}

extern "C" int dasac_bn_stats(const float* z, int N, int C, int64_t HW, double* sums, void* workspace, size_t ws_bytes,
                              dasac_stream_t stream) {
  DASAC_REQUIRE(z && sums && workspace && N > 0 && C > 0 && HW > 0 && HW < (1ll << 31), "bn_stats: bad arguments");
  if (ws_bytes < dasac_bn_stats_workspace(N, C, HW)) return fail(DASAC_EWORKSPACE, "bn_stats: workspace too small");
  hipStream_t s = as_stream(stream);
  const int chunks = (int)((HW + kBnChunk - 1) / kBnChunk);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_stats, dim3((unsigned)chunks, N * C), dim3(256), 0, s, z, C, (int)HW, partial);
  DASAC_CHECK_LAUNCH("bn_stats");
  hipLaunchKernelGGL(bn_sums_finish, dim3(C), dim3(64), 0, s, partial, N, C, chunks, sums, (float*)nullptr, (float*)nullptr);
  DASAC_CHECK_LAUNCH("bn_sums_finish");
  return DASAC_OK;
}

static int bn_finalize_launch(const double* sums, const float* tile_stats, int n_tiles, int mpad, double count,
                              const double* count_dev, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int C, float* scale,
                              float* shift, float* mean, float* invstd, dasac_stream_t stream) {
  DASAC_REQUIRE((sums || (tile_stats && n_tiles > 0 && mpad >= C)) && gamma && beta && scale && shift && mean && invstd && C > 0 &&
                    (count > 0 || count_dev),
                "bn_train_finalize: bad arguments");
  hipLaunchKernelGGL(bn_train_finalize, dim3((C + 63) / 64), dim3(64), 0, as_stream(stream), sums, tile_stats, n_tiles, mpad, count,
                     count_dev, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, C, scale, shift, mean, invstd);
  DASAC_CHECK_LAUNCH("bn_train_finalize");
  return DASAC_OK;
}

extern "C" int dasac_bn_train_finalize(const double* sums, double count, const double* count_dev, const float* gamma,
                                       const float* beta, float* running_mean, float* running_var,
                                       int64_t* num_batches_tracked, float momentum, float eps, int C, float* scale,
                                       float* shift, float* mean, float* invstd, dasac_stream_t stream) {
  DASAC_REQUIRE(sums, "bn_train_finalize: null sums");
  return bn_finalize_launch(sums, nullptr, 0, 0, count, count_dev, gamma, beta, running_mean, running_var, num_batches_tracked,
                            momentum, eps, C, scale, shift, mean, invstd, stream);
}

extern "C" int dasac_bn_train_finalize_tiles(const float* tile_stats, int n_tiles, int mpad, double count, const float* gamma,
                                             const float* beta, float* running_mean, float* running_var,
                                             int64_t* num_batches_tracked, float momentum, float eps, int C, float* scale,
                                             float* shift, float* mean, float* invstd, dasac_stream_t stream) {
  DASAC_REQUIRE(tile_stats, "bn_train_finalize_tiles: null statistics");
  return bn_finalize_launch(nullptr, tile_stats, n_tiles, mpad, count, nullptr, gamma, beta, running_mean, running_var,
                            num_batches_tracked, momentum, eps, C, scale, shift, mean, invstd, stream);
}

extern "C" int dasac_bn_tile_stats_reduce(const float* tile_stats, int n_tiles, int C, int mpad, double* sums,
                                          dasac_stream_t stream) {
  DASAC_REQUIRE(tile_stats && sums && n_tiles > 0 && C > 0 && mpad >= C, "bn_tile_stats_reduce: bad arguments");
  hipLaunchKernelGGL(bn_tile_stats_reduce, dim3((C + 63) / 64), dim3(64), 0, as_stream(stream), tile_stats, n_tiles, C, mpad, sums);
  DASAC_CHECK_LAUNCH("bn_tile_stats_reduce");
  return DASAC_OK;
}

extern "C" int dasac_bn_apply(const float* z, const float* scale, const float* shift, const float* res, int relu, int N,
                              int C, int64_t HW, float* y, dasac_stream_t stream) {
  DASAC_REQUIRE(z && scale && shift && y && N > 0 && C > 0 && HW > 0, "bn_apply: bad arguments");
  const int64_t total = (int64_t)N * C * HW;
  hipLaunchKernelGGL(bn_apply, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(stream), z, scale, shift, res, relu, C,
                     (int)HW, y, total);
  DASAC_CHECK_LAUNCH("bn_apply");
  return DASAC_OK;
}

extern "C" int dasac_bn_bwd_reduce(const float* dy, const float* z, const float* mean, const float* invstd, int N, int C,
                                   int64_t HW, double* sums, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                                   dasac_stream_t stream) {
  DASAC_REQUIRE(dy && z && mean && invstd && sums && workspace && N > 0 && C > 0 && HW > 0 && HW < (1ll << 31),
                "bn_bwd_reduce: bad arguments");
  if (ws_bytes < dasac_bn_stats_workspace(N, C, HW)) return fail(DASAC_EWORKSPACE, "bn_bwd_reduce: workspace too small");
  hipStream_t s = as_stream(stream);
  const int chunks = (int)((HW + kBnChunk - 1) / kBnChunk);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_bwd_reduce, dim3((unsigned)chunks, N * C), dim3(256), 0, s, dy, z, mean, invstd, C, (int)HW, partial);
  DASAC_CHECK_LAUNCH("bn_bwd_reduce");
  hipLaunchKernelGGL(bn_sums_finish, dim3(C), dim3(64), 0, s, partial, N, C, chunks, sums, dbeta, dgamma);
  DASAC_CHECK_LAUNCH("bn_sums_finish");
  return DASAC_OK;
}

extern "C" int dasac_bn_train_apply_tiles(const float* z, const float* tile_stats, int n_tiles, int mpad, double count,
                                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                                          int64_t* num_batches_tracked, float momentum, float eps, const float* res, int relu,
                                          int N, int C, int64_t HW, float* y, float* mean, float* invstd, dasac_stream_t stream) {
  DASAC_REQUIRE(z && tile_stats && gamma && beta && y && mean && invstd && n_tiles > 0 && mpad >= C && count > 0 && N > 0 && C > 0 &&
                    HW > 0 && HW < (1ll << 31) && (int64_t)N * C < 65536,
                "bn_train_apply_tiles: bad arguments");
  hipLaunchKernelGGL(bn_apply_tiles, dim3((unsigned)((HW + kBnBig - 1) / kBnBig), N * C), dim3(256), 0, as_stream(stream), z, tile_stats,
                     n_tiles, mpad, count, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, res, relu, C,
                     (int)HW, y, mean, invstd);
  DASAC_CHECK_LAUNCH("bn_apply_tiles");
  return DASAC_OK;
}

extern "C" int dasac_bn_bwd_fused(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma,
                                  double count, int N, int C, int64_t HW, float* dz, float* dgamma, float* dbeta, void* workspace,
                                  size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(dy && z && mean && invstd && gamma && dz && workspace && count > 0 && N > 0 && C > 0 && HW > 0 && HW < (1ll << 31) &&
                    (int64_t)N * C < 65536,
                "bn_bwd_fused: bad arguments");
  if (ws_bytes < dasac_bn_stats_workspace(N, C, HW)) return fail(DASAC_EWORKSPACE, "bn_bwd_fused: workspace too small");
  hipStream_t s = as_stream(stream);
  const int chunks = (int)((HW + kBnChunk - 1) / kBnChunk);
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_bwd_reduce, dim3((unsigned)chunks, N * C), dim3(256), 0, s, dy, z, mean, invstd, C, (int)HW, partial);
  DASAC_CHECK_LAUNCH("bn_bwd_reduce");
  hipLaunchKernelGGL(bn_bwd_apply_partials, dim3((unsigned)((HW + kBnBig - 1) / kBnBig), N * C), dim3(256), 0, s, dy, z, mean, invstd,
                     gamma, partial, N, chunks, count, C, (int)HW, dz, dgamma, dbeta);
  DASAC_CHECK_LAUNCH("bn_bwd_apply_partials");
  return DASAC_OK;
}

extern "C" int dasac_bn_bwd_apply(const float* dy, const float* z, const float* mean, const float* invstd,
                                  const float* gamma, const double* sums, double count, const double* count_dev, int N, int C,
                                  int64_t HW, float* dz, float* dgamma, float* dbeta, dasac_stream_t stream) {
  DASAC_REQUIRE(dy && z && mean && invstd && gamma && sums && dz && (count > 0 || count_dev), "bn_bwd_apply: bad arguments");
  const int64_t total = (int64_t)N * C * HW;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(bn_bwd_apply, dim3(stream_grid(total, 256)), dim3(256), 0, s, dy, z, mean, invstd, gamma, sums, count,
                     count_dev, C, (int)HW, dz, total);
  DASAC_CHECK_LAUNCH("bn_bwd_apply");
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(bn_bwd_params, dim3((C + 255) / 256), dim3(256), 0, s, sums, C, dgamma, dbeta);
    DASAC_CHECK_LAUNCH("bn_bwd_params");
  }
  return DASAC_OK;
}

// ------------------------------------------------------------------------------------------------
// Validation counts: utils/metrics.py:9-53 `Jaccard.add_sample` + the argmax of
// train.py:339-469 -- per-class true-positive / false-positive / false-negative pixel counts from the
// upsampled logits in ONE pass (the reference loops over the 19 classes with .item() syncs per batch).
// ------------------------------------------------------------------------------------------------
namespace dasac {

__global__ __launch_bounds__(256) void iou_counts(const float* __restrict__ logits, const int64_t* __restrict__ gt, int C,
                                                  int64_t HW, int64_t total, int ignore_index,
                                                  unsigned long long* __restrict__ counts) {
  __shared__ unsigned int s[3 * 64];
  for (int i = threadIdx.x; i < 3 * 64; i += 256) s[i] = 0;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int64_t b = p / HW, r = p - b * HW;
    const int64_t y = gt[p];
    if (y == ignore_index) continue;        // utils/metrics.py:28-30: only ignore_index pixels are dropped
    const float* lp = logits + b * C * HW + r;
    float best = lp[0];
    int k = 0;
    for (int c = 1; c < C; ++c) {
      const float v = lp[(int64_t)c * HW];
      if (v > best) {
        best = v;
        k = c;
      }
    }
    if (y == k) {
      atomicAdd(&s[k], 1u);                 // tp
    } else {
      atomicAdd(&s[64 + k], 1u);            // fp of the predicted class (also when gt is no class at all, e.g. -1)
      if (y >= 0 && y < C) atomicAdd(&s[128 + (int)y], 1u);      // fn of the true class
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 64; i += 256)
    if (s[i] && (i & 63) < C) atomicAdd(&counts[(i >> 6) * C + (i & 63)], (unsigned long long)s[i]);
}

}  // namespace dasac

extern "C" int dasac_iou_counts(const float* logits, const int64_t* gt, int B, int C, int64_t HW, int ignore_index,
                                int64_t* counts, dasac_stream_t stream) {
  DASAC_REQUIRE(logits && gt && counts && B > 0 && C > 0 && C <= 64 && HW > 0, "iou_counts: bad arguments");
  const int64_t total = (int64_t)B * HW;
  hipLaunchKernelGGL(iou_counts, dim3(stream_grid(total, 256, kNumCu * 8)), dim3(256), 0, as_stream(stream), logits, gt, C, HW, total,
                     ignore_index, reinterpret_cast<unsigned long long*>(counts));
  DASAC_CHECK_LAUNCH("iou_counts");
  return DASAC_OK;
}

// ------------------------------------------------------------------------------------------------
// Label preparation and Dropout2d masks (what was left on ATen inside the step)
// ------------------------------------------------------------------------------------------------
namespace dasac {

// models/sac.py:337-338: ignore_mask = (y == -1); y[ignore_mask] = 255  -- one pass, in place
__global__ __launch_bounds__(256) void label_pad_mask(int64_t* __restrict__ y, uint8_t* __restrict__ mask, int64_t n,
                                                      int64_t pad_label, int64_t ignore_label) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const bool pad = y[i] == pad_label;
    mask[i] = pad ? 1 : 0;
    if (pad) y[i] = ignore_label;
  }
}

// Philox4x32-10 (Salmon et al., SC'11): counter (i, stream offset), key = seed
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr.x, p1 = (uint64_t)0xCD9E8D57u * ctr.z;
    ctr = make_uint4((uint32_t)(p1 >> 32) ^ ctr.y ^ key.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.w ^ key.y, (uint32_t)p0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// Dropout2d (fcn.py:52,56): per (n, c) plane  keep/(1-p) with keep ~ Bernoulli(1-p)
__global__ __launch_bounds__(256) void dropout_planes(uint64_t seed, uint64_t offset, float p, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4 r = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const float u = (float)(r.x >> 8) * (1.0f / 16777216.0f);      // uniform on [0, 1), 24 bits
  out[i] = u >= p ? 1.0f / (1.0f - p) : 0.0f;
}

}  // namespace dasac

extern "C" int dasac_label_pad_mask(int64_t* labels, uint8_t* mask, int64_t n, int pad_label, int ignore_label,
                                    dasac_stream_t stream) {
  DASAC_REQUIRE(labels && mask && n > 0, "label_pad_mask: bad arguments");
  hipLaunchKernelGGL(label_pad_mask, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), labels, mask, n,
                     (int64_t)pad_label, (int64_t)ignore_label);
  DASAC_CHECK_LAUNCH("label_pad_mask");
  return DASAC_OK;
}

extern "C" int dasac_dropout_planes(uint64_t seed, uint64_t offset, float p, int64_t planes, float* keep_scale,
                                    dasac_stream_t stream) {
  DASAC_REQUIRE(keep_scale && planes > 0 && p >= 0.f && p < 1.f, "dropout_planes: bad arguments");
  hipLaunchKernelGGL(dropout_planes, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, as_stream(stream), seed, offset, p,
                     planes, keep_scale);
  DASAC_CHECK_LAUNCH("dropout_planes");
  return DASAC_OK;
}
