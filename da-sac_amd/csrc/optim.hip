// Multi-tensor kernels over every parameter in one launch: the momentum-teacher update, fused SGD / Nesterov / Adam, the
// gradient-norm control block and the per-tensor gradient health table.  multi_tensor.hpp has the (tensor, chunk) walk.
#include "multi_tensor.hpp"

namespace dasac {

// ---- momentum teacher (models/sac.py:83-102) as one multi-tensor launch --------------------------
// chunk table: for chunk i, tensor id + chunk index.  sq_chunk[i] = sum (slow-fast)^2 over the chunk (pre-update);
// if update: slow = slow*m + fast*(1-m).
struct TensorPair {
  const float* fast;
  float* slow;
  int64_t n;
};

__global__ __launch_bounds__(256) void ema_chunks(const TensorPair* __restrict__ pairs, const int2* __restrict__ chunks,
                                                  float momentum, float one_minus, int update, double* __restrict__ sq_chunk) {
  const Chunk ch = this_chunk(chunks);
  const TensorPair tp = pairs[ch.tensor];
  const int64_t base = ch.base();
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
  acc = block_sum(acc);
  if (threadIdx.x == 0) sq_chunk[blockIdx.x] = acc;      // one partial per chunk: no atomics
}

// sq[t] = sum of tensor t's chunk partials, in a fixed order (one wave per tensor; `chunks` is sorted by tensor id)
__global__ __launch_bounds__(64) void ema_tensor_sums(const int2* __restrict__ chunks, int n_chunks, const double* __restrict__ sq_chunk,
                                                      double* __restrict__ sq) {
  const int t = blockIdx.x;
  double s = 0;
  for (int i = first_chunk_of(chunks, n_chunks, t) + threadIdx.x; i < n_chunks && chunks[i].x == t; i += 64) s += sq_chunk[i];
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
struct SgdGroups {      // rows: SgdTensor of multi_tensor.hpp
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
  const Chunk ch = this_chunk(chunks);
  const SgdTensor t = tensors[ch.tensor];
  const int64_t group = CTL ? (t.group & 7) : t.group;
  const float lr = hp.lr[group], wd = hp.wd[group];
  const int64_t base = ch.base();
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
struct AdamGroups {      // rows: AdamTensor of multi_tensor.hpp
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

// CTL = false is the kernel as it has always been (`ctl` / `flags` unused); CTL = true: GradCtl above.
template <bool CTL>
__global__ __launch_bounds__(256) void adam_chunks(const AdamTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                   AdamGroups hp, AdamScalars s, const GradCtl* __restrict__ ctl, int flags) {
  const Chunk ch = this_chunk(chunks);
  const AdamTensor t = tensors[ch.tensor];
  const float wd = hp.wd[t.group & 7], neg_step = -t.step_size, bc2_sqrt = t.bc2_sqrt;
  const bool small_w = fabsf(s.w1) < 0.5f;
  const int64_t base = ch.base();
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
  if ((bits & 15) == 0 && base + kChunk <= t.n) {
#pragma unroll 2
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + (j * 256 + threadIdx.x) * 4;
      f32x4 p = *reinterpret_cast<const f32x4*>(t.p + i), g = *reinterpret_cast<const f32x4*>(t.g + i);
      f32x4 m = *reinterpret_cast<const f32x4*>(t.m + i), v = *reinterpret_cast<const f32x4*>(t.v + i);
      if (t.g2) {      // written out, as in grad_sq_chunks: on summed_grad4 the g2 branch moves ahead of the m and v loads
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
// One double partial per (tensor, chunk) of the update kernels' own tables (GradRow), no atomics; grad_norm_finish adds the
// partials in a fixed order: the same inputs give the same bits.  d = g2 + g is the fp32 sum the update applies (AccumulateGrad's
// operand order); d*d is exact in double.  Thread t owns elements (j*256 + t)*4 + e of the chunk on BOTH paths -- one dwordx4
// load per j where the chunk is whole and both pointers are 16-byte aligned, four guarded scalar loads otherwise -- and adds them
// in the same order, so the norm does not depend on where a gradient happens to lie (a view into a flat reduction buffer may sit
// at any 4-byte offset).  The two loops are written out, not one loop over summed_grad4 (tensor_stats_chunks' form): that measured
// 2.5 percent slower with a stashed gradient (profiles/pointwise_split.md).
__global__ __launch_bounds__(256) void grad_sq_chunks(const char* __restrict__ rows, int row_bytes, int n_off,
                                                      const int2* __restrict__ chunks, double* __restrict__ sq_chunk) {
  const Chunk ch = this_chunk(chunks);
  const GradRow r = grad_row(rows, row_bytes, n_off, ch.tensor);
  const float *g = r.g, *g2 = r.g2;
  const int64_t n = r.n, base = ch.base();
  double acc = 0;
  if ((((uintptr_t)g | (uintptr_t)g2) & 15) == 0 && base + kChunk <= n) {
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
  acc = block_sum(acc);
  if (threadIdx.x == 0) sq_chunk[blockIdx.x] = acc;      // one partial per chunk: no atomics
}

// total, coef and the skip flag from the chunk partials; in fp32 from the square root on, as torch.nn.utils.clip_grad_norm_
// computes them.  A NaN norm gives a NaN coef (torch.clamp keeps NaN; fminf would not).  One block, fixed summation order.
__global__ __launch_bounds__(256) void grad_norm_finish(const double* __restrict__ sq_chunk, int n_chunks, float max_norm,
                                                        GradCtl* __restrict__ ctl, int64_t* __restrict__ skipped) {
  double s = 0;
  for (int i = threadIdx.x; i < n_chunks; i += 256) s += sq_chunk[i];
  s = block_sum(s);
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(s);
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

// One partial row per (tensor, chunk), no atomics.  Rows as grad_sq_chunks reads them (GradRow); p and the state pointer may be
// null: zeros in their columns.  first_bit (the SGD table): bit 32 of `group` marks a tensor that takes its first step -- its
// momentum buffer is uninitialised memory and is NOT read.
// Thread t owns elements (j*256 + t)*4 + e on the vector and on the scalar path, each input takes the path its own pointer
// allows, and the per-thread sums run in the same order on both: the table does not depend on where a tensor lies.
__global__ __launch_bounds__(256) void tensor_stats_chunks(const char* __restrict__ rows, int row_bytes, int n_off, int first_bit,
                                                           const int2* __restrict__ chunks, double* __restrict__ partial) {
  const Chunk ch = this_chunk(chunks);
  const GradRow r = grad_row(rows, row_bytes, n_off, ch.tensor);
  const float* st = first_bit && ((r.group >> 32) & 1) ? nullptr : r.state;
  const int64_t base = ch.base(), n = r.n;
  const bool whole = base + kChunk <= n;
  const bool vec_g = whole && (((uintptr_t)r.g | (uintptr_t)r.g2) & 15) == 0;
  const bool vec_p = whole && ((uintptr_t)r.p & 15) == 0, vec_s = whole && ((uintptr_t)st & 15) == 0;
  double g_sq = 0, p_sq = 0, s_sq = 0;
  float g_max = 0.f, p_max = 0.f;
  int nonfinite = 0, zeros = 0, first = kChunk;      // first: offset inside the chunk, kChunk = none
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int off = (j * 256 + threadIdx.x) * 4;
    const int64_t i = base + off;
    const f32x4 d = summed_grad4(r.g, r.g2, i, n, vec_g);
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
    if (r.p) {      // elements beyond the end load as 0: nothing to guard
      const f32x4 v = chunk_load4(r.p, i, n, vec_p);
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
      v = v < (double)kChunk ? (double)base + v + 1.0 : 0.0;
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
    for (int i = first_chunk_of(chunks, n_chunks, t) + threadIdx.x; i < n_chunks && chunks[i].x == t; i += 64) {
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

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_ema_chunk_elems(void) { return kChunk; }

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

struct CtlArgs {      // what a _ctl entry takes on top of the plain one (`first` may be per row there; Adam has none: 0)
  const void* ctl;
  int apply_coef, honour_skip, first;
  int flags() const { return apply_coef * kCtlClip + honour_skip * kCtlSkip; }
};

// What the six step entries check, in the order that decides which message wins.  The optional checks are null where they are
// not the entry's: Nesterov's momentum, Adam's {beta1, beta2, eps}, the control block with the range of `first`.  Adam has no
// learning-rate table and passes group_wd for group_lr.
static int check_step(const char* name, const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_lr,
                      const float* group_wd, int n_groups, const float* nesterov_momentum, const double* adam, const CtlArgs* c) {
  DASAC_REQUIRE(tensors && chunks && group_lr && group_wd && n_tensors > 0 && n_chunks > 0, "%s: bad arguments", name);
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "%s: misaligned row table / chunk list", name);
  DASAC_REQUIRE(n_groups >= 1 && n_groups <= 8, "%s: 1..8 parameter groups", name);
  DASAC_REQUIRE(!nesterov_momentum || *nesterov_momentum > 0.f, "%s: Nesterov momentum requires a momentum", name);
  DASAC_REQUIRE(!adam || (adam[0] >= 0.0 && adam[0] < 1.0 && adam[1] >= 0.0 && adam[1] < 1.0 && adam[2] >= 0.0),
                "%s: betas in [0, 1), eps >= 0", name);
  DASAC_REQUIRE(!c || (c->first >= -1 && c->first <= 1), "%s: first is 0, 1 or -1 (per row)", name);
  DASAC_REQUIRE(!c || (c->ctl && ((uintptr_t)c->ctl & 15) == 0 && (c->apply_coef == 0 || c->apply_coef == 1) &&
                       (c->honour_skip == 0 || c->honour_skip == 1)),
                "%s: a 16-byte aligned control block and 0/1 flags", name);
  return DASAC_OK;
}

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
  if (int e = check_step("sgd_step", tensors, n_tensors, chunks, n_chunks, group_lr, group_wd, n_groups, nullptr, nullptr, nullptr)) return e;
  return launch_sgd<false, false>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, nullptr, 0, stream);
}

extern "C" int dasac_sgd_nesterov_step(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                       const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                                       dasac_stream_t stream) {
  if (int e = check_step("sgd_nesterov_step", tensors, n_tensors, chunks, n_chunks, group_lr, group_wd, n_groups, &momentum, nullptr, nullptr))
    return e;
  return launch_sgd<true, false>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, nullptr, 0, stream);
}

extern "C" int dasac_sgd_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_lr,
                                  const float* group_wd, int n_groups, float momentum, int first, const void* ctl, int apply_coef,
                                  int honour_skip, dasac_stream_t stream) {
  const CtlArgs c{ctl, apply_coef, honour_skip, first};
  if (int e = check_step("sgd_step_ctl", tensors, n_tensors, chunks, n_chunks, group_lr, group_wd, n_groups, nullptr, nullptr, &c)) return e;
  return launch_sgd<false, true>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, ctl, c.flags(), stream);
}

extern "C" int dasac_sgd_nesterov_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks,
                                           const float* group_lr, const float* group_wd, int n_groups, float momentum, int first,
                                           const void* ctl, int apply_coef, int honour_skip, dasac_stream_t stream) {
  const CtlArgs c{ctl, apply_coef, honour_skip, first};
  if (int e = check_step("sgd_nesterov_step_ctl", tensors, n_tensors, chunks, n_chunks, group_lr, group_wd, n_groups, &momentum, nullptr, &c))
    return e;
  return launch_sgd<true, true>(tensors, chunks, n_chunks, sgd_groups(group_lr, group_wd, n_groups), momentum, first, ctl, c.flags(), stream);
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
  const double adam[3] = {beta1, beta2, eps};
  if (int e = check_step("adam_step", tensors, n_tensors, chunks, n_chunks, group_wd, group_wd, n_groups, nullptr, adam, nullptr)) return e;
  return launch_adam<false>(tensors, chunks, n_chunks, group_wd, n_groups, beta1, beta2, eps, nullptr, 0, stream);
}

extern "C" int dasac_adam_step_ctl(const void* tensors, int n_tensors, const int32_t* chunks, int n_chunks, const float* group_wd,
                                   int n_groups, double beta1, double beta2, double eps, const void* ctl, int apply_coef,
                                   int honour_skip, dasac_stream_t stream) {
  const double adam[3] = {beta1, beta2, eps};
  const CtlArgs c{ctl, apply_coef, honour_skip, 0};
  if (int e = check_step("adam_step_ctl", tensors, n_tensors, chunks, n_chunks, group_wd, group_wd, n_groups, nullptr, adam, &c)) return e;
  return launch_adam<true>(tensors, chunks, n_chunks, group_wd, n_groups, beta1, beta2, eps, ctl, c.flags(), stream);
}

extern "C" size_t dasac_grad_norm_workspace(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(double) : 0; }

extern "C" int dasac_grad_norm(const void* tensors, int row_bytes, int n_tensors, const int32_t* chunks, int n_chunks, float max_norm,
                               void* workspace, size_t workspace_bytes, void* ctl, int64_t* skipped, dasac_stream_t stream) {
  DASAC_REQUIRE(tensors && chunks && workspace && ctl && n_tensors > 0 && n_chunks > 0, "grad_norm: bad arguments");
  DASAC_REQUIRE(rows_aligned(tensors, chunks), "grad_norm: misaligned row table / chunk list");
  int n_off;
  if (int e = grad_row_n_off("grad_norm", row_bytes, &n_off)) return e;
  DASAC_REQUIRE(workspace_bytes >= dasac_grad_norm_workspace(n_chunks) && ((uintptr_t)workspace & 7) == 0, "grad_norm: workspace too small");
  DASAC_REQUIRE(((uintptr_t)ctl & 15) == 0 && ((uintptr_t)skipped & 7) == 0, "grad_norm: misaligned control block / counter");
  DASAC_REQUIRE(max_norm == max_norm && max_norm <= 3.4028234664e38f, "grad_norm: max_norm is a finite number (<= 0: measure only)");
  hipStream_t s = as_stream(stream);
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
  int n_off;
  if (int e = grad_row_n_off("tensor_stats", row_bytes, &n_off)) return e;
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
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(tensor_stats_chunks, dim3(n_chunks), dim3(256), 0, s, reinterpret_cast<const char*>(tensors), row_bytes, n_off,
                     row_bytes == (int)sizeof(SgdTensor) ? 1 : 0, reinterpret_cast<const int2*>(chunks), partial);
  DASAC_CHECK_LAUNCH("tensor_stats_chunks");
  hipLaunchKernelGGL(tensor_stats_finish, dim3(n_rows), dim3(64), 0, s, reinterpret_cast<const int2*>(chunks), n_chunks, n_tensors, row_of,
                     partial, table, reinterpret_cast<const GradCtl*>(ctl), captured, captured_at, skipped);
  DASAC_CHECK_LAUNCH("tensor_stats_finish");
  return DASAC_OK;
}
