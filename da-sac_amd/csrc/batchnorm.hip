// BatchNorm around the conv GEMMs: frozen-BN folding and parameter gradients, per-channel sums, and the train-mode kernels.
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
  // not block_sum: this kernel adds the four wave sums left to right, ((r0 + r1) + r2) + r3, and keeps the bits it has always given
  __shared__ double red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (float)(red[0] + red[1] + red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------
// Train-mode BatchNorm (baseline / AdaBN mode: models/__init__.py:29 leaves BN un-frozen, every
// nn.SyncBatchNorm of deeplabv2.py:15 / fcn.py:8 normalises with batch statistics; train.py:281-289
// re-estimates the running statistics on target crops).  Cross-rank statistics (SyncBN) are summed by
// the caller with one RCCL all-reduce of the raw (sum, sum of squares) / (sum dy, sum dy*xhat) vectors.
// ------------------------------------------------------------------------------------------------

constexpr int kBnChunk = 256 * 16;

// The kernels below write their (s, q) block sums and the tile-statistics sum ts[2i][c], ts[2i + 1][c] out, each in the order of
// block_sum (common.hpp): no project tool times them, so they keep the instruction streams they had, and on a shared pair helper
// every one of them compiled to another (profiles/pointwise_split.md).

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

// Batch moments of a channel (sum, sum of squares, count) -> what train-mode BN needs of them.  bn_train_finalize and
// bn_apply_tiles must agree bit for bit (the engine picks between them by rank count), so both take the arithmetic from here.
// gamma is read inside and shift formed on demand: where the callers read gamma[c] and beta[c] decides their instruction order.
struct BnAffine {
  double var;      // biased, before rounding: the unbiased running variance starts from it
  float mean, varf, invstd, scale;
  __device__ float shift(float beta) const { return beta - mean * scale; }
};
__device__ __forceinline__ BnAffine bn_moments_to_affine(double s1, double s2, double count, const float* gamma, int c, float eps) {
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0) var = 0;
  const float meanf = (float)m, varf = (float)var;
  const float is = 1.f / sqrtf(varf + eps);
  return BnAffine{var, meanf, varf, is, gamma[c] * is};
}
// running stats of channel c: momentum update with the unbiased var
__device__ __forceinline__ void bn_move_running(BnAffine b, double count, float momentum, float* running_mean, float* running_var, int c) {
  const float unbiased = count > 1 ? (float)(b.var * count / (count - 1)) : b.varf;
  running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * b.mean;
  running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
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
  const BnAffine b = bn_moments_to_affine(s1, s2, count, gamma, c, eps);
  scale[c] = b.scale;
  shift[c] = b.shift(beta[c]);
  mean_out[c] = b.mean;
  invstd_out[c] = b.invstd;
  if (running_mean) bn_move_running(b, count, momentum, running_mean, running_var, c);
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
// shift with bn_train_finalize's own bn_moments_to_affine, normalises its chunk with 16-byte accesses; the block of (n = 0, chunk 0) also writes
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
  const BnAffine b = bn_moments_to_affine(s1, s2, count, gamma, c, eps);
  const float a = b.scale, sh = b.shift(beta[c]);
  if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    mean_out[c] = b.mean;
    invstd_out[c] = b.invstd;
    if (running_mean) bn_move_running(b, count, momentum, running_mean, running_var, c);
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
