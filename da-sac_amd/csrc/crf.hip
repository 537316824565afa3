// Mean-field refinement of inference label maps (dasac_crf_meanfield): a locally connected CRF in the ConvCRF form (Teichmann &
// Cipolla, 2018) -- truncated Gaussian kernels on a dilated (2r+1)^2 window, Potts compatibility -- over the fused class
// probabilities and the image, the step DeepLabv2's published pipeline ends in.  include/dasac_hip.h has the definition.
//
// One launch per mean-field iteration; iteration t reads Q^(t-1) (the caller's P for t = 1) and writes Q^t to one of two buffers of
// the caller's workspace; the last one fuses arg-max, LUT and confidence and writes probs_out (if asked for) instead.
//
// crf_iteration   one block per 16 x 64 tile of one image, a wave per row: thread (wave, lane) owns the pixels (wave + 4 i, lane),
//                 i < 4.  Lanes run along x, so every LDS read of a tap is 64 consecutive floats -- no bank conflict at any offset --
//                 and every global access of a row is 256 consecutive bytes.  (Four CONSECUTIVE pixels per lane would make each tap
//                 read a stride-4 LDS access, 4-way conflicted; the four pixels of a thread are four rows instead.)
//                 The image tile plus its r*d halo is staged ONCE per block (pixels outside the image as 0, never read from memory),
//                 the class planes of Q in chunks of `ck` <= 5 planes, as many as fit beside the image in 64 KiB.  Per chunk a
//                 thread walks the taps in row-major order of (a, b): the tap weight of each of its pixels -- the two spatial Gaussians
//                 are per-tap constants from the kernel arguments (w_app folded into the exponent), the appearance term costs one
//                 v_exp_f32 -- then one LDS read and one FMA per class of the chunk.  The weights are RECOMPUTED per chunk: held
//                 over the chunks they would take 120 x 4 registers or 480 KB of LDS; the recomputation costs about 12 vector
//                 instructions per tap and pixel beside the chunk's 5 reads and FMAs.
//                 A chunk ends with logit = log(max(P, 1e-20)) + compat * message / den parked in the OUTPUT plane of its class
//                 (each thread reads back only what it wrote itself) and an online (max, sum) of the softmax; after the last chunk
//                 the thread normalises its parked logits in class order.  Nothing is summed across threads, no atomics: the same
//                 bits on every run and wherever the tensors lie.
//
// Instantiations <CT, CIT, HT>: the image's channel count is always a template parameter (1..4) and the number of planes of a chunk
// a template parameter of the tap walk, so that no LDS read sits behind a runtime condition; C = 19 over three channels is compiled
// in, once with the halo of the default window (r d = 5: plane offsets become instruction immediates) and once for any halo.
//
// All global accesses are element loads / stores at indices checked against the image; offsets are 64-bit.
// LDS: dynamic, (Ci + ck) planes of (16 + 2 r d) x (64 + 2 r d) floats: 61.6 KB with the defaults (r d = 5, Ci = 3, ck = 5), 60 KB at
// the limits (r d = 8, Ci = 4, ck = 2): two blocks per CU.  Registers: 20 accumulators, 4 Ci centre values of the image; 96 VGPRs
// for the default shape, at most 115; no scratch (tests/test_kernel_resources_crf.py).  Time and what bounds it: profiles/crf_meanfield.md.
#include "common.hpp"

#include <cmath>

namespace dasac {

constexpr int kCrfBlock = 256;
constexpr int kCrfWaves = kCrfBlock / kWave;
constexpr int kCrfTileW = kWave, kCrfTileH = 16;       // a wave is one row of the tile
constexpr int kCrfOwn = kCrfTileH / kCrfWaves;         // pixels per thread: rows wave, wave + 4, ...
constexpr int kCrfMaxC = 32, kCrfMaxCi = 4, kCrfMaxRadius = 5, kCrfMaxDilation = 4, kCrfMaxHalo = 8, kCrfMaxIter = 16;
constexpr int kCrfChunk = 5;                           // class planes of Q staged at once, at most
constexpr int kCrfMaxTaps = (2 * kCrfMaxRadius + 1) * (2 * kCrfMaxRadius + 1) - 1;
constexpr int kCrfStage = 4;                           // loads a thread keeps in flight while it stages a plane
constexpr size_t kCrfLdsBudget = 64 * 1024;
constexpr float kCrfFloor = 1e-20f;                    // u = log(max(P, floor))

// the per-tap constants, by value in the kernel arguments (a wave reads them with scalar loads), taps in row-major order of (a, b):
// weight = exp2(app[t] + beta * sum_ch (I_i - I_j)^2) + smooth[t]
struct CrfTaps {
  float app[kCrfMaxTaps];                              // log2(w_app) - |o|^2 log2(e) / (2 theta_alpha^2); -inf when w_app == 0
  float smooth[kCrfMaxTaps];                           // w_smooth exp(-|o|^2 / (2 theta_gamma^2))
};

inline int crf_plane_floats(int halo) { return (kCrfTileH + 2 * halo) * (kCrfTileW + 2 * halo); }
// class planes per chunk: what fits beside the image's Ci planes
inline int crf_chunk(int C, int Ci, int halo) {
  const int fit = (int)(kCrfLdsBudget / (crf_plane_floats(halo) * sizeof(float))) - Ci;
  const int ck = fit < kCrfChunk ? fit : kCrfChunk;
  return ck < C ? ck : C;
}
inline size_t crf_lds_bytes(int Ci, int ck, int halo) { return (size_t)(Ci + ck) * crf_plane_floats(halo) * sizeof(float); }
// bytes of one Q buffer of the workspace
inline size_t crf_q_bytes(int B, int C, int H, int W) { return align_up((size_t)B * C * H * W * sizeof(float), 16); }

// `n` planes of `src` (plane p of this image at src + p * HW) with the tile's halo into LDS; outside the image: 0, not loaded
__device__ __forceinline__ void crf_stage(float* __restrict__ dst, const float* __restrict__ src, int n, int H, int W, int y0, int x0,
                                          int halo, int pitch, int plane, FastDiv div_pitch) {
  const int64_t HW = (int64_t)H * W;
  for (int p = 0; p < n; ++p) {
    const float* sp = src + p * HW;
    float* dp = dst + p * plane;
    for (int i0 = threadIdx.x; i0 < plane; i0 += kCrfStage * kCrfBlock) {
      float v[kCrfStage];
#pragma unroll
      for (int k = 0; k < kCrfStage; ++k) {
        const int i = i0 + k * kCrfBlock;
        const int yy = fdiv(i, div_pitch), xx = i - yy * pitch;
        const int gy = y0 - halo + yy, gx = x0 - halo + xx;
        v[k] = 0.f;
        if (i < plane && gy >= 0 && gy < H && gx >= 0 && gx < W) v[k] = sp[(int64_t)gy * W + gx];
      }
#pragma unroll
      for (int k = 0; k < kCrfStage; ++k) {
        const int i = i0 + k * kCrfBlock;
        if (i < plane) dp[i] = v[k];
      }
    }
  }
}

// The taps of one chunk of NK staged class planes, in row-major order of (a, b), for the thread's four pixels: den += weight,
// acc[k] += weight * Q_j[k].  Every LDS read is unconditional -- a read behind a runtime `k < nk` or `ch < Ci` compiles to a branch
// with a full wait after it, and the walk runs at LDS latency (measured: 3.2 ms per iteration of a 1024 x 2048 frame) -- so NK is a
// template parameter (the caller switches on it once per chunk) and so is the channel count CIT (the launcher switches on it).
template <int NK, int CIT>
__device__ __forceinline__ void crf_taps(const float* __restrict__ s_img, const float* __restrict__ s_q, int plane, int pitch,
                                         int r, int d, const CrfTaps& taps, float beta, const int (&base)[kCrfOwn],
                                         const float (&ctr)[CIT][kCrfOwn], int gx, int gy, int H, int W,
                                         float (&acc)[kCrfChunk][kCrfOwn], float (&den)[kCrfOwn]) {
  int tap = 0;
#pragma unroll 1
  for (int a = -r; a <= r; ++a) {
#pragma unroll 1
    for (int bb = -r; bb <= r; ++bb) {
      if (a == 0 && bb == 0) continue;
      const int dy = a * d, dx = bb * d;
      const float app = taps.app[tap], smooth = taps.smooth[tap];
      ++tap;
      const int off = dy * pitch + dx;
      const bool in_x = (unsigned)(gx + dx) < (unsigned)W;
#pragma unroll
      for (int i = 0; i < kCrfOwn; ++i) {
        // the neighbour's index, opaque to the optimiser: left alone it hoists base + plane offset out of the tap loops for each of
        // the 4 x (CIT + NK) reads and keeps 32 addresses in registers; like this a read is one add of a scalar plane offset
        int j = base[i] + off;
        asm volatile("" : "+v"(j));
        float dist = 0.f;
#pragma unroll
        for (int ch = 0; ch < CIT; ++ch) {
          const float diff = ctr[ch][i] - s_img[ch * plane + j];
          dist = __builtin_fmaf(diff, diff, dist);
        }
        float w = __builtin_amdgcn_exp2f(__builtin_fmaf(beta, dist, app)) + smooth;
        const bool in_y = (unsigned)(gy + kCrfWaves * i + dy) < (unsigned)H;
        w = (in_x && in_y) ? w : 0.f;                  // a neighbour outside the image does not count
        den[i] += w;
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k][i] = __builtin_fmaf(w, s_q[k * plane + j], acc[k][i]);
      }
    }
  }
}

// grid: B * tiles_y * tiles_x blocks, x fastest.  dynamic LDS: crf_lds_bytes(Ci, ck, r * d).
// q_in: Q^(t-1) [B,C,H,W]; q_out: Q^t, holds the parked logits first (never q_in, P or the image, never NULL); write_q: normalise it
// (0: the caller wants only what `last` writes: labels through the LUT and conf).  CT: C at compile time or 0; CIT: Ci, always at
// compile time; HT: r * d at compile time or 0 -- with it the plane offsets of the tap reads are instruction immediates, not one
// add each.  amdgpu_waves_per_eu: the register allocator is held to the 128 VGPRs of four waves per SIMD (left alone it takes 129-141
// for some instantiations)
template <int CT, int CIT, int HT>
__global__ __launch_bounds__(kCrfBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void crf_iteration(
    const float* __restrict__ probs, const float* __restrict__ image, const float* __restrict__ q_in, float* __restrict__ q_out, int Crt,
    int H, int W, int r, int d, int ck, float beta, float compat, const CrfTaps taps, int tiles_x, int tiles_y, FastDiv div_pitch,
    int last, int write_q, const uint8_t* __restrict__ lut, uint8_t* __restrict__ labels, float* __restrict__ conf) {
  extern __shared__ float s_crf[];
  const int C = CT > 0 ? CT : Crt;
  constexpr int Ci = CIT;
  const int halo = HT > 0 ? HT : r * d;
  const int pitch = kCrfTileW + 2 * halo, plane = (kCrfTileH + 2 * halo) * pitch;
  float* s_img = s_crf;                                // [Ci][rows][pitch]
  float* s_q = s_crf + Ci * plane;                     // [ck][rows][pitch]

  unsigned t = blockIdx.x;
  const int tx = (int)(t % (unsigned)tiles_x);
  t /= (unsigned)tiles_x;
  const int ty = (int)(t % (unsigned)tiles_y);
  const int64_t b = t / (unsigned)tiles_y;
  const int x0 = tx * kCrfTileW, y0 = ty * kCrfTileH;
  const int lane = (int)(threadIdx.x & (kWave - 1)), wave = (int)(threadIdx.x >> 6);
  const int64_t HW = (int64_t)H * W;
  const int gx = x0 + lane;

  crf_stage(s_img, image + b * Ci * HW, Ci, H, W, y0, x0, halo, pitch, plane, div_pitch);
  __syncthreads();

  int base[kCrfOwn];                                   // LDS index of the pixel itself
  bool own[kCrfOwn];                                   // the pixel lies in the image
  float ctr[CIT][kCrfOwn];
#pragma unroll
  for (int i = 0; i < kCrfOwn; ++i) {
    const int y = wave + kCrfWaves * i;
    base[i] = (halo + y) * pitch + halo + lane;
    own[i] = gx < W && y0 + y < H;
#pragma unroll
    for (int ch = 0; ch < CIT; ++ch) ctr[ch][i] = s_img[ch * plane + base[i]];
  }

  float mx[kCrfOwn], sum[kCrfOwn];                     // the online softmax over the chunks
#pragma unroll
  for (int i = 0; i < kCrfOwn; ++i) {
    mx[i] = -INFINITY;
    sum[i] = 0.f;
  }

  for (int c0 = 0; c0 < C; c0 += ck) {
    const int nk = C - c0 < ck ? C - c0 : ck;
    if (c0 > 0) __syncthreads();                       // every thread is done with the previous chunk's planes
    crf_stage(s_q, q_in + (b * C + c0) * HW, nk, H, W, y0, x0, halo, pitch, plane, div_pitch);
    __syncthreads();

    float acc[kCrfChunk][kCrfOwn], den[kCrfOwn];
#pragma unroll
    for (int i = 0; i < kCrfOwn; ++i) {
      den[i] = 0.f;
#pragma unroll
      for (int k = 0; k < kCrfChunk; ++k) acc[k][i] = 0.f;
    }
    switch (nk) {                                      // one branch-free tap walk per number of planes: no LDS read behind a condition
      case 5: crf_taps<5, CIT>(s_img, s_q, plane, pitch, r, d, taps, beta, base, ctr, gx, y0 + wave, H, W, acc, den); break;
      case 4: crf_taps<4, CIT>(s_img, s_q, plane, pitch, r, d, taps, beta, base, ctr, gx, y0 + wave, H, W, acc, den); break;
      case 3: crf_taps<3, CIT>(s_img, s_q, plane, pitch, r, d, taps, beta, base, ctr, gx, y0 + wave, H, W, acc, den); break;
      case 2: crf_taps<2, CIT>(s_img, s_q, plane, pitch, r, d, taps, beta, base, ctr, gx, y0 + wave, H, W, acc, den); break;
      default: crf_taps<1, CIT>(s_img, s_q, plane, pitch, r, d, taps, beta, base, ctr, gx, y0 + wave, H, W, acc, den); break;
    }

    // the chunk's logits: parked in q_out, and into the online (max, sum)
#pragma unroll
    for (int i = 0; i < kCrfOwn; ++i) {
      if (!own[i]) continue;
      const int64_t pix = (int64_t)(y0 + wave + kCrfWaves * i) * W + gx;
      float l[kCrfChunk], cmax = -INFINITY;
#pragma unroll
      for (int k = 0; k < kCrfChunk; ++k)
        if (k < nk) {
          const int64_t at = (b * C + c0 + k) * HW + pix;
          const float u = logf(fmaxf(probs[at], kCrfFloor));
          const float m = den[i] > 0.f ? acc[k][i] / den[i] : 0.f;
          l[k] = u + compat * m;
          q_out[at] = l[k];
          cmax = fmaxf(cmax, l[k]);
        }
      const float nmax = fmaxf(mx[i], cmax);
      float s = sum[i] * expf(mx[i] - nmax);           // exp(-inf) = 0 at the first chunk
#pragma unroll
      for (int k = 0; k < kCrfChunk; ++k)
        if (k < nk) s += expf(l[k] - nmax);
      mx[i] = nmax;
      sum[i] = s;
    }
  }

  // normalise: every thread its own parked logits, classes in order; the last iteration takes the arg-max of Q (first maximum wins)
#pragma unroll
  for (int i = 0; i < kCrfOwn; ++i) {
    if (!own[i]) continue;
    const int64_t pix = (int64_t)(y0 + wave + kCrfWaves * i) * W + gx;
    float best = -1.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const int64_t at = (b * C + c) * HW + pix;
      const float q = expf(q_out[at] - mx[i]) / sum[i];
      if (write_q) q_out[at] = q;
      if (q > best) {
        best = q;
        arg = c;
      }
    }
    if (last) {
      labels[b * HW + pix] = lut ? lut[arg] : (uint8_t)arg;
      if (conf) conf[b * HW + pix] = best;
    }
  }
}

inline bool crf_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace dasac

extern "C" size_t dasac_crf_meanfield_workspace(int B, int C, int H, int W, int n_iter) {
  using namespace dasac;
  if (B <= 0 || C < 1 || C > kCrfMaxC || H <= 0 || W <= 0 || n_iter < 1 || n_iter > kCrfMaxIter) return 0;
  return (size_t)(n_iter < 2 ? 1 : 2) * crf_q_bytes(B, C, H, W);
}

extern "C" int dasac_crf_meanfield(const float* probs, const float* image, int B, int C, int Ci, int H, int W, int radius, int dilation,
                                   float w_app, float theta_alpha, float theta_beta, float w_smooth, float theta_gamma, float compat,
                                   int n_iter, const uint8_t* lut, uint8_t* labels, float* conf, float* probs_out, void* workspace,
                                   size_t ws_bytes, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(probs && image && labels && workspace, "crf_meanfield: null probs, image, labels or workspace");
  DASAC_REQUIRE(B > 0 && H > 0 && W > 0, "crf_meanfield: B, H and W must be positive");
  DASAC_REQUIRE(C >= 1 && C <= kCrfMaxC, "crf_meanfield: C must be in 1..%d", kCrfMaxC);
  DASAC_REQUIRE(Ci >= 1 && Ci <= kCrfMaxCi, "crf_meanfield: the image must have 1..%d channels", kCrfMaxCi);
  DASAC_REQUIRE(radius >= 1 && radius <= kCrfMaxRadius, "crf_meanfield: the radius must be in 1..%d", kCrfMaxRadius);
  DASAC_REQUIRE(dilation >= 1 && dilation <= kCrfMaxDilation && radius * dilation <= kCrfMaxHalo,
                "crf_meanfield: the dilation must be in 1..%d and radius * dilation at most %d", kCrfMaxDilation, kCrfMaxHalo);
  DASAC_REQUIRE(n_iter >= 1 && n_iter <= kCrfMaxIter, "crf_meanfield: n_iter must be in 1..%d", kCrfMaxIter);
  DASAC_REQUIRE(theta_alpha > 0.f && theta_beta > 0.f && theta_gamma > 0.f && std::isfinite(theta_alpha) && std::isfinite(theta_beta) &&
                    std::isfinite(theta_gamma),
                "crf_meanfield: theta_alpha, theta_beta and theta_gamma must be positive and finite");
  DASAC_REQUIRE(w_app >= 0.f && w_smooth >= 0.f && w_app + w_smooth > 0.f && std::isfinite(w_app) && std::isfinite(w_smooth),
                "crf_meanfield: w_app and w_smooth must be finite, >= 0 and not both 0");
  DASAC_REQUIRE(compat >= 0.f && std::isfinite(compat), "crf_meanfield: compat must be finite and >= 0");
  const size_t limit = (4ull << 30) - 4096;
  const size_t hw = (size_t)H * W;
  DASAC_REQUIRE(hw * B * C * sizeof(float) < limit && hw * B * Ci * sizeof(float) < limit,
                "crf_meanfield: every tensor must stay below 4 GiB - 4 KiB");
  const size_t q_bytes = hw * B * C * sizeof(float), i_bytes = hw * B * Ci * sizeof(float), m_bytes = hw * B;
  const uintptr_t align4 = reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(conf) |
                           reinterpret_cast<uintptr_t>(probs_out);
  DASAC_REQUIRE((align4 & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0,
                "crf_meanfield: fp32 tensors must be aligned to 4 bytes, the workspace to 16");
  const size_t need = dasac_crf_meanfield_workspace(B, C, H, W, n_iter);
  const void* ins[2] = {probs, image};
  const size_t in_bytes[2] = {q_bytes, i_bytes};
  const void* outs[4] = {labels, conf, probs_out, workspace};
  const size_t out_bytes[4] = {m_bytes, m_bytes * sizeof(float), q_bytes, need};
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 2; ++i)
      DASAC_REQUIRE(!crf_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "crf_meanfield: an output or the workspace overlaps an input");
    for (int p = o + 1; p < 4; ++p)
      DASAC_REQUIRE(!crf_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]), "crf_meanfield: outputs and workspace overlap each other");
  }
  if (ws_bytes < need) return fail(DASAC_EWORKSPACE, "crf_meanfield: workspace too small (%zu < %zu)", ws_bytes, need);

  const int halo = radius * dilation;
  const int ck = crf_chunk(C, Ci, halo);
  const size_t lds = crf_lds_bytes(Ci, ck, halo);
  DASAC_REQUIRE(ck >= 1 && lds <= kCrfLdsBudget, "crf_meanfield: the tile does not fit the LDS budget");
  const int tiles_x = (W + kCrfTileW - 1) / kCrfTileW, tiles_y = (H + kCrfTileH - 1) / kCrfTileH;
  DASAC_REQUIRE((int64_t)tiles_x * tiles_y * B <= 0x7fffffffll, "crf_meanfield: B * H * W too large for one launch");

  // the per-tap constants, in double: the spatial Gaussians, and w_app as a summand of the appearance exponent (base 2)
  CrfTaps taps = {};
  const double log2e = 1.4426950408889634;
  const double la = w_app > 0.f ? std::log2((double)w_app) : -INFINITY;
  int tap = 0;
  for (int a = -radius; a <= radius; ++a)
    for (int bb = -radius; bb <= radius; ++bb) {
      if (a == 0 && bb == 0) continue;
      const double o2 = (double)(a * a + bb * bb) * dilation * dilation;
      taps.app[tap] = (float)(la - o2 * log2e / (2.0 * theta_alpha * theta_alpha));
      taps.smooth[tap] = (float)(w_smooth * std::exp(-o2 / (2.0 * (double)theta_gamma * theta_gamma)));
      ++tap;
    }
  const float beta = (float)(-log2e / (2.0 * (double)theta_beta * theta_beta));

  float* q[2] = {static_cast<float*>(workspace),
                 reinterpret_cast<float*>(static_cast<uint8_t*>(workspace) + (n_iter < 2 ? 0 : crf_q_bytes(B, C, H, W)))};
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)(tiles_x * tiles_y * B)), block(kCrfBlock);
  const FastDiv div_pitch = fast_div(kCrfTileW + 2 * halo);
  const float* src = probs;
  for (int it = 1; it <= n_iter; ++it) {
    const int last = it == n_iter;
    float* dst = (last && probs_out) ? probs_out : q[(it - 1) & 1];
    const int write_q = !last || probs_out != nullptr;   // the last Q itself is wanted only as probs_out
#define DASAC_CRF_LAUNCH(CT, CIT, HT)                                                                                                  \
  hipLaunchKernelGGL((crf_iteration<CT, CIT, HT>), grid, block, lds, s, probs, image, src, dst, C, H, W, radius, dilation, ck, beta,      \
                     compat, taps, tiles_x, tiles_y, div_pitch, last, write_q, lut, labels, conf)
    if (C == 19 && Ci == 3) {                            // the shape of the project's own models: 19 classes over an RGB image
      if (halo == 5) {                                   // ... and the default window
        DASAC_CRF_LAUNCH(19, 3, 5);
      } else {
        DASAC_CRF_LAUNCH(19, 3, 0);
      }
    } else if (Ci == 1) {
      DASAC_CRF_LAUNCH(0, 1, 0);
    } else if (Ci == 2) {
      DASAC_CRF_LAUNCH(0, 2, 0);
    } else if (Ci == 3) {
      DASAC_CRF_LAUNCH(0, 3, 0);
    } else {
      DASAC_CRF_LAUNCH(0, 4, 0);
    }
#undef DASAC_CRF_LAUNCH
    DASAC_CHECK_LAUNCH("crf_iteration");
    src = dst;
  }
  return DASAC_OK;
}
