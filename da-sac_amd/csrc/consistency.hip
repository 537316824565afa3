// Label-free view consistency (dasac_view_consistency): how far the teacher's T aligned views of a target image agree, as exact
// integer tables -- a diagnostic the reference does not have.  The input is the tensor `warp_pool` writes for every target step,
// `teacher_aligned`: fp32 [N*T, C, HW] probabilities in the reference frame, zero where a view does not reach.
//
// Per group n, pixel p, view t (include/dasac_hip.h has the full definitions):
//   z_t = sum_c aligned[n,t,c,p]  fp32, ascending c          the view's bilinear coverage; covered when z_t >= cover
//   a_t = argmax_c aligned[n,t,c,p]                          first maximum wins (strict >)
//   c*  = argmax_c sum_t aligned[n,t,c,p]                    fp32, ascending t, ALL views (the pooled sum's own operands)
//   k   = covered views, m = covered views with a_t == c*
//   agree[c*][k][m] += 1 (k >= 1), agree[C][0][0] += 1 (k == 0); flips[a_t][a_u] += 1 per covered pair t < u;
//   per_view[t] += (covered, covered and a_t == c*)
//
// Streaming shape (as validation.hip): lanes along pixels, four consecutive pixels per thread, every (t, c) plane ONE
// dwordx4 load declared 4-byte aligned (at 769 x 769 the planes sit at every 4-byte phase); the last 1..3 pixels of an image are
// read element by element, so no load touches an element outside its own (n, t, c) plane.  The loop runs c outside, t inside: one
// pass gives z_t (ascending c) and the class sum S_c (ascending t) in their prescribed orders.  Live state: per view the running
// maximum, its arg-max and z_t; the running consensus maximum; the quad in flight.  No S[C] array, no scratch.
//
// Counting: integers only -- u32 LDS histograms per wave, one u64 global add per non-zero bin per block: exact, the same bits on
// every run.  A block takes at most 2^27 pixels, so a bin (a pixel adds up to 28 pairs at T = 8) stays below 2^32.  Label maps are
// a few large regions where every view agrees, so keys are merged before LDS: a thread whose four pixels share one `agree` key
// joins the wave-wide match of count_stream.hpp -- one lane adds 4 x (lanes holding the key), and, when that key says
// m == k, the k(k-1)/2 agreeing pairs of all those pixels with ONE add at flips[c*][c*].  Elsewhere a pixel whose covered views
// agree makes one flips add, and only a disagreeing pixel adds pair by pair.  per_view is kept in registers across the loop: the
// counts are taken wave-wide (ballots), so they are scalar registers and need no reduction at the end -- one LDS add per wave.
//
// Registers: C = 19 with T = 2 and T = 4 compiled in (the class loop in trips of a dozen loads: fully unrolled, all 76 loads are
// hoisted and spill); the runtime path (T <= 8, C <= 32) packs a view's four arg-maxes into one register.  Every load is "scalar
// plane base + 32-bit lane offset", which saves the 64-bit vector address per load in flight.  <= 128 VGPRs, four waves per SIMD.
#include "count_stream.hpp"

namespace dasac {

constexpr int kVcBlock = kCountBlock;                        // 4 waves, each with its own agree + flips histogram
constexpr int kVcWaves = kVcBlock / kWave;
constexpr int kVcMaxViews = DASAC_CONSISTENCY_MAX_VIEWS;
constexpr int kVcMaxC = 32;
constexpr int kVcBlocksPerCu = 2;                      // the grid aims at no fewer (profiles/view_consistency.md)
constexpr int64_t kVcMaxBlockQuads = 1ll << 25;        // 2^27 pixels x 28 pairs < 2^32: a block's u32 bins can not overflow

// TM views of four pixels: running maximum, arg-max (PACK: the four pixels' classes in the bytes of one register) and coverage sum
template <int TM, bool PACK>
struct VcViews {
  float best[TM][4], z[TM][4];
  unsigned arg[TM][PACK ? 1 : 4];
  float cmax[4];
  int carg[4];

  __device__ __forceinline__ int label(int t, int e) const { return PACK ? (int)((arg[t][0] >> (8 * e)) & 0xffu) : (int)arg[t][e]; }
  __device__ __forceinline__ void take(int t, int e, bool gt, int c) {
    if constexpr (PACK) {
      arg[t][0] = gt ? ((arg[t][0] & ~(0xffu << (8 * e))) | ((unsigned)c << (8 * e))) : arg[t][0];
    } else {
      arg[t][e] = gt ? (unsigned)c : arg[t][e];
    }
  }
};

// a block-uniform pointer, pinned to scalar registers: the compiler then keeps "scalar base + 32-bit lane offset" as the address of
// every load instead of folding the lane offset into one 64-bit vector address per plane (two more registers per load in flight)
#define VC_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ const VC_GLOBAL char* vc_scalar(const float* p) {
  const unsigned long long u = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return (const VC_GLOBAL char*)(((unsigned long long)hi << 32) | lo);
}

// class c of every view at one quad: p = plane (n, 0, c), the same for the whole block, views `view_stride` apart; `off` = the
// quad's first pixel in BYTES (HW < 2^30), so every load is a scalar base plus one 32-bit lane offset
template <int TM, bool PACK, bool FULL, bool FIRST>
__device__ __forceinline__ void vc_class(VcViews<TM, PACK>& s, const float* __restrict__ p, unsigned off, int T, int64_t view_stride,
                                         int nx, int c) {
  // FULL: one 16-byte load per plane.  Otherwise element by element, an absent pixel reading the quad's last present one again (its
  // value is never counted): no branch around a load, and no load outside the plane
  unsigned off1 = off + (nx > 1 ? 4u : 0u), off2 = off + (nx > 2 ? 8u : nx > 1 ? 4u : 0u);
  asm volatile("" : "+v"(off));                      // keeps the 32-bit offsets' widening next to their loads (see vc_scalar)
  if constexpr (!FULL) asm volatile("" : "+v"(off1), "+v"(off2));
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < TM; ++t)
    if (t < T) {
      const VC_GLOBAL char* tp = vc_scalar(p + t * view_stride);
      f32x4u v = f32x4u{0.f, 0.f, 0.f, 0.f};
      if constexpr (FULL) {
        v = *(const VC_GLOBAL f32x4u*)(tp + off);
      } else {
        v[0] = *(const VC_GLOBAL float*)(tp + off);
        v[1] = *(const VC_GLOBAL float*)(tp + off1);
        v[2] = *(const VC_GLOBAL float*)(tp + off2);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sum[e] = t == 0 ? v[e] : sum[e] + v[e];        // ascending t
        if constexpr (FIRST) {
          s.z[t][e] = v[e];
          s.best[t][e] = v[e];
        } else {
          s.z[t][e] += v[e];                           // ascending c
          const bool gt = v[e] > s.best[t][e];
          s.best[t][e] = gt ? v[e] : s.best[t][e];
          s.take(t, e, gt, c);
        }
      }
      if constexpr (FIRST) {
#pragma unroll
        for (int e = 0; e < (PACK ? 1 : 4); ++e) s.arg[t][e] = 0u;
      }
    }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (FIRST) {
      s.cmax[e] = sum[e];
      s.carg[e] = 0;
    } else if (sum[e] > s.cmax[e]) {
      s.cmax[e] = sum[e];
      s.carg[e] = c;
    }
  }
}

template <int CT, int TM, bool PACK, bool FULL>
__device__ __forceinline__ void vc_scan(VcViews<TM, PACK>& s, const float* __restrict__ p, unsigned off, int C, int T, int64_t HW,
                                        int nx) {
  const int64_t view_stride = (int64_t)C * HW;
  vc_class<TM, PACK, FULL, true>(s, p, off, T, view_stride, nx, 0);
  if constexpr (CT > 0) {
    // a dozen quads in flight per trip: unrolled over all classes the loads are hoisted together and their registers spill
    constexpr int kStep = TM <= 2 ? 6 : 3;
    static_assert((CT - 1) % kStep == 0, "the class loop takes whole trips");
#pragma unroll 1
    for (int c0 = 1; c0 < CT; c0 += kStep) {
#pragma unroll
      for (int i = 0; i < kStep; ++i) vc_class<TM, PACK, FULL, false>(s, p + (int64_t)(c0 + i) * HW, off, T, view_stride, nx, c0 + i);
    }
  } else {
    for (int c = 1; c < C; ++c) vc_class<TM, PACK, FULL, false>(s, p + (int64_t)c * HW, off, T, view_stride, nx, c);
  }
}

// the covered pairs of one pixel whose covered views (bits of `cm`; labels in the bytes of `lab`) are not all c*
__device__ __forceinline__ void vc_pairs(unsigned int* __restrict__ hf, unsigned long long lab, unsigned cm, int C) {
  const int k = __popc(cm);
  const unsigned first = (unsigned)(lab >> (8 * (__ffs((int)cm) - 1))) & 0xffu;
  bool same = true;
  for (unsigned r = cm; r; r &= r - 1) same = same && ((unsigned)(lab >> (8 * (__ffs((int)r) - 1))) & 0xffu) == first;
  if (same) {                                          // the views agree on a class the consensus did not take (rim weights)
    atomicAdd(&hf[first * C + first], (unsigned)(k * (k - 1) / 2));
    return;
  }
  for (unsigned r = cm; r; r &= r - 1) {
    const unsigned at = (unsigned)(lab >> (8 * (__ffs((int)r) - 1))) & 0xffu;
    for (unsigned u = r & (r - 1); u; u &= u - 1) atomicAdd(&hf[at * C + ((unsigned)(lab >> (8 * (__ffs((int)u) - 1))) & 0xffu)], 1u);
  }
}

// grid: N * blocks_per_group blocks; block (n, j) takes quads [j * per, (j + 1) * per) of group n (quad = 4 consecutive pixels).
// dynamic LDS: (kVcWaves * ((C+1)(T+1)^2 + C^2) + 2T) * 4 bytes
template <int CT, int TT>
__global__ __launch_bounds__(kVcBlock) void view_consistency(const float* __restrict__ aligned, int Crt, int Trt, int64_t HW,
                                                             int blocks_per_group, int64_t per, float cover,
                                                             unsigned long long* __restrict__ agree,
                                                             unsigned long long* __restrict__ flips,
                                                             unsigned long long* __restrict__ per_view) {
  extern __shared__ unsigned int s_vc[];
  constexpr int TM = TT > 0 ? TT : kVcMaxViews;
  constexpr bool PACK = TT == 0;
  const int C = CT > 0 ? CT : Crt;
  const int T = TT > 0 ? TT : Trt;
  const int side = T + 1;
  const int n_agree = (C + 1) * side * side, n_flips = C * C, n_wave = n_agree + n_flips;
  for (int i = threadIdx.x; i < kVcWaves * n_wave + 2 * T; i += kVcBlock) s_vc[i] = 0;
  __syncthreads();

  // the division runs on the vector unit: back to a scalar register, or every plane pointer derived from it becomes a vector pair
  const int64_t n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)blocks_per_group));
  const int j = (int)(blockIdx.x - n * blocks_per_group);
  const int64_t n_quads = (HW + 3) >> 2;
  const unsigned q0 = (unsigned)(j * per);               // quads fit 32 bits (HW < 2^30), and so do their byte offsets in a plane
  const unsigned q1 = (unsigned)(q0 + per > n_quads ? n_quads : q0 + per);
  const float* group = aligned + n * T * C * HW;
  unsigned int* ha = s_vc + (int)(threadIdx.x >> 6) * n_wave;
  unsigned int* hf = ha + n_agree;
  unsigned int* hv = s_vc + kVcWaves * n_wave;
  const int lane = (int)(threadIdx.x & (kWave - 1));

  // per_view: wave-wide counts (ballots), the same in every lane of the wave -- scalar registers across the loop.  The loop is
  // therefore the same for all lanes: a lane past the block's last quad runs it with nx = 0, which loads and counts nothing
  unsigned pv_cov[TM], pv_hit[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) pv_cov[t] = pv_hit[t] = 0u;

  for (unsigned qb = q0; qb < q1; qb += kVcBlock) {
    const unsigned q = qb + threadIdx.x;
    const int64_t left = HW - ((int64_t)q << 2);
    const int nx = q >= q1 ? 0 : left >= 4 ? 4 : (int)left;      // 1..4 inside: q < ceil(HW / 4)
    VcViews<TM, PACK> s;
    if (nx == 4) {
      vc_scan<CT, TM, PACK, true>(s, group, q << 4, C, T, HW, nx);
    } else {
      vc_scan<CT, TM, PACK, false>(s, group, nx ? q << 4 : 0u, C, T, HW, nx);      // nx = 0 reads pixel 0 and counts nothing
    }

    int key[4], kk[4], mm[4];
    unsigned cm[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cm[e] = 0u;
      mm[e] = 0;
#pragma unroll
      for (int t = 0; t < TM; ++t)
        if (t < T) {
          const bool cov = e < nx && s.z[t][e] >= cover;
          const bool hit = cov && s.label(t, e) == s.carg[e];
          cm[e] |= cov ? 1u << t : 0u;
          mm[e] += hit ? 1 : 0;
          pv_cov[t] += (unsigned)__popcll(__ballot(cov));
          pv_hit[t] += (unsigned)__popcll(__ballot(hit));
        }
      kk[e] = __popc(cm[e]);
      key[e] = e >= nx ? -1 : kk[e] == 0 ? C * side * side : (s.carg[e] * side + kk[e]) * side + mm[e];
    }

    const bool merged = key[1] == key[0] && key[2] == key[0] && key[3] == key[0] && key[0] >= 0;
    if (merged) {
      // one add per distinct key of the wave, and one for its unanimous pairs
      bool leader;
      const unsigned count = 4u * wave_match(key[0], leader);
      const unsigned pairs = mm[0] == kk[0] ? (unsigned)(kk[0] * (kk[0] - 1) / 2) : 0u;
      if (leader) {
        atomicAdd(&ha[key[0]], count);
        if (pairs) atomicAdd(&hf[s.carg[0] * C + s.carg[0]], count * pairs);
      }
    } else {
      count_runs4(ha, key);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (kk[e] >= 2) {
        if (mm[e] == kk[e]) {
          if (!merged) atomicAdd(&hf[s.carg[e] * C + s.carg[e]], (unsigned)(kk[e] * (kk[e] - 1) / 2));
        } else {
          unsigned long long lab = 0ull;
#pragma unroll
          for (int t = 0; t < TM; ++t)
            if (t < T) lab |= (unsigned long long)s.label(t, e) << (8 * t);
          vc_pairs(hf, lab, cm[e], C);
        }
      }
  }

#pragma unroll
  for (int t = 0; t < TM; ++t)
    if (t < T) {
      if (lane == 0) {
        if (pv_cov[t]) atomicAdd(&hv[2 * t], pv_cov[t]);
        if (pv_hit[t]) atomicAdd(&hv[2 * t + 1], pv_hit[t]);
      }
    }

  __syncthreads();
  for (int i = threadIdx.x; i < n_wave; i += kVcBlock) {      // not flush_bins: agree and flips are one table here, two outside
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kVcWaves; ++w) sum += s_vc[w * n_wave + i];
    if (sum) atomicAdd(i < n_agree ? &agree[i] : &flips[i - n_agree], sum);
  }
  flush_bins(hv, 1, 0, 2 * T, per_view);
}

}  // namespace dasac

extern "C" int dasac_view_consistency(const float* aligned, int N, int T, int C, int64_t HW, float cover, int64_t* agree,
                                      int64_t* flips, int64_t* per_view, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(aligned && agree && flips && per_view, "view_consistency: null aligned, agree, flips or per_view");
  DASAC_REQUIRE(T >= 1 && T <= kVcMaxViews, "view_consistency: T must be in 1..%d", kVcMaxViews);
  DASAC_REQUIRE(C >= 1 && C <= kVcMaxC, "view_consistency: C must be in 1..%d", kVcMaxC);
  DASAC_REQUIRE(N > 0 && HW > 0 && HW < (1ll << 30) && (int64_t)N * T < (1ll << 31), "view_consistency: bad shape");
  DASAC_REQUIRE((reinterpret_cast<uintptr_t>(aligned) & 3u) == 0 && (reinterpret_cast<uintptr_t>(agree) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(flips) & 7u) == 0 && (reinterpret_cast<uintptr_t>(per_view) & 7u) == 0,
                "view_consistency: fp32 / int64 tensors must be aligned to their element size");
  // whole quads per thread: as many as still leave kVcBlocksPerCu blocks per CU (measured: two quads per thread in 512-578 blocks
  // beat one in twice as many and three in fewer), never more than keep a block's u32 bins exact
  const int64_t n_quads = (HW + 3) >> 2;
  const int64_t fill = ((int64_t)(kNumCu - reserved_cus()) * kVcBlocksPerCu + N - 1) / N;
  int64_t per = n_quads / (fill * kVcBlock);
  per = (per < 1 ? 1 : per) * kVcBlock;
  if (per > kVcMaxBlockQuads) per = kVcMaxBlockQuads;
  const int64_t bpg = (n_quads + per - 1) / per;
  DASAC_REQUIRE(bpg * N <= 0x7fffffffll, "view_consistency: N * HW too large for one launch");
  const size_t lds = ((size_t)kVcWaves * ((size_t)(C + 1) * (T + 1) * (T + 1) + (size_t)C * C) + 2 * (size_t)T) * sizeof(unsigned int);
  const dim3 grid((unsigned)(bpg * N)), block(kVcBlock);
  unsigned long long* out_a = reinterpret_cast<unsigned long long*>(agree);
  unsigned long long* out_f = reinterpret_cast<unsigned long long*>(flips);
  unsigned long long* out_v = reinterpret_cast<unsigned long long*>(per_view);
#define DASAC_VC_LAUNCH(CT, TT)                                                                                                   \
  hipLaunchKernelGGL((view_consistency<CT, TT>), grid, block, lds, as_stream(stream), aligned, C, T, HW, (int)bpg, per, cover,   \
                     out_a, out_f, out_v)
  if (C == 19 && T == 4) DASAC_VC_LAUNCH(19, 4);
  else if (C == 19 && T == 2) DASAC_VC_LAUNCH(19, 2);
  else DASAC_VC_LAUNCH(0, 0);
#undef DASAC_VC_LAUNCH
  DASAC_CHECK_LAUNCH("view_consistency");
  return DASAC_OK;
}
