// Implicit-GEMM convolution on the gfx950 matrix cores: exact fp32 (v_mfma_f32_32x32x2_f32, the default) or,
// opt-in per call (template flag X3), split-bf16 products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
//
// Replaces every nn.Conv2d call of the reference backbone (models/deeplabv2.py:59,65-66,70,107,
// 122,147-148,262-263; models/fcn.py:49,53,57,78,88) -- 1x1, dilated 3x3, 7x7/2 stem, and the
// four-branch ASPP sum as ONE contraction -- for forward, data-gradient and weight-gradient.
// This file: the forward / data-gradient GEMM with its three schedules.  conv_wgrad.hip: the weight gradient; conv_pack.hip: the gather
// table and the weight packers; conv_expanded.hip: the tap-expanded ASPP path; conv_common.hpp: what they share.  Which schedule a
// launch gets, its grid and its workspace (gemm_plan) and the block maps of the three schedules are conv_plan.hpp's: plain C++,
// compared with tests/gemm_schedule_ref.py and walked block by block on the host by tools/conv_plan_check.cpp.
//
//   forward / dgrad :  Out[m][pix] = sum_k  Wp[k][m] * gather(X, k, pix)        (conv_gemm)
//   wgrad           :  G[m][k]     = sum_pix dZ[m][pix] * gather(X, k, pix)     (conv_wgrad)
//
// `gather` is table driven: row k of the im2col matrix is (channel plane offset, dh, dw), so one
// kernel covers any kernel size / dilation / padding / multi-branch layout; the table row is
// wave-uniform (scalar loads), lanes run along pixels (coalesced NCHW reads).  Tiles go through
// LDS (k-interleaved 16-byte words, one conflict-free ds_read_b128 per operand and 4 MFMAs), register-staged
// double buffering: the global loads of K-step t+1 are in flight while the MFMAs of step t issue.  The BN(eval) scale/shift, bias, residual add, ReLU and the ReLU-mask of the backward
// pass are folded into the epilogue ("ABN": conv+BN+ReLU in one pass, no extra HBM round trip).
//
// Roofline: MFMA-bound, 2*M*Npix*K flops per launch against the 157.3 TFLOP/s fp32 matrix peak
// (X3: three bf16 MFMAs per product -> 2500/3 TFLOP/s equivalent; today limited by the fp32 -> LDS staging).
#include "conv_common.hpp"

#include <atomic>
#include <type_traits>

namespace dasac {

#ifdef DASAC_TRACE_TILES
// Diagnostic build only (tools/tile_timeline.py): per tile-per-block workgroup four s_memtime stamps -- start, first tile in LDS,
// end of the K loop, end of the epilogue -- plus the hardware XCC / CU ids.  Never part of the shipped library.
__device__ unsigned long long* g_tile_trace = nullptr;
__device__ __forceinline__ void trace_stamp(int slot) {
  if (g_tile_trace && threadIdx.x == 0) g_tile_trace[(size_t)blockIdx.x * 8 + slot] = __builtin_amdgcn_s_memtime();
}
#define DASAC_STAMP(slot) trace_stamp(slot)
#else
#define DASAC_STAMP(slot)
#endif

struct Epilogue {
  const float* shift;   // [M] or null (the BN scale is folded into the packed weights)
  const float* res;     // same layout as out, or null  (added before ReLU)
  const float* mask;    // same layout as out, or null  (out = mask>0 ? out : 0, ReLU backward)
  int relu;
  // ReLU pattern as ONE BIT per element instead of a whole fp32 activation read back only to test `> 0`:
  //   bits[m][pix >> 5] bit (pix & 31), pix = flattened (n, oh, ow) index of the GEMM's pixel axis, w32 = ceil(Npix / 32) words
  //   per row.  A 32-pixel group of a tile is 32-aligned (tiles start at multiples of 128), so every word belongs to exactly one
  //   wave: the producer (forward conv with ReLU) writes obits from wave ballots, the consumer (the data-gradient GEMM whose
  //   output has the producer's shape) reads mbits -- 1/32 of the fp32 mask's bytes.
  const unsigned* mbits;   // consumer: out = bit ? out : 0    (exclusive with `mask`)
  unsigned* obits;         // producer: bit = out > 0 (after ReLU); ostride must be 1
  int w32;
  // BITS == 3 (batch-statistics BatchNorm behind this conv, deeplabv2.py:15 in baseline / AdaBN mode): the epilogue also
  // leaves, per 128-pixel tile, the per-channel sum and sum of squares of what it stores -- stats[pixel tile][0|1][Mpad] --
  // so that the stand-alone statistics pass over z (one full read of the activation per BN layer) disappears.  Every slot
  // of a tile is written by exactly one workgroup; a fixed-order sum over the tiles follows (bn_train_finalize): deterministic.
  float* stats;
};

// BITS == 4 (batched launch: the 16 point GEMMs of a Winograd convolution as ONE grid, blockIdx.y = batch entry): `batch`
// independent GEMMs of identical geometry whose operands lie `*_stride` ELEMENTS apart.  No epilogue operands at all.  Its own
// parameter type, so that the kernel arguments -- and with them the code -- of every other instantiation stay what they were.
struct BatchedEpilogue : Epilogue {
  int64_t x_stride, w_stride, out_stride;
};

// v_writelane_b32 (this clang exposes no __builtin_amdgcn_writelane; the LLVM intrinsic is reachable through its asm label, the way
// the HIP headers reach llvm.amdgcn.s.barrier).  Rounds 3-4 emitted the instruction from inline asm, which hides it from the
// hazard recogniser: gfx940+ needs two wait states between a VALU that writes an SGPR (the ballot's v_cmp) and a VALU that reads it,
// and only instruction-scheduling luck had put them there.  put_mask_rows: the two 32-bit halves of a wave ballot over accumulator
// register `rg` are the mask words of rows (rg&3) + 8*(rg>>2) (lanes 0-31) and 4 below (lanes 32-63) of a 32x32 MFMA tile: lane r
// of `acc` collects row r.
// Toolchain note: a compiler that has the builtin uses it; otherwise the intrinsic's overloaded name
// `llvm.amdgcn.writelane.i32` is the one of LLVM 19+ (ROCm >= 6.3; this image: ROCm 7.2) -- older toolchains spell it
// `llvm.amdgcn.writelane` and are not supported by this build ("toolchain").
#if __has_builtin(__builtin_amdgcn_writelane)
template <int LANE>
__device__ __forceinline__ int writelane_c(int val, int old) {
  return __builtin_amdgcn_writelane(val, LANE, old);
}
#else
extern "C" __device__ int dasac_llvm_writelane(int val, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
template <int LANE>
__device__ __forceinline__ int writelane_c(int val, int old) {
  return dasac_llvm_writelane(val, LANE, old);
}
#endif
__device__ __forceinline__ int put_mask_rows(int rg, unsigned long long ballot, int acc) {
  const int lo = (int)(unsigned)ballot, hi = (int)(unsigned)(ballot >> 32);
  switch (rg) {      // rg is the index of a fully unrolled loop: the switch folds to one case
#define DASAC_ROW_(RG)                                               \
  case RG:                                                           \
    acc = writelane_c<(RG & 3) + 8 * (RG >> 2)>(lo, acc);            \
    acc = writelane_c<(RG & 3) + 8 * (RG >> 2) + 4>(hi, acc);        \
    break;
    DASAC_ROW_(0) DASAC_ROW_(1) DASAC_ROW_(2) DASAC_ROW_(3) DASAC_ROW_(4) DASAC_ROW_(5) DASAC_ROW_(6) DASAC_ROW_(7)
    DASAC_ROW_(8) DASAC_ROW_(9) DASAC_ROW_(10) DASAC_ROW_(11) DASAC_ROW_(12) DASAC_ROW_(13) DASAC_ROW_(14) DASAC_ROW_(15)
#undef DASAC_ROW_
  }
  return acc;
}

// sum over the 32 lanes of a half-wave (all of them end up with it): four DPP adds inside each row of 16 lanes (quad
// permutes, half-row and row mirrors) and one cross-row exchange
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float half_wave_sum(float v) {
  v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);     // row_half_mirror
  v = dpp_add<0x140>(v);     // row_mirror
  return v + __shfl_xor(v, 16, 64);
}

// ------------------------------------------------------------------------------------------
// forward / dgrad kernel
// ------------------------------------------------------------------------------------------
// LDS tiles are k-interleaved: element (k, x) of a K-step lives at [(k/4)][x][k%4], so that
//   * the packed weights (stored the same way in HBM, see pack_weights) move global->LDS as 16-byte words,
//   * a thread that gathered 4 consecutive k rows of one pixel stores them with one ds_write_b128,
//   * one ds_read_b128 per operand feeds FOUR MFMAs: lane (i, h) reads k = 8g + 4h + {0..3} and MFMA
//     j of the group contracts the k pair {8g + j, 8g + 4 + j} (any pairing is valid as long as the A
//     and B operands agree) -- 8 LDS reads per 32 MFMAs instead of 32.
// FAST: the gathered tensor's channel count is a multiple of BK, so a K-step never straddles two
// taps: one (dh, dw) per step, validity and the spatial offset computed once per thread and step, the
// channel offset of each row rides in the scalar operand (zero VALU per gathered element).
// STREAMK: persistent launch (3 workers per CU).  The (tile, K-step) iteration space is cut into equal
// contiguous ranges, one per worker, so every CU gets the same amount of matrix work no matter how the
// tile count divides by the CU count (1178 tiles on 256 CUs would otherwise run 5 "rounds" for 4.6 of
// work).  A tile cut by a range boundary is finished by the worker holding its FIRST K-steps (it reaches
// them last); the other worker deposits its accumulators in `partial` as soon as it has them -- the tile segment a
// range starts with is the first thing it computes, before it waits for anything itself, so no co-residency of all
// workers is required -- and raises a flag.  The hand-off is placement independent (the per-XCD L2s are not coherent):
// deposits are written with agent-scope (sc1, write-through) 16-byte stores and read with sc1 loads, the flag is an
// agent-scope atomic that its single consumer resets (self-cleaning: no memset between launches).
// BITS: 0 = fp32 epilogue operands only; 1 = the ReLU epilogue also records its pattern as bits (Epilogue::obits);
//       2 = the epilogue masks with a recorded bit pattern (Epilogue::mbits).  Separate instantiations, so that the plain
//       kernels carry none of the extra scalar state.  3 = per-tile channel statistics (Epilogue::stats); 4 = batched launch of the
//       plain tile-per-block kernel (BatchedEpilogue): the three operand bases advance by blockIdx.y strides at the very top, the
//       buffer-descriptor extents stay those of ONE entry, so inside an entry every offset is the one the single launch forms.
// SK: 0 = one block per tile; 1 = persistent stream-K (above); 2 = one block per tile for the leading whole rounds of resident
//     blocks AND, in the same launch, the remaining `tail_tiles` tiles cut into `tail_split` K-ranges of one block each (round 6).
//     A cut tile's pieces with the LATER K-steps carry the lower block ids -- blocks are dispatched in id order, so they are resident
//     or done before the piece with the first K-steps (the owner: it adds their deposits and runs the epilogue) even starts, and
//     they wait for nothing: progress needs no co-residency.  Same sc1 deposits and self-cleaning flags as the persistent kernel,
//     but at the plain kernel's four blocks per CU (a piece is ONE tile segment: no loop over segments, deposits read a quarter
//     at a time) and without a second launch: the tail's ramp hides behind the last full round's stragglers.
template <int BM, int BN, int WAVES_M, int BK, bool FAST, int SK, bool X3, int BITS = 0>
__global__ __launch_bounds__(kThreads, SK == 1 ? kSkWorkersPerCu : 4) void conv_gemm(const float* __restrict__ X, const float* __restrict__ Wp,
                                                      const int4* __restrict__ tab, float* __restrict__ Out, GemmGeom g,
                                                      std::conditional_t<BITS == 4, BatchedEpilogue, Epilogue> ep, int m_tiles, int n_tiles,
                                                      float* __restrict__ partial, int* __restrict__ flags, int tail_tiles, int tail_split) {
  constexpr bool STREAMK = SK == 1;      // persistent: a worker loops over tile segments
  constexpr bool TAIL = SK == 2;
  constexpr bool HANDOFF = STREAMK || TAIL;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int KQ = BK / 4;                                // k quads per K-step
  constexpr int A_VEC = KQ * BM;                             // 16-byte words per weight tile
  constexpr int A_PER_T = (A_VEC + kThreads - 1) / kThreads;
  constexpr int B_Q_PASS = kThreads / BN > 0 ? kThreads / BN : 1;   // k quads covered by one pass of the block
  constexpr int B_QUADS = KQ / B_Q_PASS;                     // quads (of 4 rows) gathered per thread
  constexpr int ACC_REGS = TM * TN * 16;
  static_assert(TM >= 1 && TN >= 1 && BN <= kThreads && KQ % B_Q_PASS == 0, "tile shape");
  static_assert(!X3 || (BK == 16 && BN == 128), "split-bf16 path: one 16-deep MFMA block per K-step, a k octet per thread");
  static_assert(BITS != 4 || (SK == 0 && FAST && !X3 && BM == 128), "batched launch: the plain fp32 tile-per-block kernel only");
  if constexpr (BITS == 4) {
    // workgroup-uniform, 64-bit: entry b's tensors; everything below sees one entry exactly as a single launch would
    const int64_t b = blockIdx.y;
    X += b * ep.x_stride;
    Wp += b * ep.w_stride;
    Out += b * ep.out_stride;
  }

  __shared__ f32x4 sA[2][KQ * BM];
  __shared__ f32x4 sB[2][KQ * BN];
  // Epilogue operands that are per ROW (shift) or per row and 32-pixel group (mask words) wait in LDS from the tile's prologue
  // on: the epilogue then contains no vector-memory load except the residual's.  That matters because gfx9's vmcnt retires
  // loads AND stores in issue order -- a wait for any load issued after a store is also a wait for that store's
  // acknowledgement; rounds 1-4 interleaved 8 batches of (loads, 8 stores) and paid 8 store round trips per tile
  // (28-36 us of a 91 us workgroup life on the K = 256 layers, profiles/r3_tile_timeline.txt).
  __shared__ __attribute__((aligned(16))) float s_shift[BM];
  // byte offset of (image, oh, ow) of each of the tile's BN pixel columns inside one output row, or the poison offset: formed in
  // the prologue next to the gather's own pixel decode (the same two integer divisions), read back by the epilogue -- whose
  // instructions are only served where the co-resident K-loop waves stall, ~20 per microsecond (profiles/r5_epilogue_anatomy.txt)
  __shared__ unsigned s_vo[BN];
  __shared__ __attribute__((aligned(16))) unsigned s_mbits[BITS == 2 ? (BN / 32) * BM : 4];   // [32-pixel group][row]

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform on purpose: scalar buffer offsets
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(X, g.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(Wp, g.w_bytes);

  const int OHW = g.OH * g.OW;
  const int planeHW = g.H * g.W;
  const int bcol = t % BN;
  const int bq0 = __builtin_amdgcn_readfirstlane(t / BN);    // wave-uniform first quad
  const int a_step_bytes = KQ * g.Mpad * 16;
  const int KT = g.Kpad / BK;
  const int OutHW = g.OutH * g.OutW;
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(Out, g.out_bytes);
  const __amdgpu_buffer_rsrc_t rres = make_rsrc(ep.res ? ep.res : Out, g.out_bytes);
  const __amdgpu_buffer_rsrc_t rmsk = BITS == 2 ? make_rsrc(ep.mbits, g.M * ep.w32 * 4) : make_rsrc(ep.mask ? ep.mask : Out, g.out_bytes);
  const __amdgpu_buffer_rsrc_t rsh = make_rsrc(ep.shift ? ep.shift : Out, ep.shift ? g.M * 4 : 0);
  const bool ragged = (g.M & 7) != 0;
  const __amdgpu_buffer_rsrc_t rpart = make_rsrc(HANDOFF ? (const void*)partial : (const void*)Out,
                                                 HANDOFF ? (STREAMK ? kSkWorkers : kTailSlots) * ACC_REGS * kThreads * 4 : 0);

  // ---- which part of the iteration space is mine --------------------------------------------
  // one block per tile (SK == 0): conv_plan.hpp's map.  The two hand-off schedules keep their maps written out below: on the header's
  // functions a timing row of each missed (profiles/conv_plan.md); tests/gemm_schedule_ref.py restates them.
  // (written as one initialiser and one return at this level, not inside `if constexpr (SK == 0)`: only so do all instantiations
  // keep the instruction streams they had with the map written inline, profiles/conv_plan.md section 3)
  const GemmWork tile_work = SK == 0 ? gemm_tile_work(blockIdx.x, m_tiles, n_tiles, KT) : GemmWork{true, 0, 0};
  if (!tile_work.has_work) return;
  // block b runs on XCD b%8: tiles (or ranges) that are adjacent -- same activation tile, next M tile --
  // go to the same XCD so that they share its L2.
  const int bid = blockIdx.x;
  const int xcd = bid % kNumXcd, slot = bid / kNumXcd;
  int it, it_end;                                            // (tile, K-step) space: tiles*KT < 2^31 (checked by the host)
  int my_range = 0;
  // stream-K ranges: G workers (= gridDim.x: 3 per CU on all CUs, or on fewer when CUs are left to overlapped collectives,
  // dasac_set_reserved_cus) split the (tile, K-step) space into contiguous ranges of sk_per or sk_per + 1 steps
  // (the first sk_rem ranges get the extra one): range r starts at r * sk_per + min(r, sk_rem)
  int sk_per = 0, sk_rem = 0;
  auto sk_start = [&](int r) { return r * sk_per + min(r, sk_rem); };
  if (SK == 0) {
    it = tile_work.it;
    it_end = tile_work.it_end;
  } else if (STREAMK) {
    const int G = gridDim.x;
    my_range = xcd * (G / kNumXcd) + slot;
    const int sk_total = m_tiles * n_tiles * KT;             // < 2^31 (checked by the host)
    sk_per = sk_total / G;
    sk_rem = sk_total - sk_per * G;
    it = sk_start(my_range);
    it_end = sk_start(my_range + 1);
  } else {
    // each XCD owns a CONTIGUOUS run of pixel tiles (spatial neighbours share halo rows in its L2)
    const int per_xcd = (n_tiles + kNumXcd - 1) / kNumXcd;
    const int lead_blocks = per_xcd * kNumXcd * m_tiles;       // == gridDim.x without a tail
    if (bid < lead_blocks) {
      const int n_local = slot / m_tiles;
      const int n_tile = xcd * per_xcd + n_local;
      if (n_local >= per_xcd || n_tile >= n_tiles) return;
      it = (n_tile * m_tiles + slot % m_tiles) * KT;
      it_end = it + KT;
    } else {
      // tail piece q: K-range `part` (later ranges first) of tail tile tr; the tail tiles follow the n_tiles leading pixel tiles;
      // runs of adjacent tiles (the M tiles of a pixel tile, neighbouring pixel tiles) go to one XCD, like the leading part
      const int q = bid - lead_blocks;
      const int per_x = (tail_tiles + kNumXcd - 1) / kNumXcd;
      const int part_rev = q / (per_x * kNumXcd), ql = q - part_rev * (per_x * kNumXcd);
      const int tl = ql / kNumXcd;                             // ql % kNumXcd == xcd (lead_blocks and per_x * kNumXcd are multiples of 8)
      const int tr = xcd * per_x + tl;
      if (tr >= tail_tiles) return;
      const int part = tail_split - 1 - part_rev;
      const int tile = n_tiles * m_tiles + tr;
      // balanced K-ranges: part p holds steps [p*KT/s, (p+1)*KT/s)
      it = tile * KT + part * KT / tail_split;                 // (KT <= 2^15 or so: no overflow)
      it_end = tile * KT + (part + 1) * KT / tail_split;
      my_range = tr * (tail_split - 1) + part - 1;             // deposit / flag slot of a non-owner piece (part >= 1)
    }
  }

  // (a do-while whose back edge exists only in the persistent variant: the tile-per-block kernel runs the body once -- it returned
  // above if it has no tile --, and the compiler must SEE that, or every K-loop invariant stays live across the epilogue
  // and its register pressure pushes them into spill slots that are then re-read inside the K loop)
  do {
    const int tile = it / KT;
    const int ks = it - tile * KT;
    const int ke = min(KT, ks + (it_end - it));
    it += ke - ks;
    const int m0 = (tile % m_tiles) * BM, n0 = (g.n_tile0 + tile / m_tiles) * BN;

    // ---- this thread's pixel column of the gather -------------------------------------------
    int pixbase, ih0, iw0;
    unsigned pro_vo = kPoison;
    {
      const int pix = n0 + bcol;
      if (pix < g.Npix) {
        const int n = pix / OHW, r = pix - n * OHW;
        const int oh = r / g.OW, ow = r - oh * g.OW;
        ih0 = oh * g.stride;
        iw0 = ow * g.stride;
        pixbase = n * g.CxHW + ih0 * g.W + iw0;
        pro_vo = (unsigned)(n * g.M * OutHW + oh * g.ostride * g.OutW + ow * g.ostride) * 4u;
      } else {
        ih0 = -kInvalid;     // every tap out of bounds -> poison offsets -> zeros
        iw0 = 0;
        pixbase = 0;
      }
    }
    // weight tile: per-thread byte offsets inside a K-step, the K-step itself goes in the scalar offset
    unsigned voff_a[A_PER_T];
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int v = t + i * kThreads;
      const int q = v / BM, m = v - q * BM;
      voff_a[i] = (unsigned)(q * g.Mpad + m0 + m) * 16u;
    }

    f32x4 ra[A_PER_T];
    f32x4 rb[B_QUADS];

#define DASAC_LOAD_TILE(kt)                                                                          \
  {                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < A_PER_T; ++i) {                                            \
      if (A_VEC % kThreads == 0 || t + i * kThreads < A_VEC) ra[i] = buf_f32x4(rw, voff_a[i], (kt) * a_step_bytes); \
    }                                                                                                \
    if (FAST) {                                                                                      \
      const int4 e = tab[(kt) * BK]; /* one tap per K-step: (koff, dh, dw, channel offset) */        \
      const int ih = ih0 + e.y, iw = iw0 + e.z;                                                      \
      const bool ok = ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);               \
      /* the K-step's tap and first channel plane ride in the per-lane offset (one VALU add); what is left for the */ \
      /* scalar operand -- the row's plane within the step -- is loop invariant: no scalar arithmetic per load      */ \
      const unsigned voff = ok ? (unsigned)(pixbase + e.x) * 4u : kPoison;                           \
      _Pragma("unroll") for (int r = 0; r < B_QUADS; ++r) {                                          \
        const int row0 = X3 ? 8 * bq0 + 4 * r : 4 * (bq0 + r * B_Q_PASS);                            \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                \
          rb[r][j] = buf_f32(rx, voff, (row0 + j) * planeHW * 4);                                    \
      }                                                                                              \
    } else {                                                                                         \
      int4 te[B_QUADS * 4]; /* all table rows of this K-step first: one batch of scalar loads */     \
      _Pragma("unroll") for (int r = 0; r < B_QUADS; ++r)                                            \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                \
          te[r * 4 + j] = tab[(kt) * BK + (X3 ? 8 * bq0 + 4 * r : 4 * (bq0 + r * B_Q_PASS)) + j];    \
      _Pragma("unroll") for (int r = 0; r < B_QUADS; ++r) {                                          \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                              \
          const int4 e = te[r * 4 + j];                                                              \
          const int ih = ih0 + e.y, iw = iw0 + e.z;                                                  \
          const bool ok = ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);           \
          rb[r][j] = buf_f32(rx, ok ? (unsigned)(pixbase + e.x) * 4u : kPoison, 0);                  \
        }                                                                                            \
      }                                                                                              \
    }                                                                                                \
  }
#define DASAC_STORE_TILE(buf)                                                                        \
  {                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < A_PER_T; ++i) {                                            \
      const int v = t + i * kThreads;                                                                \
      if (A_VEC % kThreads == 0 || v < A_VEC) sA[buf][v] = ra[i];                                    \
    }                                                                                                \
    if (X3) {                                                                                        \
      f32x4 hi, lo;                                                                                  \
      split_bf16(rb[0], rb[B_QUADS - 1], hi, lo);                                                    \
      sB[buf][(2 * bq0) * BN + bcol] = hi;                                                           \
      sB[buf][(2 * bq0 + 1) * BN + bcol] = lo;                                                       \
    } else {                                                                                         \
      _Pragma("unroll") for (int r = 0; r < B_QUADS; ++r) sB[buf][(bq0 + r * B_Q_PASS) * BN + bcol] = rb[r]; \
    }                                                                                                \
  }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    DASAC_STAMP(0);
    // the tile's per-row epilogue operands (consumed only by the worker that runs the epilogue: ks == 0)
    float pro_shift = 0.f;
    unsigned pro_bits[BITS == 2 ? (BN / 32) * BM / kThreads : 1];
    if (!HANDOFF || ks == 0) {
      if (t < BM) pro_shift = buf_f32(rsh, (unsigned)(m0 + t) * 4u, 0);      // rows past M (and a null shift: 0 records) read 0
      if constexpr (BITS == 2) {
        static_assert(BITS != 2 || ((BN / 32) * BM) % kThreads == 0, "mask words per tile");
#pragma unroll
        for (int u = 0; u < (BN / 32) * BM / kThreads; ++u) {
          const int idx = t + u * kThreads, c = idx / BM, row = idx - c * BM;
          const int wcol = (n0 >> 5) + c;
          pro_bits[u] = __builtin_amdgcn_raw_buffer_load_b32(
              rmsk, (m0 + row < g.M && wcol < ep.w32) ? (unsigned)((m0 + row) * ep.w32 + wcol) * 4u : kPoison, 0, 0);
        }
      }
    }
    DASAC_LOAD_TILE(ks);
    DASAC_STORE_TILE(ks & 1);
    if (!HANDOFF || ks == 0) {
      if (t < BM) s_shift[t] = pro_shift;
      if (t < BN) s_vo[t] = pro_vo;
      if constexpr (BITS == 2) {
#pragma unroll
        for (int u = 0; u < (BN / 32) * BM / kThreads; ++u) s_mbits[t + u * kThreads] = pro_bits[u];
      }
    }
    __syncthreads();
    DASAC_STAMP(1);
    for (int kt = ks; kt < ke; ++kt) {
      const int buf = kt & 1;
      const bool more = kt + 1 < ke;
      if (more) DASAC_LOAD_TILE(kt + 1);
      f32x4 a4[BK / 8][TM], b4[BK / 8][TN];
      if (X3) {
        // quad slot q of the tile = (k octet lh, half h): h = 0 the bf16 heads, h = 1 the bf16 tails
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int i = 0; i < TM; ++i) a4[h][i] = sA[buf][(2 * lh + h) * BM + wm * WM + i * 32 + li];
#pragma unroll
          for (int j = 0; j < TN; ++j) b4[h][j] = sB[buf][(2 * lh + h) * BN + wn * WN + j * 32 + li];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            // x*y ~ xl*yh + xh*yl + xh*yh (the tail*tail term is below 2^-16 of the product), fp32 accumulate
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a4[1][i]), as_bf16x8(b4[0][j]), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a4[0][i]), as_bf16x8(b4[1][j]), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a4[0][i]), as_bf16x8(b4[0][j]), acc[i][j], 0, 0, 0);
          }
      } else {
#pragma unroll
      for (int gq = 0; gq < BK / 8; ++gq) {
        const int q = 2 * gq + lh;
#pragma unroll
        for (int i = 0; i < TM; ++i) a4[gq][i] = sA[buf][q * BM + wm * WM + i * 32 + li];
#pragma unroll
        for (int j = 0; j < TN; ++j) b4[gq][j] = sB[buf][q * BN + wn * WN + j * 32 + li];
      }
#pragma unroll
      for (int gq = 0; gq < BK / 8; ++gq) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[gq][i].x, b4[gq][j].x, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[gq][i].y, b4[gq][j].y, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[gq][i].z, b4[gq][j].z, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[gq][i].w, b4[gq][j].w, acc[i][j], 0, 0, 0);
          }
      }
      }
      if (more) DASAC_STORE_TILE(buf ^ 1);
      __syncthreads();
    }
#undef DASAC_LOAD_TILE
#undef DASAC_STORE_TILE

    if (HANDOFF) {
      // Hand-off of a tile cut by range boundaries: the worker holding a tile's LATER K-steps deposits its accumulators in
      // `partial` and raises a flag, the worker holding the FIRST K-steps (the owner) adds the deposits and runs the epilogue.
      // Deposits are agent-scope (sc1) write-through stores read back with sc1 loads -- placement independent (the per-XCD
      // L2s are not coherent with each other), no buffer_wbl2 / buffer_inv fences.  (Measured in round 3: routing the
      // deposits of same-XCD neighbours through L2 with plain accesses instead -- whole tiles per XCD, hardware XCC id
      // checked -- changes nothing: 116.2 vs 113.2 us on the layer3 3x3 remainder.  The ~25 us a remainder launch costs
      // beyond its K-steps is ramp, hand-off latency and epilogue, not the 2 x 50 MB of deposit traffic.)
      constexpr int kAux = kAuxSc1;
      int c_first = 0, c_count = 0;
      if (ks > 0) {
        // partial layout [range][32x32 sub-tile][quarter][thread][4]: 16-byte stores, a wave writes 1 KB contiguous
        const int dst0 = my_range * (ACC_REGS * kThreads * 4);     // bytes; scalar
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
              __builtin_amdgcn_raw_buffer_store_b128(
                  u32x4{__float_as_uint(acc[i][j][4 * r4]), __float_as_uint(acc[i][j][4 * r4 + 1]), __float_as_uint(acc[i][j][4 * r4 + 2]),
                        __float_as_uint(acc[i][j][4 * r4 + 3])},
                  rpart, (unsigned)t * 16u, dst0 + ((i * TN + j) * 4 + r4) * kThreads * 16, kAux);
            asm volatile("" ::: "memory");
          }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every wave's stores are acknowledged (L2 / memory)
        __syncthreads();
        if (t == 0) __hip_atomic_store(&flags[my_range], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (ke < KT) {
        // I hold the FIRST K-steps; the rest was deposited by the following range(s), each at the very start of its work
        // (a range shorter than a tile -- fewer tiles than workers -- makes several of them contribute).  Ranges are never
        // empty (the host picks this schedule only with >= 1 K-step per worker).
        const int tile_end = (tile + 1) * KT;
        int n_contrib = 1;                                     // contributors are my_range + 1 .. my_range + n_contrib
        if (TAIL) {                                            // the tile's other pieces: slots tr * (s - 1) + 0 .. s - 2
          my_range = (tile - n_tiles * m_tiles) * (tail_split - 1) - 1;
          n_contrib = tail_split - 1;
        } else {
          while (sk_start(my_range + n_contrib + 1) < tile_end) ++n_contrib;
        }
        if (t == 0) {
          // Progress does not need all workers resident: a range deposits at the very START of its work, before it waits for
          // anything, and blocks are dispatched in id order, so the depositor of r is at worst the next block to get a slot.
          // A wait that still outlasts ~2^26 sleeps (seconds) means the depositor died: abort the kernel (the stream reports
          // a launch failure) instead of summing a slot that was never written.  ALL flags are collected before the first
          // load: the depositors reach their boundaries together, so this costs one wait, not one per contributor.
          for (int r = my_range + 1; r <= my_range + n_contrib; ++r) {
            int spins = 0;
            while (__hip_atomic_load(&flags[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
              __builtin_amdgcn_s_sleep(8);
              if (++spins >= (1 << 26)) __builtin_trap();
            }
            // self-cleaning flags: a range deposits at most once per launch and this worker is its only consumer, so the
            // flag can go back to 0 right here -- the next launch on the stream finds the array zeroed (no memset per conv)
            __hip_atomic_store(&flags[r], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        __syncthreads();
        c_first = my_range + 1;
        c_count = n_contrib;
      }
      // the owner adds its contributors' deposits (a loop that runs zero times for everybody else: written outside the branches
      // above so that the accumulators are loop-carried in place instead of being merged -- copied, at 128 registers spilled --
      // at the join of three paths)
      {
        for (int r = c_first; r < c_first + c_count; ++r) {
          const int src0 = r * (ACC_REGS * kThreads * 4);
          // half a deposit in flight at a time: 8 x 16-byte loads per thread (a whole one -- 64 more registers next to the 64
          // accumulators -- does not fit the 168 registers of 3 workers per CU without spilling); a quarter in the tail pieces'
          // 128-register kernel
          constexpr int NB = TAIL ? 4 : 2;
          constexpr int QH = TM * TN * 4 / NB;
#pragma unroll
          for (int hb = 0; hb < NB; ++hb) {
            f32x4 pv[QH];
#pragma unroll
            for (int q = 0; q < QH; ++q) {
              const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rpart, (unsigned)t * 16u, src0 + (hb * QH + q) * kThreads * 16, kAux);
              pv[q] = f32x4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
            }
#pragma unroll
            for (int q = 0; q < QH; ++q) {
              const int qq = hb * QH + q, sub = qq >> 2, r4 = qq & 3;
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[sub / TN][sub % TN][4 * r4 + e] += pv[q][e];
            }
            asm volatile("" ::: "memory");
          }
        }
      }
    }

    // ---- epilogue: (+shift | bias) (+residual) (ReLU) (ReLU-backward mask) -> store ----------------
    // The BN scale is already folded into the packed weights.  All traffic goes through buffer
    // descriptors: per-lane voffset = pixel position (+ the lane-half's 4-row step), the row offset is
    // scalar; loads of a 16-row group are issued as one batch before any of them is consumed.
    const bool deposited = HANDOFF && ks > 0;                // this worker only contributed a partial sum
    DASAC_STAMP(2);
    // (Round 5, measured: __builtin_amdgcn_s_setprio(3) for the epilogue changes nothing -- 21.0 vs 21.3 us from the end of the K loop to
    // the last store issued, profiles/r5_epilogue_anatomy.txt: a wave with an MFMA ready is served first whatever the priorities are.
    // An s_nop 15 after every (second, fourth) MFMA of the short-K launches, to open issue windows for co-resident prologue /
    // epilogue waves, buys 1-2.5 % on the K = 256 layers and costs 0.7 % at K = 4608: not kept.)
    if (!deposited) {
    if constexpr (BITS != 3) {
    // Per 32-pixel column group j: ONE batch of loads (the residual and / or an fp32 mask, TM x 16 values; shift and mask words
    // come from LDS), then the arithmetic and the TM x 16 stores.  A layer without residual issues no vector-memory load here
    // at all -- 64 stores back to back, the workgroup ends one acknowledgement after the last; with a residual the second
    // batch's wait covers the first batch's stores: two store round trips per tile instead of eight.
    // FULL: the tile's BM rows all exist (every tile of a layer whose channel count is a multiple of BM): no row tests.
    // (the plane size is laundered through an empty asm so that none of the 64 per-row scalar offsets derived from it is
    // computed -- and kept alive in SGPRs, then spilled into VGPR lanes -- ahead of the K loop)
    int OutHWe = OutHW;
    asm volatile("" : "+s"(OutHWe));
    auto epilogue = [&](auto full_tag) __attribute__((always_inline)) {
      constexpr bool FULL = decltype(full_tag)::value;
      // row of accumulator register rg of row group i: mrow + (rg&3) + 8*(rg>>2), + 4*lh in the lane offset -> a row exists
      // iff its lane-independent part is below M - 4*lh (one per-lane limit, a compare and a select per access)
      const int mlim = g.M - 4 * lh;
      const unsigned lane_bit = 1u << li;                      // this lane's pixel inside a mask word
#define DASAC_ROW(i, rg) (m0 + wm * WM + (i) * 32 + ((rg) & 3) + 8 * ((rg) >> 2))
#define DASAC_VOFF(i, rg) (FULL ? vo : (DASAC_ROW(i, rg) < mlim ? vo : kPoison))
      // one batch: row groups I0 .. I0+NI-1 of column group j
      auto batch = [&](int j, unsigned vo, auto i0_tag, auto ni_tag, auto relu_tag) __attribute__((always_inline)) {
        constexpr int I0 = decltype(i0_tag)::value, NI = decltype(ni_tag)::value;
        constexpr bool RELU = decltype(relu_tag)::value;     // compile time: a run-time flag costs a v_max AND a select per element
        const int wcol = (n0 + wn * WN + j * 32) >> 5;          // this wave's 32-pixel group = one word column of the bit masks
        float rs[NI][16], mk[NI][16];
        if (ep.res) {
#pragma unroll
          for (int i = I0; i < I0 + NI; ++i)
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) rs[i - I0][rg] = buf_f32(rres, DASAC_VOFF(i, rg), DASAC_ROW(i, rg) * OutHWe * 4);
        }
        if (BITS != 2 && ep.mask) {          // fp32 mask: the ReLU-backward pattern read from the activation itself
#pragma unroll
          for (int i = I0; i < I0 + NI; ++i)
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) mk[i - I0][rg] = buf_f32(rmsk, DASAC_VOFF(i, rg), DASAC_ROW(i, rg) * OutHWe * 4);
        }
#pragma unroll
        for (int i = I0; i < I0 + NI; ++i) {
          const int mrow = m0 + wm * WM + i * 32;
          if (!FULL && mrow >= g.M) continue;                  // whole 32-row group beyond M (uniform)
          const int lrow = wm * WM + i * 32 + 4 * lh;            // + 8*q + e: the four rows of accumulator registers 4q .. 4q+3
          int bitrows = 0;                                     // producer: lane r collects the mask word of row mrow + r
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 sh4 = *reinterpret_cast<const f32x4*>(&s_shift[lrow + 8 * q]);
            u32x4 mb4 = u32x4{0u, 0u, 0u, 0u};
            if constexpr (BITS == 2) mb4 = *reinterpret_cast<const u32x4*>(&s_mbits[(wn * (WN / 32) + j) * BM + lrow + 8 * q]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int rg = 4 * q + e;
              float v = acc[i][j][rg] + sh4[e];
              if (ep.res) v = v + rs[i - I0][rg];
              if constexpr (RELU) v = fmaxf(v, 0.f);
              if (BITS != 2 && ep.mask) v = mk[i - I0][rg] > 0.f ? v : 0.f;
              if constexpr (BITS == 2) v = (mb4[e] & lane_bit) ? v : 0.f;
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, DASAC_VOFF(i, rg), DASAC_ROW(i, rg) * OutHWe * 4, 0);
              if constexpr (BITS == 1)      // lanes 0-31 hold row (rg&3) + 8*(rg>>2), lanes 32-63 the row 4 below it: two words per ballot
                bitrows = put_mask_rows(rg, __builtin_amdgcn_ballot_w64(v > 0.f), bitrows);
            }
          }
          if constexpr (BITS == 1) {
            // (a 32-pixel group of the last tile may lie entirely past the last pixel: no word exists for it)
            if (lane < 32 && mrow + lane < g.M && wcol < ep.w32) ep.obits[(size_t)(mrow + lane) * ep.w32 + wcol] = (unsigned)bitrows;
          }
        }
        asm volatile("" ::: "memory");     // the next batch's loads stay behind this batch's stores (registers -> occupancy)
      };
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        unsigned vo = s_vo[wn * WN + j * 32 + li];
        vo = vo == kPoison ? kPoison : vo + (unsigned)(4 * lh * OutHWe) * 4u;      // + the lane half's four rows
        using c0 = std::integral_constant<int, 0>;
        using c1 = std::integral_constant<int, 1>;
        auto run = [&](auto relu_tag) __attribute__((always_inline)) {
          if (TM == 2 && BITS != 2 && ep.res && ep.mask) {   // residual AND fp32 mask: 2 x 16 loaded values per row group -> one group per batch
            batch(j, vo, c0{}, c1{}, relu_tag);
            if constexpr (TM == 2) batch(j, vo, c1{}, c1{}, relu_tag);
          } else {
            batch(j, vo, c0{}, std::integral_constant<int, TM>{}, relu_tag);
          }
        };
        if (ep.relu) run(std::true_type{});
        else run(std::false_type{});
      }
#undef DASAC_ROW
#undef DASAC_VOFF
    };
    if (m0 + BM <= g.M) epilogue(std::true_type{});
    else epilogue(std::false_type{});
    } else {
      // ---- BITS == 3: raw convolution (+ bias) in front of a batch-statistics BatchNorm.  No residual / ReLU / mask here (they
      // follow the normalisation); instead the per-row sum and sum of squares of the stored values.  Row groups are the OUTER
      // loop so that only one group's 2 x 16 running sums are live next to the accumulators.  Lane (li, lh) holds, per
      // accumulator register rg, the sum over ITS pixels of row i*32 + (rg&3) + 8*(rg>>2) + 4*lh: sum over the 32 lanes of
      // the half-wave, lane li == rg keeps row rg's total, the WAVES_N waves of a row meet in LDS (the operand tiles are
      // dead: the K loop ended with a barrier), 2*BM coalesced floats go out per tile.
      static_assert(BITS != 3 || (BM == 128 && WAVES_N == 2 && TN == 2), "stats epilogue: 128-row tile, two pixel waves");
      float* sst = reinterpret_cast<float*>(&sA[0][0]);        // [2][BM][WAVES_N]
      unsigned vo[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int pix = n0 + wn * WN + j * 32 + li;
        vo[j] = kPoison;
        if (pix < g.Npix) {
          const int n = pix / OHW, r = pix - n * OHW;
          const int oh = r / g.OW, ow = r - oh * g.OW;
          vo[j] = (unsigned)(n * g.M * OutHW + oh * g.ostride * g.OutW + ow * g.ostride + 4 * lh * OutHW) * 4u;
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int mrow = m0 + wm * WM + i * 32;
        float ms = 0.f, mq = 0.f;
        if (mrow < g.M) {                                        // (uniform) a whole 32-row group beyond M contributes zeros
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            float sh[8];
            bool rowok[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int rg = half * 8 + u;
              const int mr = mrow + (rg & 3) + 8 * (rg >> 2);
              rowok[u] = ragged ? (mr + 4 * lh < g.M) : (mr < g.M);
              sh[u] = s_shift[wm * WM + i * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * lh];    // 0 for rows past M / no bias
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int rg = half * 8 + u;
              const int roff = (mrow + (rg & 3) + 8 * (rg >> 2)) * OutHW * 4;
              float ss = 0.f, qq = 0.f;
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                const float v = acc[i][j][rg] + sh[u];
                const unsigned vr = rowok[u] ? vo[j] : kPoison;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, vr, roff, 0);
                const float vv = vr != kPoison ? v : 0.f;        // pixels / rows past the tensor count as 0
                ss += vv;
                qq = __builtin_fmaf(vv, vv, qq);
              }
              const float rs_ = half_wave_sum(ss), rq_ = half_wave_sum(qq);
              ms = li == rg ? rs_ : ms;
              mq = li == rg ? rq_ : mq;
            }
            asm volatile("" ::: "memory");
          }
        }
        if (li < 16) {
          const int row = wm * WM + i * 32 + (li & 3) + 8 * (li >> 2) + 4 * lh;
          sst[row * WAVES_N + wn] = ms;
          sst[(BM + row) * WAVES_N + wn] = mq;
        }
      }
      __syncthreads();
      {
        const int which = t / BM, row = t - which * BM;          // 256 threads = {sum, sum of squares} x 128 rows
        const float tot = sst[(which * BM + row) * WAVES_N] + sst[(which * BM + row) * WAVES_N + 1];
        ep.stats[((size_t)(n0 / BN) * 2 + which) * g.Mpad + m0 + row] = tot;
      }
    }
    }
#ifdef DASAC_TRACE_TILES
    DASAC_STAMP(5);                                    // the epilogue's stores have been issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // ... and acknowledged
    DASAC_STAMP(3);
    if (g_tile_trace && threadIdx.x == 0) g_tile_trace[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf;
#endif
    if (STREAMK) __syncthreads();      // LDS is reused by the next tile of this worker
  } while (STREAMK && it < it_end);
}

// The persistent grid (3 workers per CU x 256 CUs) and the XCD mapping are sized for the full MI355X; a device with
// fewer CUs (partitioned modes, other parts) gets the tile-per-block schedule only.  The answer is per device id
// (a process may drive several devices / switch with hipSetDevice).  It is gemm_plan's `full_chip` (conv_plan.hpp).
static bool persistent_grid_fits() {
  constexpr int kMaxDev = 64;
  static std::atomic<signed char> cache[kMaxDev];          // 0 unknown, 1 fits, -1 does not
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const bool cached = dev >= 0 && dev < kMaxDev;
  if (cached && cache[dev].load(std::memory_order_relaxed) != 0) return cache[dev].load(std::memory_order_relaxed) > 0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  const bool ok = cus >= kNumCu;
  if (cached) cache[dev].store(ok ? 1 : -1, std::memory_order_relaxed);
  return ok;
}

// one launch by its plan (conv_plan.hpp: gemm_plan); g.n_tile0 is the plan's
template <int BM, int BN, int WAVES_M, int BK, bool FAST, bool X3 = false, int BITS = 0>
static int launch_gemm(const float* X, const float* Wp, const int4* tab, float* Out, const GemmGeom& g, const Epilogue& ep,
                       const GemmPlan& p, void* workspace, size_t ws_bytes, hipStream_t s) {
  if ((long long)p.m_tiles * (p.n_tiles + kNumXcd) * p.k_steps >= (1ll << 31)) return fail(DASAC_EINVAL, "conv_gemm: iteration space exceeds 2^31");
  if (ws_bytes < p.workspace_bytes) return fail(DASAC_EWORKSPACE, "conv_gemm: workspace too small (%zu < %zu)", ws_bytes, p.workspace_bytes);
  float* partial = p.uses_workspace ? reinterpret_cast<float*>(workspace) : nullptr;
  int* flags = p.uses_workspace ? reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + kPartialBytes) : nullptr;
  switch (p.kind) {
    case kGemmTail:
      if constexpr (BM == 128)
        hipLaunchKernelGGL((conv_gemm<BM, BN, WAVES_M, BK, FAST, 2, X3, BITS>), dim3(p.grid), dim3(kThreads), 0, s, X, Wp, tab, Out, g, ep,
                           p.m_tiles, p.lead_n, partial, flags, p.tail_tiles, p.split);
      break;
    case kGemmStreamK:
      if constexpr (BM == 128)
        hipLaunchKernelGGL((conv_gemm<BM, BN, WAVES_M, BK, FAST, 1, X3, BITS>), dim3(p.grid), dim3(kThreads), 0, s, X, Wp, tab, Out, g, ep,
                           p.m_tiles, p.n_tiles, partial, flags, 0, 1);
      break;
    default:
      hipLaunchKernelGGL((conv_gemm<BM, BN, WAVES_M, BK, FAST, 0, X3, BITS>), dim3(p.grid), dim3(kThreads), 0, s, X, Wp, tab, Out, g, ep,
                         p.m_tiles, p.n_tiles, nullptr, nullptr, 0, 1);
  }
  return DASAC_OK;
}

}  // namespace dasac

using namespace dasac;

// the plan of dasac_conv_gemm over the whole tensor with a workspace, schedule 0: what the three queries below report
static GemmPlan whole_plan(int Nb, int OH, int OW, int M, int K) {
  const int64_t Npix = (int64_t)Nb * OH * OW;
  return gemm_plan(M, K, Npix, 0, Npix, 0, true, reserved_cus(), persistent_grid_fits());
}

// 1 when this shape's own schedule is the persistent stream-K one (a split-K tail, where dasac_conv_gemm_tail_split finds one,
// goes first)
extern "C" int dasac_conv_gemm_schedule(int Nb, int OH, int OW, int M, int K) { return whole_plan(Nb, OH, OW, M, K).wants_streamk ? 1 : 0; }

// (Rounds 2-5 issued a long-K conv whose tile count leaves a ragged last round as TWO launches -- whole rounds one block per tile,
// the remainder on the persistent stream-K schedule (dasac_conv_gemm_plan) -- so that the lockstep K walk of the leading rounds
// keeps sharing halo rows in L2.  Round 6 folded the remainder into the first launch: tail_plan / conv_gemm<SK = 2>.
// Measured on one box, cfg-3 fused step: GEMM kernel time 273.5 -> 272.6 ms, 169 launches per step gone; a piece's prologue and
// deposit / epilogue cost what the second launch's ramp and hand-off did: profiles/r6_tail_and_qtap_ab.txt.)
extern "C" size_t dasac_conv_gemm_workspace(void) { return kGemmWorkspaceBytes; }

// K-ranges per tail tile when dasac_conv_gemm (schedule 0, whole tensor, workspace given) runs this shape as ONE launch of whole
// rounds of tile-per-block workgroups + a split-K tail; 0 = it does not (then dasac_conv_gemm_schedule tells the rest)
extern "C" int dasac_conv_gemm_tail_split(int Nb, int OH, int OW, int M, int K) { return whole_plan(Nb, OH, OW, M, K).split; }

#ifdef DASAC_TRACE_TILES
extern "C" int dasac_debug_set_tile_trace(void* buffer) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(buffer);
  return hipMemcpyToSymbol(HIP_SYMBOL(dasac::g_tile_trace), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" size_t dasac_relu_bits_words(int M, int64_t Npix) { return (size_t)M * (size_t)((Npix + 31) / 32); }
// 1 when dasac_conv_gemm (fp32) can record / consume bit masks for an output of M channels over a gathered tensor of Cx channels
extern "C" int dasac_conv_gemm_bits_ok(int M, int Cx) { return (pick_bm(dasac_conv_mpad(M)) == 128 && Cx % kBK == 0) ? 1 : 0; }

static int conv_gemm_impl(bool x3, const float* x, const float* packed, const int32_t* table, float* out, int Nb, int Cx, int H,
                          int W, int OH, int OW, int stride, int M, int K, int OutH, int OutW, int ostride, const float* shift,
                          const float* res, const float* mask, const uint32_t* mask_bits, uint32_t* relu_bits_out, int relu,
                          int pix_begin, int pix_count, int schedule, void* workspace, size_t ws_bytes, dasac_stream_t stream,
                          float* stats = nullptr) {
  DASAC_REQUIRE(x && packed && table && out, "conv_gemm: null pointer");
  DASAC_REQUIRE(((uintptr_t)table & 15) == 0, "conv_gemm: misaligned table (16-byte rows)");
  DASAC_REQUIRE(!stats || (!x3 && !mask_bits && !relu_bits_out && dasac_conv_gemm_bits_ok(M, Cx) && ostride == 1),
                "conv_gemm_stats: needs the 128-row fp32 tile with Cx %% 16 == 0 (dasac_conv_gemm_stats_ok), no bit masks");
  DASAC_REQUIRE(!(mask && mask_bits), "conv_gemm: give the ReLU pattern as fp32 mask OR as bit mask");
  DASAC_REQUIRE(!(mask_bits || relu_bits_out) || (ostride == 1 && OutH == OH && OutW == OW),
                "conv_gemm: bit masks index the GEMM's own pixel axis (ostride must be 1)");
  DASAC_REQUIRE(!relu_bits_out || relu, "conv_gemm: relu_bits_out records the pattern of a ReLU epilogue");
  DASAC_REQUIRE(!(x3 && (mask_bits || relu_bits_out)), "conv_gemm_x3: bit masks are implemented for the fp32 kernel only");
  DASAC_REQUIRE(!stats || (!res && !relu), "conv_gemm_stats: the statistics epilogue stores the raw convolution (+ shift): no residual, no ReLU");
  GemmGeom g;
  const int Mpad = dasac_conv_mpad(M), Kloop = (K + kBK - 1) / kBK * kBK;   // table/pack are padded to 128 >= Kloop
  int rc = fill_geom(g, Nb, Cx, H, W, OH, OW, stride, M, Mpad, Kloop, OutH, OutW, ostride);
  if (rc) return rc;
  DASAC_REQUIRE((int64_t)dasac_conv_kpad(K) * Mpad * 4 < (1ll << 31), "conv: packed weights exceed 2 GiB");
  g.w_bytes = dasac_conv_kpad(K) * Mpad * 4;
  Epilogue ep{shift, res, mask, relu, mask_bits, relu_bits_out, (g.Npix + 31) / 32, stats};
  DASAC_REQUIRE((int64_t)M * ep.w32 * 4 < (1ll << 31), "conv_gemm: bit mask exceeds the 2 GiB buffer-descriptor window");
  const int4* tab = reinterpret_cast<const int4*>(table);
  hipStream_t s = as_stream(stream);
  const bool fast = Cx % kBK == 0;      // a K-step never straddles two taps
  // pixel range of this launch (whole tiles; the last one may be ragged only at the end of the tensor)
  const int pix_end = pix_count > 0 ? pix_begin + pix_count : g.Npix;
  DASAC_REQUIRE(schedule >= 0 && schedule <= 2, "conv_gemm: schedule must be 0 (auto), 1 (tile per block) or 2 (stream-K)");
  const int bm = pick_bm(Mpad), bn = bm == 32 ? 256 : 128;
  DASAC_REQUIRE(pix_begin >= 0 && pix_begin < g.Npix && pix_begin % bn == 0 && pix_end > pix_begin && pix_end <= g.Npix &&
                    (pix_end == g.Npix || pix_end % bn == 0),
                "conv_gemm: pixel range [%d, %d) must consist of whole %d-pixel tiles", pix_begin, pix_end, bn);
  // the 64- and 32-row tiles have the tile-per-block kernel only: their plan is that whatever was asked for
  const GemmPlan p = gemm_plan(M, K, g.Npix, pix_begin, pix_end, schedule, workspace != nullptr, reserved_cus(), persistent_grid_fits());
  g.n_tile0 = p.n_tile0;
  const char* what = "conv_gemm";
  if (x3) {
    DASAC_REQUIRE(bm >= 64, "conv_gemm_x3: needs M > 32 (use dasac_conv_gemm for skinny outputs)");
    what = "conv_gemm_x3";
    if (bm == 128)
      rc = fast ? launch_gemm<128, 128, 2, kBK, true, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
                : launch_gemm<128, 128, 2, kBK, false, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
    else
      rc = fast ? launch_gemm<64, 128, 2, kBK, true, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
                : launch_gemm<64, 128, 2, kBK, false, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  } else if (stats) {
    what = "conv_gemm_stats";
    rc = launch_gemm<128, 128, 2, kBK, true, false, 3>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  } else if (mask_bits || relu_bits_out) {
    DASAC_REQUIRE(dasac_conv_gemm_bits_ok(M, Cx) && !(mask_bits && relu_bits_out),
                  "conv_gemm: bit masks need the 128-row fp32 tile with Cx %% 16 == 0 (dasac_conv_gemm_bits_ok), one direction per call");
    rc = relu_bits_out ? launch_gemm<128, 128, 2, kBK, true, false, 1>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
                       : launch_gemm<128, 128, 2, kBK, true, false, 2>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  } else if (bm == 128) {
    rc = fast ? launch_gemm<128, 128, 2, kBK, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
              : launch_gemm<128, 128, 2, kBK, false>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  } else if (bm == 64) {
    rc = fast ? launch_gemm<64, 128, 2, kBK, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
              : launch_gemm<64, 128, 2, kBK, false>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  } else {
    rc = fast ? launch_gemm<32, 256, 1, kBK, true>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s)
              : launch_gemm<32, 256, 1, kBK, false>(x, packed, tab, out, g, ep, p, workspace, ws_bytes, s);
  }
  if (rc) return rc;
  DASAC_CHECK_LAUNCH(what);
  return DASAC_OK;
}

extern "C" int dasac_conv_gemm(const float* x, const float* packed, const int32_t* table, float* out, int Nb, int Cx,
                               int H, int W, int OH, int OW, int stride, int M, int K, int OutH, int OutW, int ostride,
                               const float* shift, const float* res, const float* mask, const uint32_t* mask_bits,
                               uint32_t* relu_bits_out, int relu, int pix_begin, int pix_count, int schedule,
                               void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  return conv_gemm_impl(false, x, packed, table, out, Nb, Cx, H, W, OH, OW, stride, M, K, OutH, OutW, ostride, shift, res, mask,
                        mask_bits, relu_bits_out, relu, pix_begin, pix_count, schedule, workspace, ws_bytes, stream);
}

// `batch` GEMMs of one geometry as ONE launch of the tile-per-block kernel (grid y = batch entry): see include/dasac_hip.h.
// A launch of few tiles leaves the last round of resident workgroups mostly empty (the 604 tiles of a layer4 Winograd point GEMM:
// 2.36 per CU); sixteen of them in one grid fill 9.4 rounds.  x-fastest dispatch keeps one entry's weight matrix in L2 while
// its tiles run, and gridDim.x stays a multiple of 8, so blockIdx.x % 8 still names the XCD.
extern "C" int dasac_conv_gemm_batched(const float* x, const float* packed, const int32_t* table, float* out, int Nb, int Cx,
                                       int H, int W, int OH, int OW, int stride, int M, int K, int OutH, int OutW, int ostride,
                                       int batch, int64_t x_stride, int64_t packed_stride, int64_t out_stride, dasac_stream_t stream) {
  DASAC_REQUIRE(batch >= 1 && batch <= 65535, "conv_gemm_batched: batch %d outside 1..65535 (grid y)", batch);
  DASAC_REQUIRE(x && packed && table && out, "conv_gemm_batched: null pointer");
  DASAC_REQUIRE(((uintptr_t)table & 15) == 0, "conv_gemm_batched: misaligned table (16-byte rows)");
  DASAC_REQUIRE(Cx > 0 && Cx % kBK == 0, "conv_gemm_batched: gathered channels %d must be a multiple of %d", Cx, kBK);
  GemmGeom g;
  const int Mpad = dasac_conv_mpad(M), Kloop = (K + kBK - 1) / kBK * kBK;
  DASAC_REQUIRE(pick_bm(Mpad) == 128, "conv_gemm_batched: needs the 128-row tile (padded M = %d)", Mpad);
  int rc = fill_geom(g, Nb, Cx, H, W, OH, OW, stride, M, Mpad, Kloop, OutH, OutW, ostride);   // per entry: 4 GiB window, 2^30 elements
  if (rc) return rc;
  const int64_t w_elems = (int64_t)dasac_conv_kpad(K) * Mpad;
  DASAC_REQUIRE(w_elems * 4 < (1ll << 31), "conv: packed weights exceed 2 GiB");
  g.w_bytes = (unsigned)(w_elems * 4);
  const int64_t x_elems = (int64_t)Nb * Cx * H * W, out_elems = (int64_t)Nb * M * OutH * OutW;
  if (batch > 1 || x_stride || packed_stride || out_stride) {
    DASAC_REQUIRE(x_stride >= x_elems && packed_stride >= w_elems && out_stride >= out_elems,
                  "conv_gemm_batched: a per-batch stride is smaller than one entry (x %lld < %lld, packed %lld < %lld or out %lld < %lld)",
                  (long long)x_stride, (long long)x_elems, (long long)packed_stride, (long long)w_elems, (long long)out_stride, (long long)out_elems);
    DASAC_REQUIRE(x_stride % 4 == 0 && packed_stride % 4 == 0 && out_stride % 4 == 0,
                  "conv_gemm_batched: per-batch strides must be multiples of 4 elements (16-byte aligned entries)");
  }
  const int n_tiles = (g.Npix + 127) / 128, m_tiles = (M + 127) / 128;
  if ((long long)m_tiles * (n_tiles + kNumXcd) * (g.Kpad / kBK) >= (1ll << 31)) return fail(DASAC_EINVAL, "conv_gemm: iteration space exceeds 2^31");
  // no epilogue operands: the signature has none to give
  BatchedEpilogue ep{{nullptr, nullptr, nullptr, 0, nullptr, nullptr, (g.Npix + 31) / 32, nullptr}, x_stride, packed_stride, out_stride};
  hipLaunchKernelGGL((conv_gemm<128, 128, 2, kBK, true, 0, false, 4>), dim3(round_up_xcd(n_tiles) * m_tiles, batch), dim3(kThreads), 0,
                     as_stream(stream), x, packed, reinterpret_cast<const int4*>(table), out, g, ep, m_tiles, n_tiles, nullptr, nullptr, 0, 1);
  DASAC_CHECK_LAUNCH("conv_gemm_batched");
  return DASAC_OK;
}

// dasac_conv_gemm whose epilogue also leaves per-tile channel statistics (batch-statistics BatchNorm behind the conv):
// stats [dasac_conv_gemm_stats_tiles(Nb, OH, OW)][2][dasac_conv_mpad(M)] floats = per 128-pixel tile the sum and the sum of
// squares of every output row as stored (shift / bias included) -- dasac_bn_train_finalize adds the tiles in a fixed order.
extern "C" int dasac_conv_gemm_stats_ok(int M, int Cx) { return dasac_conv_gemm_bits_ok(M, Cx); }
extern "C" int dasac_conv_gemm_stats_tiles(int Nb, int OH, int OW) { return (int)(((int64_t)Nb * OH * OW + 127) / 128); }
extern "C" int dasac_conv_gemm_stats(const float* x, const float* packed, const int32_t* table, float* out, int Nb, int Cx,
                                     int H, int W, int OH, int OW, int stride, int M, int K, int OutH, int OutW, int ostride,
                                     const float* shift, const float* res, int relu, int pix_begin, int pix_count, int schedule,
                                     void* workspace, size_t ws_bytes, float* stats, dasac_stream_t stream) {
  DASAC_REQUIRE(stats, "conv_gemm_stats: null statistics buffer");
  return conv_gemm_impl(false, x, packed, table, out, Nb, Cx, H, W, OH, OW, stride, M, K, OutH, OutW, ostride, shift, res, nullptr,
                        nullptr, nullptr, relu, pix_begin, pix_count, schedule, workspace, ws_bytes, stream, stats);
}

extern "C" int dasac_conv_gemm_x3(const float* x, const void* packed_x3, const int32_t* table, float* out, int Nb, int Cx,
                                  int H, int W, int OH, int OW, int stride, int M, int K, int OutH, int OutW, int ostride,
                                  const float* shift, const float* res, const float* mask, const uint32_t* mask_bits,
                                  uint32_t* relu_bits_out, int relu, int pix_begin, int pix_count, int schedule, void* workspace,
                                  size_t ws_bytes, dasac_stream_t stream) {
  return conv_gemm_impl(true, x, reinterpret_cast<const float*>(packed_x3), table, out, Nb, Cx, H, W, OH, OW, stride, M, K, OutH, OutW, ostride,
                        shift, res, mask, mask_bits, relu_bits_out, relu, pix_begin, pix_count, schedule, workspace, ws_bytes, stream);
}
