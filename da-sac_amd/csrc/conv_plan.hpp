// The integer rules of the conv GEMM (conv_gemm.hip) and of the pixel-split weight gradient (conv_wgrad.hip), in one place:
//   host rules   -- padding, the M tile, which of the three GEMM schedules a launch gets, its grid and workspace (gemm_plan), the weight
//                   gradient's tiles, pixel splits, grid and workspace layout (wgrad_plan, wgrad_batched_plan);
//   device maps  -- block id -> tile of the one-block-per-tile GEMM (the SK = 0 kernels), and block id -> (m tile, k tile, split,
//                   pixel range) of the weight gradient; compiled for the host AND the device.
// No HIP header is needed: the launchers and the kernels call exactly what the stand-alone host check (tools/conv_plan_check.cpp,
// tests/test_conv_plan_host.py) compares with tests/gemm_schedule_ref.py on more than 5000 shapes at every reserved-CU setting and
// walks block by block.  The stream-K and tail block maps of conv_gemm are NOT here: moved to this header their kernels compiled to
// other instruction streams and a timing row of each schedule missed its bound (profiles/conv_plan.md, section 3), so they stay
// written inside the kernel and tests/gemm_schedule_ref.py remains their only restatement.
// The weight gradient's map is three functions (wgrad_list_index, wgrad_tile, wgrad_pixels) and the early return stays in the two
// kernels, instead of one function returning `has_work`: written that way, and only that way, conv_wgrad and conv_wgrad_batched
// keep the instruction streams they had with the decode written inline.  That identity holds for the toolchain it was compared
// on; the maps' correctness does not rest on it -- the host walk checks the functions themselves.
#pragma once
#include <cstddef>
#include <cstdint>

#include "chip.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DASAC_PLAN_HD __host__ __device__ __forceinline__
#else
#define DASAC_PLAN_HD inline
#endif

namespace dasac {

// ---- constants ---------------------------------------------------------------------------------------------------------------
constexpr int kBK = 16;                                  // K-step of the forward/dgrad kernel
constexpr int kSkWorkersPerCu = 3;                       // persistent 128x128 workers per CU (<=168 registers, 32 KB LDS each; four spill: EXPERIMENTS.md)
constexpr int kSkWorkers = kNumCu * kSkWorkersPerCu;     // 768, multiple of 8: the grid of every stream-K launch on the whole chip
constexpr int kTileSlots = kNumCu * 4;                   // resident blocks of the tile-per-block kernel (4 per CU)
constexpr int kTailSlots = 2048;                         // deposit / flag slots of the split-K tail (SK == 2): 128 MB of workspace
// the tail planner (a sweep of the minimum piece length 8 .. 32 K-steps and of the fixed cost 6 .. 20 moved the three tail shapes of
// the step by less than 1 %: tools/experiments/r6_tail_sweep.sh, EXPERIMENTS.md)
constexpr int kTailMinSteps = 8;                         // fewest K-steps of a piece
constexpr double kTailPieceCost = 6.0;                   // a piece's fixed cost in K-steps: prologue, deposit or epilogue
constexpr int kTailMaxSplit = 8;                         // most K-ranges per tail tile
// workspace of the two hand-off schedules (128 x 128 tiles only): a deposit per slot of the larger one, then the flags
constexpr size_t kDepositBytes = (size_t)128 * 128 * sizeof(float);
constexpr size_t kPartialBytes = (size_t)(kTailSlots > kSkWorkers ? kTailSlots : kSkWorkers) * kDepositBytes;
constexpr size_t kGemmWorkspaceBytes = kPartialBytes + (size_t)(kTailSlots + 1) * sizeof(int);

constexpr int kWgPix = 32;         // weight gradient: pixels per K-step
// At least 256 pixels (8 K-steps) per split.  Rounds 1-3 asked for 1024: at batch 2 (cfg-2: 18 818 pixels) that capped the 16-tile
// 1x1 layers at 19 splits = 304 blocks for 768 slots; measured in round 4 (profiles/r4_wgrad_split_granularity.txt, cfg-2):
// 1024 -> 512 -> 256 pixels: weight gradients 18.7 -> 16.3 -> 15.4 ms/step (90 -> 103 -> 109 TFLOP/s).  Large batches are
// unaffected (the cap of 64 splits binds first).
constexpr int kWgMinPix = 256;
// 3 resident blocks per CU (<= 168 registers).  Measured in round 3: both 128x128 kernels also fit 128 registers (2 / 44 spill
// instructions outside the MFMA loop) and 4 x 36 KB of LDS, but at 4 blocks per CU the step's weight-gradient time goes from
// 109.2 to 114.0 ms (123.1 -> 117.9 TFLOP/s): occupancy is not what the pixel loop lacks.  Nor is it the dZ loads of the 3x3
// layers: dZ through the four-pixels-per-lane loader (dwordx4 + ds_write_b128, the gathered operand unchanged) gives 109.6 vs
// 109.1 ms.
constexpr int kWgSlots = kNumCu * 3;
constexpr int kWgMaxSplits = 64;
// few tiles x many pixels (layer1 / stem: 2 tiles, 298k..1.2M pixels): more splits, or 128 blocks would face 768 slots
constexpr int kWgFewTiles = 12;                          // measured: no gain at 97x97 resolution
constexpr int kWgManyPix = 200000;
// a tensor behind one buffer descriptor: unsigned 32-bit byte offsets, the largest one is the poison (conv_common.hpp)
constexpr int64_t kMaxTensorBytes = (1ll << 32) - 4096;

// ---- host rules: padding and tiles -------------------------------------------------------------------------------------------
inline int conv_mpad(int M) { return M > 64 ? (M + 127) / 128 * 128 : (M > 32 ? 64 : 32); }
inline int conv_kpad(int K) { return (K + 127) / 128 * 128; }
// M tile chosen from the padded channel count: 128 | 64 | 32
inline int pick_bm(int Mpad) { return Mpad % 128 == 0 ? 128 : (Mpad % 64 == 0 ? 64 : 32); }
// grids whose kernels read blockIdx.x % kNumXcd as the XCD are whole multiples of it
DASAC_PLAN_HD int round_up_xcd(int n) { return (n + kNumXcd - 1) / kNumXcd * kNumXcd; }

// ---- host rules: the GEMM's schedule -----------------------------------------------------------------------------------------
// workers of a persistent stream-K launch: 3 per CU on the CUs this process does not leave to overlapped collectives.  `reserved` is
// read ONCE per launch decision (reserved_cus()) and handed through: a concurrent dasac_set_reserved_cus must not make the
// eligibility test, the schedule choice and the grid size of one launch disagree.
inline int sk_workers(int reserved) { return (kNumCu - reserved) * kSkWorkersPerCu; }

// stream-K pays when the tile count leaves the last round of resident blocks mostly empty (on a device with all 256 CUs: the
// caller's `full_chip`).
inline bool want_streamk(int tiles, int k_steps, int reserved) {
  if ((long long)tiles * k_steps < sk_workers(reserved)) return false;                  // every range gets >= 1 K-step
  // measured: the persistent schedule (3 workers/CU, <=168 registers) wins on long contractions whose tile count
  // fills the last round of the plain launch badly; short-K 1x1 layers are better off with the plain kernel's
  // 4 blocks per CU (128 registers) even with a partly empty last round (85 vs 99 TFLOP/s at K = 256) -- unless
  // the launch would leave most of the chip idle (small batches: 296 tiles at B = 2, 148 at B = 1).
  const int resident = (kNumCu - reserved) * 3;
  const int rounds = (tiles + resident - 1) / resident;
  const double eff = (double)tiles / ((double)rounds * resident);
  return k_steps >= 64 ? eff < 0.93 : (k_steps >= 16 && eff < 0.6);
}

// Split-K tail (SK == 2) of a launch over ALL n_tiles pixel tiles: the leading whole rounds of resident blocks run one block per
// tile, the remaining R tiles are cut into `split` K-ranges so that the pieces fill (a whole number of) rounds again.  Chosen for
// the shapes the persistent schedule was chosen for in rounds 2-5 (want_streamk) when at least one whole round leads.  The split
// minimises rounds x (K-steps per piece + a piece's fixed cost).  Returns 0 = no tail.
inline int tail_plan(int m_tiles, int n_tiles, int k_steps, int reserved, int& lead_n) {
  const int tiles = m_tiles * n_tiles;
  if (!want_streamk(tiles, k_steps, reserved)) return 0;
  lead_n = (tiles / kTileSlots) * kTileSlots / m_tiles;          // pixel tiles of the leading whole rounds
  // (fewer tiles than resident blocks -- small batches, cfg-2's 296 tiles -- stay on the persistent kernel: the same launches as pure
  // split-K pieces of this kernel, 4 blocks per CU, measured 35.4 against 33.9 ms per cfg-2 step: equal ranges balance better than
  // equal pieces when nothing leads; profiles/EXPERIMENTS.md round 6)
  if (lead_n <= 0 || lead_n >= n_tiles) return 0;
  const int R = (n_tiles - lead_n) * m_tiles;
  int best = 0;
  double best_cost = 0.0;
  for (int sp = 1; sp <= kTailMaxSplit && sp * kTailMinSteps <= k_steps; ++sp) {
    if ((long long)R * (sp - 1) > kTailSlots) break;
    const int rounds = (R * sp + kTileSlots - 1) / kTileSlots;
    const double cost = rounds * ((double)k_steps / sp + kTailPieceCost);
    if (best == 0 || cost < best_cost - 1e-9) {
      best = sp;
      best_cost = cost;
    }
  }
  return best;
}

// One launch of the forward / data-gradient GEMM.  `kind` is the kernel's SK template argument.
enum GemmKind { kGemmTiles = 0, kGemmStreamK = 1, kGemmTail = 2 };
struct GemmPlan {
  int kind, grid;
  int bm, bn, m_tiles, n_tiles, n_tile0, k_steps;   // the tile, the launch's tiles (n_tile0: its first pixel tile), K-steps
  int lead_n, tail_tiles, split;                    // tail: pixel tiles of the leading rounds, tiles cut, K-ranges per cut tile; else 0
  bool wants_streamk;                               // the shape's own preference, whatever this launch got (dasac_conv_gemm_schedule)
  bool uses_workspace;
  size_t workspace_bytes;                           // what a launch of this kind needs (0: none)
};
// M x K over the pixels [pix_begin, pix_end) of Npix (whole tiles; the last one may be ragged only at the end of the tensor).
// schedule 0 = pick (split-K tail over a whole tensor, else want_streamk), 1 = one block per tile, 2 = stream-K (which needs a K-step
// per worker).  The hand-off schedules exist for the 128-row tile, with a workspace, on the whole chip (`full_chip`: the persistent
// grid and the XCD mapping are sized for the full MI355X; the launcher asks the device).
inline GemmPlan gemm_plan(int M, int K, int64_t Npix, int64_t pix_begin, int64_t pix_end, int schedule, bool workspace, int reserved,
                          bool full_chip) {
  GemmPlan p{};
  p.bm = pick_bm(conv_mpad(M));
  p.bn = p.bm == 32 ? 256 : 128;
  p.m_tiles = (M + p.bm - 1) / p.bm;
  p.n_tile0 = (int)(pix_begin / p.bn);
  p.n_tiles = (int)((pix_end - pix_begin + p.bn - 1) / p.bn);
  p.k_steps = (K + kBK - 1) / kBK;
  const bool handoff = p.bm == 128 && full_chip;
  const bool whole = p.n_tile0 == 0 && (long long)p.n_tiles * p.bn >= Npix;
  p.wants_streamk = handoff && want_streamk(p.m_tiles * p.n_tiles, p.k_steps, reserved);
  int lead_n = 0;
  const int split = (handoff && workspace && schedule == 0 && whole) ? tail_plan(p.m_tiles, p.n_tiles, p.k_steps, reserved, lead_n) : 0;
  const bool sk_ok = handoff && workspace && (long long)p.m_tiles * p.n_tiles * p.k_steps >= sk_workers(reserved);
  if (split > 0) {
    p.kind = kGemmTail;
    p.lead_n = lead_n;
    p.tail_tiles = (p.n_tiles - lead_n) * p.m_tiles;
    p.split = split;
    p.grid = round_up_xcd(lead_n) * p.m_tiles + round_up_xcd(p.tail_tiles) * split;
  } else if (sk_ok && (schedule == 2 || (schedule == 0 && p.wants_streamk))) {
    p.kind = kGemmStreamK;
    p.grid = sk_workers(reserved);
  } else {
    p.kind = kGemmTiles;
    p.grid = round_up_xcd(p.n_tiles) * p.m_tiles;
  }
  p.uses_workspace = p.kind != kGemmTiles;
  p.workspace_bytes = p.uses_workspace ? kGemmWorkspaceBytes : 0;
  return p;
}

// ---- host rules: the weight gradient -----------------------------------------------------------------------------------------
inline int wgrad_bn(int Cx) { return (Cx % 128 != 0 && Cx % 64 == 0) ? 64 : 128; }   // k-tile rows: one tap per tile when possible

// Number of pixel splits: every block of a wgrad launch runs for the same time, so pick the split count in 1..max_splits whose block
// total fills whole rounds of resident blocks.
inline int fill_rounds(int tiles, int max_splits, int slots) {
  int best = 1;
  double best_eff = 0.0;
  for (int sp = 1; sp <= max_splits; ++sp) {
    const int blocks = tiles * sp;
    const int rounds = (blocks + slots - 1) / slots;
    const double eff = (double)blocks / ((double)rounds * slots);
    if (eff > best_eff + 0.02) {                             // prefer fewer splits unless clearly better
      best_eff = eff;
      best = sp;
    }
  }
  return best;
}
// `cap`: kWgMaxSplits, or more where few tiles face many pixels
inline int wgrad_splits(int tiles, int64_t Npix, int cap) {
  int64_t max_splits = (Npix + kWgMinPix - 1) / kWgMinPix;
  if (max_splits > cap) max_splits = cap;
  return fill_rounds(tiles, (int)max_splits, kWgSlots);
}
inline int wgrad_splits(int Mpad, int Kpad, int Npix, int bm, int bnk) {
  const int tiles = (Mpad / bm) * (Kpad / bnk);
  return wgrad_splits(tiles, Npix, (tiles < kWgFewTiles && Npix >= kWgManyPix) ? (kWgSlots + tiles - 1) / tiles : kWgMaxSplits);
}
// pixels per split: an equal share rounded UP to whole K-steps, so trailing splits can start at or past the last pixel
inline int wgrad_per(int Npix, int splits) { return ((Npix + splits - 1) / splits + kWgPix - 1) / kWgPix * kWgPix; }

// Where a weight-gradient launch puts its slabs: the M tile, the k-tile width (one tap per tile when the channel count allows), the
// pixel splits and the workspace [splits][Mpad][Kpad] slabs, then [splits][Mpad] channel sums.  conv_wgrad writes by it and the
// finishers find Psum behind `splits` slabs by it: one rule, because two spellings that drift apart would read the wrong slab silently.
struct WgradPlan {
  int Mpad, Kpad, bm, bnk, m_tiles, k_tiles;
  int splits, per, grid;             // pixel splits, pixels per split (whole K-steps), blocks
  size_t slab, psum_offset;          // floats: one split's slab, where the channel sums start
  size_t workspace_bytes;            // upper bound over both k-tile widths (the width depends on Cx, which the size query does not know)
};
inline WgradPlan wgrad_plan(int M, int K, int Cx, int Npix) {
  WgradPlan p;
  p.Mpad = conv_mpad(M);
  p.Kpad = conv_kpad(K);
  p.bm = pick_bm(p.Mpad);
  p.bnk = (M % 8 == 0 && p.bm != 32) ? wgrad_bn(Cx) : 128;
  p.m_tiles = p.Mpad / p.bm;
  p.k_tiles = p.Kpad / p.bnk;
  p.splits = wgrad_splits(p.Mpad, p.Kpad, Npix, p.bm, p.bnk);
  p.per = wgrad_per(Npix, p.splits);
  p.grid = round_up_xcd(p.m_tiles * p.k_tiles * p.splits);
  p.slab = (size_t)p.Mpad * p.Kpad;
  p.psum_offset = (size_t)p.splits * p.slab;
  const int s128 = wgrad_splits(p.Mpad, p.Kpad, Npix, p.bm, 128), s64 = wgrad_splits(p.Mpad, p.Kpad, Npix, p.bm, 64);
  p.workspace_bytes = (size_t)(s128 > s64 ? s128 : s64) * p.Mpad * (p.Kpad + 1) * sizeof(float);     // slabs + per-split channel sums
  return p;
}

// `batch` weight gradients over plain matrices A [batch][M][T], B [batch][C][T] as one launch: the splits are chosen over all
// batch * m_tiles * k_tiles tiles (the same rule, the plain cap); splits == 0 = the launch does not take this shape.  Workspace:
// [splits][batch][M][C] slabs, then [splits][M] row sums.
struct WgradBatchedPlan {
  int m_tiles, k_tiles, splits, per, grid;          // grid: blocks per batch entry (grid x)
  size_t psum_offset, workspace_bytes;
};
inline WgradBatchedPlan wgrad_batched_plan(int batch, int M, int C, int T) {
  WgradBatchedPlan p{};
  if (batch < 1 || batch > 65535 || M <= 0 || C <= 0 || T <= 0 || M % 128 || C % 128 || T % 4) return p;
  if ((int64_t)M * T * 4 >= (1ll << 31) || (int64_t)C * T * 4 >= (1ll << 31)) return p;   // an entry's window, the scalar row offsets
  if ((int64_t)batch * M * C * 4 > kMaxTensorBytes) return p;                               // one split's slabs: at most 2^16 tiles
  const int splits = wgrad_splits(batch * (M / 128) * (C / 128), T, kWgMaxSplits);
  if ((int64_t)splits * batch * M * C * 4 > kMaxTensorBytes) return p;
  p.m_tiles = M / 128;
  p.k_tiles = C / 128;
  p.splits = splits;
  p.per = wgrad_per(T, splits);
  p.grid = round_up_xcd(p.m_tiles * p.k_tiles * splits);
  p.psum_offset = (size_t)splits * batch * M * C;
  p.workspace_bytes = (size_t)splits * ((size_t)batch * M * C + M) * sizeof(float);          // slabs + per-split row sums
  return p;
}

// ---- device map: the GEMM, one block per tile ---------------------------------------------------------------------------------
// Block b runs on XCD b % 8: tiles that are adjacent -- same activation tile, next M tile -- go to the same XCD so that they share
// its L2.  A block's work is [it, it_end) of the (tile, K-step) space (tile-major; tiles * KT < 2^31, checked by the host).  (The
// maps of the two hand-off schedules -- stream-K ranges, tail pieces, their deposit slots -- are written inside conv_gemm: on
// functions of this header one timing row of each missed its bound, profiles/conv_plan.md.)
struct GemmWork {
  bool has_work;
  int it, it_end;
};

// one block per tile: each XCD owns a CONTIGUOUS run of pixel tiles (spatial neighbours share halo rows in its L2)
// (no early return in the maps: `has_work` is a plain comparison, the kernel returns on it and the compiler sinks the rest behind
// that branch -- the code the kernels had with the map written inline)
DASAC_PLAN_HD GemmWork gemm_tile_work(int bid, int m_tiles, int n_tiles, int KT) {
  const int xcd = bid % kNumXcd, slot = bid / kNumXcd;
  const int per_xcd = (n_tiles + kNumXcd - 1) / kNumXcd;
  const int n_local = slot / m_tiles;
  const int n_tile = xcd * per_xcd + n_local;
  const int it = (n_tile * m_tiles + slot % m_tiles) * KT;
  return GemmWork{!(n_local >= per_xcd || n_tile >= n_tiles), it, it + KT};
}

// ---- device map: the weight gradient -----------------------------------------------------------------------------------------
// Block b runs on XCD b % 8: give every XCD a CONTIGUOUS run of the (split-major) block list, so that the tiles of a pixel split --
// which all stream the same dZ and X pixels -- meet in one L2 instead of being fetched by all eight.  p_end <= p_begin: a trailing
// split without pixels (its block still writes a slab of zeros).
struct WgradTile {
  int m_tile, k_tile, split;
};
struct PixelRange {
  int begin, end;
};
// position of block `bid` in the split-major block list; at or past n_blocks: a block without work.  (`bid`: an int, or the kernel's
// blockIdx.x ITSELF, unread -- it is then read here, after the blocks per XCD are formed, where the kernels always read it: the
// compiler keeps that order, and with it the kernels' instruction streams.)
template <typename Bid>
DASAC_PLAN_HD int wgrad_list_index(const Bid& bid, int n_blocks) {
  const int per_xcd = (n_blocks + kNumXcd - 1) / kNumXcd;
  return ((int)(unsigned)bid % kNumXcd) * per_xcd + (int)(unsigned)bid / kNumXcd;
}
DASAC_PLAN_HD WgradTile wgrad_tile(int lb, int m_tiles, int k_tiles) {
  const int tile = lb % (m_tiles * k_tiles), split = lb / (m_tiles * k_tiles);
  return WgradTile{tile % m_tiles, tile / m_tiles, split};
}
DASAC_PLAN_HD PixelRange wgrad_pixels(int split, int pix_per_split, int Npix) {
  const int p_begin = split * pix_per_split;
  const int p_last = p_begin + pix_per_split;
  return PixelRange{p_begin, p_last < Npix ? p_last : Npix};
}

}  // namespace dasac
