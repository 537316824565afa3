// The SAC head on MI355X, the losses: cross entropy / focal cross entropy over [B,C,H,W] fp32 logits (C = 19), and its backward
// fused with the transpose of the bilinear upsampling.  HBM-bound streaming passes: lanes run along pixels (coalesced NCHW plane
// reads), the class dimension is a register loop.
//
//   ce_loss            models/deeplabv2.py:223-224, models/sac.py:119-149  CE / focal CE(+conf) value and dlogits
//   ce_bwd_rows[_wave] the same gradient taken straight to the stride-8 logits (upsample_bwd_x fused in; upsample.hip's
//                      upsample_bwd_y finishes)
// The index rules of the fused backward and the two launch plans are upsample_index.hpp's (tools/ce_bwd_plan_check.cpp walks them).
#include "head_common.hpp"
#include "upsample_index.hpp"

#include <algorithm>
#include <atomic>

namespace dasac {

constexpr float kQ28 = 268435456.f;      // fixed-point scale of the order-independent (integer) per-class sums

// ---- cross entropy -------------------------------------------------------------------------
// Each thread loops over the B images of its pixels (needed by the cross-batch product
// of sac.py:148):   loss = sum_hw pw(hw) * sum_b ce_b(hw),
//   mode 0  plain mean (deeplabv2.py:224, sac.py:132):  pw = 1/(B*HW)
//   mode 1  focal_ce_conf (sac.py:148):                 pw = sum_i conf_i(hw) / (B*B*HW)
// ce_b = -cw[y]*log_softmax(x)[y], 0 where y == 255.  dlogits (optional) = pw * cw[y] * (softmax - onehot).
// per_class (optional, [C] Q28 fixed-point accumulators): sum over pixels of ce scattered by label (ignored pixels add nothing).
// Four consecutive pixels per thread (the [B,C,HW] layout is contiguous in the flattened pixel index): every class plane
// is one 4-byte-aligned dwordx4 load and all CT of an image are in flight together.
template <int CT>
__global__ __launch_bounds__(kHB) void ce_loss(const float* __restrict__ x, const int64_t* __restrict__ y,
                                               const float* __restrict__ cw, const float* __restrict__ conf, int B, int Crt,
                                               int HW, int mode, const float* __restrict__ gscale, float* __restrict__ dx,
                                               double* __restrict__ partial, unsigned long long* __restrict__ per_class) {
  const int C = CT < kMaxC ? CT : Crt;
  double lsum = 0.0;
  __shared__ unsigned long long s_pc[kMaxC];
  if (per_class) {
    if (threadIdx.x < kMaxC) s_pc[threadIdx.x] = 0ull;
    __syncthreads();
  }
  const float gs = gscale ? gscale[0] : 1.f;   // upstream gradient of the scalar loss (device side)
  const float norm = mode == 1 ? 1.f / ((float)B * (float)B * (float)HW) : 1.f / ((float)B * (float)HW);
  const int items = (HW + 3) >> 2;
  for (int it = blockIdx.x * kHB + threadIdx.x; it < items; it += gridDim.x * kHB) {
    const int p = it * 4, nx = min(4, HW - p);
    float cs[4] = {1.f, 1.f, 1.f, 1.f};
    if (mode == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[e] = 0.f;
      for (int b = 0; b < B; ++b) {
        if (nx == 4) {
          const f32x4u cv = *reinterpret_cast<const f32x4u*>(conf + (size_t)b * HW + p);
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[e] += cv[e];
        } else {
#pragma unroll
          for (int e = 0; e < 3; ++e)
            if (e < nx) cs[e] += conf[(size_t)b * HW + p + e];
        }
      }
    }
    float pw[4], cesum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) pw[e] = cs[e] * norm;
    for (int b = 0; b < B; ++b) {
      const size_t base = (size_t)b * C * HW + p;
      f32x4u v[CT];
      if (nx == 4) {                                     // ONE branch around all CT loads, not one per plane
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) v[c] = load_quad(x + base + (size_t)c * HW, 4);
      } else {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) v[c] = load_quad(x + base + (size_t)c * HW, nx);
      }
      int64_t lab[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) lab[e] = e < nx ? y[(size_t)b * HW + p + e] : (int64_t)-1;
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, den[4] = {0.f, 0.f, 0.f, 0.f}, xl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
#pragma unroll
          for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], v[c][e]);
        }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (c == lab[e]) xl[e] = v[c][e];
            const float ex = expf(v[c][e] - mx[e]);
            den[e] += ex;
            v[c][e] = ex;
          }
        }
      float k[4], gw[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool valid = lab[e] >= 0 && lab[e] < C;   // 255 (ignore) and anything out of range carry no loss
        const float wgt = valid ? (cw ? cw[lab[e]] : 1.f) : 0.f;
        const float ce = valid ? wgt * (logf(den[e]) - (xl[e] - mx[e])) : 0.f;
        cesum[e] += ce;
        // Q28 two's-complement fixed point: integer adds commute, so the scatter is bit-identical from run to run
        // (exact for ce >= 2^-4, 2^-29 rounding below; |ce| clamped to 4096: N*4096*2^28 < 2^63 for N < 2^23 pixels)
        if (per_class && valid && ce != 0.f && e < nx)
          atomicAdd(&s_pc[lab[e]], (unsigned long long)__float2ll_rn(fminf(fmaxf(ce, -4096.f), 4096.f) * kQ28));
        gw[e] = pw[e] * gs * wgt;
        k[e] = gw[e] / den[e];
      }
      if (dx) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) {
            f32x4u d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = k[e] * v[c][e] - ((c == lab[e]) ? gw[e] : 0.f);
            store_quad(dx + base + (size_t)c * HW, d, nx);
          }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nx) lsum += (double)pw[e] * (double)cesum[e];
  }
  __shared__ double red[kHB / 64];
  lsum = wave_sum(lsum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  if (per_class && threadIdx.x < C && s_pc[threadIdx.x] != 0ull) atomicAdd(&per_class[threadIdx.x], s_pc[threadIdx.x]);
}

__global__ void ce_finish(const double* __restrict__ partial, int n, float* __restrict__ loss,
                          const unsigned long long* __restrict__ per_class, float* __restrict__ per_class_out, int C, double pc_norm) {
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = (float)s;
  if (per_class_out && threadIdx.x < C)
    per_class_out[threadIdx.x] = (float)((double)(long long)per_class[threadIdx.x] * (1.0 / 268435456.0) * pc_norm);
}

// ---- cross-entropy backward straight into the low-resolution gradient (K15 -> K9^T) ------------------------------
// The loss is a function of logits_up = U(logits) with U the bilinear (ac=True) upsampling; its gradient w.r.t. the
// stride-8 logits is U^T applied to the per-pixel d loss / d logits_up.  The two-kernel path wrote that full-resolution
// tensor (359.5 MB for 8 crops) and read it back; here one block per high-res row (b, y) keeps it in LDS:
//   phase 1  lanes along x (coalesced class-plane reads): softmax + the ce_loss weights -> d[c][x] in LDS,
//   phase 2  x-reduction with the horizontal tap weights -> tmp[(b,c)][y][j]   (same weights, same summation order as
//            upsample_bwd_x, so the result is the two-kernel path's bit for bit),
// and upsample_bwd_y finishes with the vertical taps.  LDS index x + x/8 spreads the stride-8 phase-2 reads over all banks.

// Round 4: a block handles a SEGMENT of `seg_cols` low-resolution columns of one high-res row (the x range their taps touch,
// a few hundred pixels) instead of the whole row: 19 x ~300 floats of LDS instead of 19 x 867 (66 KB, two blocks per CU whose
// two serial phases rarely overlapped) -- six 128-thread blocks per CU, phases of different blocks overlap.  The pixels between
// two segments' column ranges are evaluated by both (softmax is per pixel: same bits); every column is summed by ONE block over
// ascending x exactly as before, so the result stays bit-identical to dasac_ce_loss(dlogits) + dasac_upsample_bwd.
// cs[p] = sum_i conf_i[p] in image order (0 + c_0 + c_1 + ...: the order every row block used to repeat for itself, B times over)
__global__ __launch_bounds__(256) void conf_pixel_sums(const float* __restrict__ conf, int B, int HW, float* __restrict__ cs) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a += conf[(size_t)bb * HW + p];
    cs[p] = a;
  }
}

constexpr int kCB = 128;
template <int CT>
__global__ __launch_bounds__(kCB) void ce_bwd_rows(const float* __restrict__ xup, const int64_t* __restrict__ y,
                                                  const float* __restrict__ cw, const float* __restrict__ conf, int B, int Crt,
                                                  int H, int W, int w, float sw, int mode, const float* __restrict__ gscale,
                                                  float* __restrict__ tmp, int seg_cols, int n_seg, int pitch,
                                                  const float* __restrict__ cs_pix) {
  extern __shared__ float s_d[];                      // [C][pitch]
  const int C = CT < kMaxC ? CT : Crt;
  const int seg = blockIdx.x % n_seg, rowid = blockIdx.x / n_seg;
  const int b = rowid / H, oy = rowid - b * H;
  const int j0 = seg * seg_cols, j1 = min(w, j0 + seg_cols);
  int xs, xe;
  segment_range(j0, j1, sw, W, xs, xe);
  const int HW = H * W;
  const float gs = gscale ? gscale[0] : 1.f;
  const float norm = mode == 1 ? 1.f / ((float)B * (float)B * (float)HW) : 1.f / ((float)B * (float)HW);
  // phase 1: four consecutive pixels per thread -- every class plane is ONE (4-byte aligned) dwordx4 load and all CT of
  // them are in flight together (compile-time class count: no per-class predicate between the loads)
  for (int ox = xs + threadIdx.x * 4; ox <= xe; ox += kCB * 4) {
    const int nx = min(4, W - ox);
    const int p = oy * W + ox;
    const size_t base = (size_t)b * C * HW + p;
    f32x4u v[CT];
    if (nx == 4) {                                     // ONE branch around all CT loads, not one per plane
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) v[c] = load_quad(xup + base + (size_t)c * HW, 4);
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) v[c] = load_quad(xup + base + (size_t)c * HW, nx);
    }
    float cs[4] = {1.f, 1.f, 1.f, 1.f};
    if (mode == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[e] = 0.f;
      if (cs_pix) {                                       // sum_i conf_i per pixel, added up ONCE per launch (conf_pixel_sums)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nx) cs[e] = cs_pix[p + e];
      } else if (nx == 4) {
#pragma unroll 8
        for (int bb = 0; bb < B; ++bb) {
          const f32x4u cv = *reinterpret_cast<const f32x4u*>(conf + (size_t)bb * HW + p);
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[e] += cv[e];
        }
      } else {
        for (int bb = 0; bb < B; ++bb) {
          const float* cp = conf + (size_t)bb * HW + p;
#pragma unroll
          for (int e = 0; e < 3; ++e)
            if (e < nx) cs[e] += cp[e];
        }
      }
    }
    int64_t lab[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lab[e] = e < nx ? y[(size_t)b * HW + p + e] : (int64_t)-1;
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], v[c][e]);
      }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[c][e] = expf(v[c][e] - mx[e]);
          den[e] += v[c][e];
        }
      }
    float k[4], gw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool valid = lab[e] >= 0 && lab[e] < C;
      const float wgt = valid ? (cw ? cw[lab[e]] : 1.f) : 0.f;
      const float gpw = cs[e] * norm * gs;
      gw[e] = gpw * wgt;
      k[e] = gw[e] / den[e];
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nx) s_d[c * pitch + ce_lds_index(ox + e - xs)] = k[e] * v[c][e] - ((c == lab[e]) ? gw[e] : 0.f);
      }
  }
  __syncthreads();
  // phase 2: thread -> (column j, class group).  The tap weights of column j are computed once (registers) and reused
  // for every class of the group; the sum runs over ascending x like upsample_bwd_x does.
  constexpr int kMaxSpan = 24;                           // 2/scale + 3 taps: covers up-factors to 10
  const int nj = j1 - j0;
  const int groups = max(1, min(C, kCB / max(nj, 1)));
  for (int o = threadIdx.x; o < nj * groups; o += kCB) {
    const int j = j0 + o % nj, g0 = o / nj;
    int lo, hi;
    src_range(j, sw, W, lo, hi);
    const int n = hi - lo + 1;
    if (n <= kMaxSpan) {
      float wt[kMaxSpan];
      int li[kMaxSpan];
#pragma unroll
      for (int i = 0; i < kMaxSpan; ++i) {
        wt[i] = i < n ? weight_to(lo + i, sw, w, j) : 0.f;
        li[i] = ce_lds_index(min(lo + i, W - 1) - xs);
      }
      for (int c = g0; c < C; c += groups) {
        const float* row = s_d + c * pitch;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxSpan; ++i)
          if (i < n) acc += wt[i] * row[li[i]];
        tmp[((size_t)(b * C + c) * H + oy) * w + j] = acc;
      }
    } else {
      for (int c = g0; c < C; c += groups) {
        float acc = 0.f;
        for (int xx = lo; xx <= hi; ++xx) acc += weight_to(xx, sw, w, j) * s_d[c * pitch + ce_lds_index(xx - xs)];
        tmp[((size_t)(b * C + c) * H + oy) * w + j] = acc;
      }
    }
  }
}

// Round 5: the same two phases with ONE WAVE per block walking `rows` consecutive high-res rows of its segment.
// What the kernel above spends its time on (tools/isa_count.py, the PMC table): every block loads, waits, computes, synchronises
// and reduces exactly once -- the 19 plane loads of a row are never in flight while anything else happens, each row rebuilds the
// (row-independent) tap weights of its columns (as many instructions as the reduction itself), and 75 of its 128 threads have a
// quad in phase 1.  Here
//   * the x range of a segment is at most 256 pixels = one quad per lane, and the NEXT row's planes, labels and confidence sums
//     are requested right after this row's softmax has left the registers: they land during phase 2;
//   * a thread keeps its column's SPAN tap weights and LDS indices in registers for all rows;
//   * a one-wave block needs no cross-wave barrier, and seven of them fit a CU (22 KB of LDS each).
// Per pixel and per column the arithmetic and its order are those of ce_bwd_rows: identical bits.
constexpr int kCW = 64;
static_assert(kCW == kCeWaveLanes, "ce_wave_plan sizes its segments for this block");
template <int CT, int SPAN>
__global__ __launch_bounds__(kCW, 2) void ce_bwd_rows_wave(const float* __restrict__ xup, const int64_t* __restrict__ y,
                                                       const float* __restrict__ cw, int B, int H, int W, int w, float sw, int mode,
                                                       const float* __restrict__ gscale, float* __restrict__ tmp, int seg_cols,
                                                       int n_seg, int pitch, const float* __restrict__ cs_pix, int rows, int n_chunks) {
  extern __shared__ float s_d[];                      // [CT][pitch]
  const int seg = blockIdx.x % n_seg, rest = blockIdx.x / n_seg;
  const int rc = rest % n_chunks, b = rest / n_chunks;
  const int y0 = rc * rows, y1 = min(H, y0 + rows);
  const int j0 = seg * seg_cols, j1 = min(w, j0 + seg_cols);
  int xs, xe;
  segment_range(j0, j1, sw, W, xs, xe);
  const int HW = H * W;
  const float gs = gscale ? gscale[0] : 1.f;
  const float norm = mode == 1 ? 1.f / ((float)B * (float)B * (float)HW) : 1.f / ((float)B * (float)HW);
  // phase-1 role: the quad at xs + 4 * lane (ce_wave_plan guarantees xe - xs < 256 and W >= 4).  A quad that hangs over the end
  // of the row is LOADED four pixels back from the row's end and rotated into place (one lane of one segment per row): every
  // load is a full dwordx4, and a quad's four LDS slots are consecutive (xs and the quads are multiples of 4, the index skew
  // steps every 8), so the 76 LDS writes take 19 base registers + immediate offsets.
  const int ox = xs + (int)threadIdx.x * 4;
  const bool act = ox <= xe;
  const int rot = max(0, ox + 4 - W), ox_ld = ox - rot;
  // phase-2 role: column j, classes g0, g0 + groups, ...
  const int nj = j1 - j0;
  const int groups = max(1, min(CT, kCW / nj));
  const bool red = (int)threadIdx.x < nj * groups;
  const int j = j0 + (int)threadIdx.x % nj, g0 = (int)threadIdx.x / nj;
  // its taps: src_range is generous by two positions on either side; the zero weights at both ends are dropped, and the slots
  // behind the last tap (up to SPAN) carry weight 0 on that tap's LDS index.  acc starts at +0 and can never become -0, so
  // adding 0 * (a finite gradient) anywhere leaves every bit of the sum as it is: no predicate on the accumulation.
  int lo, hi;
  ce_taps(j, sw, W, w, lo, hi);
  const int n = hi - lo + 1;                              // <= SPAN (ce_wave_plan)
  float wt[SPAN];
  unsigned la[SPAN];                                      // LDS byte offsets inside a class row
#pragma unroll
  for (int i = 0; i < SPAN; ++i) {
    wt[i] = i < n ? weight_to(lo + i, sw, w, j) : 0.f;
    la[i] = (unsigned)ce_lds_index(min(lo + i, hi) - xs) * 4u;
  }
  const unsigned row_bytes = (unsigned)pitch * 4u;
  float* const tmp_col = tmp + ((size_t)b * CT * H) * w + j;  // + (c * H + oy) * w
  __shared__ float s_cw[CT];                              // class weights: an LDS lookup by label, not a dependent global load
  if (threadIdx.x < CT) s_cw[threadIdx.x] = cw ? cw[threadIdx.x] : 1.f;
  __syncthreads();
  f32x4u v[CT];
  f32x4u cs;
  int64_t lab[4];
  auto load_row = [&](int oy) {
    if (!act) return;
    const int p = oy * W + ox_ld;
    const float* base = xup + (size_t)b * CT * HW + p;
    const int64_t* yp = y + (size_t)b * HW + p;
#pragma unroll
    for (int c = 0; c < CT; ++c) v[c] = *reinterpret_cast<const f32x4u*>(base + (size_t)c * HW);
    const i64x2u l01 = *reinterpret_cast<const i64x2u*>(yp), l23 = *reinterpret_cast<const i64x2u*>(yp + 2);
    lab[0] = l01[0]; lab[1] = l01[1]; lab[2] = l23[0]; lab[3] = l23[1];
    cs = mode == 1 ? *reinterpret_cast<const f32x4u*>(cs_pix + p) : f32x4u{1.f, 1.f, 1.f, 1.f};
  };
  load_row(y0);
  for (int oy = y0; oy < y1; ++oy) {
    if (act) {
      if (rot) {                                          // element e <- element e + rot (what lands beyond the row is never read)
        auto turn = [&](auto& q) {
          q[0] = rot == 1 ? q[1] : (rot == 2 ? q[2] : q[3]);
          q[1] = rot == 1 ? q[2] : q[3];
          q[2] = q[3];
        };
#pragma unroll
        for (int c = 0; c < CT; ++c) turn(v[c]);
        turn(cs);
      }
      int lb[4];                                          // label, or -1 (ignored / out of range: matches no class)
#pragma unroll
      for (int e = 0; e < 4; ++e) lb[e] = (lab[e] >= 0 && lab[e] < CT) ? (int)lab[e] : -1;
      if (rot) {
        lb[0] = rot == 1 ? lb[1] : (rot == 2 ? lb[2] : lb[3]);
        lb[1] = rot == 1 ? lb[2] : lb[3];
        lb[2] = lb[3];
      }
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx[e] = fmaxf(mx[e], v[c][e]);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[c][e] = expf(v[c][e] - mx[e]);
          den[e] += v[c][e];
        }
      float k[4], gw[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float wgt = lb[e] >= 0 ? s_cw[max(lb[e], 0)] : 0.f;
        const float gpw = cs[e] * norm * gs;
        gw[e] = gpw * wgt;
        k[e] = gw[e] / den[e];
      }
      float* wr = s_d + ce_lds_index(ox - xs);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[c * pitch + e] = k[e] * v[c][e] - ((c == lb[e]) ? gw[e] : 0.f);
    }
    __builtin_amdgcn_sched_barrier(0);                    // not earlier: the next row reuses this row's 76 registers
    if (oy + 1 < y1) load_row(oy + 1);                    // in flight while this row is reduced
    __syncthreads();
    if (red) {
#pragma unroll 1
      for (int c = g0; c < CT; c += groups) {
        const char* row = reinterpret_cast<const char*>(s_d) + (unsigned)c * row_bytes;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < SPAN; ++i) acc += wt[i] * *reinterpret_cast<const float*>(row + la[i]);
        tmp_col[(unsigned)(c * H + oy) * (unsigned)w] = acc;
      }
    }
    __syncthreads();
  }
}

}  // namespace dasac

using namespace dasac;

static int ce_blocks(int64_t HW) { return stream_grid((HW + 3) / 4, kHB, kNumCu * 8); }

extern "C" size_t dasac_ce_loss_workspace(int B, int C, int64_t HW) {
  return align_up((size_t)ce_blocks(HW) * sizeof(double), 256) + align_up((size_t)kMaxC * sizeof(double), 256);
}

extern "C" int dasac_ce_loss(const float* logits, const int64_t* labels, const float* class_weight, const float* conf,
                             int B, int C, int64_t HW, int mode, const float* gscale, float* loss, float* dlogits,
                             float* per_class, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(logits && labels && loss && workspace, "ce_loss: null pointer");
  DASAC_REQUIRE(B > 0 && C > 0 && C <= kMaxC && HW > 0 && HW < (1ll << 31) && (mode == 0 || (mode == 1 && conf)), "ce_loss: bad arguments");
  if (ws_bytes < dasac_ce_loss_workspace(B, C, HW)) return fail(DASAC_EWORKSPACE, "ce_loss: workspace too small");
  hipStream_t s = as_stream(stream);
  const int blocks = ce_blocks(HW);
  double* partial = reinterpret_cast<double*>(workspace);
  unsigned long long* pc =
      reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + align_up((size_t)blocks * sizeof(double), 256));
  if (per_class) DASAC_HIP(hipMemsetAsync(pc, 0, kMaxC * sizeof(double), s));
  dispatch_classes(C, [&](auto ct) {
    hipLaunchKernelGGL(ce_loss<decltype(ct)::value>, dim3(blocks), dim3(kHB), 0, s, logits, labels, class_weight, conf, B, C, (int)HW, mode,
                       gscale, dlogits, partial, per_class ? pc : nullptr);
  });
  DASAC_CHECK_LAUNCH("ce_loss");
  hipLaunchKernelGGL(ce_finish, dim3(1), dim3(64), 0, s, partial, blocks, loss, pc, per_class, C, 1.0 / ((double)HW * B));
  DASAC_CHECK_LAUNCH("ce_finish");
  return DASAC_OK;
}

// tmp [B*C][H][w] floats, then (rounded up to 256 bytes) room for the per-pixel confidence sums of mode 1: H * kCeMaxW floats would
// over-allocate, so the sums live in the tail only when H * W is known to fit -- the launcher checks ws_bytes and falls back
static size_t ce_bwd_tmp_bytes(int B, int C, int H, int w) { return align_up((size_t)B * C * H * w * sizeof(float), 256); }
extern "C" size_t dasac_ce_loss_bwd_low_workspace(int B, int C, int H, int w) {
  // the confidence sums need H*W floats; W is not an argument here: w * 16 covers every up-factor to 16 (the backbone's is 8)
  return ce_bwd_tmp_bytes(B, C, H, w) + (size_t)H * w * 16 * sizeof(float);
}

extern "C" int dasac_ce_loss_bwd_low(const float* logits_up, const int64_t* labels, const float* class_weight, const float* conf,
                                     int B, int C, int H, int W, int h, int w, int mode, const float* gscale, float* grad_low,
                                     void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(logits_up && labels && grad_low && workspace, "ce_loss_bwd_low: null pointer");
  DASAC_REQUIRE(B > 0 && C > 0 && C <= kMaxC && H > 0 && W > 0 && h > 0 && w > 0 && (int64_t)H * W < (1ll << 31) &&
                    (mode == 0 || (mode == 1 && conf)),
                "ce_loss_bwd_low: bad arguments");
  if (ws_bytes < ce_bwd_tmp_bytes(B, C, H, w)) return fail(DASAC_EWORKSPACE, "ce_loss_bwd_low: workspace too small");
  const float sw = ac_scale(w, W);
  const CeRowsPlan rp = ce_rows_plan(w, W, sw);
  const size_t lds = (size_t)C * rp.pitch * sizeof(float);
  DASAC_REQUIRE(lds <= 160 * 1024, "ce_loss_bwd_low: a segment of C x W gradients does not fit LDS");
  hipStream_t s = as_stream(stream);
  float* tmp = reinterpret_cast<float*>(workspace);
  if (lds > 64 * 1024) {                                 // raise the kernels' dynamic-LDS limit once per device, not per launch
    static std::atomic<unsigned long long> raised{0};
    int dev = 0;
    DASAC_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
      DASAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ce_bwd_rows<19>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      DASAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ce_bwd_rows<kMaxC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised.fetch_or(bit, std::memory_order_relaxed);
    }
  }
  DASAC_REQUIRE((int64_t)B * H * rp.n_seg < (1ll << 31), "ce_loss_bwd_low: grid too large");
  // mode 1: every image's rows need sum_i conf_i of their pixels -- B x B plane reads if each block adds them up itself; one pass
  // into the workspace tail instead (when the caller's workspace has the room: H * W floats behind tmp)
  const float* cs_pix = nullptr;
  if (mode == 1 && B > 1 && ws_bytes >= ce_bwd_tmp_bytes(B, C, H, w) + (size_t)H * W * sizeof(float)) {
    float* cs = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + ce_bwd_tmp_bytes(B, C, H, w));
    hipLaunchKernelGGL(conf_pixel_sums, dim3(stream_grid((int64_t)H * W, 256)), dim3(256), 0, s, conf, B, H * W, cs);
    DASAC_CHECK_LAUNCH("conf_pixel_sums");
    cs_pix = cs;
  }
  // the one-wave kernel: 19 classes, confidence sums precomputed, and what ce_wave_plan asks of the geometry
  bool wave_done = false;
  if (C == 19 && (mode == 0 || cs_pix)) {
    const CeWavePlan wp = ce_wave_plan(B, H, w, W, sw, kNumCu - reserved_cus());
    if (wp.ok) {
      const dim3 grid((unsigned)(B * wp.n_chunks * wp.n_seg));
      const size_t wlds = (size_t)C * wp.pitch * sizeof(float);
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kCW), wlds, s, logits_up, labels, class_weight, B, H, W, w, sw, mode, gscale, tmp, wp.cols,
                           wp.n_seg, wp.pitch, cs_pix, wp.rows, wp.n_chunks);
      };
      if (wp.taps <= 16) launch(ce_bwd_rows_wave<19, 16>); else launch(ce_bwd_rows_wave<19, 24>);
      wave_done = true;
    }
  }
  if (!wave_done)
    dispatch_classes(C, [&](auto ct) {
      hipLaunchKernelGGL(ce_bwd_rows<decltype(ct)::value>, dim3(B * H * rp.n_seg), dim3(kCB), lds, s, logits_up, labels, class_weight, conf,
                         B, C, H, W, w, sw, mode, gscale, tmp, rp.seg_cols, rp.n_seg, rp.pitch, cs_pix);
    });
  DASAC_CHECK_LAUNCH("ce_bwd_rows");
  return launch_upsample_bwd_y(tmp, (int64_t)B * C, H, h, w, nullptr, grad_low, s);
}
