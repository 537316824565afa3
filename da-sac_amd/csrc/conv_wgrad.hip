// Weight gradient of the implicit-GEMM convolution (conv_gemm.hip has the contraction and the gather it shares):
//   G[m][k] = sum_pix dZ[m][pix] * gather(X, k, pix)
// as per-split partial slabs (conv_wgrad; conv_wgrad_batched for the 16 point contractions of a Winograd weight gradient) and the
// fixed-order reductions of those slabs into dW.  Replaces the weight half of autograd's convolution backward for every nn.Conv2d of
// the reference backbone (models/deeplabv2.py:59,65-66,70,107; models/fcn.py:49,53,57,78,88).
// Tiles, pixel splits, grid and workspace layout of a launch (wgrad_plan, wgrad_batched_plan) and the block map both kernels decode
// their block id with are conv_plan.hpp's: plain C++, walked on the host by tools/conv_plan_check.cpp.
#include "conv_common.hpp"

namespace dasac {

// ------------------------------------------------------------------------------------------
// weight-gradient kernel: reduction over pixels, split across blocks
//   P[split][m][k] = sum_{pix in chunk} dZ[m][pix] * gather(X,k,pix)
// LDS tiles keep the natural [row][pix] order with an odd row pitch (33) so that both the
// coalesced tile writes and the strided MFMA operand reads are bank-conflict free.
// ------------------------------------------------------------------------------------------
constexpr int kWgPitch = 36;   // row pitch (floats): 16-byte aligned rows, 16 consecutive rows x 4 dwords hit 64 distinct banks

// FAST: Cx % BN == 0 (the 128 im2col rows of a block belong to ONE tap) and M % 8 == 0: one (dh, dw)
// per block, the per-row part of both operand addresses is a scalar offset, the pixel position is
// advanced incrementally (no divisions in the loop) -> ~25 VALU per 64 MFMAs.
// X3: split-bf16 arithmetic (see conv_gemm).  The loader is unchanged (lane = pixel); every element is split
// into bf16 head + tail on its way to LDS (three VALU each: v_cvt_pk_bf16_f32 with the value in the HIGH half
// gives the head as an fp32 bit pattern directly) and stored with 16-bit writes into [octet of 8 pixels][row][8]
// operand words; the octet pitch rows+2 keeps the 64 lanes of a store on distinct banks and the 16-byte MFMA
// operand reads of consecutive rows contiguous.
template <int BM, int BN, int WAVES_M, bool FAST, bool X3, bool QUAD = false, bool QTAP = false>
__global__ __launch_bounds__(kThreads, 3) void conv_wgrad(const float* __restrict__ dZ, const float* __restrict__ X,
                                                       const int4* __restrict__ tab, float* __restrict__ P,
                                                       float* __restrict__ Psum, GemmGeom g, int m_tiles, int k_tiles,
                                                       int n_splits, int pix_per_split) {
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int A_LOADS = BM / 8, B_LOADS = BN / 8;      // 8 rows of 32 pixels per pass of 256 threads

  // ONE LDS stage (34 KB for the 128x128 tile -> 4 blocks per CU); the next tile waits in registers while the
  // MFMAs run, two barriers per step.  More co-resident blocks hide the extra barrier (measured).
  constexpr int PA = BM + 2, PB = BN + 2;                // X3: operand words per pixel octet (rows + 2)
  __shared__ __attribute__((aligned(16))) float sA[1][X3 ? 32 * PA : BM * kWgPitch];   // X3: [head|tail][4 octets][PA] x 16 B
  __shared__ __attribute__((aligned(16))) float sB[1][X3 ? 32 * PB : BN * kWgPitch];

  // which (m tile, k tile, pixel split) is mine: conv_plan.hpp
  const int n_blocks = m_tiles * k_tiles * n_splits;
  const int lb = wgrad_list_index(blockIdx.x, n_blocks);
  if (lb >= n_blocks) return;
  const WgradTile work = wgrad_tile(lb, m_tiles, k_tiles);
  const int m_tile = work.m_tile, k_tile = work.k_tile, split = work.split;
  const int m0 = m_tile * BM, kb0 = k_tile * BN;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform on purpose: scalar buffer offsets
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;
  const int pl = t & 31, prow = t >> 5;                  // loader: pixel lane, row within pass

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(X, g.x_bytes);
  const __amdgpu_buffer_rsrc_t rz = make_rsrc(dZ, g.z_bytes);

  const int OHW = g.OH * g.OW;
  const int planeHW = g.H * g.W;
  const PixelRange px = wgrad_pixels(split, pix_per_split, g.Npix);
  const int p_begin = px.begin, p_end = px.end;
  const int steps = (p_end - p_begin + kWgPix - 1) / kWgPix;

  // generic path: table rows of this thread's B loads are fixed for the whole kernel (offset, dh:dw packed)
  int te_off[FAST ? 1 : B_LOADS], te_d[FAST ? 1 : B_LOADS];
  int4 e0 = make_int4(0, 0, 0, 0);
  if (FAST) {
    e0 = tab[kb0];                                       // the block's tap: (koff, dh, dw, channel offset)
  } else {
#pragma unroll
    for (int r = 0; r < B_LOADS; ++r) {
      const int4 e = tab[kb0 + prow + r * 8];
      te_off[r] = e.x;
      te_d[r] = e.y >= kInvalid ? (int)0x80000000 : ((e.y << 16) | (e.z & 0xffff));   // dh = -32768 never in bounds
    }
  }

  const bool do_sums = (k_tile == 0) && (Psum != nullptr);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if constexpr (QUAD) {
    // ---- 1x1 stride-1 convolutions (host: one tap at (0,0), H == OH, W == OW, M % 32 == 0): FOUR consecutive pixels per lane.
    // Both operands are plain [row][pixel] matrices there, so a lane's four pixels are 16 contiguous bytes: per 64 MFMAs a
    // thread issues 4+4 dwordx4 loads and 4+4 ds_write_b128 instead of 16+16 dword loads and 16+16 ds_write_b32.  Quads that
    // leave the split or the image (the dz / x tensors are [N][rows][OH*OW]: a quad may straddle two images) send their
    // whole wave through a per-element path for that step.
    static_assert(FAST && !X3 && BM % 32 == 0 && BN % 32 == 0, "quad loader: fp32, one tap per k tile, 32-row passes");
    static_assert(!QTAP || QUAD, "the tap variant extends the quad loader");
    // QTAP (round 6): the same loader for "same"-padded stride-1 k x k convolutions (host: H == OH, W == OW >= 4, one tap per k
    // tile).  Tap (dh, dw) reads x at flat position p + dh*W + dw of the SAME plane -- contiguous for a lane's four consecutive
    // pixels whatever row boundary lies between them -- so the gathered operand takes 16-byte loads too; what the tap changes is
    // VALIDITY (the convolution's zero padding), and that is per pixel: out-of-image taps are zeroed after the load.  Most quads
    // need nothing (one compare chain + a ballot); only waves that touch a row end or the first / last dh rows run the
    // per-element masks.  Earlier rounds kept these layers on the dword loader because "tap shifts break 16-byte runs at every
    // 97-pixel row": they break ALIGNMENT (dwordx4 needs 4 bytes) and validity, not contiguity.
    constexpr int AQ = BM / 32, BQ = BN / 32;
    const int pq = t & 7, prow4 = t >> 3;                  // loader: pixel quad of the step, row within a 32-row pass
    f32x4 qa[AQ], qb[BQ];
    float qsum[AQ];
#pragma unroll
    for (int i = 0; i < AQ; ++i) qsum[i] = 0.f;
    const int zimg_q = g.M * OHW;
    int pix = p_begin + 4 * pq;                            // first pixel of this thread's quad (advanced by kWgPix per step)
    int pn = pix / OHW, prr = pix - pn * OHW;              // image, flat position inside it
    int qoh = 0, qow = 0;                                  // QTAP: row / column of the quad's first pixel
    if (QTAP) {
      qoh = prr / g.OW;
      qow = prr - qoh * g.OW;
    }
    const int tap_off = QTAP ? e0.x - e0.w : 0;            // dh*W + dw
    const unsigned x_elems = g.x_bytes >> 2;
    // x offset of (image, k tile's first channel + prow4, quad start + tap), in elements.  The k tile's first channel rides in the
    // per-lane part so that it is negative only in the first rows of image 0, channel 0 (those quads take the per-element path:
    // a wrapped unsigned offset fails the range check whatever the scalar offset adds)
#define DASAC_WGQ_LOAD()                                                                             \
  {                                                                                                  \
    const int xo = pn * g.CxHW + (QTAP ? e0.w : 0) + prr + tap_off + prow4 * planeHW;                \
    /* (the channel step of the loads below rides in the scalar offset, which the hardware's range check leaves out: a tap  \
       quad of the last image's last channels must not run past the end of x -- the per-element path poisons those lanes) */ \
    const bool whole = (pix + 3 < p_end) & (prr + 3 < OHW) &                                         \
                       (!QTAP || (xo >= 0 && (unsigned)(xo + 3 + (BQ - 1) * 32 * planeHW) < x_elems)); \
    if (__builtin_amdgcn_ballot_w64(!whole) == 0) {                                                  \
      const unsigned vz = (unsigned)(pn * zimg_q + prr + prow4 * OHW) * 4u;                          \
      const unsigned vx = (unsigned)xo * 4u;                                                         \
      _Pragma("unroll") for (int i = 0; i < AQ; ++i) qa[i] = buf_f32x4(rz, vz, (m0 + i * 32) * OHW * 4); \
      _Pragma("unroll") for (int i = 0; i < BQ; ++i) qb[i] = buf_f32x4(rx, vx, ((QTAP ? 0 : e0.w) + i * 32 * planeHW) * 4); \
      if (QTAP) {                                                                                    \
        const int c0 = qow + e0.z;                                                                   \
        const bool inside = ((unsigned)(qoh + e0.y) < (unsigned)g.H) & (c0 >= 0) & (c0 + 3 < g.W) & (qow + 3 < g.OW); \
        if (__builtin_amdgcn_ballot_w64(!inside) != 0) {                                             \
          _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                            \
            int ow_e = qow + e, oh_e = qoh;                                                          \
            if (ow_e >= g.OW) { ow_e -= g.OW; ++oh_e; }                                              \
            const bool ok = ((unsigned)(oh_e + e0.y) < (unsigned)g.H) & ((unsigned)(ow_e + e0.z) < (unsigned)g.W); \
            _Pragma("unroll") for (int i = 0; i < BQ; ++i) qb[i][e] = ok ? qb[i][e] : 0.f;           \
          }                                                                                          \
        }                                                                                            \
      }                                                                                              \
    } else {                                                                                         \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                \
        int re = prr + e, ne = pn;                                                                   \
        while (re >= OHW) { re -= OHW; ++ne; } /* maps smaller than a quad: several images per quad */ \
        const bool ve = pix + e < p_end;                                                             \
        bool vt = ve;                                                                                \
        if (QTAP) {                                                                                  \
          const int oh_e = re / g.OW, ow_e = re - oh_e * g.OW;                                       \
          vt = ve & ((unsigned)(oh_e + e0.y) < (unsigned)g.H) & ((unsigned)(ow_e + e0.z) < (unsigned)g.W); \
        }                                                                                            \
        const unsigned vz = ve ? (unsigned)(ne * zimg_q + re + prow4 * OHW) * 4u : kPoison;          \
        const unsigned vx = vt ? (unsigned)(ne * g.CxHW + re + tap_off + prow4 * planeHW) * 4u : kPoison; \
        _Pragma("unroll") for (int i = 0; i < AQ; ++i) qa[i][e] = buf_f32(rz, vz, (m0 + i * 32) * OHW * 4); \
        _Pragma("unroll") for (int i = 0; i < BQ; ++i) qb[i][e] = buf_f32(rx, vx, (e0.w + i * 32 * planeHW) * 4); \
      }                                                                                              \
    }                                                                                                \
    if (do_sums) {                                                                                   \
      _Pragma("unroll") for (int i = 0; i < AQ; ++i) qsum[i] += (qa[i].x + qa[i].y) + (qa[i].z + qa[i].w); \
    }                                                                                                \
    pix += kWgPix;                                                                                   \
    prr += kWgPix;                                                                                   \
    if (QTAP) {                                                                                      \
      qow += kWgPix;                                                                                 \
      while (qow >= g.OW) { qow -= g.OW; ++qoh; }                                                    \
    }                                                                                                \
    while (prr >= OHW) { prr -= OHW; ++pn; if (QTAP) qoh -= g.OH; }                                  \
  }
#define DASAC_WGQ_STORE()                                                                            \
  {                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < AQ; ++i)                                                   \
      *reinterpret_cast<f32x4*>(&sA[0][(prow4 + i * 32) * kWgPitch + 4 * pq]) = qa[i];               \
    _Pragma("unroll") for (int i = 0; i < BQ; ++i)                                                   \
      *reinterpret_cast<f32x4*>(&sB[0][(prow4 + i * 32) * kWgPitch + 4 * pq]) = qb[i];               \
  }
    if (steps > 0) {
      DASAC_WGQ_LOAD();
      DASAC_WGQ_STORE();
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      if (s + 1 < steps) DASAC_WGQ_LOAD();
      const float* a_base = &sA[0][(wm * WM + li) * kWgPitch + 4 * lh];
      const float* b_base = &sB[0][(wn * WN + li) * kWgPitch + 4 * lh];
#pragma unroll
      for (int gq = 0; gq < kWgPix / 8; ++gq) {
        f32x4 a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(a_base + i * 32 * kWgPitch + 8 * gq);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(b_base + j * 32 * kWgPitch + 8 * gq);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
      if (s + 1 < steps) {
        DASAC_WGQ_STORE();
        __syncthreads();
      }
    }
#undef DASAC_WGQ_LOAD
#undef DASAC_WGQ_STORE
    if (do_sums) {
      // the 8 lanes of a row hold its 32 pixels (4 each): butterfly over the three low lane bits
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        float v = qsum[i];
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (pq == 0) Psum[(size_t)split * g.Mpad + m0 + prow4 + i * 32] = v;
      }
    }
  } else {
  float ra[A_LOADS], rb[B_LOADS];
  float rsum[A_LOADS];                                   // per-row sums of dZ (only the k_tile 0 blocks)
#pragma unroll
  for (int i = 0; i < A_LOADS; ++i) rsum[i] = 0.f;
  const int zimg = g.M * OHW;                            // dZ image stride

  // pixel cursor of this thread (advanced by kWgPix per step)
  int pix = p_begin + pl;
  int pn = pix / OHW, prr = pix - pn * OHW;
  int poh = prr / g.OW, pow_ = prr - poh * g.OW;

#define DASAC_WG_LOAD()                                                                              \
  {                                                                                                  \
    const bool pv = pix < p_end;                                                                     \
    const int zbase = pn * zimg + poh * g.OW + pow_;                                                 \
    const int ih0 = poh * g.stride, iw0 = pow_ * g.stride;                                           \
    const int xbase = pn * g.CxHW + ih0 * g.W + iw0;                                                 \
    if (FAST) {                                                                                      \
      const unsigned vz = pv ? (unsigned)(zbase + prow * OHW) * 4u : kPoison;                        \
      /* rows past M (last, partial M tile) re-read the last valid 8-row group: their products land */ \
      /* in slab rows >= M that nobody reads -- no per-row branch or select in the loop            */ \
      _Pragma("unroll") for (int i = 0; i < A_LOADS; ++i)                                            \
        ra[i] = buf_f32(rz, vz, min(m0 + i * 8, g.M - 8) * OHW * 4);                                 \
      if (do_sums) {                                                                                 \
        _Pragma("unroll") for (int i = 0; i < A_LOADS; ++i) rsum[i] += ra[i];                        \
      }                                                                                              \
      const int ih = ih0 + e0.y, iw = iw0 + e0.z;                                                    \
      const bool ok = pv & ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);          \
      const unsigned vx = ok ? (unsigned)(xbase + (e0.x - e0.w) + prow * planeHW) * 4u : kPoison;    \
      _Pragma("unroll") for (int i = 0; i < B_LOADS; ++i) rb[i] = buf_f32(rx, vx, (e0.w + i * 8 * planeHW) * 4); \
    } else {                                                                                         \
      _Pragma("unroll") for (int i = 0; i < A_LOADS; ++i) {                                          \
        const int m = m0 + prow + i * 8;                                                             \
        ra[i] = buf_f32(rz, (pv & (m < g.M)) ? (unsigned)(zbase + m * OHW) * 4u : kPoison, 0);       \
        if (do_sums) rsum[i] += ra[i];                                                               \
      }                                                                                              \
      _Pragma("unroll") for (int i = 0; i < B_LOADS; ++i) {                                          \
        const int ih = ih0 + (te_d[i] >> 16), iw = iw0 + (int)(short)(te_d[i] & 0xffff);             \
        const bool ok = pv & ((unsigned)ih < (unsigned)g.H) & ((unsigned)iw < (unsigned)g.W);        \
        rb[i] = buf_f32(rx, ok ? (unsigned)(xbase + te_off[i]) * 4u : kPoison, 0);                   \
      }                                                                                              \
    }                                                                                                \
    /* advance the cursor by one step */                                                             \
    pix += kWgPix;                                                                                   \
    pow_ += kWgPix;                                                                                  \
    while (pow_ >= g.OW) { pow_ -= g.OW; ++poh; }                                                    \
    while (poh >= g.OH) { poh -= g.OH; ++pn; }                                                       \
  }
#define DASAC_WG_STORE(buf)                                                                          \
  if (X3) {                                                                                          \
    unsigned short* a16 = reinterpret_cast<unsigned short*>(&sA[buf][0]);                            \
    unsigned short* b16 = reinterpret_cast<unsigned short*>(&sB[buf][0]);                            \
    _Pragma("unroll") for (int i = 0; i < A_LOADS; ++i) {                                            \
      const unsigned h = pack_bf16(0.f, ra[i]);                                                      \
      const unsigned l = pack_bf16(0.f, ra[i] - __uint_as_float(h));                                 \
      const int e = (((pl >> 3) * PA + prow + i * 8) << 3) + (pl & 7);                               \
      a16[e] = (unsigned short)(h >> 16);                                                            \
      a16[32 * PA + e] = (unsigned short)(l >> 16);                                                  \
    }                                                                                                \
    _Pragma("unroll") for (int i = 0; i < B_LOADS; ++i) {                                            \
      const unsigned h = pack_bf16(0.f, rb[i]);                                                      \
      const unsigned l = pack_bf16(0.f, rb[i] - __uint_as_float(h));                                 \
      const int e = (((pl >> 3) * PB + prow + i * 8) << 3) + (pl & 7);                               \
      b16[e] = (unsigned short)(h >> 16);                                                            \
      b16[32 * PB + e] = (unsigned short)(l >> 16);                                                  \
    }                                                                                                \
  } else {                                                                                           \
    _Pragma("unroll") for (int i = 0; i < A_LOADS; ++i) sA[buf][(prow + i * 8) * kWgPitch + pl] = ra[i]; \
    _Pragma("unroll") for (int i = 0; i < B_LOADS; ++i) sB[buf][(prow + i * 8) * kWgPitch + pl] = rb[i]; \
  }

  if (steps > 0) {
    DASAC_WG_LOAD();
    DASAC_WG_STORE(0);
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) DASAC_WG_LOAD();
    if (X3) {
      const f32x4* a4 = reinterpret_cast<const f32x4*>(&sA[0][0]) + wm * WM + li;
      const f32x4* b4 = reinterpret_cast<const f32x4*>(&sB[0][0]) + wn * WN + li;
#pragma unroll
      for (int kb = 0; kb < kWgPix / 16; ++kb) {
        const int oct = 2 * kb + lh;                     // this lane half's 8 pixels of the 16-pixel MFMA block
        f32x4 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          ah[i] = a4[oct * PA + i * 32];
          al[i] = a4[(4 + oct) * PA + i * 32];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          bh[j] = b4[oct * PB + j * 32];
          bl[j] = b4[(4 + oct) * PB + j * 32];
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(al[i]), as_bf16x8(bh[j]), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(ah[i]), as_bf16x8(bl[j]), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(ah[i]), as_bf16x8(bh[j]), acc[i][j], 0, 0, 0);
          }
      }
    } else {
    // one ds_read_b128 per operand feeds FOUR MFMAs: lane half lh holds pixels 8g + 4*lh + {0..3} of its row and MFMA e
    // contracts the pixel pair {8g + e, 8g + 4 + e} (any pairing is valid as long as both operands agree)
    const float* a_base = &sA[0][(wm * WM + li) * kWgPitch + 4 * lh];
    const float* b_base = &sB[0][(wn * WN + li) * kWgPitch + 4 * lh];
#pragma unroll
    for (int gq = 0; gq < kWgPix / 8; ++gq) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(a_base + i * 32 * kWgPitch + 8 * gq);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(b_base + j * 32 * kWgPitch + 8 * gq);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    }
    __syncthreads();
    if (s + 1 < steps) {
      DASAC_WG_STORE(0);
      __syncthreads();
    }
  }
#undef DASAC_WG_LOAD
#undef DASAC_WG_STORE

  if (do_sums) {
    // the 32 lanes of a half-wave hold the 32 pixels of the same rows: butterfly inside the half
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
      float v = rsum[i];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (pl == 0) Psum[(size_t)split * g.Mpad + m0 + prow + i * 8] = v;
    }
  }
  }   // !QUAD
  // partial slab [split][Mpad][Kpad], k contiguous
  float* slab = P + (size_t)split * g.Mpad * g.Kpad;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int k = kb0 + wn * WN + j * 32 + li;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int m = m0 + wm * WM + i * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * lh;
        slab[(size_t)m * g.Kpad + k] = acc[i][j][rg];
      }
  }
}

// Batched weight gradient over plain matrices (the 16 point contractions of a Winograd weight gradient as ONE grid, blockIdx.y =
// batch entry):  P[split][b][m][c] = sum_{t in split} A[b][m][t] * B[b][c][t],  A [batch][M][T], B [batch][C][T] row-major, entries
// a_stride / b_stride ELEMENTS apart.  Per entry this is the QUAD case of conv_wgrad above -- the same 128 x 128 tile, LDS layout,
// four-pixels-per-lane loader, MFMA loop and XCD-contiguous block order -- with what plain matrices make unnecessary left out: no tap,
// no image boundary (host: M, C multiples of 128 and T, the split length and the strides multiples of 4, so a lane's quad lies
// wholly inside its row and its split or wholly outside, and an outside quad reads zeros through the poison offset).  A kernel of its
// own, so that conv_wgrad's instantiations compile to the code they had (for the same reason the MFMA step and the slab store stay
// written out in both: on shared helpers the quad loaders compiled to another stream, profiles/conv_split.md).  The pixel splits are chosen over batch x m_tiles x k_tiles
// tiles: one entry alone would be cut into many short splits (layer4: 16 tiles -> 48 splits of 13 K-steps; batched: 256 tiles x 3
// splits of 200).  Fixed summation order, no atomics.  Psum[split][m] = the split's row sums of entry `sum_entry` of A (k tile 0).
struct WgradBatch {
  int M, C, T;
  int m_tiles, k_tiles, n_splits, pix_per_split;
  int sum_entry;                   // entry whose row sums go to Psum (the Winograd point that is the tile's pixel sum)
  int64_t a_stride, b_stride;
};

__global__ __launch_bounds__(kThreads, 3) void conv_wgrad_batched(const float* __restrict__ A, const float* __restrict__ B,
                                                                float* __restrict__ P, float* __restrict__ Psum, WgradBatch w) {
  constexpr int BM = 128, BN = 128, WAVES_M = 2, WAVES_N = 2;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int AQ = BM / 32, BQ = BN / 32;
  __shared__ __attribute__((aligned(16))) float sA[BM * kWgPitch];
  __shared__ __attribute__((aligned(16))) float sB[BN * kWgPitch];

  const int n_blocks = w.m_tiles * w.k_tiles * w.n_splits;
  const int lb = wgrad_list_index(blockIdx.x, n_blocks);
  if (lb >= n_blocks) return;
  const WgradTile work = wgrad_tile(lb, w.m_tiles, w.k_tiles);
  const int entry = blockIdx.y;
  const int m_tile = work.m_tile, k_tile = work.k_tile, split = work.split;
  const int m0 = m_tile * BM, kb0 = k_tile * BN;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, lh = lane >> 5;
  const int pq = t & 7, prow4 = t >> 3;                    // loader: pixel quad of the step, row within a 32-row pass

  // one entry's window each: inside an entry every offset is below M*T (C*T) elements, host-checked to fit 31 bits of bytes
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(A + (size_t)entry * w.a_stride, (unsigned)(w.M * w.T) * 4u);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(B + (size_t)entry * w.b_stride, (unsigned)(w.C * w.T) * 4u);

  const PixelRange px = wgrad_pixels(split, w.pix_per_split, w.T);
  const int p_begin = px.begin, p_end = px.end;
  const int steps = (p_end - p_begin + kWgPix - 1) / kWgPix;
  const bool do_sums = (k_tile == 0) && (entry == w.sum_entry);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 qa[AQ], qb[BQ];
  float qsum[AQ];
#pragma unroll
  for (int i = 0; i < AQ; ++i) qsum[i] = 0.f;
  int pix = p_begin + 4 * pq;                              // first pixel of this thread's quad (advanced by kWgPix per step)
  // 16-byte loads: the poison is 2^31, not kPoison -- an entry's window is below 2^31 bytes (host), so all four dwords of a poisoned
  // quad lie past it without the offset wrapping
  constexpr unsigned kQuadPoison = 0x80000000u;
#define DASAC_WGB_LOAD()                                                                             \
  {                                                                                                  \
    const unsigned v = pix < p_end ? (unsigned)(prow4 * w.T + pix) * 4u : kQuadPoison;               \
    _Pragma("unroll") for (int i = 0; i < AQ; ++i) qa[i] = buf_f32x4(ra, v, (m0 + i * 32) * w.T * 4); \
    _Pragma("unroll") for (int i = 0; i < BQ; ++i) qb[i] = buf_f32x4(rb, v, (kb0 + i * 32) * w.T * 4); \
    if (do_sums) {                                                                                   \
      _Pragma("unroll") for (int i = 0; i < AQ; ++i) qsum[i] += (qa[i].x + qa[i].y) + (qa[i].z + qa[i].w); \
    }                                                                                                \
    pix += kWgPix;                                                                                   \
  }
#define DASAC_WGB_STORE()                                                                            \
  {                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < AQ; ++i)                                                   \
      *reinterpret_cast<f32x4*>(&sA[(prow4 + i * 32) * kWgPitch + 4 * pq]) = qa[i];                  \
    _Pragma("unroll") for (int i = 0; i < BQ; ++i)                                                   \
      *reinterpret_cast<f32x4*>(&sB[(prow4 + i * 32) * kWgPitch + 4 * pq]) = qb[i];                  \
  }
  if (steps > 0) {
    DASAC_WGB_LOAD();
    DASAC_WGB_STORE();
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) DASAC_WGB_LOAD();
    const float* a_base = &sA[(wm * WM + li) * kWgPitch + 4 * lh];
    const float* b_base = &sB[(wn * WN + li) * kWgPitch + 4 * lh];
#pragma unroll
    for (int gq = 0; gq < kWgPix / 8; ++gq) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(a_base + i * 32 * kWgPitch + 8 * gq);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(b_base + j * 32 * kWgPitch + 8 * gq);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    if (s + 1 < steps) {
      DASAC_WGB_STORE();
      __syncthreads();
    }
  }
#undef DASAC_WGB_LOAD
#undef DASAC_WGB_STORE
  if (do_sums) {
    // the 8 lanes of a row hold its 32 pixels (4 each): butterfly over the three low lane bits
#pragma unroll
    for (int i = 0; i < AQ; ++i) {
      float v = qsum[i];
#pragma unroll
      for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (pq == 0) Psum[(size_t)split * w.M + m0 + prow4 + i * 32] = v;
    }
  }
  // partial slab [split][entry][M][C], c contiguous
  float* slab = P + ((size_t)split * gridDim.y + entry) * w.M * w.C;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int k = kb0 + wn * WN + j * 32 + li;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int m = m0 + wm * WM + i * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * lh;
        slab[(size_t)m * w.C + k] = acc[i][j][rg];
      }
  }
}

// sum over the pixel splits of one slab element: four independent chains so that the loads of several slabs are in
// flight together (the slabs are 1-64 separate HBM streams)
__device__ __forceinline__ float sum_splits(const float* __restrict__ p, size_t slab, int splits) {
  float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
  int s = 0;
  for (; s + 4 <= splits; s += 4) {
    g0 += p[(size_t)s * slab];
    g1 += p[(size_t)(s + 1) * slab];
    g2 += p[(size_t)(s + 2) * slab];
    g3 += p[(size_t)(s + 3) * slab];
  }
  for (; s < splits; ++s) g0 += p[(size_t)s * slab];
  return (g0 + g1) + (g2 + g3);
}

// dW[co][ci][tap] = scale[co] * sum_s P[s][co][(tap0+tap)*Cin+ci];  dot[row][co] = this block's part of sum W*G (unscaled G);
// sum_dz[co] = sum_s Psum[s][co]
// grid (chunks of 64 input channels, output channels), 256 threads = 64 channels x 4 split lanes.  A thread adds the splits
// s = lane, lane + 4, ... of up to 9 taps of ITS channel (9 independent, coalesced slab loads in flight per step); the four
// lanes meet in LDS and the block writes its 64 x taps gradients in dW's own order -- one contiguous run per block, where the
// tap-major slab order would touch every 36-byte [ci] group of a 3x3 layer nine times from nine places.  The dot term
// leaves as one PARTIAL per block, dot[blockIdx.x][co] (dasac_conv_wgrad_dot_rows rows): bn_param_grads adds the rows in a fixed
// order, so the gamma gradient is bit-identical from run to run (rounds 1-3 combined them with float atomics).
constexpr int kWrTaps = 9;
__global__ __launch_bounds__(256) void wgrad_reduce_scalar(const float* __restrict__ P, const float* __restrict__ Psum, int splits,
                                                    int Mpad, int Kpad, const float* __restrict__ Wt,
                                                    const float* __restrict__ scale, float* __restrict__ dW,
                                                    float* __restrict__ dot, float* __restrict__ sum_dz, int Cin, int taps,
                                                    int tap0, int flat_cin) {
  // flat_cin > 0 (few input channels: the stem, VGG's first conv): the caller passes Cin = true Cin * taps and taps = 1, the
  // 64 channel lanes then run along the slab's whole k axis (a 3-channel layer would use 3 of them); dW's index is remapped.
  const int co = blockIdx.y;
  const int tx = threadIdx.x, c = tx & 63, q = tx >> 6;
  if (sum_dz && blockIdx.x == 0 && q == 0) {                 // one wave: the splits' channel sums in parallel
    float sv = 0.f;
    for (int s2 = c; s2 < splits; s2 += 64) sv += Psum[(size_t)s2 * Mpad + co];
    sv = wave_sum(sv);
    if (c == 0) sum_dz[co] = sv;
  }
  __shared__ float red[4][kWrTaps][64];
  const int ci0 = blockIdx.x * 64, ci = ci0 + c;
  const float sc = scale ? scale[co] : 1.f;
  const size_t slab = (size_t)Mpad * Kpad;
  float part = 0.f;
  for (int tb = 0; tb < taps; tb += kWrTaps) {
    const int nt = min(kWrTaps, taps - tb);
    float acc[kWrTaps];
#pragma unroll
    for (int u = 0; u < kWrTaps; ++u) acc[u] = 0.f;
    if (ci < Cin) {
      const float* p0 = P + (size_t)co * Kpad + (size_t)(tap0 + tb) * Cin + ci;
#pragma unroll 4
      for (int s2 = q; s2 < splits; s2 += 4) {         // unrolled: the loads of four splits are issued before the first add
        const float* ps = p0 + (size_t)s2 * slab;
#pragma unroll
        for (int u = 0; u < kWrTaps; ++u)
          if (u < nt) acc[u] += ps[(size_t)u * Cin];
      }
    }
#pragma unroll
    for (int u = 0; u < kWrTaps; ++u) red[q][u][c] = acc[u];
    __syncthreads();
    for (int e = tx; e < 64 * nt; e += 256) {                // (channel, tap) pairs in dW order
      const int c2 = e / nt, u2 = e - c2 * nt;
      if (ci0 + c2 < Cin) {
        const float gsum = (red[0][u2][c2] + red[1][u2][c2]) + (red[2][u2][c2] + red[3][u2][c2]);
        size_t widx = ((size_t)co * Cin + ci0 + c2) * taps + tb + u2;
        if (flat_cin > 0) {                                    // k = tap * Cin_true + ci  ->  [co][ci][tap]
          const int k = ci0 + c2, tap = k / flat_cin, ci_t = k - tap * flat_cin;
          widx = ((size_t)co * flat_cin + ci_t) * (Cin / flat_cin) + tap;
        }
        if (dot) part += gsum * Wt[widx];
        dW[widx] = gsum * sc;
      }
    }
    __syncthreads();
  }
  if (dot) {
    __shared__ float redd[4];
    part = wave_sum(part);
    if (c == 0) redd[q] = part;
    __syncthreads();
    if (tx == 0) dot[(size_t)blockIdx.x * gridDim.y + co] = (redd[0] + redd[1]) + (redd[2] + redd[3]);   // partial row: no atomics
  }
}

// The same reduction for layers whose channel count is a multiple of 64 (every layer that matters): a thread owns FOUR consecutive
// input channels (one 16-byte slab load per tap and split) and the 256 threads are 16 channel quads x 16 split lanes -- four times
// the bytes in flight per thread of the scalar kernel above (which moved its slabs at 1.5 TB/s).  The four split lanes of a wave
// meet in a butterfly, the four waves in LDS; output and dot term exactly as above.
__global__ __launch_bounds__(256) void wgrad_reduce(const float* __restrict__ P, const float* __restrict__ Psum, int splits,
                                                    int Mpad, int Kpad, const float* __restrict__ Wt,
                                                    const float* __restrict__ scale, float* __restrict__ dW,
                                                    float* __restrict__ dot, float* __restrict__ sum_dz, int Cin, int taps,
                                                    int tap0) {
  const int co = blockIdx.y;
  const int tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  const int c4 = lane & 15, q = wave * 4 + (lane >> 4);      // channel quad, split lane 0..15
  if (sum_dz && blockIdx.x == 0 && wave == 0) {              // one wave: the splits' channel sums in parallel
    float sv = 0.f;
    for (int s2 = lane; s2 < splits; s2 += 64) sv += Psum[(size_t)s2 * Mpad + co];
    sv = wave_sum(sv);
    if (lane == 0) sum_dz[co] = sv;
  }
  __shared__ float red[4][kWrTaps][64];
  const int ci0 = blockIdx.x * 64;
  const float sc = scale ? scale[co] : 1.f;
  const size_t slab = (size_t)Mpad * Kpad;
  float part = 0.f;
  for (int tb = 0; tb < taps; tb += kWrTaps) {
    const int nt = min(kWrTaps, taps - tb);
    f32x4 acc[kWrTaps];
#pragma unroll
    for (int u = 0; u < kWrTaps; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* p0 = P + (size_t)co * Kpad + (size_t)(tap0 + tb) * Cin + ci0 + 4 * c4;      // 16-byte aligned: Kpad, Cin, ci0 % 64 == 0
#pragma unroll 2
    for (int s2 = q; s2 < splits; s2 += 16) {
      const float* ps = p0 + (size_t)s2 * slab;
#pragma unroll
      for (int u = 0; u < kWrTaps; ++u)
        if (u < nt) acc[u] += *reinterpret_cast<const f32x4*>(ps + (size_t)u * Cin);
    }
#pragma unroll
    for (int u = 0; u < kWrTaps; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[u][e];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        acc[u][e] = v;
      }
      if (lane < 16) *reinterpret_cast<f32x4*>(&red[wave][u][4 * c4]) = acc[u];
    }
    __syncthreads();
    for (int e = tx; e < 64 * nt; e += 256) {                // (channel, tap) pairs in dW order
      const int c2 = e / nt, u2 = e - c2 * nt;
      const float gsum = (red[0][u2][c2] + red[1][u2][c2]) + (red[2][u2][c2] + red[3][u2][c2]);
      const size_t widx = ((size_t)co * Cin + ci0 + c2) * taps + tb + u2;
      if (dot) part += gsum * Wt[widx];
      dW[widx] = gsum * sc;
    }
    __syncthreads();
  }
  if (dot) {
    __shared__ float redd[4];
    part = wave_sum(part);
    if (lane == 0) redd[wave] = part;
    __syncthreads();
    if (tx == 0) dot[(size_t)blockIdx.x * gridDim.y + co] = (redd[0] + redd[1]) + (redd[2] + redd[3]);   // partial row: no atomics
  }
}

// The same reduction for ONE-tap layers (every 1x1 convolution: half of the step's weight-gradient launches).  With taps == 1 the slab
// order IS dW's order, so no transposition through LDS is needed, and the 16 x 16 arrangement above leaves a thread three 16-byte loads
// at 48 splits (measured stand-alone: 25 us for 50 MB = 2.0 TB/s, the 2048 x 512 layer 68 us = 0.74 TB/s over 16 384 blocks).  Here a block
// owns one output channel and 256 input channels -- 64 channel quads x 4 split lanes, a wave per split lane --, a thread streams
// splits / 4 slabs with four loads in flight; the four waves meet in LDS and wave w then holds 64-channel chunk w of the block: its dot
// partial comes out of the same wave butterfly as the general kernel's, row (4 * blockIdx.x + w).
__global__ __launch_bounds__(256) void wgrad_reduce_1x1(const float* __restrict__ P, const float* __restrict__ Psum, int splits, int Mpad,
                                                        int Kpad, const float* __restrict__ Wt, const float* __restrict__ scale,
                                                        float* __restrict__ dW, float* __restrict__ dot, float* __restrict__ sum_dz,
                                                        int Cin) {
  const int co = blockIdx.y;
  const int tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  if (sum_dz && blockIdx.x == 0 && wave == 0) {              // one wave: the splits' channel sums in parallel
    float sv = 0.f;
    for (int s2 = lane; s2 < splits; s2 += 64) sv += Psum[(size_t)s2 * Mpad + co];
    sv = wave_sum(sv);
    if (lane == 0) sum_dz[co] = sv;
  }
  __shared__ __attribute__((aligned(16))) float red[4][256];
  const int ci0 = blockIdx.x * 256, cq = ci0 + 4 * lane;     // this thread's channel quad
  const size_t slab = (size_t)Mpad * Kpad;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < Cin) {
    const float* p0 = P + (size_t)co * Kpad + cq;
#pragma unroll 4
    for (int s2 = wave; s2 < splits; s2 += 4) acc += *reinterpret_cast<const f32x4*>(p0 + (size_t)s2 * slab);
  }
  *reinterpret_cast<f32x4*>(&red[wave][4 * lane]) = acc;
  __syncthreads();
  const int ci = ci0 + tx;                                   // one channel per thread now; wave w = 64-channel chunk w of the block
  float part = 0.f;
  if (ci < Cin) {
    const float gsum = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    const size_t widx = (size_t)co * Cin + ci;
    if (dot) part = gsum * Wt[widx];
    dW[widx] = gsum * (scale ? scale[co] : 1.f);
  }
  if (dot && ci0 + 64 * wave < Cin) {
    part = wave_sum(part);
    if (lane == 0) dot[(size_t)(4 * blockIdx.x + wave) * gridDim.y + co] = part;
  }
}

// dW[co][ci][tap] = sum_s P[s][(tap0+tap)*Cp + co][ci]
__global__ __launch_bounds__(256) void wgrad_reduce_expanded(const float* __restrict__ P, int splits, int Mpad, int Kpad,
                                                             float* __restrict__ dW, int Cout, int Cin, int taps, int tap0,
                                                             int Cp) {
  const int64_t total = (int64_t)Cout * taps * Cin;
  const size_t slab = (size_t)Mpad * Kpad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ci = (int)(i % Cin);                       // slab reads coalesce along ci
    const int64_t r = i / Cin;
    const int tap = (int)(r % taps), co = (int)(r / taps);
    const size_t idx = (size_t)((tap0 + tap) * Cp + co) * Kpad + ci;
    dW[((size_t)co * Cin + ci) * taps + tap] = sum_splits(P + idx, slab, splits);
  }
}

template <int BM, int BN, int WAVES_M, bool FAST>
static void launch_wgrad(bool x3, const float* dZ, const float* X, const int4* tab, float* P, float* Psum, const GemmGeom& g,
                         const WgradPlan& p, hipStream_t s) {
  if (x3)
    hipLaunchKernelGGL((conv_wgrad<BM, BN, WAVES_M, FAST, true>), dim3(p.grid), dim3(kThreads), 0, s, dZ, X, tab, P,
                       Psum, g, p.m_tiles, p.k_tiles, p.splits, p.per);
  else
    hipLaunchKernelGGL((conv_wgrad<BM, BN, WAVES_M, FAST, false>), dim3(p.grid), dim3(kThreads), 0, s, dZ, X, tab, P,
                       Psum, g, p.m_tiles, p.k_tiles, p.splits, p.per);
}

}  // namespace dasac

using namespace dasac;

// (the size does not depend on the gathered channel count: the bound over both k-tile widths)
extern "C" size_t dasac_conv_wgrad_workspace(int Nb, int OH, int OW, int M, int K) { return wgrad_plan(M, K, 0, Nb * OH * OW).workspace_bytes; }

// dz [Nb,M,OH,OW], x [Nb,Cx,H,W] -> slabs in workspace -> dW (one or several weight tensors of a fused conv)
static int conv_wgrad_impl(bool x3, const float* dz, const float* x, const int32_t* table, int Nb, int Cx, int H, int W, int OH,
                           int OW, int stride, int M, int K, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(dz && x && table && workspace, "conv_wgrad: null pointer");
  DASAC_REQUIRE(((uintptr_t)table & 15) == 0, "conv_wgrad: misaligned table (16-byte rows)");
  GemmGeom g;
  int rc = fill_geom(g, Nb, Cx, H, W, OH, OW, stride, M, conv_mpad(M), conv_kpad(K), OH, OW, 1);
  if (rc) return rc;
  const WgradPlan p = wgrad_plan(M, K, Cx, g.Npix);
  const int bm = p.bm;
  // the size function itself (the larger of both k-tile widths' split counts, so never less than this launch writes): what it
  // states is what is asked for, whatever Cx turns out to be
  if (ws_bytes < p.workspace_bytes) return fail(DASAC_EWORKSPACE, "conv_wgrad: workspace too small");
  const int4* tab = reinterpret_cast<const int4*>(table);
  float* P = reinterpret_cast<float*>(workspace);
  float* Psum = P + p.psum_offset;
  hipStream_t s = as_stream(stream);
  const bool fast = (Cx % 128 == 0) && (M % 8 == 0);   // a 128-row k tile sits inside one tap
  if (p.bnk == 64) {                                   // Cx = 64, 192, ...: 64-row k tiles, still one tap each
    if (bm == 128) launch_wgrad<128, 64, 2, true>(x3, dz, x, tab, P, Psum, g, p, s);
    else launch_wgrad<64, 64, 2, true>(x3, dz, x, tab, P, Psum, g, p, s);
    DASAC_CHECK_LAUNCH("conv_wgrad");
    return DASAC_OK;
  }
  switch (bm) {
    case 128: {
      // 1x1 stride-1 layers: both operands are plain [row][pixel] matrices -> four pixels per lane (conv_wgrad<..., QUAD>)
      const bool same = fast && !x3 && stride == 1 && H == OH && W == OW && M % 128 == 0;
      const bool quad = same && K == Cx;                                                   // one tap, no padding
      // "same"-padded k x k layers (every 3x3 of the bottlenecks): the quad loader with per-pixel tap validity (QTAP)
      const bool qtap = same && K > Cx && K % Cx == 0 && W >= 4;
      if (quad || qtap) {
        if (quad)
          hipLaunchKernelGGL((conv_wgrad<128, 128, 2, true, false, true, false>), dim3(p.grid), dim3(kThreads), 0, s, dz, x, tab, P, Psum, g,
                             p.m_tiles, p.k_tiles, p.splits, p.per);
        else
          hipLaunchKernelGGL((conv_wgrad<128, 128, 2, true, false, true, true>), dim3(p.grid), dim3(kThreads), 0, s, dz, x, tab, P, Psum, g,
                             p.m_tiles, p.k_tiles, p.splits, p.per);
      } else if (fast) launch_wgrad<128, 128, 2, true>(x3, dz, x, tab, P, Psum, g, p, s);
      else launch_wgrad<128, 128, 2, false>(x3, dz, x, tab, P, Psum, g, p, s);
      break;
    }
    case 64:
      if (fast) launch_wgrad<64, 128, 2, true>(x3, dz, x, tab, P, Psum, g, p, s);
      else launch_wgrad<64, 128, 2, false>(x3, dz, x, tab, P, Psum, g, p, s);
      break;
    default: launch_wgrad<32, 128, 1, false>(x3, dz, x, tab, P, Psum, g, p, s); break;
  }
  DASAC_CHECK_LAUNCH("conv_wgrad");
  return DASAC_OK;
}

extern "C" int dasac_conv_wgrad(const float* dz, const float* x, const int32_t* table, int Nb, int Cx, int H, int W, int OH,
                                int OW, int stride, int M, int K, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  return conv_wgrad_impl(false, dz, x, table, Nb, Cx, H, W, OH, OW, stride, M, K, workspace, ws_bytes, stream);
}

extern "C" int dasac_conv_wgrad_x3(const float* dz, const float* x, const int32_t* table, int Nb, int Cx, int H, int W, int OH,
                                   int OW, int stride, int M, int K, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  return conv_wgrad_impl(true, dz, x, table, Nb, Cx, H, W, OH, OW, stride, M, K, workspace, ws_bytes, stream);
}

extern "C" int dasac_conv_wgrad_dot_rows(int Cin, int taps) { return Cin < 32 ? (Cin * taps + 63) / 64 : (Cin + 63) / 64; }

extern "C" int dasac_conv_wgrad_finish(const void* workspace, int Nb, int OH, int OW, int M, int K, const float* w,
                                       const float* scale, float* dw, float* dot, float* sum_dz, int Cin, int taps,
                                       int tap0, dasac_stream_t stream) {
  DASAC_REQUIRE(workspace && w && dw, "conv_wgrad_finish: null pointer");
  DASAC_REQUIRE(!dot || (tap0 == 0 && Cin * taps == K), "conv_wgrad_finish: the dot term is defined for single-branch convolutions");
  const WgradPlan p = wgrad_plan(M, K, Cin, Nb * OH * OW);
  const int Mpad = p.Mpad, Kpad = p.Kpad, splits = p.splits;
  const float* P = reinterpret_cast<const float*>(workspace);
  const float* Psum = P + p.psum_offset;
  if (Cin < 32)      // lanes along the whole k axis (see the kernel); tap0 * Cin is this branch's first k
    hipLaunchKernelGGL(wgrad_reduce_scalar, dim3((Cin * taps + 63) / 64, M), dim3(256), 0, as_stream(stream), P + (size_t)tap0 * Cin, Psum,
                       splits, Mpad, Kpad, w, scale, dw, dot, sum_dz, Cin * taps, 1, 0, Cin);
  else if (Cin % 64 != 0)
    hipLaunchKernelGGL(wgrad_reduce_scalar, dim3((Cin + 63) / 64, M), dim3(256), 0, as_stream(stream), P, Psum, splits, Mpad, Kpad, w,
                       scale, dw, dot, sum_dz, Cin, taps, tap0, 0);
  else if (taps == 1 && tap0 == 0 && K == Cin)
    hipLaunchKernelGGL(wgrad_reduce_1x1, dim3((Cin + 255) / 256, M), dim3(256), 0, as_stream(stream), P, Psum, splits, Mpad, Kpad, w, scale,
                       dw, dot, sum_dz, Cin);
  else
    hipLaunchKernelGGL(wgrad_reduce, dim3(Cin / 64, M), dim3(256), 0, as_stream(stream), P, Psum, splits, Mpad, Kpad, w, scale, dw, dot,
                       sum_dz, Cin, taps, tap0);
  DASAC_CHECK_LAUNCH("wgrad_reduce");
  return DASAC_OK;
}

// `batch` weight gradients over plain matrices as ONE launch (conv_wgrad_batched above; include/dasac_hip.h).  The pixel splits
// are chosen over all batch * m_tiles * k_tiles tiles; 0 = the launch does not take this shape.
extern "C" int dasac_conv_wgrad_batched_splits(int batch, int M, int C, int T) { return wgrad_batched_plan(batch, M, C, T).splits; }
extern "C" size_t dasac_conv_wgrad_batched_workspace(int batch, int M, int C, int T) { return wgrad_batched_plan(batch, M, C, T).workspace_bytes; }

extern "C" int dasac_conv_wgrad_batched(const float* a, const float* b, int batch, int M, int C, int T, int64_t a_stride,
                                        int64_t b_stride, int sum_entry, void* workspace, size_t ws_bytes, dasac_stream_t stream) {
  DASAC_REQUIRE(a && b && workspace, "conv_wgrad_batched: null pointer");
  DASAC_REQUIRE(sum_entry >= 0 && sum_entry < batch, "conv_wgrad_batched: sum_entry %d outside 0..batch-1", sum_entry);
  const WgradBatchedPlan p = wgrad_batched_plan(batch, M, C, T);
  DASAC_REQUIRE(p.splits > 0, "conv_wgrad_batched: needs batch in 1..65535, M and C multiples of 128, T a multiple of 4, entries below 2 GiB "
                            "and slabs inside the 4 GiB window (batch %d, M %d, C %d, T %d)", batch, M, C, T);
  DASAC_REQUIRE(a_stride >= (int64_t)M * T && b_stride >= (int64_t)C * T && a_stride % 4 == 0 && b_stride % 4 == 0,
                "conv_wgrad_batched: a per-batch stride is smaller than one entry or not a multiple of 4 elements");
  if (ws_bytes < p.workspace_bytes) return fail(DASAC_EWORKSPACE, "conv_wgrad_batched: workspace too small");
  float* P = reinterpret_cast<float*>(workspace);
  float* Psum = P + p.psum_offset;
  const WgradBatch w{M, C, T, p.m_tiles, p.k_tiles, p.splits, p.per, sum_entry, a_stride, b_stride};
  hipLaunchKernelGGL(conv_wgrad_batched, dim3(p.grid, batch), dim3(kThreads), 0, as_stream(stream), a, b, P, Psum, w);
  DASAC_CHECK_LAUNCH("conv_wgrad_batched");
  return DASAC_OK;
}

extern "C" int dasac_conv_wgrad_finish_expanded(const void* workspace, int Nb, int OH, int OW, int E, int Cin, float* dw,
                                                int Cout, int taps, int tap0, int Cp, dasac_stream_t stream) {
  DASAC_REQUIRE(workspace && dw, "conv_wgrad_finish_expanded: null pointer");
  const WgradPlan p = wgrad_plan(E, Cin, Cin, Nb * OH * OW);
  hipLaunchKernelGGL(wgrad_reduce_expanded, dim3(stream_grid((int64_t)Cout * taps * Cin, 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float*>(workspace), p.splits, p.Mpad, p.Kpad, dw, Cout, Cin, taps, tap0, Cp);
  DASAC_CHECK_LAUNCH("wgrad_reduce_expanded");
  return DASAC_OK;
}
