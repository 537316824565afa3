// Operands of the implicit-GEMM convolution (conv_gemm.hip, conv_wgrad.hip): the gather table that turns a kernel size / dilation /
// padding / multi-branch layout into im2col rows, and the weight packers (k-interleaved fp32, all layers in one launch, split-bf16).
// Replaces the weight layouts nn.Conv2d keeps implicitly (models/deeplabv2.py:59,65-66,70,107; models/fcn.py:49,53,57,78,88).
#include "conv_common.hpp"

namespace dasac {

struct TapGroups {
  int n;             // number of branches (1, or 4 for the fused ASPP)
  int kh[4], kw[4], dil[4], pad[4];
};

// table row k -> (tap, c); tap enumerates (branch, kh, kw).
//   order 0 (tap-major):    k = tap*C + c                         -- weight-gradient tiles want one tap per 128 rows
//   order 1 (chunk-major):  k = ((c/16)*taps + tap)*16 + c%16     -- forward / data gradient: consecutive K-steps
//       walk the taps of the SAME 16 channel planes, so the shifted re-reads of a dilated 3x3 hit L2
//       instead of streaming the whole channel range between two taps (needs C % 16 == 0)
__device__ __forceinline__ void decode_k(int k, int C, int taps, int order, int& tap, int& c) {
  if (order == 0) {
    tap = k / C;
    c = k - tap * C;
  } else {
    const int blk = k >> 4, chunk = blk / taps;
    tap = blk - chunk * taps;
    c = chunk * 16 + (k & 15);
  }
}
__device__ __forceinline__ int encode_k(int tap, int c, int C, int taps, int order) {
  return order == 0 ? tap * C + c : (((c >> 4) * taps + tap) << 4) + (c & 15);
}

__global__ void build_table(int4* tab, TapGroups tg, int C, int K, int Kpad, int planeHW, int W, int sign, int taps,
                            int order) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Kpad) return;
  int4 e = make_int4(0, kInvalid, kInvalid, 0);
  if (k < K) {
    int tap, c;
    decode_k(k, C, taps, order, tap, c);
    int b = 0;
    while (b < tg.n - 1 && tap >= tg.kh[b] * tg.kw[b]) {
      tap -= tg.kh[b] * tg.kw[b];
      ++b;
    }
    const int kh = tap / tg.kw[b], kw = tap - kh * tg.kw[b];
    const int dh = sign * (kh * tg.dil[b] - tg.pad[b]), dw = sign * (kw * tg.dil[b] - tg.pad[b]);
    e = make_int4(c * planeHW + dh * W + dw, dh, dw, c * planeHW);
  }
  tab[k] = e;
}

// mode 0 (forward):  Wp[(tap0+tap)*Cin + ci][co] = W[co][ci][tap] * (scale ? scale[co] : 1)
// mode 1 (dgrad):    Wp[(tap0+tap)*Cout + co][ci] = W[co][ci][tap] * (scale ? scale[co] : 1)
__global__ void pack_weights(const float* __restrict__ Wt, const float* __restrict__ scale, float* __restrict__ Wp,
                             int Cout, int Cin, int taps, int tap0, int total_taps, int Mpad, int mode, int order) {
  const int C = mode == 0 ? Cin : Cout;
  const int rows = taps * C;
  const int64_t total = (int64_t)rows * Mpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / Mpad), m = (int)(i - (int64_t)row * Mpad);
    const int tap = row / C, c = row - tap * C;
    float v = 0.f;
    if (mode == 0) {
      if (m < Cout) {
        v = Wt[((int64_t)m * Cin + c) * taps + tap];
        if (scale) v = v * scale[m];
      }
    } else {
      if (m < Cin) {
        v = Wt[((int64_t)c * Cin + m) * taps + tap];
        if (scale) v = v * scale[c];
      }
    }
    const int64_t k = encode_k(tap0 + tap, c, C, total_taps, order);
    Wp[((k >> 2) * Mpad + m) * 4 + (k & 3)] = v;   // k-interleaved: [(k/4)][m][k%4]
  }
}

// All (single-branch) convolutions of a network in ONE launch: job j describes one packed operand (forward or data-gradient
// layout of one layer), chunk (j, c) covers kPackChunk consecutive floats of its output -- the K padding rows and the M padding
// columns are written as zeros here, so no memset per layer either.  Replaces ~2 x 104 pack_weights launches per optimiser step.
constexpr int kPackChunk = 256 * 32;
__global__ __launch_bounds__(256) void pack_weights_multi(const dasac_pack_job* __restrict__ jobs, const int2* __restrict__ chunks) {
  const int2 ch = chunks[blockIdx.x];
  const dasac_pack_job jb = jobs[ch.x];
  const int C = jb.mode == 0 ? jb.Cin : jb.Cout;
  const int K = jb.taps * C;
  const int64_t total = (int64_t)jb.Kpad * jb.Mpad;
  const int64_t base = (int64_t)ch.y * kPackChunk;
  const int row4 = jb.Mpad * 4;
#pragma unroll 4
  for (int u = 0; u < kPackChunk / 256; ++u) {
    const int64_t j = base + u * 256 + threadIdx.x;             // == offset in the packed operand [(k/4)][Mpad][4]
    if (j >= total) break;
    const int kq = (int)(j / row4), rem = (int)(j - (int64_t)kq * row4);
    const int m = rem >> 2, k = kq * 4 + (rem & 3);
    float v = 0.f;
    if (k < K) {
      int tap, c;
      decode_k(k, C, jb.taps, jb.order, tap, c);
      if (jb.mode == 0) {
        if (m < jb.Cout) {
          v = jb.w[((int64_t)m * jb.Cin + c) * jb.taps + tap];
          if (jb.scale) v = v * jb.scale[m];
        }
      } else if (m < jb.Cin) {
        v = jb.w[((int64_t)c * jb.Cin + m) * jb.taps + tap];
        if (jb.scale) v = v * jb.scale[c];
      }
    }
    jb.out[j] = v;
  }
}

// fp32 packed weights [(k/4)][Mpad][4] -> split-bf16 operands: K-step t (16 k) holds four slots of Mpad
// 16-byte words, slot 2*o + h = octet o (k = 16t + 8o .. +7), h = 0 heads / 1 tails -- the same addressing
// as the fp32 tile (slot == quad), so conv_gemm's weight path is shared.
// Both operands are read and written through element-aligned vectors: a packed operand may sit at any 4-byte phase.
__global__ void pack_x3(const f32x4u* Wp, f32x4u* Wx, int Mpad, int Kpad) {   // Wx may alias Wp (in-place conversion)
  const int64_t total = (int64_t)(Kpad / 8) * Mpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t oct = i / Mpad;                  // global octet index = 2*t + o
    const int m = (int)(i - oct * Mpad);
    f32x4 heads, tails;
    split_bf16(Wp[(2 * oct) * Mpad + m], Wp[(2 * oct + 1) * Mpad + m], heads, tails);
    Wx[(2 * oct) * Mpad + m] = heads;
    Wx[(2 * oct + 1) * Mpad + m] = tails;
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_conv_mpad(int M) { return conv_mpad(M); }
extern "C" int dasac_conv_kpad(int K) { return conv_kpad(K); }

extern "C" int dasac_conv_table(const int32_t* kh, const int32_t* kw, const int32_t* dil, const int32_t* pad,
                                int n_branches, int C, int plane_h, int plane_w, int transposed, int order, int32_t* table,
                                dasac_stream_t stream) {
  DASAC_REQUIRE(kh && kw && dil && pad && table, "conv_table: null pointer");
  DASAC_REQUIRE(n_branches >= 1 && n_branches <= 4 && C > 0, "conv_table: bad branches/C");
  DASAC_REQUIRE(((uintptr_t)table & 15) == 0, "conv_table: misaligned table (16-byte rows)");
  TapGroups tg;
  tg.n = n_branches;
  int taps = 0;
  for (int b = 0; b < n_branches; ++b) {
    tg.kh[b] = kh[b]; tg.kw[b] = kw[b]; tg.dil[b] = dil[b]; tg.pad[b] = pad[b];
    taps += kh[b] * kw[b];
  }
  for (int b = n_branches; b < 4; ++b) tg.kh[b] = tg.kw[b] = tg.dil[b] = tg.pad[b] = 1;
  const int K = taps * C, Kpad = dasac_conv_kpad(K);
  DASAC_REQUIRE(order == 0 || (order == 1 && C % 16 == 0), "conv_table: chunk-major order needs C %% 16 == 0");
  hipLaunchKernelGGL(build_table, dim3((Kpad + 255) / 256), dim3(256), 0, as_stream(stream), reinterpret_cast<int4*>(table),
                     tg, C, K, Kpad, plane_h * plane_w, plane_w, transposed ? -1 : 1, taps, order);
  DASAC_CHECK_LAUNCH("build_table");
  return DASAC_OK;
}

extern "C" int dasac_conv_pack(const float* w, const float* scale, int Cout, int Cin, int taps, int tap0, int total_taps,
                               int transposed, int order, float* packed, dasac_stream_t stream) {
  DASAC_REQUIRE(w && packed, "conv_pack: null pointer");
  const int M = transposed ? Cin : Cout, C = transposed ? Cout : Cin;
  const int Mpad = dasac_conv_mpad(M), K = total_taps * C, Kpad = dasac_conv_kpad(K);
  hipStream_t s = as_stream(stream);
  if (tap0 == 0 && Kpad > K) DASAC_HIP(hipMemsetAsync(packed, 0, (size_t)Kpad * Mpad * sizeof(float), s));   // zero K padding
  const int64_t total = (int64_t)taps * C * Mpad;
  DASAC_REQUIRE(order == 0 || (order == 1 && C % 16 == 0), "conv_pack: chunk-major order needs C %% 16 == 0");
  hipLaunchKernelGGL(pack_weights, dim3(stream_grid(total, 256)), dim3(256), 0, s, w, scale, packed, Cout, Cin, taps, tap0,
                     total_taps, Mpad, transposed ? 1 : 0, order);
  DASAC_CHECK_LAUNCH("pack_weights");
  return DASAC_OK;
}

extern "C" int dasac_pack_chunk_elems(void) { return kPackChunk; }

extern "C" int dasac_conv_pack_multi(const dasac_pack_job* jobs, const int32_t* chunks, int n_chunks, dasac_stream_t stream) {
  DASAC_REQUIRE(jobs && chunks && n_chunks > 0, "conv_pack_multi: bad arguments");
  DASAC_REQUIRE((((uintptr_t)jobs | (uintptr_t)chunks) & 7) == 0, "conv_pack_multi: misaligned job table / chunk list");
  hipLaunchKernelGGL(pack_weights_multi, dim3(n_chunks), dim3(256), 0, as_stream(stream), jobs, reinterpret_cast<const int2*>(chunks));
  DASAC_CHECK_LAUNCH("pack_weights_multi");
  return DASAC_OK;
}

extern "C" int dasac_conv_pack_x3(const float* packed, int M, int K, void* packed_x3, dasac_stream_t stream) {
  DASAC_REQUIRE(packed && packed_x3, "conv_pack_x3: null pointer");
  const int Mpad = dasac_conv_mpad(M), Kpad = dasac_conv_kpad(K);
  hipLaunchKernelGGL(pack_x3, dim3(stream_grid((int64_t)(Kpad / 8) * Mpad, 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const f32x4u*>(packed), reinterpret_cast<f32x4u*>(packed_x3), Mpad, Kpad);
  DASAC_CHECK_LAUNCH("pack_x3");
  return DASAC_OK;
}
