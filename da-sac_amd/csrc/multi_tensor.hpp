// The (tensor, chunk) walk of the multi-tensor kernels (momentum teacher, fused optimisers, gradient norm, gradient health table):
// one block per chunk of kChunk elements of one tensor, `chunks` an int32 (tensor id, chunk index) list sorted by tensor id.
#pragma once
#include <cstddef>

#include "common.hpp"

namespace dasac {

constexpr int kChunk = 256 * 16;      // dasac_ema_chunk_elems()

typedef float f32x4 __attribute__((ext_vector_type(4)));      // 16-byte aligned: one global_load/store_dwordx4

struct Chunk {
  int tensor, index;
  __device__ int64_t base() const { return (int64_t)index * kChunk; }      // its first element inside the tensor
};
__device__ __forceinline__ Chunk this_chunk(const int2* chunks) {      // the block's own
  const int2 ch = chunks[blockIdx.x];
  return Chunk{ch.x, ch.y};
}

// the first chunk whose tensor id is >= t: where tensor t's contiguous run of chunks (and of chunk partials) starts
__device__ __forceinline__ int first_chunk_of(const int2* chunks, int n_chunks, int t) {
  int lo = 0, hi = n_chunks;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunks[mid].x < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// elements i .. i+3 of a tensor of n: one dwordx4 load where `vec` (whole chunk, 16-byte aligned pointer), four guarded scalar
// loads otherwise (0 beyond the end)
__device__ __forceinline__ f32x4 chunk_load4(const float* x, int64_t i, int64_t n, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = i + e < n ? x[i + e] : 0.f;
  return v;
}

// the gradient a step applies to elements i .. i+3: g, or g2 + g in AccumulateGrad's operand order (g2: the gradient the driver
// set aside while a second backward pass ran).  tensor_stats_chunks takes it from here; adam_chunks and grad_sq_chunks write the
// same sum out, because on this helper they compiled to slower code (profiles/pointwise_split.md).
__device__ __forceinline__ f32x4 summed_grad4(const float* g, const float* g2, int64_t i, int64_t n, bool vec) {
  f32x4 d = chunk_load4(g, i, n, vec);
  if (g2) {
    const f32x4 d2 = chunk_load4(g2, i, n, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = d2[e] + d[e];
  }
  return d;
}

// ---- rows of the optimiser tables (dasac_hip/optim.py builds them as int64 rows) ----------------------------------------------
struct SgdTensor {
  float* p;
  const float *g, *g2;
  float* buf;
  int64_t n, group;
};
struct AdamTensor {
  float* p;
  const float *g, *g2;
  float *m, *v;
  int64_t n;
  int32_t group, reserved;
  float step_size, bc2_sqrt;
};
static_assert(sizeof(SgdTensor) == 48 && sizeof(AdamTensor) == 64, "6 and 8 x 8 bytes");

// What the kernels that serve BOTH tables read of a row: the two layouts agree on everything but where n lies.
struct GradRow {
  const float *p, *g, *g2, *state;      // state: momentum_buffer / exp_avg
  int64_t n, group;                     // group: the 8 bytes after n (SGD: bit 32 marks a tensor that takes its first step)
};
static_assert(offsetof(SgdTensor, p) == 0 && offsetof(AdamTensor, p) == 0 && offsetof(SgdTensor, g) == 8 && offsetof(AdamTensor, g) == 8 &&
                  offsetof(SgdTensor, g2) == 16 && offsetof(AdamTensor, g2) == 16 && offsetof(SgdTensor, buf) == 24 &&
                  offsetof(AdamTensor, m) == 24 && offsetof(SgdTensor, group) == offsetof(SgdTensor, n) + 8 &&
                  offsetof(AdamTensor, group) == offsetof(AdamTensor, n) + 8,
              "GradRow: p, g, g2 and the state pointer at bytes 0, 8, 16 and 24 of either row, `group` right after n");
__device__ __forceinline__ GradRow grad_row(const char* rows, int row_bytes, int n_off, int tensor) {
  const char* row = rows + (size_t)tensor * row_bytes;
  const auto ptr = [&](int off) { return *reinterpret_cast<const float* const*>(row + off); };
  return GradRow{ptr(0), ptr(8), ptr(16), ptr(24), *reinterpret_cast<const int64_t*>(row + n_off),
                 *reinterpret_cast<const int64_t*>(row + n_off + 8)};
}

// host: the byte offset of n in a row of `row_bytes`; a row_bytes that names neither table is entry point `what`'s error
inline int grad_row_n_off(const char* what, int row_bytes, int* n_off) {
  DASAC_REQUIRE(row_bytes == (int)sizeof(SgdTensor) || row_bytes == (int)sizeof(AdamTensor),
                "%s: row_bytes names the table, 48 (dasac_sgd_step) or 64 (dasac_adam_step)", what);
  *n_off = row_bytes == (int)sizeof(SgdTensor) ? (int)offsetof(SgdTensor, n) : (int)offsetof(AdamTensor, n);
  return DASAC_OK;
}

}  // namespace dasac
