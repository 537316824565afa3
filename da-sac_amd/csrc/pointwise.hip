// Element-wise helpers: Dropout2d scaling and its Philox masks, gradient joins, ReLU masking, label preparation.  iou_counts, the
// one-layer ancestor of mask_counts, stays at the end: tests/test_kernel_resources_counts.py states what validation.hip holds.
#include "common.hpp"

namespace dasac {

// y[n,c,:] = x[n,c,:] * m[n,c]   (Dropout2d with an explicit keep/(1-p) mask, fcn.py:52,56)
__global__ __launch_bounds__(256) void scale_planes(const float* __restrict__ x, const float* __restrict__ m, int HW,
                                                    float* __restrict__ y, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    y[i] = x[i] * m[i / HW];
}

// out = a + b (gradient joins); c = a*alpha elementwise helpers
__global__ __launch_bounds__(256) void add2(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                            int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = a[i] + b[i];
}

__global__ __launch_bounds__(256) void relu_mask(const float* __restrict__ dy, const float* __restrict__ y,
                                                 float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// models/sac.py:337-338: ignore_mask = (y == -1); y[ignore_mask] = 255  -- one pass, in place
__global__ __launch_bounds__(256) void label_pad_mask(int64_t* __restrict__ y, uint8_t* __restrict__ mask, int64_t n,
                                                      int64_t pad_label, int64_t ignore_label) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const bool pad = y[i] == pad_label;
    mask[i] = pad ? 1 : 0;
    if (pad) y[i] = ignore_label;
  }
}

// Philox4x32-10 (Salmon et al., SC'11): counter (i, stream offset), key = seed
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr.x, p1 = (uint64_t)0xCD9E8D57u * ctr.z;
    ctr = make_uint4((uint32_t)(p1 >> 32) ^ ctr.y ^ key.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.w ^ key.y, (uint32_t)p0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// Dropout2d (fcn.py:52,56): per (n, c) plane  keep/(1-p) with keep ~ Bernoulli(1-p)
__global__ __launch_bounds__(256) void dropout_planes(uint64_t seed, uint64_t offset, float p, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4 r = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const float u = (float)(r.x >> 8) * (1.0f / 16777216.0f);      // uniform on [0, 1), 24 bits
  out[i] = u >= p ? 1.0f / (1.0f - p) : 0.0f;
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_scale_planes(const float* x, const float* plane_scale, int64_t planes, int64_t HW, float* y,
                                  dasac_stream_t stream) {
  DASAC_REQUIRE(x && plane_scale && y && planes > 0 && HW > 0, "scale_planes: bad arguments");
  const int64_t total = planes * HW;
  hipLaunchKernelGGL(scale_planes, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(stream), x, plane_scale, (int)HW, y, total);
  DASAC_CHECK_LAUNCH("scale_planes");
  return DASAC_OK;
}

extern "C" int dasac_add(const float* a, const float* b, float* out, int64_t n, dasac_stream_t stream) {
  DASAC_REQUIRE(a && b && out && n > 0, "add: bad arguments");
  hipLaunchKernelGGL(add2, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), a, b, out, n);
  DASAC_CHECK_LAUNCH("add");
  return DASAC_OK;
}

extern "C" int dasac_relu_mask(const float* dy, const float* y, float* out, int64_t n, dasac_stream_t stream) {
  DASAC_REQUIRE(dy && y && out && n > 0, "relu_mask: bad arguments");
  hipLaunchKernelGGL(relu_mask, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), dy, y, out, n);
  DASAC_CHECK_LAUNCH("relu_mask");
  return DASAC_OK;
}

extern "C" int dasac_label_pad_mask(int64_t* labels, uint8_t* mask, int64_t n, int pad_label, int ignore_label,
                                    dasac_stream_t stream) {
  DASAC_REQUIRE(labels && mask && n > 0, "label_pad_mask: bad arguments");
  hipLaunchKernelGGL(label_pad_mask, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), labels, mask, n,
                     (int64_t)pad_label, (int64_t)ignore_label);
  DASAC_CHECK_LAUNCH("label_pad_mask");
  return DASAC_OK;
}

extern "C" int dasac_dropout_planes(uint64_t seed, uint64_t offset, float p, int64_t planes, float* keep_scale,
                                    dasac_stream_t stream) {
  DASAC_REQUIRE(keep_scale && planes > 0 && p >= 0.f && p < 1.f, "dropout_planes: bad arguments");
  hipLaunchKernelGGL(dropout_planes, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, as_stream(stream), seed, offset, p,
                     planes, keep_scale);
  DASAC_CHECK_LAUNCH("dropout_planes");
  return DASAC_OK;
}

// ------------------------------------------------------------------------------------------------
// Validation counts: utils/metrics.py:9-53 `Jaccard.add_sample` + the argmax of
// train.py:339-469 -- per-class true-positive / false-positive / false-negative pixel counts from the
// upsampled logits in ONE pass (the reference loops over the 19 classes with .item() syncs per batch).
// ------------------------------------------------------------------------------------------------
namespace dasac {

__global__ __launch_bounds__(256) void iou_counts(const float* __restrict__ logits, const int64_t* __restrict__ gt, int C,
                                                  int64_t HW, int64_t total, int ignore_index,
                                                  unsigned long long* __restrict__ counts) {
  __shared__ unsigned int s[3 * 64];
  for (int i = threadIdx.x; i < 3 * 64; i += 256) s[i] = 0;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int64_t b = p / HW, r = p - b * HW;
    const int64_t y = gt[p];
    if (y == ignore_index) continue;        // utils/metrics.py:28-30: only ignore_index pixels are dropped
    const float* lp = logits + b * C * HW + r;
    float best = lp[0];
    int k = 0;
    for (int c = 1; c < C; ++c) {
      const float v = lp[(int64_t)c * HW];
      if (v > best) {
        best = v;
        k = c;
      }
    }
    if (y == k) {
      atomicAdd(&s[k], 1u);                 // tp
    } else {
      atomicAdd(&s[64 + k], 1u);            // fp of the predicted class (also when gt is no class at all, e.g. -1)
      if (y >= 0 && y < C) atomicAdd(&s[128 + (int)y], 1u);      // fn of the true class
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 64; i += 256)
    if (s[i] && (i & 63) < C) atomicAdd(&counts[(i >> 6) * C + (i & 63)], (unsigned long long)s[i]);
}

}  // namespace dasac

extern "C" int dasac_iou_counts(const float* logits, const int64_t* gt, int B, int C, int64_t HW, int ignore_index,
                                int64_t* counts, dasac_stream_t stream) {
  DASAC_REQUIRE(logits && gt && counts && B > 0 && C > 0 && C <= 64 && HW > 0, "iou_counts: bad arguments");
  const int64_t total = (int64_t)B * HW;
  hipLaunchKernelGGL(iou_counts, dim3(stream_grid(total, 256, kNumCu * 8)), dim3(256), 0, as_stream(stream), logits, gt, C, HW, total,
                     ignore_index, reinterpret_cast<unsigned long long*>(counts));
  DASAC_CHECK_LAUNCH("iou_counts");
  return DASAC_OK;
}
