// The trainer's epoch summary panels (base_trainer.py:75-198 `BaseTrainer._visualise`, helpers :220-270), rendered where the
// tensors are: ONE launch per batch renders every panel of every image from a small device job table, and thumbnails leave the
// device instead of activations.
//
// What the reference does on the host, per panel (h x w = TB.IM_SIZE, 256 x 256 by default):
//   downsize(x)  F.interpolate(x.float(), (h, w), mode="bilinear", align_corners=True)             (:99-109)
//   denorm(x)    x * STD + MEAN per channel, two roundings                                         (dataloader_seg.py:124-138)
//   cmap(l)      labels through Pillow: saturated to 0..255, palette lookup, / 255                 (:228-248)
//   inferno(v)   256-entry colour table at trunc(v * 256) in float32, clipped to 0..255            (:250-256)
// and four kinds of panel:
//   IMAGE   downsize(denorm(image))                                                                (:119, :148, :172)
//   LABELS  0.3 * backdrop + 0.7 * downsize(cmap(labels))       colours at full resolution         (:123-131)
//   SCORES  p = downsize(softmax(scores, 1) or scores); conf, idx = p.max(1)                       (:134-145, :152-165)
//           panel `column`:  0.3 * backdrop + 0.7 * cmap(idx)    colours at panel resolution
//           panel `column2`: 0.3 * backdrop + 0.7 * inferno(1 - conf)            -- two panels from one read of the scores
//   CONF    0.3 * backdrop + 0.7 * inferno(1 - downsize(conf))                                     (:179-183)
// where backdrop = downsize(denorm(backdrop image)).  An overlay's backdrop is recomputed by the thread that needs it (4 taps x 3
// channels) instead of being read back from the IMAGE panel, so the panels are independent and one launch suffices.  The softmax
// is taken at each of the four taps and every class is resized on its own, as the reference does at full resolution; no
// full-resolution intermediate exists.  Arg-max: the first maximum wins (strict >), an all-zero pixel gives class 0.
//
// Resize weights: ATen's align_corners=True ones, tap_ac / ac_scale of bilinear.hpp; both tap indices stay inside the plane
// whatever the scale is: shrinking, enlarging, extent 1, any H x W.
//
// Shape: block = 64 lanes along output x by 4 output rows; (job, image) = blockIdx.z, so the job record, the image
// bases and the row taps are wave-uniform; a lane adds ONE 32-bit element offset per tap to a scalar plane base.  Plain loads and
// stores only.  The kernel is latency- and launch-bound (<= 76 gathers per pixel task); it has no bandwidth target.
//
// The strip is float32 [B,3,h,P*w] (the reference's `visuals`); the same thread can also write the u8 rows the reference's
// `_visualise_grid` makes of it (:264: `.mul(255).clamp(0, 255).byte()`, truncation).  dasac_vis_grid lays float rows out as
// torchvision's make_grid(nrow=1, padding, pad_value) does (:269).
#include "bilinear.hpp"
#include "common.hpp"

namespace dasac {

constexpr int kVisX = 64, kVisY = 4;                   // one wave per output row segment
constexpr float kVisAlpha = 0.3f;                      // base_trainer.py:124: 0.3 * image + 0.7 * colours

struct VisNorm {                                       // by value
  float mean[3], std[3];
};

// downsize(denorm(img))[ch] at the pixel; `plane` = the channel's H x W plane
__device__ __forceinline__ float vis_image(const float* __restrict__ plane, const TapPix& p, float mean, float std) {
  return tap_mix(p, plane[p.o00] * std + mean, plane[p.o01] * std + mean, plane[p.o10] * std + mean, plane[p.o11] * std + mean);
}

__device__ __forceinline__ int vis_saturate(int64_t v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }

__device__ __forceinline__ int vis_cmap_index(float v) {      // matplotlib Colormap.__call__ on a float32 array, N = 256
  const float xa = v * 256.f;
  if (!(xa >= 0.f)) return 0;
  if (xa >= 256.f) return 255;
  return (int)xa;
}

__device__ __forceinline__ void vis_store(float* __restrict__ strip, uint8_t* __restrict__ rows, size_t base, unsigned off, float v) {
  strip[base + off] = v;
  if (rows) {
    float q = v * 255.f;
    q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);       // a NaN becomes 0, as `.byte()` of a clamped NaN is not defined anyway
    rows[base + off] = (uint8_t)(int)q;
  }
}

// grid: (ceil(w / 64), ceil(h / 4), n_jobs * B)
__global__ __launch_bounds__(kVisX * kVisY) void vis_panels(const dasac_vis_job* __restrict__ jobs, int B, int h, int w, int P,
                                                            const VisNorm norm, const uint8_t* __restrict__ palette,
                                                            const float* __restrict__ cmap, float* __restrict__ strip,
                                                            uint8_t* __restrict__ rows) {
  const int jb = blockIdx.z;
  const int j = jb / B, b = jb - j * B;                // wave-uniform
  const dasac_vis_job job = jobs[j];
  const int x = blockIdx.x * kVisX + (int)(threadIdx.x & (kVisX - 1));
  const int y = blockIdx.y * kVisY + (int)(threadIdx.x >> 6);
  if (x >= w || y >= h) return;

  const int H = job.H, W = job.W, C = job.C;
  const size_t HW = (size_t)H * W;
  const TapPix p = tap_pix(tap_ac(y, ac_scale(H, h), H), tap_ac(x, ac_scale(W, w), W), W);

  const size_t plane_out = (size_t)h * P * w;          // one channel of one image of the strip
  const size_t obase = (size_t)b * 3 * plane_out;      // scalar
  const unsigned ooff = (unsigned)(y * (P * w) + job.column * w + x);
  const unsigned ooff2 = (unsigned)(y * (P * w) + job.column2 * w + x);

  if (job.kind == DASAC_VIS_IMAGE) {
    const float* img = reinterpret_cast<const float*>(job.src) + (size_t)b * 3 * HW;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      vis_store(strip, rows, obase + ch * plane_out, ooff, vis_image(img + ch * HW, p, norm.mean[ch], norm.std[ch]));
    return;
  }

  float back[3];
  {
    const float* img = job.backdrop + (size_t)b * 3 * HW;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) back[ch] = kVisAlpha * vis_image(img + ch * HW, p, norm.mean[ch], norm.std[ch]);
  }

  if (job.kind == DASAC_VIS_LABELS) {
    const int64_t* lab = reinterpret_cast<const int64_t*>(job.src) + (size_t)b * HW;
    const int l00 = vis_saturate(lab[p.o00]) * 3, l01 = vis_saturate(lab[p.o01]) * 3;
    const int l10 = vis_saturate(lab[p.o10]) * 3, l11 = vis_saturate(lab[p.o11]) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float rgb = tap_mix(p, (float)palette[l00 + ch] / 255.f, (float)palette[l01 + ch] / 255.f,
                                (float)palette[l10 + ch] / 255.f, (float)palette[l11 + ch] / 255.f);
      vis_store(strip, rows, obase + ch * plane_out, ooff, back[ch] + 0.7f * rgb);
    }
    return;
  }

  float conf;
  if (job.kind == DASAC_VIS_SCORES) {
    const float* sc = reinterpret_cast<const float*>(job.src) + (size_t)b * C * HW;
    // softmax at each tap: F.softmax(x, 1) = exp(x - max) / sum exp(x - max)
    float m00 = 0.f, m01 = 0.f, m10 = 0.f, m11 = 0.f, r00 = 1.f, r01 = 1.f, r10 = 1.f, r11 = 1.f;
    if (job.softmax) {
      m00 = m01 = m10 = m11 = -INFINITY;
      for (int c = 0; c < C; ++c) {
        const float* pl = sc + (size_t)c * HW;
        m00 = fmaxf(m00, pl[p.o00]);
        m01 = fmaxf(m01, pl[p.o01]);
        m10 = fmaxf(m10, pl[p.o10]);
        m11 = fmaxf(m11, pl[p.o11]);
      }
      float d00 = 0.f, d01 = 0.f, d10 = 0.f, d11 = 0.f;
      for (int c = 0; c < C; ++c) {
        const float* pl = sc + (size_t)c * HW;
        d00 += expf(pl[p.o00] - m00);
        d01 += expf(pl[p.o01] - m01);
        d10 += expf(pl[p.o10] - m10);
        d11 += expf(pl[p.o11] - m11);
      }
      r00 = d00, r01 = d01, r10 = d10, r11 = d11;
    }
    int best = 0;
    float bp = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const float* pl = sc + (size_t)c * HW;
      float v00 = pl[p.o00], v01 = pl[p.o01], v10 = pl[p.o10], v11 = pl[p.o11];
      if (job.softmax) {
        v00 = expf(v00 - m00) / r00;
        v01 = expf(v01 - m01) / r01;
        v10 = expf(v10 - m10) / r10;
        v11 = expf(v11 - m11) / r11;
      }
      const float v = tap_mix(p, v00, v01, v10, v11);
      if (v > bp) {                                    // strict: the first maximum wins, as Tensor.max(1)
        bp = v;
        best = c;
      }
    }
    conf = bp;
    const int l = vis_saturate(best) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      vis_store(strip, rows, obase + ch * plane_out, ooff, back[ch] + 0.7f * ((float)palette[l + ch] / 255.f));
  } else {                                             // DASAC_VIS_CONF: one plane per image
    const float* pl = reinterpret_cast<const float*>(job.src) + (size_t)b * HW;
    conf = tap_mix(p, pl[p.o00], pl[p.o01], pl[p.o10], pl[p.o11]);
  }
  const int k = vis_cmap_index(1.f - conf) * 3;
  const unsigned o = job.kind == DASAC_VIS_SCORES ? ooff2 : ooff;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) vis_store(strip, rows, obase + ch * plane_out, o, back[ch] + 0.7f * cmap[k + ch]);
}

// grid[c][Y][X]: pad_value everywhere, row k of the strip at Y = k * (h + pad) + pad, X = pad; pad = 0 for a single row
__global__ __launch_bounds__(256) void vis_grid(const float* __restrict__ strip, int B, int h, int wt, int pad, int pad_u8,
                                                uint8_t* __restrict__ grid, int GH, int GW) {
  const int X = blockIdx.x * 256 + (int)threadIdx.x, Y = blockIdx.y, c = blockIdx.z;
  if (X >= GW) return;
  int v = pad_u8;
  const int x = X - pad;
  const int k = Y / (h + pad), y = Y - k * (h + pad) - pad;      // scalar
  if (k < B && y >= 0 && x >= 0 && x < wt) {
    float q = strip[(((size_t)k * 3 + c) * h + y) * wt + x] * 255.f;
    q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
    v = (int)q;
  }
  grid[((size_t)c * GH + Y) * GW + X] = (uint8_t)v;
}

}  // namespace dasac

extern "C" int dasac_vis_panels(const dasac_vis_job* jobs, const dasac_vis_job* jobs_host, int n_jobs, int B, int h, int w,
                                int P, const float* mean3, const float* std3, const uint8_t* palette, const float* cmap,
                                float* strip, uint8_t* rows_u8, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(jobs && jobs_host && mean3 && std3 && palette && cmap && strip, "vis_panels: null pointer");
  DASAC_REQUIRE(n_jobs > 0 && B > 0 && h > 0 && w > 0 && P > 0, "vis_panels: n_jobs, B, h, w and P must be positive");
  DASAC_REQUIRE((int64_t)n_jobs * B <= 65535 && (h + kVisY - 1) / kVisY <= 65535, "vis_panels: too many jobs x images or rows");
  DASAC_REQUIRE((int64_t)h * P * w <= 0x7fffffffll, "vis_panels: one channel of the strip must stay below 2^31 elements");
  for (int j = 0; j < n_jobs; ++j) {                   // the host copy of the table is what the bounds are checked on
    const dasac_vis_job& q = jobs_host[j];
    DASAC_REQUIRE(q.kind >= DASAC_VIS_IMAGE && q.kind <= DASAC_VIS_CONF, "vis_panels: job %d: unknown kind %d", j, q.kind);
    DASAC_REQUIRE(q.src && (q.kind == DASAC_VIS_IMAGE || q.backdrop), "vis_panels: job %d: null source or backdrop", j);
    DASAC_REQUIRE(q.H > 0 && q.W > 0 && (int64_t)q.H * q.W <= 0x7fffffffll, "vis_panels: job %d: bad source size", j);
    DASAC_REQUIRE(q.kind != DASAC_VIS_SCORES || q.C > 0, "vis_panels: job %d: scores need C > 0", j);
    DASAC_REQUIRE(q.column >= 0 && q.column < P, "vis_panels: job %d: column %d outside the strip of %d panels", j, q.column, P);
    DASAC_REQUIRE(q.kind != DASAC_VIS_SCORES || (q.column2 >= 0 && q.column2 < P && q.column2 != q.column),
                  "vis_panels: job %d: second column %d outside the strip of %d panels", j, q.column2, P);
    const uintptr_t a = reinterpret_cast<uintptr_t>(q.src);
    DASAC_REQUIRE((a & (q.kind == DASAC_VIS_LABELS ? 7u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(q.backdrop) & 3u) == 0,
                  "vis_panels: job %d: fp32 / int64 tensors must be aligned to their element size", j);
  }
  DASAC_REQUIRE((reinterpret_cast<uintptr_t>(strip) & 3u) == 0 && (reinterpret_cast<uintptr_t>(cmap) & 3u) == 0,
                "vis_panels: fp32 tensors must be 4-byte aligned");
  VisNorm norm;
  for (int i = 0; i < 3; ++i) norm.mean[i] = mean3[i], norm.std[i] = std3[i];
  const dim3 grid((unsigned)((w + kVisX - 1) / kVisX), (unsigned)((h + kVisY - 1) / kVisY), (unsigned)(n_jobs * B));
  hipLaunchKernelGGL(vis_panels, grid, dim3(kVisX * kVisY), 0, as_stream(stream), jobs, B, h, w, P, norm, palette, cmap, strip,
                     rows_u8);
  DASAC_CHECK_LAUNCH("vis_panels");
  return DASAC_OK;
}

extern "C" int dasac_vis_grid(const float* strip, int B, int h, int wt, int padding, float pad_value, uint8_t* grid,
                              dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(strip && grid, "vis_grid: null pointer");
  DASAC_REQUIRE(B > 0 && h > 0 && wt > 0 && padding >= 0, "vis_grid: bad shape");
  const int pad = B > 1 ? padding : 0;                 // make_grid returns a single image as it is
  const int64_t GH = (int64_t)B * (h + pad) + pad, GW = (int64_t)wt + pad;
  DASAC_REQUIRE(GH <= 65535 && GW <= 0x7fffffffll, "vis_grid: grid too large");
  float q = pad_value * 255.f;
  q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
  const dim3 g((unsigned)((GW + 255) / 256), (unsigned)GH, 3);
  hipLaunchKernelGGL(vis_grid, g, dim3(256), 0, as_stream(stream), strip, B, h, wt, pad, (int)q, grid, (int)GH, (int)GW);
  DASAC_CHECK_LAUNCH("vis_grid");
  return DASAC_OK;
}
