// Class statistics for importance-sampled target selection (stage 2 of the reference's schedule):
//   tools/compute_IS_weights.py:58-83 counts, per label PNG, the pixels of every value but 255 on the host
//   (np.unique + one compare-and-sum per value).  Here the label maps are already on the device as uint8
//   (driver.infer_label_maps), so the counts come from one launch per batch: a per-image 256-bin histogram.
//
// Integer arithmetic only: u32 LDS adds per wave, one u64 global add per non-zero bin per block -- exact, and the same
// bits on every run whatever the order the adds arrive in.
//
// Label maps are mostly large uniform regions, which is the worst input of a one-atomic-per-pixel LDS histogram (64 lanes
// adding to one address serialise).  So runs are merged before they reach LDS:
//   * a lane whose 16 bytes are all equal takes part in a wave-wide match: per distinct value among those lanes ONE lane
//     adds 16 x (number of lanes holding it) -- a wave inside a uniform region does one LDS add per KiB;
//   * every other lane walks its 16 bytes and adds once per run of equal neighbours.
//
// Bounds: each image is split into an unaligned head (< 16 bytes, up to the first 16-byte boundary of the ADDRESS), whole
// 16-byte vectors, and a tail (< 16 bytes).  Vectors are loaded only from [first boundary, first boundary + 16 * n_vec),
// head and tail byte by byte -- no load touches a byte outside its own image, so none leaves [labels, labels + B*HW).
#include "common.hpp"

namespace dasac {

constexpr int kHistBlock = 256;                        // 4 waves, each with a private 256 x u32 histogram (1 KiB)
constexpr int kHistWaves = kHistBlock / kWave;
constexpr int64_t kHistMaxBlockPixels = 1ll << 31;     // a block's u32 bins can not overflow: it sees at most 2^31 + 30 pixels

// adds one lane's 16 bytes (all lanes that call this are active together; `h` is the wave's own histogram)
__device__ __forceinline__ void hist_add16(unsigned int* __restrict__ h, const uint4 v) {
  const unsigned first = v.x & 255u;
  const bool uniform = v.x == first * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x;
  if (uniform) {
    // wave-wide match over the lanes that hold one value each: one add per distinct value.  Its own loop and its own flush, not
    // wave_match / flush_bins of count_stream.hpp: with the add behind the loop the compiler merges it with the walk's last add
    // below, at 69 more instructions, and the 8 us rows did not hold the parent's time (profiles/count_stream_refactor.md)
    const int lane = (int)(threadIdx.x & (kWave - 1));
    bool pending = true;
    while (pending) {
      const unsigned lead = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
      const unsigned long long same = __ballot(first == lead);
      if (first == lead) {
        if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[lead], 16u * (unsigned)__popcll(same));
        pending = false;
      }
    }
  } else {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned cur = first, run = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const unsigned b = (w[i >> 2] >> (8 * (i & 3))) & 255u;
      if (b == cur) {
        ++run;
      } else {
        atomicAdd(&h[cur], run);
        cur = b;
        run = 1;
      }
    }
    atomicAdd(&h[cur], run);
  }
}

// grid: B * blocks_per_image blocks; block (b, j) takes the j-th share of image b's 16-byte vectors, block (b, 0) also the
// image's head and tail bytes.
__global__ __launch_bounds__(kHistBlock) void label_hist(const uint8_t* __restrict__ labels, int64_t HW, int blocks_per_image,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned int s[kHistWaves][256];
  for (int i = threadIdx.x; i < kHistWaves * 256; i += kHistBlock) (&s[0][0])[i] = 0;
  __syncthreads();

  const int64_t b = blockIdx.x / (unsigned)blocks_per_image;
  const int j = (int)(blockIdx.x - b * blocks_per_image);
  const uint8_t* img = labels + b * HW;
  int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(img) & 15u)) & 15u);
  if (head > HW) head = HW;
  const int64_t n_vec = (HW - head) >> 4;
  const int64_t tail = HW - head - (n_vec << 4);       // 0..15
  unsigned int* h = s[threadIdx.x >> 6];

  if (j == 0) {                                        // < 16 + 16 single bytes, all inside the image
    const int t = threadIdx.x;
    if (t < head) atomicAdd(&h[img[t]], 1u);
    if (t >= 32 && t - 32 < tail) atomicAdd(&h[img[head + (n_vec << 4) + (t - 32)]], 1u);
  }

  const int64_t per = (n_vec + blocks_per_image - 1) / blocks_per_image;
  const int64_t v0 = j * per;
  int64_t v1 = v0 + per;
  if (v1 > n_vec) v1 = n_vec;
  const uint4* vec = reinterpret_cast<const uint4*>(img + head);        // 16-byte aligned by construction
  int64_t i = v0;
  for (; i + 4 * kHistBlock <= v1; i += 4 * kHistBlock) {               // four loads in flight per lane
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = vec[i + k * kHistBlock + threadIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) hist_add16(h, v[k]);
  }
  for (i += threadIdx.x; i < v1; i += kHistBlock) hist_add16(h, vec[i]);

  __syncthreads();
  {
    const int t = threadIdx.x;                         // kHistBlock == 256 bins
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kHistWaves; ++w) sum += s[w][t];
    if (sum) atomicAdd(&counts[b * 256 + t], sum);
  }
}

}  // namespace dasac

extern "C" int dasac_label_hist(const uint8_t* labels, int B, int64_t HW, int64_t* counts, dasac_stream_t stream) {
  using namespace dasac;
  DASAC_REQUIRE(labels && counts && B > 0 && HW > 0, "label_hist: bad arguments");
  // blocks per image: about 16 KiB per block (4 vectors per lane) until the grid holds ~16 blocks per CU, and never fewer
  // than keeps a block's pixel count at or below 2^31 (u32 bins)
  int64_t bpi = (HW + 16 * 4 * kHistBlock - 1) / (16 * 4 * kHistBlock);
  const int64_t fill = ((kNumCu - reserved_cus()) * 16 + B - 1) / B;
  if (bpi > fill) bpi = fill;
  const int64_t need = (HW + kHistMaxBlockPixels - 1) / kHistMaxBlockPixels;
  if (bpi < need) bpi = need;
  DASAC_REQUIRE(bpi * B <= 0x7fffffffll, "label_hist: B * HW too large for one launch");
  hipLaunchKernelGGL(label_hist, dim3((unsigned)(bpi * B)), dim3(kHistBlock), 0, as_stream(stream), labels, HW, (int)bpi,
                     reinterpret_cast<unsigned long long*>(counts));
  DASAC_CHECK_LAUNCH("label_hist");
  return DASAC_OK;
}
