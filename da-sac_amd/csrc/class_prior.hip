// The SAC head on MI355X, the running class prior.
//
//   class_state        models/sac.py:104-117,120,151-152                  running class prior, discount, focal weights
#include "common.hpp"

namespace dasac {

// ---- class prior state (19 floats; one wave) ------------------------------------------------------
// chi update (sac.py:104-117) from the class sums of this batch, then the two derived vectors:
//   disc = 1 - exp(-chi/beta) (sac.py:152), focal = (1 - max(chi,0))^p (sac.py:120,135)
__global__ void class_state(float* __restrict__ chi, const double* __restrict__ csum, double count_hw, int B, int C,
                            float beta, float momentum, float tolerance, int update, float focal_p,
                            float* __restrict__ disc, float* __restrict__ focal) {
  const int c = threadIdx.x;
  if (c >= C) return;
  float v = chi[c];
  if (update) {
    // probs.mean(0).view(C,-1).mean(-1): mean over the batch, then over pixels
    const float avg = (float)((csum[c] / (double)B) / count_hw);
    if (avg > tolerance && v == beta) v = avg;
    v = v * momentum;
    v = v + (1.f - momentum) * avg;
    chi[c] = v;
  }
  // exp correctly rounded to fp32 through the fp64 library (19 lanes: free).  NOT guaranteed bit-equal to the reference's CPU ATen
  // (Sleef's 1-ULP expf for full vectors, libm's for vector tails -- which of the 19 classes take which depends on the host's
  // vector width): the module's default evaluates these vectors on the host for that reason (ops.HostClassVectors); this output
  // serves `SAC.device_thresholds = True` (no host round trip in the step; thresholds within 1 ULP of the host's).
  if (disc) disc[c] = 1.f - (float)exp((double)(-(v / beta)));
  if (focal) {
    const float base = 1.f - fmaxf(v, 0.f);
    float r;
    if (focal_p == 3.f) r = base * base * base;
    else if (focal_p == 2.f) r = base * base;
    else if (focal_p == 1.f) r = base;
    else r = powf(base, focal_p);
    focal[c] = r;
  }
}

}  // namespace dasac

using namespace dasac;

extern "C" int dasac_class_state(float* running_conf, const double* class_sums, int B, int64_t HW, int C, float beta,
                                 float stat_momentum, int update, float focal_p, float* disc, float* focal,
                                 dasac_stream_t stream) {
  DASAC_REQUIRE(running_conf && C > 0 && C <= 64 && (!update || class_sums), "class_state: bad arguments");
  hipLaunchKernelGGL(class_state, dim3(1), dim3(64), 0, as_stream(stream), running_conf, class_sums, (double)HW, B, C, beta,
                     stat_momentum, 1e-8f, update, focal_p, disc, focal);
  DASAC_CHECK_LAUNCH("class_state");
  return DASAC_OK;
}
