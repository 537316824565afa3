"""The float64 yardstick shared by the test_gpu_*_fp64 / *_exact modules (a helper, not a conftest).  For every toleranced tensor,
with conftest's rel_err,
    err(HIP vs fp64) <= 2 * err(ATen-fp32-on-CPU vs fp64) + 1e-6
(the factor of test_resnet101_gradients_fp64_arbitration; 1e-6 is about 8 fp32 ulp of the tensor's max and covers the cases where
ATen lands exactly).  A ratio of 0.5 is an error equal to float32 ATen's."""
from conftest import rel_err

FLOOR = 1e-6


def _ratio(got, ref64, aten32, extra_abs=0.0):
    """err_hip / bound with bound = 2 * err_aten + FLOOR (+ extra_abs relative to the reference's max)."""
    scale = float(ref64.abs().max().clamp_min(1e-30))
    return rel_err(got, ref64) / (2.0 * rel_err(aten32, ref64) + FLOOR + extra_abs / scale)


def _report(what, case, ratios):
    print("{} {}: {}".format(what, case, ", ".join("{} {:.3g}".format(k, v) for k, v in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, (what, case, k, v)        # also false for NaN
