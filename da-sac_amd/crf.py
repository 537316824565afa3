"""Parameters of the mean-field CRF refinement of inference label maps (ops.crf_meanfield, driver.crf_refine; the arithmetic is
defined in include/dasac_hip.h: dasac_crf_meanfield).

The defaults are STARTING VALUES in the range the ConvCRF and DeepLab papers use, with theta_beta in the units of the normalised
image.  Nobody has measured their effect on a real checkpoint -- none is available to this project -- so they carry no claim about
mIoU or Boundary IoU: tune them on a validation set with `validation_iou(..., crf=params, boundary_radius=R)`."""
import math

# the limits of dasac_crf_meanfield
MAX_RADIUS, MAX_DILATION, MAX_HALO, MAX_ITER = 5, 4, 8, 16
FIELDS = ("radius", "dilation", "w_app", "theta_alpha", "theta_beta", "w_smooth", "theta_gamma", "compat", "n_iter")


class CrfParams:
    """radius r, dilation d: the window is the (2r+1)^2 taps at offsets (d a, d b), the pixel itself left out; r in 1..5, d in 1..4,
    r d <= 8.  Kernel weight of a tap at offset o between pixels i and j:
        w_app exp(-|o|^2 / (2 theta_alpha^2) - |I_i - I_j|^2 / (2 theta_beta^2)) + w_smooth exp(-|o|^2 / (2 theta_gamma^2))
    compat: the Potts weight of the normalised message; n_iter: parallel mean-field updates, 1..16.  Validated on construction
    (ValueError) and immutable afterwards."""
    __slots__ = FIELDS

    def __init__(self, radius=5, dilation=1, w_app=1.0, theta_alpha=4.0, theta_beta=0.5, w_smooth=0.3, theta_gamma=1.5, compat=4.0,
                 n_iter=5):
        def integer(name, v, lo, hi):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError("CrfParams: {} must be an integer in {}..{} (got {!r})".format(name, lo, hi, v))
            return v

        def real(name, v, positive):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (positive and v <= 0):
                raise ValueError("CrfParams: {} must be a finite number {} 0 (got {!r})".format(name, ">" if positive else ">=", v))
            return float(v)
        values = dict(radius=integer("radius", radius, 1, MAX_RADIUS), dilation=integer("dilation", dilation, 1, MAX_DILATION),
                      w_app=real("w_app", w_app, False), theta_alpha=real("theta_alpha", theta_alpha, True),
                      theta_beta=real("theta_beta", theta_beta, True), w_smooth=real("w_smooth", w_smooth, False),
                      theta_gamma=real("theta_gamma", theta_gamma, True), compat=real("compat", compat, False),
                      n_iter=integer("n_iter", n_iter, 1, MAX_ITER))
        if values["radius"] * values["dilation"] > MAX_HALO:
            raise ValueError("CrfParams: radius * dilation must be at most {} (got {} * {})".format(MAX_HALO, radius, dilation))
        if values["w_app"] + values["w_smooth"] <= 0:
            raise ValueError("CrfParams: w_app and w_smooth must not both be 0")
        for k, v in values.items():
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("CrfParams is immutable; build a new one with replace()")

    def replace(self, **changes):
        """A new, validated CrfParams with some fields changed."""
        return CrfParams(**dict(self.as_dict(), **changes))

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS}

    def __eq__(self, other):
        return isinstance(other, CrfParams) and self.as_dict() == other.as_dict()

    __hash__ = None

    def __repr__(self):
        return "CrfParams({})".format(", ".join("{}={!r}".format(k, getattr(self, k)) for k in FIELDS))

    def describe(self):
        """One line for the log."""
        side = 2 * self.radius + 1
        return ("CRF: {}x{} window, dilation {} ({} taps, reach {} px), appearance {:g} (theta_alpha {:g} px, theta_beta {:g}), "
                "smoothness {:g} (theta_gamma {:g} px), compat {:g}, {} iteration{}".format(
                    side, side, self.dilation, side * side - 1, self.radius * self.dilation, self.w_app, self.theta_alpha, self.theta_beta,
                    self.w_smooth, self.theta_gamma, self.compat, self.n_iter, "" if self.n_iter == 1 else "s"))
