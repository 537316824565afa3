"""The mean-field CRF without a GPU: tests/crf_ref.py against a per-pixel restatement and against the identities of the definition,
crf.CrfParams' validation, the one synthetic behaviour the feature is for (a noisy classifier over a clean image), and the cap on
the pixels the GPU parity test may exempt from the exact label comparison."""
import math

import pytest
import torch

import crf_ref as CR
from crf import CrfParams


def _loops(P, I, p):
    """The definition pixel by pixel in Python floats."""
    B, C, H, W = P.shape
    P, I = P.double(), I.double()
    Q = P.clone()
    for _ in range(p.n_iter):
        new = torch.zeros_like(Q)
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    den, m = 0.0, [0.0] * C
                    for dy, dx in CR.taps(p):
                        yy, xx = y + dy, x + dx
                        if not (0 <= yy < H and 0 <= xx < W):
                            continue
                        o2 = dy * dy + dx * dx
                        dist = sum(float(I[b, ch, y, x] - I[b, ch, yy, xx]) ** 2 for ch in range(I.shape[1]))
                        k = p.w_app * math.exp(-o2 / (2 * p.theta_alpha ** 2) - dist / (2 * p.theta_beta ** 2)) + \
                            p.w_smooth * math.exp(-o2 / (2 * p.theta_gamma ** 2))
                        den += k
                        for c in range(C):
                            m[c] += k * float(Q[b, c, yy, xx])
                    logit = [math.log(max(float(P[b, c, y, x]), 1e-20)) + p.compat * (m[c] / den if den > 0 else 0.0) for c in range(C)]
                    top = max(logit)
                    e = [math.exp(v - top) for v in logit]
                    for c in range(C):
                        new[b, c, y, x] = e[c] / sum(e)
        Q = new
    return Q


@pytest.mark.parametrize("r,d,n", [(1, 1, 2), (2, 2, 1), (5, 1, 2)])
def test_crf_ref_equals_the_per_pixel_loops(r, d, n):
    P, I, _ = CR.scene(1, 3, 5, 4, 7)
    P = P * 0.9                                                          # Q^0 = P as given, not renormalised
    p = CrfParams(radius=r, dilation=d, n_iter=n)
    assert float((CR.crf_ref(P, I, p) - _loops(P, I, p)).abs().max()) < 1e-12


def test_no_compatibility_returns_p_renormalised_whatever_the_image():
    P, I, _ = CR.scene(2, 5, 9, 11, 1)
    P = P * torch.rand(2, 1, 9, 11, generator=torch.Generator().manual_seed(2)).clamp_min(0.1)
    want = P.double() / P.double().sum(1, keepdim=True)
    for image in (I, torch.zeros_like(I), I * 100):
        assert float((CR.crf_ref(P, image, CrfParams(compat=0.0, n_iter=3)) - want).abs().max()) < 1e-12


def test_a_single_pixel_is_the_softmax_of_the_unary():
    P = torch.tensor([0.2, 0.5, 0.0, 0.1]).view(1, 4, 1, 1)
    got = CR.crf_ref(P, torch.randn(1, 3, 1, 1), CrfParams())
    want = torch.softmax(torch.log(P.double().clamp_min(1e-20)), 1)
    assert float((got - want).abs().max()) < 1e-15 and float(got[0, 2, 0, 0]) < 1e-19


def test_mirroring_the_inputs_mirrors_the_result():
    P, I, _ = CR.scene(1, 6, 13, 17, 3)
    p = CrfParams(radius=3, dilation=2, n_iter=3)
    for dims in ((-1,), (-2,), (-1, -2)):
        assert float((CR.crf_ref(P.flip(dims), I.flip(dims), p) - CR.crf_ref(P, I, p).flip(dims)).abs().max()) < 1e-12


def test_one_hot_probabilities_keep_their_labels():
    _, I, gt = CR.scene(2, 7, 12, 15, 4)
    lab = torch.randint(0, 7, gt.shape, generator=torch.Generator().manual_seed(5))
    P = torch.nn.functional.one_hot(lab, 7).permute(0, 3, 1, 2).float()
    Q = CR.crf_ref(P, I, CrfParams())
    assert torch.equal(Q.argmax(1), lab) and float(Q.max(1).values.min()) > 1 - 1e-12


def test_crf_params_defaults_and_description():
    p = CrfParams()
    assert p.as_dict() == dict(radius=5, dilation=1, w_app=1.0, theta_alpha=4.0, theta_beta=0.5, w_smooth=0.3, theta_gamma=1.5,
                               compat=4.0, n_iter=5)
    text = p.describe()
    assert "\n" not in text and "11x11" in text and "120 taps" in text and "5 iterations" in text and "theta_beta 0.5" in text
    assert p.replace(n_iter=1) == CrfParams(n_iter=1) and p.replace(n_iter=1) != p and "1 iteration" in p.replace(n_iter=1).describe()
    with pytest.raises(AttributeError):
        p.radius = 3


@pytest.mark.parametrize("bad", [dict(radius=0), dict(radius=6), dict(radius=2.0), dict(dilation=0), dict(dilation=5),
                                 dict(radius=3, dilation=3), dict(radius=5, dilation=2), dict(n_iter=0), dict(n_iter=17),
                                 dict(n_iter=True), dict(theta_alpha=0), dict(theta_beta=0.0), dict(theta_gamma=-1.0),
                                 dict(theta_beta=float("inf")), dict(theta_alpha=float("nan")), dict(w_app=-0.1), dict(w_smooth=-1),
                                 dict(w_app=0, w_smooth=0), dict(compat=-1e-9), dict(compat=float("inf")), dict(compat=float("nan")),
                                 dict(w_app="1")])
def test_crf_params_refuse_every_out_of_range_field(bad):
    with pytest.raises(ValueError):
        CrfParams(**bad)


def test_crf_params_accept_the_limits():
    for ok in (dict(radius=1, dilation=4), dict(radius=2, dilation=4), dict(radius=4, dilation=2), dict(radius=5, dilation=1),
               dict(n_iter=1), dict(n_iter=16), dict(w_app=0), dict(w_smooth=0), dict(compat=0)):
        CrfParams(**ok)


def test_ops_crf_meanfield_refuses_cpu_tensors():
    from dasac_hip import ops, DasacError
    P, I, _ = CR.scene(1, 3, 4, 4, 0)
    with pytest.raises(DasacError):
        ops.crf_meanfield(P, I, CrfParams())
    import driver
    with pytest.raises(DasacError):
        driver.crf_refine(P, I, CrfParams())


@pytest.mark.parametrize("shape,n_iter", [((2, 19, 41, 139), 5), ((2, 19, 37, 53), 4)])
def test_the_crf_more_than_halves_the_pixel_error_of_a_noisy_classifier(shape, n_iter):
    """The one synthetic behaviour: on `scene` the float64 result's pixel error against the ground truth is below half that of
    argmax P (with this seed: 41 x 139, 5 iterations, 0.544 -> 0.080; 37 x 53, 4 iterations, 0.540 -> 0.100)."""
    P, I, gt = CR.scene(*shape, 11)
    before = float((P.argmax(1) != gt).double().mean())
    after = float((CR.crf_ref(P, I, CrfParams(n_iter=n_iter)).argmax(1) != gt).double().mean())
    print("pixel error {} x {}: argmax P {:.3f}, after {} iterations {:.3f}".format(shape[2], shape[3], before, n_iter, after))
    assert before > 0.4 and after < 0.5 * before


@pytest.mark.parametrize("case", CR.CASES, ids=lambda c: "x".join(map(str, c)))
def test_exempt_pixels_of_the_gpu_parity_cases_stay_under_half_a_percent(case):
    """Labels are compared exactly on the GPU except where the float64 top-two gap is at most twice the allowed absolute Q error;
    those pixels are at most 0.5 % of a case, and the float32 emulation flips no label outside them."""
    _, _, _, Q64, Q32 = CR.case_reference(case)
    exempt = CR.exempt_pixels(case)
    gap = CR.labels_of(Q64)[2]
    err32 = float((Q32.double() - Q64).abs().max())
    flips = CR.labels_of(Q32)[0] != CR.labels_of(Q64)[0]
    print("case {}: float32 emulation error {:.2e}, allowed {:.2e}, smallest gap {:.2e}, exempt {} of {}, float32 label flips {}".format(
        case, err32, CR.allowed_abs_error(Q64, Q32), float(gap.min()), int(exempt.sum()), exempt.numel(), int(flips.sum())))
    assert int(exempt.sum()) <= 0.005 * exempt.numel()
    assert not bool((flips & ~exempt).any())
