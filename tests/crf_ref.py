"""The mean-field CRF of include/dasac_hip.h (dasac_crf_meanfield) restated in torch on the CPU, the synthetic scene its tests run
on, and the parity cases the CPU and the GPU tests share (a helper, not a conftest).

    u_i[c]  = log(max(P_i[c], 1e-20)),  Q^0 = P
    k_ij    = w_app exp(-|o|^2 / (2 theta_alpha^2) - sum_ch (I_i - I_j)^2 / (2 theta_beta^2)) + w_smooth exp(-|o|^2 / (2 theta_gamma^2))
              for the taps o = (d a, d b), a, b in [-r, r], (a, b) != (0, 0), row-major in (a, b), j = i + o inside the image
    m_i[c]  = sum_j k_ij Q^(t-1)_j[c] / sum_j k_ij   (0 when no neighbour lies in the image)
    Q^t_i   = softmax_c(u_i[c] + compat m_i[c])
"""
import functools

import torch
import torch.nn.functional as F

from crf import CrfParams

FLOOR = 1e-20


def taps(params):
    """[(dy, dx)] in the order the definition sums them."""
    r, d = params.radius, params.dilation
    return [(a * d, b * d) for a in range(-r, r + 1) for b in range(-r, r + 1) if (a, b) != (0, 0)]


def crf_ref(P, I, params, dtype=torch.float64):
    """Q after params.n_iter updates, [B,C,H,W] in `dtype`, every operation in `dtype` on the CPU."""
    P, I = P.detach().cpu().to(dtype), I.detach().cpu().to(dtype)
    B, C, H, W = P.shape
    h = params.radius * params.dilation
    pad = (h, h, h, h)
    window = lambda t, dy, dx: t[..., h + dy:h + dy + H, h + dx:h + dx + W]
    I_pad, inside = F.pad(I, pad), F.pad(torch.ones(1, H, W, dtype=dtype), pad)
    ks, den = [], torch.zeros(B, H, W, dtype=dtype)
    for dy, dx in taps(params):
        o2 = float(dy * dy + dx * dx)
        dist = ((I - window(I_pad, dy, dx)) ** 2).sum(1)
        k = params.w_app * torch.exp(-o2 / (2 * params.theta_alpha ** 2) - dist / (2 * params.theta_beta ** 2))
        k = (k + params.w_smooth * torch.exp(torch.tensor(-o2 / (2 * params.theta_gamma ** 2), dtype=dtype))) * window(inside, dy, dx)
        ks.append(k)
        den = den + k
    u = torch.log(P.clamp_min(FLOOR))
    Q = P
    for _ in range(params.n_iter):
        Q_pad, m = F.pad(Q, pad), torch.zeros_like(P)
        for (dy, dx), k in zip(taps(params), ks):
            m = m + k[:, None] * window(Q_pad, dy, dx)
        m = torch.where(den[:, None] > 0, m / den[:, None].clamp_min(torch.finfo(dtype).tiny), torch.zeros_like(m))
        Q = torch.softmax(u + params.compat * m, 1)
    return Q


def labels_of(Q):
    """(arg-max with the first maximum winning, the winning value, the gap between the two largest values) of Q [B,C,H,W]."""
    conf, lab = Q.max(1).values, Q.argmax(1)                          # torch.argmax: the first index that holds the maximum
    gap = torch.full_like(conf, float("inf"))
    if Q.shape[1] > 1:
        top = Q.topk(2, 1).values
        gap = top[:, 0] - top[:, 1]
    return lab, conf, gap


def scene(B, C, H, W, seed):
    """(P fp32 [B,C,H,W], I fp32 [B,3,H,W], gt int64 [B,H,W]): a piecewise constant ground truth -- a 3 x 2 grid of classes
    (3x // W + 3 (2y // H)) % C with a centred disc of class C - 1 of radius min(H, W) / 4 --, one random colour in [-2, 2]^3 per class,
    the image = colour + 0.15 N(0, 1), and P = softmax(2 onehot + 1.2 N(0, 1)): a noisy classifier whose arg-max is wrong at about
    half the pixels while the image still tells the regions apart."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gt = (3 * x // W + 3 * (2 * y // H)) % C
    disc = (y - (H - 1) / 2) ** 2 + (x - (W - 1) / 2) ** 2 <= (min(H, W) / 4) ** 2
    gt = torch.where(disc, torch.full_like(gt, C - 1), gt)[None].repeat(B, 1, 1)
    colour = torch.rand(C, 3, generator=g) * 4 - 2
    I = colour[gt].permute(0, 3, 1, 2) + 0.15 * torch.randn(B, 3, H, W, generator=g)
    onehot = F.one_hot(gt, C).permute(0, 3, 1, 2).float()
    P = torch.softmax(2 * onehot + 1.2 * torch.randn(B, C, H, W, generator=g), 1)
    return P.contiguous(), I.contiguous(), gt


# (B, C, H, W, r, d, n_iter), other parameters at their defaults except theta_alpha = 0.8 r d.  The kernel's tile is 16 x 64: the first
# case covers two tiles and a ragged rest on both axes; then dilation; generic C with an even iteration count; a window larger than
# the image; one pixel; one iteration (no ping-pong); both limits at once (C = 32, r d = 8); one class (Q = 1).
CASES = [(2, 19, 41, 139, 5, 1, 5), (2, 19, 37, 53, 2, 3, 3), (1, 7, 23, 70, 3, 2, 4), (1, 19, 9, 7, 5, 1, 2), (1, 19, 1, 1, 5, 1, 3),
         (2, 2, 5, 3, 1, 1, 1), (1, 32, 20, 67, 2, 4, 2), (1, 1, 6, 9, 2, 1, 2)]
FLOOR_REL = 1e-6              # fp64_yardstick.FLOOR


def case_params(case):
    r, d, n = case[4:]
    return CrfParams(radius=r, dilation=d, theta_alpha=0.8 * r * d, n_iter=n)


def case_seed(case):
    return 100 * case[2] + case[3] + case[4]


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(P, I, params, Q in float64, Q of the float32 emulation): computed once per case and shared; nobody writes to them."""
    P, I, _ = scene(*case[:4], case_seed(case))
    params = case_params(case)
    return P, I, params, crf_ref(P, I, params, torch.float64), crf_ref(P, I, params, torch.float32)


def allowed_abs_error(Q64, Q32):
    """The absolute Q error the yardstick allows a case: (2 err(float32 emulation vs float64) + 1e-6) max|Q64|, err = max|diff| /
    max|Q64| (conftest.rel_err)."""
    scale = float(Q64.abs().max())
    return (2.0 * float((Q32.double() - Q64).abs().max()) / scale + FLOOR_REL) * scale


def exempt_pixels(case):
    """bool [B,H,W]: where the float64 top-two gap is at most twice the allowed absolute Q error -- the only pixels whose label may
    differ from the float64 one."""
    _, _, _, Q64, Q32 = case_reference(case)
    return labels_of(Q64)[2] <= 2.0 * allowed_abs_error(Q64, Q32)
