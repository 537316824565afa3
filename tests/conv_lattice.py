"""Operands on which every conv GEMM path must be BIT-exact, their float64 references and the condition that makes it so.

fp32 adds and multiplies of integers are exact while every intermediate stays below 2^24 in magnitude, so on integer operands
(with power-of-two per-channel scales) any summation order -- one block per tile, stream-K, the split-K tail, the pixel-split
weight gradient, the Winograd transforms, three bf16 MFMAs per product -- gives the same bits as an integer reference.  A kernel
result that differs from the reference on these inputs has a dropped, duplicated or misaddressed term or an unwritten element:
there is no rounding to hide behind, hence no tolerance anywhere.

Everything here is computed on the CPU from the reference operands alone (float64 ATen); nothing reads a kernel's output.
Plain helper module: test_conv_exact_cpu.py checks the lattice claims, test_gpu_conv_exact.py runs the kernels."""
import numpy as np
import torch
import torch.nn.functional as F

P24 = float(2 ** 24)          # integers of magnitude < 2^24 are exact in fp32, and so is every sum of them that stays below it
ZERO_FRACTION = 1.0 / 3.0     # a third of every operand is zero: mixed ReLU / mask patterns, taps that contribute nothing
SCALES = (0.5, 1.0, 2.0, 4.0)


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, hi, g, zero=ZERO_FRACTION, lo=1):
    """fp32 tensor: magnitude uniform in lo..hi, random sign, `zero` of the entries zeroed."""
    mag = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    keep = (torch.rand(tuple(shape), generator=g) >= zero).float()
    return mag * sign * keep


def pow2(n, g):
    return torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=g)]


def tailed(shape, g, zero=ZERO_FRACTION):
    """Split-bf16 operand WITH a tail: +-(256 a + b), a in 1..3, b in {-1, 0, 1} (257 = head 256 + tail 1; 10 significant bits
    at most, bf16 keeps 8), a third zeroed."""
    a = torch.randint(1, 4, tuple(shape), generator=g).float()
    b = torch.randint(-1, 2, tuple(shape), generator=g).float()
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    keep = (torch.rand(tuple(shape), generator=g) >= zero).float()
    return sign * (256 * a + b) * keep


def out_hw(branches, stride, H, W):
    kh, kw, d, p = branches[0]
    return (H + 2 * p - d * (kh - 1) - 1) // stride + 1, (W + 2 * p - d * (kw - 1) - 1) // stride + 1


# ----------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------
def plain_operands(cin, cout, branches, stride, shape, seed=0, x_hi=3, w_hi=2, nonneg_x=False):
    """The plain lattice: x, dz, res integers in [-3, 3], w in [-2, 2], shift in [-8, 8], scale in {0.5, 1, 2, 4}."""
    N, H, W = shape
    OH, OW = out_hw(branches, stride, H, W)
    g = gen(1000 * seed + 7 * cin + 3 * cout + H + W)
    x = ints((N, cin, H, W), x_hi, g)
    if nonneg_x:
        x = x.abs()
    return {
        "x": x,
        "ws": [ints((cout, cin, kh, kw), w_hi, g) for kh, kw, _, _ in branches],
        "dz": ints((N, cout, OH, OW), 3, g),
        "shift": ints((cout,), 8, g),
        "scale": pow2(cout, g),
        "res_out": ints((N, cout, OH, OW), 3, g),
        "res_in": ints((N, cin, H, W), 3, g),
        "mask_in": ints((N, cin, H, W), 3, g),           # an fp32 activation: kept where > 0
        "mask_out": ints((N, cout, OH, OW), 3, g),
    }


def stats_operands(cin, cout, branch, shape, seed=0):
    """The statistics lattice: x and w in {-1, 0, 1}, so that a tile's sum of SQUARES of the outputs stays exact too."""
    ops = plain_operands(cin, cout, [branch], 1, shape, seed + 50, x_hi=1, w_hi=1)
    return {"x": ops["x"], "ws": ops["ws"], "bias": ops["shift"]}


def x3_operands(cls, cin, cout, branches, stride, shape, seed=0):
    """Split-bf16 lattices.  A product of the bf16x3 kernels is ah*bh + ah*bl + al*bh (the tail x tail term is dropped); with one
    operand of every product bf16-exact (tail 0) the dropped term is exactly zero and each class exercises one cross term:
      class "A": the streamed operand carries the tail -- activations x (forward), dz (data gradient, weight gradient) -- and
                 the other one -- weights; x in the weight gradient -- is a bf16-exact integer in [-2, 2];
      class "B": the roles swapped.
    Returns the operand pairs per GEMM: fwd (x, ws), dgrad (dz, ws), wgrad (dz, x), and the plain-lattice epilogue operands."""
    assert cls in ("A", "B")
    N, H, W = shape
    OH, OW = out_hw(branches, stride, H, W)
    g = gen(4000 + 1000 * seed + 7 * cin + 3 * cout + H + W + (0 if cls == "A" else 17))
    big = lambda s: tailed(s, g)
    small = lambda s: ints(s, 2, g)
    first, second = (big, small) if cls == "A" else (small, big)
    wshapes = [(cout, cin, kh, kw) for kh, kw, _, _ in branches]
    return {
        "fwd": (first((N, cin, H, W)), [second(s) for s in wshapes]),
        "dgrad": (first((N, cout, OH, OW)), [second(s) for s in wshapes]),
        "wgrad": (first((N, cout, OH, OW)), second((N, cin, H, W))),
        "shift": ints((cout,), 8, g),
        "res_out": ints((N, cout, OH, OW), 3, g),
        "mask_in": ints((N, cin, H, W), 3, g),
    }


# ----------------------------------------------------------------------------------------------
# references (float64 by default; the same functions in float32 are ATen's own summation order)
# ----------------------------------------------------------------------------------------------
def _scaled(ws, scale, dtype):
    return [w.to(dtype) * (1 if scale is None else scale.to(dtype).view(-1, 1, 1, 1)) for w in ws]


def conv_fwd(x, ws, branches, stride, scale=None, dtype=torch.float64):
    """sum_b conv2d(x, scale * w_b)."""
    return sum(F.conv2d(x.to(dtype), w, None, stride, p, d) for w, (_, _, d, p) in zip(_scaled(ws, scale, dtype), branches))


def conv_dx(dz, ws, branches, stride, in_hw, scale=None, dtype=torch.float64):
    """sum_b conv_transpose2d(dz, scale * w_b): the data gradient (off-lattice positions of a strided conv are zero)."""
    H, W = in_hw
    OH, OW = dz.shape[2:]
    out = 0
    for w, (kh, kw, d, p) in zip(_scaled(ws, scale, dtype), branches):
        oph = H - ((OH - 1) * stride - 2 * p + d * (kh - 1) + 1)
        opw = W - ((OW - 1) * stride - 2 * p + d * (kw - 1) + 1)
        out = out + F.conv_transpose2d(dz.to(dtype), w, None, stride, p, (oph, opw), 1, d)
    return out


def conv_dw(dz, x, ws, branches, stride, scale=None, dtype=torch.float64):
    """[scale[co] * sum over batch and pixels of dz * shifted x per branch]: autograd of the forward."""
    wr = [w.to(dtype).requires_grad_(True) for w in ws]
    s = 1 if scale is None else scale.to(dtype).view(-1, 1, 1, 1)
    out = sum(F.conv2d(x.to(dtype), w * s, None, stride, p, d) for w, (_, _, d, p) in zip(wr, branches))
    return list(torch.autograd.grad(out, wr, dz.to(dtype)))


def f32(t):
    """The float64 reference as the fp32 tensor a kernel must reproduce bit for bit; the reference itself must be an integer
    lattice point that fp32 holds."""
    r = t.to(torch.float32)
    assert torch.equal(r.double(), t), "the reference is not representable in fp32"
    return r


# ----------------------------------------------------------------------------------------------
# the exactness precondition: per-output sum of |a||b| (the same convolution on absolute values, float64) below 2^24
# ----------------------------------------------------------------------------------------------
def _below(t, limit=P24):
    return bool(float(torch.as_tensor(t).abs().max()) < limit)


def exact_ok(x, ws, branches, stride, dz=None, scale=None, shift=None, res_out=None, res_in=None, dtype=torch.float64,
             parts=("fwd", "dx", "dw")):
    """True when every partial sum of the forward (x, ws, with its epilogue operands), the data gradient (dz, ws, with its
    residual) and the weight gradient (dz, x; scaled and unscaled: the kernel multiplies by scale last) stays below 2^24
    whatever the order.  `parts` names the contractions the caller runs on these operands."""
    xa, wa = x.abs(), [w.abs() for w in ws]
    sa = None if scale is None else scale.abs()
    ok = True
    if "fwd" in parts:
        fwd = conv_fwd(xa, wa, branches, stride, sa, dtype)
        if shift is not None:
            fwd = fwd + shift.abs().to(dtype).view(1, -1, 1, 1)
        if res_out is not None:
            fwd = fwd + res_out.abs().to(dtype)
        ok = ok and _below(fwd)
    if dz is not None and "dx" in parts:
        dx = conv_dx(dz.abs(), wa, branches, stride, x.shape[2:], sa, dtype)
        if res_in is not None:
            dx = dx + res_in.abs().to(dtype)
        ok = ok and _below(dx)
    if dz is not None and "dw" in parts:
        for dw in conv_dw(dz.abs(), xa, wa, branches, stride, None, dtype):
            ok = ok and _below(dw) and (sa is None or _below(dw * sa.to(dtype).view(-1, 1, 1, 1)))
        ok = ok and _below(dz.abs().to(dtype).sum((0, 2, 3)))                 # sum_dz
    return ok


def tile_sums(out, tile=128):
    """(sum, sum of squares) [tiles, M] of `out` [N, M, OH, OW] over the tiles of `tile` consecutive flattened (n, oh, ow) pixels."""
    N, M, OH, OW = out.shape
    flat = out.double().permute(1, 0, 2, 3).reshape(M, -1)
    tiles = (flat.shape[1] + tile - 1) // tile
    flat = F.pad(flat, (0, tiles * tile - flat.shape[1])).view(M, tiles, tile)
    return flat.sum(-1).t().contiguous(), (flat * flat).sum(-1).t().contiguous()


def stats_exact_ok(out, tile=128):
    """Tile statistics: sum |out| and sum out^2 over ANY `tile` consecutive pixels below 2^24 (a superset of the aligned tiles)."""
    N, M, OH, OW = out.shape
    flat = out.double().permute(1, 0, 2, 3).reshape(M, -1)
    for v in (flat.abs(), flat * flat):
        c = F.pad(v.cumsum(1), (1, 0))
        n = c.shape[1] - 1
        win = c[:, min(tile, n):] - c[:, :n + 1 - min(tile, n)]
        if not _below(win):
            return False
    return True


def dot_rows_ref(w, g_unscaled, block=64, flat=False):
    """[rows, Cout]: row r = sum over input channels 64 r .. 64 r + 63 and taps of W * G (G: the UNSCALED weight gradient).
    flat (layers of fewer than 32 input channels): the rows run along the whole k axis instead, k = tap * Cin + ci; the row count
    of either form is dasac_conv_wgrad_dot_rows(Cin, taps)."""
    cout, cin = w.shape[:2]
    prod = (w.double() * g_unscaled.double()).reshape(cout, cin, -1)
    if flat:
        prod, cin = prod.transpose(1, 2).reshape(cout, -1), prod.shape[1] * prod.shape[2]
    else:
        prod = prod.sum(-1)                                                           # [cout, cin]
    rows = (cin + block - 1) // block
    prod = F.pad(prod, (0, rows * block - cin)).view(cout, rows, block).sum(-1)
    return prod.t().contiguous()


def dot_exact_ok(w, dz, x, branches, stride):
    """sum |W||G| per 64-channel block below 2^24, with |G| bounded by sum |dz||x|."""
    (ga,) = conv_dw(dz.abs(), x.abs(), [w.abs()], branches, stride)
    return _below(dot_rows_ref(w.abs(), ga, flat=w.shape[1] < 32))


def bn_param_grads_ref(dot, sum_dz, mean, invstd, scale, conv_bias):
    """dgamma = invstd * (sum_rows dot + (bias - mean) * sum_dz), dbeta = sum_dz, dbias = scale * sum_dz (float64)."""
    d = dot.double().sum(0)
    s = sum_dz.double()
    return invstd.double() * (d + (conv_bias.double() - mean.double()) * s), s, scale.double() * s


def bn_param_grads_exact_ok(dot_abs, sum_dz_abs, mean, conv_bias):
    return _below(dot_abs.double().sum(0) + (conv_bias.abs().double() + mean.abs().double()) * sum_dz_abs.double())


# ----------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3): the transforms as csrc/winograd.hip writes them
# ----------------------------------------------------------------------------------------------
WG = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
WBT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
WAT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def winograd_quantum(scale):
    """Spacing of the transformed-filter lattice: g = scale * w is a multiple of min(scale, 1), G g G^T halves it twice."""
    return 0.25 * min(1.0, float(scale.min()) if scale is not None else 1.0)


def winograd_exact_ok(x, w, dilation, scale=None, quantum=None):
    """Point GEMMs: with U on a lattice of spacing q (1/4 for integer g) and V integer, every product is a multiple of q and the
    sums are exact while sum |U||V| < 2^24 q (2^22 at q = 1/4).  Bounded from above for every 4x4 patch origin (a superset of
    the tiles) and every output channel at once: |V| <= |B^T| |d| |B| is a 4x4 dilated correlation of |x|, |U| <= max over m.
    The output transform adds nine integers of the point results: 9 x the bound below 2^24 as well."""
    s = 1.0 if scale is None else scale.double().view(-1, 1, 1, 1)
    g = (w.double() * s).numpy()
    u = np.abs(np.einsum("ai,mcij,bj->abmc", WG, g, WG)).max(axis=2)                      # [4, 4, C]: max over m of |U|
    k = np.einsum("abc,ay,bx->abcyx", u, np.abs(WBT), np.abs(WBT)).reshape(16, -1, 4, 4)   # |U| |B^T|[a][ky] |B^T|[b][kx]
    bound = F.conv2d(x.abs().double(), torch.from_numpy(k), None, 1, 3 * dilation, dilation)
    q = winograd_quantum(scale) if quantum is None else quantum
    return _below(bound, P24 * q) and _below(9 * bound)


def winograd_emulate(x, w, dilation, scale=None):
    """numpy fp32 emulation of the three transforms around fp32 point sums, per output 2x2 tile of every dilation phase, with the
    operation order of csrc/winograd.hip.  x [N,C,H,W], w [M,C,3,3] -> out [N,M,H,W] fp32 (padding == dilation)."""
    f = np.float32
    xn, wn = x.numpy().astype(f), w.numpy().astype(f)
    if scale is not None:
        wn = wn * scale.numpy().astype(f).reshape(-1, 1, 1, 1)
    half = f(0.5)
    # filter: t = G g (rows), u = t G^T (columns), as filter_transform
    t = np.stack([wn[:, :, 0], half * ((wn[:, :, 0] + wn[:, :, 2]) + wn[:, :, 1]), half * ((wn[:, :, 0] + wn[:, :, 2]) - wn[:, :, 1]),
                  wn[:, :, 2]], axis=2)                                                    # [M, C, 4, 3]
    u = np.stack([t[..., 0], half * ((t[..., 0] + t[..., 2]) + t[..., 1]), half * ((t[..., 0] + t[..., 2]) - t[..., 1]), t[..., 2]],
                 axis=3)                                                                   # [M, C, 4, 4]
    N, C, H, W = xn.shape
    M, d = wn.shape[0], dilation
    out = np.zeros((N, M, H, W), dtype=f)
    for py in range(min(d, H)):
        for px in range(min(d, W)):
            sub = xn[:, :, py::d, px::d]                                                   # one phase: a dense 3x3, padding 1
            h, w_ = sub.shape[2:]
            th, tw = (h + 1) // 2, (w_ + 1) // 2
            pad = np.zeros((N, C, 2 * th + 2, 2 * tw + 2), dtype=f)
            pad[:, :, 1:1 + h, 1:1 + w_] = sub
            res = np.zeros((N, M, 2 * th, 2 * tw), dtype=f)
            for ty in range(th):
                for tx in range(tw):
                    dd = pad[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]                   # [N, C, 4, 4]
                    r = np.stack([dd[:, :, 0] - dd[:, :, 2], dd[:, :, 1] + dd[:, :, 2], dd[:, :, 2] - dd[:, :, 1],
                                  dd[:, :, 1] - dd[:, :, 3]], axis=2)                      # B^T d
                    v = np.stack([r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 2] - r[..., 1], r[..., 1] - r[..., 3]],
                                 axis=3)                                                   # (B^T d) B
                    y = np.einsum("mcab,ncab->nmab", u, v).astype(f)                        # 16 point sums over c (fp32)
                    for ey in range(2):
                        for ex in range(2):
                            sy, sx = f(-1 if ey else 1), f(-1 if ex else 1)
                            row = [(y[:, :, ey + j, ex] + sx * y[:, :, ey + j, ex + 1]) + sx * y[:, :, ey + j, ex + 2] for j in range(3)]
                            res[:, :, 2 * ty + ey, 2 * tx + ex] = (row[0] + sy * row[1]) + sy * row[2]
            out[:, :, py::d, px::d] = res[:, :, :h, :w_]
    return torch.from_numpy(out)


# ----------------------------------------------------------------------------------------------
# split-bf16: head = bf16(x) (round to nearest even), tail = bf16(x - head), as split_bf16 of csrc/conv_common.hpp
# ----------------------------------------------------------------------------------------------
def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def bf16_split(t):
    a = t.numpy().astype(np.float32)
    head = bf16_round(a)
    tail = bf16_round(a - head)
    return head, tail


# ----------------------------------------------------------------------------------------------
# ReLU bit masks (include/dasac_hip.h: bit (pix & 31) of word [m][pix >> 5], pix = flattened (n, oh, ow))
# ----------------------------------------------------------------------------------------------
def unpack_bits(words, shape):
    """int32 words [M * ceil(Npix / 32)] -> bool [N, M, OH, OW]."""
    N, M, OH, OW = shape
    npix = N * OH * OW
    w = words.view(M, -1).to(torch.int64) & 0xFFFFFFFF
    pix = torch.arange(npix, device=words.device)
    return ((w[:, pix >> 5] >> (pix & 31)) & 1).bool().view(M, N, OH, OW).permute(1, 0, 2, 3)


# ----------------------------------------------------------------------------------------------
# the cases of test_gpu_conv_exact.py (test_conv_exact_cpu.py checks the lattice claims for the same ones)
# ----------------------------------------------------------------------------------------------
SCHEDULE_CASE = ("schedules", 128, 256, [(3, 3, 2, 2)], 1, (2, 33, 41))          # 44 tiles x 72 K-steps: stream-K when asked
# the smallest split-K tail: 8 x 129 = 1032 tiles of 128 x 128 (one leading round of 1024, 8 tail tiles), 72 K-steps
TAIL_CASE = ("tail", 128, 1024, [(3, 3, 2, 2)], 1, (1, 129, 128))
# M = 256: 128-pixel tiles, 1650 pixels (13 tiles, the last ragged); M = 19: the 32-row tile over 256-pixel tiles, 1311 pixels (6 tiles)
PIX_CASES = [("pix_m256", 64, 256, [(1, 1, 1, 0)], 1, (2, 25, 33)), ("pix_m19", 48, 19, [(3, 3, 1, 1)], 1, (3, 19, 23))]
BATCHED = (3, 16, 136, 129)                                                       # entries, C, M (padded to 256), T (two pixel tiles)
X3_BATCH = 2


# ----------------------------------------------------------------------------------------------
# the cases of test_gpu_conv_schedules_exact.py: the hand-off schedules and the weight gradient's split plans at the points where
# their integer rules branch (gemm_schedule_ref.py names what each plan reaches; test_gemm_schedule_cpu.py checks that from the
# model, test_conv_exact_cpu.py the lattice claims).  Same layout: name, cin, cout, branches, stride, (N, H, W)
# ----------------------------------------------------------------------------------------------
_P1, _P3 = [(1, 1, 1, 0)], [(3, 3, 1, 1)]
STREAMK_CASES = [
    ("spans", 256, 1024, _P1, 1, (1, 160, 160)),             # 1600 tiles x 16 steps, 33 per range: deposit, whole tiles, then own
    ("whole_tile_ranges", 256, 1024, _P1, 1, (1, 100, 128)),  # 800 tiles x 16 steps: ranges 512 .. 767 are exactly one tile
    ("aligned", 1024, 256, _P1, 1, (1, 48, 64)),             # 48 tiles x 64 steps = 768 x 4: no remainder, ranges start on tiles
    ("many_contributors", 256, 128, _P3, 1, (1, 24, 32)),    # 6 tiles x 144 steps: 143 contributors to one tile
    ("ragged", 128, 200, _P3, 1, (1, 50, 60)),               # M = 200: two M tiles, rows past M; 3000 pixels: a ragged last tile
    ("three_m_tiles", 1168, 384, _P1, 1, (1, 25, 40)),       # m_tiles = 3, 73 K-steps
]
STREAMK_RESERVED_CASES = STREAMK_CASES[:3] + [SCHEDULE_CASE]  # run at every reserved-CU setting below
RESERVED = (0, 8, 64, 128)
# split-K tails, the library's own choice
TAIL_CASES = [
    ("split5", 1168, 1024, _P1, 1, (2, 1, 9767)),            # 73 steps in 5 ranges, 200 tail tiles, 19534 pixels: ragged last tile
    ("m3", 1040, 384, _P1, 1, (5, 121, 73)),                 # m_tiles = 3: 1023 leading tiles, 15 tail tiles, 65 steps in 8 ranges
    ("m5", 1040, 640, _P1, 1, (1, 160, 172)),                # m_tiles = 5: 1020 leading tiles, 55 tail tiles
    ("two_rounds", 1024, 1024, _P1, 1, (1, 160, 208)),       # 2048 leading tiles, 32 tail tiles
    ("reserved8", 1040, 1024, _P1, 1, (1, 128, 140)),        # planned for 248 CUs: 96 tail tiles
]
TAIL_RESERVED = {"reserved8": 8}                             # name -> reserved CUs the plan is made for (0 otherwise)
# weight gradients
WGRAD_CASES = [
    ("quad", 128, 128, _P1, 1, (1, 59, 70)),                 # 4130 pixels: 16 splits of 288, one empty, the last one 98 pixels
    ("qtap", 128, 128, _P3, 1, (1, 59, 70)),                 # the same over 9 k tiles
    ("k_tile_64", 192, 128, _P1, 1, (1, 59, 70)),            # 64-row k tiles
    ("strided_fast", 128, 256, _P1, 2, (1, 150, 150)),       # 5625 pixels
    ("generic", 48, 19, _P3, 1, (1, 70, 75)),                # the 32-row tile: 20 splits, one empty
    ("bm64", 32, 64, _P3, 1, (1, 70, 75)),                   # the 64-row tile
    ("splits64", 256, 256, _P1, 1, (1, 128, 129)),           # 16512 pixels: 64 splits, 6 empty (the 1x1 reduce kernel)
    ("splits64_3x3", 128, 128, _P3, 1, (1, 128, 129)),       # the same plan over 9 k tiles: the tap-walking reduce kernel at 64 splits
    ("cap_branch", 128, 128, _P1, 1, (1, 448, 448)),         # one tile x 200704 pixels: 768 splits
    ("cap_branch_stem", 3, 64, [(7, 7, 1, 3)], 2, (1, 897, 897)),   # two tiles x 201601 pixels: 384 splits
]
# name -> (x_hi, w_hi) where the long pixel sums need smaller operands than the plain lattice's (3, 2)
WGRAD_HI = {"cap_branch": (1, 1), "cap_branch_stem": (1, 1), "splits64_3x3": (1, 1)}
WGRAD_X3_CASES = [c for c in WGRAD_CASES if c[0] in ("quad", "splits64")]
STREAMK_X3_CASES = [STREAMK_CASES[0], SCHEDULE_CASE]


def gemm_shape(case):
    """(M, Npix, K) of a case's forward GEMM."""
    name, cin, cout, branches, stride, (N, H, W) = case
    OH, OW = out_hw(branches, stride, H, W)
    return cout, N * OH * OW, cin * sum(kh * kw for kh, kw, _, _ in branches)


def wgrad_operands(case):
    name, cin, cout, branches, stride, shape = case
    x_hi, w_hi = WGRAD_HI.get(name, (3, 2))
    return plain_operands(cin, cout, branches, stride, shape, x_hi=x_hi, w_hi=w_hi)


def case_lists():
    """The case lists of the existing kernel tests, cut down as the exact tests use them (imported here, on demand, so that both
    exact test files share one definition)."""
    from test_gpu_bf16x3 import CASES as bf16_cases
    from test_gpu_conv import CASES as conv_cases, STATS_CASES as stats_cases
    from test_gpu_expanded_conv import CASES as expanded_cases
    from test_gpu_winograd import SHAPES as wino_shapes
    conv = [c for c in conv_cases if c[0] != "7x7_fcn_head_cfg5"]
    return {
        # name, cin, cout, branches[(kh,kw,dil,pad)], stride, (N,H,W): the smallest shapes that reach each loader
        "conv": conv,
        # 256 input channels, one branch: four partial dot rows (the general and the one-tap reduction, a strided 1x1, several pixel splits)
        "dot": [c for c in conv if c[1] == 256 and len(c[3]) == 1],
        "stats": stats_cases[:3],
        "winograd": list(wino_shapes),
        "x3": [c for c in bf16_cases if c[0] != 512],
        # the tap-expanded cases whose float64 reference (forward, two gradients, their absolute-value twins) takes under a second
        "expanded": [c for c in expanded_cases if c[4][0] * c[4][1] * c[4][2] * c[1] * c[2] * sum(b[0] * b[1] for b in c[3]) < 2e8],
    }


def x3_exact_ok(o, branches, stride):
    """The precondition of the three split-bf16 GEMMs on their own operand pairs."""
    (x, ws), (dz, wd), (gz, gx) = o["fwd"], o["dgrad"], o["wgrad"]
    return (exact_ok(x, ws, branches, stride, None, None, o["shift"], o["res_out"], parts=("fwd",))
            and exact_ok(gx, wd, branches, stride, dz, parts=("dx",)) and exact_ok(gx, ws, branches, stride, gz, parts=("dw",)))


def expanded_operands(case):
    name, cin, cout, branches, shape, prec = case
    return plain_operands(cin, cout, branches, 1, shape, seed=3, nonneg_x=True)      # x: a ReLU output, as the classifier's input is
