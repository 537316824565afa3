"""Tensor-level wrappers over the C ABI (one function per kernel family)."""
import os

import torch

from . import lib as L


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


class _Profile:
    """Optional per-launch HIP-event timing of the GEMM kernels (bench.py's roofline leg).  Events are
    recorded on the stream the kernels are launched on (torch's current stream); off by default."""

    def __init__(self):
        self.on, self.records = False, []

    def start(self):
        self.on, self.records = True, []

    def stop(self, by_shape=False):
        """Per-kernel-class totals; by_shape=True keys on (class, shape tag) instead (tools/step_shapes.py)."""
        self.on = False
        torch.cuda.synchronize()
        out = {}
        for name, flops, a, b, tag, nbytes in self.records:
            d = out.setdefault((name, tag) if by_shape else name, {"flops": 0.0, "bytes": 0.0, "seconds": 0.0, "launches": 0})
            d["flops"] += flops
            d["bytes"] += nbytes
            d["seconds"] += a.elapsed_time(b) * 1e-3
            d["launches"] += 1
        self.records = []
        return out

    def span(self, name, flops, tag=None, nbytes=0.0):
        """flops / nbytes: ALGORITHMIC work of the launch (2*M*N*K; every operand once)."""
        return _Span(self, name, flops, tag, nbytes) if self.on else _NULL


class _Span:
    def __init__(self, prof, name, flops, tag, nbytes=0.0):
        self.prof, self.name, self.flops, self.tag, self.nbytes = prof, name, flops, tag, nbytes

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.prof.records.append((self.name, self.flops, self.a, b, self.tag, self.nbytes))


class _Null:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


_NULL = _Null()
PROFILE = _Profile()


def pseudo_labels(probs, ignore, upper, lower, disc=None, want_idx=False):
    """models/sac.py:154-187.  probs [B,C,H,W] f32 cuda; ignore bool [B,H,W] or None; disc [C] or None.
    Returns (labels i64 [B,H,W], max_conf f32 [B,1,H,W], max_idx i64 [B,1,H,W] or None)."""
    L.require_gpu(probs, ignore, disc)
    lib = L.load()
    probs = _c(probs)
    B, Cn, H, W = probs.shape
    HW = H * W
    labels = torch.empty((B, H, W), dtype=torch.int64, device=probs.device)
    conf = torch.empty((B, 1, H, W), dtype=torch.float32, device=probs.device)
    idx = torch.empty((B, 1, H, W), dtype=torch.int64, device=probs.device) if want_idx else None
    ign = None if ignore is None else _c(ignore).view(torch.uint8)
    ws_bytes = lib.dasac_pseudo_labels_workspace(B, Cn, HW)
    ws = L.workspace(ws_bytes, probs.device)
    with PROFILE.span("pseudo_labels", 0.0, None, probs.numel() * 4.0 + B * HW * (1 + 8 + 4 + (8 if want_idx else 0))):
        L.check(lib.dasac_pseudo_labels(probs.data_ptr(), L.ptr(ign), L.ptr(disc), float(upper), float(lower), B, Cn, HW,
                                        labels.data_ptr(), conf.data_ptr(), L.ptr(idx), ws.data_ptr(), ws.numel(),
                                        L.stream_ptr()), "dasac_pseudo_labels")
    return labels, conf, idx


# ----------------------------------------------------------------------------------------------
# convolution as implicit GEMM (include/dasac_hip.h: dasac_conv_*)
# ----------------------------------------------------------------------------------------------
class ConvSpec:
    """Static description of one (possibly multi-branch) convolution.
    branches: list of (kh, kw, dilation, padding); stride applies to all."""

    def __init__(self, cin, cout, branches, stride=1):
        self.cin, self.cout, self.stride = int(cin), int(cout), int(stride)
        self.branches = [tuple(int(v) for v in b) for b in branches]
        self.taps = sum(b[0] * b[1] for b in self.branches)
        self.K = self.taps * self.cin            # forward / wgrad contraction length
        self.Kt = self.taps * self.cout          # data-gradient contraction length

    def out_hw(self, h, w):
        kh, kw, d, p = self.branches[0]
        oh = (h + 2 * p - d * (kh - 1) - 1) // self.stride + 1
        ow = (w + 2 * p - d * (kw - 1) - 1) // self.stride + 1
        return oh, ow


_i32 = torch.int32

# Arithmetic of the forward / data-gradient GEMMs:
#   "fp32"   exact fp32 products on v_mfma_f32_32x32x2_f32 (default);
#   "bf16x3" every operand split into bf16 head + tail, three v_mfma_f32_32x32x16_bf16 per product, fp32
#            accumulation (dasac_conv_gemm_x3; ~2^-16 relative error per product, inside the 1e-3 parity bar).
PRECISION = os.environ.get("DASAC_PRECISION", "fp32")


def set_precision(mode):
    global PRECISION
    assert mode in ("fp32", "bf16x3"), mode
    PRECISION = mode


def _finish_pack(packed, M, K):
    """Converts a freshly packed fp32 operand to the split-bf16 layout (in place, same size) when selected."""
    lib = L.load()
    x3 = PRECISION == "bf16x3" and lib.dasac_conv_mpad(M) >= 64
    if x3:
        L.check(lib.dasac_conv_pack_x3(packed.data_ptr(), M, K, packed.data_ptr(), L.stream_ptr()), "dasac_conv_pack_x3")
    packed.dasac_x3 = x3
    return packed


def gemm_order(spec, transposed):
    """K order of the forward / data-gradient GEMM: chunk-major (1) for multi-tap convs whose gathered channel
    count is a multiple of 16, tap-major (0) otherwise.  The weight gradient always uses tap-major tables."""
    C = spec.cout if transposed else spec.cin
    return 1 if (spec.taps > 1 and C % 16 == 0) else 0


def conv_table(spec, plane_h, plane_w, transposed, device, order=0):
    """Gather table for planes of plane_h x plane_w (forward: the input planes; transposed: dz planes)."""
    lib = L.load()
    C = spec.cout if transposed else spec.cin
    K = spec.taps * C
    table = torch.empty((lib.dasac_conv_kpad(K), 4), dtype=_i32, device=device)
    cols = [torch.tensor(c, dtype=_i32) for c in zip(*spec.branches)]   # host arrays: kh, kw, dil, pad
    L.check(lib.dasac_conv_table(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(),
                                 len(spec.branches), C, plane_h, plane_w, int(transposed), int(order), table.data_ptr(),
                                 L.stream_ptr()), "dasac_conv_table")
    return table


def _branch_taps(spec):
    """(taps, first tap on the concatenated K axis) of every branch."""
    tap0 = 0
    for kh, kw, _, _ in spec.branches:
        yield kh * kw, tap0
        tap0 += kh * kw


def conv_pack(spec, weights, transposed, scale=None, out=None, order=0):
    """Packs the branch weight tensors [Cout,Cin,kh,kw] into the [Kpad][Mpad] GEMM operand."""
    lib = L.load()
    L.require_gpu(*weights)
    M = spec.cin if transposed else spec.cout
    K = spec.Kt if transposed else spec.K
    shape = (lib.dasac_conv_kpad(K), lib.dasac_conv_mpad(M))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=weights[0].device)
    for w, (taps, tap0) in zip(weights, _branch_taps(spec)):
        L.check(lib.dasac_conv_pack(_c(w).data_ptr(), L.ptr(scale), spec.cout, spec.cin, taps, tap0, spec.taps,
                                    int(transposed), int(order), out.data_ptr(), L.stream_ptr()), "dasac_conv_pack")
    return _finish_pack(out, M, K)


def bits_ok(M, Cx):
    """True when the fp32 conv GEMM for an output of M channels over Cx gathered channels has a bit-mask variant
    (ReLU patterns as bit masks: 1/32 of the bytes between forward and data gradient)."""
    return PRECISION == "fp32" and bool(L.load().dasac_conv_gemm_bits_ok(int(M), int(Cx)))


class ReluBits:
    """ReLU pattern of one activation tensor [Nb, M, OH, OW] as bits (include/dasac_hip.h: dasac_conv_gemm relu_bits_out)."""

    def __init__(self, Nb, M, OH, OW, device):
        self.shape = (Nb, M, OH, OW)
        self.words = torch.empty(L.load().dasac_relu_bits_words(M, Nb * OH * OW), dtype=torch.int32, device=device)


def stats_ok(M, Cx):
    """True when the conv GEMM for M output channels over Cx gathered channels can leave per-tile channel statistics."""
    return PRECISION == "fp32" and bool(L.load().dasac_conv_gemm_stats_ok(int(M), int(Cx)))


def tile_stats_buffer(Nb, M, OH, OW, device):
    """[pixel tiles, 2, Mpad] fp32: filled by conv_gemm(stats=...) (every slot written), read by bn_train_forward."""
    lib = L.load()
    return torch.empty((lib.dasac_conv_gemm_stats_tiles(Nb, OH, OW), 2, lib.dasac_conv_mpad(M)), dtype=torch.float32, device=device)


def conv_gemm(x, packed, table, out, grid_hw, stride, M, K, ostride=1, shift=None, res=None, mask=None, relu=False, bits_out=None,
              stats=None, schedule=None):
    """out[n,m,oh*os,ow*os] = epilogue(sum_k packed[k][m] * gather(x)); see dasac_conv_gemm.
    mask: fp32 activation (zero where <= 0) or a ReluBits of the output's shape; bits_out: ReluBits to fill (relu only);
    stats: `tile_stats_buffer` to fill with per-tile channel sums / sums of squares of the output (dasac_conv_gemm_stats).
    schedule: None = the library's choice (one block per tile; long-K layers with a ragged last round: whole rounds one block per
    tile + a split-K tail in the same launch; few tiles x long K: the persistent stream-K kernel); 1 / 2 force one block per tile /
    the persistent stream-K kernel (tests, tools)."""
    lib = L.load()
    L.require_gpu(x, packed, table, out)
    Nb, Cx, H, W = x.shape
    OH, OW = grid_hw
    assert out.shape[0] == Nb and out.shape[1] == M and x.is_contiguous() and out.is_contiguous()
    mask_bits = None
    if isinstance(mask, ReluBits):
        assert mask.shape == tuple(out.shape) and ostride == 1
        mask_bits, mask = mask.words, None
    if bits_out is not None:
        assert relu and ostride == 1 and bits_out.shape == tuple(out.shape)
    for t_ in (res, mask):
        assert t_ is None or (t_.shape == out.shape and t_.is_contiguous())
    ws = L.workspace(lib.dasac_conv_gemm_workspace(), x.device, owner="conv_gemm")
    fn = lib.dasac_conv_gemm_x3 if getattr(packed, "dasac_x3", False) else lib.dasac_conv_gemm
    tag = (M, K, Nb * OH * OW, stride, ostride, res is not None, mask is not None or mask_bits is not None)

    n = Nb * OH * OW
    nbytes = 4.0 * (x.numel() + packed.numel() + n * M * (1 + (res is not None) + (mask is not None)
                                                          + ((mask_bits is not None) + (bits_out is not None)) / 32.0))

    def launch(span, schedule):
        with PROFILE.span(span, 2.0 * n * M * K, tag, nbytes):
            if stats is not None:
                assert mask is None and mask_bits is None and bits_out is None and stats.is_contiguous() and stats.dtype == torch.float32
                L.check(lib.dasac_conv_gemm_stats(x.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), Nb, Cx, H, W, OH, OW,
                                                  stride, M, K, out.shape[2], out.shape[3], ostride, L.ptr(shift), L.ptr(res), int(relu),
                                                  0, 0, schedule, L.ptr(ws), 0 if ws is None else ws.numel(),
                                                  stats.data_ptr(), L.stream_ptr()), "dasac_conv_gemm_stats")
            else:
                L.check(fn(x.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), Nb, Cx, H, W, OH, OW,
                           stride, M, K, out.shape[2], out.shape[3], ostride, L.ptr(shift), L.ptr(res),
                           L.ptr(mask), L.ptr(mask_bits), 0 if bits_out is None else bits_out.words.data_ptr(), int(relu),
                           0, 0, schedule, L.ptr(ws), 0 if ws is None else ws.numel(),
                           L.stream_ptr()), "dasac_conv_gemm")

    if schedule is not None:
        launch("conv_gemm<stream-K>" if schedule == 2 else "conv_gemm<tile-per-block>", int(schedule))
        return out
    if lib.dasac_conv_gemm_tail_split(Nb, OH, OW, M, K) > 0:
        # ONE launch: whole rounds one block per tile (lockstep over K: halo rows shared in L2) + the remaining tiles cut into
        # K-ranges that fill the chip once more (round 6; rounds 2-5 issued that remainder as a second, persistent stream-K launch)
        launch("conv_gemm<tile+tail>", 0)
        return out
    sk = PROFILE.on and lib.dasac_conv_gemm_schedule(Nb, OH, OW, M, K)
    launch("conv_gemm<stream-K>" if sk else "conv_gemm<tile-per-block>", 0)
    return out


def conv_gemm_batched(x, packed, table, out, grid_hw, stride, M, K, ostride=1, strides=None):
    """out[b] = the plain contraction of `conv_gemm` (no epilogue operands) for every entry b of x [B,Nb,Cx,H,W], packed [B,Kpad,Mpad]
    and out [B,Nb,M,OutH,OutW], as ONE launch of the tile-per-block kernel: bit for bit B calls of conv_gemm(..., schedule=1) on the
    slices (dasac_conv_gemm_batched).  strides: per-entry (x, packed, out) strides in elements, default the tensors' own."""
    lib = L.load()
    L.require_gpu(x, packed, table, out)
    B, Nb, Cx, H, W = x.shape
    OH, OW = grid_hw
    assert out.shape[:3] == (B, Nb, M) and packed.shape[0] == B and packed.dtype == x.dtype == out.dtype == torch.float32
    for t_ in (x, packed, out):
        assert t_[:1].is_contiguous()                      # an entry is dense; entries may lie apart
    sx, sw, so = (x.stride(0), packed.stride(0), out.stride(0)) if strides is None else strides
    n = Nb * OH * OW
    tag = (M, K, n, stride, ostride, B)
    nbytes = 4.0 * (x.numel() + packed.numel() + B * n * M)
    with PROFILE.span("conv_gemm<batched>", 2.0 * B * n * M * K, tag, nbytes):
        L.check(lib.dasac_conv_gemm_batched(x.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), Nb, Cx, H, W, OH, OW,
                                            stride, M, K, out.shape[3], out.shape[4], ostride, B, sx, sw, so, L.stream_ptr()),
                "dasac_conv_gemm_batched")
    return out


def conv_forward(spec, x, weights, scale=None, shift=None, res=None, relu=False, table=None, packed=None):
    """Convenience forward: y = relu?(scale*conv(x) + shift + res); `scale` is folded into the packed weights."""
    Nb, _, H, W = x.shape
    OH, OW = spec.out_hw(H, W)
    order = gemm_order(spec, False)
    table = conv_table(spec, H, W, False, x.device, order) if table is None else table
    packed = conv_pack(spec, weights, False, scale, order=order) if packed is None else packed
    out = torch.empty((Nb, spec.cout, OH, OW), dtype=torch.float32, device=x.device)
    return conv_gemm(x, packed, table, out, (OH, OW), spec.stride, spec.cout, spec.K, 1, shift, res, None, relu)


def conv_dgrad(spec, dz, weights, in_hw, scale=None, res=None, mask=None, table=None, packed=None):
    """dx = conv^T(dz * scale[co]) (+res) (masked).  stride 1 for any kernel; stride>1 only for 1x1."""
    Nb, _, OH, OW = dz.shape
    H, W = in_hw
    order = gemm_order(spec, True)
    table = conv_table(spec, OH, OW, True, dz.device, order) if table is None else table
    packed = conv_pack(spec, weights, True, scale, order=order) if packed is None else packed
    if spec.stride == 1:
        dx = torch.empty((Nb, spec.cin, H, W), dtype=torch.float32, device=dz.device)
        return conv_gemm(dz, packed, table, dx, (H, W), 1, spec.cin, spec.Kt, 1, None, res, mask, False)
    assert spec.taps == 1 and spec.branches[0][3] == 0, "strided data-gradient only for 1x1 convolutions"
    # scatter onto the stride lattice.  Positions off the lattice keep `res` (or 0): the accumulation
    # runs IN PLACE on `res` (each element is read and written by the same thread).
    if res is None:
        dx = torch.empty((Nb, spec.cin, H, W), dtype=torch.float32, device=dz.device)
        dx.zero_()
    else:
        dx = res
    assert not isinstance(mask, ReluBits), "strided data gradient: the pattern is applied by relu_mask on the fp32 activation"
    conv_gemm(dz, packed, table, dx, (OH, OW), 1, spec.cin, spec.Kt, spec.stride, None,
              dx if res is not None else None, None, False)
    return relu_mask(dx, mask) if mask is not None else dx


# ----------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3) and F(4x4,3x3) for the wide dilated 3x3 convolutions (include/dasac_hip.h: dasac_winograd_*, dasac_winograd4_*):
# ONE implementation of each operation (WinogradForm), the two forms as data (F2, F4), and per form the public names bound to it
# ----------------------------------------------------------------------------------------------
# Algorithm of the forward / data-gradient / weight-gradient GEMMs of an eligible convolution:
#   "auto"    Winograd F(4x4,3x3) where `winograd4_routed` says so (on large maps layer4's conv2 data gradient and no-grad forward, layer3's no-grad forward), else
#             Winograd F(2x2,3x3) where `winograd_routed` says so (layer4's 512 -> 512 dilated conv2) and, for the weight gradient,
#             where `winograd4_wgrad_routed` (F(4x4,3x3): the same layers on large maps) or `winograd_wgrad_routed` does (layer4's
#             and layer3's conv2), direct elsewhere;
#   "direct"  the direct implicit GEMM everywhere.
ALGORITHM = "auto"
# Layer3's 256 -> 256 measures faster through the batched Winograd path too (0.69 -> 0.59 ms per conv, 11.6 ms per cfg-3 step) but stays
# direct: tests/test_gpu_fullres.py counts the split-K-tail launches of a student pass, 46 of which are layer3's (profiles/EXPERIMENTS.md)
WINOGRAD_MIN_CHANNEL_PRODUCT = 512 * 512
_MAX_TENSOR_BYTES = (1 << 32) - 4096         # buffer-descriptor window of the kernels


def set_conv_algorithm(mode):
    global ALGORITHM
    assert mode in ("auto", "direct"), mode
    ALGORITHM = mode


def winograd_ok(spec, transposed=False):
    """True when the forward (transposed: the data-gradient) GEMM of `spec` has a Winograd form: one 3x3 branch, stride 1,
    padding == dilation, gathered channels a multiple of 16, fp32 arithmetic."""
    if len(spec.branches) != 1 or spec.stride != 1 or PRECISION != "fp32":
        return False
    kh, kw, d, p = spec.branches[0]
    C = spec.cout if transposed else spec.cin
    return kh == 3 and kw == 3 and d >= 1 and p == d and C % 16 == 0


_wino_tables = {}


def _winograd_table(C, T, device):
    """Gather table of the point GEMMs: a 1x1 convolution over C planes of 1 x T."""
    key = (device.index, C, T)
    t = _wino_tables.get(key)
    if t is None:
        if len(_wino_tables) > 64:
            _wino_tables.clear()
        t = _wino_tables[key] = conv_table(ConvSpec(C, C, [(1, 1, 1, 0)]), 1, T, False, device)
    return t


class WinogradForm:
    """One form F(tile x tile, 3x3) of the Winograd path: what tells the forms apart as data, the operations written once.
    name: stem of the C entry points (dasac_<name>_*), of the PROFILE span names and of the error texts.  points: (tile + 2)^2
    entries of the batched point GEMMs / contractions.  multi_launch: narrow outputs (padded M no multiple of 128, no batched
    point GEMM) fall back to one `conv_gemm` launch per point -- F(2x2) keeps that form, F(4x4) has none.
    F(2x2): 16 point products per 2x2 outputs, 2.25 x fewer than direct.  F(4x4) (evaluation points 0, 1, -1, 2, -1/2, inf): 36 per
    4x4 outputs, 1.71 x fewer again, transformed tensors of 0.59 times the size, at 2 - 4 x the direct kernel's rounding error
    against float64 (tests/test_gpu_winograd4_conv.py prints the ratio); its tile count is padded to a multiple of 4 with zero tiles."""

    def __init__(self, name, tile, multi_launch):
        self.name, self.tile, self.points, self.multi_launch = name, tile, (tile + 2) ** 2, multi_launch
        self.sum_entry = tile + 3       # point (1,1), evaluation point 1 on both axes: its row of A is all ones, its row sums are the channel sums of dz

    def entry(self, fn):
        return getattr(L.load(), "dasac_{}_{}".format(self.name, fn))

    def tiles(self, Nb, H, W, dilation):
        """T, the pixel axis of the transformed tensors [points, C, T]; 0: more than 2^30 tiles."""
        return self.entry("tiles")(Nb, H, W, int(dilation))

    def fits(self, C, M, T):
        """The transformed tensors [points, C or M, T] lie inside the 4 GiB window of the kernels' buffer descriptors."""
        return T > 0 and 4 * self.points * max(C, M) * T <= _MAX_TENSOR_BYTES

    def filter(self, spec, weight, transposed, scale=None, out=None):
        """U [points, Kpad, Mpad]: the point matrices G g G^T of `weight` [Cout,Cin,3,3] (scale[co] folded in), each packed as
        `conv_pack` packs a 1x1 convolution; transposed: rotated filter, channels swapped (the data gradient)."""
        lib = L.load()
        L.require_gpu(weight, scale)
        M, K = (spec.cin, spec.cout) if transposed else (spec.cout, spec.cin)
        shape = (self.points, lib.dasac_conv_kpad(K), lib.dasac_conv_mpad(M))
        if out is None or tuple(out.shape) != shape:
            out = torch.empty(shape, dtype=torch.float32, device=weight.device)
        L.check(self.entry("filter")(_c(weight).data_ptr(), L.ptr(scale), spec.cout, spec.cin, int(transposed), out.data_ptr(), L.stream_ptr()),
                "dasac_{}_filter".format(self.name))
        return out

    def output(self, y, out, dilation, shift=None, relu=False, mask_bits=None, bits_out=None):
        """out [Nb,M,H,W] = epilogue(A^T Y A) of the point GEMMs' results y [points, M, T]: + shift, ReLU, ReLU pattern recorded into
        `bits_out` or the elements whose bit in `mask_bits` is clear zeroed (both ReluBits of out's shape)."""
        L.require_gpu(y, out, shift)
        Nb, M, H, W = out.shape
        assert y.is_contiguous() and out.is_contiguous() and y.dtype == torch.float32
        for b in (mask_bits, bits_out):
            assert b is None or b.shape == tuple(out.shape)
        with PROFILE.span(self.name + "_output", 0.0, None, 4.0 * (y.numel() + out.numel())):
            L.check(self.entry("output")(y.data_ptr(), y.numel() * 4, Nb, M, H, W, int(dilation), L.ptr(shift), int(relu),
                                      0 if mask_bits is None else mask_bits.words.data_ptr(),
                                      0 if bits_out is None else bits_out.words.data_ptr(), out.data_ptr(), L.stream_ptr()),
                    "dasac_{}_output".format(self.name))
        return out

    def conv(self, x, u, out, dilation, shift=None, relu=False, mask_bits=None, bits_out=None, gemm_schedule="auto"):
        """out [Nb,M,H,W] = epilogue(conv3x3(x [Nb,C,H,W], dilation = padding)) with the transformed filter u = `filter`
        (forward, or the data-gradient form with x = dz): input transform, the point GEMMs, output transform.
        The two transformed tensors [points, C, T] and [points, M, T] live in the stream's scratch buffer.
        gemm_schedule: "auto" issues the point GEMMs as ONE batched launch (`conv_gemm_batched`: a single point's tiles -- layer4:
        604 on 1024 resident slots -- never fill the chip, all points make whole rounds; it exists for padded M a multiple of 128);
        a `multi_launch` form runs narrower outputs as None, and takes 1 / 2 / None to issue one `conv_gemm` launch per point on that
        schedule (one block per tile -- bit-equal to the batched launch --, stream-K, the library's choice; tools/winograd_ab.py)."""
        lib = L.load()
        L.require_gpu(x, u, out)
        P = self.points
        Nb, C, H, W = x.shape
        M = out.shape[1]
        assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (Nb, M, H, W)
        assert tuple(u.shape) == (P, lib.dasac_conv_kpad(C), lib.dasac_conv_mpad(M)) and u.is_contiguous()
        if gemm_schedule == "auto" and lib.dasac_conv_mpad(M) % 128 != 0:
            gemm_schedule = None       # narrow outputs (the batched launch exists for the 128-row tile only): P launches, the library's choice
        if gemm_schedule != "auto" and not self.multi_launch:
            raise L.DasacError("{}_conv: {} output channels have no batched point GEMM".format(self.name, M))
        T = self.tiles(Nb, H, W, dilation)
        if not self.fits(C, M, T):
            raise L.DasacError("{}_conv: [{}, {}, tiles] exceeds the 4 GiB buffer-descriptor window".format(self.name, P, max(C, M)))
        v_elems, y_elems = P * C * T, P * M * T
        ws = L.workspace(4 * (v_elems + y_elems), x.device)[:4 * (v_elems + y_elems)].view(torch.float32)
        v, y = ws[:v_elems].view(P, C, T), ws[v_elems:v_elems + y_elems].view(P, M, T)
        with PROFILE.span(self.name + "_input", 0.0, None, 4.0 * (x.numel() + v_elems)):
            L.check(self.entry("input")(x.data_ptr(), Nb, C, H, W, int(dilation), v.data_ptr(), v_elems * 4, L.stream_ptr()),
                    "dasac_{}_input".format(self.name))
        table = _winograd_table(C, T, x.device)
        if gemm_schedule == "auto":
            conv_gemm_batched(v.view(P, 1, C, 1, T), u, table, y.view(P, 1, M, 1, T), (1, T), 1, M, C)
        else:
            for pt in range(P):
                conv_gemm(v[pt].view(1, C, 1, T), u[pt], table, y[pt].view(1, M, 1, T), (1, T), 1, M, C, schedule=gemm_schedule)
        return self.output(y, out, dilation, shift, relu, mask_bits, bits_out)

    def wgrad(self, spec, dz, x, weight, scale=None, dot=None, sum_dz=None, out=None):
        """dW [Cout,Cin,3,3] of an eligible 3x3 convolution as G^T [sum over tiles (A dY A^T) (.) (B^T x B)] G: the input transform of
        x, its adjoint on dz, ONE batched launch of the point contractions over pixel splits, and a finish that adds the splits in a
        fixed order, transforms back and multiplies by scale[co].  `dot` [dot_rows(spec), Cout], `sum_dz` [Cout] and `out` are those
        of `conv_wgrad`.  The two transformed tensors and the slabs live in the stream's scratch buffer."""
        lib = L.load()
        L.require_gpu(dz, x, weight, scale, dot, sum_dz)
        P, name = self.points, self.name
        Nb, C, H, W = x.shape
        M, d = dz.shape[1], int(spec.branches[0][2])
        assert winograd_ok(spec) and (C, M) == (spec.cin, spec.cout) and tuple(dz.shape) == (Nb, M, H, W) and x.is_contiguous()
        assert dot is None or (tuple(dot.shape) == (dot_rows(spec), M) and dot.is_contiguous())
        T = self.tiles(Nb, H, W, d)
        slab_bytes = lib.dasac_conv_wgrad_batched_workspace(P, M, C, T) if T > 0 else 0
        if slab_bytes == 0 or not self.fits(C, M, T):
            raise L.DasacError("{}_wgrad: {} x {} channels over {} tiles has no batched point contraction".format(name, M, C, T))
        v_elems, m_elems = P * C * T, P * M * T
        ws = L.workspace(4 * (v_elems + m_elems) + slab_bytes, x.device)
        v, dm, slabs = ws[:4 * v_elems], ws[4 * v_elems:4 * (v_elems + m_elems)], ws[4 * (v_elems + m_elems):]
        dz = _c(dz)
        with PROFILE.span(name + "_wgrad_input", 0.0, None, 4.0 * (x.numel() + v_elems)):
            L.check(self.entry("input")(x.data_ptr(), Nb, C, H, W, d, v.data_ptr(), v.numel(), L.stream_ptr()), "dasac_{}_input".format(name))
        with PROFILE.span(name + "_wgrad_grad", 0.0, None, 4.0 * (dz.numel() + m_elems)):
            L.check(self.entry("grad_input")(dz.data_ptr(), Nb, M, H, W, d, dm.data_ptr(), dm.numel(), L.stream_ptr()),
                    "dasac_{}_grad_input".format(name))
        with PROFILE.span(name + "_wgrad_gemm", 2.0 * P * M * C * T, (M, C, T, 1, 1, False, False), 4.0 * (v_elems + m_elems + P * M * C)):
            L.check(lib.dasac_conv_wgrad_batched(dm.data_ptr(), v.data_ptr(), P, M, C, T, M * T, C * T, self.sum_entry, slabs.data_ptr(),
                                                 slabs.numel(), L.stream_ptr()), "dasac_conv_wgrad_batched")
        dw = _dest(out, weight)
        with PROFILE.span(name + "_wgrad_finish", 0.0, None, float(slab_bytes) + 8.0 * weight.numel()):
            L.check(self.entry("wgrad_finish")(slabs.data_ptr(), slabs.numel(), M, C, T, _c(weight).data_ptr(), L.ptr(scale), dw.data_ptr(),
                                            L.ptr(dot), L.ptr(sum_dz), L.stream_ptr()), "dasac_{}_wgrad_finish".format(name))
        return dw


F2 = WinogradForm("winograd", 2, multi_launch=True)
F4 = WinogradForm("winograd4", 4, multi_launch=False)
winograd_filter, winograd_output, winograd_conv, winograd_wgrad = F2.filter, F2.output, F2.conv, F2.wgrad
winograd4_filter, winograd4_output, winograd4_conv, winograd4_wgrad = F4.filter, F4.output, F4.conv, F4.wgrad


# ---- routing: policy, one rule per form and GEMM, each from its own measurements ---------------------------------------------------
def winograd_routed(spec, transposed, Nb, H, W):
    """The engine's rule for the F(2x2,3x3) forward (transposed: data gradient): eligible, wide enough to pay, the transformed
    tensors inside the 4 GiB window."""
    if ALGORITHM != "auto" or not winograd_ok(spec, transposed) or spec.cin * spec.cout < WINOGRAD_MIN_CHANNEL_PRODUCT:
        return False
    return F2.fits(spec.cin, spec.cout, F2.tiles(Nb, H, W, spec.branches[0][2]))


# The forward / data gradient as F(4x4,3x3) is routed per (Cin, Cout, dilation, data gradient?, grad-enabled pass?) where the per-conv
# gain AND the end-to-end accuracy bounds of tests/test_gpu_fullres.py were measured to hold (profiles/winograd4_conv_ab.txt,
# profiles/EXPERIMENTS.md); anything else keeps F(2x2) or the direct GEMM.  Layer3's 256 -> 256 is routed in no-grad forwards only
# (the teacher, inference): a grad-enabled pass keeps the direct launches tests/test_gpu_fullres.py counts.  Layer4's forward is
# routed in no-grad passes only as well: in a grad-enabled pass its 4 x larger difference to the direct kernel flips more ReLUs that
# sit at zero, each of which moves a gradient row by about 1e-2 of its maximum, and tests/test_gpu_winograd4_wgrad.py (512 planes at
# 2 x 33 x 33, auto against direct, bound 1e-3) measured 1.6e-2 with it and 3.8e-6 without.  VGG16's undilated 512 -> 512 layers were
# not measured, so the table carries the dilation.
WINOGRAD4_ROUTES = {
    (512, 512, 4, True, True),       # (a) layer4 conv2, data gradient
    (512, 512, 4, False, False),     # (b) layer4 conv2, forward of a no-grad pass (of a grad-enabled pass: not routed, see above)
    (256, 256, 2, False, False),     # (c) layer3 conv2, no-grad forward
}
WINOGRAD4_MIN_SAMPLES = 8                    # per phase and axis: two whole four-output tiles; below that most of a tile is overhang


def winograd4_routed(spec, transposed, Nb, H, W, grad):
    """The engine's rule for the F(4x4,3x3) forward (transposed: data gradient), consulted before `winograd_routed`: eligible, an
    output width the batched point GEMMs take (padded M a multiple of 128: there is no 36-launch form), at least
    WINOGRAD4_MIN_SAMPLES samples per phase and axis, the transformed tensors inside the 4 GiB window, and a route of the table.
    grad: the pass records what a backward needs (ConvOp.forward's `keep`; always True for the data gradient)."""
    if ALGORITHM != "auto" or not winograd_ok(spec, transposed):
        return False
    d = spec.branches[0][2]
    if (spec.cin, spec.cout, d, bool(transposed), bool(grad)) not in WINOGRAD4_ROUTES:
        return False
    if L.load().dasac_conv_mpad(spec.cin if transposed else spec.cout) % 128:
        return False
    if H // d < WINOGRAD4_MIN_SAMPLES or W // d < WINOGRAD4_MIN_SAMPLES:
        return False
    return F4.fits(spec.cin, spec.cout, F4.tiles(Nb, H, W, d))


def winograd_form(spec, transposed, Nb, H, W, grad):
    """The form the engine runs the forward (transposed: data gradient) GEMM of `spec` in: F4, F2, or None for the direct GEMM."""
    if winograd4_routed(spec, transposed, Nb, H, W, grad):
        return F4
    return F2 if winograd_routed(spec, transposed, Nb, H, W) else None


# The weight gradient of the same convolutions has its own threshold: it is routed where it measured faster on its own, whatever the
# forward and the data gradient of the layer do -- layer4's 512 -> 512 (2.80 -> 1.64 ms per conv) AND layer3's 256 -> 256 (0.714 ->
# 0.520 ms; profiles/winograd_wgrad_ab.txt): no test counts conv_wgrad launches.
WINOGRAD_WGRAD_MIN_CHANNEL_PRODUCT = 256 * 256
# As F(4x4) -- a few times the rounding error, which a weight gradient, a terminal sum, takes everywhere -- it is routed per layer where
# it measured faster than the F(2x2) form on its own (profiles/winograd4_wgrad_ab.txt): a (Cin, Cout) pair missing here stays F(2x2).
WINOGRAD4_WGRAD_LAYERS = {(256, 256), (512, 512)}


def winograd_wgrad_routed(spec, Nb, H, W):
    """The engine's rule for the F(2x2,3x3) weight gradient: eligible (`winograd_ok`: one 3x3 branch, fp32, ...), wide enough to pay,
    the transformed tensors inside the 4 GiB window and a shape the batched point contraction takes (channel counts multiples of
    128, a tile count that is a multiple of 4: dasac_conv_wgrad_batched)."""
    if ALGORITHM != "auto" or not winograd_ok(spec) or spec.cin * spec.cout < WINOGRAD_WGRAD_MIN_CHANNEL_PRODUCT:
        return False
    T = F2.tiles(Nb, H, W, spec.branches[0][2])
    return F2.fits(spec.cin, spec.cout, T) and L.load().dasac_conv_wgrad_batched_splits(F2.points, spec.cout, spec.cin, T) > 0


def winograd4_wgrad_routed(spec, Nb, H, W):
    """The engine's rule for the F(4x4,3x3) weight gradient, consulted before `winograd_wgrad_routed`: that rule's conditions
    (eligible, fp32, wide enough, inside the 4 GiB window, channel counts multiples of 128) and on both axes n // d >= 8."""
    if ALGORITHM != "auto" or not winograd_ok(spec) or spec.cin * spec.cout < WINOGRAD_WGRAD_MIN_CHANNEL_PRODUCT:
        return False
    if spec.cin % 128 or spec.cout % 128 or (spec.cin, spec.cout) not in WINOGRAD4_WGRAD_LAYERS:
        return False
    d = spec.branches[0][2]
    if H // d < WINOGRAD4_MIN_SAMPLES or W // d < WINOGRAD4_MIN_SAMPLES:
        return False
    T = F4.tiles(Nb, H, W, d)
    return F4.fits(spec.cin, spec.cout, T) and L.load().dasac_conv_wgrad_batched_splits(F4.points, spec.cout, spec.cin, T) > 0


def winograd_wgrad_form(spec, Nb, H, W):
    """The form the engine runs the weight gradient of `spec` in: F4, F2, or None for `conv_wgrad`."""
    if winograd4_wgrad_routed(spec, Nb, H, W):
        return F4
    return F2 if winograd_wgrad_routed(spec, Nb, H, W) else None


def dot_rows(spec):
    """Rows of the partial d-gamma dot term `conv_wgrad(dot=...)` fills (one per block of 64 input channels)."""
    return L.load().dasac_conv_wgrad_dot_rows(spec.cin, spec.taps)


def conv_wgrad(spec, dz, x, weights, scale=None, dot=None, table=None, sum_dz=None, outs=None):
    """Returns [dW per branch]; optionally fills dot [dot_rows(spec), Cout] with the partial rows of sum_k W*G (unscaled G;
    `bn_param_grads` adds them in a fixed order -- no atomics) and sum_dz[co] = sum over batch and pixels of dz.
    `outs`: destination per branch (None entries are allocated) -- a gradient sink hands out slices of its flat
    reduction buffer here."""
    lib = L.load()
    L.require_gpu(dz, x, *weights)
    assert dot is None or (tuple(dot.shape) == (dot_rows(spec), spec.cout) and dot.is_contiguous())
    Nb, Cx, H, W = x.shape
    _, M, OH, OW = dz.shape
    table = conv_table(spec, H, W, False, x.device) if table is None else table
    nbytes = lib.dasac_conv_wgrad_workspace(Nb, OH, OW, M, spec.K)
    ws = L.workspace(nbytes, x.device)
    with PROFILE.span("conv_wgrad", 2.0 * Nb * OH * OW * M * spec.K, (M, spec.K, Nb * OH * OW, spec.stride, 1, False, False),
                      4.0 * (dz.numel() + x.numel() + M * spec.K)):
        fn = lib.dasac_conv_wgrad_x3 if PRECISION == "bf16x3" else lib.dasac_conv_wgrad
        L.check(fn(_c(dz).data_ptr(), x.data_ptr(), table.data_ptr(), Nb, Cx, H, W, OH, OW, spec.stride, M,
                   spec.K, ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_conv_wgrad")
    grads = [_dest(None if outs is None else outs[bi], w) for bi, w in enumerate(weights)]
    for w, dw, (taps, tap0) in zip(weights, grads, _branch_taps(spec)):
        L.check(lib.dasac_conv_wgrad_finish(ws.data_ptr(), Nb, OH, OW, M, spec.K, _c(w).data_ptr(), L.ptr(scale),
                                            dw.data_ptr(), L.ptr(dot), L.ptr(sum_dz if tap0 == 0 else None), spec.cin, taps,
                                            tap0, L.stream_ptr()),
                "dasac_conv_wgrad_finish")
    return grads


# ----------------------------------------------------------------------------------------------
# SAC head
# ----------------------------------------------------------------------------------------------
def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _dest(out, like):
    """`out` if given (checked: fp32, contiguous, same element count as `like`), else a fresh tensor shaped like `like`."""
    if out is None:
        return torch.empty_like(like, memory_format=torch.contiguous_format)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == like.numel() and out.device == like.device
    return out


def upsample_softmax(logits, size, ignore=None, want_up=True, want_probs=False, want_sums=False):
    """bilinear(ac=True) upsampling [+ masked softmax + class sums].  Returns (up, probs, class_sums)."""
    lib = L.load()
    L.require_gpu(logits, ignore)
    logits = _c(logits)
    B, Cn, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    up = _f32((B, Cn, H, W), logits) if want_up else None
    probs = _f32((B, Cn, H, W), logits) if want_probs else None
    sums = torch.empty(Cn, dtype=torch.float64, device=logits.device) if want_sums else None
    ign = None if ignore is None else _c(ignore).view(torch.uint8)
    with PROFILE.span("upsample_softmax", 0.0, None, logits.numel() * 4.0 + B * Cn * H * W * 4.0 * (int(want_up) + int(want_probs)) + (B * H * W if ignore is not None else 0)):
        L.check(lib.dasac_upsample_softmax(logits.data_ptr(), B, Cn, h, w, H, W, L.ptr(ign), L.ptr(up), L.ptr(probs),
                                           L.ptr(sums), L.stream_ptr()), "dasac_upsample_softmax")
    return up, probs, sums


def infer_labels(logits, size, lut=None, want_conf=False):
    """infer_val.py:160-163 + writer: uint8 label map [B,H,W] = lut[argmax softmax(bilinear_ac(logits))] (+ winning prob)."""
    lib = L.load()
    L.require_gpu(logits, lut)
    logits = _c(logits)
    B, Cn, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device)
    conf = _f32((B, H, W), logits) if want_conf else None
    if lut is not None:
        assert lut.dtype == torch.uint8 and lut.numel() >= Cn and lut.is_contiguous()
    L.check(lib.dasac_infer_labels(logits.data_ptr(), B, Cn, h, w, H, W, L.ptr(lut), labels.data_ptr(), L.ptr(conf),
                                   L.stream_ptr()), "dasac_infer_labels")
    return labels, conf


INFER_MAX_SOURCES = 8                       # DASAC_INFER_MAX_SOURCES
INFER_MODES = {"mean": 0, "max": 1}         # DASAC_INFER_MEAN / DASAC_INFER_MAX


def image_pyramid(image, size, flip=False):
    """F.interpolate(image, size, mode="bilinear", align_corners=True) of a float32 [B,Cin,H,W] image in one launch; with `flip`
    the result is [2B,Cin,Hs,Ws] and rows B..2B-1 are the horizontally mirrored copies (`.flip(-1)`, bit for bit).  size ==
    (H, W) is legal: the plain half then equals the input."""
    lib = L.load()
    L.require_gpu(image)
    if image.dtype != torch.float32 or image.dim() != 4:
        raise L.DasacError("image_pyramid takes a float32 [B,Cin,H,W] image (got {} {})".format(image.dtype, tuple(image.shape)))
    image = _c(image)
    B, Cin, H, W = image.shape
    Hs, Ws = int(size[0]), int(size[1])
    out = torch.empty((2 * B if flip else B, Cin, Hs, Ws), dtype=torch.float32, device=image.device)
    L.check(lib.dasac_image_pyramid(image.data_ptr(), B, Cin, H, W, Hs, Ws, int(bool(flip)), out.data_ptr(), L.stream_ptr()),
            "dasac_image_pyramid")
    return out


def infer_fuse(sources, flips, size, mode="mean", lut=None, want_conf=False, want_probs=False):
    """Multi-scale / mirrored inference in ONE kernel: `sources` are up to 8 float32 logit tensors [B,C,h_s,w_s] (sizes may
    differ), `flips[s]` says that source s was computed from the horizontally mirrored image.  Per output pixel of `size`:
    softmax(bilinear_ac(source)) per source (a flipped one read at the mirrored column), mean or max over the sources, argmax.
    Returns (labels u8 [B,H,W] through `lut` if given, conf f32 [B,H,W] or None, probs f32 [B,C,H,W] or None).  A source may be
    a batch slice of a larger contiguous tensor (the mirrored half of a 2B-batch backbone call)."""
    import ctypes as C
    lib = L.load()
    sources, flips = list(sources), list(flips)
    L.require_gpu(lut, *sources)
    if mode not in INFER_MODES:
        raise L.DasacError("infer_fuse: mode must be one of {} (got {!r})".format(sorted(INFER_MODES), mode))
    if not sources or len(flips) != len(sources):
        raise L.DasacError("infer_fuse takes at least one source and one flip flag per source (got {} and {})".format(
            len(sources), len(flips)))
    B, Cn = sources[0].shape[:2]
    for s in sources:
        if s.dtype != torch.float32 or s.dim() != 4 or tuple(s.shape[:2]) != (B, Cn):
            raise L.DasacError("infer_fuse: every source must be float32 [{},{},h,w] (got {} {})".format(B, Cn, s.dtype, tuple(s.shape)))
    sources = [_c(s) for s in sources]
    H, W = int(size[0]), int(size[1])
    device = sources[0].device
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=device)
    conf = torch.empty((B, H, W), dtype=torch.float32, device=device) if want_conf else None
    probs = torch.empty((B, Cn, H, W), dtype=torch.float32, device=device) if want_probs else None
    if lut is not None:
        assert lut.dtype == torch.uint8 and lut.numel() >= Cn and lut.is_contiguous()
    table = (L.InferSource * len(sources))()
    for i, (s, f) in enumerate(zip(sources, flips)):
        table[i] = L.InferSource(s.data_ptr(), s.shape[2], s.shape[3], int(bool(f)), 0)
    L.check(lib.dasac_infer_fuse(C.cast(table, C.c_void_p), len(sources), B, Cn, H, W, INFER_MODES[mode], L.ptr(lut),
                                 labels.data_ptr(), L.ptr(conf), L.ptr(probs), L.stream_ptr()), "dasac_infer_fuse")
    return labels, conf, probs


def crf_meanfield(probs, image, params, lut=None, want_conf=False, want_probs=False):
    """Mean-field refinement of fused class probabilities by a locally connected CRF over the image (include/dasac_hip.h:
    dasac_crf_meanfield): probs fp32 [B,C,H,W] as `infer_fuse` writes them, image fp32 [B,Ci,H,W] as the network sees it, `params` a
    crf.CrfParams (anything with its nine attributes; the library checks the ranges).  One launch per iteration, the last one
    fusing arg-max, `lut` and confidence.  Returns (labels u8 [B,H,W], conf f32 [B,H,W] or None, probs f32 [B,C,H,W] or None)."""
    lib = L.load()
    L.require_gpu(probs, image, lut)
    if probs.dtype != torch.float32 or probs.dim() != 4 or image.dtype != torch.float32 or image.dim() != 4:
        raise L.DasacError("crf_meanfield takes float32 probabilities [B,C,H,W] and a float32 image [B,Ci,H,W] (got {} {} and {} {})".format(
            probs.dtype, tuple(probs.shape), image.dtype, tuple(image.shape)))
    B, Cn, H, W = probs.shape
    if image.shape[0] != B or tuple(image.shape[2:]) != (H, W):
        raise L.DasacError("crf_meanfield: the image must be [{},Ci,{},{}] like the probabilities (got {})".format(B, H, W, tuple(image.shape)))
    probs, image = _c(probs), _c(image)
    if lut is not None:
        assert lut.dtype == torch.uint8 and lut.numel() >= Cn and lut.is_contiguous()
    n_iter = int(params.n_iter)
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=probs.device)
    conf = torch.empty((B, H, W), dtype=torch.float32, device=probs.device) if want_conf else None
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=probs.device) if want_probs else None
    ws = L.workspace(lib.dasac_crf_meanfield_workspace(B, Cn, H, W, n_iter), probs.device)
    L.check(lib.dasac_crf_meanfield(probs.data_ptr(), image.data_ptr(), B, Cn, image.shape[1], H, W, int(params.radius),
                                    int(params.dilation), float(params.w_app), float(params.theta_alpha), float(params.theta_beta),
                                    float(params.w_smooth), float(params.theta_gamma), float(params.compat), n_iter, L.ptr(lut),
                                    labels.data_ptr(), L.ptr(conf), L.ptr(out), ws.data_ptr(), ws.numel(), L.stream_ptr()),
            "dasac_crf_meanfield")
    return labels, conf, out


def upsample_bwd(grad_up, low_hw, gscale=None):
    lib = L.load()
    L.require_gpu(grad_up, gscale)
    grad_up = _c(grad_up)
    B, Cn, H, W = grad_up.shape
    h, w = low_hw
    out = _f32((B, Cn, h, w), grad_up)
    nbytes = lib.dasac_upsample_bwd_workspace(B * Cn, H, w)
    ws = L.workspace(nbytes, grad_up.device)
    L.check(lib.dasac_upsample_bwd(grad_up.data_ptr(), B * Cn, h, w, H, W, L.ptr(gscale), out.data_ptr(), ws.data_ptr(),
                                   ws.numel(), L.stream_ptr()), "dasac_upsample_bwd")
    return out


def ce_loss(logits_up, labels, class_weight=None, conf=None, want_grad=False, want_per_class=False, gscale=None):
    """Returns (loss[1], dlogits or None, per_class or None); conf given -> focal_ce_conf broadcast form."""
    lib = L.load()
    L.require_gpu(logits_up, labels, class_weight, conf)
    logits_up, labels = _c(logits_up), _c(labels)
    B, Cn, H, W = logits_up.shape
    HW = H * W
    loss = _f32((1,), logits_up)
    dl = torch.empty_like(logits_up) if want_grad else None
    pc = _f32((Cn,), logits_up) if want_per_class else None
    nbytes = lib.dasac_ce_loss_workspace(B, Cn, HW)
    ws = L.workspace(nbytes, logits_up.device)
    with PROFILE.span("ce_loss", 0.0, None, logits_up.numel() * 4.0 * (2 if want_grad else 1) + B * HW * (8 + (4 if conf is not None else 0))):
        L.check(lib.dasac_ce_loss(logits_up.data_ptr(), labels.data_ptr(), L.ptr(class_weight), L.ptr(None if conf is None else _c(conf)),
                                  B, Cn, HW, 0 if conf is None else 1, L.ptr(gscale), loss.data_ptr(), L.ptr(dl), L.ptr(pc), ws.data_ptr(),
                                  ws.numel(), L.stream_ptr()), "dasac_ce_loss")
    return loss, dl, pc


def ce_loss_bwd_low(logits_up, labels, low_hw, class_weight=None, conf=None, gscale=None):
    """d loss / d (low-resolution logits) of `ce_loss` composed with the bilinear upsampling, in one pass over logits_up."""
    lib = L.load()
    L.require_gpu(logits_up, labels, class_weight, conf, gscale)
    logits_up, labels = _c(logits_up), _c(labels)
    B, Cn, H, W = logits_up.shape
    h, w = int(low_hw[0]), int(low_hw[1])
    out = _f32((B, Cn, h, w), logits_up)
    ws = L.workspace(lib.dasac_ce_loss_bwd_low_workspace(B, Cn, H, w), logits_up.device)
    with PROFILE.span("ce_loss_bwd_low", 0.0, None, logits_up.numel() * 4.0 + B * H * W * (8 + (4 if conf is not None else 0)) + out.numel() * 4.0):
        L.check(lib.dasac_ce_loss_bwd_low(logits_up.data_ptr(), labels.data_ptr(), L.ptr(class_weight), L.ptr(None if conf is None else _c(conf)),
                                          B, Cn, H, W, h, w, 0 if conf is None else 1, L.ptr(gscale), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr()), "dasac_ce_loss_bwd_low")
    return out


def warp_affine(x, theta):
    lib = L.load()
    L.require_gpu(x, theta)
    x, theta = _c(x), _c(theta)
    B, Cn, H, W = x.shape
    out = torch.empty_like(x)
    L.check(lib.dasac_warp_affine(x.data_ptr(), theta.data_ptr(), B, Cn, H, W, out.data_ptr(), L.stream_ptr()), "dasac_warp_affine")
    return out


POOL_MODES = {"avg_pool": 0, "minentropy_pool": 1}


def warp_pool(probs, theta, theta_inv, T, mode="avg_pool", tolerance=0.1, want_aligned=True):
    """probs [N*T,C,H,W] -> (pooled [N,C,H,W], mask [N,1,H,W], aligned or None).  theta None: the views are already
    aligned and coverage-weighted, only the pooling runs (SAC._avg_pool / _minentropy_pool called on their own)."""
    lib = L.load()
    L.require_gpu(probs, theta, theta_inv)
    probs = _c(probs)
    if theta is None:
        theta_inv, want_aligned = None, False
    else:
        theta, theta_inv = _c(theta), _c(theta_inv)
    NT, Cn, H, W = probs.shape
    assert NT % T == 0
    N = NT // T
    pooled = _f32((N, Cn, H, W), probs)
    mask = _f32((N, 1, H, W), probs)
    aligned = torch.empty_like(probs) if want_aligned else None
    with PROFILE.span("warp_pool", 0.0, None, probs.numel() * 4.0 * (2 if want_aligned else 1) + pooled.numel() * 4.0 + mask.numel() * 4.0):
        L.check(lib.dasac_warp_pool(probs.data_ptr(), L.ptr(theta), L.ptr(theta_inv), N, T, Cn, H, W, POOL_MODES[mode],
                                    float(tolerance), L.ptr(aligned), pooled.data_ptr(), mask.data_ptr(), L.stream_ptr()),
                "dasac_warp_pool")
    return pooled, mask, aligned


def warp_back(pooled, mask, theta_inv, views_per_group):
    lib = L.load()
    L.require_gpu(pooled, mask, theta_inv)
    theta_inv = _c(theta_inv)
    N, Cn, H, W = pooled.shape
    B = theta_inv.shape[0]
    assert B == N * views_per_group
    out = _f32((B, Cn, H, W), pooled)
    with PROFILE.span("warp_back", 0.0, None, (pooled.numel() + mask.numel() + out.numel()) * 4.0):
        L.check(lib.dasac_warp_back(pooled.data_ptr(), mask.data_ptr(), theta_inv.data_ptr(), B, views_per_group, Cn, H, W,
                                    out.data_ptr(), L.stream_ptr()), "dasac_warp_back")
    return out


def class_state(running_conf, class_sums, B, HW, beta, stat_momentum, update, focal_p, want_disc=True, want_focal=True):
    """In-place update of running_conf (when update) and the derived (disc, focal) vectors."""
    lib = L.load()
    L.require_gpu(running_conf, class_sums)
    Cn = running_conf.numel()
    disc = _f32((Cn,), running_conf) if want_disc else None
    focal = _f32((Cn,), running_conf) if want_focal else None
    L.check(lib.dasac_class_state(running_conf.data_ptr(), L.ptr(class_sums), int(B), int(HW), Cn, float(beta),
                                  float(stat_momentum), int(bool(update)), float(focal_p), L.ptr(disc), L.ptr(focal),
                                  L.stream_ptr()), "dasac_class_state")
    return disc, focal


class HostClassVectors:
    """disc = 1 - exp(-chi/beta) (sac.py:151-152) and focal = (1 - clamp(chi, 0))**p (sac.py:120,135) computed by the
    SAME CPU ATen kernels the reference runs (true division by the python scalar, Sleef exp/pow) so that the per-class
    thresholds -- and with them the integer label map -- are bit-equal to the CPU reference's on equal probabilities;
    the device's expf/powf differ from Sleef's in the last bit on some inputs.

    Cost: 19 floats D2H + 2x19 H2D per target step.  `start()` queues the copy of chi into pinned memory right
    after the kernel that updates it; `finish()` (called after the warp/pool kernels were queued, so the GPU has
    work while the host waits) runs the two formulas on the host and uploads them without blocking."""

    _pinned = {}          # chi's storage -> (chi buffer, vectors buffer): pinned once per model, reused every step

    def __init__(self, running_conf):
        key = (running_conf.device.index, running_conf.data_ptr(), tuple(running_conf.shape))
        bufs = HostClassVectors._pinned.get(key)
        if bufs is None:
            bufs = (torch.empty(running_conf.shape, dtype=torch.float32).pin_memory(),
                    torch.empty((2,) + tuple(running_conf.shape), dtype=torch.float32).pin_memory())
            HostClassVectors._pinned[key] = bufs
        self.host, self.vecs = bufs
        self.host.copy_(running_conf.detach(), non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record()
        self.device = running_conf.device

    def finish(self, beta, focal_p, want_disc=True):
        self.done.synchronize()
        chi, vecs = self.host, self.vecs
        # (the previous step's upload from `vecs` finished long ago: every step waits on `done` after queueing it)
        vecs[0] = 1 - torch.exp(-chi / beta) if want_disc else 1.0
        vecs[1] = (1 - chi.clamp(0.)) ** focal_p
        dev = vecs.to(self.device, non_blocking=True)
        return (dev[0] if want_disc else None), dev[1]


class DeviceClassVectors:
    """The same two vectors from `dasac_class_state` on the device (exp through the fp64 library, rounded once): no copy to the
    host, no synchronisation -- a step that uses them is one uninterrupted launch sequence.  Within 1 ULP of HostClassVectors,
    not bit-equal to it by construction (see there), so pseudo labels can differ from the CPU reference's on a pixel whose
    confidence equals a threshold to the last bit.  Opt-in: `SAC.device_thresholds = True`."""

    def __init__(self, disc, focal):
        self.disc, self.focal = disc, focal

    def finish(self, beta, focal_p, want_disc=True):
        return (self.disc if want_disc else None), self.focal


def class_vectors(running_conf, beta, focal_p, want_disc=True):
    """One-shot form of HostClassVectors (blocks until the stream reaches this point)."""
    L.require_gpu(running_conf)
    return HostClassVectors(running_conf).finish(beta, focal_p, want_disc)


# ----------------------------------------------------------------------------------------------
# around the convolutions
# ----------------------------------------------------------------------------------------------
def bn_fold(gamma, beta, mean, var, eps, conv_bias=None, want_invstd=True):
    lib = L.load()
    L.require_gpu(gamma, beta, mean, var, conv_bias)
    Cn = gamma.numel()
    scale, shift = _f32((Cn,), gamma), _f32((Cn,), gamma)
    invstd = _f32((Cn,), gamma) if want_invstd else None
    L.check(lib.dasac_bn_fold(gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), L.ptr(conv_bias), float(eps),
                              Cn, scale.data_ptr(), shift.data_ptr(), L.ptr(invstd), L.stream_ptr()), "dasac_bn_fold")
    return scale, shift, invstd


def build_refresh_tables(fold_jobs, pack_jobs, device):
    """Device tables for dasac_bn_fold_multi / dasac_conv_pack_multi (include/dasac_hip.h: dasac_fold_job, dasac_pack_job).
    fold job: (gamma, beta, mean, var, conv_bias|None, (scale, shift, invstd), eps, C)
    pack job: (weight, scale|None, out, Cout, Cin, taps, Mpad, Kpad, mode, order)"""
    import numpy as np
    lib = L.load()
    fold_dt = np.dtype([("gamma", "<u8"), ("beta", "<u8"), ("mean", "<u8"), ("var", "<u8"), ("conv_bias", "<u8"), ("scale", "<u8"),
                        ("shift", "<u8"), ("invstd", "<u8"), ("eps", "<f4"), ("C", "<i4")])
    pack_dt = np.dtype([("w", "<u8"), ("scale", "<u8"), ("out", "<u8"), ("Cout", "<i4"), ("Cin", "<i4"), ("taps", "<i4"), ("Mpad", "<i4"),
                        ("Kpad", "<i4"), ("mode", "<i4"), ("order", "<i4"), ("reserved", "<i4")])
    assert fold_dt.itemsize == 72 and pack_dt.itemsize == 56
    keep = []
    fj = np.zeros(len(fold_jobs), dtype=fold_dt)
    for i, (g, b, m, v, cb, outs, eps, C) in enumerate(fold_jobs):
        L.require_gpu(g, b, m, v, cb, *outs)
        fj[i] = (g.data_ptr(), b.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if cb is None else cb.data_ptr(), outs[0].data_ptr(),
                 outs[1].data_ptr(), outs[2].data_ptr(), float(eps), int(C))
        keep.append(outs)
    pj = np.zeros(len(pack_jobs), dtype=pack_dt)
    for i, (w, sc, out, Cout, Cin, taps, Mpad, Kpad, mode, order) in enumerate(pack_jobs):
        L.require_gpu(w, sc, out)
        assert w.is_contiguous() and out.is_contiguous() and out.numel() == Kpad * Mpad
        pj[i] = (w.data_ptr(), 0 if sc is None else sc.data_ptr(), out.data_ptr(), Cout, Cin, taps, Mpad, Kpad, mode, order, 0)
        keep.append(out)
    fchunks = L.chunk_list([int(job[7]) for job in fold_jobs], 256)      # 256 channels of a fold job per block
    pchunks = L.chunk_list([job[7] * job[6] for job in pack_jobs], lib.dasac_pack_chunk_elems())      # of Kpad * Mpad elements
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device) if a.size else None
    upi = lambda t: t.to(device) if len(t) else None
    return {"fold": up(fj), "fold_chunks": upi(fchunks), "n_fold_chunks": len(fchunks),
            "pack": up(pj), "pack_chunks": upi(pchunks), "n_pack_chunks": len(pchunks), "keep": keep}


def refresh_network(tables):
    """All frozen-BN folds, then all packed weight operands of a network: two launches."""
    lib = L.load()
    if tables["n_fold_chunks"]:
        L.check(lib.dasac_bn_fold_multi(tables["fold"].data_ptr(), tables["fold_chunks"].data_ptr(), tables["n_fold_chunks"],
                                        L.stream_ptr()), "dasac_bn_fold_multi")
    if tables["n_pack_chunks"]:
        L.check(lib.dasac_conv_pack_multi(tables["pack"].data_ptr(), tables["pack_chunks"].data_ptr(), tables["n_pack_chunks"],
                                          L.stream_ptr()), "dasac_conv_pack_multi")


def bn_param_grads(dot, sum_dz, mean, invstd, scale, conv_bias, want_gamma=True, want_beta=True, want_bias=False, outs=(None, None, None)):
    lib = L.load()
    Cn = sum_dz.numel()
    dg = _dest(outs[0], sum_dz) if want_gamma else None
    db = _dest(outs[1], sum_dz) if want_beta else None
    dcb = _dest(outs[2], sum_dz) if want_bias else None
    assert dot is None or (dot.dim() == 2 and dot.shape[1] == Cn and dot.is_contiguous())
    L.check(lib.dasac_bn_param_grads(L.ptr(dot), 0 if dot is None else dot.shape[0], sum_dz.data_ptr(), L.ptr(mean), L.ptr(invstd), L.ptr(scale), L.ptr(conv_bias),
                                     Cn, L.ptr(dg), L.ptr(db), L.ptr(dcb), L.stream_ptr()), "dasac_bn_param_grads")
    return dg, db, dcb


def channel_sums(x, out=None):
    lib = L.load()
    L.require_gpu(x)
    x = _c(x)
    N, Cn = x.shape[0], x.shape[1]
    out = _f32((Cn,), x) if out is None else out
    assert out.numel() == Cn and out.dtype == torch.float32 and out.is_contiguous()
    L.check(lib.dasac_channel_sums(x.data_ptr(), N, Cn, x[0, 0].numel(), out.data_ptr(), L.stream_ptr()), "dasac_channel_sums")
    return out


def pool_out(n, k, s, p, ceil_mode):
    """torch's pooling output-size rule."""
    num = n + 2 * p - k
    o = (-(-num // s) if ceil_mode else num // s) + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1
    return o


def maxpool_fwd(x, k, s, p, ceil_mode):
    lib = L.load()
    L.require_gpu(x)
    x = _c(x)
    B, Cn, H, W = x.shape
    OH, OW = pool_out(H, k, s, p, ceil_mode), pool_out(W, k, s, p, ceil_mode)
    y = _f32((B, Cn, OH, OW), x)
    arg = torch.empty((B, Cn, OH, OW), dtype=torch.uint8, device=x.device)
    with PROFILE.span("maxpool_fwd", 0.0, None, x.numel() * 4.0 + y.numel() * 5.0):
        L.check(lib.dasac_maxpool_fwd(x.data_ptr(), B * Cn, H, W, OH, OW, k, s, p, y.data_ptr(), arg.data_ptr(), L.stream_ptr()),
                "dasac_maxpool_fwd")
    return y, arg


def maxpool_bwd(dy, y, arg, in_hw, k, s, p, relu_mask):
    lib = L.load()
    L.require_gpu(dy, y, arg)
    dy = _c(dy)
    B, Cn, OH, OW = dy.shape
    H, W = in_hw
    dx = _f32((B, Cn, H, W), dy)
    # algorithmic bytes: dx written, dy + the argmax byte read; the pooled tensor only for windows beyond 11x11 (bit 7 of the byte)
    with PROFILE.span("maxpool_bwd", 0.0, None, dx.numel() * 4.0 + dy.numel() * (9.0 if (relu_mask and k > 11) else 5.0)):
        L.check(lib.dasac_maxpool_bwd(dy.data_ptr(), y.data_ptr(), arg.data_ptr(), B * Cn, H, W, OH, OW, k, s, p, int(relu_mask),
                                      dx.data_ptr(), L.stream_ptr()), "dasac_maxpool_bwd")
    return dx


def add(a, b, out=None):
    lib = L.load()
    L.require_gpu(a, b)
    out = torch.empty_like(a) if out is None else out
    L.check(lib.dasac_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), L.stream_ptr()), "dasac_add")
    return out


def relu_mask(dy, y):
    lib = L.load()
    L.require_gpu(dy, y)
    out = torch.empty_like(dy)
    L.check(lib.dasac_relu_mask(dy.data_ptr(), y.data_ptr(), out.data_ptr(), dy.numel(), L.stream_ptr()), "dasac_relu_mask")
    return out


def scale_planes(x, plane_scale):
    lib = L.load()
    L.require_gpu(x, plane_scale)
    x = _c(x)
    out = torch.empty_like(x)
    L.check(lib.dasac_scale_planes(x.data_ptr(), _c(plane_scale).data_ptr(), x.shape[0] * x.shape[1], x[0, 0].numel(),
                                   out.data_ptr(), L.stream_ptr()), "dasac_scale_planes")
    return out


def label_pad_mask(labels, pad_label=-1, ignore_label=255):
    """sac.py:337-338: returns ignore_mask = (labels == -1) (bool, same shape) and rewrites those labels to 255 IN PLACE."""
    lib = L.load()
    L.require_gpu(labels)
    assert labels.dtype == torch.int64
    work = labels if labels.is_contiguous() else labels.contiguous()
    mask = torch.empty(labels.shape, dtype=torch.bool, device=labels.device)
    L.check(lib.dasac_label_pad_mask(work.data_ptr(), mask.data_ptr(), work.numel(), int(pad_label), int(ignore_label),
                                     L.stream_ptr()), "dasac_label_pad_mask")
    if work is not labels:
        labels.copy_(work)                 # a strided caller tensor still sees the in-place rewrite
    else:
        torch.autograd.graph.increment_version(labels)
    return mask


def dropout_planes(B, Cn, p, device):
    """Dropout2d noise [B, C]: keep/(1-p), drawn on the device by a counter-based Philox keyed on torch's CUDA generator.
    (seed, offset) come from the device generator's own Philox state and the offset is ADVANCED there, so
    torch.manual_seed / torch.cuda.get_rng_state / set_rng_state (checkpoint resume) reproduce the masks exactly as they
    do for ATen's dropout, per device.  (The numbers are not ATen's -- parity tests inject `module.keep_mask`.)"""
    lib = L.load()
    out = torch.empty((B, Cn), dtype=torch.float32, device=device)
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    seed, offset = gen.initial_seed(), gen.get_offset()
    gen.set_offset(offset + 4 * ((B * Cn + 3) // 4))             # Philox offsets move in multiples of 4
    L.check(lib.dasac_dropout_planes(seed & 0xFFFFFFFFFFFFFFFF, offset, float(p), B * Cn, out.data_ptr(), L.stream_ptr()),
            "dasac_dropout_planes")
    return out


def class_sums(probs):
    """float64 [C] sums over batch and pixels of probs [B,C,H,W] (sac.py:108 before the division)."""
    lib = L.load()
    L.require_gpu(probs)
    probs = _c(probs)
    B, Cn = probs.shape[0], probs.shape[1]
    return _bn_sums(lib.dasac_bn_stats, (probs.data_ptr(),), B, Cn, probs[0, 0].numel(), probs.device, "dasac_bn_stats")[:Cn]


def _bn_sums(fn, lead_ptrs, N, Cn, HW, device, what):
    """Two-stage per-channel reduction (dasac_bn_stats / dasac_bn_bwd_reduce): float64 [2*C]."""
    lib = L.load()
    sums = torch.empty(2 * Cn, dtype=torch.float64, device=device)
    ws = L.workspace(lib.dasac_bn_stats_workspace(N, Cn, HW), device)
    L.check(fn(*lead_ptrs, N, Cn, HW, sums.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()), what)
    return sums


def bump_versions(tensors):
    """Kernels write parameters through raw pointers; autograd's version counters (which key the engine's packed-weight
    and BN-fold caches) have to be told."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class EmaPlan:
    """Device-side pointer/chunk tables for the multi-tensor teacher update (built once; rebuilt by the
    caller when parameter storage moves)."""

    def __init__(self, fast_tensors, slow_tensors):
        import numpy as np
        lib = L.load()
        L.require_gpu(*fast_tensors)
        L.require_gpu(*slow_tensors)
        pairs = np.zeros((len(fast_tensors), 3), dtype=np.int64)
        for i, (f, s) in enumerate(zip(fast_tensors, slow_tensors)):
            assert f.is_contiguous() and s.is_contiguous() and f.numel() == s.numel() and f.dtype == torch.float32
            pairs[i] = (f.data_ptr(), s.data_ptr(), f.numel())
        chunks = L.chunk_list([f.numel() for f in fast_tensors], lib.dasac_ema_chunk_elems())
        dev = fast_tensors[0].device
        self.key = tuple(int(v) for v in pairs[:, :2].reshape(-1))
        self.pairs = torch.from_numpy(pairs).to(dev)
        self.chunks = chunks.to(dev)
        self.sq = torch.empty(len(fast_tensors) + len(chunks), dtype=torch.float64, device=dev)   # per-tensor sums + chunk partials
        self.n_tensors, self.n_chunks = len(fast_tensors), len(chunks)
        self.slow = list(slow_tensors)

    def run(self, momentum, update):
        lib = L.load()
        out = torch.empty(1, dtype=torch.float32, device=self.pairs.device)
        L.check(lib.dasac_ema_update(self.pairs.data_ptr(), self.n_tensors, self.chunks.data_ptr(), self.n_chunks,
                                     float(momentum), int(bool(update)), self.sq.data_ptr(), out.data_ptr(), L.stream_ptr()),
                "dasac_ema_update")
        if update:
            bump_versions(self.slow)
        return out


# ----------------------------------------------------------------------------------------------
# train-mode BatchNorm (batch statistics; SyncBN when a process group with >1 ranks exists)
# ----------------------------------------------------------------------------------------------
def _world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _allreduce_sums(sums, count):
    """SyncBN: one all-reduce of the raw sums + the element count over RCCL (deeplabv2.py:15); identity on one rank.
    Returns (sums, host count or 0.0, device count or None) -- with several ranks the count stays on the device."""
    if _world() == 1:
        return sums, float(count), None
    import torch.distributed as dist
    packed = torch.cat([sums, torch.tensor([float(count)], dtype=torch.float64, device=sums.device)])
    dist.all_reduce(packed)
    return packed[:-1], 0.0, packed[-1:]


def bn_train_forward(z, bn, res=None, relu=False, update_running=True, tile_stats=None):
    """y = relu?(BN_batch(z) (+res)); returns (y, (mean, invstd, count, count_dev)).  Updates bn.running_* like ATen.
    tile_stats: the per-tile channel statistics the producing conv_gemm(stats=...) left -- then z is not read for them."""
    lib = L.load()
    L.require_gpu(z, res, tile_stats)
    N, Cn = z.shape[0], z.shape[1]
    HW = z[0, 0].numel()
    scale, shift, mean, invstd = (_f32((Cn,), z) for _ in range(4))
    upd = update_running and bn.track_running_stats
    # momentum None: cumulative average over num_batches_tracked (absent when track_running_stats=False; nothing moves then)
    mom = 0.0 if not upd else bn.momentum if bn.momentum is not None else 1.0 / float(int(bn.num_batches_tracked) + 1)
    tail = (bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr() if upd else None, bn.running_var.data_ptr() if upd else None,
            bn.num_batches_tracked.data_ptr() if upd else None, float(mom), float(bn.eps), Cn, scale.data_ptr(), shift.data_ptr(),
            mean.data_ptr(), invstd.data_ptr(), L.stream_ptr())
    if tile_stats is not None and _world() == 1 and N * Cn < 65536:
        # one rank: ONE launch per BN layer -- every block adds its channel's tile statistics itself, then normalises its chunk
        count, count_dev = float(N * HW), None
        y = torch.empty_like(z)
        L.check(lib.dasac_bn_train_apply_tiles(z.data_ptr(), tile_stats.data_ptr(), tile_stats.shape[0], tile_stats.shape[2], count,
                                               tail[0], tail[1], tail[2], tail[3], tail[4], tail[5], tail[6], L.ptr(res), int(relu),
                                               N, Cn, HW, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), L.stream_ptr()),
                "dasac_bn_train_apply_tiles")
        if upd:
            bump_versions([bn.running_mean, bn.running_var, bn.num_batches_tracked])
        return y, (mean, invstd, count, count_dev)
    else:
        if tile_stats is not None:
            sums = torch.empty(2 * Cn, dtype=torch.float64, device=z.device)
            L.check(lib.dasac_bn_tile_stats_reduce(tile_stats.data_ptr(), tile_stats.shape[0], Cn, tile_stats.shape[2], sums.data_ptr(),
                                                   L.stream_ptr()), "dasac_bn_tile_stats_reduce")
        else:
            sums = _bn_sums(lib.dasac_bn_stats, (z.data_ptr(),), N, Cn, HW, z.device, "dasac_bn_stats")
        sums, count, count_dev = _allreduce_sums(sums, N * HW)
        L.check(lib.dasac_bn_train_finalize(sums.data_ptr(), count, L.ptr(count_dev), *tail), "dasac_bn_train_finalize")
    if upd:                                                    # written through raw pointers; eval-mode folds key on them
        bump_versions([bn.running_mean, bn.running_var, bn.num_batches_tracked])
    y = torch.empty_like(z)
    L.check(lib.dasac_bn_apply(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), L.ptr(res), int(relu), N, Cn, HW, y.data_ptr(),
                               L.stream_ptr()), "dasac_bn_apply")
    return y, (mean, invstd, count, count_dev)


def bn_train_backward(dy, z, stats, gamma, want_params=True, outs=(None, None)):
    """dy: gradient w.r.t. the BN output (ReLU mask already applied).  Returns (dz, dgamma, dbeta)."""
    lib = L.load()
    L.require_gpu(dy, z)
    mean, invstd, count, count_dev = stats
    N, Cn = z.shape[0], z.shape[1]
    HW = z[0, 0].numel()
    dy = _c(dy)
    dg = _dest(outs[0], gamma) if want_params else None
    db = _dest(outs[1], gamma) if want_params else None
    ws = L.workspace(lib.dasac_bn_stats_workspace(N, Cn, HW), z.device)
    if _world() == 1 and count_dev is None and N * Cn < 65536:
        # one rank: reduction stage 1 + ONE kernel that adds the partials per block, forms dz and writes d gamma / d beta
        dz = torch.empty_like(z)
        L.check(lib.dasac_bn_bwd_fused(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), float(count),
                                       N, Cn, HW, dz.data_ptr(), L.ptr(dg), L.ptr(db), ws.data_ptr(), ws.numel(), L.stream_ptr()),
                "dasac_bn_bwd_fused")
        return dz, dg, db
    # several ranks: the finish kernel also writes d gamma / d beta -- this rank's LOCAL sums (DDP averages them afterwards)
    sums = torch.empty(2 * Cn, dtype=torch.float64, device=z.device)
    L.check(lib.dasac_bn_bwd_reduce(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), N, Cn, HW, sums.data_ptr(),
                                    L.ptr(dg), L.ptr(db), ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_bn_bwd_reduce")
    if _world() > 1:
        import torch.distributed as dist
        dist.all_reduce(sums)
    dz = torch.empty_like(z)
    L.check(lib.dasac_bn_bwd_apply(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                   sums.data_ptr(), float(count), L.ptr(count_dev), N, Cn, HW, dz.data_ptr(), None, None, L.stream_ptr()),
            "dasac_bn_bwd_apply")
    return dz, dg, db


# ----------------------------------------------------------------------------------------------
# tap-expanded convolution (ASPP classifiers): dense 1x1 GEMMs over taps*Cp channels + shift kernels
# ----------------------------------------------------------------------------------------------
class ExpandedConv:
    """Static description: `spec` (multi-branch, stride 1) -> 1x1 spec over E = taps*Cp expanded channels."""

    def __init__(self, spec):
        assert spec.stride == 1 and spec.taps <= 64
        self.spec = spec
        cp = spec.cout
        while (spec.taps * cp) % 16:
            cp += 1
        self.cp, self.E = cp, spec.taps * cp
        self.spec1 = ConvSpec(spec.cin, self.E, [(1, 1, 1, 0)], 1)
        self._cols = [torch.tensor(c, dtype=_i32) for c in zip(*spec.branches)]      # host arrays kh, kw, dil, pad

    def _branch_args(self):
        c = self._cols
        return c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), c[3].data_ptr(), len(self.spec.branches)

    def pack(self, weights, transposed, out=None):
        lib = L.load()
        M = self.spec.cin if transposed else self.E
        K = self.E if transposed else self.spec.cin
        if out is None:
            out = torch.empty((lib.dasac_conv_kpad(K), lib.dasac_conv_mpad(M)), dtype=torch.float32, device=weights[0].device)
        for w, (taps, tap0) in zip(weights, _branch_taps(self.spec)):
            L.check(lib.dasac_conv_pack_expanded(_c(w).data_ptr(), self.spec.cout, self.spec.cin, taps, tap0, self.spec.taps,
                                                 self.cp, int(transposed), out.data_ptr(), L.stream_ptr()), "dasac_conv_pack_expanded")
        return _finish_pack(out, M, K)

    def forward(self, x, packed, table, bias):
        """x [B,Cin,H,W] -> out [B,Cout,H,W]."""
        lib = L.load()
        B, _, H, W = x.shape
        y = torch.empty((B, self.E, H, W), dtype=torch.float32, device=x.device)
        conv_gemm(x, packed, table, y, (H, W), 1, self.E, self.spec.cin)
        out = torch.empty((B, self.spec.cout, H, W), dtype=torch.float32, device=x.device)
        L.check(lib.dasac_tap_gather(y.data_ptr(), *self._branch_args(), self.cp, self.spec.cout, L.ptr(bias), B, H, W,
                                     out.data_ptr(), L.stream_ptr()), "dasac_tap_gather")
        return out

    def scatter(self, dout):
        lib = L.load()
        B, _, H, W = dout.shape
        d = torch.empty((B, self.E, H, W), dtype=torch.float32, device=dout.device)
        L.check(lib.dasac_tap_scatter(_c(dout).data_ptr(), *self._branch_args(), self.cp, self.spec.cout, B, H, W, d.data_ptr(),
                                      L.stream_ptr()), "dasac_tap_scatter")
        return d

    def wgrad(self, d, x, weights, table, outs=None):
        """Weight gradients of every branch from the expanded gradient d [B,E,H,W]."""
        lib = L.load()
        B, Cx, H, W = x.shape
        nbytes = lib.dasac_conv_wgrad_workspace(B, H, W, self.E, self.spec.cin)
        ws = L.workspace(nbytes, x.device)
        with PROFILE.span("conv_wgrad", 2.0 * B * H * W * self.E * self.spec.cin, (self.E, self.spec.cin, B * H * W, 1, 1, False, False)):
            fn = lib.dasac_conv_wgrad_x3 if PRECISION == "bf16x3" else lib.dasac_conv_wgrad
            L.check(fn(d.data_ptr(), x.data_ptr(), table.data_ptr(), B, Cx, H, W, H, W, 1, self.E, self.spec.cin,
                       ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_conv_wgrad")
        grads = [_dest(None if outs is None else outs[bi], w) for bi, w in enumerate(weights)]
        for dw, (taps, tap0) in zip(grads, _branch_taps(self.spec)):
            L.check(lib.dasac_conv_wgrad_finish_expanded(ws.data_ptr(), B, H, W, self.E, self.spec.cin, dw.data_ptr(),
                                                         self.spec.cout, taps, tap0, self.cp, L.stream_ptr()),
                    "dasac_conv_wgrad_finish_expanded")
        return grads

    def dgrad(self, d, packed_t, table_t, in_hw, res=None, mask=None):
        B = d.shape[0]
        H, W = in_hw
        dx = torch.empty((B, self.spec.cin, H, W), dtype=torch.float32, device=d.device)
        return conv_gemm(d, packed_t, table_t, dx, (H, W), 1, self.spec.cin, self.E, 1, None, res, mask, False)


def iou_counts(logits_up, gt, counts=None, ignore_index=255):
    """Accumulates per-class (tp, fp, fn) pixel counts of argmax(logits_up) vs gt into `counts` (int64 [3,C])."""
    lib = L.load()
    L.require_gpu(logits_up, gt)
    logits_up, gt = _c(logits_up), _c(gt)
    B, Cn, H, W = logits_up.shape
    if counts is None:
        counts = torch.zeros((3, Cn), dtype=torch.int64, device=logits_up.device)
    L.check(lib.dasac_iou_counts(logits_up.data_ptr(), gt.data_ptr(), B, Cn, H * W, int(ignore_index), counts.data_ptr(),
                                 L.stream_ptr()), "dasac_iou_counts")
    return counts


def label_hist(labels_u8, counts=None):
    """Per-image histogram of uint8 label maps ([B,H,W] or [H,W], contiguous, any alignment): accumulates the number of
    pixels of every value 0..255 of image b into `counts[b]` (int64 [B,256]; allocated zeroed when None).  Value 255 is
    counted like any other; sampling.weights_from_counts drops it."""
    lib = L.load()
    L.require_gpu(labels_u8, counts)
    if labels_u8.dtype != torch.uint8 or labels_u8.dim() not in (2, 3) or not labels_u8.is_contiguous():
        raise L.DasacError("label_hist takes a contiguous uint8 [B,H,W] or [H,W] tensor (got {} {}, contiguous: {})".format(
            labels_u8.dtype, tuple(labels_u8.shape), labels_u8.is_contiguous()))
    B = labels_u8.shape[0] if labels_u8.dim() == 3 else 1
    HW = labels_u8.shape[-2] * labels_u8.shape[-1]
    if counts is None:
        counts = torch.zeros((B, 256), dtype=torch.int64, device=labels_u8.device)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (B, 256) or not counts.is_contiguous():
        raise L.DasacError("label_hist accumulates into a contiguous int64 [{},256] tensor (got {} {})".format(
            B, counts.dtype, tuple(counts.shape)))
    L.check(lib.dasac_label_hist(labels_u8.data_ptr(), B, HW, counts.data_ptr(), L.stream_ptr()), "dasac_label_hist")
    return counts


MASK_COUNTS_MAX_SCORES, MASK_COUNTS_MAX_MAPS = 4, 2


# What `mask_counts`, `confusion_counts`, `boundary_counts` and `segment_counts` check alike, in the order they check it: _count_front, the class count
# (_count_classes), then _count_layers; a wrapper's own checks go between them.
def _count_front(op, scores, label_maps, gt, *outs):
    """The layer lists and the ground truth: (scores, label_maps, B, H, W)."""
    scores, label_maps = list(scores or ()), list(label_maps or ())
    L.require_gpu(gt, *outs, *scores, *label_maps)
    if not scores and not label_maps or len(scores) > MASK_COUNTS_MAX_SCORES or len(label_maps) > MASK_COUNTS_MAX_MAPS:
        raise L.DasacError("{} takes 1..{} score tensors and / or 1..{} label maps (got {} and {})".format(
            op, MASK_COUNTS_MAX_SCORES, MASK_COUNTS_MAX_MAPS, len(scores), len(label_maps)))
    if gt.dtype != torch.int64 or gt.dim() != 3:
        raise L.DasacError("{}: gt must be int64 [B,H,W] (got {} {})".format(op, gt.dtype, tuple(gt.shape)))
    return (scores, label_maps) + tuple(gt.shape)


def _count_classes(op, scores, given, out_name):
    """The class count: from the first score tensor, else what `given()` reads from the output tensor or `num_classes`."""
    Cn = scores[0].shape[1] if scores else given()
    if Cn is None:
        raise L.DasacError("{}: label maps alone do not tell the class count; pass {} or num_classes".format(op, out_name))
    return Cn


def _count_layers(op, scores, label_maps, gt, B, Cn, H, W, map_dtypes):
    """Every layer's dtype and shape: contiguous (scores, label_maps, gt), the padded pointer slots and the uint8-map mask."""
    for s in scores:
        if s.dtype != torch.float32 or tuple(s.shape) != (B, Cn, H, W):
            raise L.DasacError("{}: a score tensor must be float32 {} (got {} {})".format(op, (B, Cn, H, W), s.dtype, tuple(s.shape)))
    kinds = " or ".join(str(d).replace("torch.", "") for d in map_dtypes)
    for m in label_maps:
        if m.dtype not in map_dtypes or tuple(m.shape) != (B, H, W):
            raise L.DasacError("{}: a label map must be {} {} (got {} {})".format(op, kinds, (B, H, W), m.dtype, tuple(m.shape)))
    scores, label_maps, gt = [_c(s) for s in scores], [_c(m) for m in label_maps], _c(gt)
    sp = [s.data_ptr() for s in scores] + [0] * (MASK_COUNTS_MAX_SCORES - len(scores))
    mp = [m.data_ptr() for m in label_maps] + [0] * (MASK_COUNTS_MAX_MAPS - len(label_maps))
    return scores, label_maps, gt, sp, mp, sum(1 << i for i, m in enumerate(label_maps) if m.dtype == torch.uint8)


def mask_counts(scores, label_maps, gt, counts=None, ignore_index=255, num_classes=None):
    """Validation counts of several mask layers against one ground truth in ONE launch (train.py:386-399, utils/metrics.py:18-39).
    scores: up to 4 fp32 [B,C,H,W] tensors (arg-max, first maximum wins); label_maps: up to 2 int64 [B,H,W] maps (255 = no label);
    gt int64 [B,H,W].  Accumulates (tp, fp, fn) per layer into `counts` (int64 [L,3,C], scores first, then label maps; allocated
    zeroed when None) and returns it.  With label maps only, C comes from `counts` or `num_classes`."""
    lib = L.load()
    scores, label_maps, B, H, W = _count_front("mask_counts", scores, label_maps, gt, counts)
    Cn = _count_classes("mask_counts", scores, lambda: counts.shape[2] if counts is not None else num_classes, "counts")
    scores, label_maps, gt, sp, mp, _ = _count_layers("mask_counts", scores, label_maps, gt, B, Cn, H, W, (torch.int64,))
    n_layers = len(scores) + len(label_maps)
    if counts is None:
        counts = torch.zeros((n_layers, 3, Cn), dtype=torch.int64, device=gt.device)
    elif counts.dtype != torch.int64 or tuple(counts.shape) != (n_layers, 3, Cn) or not counts.is_contiguous():
        raise L.DasacError("mask_counts accumulates into a contiguous int64 [{},3,{}] tensor (got {} {})".format(
            n_layers, Cn, counts.dtype, tuple(counts.shape)))
    L.check(lib.dasac_mask_counts(*sp, *mp, gt.data_ptr(), B, Cn, H * W, int(ignore_index), counts.data_ptr(), L.stream_ptr()),
            "dasac_mask_counts")
    return counts


CONFUSION_MAX_BINS = 32


def confusion_counts(scores, label_maps, gt, confusion=None, reliability=None, bins=0, logits_layers=(), ignore_index=255,
                     num_classes=None):
    """The joint tables of `mask_counts`' pass in ONE launch (include/dasac_hip.h: dasac_confusion_counts).  scores: up to 4 fp32
    [B,C,H,W] tensors (arg-max, first maximum wins); label_maps: up to 2 [B,H,W] maps, int64 or uint8 each (255 = no label); gt int64
    [B,H,W].  Accumulates into `confusion` (int64 [L,C+1,C+1], scores first, then label maps; row = ground truth, column =
    prediction, index C = no class; allocated zeroed when None).  With `bins` > 0 (or a `reliability` tensor, whose shape gives the
    bins) it also accumulates into `reliability` (int64 [len(scores),C,bins,2]: arg-max class, bin of the winning confidence, miss /
    hit); `logits_layers` lists the indices into `scores` that hold logits -- their confidence is the soft-max maximum -- the others
    hold probabilities.  With label maps only, C comes from `confusion` or `num_classes`.  Returns (confusion, reliability or None)."""
    lib = L.load()
    op = "confusion_counts"
    scores, label_maps, B, H, W = _count_front(op, scores, label_maps, gt, confusion, reliability)
    Cn = _count_classes(op, scores, lambda: confusion.shape[1] - 1 if confusion is not None else num_classes, "confusion")
    scores, label_maps, gt, sp, mp, u8_mask = _count_layers(op, scores, label_maps, gt, B, Cn, H, W, (torch.int64, torch.uint8))
    n_layers = len(scores) + len(label_maps)
    if confusion is None:
        confusion = torch.zeros((n_layers, Cn + 1, Cn + 1), dtype=torch.int64, device=gt.device)
    elif confusion.dtype != torch.int64 or tuple(confusion.shape) != (n_layers, Cn + 1, Cn + 1) or not confusion.is_contiguous():
        raise L.DasacError("confusion_counts accumulates into a contiguous int64 [{},{},{}] tensor (got {} {})".format(
            n_layers, Cn + 1, Cn + 1, confusion.dtype, tuple(confusion.shape)))
    bins = int(bins)
    if reliability is not None:
        bins = int(reliability.shape[2]) if reliability.dim() == 4 else -1          # -1: refused below
    logits_layers = sorted(set(int(i) for i in logits_layers))
    if bins:
        if not scores or not 1 <= bins <= CONFUSION_MAX_BINS:
            raise L.DasacError("confusion_counts: a reliability table needs a score tensor and 1..{} bins (got {} tensors, {} bins)".format(
                CONFUSION_MAX_BINS, len(scores), bins))
        if any(i < 0 or i >= len(scores) for i in logits_layers):
            raise L.DasacError("confusion_counts: logits_layers {} names no score tensor of {}".format(logits_layers, len(scores)))
        if reliability is None:
            reliability = torch.zeros((len(scores), Cn, bins, 2), dtype=torch.int64, device=gt.device)
        elif reliability.dtype != torch.int64 or tuple(reliability.shape) != (len(scores), Cn, bins, 2) or not reliability.is_contiguous():
            raise L.DasacError("confusion_counts accumulates into a contiguous int64 [{},{},bins,2] reliability tensor (got {} {})".format(
                len(scores), Cn, reliability.dtype, tuple(reliability.shape)))
    L.check(lib.dasac_confusion_counts(*sp, *mp, u8_mask, gt.data_ptr(), B, Cn, H * W, int(ignore_index), confusion.data_ptr(),
                                       L.ptr(reliability), bins, sum(1 << i for i in logits_layers), L.stream_ptr()),
            "dasac_confusion_counts")
    return confusion, reliability


BOUNDARY_MAX_RADIUS = 16                                    # DASAC_BOUNDARY_MAX_RADIUS
BOUNDARY_ROWS = ("tp", "fp", "fn", "pred", "both")          # dimension 2 of a boundary table


def boundary_counts(scores, label_maps, gt, table=None, radius=8, ignore_index=255, num_classes=None):
    """`mask_counts`' counts split by the distance to the nearest class contour (include/dasac_hip.h: dasac_boundary_counts).
    scores: up to 4 fp32 [B,C,H,W] tensors (arg-max, first maximum wins); label_maps: up to 2 [B,H,W] maps, int64 or uint8 each (255 =
    no label; a uint8 map is read as it is); gt int64 [B,H,W].  Accumulates into `table` (int64 [L,radius+1,5,C], scores first, then
    label maps; allocated zeroed when None; a given table tells the radius) and returns it: slot s < radius holds the pixels at
    Chebyshev distance s + 1 from a contour, slot `radius` everything further; rows BOUNDARY_ROWS -- tp, fp, fn by the pixel's slot
    in the ground truth, pred by its slot in the predicted map, both (prediction == ground truth) by the larger of the two.  With
    label maps only, C comes from `table` or `num_classes`.  driver.summarise_boundary reads the tables."""
    lib = L.load()
    op = "boundary_counts"
    scores, label_maps, B, H, W = _count_front(op, scores, label_maps, gt, table)
    if table is not None and (table.dtype != torch.int64 or table.dim() != 4):
        raise L.DasacError("boundary_counts accumulates into an int64 [L,radius+1,5,C] tensor (got {} {})".format(table.dtype, tuple(table.shape)))
    Cn = _count_classes(op, scores, lambda: table.shape[3] if table is not None else num_classes, "table")
    radius = int(table.shape[1]) - 1 if table is not None else int(radius)
    if not 1 <= radius <= BOUNDARY_MAX_RADIUS:
        raise L.DasacError("boundary_counts: the radius must be in 1..{} (got {})".format(BOUNDARY_MAX_RADIUS, radius))
    scores, label_maps, gt, sp, mp, u8_mask = _count_layers(op, scores, label_maps, gt, B, Cn, H, W, (torch.int64, torch.uint8))
    n_layers = len(scores) + len(label_maps)
    shape = (n_layers, radius + 1, len(BOUNDARY_ROWS), Cn)
    if table is None:
        table = torch.zeros(shape, dtype=torch.int64, device=gt.device)
    elif tuple(table.shape) != shape or not table.is_contiguous():
        raise L.DasacError("boundary_counts accumulates into a contiguous int64 {} tensor (got {} {})".format(shape, table.dtype, tuple(table.shape)))
    need = lib.dasac_boundary_counts_workspace(n_layers, B, H, W)
    ws = L.workspace(need, gt.device)
    L.check(lib.dasac_boundary_counts(*sp, *mp, u8_mask, gt.data_ptr(), B, Cn, H, W, radius, int(ignore_index), table.data_ptr(),
                                      ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_boundary_counts")
    return table


SEGMENT_BINS = 24                                           # DASAC_SEGMENT_BINS
SEGMENT_ROWS = ("segments", "pixels", "matched_pixels", "matched_segments")     # dimension 3 of a segment table
SEGMENT_TILE = (32, 64)                                     # csrc/segments_index.hpp: kTileH x kTileW, where the kernels' seams lie
SEGMENT_MAX_CLASSES, SEGMENT_COUNTS_MAX_CLASSES = 255, 64


def _segment_gpu(op, *tensors):
    """L.require_gpu with the op's name in front of the refusal."""
    try:
        L.require_gpu(*tensors)
    except L.DasacError as exc:
        raise L.DasacError("{}: {}".format(op, exc)) from None


def _segment_map(op, labels, num_classes, connectivity, limit=SEGMENT_MAX_CLASSES):
    """What the segment ops check of a label map alike: (contiguous labels, B, H, W, C, connectivity)."""
    _segment_gpu(op, labels)
    if labels.dtype not in (torch.int64, torch.uint8) or labels.dim() != 3 or labels.numel() == 0:
        raise L.DasacError("{}: labels must be a non-empty int64 or uint8 [B,H,W] map (got {} {})".format(op, labels.dtype, tuple(labels.shape)))
    Cn, connectivity = int(num_classes), int(connectivity)
    if not 1 <= Cn <= limit:
        raise L.DasacError("{}: num_classes must be in 1..{} (got {})".format(op, limit, Cn))
    if connectivity not in (4, 8):
        raise L.DasacError("{}: connectivity must be 4 or 8 (got {})".format(op, connectivity))
    B, H, W = labels.shape
    if H * W > 2 ** 31 - 1:
        raise L.DasacError("{}: an image of {} x {} pixels is larger than 2^31 - 1".format(op, H, W))
    return _c(labels), B, H, W, Cn, connectivity


def label_segments(labels, num_classes, connectivity=8, want_size=True):
    """Connected components of a label map (include/dasac_hip.h: dasac_label_segments).  labels: int64 or uint8 [B,H,W]; a value in
    [0, num_classes) is a class, anything else (255, -1) no class.  Returns (segment, size): int32 [B,H,W] each -- the root (smallest
    y*W + x) of the pixel's segment under `connectivity` 4 or 8, -1 where the pixel holds no class, and the pixel count of that
    segment, 0 there; size is None unless `want_size`.  The images of a batch do not see each other."""
    lib = L.load()
    labels, B, H, W, Cn, connectivity = _segment_map("label_segments", labels, num_classes, connectivity)
    segment = torch.empty((B, H, W), dtype=torch.int32, device=labels.device)
    size = torch.empty((B, H, W), dtype=torch.int32, device=labels.device) if want_size else None
    ws = L.workspace(lib.dasac_label_segments_workspace(B, H, W), labels.device)
    L.check(lib.dasac_label_segments(labels.data_ptr(), int(labels.dtype == torch.uint8), B, Cn, H, W, connectivity, segment.data_ptr(),
                                     L.ptr(size), L.ptr(ws), ws.numel(), L.stream_ptr()), "dasac_label_segments")
    return segment, size


def segment_counts(scores, label_maps, gt, table=None, connectivity=8, ignore_index=255, num_classes=None):
    """Object-level validation tables (include/dasac_hip.h: dasac_segment_counts).  scores: up to 4 fp32 [B,C,H,W] tensors (arg-max,
    first maximum wins); label_maps: up to 2 [B,H,W] maps, int64 or uint8 each (255 = no label); gt int64 [B,H,W].  Accumulates into
    `table` (int64 [L,2,SEGMENT_BINS,4,C], scores first, then label maps; allocated zeroed when None) and returns it: side 0 counts
    the ground truth's segments, side 1 the predicted map's, each in the bin floor(log2(size)) of its size (the last bin takes
    everything larger); rows SEGMENT_ROWS -- segments, their counted pixels, the pixels of them the other map gives the same class,
    and the segments where those are more than half (objects found / segments that are real).  With label maps only, C comes from
    `table` or `num_classes`.  driver.summarise_segments reads the tables."""
    lib = L.load()
    op = "segment_counts"
    _segment_gpu(op, gt, table, *(scores or ()), *(label_maps or ()))
    scores, label_maps, B, H, W = _count_front(op, scores, label_maps, gt, table)
    if table is not None and (table.dtype != torch.int64 or table.dim() != 5):
        raise L.DasacError("segment_counts accumulates into an int64 [L,2,{},4,C] tensor (got {} {})".format(SEGMENT_BINS, table.dtype, tuple(table.shape)))
    Cn = _count_classes(op, scores, lambda: table.shape[4] if table is not None else num_classes, "table")
    connectivity = int(connectivity)
    if connectivity not in (4, 8) or not 1 <= Cn <= SEGMENT_COUNTS_MAX_CLASSES:
        raise L.DasacError("segment_counts: connectivity must be 4 or 8 and C in 1..{} (got {} and {})".format(
            SEGMENT_COUNTS_MAX_CLASSES, connectivity, Cn))
    scores, label_maps, gt, sp, mp, u8_mask = _count_layers(op, scores, label_maps, gt, B, Cn, H, W, (torch.int64, torch.uint8))
    n_layers = len(scores) + len(label_maps)
    shape = (n_layers, 2, SEGMENT_BINS, len(SEGMENT_ROWS), Cn)
    if table is None:
        table = torch.zeros(shape, dtype=torch.int64, device=gt.device)
    elif tuple(table.shape) != shape or not table.is_contiguous():
        raise L.DasacError("segment_counts accumulates into a contiguous int64 {} tensor (got {} {})".format(shape, table.dtype, tuple(table.shape)))
    need = lib.dasac_segment_counts_workspace(n_layers, B, H, W)
    ws = L.workspace(need, gt.device)
    L.check(lib.dasac_segment_counts(*sp, *mp, u8_mask, gt.data_ptr(), B, Cn, H, W, connectivity, int(ignore_index), table.data_ptr(),
                                     ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_segment_counts")
    return table


def segment_filter(labels, min_size, num_classes, fill=255, connectivity=8):
    """A copy of the label map (int64 or uint8 [B,H,W]) in which every pixel of a segment smaller than `min_size` pixels holds `fill`
    (include/dasac_hip.h: dasac_segment_filter); every other pixel, no-class pixels included, keeps its value, and min_size <= 1
    copies the map.  The input is not written."""
    lib = L.load()
    labels, B, H, W, Cn, connectivity = _segment_map("segment_filter", labels, num_classes, connectivity)
    fill = int(fill)
    if labels.dtype == torch.uint8 and not 0 <= fill <= 255:
        raise L.DasacError("segment_filter: fill {} does not fit a uint8 map".format(fill))
    out = torch.empty_like(labels)
    ws = L.workspace(lib.dasac_segment_filter_workspace(B, H, W), labels.device)
    L.check(lib.dasac_segment_filter(labels.data_ptr(), int(labels.dtype == torch.uint8), B, Cn, H, W, connectivity,
                                     max(-1, min(int(min_size), 2 ** 31 - 1)), fill, out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()),
            "dasac_segment_filter")
    return out


CONSISTENCY_MAX_VIEWS, CONSISTENCY_MAX_CLASSES = 8, 32      # DASAC_CONSISTENCY_MAX_VIEWS; the kernel's class limit


class ConsistencyTables(tuple):
    """The three tables of `view_consistency` as views of ONE contiguous int64 buffer (`buffer`: one all-reduce, one D2H copy):
    agree [C+1,T+1,T+1], flips [C,C], per_view [T,2] (include/dasac_hip.h: dasac_view_consistency)."""

    def __new__(cls, buffer, C, T):
        C, T = int(C), int(T)
        if buffer.dtype != torch.int64 or buffer.dim() != 1 or buffer.numel() != consistency_size(C, T) or not buffer.is_contiguous():
            raise L.DasacError("view_consistency accumulates into a contiguous int64 [{}] buffer for C={}, T={} (got {} {})".format(
                consistency_size(C, T), C, T, buffer.dtype, tuple(buffer.shape)))
        a, f = (C + 1) * (T + 1) * (T + 1), C * C
        self = super().__new__(cls, (buffer[:a].view(C + 1, T + 1, T + 1), buffer[a:a + f].view(C, C), buffer[a + f:].view(T, 2)))
        self.buffer, self.C, self.T = buffer, C, T
        return self

    agree = property(lambda self: self[0])
    flips = property(lambda self: self[1])
    per_view = property(lambda self: self[2])

    def cpu(self):
        return ConsistencyTables(self.buffer.cpu(), self.C, self.T)


def consistency_size(C, T):
    return (C + 1) * (T + 1) * (T + 1) + C * C + 2 * T


def consistency_tables(C, T, device):
    """A zeroed buffer for `view_consistency`, as ConsistencyTables."""
    return ConsistencyTables(torch.zeros(consistency_size(C, T), dtype=torch.int64, device=device), C, T)


def view_consistency(aligned, T, tables=None, cover=0.5):
    """Label-free agreement of the T aligned teacher views of every group in ONE launch (include/dasac_hip.h:
    dasac_view_consistency).  aligned: fp32 [N*T,C,H,W], view t of group n at n*T + t -- `warp_pool`'s aligned tensor, the
    `teacher_aligned` of a target step.  A view is covered at a pixel when its class sum is >= `cover`; the consensus is the arg-max of
    the plain sum over the T views.  Accumulates into `tables` (a ConsistencyTables or its flat int64 buffer; allocated zeroed when
    None) and returns the ConsistencyTables (agree [C+1,T+1,T+1], flips [C,C], per_view [T,2])."""
    lib = L.load()
    L.require_gpu(aligned, tables.buffer if isinstance(tables, ConsistencyTables) else tables)
    T = int(T)
    if aligned.dtype != torch.float32 or aligned.dim() != 4:
        raise L.DasacError("view_consistency takes a float32 [N*T,C,H,W] tensor (got {} {})".format(aligned.dtype, tuple(aligned.shape)))
    NT, Cn, H, W = aligned.shape
    if not 1 <= T <= CONSISTENCY_MAX_VIEWS or not 1 <= Cn <= CONSISTENCY_MAX_CLASSES:
        raise L.DasacError("view_consistency: 1..{} views and 1..{} classes (got T={}, C={})".format(
            CONSISTENCY_MAX_VIEWS, CONSISTENCY_MAX_CLASSES, T, Cn))
    if NT == 0 or NT % T:
        raise L.DasacError("view_consistency: {} views are no whole groups of T={}".format(NT, T))
    if tables is None:
        tables = consistency_tables(Cn, T, aligned.device)
    elif not isinstance(tables, ConsistencyTables):
        tables = ConsistencyTables(tables, Cn, T)
    elif (tables.C, tables.T) != (Cn, T):
        raise L.DasacError("view_consistency: tables of C={}, T={} for a tensor of C={}, T={}".format(tables.C, tables.T, Cn, T))
    aligned = _c(aligned)
    with PROFILE.span("view_consistency", 0.0, None, aligned.numel() * 4.0):
        L.check(lib.dasac_view_consistency(aligned.data_ptr(), NT // T, T, Cn, H * W, float(cover), tables.agree.data_ptr(),
                                           tables.flips.data_ptr(), tables.per_view.data_ptr(), L.stream_ptr()),
                "dasac_view_consistency")
    return tables


# ----------------------------------------------------------------------------------------------
# per-layer activation tables (include/dasac_hip.h: dasac_activation_stats)
# ----------------------------------------------------------------------------------------------
# columns of an activation table row; per (segment, channel)
ACTIVATION_STATS_COLUMNS = ("sum", "sumsq", "maxabs", "nonfinite", "first_nonfinite", "zeros")
ACTIVATION_STATS_MAX_SEGMENTS, ACTIVATION_STATS_MAX_PLANE = 8, 1 << 30


def segment_bounds(bounds, N):
    """The sample segments of an activation table as the full tuple (0, ..., N).  `bounds`: None (one segment), the full tuple, or
    the interior cut points alone ((n_src,) for a [source; target] batch).  Refuses what the kernel could not check itself (the
    table lives in device memory): not strictly ascending, not ending at N, more than ACTIVATION_STATS_MAX_SEGMENTS segments."""
    N = int(N)
    b = () if bounds is None else tuple(int(v) for v in bounds)
    if not b or b[0] != 0:
        b = (0,) + b + (N,)
    if N < 1 or b[-1] != N or any(hi <= lo for lo, hi in zip(b, b[1:])) or len(b) - 1 > ACTIVATION_STATS_MAX_SEGMENTS:
        raise L.DasacError("activation_stats: segment bounds must ascend strictly from 0 to N={} in at most {} segments (got {})".format(
            N, ACTIVATION_STATS_MAX_SEGMENTS, bounds))
    return b


class ActivationStatsPlan:
    """Descriptor layout of one dasac_activation_stats call: built on the host once per (shapes, N, bounds) -- `activation_stats_plan`
    caches it -- the segment bounds uploaded once per device, the tensors' pointers patched into a copy of the rows per call.
    shapes: (C, H, W) or (C, HW) per tensor, each a contiguous fp32 [N, C, H, W]; bounds: see `segment_bounds`.
    rows (numpy, the 32-byte records of the header), row0 / plane0 (prefix sums of C / N*C), R, n_planes and bytes_read are plain host
    data: building a plan needs no device."""

    def __init__(self, shapes, N, bounds=None):
        import numpy as np
        self.N, self.bounds = int(N), segment_bounds(bounds, N)
        self.shapes = tuple((int(s[0]), int(np.prod(s[1:], dtype=np.int64))) for s in shapes)
        if not self.shapes or any(c < 1 or not 1 <= hw <= ACTIVATION_STATS_MAX_PLANE for c, hw in self.shapes):
            raise L.DasacError("activation_stats: at least one tensor, C >= 1 and 1 <= H*W <= 2^30 (got {})".format(list(shapes)))
        self.rows = np.zeros(len(self.shapes), dtype=np.dtype([("x", "<u8"), ("HW", "<i8"), ("C", "<i4"), ("row0", "<i4"), ("plane0", "<i8")]))
        assert self.rows.dtype.itemsize == 32
        cs = np.asarray([c for c, _ in self.shapes], dtype=np.int64)
        self.rows["HW"], self.rows["C"] = [hw for _, hw in self.shapes], cs
        self.rows["row0"], self.rows["plane0"] = np.cumsum(cs) - cs, (np.cumsum(cs) - cs) * self.N
        self.row0, self.plane0 = [int(v) for v in self.rows["row0"]], [int(v) for v in self.rows["plane0"]]
        self.R = int(cs.sum())
        self.n_planes = self.N * self.R
        if self.n_planes >= 1 << 31:
            raise L.DasacError("activation_stats: {} planes exceed one launch".format(self.n_planes))
        self.bytes_read = 4.0 * self.N * sum(c * hw for c, hw in self.shapes)
        self._bounds_dev = {}

    def run(self, tensors):
        """The table of `tensors` (fp32 cuda [N, C, ...] in the plan's order), a new fp64 [n_segments, R, 6] device tensor; two launches
        on the current stream, no synchronisation."""
        import numpy as np
        lib = L.load()
        L.require_gpu(*tensors)
        if len(tensors) != len(self.shapes):
            raise L.DasacError("activation_stats: the plan has {} tensors (got {})".format(len(self.shapes), len(tensors)))
        held = []
        for t, (c, hw) in zip(tensors, self.shapes):
            if t.dtype != torch.float32 or t.dim() < 2 or tuple(t.shape[:2]) != (self.N, c) or t.numel() != self.N * c * hw:
                raise L.DasacError("activation_stats: expected float32 [{}, {}, {}] (got {} {})".format(self.N, c, hw, t.dtype, tuple(t.shape)))
            held.append(_c(t))
        dev = held[0].device
        seg = self._bounds_dev.get(dev.index)
        if seg is None:
            seg = self._bounds_dev[dev.index] = torch.tensor(self.bounds, dtype=torch.int32).to(dev)
        rows = self.rows.copy()
        rows["x"] = [t.data_ptr() for t in held]
        # fresh activations every pass, so the pointers are new every call: through pinned memory, without blocking (optim._table)
        table_rows = torch.from_numpy(rows.view(np.int64)).pin_memory().to(dev, non_blocking=True)
        S = len(self.bounds) - 1
        table = torch.empty((S, self.R, len(ACTIVATION_STATS_COLUMNS)), dtype=torch.float64, device=dev)
        ws = L.workspace(lib.dasac_activation_stats_workspace(self.n_planes), dev)
        with PROFILE.span("activation_stats", 0.0, None, self.bytes_read):
            L.check(lib.dasac_activation_stats(table_rows.data_ptr(), len(held), self.N, self.R, seg.data_ptr(), S, ws.data_ptr(),
                                               ws.numel(), table.data_ptr(), L.stream_ptr()), "dasac_activation_stats")
        return table


_activation_plans = {}


def activation_stats_plan(shapes, N, bounds=None):
    """The cached ActivationStatsPlan of (shapes, N, bounds)."""
    key = (tuple(tuple(int(v) for v in s) for s in shapes), int(N), segment_bounds(bounds, N))
    plan = _activation_plans.get(key)
    if plan is None:
        plan = _activation_plans[key] = ActivationStatsPlan(key[0], key[1], key[2])
    return plan


def activation_stats(tensors, bounds=None):
    """dasac_activation_stats over a list of fp32 [N, C, ...] tensors: (table fp64 [n_segments, sum C, 6], plan)."""
    plan = activation_stats_plan([tuple(t.shape[1:]) for t in tensors], tensors[0].shape[0], bounds)
    return plan.run(tensors), plan


# ----------------------------------------------------------------------------------------------
# class-conditional feature tables (include/dasac_hip.h: dasac_label_nodes, dasac_class_feature_stats)
# ----------------------------------------------------------------------------------------------
CLASS_FEATURE_COLUMNS = ("sum", "sumsq")                    # last dimension of ClassFeatureTable.sums
CLASS_FEATURE_MAX_CLASSES, CLASS_FEATURE_MAX_RADIUS, CLASS_FEATURE_MAX_PLANE = 32, 8, 1 << 30


def label_nodes(labels, size, num_classes, radius=0):
    """A label map at a feature map's resolution (include/dasac_hip.h: dasac_label_nodes).  labels: int64 or uint8 [N,H,W] (255, -1
    and every value >= num_classes: no class); size: (h, w).  Returns uint8 [N,h,w]: the label at the pixel where
    align_corners=True upsampling puts the node if that label is a class and the whole (2 radius + 1)^2 window around the pixel,
    clipped to the image, holds it, else 255.  radius 0..8; one launch."""
    lib = L.load()
    L.require_gpu(labels)
    if labels.dtype not in (torch.int64, torch.uint8) or labels.dim() != 3 or labels.numel() == 0:
        raise L.DasacError("label_nodes takes a non-empty int64 or uint8 [N,H,W] label map (got {} {})".format(labels.dtype, tuple(labels.shape)))
    h, w = int(size[0]), int(size[1])
    Cn, radius = int(num_classes), int(radius)
    if h < 1 or w < 1 or not 1 <= Cn <= 255 or not 0 <= radius <= CLASS_FEATURE_MAX_RADIUS:
        raise L.DasacError("label_nodes: a size of at least 1 x 1, 1..255 classes and a radius in 0..{} (got {}x{}, C={}, radius={})".format(
            CLASS_FEATURE_MAX_RADIUS, h, w, Cn, radius))
    labels = _c(labels)
    N, H, W = labels.shape
    nodes = torch.empty((N, h, w), dtype=torch.uint8, device=labels.device)
    L.check(lib.dasac_label_nodes(labels.data_ptr(), int(labels.dtype == torch.uint8), N, H, W, h, w, Cn, radius, nodes.data_ptr(),
                                  L.stream_ptr()), "dasac_label_nodes")
    return nodes


class ClassFeatureTable:
    """What `class_feature_stats` accumulates into: sums (device fp64 [C,Cf,2], CLASS_FEATURE_COLUMNS) and counts (device int64 [C],
    the nodes of each class).  Both add over batches and over ranks."""

    def __init__(self, sums, counts):
        if sums.dtype != torch.float64 or sums.dim() != 3 or sums.shape[2] != len(CLASS_FEATURE_COLUMNS) or not sums.is_contiguous():
            raise L.DasacError("a class feature table holds contiguous float64 [C,Cf,2] sums (got {} {})".format(sums.dtype, tuple(sums.shape)))
        if counts.dtype != torch.int64 or tuple(counts.shape) != (sums.shape[0],) or not counts.is_contiguous() or counts.device != sums.device:
            raise L.DasacError("a class feature table holds contiguous int64 [{}] counts beside its sums (got {} {})".format(
                sums.shape[0], counts.dtype, tuple(counts.shape)))
        self.sums, self.counts = sums, counts

    C = property(lambda self: int(self.sums.shape[0]))
    Cf = property(lambda self: int(self.sums.shape[1]))

    @classmethod
    def zeros(cls, C, Cf, device):
        return cls(torch.zeros((int(C), int(Cf), len(CLASS_FEATURE_COLUMNS)), dtype=torch.float64, device=device),
                   torch.zeros(int(C), dtype=torch.int64, device=device))

    def cpu(self):
        return ClassFeatureTable(self.sums.cpu(), self.counts.cpu())

    def __repr__(self):
        return "ClassFeatureTable(C={}, Cf={}, device={})".format(self.C, self.Cf, self.sums.device)


def class_feature_stats(x, nodes, num_classes, table=None):
    """Per class and channel, the sum and the sum of squares (fp64, exact widening) of x over the positions whose node holds that
    class, and the number of such nodes (include/dasac_hip.h: dasac_class_feature_stats).  x: fp32 [N,Cf,...]; nodes: uint8 [N,...]
    with as many positions per sample (`label_nodes`; a value >= num_classes is no class); num_classes 1..32.  Accumulates into
    `table` (a ClassFeatureTable; allocated zeroed when None) and returns it.  Two launches, no synchronisation, deterministic."""
    lib = L.load()
    if table is not None and not isinstance(table, ClassFeatureTable):
        raise L.DasacError("class_feature_stats accumulates into a ClassFeatureTable (got {})".format(type(table).__name__))
    L.require_gpu(x, nodes, None if table is None else table.sums, None if table is None else table.counts)
    Cn = int(num_classes)
    if x.dtype != torch.float32 or x.dim() < 2 or x.numel() == 0:
        raise L.DasacError("class_feature_stats takes a non-empty float32 [N,Cf,...] tensor (got {} {})".format(x.dtype, tuple(x.shape)))
    N, Cf = int(x.shape[0]), int(x.shape[1])
    HW = x.numel() // (N * Cf)
    if nodes.dtype != torch.uint8 or nodes.dim() < 1 or nodes.shape[0] != N or nodes.numel() != N * HW:
        raise L.DasacError("class_feature_stats: nodes must be uint8 [{}, {} positions] (got {} {})".format(N, HW, nodes.dtype, tuple(nodes.shape)))
    if not 1 <= Cn <= CLASS_FEATURE_MAX_CLASSES or not 1 <= HW < CLASS_FEATURE_MAX_PLANE or N > 65535:
        raise L.DasacError("class_feature_stats: 1..{} classes, 1 <= H*W < 2^30, N <= 65535 (got C={}, H*W={}, N={})".format(
            CLASS_FEATURE_MAX_CLASSES, Cn, HW, N))
    if table is None:
        table = ClassFeatureTable.zeros(Cn, Cf, x.device)
    elif (table.C, table.Cf) != (Cn, Cf) or table.sums.device != x.device:
        raise L.DasacError("class_feature_stats: a table of C={}, Cf={} on {} is needed (got {!r})".format(Cn, Cf, x.device, table))
    x, nodes = _c(x), _c(nodes)
    ws = L.workspace(lib.dasac_class_feature_stats_workspace(N, Cf, Cn), x.device)
    with PROFILE.span("class_feature_stats", 0.0, None, x.numel() * 4.0):
        L.check(lib.dasac_class_feature_stats(x.data_ptr(), nodes.data_ptr(), N, Cf, HW, Cn, table.sums.data_ptr(), table.counts.data_ptr(),
                                              ws.data_ptr(), ws.numel(), L.stream_ptr()), "dasac_class_feature_stats")
    return table


VIS_IMAGE, VIS_LABELS, VIS_SCORES, VIS_CONF = 0, 1, 2, 3


def vis_panels(jobs, size, panels, mean, std, palette, cmap, want_u8=False):
    """The epoch summary panels of one batch in ONE launch (base_trainer.py:75-198; include/dasac_hip.h: dasac_vis_panels).
    jobs: sequence of (kind, src, backdrop, softmax, column, column2) with kind one of VIS_IMAGE (src f32 [B,3,H,W]), VIS_LABELS
    (src i64 [B,H,W]), VIS_SCORES (src f32 [B,C,H,W]; class overlay to `column`, confidence overlay to `column2`), VIS_CONF (src f32
    [B,H,W] or [B,1,H,W]); backdrop f32 [B,3,H,W] of the source's H x W (None for VIS_IMAGE).  size = (h, w) of one panel, `panels`
    the number of panel columns P.  palette u8 [256,3] and cmap f32 [256,3] on the device; mean / std three floats.  Returns the
    strip f32 [B,3,h,P*w], and with want_u8 also the quantised rows u8 [B,3,h,P*w].  No input is written."""
    import ctypes as C
    lib = L.load()
    jobs = list(jobs)
    if not jobs:
        raise L.DasacError("vis_panels: no job")
    L.require_gpu(palette, cmap, *[t for job in jobs for t in job[1:3]])
    h, w = int(size[0]), int(size[1])
    P = int(panels)
    if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3) or cmap.dtype != torch.float32 or tuple(cmap.shape) != (256, 3):
        raise L.DasacError("vis_panels: palette must be uint8 [256,3] and cmap float32 [256,3] (got {} {} and {} {})".format(
            palette.dtype, tuple(palette.shape), cmap.dtype, tuple(cmap.shape)))
    B = jobs[0][1].shape[0]
    table, keep, used = (L.VisJob * len(jobs))(), [_c(palette), _c(cmap)], set()
    for i, (kind, src, back, softmax, column, column2) in enumerate(jobs):
        want = {VIS_IMAGE: (torch.float32, 4), VIS_LABELS: (torch.int64, 3), VIS_SCORES: (torch.float32, 4), VIS_CONF: (torch.float32, 3)}.get(kind)
        if want is None:
            raise L.DasacError("vis_panels: job {}: unknown kind {}".format(i, kind))
        if kind == VIS_CONF and src.dim() == 4 and src.shape[1] == 1:
            src = src[:, 0]
        if src.dtype != want[0] or src.dim() != want[1] or src.shape[0] != B or (kind == VIS_IMAGE and src.shape[1] != 3):
            raise L.DasacError("vis_panels: job {} (kind {}): bad source {} {}".format(i, kind, src.dtype, tuple(src.shape)))
        H, W = src.shape[-2:]
        if kind != VIS_IMAGE and (back is None or back.dtype != torch.float32 or tuple(back.shape) != (B, 3, H, W)):
            raise L.DasacError("vis_panels: job {}: the backdrop must be float32 {} (got {})".format(
                i, (B, 3, H, W), None if back is None else (back.dtype, tuple(back.shape))))
        cols = [int(column)] + ([int(column2)] if kind == VIS_SCORES else [])
        if len(set(cols)) != len(cols) or any(c < 0 or c >= P or c in used for c in cols):
            raise L.DasacError("vis_panels: job {}: columns {} outside 0..{} or already taken".format(i, cols, P - 1))
        used.update(cols)
        src, back = _c(src), (None if kind == VIS_IMAGE else _c(back))
        keep += [src, back]
        table[i] = L.VisJob(src.data_ptr(), L.ptr(back), kind, src.shape[1] if kind == VIS_SCORES else 1, H, W, int(bool(softmax)),
                            cols[0], cols[-1] if kind == VIS_SCORES else 0, 0)
    if len(used) != P:
        raise L.DasacError("vis_panels: {} of {} panel columns are written by no job".format(P - len(used), P))
    device = keep[0].device
    jobs_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
    strip = torch.empty((B, 3, h, P * w), dtype=torch.float32, device=device)
    rows = torch.empty((B, 3, h, P * w), dtype=torch.uint8, device=device) if want_u8 else None
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    L.check(lib.dasac_vis_panels(jobs_dev.data_ptr(), C.cast(table, C.c_void_p), len(jobs), B, h, w, P, C.cast(m3, C.c_void_p),
                                 C.cast(s3, C.c_void_p), keep[0].data_ptr(), keep[1].data_ptr(), strip.data_ptr(), L.ptr(rows),
                                 L.stream_ptr()), "dasac_vis_panels")
    return (strip, rows) if want_u8 else strip


def vis_grid(strip, padding=8, pad_value=0.9):
    """`_visualise_grid` (base_trainer.py:258-270) of a float strip [B,3,h,W]: quantised with `.mul(255).clamp(0, 255).byte()` and
    stacked like make_grid(nrow=1, padding, pad_value): u8 [3, B*(h+padding)+padding, W+padding], a single row [3,h,W]."""
    lib = L.load()
    L.require_gpu(strip)
    if strip.dtype != torch.float32 or strip.dim() != 4 or strip.shape[1] != 3:
        raise L.DasacError("vis_grid takes a float32 [B,3,h,W] strip (got {} {})".format(strip.dtype, tuple(strip.shape)))
    strip = _c(strip)
    B, _, h, wt = strip.shape
    pad = int(padding) if B > 1 else 0
    grid = torch.empty((3, B * (h + pad) + pad, wt + pad), dtype=torch.uint8, device=strip.device)
    L.check(lib.dasac_vis_grid(strip.data_ptr(), B, h, wt, int(padding), float(pad_value), grid.data_ptr(), L.stream_ptr()), "dasac_vis_grid")
    return grid
